// Key-point AP under OKS on the device (fp32 / fp64 / integers only: both builds of the library export identical code).
// One update (udapose_ap_match), three launches:
//   ap_rank_k   : a detection's area, whether it is refused, and the order of all M (descending score, equal scores by ascending index,
//                 refused ones last): pose_pair.h's key and rank by counting, keys staged once in LDS, as in pose_rescore_k
//   ap_frames_k : one work-group: detections and labels per frame (LDS integer counts), the record offset of every frame by common.h's
//                 block scan in ascending frame id - the sequence order is part of the result, nothing is appended in arrival order - and
//                 the counts
//   ap_match_k  : a wave per frame.  Phase 1, lane = label: the OKS tile [<= max_dets][64] in LDS, the labels' key points staged [K][64]
//                 as oks_matrix_k stages its columns; the per-joint term and the visibility word are pose_pair.h's, the ones of
//                 oks_matrix_k.  Phase 2, lane = (range a, threshold t): cocoapi's greedy walk, the matched set and the range's ignore
//                 set one 64-bit register each, one loop over set bits run for the counted labels, then for the ignored ones; the
//                 record's two words are two ballots
// The tables (udapose_ap_curve), two launches, N read from the device counter:
//   ap_sort_k   : a work-group ranks 256 records against all N keys streamed through LDS in tiles (the same rank by counting: O(N^2)
//                 compares, stable, deterministic), then scatters the three record fields into sorted order
//   ap_curve_k  : a work-group per (t, a): block scans of the integer tp / fp flags, pr and rc in fp64 with the one IEEE division each,
//                 the envelope as per-chunk maxima and their suffix maxima, per recall point a bisection on the monotone rc
// Integer atomics on the int64 counters only; no floating-point atomics; nothing is read back: capturable, a replay appends again.
#include <float.h>
#include <math.h>
#include "losses.h"
#include "pose_pair.h"
#include "pose_ws.h"

#pragma clang fp contract(off)

namespace {
constexpr int MAX_M = UDAPOSE_NMS_MAX_POSES, MAX_F = UDAPOSE_AP_MAX_FRAMES;
constexpr int MAX_L = UDAPOSE_AP_MAX_LABELS_PER_FRAME, MAX_C = UDAPOSE_AP_MAX_COMBOS, MAX_R = UDAPOSE_AP_MAX_RECALL_POINTS;
constexpr int MAX_CAP = UDAPOSE_AP_MAX_CAPACITY, NCNT = UDAPOSE_AP_COUNTERS;
static_assert(MAX_L == 64 && MAX_C == 64, "a lane per label, a lane per (range, threshold)");
enum { C_RECORDS = 0, C_DROPPED, C_REFUSED, C_CUT, C_OVERFLOW, C_BAD_LABELS };

// ---------------------------------------------------------------------------------------------------------------- the order of an update
struct DetInfo { float area; bool refused; };

// area: the given one, or (max_k x - min_k x) * (max_k y - min_k y) over all K joints (cocoapi loadRes); refused: valid == 0, a score,
// coordinate or given area that is not finite, a frame outside [0, F)
__device__ __forceinline__ DetInfo det_info(int m, const float* __restrict__ kp, const float* __restrict__ score, const int* __restrict__ frame,
                                            const unsigned char* __restrict__ valid, const float* __restrict__ area, int K, int F) {
    const float2* p = (const float2*)kp + (size_t)m * K;
    float2 q = p[0];
    float x0 = q.x, x1 = q.x, y0 = q.y, y1 = q.y;
    bool bad = !finite_f(q.x) || !finite_f(q.y);
    for (int k = 1; k < K; ++k) {
        q = p[k];
        bad |= !finite_f(q.x) || !finite_f(q.y);
        x0 = fminf(x0, q.x); x1 = fmaxf(x1, q.x);
        y0 = fminf(y0, q.y); y1 = fmaxf(y1, q.y);
    }
    DetInfo r;
    r.area = area ? area[m] : (x1 - x0) * (y1 - y0);
    r.refused = bad || (valid && valid[m] == 0) || !finite_f(score[m]) || (area && !finite_f(r.area)) || (unsigned int)frame[m] >= (unsigned int)F;
    return r;
}

__global__ __launch_bounds__(RANK_TPB) void ap_rank_k(const float* __restrict__ kp, const float* __restrict__ score, const int* __restrict__ frame,
                                                      const unsigned char* __restrict__ valid, const float* __restrict__ area, int M, int K, int F,
                                                      int* __restrict__ order, int* __restrict__ ofr, float* __restrict__ darea) {
    __shared__ __attribute__((aligned(16))) unsigned int keys[MAX_M];
    __shared__ int part[RANK_PARTS][RANK_ITEMS];
    const int t = threadIdx.x, i0 = blockIdx.x * RANK_ITEMS;
    const int Mpad = rank_padded(M);
    for (int m = t; m < Mpad; m += RANK_TPB) {
        unsigned int key = POSE_KEY_REFUSED;
        if (m < M) {
            const DetInfo r = det_info(m, kp, score, frame, valid, area, K, F);
            key = order_key(score[m], r.refused);
            if (m >= i0 && m < i0 + RANK_ITEMS) darea[m] = r.area;
        }
        keys[m] = key;
    }
    __syncthreads();
    const int p = t & (RANK_ITEMS - 1), q = t / RANK_ITEMS, i = i0 + p;
    const unsigned int ki = i < M ? keys[i] : 0u;
    const int per = Mpad / RANK_PARTS;
    const int rank = rank_finish(part, q, p, rank_count(keys + q * per, per, q * per, ki, i));
    if (q == 0 && i < M) {
        order[rank] = i;
        ofr[rank] = ki == POSE_KEY_REFUSED ? -1 : frame[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- frames and record offsets
constexpr int FR_TPB = 1024, FR_PER = MAX_F / FR_TPB;

__global__ __launch_bounds__(FR_TPB) void ap_frames_k(const int* __restrict__ ofr, int M, const int* __restrict__ gt_frame, int G, int F, int max_dets,
                                                      int capacity, int* __restrict__ rec_off, long long* __restrict__ counters) {
    __shared__ int cd[MAX_F], cl[MAX_F];
    __shared__ int wsum[FR_TPB / 64];
    __shared__ int tot[4];      // refused, bad labels, cut, overflow frames
    __shared__ long long s_base;
    const int t = threadIdx.x;
    for (int f = t; f < F; f += FR_TPB) { cd[f] = 0; cl[f] = 0; }
    if (t < 4) tot[t] = 0;
    if (t == 0) s_base = counters[C_RECORDS];
    __syncthreads();
    int refused = 0, bad = 0;
    for (int r = t; r < M; r += FR_TPB) {
        const int f = ofr[r];
        if (f < 0) ++refused;
        else atomicAdd(&cd[f], 1);
    }
    for (int g = t; g < G; g += FR_TPB) {
        const int f = gt_frame[g];
        if ((unsigned int)f >= (unsigned int)F) ++bad;
        else atomicAdd(&cl[f], 1);
    }
    __syncthreads();
    int n[FR_PER], local = 0, cut = 0, over = 0;
#pragma unroll
    for (int e = 0; e < FR_PER; ++e) {
        const int f = t * FR_PER + e;
        n[e] = 0;
        if (f < F) {
            if (cl[f] > MAX_L) ++over;      // left out whole: neither its labels nor its detections count
            else { n[e] = min(cd[f], max_dets); cut += cd[f] - n[e]; }
        }
        local += n[e];
    }
    const int tally[4] = {refused, bad, cut, over};
    for (int e = 0; e < 4; ++e) {
        const int v = wave_sum(tally[e]);
        if ((t & 63) == 0 && v) atomicAdd(&tot[e], v);
    }
    int total;      // (the scan's barriers publish tot as well)
    int excl = block_scan_incl<FR_TPB / 64>(local, wsum, total) - local;
    const long long base = s_base;
#pragma unroll
    for (int e = 0; e < FR_PER; ++e) {
        const int f = t * FR_PER + e;
        if (f < F) rec_off[f] = cl[f] > MAX_L ? -1 : (int)base + excl;      // (base <= capacity <= 2^18, excl <= 4096 * 64)
        excl += n[e];
    }
    if (t == 0) {
        const long long all = base + total, stored = all < capacity ? all : capacity;
        counters[C_RECORDS] = stored;
        counters[C_DROPPED] += all - stored;
        counters[C_REFUSED] += tot[0];
        counters[C_BAD_LABELS] += tot[1];
        counters[C_CUT] += tot[2];
        counters[C_OVERFLOW] += tot[3];
    }
}

// ---------------------------------------------------------------------------------------------------------------- matching
static inline size_t match_lds_bytes(int K, int max_dets) {
    return (size_t)(MAX_L + 1) * K * sizeof(float2) + (size_t)max_dets * MAX_L * sizeof(float) + (size_t)K * sizeof(float) + 2 * 64 * sizeof(int);
}

__global__ __launch_bounds__(64) void ap_match_k(const float* __restrict__ kp, const float* __restrict__ score, const float* __restrict__ darea,
                                                 const int* __restrict__ order, const int* __restrict__ ofr, int M, const float* __restrict__ gt_kp,
                                                 const float* __restrict__ gt_visible, const float* __restrict__ gt_area,
                                                 const int* __restrict__ gt_frame, const unsigned char* __restrict__ gt_ignore, int G, int K,
                                                 const float* __restrict__ sigmas, const float* __restrict__ thr, int T,
                                                 const float* __restrict__ ranges, int A, int max_dets, const int* __restrict__ rec_off,
                                                 float* __restrict__ rec_score, u64* __restrict__ rec_matched, u64* __restrict__ rec_ignored,
                                                 int capacity, long long* __restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float2* tl = (float2*)lds;                         // [K][64] the labels' key points, lane-consecutive
    float2* td = tl + (size_t)MAX_L * K;               // [K] one detection's key points, read as broadcasts
    float* tile = (float*)(td + K);                    // [max_dets][64] oks(d, label)
    float* vk = tile + (size_t)max_dets * MAX_L;       // [K] (2 sigma_k)^2
    int* detl = (int*)(vk + K);                        // [64] the frame's detections in their order
    int* labl = detl + 64;                             // [64] the frame's labels by ascending index
    const int f = blockIdx.x, lane = threadIdx.x;
    const int off = rec_off[f];
    if (off < 0) return;      // more than 64 labels
    const u64 below = (1ull << lane) - 1ull;
    int nl = 0;
    for (int g0 = 0; g0 < G; g0 += 64) {
        const int g = g0 + lane;
        const bool ok = g < G && gt_frame[g] == f;
        const u64 b = __ballot(ok);
        if (ok) labl[nl + __popcll(b & below)] = g;      // (ap_frames_k counted them: at most 64)
        nl += __popcll(b);
    }
    int nd = 0;
    for (int r0 = 0; r0 < M && nd < max_dets; r0 += 64) {
        const int r = r0 + lane;
        const bool ok = r < M && ofr[r] == f;
        const u64 b = __ballot(ok);
        const int pos = nd + __popcll(b & below);
        if (ok && pos < max_dets) detl[pos] = order[r];
        nd += __popcll(b);
    }
    nd = min(nd, max_dets);
    for (int k = lane; k < K; k += 64) vk[k] = oks_sigma_sq(sigmas[k]);
    __syncthreads();
    // phase 1: lane = label
    for (int e = lane; e < MAX_L * K; e += 64) {
        const int jj = e / K, k = e - jj * K;
        tl[k * MAX_L + jj] = jj < nl ? ((const float2*)gt_kp)[(size_t)labl[jj] * K + k] : make_float2(0.f, 0.f);
    }
    const bool have = lane < nl;
    const int g = have ? labl[lane] : 0;
    const u64 vb = !have ? 0ull : gt_visible ? visible_bits(gt_visible + (size_t)g * K, K) : full_bits(K);
    const int nvis = __popcll(vb);
    const float ga = have ? gt_area[g] : 0.f;
    const float Aj = oks_rect_area(ga);
    const bool base_ign = nvis == 0 || (gt_ignore && have && gt_ignore[g] != 0);
    __syncthreads();
    for (int d = 0; d < nd; ++d) {
        const int m = detl[d];
        for (int k = lane; k < K; k += 64) td[k] = ((const float2*)kp)[(size_t)m * K + k];
        __syncthreads();
        float acc = 0.f;      // (written out, as oks_matrix_k's four-row loop is: see there)
        for (int k = 0; k < K; ++k) {
            const float term = oks_term(td[k], tl[k * MAX_L + lane], vk[k], Aj);      // (prediction, label: oks_matrix_k's operand order)
            if ((vb >> k) & 1ull) acc += term;
        }
        tile[d * MAX_L + lane] = oks_rect_mean(acc, nvis);
        __syncthreads();
    }
    // phase 2: lane = a * T + t
    const bool active = lane < T * A;
    const int a = active ? lane / T : 0, t = lane - a * T;
    const float thr_t = thr[active ? t : 0], lo = ranges[2 * a], hi = ranges[2 * a + 1];
    u64 ign = 0ull;
    for (int aa = 0; aa < A; ++aa) {
        const float l2 = ranges[2 * aa], h2 = ranges[2 * aa + 1];
        const u64 w = __ballot(have && (base_ign || ga < l2 || ga > h2));
        if (aa == a) ign = w;
    }
    const u64 nonign = full_bits(nl) & ~ign;
    if (active && t == 0) counter_add(counters + NCNT + a, (long long)__popcll(nonign));
    u64 matched = 0ull;
    for (int d = 0; d < nd; ++d) {
        const int m = detl[d];
        float best = thr_t;
        int mg = -1;
        // the last label of set w, in ascending index, whose oks is not below the best so far
        auto walk = [&](u64 w) {
            while (w) {
                const int j = __ffsll((long long)w) - 1;
                w &= w - 1ull;
                const float o = tile[d * MAX_L + j];
                if (o < best) continue;
                best = o;
                mg = j;
            }
        };
        if (active) {
            walk(nonign & ~matched);
            if (mg < 0) walk(ign & ~matched);      // an ignored label is reached only when no counted one was
        }
        const float da = darea[m];
        const bool dm = mg >= 0;
        const bool di = dm ? (bool)((ign >> mg) & 1ull) : (da < lo || da > hi);
        if (dm) matched |= 1ull << mg;
        const u64 wm = __ballot(active && dm), wi = __ballot(active && di);
        const long long pos = (long long)off + d;
        if (lane == 0 && pos < capacity) {
            rec_score[pos] = score[m];
            rec_matched[pos] = wm;
            rec_ignored[pos] = wi;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the sort of the records
constexpr int SO_TILE = 4096, SO_PER = SO_TILE / RANK_PARTS;

__device__ __forceinline__ int record_count(const long long* __restrict__ counters, int capacity) {
    const long long n = counters[C_RECORDS];
    return (int)(n < 0 ? 0 : (n < capacity ? n : capacity));
}

// rank(i) = #{j: key_j < key_i, or equal with j < i}; the index is the sequence number (records are appended in sequence order)
__global__ __launch_bounds__(RANK_TPB) void ap_sort_k(const float* __restrict__ rs, const u64* __restrict__ rm, const u64* __restrict__ ri,
                                                      const long long* __restrict__ counters, int capacity, float* __restrict__ ss,
                                                      u64* __restrict__ sm, u64* __restrict__ si) {
    __shared__ __attribute__((aligned(16))) unsigned int tile[SO_TILE];
    __shared__ int part[RANK_PARTS][RANK_ITEMS];
    const int N = record_count(counters, capacity), i0 = blockIdx.x * RANK_ITEMS;
    if (i0 >= N) return;
    const int t = threadIdx.x, p = t & (RANK_ITEMS - 1), q = t / RANK_ITEMS, i = i0 + p;
    const unsigned int ki = i < N ? order_key(rs[i], false) : 0u;
    int count = 0;
    for (int j0 = 0; j0 < N; j0 += SO_TILE) {
        __syncthreads();
        for (int e = t; e < SO_TILE; e += RANK_TPB) tile[e] = j0 + e < N ? order_key(rs[j0 + e], false) : POSE_KEY_REFUSED;
        __syncthreads();
        if (j0 + q * SO_PER < N) count += rank_count(tile + q * SO_PER, SO_PER, j0 + q * SO_PER, ki, i);
    }
    const int rank = rank_finish(part, q, p, count);
    if (q == 0 && i < N) {
        ss[rank] = rs[i];
        sm[rank] = rm[i];
        si[rank] = ri[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- the curves
constexpr int CV_TPB = 1024, CV_WAVES = CV_TPB / 64, CV_MAX_CHUNKS = MAX_CAP / CV_TPB;

__device__ __forceinline__ double precision_at(int tp, int fp) { return (double)tp / ((double)(fp + tp) + DBL_EPSILON); }

// the block's maximum, given to thread 0 (others get a partial one); opens with a barrier (red may still be read)
__device__ __forceinline__ double block_max0(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < CV_WAVES; ++w) v = fmax(v, red[w]);
    return v;
}

__global__ __launch_bounds__(CV_TPB) void ap_curve_k(const float* __restrict__ ss, const u64* __restrict__ sm, const u64* __restrict__ si,
                                                     const long long* __restrict__ counters, int capacity, int T, int A,
                                                     const double* __restrict__ rp, int R, int* tpc, int* fpc, double* __restrict__ precision,
                                                     float* __restrict__ scores, double* __restrict__ recall) {
    __shared__ int wsum[CV_WAVES];
    __shared__ double wmax[CV_WAVES];
    __shared__ double sufmax[CV_MAX_CHUNKS + 1];
    __shared__ int s_q[MAX_R];
    const int b = blockIdx.x, a = b / T, t = b - a * T, tid = threadIdx.x;
    const int N = record_count(counters, capacity);
    const long long npig = counters[NCNT + a];
    if (npig <= 0) {
        for (int r = tid; r < R; r += CV_TPB) {
            precision[((size_t)t * R + r) * A + a] = -1.0;
            scores[((size_t)t * R + r) * A + a] = -1.f;
        }
        if (tid == 0) recall[(size_t)t * A + a] = -1.0;
        return;
    }
    int* tp = tpc + (size_t)b * capacity;
    int* fp = fpc + (size_t)b * capacity;
    const int nch = (N + CV_TPB - 1) / CV_TPB;
    int btp = 0, bfp = 0;
    for (int c = 0; c < nch; ++c) {
        const int i = c * CV_TPB + tid;
        int fl = 0;      // tp in the low half, fp in the high half: a chunk holds at most 1024 of either
        if (i < N && !((si[i] >> b) & 1ull)) fl = ((sm[i] >> b) & 1ull) ? 1 : 0x10000;
        int total;
        const int inc = block_scan_incl<CV_WAVES>(fl, wsum, total);
        const int ctp = btp + (inc & 0xffff), cfp = bfp + (inc >> 16);
        double pr = -1.0;
        if (i < N) {
            tp[i] = ctp;
            fp[i] = cfp;
            pr = precision_at(ctp, cfp);
        }
        pr = block_max0(pr, wmax);
        if (tid == 0) sufmax[c] = pr;
        btp += total & 0xffff;
        bfp += total >> 16;
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        sufmax[nch] = -1.0;
        for (int c = nch - 1; c >= 0; --c) sufmax[c] = fmax(sufmax[c], sufmax[c + 1]);
        recall[(size_t)t * A + a] = N ? (double)btp / (double)npig : 0.0;
    }
    if (tid < R) {      // the first index with rc >= the recall point (N: none)
        const double want = rp[tid];
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((double)tp[mid] / (double)npig >= want) hi = mid;
            else lo = mid + 1;
        }
        s_q[tid] = lo;
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        const int q = s_q[r];      // (uniform)
        const size_t o = ((size_t)t * R + r) * A + a;
        if (q >= N) {
            if (tid == 0) { precision[o] = 0.0; scores[o] = 0.f; }
            continue;
        }
        const int c = q / CV_TPB, i = c * CV_TPB + tid;
        double v = -1.0;
        if (i >= q && i < N) v = precision_at(tp[i], fp[i]);
        v = block_max0(v, wmax);
        if (tid == 0) { precision[o] = fmax(v, sufmax[c + 1]); scores[o] = ss[q]; }
    }
}

bool bad_table(int T, int A) { return T < 1 || A < 1 || T * A > MAX_C; }
bool bad_update(int M, int G, int F) { return bad_poses(M) || bad_poses(G) || F < 1 || F > MAX_F; }
bool bad_capacity(int capacity) { return capacity < 1 || capacity > MAX_CAP; }
}  // namespace

size_t ap_match_ws_bytes(int M, int G, int F) { return bad_update(M, G, F) ? 0 : ApMatchWs(nullptr, M, F).bytes; }

int ap_match(hipStream_t s, const float* kp, const float* score, const int* frame_idx, const unsigned char* valid, const float* area, int M,
             const float* gt_kp, const float* gt_visible, const float* gt_area, const int* gt_frame, const unsigned char* gt_ignore, int G, int K,
             int F, const float* sigmas, const float* thresholds, int T, const float* ranges, int A, int max_dets, void* ws, float* rec_score,
             unsigned long long* rec_matched, unsigned long long* rec_ignored, int capacity, long long* counters) {
    // every check ahead of the first launch: an error leaves nothing written
    if (!kp || !score || !frame_idx || !gt_kp || !gt_area || !gt_frame || !sigmas || !thresholds || !ranges || !ws || !rec_score || !rec_matched ||
        !rec_ignored || !counters)
        return UDAPOSE_ERR_ARG;
    if (bad_update(M, G, F) || bad_keypoints(K) || bad_table(T, A)) return UDAPOSE_ERR_ARG;
    if (max_dets < 1 || max_dets > 64 || bad_capacity(capacity) || ((uintptr_t)ws & 7u)) return UDAPOSE_ERR_ARG;
    const ApMatchWs w(ws, M, F);
    hipLaunchKernelGGL(ap_rank_k, dim3((M + RANK_ITEMS - 1) / RANK_ITEMS), dim3(RANK_TPB), 0, s, kp, score, frame_idx, valid, area, M, K, F, w.order,
                       w.ofr, w.darea);
    int e = udapose_check_launch();
    if (e != UDAPOSE_OK) return e;
    hipLaunchKernelGGL(ap_frames_k, dim3(1), dim3(FR_TPB), 0, s, w.ofr, M, gt_frame, G, F, max_dets, capacity, w.rec_off, counters);
    e = udapose_check_launch();
    if (e != UDAPOSE_OK) return e;
    hipLaunchKernelGGL(ap_match_k, dim3(F), dim3(64), match_lds_bytes(K, max_dets), s, kp, score, w.darea, w.order, w.ofr, M, gt_kp, gt_visible, gt_area,
                       gt_frame, gt_ignore, G, K, sigmas, thresholds, T, ranges, A, max_dets, w.rec_off, rec_score, rec_matched, rec_ignored, capacity,
                       counters);
    return udapose_check_launch();
}

size_t ap_curve_ws_bytes(int capacity, int T, int A) {
    return (bad_capacity(capacity) || bad_table(T, A)) ? 0 : ApCurveWs(nullptr, capacity, T, A).bytes;
}

int ap_curve(hipStream_t s, const float* rec_score, const unsigned long long* rec_matched, const unsigned long long* rec_ignored, int capacity,
             const long long* counters, int T, int A, const double* recall_points, int R, void* ws, double* precision, float* scores,
             double* recall) {
    if (!rec_score || !rec_matched || !rec_ignored || !counters || !recall_points || !ws || !precision || !scores || !recall) return UDAPOSE_ERR_ARG;
    if (bad_capacity(capacity) || bad_table(T, A) || R < 1 || R > MAX_R || ((uintptr_t)ws & 7u)) return UDAPOSE_ERR_ARG;
    const ApCurveWs w(ws, capacity, T, A);
    hipLaunchKernelGGL(ap_sort_k, dim3((capacity + RANK_ITEMS - 1) / RANK_ITEMS), dim3(RANK_TPB), 0, s, rec_score, rec_matched, rec_ignored, counters,
                       capacity, w.ss, w.sm, w.si);
    const int e = udapose_check_launch();
    if (e != UDAPOSE_OK) return e;
    hipLaunchKernelGGL(ap_curve_k, dim3(T * A), dim3(CV_TPB), 0, s, w.ss, w.sm, w.si, counters, capacity, T, A, recall_points, R, w.tpc, w.fpc, precision,
                       scores, recall);
    return udapose_check_launch();
}
