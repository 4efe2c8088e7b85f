// Device pieces shared by the convolution kernels (igemm.hip, wgrad.hip, patchconv.hip): each is stated here once.
//   compile-time loops, counted vmcnt waits, the LDS-DMA instruction, the transposing-read fragment, the LDS chunk swizzle,
//   the f16x2 three-MFMA product, the row -> (n, i, j) -> output pixel maps of a tap plan, and the LDS ring of DMA stages.
// Everything is __forceinline__ and takes the scalar fields it reads, never a whole parameter block.
#pragma once
#include "common.h"

template <int U> struct IC {
    static constexpr int value = U;
    constexpr operator int() const { return U; }
};
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) { static_for<N - 1>(f); f(IC<N - 1>{}); }
}

template <int N> __device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 24, "vmcnt range");
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if constexpr (N == 18) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    else if constexpr (N == 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else static_assert(N < 0, "add the vmcnt literal");
}

// global_load_lds_dwordx4: every lane's 16 bytes at `src` go to LDS at the wave-uniform `dst` + 16 * lane (no staging registers)
__device__ __forceinline__ void lds_dma16(const void* src, void* dst) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}

// two ds_read_b64_tr_b16: the 8-deep MFMA 16x16x32 fragment of a tile staged [pixels][channels] (k 0..3 from `lo`, 4..7 from `hi`)
__device__ __forceinline__ elem8 tr_frag(const char* lo, const char* hi) {
    union { struct { s16x4 a, b; } s; elem8 v; } u;
    u.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, lo));
    u.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, hi));
    return u.v;
}

// XOR swizzle of the 16-byte chunk index inside a 128-byte LDS row: makes the ds_read_b128 fragment reads (lane l ->
// row l&15, chunk l>>4) conflict-free (2 rows per 256-byte bank row; derivation in DESIGN.md)
__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

// f16x2 product of one fragment pair (common.h): h.h into acc, the cross terms h.l + l.h (scaled by 2^11) into acc2
__device__ __forceinline__ void sp_mfma3(const half8& ah, const half8& al, const half8& bh, const half8& bl, f32x4& acc, f32x4& acc2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc2, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc2, 0, 0, 0);
}

// row m of a tap plan's Hg x Wg row grid -> (n, i, j)
struct RowNIJ { uint32_t n, i, j; };
__device__ __forceinline__ RowNIJ row_nij(uint32_t m, const FastDiv& div_hw, const FastDiv& div_w, int Hg, int Wg) {
    RowNIJ r;
    r.n = fdiv(m, div_hw);
    const uint32_t rem = m - r.n * (uint32_t)(Hg * Wg);
    r.i = fdiv(rem, div_w);
    r.j = rem - r.i * (uint32_t)Wg;
    return r;
}
// output pixel (i * os + oa, j * os + ob) of a row in class (oa, ob): false when it falls outside the Ho x Wo map (opix is left alone then)
__device__ __forceinline__ bool out_pixel(const RowNIJ& r, int os, int oa, int ob, int Ho, int Wo, size_t& opix) {
    const uint32_t oh = r.i * os + oa, ow = r.j * os + ob;
    if (oh >= (uint32_t)Ho || ow >= (uint32_t)Wo) return false;
    opix = ((size_t)r.n * Ho + oh) * Wo + ow;
    return true;
}

// NS-deep LDS ring of DMA stages, LPS DMA instructions per wave and stage: counted vmcnt waits and ONE raw s_barrier per stage, so NS-1
// stages of loads stay in flight across barriers while the MFMAs of the current stage run.  issue(stage, buffer) starts a stage's loads,
// compute(buffer) consumes a landed one.  Two loops over the same step: run_unrolled names the buffers at compile time (IC<>: LDS addresses
// fold to constants), run passes them as integers.
template <int NS, int LPS>
struct Ring {
    int issued = 0;
    // NS-1 stages in flight
    template <typename Issue> __device__ __forceinline__ void prologue(int nsteps, Issue&& issue) {
        static_for<NS - 1>([&](auto u) __attribute__((always_inline)) {
            if (u < nsteps) { issue((int)u, u); ++issued; }
        });
    }
    // stage st has landed (at most issued - st - 1 younger stages may still be in flight) in every wave; buffer (st - 1) % NS is free
    __device__ __forceinline__ void landed(int st) const {
        if (issued - st - 1 >= NS - 2) wait_vmcnt<LPS*(NS - 2)>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
    }
    // at_barrier(st): the caller's hook between the barrier and the re-issue (igemm_kernel's timeline stamp)
    template <typename Issue, typename Compute, typename Hook>
    __device__ __forceinline__ void run_unrolled(int nsteps, Issue&& issue, Compute&& compute, Hook&& at_barrier) {
        for (int st0 = 0; st0 < nsteps; st0 += NS) {
            static_for<NS>([&](auto u) __attribute__((always_inline)) {
                constexpr int U = decltype(u)::value;
                const int st = st0 + U;
                if (st < nsteps) {
                    landed(st);
                    at_barrier(st);
                    if (issued < nsteps) { issue(issued, IC<(U + NS - 1) % NS>{}); ++issued; }
                    compute(u);
                }
            });
        }
    }
    // one step of the runtime-buffer loop: stage st has landed, the next stage goes into the buffer that became free
    template <typename Issue> __device__ __forceinline__ void step(int st, int nsteps, Issue&& issue) {
        landed(st);
        if (issued < nsteps) { issue(issued, issued % NS); ++issued; }
    }
    template <typename Issue, typename Compute>
    __device__ __forceinline__ void run(int nsteps, Issue&& issue, Compute&& compute) {
        for (int st = 0; st < nsteps; ++st) {
            step(st, nsteps, issue);
            compute(st % NS);
        }
    }
};
