// Host launchers of the heat-map, loss and evaluation kernels.
#pragma once
#include "common.h"

// heatmap.hip
int hm_sqdiff_rows(hipStream_t s, const float* a, const float* b, const float* w, const unsigned char* mask, int R, int HW, float half,
                   float* rows, float* mean_out, const unsigned char* valid, const float* count, int Kc);
int hm_sqdiff_bwd(hipStream_t s, const float* a, const float* b, const float* w, const unsigned char* mask, const float* gscale, float coef,
                  int R, int HW, float* da, const unsigned char* valid, const float* count, int Kc);
int hm_mask_count(hipStream_t s, const unsigned char* m, size_t n, float* count);
int hm_argmax_rectify(hipStream_t s, const float* hm, int R, int H, int W, float* maxv, int* idx, float* preds, float* rect, const float* patch,
                      int rad);
int hm_kth_mask(hipStream_t s, const float* act, const float* tm, int n, int k, float* thr_out, unsigned char* mask, const float* act_local,
                int n_local);
int hm_kth_mask_dev(hipStream_t s, const float* act, const float* tm, int n, const int* k_dev, float* thr_out, unsigned char* mask,
                    const float* act_local, int n_local);
int hm_pck(hipStream_t s, const float* pred, const float* gt, int B, int K, float nh, float nw, float thr, float* acc, float* avg_cnt);
// pck_curve.hip
int pck_accumulate(hipStream_t s, const float* pred, const float* gt, const unsigned char* visible, const float* norm, int B, int K, float nh,
                   float nw, const float* thr, int T, long long* state);
int pck_accumulate_heatmaps(hipStream_t s, const float* out, const float* target, const float* norm, int B, int K, int H, int W,
                            const float* thr, int T, long long* state, float* preds);
// select.hip
int sel_topk(hipStream_t s, const float* rows, const float* wfac, const unsigned char* mfac, int N, int K, int topk, int largest,
             unsigned char* sel, float* sample, float* mean_out);
int sel_topk_sqdiff_bwd(hipStream_t s, const float* a, const float* b, const float* w, const unsigned char* sel, const float* gscale, int N,
                        int K, int HW, int topk, int half, float* da);
int sel_joint_kth_mask(hipStream_t s, const float* pool, int n_pool, int K, int k, const float* tm, const float* act_local, int n_local,
                       float* thr_out, unsigned char* mask);
int sel_joint_kth_mask_dev(hipStream_t s, const float* pool, int n_pool, int K, const int* k_dev, const float* tm, const float* act_local,
                           int n_local, float* thr_out, unsigned char* mask);
int sel_thr_mask(hipStream_t s, const float* act, const float* tm, size_t n, const float* thr_dev, unsigned char* mask);
// softmax_loss.hip
int sml_kl_fwd(hipStream_t st, const float* s, const float* g, const float* w, float eps, int R, int group, int HW, float* rows, float* stats,
               float* out);
int sml_kl_bwd(hipStream_t st, const float* s, const float* g, const float* w, float eps, const float* stats, const float* gscale, int R, int HW,
               float* ds);
int sml_ent_fwd(hipStream_t st, const float* s, int R, int group, int HW, float thr, float* rows, float* stats, float* out, float* count);
int sml_ent_bwd(hipStream_t st, const float* s, const float* rows, const float* stats, const float* count, const float* gscale, float thr, int R,
                int HW, float* ds);
int sml_cons_fwd(hipStream_t st, int mode, const float* s, const float* t, const unsigned char* mask, const unsigned char* valid,
                 const float* count, int R, int Kc, int HW, float* rows, float* stats, float* out);
int sml_cons_bwd(hipStream_t st, int mode, const float* s, const float* t, const unsigned char* mask, const unsigned char* valid,
                 const float* count, const float* stats, const float* gscale, int R, int Kc, int HW, float* ds);
// softargmax.hip
int sa_fwd(hipStream_t st, const float* hm, int R, int H, int W, float beta, int window, float* coords, float* maxv, int* idx, float* stats);
int sa_bwd(hipStream_t st, const float* hm, const float* g, const int* idx, const float* stats, int R, int H, int W, float beta, int window,
           float* dh);
int sa_coord_fwd(hipStream_t st, const float* hm, const float* tgt, const float* w, const unsigned char* mask, int R, int group, int H, int W,
                 float beta, int window, int norm, float* rows, int* idx, float* stats, float* out);
int sa_coord_bwd(hipStream_t st, const float* hm, const float* tgt, const float* w, const unsigned char* mask, const int* idx, const float* stats,
                 const float* gscale, int R, int H, int W, float beta, int window, int norm, float* dh);
// coral.hip
long long coral_ws_bytes(int N, int K, int H, int W, int down);
int coral_fwd(hipStream_t st, const float* src, const float* tgt, int N, int K, int H, int W, int down, void* ws, float* coef, float* loss);
int coral_bwd(hipStream_t st, const float* src, const float* tgt, const float* coef, const float* gscale, int N, int K, int H, int W, int down,
              float* dsrc, float* dtgt);
// prior_map.hip
int pm_weights(hipStream_t s, const float* sd, int K, float gamma, float epsilon, int v3, float* w);
int pm_map(hipStream_t s, const float* coords, const float* conf, const float* mean, const float* w, const float* hm, int B, int K, int H, int W,
           float sigma, int v3, float* out);
int pm_pair_accumulate(hipStream_t s, const float* coords, const unsigned char* vis, int M, int K, double* acc);
int pm_pair_finish(hipStream_t s, const double* acc, int K, float* mean, float* sd);
// flip.hip
int flip_hbatch(hipStream_t s, const float* src, float* dst, int N, size_t rows_per_image, int W, int keep_original);
int flip_merge(hipStream_t s, const float* a, const float* f, const int* perm, int N, int K, int H, int W, int shift, int mode, float* out,
               float* maxv, int* idx, float* preds);
// refine.hip
int refine_decode(hipStream_t s, const float* hm, int R, int H, int W, int mode, int kernel, float sigma, float* coords, float* maxv, int* idx);
// pose_nms.hip
int pose_rescore(hipStream_t s, const float* kp, const float* conf, const float* boxes, const unsigned char* status, const float* box_score,
                 const float* vis_thr, int M, int K, float* score, int* order, float* area, unsigned char* refused);
int oks_matrix(hipStream_t s, const float* kp_a, const float* area_a, int Ma, const float* kp_b, const float* area_b, const float* visible_b, int Mb,
               int K, const float* sigmas, const int* frame_idx, const unsigned char* refused, const float* oks_thr, float* out,
               unsigned long long* mask);
int pose_nms_sweep(hipStream_t s, const unsigned long long* mask, const int* order, const unsigned char* refused, int M, unsigned char* keep,
                   int* n_keep, int* suppressed_by);
size_t pose_nms_ws_bytes(int M);
int pose_nms(hipStream_t s, const float* kp, const float* conf, const float* boxes, const int* frame_idx, const unsigned char* status,
             const float* box_score, const float* sigmas, const float* vis_thr, const float* oks_thr, int M, int K, void* ws, float* score, int* order,
             unsigned char* keep, int* n_keep, int* suppressed_by, float* oks_out);
// pose_ap.hip
size_t ap_match_ws_bytes(int M, int G, int F);
int ap_match(hipStream_t s, const float* kp, const float* score, const int* frame_idx, const unsigned char* valid, const float* area, int M,
             const float* gt_kp, const float* gt_visible, const float* gt_area, const int* gt_frame, const unsigned char* gt_ignore, int G, int K,
             int F, const float* sigmas, const float* thresholds, int T, const float* ranges, int A, int max_dets, void* ws, float* rec_score,
             unsigned long long* rec_matched, unsigned long long* rec_ignored, int capacity, long long* counters);
size_t ap_curve_ws_bytes(int capacity, int T, int A);
int ap_curve(hipStream_t s, const float* rec_score, const unsigned long long* rec_matched, const unsigned long long* rec_ignored, int capacity,
             const long long* counters, int T, int A, const double* recall_points, int R, void* ws, double* precision, float* scores,
             double* recall);
