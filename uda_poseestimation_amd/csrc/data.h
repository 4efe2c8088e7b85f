// Host launchers of the data pipeline: warps, occlusion and patches (affine.hip), the merge of the teacher's views (view_merge.hip), image augmentation and label maps (augment.hip), box crops and their coordinate maps (box_crop.hip), the strong view's colour ops and erase (strong_aug.hip).
#pragma once
#include "common.h"

// ToTensor + Normalize of one byte-range value v (0 .. 255; an integer in aug_to_tensor_k, any fp32 value in box_crop_k): float32 operations
// in torch's order.  Stated once: wherever v is an integer, box_crop_k's normalised output has the bits of aug_to_tensor_k's.
__device__ __forceinline__ float to_tensor_norm(float v, float mean, float std) { return (v / 255.f - mean) / std; }

// affine.hip
int occlusion_pick(hipStream_t s, const float* conf, const int* idx, const float* u, int N, int K, int w, double ratio, int image_size, float rate,
                   float thresh, int occ, int* boxes, unsigned char* apply);
int select_rows(hipStream_t s, float* dst, const float* a, const float* b, const unsigned char* flag, int N, size_t row);
int patch_paste(hipStream_t s, float* img, const int* boxes, int n, int C, int H, int W, int max_patch_elems);
int affine_recon_thetas(hipStream_t s, const double* params, int N, double ratio, float* fwd, float* back);
int affine_warp_chain(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward);
int affine_warp_chain_bilinear(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward);
int affine_warp_chain_mirror(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage, int backward,
                             const unsigned char* mirror, const int* perm);
int affine_warp_chain_bilinear_mirror(hipStream_t s, const float* src, float* dst, const float* theta, int N, int C, int H, int W, int nstage,
                                      int backward, const unsigned char* mirror, const int* perm);
int affine_mean_views(hipStream_t s, const float* const* srcs, int k, float* dst, size_t n);
// view_merge.hip
int affine_view_merge(hipStream_t s, const float* const* srcs, int k, int R, int H, int W, int mode, const float* radius_dev, int min_views,
                      float* mean, int* peaks, float* maxvals, int* inliers, int* n_inliers, int* spread2, float* agree, float* energy);
// augment.hip
int aug_resized_crop_u8(hipStream_t s, const unsigned char* src, unsigned char* dst, unsigned char* tmp, const int* box, const int* bounds,
                        const int* coef, int N, int Hs, int Ws, int S, int ksize);
int aug_gaussian_blur_u8(hipStream_t s, unsigned char* img, unsigned char* tmp, const unsigned int* prm, int N, int H, int W);
int aug_affine_u8(hipStream_t s, const unsigned char* src, unsigned char* dst, const long long* coef, int N, int H, int W);
int aug_hflip_u8(hipStream_t s, const unsigned char* src, unsigned char* dst, const unsigned char* flag, int N, int H, int W);
int aug_color_op(hipStream_t s, unsigned char* img, const int* op, const float* factor, int* mean_scratch, int N, int HW);
int aug_to_tensor(hipStream_t s, const unsigned char* img, float* out, int N, int HW, const float* mean3, const float* std3);
int aug_gaussian_labels(hipStream_t s, const double* kp, const float* vis, float* target, float* weight, int R, int Hh, int Wh, double stride_x,
                        double stride_y, const float* patch, int rad);
int aug_gaussian_labels_subpixel(hipStream_t s, const double* kp, const float* vis, float* target, float* weight, int R, int Hh, int Wh,
                                 double stride_x, double stride_y, double sigma, int rad);
int aug_draw_labelmap_ori(hipStream_t s, const float* pt, const float* vis, const unsigned char* gate, float* target, float* weight, int R, int Hh,
                          int Wh, float r3, const float* patch, int psize);
// box_crop.hip
int box_crop(hipStream_t s, const unsigned char* frames, int F, int Hs, int Ws, const int* frame_idx, const float* boxes, int M, int Ho, int Wo,
             const float* mean3, const float* std3, int mirror, float* out_f32, unsigned char* out_u8, unsigned char* status);
int box_coords_to_image(hipStream_t s, const float* coords, const float* boxes, int M, int K, float stride_x, float stride_y, int Ho, int Wo,
                        float* out);
// strong_aug.hip
int aug_point_op(hipStream_t s, unsigned char* img, const int* op, const int* param, const double* inv_scale, unsigned char* lut, int N, int HW);
int aug_sharpness_u8(hipStream_t s, unsigned char* img, unsigned char* tmp, const int* op, const float* factor, int N, int H, int W);
int aug_erase_f32(hipStream_t s, float* x, const int* box, float v0, float v1, float v2, int N, int H, int W);
