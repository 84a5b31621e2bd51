// Internal launchers of guidance.hip that take the public per-step coefficient struct.
#pragma once
#include "../../include/cgd_mi355x.h"
#include "common.h"

typedef cgd_step_coef StepCoef;

// The guided pred_xstart of one evaluation at (xv, k), condition_score_with_grad: eps of the model's prediction x0v, shifted by the guidance
// gradient gv (already scaled by the magnitude clamp), and the pred_xstart that eps implies.  Shared by mode 1 of sample_update_kernel
// (guidance.hip), the multistep update (plms.hip), the DPM-Solver++ update (dpm.hip) and the first launch of its thresholding (threshold.hip).
__device__ __forceinline__ float guided_x0(const StepCoef& k, float xv, float x0v, float gv) {
  float e = (k.sqrt_recip * xv - x0v) / k.sqrt_recipm1;
  e -= k.sqrt_one_minus_ab * gv;
  return k.sqrt_recip * xv - k.sqrt_recipm1 * e;
}

int cgd_launch_pmv_blend(cgd_ctx* ctx, const float* x, const float* out6, float* x0, float* mean, float* logvar, float* xin, int B,
                         int H, int W, const StepCoef& k, hipStream_t s);
int cgd_launch_guidance_combine(cgd_ctx* ctx, const float* gclip, const float* xin, const float* x0, float* gdir, float* seed6,
                                float* part, int B, int H, int W, const StepCoef& k, float tv_scale, float range_scale,
                                float sat_scale, hipStream_t s);
int cgd_launch_grad_finish(cgd_ctx* ctx, const float* gdir, const float* gunet, float* g, float* part, int B, int H, int W,
                           hipStream_t s);
int cgd_launch_scalars(cgd_ctx* ctx, const float* clip_part, int n_clip, const float* l_part, const float* g_part, int B, int H, int W,
                       int use_magnitude, float* scalars, hipStream_t s);
int cgd_launch_sample_update(cgd_ctx* ctx, const float* x, const float* x0, const float* mean, const float* logvar, const float* g,
                             const float* noise, const float* scalars, float* sample, float* x0_out, int B, int H, int W,
                             const StepCoef& k, int mode, hipStream_t s);
// direction.hip
int cgd_launch_directional_loss(cgd_ctx* ctx, const float* emb, const float* src_emb, const float* dirs_n, const float* weights, float* demb,
                                float* loss_part, int cutn, int B, int Bs, int P, int D, float scale, int accumulate, hipStream_t s);
// region prompts (include/cgd_mi355x.h, cgd_spherical_loss_regions): what the `_regions` entries take on top of the plain ones.  All device
// memory but region_of_host, the caller's host copy of region_of that cgd_check_regions reads
struct cgd_regions {
  const int* sat;
  const int* region_of;
  const int* region_of_host;
  const float* power;
  const int* geo;
  int R, H, W;
};
// regions.hip: -2 (with the reason) for a null pointer, R < 1, a frame whose table does not fit int32 or a region_of entry outside [-1, R)
int cgd_check_regions(cgd_ctx* ctx, const cgd_regions& rg, int P);
int cgd_launch_region_coverage(cgd_ctx* ctx, const cgd_regions& rg, float* out, int cutn, int P, hipStream_t s);
int cgd_launch_spherical_loss_regions(cgd_ctx* ctx, const float* emb, const float* targets_n, const float* weights, float* demb,
                                      float* loss_part, int cutn, int B, int P, int D, float scale, const cgd_regions& rg, hipStream_t s);
int cgd_launch_directional_loss_regions(cgd_ctx* ctx, const float* emb, const float* src_emb, const float* dirs_n, const float* weights,
                                        float* demb, float* loss_part, int cutn, int B, int Bs, int P, int D, float scale, int accumulate,
                                        const cgd_regions& rg, hipStream_t s);
// aesthetic.hip
int cgd_launch_aesthetic_loss(cgd_ctx* ctx, const float* emb, const float* head, float* demb, float* loss_part, float* score, int cutn, int B,
                              int D, float scale, int accumulate, hipStream_t s);
// plms.hip
int cgd_launch_multistep_update(cgd_ctx* ctx, const float* x, const float* x_eval, const float* x0, const float* g, const float* scalars,
                                const float* noise, const float* const* eps_hist, float* eps_out, float* sample, float* x0_out, int B,
                                int H, int W, const StepCoef& k, const StepCoef* k_step, const cgd_multistep& m, hipStream_t s);
// dpm.hip
int cgd_launch_dpmpp_update(cgd_ctx* ctx, const float* x, const float* x0, const float* g, const float* scalars, const float* noise,
                            const float* x0_hist, float* x0c_out, float* sample, float* x0_out, int B, int H, int W, const StepCoef& k,
                            const cgd_dpmpp& d, hipStream_t s);
int cgd_launch_dpmpp_update_thr(cgd_ctx* ctx, const float* x, const float* x0, const float* x0c, const float* thr3, const float* noise,
                                const float* x0_hist, float* x0c_out, float* sample, float* x0_out, int B, int H, int W, const StepCoef& k,
                                const cgd_dpmpp& d, hipStream_t s);
// threshold.hip
int cgd_launch_abs_quantile(cgd_ctx* ctx, const float* v, int B, long n, long k, float frac, float floor, float cap, float* out3,
                            void* scratch, hipStream_t s);
int cgd_launch_dpmpp_threshold(cgd_ctx* ctx, const float* x, const float* x0, const float* g, const float* scalars, float* x0c, int B, int H,
                               int W, const StepCoef& kc, long k, float frac, float floor, float cap, float* thr3, void* scratch,
                               hipStream_t s);
