// Update of the multistep samplers: PLMS (pseudo linear multistep, Liu et al., ICLR 2022, as guided_diffusion's `plms_sample`) and
// DDIM with eta > 0 (`ddim_sample_with_grad`'s sigma term).  One elementwise launch per guided evaluation does the whole update: the
// guided eps of the evaluation (condition_score_with_grad, as mode 1 of sample_update_kernel), the Adams-Bashforth combination with the
// eps history, x0' and the mean, the t != 0 select and the stores of sample, pred_xstart and this evaluation's eps.
// All tensors are NCHW fp32 (B,3,H,W); the history buffers belong to the caller (cgd_amd.sampler rotates them by pointer).
#include "common.h"
#include <algorithm>

#include "guidance.h"

namespace {

struct Hist {
  const float* e[3];  // previous eps, newest first
};

// phase 0: Adams-Bashforth of `order` terms (eps of this evaluation + order-1 of the history); writes eps_out, sample, x0_out
// phase 1: start-step predictor at (x, t): eps_out = eps_a, sample = x0c * sqrt(abar_prev) + sqrt(1 - abar_prev) * eps_a, x0_out
// phase 2: start-step corrector at (x_eval = predictor, t - 1) with k; eps' = (eps_a + eps_b) / 2 and the update with ks (t) from x
// phase 3: DDIM with eta: sample = x0c * sqrt(abar_prev) + dir * eps + [t != 0] sigma * noise, x0_out
__global__ __launch_bounds__(256) void multistep_update_kernel(const float* __restrict__ x, const float* __restrict__ xe,
                                                               const float* __restrict__ x0, const float* __restrict__ g,
                                                               const float* __restrict__ scalars, const float* __restrict__ noise,
                                                               Hist h, float* __restrict__ eps_out, float* __restrict__ sample,
                                                               float* __restrict__ x0_out, long total, StepCoef k, StepCoef ks,
                                                               int phase, int order, float sigma, float dir) {
  const float fct = scalars ? scalars[7] : 1.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    // guided eps of the evaluation at (xe, k): exactly the arithmetic of sample_update_kernel mode 1
    const float xv = xe[i], x0v = x0[i];
    const float gv = g ? g[i] * fct : 0.f;
    const float x0c = guided_x0(k, xv, x0v, gv);
    const float eps = (k.sqrt_recip * xv - x0c) / k.sqrt_recipm1;
    if (phase == 3) {
      const float s = x0c * k.sqrt_ab_prev + dir * eps;
      sample[i] = k.nonzero ? s + sigma * noise[i] : s;
      x0_out[i] = x0v;
      continue;
    }
    if (phase == 1) {
      eps_out[i] = eps;
      sample[i] = x0c * k.sqrt_ab_prev + k.sqrt_one_minus_ab_prev * eps;
      x0_out[i] = x0v;
      continue;
    }
    float ep, xs;
    if (phase == 2) {
      ep = (h.e[0][i] + eps) * 0.5f;
      xs = x[i];
    } else {
      eps_out[i] = eps;
      xs = xv;
      if (order == 1) {
        ep = eps;
      } else if (order == 2) {
        ep = (3.f * eps - h.e[0][i]) * 0.5f;
      } else if (order == 3) {
        ep = (23.f * eps - 16.f * h.e[0][i] + 5.f * h.e[1][i]) * (1.f / 12.f);
      } else {
        ep = (55.f * eps - 59.f * h.e[0][i] + 37.f * h.e[1][i] - 9.f * h.e[2][i]) * (1.f / 24.f);
      }
    }
    const float xp = ks.sqrt_recip * xs - ks.sqrt_recipm1 * ep;
    const float mean = xp * ks.sqrt_ab_prev + ks.sqrt_one_minus_ab_prev * ep;
    sample[i] = ks.nonzero ? mean : x0c;
    if (phase == 0) x0_out[i] = x0v;
  }
}

}  // namespace

int cgd_launch_multistep_update(cgd_ctx* ctx, const float* x, const float* x_eval, const float* x0, const float* g, const float* scalars,
                                const float* noise, const float* const* eps_hist, float* eps_out, float* sample, float* x0_out, int B,
                                int H, int W, const StepCoef& k, const StepCoef* k_step, const cgd_multistep& m, hipStream_t s) {
  if (m.phase < 0 || m.phase > 3) CGD_FAIL(ctx, "multistep update: phase must be 0 (Adams-Bashforth), 1 (predictor), 2 (corrector) or 3 (DDIM eta)");
  if (m.phase == 0 && (m.order < 1 || m.order > 4)) CGD_FAIL(ctx, "multistep update: order must be 1..4");
  if (B <= 0 || H <= 0 || W <= 0) CGD_FAIL(ctx, "multistep update: empty shape");
  const int need_hist = m.phase == 0 ? m.order - 1 : (m.phase == 2 ? 1 : 0);
  Hist h = {{nullptr, nullptr, nullptr}};
  if (need_hist > 0 && !eps_hist) CGD_FAIL(ctx, "multistep update: the eps history is missing");
  for (int j = 0; j < need_hist; ++j) {
    h.e[j] = eps_hist[j];
    if (!h.e[j]) CGD_FAIL(ctx, "multistep update: an eps history entry the order needs is NULL");
  }
  if (!x || !x0 || !sample) CGD_FAIL(ctx, "multistep update: x, pred_xstart and sample are required");
  if (m.phase != 2 && !x0_out) CGD_FAIL(ctx, "multistep update: pred_xstart_out is required");
  if ((m.phase == 0 || m.phase == 1) && !eps_out) CGD_FAIL(ctx, "multistep update: eps_out is required");
  if (m.phase == 2 && (!x_eval || !k_step)) CGD_FAIL(ctx, "multistep update: the corrector needs the predictor (x_eval) and the step's coefficients");
  if (m.phase == 2 && !k_step->nonzero) CGD_FAIL(ctx, "multistep update: a start step cannot run at t == 0");
  if (m.phase == 3 && k.nonzero && !noise) CGD_FAIL(ctx, "multistep update: DDIM with eta needs the step noise");
  const long total = (long)B * 3 * H * W;
  CGD_LAUNCH(multistep_update_kernel, dim3(grid_for(total)), dim3(256), 0, s, x, x_eval ? x_eval : x, x0, g, scalars, noise, h, eps_out,
             sample, x0_out, total, k, k_step ? *k_step : k, m.phase, m.order, m.sigma, m.dir);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
