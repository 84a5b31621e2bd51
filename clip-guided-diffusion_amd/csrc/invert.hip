// DDIM inversion of an init image (guided_diffusion's ddim_reverse_sample): the update of one inversion step, which takes the state from
// level i up to level i + 1 along the deterministic DDIM ODE.  One elementwise launch after the UNet forward:
//   eps         = out6[:, 0:3]                       (the model's 6-channel output read in place; the variance planes 3..5 are never touched)
//   pred_xstart = sqrt_recip x - sqrt_recipm1 eps
//   x_next      = sqrt(abar_next) pred_xstart + sqrt(1 - abar_next) eps
//   noise_out   = (x_next - sqrt(abar_next) init) / sqrt(1 - abar_next)        (optional: the tensor that q_samples init to x_next)
// eps is the model's own output.  Upstream re-derives it from pred_xstart, (sqrt_recip x - pred_xstart) / sqrt_recipm1; with
// clip_denoised=False the two are equal in exact arithmetic, but that form divides by sqrt_recipm1[0] ~ 0.01 at the clean end of the schedule
// and an fp32 round trip (constant eps, ddim50) loses 2e-4 in absolute terms through it.
// It replaces cgd_pmv_blend + cgd_sample_update for this purpose: no mean, log-variance or x_in is materialised and the variance planes are
// not read.  x, x_next, pred_xstart, noise_out: NCHW fp32 (B,3,H,W); out6 (B,6,H,W); init (1 or B,3,H,W).  No LDS, no scratch.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "elem_pack.h"
#include "kernels.h"

namespace {

using namespace elem_pack;

struct ReverseArgs {
  const float* x;
  const float* out6;
  const float* init;  // or null, read only for noise_out
  float* xn;
  float* x0;          // or null
  float* noise;       // or null
  float a, b;         // sqrt_recip, sqrt_recipm1 of level i
  float sa, sb, isb;  // sqrt(abar_next), sqrt(1 - abar_next), 1 / sqrt(1 - abar_next)
};

// grid.y walks the B * 3 planes, grid.x the plane in units of V floats (V = 4 needs HW % 4 == 0 and 16-byte aligned pointers: a unit then
// never straddles two planes).  The eps plane of sample b, channel c is plane b * 6 + c of out6.
template <int V>
__global__ __launch_bounds__(256) void ddim_reverse_kernel(ReverseArgs a, int planes, int HW, int init_b) {
  const int units = HW / V;
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const int b = p / 3, c = p - 3 * b;
    const long po = (long)p * HW;
    const long eo = (long)(b * 6 + c) * HW;
    const long io = (long)((init_b == 1 ? 0 : b) * 3 + c) * HW;
    for (long u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
      const long o = u * V;
      float x[V], eps[V], iv[V], x0[V], xn[V], nz[V];
      load<V>(a.x + po + o, x);
      load<V>(a.out6 + eo + o, eps);
      if (a.noise) load<V>(a.init + io + o, iv);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        x0[e] = a.a * x[e] - a.b * eps[e];
        xn[e] = a.sa * x0[e] + a.sb * eps[e];
        if (a.noise) nz[e] = (xn[e] - a.sa * iv[e]) * a.isb;
      }
      store<V>(a.xn + po + o, xn);
      if (a.x0) store<V>(a.x0 + po + o, x0);
      if (a.noise) store<V>(a.noise + po + o, nz);
    }
  }
}

}  // namespace

int cgd_launch_ddim_reverse_update(cgd_ctx* ctx, const float* x, const float* out6, const float* init, float* x_next, float* x0,
                                   float* noise_out, int B, int H, int W, int init_batch, const cgd_reverse_coef& k, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) CGD_FAIL(ctx, "ddim reverse update: empty shape");
  if (!x || !out6 || !x_next) CGD_FAIL(ctx, "ddim reverse update: x, the model output and x_next are required");
  if (x_next == x || x0 == x || noise_out == x) CGD_FAIL(ctx, "ddim reverse update: no output may alias x");
  if ((x0 && x0 == x_next) || (noise_out && (noise_out == x_next || noise_out == x0)))
    CGD_FAIL(ctx, "ddim reverse update: x_next, pred_xstart and noise_out must be distinct buffers");
  if (noise_out && !init) CGD_FAIL(ctx, "ddim reverse update: noise_out needs the init image");
  if (init && init_batch != 1 && init_batch != B) CGD_FAIL(ctx, "ddim reverse update: init must have batch 1 or B");
  if (noise_out && (k.sqrt_one_minus_ab_next == 0.f || k.inv_sqrt_one_minus_ab_next == 0.f))
    CGD_FAIL(ctx, "ddim reverse update: the implied noise is undefined where sqrt(1 - abar_next) is 0");
  if ((long)H * W > INT32_MAX || (long)B * 6 > INT32_MAX) CGD_FAIL(ctx, "ddim reverse update: a plane or the plane count exceeds 2^31 - 1");
  ReverseArgs a = {x, out6, noise_out ? init : nullptr, x_next, x0, noise_out, k.sqrt_recip, k.sqrt_recipm1, k.sqrt_ab_next,
                   k.sqrt_one_minus_ab_next, k.inv_sqrt_one_minus_ab_next};
  const int planes = B * 3, HW = H * W;
  plane_walk(HW, planes, [&](auto v, dim3 grid) {
    CGD_LAUNCH(ddim_reverse_kernel<decltype(v)::value>, grid, dim3(256), 0, s, a, planes, HW, init_batch);
  }, x, out6, a.init, x_next, x0, noise_out);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
