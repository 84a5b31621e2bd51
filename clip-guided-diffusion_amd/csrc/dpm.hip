// DPM-Solver++(2M) sampling (Lu et al., 2022: data prediction, multistep, deterministic and SDE): the update after one guided evaluation at
// (x, t), which takes the state from level t to level t - 1.  One elementwise launch does the whole update:
//   x0c             = the guided pred_xstart of the evaluation (guided_x0 of guidance.h: condition_score_with_grad, as cgd_multistep_update and
//                     mode 1 of cgd_sample_update; g scaled by scalars[7] when scalars is given, g may be null)
//   D               = c_r != 0 ? x0c + c_r (x0c - x0_hist) : x0c               (x0_hist: the x0c of the step before)
//   sample          = t != 0 ? c_x x + c_d D (+ c_n noise when c_n != 0) : x0c   (a select: no 0 * inf at the clean end)
//   x0c_out         = x0c                                                      (the next step's x0_hist; the caller rotates two buffers by pointer)
//   pred_xstart_out = pred_xstart                                              (the unguided prediction, as the other updates yield)
// The coefficients come from the host in float64 (cgd_amd.diffusion.SpacedDiffusion.dpmpp_coef).  All tensors are NCHW fp32 (B,3,H,W).
// No LDS, no scratch.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "elem_pack.h"
#include "guidance.h"

#include <algorithm>

namespace {

using namespace elem_pack;

struct DpmArgs {
  const float* x;
  const float* x0;
  const float* g;        // or null
  const float* scalars;  // or null
  const float* noise;    // or null, read only when c_n != 0 and t != 0
  const float* hist;     // or null, read only when c_r != 0
  float* x0c;            // or null
  float* sample;
  float* x0o;            // or null
  float cx, cd, cr, cn;
};

// grid.y walks the B * 3 planes, grid.x the plane in units of V floats (V = 4 needs HW % 4 == 0 and 16-byte aligned pointers: a unit then
// never straddles two planes)
template <int V>
__global__ __launch_bounds__(256) void dpmpp_update_kernel(DpmArgs a, StepCoef k, int planes, int HW) {
  const int units = HW / V;
  const float fct = a.scalars ? a.scalars[7] : 1.f;
  const bool second = a.cr != 0.f, noisy = a.cn != 0.f && k.nonzero;
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const long po = (long)p * HW;
    for (long u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
      const long o = po + u * V;
      float x[V], x0[V], g[V], nz[V], hs[V], x0c[V], s[V];
      load<V>(a.x + o, x);
      load<V>(a.x0 + o, x0);
      if (a.g) load<V>(a.g + o, g);
      if (second) load<V>(a.hist + o, hs);
      if (noisy) load<V>(a.noise + o, nz);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        x0c[e] = guided_x0(k, x[e], x0[e], a.g ? g[e] * fct : 0.f);
        const float d = second ? x0c[e] + a.cr * (x0c[e] - hs[e]) : x0c[e];
        float m = a.cx * x[e] + a.cd * d;
        if (noisy) m += a.cn * nz[e];
        s[e] = k.nonzero ? m : x0c[e];
      }
      store<V>(a.sample + o, s);
      if (a.x0c) store<V>(a.x0c + o, x0c);
      if (a.x0o) store<V>(a.x0o + o, x0);
    }
  }
}

}  // namespace

int cgd_launch_dpmpp_update(cgd_ctx* ctx, const float* x, const float* x0, const float* g, const float* scalars, const float* noise,
                            const float* x0_hist, float* x0c_out, float* sample, float* x0_out, int B, int H, int W, const StepCoef& k,
                            const cgd_dpmpp& d, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) CGD_FAIL(ctx, "dpmpp update: empty shape");
  if (!x || !x0 || !sample) CGD_FAIL(ctx, "dpmpp update: x, pred_xstart and sample are required");
  if (d.c_r != 0.f && !x0_hist) CGD_FAIL(ctx, "dpmpp update: a second-order step (c_r != 0) needs the guided pred_xstart of the step before");
  if (d.c_n != 0.f && k.nonzero && !noise) CGD_FAIL(ctx, "dpmpp update: the SDE step (c_n != 0) needs the step noise");
  if (sample == x || (x0c_out && x0c_out == x) || (x0_out && x0_out == x)) CGD_FAIL(ctx, "dpmpp update: no output may alias x");
  if ((x0c_out && x0c_out == sample) || (x0_out && (x0_out == sample || x0_out == x0c_out)))
    CGD_FAIL(ctx, "dpmpp update: sample, x0c_out and pred_xstart_out must be distinct buffers");
  if ((long)H * W > INT32_MAX || (long)B * 3 > INT32_MAX) CGD_FAIL(ctx, "dpmpp update: a plane or the plane count exceeds 2^31 - 1");
  DpmArgs a = {x, x0, g, scalars, noise, x0_hist, x0c_out, sample, x0_out, d.c_x, d.c_d, d.c_r, d.c_n};
  const int planes = B * 3, HW = H * W;
  const bool vec = HW % 4 == 0 && aligned16(x) && aligned16(x0) && aligned16(g) && aligned16(noise) && aligned16(x0_hist) &&
                   aligned16(x0c_out) && aligned16(sample) && aligned16(x0_out);
  const int units = vec ? HW / 4 : HW;
  const dim3 grid(std::min(cdiv(units, 256), 1024), std::min(planes, 65535));
  if (vec)
    CGD_LAUNCH(dpmpp_update_kernel<4>, grid, dim3(256), 0, s, a, k, planes, HW);
  else
    CGD_LAUNCH(dpmpp_update_kernel<1>, grid, dim3(256), 0, s, a, k, planes, HW);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
