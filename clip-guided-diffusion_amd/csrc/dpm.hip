// DPM-Solver++(2M) sampling (Lu et al., 2022: data prediction, multistep, deterministic and SDE): the update after one guided evaluation at
// (x, t), which takes the state from level t to level t - 1.  One elementwise launch does the whole update:
//   x0c             = the guided pred_xstart of the evaluation (guided_x0 of guidance.h: condition_score_with_grad, as cgd_multistep_update and
//                     mode 1 of cgd_sample_update; g scaled by scalars[7] when scalars is given, g may be null)
//   D               = c_r != 0 ? x0c + c_r (x0c - x0_hist) : x0c               (x0_hist: the x0c of the step before)
//   sample          = t != 0 ? c_x x + c_d D (+ c_n noise when c_n != 0) : x0c   (a select: no 0 * inf at the clean end)
//   x0c_out         = x0c                                                      (the next step's x0_hist; the caller rotates two buffers by pointer)
//   pred_xstart_out = pred_xstart                                              (the unguided prediction, as the other updates yield)
// With dynamic thresholding (threshold.hip) the same kernel takes x0c from the buffer cgd_dpmpp_threshold wrote and the sample's scale s_b
// from thr3[b * 3 + 2] (device memory: the host never reads it and nothing synchronises): x0c = clamp(x0c, -s_b, s_b) / s_b, a true division.
// The coefficients come from the host in float64 (cgd_amd.diffusion.SpacedDiffusion.dpmpp_coef).  All tensors are NCHW fp32 (B,3,H,W).
// No LDS, no scratch.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "elem_pack.h"
#include "guidance.h"

namespace {

using namespace elem_pack;

// One layout for both instantiations (their kernel arguments stay where they were): two slots hold what the instantiation's x0c comes
// from, and each instantiation reads them under its own names.
struct DpmArgs {
  const float* x;
  const float* x0;
  const float* slot2;     // plain: g, or null.  THR: the x0c buffer of cgd_dpmpp_threshold
  const float* slot3;     // plain: scalars, or null.  THR: thr3 of cgd_dpmpp_threshold
  const float* noise;     // or null, read only when c_n != 0 and t != 0
  const float* hist;      // or null, read only when c_r != 0
  float* x0c;             // or null
  float* sample;
  float* x0o;             // or null
  float cx, cd, cr, cn;
  __host__ __device__ const float* g() const { return slot2; }
  __host__ __device__ const float* scalars() const { return slot3; }
  __host__ __device__ const float* x0c_in() const { return slot2; }
  __host__ __device__ const float* thr3() const { return slot3; }
};

// grid.y walks the B * 3 planes, grid.x the plane in units of V floats (V = 4 needs HW % 4 == 0 and 16-byte aligned pointers: a unit then
// never straddles two planes).  THR false: x0c is guided_x0 of the evaluation.  THR true: x0c is read, clamped to its sample's scale and
// divided by it; pred_xstart is read only when it is written out.
template <int V, bool THR>
__global__ __launch_bounds__(256) void dpmpp_update_kernel(DpmArgs a, StepCoef k, int planes, int HW) {
  const int units = HW / V;
  const float fct = (!THR && a.scalars()) ? a.scalars()[7] : 1.f;
  const bool second = a.cr != 0.f, noisy = a.cn != 0.f && k.nonzero;
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const long po = (long)p * HW;
    const float sb = THR ? a.thr3()[(p / 3) * 3 + 2] : 1.f;
    for (long u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
      const long o = po + u * V;
      float x[V], x0[V], g[V], nz[V], hs[V], x0c[V], s[V];
      load<V>(a.x + o, x);
      if (THR) load<V>(a.x0c_in() + o, x0c);
      if (!THR || a.x0o) load<V>(a.x0 + o, x0);
      if (!THR && a.g()) load<V>(a.g() + o, g);
      if (second) load<V>(a.hist + o, hs);
      if (noisy) load<V>(a.noise + o, nz);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        x0c[e] = THR ? fminf(fmaxf(x0c[e], -sb), sb) / sb : guided_x0(k, x[e], x0[e], a.g() ? g[e] * fct : 0.f);
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

// the checks and the launch of both entry points; a message is put together only where a check fails
#define DPM_FAIL(msg) CGD_FAIL(ctx, std::string(THR ? "dpmpp thresholded update: " : "dpmpp update: ") + msg)
template <bool THR>
int launch_update(cgd_ctx* ctx, const DpmArgs& a, int B, int H, int W, const StepCoef& k, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) DPM_FAIL("empty shape");
  if (!a.x || !a.x0 || !a.sample) DPM_FAIL("x, pred_xstart and sample are required");
  if (THR && (!a.x0c_in() || !a.thr3())) DPM_FAIL("the x0c buffer and thr3 of cgd_dpmpp_threshold are required");
  if (a.cr != 0.f && !a.hist)
    DPM_FAIL("a second-order step (c_r != 0) needs the " + (THR ? "thresholded" : "guided") + " pred_xstart of the step before");
  if (a.cn != 0.f && k.nonzero && !a.noise) DPM_FAIL("the SDE step (c_n != 0) needs the step noise");
  if (a.sample == a.x || (a.x0c && a.x0c == a.x) || (a.x0o && a.x0o == a.x)) DPM_FAIL("no output may alias x");
  if ((a.x0c && a.x0c == a.sample) || (a.x0o && (a.x0o == a.sample || a.x0o == a.x0c)))
    DPM_FAIL("sample, x0c_out and pred_xstart_out must be distinct buffers");
  if (THR && (a.sample == a.x0c_in() || (a.x0c && a.x0c == a.x0c_in()) || (a.x0o && a.x0o == a.x0c_in()))) DPM_FAIL("no output may alias x0c");
  if ((long)H * W > INT32_MAX || (long)B * 3 > INT32_MAX) DPM_FAIL("a plane or the plane count exceeds 2^31 - 1");
  const int planes = B * 3, HW = H * W;
  plane_walk(HW, planes, [&](auto v, dim3 grid) {
    CGD_LAUNCH((dpmpp_update_kernel<decltype(v)::value, THR>), grid, dim3(256), 0, s, a, k, planes, HW);
  }, a.x, a.x0, a.slot2, a.noise, a.hist, a.x0c, a.sample, a.x0o);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
#undef DPM_FAIL

}  // namespace

int cgd_launch_dpmpp_update(cgd_ctx* ctx, const float* x, const float* x0, const float* g, const float* scalars, const float* noise,
                            const float* x0_hist, float* x0c_out, float* sample, float* x0_out, int B, int H, int W, const StepCoef& k,
                            const cgd_dpmpp& d, hipStream_t s) {
  return launch_update<false>(ctx, {x, x0, g, scalars, noise, x0_hist, x0c_out, sample, x0_out, d.c_x, d.c_d, d.c_r, d.c_n}, B, H, W, k, s);
}

int cgd_launch_dpmpp_update_thr(cgd_ctx* ctx, const float* x, const float* x0, const float* x0c, const float* thr3, const float* noise,
                                const float* x0_hist, float* x0c_out, float* sample, float* x0_out, int B, int H, int W, const StepCoef& k,
                                const cgd_dpmpp& d, hipStream_t s) {
  return launch_update<true>(ctx, {x, x0, x0c, thr3, noise, x0_hist, x0c_out, sample, x0_out, d.c_x, d.c_d, d.c_r, d.c_n}, B, H, W, k, s);
}
