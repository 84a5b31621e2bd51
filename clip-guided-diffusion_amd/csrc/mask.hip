// Masked sampling (inpainting / outpainting of an init image): the merge that follows every sampler update.  One elementwise launch forms the
// known region at the level the update produced, known = sqrt(abar_prev) init + sqrt(1 - abar_prev) n_known, merges sample and pred_xstart
// in place under the mask (1 = regenerate, 0 = keep) and, for a resampling repeat, writes the state taken back up one level into a separate
// buffer.  The mask's endpoints are selects, not multiplies: where the mask is 0 nothing of `sample` reaches the output (a non-finite value
// there would survive 0 * x), where it is 1 the outputs keep their bits.
// sample, pred_xstart, n_known, n_re, x_re: NCHW fp32 (B,3,H,W); init (1 or B,3,H,W); mask (1 or B, 1 or 3, H, W).
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "elem_pack.h"
#include "kernels.h"

namespace {

using namespace elem_pack;

struct MergeArgs {
  float* sample;
  float* x0;           // or null
  const float* init;
  const float* mask;
  const float* nk;     // or null (then the known region is sa * init)
  const float* nre;    // or null
  float* xre;          // or null, present with nre
  float sa, sb;        // sqrt(abar_prev), sqrt(1 - abar_prev)
  float ra, rb;        // sqrt(abar / abar_prev), sqrt(1 - abar / abar_prev)
};

// The known region, sa * init (+ sb * n_known): two rounded products and a rounded sum.  Contraction into a fused multiply-add is switched off
// here, so the kept region is the fp32 value of the formula as written and a host can reproduce it bit for bit.
__device__ __forceinline__ float known_value(float sa, float iv, float sb, float nk, bool with_noise) {
#pragma clang fp contract(off)
  const float a = sa * iv;
  if (!with_noise) return a;
  const float b = sb * nk;
  return a + b;
}

// grid.y walks the B * 3 planes, grid.x the plane in units of V floats (V = 4 needs HW % 4 == 0 and 16-byte aligned pointers: a unit then
// never straddles two planes, and the broadcast operands are indexed per plane without a division per element)
template <int V>
__global__ __launch_bounds__(256) void masked_merge_kernel(MergeArgs a, int planes, int HW, int init_b, int mask_b, int mask_c) {
  const int units = HW / V;
  for (int p = blockIdx.y; p < planes; p += gridDim.y) {
    const int b = p / 3, c = p - 3 * b;
    const long po = (long)p * HW;
    const long io = (long)((init_b == 1 ? 0 : b) * 3 + c) * HW;
    const long mo = (long)((mask_b == 1 ? 0 : b) * mask_c + (mask_c == 1 ? 0 : c)) * HW;
    for (long u = blockIdx.x * blockDim.x + threadIdx.x; u < units; u += gridDim.x * blockDim.x) {
      const long o = u * V;
      float s[V], x0[V], iv[V], m[V], nk[V], nre[V], xre[V];
      load<V>(a.sample + po + o, s);
      load<V>(a.init + io + o, iv);
      load<V>(a.mask + mo + o, m);
      if (a.x0) load<V>(a.x0 + po + o, x0);
      if (a.nk) load<V>(a.nk + po + o, nk);
      if (a.nre) load<V>(a.nre + po + o, nre);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float known = known_value(a.sa, iv[e], a.sb, nk[e], a.nk != nullptr);
        const float keep = 1.f - m[e];
        const float sm = m[e] * s[e] + keep * known;
        s[e] = m[e] == 0.f ? known : (m[e] == 1.f ? s[e] : sm);
        if (a.x0) {
          const float xm = m[e] * x0[e] + keep * iv[e];
          x0[e] = m[e] == 0.f ? iv[e] : (m[e] == 1.f ? x0[e] : xm);
        }
        if (a.nre) xre[e] = a.ra * s[e] + a.rb * nre[e];
      }
      store<V>(a.sample + po + o, s);
      if (a.x0) store<V>(a.x0 + po + o, x0);
      if (a.nre) store<V>(a.xre + po + o, xre);
    }
  }
}

}  // namespace

int cgd_launch_masked_merge(cgd_ctx* ctx, float* sample, float* x0, const float* init, const float* mask, const float* n_known,
                            const float* n_re, float* x_re, int B, int H, int W, int init_batch, int mask_batch, int mask_channels,
                            const cgd_mask_coef& k, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) CGD_FAIL(ctx, "masked merge: empty shape");
  if (!sample || !init || !mask) CGD_FAIL(ctx, "masked merge: sample, init and mask are required");
  if (init_batch != 1 && init_batch != B) CGD_FAIL(ctx, "masked merge: init must have batch 1 or B");
  if (mask_batch != 1 && mask_batch != B) CGD_FAIL(ctx, "masked merge: mask must have batch 1 or B");
  if (mask_channels != 1 && mask_channels != 3) CGD_FAIL(ctx, "masked merge: mask must have 1 or 3 channels");
  if ((n_re != nullptr) != (x_re != nullptr)) CGD_FAIL(ctx, "masked merge: the re-noise draw and its output come together");
  if (!n_known && k.sqrt_one_minus_ab_prev != 0.f) CGD_FAIL(ctx, "masked merge: the known region's noise is missing (its coefficient is not 0)");
  const int present = (x0 ? CGD_MASK_PRED_XSTART : 0) | (n_known ? CGD_MASK_N_KNOWN : 0) | (n_re ? CGD_MASK_RENOISE : 0);
  if (k.flags != present) CGD_FAIL(ctx, "masked merge: the flags do not name the optional buffers that were passed");
  if ((long)H * W > INT32_MAX || (long)B * 3 > INT32_MAX) CGD_FAIL(ctx, "masked merge: a plane or the plane count exceeds 2^31 - 1");
  MergeArgs a = {sample, x0, init, mask, n_known, n_re, x_re, k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev, k.renoise_x, k.renoise_n};
  const int planes = B * 3, HW = H * W;
  plane_walk(HW, planes, [&](auto v, dim3 grid) {
    CGD_LAUNCH(masked_merge_kernel<decltype(v)::value>, grid, dim3(256), 0, s, a, planes, HW, init_batch, mask_batch, mask_channels);
  }, sample, x0, init, mask, n_known, n_re, x_re);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
