// Directional CLIP loss of a prompt-pair edit (StyleGAN-NADA, Gal et al. 2021; DiffusionCLIP, Kim et al. 2022) with its gradient, written
// without autograd like the spherical loss of guidance.hip.  Per embedding row r = cut * B + b, with e the generated image's embedding, s the
// source image's embedding of the same cutout and d_p unit text directions:
//   e^ = e / max(|e|, 1e-12)      s^ = s / max(|s|, 1e-12)      delta = e^ - s^      n = |delta|
//   cos_p = delta . d_p / n       if n > 1e-6, else 0 (the row then has no gradient: the direction of a zero vector is undefined)
//   loss_part[r] = c sum_p w_bp (1 - cos_p)                                                   c = clip_guidance_scale / cutn
//   d_emb[r] (+)= c (I - e^ e^T) [ sum_p -w_bp (d_p - cos_p delta / n) / n ] / max(|e|, 1e-12)
// The bracket is evaluated as (-(sum_p w_bp d_p) + (sum_p w_bp cos_p) delta / n) / n, so every direction row is read once.
// One wavefront per row; e^, delta and sum_p w_bp d_p live in registers (three arrays of 32 per lane: D <= 2048), reductions by __shfl_xor,
// no LDS.  The source embedding gets no gradient.  All tensors fp32.
#include "common.h"
#include "guidance.h"
#include "region_cov.h"

namespace {

// Instantiated without RG it is the plain loss, with the same arguments and machine code as before it was a template; with RG = RegionArgs
// (cgd_directional_loss_regions) w_bp is scaled by the coverage of the row's cut (region_cov.h), and a row whose every column is skipped has
// loss 0 and no gradient, like a row without a direction.
template <class... RG>
__global__ __launch_bounds__(64) void directional_loss_kernel(const float* __restrict__ emb, const float* __restrict__ src,
                                                              const float* __restrict__ dn /*unit rows*/, const float* __restrict__ wts,
                                                              float* __restrict__ demb, float* __restrict__ loss_part, int B, int Bs, int P,
                                                              int D, float coef, int accumulate, RG... rg) {
  constexpr bool REGIONS = sizeof...(RG) > 0;
  const int row = blockIdx.x, b = row % B, cut = row / B, lane = threadIdx.x;
  constexpr int MAXE = 32;  // D <= 2048
  const float* e = emb + (long)row * D;
  const float* sp = src + ((long)cut * Bs + (Bs == 1 ? 0 : b)) * D;
  float ev[MAXE], dv[MAXE], av[MAXE];
  float nn = 0.f, ss = 0.f;
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    const int c = lane + 64 * k;
    ev[k] = c < D ? e[c] : 0.f;
    dv[k] = c < D ? sp[c] : 0.f;
    av[k] = 0.f;
    nn += ev[k] * ev[k];
    ss += dv[k] * dv[k];
  }
  for (int o = 32; o > 0; o >>= 1) {
    nn += __shfl_xor(nn, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  const float inv = 1.f / fmaxf(sqrtf(nn), 1e-12f);
  const float invs = 1.f / fmaxf(sqrtf(ss), 1e-12f);
  float n2 = 0.f;
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    ev[k] *= inv;                    // e^
    dv[k] = ev[k] - dv[k] * invs;  // delta (exact zeros beyond D)
    n2 += dv[k] * dv[k];
  }
  for (int o = 32; o > 0; o >>= 1) n2 += __shfl_xor(n2, o, 64);
  const float n = sqrtf(n2);
  bool live = n > 1e-6f;
  const float invn = live ? 1.f / n : 0.f;
  float wsum = 0.f, wcos = 0.f;
  bool any = false;
  for (int p = 0; p < P; ++p) {
    float w = wts[(long)b * P + p];
    if constexpr (REGIONS) {
      if (w != 0.f) w *= region_weight(rg..., cut, p);
    }
    if (w == 0.f) continue;
    any = true;
    const float* y = dn + (long)p * D;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < MAXE; ++k) {
      const int c = lane + 64 * k;
      const float yv = c < D ? y[c] : 0.f;
      dot += dv[k] * yv;
      av[k] += w * yv;
    }
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    wsum += w;
    wcos += w * (dot * invn);  // cos_p = 0 on a row without a direction
  }
  if (lane == 0) loss_part[row] = REGIONS && !any ? 0.f : coef * (wsum - wcos);
  if constexpr (REGIONS) live = live && any;
  float* out = demb + (long)row * D;
  if (!live) {  // no gradient: exact zeros, or the accumulated values as they are
    if (!accumulate) {
#pragma unroll
      for (int k = 0; k < MAXE; ++k) {
        const int c = lane + 64 * k;
        if (c < D) out[c] = 0.f;
      }
    }
    return;
  }
  // g = (-(sum_p w d_p) + (sum_p w cos_p) delta / n) / n ;  de = c (I - e^ e^T) g / |e|
  const float f = wcos * invn;
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    av[k] = (f * dv[k] - av[k]) * invn;
    dot += av[k] * ev[k];
  }
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    const int c = lane + 64 * k;
    if (c < D) {
      const float v = coef * (av[k] - dot * ev[k]) * inv;
      out[c] = accumulate ? __fadd_rn(out[c], v) : v;  // (no contraction with the product above: the sum of the two launches' values)
    }
  }
}

}  // namespace

int cgd_launch_directional_loss(cgd_ctx* ctx, const float* emb, const float* src_emb, const float* dirs_n, const float* weights, float* demb,
                                float* loss_part, int cutn, int B, int Bs, int P, int D, float scale, int accumulate, hipStream_t s) {
  if (D > 2048) CGD_FAIL(ctx, "directional loss: embedding dim > 2048");
  if (Bs != 1 && Bs != B) CGD_FAIL(ctx, "directional loss: the source batch must be 1 or B");
  if (cutn < 1 || B < 1 || P < 1 || D < 1) CGD_FAIL(ctx, "directional loss: cutn, B, P and D must be positive");
  if (!emb || !src_emb || !dirs_n || !weights || !demb || !loss_part) CGD_FAIL(ctx, "directional loss: null pointer");
  CGD_LAUNCH(directional_loss_kernel<>, dim3(cutn * B), dim3(64), 0, s, emb, src_emb, dirs_n, weights, demb, loss_part, B, Bs, P, D,
             scale / (float)cutn, accumulate ? 1 : 0);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_directional_loss_regions(cgd_ctx* ctx, const float* emb, const float* src_emb, const float* dirs_n, const float* weights,
                                        float* demb, float* loss_part, int cutn, int B, int Bs, int P, int D, float scale, int accumulate,
                                        const cgd_regions& rg, hipStream_t s) {
  if (D > 2048) CGD_FAIL(ctx, "directional loss: embedding dim > 2048");
  if (Bs != 1 && Bs != B) CGD_FAIL(ctx, "directional loss: the source batch must be 1 or B");
  if (cutn < 1 || B < 1 || P < 1 || D < 1) CGD_FAIL(ctx, "directional loss: cutn, B, P and D must be positive");
  if (!emb || !src_emb || !dirs_n || !weights || !demb || !loss_part) CGD_FAIL(ctx, "directional loss: null pointer");
  CGD_TRY(cgd_check_regions(ctx, rg, P));
  CGD_LAUNCH(directional_loss_kernel<RegionArgs>, dim3(cutn * B), dim3(64), 0, s, emb, src_emb, dirs_n, weights, demb, loss_part, B, Bs, P, D,
             scale / (float)cutn, accumulate ? 1 : 0, RegionArgs{rg.sat, rg.region_of, rg.power, rg.geo, rg.H, rg.W});
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
