// Aesthetic-predictor guidance on the CLIP image embeddings (the LAION aesthetic predictors: a head that is affine in the normalised embedding),
// with its gradient, written without autograd like the spherical loss of guidance.hip and the directional loss of direction.hip.  Per embedding
// row r = cut * B + b, with e the row of emb and the head (a, beta) stored as D + 1 floats (a, then beta):
//   e^ = e / max(|e|, 1e-12)      s_r = a . e^ + beta  (the predicted score of the cutout)      c = scale / cutn
//   loss_part[r] = -c s_r
//   d_emb[r] (+)= -c (a - (a . e^) e^) / max(|e|, 1e-12)
//   score[r]     = s_r            (optional: a null pointer is not written)
// A row of exact zeros has s_r = beta and no gradient (exact zeros, or the accumulated values as they are), like direction.hip's row without a
// direction; F.normalize's autograd would return a * 1e12 there.  One wavefront per row; e^ and a live in registers (two arrays of 32 per lane:
// D <= 2048, element lane + 64 k), reductions by __shfl_xor in a fixed order, no LDS, no atomics.  All tensors fp32.
#include "common.h"
#include "guidance.h"

namespace {

__global__ __launch_bounds__(64) void aesthetic_loss_kernel(const float* __restrict__ emb, const float* __restrict__ head,
                                                            float* __restrict__ demb, float* __restrict__ loss_part, float* __restrict__ score,
                                                            int D, float coef, int accumulate) {
  const int row = blockIdx.x, lane = threadIdx.x;
  constexpr int MAXE = 32;  // D <= 2048
  const float* e = emb + (long)row * D;
  float ev[MAXE], av[MAXE];
  float nn = 0.f;
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    const int c = lane + 64 * k;
    ev[k] = c < D ? e[c] : 0.f;
    av[k] = c < D ? head[c] : 0.f;
    nn += ev[k] * ev[k];
  }
  for (int o = 32; o > 0; o >>= 1) nn += __shfl_xor(nn, o, 64);
  const float norm = sqrtf(nn);
  const float inv = 1.f / fmaxf(norm, 1e-12f);
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    ev[k] *= inv;  // e^ (exact zeros beyond D, and everywhere on a zero row)
    dot += av[k] * ev[k];
  }
  for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
  const float s = dot + head[D];
  const float nc = -coef;
  if (lane == 0) {
    loss_part[row] = nc * s;
    if (score) score[row] = s;
  }
  float* out = demb + (long)row * D;
  if (!(norm > 0.f)) {  // no gradient: exact zeros, or the accumulated values as they are
    if (!accumulate) {
#pragma unroll
      for (int k = 0; k < MAXE; ++k) {
        const int c = lane + 64 * k;
        if (c < D) out[c] = 0.f;
      }
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < MAXE; ++k) {
    const int c = lane + 64 * k;
    if (c < D) {
      const float v = nc * (av[k] - dot * ev[k]) * inv;
      out[c] = accumulate ? __fadd_rn(out[c], v) : v;  // (no contraction with the product above: the sum of the launches' values)
    }
  }
}

}  // namespace

// refusals go to the context's error string when there is a context: the arguments are judged before the context is needed (as in warp.hip), so
// a caller without a GPU still learns that they are refused
#define AES_FAIL(ctx, msg)            \
  do {                                \
    if (ctx) (ctx)->err = (msg);      \
    return -2;                        \
  } while (0)

int cgd_launch_aesthetic_loss(cgd_ctx* ctx, const float* emb, const float* head, float* demb, float* loss_part, float* score, int cutn, int B,
                              int D, float scale, int accumulate, hipStream_t s) {
  if (D > 2048) AES_FAIL(ctx, "aesthetic loss: embedding dim > 2048");
  if (cutn < 1 || B < 1 || D < 1) AES_FAIL(ctx, "aesthetic loss: cutn, B and D must be positive");
  if ((long)cutn * B > 2147483647L) AES_FAIL(ctx, "aesthetic loss: cutn * B does not fit a grid");
  if (!emb || !head || !demb || !loss_part) AES_FAIL(ctx, "aesthetic loss: null pointer");
  if (!ctx) return -3;
  CGD_LAUNCH(aesthetic_loss_kernel, dim3(cutn * B), dim3(64), 0, s, emb, head, demb, loss_part, score, D, scale / (float)cutn,
             accumulate ? 1 : 0);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
