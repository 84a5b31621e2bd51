// Gram matrices of tall-skinny activations on MI355X: per sample G = scale * A^T A for A [B * N][C] (fp32 rows, row stride lda >= C), C in
// {64, 128, 256, 512}, any N >= 1: the contraction of the VGG style loss (lpips.hip), where K runs over up to 65536 pixels and the output is
// 64 x 64 .. 512 x 512.  Nothing else in the library is shaped for it (the GEMM kernels split K at most a few ways and want K-contiguous operands).
//   gram_slab_kernel  : K (pixels) is split over workgroups in slabs of SR = 16384 / C rows (64 KB of LDS, two workgroups per CU); a slab never
//                       spans two samples, rows beyond N come in as zeros (out-of-range buffer-load offsets).  The slab is staged through LDS once
//                       and every output tile is contracted from it on exact fp32 products (v_mfma_f32_32x32x2_f32: a pixel is the MFMA's k, so
//                       both operands are plain 4-byte LDS reads of 32 consecutive channels, conflict-free without padding).  Only the tiles on or
//                       below the diagonal are computed; a wavefront owns one (32 MB)^2 tile at a time (MB = 1 at C = 64, else 2).  With few slabs
//                       (the deep taps) the tile list is dealt over gridDim.y workgroups per slab, each of which stages the slab (from L2).
//   gram_finish_kernel: sums the slab partials in a fixed order (four interleaved chains per element, combined as (0 + 1) + (2 + 3)), mirrors the
//                       lower triangle and writes G, or D = gk (G - Gs) with per-workgroup partial sums of (G - Gs)^2.  No floating-point atomics:
//                       results are bit-identical from run to run.
#include <algorithm>

#include "kernels.h"
#include "mfma_stage.h"

namespace {

constexpr int GRAM_LDS_FLOATS = 16384;  // one slab: 64 KB

template <int C, int MB>
__global__ __launch_bounds__(256) void gram_slab_kernel(const float* __restrict__ A, long lda, int N, float* __restrict__ part) {
  constexpr int SR = GRAM_LDS_FLOATS / C;  // rows per slab
  constexpr int TS = 32 * MB, T = C / TS, NT = T * (T + 1) / 2;
  constexpr int CQ = C / 4;
  __shared__ float sm[SR * C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slab = blockIdx.x, nslab = gridDim.x, b = blockIdx.z;
  const int row0 = slab * SR;
  const int nvalid = min(SR, N - row0);
  const float* base = A + ((long)b * N + row0) * lda;
  const unsigned records = (unsigned)(((long)(nvalid - 1) * lda + C) * 4);  // bytes up to the end of the slab's last valid row
  const __amdgpu_buffer_rsrc_t rs = cgd_buf_rsrc(base, records);
#pragma unroll
  for (int it = 0; it < SR * CQ / 256; ++it) {
    const int q = it * 256 + tid, row = q / CQ, cq = q - row * CQ;
    // a row >= nvalid lies at or beyond `records`: the load returns zeros and touches no memory
    *(cgd_i32x4*)&sm[row * C + cq * 4] = cgd_buf_load16(rs, (int)((row * lda + cq * 4) * 4), 0);
  }
  __syncthreads();
  const int kend = (nvalid + 7) & ~7;  // eight rows (four MFMA steps) per trip; the rows in [nvalid, kend) are zeros, kend <= SR
  const int l31 = lane & 31, hh = lane >> 5;
  float* out = part + ((long)b * nslab + slab) * NT * (TS * TS);
  for (int t = blockIdx.y * 4 + wave; t < NT; t += 4 * gridDim.y) {
    int ti = 0, tj = t;  // t = ti (ti + 1) / 2 + tj, tj <= ti
    while (tj > ti) {
      tj -= ti + 1;
      ++ti;
    }
    cgd_f32x16 acc[MB][MB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int j = 0; j < MB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const float* pa = sm + hh * C + ti * TS + l31;
    const float* pb = sm + hh * C + tj * TS + l31;
    for (int k8 = 0; k8 < kend; k8 += 8) {
#pragma unroll
      for (int u = 0; u < 8; u += 2) {
        const int k = k8 + u;
        float a[MB], bb[MB];
#pragma unroll
        for (int i = 0; i < MB; ++i) {
          a[i] = pa[k * C + 32 * i];
          bb[i] = pb[k * C + 32 * i];
        }
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
          for (int j = 0; j < MB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bb[j], acc[i][j], 0, 0, 0);
      }
    }
    // tile element [row = channel of ti][col = channel of tj]; accumulator register r of lane (l31, hh) is row (r & 3) + 8 (r >> 2) + 4 hh, col l31
    float* o = out + (long)t * (TS * TS);
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
      for (int j = 0; j < MB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[(32 * i + (r & 3) + 8 * (r >> 2) + 4 * hh) * TS + 32 * j + l31] = acc[i][j][r];
  }
}

// 64 outputs per workgroup, four wavefronts = four interleaved slab chains per output.  LOSS: out = gk (scale sum - Gs) and
// lpart[b * lstride + blockIdx.x] = lw * sum over the 64 outputs of (scale sum - Gs)^2; else out = scale sum.
template <bool LOSS>
__global__ __launch_bounds__(256) void gram_finish_kernel(const float* __restrict__ part, int nslab, int C, int TS, float scale, float* __restrict__ out,
                                                          const float* __restrict__ Gs, float gk, float lw, float* __restrict__ lpart, long lstride) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, q = threadIdx.x >> 6, b = blockIdx.y;
  const int o = blockIdx.x * 64 + lane, i = o / C, j = o - i * C;
  const int hi = max(i, j), lo = min(i, j);  // the lower triangle holds the value: G is exactly symmetric
  const int T = C / TS, NT = T * (T + 1) / 2, ti = hi / TS, tj = lo / TS;
  const long tile = (long)TS * TS, off = (long)(ti * (ti + 1) / 2 + tj) * tile + (hi - ti * TS) * TS + (lo - tj * TS);
  const float* p = part + (long)b * nslab * NT * tile + off;
  float s = 0.f;
#pragma unroll 8
  for (int k = q; k < nslab; k += 4) s += p[(long)k * NT * tile];
  red[q][lane] = s;
  __syncthreads();
  if (q) return;
  const float v = ((red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane])) * scale;
  if (!LOSS) {
    out[(long)b * C * C + o] = v;
    return;
  }
  const float d = v - Gs[o];
  out[(long)b * C * C + o] = gk * d;
  float l = d * d;
  for (int m = 32; m > 0; m >>= 1) l += __shfl_xor(l, m, 64);
  if (lane == 0) lpart[(long)b * lstride + blockIdx.x] = lw * l;
}

}  // namespace

int cgd_gram_loss_parts(int C) { return C * C / 64; }

int cgd_launch_gram(cgd_ctx* ctx, const float* A, int lda, int B, int N, int C, float scale, float* out, const float* Gs, float gk, float lw,
                    float* lpart, long lstride, hipStream_t s) {
  if (C != 64 && C != 128 && C != 256 && C != 512) CGD_FAIL(ctx, "gram: C must be 64, 128, 256 or 512");
  if (B < 1 || N < 1) CGD_FAIL(ctx, "gram: B and N must be at least 1");
  if (lda < C || (lda & 3) || lda > (1 << 20)) CGD_FAIL(ctx, "gram: lda must be a multiple of 4 in [C, 2^20]");
  if (((uintptr_t)A & 15) || !out) CGD_FAIL(ctx, "gram: A must be 16-byte aligned");
  if (Gs && !lpart) CGD_FAIL(ctx, "gram: the loss form needs a partial-sum buffer");
  CGD_TRY(cgd_flush_pending(ctx, s));  // the slab partials go into the split-K workspace
  const int SR = GRAM_LDS_FLOATS / C, TS = C == 64 ? 32 : 64, T = C / TS, NT = T * (T + 1) / 2;
  const int nslab = cdiv(N, SR);
  const size_t per_sample = (size_t)nslab * NT * TS * TS * sizeof(float);
  const int bmax = (int)std::min<size_t>(ctx->ws_bytes / per_sample, 65535);
  if (bmax < 1) CGD_FAIL(ctx, "gram: the slab partials of one sample do not fit the workspace");
  for (int b0 = 0; b0 < B; b0 += bmax) {
    const int nb = std::min(bmax, B - b0);
    // about two workgroups per CU: with few slabs the tile list is dealt over several workgroups per slab
    const int nsplit = std::max(1, std::min(cdiv(NT, 4), cdiv(2L * ctx->num_cu, (long)nb * nslab)));
    const float* Ab = A + (long)b0 * N * lda;
    const dim3 grid(nslab, nsplit, nb);
    switch (C) {
      case 64: CGD_LAUNCH((gram_slab_kernel<64, 1>), grid, dim3(256), 0, s, Ab, (long)lda, N, ctx->ws); break;
      case 128: CGD_LAUNCH((gram_slab_kernel<128, 2>), grid, dim3(256), 0, s, Ab, (long)lda, N, ctx->ws); break;
      case 256: CGD_LAUNCH((gram_slab_kernel<256, 2>), grid, dim3(256), 0, s, Ab, (long)lda, N, ctx->ws); break;
      default: CGD_LAUNCH((gram_slab_kernel<512, 2>), grid, dim3(256), 0, s, Ab, (long)lda, N, ctx->ws); break;
    }
    float* ob = out + (long)b0 * C * C;
    if (Gs)
      CGD_LAUNCH((gram_finish_kernel<true>), dim3(C * C / 64, nb), dim3(256), 0, s, ctx->ws, nslab, C, TS, scale, ob, Gs, gk, lw,
                 lpart + (long)b0 * lstride, lstride);
    else
      CGD_LAUNCH((gram_finish_kernel<false>), dim3(C * C / 64, nb), dim3(256), 0, s, ctx->ws, nslab, C, TS, scale, ob, nullptr, 0.f, 0.f, nullptr, 0L);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
