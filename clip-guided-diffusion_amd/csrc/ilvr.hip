// ILVR (Choi et al., 2021): the refinement that follows every sampler update when sampling is conditioned on a reference image's low
// frequencies.  With D the (n / N, n) antialiased cubic down-resize and U the (n, n / N) cubic up-resize of an extent n (ResizeRight,
// pad_mode='constant': taps outside the extent read zero, rows are not renormalised; the rows of resize_rows.h), P = U D per axis and
// phi(z) = P_H z P_W^T per plane:
//   known        = sa * ref + sb * noise                       (two rounded products and a rounded sum, not fused; as mask.hip)
//   sample      += phi(known - sample)
//   pred_xstart += phi(ref   - pred_xstart)                    (when pred_xstart is passed)
// sample, pred_xstart, noise: NCHW fp32 (B,3,H,W); ref (1 or B,3,H,W); scratch: one (B,3,H/N,W/N) low-resolution image per pair.
//
// Two launches, whatever B; the pred_xstart pair rides in both as grid.z = 1.
//   down: one workgroup per (low-resolution row i, plane, pair).  The difference d is formed on load.  Vertical pass: the 4N taps of row i
//         are cut into S segments, work item (segment, column) sums its taps in order into LDS, then the S partial sums of a column are added
//         in order.  Horizontal pass: G = min(4N, 64) lanes share an output, lane l summing taps l, l + G, ... in order, then a fixed butterfly.
//   up:   every frame pixel gathers its 4 x 4 low-resolution taps and adds the sum in place.
// Gather form, no atomics, fixed summation order: the same bits on every run.  The weight rows are built in LDS from (extent, factor):
// a down row of an exact factor is the same for every output, shifted by N (left_o = left_0 + o N, the tap distances do not depend on
// o), so one row of 4N weights per axis serves a workgroup; the up rows repeat with period N (left_o = left_{o mod N} + o / N).
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "kernels.h"
#include "resize_rows.h"

#include <algorithm>

namespace {

constexpr int ILVR_MAX_LDS = 64 * 1024;  // bytes of dynamic LDS a launch may ask for
constexpr int ILVR_DOWN_THREADS = 1024;  // most threads of a down workgroup

struct IlvrArgs {
  float* sample;
  float* x0;           // or null
  const float* ref;
  const float* noise;  // or null (then known = sa * ref)
  float* low;          // [pairs][B * 3][H / N][W / N]
  float sa, sb;
};

// as known_value of mask.hip: contraction off, so a host reproduces the value bit for bit
__device__ __forceinline__ float ilvr_known(float sa, float rv, float sb, float nv, bool with_noise) {
#pragma clang fp contract(off)
  const float a = sa * rv;
  if (!with_noise) return a;
  const float b = sb * nv;
  return a + b;
}

// the down row of extent n and factor N into w[0 .. 4N-1] with resize_row's arithmetic stated for a workgroup: the kernel values in
// parallel, their sum by one thread in tap order, the scaling in parallel.  `inv`: one float of LDS.  Ends behind a barrier.
__device__ inline void ilvr_down_row(int n, int N, float* w, float* inv, int tid, int nt) {
#pragma clang fp contract(off)
  const int T = 4 * N, m = n / N;
  const int left = resize_left(n, m, 0);
  for (int t = tid; t < T; t += nt) w[t] = resize_k(n, m, 0, left + t);
  __syncthreads();
  if (tid == 0) {
    float sum = 0.f;
    for (int t = 0; t < T; ++t) sum += w[t];
    *inv = 1.f / (sum == 0.f ? 1.f : sum);
  }
  __syncthreads();
  const float s = *inv;
  for (int t = tid; t < T; t += nt) w[t] *= s;
  __syncthreads();
}

// LDS: wy [4N] | wx [4N] | part [S][W] | v [W] | inv [1]
// grid.x = low-resolution row, grid.y = plane b * 3 + c, grid.z = pair (0 sample, 1 pred_xstart); blockDim.x a multiple of 64
__global__ __launch_bounds__(ILVR_DOWN_THREADS) void ilvr_down_kernel(IlvrArgs a, int planes, int H, int W, int N, int S, int ref_b) {
  extern __shared__ __align__(16) float lds[];
  const int T = 4 * N, Hl = H / N, Wl = W / N;
  float* wy = lds;
  float* wx = wy + T;
  float* part = wx + T;
  float* v = part + S * W;
  float* inv = v + W;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int i = blockIdx.x, p = blockIdx.y, pair = blockIdx.z;
  ilvr_down_row(H, N, wy, inv, tid, nt);
  ilvr_down_row(W, N, wx, inv, tid, nt);
  const int b = p / 3, c = p - 3 * b;
  const long HW = (long)H * W;
  const float* cur = (pair ? a.x0 : a.sample) + (long)p * HW;
  const float* ref = a.ref + (long)((ref_b == 1 ? 0 : b) * 3 + c) * HW;
  const bool with_noise = !pair && a.noise != nullptr;
  const float* noi = with_noise ? a.noise + (long)p * HW : nullptr;
  const float sa = pair ? 1.f : a.sa;
  // vertical pass: part[seg][x] = sum over the segment's taps t, in order, of wy[t] * d[y0 + t][x]; taps outside the frame read zero
  const int y0 = i * N + resize_left(H, Hl, 0), seg_len = T / S;
  for (int e = tid; e < S * W; e += nt) {
    const int seg = e / W, x = e - seg * W;
    const int t_lo = max(seg * seg_len, -y0), t_hi = min((seg + 1) * seg_len, H - y0);
    float acc = 0.f;
#pragma unroll 4
    for (int t = t_lo; t < t_hi; ++t) {
      const long q = (long)(y0 + t) * W + x;
      const float d = ilvr_known(sa, ref[q], a.sb, with_noise ? noi[q] : 0.f, with_noise) - cur[q];
      acc += wy[t] * d;
    }
    part[seg * W + x] = acc;
  }
  __syncthreads();
  for (int x = tid; x < W; x += nt) {
    float s = part[x];
    for (int seg = 1; seg < S; ++seg) s += part[seg * W + x];
    v[x] = s;
  }
  __syncthreads();
  // horizontal pass: G lanes per output column j (consecutive lanes read consecutive LDS words)
  const int G = T < 64 ? T : 64;
  const int sub = tid & (G - 1), grp = tid / G, ngrp = nt / G;
  const int x_left = resize_left(W, Wl, 0);
  float* low = a.low + (((long)pair * planes + p) * Hl + i) * Wl;
  for (int j0 = 0; j0 < Wl; j0 += ngrp) {  // (uniform per workgroup: every lane reaches the butterfly)
    const int j = j0 + grp;
    const bool live = j < Wl;
    const int x0 = j * N + x_left;
    float acc = 0.f;
    if (live) {
      for (int t = sub; t < T; t += G) {
        const int xx = x0 + t;
        if ((unsigned)xx < (unsigned)W) acc += wx[t] * v[xx];
      }
    }
    for (int o = 1; o < G; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (live && sub == 0) low[j] = acc;
  }
}

// LDS: wyT [4][N] | wxT [4][N] | lefty [N] | leftx [N]: the up rows of the N phases, tap-major (consecutive lanes, consecutive phases)
// grid.x walks the plane's pixels, grid.y = plane, grid.z = pair
__global__ __launch_bounds__(256) void ilvr_up_kernel(IlvrArgs a, int planes, int H, int W, int N) {
  extern __shared__ __align__(16) float lds[];
  const int Hl = H / N, Wl = W / N, tid = threadIdx.x;
  float* wyT = lds;
  float* wxT = wyT + 4 * N;
  int* lefty = (int*)(wxT + 4 * N);
  int* leftx = lefty + N;
  for (int e = tid; e < 2 * N; e += 256) {
    const int ph = e < N ? e : e - N;
    float w[4];
    const int left = resize_row(e < N ? Hl : Wl, e < N ? H : W, ph, 4, w);
    float* dst = e < N ? wyT : wxT;
#pragma unroll
    for (int t = 0; t < 4; ++t) dst[t * N + ph] = w[t];
    (e < N ? lefty : leftx)[ph] = left;
  }
  __syncthreads();
  const int p = blockIdx.y, pair = blockIdx.z;
  const long HW = (long)H * W;
  float* out = (pair ? a.x0 : a.sample) + (long)p * HW;
  const float* low = a.low + ((long)pair * planes + p) * Hl * Wl;
  for (long q = (long)blockIdx.x * 256 + tid; q < HW; q += (long)gridDim.x * 256) {
    const int y = (int)(q / W), x = (int)(q - (long)y * W);
    const int ky = y / N, py = y - ky * N, kx = x / N, px = x - kx * N;
    const int ly = lefty[py] + ky, lx = leftx[px] + kx;
    float acc = 0.f;
#pragma unroll
    for (int ty = 0; ty < 4; ++ty) {
      const int yy = ly + ty;
      if ((unsigned)yy >= (unsigned)Hl) continue;
      float r = 0.f;
#pragma unroll
      for (int tx = 0; tx < 4; ++tx) {
        const int xx = lx + tx;
        if ((unsigned)xx < (unsigned)Wl) r += wxT[tx * N + px] * low[yy * Wl + xx];
      }
      acc += wyT[ty * N + py] * r;
    }
    if (acc != 0.f) out[q] += acc;  // a zero correction leaves the bits alone (-0 + 0 would turn into +0)
  }
}

bool ilvr_factor_ok(int H, int W, int N) { return N >= 2 && N <= 64 && (N & (N - 1)) == 0 && H % N == 0 && W % N == 0; }

}  // namespace

long cgd_ilvr_scratch(int B, int H, int W, int factor, int with_x0) {
  if (B <= 0 || H <= 0 || W <= 0 || !ilvr_factor_ok(H, W, factor)) return 0;
  return (with_x0 ? 2L : 1L) * B * 3 * (H / factor) * (W / factor);
}

int cgd_launch_ilvr_refine(cgd_ctx* ctx, float* sample, float* x0, const float* ref, const float* noise, float* scratch, int B, int H, int W,
                           int ref_batch, int factor, float sa, float sb, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) CGD_FAIL(ctx, "ilvr refine: empty shape");
  if (!sample || !ref || !scratch) CGD_FAIL(ctx, "ilvr refine: sample, ref and scratch are required");
  if (!ilvr_factor_ok(H, W, factor)) CGD_FAIL(ctx, "ilvr refine: the factor must be a power of two in [2, 64] that divides H and W");
  if (ref_batch != 1 && ref_batch != B) CGD_FAIL(ctx, "ilvr refine: ref must have batch 1 or B");
  if (!noise && sb != 0.f) CGD_FAIL(ctx, "ilvr refine: the reference's noise is missing (its coefficient is not 0)");
  if ((long)H * W > INT32_MAX || (long)B * 3 > 65535 || H / factor > 65535)
    CGD_FAIL(ctx, "ilvr refine: a plane exceeds 2^31 - 1 pixels or the grid 65535 planes or low-resolution rows");
  const int N = factor, T = 4 * N, planes = B * 3, pairs = x0 ? 2 : 1;
  // tap segments of the vertical pass: as many as fill the workgroup (a power of two, so it divides 4N)
  int S = 1;
  while (2 * S <= T && (long)2 * S * W <= ILVR_DOWN_THREADS) S *= 2;
  const int threads = (int)std::min<long>(ILVR_DOWN_THREADS, ((long)S * W + 63) / 64 * 64);
  const size_t lds_down = (2 * (size_t)T + (size_t)S * W + W + 1) * 4, lds_up = 10 * (size_t)N * 4;
  if (lds_down > ILVR_MAX_LDS) CGD_FAIL(ctx, "ilvr refine: a frame row does not fit the LDS");
  IlvrArgs a = {sample, x0, ref, sb != 0.f ? noise : nullptr, scratch, sa, sb};
  CGD_LAUNCH(ilvr_down_kernel, dim3(H / N, planes, pairs), dim3(threads), lds_down, s, a, planes, H, W, N, S, ref_batch);
  const int gx = (int)std::min<long>(cdiv((long)H * W, 256), 4096);
  CGD_LAUNCH(ilvr_up_kernel, dim3(gx, planes, pairs), dim3(256), lds_up, s, a, planes, H, W, N);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
