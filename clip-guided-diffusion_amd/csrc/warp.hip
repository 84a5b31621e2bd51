// 2D animation (Disco Diffusion's 2D mode, Deforum): what runs once per frame between two sampling runs.  Three plane kernels on NCHW fp32.
//   frame warp:    dst[b,c,y,x] = interp(src[b,c], sx, sy), (sx, sy) = (m0 x + m1 y + m2, m3 x + m4 y + m5): the host's inverse map, pixel
//                  centres on integers.  The coordinates, their floor and the fractions are fp64 (an fp32 coordinate near x = 500 is 3e-5 px
//                  off, which on a noisy state is the project's tolerance); the fractions then become fp32, and weights and sums are fp32.
//                  Bilinear (taps floor, floor + 1) or bicubic (Keys kernel, a = -0.75: OpenCV's INTER_CUBIC, torch's bicubic; NOT the
//                  a = -0.5 of resize_rows.h; taps floor - 1 .. floor + 2), separable: the x taps of a row are summed in ascending order, then
//                  the row results in ascending y.  Every tap index goes through the border rule on its own: wrap (i mod n), reflect without
//                  repeating the edge (period 2 (n - 1): OpenCV's REFLECT_101, torch's reflection with align_corners=True) or replicate.
//                  At fraction 0 the weights are exactly (1, 0) / (0, 1, 0, 0): the identity and integer shifts copy bits.
//   channel stats: per plane (mean, population standard deviation); sums of x and x^2 in fp64, thread t summing elements t, t + T, ... in
//                  order, then a fixed tree over the T threads.  One workgroup per plane.
//   color match:   x <- x + amount ((mu_ref + (x - mu_x) r) - x) in place, r = sigma_ref / sigma_x (1 where sigma_x < 1e-6).
// Gather form, no atomics, no scratch buffer: the same bits on every run.  Plane offsets are 64-bit; a plane holds fewer than 2^31 pixels.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "kernels.h"
#include "warp_sample.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace {

constexpr int STATS_THREADS = 1024;

struct WarpArgs {
  double m[6];
  int interp, border, clamp;
};

// grid.x walks the plane's pixels, grid.y the planes (stride loop)
template <int INTERP, int BORDER>
__global__ __launch_bounds__(WARP_THREADS) void frame_warp_kernel(const float* __restrict__ src, float* __restrict__ dst, long planes, int H,
                                                                  int W, WarpArgs a) {
  const long HW = (long)H * W;
  const long q = (long)blockIdx.x * WARP_THREADS + threadIdx.x;
  if (q >= HW) return;
  const int y = (int)(q / W), x = (int)(q - (long)y * W);
  double sx, sy;
  {
#pragma clang fp contract(off)
    sx = a.m[0] * (double)x + a.m[1] * (double)y + a.m[2];
    sy = a.m[3] * (double)x + a.m[4] * (double)y + a.m[5];
  }
  const double fx0 = floor(sx), fy0 = floor(sy);
  const float tx = (float)(sx - fx0), ty = (float)(sy - fy0);
  const int ix = (int)fx0, iy = (int)fy0;
  if (INTERP == 0) {
    const int x0 = warp_index<BORDER>(ix, W), x1 = warp_index<BORDER>(ix + 1, W);
    const int r0 = warp_index<BORDER>(iy, H) * W, r1 = warp_index<BORDER>(iy + 1, H) * W;
    const float wx0 = 1.f - tx, wy0 = 1.f - ty;
    for (long p = blockIdx.y; p < planes; p += gridDim.y) {
      const float* s = src + p * HW;
      float a0 = wx0 * s[r0 + x0];
      a0 += tx * s[r0 + x1];
      float a1 = wx0 * s[r1 + x0];
      a1 += tx * s[r1 + x1];
      float v = wy0 * a0;
      v += ty * a1;
      if (a.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
      dst[p * HW + q] = v;
    }
  } else {
    const int x0 = warp_index<BORDER>(ix - 1, W), x1 = warp_index<BORDER>(ix, W), x2 = warp_index<BORDER>(ix + 1, W),
              x3 = warp_index<BORDER>(ix + 2, W);
    const int r0 = warp_index<BORDER>(iy - 1, H) * W, r1 = warp_index<BORDER>(iy, H) * W, r2 = warp_index<BORDER>(iy + 1, H) * W,
              r3 = warp_index<BORDER>(iy + 2, H) * W;
    float wx0, wx1, wx2, wx3, wy0, wy1, wy2, wy3;
    cubic_weights(tx, wx0, wx1, wx2, wx3);
    cubic_weights(ty, wy0, wy1, wy2, wy3);
    for (long p = blockIdx.y; p < planes; p += gridDim.y) {
      const float* s = src + p * HW;
#define WARP_ROW(r) (((wx0 * s[(r) + x0] + wx1 * s[(r) + x1]) + wx2 * s[(r) + x2]) + wx3 * s[(r) + x3])
      const float a0 = WARP_ROW(r0), a1 = WARP_ROW(r1), a2 = WARP_ROW(r2), a3 = WARP_ROW(r3);
#undef WARP_ROW
      float v = ((wy0 * a0 + wy1 * a1) + wy2 * a2) + wy3 * a3;
      if (a.clamp) v = fminf(fmaxf(v, -1.f), 1.f);
      dst[p * HW + q] = v;
    }
  }
}

// one workgroup per plane (stride loop over grid.x); stats [planes][2] = (mean, population standard deviation)
__global__ __launch_bounds__(STATS_THREADS) void channel_stats_kernel(const float* __restrict__ x, float* __restrict__ stats, long planes,
                                                                      long HW) {
  __shared__ double s1[STATS_THREADS], s2[STATS_THREADS];
  const int tid = threadIdx.x;
  for (long p = blockIdx.x; p < planes; p += gridDim.x) {
    const float* xp = x + p * HW;
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (long q = tid; q < HW; q += STATS_THREADS) {
      const double v = (double)xp[q];
      a += v;
      b += v * v;
    }
    s1[tid] = a;
    s2[tid] = b;
    __syncthreads();
    for (int o = STATS_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) {
        s1[tid] += s1[tid + o];
        s2[tid] += s2[tid + o];
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double mean = s1[0] / (double)HW;
      const double var = s2[0] / (double)HW - mean * mean;
      stats[2 * p] = (float)mean;
      stats[2 * p + 1] = (float)sqrt(var > 0.0 ? var : 0.0);
    }
    __syncthreads();  // the sums are read before the next plane overwrites them
  }
}

// grid.x walks the plane's pixels, grid.y the planes (stride loop)
__global__ __launch_bounds__(WARP_THREADS) void color_match_kernel(float* __restrict__ x, const float* __restrict__ stats_x,
                                                                   const float* __restrict__ stats_ref, long planes, int C, long HW,
                                                                   int ref_batch, float amount, int clamp) {
  const long q = (long)blockIdx.x * WARP_THREADS + threadIdx.x;
  if (q >= HW) return;
  for (long p = blockIdx.y; p < planes; p += gridDim.y) {
    const long pr = ref_batch == 1 ? p % C : p;
    const float mx = stats_x[2 * p], sdx = stats_x[2 * p + 1];
    const float mr = stats_ref[2 * pr], sdr = stats_ref[2 * pr + 1];
    const float r = sdx < 1e-6f ? 1.f : sdr / sdx;
    const float v = x[p * HW + q];
    const float d = amount * ((mr + (v - mx) * r) - v);
    float o = d != 0.f ? v + d : v;  // a zero correction leaves the bits alone
    if (clamp) o = fminf(fmaxf(o, -1.f), 1.f);
    x[p * HW + q] = o;
  }
}

// refusals go to the context's error string when there is a context: the arguments are judged before the context is needed, so a caller
// without a GPU still learns that they are refused
#define WARP_FAIL(ctx, msg)           \
  do {                                \
    if (ctx) (ctx)->err = (msg);      \
    return -2;                        \
  } while (0)

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

const char* shape_error(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return "sizes must be positive";
  if ((long)H * W >= (1L << 31)) return "a plane must hold fewer than 2^31 pixels";
  if ((long)B * C >= (1L << 31)) return "B * C must stay below 2^31";
  return nullptr;
}

template <int INTERP>
void launch_warp(int border, dim3 grid, hipStream_t s, const float* src, float* dst, long planes, int H, int W, const WarpArgs& a) {
  if (border == 0) CGD_LAUNCH((frame_warp_kernel<INTERP, 0>), grid, dim3(WARP_THREADS), 0, s, src, dst, planes, H, W, a);
  else if (border == 1) CGD_LAUNCH((frame_warp_kernel<INTERP, 1>), grid, dim3(WARP_THREADS), 0, s, src, dst, planes, H, W, a);
  else CGD_LAUNCH((frame_warp_kernel<INTERP, 2>), grid, dim3(WARP_THREADS), 0, s, src, dst, planes, H, W, a);
}

}  // namespace

int cgd_launch_frame_warp(cgd_ctx* ctx, const float* src, float* dst, int B, int C, int H, int W, const cgd_warp* w, hipStream_t s) {
  if (!src || !dst || !w) WARP_FAIL(ctx, "frame warp: src, dst and the warp are required");
  if (src == dst) WARP_FAIL(ctx, "frame warp: dst must not alias src");
  if (misaligned(src) || misaligned(dst)) WARP_FAIL(ctx, "frame warp: pointers must be 4-byte aligned");
  if (const char* e = shape_error(B, C, H, W)) WARP_FAIL(ctx, std::string("frame warp: ") + e);
  if (w->interp != 0 && w->interp != 1) WARP_FAIL(ctx, "frame warp: interp must be 0 (bilinear) or 1 (bicubic)");
  if (w->border < 0 || w->border > 2) WARP_FAIL(ctx, "frame warp: border must be 0 (wrap), 1 (reflect) or 2 (replicate)");
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(w->m[i])) WARP_FAIL(ctx, "frame warp: the matrix has a non-finite entry");
  for (int k = 0; k < 4; ++k) {  // the map is affine: its extremes over the frame are at the corners
    const double x = (k & 1) ? W - 1 : 0, y = (k & 2) ? H - 1 : 0;
    const double sx = w->m[0] * x + w->m[1] * y + w->m[2], sy = w->m[3] * x + w->m[4] * y + w->m[5];
    if (!(std::fabs(sx) <= WARP_MAX_COORD) || !(std::fabs(sy) <= WARP_MAX_COORD))
      WARP_FAIL(ctx, "frame warp: the matrix maps a frame corner beyond +-2^30");
  }
  if (!ctx) return -3;
  WarpArgs a;
  for (int i = 0; i < 6; ++i) a.m[i] = w->m[i];
  a.interp = w->interp, a.border = w->border, a.clamp = w->clamp != 0;
  const long planes = (long)B * C;
  const dim3 grid(cdiv((long)H * W, WARP_THREADS), (unsigned)std::min<long>(planes, 64));
  if (w->interp == 0) launch_warp<0>(w->border, grid, s, src, dst, planes, H, W, a);
  else launch_warp<1>(w->border, grid, s, src, dst, planes, H, W, a);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_channel_stats(cgd_ctx* ctx, const float* x, float* stats, int B, int C, int H, int W, hipStream_t s) {
  if (!x || !stats) WARP_FAIL(ctx, "channel stats: x and stats are required");
  if (misaligned(x) || misaligned(stats)) WARP_FAIL(ctx, "channel stats: pointers must be 4-byte aligned");
  if (const char* e = shape_error(B, C, H, W)) WARP_FAIL(ctx, std::string("channel stats: ") + e);
  if (!ctx) return -3;
  const long planes = (long)B * C;
  CGD_LAUNCH(channel_stats_kernel, dim3((unsigned)std::min<long>(planes, 65535)), dim3(STATS_THREADS), 0, s, x, stats, planes, (long)H * W);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_color_match(cgd_ctx* ctx, float* x, const float* stats_x, const float* stats_ref, int ref_batch, float amount, int clamp, int B,
                           int C, int H, int W, hipStream_t s) {
  if (!x || !stats_x || !stats_ref) WARP_FAIL(ctx, "color match: x, stats_x and stats_ref are required");
  if (misaligned(x) || misaligned(stats_x) || misaligned(stats_ref)) WARP_FAIL(ctx, "color match: pointers must be 4-byte aligned");
  if (const char* e = shape_error(B, C, H, W)) WARP_FAIL(ctx, std::string("color match: ") + e);
  if (ref_batch != 1 && ref_batch != B) WARP_FAIL(ctx, "color match: ref_batch must be 1 or B");
  if (!(amount >= 0.f && amount <= 1.f)) WARP_FAIL(ctx, "color match: amount must lie in [0, 1]");
  if (!ctx) return -3;
  const long planes = (long)B * C;
  const dim3 grid(cdiv((long)H * W, WARP_THREADS), (unsigned)std::min<long>(planes, 64));
  CGD_LAUNCH(color_match_kernel, grid, dim3(WARP_THREADS), 0, s, x, stats_x, stats_ref, planes, C, (long)H * W, ref_batch, amount, clamp != 0);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
