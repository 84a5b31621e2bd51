// Video mode of the animation driver (Disco Diffusion's video input and Warp notebooks, Deforum's hybrid video): frame k starts from the
// stylised frame k - 1, moved the way the clip moved.  The motion is estimated here: dense pyramidal Lucas-Kanade flow in the PATCH form
// (each pixel moves its whole window by its own flow), and a warp that follows a flow and knows where not to trust it
// (include/cgd_mi355x.h: cgd_flow_estimate, cgd_op_flow_level, cgd_frame_warp_flow).  NCHW fp32; pixel centres sit on integers.
//   flow:       (B, 2, H, W), channel 0 the x displacement in pixels, channel 1 the y displacement; cgd_flow_estimate(tmpl, img) returns F
//               with img(p + F(p)) ~ tmpl(p).
//   luminance:  C == 3: Y = (0.2989 R + 0.587 G) + 0.114 B, three rounded fp32 products and two rounded sums (the cutout kernels'
//               constants); C == 1: the plane itself.  Both frames of the whole batch become 2B planes, the templates first.
//   pyramid:    level 0 is Y; level l + 1 is the antialiased cubic resize (the launcher behind cgd_op_resize_cubic, taps outside the frame
//               read at the nearest edge pixel) of level l to (ceil(H_l / 2), ceil(W_l / 2)), all 2B planes in one launch.  The level count
//               is the largest L <= levels whose coarsest level has a shorter side of at least 2 radius + 1, and at least 1.
//   a level:    one launch runs all `iters` iterations: a pixel reads only its own flow, so the update is in place and needs no second
//               buffer.  The coarsest level starts from zero; a finer level (Hf, Wf) reads the coarser flow (Hc, Wc) bilinearly at
//               ((x + 0.5) Wc / Wf - 0.5, (y + 0.5) Hc / Hf - 0.5): fp64 coordinates, position clamped into the frame (replicate border),
//               fp64 taps and weights; the result times Wf / Wc (x) or Hf / Hc (y) in fp64, then rounded to fp32.
//   iteration:  at pixel p with flow u, over the window q = p + (dx, dy), |dx|, |dy| <= radius, q inside the frame, ascending dy, then
//               ascending dx: b the template level, bx = (b(qx + 1, qy) - b(qx - 1, qy)) / 2 and by likewise (replicate border);
//               s = q + u in fp64, the sample counts when 0 <= sx <= W - 1 and 0 <= sy <= H - 1 and contributes to NOTHING otherwise;
//               a(s) bilinear, split in fp64 with fp32 weights as cgd_frame_warp splits; e = b(q) - a(s).  fp32 sums in that order:
//               Sxx = sum bx^2, Syy = sum by^2, Gxy = sum bx by, rx = sum bx e, ry = sum by e;  Gxx = lambda + Sxx, Gyy = lambda + Syy,
//               det = Gxx Gyy - Gxy^2, du = (Gyy rx - Gxy ry) / det, dv = (Gxx ry - Gxy rx) / det.  A non-finite step is zero, a step
//               longer than max_step is scaled to that length, then u += (du, dv).
//   staging:    the template tile with its halo of radius + 1 is staged in LDS once per workgroup (indices clamped into the frame: the
//               replicate border of the differences); bx and by are derived from the staged tile; img is read through the cache.
//   warp:       dst(p) = w S(p + F(p)) + (1 - w) fallback(p), w = blend m(p).  S samples src exactly as cgd_frame_warp does (warp_index and
//               cubic_weights of warp_sample.h, the same split, taps, summation order and clamp; position p + (double)F(p), clamped to
//               +-2^30).  m = 1 without flow_back.  With flow_back (the flow of the opposite direction) Fb is read bilinearly at
//               s = p + F(p) (fp64 taps, as the depth lookup of warp3d.hip) and m = 0 when s lies outside [0, W - 1] x [0, H - 1], when Fb(s)
//               is not finite, or unless |F + Fb|^2 <= alpha (|F|^2 + |Fb|^2) + beta in fp64 (the forward-backward check of Sundaram et
//               al.).  A non-finite F reads as zero flow with m = 0.  w == 1 stores the sample's bits, w == 0 the fallback's.
// Fixed summation order, no atomics: the same bits on every run.  Plane offsets are 64-bit; every tap index is clamped or goes through
// a border rule, a sample position that is not inside the frame (NaN included) is never turned into an index.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "kernels.h"
#include "warp_sample.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace {

constexpr int FLOW_TILE = 16;                                   // pixels per workgroup side: 256 threads
constexpr int FLOW_MAX_RADIUS = 7;
constexpr int FLOW_SIDE = FLOW_TILE + 2 * (FLOW_MAX_RADIUS + 1);  // staged tile side at the largest radius

struct FlowLevelArgs {
  int H, W, Hc, Wc, iters, radius;
  float lambda, max_step;
};

// D at (sx, sy): bilinear, position clamped into the frame (replicate border), fp64 taps and weights; a tap of weight 0 is not read into
// the sum.  The depth lookup of warp3d.hip, restated.
__device__ __forceinline__ double bilinear64(const float* __restrict__ D, int H, int W, double sx, double sy) {
#pragma clang fp contract(off)
  const double px = fmin(fmax(sx, 0.0), (double)(W - 1)), py = fmin(fmax(sy, 0.0), (double)(H - 1));
  const double fx = floor(px), fy = floor(py);
  const double tx = px - fx, ty = py - fy;
  const int x0 = (int)fx, y0 = (int)fy;
  const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
  const float* r0 = D + (long)y0 * W;
  const float* r1 = D + (long)y1 * W;
  const double d00 = (double)r0[x0], d10 = (double)r1[x0];
  const double a0 = tx == 0.0 ? d00 : (1.0 - tx) * d00 + tx * (double)r0[x1];
  if (ty == 0.0) return a0;
  const double a1 = tx == 0.0 ? d10 : (1.0 - tx) * d10 + tx * (double)r1[x1];
  return (1.0 - ty) * a0 + ty * a1;
}

// planes [0, B): luminance of tmpl, [B, 2B): of img; grid.x walks the pixels, grid.y the planes (stride loop)
__global__ __launch_bounds__(WARP_THREADS) void flow_luma_kernel(const float* __restrict__ tmpl, const float* __restrict__ img,
                                                                 float* __restrict__ out, int B, int C, long HW) {
  const long q = (long)blockIdx.x * WARP_THREADS + threadIdx.x;
  if (q >= HW) return;
  for (int p = blockIdx.y; p < 2 * B; p += gridDim.y) {
    const float* s = (p < B ? tmpl + (long)p * C * HW : img + (long)(p - B) * C * HW) + q;
    float y = s[0];
    if (C == 3) {
#pragma clang fp contract(off)
      const float r = 0.2989f * s[0], g = 0.587f * s[HW], b = 0.114f * s[2 * HW];
      y = (r + g) + b;
    }
    out[(long)p * HW + q] = y;
  }
}

// one pyramid level, all iterations: bt, im (B, H, W) template and image planes, coarse (B, 2, Hc, Wc) or null, flow (B, 2, H, W) written only
__global__ __launch_bounds__(FLOW_TILE* FLOW_TILE) void flow_level_kernel(const float* __restrict__ bt, const float* __restrict__ im,
                                                                          const float* __restrict__ coarse, float* __restrict__ flow,
                                                                          FlowLevelArgs k) {
  __shared__ float tile[FLOW_SIDE * FLOW_SIDE];
  const int R = k.radius, halo = R + 1, side = FLOW_TILE + 2 * halo;  // side <= FLOW_SIDE: the launcher keeps radius <= FLOW_MAX_RADIUS
  const int H = k.H, W = k.W;
  const long HW = (long)H * W, bi = blockIdx.z;
  const float* b = bt + bi * HW;
  const float* a = im + bi * HW;
  const int tx0 = blockIdx.x * FLOW_TILE, ty0 = blockIdx.y * FLOW_TILE;
  for (int i = threadIdx.x; i < side * side; i += FLOW_TILE * FLOW_TILE) {
    const int ly = i / side, lx = i - ly * side;
    const int gy = min(max(ty0 + ly - halo, 0), H - 1), gx = min(max(tx0 + lx - halo, 0), W - 1);
    tile[i] = b[(long)gy * W + gx];
  }
  __syncthreads();
  const int tx = threadIdx.x & (FLOW_TILE - 1), ty = threadIdx.x / FLOW_TILE;
  const int x = tx0 + tx, y = ty0 + ty;
  if (x >= W || y >= H) return;
  float u = 0.f, v = 0.f;
  if (coarse) {
#pragma clang fp contract(off)
    const int Hc = k.Hc, Wc = k.Wc;
    const long HWc = (long)Hc * Wc;
    const double cx = ((double)x + 0.5) * (double)Wc / (double)W - 0.5, cy = ((double)y + 0.5) * (double)Hc / (double)H - 0.5;
    const float* cu = coarse + bi * 2 * HWc;
    u = (float)(bilinear64(cu, Hc, Wc, cx, cy) * ((double)W / (double)Wc));
    v = (float)(bilinear64(cu + HWc, Hc, Wc, cx, cy) * ((double)H / (double)Hc));
  }
  const int dy0 = max(-R, -y), dy1 = min(R, H - 1 - y), dx0 = max(-R, -x), dx1 = min(R, W - 1 - x);  // the window inside the frame
  const double xmax = (double)(W - 1), ymax = (double)(H - 1);
  for (int it = 0; it < k.iters; ++it) {
    float sxx = 0.f, syy = 0.f, sxy = 0.f, rx = 0.f, ry = 0.f;
    for (int dy = dy0; dy <= dy1; ++dy) {
      const double sy = (double)(y + dy) + (double)v;
      if (!(sy >= 0.0 && sy <= ymax)) continue;  // a NaN flow fails too
      const double fy0 = floor(sy);
      const float fy = (float)(sy - fy0), wy0 = 1.f - fy;
      const int iy = (int)fy0, iy1 = iy + 1 < H ? iy + 1 : H - 1;
      const float* r0 = a + (long)iy * W;
      const float* r1 = a + (long)iy1 * W;
      const int lrow = (ty + halo + dy) * side + tx + halo;
      for (int dx = dx0; dx <= dx1; ++dx) {
        const double sx = (double)(x + dx) + (double)u;
        if (!(sx >= 0.0 && sx <= xmax)) continue;
        const double fx0 = floor(sx);
        const float fx = (float)(sx - fx0), wx0 = 1.f - fx;
        const int ix = (int)fx0, ix1 = ix + 1 < W ? ix + 1 : W - 1;
        const int li = lrow + dx;
        const float bq = tile[li];
        const float gx = (tile[li + 1] - tile[li - 1]) * 0.5f, gy = (tile[li + side] - tile[li - side]) * 0.5f;
        float a0 = wx0 * r0[ix];
        a0 += fx * r0[ix1];
        float a1 = wx0 * r1[ix];
        a1 += fx * r1[ix1];
        float av = wy0 * a0;
        av += fy * a1;
        const float e = bq - av;
        sxx += gx * gx;
        syy += gy * gy;
        sxy += gx * gy;
        rx += gx * e;
        ry += gy * e;
      }
    }
    const float gxx = k.lambda + sxx, gyy = k.lambda + syy;
    const float det = gxx * gyy - sxy * sxy;
    float du = (gyy * rx - sxy * ry) / det, dv = (gxx * ry - sxy * rx) / det;
    if (!(isfinite(du) && isfinite(dv))) {
      du = dv = 0.f;
    } else {
      const float len = sqrtf(du * du + dv * dv);
      if (len > k.max_step) {
        const float s = k.max_step / len;
        du *= s;
        dv *= s;
      }
    }
    u += du;
    v += dv;
  }
  float* fo = flow + bi * 2 * HW + (long)y * W + x;
  fo[0] = u;
  fo[HW] = v;
}

struct WarpFlowArgs {
  float blend, alpha, beta;
  int clamp, flow_per_sample, have_fallback;
};

// grid.x walks the plane's pixels, grid.y the coordinate sets (stride loop), grid.z the planes of a set (stride loop)
template <int INTERP, int BORDER, bool BACK>
__global__ __launch_bounds__(WARP_THREADS) void frame_warp_flow_kernel(const float* __restrict__ src, const float* __restrict__ flow,
                                                                       const float* __restrict__ flow_back,
                                                                       const float* __restrict__ fallback, float* __restrict__ dst,
                                                                       float* __restrict__ mask_out, long sets, long planes_per_set,
                                                                       long masks_per_set, int H, int W, WarpFlowArgs c) {
  const long HW = (long)H * W;
  const long q = (long)blockIdx.x * WARP_THREADS + threadIdx.x;
  if (q >= HW) return;
  const int y = (int)(q / W), x = (int)(q - (long)y * W);
  for (long g = blockIdx.y; g < sets; g += gridDim.y) {
    const float* F = flow + (c.flow_per_sample ? g * 2 * HW : 0);
    float Fx = F[q], Fy = F[HW + q];
    float m = 1.f;
    if (!(isfinite(Fx) && isfinite(Fy))) Fx = Fy = 0.f, m = 0.f;
    double sx = (double)x + (double)Fx, sy = (double)y + (double)Fy;
    if (BACK) {
#pragma clang fp contract(off)
      if (!(sx >= 0.0 && sx <= (double)(W - 1) && sy >= 0.0 && sy <= (double)(H - 1))) {
        m = 0.f;
      } else {
        const float* Fb = flow_back + (c.flow_per_sample ? g * 2 * HW : 0);
        const double bx = bilinear64(Fb, H, W, sx, sy), by = bilinear64(Fb + HW, H, W, sx, sy);
        const double ex = (double)Fx + bx, ey = (double)Fy + by;
        const double lhs = ex * ex + ey * ey;
        const double rhs = (double)c.alpha * (((double)Fx * (double)Fx + (double)Fy * (double)Fy) + (bx * bx + by * by)) + (double)c.beta;
        if (!(isfinite(bx) && isfinite(by)) || !(lhs <= rhs)) m = 0.f;
      }
    }
    sx = fmin(fmax(sx, -WARP_MAX_COORD), WARP_MAX_COORD);
    sy = fmin(fmax(sy, -WARP_MAX_COORD), WARP_MAX_COORD);
    if (mask_out && blockIdx.z == 0)
      for (long j = 0; j < masks_per_set; ++j) mask_out[(g * masks_per_set + j) * HW + q] = m;
    const float w = c.have_fallback ? c.blend * m : 1.f;  // without a fallback (blend 1, no flow_back) the sample is stored whatever m
    const float w1 = 1.f - w;
    const long first = g * planes_per_set + blockIdx.z, end = (g + 1) * planes_per_set, step = gridDim.z;
    // the reader of frame_warp_kernel (warp.hip), statement for statement, up to the store
    const double fx0 = floor(sx), fy0 = floor(sy);
    const float tx = (float)(sx - fx0), ty = (float)(sy - fy0);
    const int ix = (int)fx0, iy = (int)fy0;
#define WARP_FLOW_STORE(p, v)                                       \
  do {                                                              \
    float o__ = (v);                                                \
    if (c.clamp) o__ = fminf(fmaxf(o__, -1.f), 1.f);                \
    if (w != 1.f) {                                                 \
      const float fb__ = fallback[(p) * HW + q];                    \
      o__ = w == 0.f ? fb__ : w * o__ + w1 * fb__;                  \
    }                                                               \
    dst[(p) * HW + q] = o__;                                        \
  } while (0)
    if (INTERP == 0) {
      const int x0 = warp_index<BORDER>(ix, W), x1 = warp_index<BORDER>(ix + 1, W);
      const int r0 = warp_index<BORDER>(iy, H) * W, r1 = warp_index<BORDER>(iy + 1, H) * W;
      const float wx0 = 1.f - tx, wy0 = 1.f - ty;
      for (long p = first; p < end; p += step) {
        const float* s = src + p * HW;
        float a0 = wx0 * s[r0 + x0];
        a0 += tx * s[r0 + x1];
        float a1 = wx0 * s[r1 + x0];
        a1 += tx * s[r1 + x1];
        float v = wy0 * a0;
        v += ty * a1;
        WARP_FLOW_STORE(p, v);
      }
    } else {
      const int x0 = warp_index<BORDER>(ix - 1, W), x1 = warp_index<BORDER>(ix, W), x2 = warp_index<BORDER>(ix + 1, W),
                x3 = warp_index<BORDER>(ix + 2, W);
      const int r0 = warp_index<BORDER>(iy - 1, H) * W, r1 = warp_index<BORDER>(iy, H) * W, r2 = warp_index<BORDER>(iy + 1, H) * W,
                r3 = warp_index<BORDER>(iy + 2, H) * W;
      float wx0, wx1, wx2, wx3, wy0, wy1, wy2, wy3;
      cubic_weights(tx, wx0, wx1, wx2, wx3);
      cubic_weights(ty, wy0, wy1, wy2, wy3);
      for (long p = first; p < end; p += step) {
        const float* s = src + p * HW;
#define WARP_ROW(r) (((wx0 * s[(r) + x0] + wx1 * s[(r) + x1]) + wx2 * s[(r) + x2]) + wx3 * s[(r) + x3])
        const float a0 = WARP_ROW(r0), a1 = WARP_ROW(r1), a2 = WARP_ROW(r2), a3 = WARP_ROW(r3);
#undef WARP_ROW
        const float v = ((wy0 * a0 + wy1 * a1) + wy2 * a2) + wy3 * a3;
        WARP_FLOW_STORE(p, v);
      }
    }
#undef WARP_FLOW_STORE
  }
}

// refusals go to the context's error string when there is a context: the arguments are judged before the context is needed
#define FLOW_FAIL(ctx, what, msg)                            \
  do {                                                       \
    if (ctx) (ctx)->err = std::string(what ": ") + (msg);    \
    return -2;                                               \
  } while (0)

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

bool overlap(const float* a, long na, const float* b, long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

const char* params_error(const cgd_flow_params* p) {
  if (!p) return "the parameters are required";
  if (p->radius < 1 || p->radius > FLOW_MAX_RADIUS) return "radius must lie in 1..7";
  if (p->iters < 1 || p->iters > 16) return "iters must lie in 1..16";
  if (p->levels < 1 || p->levels > 8) return "levels must lie in 1..8";
  if (!std::isfinite(p->lambda) || !(p->lambda > 0.f)) return "lambda must be finite and positive";
  if (!std::isfinite(p->max_step) || !(p->max_step > 0.f)) return "max_step must be finite and positive";
  return nullptr;
}

const char* frame_error(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return "sizes must be positive";
  if ((long)H * W >= (1L << 31)) return "a plane must hold fewer than 2^31 pixels";
  if (B > 32767 || cdiv(H, FLOW_TILE) > 65535) return "at most 32767 samples and 1048560 rows";
  return nullptr;
}

int levels_of(int H, int W, int levels, int radius) {
  int L = 1;
  for (int l = 1; l < levels; ++l) {
    H = (H + 1) / 2, W = (W + 1) / 2;
    if (std::min(H, W) < 2 * radius + 1) break;
    L = l + 1;
  }
  return L;
}

void launch_level(hipStream_t s, const float* b, const float* a, const float* coarse, int Hc, int Wc, float* flow, int B, int H, int W,
                  const cgd_flow_params& p) {
  const FlowLevelArgs k = {H, W, Hc, Wc, p.iters, p.radius, p.lambda, p.max_step};
  const dim3 grid(cdiv(W, FLOW_TILE), cdiv(H, FLOW_TILE), B);
  CGD_LAUNCH(flow_level_kernel, grid, dim3(FLOW_TILE * FLOW_TILE), 0, s, b, a, coarse, flow, k);
}

template <int INTERP, bool BACK>
void launch_warp_flow(int border, dim3 grid, hipStream_t s, const float* src, const float* flow, const float* back, const float* fallback,
                      float* dst, float* mask, long sets, long pps, long mps, int H, int W, const WarpFlowArgs& a) {
  if (border == 0)
    CGD_LAUNCH((frame_warp_flow_kernel<INTERP, 0, BACK>), grid, dim3(WARP_THREADS), 0, s, src, flow, back, fallback, dst, mask, sets, pps, mps, H, W, a);
  else if (border == 1)
    CGD_LAUNCH((frame_warp_flow_kernel<INTERP, 1, BACK>), grid, dim3(WARP_THREADS), 0, s, src, flow, back, fallback, dst, mask, sets, pps, mps, H, W, a);
  else
    CGD_LAUNCH((frame_warp_flow_kernel<INTERP, 2, BACK>), grid, dim3(WARP_THREADS), 0, s, src, flow, back, fallback, dst, mask, sets, pps, mps, H, W, a);
}

}  // namespace

extern "C" {

int cgd_flow_levels(int H, int W, int levels, int radius) {
  if (H <= 0 || W <= 0 || levels < 1 || levels > 8 || radius < 1 || radius > FLOW_MAX_RADIUS) return 0;
  return levels_of(H, W, levels, radius);
}

// pyramid: per level 2B planes; then the flows of the levels above the finest, (B, 2, H_l, W_l) each
long cgd_flow_scratch_floats(int B, int H, int W, int levels, int radius) {
  if (frame_error(B, H, W) || levels < 1 || levels > 8 || radius < 1 || radius > FLOW_MAX_RADIUS) return 0;
  const int L = levels_of(H, W, levels, radius);
  long n = 0;
  for (int l = 0; l < L; ++l) {
    n += 2L * B * H * W * (l == 0 ? 1 : 2);
    H = (H + 1) / 2, W = (W + 1) / 2;
  }
  return n;
}

int cgd_op_flow_level(cgd_ctx* ctx, const float* b, const float* a, const float* coarse, int Hc, int Wc, float* flow, int B, int H, int W,
                      const cgd_flow_params* p, void* stream) {
  if (!b || !a || !flow) FLOW_FAIL(ctx, "flow level", "b, a and flow are required");
  if (misaligned(b) || misaligned(a) || misaligned(coarse) || misaligned(flow)) FLOW_FAIL(ctx, "flow level", "pointers must be 4-byte aligned");
  if (const char* e = frame_error(B, H, W)) FLOW_FAIL(ctx, "flow level", e);
  if (const char* e = params_error(p)) FLOW_FAIL(ctx, "flow level", e);
  if (coarse && (Hc <= 0 || Wc <= 0 || (long)Hc * Wc >= (1L << 31))) FLOW_FAIL(ctx, "flow level", "the coarser level's sizes must be positive, a plane below 2^31 pixels");
  const long HW = (long)H * W;
  if (overlap(flow, 2 * B * HW, b, B * HW) || overlap(flow, 2 * B * HW, a, B * HW) ||
      (coarse && overlap(flow, 2 * B * HW, coarse, 2L * B * Hc * Wc)))
    FLOW_FAIL(ctx, "flow level", "flow must not alias an input");
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  launch_level((hipStream_t)stream, b, a, coarse, coarse ? Hc : 1, coarse ? Wc : 1, flow, B, H, W, *p);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_flow_estimate(cgd_ctx* ctx, const float* tmpl, const float* img, float* flow, float* scratch, int B, int C, int H, int W,
                      const cgd_flow_params* p, void* stream) {
  if (!tmpl || !img || !flow || !scratch) FLOW_FAIL(ctx, "flow estimate", "tmpl, img, flow and scratch are required");
  if (misaligned(tmpl) || misaligned(img) || misaligned(flow) || misaligned(scratch)) FLOW_FAIL(ctx, "flow estimate", "pointers must be 4-byte aligned");
  if (const char* e = frame_error(B, H, W)) FLOW_FAIL(ctx, "flow estimate", e);
  if (C != 1 && C != 3) FLOW_FAIL(ctx, "flow estimate", "C must be 1 or 3");
  if (const char* e = params_error(p)) FLOW_FAIL(ctx, "flow estimate", e);
  if ((long)H * W >= (1L << 30) && levels_of(H, W, p->levels, p->radius) > 1)  // the limit of the resize behind the pyramid
    FLOW_FAIL(ctx, "flow estimate", "a plane of 2^30 pixels or more runs with one level only (levels = 1)");
  const long HW = (long)H * W, nin = (long)B * C * HW, nflow = 2L * B * HW, nscr = cgd_flow_scratch_floats(B, H, W, p->levels, p->radius);
  if (overlap(flow, nflow, tmpl, nin) || overlap(flow, nflow, img, nin)) FLOW_FAIL(ctx, "flow estimate", "flow must not alias an input");
  if (overlap(scratch, nscr, tmpl, nin) || overlap(scratch, nscr, img, nin) || overlap(scratch, nscr, flow, nflow))
    FLOW_FAIL(ctx, "flow estimate", "scratch must not overlap tmpl, img or flow");
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  hipStream_t s = (hipStream_t)stream;
  const int L = levels_of(H, W, p->levels, p->radius);
  int hs[8], ws[8];
  float* pyr[8];
  float* fl[8];
  float* at = scratch;
  for (int l = 0; l < L; ++l) {
    hs[l] = l ? (hs[l - 1] + 1) / 2 : H, ws[l] = l ? (ws[l - 1] + 1) / 2 : W;
    pyr[l] = at;
    at += 2L * B * hs[l] * ws[l];
  }
  fl[0] = flow;
  for (int l = 1; l < L; ++l) {
    fl[l] = at;
    at += 2L * B * hs[l] * ws[l];
  }
  const dim3 lgrid(cdiv(HW, WARP_THREADS), (unsigned)std::min(2 * B, 64));
  CGD_LAUNCH(flow_luma_kernel, lgrid, dim3(WARP_THREADS), 0, s, tmpl, img, pyr[0], B, C, HW);
  for (int l = 1; l < L; ++l)
    CGD_TRY(cgd_launch_resize_cubic(ctx, pyr[l - 1], pyr[l], 2 * B, hs[l - 1], ws[l - 1], hs[l], ws[l], 1.f, 0.f, 0.f, 0, s));
  for (int l = L - 1; l >= 0; --l) {
    const bool top = l == L - 1;
    launch_level(s, pyr[l], pyr[l] + (long)B * hs[l] * ws[l], top ? nullptr : fl[l + 1], top ? 1 : hs[l + 1], top ? 1 : ws[l + 1], fl[l], B,
                 hs[l], ws[l], *p);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_frame_warp_flow(cgd_ctx* ctx, const float* src, const float* flow, const float* flow_back, const float* fallback, float* dst,
                        float* mask_out, int flow_batch, int B, int C, int H, int W, const cgd_warp_flow* w, void* stream) {
  if (!src || !flow || !dst || !w) FLOW_FAIL(ctx, "frame warp flow", "src, flow, dst and the settings are required");
  if (misaligned(src) || misaligned(flow) || misaligned(flow_back) || misaligned(fallback) || misaligned(dst) || misaligned(mask_out))
    FLOW_FAIL(ctx, "frame warp flow", "pointers must be 4-byte aligned");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) FLOW_FAIL(ctx, "frame warp flow", "sizes must be positive");
  if ((long)H * W >= (1L << 31)) FLOW_FAIL(ctx, "frame warp flow", "a plane must hold fewer than 2^31 pixels");
  if ((long)B * C >= (1L << 31)) FLOW_FAIL(ctx, "frame warp flow", "B * C must stay below 2^31");
  if (flow_batch != 1 && flow_batch != B) FLOW_FAIL(ctx, "frame warp flow", "flow_batch must be 1 or B");
  if (w->interp != 0 && w->interp != 1) FLOW_FAIL(ctx, "frame warp flow", "interp must be 0 (bilinear) or 1 (bicubic)");
  if (w->border < 0 || w->border > 2) FLOW_FAIL(ctx, "frame warp flow", "border must be 0 (wrap), 1 (reflect) or 2 (replicate)");
  if (!(w->blend >= 0.f && w->blend <= 1.f)) FLOW_FAIL(ctx, "frame warp flow", "blend must lie in [0, 1]");
  if (!std::isfinite(w->alpha) || !std::isfinite(w->beta) || w->alpha < 0.f || w->beta < 0.f)
    FLOW_FAIL(ctx, "frame warp flow", "alpha and beta must be finite and not negative");
  if (!fallback && (w->blend != 1.f || flow_back)) FLOW_FAIL(ctx, "frame warp flow", "a fallback is required unless blend is 1 and there is no flow_back");
  const long HW = (long)H * W, planes = (long)B * C, n = planes * HW, nf = 2L * flow_batch * HW, nm = (long)B * HW;
  if (overlap(dst, n, src, n) || overlap(dst, n, flow, nf) || overlap(dst, n, flow_back, nf) || overlap(dst, n, fallback, n))
    FLOW_FAIL(ctx, "frame warp flow", "dst must not alias an input");
  if (overlap(mask_out, nm, src, n) || overlap(mask_out, nm, flow, nf) || overlap(mask_out, nm, flow_back, nf) ||
      overlap(mask_out, nm, fallback, n) || overlap(mask_out, nm, dst, n))
    FLOW_FAIL(ctx, "frame warp flow", "mask_out must not alias dst or an input");
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  WarpFlowArgs a;
  a.blend = w->blend, a.alpha = w->alpha, a.beta = w->beta;
  a.clamp = w->clamp != 0, a.flow_per_sample = flow_batch == B && B > 1, a.have_fallback = fallback != nullptr;
  const long sets = a.flow_per_sample ? B : 1, pps = planes / sets, mps = B / sets;
  const long bx = cdiv(HW, WARP_THREADS), gy = std::min<long>(sets, 64);
  const long gz = std::max<long>(1, std::min<long>(std::min<long>(pps, 64), 512 / (bx * gy)));
  const dim3 grid((unsigned)bx, (unsigned)gy, (unsigned)gz);
  hipStream_t s = (hipStream_t)stream;
  if (flow_back) {
    if (w->interp == 0) launch_warp_flow<0, true>(w->border, grid, s, src, flow, flow_back, fallback, dst, mask_out, sets, pps, mps, H, W, a);
    else launch_warp_flow<1, true>(w->border, grid, s, src, flow, flow_back, fallback, dst, mask_out, sets, pps, mps, H, W, a);
  } else {
    if (w->interp == 0) launch_warp_flow<0, false>(w->border, grid, s, src, flow, flow_back, fallback, dst, mask_out, sets, pps, mps, H, W, a);
    else launch_warp_flow<1, false>(w->border, grid, s, src, flow, flow_back, fallback, dst, mask_out, sets, pps, mps, H, W, a);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

}  // extern "C"
