// 3D animation (Disco Diffusion's 3D mode, Deforum): frame k starts from frame k - 1 seen by a pinhole camera that has moved, with a depth
// for every pixel, so that near things move faster than far ones.  One gather kernel on NCHW fp32 (include/cgd_mi355x.h: cgd_frame_warp3d).
//   camera:   x right, y down, z into the screen; pixel centres on integers, principal point (cx, cy), focal length f pixels.  A source
//             position q with depth z > 0 is the point X = z ((qx - cx) / f, (qy - cy) / f, 1); between two frames X' = R X + T; the image of X'
//             is (cx, cy) + f (X'x, X'y) / X'z.
//   backward: destination pixel p reads the source at G(p, z), the exact inverse of that map for a source point of depth z:
//               r = ((px - cx) / f, (py - cy) / f, 1),  a = R^T r with a_z <- max(a_z, 1e-6),  b = R^T T (the launcher's),
//               lambda = max((z + b_z) / a_z, near),  Xs = lambda a - b,  G = (cx + f Xs_x / z, cy + f Xs_y / z)
//   depth:    flat (z = max(z0, near): a homography) or a map D (depth_batch, 1, H, W).  The depth belongs to the unknown source pixel:
//             s_0 = p, s_{k+1} = G(p, max(D(s_k), near)), `iters` steps.  D(s) is bilinear with a replicate border, taps and weights fp64; a tap
//             of weight 0 is not read into the sum, so an integer position gives the stored value; fmax makes a NaN depth read as near.
//   sampling: the final position is clamped to +-2^30 (NaN to -2^30) and handed to warp_sample_planes, the 2D kernel's reader restated on
//             the shared warp_index / cubic_weights (warp_sample.h): the same taps, borders, fp32 weights and summation order.
// All of the coordinate arithmetic is fp64 with contraction off.  The position is computed once per pixel and coordinate set (one set for
// the whole batch unless every sample has a depth map of its own), then the planes are looped.  Gather form, no atomics, no scratch buffer:
// the same bits on every run.  Plane offsets are 64-bit; every tap index goes through a border rule and every depth tap through a clamp.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "kernels.h"
#include "warp_sample.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace {

struct Warp3dArgs {
  double R[9], b[3];  // R row-major (a = R^T r reads its columns), b = R^T T
  double f, cx, cy, z0, near;
  int iters, clamp, depth_per_sample;
};

// D at (sx, sy): bilinear, replicate border (the clamp of the position; NaN reads 0), fp64 taps and weights
__device__ __forceinline__ double depth_at(const float* __restrict__ D, int H, int W, double sx, double sy) {
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

// dst[p][q] = interp(src[p], sx, sy) for the planes p = first, first + step, ... < end; |sx|, |sy| <= 2^30.  The reader of frame_warp_kernel
// (warp.hip), statement for statement: the position is floored and split in fp64, the fractions become fp32, weights and sums are fp32, the
// x taps of a row in ascending order, then the rows in ascending y.  (That kernel keeps its own text: its machine code is the one measured.)
template <int INTERP, int BORDER>
__device__ __forceinline__ void warp_sample_planes(const float* src, float* dst, long first, long end, long step, int H,
                                                   int W, long HW, long q, double sx, double sy, int clamp) {
  const double fx0 = floor(sx), fy0 = floor(sy);
  const float tx = (float)(sx - fx0), ty = (float)(sy - fy0);
  const int ix = (int)fx0, iy = (int)fy0;
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
      if (clamp) v = fminf(fmaxf(v, -1.f), 1.f);
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
    for (long p = first; p < end; p += step) {
      const float* s = src + p * HW;
#define WARP_ROW(r) (((wx0 * s[(r) + x0] + wx1 * s[(r) + x1]) + wx2 * s[(r) + x2]) + wx3 * s[(r) + x3])
      const float a0 = WARP_ROW(r0), a1 = WARP_ROW(r1), a2 = WARP_ROW(r2), a3 = WARP_ROW(r3);
#undef WARP_ROW
      float v = ((wy0 * a0 + wy1 * a1) + wy2 * a2) + wy3 * a3;
      if (clamp) v = fminf(fmaxf(v, -1.f), 1.f);
      dst[p * HW + q] = v;
    }
  }
}

// grid.x walks the plane's pixels, grid.y the coordinate sets (stride loop), grid.z the planes of a set (stride loop)
template <int INTERP, int BORDER, bool MAP>
__global__ __launch_bounds__(WARP_THREADS) void frame_warp3d_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                    const float* __restrict__ depth, long sets, long planes_per_set, int H,
                                                                    int W, Warp3dArgs c) {
  const long HW = (long)H * W;
  const long q = (long)blockIdx.x * WARP_THREADS + threadIdx.x;
  if (q >= HW) return;
  const int y = (int)(q / W), x = (int)(q - (long)y * W);
  double ax, ay, az;
  {
#pragma clang fp contract(off)
    const double rx = ((double)x - c.cx) / c.f, ry = ((double)y - c.cy) / c.f;
    ax = (c.R[0] * rx + c.R[3] * ry) + c.R[6];
    ay = (c.R[1] * rx + c.R[4] * ry) + c.R[7];
    az = fmax((c.R[2] * rx + c.R[5] * ry) + c.R[8], 1e-6);
  }
  for (long g = blockIdx.y; g < sets; g += gridDim.y) {
    double sx = (double)x, sy = (double)y;
    {
#pragma clang fp contract(off)
      const float* D = MAP ? depth + (c.depth_per_sample ? g * HW : 0) : nullptr;
      const int iters = MAP ? c.iters : 1;
      for (int k = 0; k < iters; ++k) {
        const double z = fmax(MAP ? depth_at(D, H, W, sx, sy) : c.z0, c.near);
        const double lambda = fmax((z + c.b[2]) / az, c.near);
        const double Xx = lambda * ax - c.b[0], Xy = lambda * ay - c.b[1];
        sx = c.cx + c.f * Xx / z;
        sy = c.cy + c.f * Xy / z;
      }
      sx = fmin(fmax(sx, -WARP_MAX_COORD), WARP_MAX_COORD);
      sy = fmin(fmax(sy, -WARP_MAX_COORD), WARP_MAX_COORD);
    }
    const long first = g * planes_per_set;
    warp_sample_planes<INTERP, BORDER>(src, dst, first + blockIdx.z, first + planes_per_set, gridDim.z, H, W, HW, q, sx, sy, c.clamp);
  }
}

#define WARP3D_FAIL(ctx, msg)                                 \
  do {                                                        \
    if (ctx) (ctx)->err = std::string("frame warp 3d: ") + (msg); \
    return -2;                                                \
  } while (0)

bool overlap(const float* a, long na, const float* b, long nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb * 4 && b0 < a0 + (uintptr_t)na * 4;
}

template <int INTERP, bool MAP>
void launch3d(int border, dim3 grid, hipStream_t s, const float* src, float* dst, const float* depth, long sets, long pps, int H, int W,
              const Warp3dArgs& a) {
  if (border == 0) CGD_LAUNCH((frame_warp3d_kernel<INTERP, 0, MAP>), grid, dim3(WARP_THREADS), 0, s, src, dst, depth, sets, pps, H, W, a);
  else if (border == 1) CGD_LAUNCH((frame_warp3d_kernel<INTERP, 1, MAP>), grid, dim3(WARP_THREADS), 0, s, src, dst, depth, sets, pps, H, W, a);
  else CGD_LAUNCH((frame_warp3d_kernel<INTERP, 2, MAP>), grid, dim3(WARP_THREADS), 0, s, src, dst, depth, sets, pps, H, W, a);
}

}  // namespace

int cgd_launch_frame_warp3d(cgd_ctx* ctx, const float* src, float* dst, const float* depth, int depth_batch, int B, int C, int H, int W,
                            const cgd_camera* cam, hipStream_t s) {
  if (!src || !dst || !cam) WARP3D_FAIL(ctx, "src, dst and the camera are required");
  if (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)depth) & 3) WARP3D_FAIL(ctx, "pointers must be 4-byte aligned");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) WARP3D_FAIL(ctx, "sizes must be positive");
  if ((long)H * W >= (1L << 31)) WARP3D_FAIL(ctx, "a plane must hold fewer than 2^31 pixels");
  if ((long)B * C >= (1L << 31)) WARP3D_FAIL(ctx, "B * C must stay below 2^31");
  if (depth && depth_batch != 1 && depth_batch != B) WARP3D_FAIL(ctx, "depth_batch must be 1 or B");
  const long HW = (long)H * W, planes = (long)B * C;
  if (overlap(dst, planes * HW, src, planes * HW)) WARP3D_FAIL(ctx, "dst must not alias src");
  if (depth && overlap(dst, planes * HW, depth, depth_batch * HW)) WARP3D_FAIL(ctx, "dst must not alias depth");
  if (cam->interp != 0 && cam->interp != 1) WARP3D_FAIL(ctx, "interp must be 0 (bilinear) or 1 (bicubic)");
  if (cam->border < 0 || cam->border > 2) WARP3D_FAIL(ctx, "border must be 0 (wrap), 1 (reflect) or 2 (replicate)");
  if (cam->iters < 1 || cam->iters > 4) WARP3D_FAIL(ctx, "iters must lie in 1..4");
  bool finite = std::isfinite(cam->f) && std::isfinite(cam->cx) && std::isfinite(cam->cy) && std::isfinite(cam->z0) && std::isfinite(cam->near);
  for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(cam->R[i]);
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(cam->T[i]);
  if (!finite) WARP3D_FAIL(ctx, "the camera has a non-finite entry");
  if (!(cam->f > 0) || !(cam->z0 > 0) || !(cam->near > 0)) WARP3D_FAIL(ctx, "f, z0 and near must be positive");
  const double* R = cam->R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0);
      if (!(std::fabs(d) <= 1e-9)) WARP3D_FAIL(ctx, "R is no rotation: max |R R^T - I| exceeds 1e-9");
    }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (!(det > 0)) WARP3D_FAIL(ctx, "R is no rotation: its determinant is negative");
  bool identity = cam->T[0] == 0 && cam->T[1] == 0 && cam->T[2] == 0;
  for (int i = 0; i < 9; ++i) identity = identity && R[i] == (i % 4 == 0 ? 1.0 : 0.0);
  if (identity) {  // G(p, z) = p whatever the depth, but the arithmetic above does not give it to the bit: the affine kernel's identity does
    cgd_warp w = {{1, 0, 0, 0, 1, 0}, cam->interp, cam->border, cam->clamp};
    return cgd_launch_frame_warp(ctx, src, dst, B, C, H, W, &w, s);
  }
  if (!ctx) return -3;
  Warp3dArgs a;
  for (int i = 0; i < 9; ++i) a.R[i] = R[i];
  for (int i = 0; i < 3; ++i) a.b[i] = R[i] * cam->T[0] + R[3 + i] * cam->T[1] + R[6 + i] * cam->T[2];
  a.f = cam->f, a.cx = cam->cx, a.cy = cam->cy, a.z0 = cam->z0, a.near = cam->near;
  a.iters = cam->iters, a.clamp = cam->clamp != 0, a.depth_per_sample = depth && depth_batch == B && B > 1;
  const long sets = a.depth_per_sample ? B : 1, pps = planes / sets;
  // the position costs far more than the affine kernel's, so the planes of a set are looped; they are spread over grid.z only while the
  // frame alone leaves compute units idle (about two workgroups for each of the 256)
  const long bx = cdiv(HW, WARP_THREADS), gy = std::min<long>(sets, 64);
  const long gz = std::max<long>(1, std::min<long>(std::min<long>(pps, 64), 512 / (bx * gy)));
  const dim3 grid((unsigned)bx, (unsigned)gy, (unsigned)gz);
  if (depth) {
    if (cam->interp == 0) launch3d<0, true>(cam->border, grid, s, src, dst, depth, sets, pps, H, W, a);
    else launch3d<1, true>(cam->border, grid, s, src, dst, depth, sets, pps, H, W, a);
  } else {
    if (cam->interp == 0) launch3d<0, false>(cam->border, grid, s, src, dst, depth, sets, pps, H, W, a);
    else launch3d<1, false>(cam->border, grid, s, src, dst, depth, sets, pps, H, W, a);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
