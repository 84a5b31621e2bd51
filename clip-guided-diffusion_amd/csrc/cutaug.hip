// Augmented cutouts (`use_augs=True`, the reference's modules.py:13-24 between the crop and the pool), forward and adjoint.
//
// Per (cutout k, sample b), with crop (oy, ox, h, w) and the per-cutout parameter record of include/cgd_mi355x.h, in [0,1] space:
//   z1  = flip_k((x_in[b, :, oy:oy+h, ox:ox+w] + 1) / 2) + n1          flip along W
//   z2  = affine_nearest_k(z1) + n2                                     rotation about the centre + integer translation, fill 0
//   z3  = (perspective_bilinear_k(z2) if persp_k else z2) + n3          fill 0, weights not renormalised
//   z4  = (gray3_k(z3) if gray_k else z3) + n4                          ITU-R 601-2 luma broadcast to 3 channels
//   out = (adaptive_avg_pool(z4, cs) - mean_c) / std_c                  layout 0 (N,3,cs,cs) or layout 1 (ViT patch rows)
// The source coordinates of both resamplings come from aug_affine_src / aug_persp_taps, shared by the kernels and the host-only
// cgd_op_aug_sample_map: they restate guidance.py's aug_affine / aug_perspective -> _sample_grid -> grid_sample(align_corners=False)
// op by op in float32 (no contraction, true division, nearest = round half to even), so the nearest picks are the CPU oracle's.
//
// The adjoint is a gather in three launches, no atomics, fixed summation order (bit-reproducible like cutouts_bwd_kernel):
//   1. pool + normalise + grayscale adjoint -> dz3 plane per (k, b)                      (cutaug_bwd_pool_kernel)
//   2. perspective adjoint: every z2 pixel q gathers from the output pixels whose bilinear taps include q, found in the bounding box
//      of the inverse homography's image of [q-1, q+1]^2 and confirmed by recomputing their forward taps    (cutaug_bwd_persp_kernel)
//   3. nearest-affine adjoint + flip + crop: every image pixel gathers, over the cutouts in order, from the z2 pixels of a 3x3 box
//      around its inverse-rotated position whose forward pick is exactly it; (+)= into g_in               (cutaug_bwd_gather_kernel)
// The noise terms are additive and do not enter the adjoint.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace {

__constant__ float kAugMean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
__constant__ float kAugStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};

// parameter record fields (include/cgd_mi355x.h)
enum { P_FLIP = 0, P_COS = 1, P_SIN = 2, P_TX = 3, P_TY = 4, P_PERSP = 5, P_CO = 6, P_GRAY = 14 };

// grid_sample(align_corners=False) unnormalisation of the grid value g = coord / (size / 2) that _sample_grid forms
__host__ __device__ inline float aug_unnormalize(float coord, int size) {
#pragma clang fp contract(off)
  const float half = (float)size * 0.5f;
  const float g = coord / half;
  return ((g + 1.f) * (float)size - 1.f) / 2.f;
}

// aug_affine: output pixel (i, j) of an h x w crop -> row-major index of the nearest source pixel, or -1 (fill 0)
__host__ __device__ inline int aug_affine_src(const float* p, int i, int j, int h, int w) {
#pragma clang fp contract(off)
  const float c = p[P_COS], s = p[P_SIN];
  const float xo = ((float)j + 0.5f - (float)w * 0.5f) - p[P_TX];
  const float yo = ((float)i + 0.5f - (float)h * 0.5f) - p[P_TY];
  const float xi = c * xo + s * yo;
  const float yi = (-s) * xo + c * yo;
  const float ix = aug_unnormalize(xi, w), iy = aug_unnormalize(yi, h);
  if (!(ix > -2.f && ix < (float)w + 1.f && iy > -2.f && iy < (float)h + 1.f)) return -1;  // also rejects NaN
  const int x = (int)nearbyintf(ix), y = (int)nearbyintf(iy);
  return (x >= 0 && x < w && y >= 0 && y < h) ? y * w + x : -1;
}

struct PerspTaps {
  int idx[4];  // nw, ne, sw, se source indices (row-major in the crop), -1 outside (fill 0)
  float wt[4]; // bilinear weights, 0 for the taps outside
};

// aug_perspective: output pixel (i, j) -> the four bilinear taps of grid_sample on the h x w plane
__host__ __device__ inline PerspTaps aug_persp_taps(const float* p, int i, int j, int h, int w) {
#pragma clang fp contract(off)
  const float* co = p + P_CO;
  const float xs = (float)j + 0.5f, ys = (float)i + 0.5f;
  const float den = co[6] * xs + co[7] * ys + 1.f;
  const float xi = (co[0] * xs + co[1] * ys + co[2]) / den - (float)w * 0.5f;
  const float yi = (co[3] * xs + co[4] * ys + co[5]) / den - (float)h * 0.5f;
  const float ix = aug_unnormalize(xi, w), iy = aug_unnormalize(yi, h);
  PerspTaps t;
  if (!(ix > -2.f && ix < (float)w + 1.f && iy > -2.f && iy < (float)h + 1.f)) {  // all four taps outside (or NaN)
    for (int k = 0; k < 4; ++k) {
      t.idx[k] = -1;
      t.wt[k] = 0.f;
    }
    return t;
  }
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wy1 = iy - fy, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
  const float wts[4] = {wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + (k & 1), y = y0 + (k >> 1);
    const bool in = x >= 0 && x < w && y >= 0 && y < h;
    t.idx[k] = in ? y * w + x : -1;
    t.wt[k] = in ? wts[k] : 0.f;
  }
  return t;
}

__device__ inline bool crop_ok(int oy, int ox, int h, int w, int H, int W) {
  return h > 0 && w > 0 && oy >= 0 && ox >= 0 && oy + h <= H && ox + w <= W;
}

// output index of pooled pixel (i, j), channel c, of row nb = cut * B + b (both layouts of cutouts_fwd_kernel)
__device__ inline long out_index(long nb, int c, int i, int j, int cs, int layout, int P) {
  if (!layout) return ((nb * 3 + c) * cs + i) * cs + j;
  const int g = cs / P, ip = i / P, jp = j / P;
  return (nb * g * g + (long)ip * g + jp) * (3L * P * P) + (long)c * P * P + (i - ip * P) * P + (j - jp * P);
}

// grid.y = (cut, b) row of this launch, grid.x covers the cs * cs pooled pixels; one thread owns all 3 channels (grayscale mixes them)
__global__ __launch_bounds__(256) void cutaug_fwd_kernel(const float* __restrict__ x, const int* __restrict__ coords,
                                                         const float* __restrict__ params, const float* __restrict__ noise,
                                                         const int64_t* __restrict__ noise_off, float* __restrict__ out, int B, int H,
                                                         int W, int cs, int layout, int P) {
  const int nb = blockIdx.y, b = nb % B, cut = nb / B;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= cs * cs) return;
  const int i = pix / cs, j = pix - i * cs;
  const int oy = coords[cut * 4 + 0], ox = coords[cut * 4 + 1], h = coords[cut * 4 + 2], w = coords[cut * 4 + 3];
  if (!crop_ok(oy, ox, h, w, H, W)) {  // a crop outside the image reads nothing: its row is NaN
    for (int c = 0; c < 3; ++c) out[out_index(nb, c, i, j, cs, layout, P)] = NAN;
    return;
  }
  const float* pr = params + cut * 16;
  const bool flip = pr[P_FLIP] != 0.f, persp = pr[P_PERSP] != 0.f, gray = pr[P_GRAY] != 0.f;
  const long hw = (long)h * w, plane = 3L * hw * B;  // one noise plane n_s is (B,3,h,w)
  const float* nz = noise ? noise + noise_off[cut] + (long)b * 3 * hw : nullptr;
  const float* xb = x + (long)b * 3 * H * W + (long)oy * W + ox;
  // z2 at crop pixel q (all 3 channels)
  auto z2 = [&](int q, float* v) {
    const int r = aug_affine_src(pr, q / w, q % w, h, w);
    if (r >= 0) {
      const int ry = r / w, rx = r - ry * w, sx = flip ? w - 1 - rx : rx;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[c] = (xb[(long)c * H * W + (long)ry * W + sx] + 1.f) * 0.5f;
        if (nz) v[c] += nz[c * hw + r];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = 0.f;
    }
    if (nz) {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] += nz[plane + c * hw + q];
    }
  };
  const int ys = i * h / cs, ye = ((i + 1) * h + cs - 1) / cs;
  const int xs = j * w / cs, xe = ((j + 1) * w + cs - 1) / cs;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int yy = ys; yy < ye; ++yy) {
    for (int xx = xs; xx < xe; ++xx) {
      const int q = yy * w + xx;
      float v[3];
      if (persp) {
        const PerspTaps t = aug_persp_taps(pr, yy, xx, h, w);
        v[0] = v[1] = v[2] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (t.idx[k] < 0) continue;
          float u[3];
          z2(t.idx[k], u);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[c] += u[c] * t.wt[k];
        }
      } else {
        z2(q, v);
      }
      if (nz) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += nz[2 * plane + c * hw + q];
      }
      if (gray) v[0] = v[1] = v[2] = 0.2989f * v[0] + 0.587f * v[1] + 0.114f * v[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += nz ? v[c] + nz[3 * plane + c * hw + q] : v[c];
    }
  }
  const float inv = 1.f / (float)((ye - ys) * (xe - xs));
#pragma unroll
  for (int c = 0; c < 3; ++c) out[out_index(nb, c, i, j, cs, layout, P)] = (acc[c] * inv - kAugMean[c]) / kAugStd[c];
}

// stage 1: dz3[(cut,b)][c][y][x] of crop pixel (y, x) = grayscale adjoint of (pool + normalise adjoint of d_out)
// grid.y = (cut, b), grid.x covers H * W (threads beyond the crop's h * w return); dz3 plane stride H * W
__global__ __launch_bounds__(256) void cutaug_bwd_pool_kernel(const float* __restrict__ dout, const int* __restrict__ coords,
                                                              const float* __restrict__ params, float* __restrict__ dz3, int B, int H,
                                                              int W, int cs, int layout, int P) {
  const int nb = blockIdx.y, cut = nb / B;
  const int pix = blockIdx.x * 256 + threadIdx.x;
  const int oy = coords[cut * 4 + 0], ox = coords[cut * 4 + 1], h = coords[cut * 4 + 2], w = coords[cut * 4 + 3];
  if (!crop_ok(oy, ox, h, w, H, W) || pix >= h * w) return;
  const int y = pix / w, x = pix - y * w;
  const int i0 = y * cs / h, i1 = min(cs - 1, ((y + 1) * cs - 1) / h);
  const int j0 = x * cs / w, j1 = min(cs - 1, ((x + 1) * cs - 1) / w);
  float d[3] = {0.f, 0.f, 0.f};
  for (int i = i0; i <= i1; ++i) {
    const int bh = ((i + 1) * h + cs - 1) / cs - i * h / cs;
    for (int j = j0; j <= j1; ++j) {
      const float inv = 1.f / (float)(bh * (((j + 1) * w + cs - 1) / cs - j * w / cs));
#pragma unroll
      for (int c = 0; c < 3; ++c) d[c] += dout[out_index(nb, c, i, j, cs, layout, P)] * inv;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] /= kAugStd[c];
  if (params[cut * 16 + P_GRAY] != 0.f) {
    const float t = d[0] + d[1] + d[2];
    d[0] = 0.2989f * t;
    d[1] = 0.587f * t;
    d[2] = 0.114f * t;
  }
  float* o = dz3 + (long)nb * 3 * H * W + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[(long)c * H * W] = d[c];
}

// stage 2 (cutouts with the perspective only): dz2[q] = sum over output pixels p whose bilinear taps include q of weight * dz3[p]
__global__ __launch_bounds__(256) void cutaug_bwd_persp_kernel(const int* __restrict__ coords, const float* __restrict__ params,
                                                               const float* __restrict__ dz3, float* __restrict__ dz2, int B, int H, int W) {
  const int nb = blockIdx.y, cut = nb / B;
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int oy = coords[cut * 4 + 0], ox = coords[cut * 4 + 1], h = coords[cut * 4 + 2], w = coords[cut * 4 + 3];
  const float* pr = params + cut * 16;
  if (pr[P_PERSP] == 0.f || !crop_ok(oy, ox, h, w, H, W) || q >= h * w) return;
  const int qy = q / w, qx = q - qy * w;
  // q is a tap of p iff the source position of p lies in (q-1, q+1)^2; in the homography's pixel-edge coordinates (source index + 0.5)
  // that is the box [qx - 0.5, qx + 1.5] x [qy - 0.5, qy + 1.5].  Its preimage under the homography is the convex quadrilateral of the
  // corners' images when the line at infinity misses the box (one sign of the homogeneous coordinate at all four corners); the
  // candidates p are the bounding box of that quadrilateral, widened by one pixel, and every candidate is confirmed below
  const float* co = pr + P_CO;
  const float a = co[0], bb = co[1], c = co[2], d = co[3], e = co[4], f = co[5], g = co[6], hh = co[7];
  // adjugate of [[a, b, c], [d, e, f], [g, h, 1]]
  const float m00 = e - f * hh, m01 = c * hh - bb, m02 = bb * f - c * e;
  const float m10 = f * g - d, m11 = a - c * g, m12 = c * d - a * f;
  const float m20 = d * hh - e * g, m21 = bb * g - a * hh, m22 = a * e - bb * d;
  int i_lo = 0, i_hi = h - 1, j_lo = 0, j_hi = w - 1;
  float umin = 1e30f, umax = -1e30f, vmin = 1e30f, vmax = -1e30f;
  int pos = 0, neg = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float X = (float)qx + ((k & 1) ? 1.5f : -0.5f), Y = (float)qy + ((k >> 1) ? 1.5f : -0.5f);
    const float wz = m20 * X + m21 * Y + m22;
    pos += wz > 0.f;
    neg += wz < 0.f;
    const float u = (m00 * X + m01 * Y + m02) / wz, v = (m10 * X + m11 * Y + m12) / wz;
    umin = fminf(umin, u);
    umax = fmaxf(umax, u);
    vmin = fminf(vmin, v);
    vmax = fmaxf(vmax, v);
  }
  // RandomPerspective(0.4) draws keep the vanishing line well away from the crop (tests/test_cutaug_host.py pins one sign of the
  // homogeneous coordinate over the crop widened by 1.5 px for thousands of draws), so the whole-crop scan below is for arbitrary records
  const float lim = 4.f * (float)(h + w);
  if ((pos == 4 || neg == 4) && umin > -lim && umax < lim && vmin > -lim && vmax < lim) {  // (u, v) = (j + 0.5, i + 0.5)
    j_lo = max(0, (int)floorf(umin - 0.5f) - 1);
    j_hi = min(w - 1, (int)ceilf(umax - 0.5f) + 1);
    i_lo = max(0, (int)floorf(vmin - 0.5f) - 1);
    i_hi = min(h - 1, (int)ceilf(vmax - 0.5f) + 1);
  }
  const long HW = (long)H * W;
  const float* src = dz3 + (long)nb * 3 * HW;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int i = i_lo; i <= i_hi; ++i) {
    for (int j = j_lo; j <= j_hi; ++j) {
      const PerspTaps t = aug_persp_taps(pr, i, j, h, w);
      float wt = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) wt += t.idx[k] == q ? t.wt[k] : 0.f;
      if (wt == 0.f) continue;
      const int p = i * w + j;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += wt * src[ch * HW + p];
    }
  }
  float* o = dz2 + (long)nb * 3 * HW + q;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) o[ch * HW] = acc[ch];
}

constexpr int GA_SUB = 8;  // lanes per image pixel in cutaug_bwd_gather_kernel
// stage 3: G[b,c,y,x] (+)= 0.5 * sum over the cutouts covering (y, x) of the z2 adjoint gathered through the nearest affine pick and
// the flip; dz2 = the stage-2 planes for cutouts with the perspective, the stage-1 planes otherwise.  GA_SUB lanes share a pixel, lane
// `sub` walking cutouts sub, sub + GA_SUB, ... in order, then a fixed 3-step butterfly: a fixed summation order (bit-reproducible) and
// GA_SUB times the wavefronts of a thread-per-pixel gather (at 256 x 256 that one had a single wavefront per SIMD).  grid.y = b
__global__ __launch_bounds__(256) void cutaug_bwd_gather_kernel(const int* __restrict__ coords, const float* __restrict__ params,
                                                                const float* __restrict__ dz3, const float* __restrict__ dz2,
                                                                float* __restrict__ G, int B, int H, int W, int cutn, int accumulate) {
  const int b = blockIdx.y;
  const int sub = threadIdx.x & (GA_SUB - 1);
  const int pix = (blockIdx.x * 256 + threadIdx.x) / GA_SUB;
  const bool live = pix < H * W;  // dead lanes still take part in the butterfly
  const int pp = live ? pix : 0;
  const int y = pp / W, x = pp - y * W;
  const long HW = (long)H * W;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int cut = sub; cut < cutn; cut += GA_SUB) {
    const int oy = coords[cut * 4 + 0], ox = coords[cut * 4 + 1], h = coords[cut * 4 + 2], w = coords[cut * 4 + 3];
    if (!crop_ok(oy, ox, h, w, H, W)) continue;
    const int ry = y - oy, rx0 = x - ox;
    if ((unsigned)ry >= (unsigned)h || (unsigned)rx0 >= (unsigned)w) continue;
    const float* pr = params + cut * 16;
    const int rx = pr[P_FLIP] != 0.f ? w - 1 - rx0 : rx0;  // z1 pixel holding this image pixel
    const int r = ry * w + rx;
    // invert the rotation: z2 pixels whose pick is r lie within 0.71 px of (jq, iq) in each coordinate
    const float c = pr[P_COS], s = pr[P_SIN];
    const float vx = (float)rx + 0.5f - (float)w * 0.5f, vy = (float)ry + 0.5f - (float)h * 0.5f;
    const float jq = c * vx - s * vy + pr[P_TX] - 0.5f + (float)w * 0.5f;
    const float iq = s * vx + c * vy + pr[P_TY] - 0.5f + (float)h * 0.5f;
    if (!(jq > -3.f && jq < (float)w + 2.f && iq > -3.f && iq < (float)h + 2.f)) continue;
    const int j0 = (int)floorf(jq + 0.5f), i0 = (int)floorf(iq + 0.5f);
    const float* src = (pr[P_PERSP] != 0.f ? dz2 : dz3) + ((long)cut * B + b) * 3 * HW;
    for (int di = -1; di <= 1; ++di) {
      const int qi = i0 + di;
      if ((unsigned)qi >= (unsigned)h) continue;
      for (int dj = -1; dj <= 1; ++dj) {
        const int qj = j0 + dj;
        if ((unsigned)qj >= (unsigned)w || aug_affine_src(pr, qi, qj, h, w) != r) continue;
        const int q = qi * w + qj;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[ch] += src[ch * HW + q];
      }
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int o = 1; o < GA_SUB; o <<= 1) acc[ch] += __shfl_xor(acc[ch], o, 64);
  }
  if (live && sub == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const long idx = ((long)b * 3 + ch) * HW + pix;
      const float v = acc[ch] * 0.5f;  // d((x + 1) / 2) / dx
      G[idx] = accumulate ? G[idx] + v : v;
    }
  }
}

// the kernels index with 32-bit ints below these bounds (offsets that can exceed them are formed in 64 bits)
int check_shape(cgd_ctx* ctx, int B, int H, int W, int cutn, int cs, int layout, int P) {
  if (layout && (P <= 0 || cs % P)) CGD_FAIL(ctx, "cutouts_aug: cut size must be a multiple of the patch size");
  if (B <= 0 || H <= 0 || W <= 0 || cutn < 0 || cs <= 0 || B > 65535) CGD_FAIL(ctx, "cutouts_aug: size out of range");
  const long lim = (1L << 31) - 1;
  if ((long)B * 3 * H * W > lim || (long)cs * cs * 3 * B * std::max(cutn, 1) > lim || (long)(cs + 1) * std::max(H, W) > lim ||
      (long)cutn * B * 3 * H * W > lim || (long)H * W * GA_SUB > lim)
    CGD_FAIL(ctx, "cutouts_aug: offsets do not fit 31 bits");
  return 0;
}

}  // namespace

// largest number of (cut, b) rows per launch: grid.y <= 65535
static int rows_per_launch(int B, int cutn) { return (int)std::min<long>(std::max(cutn, 1), 65535 / B); }

size_t cgd_cutouts_aug_scratch(int B, int H, int W, int cutn) {
  return (B <= 0 || H <= 0 || W <= 0 || cutn <= 0) ? 0 : 2 * (size_t)rows_per_launch(B, cutn) * B * 3 * H * W;
}

int cgd_launch_cutouts_aug_fwd(cgd_ctx* ctx, const float* x_in, const int* coords, const float* params, const float* noise,
                               const int64_t* noise_off, float* out, int B, int H, int W, int cutn, int cs, int layout, int P,
                               hipStream_t s) {
  CGD_TRY(check_shape(ctx, B, H, W, cutn, cs, layout, P));
  if (noise && !noise_off) CGD_FAIL(ctx, "cutouts_aug: noise needs its per-cutout offsets");
  const int per = rows_per_launch(B, cutn);
  for (int k0 = 0; k0 < cutn; k0 += per) {
    const int nk = std::min(per, cutn - k0);
    CGD_LAUNCH(cutaug_fwd_kernel, dim3(cdiv((long)cs * cs, 256), nk * B), dim3(256), 0, s, x_in, coords + 4 * k0, params + 16 * k0,
               noise, noise ? noise_off + k0 : nullptr, out + (long)k0 * B * 3 * cs * cs, B, H, W, cs, layout, P);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_cutouts_aug_bwd(cgd_ctx* ctx, const float* dout, const int* coords, const float* params, float* G, float* scratch, int B,
                               int H, int W, int cutn, int cs, int layout, int P, int accumulate, hipStream_t s) {
  CGD_TRY(check_shape(ctx, B, H, W, cutn, cs, layout, P));
  if (!scratch) CGD_FAIL(ctx, "cutouts_aug: the adjoint needs its scratch (cgd_cutouts_aug_scratch_floats)");
  const int per = rows_per_launch(B, cutn);
  const long HW = (long)H * W;
  float* dz3 = scratch;
  float* dz2 = scratch + (long)per * B * 3 * HW;
  if (cutn == 0) {  // no cutout: the adjoint is zero
    if (!accumulate) CGD_HIP(ctx, hipMemsetAsync(G, 0, sizeof(float) * B * 3 * HW, s));
    return 0;
  }
  // runs of cutouts reuse the scratch in stream order; each run's gather adds into G after the first
  for (int k0 = 0; k0 < cutn; k0 += per) {
    const int nk = std::min(per, cutn - k0);
    const int* ck = coords + 4 * k0;
    const float* pk = params + 16 * k0;
    CGD_LAUNCH(cutaug_bwd_pool_kernel, dim3(cdiv(HW, 256), nk * B), dim3(256), 0, s, dout + (long)k0 * B * 3 * cs * cs, ck, pk, dz3, B,
               H, W, cs, layout, P);
    CGD_LAUNCH(cutaug_bwd_persp_kernel, dim3(cdiv(HW, 256), nk * B), dim3(256), 0, s, ck, pk, dz3, dz2, B, H, W);
    CGD_LAUNCH(cutaug_bwd_gather_kernel, dim3(cdiv(HW * GA_SUB, 256), B), dim3(256), 0, s, ck, pk, dz3, dz2, G, B, H, W, nk,
               (accumulate || k0 > 0) ? 1 : 0);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_aug_sample_map(const float* params, int h, int w, int32_t* affine_src, int32_t* persp_idx, float* persp_w) {
  if (!params || !affine_src || !persp_idx || !persp_w) return -3;
  if (h <= 0 || w <= 0 || (long)h * w > (1L << 24)) return -2;
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < w; ++j) {
      const int p = i * w + j;
      affine_src[p] = aug_affine_src(params, i, j, h, w);
      const PerspTaps t = aug_persp_taps(params, i, j, h, w);
      for (int k = 0; k < 4; ++k) {
        persp_idx[4 * p + k] = t.idx[k];
        persp_w[4 * p + k] = t.wt[k];
      }
    }
  return 0;
}
