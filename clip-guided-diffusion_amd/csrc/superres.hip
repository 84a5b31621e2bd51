// The conditioned stem of guided-diffusion's super-resolution UNets (SuperResModel.forward):
//   y = conv3x3(cat([x, F.interpolate(low_res, (H, W), mode="bilinear")], dim=1), W, b)          x (B,3,H,W) NCHW -> y NHWC
// in ONE launch and without the (B,6,H,W) tensor: the three conditioning planes of a tile's halo patch are interpolated while the patch
// is staged into LDS (`low` is at most 3 x 128 x 128 floats and stays in L2).
//
// The interpolation is F.interpolate(..., mode="bilinear", align_corners=False), stated per axis with exact integer geometry for an
// extent n_in resized to n_out:
//   src_d = max(((2d+1) n_in - n_out) / (2 n_out), 0),  i0 = floor(src_d),  i1 = i0 + (i0 < n_in - 1),  weights 1 - (src_d - i0), src_d - i0
// i0 and the remainder are integer arithmetic; only the fraction and the two-tap blends are float32.  At n_in == n_out the fraction is 0 and
// the plane passes through exactly.
// Zero padding belongs to the CONCATENATED tensor: outside the H x W frame all six channels read 0; inside it the interpolation clamps at
// the low-res border.
//
// Register plan (thin_in_direct_kernel<6> keeps 54 float4 weights per lane and lost to the im2col route for it): the 54 x Cout weights
// sit in LDS, k-major, and a lane owns 4 output channels x 8 adjacent pixels (32 accumulators).  Every weight float4 read from LDS feeds
// 32 FMAs, every patch row segment (10 floats: two 16-byte and one 8-byte broadcast read) feeds 96.
#include "common.h"
#include "mfma_stage.h"

namespace {

constexpr int SR_TH = 2, SR_TW = 64, SR_PX = 8;   // tile rows x columns, adjacent pixels per lane
constexpr int SR_PW = SR_TW + 4;                  // patch row pitch (floats): columns x0 - 1 .. x0 + 64, 16-byte rows
constexpr int SR_PROWS = SR_TH + 2;
constexpr int SR_KK = 54;                         // 9 taps x 6 channels

// the two taps of output d of an n_in -> n_out axis: i0, i1 and the weight of i1
__device__ inline void sr_taps(int d, int n_in, int n_out, int& i0, int& i1, float& f) {
  int num = (2 * d + 1) * n_in - n_out;
  if (num < 0) num = 0;
  const int den = 2 * n_out;
  i0 = num / den;
  f = (float)(num - i0 * den) / (float)den;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
}

// grid.x walks the (b, tile row, tile column) tiles; the weights are staged once per workgroup
__global__ __launch_bounds__(256) void sr_stem_kernel(const float* __restrict__ x, const float* __restrict__ low, int B_low, int lh, int lw,
                                                      const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y,
                                                      int ldy, int Bn, int H, int W, int Cout, int vec_store) {
  extern __shared__ __attribute__((aligned(16))) float sm[];  // weights [54][Cout + 4], then the patch [6][SR_PROWS][SR_PW]
  const int LP = Cout + 4;
  float* wsm = sm;
  float* patch = sm + SR_KK * LP;
  const int tid = threadIdx.x;
  for (int i = tid; i < SR_KK * Cout; i += 256) {
    const int co = i / SR_KK, k = i - co * SR_KK;
    wsm[k * LP + co] = w[i];
  }
  const int Q = Cout >> 2;  // channel quads
  const int tiles_x = (W + SR_TW - 1) / SR_TW, tiles_y = (H + SR_TH - 1) / SR_TH;
  const long ntiles = (long)Bn * tiles_y * tiles_x;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int b = (int)(t / ((long)tiles_y * tiles_x));
    const int tr = (int)(t - (long)b * tiles_y * tiles_x);
    const int y0 = (tr / tiles_x) * SR_TH, x0 = (tr % tiles_x) * SR_TW;
    __syncthreads();  // the previous tile's readers are done with the patch (first pass: nothing to wait for but the cost is one barrier)
    const float* xb = x + (long)b * 3 * H * W;
    const float* lb = low + (long)(B_low == 1 ? 0 : b) * 3 * lh * lw;
    for (int i = tid; i < SR_PROWS * (SR_TW + 2); i += 256) {
      const int py = i / (SR_TW + 2), px = i - py * (SR_TW + 2);
      const int sy = y0 + py - 1, sx = x0 + px - 1;
      float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W) {
        int iy0, iy1, ix0, ix1;
        float fy, fx;
        sr_taps(sy, lh, H, iy0, iy1, fy);
        sr_taps(sx, lw, W, ix0, ix1, fx);
        const float gy = 1.f - fy, gx = 1.f - fx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c] = xb[((long)c * H + sy) * W + sx];
          const float* lp = lb + (long)c * lh * lw;
          const float r0 = gx * lp[iy0 * lw + ix0] + fx * lp[iy0 * lw + ix1];
          const float r1 = gx * lp[iy1 * lw + ix0] + fx * lp[iy1 * lw + ix1];
          v[3 + c] = gy * r0 + fy * r1;
        }
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) patch[(c * SR_PROWS + py) * SR_PW + px] = v[c];
    }
    __syncthreads();
    // items: (row of the tile, group of 8 adjacent pixels, channel quad); consecutive lanes take consecutive quads
    const int nitems = SR_TH * (SR_TW / SR_PX) * Q;
    for (int item = tid; item < nitems; item += 256) {
      const int q = item % Q, pg = item / Q;
      const int r = pg / (SR_TW / SR_PX), p = (pg % (SR_TW / SR_PX)) * SR_PX;
      const int yy = y0 + r;
      if (yy >= H || x0 + p >= W) continue;
      cgd_f32x4 acc[SR_PX];
      const cgd_f32x4 bv = bias ? cgd_f32x4{bias[4 * q], bias[4 * q + 1], bias[4 * q + 2], bias[4 * q + 3]} : cgd_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < SR_PX; ++j) acc[j] = bv;
#pragma unroll 1
      for (int ci = 0; ci < 6; ++ci)  // (not unrolled: the scheduler hoists every LDS read of an unrolled body and runs out of registers)
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const float* row = patch + (ci * SR_PROWS + r + ky) * SR_PW + p;
          const cgd_f32x4 a0 = *(const cgd_f32x4*)row, a1 = *(const cgd_f32x4*)(row + 4);
          const float a8 = row[8], a9 = row[9];
          const float v[10] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3], a8, a9};
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const cgd_f32x4 wv = *(const cgd_f32x4*)&wsm[((ky * 3 + kx) * 6 + ci) * LP + 4 * q];
#pragma unroll
            for (int j = 0; j < SR_PX; ++j) acc[j] += v[j + kx] * wv;
          }
        }
      float* yrow = y + (((long)b * H + yy) * W + x0 + p) * ldy + 4 * q;
      const int nx = min(SR_PX, W - x0 - p);
#pragma unroll
      for (int j = 0; j < SR_PX; ++j) {
        if (j >= nx) break;
        float* yp = yrow + (long)j * ldy;
        if (vec_store) {
          *(cgd_f32x4*)yp = acc[j];
        } else {
          yp[0] = acc[j][0]; yp[1] = acc[j][1]; yp[2] = acc[j][2]; yp[3] = acc[j][3];
        }
      }
    }
  }
}

}  // namespace

int cgd_launch_sr_stem(cgd_ctx* ctx, const float* x, const float* low, int B_low, int lh, int lw, const float* w, const float* bias, float* y,
                       int ldy, int Bn, int H, int W, int Cout, hipStream_t s) {
  if (ldy <= 0) ldy = Cout;
  if (!x || !low || !w || !y) CGD_FAIL(ctx, "sr_stem: x, low, the weight and y are required");
  if (Bn <= 0 || H <= 0 || W <= 0 || lh <= 0 || lw <= 0) CGD_FAIL(ctx, "sr_stem: empty frame or low-resolution image");
  if (Cout <= 0 || Cout % 4 || Cout > 256) CGD_FAIL(ctx, "sr_stem: Cout must be a multiple of 4, at most 256");
  if (B_low != 1 && B_low != Bn) CGD_FAIL(ctx, "sr_stem: the low-resolution batch must be 1 or the batch of x");
  if (ldy < Cout) CGD_FAIL(ctx, "sr_stem: ldy is smaller than Cout");
  // the integer geometry of sr_taps: (2 d + 1) n_in and 2 n_out in 32 bits
  if ((long)(2L * H + 1) * lh > 0x7fffffffL || (long)(2L * W + 1) * lw > 0x7fffffffL) CGD_FAIL(ctx, "sr_stem: frame x low-resolution extent overflows");
  const size_t sh = ((size_t)SR_KK * (Cout + 4) + (size_t)6 * SR_PROWS * SR_PW) * sizeof(float);  // <= 62688 bytes at Cout 256
  const long ntiles = (long)Bn * cdiv(H, SR_TH) * cdiv(W, SR_TW);
  const int blocks = (int)std::min<long>(ntiles, (long)(ctx->num_cu > 0 ? ctx->num_cu : 256) * 3);  // 3 workgroups per CU fit its LDS at Cout 192
  const int vec = (ldy & 3) == 0 && ((uintptr_t)y & 15) == 0;
  CGD_LAUNCH(sr_stem_kernel, dim3(blocks), dim3(256), sh, s, x, low, B_low, lh, lw, w, bias, y, ldy, Bn, H, W, Cout, vec);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
