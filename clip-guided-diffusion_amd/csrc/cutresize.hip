// Antialiased-resize cutouts: crop -> (3-channel luma) -> separable cubic resize to cs x cs -> (flip along W) -> CLIP normalisation,
// forward and adjoint.  The resampler is ResizeRight's cubic resize with antialiasing and pad_mode='constant', stated per axis for a crop
// extent n resized to m (s = m / n) with exact rational geometry:
//   centre of output o in input coordinates   c_o = ((2o+1) n - m) / (2m)
//   kernel k(d) = cubic(d), support S = 4 (s >= 1);  k(d) = s cubic(s d), S = 4n / m (s < 1);  T = ceil(S) taps from left_o = ceil(c_o - S/2)
//   w_oj = k(c_o - j) / sum over ALL T taps of k (a zero sum divides by 1); taps outside [0, n) read zero and the weights are not
//   renormalised over the taps inside, so rows at the crop border sum to less than 1.
// left_o, T and the tap distances are integer arithmetic (resize_row); only the cubic polynomial is float32.  The zero padding is in
// [0,1] space: out = (Wy ((x_in crop + 1) / 2) Wx^T - mean) / std, per channel, Wy from (h, cs) and Wx from (w, cs).
//
// Both kernels build the weight rows they need in LDS from (extent, cs); no weight table crosses the host boundary.
//   forward: one workgroup per ((cut, b), band of RB output rows): vertical pass of the band into LDS (3 x RB x w), then the horizontal
//            pass, luma, flip, normalisation and the store in either output layout.
//   adjoint: 1. per ((cut, b), band of RB crop rows): normalisation / flip / luma adjoint of d_out on load, Wy^T (gather over the output
//               rows whose taps include the crop row) into LDS (3 x RB x cs), then Wx (gather over the output columns whose taps include
//               the crop column) -> the cutout's own gradient plane in scratch                                 (cutresize_bwd_plane_kernel)
//            2. every image pixel sums, over the cutouts in order, the planes of the boxes that contain it; (+)= into g_in
//                                                                                                              (cutresize_bwd_gather_kernel)
//   Gather form throughout, no atomics, fixed summation order: the same bits on every run.
#include "../../include/cgd_mi355x.h"
#include "common.h"
#include "kernels.h"
#include "resize_rows.h"

#include <algorithm>

namespace {

__constant__ float kRsMean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
__constant__ float kRsStd[3] = {0.26862954f, 0.26130258f, 0.27577711f};

constexpr int RS_MAX_LDS = 64 * 1024;  // bytes of dynamic LDS a launch may ask for
constexpr int RS_GATHER_SUB = 8;       // lanes per image pixel in cutresize_bwd_gather_kernel

__device__ inline bool box_ok(int oy, int ox, int h, int w, int H, int W) {
  return h > 0 && w > 0 && oy >= 0 && ox >= 0 && oy <= H - h && ox <= W - w;
}

// output index of resized pixel (i, j), channel c, of row nb = cut * B + b (the two layouts of cgd_cutouts_fwd)
__device__ inline long rs_out_index(long nb, int c, int i, int j, int cs, int layout, int P) {
  if (!layout) return ((nb * 3 + c) * cs + i) * cs + j;
  const int g = cs / P, ip = i / P, jp = j / P;
  return (nb * g * g + (long)ip * g + jp) * (3L * P * P) + (long)c * P * P + (i - ip * P) * P + (j - jp * P);
}

// LDS of the forward: wx [cs][TP] | wy [RB][TP] | tmp [3][RB][W] | leftx [cs] | lefty [RB]        (TP = odd row stride >= the most taps)
// grid.x = band of RB output rows, grid.y = (cut, b)
__global__ __launch_bounds__(256) void cutresize_fwd_kernel(const float* __restrict__ x, const int* __restrict__ coords,
                                                            const int* __restrict__ flags, float* __restrict__ out, int B, int H, int W,
                                                            int cs, int layout, int P, int RB, int TP) {
  extern __shared__ __align__(16) float lds[];
  float* wx = lds;
  float* wy = wx + cs * TP;
  float* tmp = wy + RB * TP;
  int* leftx = (int*)(tmp + 3 * RB * W);
  int* lefty = leftx + cs;
  const int nb = blockIdx.y, b = nb % B, cut = nb / B, tid = threadIdx.x;
  const int i0 = blockIdx.x * RB, rows = min(RB, cs - i0);
  const int oy = coords[cut * 4 + 0], ox = coords[cut * 4 + 1], h = coords[cut * 4 + 2], w = coords[cut * 4 + 3];
  if (!box_ok(oy, ox, h, w, H, W)) {  // a box outside the image reads nothing: its row is NaN
    for (int e = tid; e < rows * cs; e += 256)
      for (int c = 0; c < 3; ++c) out[rs_out_index(nb, c, i0 + e / cs, e % cs, cs, layout, P)] = NAN;
    return;
  }
  const int fl = flags[cut];
  const int Tx = resize_taps(w, cs), Ty = resize_taps(h, cs);  // <= TP (the host sizes TP for the largest extent the image allows)
  for (int j = tid; j < cs; j += 256) leftx[j] = resize_row(w, cs, j, Tx, wx + j * TP);
  for (int r = tid; r < rows; r += 256) lefty[r] = resize_row(h, cs, i0 + r, Ty, wy + r * TP);
  __syncthreads();
  // vertical pass: tmp[c][r][xx] = sum_t wy[r][t] * (crop[c][lefty[r] + t][xx] + 1) / 2, taps outside the crop read zero
  const long HW = (long)H * W;
  const float* xb = x + (long)b * 3 * HW + (long)oy * W + ox;
  for (int e = tid; e < rows * w; e += 256) {
    const int r = e / w, xx = e - r * w;
    const int y0 = lefty[r];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int t = 0; t < Ty; ++t) {
      const int yy = y0 + t;
      if ((unsigned)yy >= (unsigned)h) continue;
      const float wt = wy[r * TP + t];
      const float* p = xb + (long)yy * W + xx;
      a0 += wt * ((p[0] + 1.f) * 0.5f);
      a1 += wt * ((p[HW] + 1.f) * 0.5f);
      a2 += wt * ((p[2 * HW] + 1.f) * 0.5f);
    }
    tmp[(0 * RB + r) * W + xx] = a0;
    tmp[(1 * RB + r) * W + xx] = a1;
    tmp[(2 * RB + r) * W + xx] = a2;
  }
  __syncthreads();
  // horizontal pass, luma (it commutes with the per-channel resize), flip, normalisation
  for (int e = tid; e < rows * cs; e += 256) {
    const int r = e / cs, j = e - r * cs;
    const int x0 = leftx[j];
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int t = 0; t < Tx; ++t) {
      const int xx = x0 + t;
      if ((unsigned)xx >= (unsigned)w) continue;
      const float wt = wx[j * TP + t];
      a0 += wt * tmp[(0 * RB + r) * W + xx];
      a1 += wt * tmp[(1 * RB + r) * W + xx];
      a2 += wt * tmp[(2 * RB + r) * W + xx];
    }
    if (fl & 1) a0 = a1 = a2 = 0.2989f * a0 + 0.587f * a1 + 0.114f * a2;
    const int jo = (fl & 2) ? cs - 1 - j : j;
    out[rs_out_index(nb, 0, i0 + r, jo, cs, layout, P)] = (a0 - kRsMean[0]) / kRsStd[0];
    out[rs_out_index(nb, 1, i0 + r, jo, cs, layout, P)] = (a1 - kRsMean[1]) / kRsStd[1];
    out[rs_out_index(nb, 2, i0 + r, jo, cs, layout, P)] = (a2 - kRsMean[2]) / kRsStd[2];
  }
}

// LDS of the adjoint's stage 1: wx [cs][TP] | wy [cs][TP] | tmp [3][RB][cs] | leftx [cs] | lefty [cs]
// grid.x = band of RB crop rows (bands beyond the crop's h return), grid.y = (cut, b) of this launch; planes [(cut, b)][3][H * W], a
// crop pixel (y, xx) at y * w + xx
__global__ __launch_bounds__(256) void cutresize_bwd_plane_kernel(const float* __restrict__ dout, const int* __restrict__ coords,
                                                                  const int* __restrict__ flags, float* __restrict__ planes, int B,
                                                                  int H, int W, int cs, int layout, int P, int RB, int TP) {
  extern __shared__ __align__(16) float lds[];
  float* wx = lds;
  float* wy = wx + cs * TP;
  float* tmp = wy + cs * TP;
  int* leftx = (int*)(tmp + 3 * RB * cs);
  int* lefty = leftx + cs;
  const int nb = blockIdx.y, cut = nb / B, tid = threadIdx.x;
  const int oy = coords[cut * 4 + 0], ox = coords[cut * 4 + 1], h = coords[cut * 4 + 2], w = coords[cut * 4 + 3];
  const int y0 = blockIdx.x * RB;
  if (!box_ok(oy, ox, h, w, H, W) || y0 >= h) return;  // (uniform per workgroup)
  const int rows = min(RB, h - y0);
  const int fl = flags[cut];
  const int Tx = resize_taps(w, cs), Ty = resize_taps(h, cs);
  for (int j = tid; j < cs; j += 256) {
    leftx[j] = resize_row(w, cs, j, Tx, wx + j * TP);
    lefty[j] = resize_row(h, cs, j, Ty, wy + j * TP);
  }
  __syncthreads();
  // tmp[c][r][j] = sum over output rows i whose taps include crop row y0 + r of wy[i][y - left_i] * D[c][i][j], D = the adjoint of the
  // normalisation, the flip and the luma applied to d_out
  for (int e = tid; e < rows * cs; e += 256) {
    const int r = e / cs, j = e - r * cs, y = y0 + r;
    const int jo = (fl & 2) ? cs - 1 - j : j;
    int lo, hi;
    resize_inverse_range(h, cs, Ty, y, lo, hi);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int i = lo; i <= hi; ++i) {
      const int t = y - lefty[i];
      if ((unsigned)t >= (unsigned)Ty) continue;
      const float wt = wy[i * TP + t];
      a0 += wt * dout[rs_out_index(nb, 0, i, jo, cs, layout, P)];
      a1 += wt * dout[rs_out_index(nb, 1, i, jo, cs, layout, P)];
      a2 += wt * dout[rs_out_index(nb, 2, i, jo, cs, layout, P)];
    }
    a0 /= kRsStd[0];
    a1 /= kRsStd[1];
    a2 /= kRsStd[2];
    if (fl & 1) {
      const float s = a0 + a1 + a2;
      a0 = 0.2989f * s;
      a1 = 0.587f * s;
      a2 = 0.114f * s;
    }
    tmp[(0 * RB + r) * cs + j] = a0;
    tmp[(1 * RB + r) * cs + j] = a1;
    tmp[(2 * RB + r) * cs + j] = a2;
  }
  __syncthreads();
  const long HW = (long)H * W;
  float* pl = planes + (long)nb * 3 * HW;
  for (int e = tid; e < rows * w; e += 256) {
    const int r = e / w, xx = e - r * w;
    int lo, hi;
    resize_inverse_range(w, cs, Tx, xx, lo, hi);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int j = lo; j <= hi; ++j) {
      const int t = xx - leftx[j];
      if ((unsigned)t >= (unsigned)Tx) continue;
      const float wt = wx[j * TP + t];
      a0 += wt * tmp[(0 * RB + r) * cs + j];
      a1 += wt * tmp[(1 * RB + r) * cs + j];
      a2 += wt * tmp[(2 * RB + r) * cs + j];
    }
    const long q = (long)(y0 + r) * w + xx;
    pl[q] = a0;
    pl[HW + q] = a1;
    pl[2 * HW + q] = a2;
  }
}

// G[b,c,y,x] (+)= 0.5 * sum over the cutouts whose box contains (y, x), in order, of their plane's pixel.  RS_GATHER_SUB lanes share a
// pixel, lane `sub` walking cutouts sub, sub + RS_GATHER_SUB, ... in order, then a fixed butterfly: a fixed summation order.  grid.y = b
__global__ __launch_bounds__(256) void cutresize_bwd_gather_kernel(const int* __restrict__ coords, const float* __restrict__ planes,
                                                                   float* __restrict__ G, int B, int H, int W, int cutn, int accumulate) {
  const int b = blockIdx.y;
  const int sub = threadIdx.x & (RS_GATHER_SUB - 1);
  const long pix = ((long)blockIdx.x * 256 + threadIdx.x) / RS_GATHER_SUB;
  const long HW = (long)H * W;
  const bool live = pix < HW;  // dead lanes still take part in the butterfly
  const int pp = live ? (int)pix : 0;
  const int y = pp / W, x = pp - y * W;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int cut = sub; cut < cutn; cut += RS_GATHER_SUB) {
    const int oy = coords[cut * 4 + 0], ox = coords[cut * 4 + 1], h = coords[cut * 4 + 2], w = coords[cut * 4 + 3];
    if (!box_ok(oy, ox, h, w, H, W)) continue;
    const int ry = y - oy, rx = x - ox;
    if ((unsigned)ry >= (unsigned)h || (unsigned)rx >= (unsigned)w) continue;
    const float* src = planes + ((long)cut * B + b) * 3 * HW + (long)ry * w + rx;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) acc[ch] += src[ch * HW];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
    for (int o = 1; o < RS_GATHER_SUB; o <<= 1) acc[ch] += __shfl_xor(acc[ch], o, 64);
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

// most taps any box of an H x W image can need, as the odd LDS row stride
int taps_stride(int H, int W, int cs) { return resize_taps(std::max(H, W), cs) | 1; }

// rows per band so that the launch's LDS fits: `fixed` floats + 3 * RB * `width` floats
int band_rows(long fixed, int width) {
  for (int rb = 8; rb >= 1; rb >>= 1)
    if ((fixed + 3L * rb * width + 2L * rb) * 4 <= RS_MAX_LDS) return rb;
  return 0;
}

// the kernels index with 32-bit ints below these bounds (offsets that can exceed them are formed in 64 bits)
int check_shape(cgd_ctx* ctx, int B, int H, int W, int cutn, int cs, int layout, int P) {
  if (layout && (P <= 0 || cs % P)) CGD_FAIL(ctx, "cutouts_resize: cut size must be a multiple of the patch size");
  if (B <= 0 || H <= 0 || W <= 0 || cutn < 0 || cs <= 0 || B > 65535) CGD_FAIL(ctx, "cutouts_resize: size out of range");
  const long lim = (1L << 31) - 1;
  if ((long)B * 3 * H * W > lim || (long)cs * cs * 3 * B * std::max(cutn, 1) > lim || 8L * cs * std::max(std::max(H, W), cs) > lim ||
      (long)H * W * RS_GATHER_SUB > lim)
    CGD_FAIL(ctx, "cutouts_resize: offsets do not fit 31 bits");
  return 0;
}

}  // namespace

// largest number of (cut, b) rows per launch: grid.y <= 65535
static int rs_rows_per_launch(int B, int cutn) { return (int)std::min<long>(std::max(cutn, 1), 65535 / B); }

size_t cgd_cutouts_resize_scratch(int B, int H, int W, int cutn) {
  return (B <= 0 || H <= 0 || W <= 0 || cutn <= 0 || B > 65535) ? 0 : (size_t)rs_rows_per_launch(B, cutn) * B * 3 * H * W;
}

int cgd_launch_cutouts_resize_fwd(cgd_ctx* ctx, const float* x_in, const int* coords, const int* flags, float* out, int B, int H, int W,
                                  int cutn, int cs, int layout, int P, hipStream_t s) {
  CGD_TRY(check_shape(ctx, B, H, W, cutn, cs, layout, P));
  if (cutn > 0 && (!x_in || !coords || !flags || !out)) CGD_FAIL(ctx, "cutouts_resize: null buffer");
  const int TP = taps_stride(H, W, cs);
  const int RB = band_rows((long)cs * TP + cs + 8L * TP, W);
  if (RB == 0) CGD_FAIL(ctx, "cutouts_resize: the weight rows of this image and cut size do not fit the LDS");
  const size_t lds = ((size_t)cs * TP + (size_t)RB * TP + 3 * (size_t)RB * W + cs + RB) * 4;
  const int per = rs_rows_per_launch(B, cutn);
  for (int k0 = 0; k0 < cutn; k0 += per) {
    const int nk = std::min(per, cutn - k0);
    CGD_LAUNCH(cutresize_fwd_kernel, dim3(cdiv(cs, RB), nk * B), dim3(256), lds, s, x_in, coords + 4 * k0, flags + k0,
               out + (long)k0 * B * 3 * cs * cs, B, H, W, cs, layout, P, RB, TP);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_cutouts_resize_bwd(cgd_ctx* ctx, const float* dout, const int* coords, const int* flags, float* G, float* scratch, int B,
                                  int H, int W, int cutn, int cs, int layout, int P, int accumulate, hipStream_t s) {
  CGD_TRY(check_shape(ctx, B, H, W, cutn, cs, layout, P));
  if (!G) CGD_FAIL(ctx, "cutouts_resize: null gradient buffer");
  const long HW = (long)H * W;
  if (cutn == 0) {  // no cutout: the adjoint is zero
    if (!accumulate) CGD_HIP(ctx, hipMemsetAsync(G, 0, sizeof(float) * B * 3 * HW, s));
    return 0;
  }
  if (!dout || !coords || !flags) CGD_FAIL(ctx, "cutouts_resize: null buffer");
  if (!scratch) CGD_FAIL(ctx, "cutouts_resize: the adjoint needs its scratch (cgd_cutouts_resize_scratch_floats)");
  const int TP = taps_stride(H, W, cs);
  const int RB = band_rows(2L * cs * TP + 2L * cs, cs);
  if (RB == 0) CGD_FAIL(ctx, "cutouts_resize: the weight rows of this image and cut size do not fit the LDS");
  const size_t lds = (2 * (size_t)cs * TP + 3 * (size_t)RB * cs + 2 * (size_t)cs) * 4;
  const int per = rs_rows_per_launch(B, cutn);
  // runs of cutouts reuse the scratch in stream order; each run's gather adds into G after the first
  for (int k0 = 0; k0 < cutn; k0 += per) {
    const int nk = std::min(per, cutn - k0);
    CGD_LAUNCH(cutresize_bwd_plane_kernel, dim3(cdiv(H, RB), nk * B), dim3(256), lds, s, dout + (long)k0 * B * 3 * cs * cs,
               coords + 4 * k0, flags + k0, scratch, B, H, W, cs, layout, P, RB, TP);
    CGD_LAUNCH(cutresize_bwd_gather_kernel, dim3(cdiv(HW * RS_GATHER_SUB, 256), B), dim3(256), 0, s, coords + 4 * k0, scratch, G, B, H, W,
               nk, (accumulate || k0 > 0) ? 1 : 0);
  }
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_resize_weights(int n, int m, float* w, int32_t* left, int* taps) {
  if (!taps) return -3;
  if (n <= 0 || m <= 0 || (long)n * m > (1L << 40) || 4L * n / m > (1 << 20)) return -2;
  const int T = resize_taps(n, m);
  *taps = T;
  if (!w && !left) return 0;  // the tap count alone, to size the buffers
  if (!w || !left) return -3;
  for (int o = 0; o < m; ++o) left[o] = resize_row(n, m, o, T, w + (long)o * T);
  return 0;
}
