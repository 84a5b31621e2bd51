// DPT-Large (MiDaS v3, Ranftl et al., "Vision Transformers for Dense Prediction") on MI355X: forward only.  The depth network of 3D animation
// (cgd_amd.animate --depth_model): frame -> inverse depth -> the depth map cgd_frame_warp3d warps by.
//
//   backbone    timm vit_large_patch16_384 layout: 16 x 16 patch conv with bias (a GEMM over patch rows), class token, pos_embed (resized per grid
//               on the host, cgd_depth_set_pos_embed), `layers` pre-LN blocks (clip_block_fwd: exact GELU, LayerNorm eps 1e-6); no ln_pre, the
//               checkpoint's final norm is not used.  Only the four hooked block outputs are kept; one set of block scratch serves every layer.
//   readout     y = GELU(Linear_{2W -> W}(cat(tok, cls))) over the patch tokens: the class half of the linear is one vector per image (a few-row
//               GEMM), the token half one weight GEMM over all rows; depth_readout_kernel drops the class rows, adds the vector and applies GELU.
//   reassemble  conv1x1 W -> c_k, then ConvTranspose2d k = s = 4 / 2 (a GEMM [pixels][c] x [c][c k k] + depth_shuffle_kernel), nothing, or the
//               stride-2 conv of sconv.hip; then layer{k}_rn, a 3x3 conv to `features` channels without bias.
//   fusion      FeatureFusionBlock_custom from tap 4 down to tap 1: out = path (+ RCU1(layer_k_rn)), RCU2, bilinear x2 (align_corners = True),
//               out_conv.  out_conv is a 1x1 conv and runs on the low-resolution map in front of the upsample (they commute: the bilinear weights
//               sum to 1); the upsample's launch adds the next block's RCU1 branch.  RCU(x) = conv(relu(conv(relu(x)))) + x.
//   head        conv3x3 F -> F/2, bilinear x2, conv3x3 -> 32, then ONE launch: ReLU, the 32 -> 1 dot product, ReLU, and the depth mapping
//               depth = max((offset - inv_depth) / scale, floor).
// Activations are NHWC rows.  Channel counts that are no multiple of 32 inside the head (F / 2 of a tiny test configuration) are zero-padded.
// The net runs in the context's precision mode, like the CLIP towers.  Nothing is kept for a backward pass.
#include <algorithm>
#include <map>

#include "../../include/cgd_mi355x.h"
#include "net.h"
#include "mfma_stage.h"
#include "resize_rows.h"

namespace {

constexpr int kMaxTaps = 32;  // cgd_op_resize_cubic: at most an 8-fold reduction per axis

int grid_of(long n) { return (int)std::min<long>((n + 255) / 256, 16384); }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int pad32(int c) { return (c + 31) & ~31; }

// ---- kernels (memory-bound gathers: one float4 of channels per thread, fixed summation order, no atomics) ----------------------------
// NCHW img (B,3,h,w) -> patch rows [B*gh*gw][3*P*P], columns (c, py, px) as the patch conv's weight [W][3][P][P] has them
__global__ __launch_bounds__(256) void depth_patchify_kernel(const float* __restrict__ img, float* __restrict__ cols, int B, int h, int w, int P) {
  const int gh = h / P, gw = w / P, pq = P / 4;
  const long total = (long)B * gh * gw * 3 * P * pq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % pq);
    long r = i / pq;
    const int py = (int)(r % P); r /= P;
    const int c = (int)(r % 3); r /= 3;
    const int gx = (int)(r % gw); r /= gw;
    const int gy = (int)(r % gh);
    const int b = (int)(r / gh);
    const cgd_f32x4 v = *(const cgd_f32x4*)(img + (((long)b * 3 + c) * h + (long)gy * P + py) * w + (long)gx * P + 4 * q);
    *(cgd_f32x4*)(cols + (((long)b * gh + gy) * gw + gx) * (3L * P * P) + ((long)c * P + py) * P + 4 * q) = v;
  }
}
// out = relu(in) on [rows][4 cq] views (out may be in)
__global__ __launch_bounds__(256) void depth_relu_kernel(const float* in, int ldi, float* out, int ldo, long rows, int cq) {
  const long total = rows * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / cq;
    const int q = (int)(i - r * cq);
    cgd_f32x4 v = *(const cgd_f32x4*)(in + r * ldi + 4 * q);
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    *(cgd_f32x4*)(out + r * ldo + 4 * q) = v;
  }
}
// bilinear x2 with align_corners = True: output o reads the source position o (n - 1) / (2n - 1), in exact integer arithmetic (i0 = the
// quotient, the weight of i0 + 1 = the remainder / (2n - 1)); n = 1 is a copy.  out [B][2Hi][2Wi] rows (+ add, same shape)
__global__ __launch_bounds__(256) void depth_up2x_ac_kernel(const float* __restrict__ in, int ldi, float* __restrict__ out, int ldo,
                                                            const float* __restrict__ add, int ldadd, int B, int Hi, int Wi, int cq) {
  const int Ho = 2 * Hi, Wo = 2 * Wi;
  const long total = (long)B * Ho * Wo * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % cq);
    const long pix = i / cq;
    const int ox = (int)(pix % Wo);
    const long r = pix / Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    const int ny = oy * (Hi - 1), nx = ox * (Wi - 1);
    const int y0 = ny / (Ho - 1), x0 = nx / (Wo - 1);
    const float ly = (float)(ny - y0 * (Ho - 1)) / (float)(Ho - 1), lx = (float)(nx - x0 * (Wo - 1)) / (float)(Wo - 1);
    const int y1 = min(y0 + 1, Hi - 1), x1 = min(x0 + 1, Wi - 1);
    const float* base = in + (long)b * Hi * Wi * ldi + 4 * q;
    const cgd_f32x4 v00 = *(const cgd_f32x4*)(base + ((long)y0 * Wi + x0) * ldi), v01 = *(const cgd_f32x4*)(base + ((long)y0 * Wi + x1) * ldi),
                    v10 = *(const cgd_f32x4*)(base + ((long)y1 * Wi + x0) * ldi), v11 = *(const cgd_f32x4*)(base + ((long)y1 * Wi + x1) * ldi);
    cgd_f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (1.f - ly) * ((1.f - lx) * v00[k] + lx * v01[k]) + ly * ((1.f - lx) * v10[k] + lx * v11[k]);
    if (add) {
      const cgd_f32x4 a = *(const cgd_f32x4*)(add + pix * ldadd + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] += a[k];
    }
    *(cgd_f32x4*)(out + pix * ldo + 4 * q) = o;
  }
}
// the scatter of a ConvTranspose2d with kernel = stride = k (no overlap): g [B*H*W][k*k*Cout] (columns (ky, kx, co)) -> out [B][H k][W k] rows of
// Cout channels, out[b][y k + ky][x k + kx][co] = g[b, y, x][(ky k + kx) Cout + co] + bias[co]
__global__ __launch_bounds__(256) void depth_shuffle_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ bias,
                                                            float* __restrict__ out, int ldo, int B, int H, int W, int Cout, int k) {
  const int cq = Cout / 4, kk = k * k;
  const long total = (long)B * H * W * kk * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % cq);
    long r = i / cq;
    const int t = (int)(r % kk);
    const long pix = r / kk;
    const int x = (int)(pix % W);
    const long yb = pix / W;
    const int y = (int)(yb % H), b = (int)(yb / H);
    const int ky = t / k, kx = t - ky * k;
    cgd_f32x4 v = *(const cgd_f32x4*)(g + pix * ldg + (long)t * Cout + 4 * q);
    if (bias) {
      const cgd_f32x4 bv = *(const cgd_f32x4*)(bias + 4 * q);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] += bv[c];
    }
    const long orow = (((long)b * H + y) * k + ky) * ((long)W * k) + (long)x * k + kx;
    *(cgd_f32x4*)(out + orow * ldo + 4 * q) = v;
  }
}
// ConvTranspose2d weight [Cin][Cout][k][k] -> the GEMM's B operand [(ky k + kx) Cout + co][Cin]
__global__ __launch_bounds__(256) void depth_pack_deconv_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int kk) {
  const long total = (long)Cin * Cout * kk;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ci = (int)(i % Cin);
    const long n = i / Cin;
    const int co = (int)(n % Cout), t = (int)(n / Cout);
    wp[i] = w[((long)ci * Cout + co) * kk + t];
  }
}
// readout: out[b L + i][:] = GELU(tmp[b (L + 1) + 1 + i][:] + clsv[b][:]) (tmp: the token half of the linear over all token rows, clsv: the class
// half + bias per image); the class rows of tmp are dropped
__global__ __launch_bounds__(256) void depth_readout_kernel(const float* __restrict__ tmp, int ldt, const float* __restrict__ clsv, int ldc,
                                                            float* __restrict__ out, int ldo, int B, int L, int cq) {
  const long total = (long)B * L * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % cq);
    const long row = i / cq;
    const int b = (int)(row / L);
    const cgd_f32x4 v = *(const cgd_f32x4*)(tmp + (row + b + 1) * ldt + 4 * q), c = *(const cgd_f32x4*)(clsv + (long)b * ldc + 4 * q);
    cgd_f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float u = v[k] + c[k];
      o[k] = 0.5f * u * (1.f + erff(u * 0.70710678f));
    }
    *(cgd_f32x4*)(out + row * ldo + 4 * q) = o;
  }
}
// the head's tail: inv[r] = relu(bias + sum_c w[c] act(x[r][c])) over 32 channels (act = ReLU when relu_in), depth[r] = max((offset - inv[r]) /
// scale, floor).  Eight lanes per row, one float4 each; their partial sums meet in a fixed butterfly order.
__global__ __launch_bounds__(256) void depth_tail_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ inv, float* __restrict__ depth, long rows, int relu_in, float offset,
                                                         float scale, float floor_) {
  const long total = rows * 8;
  const int q = threadIdx.x & 7;
  const cgd_f32x4 wv = *(const cgd_f32x4*)(w + 4 * q);
  const float b0 = bias[0];
  for (long base = (long)blockIdx.x * 256; base < total; base += (long)gridDim.x * 256) {
    const long i = base + threadIdx.x;
    const bool valid = i < total;
    const long r = i >> 3;
    cgd_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (valid) v = *(const cgd_f32x4*)(x + r * ldx + 4 * q);
    if (relu_in) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
    float a = (v.x * wv.x + v.y * wv.y) + (v.z * wv.z + v.w * wv.w);
    a += __shfl_xor(a, 1, 64);
    a += __shfl_xor(a, 2, 64);
    a += __shfl_xor(a, 4, 64);
    if (valid && q == 0) {
      const float id = fmaxf(a + b0, 0.f);
      if (inv) inv[r] = id;
      if (depth) depth[r] = fmaxf((offset - id) / scale, floor_);
    }
  }
}
// antialiased cubic resize of `planes` (Hi, Wi) planes to (Ho, Wo) in gather form, out = a * resize(in) + b: the weight rows of resize_rows.h,
// with the taps that fall outside the image read at the nearest edge pixel.  One 16 x 16 tile of outputs per workgroup; its 16 + 16 weight rows
// are built once in LDS.  IDENT (same size): a copy (bit-identical when a = 1, b = 0)
template <bool IDENT>
__global__ __launch_bounds__(256) void depth_resize_kernel(const float* __restrict__ in, float* __restrict__ out, int Hi, int Wi, int Ho, int Wo, int Ty,
                                                           int Tx, float a, float b, float lo, int flags) {  // flags: bit 0 apply a / b, bit 1 apply lo
  __shared__ float wgt[2][16][kMaxTaps];
  __shared__ int left[2][16];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int ox = blockIdx.x * 16 + tx, oy = blockIdx.y * 16 + ty;
  const float* ip = in + (long)blockIdx.z * Hi * Wi;
  float* op = out + (long)blockIdx.z * Ho * Wo;
  if (IDENT) {
    if (ox < Wo && oy < Ho) {
      const float v = ip[(long)oy * Wi + ox];
      float o = (flags & 1) ? v * a + b : v;
      if (flags & 2) o = fmaxf(o, lo);
      op[(long)oy * Wo + ox] = o;
    }
    return;
  }
  if (threadIdx.x < 32) {
    const int axis = threadIdx.x >> 4, t = threadIdx.x & 15;  // 0: x rows, 1: y rows
    const int o = (axis ? blockIdx.y : blockIdx.x) * 16 + t;
    const int n = axis ? Hi : Wi, m = axis ? Ho : Wo;
    if (o < m) left[axis][t] = resize_row(n, m, o, axis ? Ty : Tx, &wgt[axis][t][0]);
  }
  __syncthreads();
  if (ox >= Wo || oy >= Ho) return;
  const int lx = left[0][tx], ly = left[1][ty];
  float acc = 0.f;
  for (int j = 0; j < Ty; ++j) {
    const int sy = min(max(ly + j, 0), Hi - 1);
    const float* rp = ip + (long)sy * Wi;
    float row = 0.f;
    for (int k = 0; k < Tx; ++k) row += wgt[0][tx][k] * rp[min(max(lx + k, 0), Wi - 1)];
    acc += wgt[1][ty][j] * row;
  }
  float o = (flags & 1) ? acc * a + b : acc;
  if (flags & 2) o = fmaxf(o, lo);
  op[(long)oy * Wo + ox] = o;
}

// ---- launchers: every refusal comes before any launch ---------------------------------------------------------------------------------
const char* rows_refusal(const void* in, int ldi, const void* out, int ldo, int C) {
  if (C <= 0 || (C & 3) || (ldi & 3) || (ldo & 3) || ldi < C || ldo < C) return "C and the row strides must be multiples of 4, strides >= C";
  if (!in || !out || !aligned16(in) || !aligned16(out)) return "in / out must be 16-byte aligned";
  return nullptr;
}
int launch_relu(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, long rows, int C, hipStream_t s) {
  if (const char* why = rows_refusal(in, ldi, out, ldo, C)) CGD_FAIL(ctx, std::string("relu_rows: ") + why);
  if (rows <= 0) CGD_FAIL(ctx, "relu_rows: rows must be positive");
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(depth_relu_kernel, dim3(grid_of(rows * (C / 4))), dim3(256), 0, s, in, ldi, out, ldo, rows, C / 4);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
int launch_up_ac(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, const float* add, int ldadd, int B, int Hi, int Wi, int C, hipStream_t s) {
  if (const char* why = rows_refusal(in, ldi, out, ldo, C)) CGD_FAIL(ctx, std::string("bilinear_up2x_ac: ") + why);
  if (B <= 0 || Hi <= 0 || Wi <= 0 || (long)B * Hi * Wi >= (1L << 28)) CGD_FAIL(ctx, "bilinear_up2x_ac: size out of range");
  if (add && ((ldadd & 3) || ldadd < C || !aligned16(add))) CGD_FAIL(ctx, "bilinear_up2x_ac: the add operand needs a 16-byte aligned pointer and a stride >= C, a multiple of 4");
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(depth_up2x_ac_kernel, dim3(grid_of((long)B * 4 * Hi * Wi * (C / 4))), dim3(256), 0, s, in, ldi, out, ldo, add, ldadd, B, Hi, Wi, C / 4);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
int launch_shuffle(cgd_ctx* ctx, const float* g, int ldg, const float* bias, float* out, int ldo, int B, int H, int W, int Cout, int k, hipStream_t s) {
  if (k != 2 && k != 4) CGD_FAIL(ctx, "deconv_shuffle: kernel = stride must be 2 or 4");
  if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0 || (Cout & 3) || (ldg & 3) || (ldo & 3) || ldg < Cout * k * k || ldo < Cout)
    CGD_FAIL(ctx, "deconv_shuffle: Cout and the row strides must be multiples of 4, strides >= the row widths");
  if ((long)B * H * W * k * k >= (1L << 28)) CGD_FAIL(ctx, "deconv_shuffle: size out of range");
  if (!g || !out || !aligned16(g) || !aligned16(out) || !aligned16(bias)) CGD_FAIL(ctx, "deconv_shuffle: g / out / bias must be 16-byte aligned");
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(depth_shuffle_kernel, dim3(grid_of((long)B * H * W * k * k * (Cout / 4))), dim3(256), 0, s, g, ldg, bias, out, ldo, B, H, W, Cout, k);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
int launch_tail(cgd_ctx* ctx, const float* x, int ldx, const float* w, const float* bias, float* inv, float* depth, long rows, int relu_in, float offset,
                float scale, float floor_, hipStream_t s) {
  if (rows <= 0 || rows >= (1L << 31) || ldx < 32 || (ldx & 3)) CGD_FAIL(ctx, "depth_head_tail: rows of 32 channels at a stride >= 32, a multiple of 4");
  if (!x || !w || !bias || (!inv && !depth) || !aligned16(x) || !aligned16(w)) CGD_FAIL(ctx, "depth_head_tail: missing or misaligned buffer");
  if (!(scale != 0.f)) CGD_FAIL(ctx, "depth_head_tail: scale must not be zero");
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(depth_tail_kernel, dim3(grid_of(rows * 8)), dim3(256), 0, s, x, ldx, w, bias, inv, depth, rows, relu_in, offset, scale, floor_);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
int launch_resize(cgd_ctx* ctx, const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, float a, float b, float lo, int clamp_lo, hipStream_t s) {
  if (planes <= 0 || planes > 65535 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) CGD_FAIL(ctx, "resize_cubic: size out of range");
  if ((long)Hi * Wi >= (1L << 30) || (long)Ho * Wo >= (1L << 30) || (Ho + 15) / 16 > 65535) CGD_FAIL(ctx, "resize_cubic: plane too large");
  const int Ty = resize_taps(Hi, Ho), Tx = resize_taps(Wi, Wo);
  if (Ty > kMaxTaps || Tx > kMaxTaps) CGD_FAIL(ctx, "resize_cubic: at most an 8-fold reduction per axis");
  if (!in || !out || in == out) CGD_FAIL(ctx, "resize_cubic: in and out are required and must differ");
  const int flags = (a == 1.f && b == 0.f ? 0 : 1) | (clamp_lo ? 2 : 0);
  const dim3 grid((Wo + 15) / 16, (Ho + 15) / 16, planes);
  if (Hi == Ho && Wi == Wo) CGD_LAUNCH(depth_resize_kernel<true>, grid, dim3(256), 0, s, in, out, Hi, Wi, Ho, Wo, Ty, Tx, a, b, lo, flags);
  else CGD_LAUNCH(depth_resize_kernel<false>, grid, dim3(256), 0, s, in, out, Hi, Wi, Ho, Wo, Ty, Tx, a, b, lo, flags);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
const char* readout_refusal(const void* tok, const void* w, const void* bias, const void* out, const void* tmp, const void* clsv, int B, int L, int W) {
  if (B <= 0 || L <= 0 || W <= 0 || (W & 31) || (long)B * (L + 1) >= (1L << 24)) return "depth_readout: W must be a multiple of 32, B and L positive";
  if (!tok || !w || !bias || !out || !tmp || !clsv) return "depth_readout: missing buffer";
  if (!aligned16(tok) || !aligned16(w) || !aligned16(bias) || !aligned16(out) || !aligned16(tmp) || !aligned16(clsv)) return "depth_readout: buffers must be 16-byte aligned";
  return nullptr;
}
// tok [B (L + 1)][W] (class token first), w [W][2W] (torch Linear: columns [token | class]), bias [W] -> out [B L][W]; tmp [B (L + 1)][W] and
// clsv [B][W] are scratch
int run_readout(cgd_ctx* ctx, const float* tok, const float* w, const float* bias, float* out, float* tmp, float* clsv, int B, int L, int W, int weight,
                hipStream_t s) {
  if (const char* why = readout_refusal(tok, w, bias, out, tmp, clsv, B, L, W)) CGD_FAIL(ctx, why);
  const long T = L + 1;
  {  // the class half, once per image: clsv[b] = w[:, W:] cls_b + bias (A rows = the class rows, T W apart)
    GemmParams p = lin(tok, (int)(T * W), w + W, W, clsv, W, bias, nullptr, 0, B, W);
    p.ldb = 2 * W;
    p.weight = weight;
    CGD_TRY(cgd_launch_gemm(ctx, p, s));
  }
  {
    GemmParams p = lin(tok, W, w, W, tmp, W, nullptr, nullptr, 0, (long)B * T, W);
    p.ldb = 2 * W;
    p.weight = weight;
    CGD_TRY(cgd_launch_gemm(ctx, p, s));
  }
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(depth_readout_kernel, dim3(grid_of((long)B * L * (W / 4))), dim3(256), 0, s, tmp, W, clsv, W, out, W, B, L, W / 4);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
const char* deconv_refusal(int B, int H, int W, int Cin, int Cout, int k) {
  if (k != 2 && k != 4) return "conv_transpose: kernel = stride must be 2 or 4";
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 31) || (Cout & 31)) return "conv_transpose: Cin and Cout must be positive multiples of 32";
  if ((long)B * H * W * k * k >= (1L << 28) || (long)Cout * k * k >= (1L << 20)) return "conv_transpose: size out of range";
  return nullptr;
}
// x [B*H*W][Cin] (stride ldx), wp: the packed weight (depth_pack_deconv_kernel) -> out [B][H k][W k] rows of Cout (stride ldo); g: scratch
// [B*H*W][Cout k k]
int run_deconv(cgd_ctx* ctx, const float* x, int ldx, const float* wp, const float* bias, float* out, int ldo, float* g, int B, int H, int W, int Cin,
               int Cout, int k, int weight, hipStream_t s) {
  if (const char* why = deconv_refusal(B, H, W, Cin, Cout, k)) CGD_FAIL(ctx, why);
  if (!x || !wp || !out || !g || !aligned16(x) || !aligned16(wp) || !aligned16(out) || !aligned16(g) || !aligned16(bias) || (ldx & 3) || ldx < Cin ||
      (ldo & 3) || ldo < Cout)
    CGD_FAIL(ctx, "conv_transpose: missing or misaligned buffer or stride");
  const int N = Cout * k * k;
  GemmParams p = lin(x, ldx, wp, Cin, g, N, nullptr, nullptr, 0, (long)B * H * W, N);
  p.weight = weight;
  CGD_TRY(cgd_launch_gemm(ctx, p, s));
  return launch_shuffle(ctx, g, N, bias, out, ldo, B, H, W, Cout, k, s);
}
int pack_deconv(cgd_ctx* ctx, const float* w, float* wp, int Cin, int Cout, int k, hipStream_t s) {
  CGD_LAUNCH(depth_pack_deconv_kernel, dim3(grid_of((long)Cin * Cout * k * k)), dim3(256), 0, s, w, wp, Cin, Cout, k * k);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

// ---- network ----------------------------------------------------------------------------------------------------------------------------
struct Conv3 {  // a 3x3 conv of stride 1; cinP / coutP: the device widths (multiples of 32, zero weights for the padding)
  std::string name;
  int cin = 0, cout = 0, cinP = 0, coutP = 0;
  bool has_bias = true;
  float *b = 0, *wpad = 0, *bpad = 0, *wf = 0, *wfp = 0;
};
struct Rcu {
  Conv3 c1, c2;
};

struct Depth : NetBase {
  cgd_depth_config cfg;
  int W = 0, PP = 0, F = 0, HC = 0;  // width, patch columns, features, the head's middle width (F / 2 padded to 32)
  int c[4] = {};
  std::vector<ClipBlock> blocks;
  ClipActs acts;  // one set of block scratch for all layers
  float *pw = 0, *pb = 0, *cls = 0, *pos = 0;
  float *ro_w[4] = {}, *ro_b[4] = {}, *pj_w[4] = {}, *pj_b[4] = {};
  float *dc_w[2] = {}, *dc_b[2] = {}, *dc_wp[2] = {};  // taps 1 and 2: ConvTranspose2d
  float *s2_w = 0, *s2_b = 0, *s2_wf = 0;              // tap 4: stride-2 conv
  Conv3 rn[4], head1, head2;
  Rcu rcu1[3], rcu2[4];  // refinenet{k}.resConfUnit1 (k = 1..3: refinenet4's is unused), resConfUnit2 (k = 1..4)
  float *oc_w[4] = {}, *oc_b[4] = {};
  float *tail_w = 0, *tail_b = 0;
  std::map<std::pair<int, int>, float*> pos_grid;  // cgd_depth_set_pos_embed: [(1 + gh gw)][W] per grid
  // last forward (cgd_depth_debug_map)
  int lastB = 0, lastgh = 0, lastgw = 0;
  bool have_fwd = false;
  bool stop_after_backbone = false;  // cgd_depth_debug_stop (benchmarks: the backbone's share of a call)
  DevBuf cols, pe, xa, xb, hook[4], ro_tmp, ro_cls, rd, pj, dg, tap[4], rnb[4], t1, t2, t3, oc, r1, cur[2], h1, hu, h2;

  int build();
  int finalize(hipStream_t s);
  int set_pos(int gh, int gw, const float* data);
  int forward(const float* img, int B, int h, int w, float offset, float scale, float floor_, float* inv, float* depth, hipStream_t s);
  void add_conv3(Conv3& cv, const std::string& name, int cin, int cout, bool bias) {
    cv.name = name; cv.cin = cin; cv.cout = cout; cv.cinP = pad32(cin); cv.coutP = pad32(cout); cv.has_bias = bias;
    add_param(name + ".weight", (int64_t)cout * cin * 9);
    if (bias) add_param(name + ".bias", cout);
  }
  int pack_conv3(Conv3& cv, hipStream_t s);
  int conv3(const float* A, const Conv3& cv, float* C, int B, int H, int Wd, const float* R, hipStream_t s) {
    GemmParams g;
    g.A = A; g.lda = cv.cinP; g.B = cv.wf; g.Bpk = cv.wfp; g.ldb = 9 * cv.cinP; g.C = C; g.ldc = cv.coutP; g.bias = cv.b; g.R = R; g.ldr = cv.coutP;
    g.M = B * H * Wd; g.N = cv.coutP; g.conv = 1; g.H = H; g.W = Wd; g.Cin = cv.cinP;
    return cgd_launch_gemm(ctx, g, s);
  }
  // y = conv2(relu(conv1(relu(x)))) + x on a (B, H, Wd) map of F channels; t1 / t2: scratch
  int run_rcu(const Rcu& r, const float* x, float* y, int B, int H, int Wd, hipStream_t s) {
    const long M = (long)B * H * Wd;
    CGD_TRY(launch_relu(ctx, x, F, t1.p, F, M, F, s));
    CGD_TRY(conv3(t1.p, r.c1, t2.p, B, H, Wd, nullptr, s));
    CGD_TRY(launch_relu(ctx, t2.p, F, t2.p, F, M, F, s));
    return conv3(t2.p, r.c2, y, B, H, Wd, x, s);
  }
};

int Depth::build() {
  W = cfg.width; F = cfg.features;
  if (cfg.patch <= 0 || (cfg.patch & 3) || cfg.patch > 64) CGD_FAIL(ctx, "depth: patch must be a multiple of 4, at most 64");
  if (W <= 0 || (W & 31) || cfg.heads <= 0 || W % cfg.heads || (W / cfg.heads != 64 && W / cfg.heads != 80))
    CGD_FAIL(ctx, "depth: width must be a multiple of 32 with a head dim of 64 or 80");
  if (cfg.layers < 1 || cfg.layers > 256 || cfg.native_grid < 1 || cfg.native_grid > 1024) CGD_FAIL(ctx, "depth: layers / native_grid out of range");
  for (int k = 0; k < 4; ++k) {
    if (cfg.hooks[k] < 0 || cfg.hooks[k] >= cfg.layers || (k && cfg.hooks[k] <= cfg.hooks[k - 1])) CGD_FAIL(ctx, "depth: hooks must be increasing block indices < layers");
    c[k] = cfg.reassemble_channels[k];
    if (c[k] <= 0 || (c[k] & 31)) CGD_FAIL(ctx, "depth: reassemble_channels must be positive multiples of 32");
  }
  if (F <= 0 || (F & 31)) CGD_FAIL(ctx, "depth: features must be a positive multiple of 32");
  PP = 3 * cfg.patch * cfg.patch;
  HC = pad32(F / 2);
  const std::string m = "pretrained.model.";
  add_param(m + "patch_embed.proj.weight", (int64_t)W * PP);
  add_param(m + "patch_embed.proj.bias", W);
  add_param(m + "cls_token", W);
  add_param(m + "pos_embed", (int64_t)(1 + cfg.native_grid * cfg.native_grid) * W);
  blocks.resize(cfg.layers);
  for (int l = 0; l < cfg.layers; ++l) {
    blocks[l].add_params(*this, m + "blocks." + std::to_string(l), W, cfg.heads, true);
    blocks[l].act = 3;
    blocks[l].eps = 1e-6f;
  }
  for (int k = 0; k < 4; ++k) {
    const std::string a = "pretrained.act_postprocess" + std::to_string(k + 1);
    add_param(a + ".0.project.0.weight", (int64_t)2 * W * W);
    add_param(a + ".0.project.0.bias", W);
    add_param(a + ".3.weight", (int64_t)c[k] * W);
    add_param(a + ".3.bias", c[k]);
    if (k < 2) {
      const int ks = k == 0 ? 4 : 2;
      add_param(a + ".4.weight", (int64_t)c[k] * c[k] * ks * ks);
      add_param(a + ".4.bias", c[k]);
    } else if (k == 3) {
      add_param(a + ".4.weight", (int64_t)c[k] * c[k] * 9);
      add_param(a + ".4.bias", c[k]);
    }
  }
  for (int k = 0; k < 4; ++k) add_conv3(rn[k], "scratch.layer" + std::to_string(k + 1) + "_rn", c[k], F, false);
  for (int k = 0; k < 4; ++k) {
    const std::string r = "scratch.refinenet" + std::to_string(k + 1);
    if (k < 3) {
      add_conv3(rcu1[k].c1, r + ".resConfUnit1.conv1", F, F, true);
      add_conv3(rcu1[k].c2, r + ".resConfUnit1.conv2", F, F, true);
    }
    add_conv3(rcu2[k].c1, r + ".resConfUnit2.conv1", F, F, true);
    add_conv3(rcu2[k].c2, r + ".resConfUnit2.conv2", F, F, true);
    add_param(r + ".out_conv.weight", (int64_t)F * F);
    add_param(r + ".out_conv.bias", F);
  }
  add_conv3(head1, "scratch.output_conv.0", F, F / 2, true);
  add_conv3(head2, "scratch.output_conv.2", F / 2, 32, true);
  add_param("scratch.output_conv.4.weight", 32);
  add_param("scratch.output_conv.4.bias", 1);
  return 0;
}

int Depth::pack_conv3(Conv3& cv, hipStream_t s) {
  const float* w = P(cv.name + ".weight");
  cv.b = cv.has_bias ? P(cv.name + ".bias") : nullptr;
  const size_t n = (size_t)cv.coutP * cv.cinP * 9;
  const bool padded = cv.cinP != cv.cin || cv.coutP != cv.cout;
  if (!cv.wf) {
    CGD_TRY(alloc(&cv.wf, n));
    CGD_TRY(alloc(&cv.wfp, cgd_hconv_packed_floats(cv.coutP, cv.cinP)));
    if (padded) {
      CGD_TRY(alloc(&cv.wpad, n));
      CGD_TRY(alloc(&cv.bpad, (size_t)cv.coutP));
    }
  }
  if (padded) {  // zero weights for the padded channels: they stay exactly zero and contribute nothing
    CGD_HIP(ctx, hipMemsetAsync(cv.wpad, 0, n * sizeof(float), s));
    CGD_HIP(ctx, hipMemsetAsync(cv.bpad, 0, (size_t)cv.coutP * sizeof(float), s));
    CGD_HIP(ctx, hipMemcpy2DAsync(cv.wpad, (size_t)cv.cinP * 9 * sizeof(float), w, (size_t)cv.cin * 9 * sizeof(float), (size_t)cv.cin * 9 * sizeof(float),
                                  (size_t)cv.cout, hipMemcpyDeviceToDevice, s));
    if (cv.b) CGD_HIP(ctx, hipMemcpyAsync(cv.bpad, cv.b, (size_t)cv.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    w = cv.wpad;
    if (cv.b) cv.b = cv.bpad;
  }
  CGD_TRY(cgd_pack_conv3x3(ctx, w, cv.wf, nullptr, cv.coutP, cv.cinP, s));
  return cgd_pack_conv3x3_frag(ctx, w, cv.wfp, cv.coutP, cv.cinP, 0, s);
}

int Depth::finalize(hipStream_t s) {
  CGD_TRY(check_all_set());
  const std::string m = "pretrained.model.";
  pw = P(m + "patch_embed.proj.weight"); pb = P(m + "patch_embed.proj.bias"); cls = P(m + "cls_token"); pos = P(m + "pos_embed");
  for (ClipBlock& b : blocks) b.lookup(*this);
  for (int k = 0; k < 4; ++k) {
    const std::string a = "pretrained.act_postprocess" + std::to_string(k + 1);
    ro_w[k] = P(a + ".0.project.0.weight"); ro_b[k] = P(a + ".0.project.0.bias");
    pj_w[k] = P(a + ".3.weight"); pj_b[k] = P(a + ".3.bias");
    if (k < 2) {
      const int ks = k == 0 ? 4 : 2;
      dc_w[k] = P(a + ".4.weight"); dc_b[k] = P(a + ".4.bias");
      if (!dc_wp[k]) CGD_TRY(alloc(&dc_wp[k], (size_t)c[k] * c[k] * ks * ks));
      CGD_TRY(pack_deconv(ctx, dc_w[k], dc_wp[k], c[k], c[k], ks, s));
    } else if (k == 3) {
      s2_w = P(a + ".4.weight"); s2_b = P(a + ".4.bias");
      if (!s2_wf) CGD_TRY(alloc(&s2_wf, (size_t)c[k] * c[k] * 9));
      CGD_TRY(cgd_pack_conv3x3(ctx, s2_w, s2_wf, nullptr, c[k], c[k], s));
    }
  }
  for (int k = 0; k < 4; ++k) {
    const std::string r = "scratch.refinenet" + std::to_string(k + 1);
    CGD_TRY(pack_conv3(rn[k], s));
    if (k < 3) {
      CGD_TRY(pack_conv3(rcu1[k].c1, s));
      CGD_TRY(pack_conv3(rcu1[k].c2, s));
    }
    CGD_TRY(pack_conv3(rcu2[k].c1, s));
    CGD_TRY(pack_conv3(rcu2[k].c2, s));
    oc_w[k] = P(r + ".out_conv.weight"); oc_b[k] = P(r + ".out_conv.bias");
  }
  CGD_TRY(pack_conv3(head1, s));
  CGD_TRY(pack_conv3(head2, s));
  tail_w = P("scratch.output_conv.4.weight"); tail_b = P("scratch.output_conv.4.bias");
  CGD_HIP(ctx, hipStreamSynchronize(s));
  finalized = true;
  have_fwd = false;
  return 0;
}

int Depth::set_pos(int gh, int gw, const float* data) {
  if (gh <= 0 || gw <= 0 || gh > 4096 || gw > 4096 || !data) CGD_FAIL(ctx, "depth: set_pos_embed needs a positive grid and the rows");
  float*& p = pos_grid[{gh, gw}];
  const size_t n = (size_t)(1 + (size_t)gh * gw) * W;
  if (!p) CGD_TRY(alloc(&p, n));
  CGD_HIP(ctx, hipMemcpy(p, data, n * sizeof(float), hipMemcpyDefault));
  return 0;
}

int Depth::forward(const float* img, int B, int h, int w, float offset, float scale, float floor_, float* inv, float* depth, hipStream_t s) {
  have_fwd = false;
  if (!finalized) CGD_FAIL(ctx, "depth: finalize() has not been called after the last set_param");
  if (B <= 0 || h <= 0 || w <= 0 || (h & 31) || (w & 31) || h % (2 * cfg.patch) || w % (2 * cfg.patch))
    CGD_FAIL(ctx, "depth: H and W must be positive multiples of 32 (and of twice the patch size)");
  if ((long)B * h * w >= (1L << 31) / 512) CGD_FAIL(ctx, "depth: batch * H * W too large");
  if (!img || (!inv && !depth) || !aligned16(img)) CGD_FAIL(ctx, "depth: img (16-byte aligned) and inv_depth or depth are required");
  if (!(scale != 0.f)) CGD_FAIL(ctx, "depth: scale must not be zero");
  const int P_ = cfg.patch, gh = h / P_, gw = w / P_, L = gh * gw, T = L + 1;
  const float* posr = nullptr;
  {
    auto it = pos_grid.find({gh, gw});
    if (it != pos_grid.end()) posr = it->second;
    else if (gh == cfg.native_grid && gw == cfg.native_grid) posr = pos;
    else CGD_FAIL(ctx, "depth: no position embedding for the " + std::to_string(gh) + " x " + std::to_string(gw) + " grid (cgd_depth_set_pos_embed)");
  }
  if (const char* why = cgd_sconv_refusal(0, c[3], c[3], 0, B, gh, gw, c[3], c[3])) CGD_FAIL(ctx, why);
  const long rows = (long)B * T, prow = (long)B * L;
  // ---- backbone
  CGD_TRY(ensure(cols, (size_t)prow * PP)); CGD_TRY(ensure(pe, (size_t)prow * W));
  CGD_TRY(ensure(xa, (size_t)rows * W)); CGD_TRY(ensure(xb, (size_t)rows * W));
  for (int k = 0; k < 4; ++k) CGD_TRY(ensure(hook[k], (size_t)rows * W));
  CGD_LAUNCH(depth_patchify_kernel, dim3(grid_of(prow * 3 * P_ * (P_ / 4))), dim3(256), 0, s, img, cols.p, B, h, w, P_);
  CGD_HIP(ctx, hipGetLastError());
  CGD_TRY(cgd_launch_gemm(ctx, lin(cols.p, PP, pw, PP, pe.p, W, pb, nullptr, 0, prow, W), s));
  CGD_TRY(cgd_launch_vit_tokens(ctx, pe.p, cls, posr, xa.p, B, T, W, s));
  const float* x = xa.p;
  for (int l = 0, k = 0; l < cfg.layers; ++l) {
    float* xo = x == xa.p ? xb.p : xa.p;
    if (k < 4 && cfg.hooks[k] == l) xo = hook[k++].p;
    CGD_TRY(clip_block_fwd(*this, blocks[l], acts, x, xo, B, T, false, s));
    x = xo;
    if (l == cfg.hooks[3]) break;  // blocks behind the last hook feed nothing
  }
  CGD_TRY(cgd_sync_pending(ctx, s));
  if (stop_after_backbone) return 0;
  // ---- readout + reassemble: tap k on the (gh, gw) * {4, 2, 1, 1/2} map
  const int mh[4] = {4 * gh, 2 * gh, gh, gh / 2}, mw[4] = {4 * gw, 2 * gw, gw, gw / 2};
  CGD_TRY(ensure(ro_tmp, (size_t)rows * W)); CGD_TRY(ensure(ro_cls, (size_t)B * W)); CGD_TRY(ensure(rd, (size_t)prow * W));
  for (int k = 0; k < 4; ++k) {
    const long mk = (long)B * mh[k] * mw[k];
    CGD_TRY(ensure(tap[k], (size_t)mk * c[k]));
    CGD_TRY(ensure(rnb[k], (size_t)mk * F));
    CGD_TRY(run_readout(ctx, hook[k].p, ro_w[k], ro_b[k], rd.p, ro_tmp.p, ro_cls.p, B, L, W, 1, s));
    float* pjo = tap[k].p;
    if (k != 2) {
      CGD_TRY(ensure(pj, (size_t)prow * c[k]));
      pjo = pj.p;
    }
    CGD_TRY(cgd_launch_gemm(ctx, lin(rd.p, W, pj_w[k], W, pjo, c[k], pj_b[k], nullptr, 0, prow, c[k]), s));
    if (k < 2) {
      const int ks = k == 0 ? 4 : 2;
      CGD_TRY(ensure(dg, (size_t)prow * c[k] * ks * ks));
      CGD_TRY(run_deconv(ctx, pj.p, c[k], dc_wp[k], dc_b[k], tap[k].p, c[k], dg.p, B, gh, gw, c[k], c[k], ks, 1, s));
    } else if (k == 3) {
      CGD_TRY(cgd_launch_sconv_fwd(ctx, pj.p, c[k], s2_wf, s2_b, tap[k].p, c[k], B, gh, gw, c[k], c[k], s));
    }
    CGD_TRY(conv3(tap[k].p, rn[k], rnb[k].p, B, mh[k], mw[k], nullptr, s));
  }
  // ---- fusion, from tap 4 down to tap 1
  const long m0 = (long)B * mh[0] * mw[0];
  CGD_TRY(ensure(t1, (size_t)m0 * F)); CGD_TRY(ensure(t2, (size_t)m0 * F)); CGD_TRY(ensure(t3, (size_t)m0 * F));
  CGD_TRY(ensure(oc, (size_t)m0 * F)); CGD_TRY(ensure(r1, (size_t)m0 * F));
  CGD_TRY(ensure(cur[0], (size_t)m0 * F)); CGD_TRY(ensure(cur[1], (size_t)m0 * 4 * F));
  const float* in = rnb[3].p;
  for (int k = 3; k >= 0; --k) {
    const long mk = (long)B * mh[k] * mw[k];
    CGD_TRY(run_rcu(rcu2[k], in, t3.p, B, mh[k], mw[k], s));
    CGD_TRY(cgd_launch_gemm(ctx, lin(t3.p, F, oc_w[k], F, oc.p, F, oc_b[k], nullptr, 0, mk, F), s));
    float* dst = k ? cur[k & 1].p : cur[1].p;  // (k = 0: the (8 gh, 8 gw) map, the largest)
    if (k) CGD_TRY(run_rcu(rcu1[k - 1], rnb[k - 1].p, r1.p, B, mh[k - 1], mw[k - 1], s));
    CGD_TRY(launch_up_ac(ctx, oc.p, F, dst, F, k ? r1.p : nullptr, F, B, mh[k], mw[k], F, s));
    in = dst;
  }
  // ---- head
  const int H2 = 2 * mh[0], W2 = 2 * mw[0];  // = h / 2, w / 2 for patch 16
  const long mhalf = (long)B * H2 * W2, mfull = 4 * mhalf;
  CGD_TRY(ensure(h1, (size_t)mhalf * HC)); CGD_TRY(ensure(hu, (size_t)mfull * HC)); CGD_TRY(ensure(h2, (size_t)mfull * 32));
  CGD_TRY(conv3(in, head1, h1.p, B, H2, W2, nullptr, s));
  CGD_TRY(launch_up_ac(ctx, h1.p, HC, hu.p, HC, nullptr, 0, B, H2, W2, HC, s));
  CGD_TRY(conv3(hu.p, head2, h2.p, B, 2 * H2, 2 * W2, nullptr, s));
  CGD_TRY(launch_tail(ctx, h2.p, 32, tail_w, tail_b, inv, depth, mfull, 1, offset, scale, floor_, s));
  lastB = B; lastgh = gh; lastgw = gw;
  have_fwd = true;
  return 0;
}

hipStream_t SS(void* s) { return (hipStream_t)s; }

}  // namespace

int cgd_launch_resize_cubic(cgd_ctx* ctx, const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, float a, float b, float lo,
                            int clamp_lo, hipStream_t s) {
  return launch_resize(ctx, in, out, planes, Hi, Wi, Ho, Wo, a, b, lo, clamp_lo, s);
}

struct cgd_depth {
  Depth net;
};

extern "C" {
int cgd_depth_create(cgd_ctx* ctx, const cgd_depth_config* cfg, cgd_depth** out) { return net_create(ctx, out, cfg); }
// host-only: the published checkpoint's own names (the groups the forward does not use are not listed)
int cgd_depth_manifest(const cgd_depth_config* cfg, void (*cb)(const char*, int64_t, void*), void* user) { return net_manifest<Depth>(cb, user, cfg); }
void cgd_depth_destroy(cgd_depth* v) { net_destroy(v); }
int cgd_depth_num_params(cgd_depth* v) { return net_num_params(v); }
int cgd_depth_param_info(cgd_depth* v, int i, char* buf, int len, int64_t* numel) { return net_param_info(v, i, buf, len, numel); }
int cgd_depth_set_param(cgd_depth* v, const char* name, const float* data, int64_t numel) { return net_set_param(v, name, data, numel); }
int cgd_depth_finalize(cgd_depth* v) { return net_finalize(v); }
int cgd_depth_set_pos_embed(cgd_depth* v, int gh, int gw, const float* data) {
  if (!v) return -3;
  DeviceScope dev_scope(v->net.ctx);
  return v->net.set_pos(gh, gw, data);
}
int cgd_depth_forward(cgd_depth* v, const float* img, int B, int H, int W, float offset, float scale, float floor_, float* inv_depth, float* depth,
                      void* stream) {
  return net_pass(v, stream, [&](hipStream_t s) { return v->net.forward(img, B, H, W, offset, scale, floor_, inv_depth, depth, s); });
}
// test support: the reassembled map of tap k (0..3) of the last forward, dense NHWC rows [B * mh * mw][c_k]; out3 = {rows per image height, width,
// channels}; out == NULL only reports the shape
int cgd_depth_debug_map(cgd_depth* v, int k, float* out, int* out3, void* stream) {
  if (!v) return -3;
  Depth& n = v->net;
  DeviceScope dev_scope(n.ctx);
  if (k < 0 || k > 3) CGD_FAIL(n.ctx, "depth: tap index must be 0..3");
  if (!n.have_fwd) CGD_FAIL(n.ctx, "depth: debug_map needs a preceding forward()");
  const int mh = k == 3 ? n.lastgh / 2 : n.lastgh << (2 - k), mw = k == 3 ? n.lastgw / 2 : n.lastgw << (2 - k);
  if (out3) { out3[0] = mh; out3[1] = mw; out3[2] = n.c[k]; }
  if (out) CGD_HIP(n.ctx, hipMemcpyAsync(out, n.tap[k].p, (size_t)n.lastB * mh * mw * n.c[k] * sizeof(float), hipMemcpyDeviceToDevice, SS(stream)));
  return 0;
}

// measurement support: after_backbone != 0 makes every later forward return behind the last hooked block, writing no output
int cgd_depth_debug_stop(cgd_depth* v, int after_backbone) {
  if (!v) return -3;
  v->net.stop_after_backbone = after_backbone != 0;
  return 0;
}

int cgd_op_relu_rows(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, int64_t rows, int C, void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  return launch_relu(ctx, in, ldi, out, ldo, rows, C, SS(stream));
}
int cgd_op_bilinear_up2x_ac(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, const float* add, int ldadd, int B, int Hi, int Wi, int C,
                            void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  return launch_up_ac(ctx, in, ldi, out, ldo, add, ldadd, B, Hi, Wi, C, SS(stream));
}
int cgd_op_conv_transpose(cgd_ctx* ctx, const float* x, int ldx, const float* w, const float* bias, float* out, int ldo, float* wpack, float* g, int B,
                          int H, int W, int Cin, int Cout, int k, void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  if (const char* why = deconv_refusal(B, H, W, Cin, Cout, k)) CGD_FAIL(ctx, why);
  if (!x || !w || !out || !wpack || !g || !aligned16(x) || !aligned16(wpack) || !aligned16(out) || !aligned16(g) || !aligned16(bias) || (ldx & 3) ||
      ldx < Cin || (ldo & 3) || ldo < Cout)
    CGD_FAIL(ctx, "conv_transpose: missing or misaligned buffer or stride");
  CGD_TRY(pack_deconv(ctx, w, wpack, Cin, Cout, k, SS(stream)));
  CGD_TRY(run_deconv(ctx, x, ldx, wpack, bias, out, ldo, g, B, H, W, Cin, Cout, k, 0, SS(stream)));
  return cgd_flush_pending(ctx, SS(stream));
}
int cgd_op_depth_readout(cgd_ctx* ctx, const float* tok, const float* w, const float* bias, float* out, float* tmp, float* clsv, int B, int L, int W,
                         void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  CGD_TRY(run_readout(ctx, tok, w, bias, out, tmp, clsv, B, L, W, 0, SS(stream)));
  return cgd_flush_pending(ctx, SS(stream));
}
int cgd_op_depth_head_tail(cgd_ctx* ctx, const float* x, int ldx, const float* w, const float* bias, float* inv_depth, float* depth, int64_t rows,
                           int relu_in, float offset, float scale, float floor_, void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  return launch_tail(ctx, x, ldx, w, bias, inv_depth, depth, rows, relu_in, offset, scale, floor_, SS(stream));
}
int cgd_op_resize_cubic(cgd_ctx* ctx, const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, float a, float b, float lo, int clamp_lo,
                        void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  return launch_resize(ctx, in, out, planes, Hi, Wi, Ho, Wo, a, b, lo, clamp_lo, SS(stream));
}
}  // extern "C"
