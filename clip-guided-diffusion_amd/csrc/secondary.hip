// Secondary diffusion model (SecondaryDiffusionImageNet2 of Katherine Crowson's CLIP-guided diffusion notebooks, also shipped with Disco
// Diffusion) on MI355X: forward and backward-to-input.
//
// A small convolutional denoiser that predicts the clean image for the guidance losses, so that CLIP's gradient returns to x_t through
// ~50 GFLOP of 3x3 convolutions (at 256x256) instead of through the UNet's backward pass.  With c = 64, cs = {64, 128, 128, 256, 256, 512}:
//   input  = cat(x, 16 constant planes [cos f | sin f]),  f = 2 pi t timestep_embed.weight^T
//   net    = ConvBlock(19, cs0), ConvBlock(cs0, cs0), Skip_1, ConvBlock(2 cs0, cs0), Conv2d(cs0, 3)         ConvBlock = conv3x3 + ReLU
//   Skip_k = cat(main_k(x), x),  main_k = AvgPool2d(2), ConvBlock(cs[k-1], cs[k]), ConvBlock(cs[k], cs[k]), Skip_{k+1},
//            ConvBlock(2 cs[k], cs[k]), ConvBlock(cs[k], cs[k-1]), bilinear x2                                (k = 1..4)
//   main_5 = AvgPool2d(2), ConvBlock(cs4, cs5), ConvBlock(cs5, cs5), ConvBlock(cs5, cs5), ConvBlock(cs5, cs4), bilinear x2
//   v = net(input),  pred = x cos(t pi / 2) - v sin(t pi / 2)
// Parameter names are the state-dict names of that nn.Sequential nesting (net.0.0.weight, net.2.main.1.0.weight, ..., net.4.weight,
// timestep_embed.weight), so the published secondary_model_imagenet_2.pth loads by name.
// Activations are NHWC rows.  The two halves of every skip concatenation are channel slices of ONE buffer per level that their producers (the
// bilinear upsample, the level's second ConvBlock) write through the row stride: no concat copy, forward or backward.  The 19-channel stem is
// zero-padded to 32 input channels; the 3-channel head and the stem's dgrad run on the thin-conv route (conv_thin.hip), which reads / writes
// the NCHW planes directly.  ReLU masks are recomputed from the stored post-ReLU activations.
// Precision: the trunk always runs in the exact-fp32 MFMA mode, like the LPIPS trunk (lpips.hip: a ReLU net's input gradient is discontinuous
// in its activations).  In that mode the launcher runs the 3x3 convolutions on the implicit-GEMM kernel (gemm.hip).
#include <algorithm>
#include <cmath>

#include "../../include/cgd_mi355x.h"
#include "net.h"
#include "mfma_stage.h"

namespace {

constexpr int NCV = 24;      // convolutions
constexpr int NRELU = 23;    // ... of which ConvBlocks (the head has no ReLU)
constexpr int STEM_CIN = 19, STEM_CINP = 32;
constexpr int NFREQ = 8;     // timestep_embed.weight [8][1] -> 16 Fourier planes
const int kCs[6] = {64, 128, 128, 256, 256, 512};
constexpr float kTwoPi = 6.283185307179586f, kHalfPi = 1.5707963267948966f;

int grid_of(long n) { return (int)std::min<long>((n + 255) / 256, 16384); }

// ---- kernels (all memory-bound: 16-byte accesses, one float4 of channels per thread) -----------------------------------------------
// NCHW x (B,3,H,W) + the 16 Fourier planes of t[b] -> the stem's NHWC rows [B*HW][32] (channels 19..31 zero).  grid.y = sample: the 16
// trigonometric values are computed once per workgroup, not per pixel.
__global__ __launch_bounds__(256) void sec_pack_kernel(const float* __restrict__ x, const float* __restrict__ t, const float* __restrict__ wemb,
                                                       float* __restrict__ out, int HW) {
  __shared__ float emb[2 * NFREQ + 16];  // [16..31]: the zero padding, so that every quad reads its values from one table
  const int b = blockIdx.y;
  if (threadIdx.x < 2 * NFREQ) {
    const float f = (kTwoPi * t[b]) * wemb[threadIdx.x & (NFREQ - 1)];
    emb[threadIdx.x] = threadIdx.x < NFREQ ? cosf(f) : sinf(f);
  } else if (threadIdx.x < 2 * NFREQ + 16) {
    emb[threadIdx.x] = 0.f;
  }
  __syncthreads();
  const long total = (long)HW * 8;
  const float* xb = x + (long)b * 3 * HW;
  float* ob = out + (long)b * HW * STEM_CINP;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i & 7);
    const long pix = i >> 3;
    cgd_f32x4 v;
    if (q == 0) {
      v = cgd_f32x4{xb[pix], xb[HW + pix], xb[2L * HW + pix], emb[0]};
    } else {
      v = cgd_f32x4{emb[4 * q - 3], emb[4 * q - 2], emb[4 * q - 1], emb[4 * q]};
    }
    *(cgd_f32x4*)(ob + pix * STEM_CINP + 4 * q) = v;
  }
}
// in place ReLU on a [rows][C] view with row stride ld
__global__ __launch_bounds__(256) void sec_relu_kernel(float* __restrict__ x, int ld, long rows, int cq) {
  const long total = rows * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / cq;
    const int q = (int)(i - r * cq);
    cgd_f32x4* p = (cgd_f32x4*)(x + r * ld + 4 * q);
    cgd_f32x4 v = *p;
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    *p = v;
  }
}
// da = da where the stored post-ReLU activation a is positive, else 0 (in place on da); both are strided views
__global__ __launch_bounds__(256) void sec_relu_bwd_kernel(const float* __restrict__ a, int lda, float* __restrict__ da, int ldd, long rows,
                                                           int cq) {
  const long total = rows * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = i / cq;
    const int q = (int)(i - r * cq);
    const cgd_f32x4 v = *(const cgd_f32x4*)(a + r * lda + 4 * q);
    cgd_f32x4* p = (cgd_f32x4*)(da + r * ldd + 4 * q);
    cgd_f32x4 d = *p;
    d.x = v.x > 0.f ? d.x : 0.f; d.y = v.y > 0.f ? d.y : 0.f; d.z = v.z > 0.f ? d.z : 0.f; d.w = v.w > 0.f ? d.w : 0.f;
    *p = d;
  }
}
// bilinear x2, align_corners = False: out[2i] = 1/4 in[i-1] + 3/4 in[i], out[2i+1] = 3/4 in[i] + 1/4 in[i+1], indices clamped at the borders,
// along both axes; in [B][Hi][Wi] rows of stride ldi, out [B][2Hi][2Wi] rows of stride ldo (a channel slice of a concat buffer).
// Written as PyTorch evaluates it: l0y (l0x v00 + l1x v01) + l1y (l0x v10 + l1x v11) with (y0, y1, l1y) = (i-1, i, 3/4) / (i, i+1, 1/4).
__global__ __launch_bounds__(256) void sec_up_fwd_kernel(const float* __restrict__ in, int ldi, float* __restrict__ out, int ldo, int B, int Hi,
                                                         int Wi, int cq) {
  const int Ho = 2 * Hi, Wo = 2 * Wi;
  const long total = (long)B * Ho * Wo * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % cq);
    const long pix = i / cq;
    const int ox = (int)(pix % Wo);
    const long r = pix / Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    // source coordinate (o + 0.5) / 2 - 0.5 clamped at 0: o = 0 -> (0, l1 = 0); even o -> (o/2 - 1, 3/4); odd o -> (o/2, 1/4)
    const int y0 = oy == 0 ? 0 : ((oy & 1) ? oy >> 1 : (oy >> 1) - 1), x0 = ox == 0 ? 0 : ((ox & 1) ? ox >> 1 : (ox >> 1) - 1);
    const float ly = oy == 0 ? 0.f : ((oy & 1) ? 0.25f : 0.75f), lx = ox == 0 ? 0.f : ((ox & 1) ? 0.25f : 0.75f);
    const int y1 = min(y0 + 1, Hi - 1), x1 = min(x0 + 1, Wi - 1);
    const float* base = in + (long)b * Hi * Wi * ldi + 4 * q;
    const cgd_f32x4 v00 = *(const cgd_f32x4*)(base + ((long)y0 * Wi + x0) * ldi), v01 = *(const cgd_f32x4*)(base + ((long)y0 * Wi + x1) * ldi),
                    v10 = *(const cgd_f32x4*)(base + ((long)y1 * Wi + x0) * ldi), v11 = *(const cgd_f32x4*)(base + ((long)y1 * Wi + x1) * ldi);
    cgd_f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (1.f - ly) * ((1.f - lx) * v00[k] + lx * v01[k]) + ly * ((1.f - lx) * v10[k] + lx * v11[k]);
    *(cgd_f32x4*)(out + pix * ldo + 4 * q) = o;
  }
}
// adjoint of the above in gather form (no atomics): input pixel i collects, per axis, the output pixels {max(2i-1, 0), 2i, 2i+1,
// min(2i+2, 2n-1)} with weights {1/4, 3/4, 3/4, 1/4} (the clamped taps of the two border outputs fall onto the border input again).
// dout [B][2Hi][2Wi] rows of stride ldo (a channel slice), din [B][Hi][Wi] rows of stride ldi
__global__ __launch_bounds__(256) void sec_up_bwd_kernel(const float* __restrict__ dout, int ldo, float* __restrict__ din, int ldi, int B, int Hi,
                                                         int Wi, int cq) {
  const int Ho = 2 * Hi, Wo = 2 * Wi;
  const long total = (long)B * Hi * Wi * cq;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int q = (int)(i % cq);
    const long pix = i / cq;
    const int ix = (int)(pix % Wi);
    const long r = pix / Wi;
    const int iy = (int)(r % Hi), b = (int)(r / Hi);
    const int ys[4] = {max(2 * iy - 1, 0), 2 * iy, 2 * iy + 1, min(2 * iy + 2, Ho - 1)};
    const int xs[4] = {max(2 * ix - 1, 0), 2 * ix, 2 * ix + 1, min(2 * ix + 2, Wo - 1)};
    const float wt[4] = {0.25f, 0.75f, 0.75f, 0.25f};
    const float* base = dout + (long)b * Ho * Wo * ldo + 4 * q;
    cgd_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      cgd_f32x4 row = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const cgd_f32x4 v = *(const cgd_f32x4*)(base + ((long)ys[a] * Wo + xs[c]) * ldo);
#pragma unroll
        for (int k = 0; k < 4; ++k) row[k] += wt[c] * v[k];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += wt[a] * row[k];
    }
    *(cgd_f32x4*)(din + pix * ldi + 4 * q) = acc;
  }
}
// head: pred = x cos(t pi / 2) - v sin(t pi / 2) and (xin != null) x_in = pred fac + x (1 - fac); all (B,3,H,W) NCHW, n4 = 3 HW / 4 per
// sample.  grid.y = sample: one cos / sin pair per workgroup.
__global__ __launch_bounds__(256) void sec_head_kernel(const float* __restrict__ v, const float* __restrict__ x, const float* __restrict__ t,
                                                       float* __restrict__ pred, float* __restrict__ xin, long n4, float fac) {
  __shared__ float cs[2];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    const float a = t[b] * kHalfPi;
    cs[0] = cosf(a);
    cs[1] = sinf(a);
  }
  __syncthreads();
  const float al = cs[0], sg = cs[1];
  const long off = (long)b * n4;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const cgd_f32x4 vv = ((const cgd_f32x4*)v)[off + i], xv = ((const cgd_f32x4*)x)[off + i];
    cgd_f32x4 p, o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      p[k] = xv[k] * al - vv[k] * sg;
      o[k] = p[k] * fac + xv[k] * (1.f - fac);
    }
    ((cgd_f32x4*)pred)[off + i] = p;
    if (xin) ((cgd_f32x4*)xin)[off + i] = o;
  }
}
// The secondary-path counterpart of guidance_combine_kernel (guidance.hip):
//   G_in = gin + tv + sat (on x_in);  G_pred = fac G_in + range (on pred);  gdir = (1 - fac) G_in + alpha G_pred;  seed = -sigma G_pred
// (pred = alpha x - sigma v, x_in = fac pred + (1 - fac) x).  per-block partial sums of the tv / range / sat losses -> part[block][3]
__global__ __launch_bounds__(256) void sec_combine_kernel(const float* __restrict__ gin, const float* __restrict__ xin, const float* __restrict__ pred,
                                                          float* __restrict__ gdir, float* __restrict__ seed, float* __restrict__ part, int B, int H,
                                                          int W, float fac, float alpha, float sigma, float tv_scale, float range_scale,
                                                          float sat_scale) {
  const int HW3 = 3 * H * W;
  const long total = (long)B * HW3;
  const float invN = 1.f / (float)HW3;
  float l_tv = 0.f, l_rng = 0.f, l_sat = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int xx = (int)(i % W);
    const int yy = (int)((i / W) % H);
    const float v = xin[i];
    const float dxr = xx + 1 < W ? xin[i + 1] - v : 0.f;
    const float dyd = yy + 1 < H ? xin[i + W] - v : 0.f;
    const float dxl = xx > 0 ? v - xin[i - 1] : 0.f;
    const float dyu = yy > 0 ? v - xin[i - W] : 0.f;
    l_tv += dxr * dxr + dyd * dyd;
    float g = gin ? gin[i] : 0.f;
    g += tv_scale * 2.f * invN * (dxl - dxr + dyu - dyd);
    const float over = v - fminf(fmaxf(v, -1.f), 1.f);
    if (sat_scale != 0.f) {
      l_sat += fabsf(over);
      g += sat_scale * (over > 0.f ? 1.f : (over < 0.f ? -1.f : 0.f)) * invN / (float)B;
    }
    const float p0 = pred[i];
    const float ro = p0 - fminf(fmaxf(p0, -1.f), 1.f);
    l_rng += ro * ro;
    const float gp = fac * g + range_scale * 2.f * invN * ro;
    gdir[i] = (1.f - fac) * g + alpha * gp;
    seed[i] = -sigma * gp;
  }
  __shared__ float red[3][4];
  for (int o = 32; o > 0; o >>= 1) {
    l_tv += __shfl_xor(l_tv, o, 64);
    l_rng += __shfl_xor(l_rng, o, 64);
    l_sat += __shfl_xor(l_sat, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][wave] = l_tv;
    red[1][wave] = l_rng;
    red[2][wave] = l_sat;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const float s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    const float sc = threadIdx.x == 0 ? tv_scale * invN : (threadIdx.x == 1 ? range_scale * invN : sat_scale * invN / (float)B);
    part[blockIdx.x * 3 + threadIdx.x] = s * sc;
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int launch_pack(cgd_ctx* ctx, const float* x, const float* t, const float* wemb, float* out, int B, int H, int W, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535) CGD_FAIL(ctx, "secondary pack: size out of range");
  if (!x || !t || !wemb || !out || !aligned16(out)) CGD_FAIL(ctx, "secondary pack: missing or misaligned buffer");
  const int HW = H * W;
  CGD_LAUNCH(sec_pack_kernel, dim3(std::min(grid_of((long)HW * 8), 4096), B), dim3(256), 0, s, x, t, wemb, out, HW);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
int launch_up(cgd_ctx* ctx, bool adjoint, const float* in, int ldi, float* out, int ldo, int B, int Hi, int Wi, int C, hipStream_t s) {
  // in / ldi: the (Hi, Wi) side, out / ldo: the (2 Hi, 2 Wi) side, whichever of the two is written
  CGD_TRY(cgd_sync_pending(ctx, s));
  if (B <= 0 || Hi <= 0 || Wi <= 0 || C <= 0 || (C & 3) || (ldi & 3) || (ldo & 3) || ldi < C || ldo < C)
    CGD_FAIL(ctx, "bilinear_up2x: C and the row strides must be multiples of 4, strides >= C");
  if (!in || !out || !aligned16(in) || !aligned16(out)) CGD_FAIL(ctx, "bilinear_up2x: in / out must be 16-byte aligned");
  if (adjoint)
    CGD_LAUNCH(sec_up_bwd_kernel, dim3(grid_of((long)B * Hi * Wi * (C / 4))), dim3(256), 0, s, out, ldo, const_cast<float*>(in), ldi, B, Hi, Wi, C / 4);
  else
    CGD_LAUNCH(sec_up_fwd_kernel, dim3(grid_of((long)B * 4 * Hi * Wi * (C / 4))), dim3(256), 0, s, in, ldi, out, ldo, B, Hi, Wi, C / 4);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
int launch_head(cgd_ctx* ctx, const float* v, const float* x, const float* t, float fac, float* pred, float* xin, int B, int H, int W,
                hipStream_t s) {
  const long n = 3L * H * W;
  if (B <= 0 || H <= 0 || W <= 0 || B > 65535 || (n & 3)) CGD_FAIL(ctx, "secondary head: 3 H W must be a multiple of 4");
  if (!v || !x || !t || !pred || !aligned16(v) || !aligned16(x) || !aligned16(pred) || !aligned16(xin))
    CGD_FAIL(ctx, "secondary head: missing or misaligned buffer");
  CGD_LAUNCH(sec_head_kernel, dim3(std::min(grid_of(n / 4), 1024), B), dim3(256), 0, s, v, x, t, pred, xin, n / 4, fac);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

// ---- network ------------------------------------------------------------------------------------------------------------------------
struct SConv {
  std::string name;      // state-dict prefix ("net.2.main.1.0")
  int level = 0;         // map = (H >> level, W >> level)
  int cin = 0, cout = 0, cinP = 0;
  float *w = 0, *b = 0;  // parameters as uploaded
  float *wpad = 0;       // stem: [cout][32][3][3] zero-padded copy
  float *wf = 0, *wd = 0;
  // forward operands: input view and output view (set per pass)
  TV in, out, din;       // din: where this conv's dgrad writes (a view of the gradient w.r.t. `in`)
};

struct Secondary : NetBase {
  static constexpr bool uses_frag_cache = false;  // conv operands only: nothing of this net lives in the context's packed-weight cache
  SConv cv[NCV];
  float* wemb = 0;
  int B = 0, H = 0, W = 0;
  bool have_fwd = false;
  // per level k = 0..4: the skip concatenation [M_k][2 cs[k]] = [up(main_{k+1}) | x_k] and its gradient; pooled input of level k + 1;
  // plain activations of the remaining ConvBlocks; v (B,3,H,W)
  DevBuf in0, cat[5], dcat[5], pin[6], dpin[6], act[NCV], dact[NCV], vbuf;
  const float* replay[NRELU] = {};
  bool replay_on = false;

  int build();
  int finalize(hipStream_t s);
  int forward(const float* x, const float* t, int Bn, int Hh, int Ww, float fac, float* pred, float* xin, hipStream_t s);
  int dgrad(const float* dv, float* dx, hipStream_t s);
  long rows(int level) const { return (long)B * (H >> level) * (W >> level); }
  int conv(const float* A, int lda, int cin, const float* Wt, const float* bias, float* C, int ldc, int cout, int level, const float* R, int ldr,
           hipStream_t s) {
    GemmParams g;
    g.A = A; g.lda = lda; g.B = Wt; g.ldb = 9 * cin; g.C = C; g.ldc = ldc; g.bias = bias; g.R = R; g.ldr = ldr;
    g.M = (int)rows(level); g.N = cout; g.conv = 1; g.H = H >> level; g.W = W >> level; g.Cin = cin;
    return cgd_launch_gemm(ctx, g, s);
  }
  void relu(const TV& v, long M, hipStream_t s) {
    CGD_LAUNCH(sec_relu_kernel, dim3(grid_of(M * (v.C / 4))), dim3(256), 0, s, v.p, v.ld, M, v.C / 4);
  }
  void relu_bwd(const TV& a, const TV& da, long M, hipStream_t s) {
    CGD_LAUNCH(sec_relu_bwd_kernel, dim3(grid_of(M * (a.C / 4))), dim3(256), 0, s, a.p, a.ld, da.p, da.ld, M, a.C / 4);
  }
};

// execution order of the 24 convolutions: 0 1 | level k = 1..4: (2k, 2k+1) | level 5: 10..13 | level k = 4..1: (14 + 2(4-k), +1) | 22 23
int Secondary::build() {
  int n = 0;
  auto add = [&](const std::string& name, int level, int cin, int cout) {
    SConv& c = cv[n++];
    c.name = name; c.level = level; c.cin = cin; c.cout = cout; c.cinP = cin == STEM_CIN ? STEM_CINP : cin;
    add_param(name + ".weight", (int64_t)cout * cin * 9);
    add_param(name + ".bias", cout);
  };
  std::string pre[6];
  pre[1] = "net.2.main";
  for (int k = 2; k <= 5; ++k) pre[k] = pre[k - 1] + ".3.main";
  add("net.0.0", 0, STEM_CIN, kCs[0]);
  add("net.1.0", 0, kCs[0], kCs[0]);
  for (int k = 1; k <= 4; ++k) {
    add(pre[k] + ".1.0", k, kCs[k - 1], kCs[k]);
    add(pre[k] + ".2.0", k, kCs[k], kCs[k]);
  }
  add(pre[5] + ".1.0", 5, kCs[4], kCs[5]);
  add(pre[5] + ".2.0", 5, kCs[5], kCs[5]);
  add(pre[5] + ".3.0", 5, kCs[5], kCs[5]);
  add(pre[5] + ".4.0", 5, kCs[5], kCs[4]);
  for (int k = 4; k >= 1; --k) {
    add(pre[k] + ".4.0", k, 2 * kCs[k], kCs[k]);
    add(pre[k] + ".5.0", k, kCs[k], kCs[k - 1]);
  }
  add("net.3.0", 0, 2 * kCs[0], kCs[0]);
  add("net.4", 0, kCs[0], 3);
  add_param("timestep_embed.weight", NFREQ);
  return n == NCV ? 0 : -2;
}

int Secondary::finalize(hipStream_t s) {
  CGD_TRY(check_all_set());
  for (int l = 0; l < NCV; ++l) {
    SConv& c = cv[l];
    c.w = P(c.name + ".weight");
    c.b = P(c.name + ".bias");
    const size_t n = (size_t)c.cout * c.cinP * 9;
    if (!c.wf) {
      CGD_TRY(alloc(&c.wf, n));
      CGD_TRY(alloc(&c.wd, n));
      if (c.cinP != c.cin) CGD_TRY(alloc(&c.wpad, n));
    }
    const float* w = c.w;
    if (c.wpad) {  // zero weights for the padded input channels: they contribute nothing forward, and their dgrad rows are never read
      CGD_HIP(ctx, hipMemsetAsync(c.wpad, 0, n * sizeof(float), s));
      CGD_HIP(ctx, hipMemcpy2DAsync(c.wpad, (size_t)c.cinP * 9 * sizeof(float), c.w, (size_t)c.cin * 9 * sizeof(float),
                                    (size_t)c.cin * 9 * sizeof(float), (size_t)c.cout, hipMemcpyDeviceToDevice, s));
      w = c.wpad;
    }
    CGD_TRY(cgd_pack_conv3x3(ctx, w, c.wf, c.wd, c.cout, c.cinP, s));
  }
  wemb = P("timestep_embed.weight");
  CGD_HIP(ctx, hipStreamSynchronize(s));
  finalized = true;
  have_fwd = false;
  return 0;
}

int Secondary::forward(const float* x, const float* t, int Bn, int Hh, int Ww, float fac, float* pred, float* xin, hipStream_t s) {
  have_fwd = false;  // a refused or failed forward leaves nothing a dgrad could belong to
  if (!finalized) CGD_FAIL(ctx, "secondary: weights not finalized");
  if (Bn <= 0 || Hh <= 0 || Ww <= 0 || (Hh & 31) || (Ww & 31)) CGD_FAIL(ctx, "secondary: H and W must be positive multiples of 32");
  if ((long)Bn * Hh * Ww >= (1L << 31) / 128) CGD_FAIL(ctx, "secondary: batch * H * W too large");
  if (!x || !t || !pred) CGD_FAIL(ctx, "secondary: x, t and pred are required");
  B = Bn; H = Hh; W = Ww;
  // buffers: concat pairs, pooled inputs, plain activations; the views of every conv
  CGD_TRY(ensure(in0, (size_t)rows(0) * STEM_CINP));
  for (int k = 0; k < 5; ++k) CGD_TRY(ensure(cat[k], (size_t)rows(k) * 2 * kCs[k]));
  for (int k = 1; k <= 5; ++k) CGD_TRY(ensure(pin[k], (size_t)rows(k) * kCs[k - 1]));
  CGD_TRY(ensure(vbuf, (size_t)B * 3 * H * W));
  auto second_half = [&](int k) { return TV{cat[k].p + kCs[k], 2 * kCs[k], kCs[k]}; };
  auto whole = [&](int k) { return TV{cat[k].p, 2 * kCs[k], 2 * kCs[k]}; };
  for (int l = 0; l < NCV - 1; ++l) {
    SConv& c = cv[l];
    const bool to_cat = l == 1 || (l >= 2 && l <= 9 && (l & 1));  // the level's second ConvBlock: x_k, the right half of cat[k]
    if (to_cat) {
      c.out = second_half(c.level);
    } else {
      CGD_TRY(ensure(act[l], (size_t)rows(c.level) * c.cout));
      c.out = TV{act[l].p, c.cout, c.cout};
    }
  }
  cv[0].in = TV{in0.p, STEM_CINP, STEM_CINP};
  for (int l = 1; l < NCV; ++l) {
    SConv& c = cv[l];
    const bool pooled = l >= 2 && l <= 10 && !(l & 1);       // first ConvBlock of levels 1..5
    const bool from_cat = l >= 14 && l <= 22 && !(l & 1);    // first ConvBlock after a SkipBlock
    if (pooled) c.in = TV{pin[c.level].p, c.cin, c.cin};
    else if (from_cat) c.in = whole(c.level);
    else c.in = cv[l - 1].out;
  }
  CGD_TRY(launch_pack(ctx, x, t, wemb, in0.p, B, H, W, s));
  int nrelu = 0;
  for (int l = 0; l < NCV - 1; ++l) {
    SConv& c = cv[l];
    const long M = rows(c.level);
    if (l >= 2 && l <= 10 && !(l & 1)) {  // AvgPool2d(2) of x_{k-1}
      const TV src = second_half(c.level - 1);
      CGD_TRY(cgd_launch_pool2x2(ctx, src.p, src.ld, c.in.p, c.in.ld, nullptr, 0, B, H >> c.level, W >> c.level, c.cin, 0.25f, s));
    }
    CGD_TRY(conv(c.in.p, c.in.ld, c.cinP, c.wf, c.b, c.out.p, c.out.ld, c.cout, c.level, nullptr, 0, s));
    relu(c.out, M, s);
    if (replay_on && replay[nrelu])
      CGD_TRY(cgd_launch_copy2d(ctx, replay[nrelu], c.cout, nullptr, 0, c.out.p, c.out.ld, M, c.cout, s));
    ++nrelu;
    if (l == 13 || (l >= 15 && l <= 21 && (l & 1))) {  // last ConvBlock of main_k: bilinear x2 into the left half of cat[k - 1]
      const int k = c.level;
      CGD_TRY(launch_up(ctx, false, c.out.p, c.out.ld, cat[k - 1].p, 2 * kCs[k - 1], B, H >> k, W >> k, c.cout, s));
    }
  }
  // head: Conv2d(cs0, 3) straight into NCHW v, then pred (and the blend)
  SConv& hd = cv[NCV - 1];
  CGD_TRY(cgd_launch_conv_thin_out(ctx, hd.in.p, hd.in.ld, hd.wf, hd.b, vbuf.p, B, H, W, hd.cin, 3, s));
  CGD_TRY(launch_head(ctx, vbuf.p, x, t, fac, pred, xin, B, H, W, s));
  CGD_HIP(ctx, hipGetLastError());
  have_fwd = true;
  return 0;
}

// dx = d(sum(v * dv)) / dx of the last forward (x enters through the stem only; t is not differentiated)
int Secondary::dgrad(const float* dv, float* dx, hipStream_t s) {
  if (!finalized) CGD_FAIL(ctx, "secondary: weights not finalized");
  if (!have_fwd) CGD_FAIL(ctx, "secondary: dgrad without a forward");
  if (!dv || !dx) CGD_FAIL(ctx, "secondary: dv and dx are required");
  for (int k = 0; k < 5; ++k) CGD_TRY(ensure(dcat[k], (size_t)rows(k) * 2 * kCs[k]));
  for (int k = 1; k <= 5; ++k) CGD_TRY(ensure(dpin[k], (size_t)rows(k) * kCs[k - 1]));
  // gradient w.r.t. the OUTPUT of conv l (post-ReLU): a plain buffer each
  TV dout[NCV];
  for (int l = 0; l < NCV - 1; ++l) {
    SConv& c = cv[l];
    CGD_TRY(ensure(dact[l], (size_t)rows(c.level) * c.cout));
    dout[l] = TV{dact[l].p, c.cout, c.cout};
  }
  // head dgrad: NCHW dv (3 channels) -> the gradient of net.3's activation, on the thin input-side conv with the head's dgrad pack
  SConv& hd = cv[NCV - 1];
  CGD_TRY(cgd_launch_conv_in(ctx, dv, hd.wd, nullptr, dout[NCV - 2].p, B, H, W, 3, hd.cin, s, dout[NCV - 2].ld));
  for (int l = NCV - 2; l >= 1; --l) {
    SConv& c = cv[l];
    const long M = rows(c.level);
    const int k = c.level;
    relu_bwd(c.out, dout[l], M, s);
    const bool pooled = l >= 2 && l <= 10 && !(l & 1);
    const bool from_cat = l >= 14 && l <= 22 && !(l & 1);
    if (from_cat) {
      // gradient of the whole concatenation; its left half is the bilinear upsample's output gradient, its right half joins x_k's
      CGD_TRY(conv(dout[l].p, dout[l].ld, c.cout, c.wd, nullptr, dcat[k].p, 2 * kCs[k], c.cin, k, nullptr, 0, s));
      const int up_src = l == 14 ? 13 : l - 1;  // the conv whose output was upsampled into cat[k]: level k + 1
      CGD_TRY(launch_up(ctx, true, dout[up_src].p, dout[up_src].ld, dcat[k].p, 2 * kCs[k], B, H >> (k + 1), W >> (k + 1), cv[up_src].cout, s));
    } else if (pooled) {
      // gradient w.r.t. the pooled input, then the pool's adjoint plus the skip gradient of x_{k-1} (the right half of dcat[k-1]); the
      // x_{k-1} producer is the conv right before this one in execution order
      CGD_TRY(conv(dout[l].p, dout[l].ld, c.cout, c.wd, nullptr, dpin[k].p, c.cin, c.cin, k, nullptr, 0, s));
      CGD_TRY(cgd_launch_upsample2x(ctx, dpin[k].p, c.cin, dout[l - 1].p, dout[l - 1].ld, dcat[k - 1].p + kCs[k - 1], 2 * kCs[k - 1], B,
                                    H >> (k - 1), W >> (k - 1), c.cin, 0.25f, s));
    } else {
      CGD_TRY(conv(dout[l].p, dout[l].ld, c.cout, c.wd, nullptr, dout[l - 1].p, dout[l - 1].ld, c.cin, k, nullptr, 0, s));
    }
  }
  // stem: ReLU mask, then the three image channels of its dgrad (rows 0..2 of the [32][9 * 64] dgrad pack) straight into NCHW
  relu_bwd(cv[0].out, dout[0], rows(0), s);
  CGD_TRY(cgd_launch_conv_thin_out(ctx, dout[0].p, dout[0].ld, cv[0].wd, nullptr, dx, B, H, W, cv[0].cout, 3, s));
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

}  // namespace

struct cgd_secondary {
  Secondary net;
};

static hipStream_t SS(void* s) { return (hipStream_t)s; }

extern "C" {
int cgd_secondary_create(cgd_ctx* ctx, cgd_secondary** out) { return net_create(ctx, out); }
int cgd_secondary_manifest(void (*cb)(const char*, int64_t, void*), void* user) { return net_manifest<Secondary>(cb, user); }
void cgd_secondary_destroy(cgd_secondary* v) { net_destroy(v); }
int cgd_secondary_num_params(cgd_secondary* v) { return net_num_params(v); }
int cgd_secondary_param_info(cgd_secondary* v, int i, char* buf, int len, int64_t* numel) { return net_param_info(v, i, buf, len, numel); }
int cgd_secondary_set_param(cgd_secondary* v, const char* name, const float* data, int64_t numel) { return net_set_param(v, name, data, numel); }
int cgd_secondary_finalize(cgd_secondary* v) { return net_finalize(v); }
int cgd_secondary_forward(cgd_secondary* v, const float* x, const float* t, int B, int H, int W, float* pred, void* stream) {
  return net_pass(v, stream, [&](hipStream_t s) {
    ExactScope exact(v->net.ctx);
    return v->net.forward(x, t, B, H, W, 0.f, pred, nullptr, s);
  });
}
int cgd_secondary_forward_blend(cgd_secondary* v, const float* x, const float* t, int B, int H, int W, float fac, float* pred, float* x_in,
                                void* stream) {
  return net_pass(v, stream, [&](hipStream_t s) {
    ExactScope exact(v->net.ctx);
    if (!x_in) {
      v->net.ctx->err = "secondary: x_in is required";
      return -2;
    }
    return v->net.forward(x, t, B, H, W, fac, pred, x_in, s);
  });
}
int cgd_secondary_dgrad(cgd_secondary* v, const float* dv_seed, float* dx, void* stream) {
  return net_pass(v, stream, [&](hipStream_t s) {
    ExactScope exact(v->net.ctx);
    return v->net.dgrad(dv_seed, dx, s);
  });
}
// test support: mask replay (as cgd_lpips_debug_replay).  acts: 23 device pointers, the post-ReLU activations of the ConvBlocks in execution
// order ([B*h*w][cout] dense NHWC rows) for the input the following forward calls are given, or NULL to switch the replay off.  Every forward
// continues from these activations, so the ReLU masks of the next dgrad are the caller's.  Not used by the product path.
int cgd_secondary_debug_replay(cgd_secondary* v, const float* const* acts) {
  if (!v) return -3;
  v->net.replay_on = acts != nullptr;
  for (int l = 0; l < NRELU; ++l) v->net.replay[l] = acts ? acts[l] : nullptr;
  return 0;
}
int cgd_secondary_head(cgd_ctx* ctx, const float* v, const float* x, const float* t, float fac, float* pred, float* x_in, int B, int H, int W,
                       void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  return launch_head(ctx, v, x, t, fac, pred, x_in, B, H, W, SS(stream));
}
int cgd_secondary_combine(cgd_ctx* ctx, const float* g_in, const float* x_in, const float* pred, float* g_direct, float* seed3, float* loss_part,
                          int B, int H, int W, float fac, float alpha, float sigma, float tv_scale, float range_scale, float sat_scale,
                          void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  if (B <= 0 || H <= 0 || W <= 0 || !x_in || !pred || !g_direct || !seed3 || !loss_part) CGD_FAIL(ctx, "secondary combine: missing buffer or empty shape");
  CGD_LAUNCH(sec_combine_kernel, dim3(cgd_guidance_part_blocks(B, H, W)), dim3(256), 0, SS(stream), g_in, x_in, pred, g_direct, seed3, loss_part,
             B, H, W, fac, alpha, sigma, tv_scale, range_scale, sat_scale);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}
int cgd_op_secondary_pack(cgd_ctx* ctx, const float* x, const float* t, const float* embed_weight, float* out, int B, int H, int W, void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  return launch_pack(ctx, x, t, embed_weight, out, B, H, W, SS(stream));
}
int cgd_op_bilinear_up2x(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, int B, int Hi, int Wi, int C, int adjoint, void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  // forward: in = the (Hi, Wi) map; adjoint: in = the gradient of the (2 Hi, 2 Wi) map, out = the gradient of the (Hi, Wi) map
  if (adjoint) return launch_up(ctx, true, out, ldo, const_cast<float*>(in), ldi, B, Hi, Wi, C, SS(stream));
  return launch_up(ctx, false, in, ldi, out, ldo, B, Hi, Wi, C, SS(stream));
}
}  // extern "C"
