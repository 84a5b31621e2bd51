// Stride-2 3x3 convolution (padding 1) and its backward to the input, as implicit GEMMs on MFMA: the `Downsample` module of the classic
// UNet architecture (improved-diffusion / guided-diffusion defaults: conv_resample = True, resblock_updown = False).
//
//   forward   y[b,oy,ox,:]  = bias + sum_{ky,kx} W[:,:,ky,kx] x[b,2oy+ky-1,2ox+kx-1,:]        M = B Ho Wo, N = Cout, K = 9 Cin
//   backward  dx[b,iy,ix,:] = (add) + sum over the taps that reach (iy, ix) of W[:,:,ky,kx]^T dy[b,oy,ox,:]
//
// The backward is a GATHER, one implicit GEMM per pixel parity of the input: per axis an even index i receives tap k = 1 from o = i / 2, an odd
// index k = 0 from o = (i + 1) / 2 (dropped at o = Ho) and k = 2 from o = (i - 1) / 2.  The four parity classes (py, px) therefore contract over
// 1, 2, 2 and 4 taps of Cout channels: 9 Cout Cin products per output pixel of the FORWARD in total, the forward's cost, no atomics, one fixed
// summation order.  The four classes run in ONE launch: the class is taken from the workgroup index, spread so that every XCD gets all four
// (a class-major grid would hand the 4-tap class to two XCDs and finish at the pace of those).
//
// Activations NHWC fp32 with a row stride; weights as cgd_pack_conv3x3 leaves them (forward [Co][(ky*3+kx)*Ci + ci], rotated / transposed
// [Ci][((2-ky)*3+(2-kx))*Co + co]): the kernel addresses a tap's K-contiguous run of either directly, no further copy.  Tiles are staged
// global -> registers -> (bf16 hi / lo split) -> LDS as in igemm_kernel (gemm.hip): one barrier per 32-deep K tile, LDS double buffer, the three
// precision modes of the context.  Loads are raw buffer loads: padding pixels, rows beyond M and weight rows beyond N carry the offset CGD_OOB,
// read zeros and touch no memory, so no value select follows them.  Byte offsets are 32-bit: an operand of 2^31 bytes or more is refused.
// Small maps split K over gridDim.y into the context's workspace; the slices are summed (with bias and `add`) by the reduce launch of
// cgd_flush_pending, in slice order: still one fixed summation order.
#include "common.h"
#include "kernels.h"
#include "mfma_stage.h"

namespace {

constexpr int SBK = 32;
constexpr int SPF = 36;  // fp32 LDS pitch (floats)
constexpr int SPH = 40;  // bf16 LDS pitch (elements)

struct SconvParams {
  int M, N, Kc;        // rows (B Ho Wo; per parity class in the backward), output columns, channels per tap of the contraction
  int Hs, Ws;          // map the rows gather from: forward (H, W) of x, backward (Ho, Wo) of dy
  int Ho, Wo;          // row decode: m = (b Ho + r) Wo + c
  int lda, ldb, ldc, ldr;
  unsigned a_bytes, b_bytes;
  int ntm, ntn;        // tiles along M (per class) and N
  int splitk;          // slices of K (gridDim.y); > 1: every slice writes its partial sums to ws[slice * ws_stride + out row * N + col]
  long ws_stride;      // = output rows * N
};

template <int MODE, int BM, int BN>
struct SSmem;
template <int BM, int BN>
struct SSmem<0, BM, BN> {
  float a[2][BM][SPF];
  float b[2][BN][SPF];
};
template <int BM, int BN>
struct SSmem<1, BM, BN> {
  __bf16 ah[2][BM][SPH], al[2][BM][SPH];
  __bf16 bh[2][BN][SPH], bl[2][BN][SPH];
};
template <int BM, int BN>
struct SSmem<2, BM, BN> {
  __bf16 ah[2][BM][SPH];
  __bf16 bh[2][BN][SPH];
};

// workgroup = (BM / WM) x (BN / 32) wavefronts, each WM x 32 outputs
template <int MODE, int DGRAD, int BM, int BN, int WM>
__global__ __launch_bounds__((BM / WM) * (BN / 32) * 64) void sconv_kernel(const float* __restrict__ Ag, const float* __restrict__ Bg, float* Cg,
                                                                          const float* __restrict__ biasg, const float* Rg, float* __restrict__ wsg,
                                                                          const SconvParams p) {
  __shared__ __attribute__((aligned(16))) SSmem<MODE, BM, BN> sm;
  constexpr int NWN = BN / 32, NT = (BM / WM) * NWN * 64;
  constexpr int MB = WM / 32;
  constexpr int RPP = NT / 8, RA = BM / RPP, RB = BN / RPP;
  static_assert(BM % RPP == 0 && BN % RPP == 0, "tile rows must be a multiple of the staging pass");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / NWN, wn = wave % NWN;
  const int l31 = lane & 31, hh = lane >> 5;

  // ---- tile (and, in the backward, parity class) of this workgroup ------------------------------------------------------------------
  int tile, py = 0, px = 0;
  if constexpr (DGRAD) {
    // blockIdx = (idx << 3) | xcd: idx & 3 = class (3 - class: the 4-tap class first), tile = (idx >> 2) * 8 + xcd
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    const int cls = 3 - (idx & 3);
    py = cls >> 1;
    px = cls & 1;
    tile = (idx >> 2) * 8 + xcd;
    if (tile >= p.ntm * p.ntn) return;
  } else {
    // XCD-contiguous remap (bijective for any grid size), as igemm_kernel
    const int nt = gridDim.x, q = nt >> 3, r = nt & 7, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
    tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int m0 = (tile / p.ntn) * BM, n0 = (tile % p.ntn) * BN;
  const int ny = DGRAD ? 1 + py : 3, nx = DGRAD ? 1 + px : 3;
  const int nkt = ny * nx * (p.Kc / SBK);

  // ---- per-thread staging rows ------------------------------------------------------------------------------------------------------------
  const int c4 = tid & 7, r0 = tid >> 3;
  int a_r[RA], a_c[RA], a_pix[RA];  // row / column of the row's pixel on the (Ho, Wo) grid, first pixel of its sample in the gathered map
  bool a_ok[RA];
#pragma unroll
  for (int j = 0; j < RA; ++j) {
    const int m = m0 + r0 + RPP * j;
    a_ok[j] = m < p.M;
    const int hw = p.Ho * p.Wo;
    const int b = m / hw, rem = m - b * hw;
    a_r[j] = rem / p.Wo;
    a_c[j] = rem - a_r[j] * p.Wo;
    a_pix[j] = b * p.Hs * p.Ws;
  }
  int b_off[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int n = n0 + r0 + RPP * j;
    b_off[j] = n < p.N ? n * p.ldb * 4 : CGD_OOB;
  }

  cgd_f32x4 ra[RA], rb[RB];

#define SC_GLOAD(KT)                                                                                                   \
  {                                                                                                                    \
    const int kbase = (KT) * SBK;                                                                                      \
    const int tap = kbase / p.Kc, kin = kbase - tap * p.Kc + c4 * 4;                                                   \
    const int ty = tap / nx, tx = tap - ty * nx;                                                                       \
    int ky, kx, dy, dx;                                                                                                \
    if constexpr (DGRAD) {                                                                                             \
      ky = py ? 2 * ty : 1;                                                                                            \
      kx = px ? 2 * tx : 1;                                                                                            \
      dy = py && !ty ? 1 : 0;                                                                                          \
      dx = px && !tx ? 1 : 0;                                                                                          \
    } else {                                                                                                           \
      ky = ty;                                                                                                         \
      kx = tx;                                                                                                         \
      dy = ky - 1;                                                                                                     \
      dx = kx - 1;                                                                                                     \
    }                                                                                                                  \
    const int wcol = ((DGRAD ? (2 - ky) * 3 + (2 - kx) : ky * 3 + kx) * p.Kc + kin) * 4;                               \
    _Pragma("unroll") for (int j = 0; j < RA; ++j) {                                                                   \
      const int yy = DGRAD ? a_r[j] + dy : 2 * a_r[j] + dy, xx = DGRAD ? a_c[j] + dx : 2 * a_c[j] + dx;                \
      const bool ok = a_ok[j] && (unsigned)yy < (unsigned)p.Hs && (unsigned)xx < (unsigned)p.Ws;                       \
      const int off = ok ? ((a_pix[j] + yy * p.Ws + xx) * p.lda + kin) * 4 : CGD_OOB;                                  \
      ra[j] = __builtin_bit_cast(cgd_f32x4, cgd_buf_load16(Ag, p.a_bytes, off, 0));                                    \
    }                                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < RB; ++j) {                                                                   \
      const int off = b_off[j] < 0 ? CGD_OOB : b_off[j] + wcol;                                                        \
      rb[j] = __builtin_bit_cast(cgd_f32x4, cgd_buf_load16(Bg, p.b_bytes, off, 0));                                    \
    }                                                                                                                  \
  }

#define SC_SSTORE(BUF)                                                        \
  {                                                                           \
    _Pragma("unroll") for (int j = 0; j < RA; ++j) {                          \
      const int row = r0 + RPP * j;                                           \
      if constexpr (MODE == 0) {                                              \
        *(cgd_f32x4*)&sm.a[BUF][row][c4 * 4] = ra[j];                         \
      } else if constexpr (MODE == 1) {                                       \
        cgd_bf16x4 hi, lo;                                                    \
        cgd_split_quad(ra[j], hi, lo);                                        \
        *(cgd_bf16x4*)&sm.ah[BUF][row][c4 * 4] = hi;                          \
        *(cgd_bf16x4*)&sm.al[BUF][row][c4 * 4] = lo;                          \
      } else {                                                                \
        *(cgd_bf16x4*)&sm.ah[BUF][row][c4 * 4] = cgd_to_bf16x4(ra[j]);        \
      }                                                                       \
    }                                                                         \
    _Pragma("unroll") for (int j = 0; j < RB; ++j) {                          \
      const int row = r0 + RPP * j;                                           \
      if constexpr (MODE == 0) {                                              \
        *(cgd_f32x4*)&sm.b[BUF][row][c4 * 4] = rb[j];                         \
      } else if constexpr (MODE == 1) {                                       \
        cgd_bf16x4 hi, lo;                                                    \
        cgd_split_quad(rb[j], hi, lo);                                        \
        *(cgd_bf16x4*)&sm.bh[BUF][row][c4 * 4] = hi;                          \
        *(cgd_bf16x4*)&sm.bl[BUF][row][c4 * 4] = lo;                          \
      } else {                                                                \
        *(cgd_bf16x4*)&sm.bh[BUF][row][c4 * 4] = cgd_to_bf16x4(rb[j]);        \
      }                                                                       \
    }                                                                         \
  }

  cgd_f32x16 acc[MB];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  // fragment maps as igemm_kernel: fp32 lane l holds A[l & 31][k = l >> 5] per product, bf16 lane l holds A[l & 31][8 (l >> 5) .. + 7]
#define SC_COMPUTE(BUF)                                                                                         \
  {                                                                                                             \
    if constexpr (MODE == 0) {                                                                                  \
      cgd_f32x4 fa[MB][4], fb[4];                                                                               \
      _Pragma("unroll") for (int i = 0; i < MB; ++i) _Pragma("unroll") for (int q = 0; q < 4; ++q)              \
          fa[i][q] = *(const cgd_f32x4*)&sm.a[BUF][wm * WM + i * 32 + l31][hh * 16 + q * 4];                    \
      _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                             \
          fb[q] = *(const cgd_f32x4*)&sm.b[BUF][wn * 32 + l31][hh * 16 + q * 4];                                \
      _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
        _Pragma("unroll") for (int i = 0; i < MB; ++i) {                                                        \
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][q].x, fb[q].x, acc[i], 0, 0, 0);                  \
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][q].y, fb[q].y, acc[i], 0, 0, 0);                  \
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][q].z, fb[q].z, acc[i], 0, 0, 0);                  \
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][q].w, fb[q].w, acc[i], 0, 0, 0);                  \
        }                                                                                                       \
      }                                                                                                         \
    } else {                                                                                                    \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                                                        \
        cgd_bf16x8 ah[MB], al[MB], bh, bl;                                                                      \
        _Pragma("unroll") for (int i = 0; i < MB; ++i) {                                                        \
          ah[i] = *(const cgd_bf16x8*)&sm.ah[BUF][wm * WM + i * 32 + l31][ks * 16 + hh * 8];                    \
          if constexpr (MODE == 1) al[i] = *(const cgd_bf16x8*)&sm.al[BUF][wm * WM + i * 32 + l31][ks * 16 + hh * 8]; \
        }                                                                                                       \
        bh = *(const cgd_bf16x8*)&sm.bh[BUF][wn * 32 + l31][ks * 16 + hh * 8];                                  \
        if constexpr (MODE == 1) bl = *(const cgd_bf16x8*)&sm.bl[BUF][wn * 32 + l31][ks * 16 + hh * 8];         \
        _Pragma("unroll") for (int i = 0; i < MB; ++i) {                                                        \
          if constexpr (MODE == 1) {                                                                            \
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh, acc[i], 0, 0, 0);                       \
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl, acc[i], 0, 0, 0);                       \
          }                                                                                                     \
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh, acc[i], 0, 0, 0);                         \
        }                                                                                                       \
      }                                                                                                         \
    }                                                                                                           \
  }

  // this workgroup's K tiles (split-K: slice blockIdx.y of p.splitk; a slice beyond the end of a short parity class contributes zeros)
  const int per = (nkt + p.splitk - 1) / p.splitk;
  const int kt0 = blockIdx.y * per, kt1 = min(nkt, kt0 + per);
  if (kt0 < kt1) {
    SC_GLOAD(kt0);
    SC_SSTORE(0);
  }
  __syncthreads();
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;
    if (more) SC_GLOAD(kt + 1);
    SC_COMPUTE(buf);
    if (more) SC_SSTORE(buf ^ 1);
    __syncthreads();
  }
#undef SC_GLOAD
#undef SC_SSTORE
#undef SC_COMPUTE

  // ---- epilogue: C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) ----------------------------------
  const int col = n0 + wn * 32 + l31;
  const bool col_ok = col < p.N;
  float bv = 0.f;
  if (biasg) bv = biasg[col_ok ? col : 0];
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    long orow[16];
    bool ok[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hh;
      ok[r] = col_ok && m < p.M;
      if constexpr (DGRAD) {
        // row m of class (py, px) is input pixel (b, 2 r + py, 2 c + px) of the (2 Ho, 2 Wo) map
        const int hw = p.Ho * p.Wo;
        const int b = m / hw, rem = m - b * hw;
        const int rr = rem / p.Wo, cc = rem - rr * p.Wo;
        orow[r] = ((long)b * 2 * p.Ho + 2 * rr + py) * (2 * p.Wo) + 2 * cc + px;
      } else {
        orow[r] = m;
      }
    }
    if (p.splitk > 1) {  // partial sums only: bias and `add` join in the reduction
      float* __restrict__ ws = wsg + (long)blockIdx.y * p.ws_stride;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (ok[r]) ws[orow[r] * p.N + col] = acc[i][r];
      continue;
    }
    // the `add` values of the whole block first (clamped addresses), then one wait
    float rv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) rv[r] = 0.f;
    if (Rg) {
#pragma unroll
      for (int r = 0; r < 16; ++r) rv[r] = Rg[ok[r] ? orow[r] * p.ldr + col : 0L];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (ok[r]) Cg[orow[r] * p.ldc + col] = acc[i][r] + bv + rv[r];
  }
}

// The tile and split-K choice of one launch: pure host logic, shared by the launcher below and by cgd_op_plan_conv_s2 (CPU tests).
// M: rows (per parity class in the backward), N: output columns, Kc: channels per tap of the contraction.
struct SconvPlan {
  int bm, bn, ntm, ntn, splitk;
  long grid;  // workgroups along gridDim.x
};
SconvPlan sconv_select(bool dgrad, int M, int N, int Kc, int num_cu, bool have_ws, size_t ws_bytes) {
  SconvPlan pl;
  // 128 x 64 tiles (four wavefronts of 64 x 32) where they give every CU a workgroup; 64 x 32 (two wavefronts of 32 x 32) below that
  const long big = (long)cdiv(M, 128) * cdiv(N, 64) * (dgrad ? 4 : 1);
  const bool small = big < num_cu;
  pl.bm = small ? 64 : 128;
  pl.bn = small ? 32 : 64;
  pl.ntm = cdiv(M, pl.bm);
  pl.ntn = cdiv(N, pl.bn);
  const long tiles = (long)pl.ntm * pl.ntn;
  pl.grid = dgrad ? (long)cdiv(tiles, 8) * 32 : tiles;
  // Split-K for the small maps (a 16 x 16 x 512 input is 16 tiles of 144 K tiles each): about two workgroups per CU, at least two K tiles per slice
  // of the shortest contraction (the backward's 1-tap class), at most 16 slices, through the context's workspace and its deferred-slice record
  // exactly as cgd_launch_gemm does it: the slices are summed, with bias and `add`, by the reduce launch of cgd_flush_pending
  const long out_rows = dgrad ? 4L * M : M;
  const long work = tiles * (dgrad ? 4 : 1);
  const int short_nkt = (dgrad ? 1 : 9) * (Kc / SBK);
  pl.splitk = 1;
  if (work < num_cu && have_ws) {
    long want = std::min<long>(std::min<long>(cdiv(2L * num_cu, work), short_nkt / 2), 16);
    while (want > 1 && (size_t)want * out_rows * N * sizeof(float) > ws_bytes) --want;
    if (want >= 2) pl.splitk = (int)want;
  }
  return pl;
}

template <int MODE, int DGRAD>
int sconv_launch_mode(cgd_ctx* ctx, const float* A, const float* Bw, float* C, const float* bias, const float* R, SconvParams p, hipStream_t s) {
  const SconvPlan pl = sconv_select(DGRAD, p.M, p.N, p.Kc, ctx->num_cu, ctx->ws != nullptr, ctx->ws_bytes);
  const bool small = pl.bm == 64;
  p.ntm = pl.ntm;
  p.ntn = pl.ntn;
  p.splitk = pl.splitk;
  const long grid = pl.grid;
  if (grid > 0x7fffffffL) CGD_FAIL(ctx, "conv3x3_s2: too many tiles for one launch");
  const long out_rows = DGRAD ? 4L * p.M : p.M;
  p.ws_stride = out_rows * p.N;
  const dim3 g((unsigned)grid, (unsigned)p.splitk);
  ProfRec pr;  // with the MFMA GEMM kernels and their split-K reduce (kind 0)
  CGD_TRY(cgd_prof_begin(ctx, &pr, CGD_PROF_GEMM, 2.0 * p.M * p.N * 9.0 * p.Kc, s));
  if (small)
    CGD_LAUNCH((sconv_kernel<MODE, DGRAD, 64, 32, 32>), g, dim3(128), 0, s, A, Bw, C, bias, R, ctx->ws, p);
  else
    CGD_LAUNCH((sconv_kernel<MODE, DGRAD, 128, 64, 64>), g, dim3(256), 0, s, A, Bw, C, bias, R, ctx->ws, p);
  CGD_HIP(ctx, hipGetLastError());
  if (p.splitk > 1) {
    PendingReduce& q = ctx->pending;
    q.valid = true;
    q.src.ws = ctx->ws; q.src.bias = bias; q.src.R = R; q.src.stride = p.ws_stride; q.src.n = p.splitk; q.src.N = p.N;
    q.src.ldr = p.ldr; q.src.alpha = 1.f;
    q.C = C; q.ldc = p.ldc; q.M = (int)out_rows; q.stream = s;
    CGD_TRY(cgd_flush_pending(ctx, s));  // not deferred: the readers of a Downsample's output and gradient are convs and element-wise kernels too
  }
  CGD_TRY(cgd_prof_stamp(ctx, &pr, s));
  cgd_prof_push(ctx, &pr);
  return 0;
}

template <int DGRAD>
int sconv_launch(cgd_ctx* ctx, const float* A, const float* Bw, float* C, const float* bias, const float* R, const SconvParams& p, hipStream_t s) {
  switch (ctx->precision) {
    case CGD_PREC_F32: return sconv_launch_mode<0, DGRAD>(ctx, A, Bw, C, bias, R, p, s);
    case CGD_PREC_BF16X3: return sconv_launch_mode<1, DGRAD>(ctx, A, Bw, C, bias, R, p, s);
    default: return sconv_launch_mode<2, DGRAD>(ctx, A, Bw, C, bias, R, p, s);
  }
}

// bytes of `rows` rows of `cols` floats at row stride ld
long extent_bytes(long rows, int ld, int cols) { return ((rows - 1) * ld + cols) * 4; }

}  // namespace

// The one predicate of what the two launchers run (host only).  ld_in: row stride of the gathered operand (x / dy), ld_out: of the written one
// (y / dx), ldadd: of the backward's `add` operand (0 = none).  B, H, W: the INPUT's (the backward's dx).  Returns nullptr when the problem is
// accepted, else the reason.
const char* cgd_sconv_refusal(int dgrad, int ld_in, int ld_out, int ldadd, int B, int H, int W, int Cin, int Cout) {
  if (B < 1 || H < 2 || W < 2) return "conv3x3_s2: B, H and W must be positive";
  if ((H | W) & 1) return "conv3x3_s2: H and W must be even (Ho = H / 2, Wo = W / 2)";
  if (Cin <= 0 || Cout <= 0 || (Cin & 31) || (Cout & 31)) return "conv3x3_s2: Cin and Cout must be positive multiples of 32";
  const int c_in = dgrad ? Cout : Cin, c_out = dgrad ? Cin : Cout;
  if (ld_in < c_in || ld_out < c_out || (ldadd && ldadd < Cin)) return "conv3x3_s2: a row stride is smaller than its channel count";
  if ((ld_in | ld_out | ldadd) & 3) return "conv3x3_s2: row strides must be multiples of 4";
  const long full = (long)B * H * W, half = full / 4;
  const long lim = 1L << 31;  // 32-bit byte offsets of the buffer loads; CGD_OOB = 2^31 marks a lane out of range
  if (extent_bytes(dgrad ? half : full, ld_in, c_in) >= lim || extent_bytes(dgrad ? full : half, ld_out, c_out) >= lim ||
      (ldadd && extent_bytes(full, ldadd, Cin) >= lim) || (long)Cin * Cout * 9 * 4 >= lim)
    return "conv3x3_s2: an operand of 2^31 bytes or more is beyond the kernel's 32-bit byte offsets";
  return nullptr;
}

// wf: the forward copy of cgd_pack_conv3x3 ([Cout][9 Cin])
int cgd_launch_sconv_fwd(cgd_ctx* ctx, const float* x, int ldx, const float* wf, const float* bias, float* y, int ldy, int B, int H, int W, int Cin,
                         int Cout, hipStream_t s) {
  if (const char* why = cgd_sconv_refusal(0, ldx, ldy, 0, B, H, W, Cin, Cout)) CGD_FAIL(ctx, why);
  if (!x || !wf || !y) CGD_FAIL(ctx, "conv3x3_s2: x, the packed weights and y are required");
  if (((uintptr_t)x | (uintptr_t)wf | (uintptr_t)y) & 15) CGD_FAIL(ctx, "conv3x3_s2: x, the packed weights and y must be 16-byte aligned");
  CGD_TRY(cgd_flush_pending(ctx, s));  // reads an activation without summing split-K slices itself
  SconvParams p = {};
  p.Ho = H / 2; p.Wo = W / 2; p.Hs = H; p.Ws = W;
  p.M = B * p.Ho * p.Wo; p.N = Cout; p.Kc = Cin;
  p.lda = ldx; p.ldb = 9 * Cin; p.ldc = ldy;
  p.a_bytes = (unsigned)extent_bytes((long)B * H * W, ldx, Cin);
  p.b_bytes = (unsigned)((long)Cout * 9 * Cin * 4);
  cgd_chanstats_invalidate(ctx, y, p.M, ldy, Cout);
  return sconv_launch<0>(ctx, x, wf, y, bias, nullptr, p, s);
}

// wd: the rotated / transposed copy of cgd_pack_conv3x3 ([Cin][9 Cout]); B, H, W: dx's
int cgd_launch_sconv_dgrad(cgd_ctx* ctx, const float* dy, int lddy, const float* wd, float* dx, int lddx, const float* add, int ldadd, int B, int H,
                           int W, int Cin, int Cout, hipStream_t s) {
  if (const char* why = cgd_sconv_refusal(1, lddy, lddx, add ? ldadd : 0, B, H, W, Cin, Cout)) CGD_FAIL(ctx, why);
  if (add && !ldadd) CGD_FAIL(ctx, "conv3x3_s2: the add operand needs its row stride");
  if (!dy || !wd || !dx) CGD_FAIL(ctx, "conv3x3_s2: dy, the packed weights and dx are required");
  if (((uintptr_t)dy | (uintptr_t)wd | (uintptr_t)dx | (uintptr_t)add) & 15) CGD_FAIL(ctx, "conv3x3_s2: dy, the packed weights, dx and add must be 16-byte aligned");
  CGD_TRY(cgd_flush_pending(ctx, s));
  SconvParams p = {};
  p.Ho = H / 2; p.Wo = W / 2; p.Hs = p.Ho; p.Ws = p.Wo;
  p.M = B * p.Ho * p.Wo; p.N = Cin; p.Kc = Cout;
  p.lda = lddy; p.ldb = 9 * Cout; p.ldc = lddx; p.ldr = ldadd;
  p.a_bytes = (unsigned)extent_bytes((long)p.M, lddy, Cout);
  p.b_bytes = (unsigned)((long)Cin * 9 * Cout * 4);
  cgd_chanstats_invalidate(ctx, dx, (long)B * H * W, lddx, Cin);
  return sconv_launch<1>(ctx, dy, wd, dx, nullptr, add, p, s);
}

// Host-only view of sconv_select (no GPU, no context; the context's fixed 256 MiB workspace): out4 = {tile rows, tile columns, split-K slices,
// workgroups of the main launch} of the forward (dgrad = 0) or the backward (dgrad = 1) of a dense (B, H, W, Cin) -> Cout problem; B, H, W: the
// INPUT's.  -2 where cgd_op_conv3x3_s2_accepts refuses the problem.  Test support, as cgd_op_attn_plan.
extern "C" int cgd_op_plan_conv_s2(int dgrad, int B, int H, int W, int Cin, int Cout, int num_cu, int* out4) {
  if (!out4) return -3;
  if (cgd_sconv_refusal(dgrad, dgrad ? Cout : Cin, dgrad ? Cin : Cout, 0, B, H, W, Cin, Cout)) return -2;
  const int M = B * (H / 2) * (W / 2);
  const SconvPlan pl = sconv_select(dgrad != 0, M, dgrad ? Cin : Cout, dgrad ? Cout : Cin, num_cu > 0 ? num_cu : cgd_ctx().num_cu, true, (size_t)256 << 20);
  out4[0] = pl.bm; out4[1] = pl.bn; out4[2] = pl.splitk; out4[3] = (int)(pl.grid * pl.splitk);
  return 0;
}
