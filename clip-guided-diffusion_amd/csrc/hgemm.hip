// Dense weight GEMM  C[M][N] = alpha * A[M][K] W[N][K]^T (+ bias[n]) (+ R[m][n])  for gfx950, bf16x3 / bf16 MFMA.
// Used for every linear layer / 1x1 convolution whose B operand is a persistent weight (ViT in_proj / out_proj / MLP, UNet
// qkv / proj_out / skip 1x1 convs): the same design as hconv2 (hconv.hip) without the halo:
//   * W is packed once (cgd_frag_cache, keyed by the weight pointer) in MFMA fragment order, bf16 hi/lo planes,
//     [N/32][K/32][kstep][plane][lane][8]: wavefronts load their B fragments straight from global/L2 into registers through
//     a 4-deep ring (two k-steps ahead); no LDS, no conversion, no barrier for the weights;
//   * A: a 128-row x 64-column chunk is converted to bf16 hi/lo once and double-buffered in LDS (73,728 B -> two workgroups
//     per CU); chunk c+2 is fetched to registers while chunk c is being multiplied, converted during k-steps 1..2 of chunk
//     c+1's predecessor, and the single barrier per chunk sits BEFORE the last k-step, so the A fragments of the next chunk's
//     first k-step are already in flight when the chunk turns over: the MFMA stream never drains at a chunk boundary;
//   * every MFMA is followed by one LDS / global load and a few conversion VALU ops (sched_group_barrier pattern);
//   * operands are swapped (D = W_frag x A_frag^T) so a lane owns 4 consecutive output columns: 16-byte epilogue accesses.
// 4 wavefronts (2 x 2), 64 x 64 outputs each; split-K over 64-column chunks through the shared workspace + reduce kernel.
#include "common.h"
#include "mfma_stage.h"

#include <algorithm>

namespace {

constexpr int GM = 128, GN = 128, GK = 64, GPH = GK + 8;  // tile, chunk width, LDS row pitch (bf16 elements)
constexpr int GPLANE = GM * GPH;

// per-wavefront timeline for benchmarks/ubench/hgemm_stamps.hip (which includes this file with CGD_HGEMM_STAMPS defined); the library build
// never defines it: H_STAMP expands to nothing there
#ifdef CGD_HGEMM_STAMPS
__device__ unsigned long long* g_hstamps;  // [workgroup (x + gridDim.x * z)][wavefront][32]: 0 entry, 1 first chunk staged, 2 + c chunk c done (level 2), 29 loop done, 30 stores issued, 31 HW id
// (the first four wavefronts stamp: K-group 1 of the KG = 2 instantiations has no records)
#define H_STAMP_AT(I, WHAT)                                                                                 \
  do {                                                                                                      \
    if (threadIdx.x < 256) WHAT(g_hstamps, (long)blockIdx.z * gridDim.x + blockIdx.x, threadIdx.x >> 6, I); \
  } while (0)
#define H_STAMP(I) H_STAMP_AT(I, CGD_STAMP)
#if CGD_HGEMM_STAMPS >= 2  // a store per chunk slows the 0.75 us chunks by ~30 %: level 1 stamps only around the loop
#define H_STAMP_CHUNK(I) H_STAMP(I)
#else
#define H_STAMP_CHUNK(I) CGD_NO_STAMP
#endif
#define H_STAMP_END()                \
  do {                               \
    H_STAMP(30);                     \
    H_STAMP_AT(31, CGD_STAMP_HW_ID); \
  } while (0)
#else
#define H_STAMP(I) CGD_NO_STAMP
#define H_STAMP_CHUNK(I) CGD_NO_STAMP
#define H_STAMP_END() CGD_NO_STAMP
#endif

struct HGemmParams {
  int lda, ldc, ldr;
  int M, N, K, splitk;
  float alpha;
  float* act_out;       // hgemm2 epilogue: C2 = act(C) (GemmParams::act_out)
  const float* act_in;  // hgemm2 epilogue: C = (...) * act'(U)
  int ld_act, act;
  int lep;         // hgemm2, bf16x3: 1 = output block through LDS, whole-line stores / operand reads (ctx->hgemm_epi)
  int skip_group;  // hgemm2, one slice: drop the first row of every group of this many rows, write the rest compactly (GemmParams)
  int nt;      // kgemm_kernel: weight-fragment loads with the non-temporal policy
  int nt_out;  // unread (non-temporal output stores measured neutral, profiles/r6_ab_nt_more.txt); kept so later fields do not move
  int nmajor;  // tile order within the XCD-contiguous runs: 0 = M-tile major (an XCD owns row panels and streams all weights),
               // 1 = N-tile major (an XCD owns weight column panels, read from HBM once and kept in its 4 MB L2; the small
               // activation matrix is what every XCD re-reads): chosen when the weights are the larger operand (N >= M)
  // hgemm2 GNB instantiation (GemmParams::gnf_*): the epilogue adds the backward of a GroupNorm + SiLU over the output's own pixels
  const float* gnf_x;      // the norm's forward input, row stride gnf_ldx
  const float* gnf_dz;     // its upstream gradient, row stride gnf_lddz
  const float* gnf_add;    // optional further addend, row stride gnf_ldadd
  const float* gnf_coef;   // [sample][N][4] {a, b, gcoef, mean}
  const float* gnf_bcoef;  // [sample][N][4] {rstd gcoef, A2, A3, 0}
  int gnf_ldx, gnf_lddz, gnf_ldadd;
  int gnf_hw;              // rows per sample (a multiple of the 128-row tile, or all M rows)
};

template <int MODE>
__global__ __launch_bounds__(256) void hgemm_kernel(const float* __restrict__ Ag, const uint4* __restrict__ Bg, float* Cg,
                                                    const float* __restrict__ biasg, const float* Rg, float* __restrict__ wsg,
                                                    const HGemmParams p) {
  constexpr int NPL = MODE == 1 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) __bf16 lds[2 * NPL * GPLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, hh = lane >> 5;

  const int ntn = (p.N + GN - 1) / GN;
  int bid = blockIdx.x;
  {
    const int nt = gridDim.x, q = nt >> 3, r = nt & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int m0 = (bid / ntn) * GM, n0 = (bid % ntn) * GN;

  // staging slots: row = (tid >> 4) + 16 j, 16 float4 per 64-column row
  const int c4 = tid & 15, r0 = tid >> 4;
  long aoff[8];
  unsigned amask = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = m0 + r0 + 16 * j;
    const bool ok = r < p.M;
    aoff[j] = (long)(ok ? r : p.M - 1) * p.lda + c4 * 4;
    amask |= ok ? (1u << j) : 0u;
  }
  int fro[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) fro[i] = (wm * 64 + i * 32 + l31) * GPH + hh * 8;

  const int nchunk = p.K / GK;
  int c0 = 0, c1 = nchunk;
  if (p.splitk > 1) {
    const int per = (nchunk + p.splitk - 1) / p.splitk;
    c0 = blockIdx.z * per;
    c1 = min(nchunk, c0 + per);
  }
  // packed weights: block (nb, k32, ks, plane) = 64 uint4; the k-steps of one 32-row block are contiguous: k-step kq at kq * 128
  const int nb0 = (n0 + wn * 64) >> 5, nbN = p.N >> 5;
  const long bstride_nb = (long)(p.K >> 5) * 4 * 64;
  const int nbc = nb0 < nbN ? nb0 : nbN - 1;
  const long bj1 = (nb0 + 1 < nbN) ? bstride_nb : 0;
  const uint4* __restrict__ Bw0 = Bg + (long)nbc * bstride_nb + lane;
  const int kq_last = c1 * 4 - 1;

  cgd_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  if (c0 >= c1) goto epilogue;  // empty split-K slice: contributes zeros

  {
    cgd_f32x4 pr[8];
    const cgd_f32x4 z4 = cgd_f32x4{0.f, 0.f, 0.f, 0.f};
#define G_PATCH_LOAD(CH)                                                                     \
  {                                                                                          \
    const float* __restrict__ Ac = Ag + (long)((CH) < c1 ? (CH) : c1 - 1) * GK;              \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) pr[j] = *(const cgd_f32x4*)(Ac + aoff[j]); \
  }
#define G_PATCH_STORE(DSTB, J0, J1)                                                                                      \
  {                                                                                                                      \
    _Pragma("unroll") for (int j = J0; j < J1; ++j) {                                                                    \
      const int row = r0 + 16 * j;                                                                                       \
      const cgd_f32x4 v = (amask >> j) & 1u ? pr[j] : z4;                                                                \
      const cgd_bf16x4 hi = cgd_to_bf16x4(v);                                                                            \
      *(cgd_bf16x4*)&(DSTB)[row * GPH + c4 * 4] = hi;                                                                    \
      if constexpr (MODE == 1) *(cgd_bf16x4*)&(DSTB)[GPLANE + row * GPH + c4 * 4] = cgd_to_bf16x4(cgd_residual4(v, hi)); \
    }                                                                                                                    \
  }
#define G_A_LOAD(DST, SRCB, Q)                                                                      \
  {                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                 \
      if constexpr (MODE == 1) DST[i][1] = *(const cgd_bf16x8*)&(SRCB)[GPLANE + fro[i] + (Q) * 16]; \
      DST[i][0] = *(const cgd_bf16x8*)&(SRCB)[fro[i] + (Q) * 16];                                   \
    }                                                                                               \
  }
#define G_B_LOAD(DST, KQ)                                                                         \
  {                                                                                               \
    const int kq_ = (KQ) < kq_last ? (KQ) : kq_last;                                              \
    const uint4* q_ = Bw0 + (long)kq_ * 128;                                                      \
    DST[0][0] = q_[0];                                                                            \
    if constexpr (MODE == 1) DST[0][1] = q_[64];                                                  \
    DST[1][0] = q_[bj1];                                                                          \
    if constexpr (MODE == 1) DST[1][1] = q_[bj1 + 64];                                            \
  }
#define G_MFMA12(AQ, BQ)                                                                                                               \
  {                                                                                                                                    \
    if constexpr (MODE == 1) {                                                                                                         \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                                      \
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, BQ[j][0]), AQ[i][1], acc[i][j], 0, 0, 0); \
      _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                                      \
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, BQ[j][1]), AQ[i][0], acc[i][j], 0, 0, 0); \
    }                                                                                                                                  \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                                        \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, BQ[j][0]), AQ[i][0], acc[i][j], 0, 0, 0);   \
  }
  // one MFMA, then one LDS read / one global read / a few conversion VALU ops / one LDS write: the own MFMA queue never drains
#define G_INTERLEAVE()                                                                            \
  {                                                                                               \
    _Pragma("unroll") for (int r = 0; r < 12; ++r) {                                              \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
      if (r % 3 == 0) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                          \
      if (r % 3 == 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                          \
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                                          \
    }                                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                            \
  }

    cgd_bf16x8 af[2][2][NPL];  // [pipeline slot][row block][plane]
    uint4 bq[4][2][NPL];   // [ring slot][column block][plane]
    // prologue: chunk c0 into buffer 0, chunk c0+1 in registers, B fragments of the first two k-steps
    G_PATCH_LOAD(c0);
    G_B_LOAD(bq[0], c0 * 4);
    G_B_LOAD(bq[1], c0 * 4 + 1);
    G_PATCH_STORE(lds, 0, 8);
    G_PATCH_LOAD(c0 + 1);
    __syncthreads();
    G_A_LOAD(af[0], lds, 0);
    for (int c = c0; c < c1; ++c) {
      const __bf16* cur = lds + ((c - c0) & 1) * (NPL * GPLANE);
      __bf16* nxt = lds + (((c - c0) & 1) ^ 1) * (NPL * GPLANE);
      const int kq = c * 4;
      // k-step 0
      G_A_LOAD(af[1], cur, 1);
      G_B_LOAD(bq[2], kq + 2);
      G_MFMA12(af[0], bq[0]);
      G_INTERLEAVE();
      // k-step 1 (+ first half of the next chunk's conversion)
      G_A_LOAD(af[0], cur, 2);
      G_B_LOAD(bq[3], kq + 3);
      G_MFMA12(af[1], bq[1]);
      G_PATCH_STORE(nxt, 0, 4);
      G_INTERLEAVE();
      // k-step 2 (+ second half; then fetch the chunk after next)
      G_A_LOAD(af[1], cur, 3);
      G_B_LOAD(bq[0], kq + 4);
      G_MFMA12(af[0], bq[2]);
      G_PATCH_STORE(nxt, 4, 8);
      G_INTERLEAVE();
      G_PATCH_LOAD(c + 2);
      __syncthreads();  // nxt fully written; every wavefront has fetched its last fragments of cur
      // k-step 3: already reads the next chunk's first fragments
      G_A_LOAD(af[0], nxt, 0);
      G_B_LOAD(bq[1], kq + 5);
      G_MFMA12(af[1], bq[3]);
      G_INTERLEAVE();
    }
#undef G_PATCH_LOAD
#undef G_PATCH_STORE
#undef G_A_LOAD
#undef G_B_LOAD
#undef G_MFMA12
#undef G_INTERLEAVE
  }

epilogue:
  // D = W x A^T in the 32x32 C/D layout: column (lane & 31) = row m of C, accumulator quad g = columns 8g + 4hh .. + 3 of C
  long mrow[2];
  bool mok[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = m0 + wm * 64 + i * 32 + l31;
    mok[i] = r < p.M;
    mrow[i] = r;
  }
  if (p.splitk > 1) {
    float* __restrict__ ws = wsg + (long)blockIdx.z * p.M * p.N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cb0 = n0 + wn * 64 + j * 32;
        if (cb0 < p.N && mok[i]) {
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(cgd_f32x4*)&ws[mrow[i] * p.N + cb0 + 8 * g + 4 * hh] =
                cgd_f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        }
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cb0 = n0 + wn * 64 + j * 32;
      if (cb0 >= p.N || !mok[i]) continue;
      cgd_f32x4 rv[4];
      if (Rg) {
#pragma unroll
        for (int g = 0; g < 4; ++g) rv[g] = *(const cgd_f32x4*)&Rg[mrow[i] * p.ldr + cb0 + 8 * g + 4 * hh];
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = cb0 + 8 * g + 4 * hh;
        cgd_f32x4 o = cgd_f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]} * p.alpha;
        if (biasg) o += cgd_f32x4{biasg[col], biasg[col + 1], biasg[col + 2], biasg[col + 3]};
        if (Rg) o += rv[g];
        *(cgd_f32x4*)&Cg[mrow[i] * p.ldc + col] = o;
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// exact (erf) GELU, activation code 3 of the fused epilogues, and its derivative: same arithmetic as elem.hip act_f / dact_f.  The k-scaled sigmoid of
// codes 1 / 2 cannot express it: hgemm2_kernel's GELU instantiations.
__device__ __forceinline__ cgd_f32x4 hg_gelu4(const cgd_f32x4 u) {
  cgd_f32x4 a;
#pragma unroll
  for (int e = 0; e < 4; ++e) a[e] = 0.5f * u[e] * (1.f + erff(u[e] * 0.70710678f));
  return a;
}
__device__ __forceinline__ cgd_f32x4 hg_dgelu4(const cgd_f32x4 u) {
  cgd_f32x4 d;
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = 0.5f * (1.f + erff(u[e] * 0.70710678f)) + u[e] * 0.3989422804f * __expf(-0.5f * u[e] * u[e]);
  return d;
}

// hgemm2_kernel: the same GEMM with the wave -> sub-tile mapping and the weight-fragment pipeline of hconv2_kernel.
//   * Why: the rocprofv3 trace of round 2 (profiles/r2_trace_step_a.txt) shows the step's kernels running back to back, i.e.
//     the time of the ViT linears (M = 800 token rows, 13-28 us for 1-4 GFLOP) is INSIDE hgemm_kernel: one workgroup per CU,
//     one wavefront per SIMD, and B fragments fetched only two k-steps (~0.3 us) ahead while the weights stream from HBM
//     (the ViT's 350 MB of packed weights do not stay in L2) at >1 us latency: the MFMA pipe waits for the ring.
//   * wavefront sub-tile TM x 32 (TM = 128 or 64 rows): the 4 wavefronts sit side by side along N and share the A chunk in
//     LDS; per k-step a wavefront issues 2 global fragment loads (hi / lo planes of ONE 32-column block) instead of 4, so an
//     8-slot register ring (7 k-steps ~ 1.2 us ahead) costs the 64 VGPRs the 4-slot ring of the 64 x 64 mapping did;
//   * TM = 64 for small M (fewer than one 128-row tile per CU): M = 800 gives 13 x N/128 workgroups instead of 7 x N/128, so
//     the N >= 2304 linears fill the chip without split-K and the others split less; two to three workgroups fit a CU
//     (LDS 36.9 KB, ~170 VGPRs), whose load stalls overlap;
//   * the loop body covers a whole period of ring base, LDS buffer and staging set (two 64-deep chunks = 8 k-steps = one turn of the ring in
//     the shipped configuration), so every ring slot, LDS buffer and register set is a compile-time constant; a shorter tail follows;
//   * A staging, conversion, barrier placement and the epilogue are those of hgemm_kernel.
// hgemm2_kernel fetches both operand streams with buffer loads (round 6; resource = the tensor, per-lane byte offset in a register that never
// changes, the chunk / k-step offset in a scalar).  What it buys: (a) the prefetches that run past the end of a slice — the weight ring is 7 k-steps
// ahead, the activation sets up to 3 chunks — used to re-read the slice's last fragments / last chunk on clamped indices (a 4-chunk slice of a
// split-K ViT linear issued 7 patch loads for 4 useful ones through the L2 path that bounds this class); with a resource of ZERO records they are
// out of range, return zeros and touch no memory — no branch in the scheduled region; (b) no 64-bit per-lane address arithmetic per load.
// The loads are mfma_stage.h's cgd_buf_load16_if: its `neg` < 0 = inside the slice; rows beyond M carry the offset CGD_OOB.

constexpr int h2_gcd(int a, int b) { return b ? h2_gcd(b, a % b) : a; }
constexpr int h2_lcm(int a, int b) { return a / h2_gcd(a, b) * b; }
// RING = weight-fragment ring depth in k-steps (a multiple of 4: slots of a chunk are ring[(4 j) % RING ..]), NSET = staging register sets of
// the activation patch (the patch is fetched NSET chunks ahead).  Defaults = the shipped configuration; benchmarks/ubench/hgemm_stamps.hip
// instantiates others to sweep the pipeline depth against the cold-L2 operand latency.
// KG = 2 (round 4): TWO wavefronts per SIMD.  The round-4 sweep (profiles/r4_hgemm_pipeline_sweep.txt) refuted the latency model: deeper
// rings / staging sets move the loop by < 10 %, but removing the weight loads or the patch path from the loop shortens it ADDITIVELY
// (0.94 -> 0.71 / 0.63 -> 0.46 us per chunk = the MFMA stream alone), and a 64 x 128 tile needs 48 KB of operands per 64-deep chunk =
// 750 cycles of the CU's 64 B/clk vector-memory path against 773 cycles of MFMA: with one wavefront per SIMD an in-order wavefront that is
// stuck issuing a vector-memory instruction into the full queue issues no MFMA either, so the two costs add instead of overlapping.
// The workgroup becomes 8 wavefronts = 2 K-groups x 4 column blocks over a 128-deep chunk: group kg multiplies k-steps 4 kg .. 4 kg + 3
// of every chunk (its own weight fragments, its own accumulators), the 512 threads stage the 64 x 128 patch together, and group 1 hands
// its partial block to group 0 through LDS before the epilogue.  Per wavefront the instruction stream of a chunk is unchanged.
// GELU: the fused activation (act_out / act_in) is the exact GELU, code 3.  A template parameter, not a branch on p.act: erff inlined into the unrolled
// epilogues nearly triples the kernel (8363 -> 22573 instructions at TM = 128), and the instantiations every other launch runs stay as they were.
// GNB (128-row tiles, bf16x3): the LDS epilogue also applies the backward of the GroupNorm + SiLU that read the same pixels (the 1x1 skip dgrad of a
// ResBlock and GN1's backward both end in the block's dx): C = alpha acc (+ bias + R) (+ add) + dz silu'(x a + b) A1 - (x - mean) A2 - A3, the
// arithmetic of gn_bwd_apply_kernel<1> (norm.hip) with this GEMM's block as its `add` operand.  x / dz / add are read and C is written once, as
// whole 128-byte lines with the non-temporal policy: the GEMM's C write, its read-back and the norm's launch go away.
template <int MODE, int TM, int RING = 8, int NSET = (TM == 64 ? 2 : 1), int KG = 1, bool GELU = false, bool GNB = false>
__global__ __launch_bounds__(256 * KG) void hgemm2_kernel(const float* __restrict__ Ag, const uint4* __restrict__ Bg, float* Cg,
                                                     const float* __restrict__ biasg, const float* Rg, float* __restrict__ wsg,
                                                     const HGemmParams p) {
  constexpr int NPL = MODE == 1 ? 2 : 1;
  constexpr int NI = TM / 32;      // 32-row blocks per wavefront
  constexpr int NPS = TM / 16;     // staging slots per thread: rows r0 + 16 j
  constexpr int GKW = GK * KG;     // chunk width of the workgroup (columns of A staged per turn)
  constexpr int GPHW = GKW + 8;    // LDS row pitch (bf16): 144 / 272 bytes, 16 consecutive rows start in 16 different 16-byte bank groups
  constexpr int PLANE = TM * GPHW;
  constexpr int DIST = RING - 1;
  static_assert(RING % 4 == 0 && RING >= 8 && NSET >= 1, "hgemm2: ring depth in whole chunks, at least two");
  static_assert(KG == 1 || (KG == 2 && MODE == 1), "hgemm2: K-groups need the LDS epilogue of the bf16x3 mode");
  static_assert(!GNB || (MODE == 1 && TM == 128 && KG == 1 && !GELU), "hgemm2: the GroupNorm-backward epilogue is the LDS epilogue of the 128-row tile");
  __shared__ __attribute__((aligned(16))) __bf16 lds[2 * NPL * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wn = (tid >> 6) & 3, kg = tid >> 8;
  const int l31 = lane & 31, hh = lane >> 5;
  H_STAMP(0);

  const int ntn = (p.N + GN - 1) / GN;
  int bid = blockIdx.x;
  {
    const int nt = gridDim.x, q = nt >> 3, r = nt & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  const int ntm = (p.M + TM - 1) / TM;
  const int m0 = (p.nmajor ? bid % ntm : bid / ntn) * TM, n0 = (p.nmajor ? bid / ntm : bid % ntn) * GN;

  const int c4 = tid & (16 * KG - 1), r0 = tid / (16 * KG);
  int aoff[NPS];
  unsigned amask = 0;
#pragma unroll
  for (int j = 0; j < NPS; ++j) {
    const int r = m0 + r0 + 16 * j;
    const bool ok = r < p.M;
    aoff[j] = (ok ? r : p.M - 1) * p.lda + c4 * 4;
    amask |= ok ? (1u << j) : 0u;
  }
  int aoffb[NPS];  // byte offsets for the buffer loads; a row beyond M is out of range: zeros without a select
#pragma unroll
  for (int j = 0; j < NPS; ++j) aoffb[j] = (amask >> j) & 1u ? aoff[j] * 4 : CGD_OOB;
  int fro[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) fro[i] = (i * 32 + l31) * GPHW + hh * 8 + kg * GK;

  const int nchunk = p.K / GKW;
  int c0 = 0, c1 = nchunk;
  if (p.splitk > 1) {
    const int per = (nchunk + p.splitk - 1) / p.splitk;
    c0 = blockIdx.z * per;
    c1 = min(nchunk, c0 + per);
  }
  const int nb0 = (n0 >> 5) + wn, nbN = p.N >> 5;
  const long bstride_nb = (long)(p.K >> 5) * 4 * 64;
  // this wavefront's k-steps in its own linear order t = 4 (chunk - c0) + j: k-step (chunk * KG + kg) * 4 + j of the packed weight block
  // Unread, but kept: without it the compiler schedules the chunk loop differently and the kernel is no longer the measured build.
  const uint4* __restrict__ Bw0 = Bg + (long)(nb0 < nbN ? nb0 : nbN - 1) * bstride_nb + lane + (long)(c0 * KG + kg) * 4 * 128;
  (void)Bw0;
  // the wavefront's weight block as a scalar base: column block and K-group are the same for all its lanes
  const int wn_s = __builtin_amdgcn_readfirstlane(wn), kg_s = __builtin_amdgcn_readfirstlane(kg);
  const int nb0_s = (n0 >> 5) + wn_s;
  const uint4* __restrict__ Bwb = Bg + (long)(nb0_s < nbN ? nb0_s : nbN - 1) * bstride_nb + (long)(c0 * KG + kg_s) * 4 * 128;
  const int t_last = (c1 - c0) * 4 - 1;

  cgd_f32x16 acc[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

  if (c0 < c1) {
    constexpr int AHEAD = NSET + 1;  // set (C - c0) % NSET holds chunk C + 1 while chunk C runs and is refilled with chunk C + AHEAD
    cgd_f32x4 prs[NSET][NPS];
#define H2_PATCH_LOAD(PR, CH)                                                                          \
  {                                                                                                    \
    const int in_ = (CH) - c1; /* < 0: inside the slice */                                             \
    const int so_ = (CH) * (GKW * 4);                                                                  \
    _Pragma("unroll") for (int j = 0; j < NPS; ++j)                                                    \
        PR[j] = __builtin_bit_cast(cgd_f32x4, cgd_buf_load16_if(Ag, 0x80000000u, in_, aoffb[j], so_)); \
  }
#define H2_PATCH_STORE(PR, DSTB, J0, J1)                               \
  {                                                                    \
    _Pragma("unroll") for (int j = J0; j < J1; ++j) {                  \
      const int row = r0 + 16 * j;                                     \
      const cgd_f32x4 v = PR[j];                                       \
      if constexpr (MODE == 1) {                                       \
        cgd_bf16x4 hi, lo;                                             \
        cgd_split_quad(v, hi, lo);                                     \
        *(cgd_bf16x4*)&(DSTB)[row * GPHW + c4 * 4] = hi;               \
        *(cgd_bf16x4*)&(DSTB)[PLANE + row * GPHW + c4 * 4] = lo;       \
      } else {                                                         \
        *(cgd_bf16x4*)&(DSTB)[row * GPHW + c4 * 4] = cgd_to_bf16x4(v); \
      }                                                                \
    }                                                                  \
  }
#define H2_A_LOAD(DST, SRCB, Q)                                                                    \
  {                                                                                                \
    _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                               \
      DST[i][0] = *(const cgd_bf16x8*)&(SRCB)[fro[i] + (Q) * 16];                                  \
      if constexpr (MODE == 1) DST[i][1] = *(const cgd_bf16x8*)&(SRCB)[PLANE + fro[i] + (Q) * 16]; \
    }                                                                                              \
  }
#define H2_B_LOAD(DST, T)                                                                                                         \
  {                                                                                                                               \
    const int in_ = (T) - t_last - 1; /* < 0: inside the slice */                                                                 \
    const int so_ = (((T) >> 2) * (4 * KG) + ((T) & 3)) * (128 * 16);                                                             \
    DST[0] = __builtin_bit_cast(uint4, cgd_buf_load16_if(Bwb, 0xffffffffu, in_, lane * 16, so_));                                 \
    if constexpr (MODE == 1) DST[1] = __builtin_bit_cast(uint4, cgd_buf_load16_if(Bwb, 0xffffffffu, in_, lane * 16 + 1024, so_)); \
  }
#define H2_MFMA(AQ, BQ)                                                                                                       \
  {                                                                                                                           \
    if constexpr (MODE == 1) {                                                                                                \
      _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                                          \
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, BQ[0]), AQ[i][1], acc[i], 0, 0, 0); \
      _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                                          \
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, BQ[1]), AQ[i][0], acc[i], 0, 0, 0); \
    }                                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                                            \
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, BQ[0]), AQ[i][0], acc[i], 0, 0, 0);   \
  }
  // after every MFMA: LDS fragment reads (NI * NPL per k-step), the two global fragment loads, a few conversion VALU ops and
  // the LDS writes of the next chunk's patch
#define H2_INTERLEAVE()                                                                           \
  {                                                                                               \
    _Pragma("unroll") for (int r = 0; r < 3 * NI; ++r) {                                          \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
      if (r % 3 != 2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                          \
      if (r % 3 == 2 && r < 6) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                 \
      __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);                                          \
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                                          \
    }                                                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                            \
  }
  // one 64-deep chunk: ring slots S .. S+3 (S = 0 or 4), LDS buffers CUR -> NXT, staging registers PR (they hold chunk C+1 on
  // entry and are refilled with chunk C+AHEAD once converted)
#define H2_CHUNK(S, CUR, NXT, C, PR)                                                              \
  {                                                                                               \
    const int kq = ((C) - c0) * 4; /* this wavefront's linear k-step index */                     \
    H2_A_LOAD(af[1], CUR, 1);                                                                     \
    H2_B_LOAD(bq[((S) + 0 + DIST) % RING], kq + 0 + DIST);                                        \
    H2_MFMA(af[0], bq[(S) + 0]);                                                                  \
    H2_INTERLEAVE();                                                                              \
    H2_A_LOAD(af[0], CUR, 2);                                                                     \
    H2_B_LOAD(bq[((S) + 1 + DIST) % RING], kq + 1 + DIST);                                        \
    H2_MFMA(af[1], bq[(S) + 1]);                                                                  \
    H2_PATCH_STORE(PR, NXT, 0, NPS / 2);                                                          \
    H2_INTERLEAVE();                                                                              \
    H2_A_LOAD(af[1], CUR, 3);                                                                     \
    H2_B_LOAD(bq[((S) + 2 + DIST) % RING], kq + 2 + DIST);                                        \
    H2_MFMA(af[0], bq[(S) + 2]);                                                                  \
    H2_PATCH_STORE(PR, NXT, NPS / 2, NPS);                                                        \
    H2_INTERLEAVE();                                                                              \
    H2_PATCH_LOAD(PR, (C) + AHEAD);                                                               \
    __syncthreads(); /* NXT fully written; every wavefront has fetched its last fragments of CUR */ \
    H2_A_LOAD(af[0], NXT, 0);                                                                     \
    H2_B_LOAD(bq[((S) + 3 + DIST) % RING], kq + 3 + DIST);                                        \
    H2_MFMA(af[1], bq[(S) + 3]);                                                                  \
    H2_INTERLEAVE();                                                                              \
    H_STAMP_CHUNK(2 + ((C) - c0 < 26 ? (C) - c0 : 26));                                           \
  }

    cgd_bf16x8 af[2][NI][NPL];  // [pipeline slot][row block][plane]
    uint4 bq[RING][NPL];    // [ring slot][plane]
    __bf16* const buf0 = lds;
    __bf16* const buf1 = lds + NPL * PLANE;
    H2_PATCH_LOAD(prs[0], c0);
#pragma unroll
    for (int q = 0; q < DIST; ++q) H2_B_LOAD(bq[q], q);
    H2_PATCH_STORE(prs[0], buf0, 0, NPS);
    // A chunk of the 64-row tile has 0.32 us of MFMA work and the L2 starts every launch cold: both operand streams see the Infinity Cache /
    // HBM latency (1.5-1.9 us), and the loop runs at (that latency) / (depth of the prefetch): activations one chunk ahead 1.4 us per chunk
    // (gemm_r2b), two ahead 0.74-0.94, four ahead 0.65-0.83 (profiles/r3_hgemm_timeline.txt).
#pragma unroll
    for (int k = 0; k < NSET; ++k) H2_PATCH_LOAD(prs[k], c0 + 1 + k);
    int c = c0;
    __syncthreads();
    H_STAMP(1);
    H2_A_LOAD(af[0], buf0, 0);
    // the loop body covers U chunks = one common period of the LDS buffer (2), the staging set (NSET) and the ring base (RING / 4), so that
    // every ring slot, buffer and register set is a compile-time constant; a shorter tail follows
    constexpr int U = h2_lcm(h2_lcm(2, NSET), RING / 4);
    for (; c + U - 1 < c1; c += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) H2_CHUNK((4 * u) % RING, ((u & 1) ? buf1 : buf0), ((u & 1) ? buf0 : buf1), c + u, prs[u % NSET]);
    }
#pragma unroll
    for (int u = 0; u < U - 1; ++u)
      if (c + u < c1) H2_CHUNK((4 * u) % RING, ((u & 1) ? buf1 : buf0), ((u & 1) ? buf0 : buf1), c + u, prs[u % NSET]);
#undef H2_PATCH_LOAD
#undef H2_PATCH_STORE
#undef H2_A_LOAD
#undef H2_B_LOAD
#undef H2_MFMA
#undef H2_INTERLEAVE
#undef H2_CHUNK
  }

  H_STAMP(29);
  // ---- epilogue: D = W x A^T in the 32x32 C/D layout: column (lane & 31) = row m of C, accumulator quad g = columns 8g + 4hh ..
  const int cb0 = n0 + wn * 32;
  if (MODE == 1 && (p.lep || KG == 2 || GNB)) {
    // Stores straight from that layout are 16-byte pieces of 64 different rows per instruction, bound by the CU's store path (the finding
    // of profiles/r3_wconv_timeline.txt for the same layout in wconv_kernel).  The staging buffers are free after the last chunk: each
    // wavefront parks its TM x 32 block in its own slab (16-byte unit q of row r at q ^ (r & 7): conflict-free both ways), reads it
    // back with 8 consecutive lanes on one row, and everything row-wise (bias, residual, activation operands, both outputs, split-K
    // slab) moves whole 128-byte lines.  Same operations per element in the same order as the per-lane epilogue below, which the
    // single-plane modes (half the LDS) and CGD_HGEMM_EPI=0 keep.
    __syncthreads();  // every wavefront has fetched its last A fragments
    float* slab = (float*)lds + wn * (TM * 32);
    if constexpr (KG == 2) {
      // K-group 1 hands its partial block to group 0 (same column block wn, same accumulator layout: lane-contiguous 16-byte
      // units, conflict-free) and is done; group 0 adds it and runs the epilogue
      if (kg == 1) {
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int g = 0; g < 4; ++g)
            *(cgd_f32x4*)&slab[((i * 4 + g) * 64 + lane) * 4] = cgd_f32x4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
      }
      __syncthreads();
      if (kg == 1) return;
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const cgd_f32x4 o = *(const cgd_f32x4*)&slab[((i * 4 + g) * 64 + lane) * 4];
          acc[i][4 * g] += o[0]; acc[i][4 * g + 1] += o[1]; acc[i][4 * g + 2] += o[2]; acc[i][4 * g + 3] += o[3];
        }
      // (the slab is rewritten below by this same wavefront: LDS operations of a wavefront complete in order)
    }
    if (cb0 >= p.N) return;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int rl = i * 32 + l31;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(cgd_f32x4*)&slab[rl * 32 + (((2 * g + hh) ^ rl) & 7) * 4] = cgd_f32x4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int rsub = lane >> 3, quad = lane & 7, col = cb0 + 4 * quad;
    const float* sl = slab + rsub * 32 + ((quad ^ rsub) & 7) * 4;  // row 8 it + rsub at sl[it * 256]
    if (p.splitk > 1) {
      float* __restrict__ ws = wsg + (long)blockIdx.z * p.M * p.N;
#pragma unroll
      for (int it = 0; it < TM / 8; ++it) {
        const long row = m0 + 8 * it + rsub;
        const cgd_f32x4 v = *(const cgd_f32x4*)&sl[it * 256];
        if (row < p.M) *(cgd_f32x4*)&ws[row * p.N + col] = v;
      }
      H_STAMP_END();
      return;
    }
    const bool hb = biasg != nullptr;
    const cgd_f32x4 z4 = cgd_f32x4{0.f, 0.f, 0.f, 0.f};
    const cgd_f32x4 bv = hb ? cgd_f32x4{biasg[col], biasg[col + 1], biasg[col + 2], biasg[col + 3]} : z4;
    const float ka = p.act == 2 ? 1.702f : 1.f;  // QuickGELU x * sigmoid(1.702 x) / SiLU
    constexpr int EB = (TM == 64 || GNB) ? 8 : 4;  // rows in flight per lane (the 96- / 128-row instantiations must stay within 256 registers)
    // GNB: the lane's four channels of the tile's sample (a tile never straddles two samples: the launcher checks)
    cgd_f32x4 gcf[4], gbf[4];
    if constexpr (GNB) {
      const long cb = ((long)(m0 / p.gnf_hw) * p.N + col) * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gcf[e] = *(const cgd_f32x4*)&p.gnf_coef[cb + 4 * e];
        gbf[e] = *(const cgd_f32x4*)&p.gnf_bcoef[cb + 4 * e];
      }
    }
#pragma unroll
    for (int i0 = 0; i0 < TM / 8; i0 += EB) {
      cgd_f32x4 v[EB], rv[EB], uv[EB];
      cgd_f32x4 gx[EB], gd[EB], ga[EB];
      long row[EB];
      bool ok[EB];
#pragma unroll
      for (int u = 0; u < EB; ++u) {
        v[u] = *(const cgd_f32x4*)&sl[(i0 + u) * 256];
        long r = m0 + 8 * (i0 + u) + rsub;
        ok[u] = r < p.M;
        if (!ok[u]) r = p.M - 1;
        if (p.skip_group) {  // (no residual / activation operand with this option: the launcher checks)
          const long grp = r / p.skip_group;
          if (r == grp * p.skip_group) ok[u] = false;
          r -= grp + 1;
          if (r < 0) r = 0;
        }
        row[u] = r;
      }
      if (Rg) {
#pragma unroll
        for (int u = 0; u < EB; ++u) rv[u] = *(const cgd_f32x4*)&Rg[row[u] * p.ldr + col];
      }
      if (p.act_in) {
#pragma unroll
        for (int u = 0; u < EB; ++u) uv[u] = *(const cgd_f32x4*)&p.act_in[row[u] * p.ld_act + col];
      }
      if constexpr (GNB) {
#pragma unroll
        for (int u = 0; u < EB; ++u) {
          gx[u] = cgd_ld16_nt<cgd_f32x4>(&p.gnf_x[row[u] * p.gnf_ldx + col]);
          gd[u] = cgd_ld16_nt<cgd_f32x4>(&p.gnf_dz[row[u] * p.gnf_lddz + col]);
          if (p.gnf_add) ga[u] = cgd_ld16_nt<cgd_f32x4>(&p.gnf_add[row[u] * p.gnf_ldadd + col]);
        }
      }
#pragma unroll
      for (int u = 0; u < EB; ++u) {
        cgd_f32x4 o = v[u] * p.alpha;
        if (hb) o += bv;
        if (Rg) o += rv[u];
        if constexpr (GNB) {  // same operations in the same order as gn_bwd_apply_kernel<1> with o (+ add) as its addend
          if (p.gnf_add) o += ga[u];
          cgd_f32x4 t;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float un = gx[u][e] * gcf[e][0] + gcf[e][1];
            const float sg = 1.f / (1.f + __expf(-un));
            const float d = gd[u][e] * (sg * (1.f + un * (1.f - sg)));
            t[e] = d * gbf[e][0] - (gx[u][e] - gcf[e][3]) * gbf[e][1] - gbf[e][2];
          }
          o = t + o;
          if (ok[u]) cgd_st16_nt(&Cg[row[u] * p.ldc + col], o);
          continue;
        }
        if (p.act_in) {  // backward through the activation: multiply by act'(u), same arithmetic as elem.hip dact_f
          cgd_f32x4 d;
          if constexpr (GELU) {
            d = hg_dgelu4(uv[u]);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float sg = 1.f / (1.f + __expf(-ka * uv[u][e]));
              d[e] = sg * (1.f + ka * uv[u][e] * (1.f - sg));
            }
          }
          o *= d;
        }
        if (ok[u]) {
          *(cgd_f32x4*)&Cg[row[u] * p.ldc + col] = o;
          if (p.act_out) {  // second output: the activated tensor, same arithmetic as elem.hip act_f
            cgd_f32x4 a;
            if constexpr (GELU) {
              a = hg_gelu4(o);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) a[e] = o[e] / (1.f + __expf(-ka * o[e]));
            }
            *(cgd_f32x4*)&p.act_out[row[u] * p.ld_act + col] = a;
          }
        }
      }
    }
    H_STAMP_END();
    return;
  }
  if (cb0 >= p.N) return;
  if (p.splitk > 1) {
    float* __restrict__ ws = wsg + (long)blockIdx.z * p.M * p.N;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const long row = m0 + i * 32 + l31;
      if (row < p.M) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *(cgd_f32x4*)&ws[row * p.N + cb0 + 8 * g + 4 * hh] = cgd_f32x4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    long row = m0 + i * 32 + l31;
    if (row >= p.M) continue;
    if (p.skip_group) {  // (no residual / activation operand with this option: the launcher checks)
      const long grp = row / p.skip_group;
      if (row == grp * p.skip_group) continue;
      row -= grp + 1;
    }
    cgd_f32x4 rv[4];
    if (Rg) {
#pragma unroll
      for (int g = 0; g < 4; ++g) rv[g] = *(const cgd_f32x4*)&Rg[row * p.ldr + cb0 + 8 * g + 4 * hh];
    }
    cgd_f32x4 uv[4];
    if (p.act_in) {
#pragma unroll
      for (int g = 0; g < 4; ++g) uv[g] = *(const cgd_f32x4*)&p.act_in[row * p.ld_act + cb0 + 8 * g + 4 * hh];
    }
    const float ka = p.act == 2 ? 1.702f : 1.f;  // QuickGELU x * sigmoid(1.702 x) / SiLU
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int col = cb0 + 8 * g + 4 * hh;
      const cgd_f32x4 av = cgd_f32x4{acc[i][4 * g], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3]};
      cgd_f32x4 o = av * p.alpha;
      if (biasg) {
        // alpha * acc + bias in ONE rounding, as the LDS epilogue above (the compiler contracts its multiply and add) and splitk_reduce_kernel do it:
        // written as a multiply and an add this path kept both roundings and differed from them in the last bit whenever alpha != 1 met a bias
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf(av[e], p.alpha, biasg[col + e]);
      }
      if (Rg) o += rv[g];
      if (p.act_in) {  // backward through the activation: multiply by act'(u), same arithmetic as elem.hip dact_f
        cgd_f32x4 d;
        if constexpr (GELU) {
          d = hg_dgelu4(uv[g]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float sg = 1.f / (1.f + __expf(-ka * uv[g][e]));
            d[e] = sg * (1.f + ka * uv[g][e] * (1.f - sg));
          }
        }
        o *= d;
      }
      *(cgd_f32x4*)&Cg[row * p.ldc + col] = o;
      if (p.act_out) {  // second output: the activated tensor, same arithmetic as elem.hip act_f
        cgd_f32x4 a;
        if constexpr (GELU) {
          a = hg_gelu4(o);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) a[e] = o[e] / (1.f + __expf(-ka * o[e]));
        }
        *(cgd_f32x4*)&p.act_out[row * p.ld_act + col] = a;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// kgemm_kernel (round 5): weight GEMMs with FEW rows (M <= 256: the 1x1 convolutions / qkv / proj_out of the UNet's 8x8 and 16x16 levels).
// hgemm2 gives such a launch M / 64 x N / 128 = 8-96 workgroups and therefore splits K 2-12 ways across workgroups to put the weight stream
// on enough CUs: 2-12 fp32 slabs + a reduce launch per GEMM (84 of the step's 181 reduce launches, VERDICT r4 "weak" 7).  Here K is split INSIDE
// the workgroup instead (kconv.hip's recipe): a workgroup owns 32 * NI rows x ONE 32-column block, its 4 wavefronts take the 16-deep k-steps
// w, w + 4, w + 8, ... (each streams only its own weight fragments, a register ring RING k-steps deep, and fetches its own 32-byte activation
// runs straight from global memory: an activation element is used by exactly one wavefront, so there is nothing to share through LDS and no
// barrier in the loop), and the four partial accumulators are summed through LDS at the end.  N / 32 x M / (32 NI) workgroups without any
// inter-workgroup split: no slabs, no reduce launch.  Same packed weights as hgemm2 (cgd_frag_cache).
template <int MODE, int NI, int RING>
__global__ __launch_bounds__(256) void kgemm_kernel(const float* __restrict__ Ag, const uint4* __restrict__ Bg, float* Cg,
                                                    const float* __restrict__ biasg, const float* Rg, const HGemmParams p) {
  constexpr int NPL = MODE == 1 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) float red[4 * NI * 16 * 64];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nbN = p.N >> 5;
  int bid = blockIdx.x;
  {
    const int nt = gridDim.x, q = nt >> 3, r = nt & 7, xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  // column-block major: the row tiles that share a weight block are neighbours on one XCD
  const int ntm = gridDim.x / nbN;
  const int mt = bid % ntm, nb = bid / ntm;
  const int m0 = mt * (32 * NI);
  const int nks = p.K >> 4;                       // 16-deep k-steps
  const int mine = (nks - w + 3) >> 2;            // k-steps w, w + 4, ... of this wavefront
  const uint4* __restrict__ Bw = Bg + ((long)nb * nks) * (2 * 64) + lane;  // k-step kq: Bw[kq * 128] (hi), Bw[kq * 128 + 64] (lo)
  bool aok[NI];  // unread, but kept: without it the compiler schedules the k-step loop differently (no longer the measured build)
#pragma unroll
  for (int i = 0; i < NI; ++i) aok[i] = m0 + 32 * i + l31 < p.M;
  (void)aok;
  // byte offset of the lane's row for the buffer loads, no clamp: a row beyond M lies beyond the resource of M rows
  int aoffb[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) aoffb[i] = ((m0 + 32 * i + l31) * p.lda + 8 * hh) * 4;
  const unsigned arec = (unsigned)p.M * (unsigned)p.lda * 4u;
  cgd_f32x16 acc[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  uint4 bq[RING][NPL];
  cgd_f32x4 aq[RING][NI][2];
#define KG_LOAD(SLOT, T)                                                                                                \
  {                                                                                                                     \
    const int t_ = (T) < mine ? (T) : mine - 1; /* clamped: the loads stay unconditional */                             \
    const int kq_ = w + 4 * t_;                                                                                         \
    bq[SLOT][0] = p.nt ? cgd_load_nt(Bw + (long)kq_ * 128) : Bw[(long)kq_ * 128];                                       \
    if constexpr (MODE == 1) bq[SLOT][1] = p.nt ? cgd_load_nt(Bw + (long)kq_ * 128 + 64) : Bw[(long)kq_ * 128 + 64];    \
    _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                                                    \
      /* rows beyond M and k-steps beyond the wavefront's last: out of range, zeros, no memory access */                \
      aq[SLOT][i][0] = __builtin_bit_cast(cgd_f32x4, cgd_buf_load16_if(Ag, arec, (T) - mine, aoffb[i], 64 * kq_));      \
      aq[SLOT][i][1] = __builtin_bit_cast(cgd_f32x4, cgd_buf_load16_if(Ag, arec, (T) - mine, aoffb[i] + 16, 64 * kq_)); \
    }                                                                                                                   \
  }
#define KG_STEP(SLOT)                                                                                                       \
  {                                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < NI; ++i) {                                                                        \
      const cgd_f32x4 a0 = aq[SLOT][i][0], a1 = aq[SLOT][i][1];                                                             \
      cgd_bf16x8 ah, al;                                                                                                    \
      {                                                                                                                     \
        const float a8_[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};                                      \
        cgd_split_oct(a8_, ah, al);                                                                                         \
      }                                                                                                                     \
      if constexpr (MODE == 1) {                                                                                            \
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, bq[SLOT][0]), al, acc[i], 0, 0, 0); \
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, bq[SLOT][1]), ah, acc[i], 0, 0, 0); \
      }                                                                                                                     \
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cgd_bf16x8, bq[SLOT][0]), ah, acc[i], 0, 0, 0);   \
    }                                                                                                                       \
  }
  if (mine > 0) {
#pragma unroll
    for (int q = 0; q < RING - 1; ++q) KG_LOAD(q, q);
    int t = 0;
    for (; t + RING <= mine; t += RING) {
#pragma unroll
      for (int u = 0; u < RING; ++u) {
        KG_LOAD((u + RING - 1) % RING, t + u + RING - 1);
        KG_STEP(u);
      }
    }
#pragma unroll
    for (int u = 0; u < RING - 1; ++u)
      if (t + u < mine) {
        KG_LOAD((u + RING - 1) % RING, t + u + RING - 1);
        KG_STEP(u);
      }
  }
#undef KG_LOAD
#undef KG_STEP
  // ---- the four K partitions meet in LDS: element (wavefront, row block i, register r, lane) at ((w * NI + i) * 16 + r) * 64 + lane (conflict-free
  //      4-byte accesses); wavefront w' then finishes registers 4 w' .. 4 w' + 3 of every row block = 4 consecutive columns 8 w' + 4 hh .. + 3
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((w * NI + i) * 16 + r) * 64 + lane] = acc[i][r];
  __syncthreads();
  const int col = nb * 32 + 8 * w + 4 * hh;
  cgd_f32x4 bv = cgd_f32x4{0.f, 0.f, 0.f, 0.f};
  if (biasg) bv = *(const cgd_f32x4*)(biasg + col);
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    cgd_f32x4 o = cgd_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] += red[((k * NI + i) * 16 + 4 * w + e) * 64 + lane];
    const long row = m0 + 32 * i + l31;
    if (row < p.M) {
      o = o * p.alpha;
      if (biasg) o += bv;
      if (Rg) o += *(const cgd_f32x4*)(Rg + row * p.ldr + col);
      *(cgd_f32x4*)(Cg + row * p.ldc + col) = o;
    }
  }
}

// w [N][ldw] row-major (k contiguous) -> fragment order [N/32][K/32][ks][plane][lane][8] (bf16 hi / lo)
__global__ __launch_bounds__(256) void pack_frag_linear_kernel(const float* __restrict__ w, int ldw, __bf16* __restrict__ out, int N, int K) {
  const long total = (long)N * K;
  const int nk32 = K >> 5;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int e = (int)(t & 7);
    long u = t >> 3;
    const int lane = (int)(u & 63);
    u >>= 6;
    const int ks = (int)(u & 1);
    u >>= 1;
    const int k32 = (int)(u % nk32), nb = (int)(u / nk32);
    const int n = nb * 32 + (lane & 31), k = k32 * 32 + ks * 16 + (lane >> 5) * 8 + e;
    const float v = w[(long)n * ldw + k];
    const __bf16 hi = (__bf16)v;
    const __bf16 lo = (__bf16)(v - (float)hi);
    const long blk = (((long)nb * nk32 + k32) * 2 + ks) * 2;  // + plane
    out[(blk + 0) * 512 + lane * 8 + e] = hi;
    out[(blk + 1) * 512 + lane * 8 + e] = lo;
  }
}

}  // namespace

bool cgd_hgemm_supported(const cgd_ctx* ctx, const GemmParams& p) {
  if (p.conv || ctx->precision == CGD_PREC_F32 || p.nbatch != 1) return false;
  if ( (p.K % GK) || (p.N & 31) || (p.lda & 3) || (p.ldb & 3)) return false;
  if ((p.ldc & 3) || ((uintptr_t)p.C & 15) || ((uintptr_t)p.A & 15)) return false;
  if (p.R && ((p.ldr & 3) || ((uintptr_t)p.R & 15))) return false;
  return true;
}

// fragment-order copy of a persistent weight, packed on first use and cached by (pointer, N, K, ldb)
static const void* cgd_frag_cache_get(cgd_ctx* ctx, const float* w, int N, int K, int ldw, hipStream_t s) {
  for (const FragEntry& e : ctx->frag_cache)
    if (e.w == w && e.N == N && e.K == K && e.ldw == ldw) return e.packed;
  FragEntry e;
  e.w = w; e.N = N; e.K = K; e.ldw = ldw; e.packed = nullptr;
  if (hipMalloc(&e.packed, (size_t)N * K * sizeof(float)) != hipSuccess) return nullptr;
  ++ctx->device_allocs;
  const long total = (long)N * K;
  CGD_LAUNCH(pack_frag_linear_kernel, dim3((int)std::min<long>(cdiv(total, 256), 4096)), dim3(256), 0, s, w, ldw, (__bf16*)e.packed, N, K);
  ctx->frag_cache.push_back(e);
  return e.packed;
}

void cgd_frag_cache_clear(cgd_ctx* ctx) {
  for (FragEntry& e : ctx->frag_cache) (void)hipFree(e.packed);
  ctx->frag_cache.clear();
}

// rows per workgroup tile: hgemm_var 0 = hgemm_kernel (128 x 128, 64 x 64 per wavefront); 1 = hgemm2_kernel with 64-row tiles
// while 128-row tiles would not give every CU a workgroup, 128 rows otherwise; 2 / 3 force hgemm2 with 128 / 64 rows
int cgd_hgemm_tile_m(const cgd_ctx* ctx, const GemmParams& p) {
  if (p.gnf_x) return GM;  // the GroupNorm-backward epilogue exists for the 128-row tile only
  if ((long)p.M * p.lda >= (1L << 29)) return GM;  // beyond hgemm2's extent (cgd_launch_hgemm, v2) hgemm_kernel runs, which maps workgroups to 128-row tiles
  if (ctx->hgemm_var == 3) return 64;
  if (ctx->hgemm_var == 1 && (long)cdiv(p.M, GM) * cdiv(p.N, GN) < ctx->num_cu) {
    // (round 5) 96-row tiles where 64-row tiles need more workgroups than the chip has CUs but 96-row tiles do not: the ViT's M = 800,
    // N = 3072 linears are 13 x 24 = 312 workgroups (56 CUs run two, the makespan is theirs) on 64 rows, 9 x 24 = 216 = one round on 96
    const long t64 = (long)cdiv(p.M, 64) * cdiv(p.N, GN), t96 = (long)cdiv(p.M, 96) * cdiv(p.N, GN);
    if (ctx->hgemm_tm96 && ctx->precision != CGD_PREC_F32 && t64 > ctx->num_cu && t96 <= ctx->num_cu) return 96;
    return 64;
  }
  return GM;
}
int cgd_hgemm_tiles(const cgd_ctx* ctx, const GemmParams& p) { return cdiv(p.M, cgd_hgemm_tile_m(ctx, p)) * cdiv(p.N, GN); }
int cgd_hgemm_chunks(const GemmParams& p) { return p.K / GK; }

// kgemm_kernel takes persistent-weight GEMMs of 5 .. kgemm_max_m rows in one slice, without the epilogue options only hgemm2 has.
// Capability (what the kernel can run: the forced tile codes 518 / 519 ask only this) apart from policy (what the automatic selection gives it;
// a forced launch used to fail with "does not support this problem" when a policy knob said no)
bool cgd_kgemm_capable(const cgd_ctx* ctx, const GemmParams& p) {
  if ((uintptr_t)p.bias & 15) return false;  // the epilogue reads the bias 16 bytes at a time
  // rows beyond M are not clamped: only the resource's extent (M * lda * 4 bytes) masks them, so the byte offset of the last row of the last
  // 64-row tile must not wrap past 2^32 back into range (few rows on a huge stride: M = 5, lda near 2^29 / 5, row 11 would land on row 1)
  if ((long)cdiv(p.M, 64) * 64 * p.lda >= (1L << 30)) return false;
  return p.weight && p.M > 4 && cgd_hgemm_supported(ctx, p) && !p.act_out && !p.act_in && !p.skip_group && !p.gnf_x && p.splitk <= 1 && (long)p.M * p.lda < (1L << 29);
}
bool cgd_kgemm_supported(const cgd_ctx* ctx, const GemmParams& p) {
  const bool rows_ok = p.M <= ctx->kgemm_max_m || (p.M <= ctx->kgemm_big_m && p.N <= ctx->kgemm_big_n);
  if (ctx->kgemm_mode == 2 && p.defer && ctx->defer_mode >= 2) return false;  // mode 2: a GEMM whose split-K slices its consumer would sum anyway stays on hgemm2
  return ctx->kgemm_mode && rows_ok && cgd_kgemm_capable(ctx, p);
}
// drops the cached fragment copy of ONE weight (tests hand over a fresh B per call, possibly at a recycled address)
void cgd_frag_cache_evict(cgd_ctx* ctx, const float* w) {
  for (size_t i = 0; i < ctx->frag_cache.size();) {
    if (ctx->frag_cache[i].w == w) {
      (void)hipFree(ctx->frag_cache[i].packed);  // waits for kernels in flight
      ctx->frag_cache.erase(ctx->frag_cache.begin() + i);
    } else {
      ++i;
    }
  }
}
int cgd_kgemm_ni(const cgd_ctx* ctx, const GemmParams& p) {  // 32-row tiles: same-box A/B (profiles/r5_ab_tm96_kgemm.txt) 64-row tiles everywhere
  (void)p;                                                      // +0.43 ms per step, 32-row tiles everywhere -0.03 against a mixed policy
  return (ctx->kgemm_var & 1) ? 2 : 1;
}
int cgd_kgemm_tiles(const cgd_ctx* ctx, const GemmParams& p) { return cdiv(p.M, 32 * cgd_kgemm_ni(ctx, p)) * (p.N >> 5); }

int cgd_launch_kgemm(cgd_ctx* ctx, const GemmParams& g, hipStream_t s) {
  const void* packed = cgd_frag_cache_get(ctx, g.B, g.N, g.K, g.ldb, s);
  if (!packed) CGD_FAIL(ctx, "kgemm: out of memory for the packed weight copy");
  HGemmParams p = {};
  p.lda = g.lda; p.ldc = g.ldc; p.ldr = g.ldr;
  p.M = g.M; p.N = g.N; p.K = g.K; p.splitk = 1; p.alpha = g.alpha;
  p.nt = ((ctx->weight_nt & 2) && g.M <= 64) ? 1 : 0;
  const int ni = cgd_kgemm_ni(ctx, g);  // A/B variants (CGD_KGEMM="<mode>,<max rows>,<variant bits>"): bit 0 = 64-row tiles, bit 2 = deep rings (10 / 6
                                        // k-steps instead of 6 / 4)
  dim3 grid(cdiv(g.M, 32 * ni) * (g.N >> 5));
  const bool x3 = ctx->precision == CGD_PREC_BF16X3;
  const bool deep = (ctx->kgemm_var & 4) != 0;
#define KG_ARGS grid, dim3(256), 0, s, g.A, (const uint4*)packed, g.C, g.bias, g.R, p
  if (ni == 2) {
    if (!x3) CGD_LAUNCH((kgemm_kernel<2, 2, 4>), KG_ARGS);
    else if (deep) CGD_LAUNCH((kgemm_kernel<1, 2, 6>), KG_ARGS);
    else CGD_LAUNCH((kgemm_kernel<1, 2, 4>), KG_ARGS);
  } else {
    if (!x3) CGD_LAUNCH((kgemm_kernel<2, 1, 6>), KG_ARGS);
    else if (deep) CGD_LAUNCH((kgemm_kernel<1, 1, 10>), KG_ARGS);
    else CGD_LAUNCH((kgemm_kernel<1, 1, 6>), KG_ARGS);
  }
#undef KG_ARGS
  return 0;
}

int cgd_launch_hgemm(cgd_ctx* ctx, const GemmParams& g, hipStream_t s) {
  const void* packed = nullptr;
  if (g.weight) {
    packed = cgd_frag_cache_get(ctx, g.B, g.N, g.K, g.ldb, s);
  } else {
    // non-persistent B (forced tile code 513, tests): pack into a scratch copy that is reused stream-ordered
    const size_t need = (size_t)g.N * g.K * sizeof(float);
    if (need > ctx->frag_tmp_bytes) {
      if (ctx->frag_tmp) {
        CGD_HIP(ctx, hipStreamSynchronize(s));
        CGD_HIP(ctx, hipFree(ctx->frag_tmp));
      }
      ctx->frag_tmp = nullptr;
      ctx->frag_tmp_bytes = 0;
      CGD_HIP(ctx, hipMalloc(&ctx->frag_tmp, need));
      ctx->frag_tmp_bytes = need;
    }
    const long total = (long)g.N * g.K;
    CGD_LAUNCH(pack_frag_linear_kernel, dim3((int)std::min<long>(cdiv(total, 256), 4096)), dim3(256), 0, s, g.B, g.ldb,
                       (__bf16*)ctx->frag_tmp, g.N, g.K);
    packed = ctx->frag_tmp;
  }
  if (!packed) CGD_FAIL(ctx, "hgemm: out of memory for the packed weight copy");
  HGemmParams p = {};
  p.lda = g.lda; p.ldc = g.ldc; p.ldr = g.ldr;
  p.M = g.M; p.N = g.N; p.K = g.K; p.splitk = g.splitk; p.alpha = g.alpha;
  p.nmajor = (ctx->tile_order == 1 || (ctx->tile_order == 0 && g.N >= g.M)) ? 1 : 0;
  p.act_out = g.act_out; p.act_in = g.act_in; p.ld_act = g.ld_act; p.act = g.act;
  p.skip_group = g.skip_group;
  p.lep = ctx->hgemm_epi;
  p.nt_out = (long)g.M * g.N * 4 > (32L << 20) ? 1 : 0;  // an output beyond the 32 MB of L2
  const bool x3 = ctx->precision == CGD_PREC_BF16X3;
  // hgemm2 addresses A with 32-bit BYTE offsets (buffer loads)
  const bool v2 = ctx->hgemm_var != 0 && (long)g.M * g.lda < (1L << 29);
  const int tm = cgd_hgemm_tile_m(ctx, g);  // GM whenever !v2
  dim3 grid(cdiv(g.M, tm) * cdiv(g.N, GN), 1, g.splitk > 1 ? g.splitk : 1);
  if (!v2 && (g.act_out || g.act_in || g.skip_group))
    CGD_FAIL(ctx, "hgemm: activation / skip_group epilogues need hgemm2, i.e. M * lda < 2^29 floats (32-bit byte offsets into A)");
  if (g.skip_group && (g.splitk > 1 || g.R || g.act_out || g.act_in))
    CGD_FAIL(ctx, "hgemm: skip_group needs hgemm2 in one slice without residual / activation operands");
  const bool gelu = (g.act_out || g.act_in) && g.act == 3;
  if (g.gnf_x) {
    // (cgd_gemm_fuses_gnb is the callers' question; this is the kernel's own list)
    if (!v2 || !x3 || g.splitk > 1 || g.act_out || g.act_in || g.skip_group || !g.gnf_dz || !g.gnf_coef || !g.gnf_bcoef)
      CGD_FAIL(ctx, "hgemm: the GroupNorm-backward epilogue needs hgemm2 in bf16x3 mode, one slice, no activation operands");
    if (g.gnf_hw <= 0 || g.M % g.gnf_hw || ((g.gnf_hw % GM) && g.gnf_hw != g.M))
      CGD_FAIL(ctx, "hgemm: the GroupNorm-backward epilogue needs samples of a multiple of 128 rows (or one sample)");
    if (((g.gnf_ldx | g.gnf_lddz | (g.gnf_add ? g.gnf_ldadd : 0)) & 3) ||
        (((uintptr_t)g.gnf_x | (uintptr_t)g.gnf_dz | (uintptr_t)g.gnf_add | (uintptr_t)g.gnf_coef | (uintptr_t)g.gnf_bcoef) & 15))
      CGD_FAIL(ctx, "hgemm: the GroupNorm-backward epilogue needs row strides that are multiples of 4 and 16-byte aligned operands");
    p.gnf_x = g.gnf_x; p.gnf_dz = g.gnf_dz; p.gnf_add = g.gnf_add; p.gnf_coef = g.gnf_coef; p.gnf_bcoef = g.gnf_bcoef;
    p.gnf_ldx = g.gnf_ldx; p.gnf_lddz = g.gnf_lddz; p.gnf_ldadd = g.gnf_ldadd; p.gnf_hw = g.gnf_hw;
  }
#define HG_ARGS grid, dim3(256), 0, s, g.A, (const uint4*)packed, g.C, g.bias, g.R, g.ws, p
  if (g.gnf_x) {
    CGD_LAUNCH((hgemm2_kernel<1, 128, 8, 1, 1, false, true>), HG_ARGS);
  } else if (!v2) {
    if (x3) CGD_LAUNCH((hgemm_kernel<1>), HG_ARGS); else CGD_LAUNCH((hgemm_kernel<2>), HG_ARGS);
  } else if (tm == 64 && x3 && g.K % (2 * GK) == 0 &&
             (ctx->hgemm_kg == 2 || (ctx->hgemm_kg == 0 && (long)grid.x * grid.z <= ctx->num_cu && g.K / (2 * GK) / (int)grid.z >= 4))) {
    // two K-groups of wavefronts per workgroup (512 threads): see hgemm2_kernel; always on the LDS epilogue.  Automatic only where the
    // micro-benchmark shows a gain (profiles/r4_hgemm_kgroups.txt): one workgroup per CU at most (an 8-wavefront workgroup has a CU to itself,
    // a second round of workgroups costs more than the loop gains) and >= 8 64-deep chunks per slice (the prologue / hand-over are longer)
    if (gelu) CGD_LAUNCH((hgemm2_kernel<1, 64, 8, 2, 2, true>), grid, dim3(512), 0, s, g.A, (const uint4*)packed, g.C, g.bias, g.R, g.ws, p);
    else CGD_LAUNCH((hgemm2_kernel<1, 64, 8, 2, 2>), grid, dim3(512), 0, s, g.A, (const uint4*)packed, g.C, g.bias, g.R, g.ws, p);
  } else if (gelu) {  // the exact-GELU epilogues (the open_clip towers' c_fc and its backward)
    if (tm == 96) {
      if (x3) CGD_LAUNCH((hgemm2_kernel<1, 96, 8, 2, 1, true>), HG_ARGS); else CGD_LAUNCH((hgemm2_kernel<2, 96, 8, 2, 1, true>), HG_ARGS);
    } else if (tm == 64) {
      if (x3) CGD_LAUNCH((hgemm2_kernel<1, 64, 8, 2, 1, true>), HG_ARGS); else CGD_LAUNCH((hgemm2_kernel<2, 64, 8, 2, 1, true>), HG_ARGS);
    } else {
      if (x3) CGD_LAUNCH((hgemm2_kernel<1, 128, 8, 1, 1, true>), HG_ARGS); else CGD_LAUNCH((hgemm2_kernel<2, 128, 8, 1, 1, true>), HG_ARGS);
    }
  } else if (tm == 96) {
    if (x3) CGD_LAUNCH((hgemm2_kernel<1, 96, 8, 2>), HG_ARGS); else CGD_LAUNCH((hgemm2_kernel<2, 96, 8, 2>), HG_ARGS);
  } else if (tm == 64) {
    if (x3) CGD_LAUNCH((hgemm2_kernel<1, 64>), HG_ARGS); else CGD_LAUNCH((hgemm2_kernel<2, 64>), HG_ARGS);
  } else {
    if (x3) CGD_LAUNCH((hgemm2_kernel<1, 128>), HG_ARGS); else CGD_LAUNCH((hgemm2_kernel<2, 128>), HG_ARGS);
  }
#undef HG_ARGS
  return 0;
}
