// Head of the noisy ImageNet classifier (guided_diffusion.unet.EncoderUNetModel with pool="attention"): AttentionPool2d, log-softmax and the
// selection of the class, forward and backward-to-input.  The trunk in front of it (the encoder half of the ADM UNet) lives in unet.hip.
//
//   tokens = [mean_p h_p | h_0 .. h_{S2-1}] + positional_embedding            T = S2 + 1 tokens of C channels
//   qkv    = qkv_proj(tokens), split in the NEW order (q, k, v = chunk(3, dim=1), then heads), each operand scaled by d^-1/4
//   a      = softmax_t(q_0 . k_t) v_t per head                                 only token 0 of the attention output is ever used
//   logits = c_proj(a),  logp = log_softmax(logits)[y]
//
// Decode-shaped work: one query row against T keys per (sample, head).  K and V of one head (T x d floats each) are staged in LDS once and
// read from there by both contractions; no T x T matrix exists and no MFMA is used.  The dense products (q of token 0, K and V of all tokens,
// c_proj, and their adjoints) run on the GEMM launcher.  Everything a pass needs lives in one scratch block sized by the call shape.
#include <algorithm>
#include <cmath>

#include "../../include/cgd_mi355x.h"
#include "net.h"
#include "mfma_stage.h"

namespace {

constexpr int NT = 256;                     // threads per workgroup of every kernel below (4 wavefronts of 64)
constexpr size_t kAttnLdsMax = 64 * 1024;   // static + dynamic LDS a workgroup may ask for without an opt-in attribute

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// reductions over the NT threads of the workgroup; red: 4 floats of LDS, free again when the call returns
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

// tok[b][0] = mean_p h[b][p] + posT[0];  tok[b][1 + p] = h[b][p] + posT[1 + p].  grid (C / 64 rounded up, B): a workgroup owns 64 channels of one
// sample; its four wavefronts walk the positions four at a time (256-byte row segments), then their partial sums meet in LDS.
__global__ __launch_bounds__(NT) void cls_tokens_fwd_kernel(const float* __restrict__ h, int ldh, const float* __restrict__ posT,
                                                            float* __restrict__ tok, int S2, int C) {
  __shared__ float part[4][64];
  const int b = blockIdx.y, lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const int T = S2 + 1;
  float sum = 0.f;
  if (c < C) {
    for (int p = grp; p < S2; p += 4) {
      const float v = h[((long)b * S2 + p) * ldh + c];
      sum += v;
      tok[((long)b * T + 1 + p) * C + c] = v + posT[(long)(1 + p) * C + c];
    }
  }
  part[grp][lane] = sum;
  __syncthreads();
  if (grp == 0 && c < C) {
    const float m = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) / (float)S2;
    tok[(long)b * T * C + c] = m + posT[c];
  }
}

// adjoint: dh[b][p] = dtok[b][1 + p] + (dtok[b][0] + dq0[b]) / S2, where dq0 is the part of token 0's gradient that came through its query
// (the K / V part of every token's gradient is dtok).  cq = C / 4: one float4 of channels per thread.
__global__ __launch_bounds__(NT) void cls_tokens_bwd_kernel(const float* __restrict__ dtok, const float* __restrict__ dq0, float* __restrict__ dh,
                                                            int lddh, int B, int S2, int cq) {
  const int T = S2 + 1, C = 4 * cq;
  const long total = (long)B * S2 * cq;
  const float inv = 1.f / (float)S2;
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int q = (int)(i % cq);
    const long r = i / cq;
    const int p = (int)(r % S2), b = (int)(r / S2);
    const cgd_f32x4 own = *(const cgd_f32x4*)(dtok + ((long)b * T + 1 + p) * C + 4 * q);
    const cgd_f32x4 t0 = *(const cgd_f32x4*)(dtok + (long)b * T * C + 4 * q);
    const cgd_f32x4 q0 = *(const cgd_f32x4*)(dq0 + (long)b * C + 4 * q);
    cgd_f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = own[k] + (t0[k] + q0[k]) * inv;
    *(cgd_f32x4*)(dh + r * lddh + 4 * q) = o;
  }
}

// LDS of the two attention kernels: K and V of one head as [T][d + 1] (the pad keeps the per-key dot products — lane t walks row t — off a
// single bank), then q, the upstream gradient of a (backward), the probabilities, the score gradients (backward), 4 floats of reduction space
__host__ __device__ inline size_t attn1_lds_floats(int T, int d) { return (size_t)2 * T * (d + 1) + 2 * d + 2 * T + 4; }

// One workgroup per (sample, head).  q [B][C], kv [B * T][2C] = [K all heads | V all heads]; P [B * heads][T] is kept for the backward;
// a [B][C].  scale = d^-1/2 (the two d^-1/4 of the operands).
__global__ __launch_bounds__(NT) void cls_attn1_fwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ P,
                                                           float* __restrict__ a, int T, int C, int heads, int d, float scale) {
  extern __shared__ float sm[];
  const int dp = d + 1;
  float* sK = sm;
  float* sV = sK + (size_t)T * dp;
  float* sq = sV + (size_t)T * dp;
  float* sp = sq + 2 * d;
  float* red = sp + 2 * T;
  const int b = blockIdx.x / heads, hh = blockIdx.x - b * heads, tid = threadIdx.x;
  const float* kvb = kv + (long)b * T * 2 * C + hh * d;
  for (int i = tid; i < T * d; i += NT) {
    const int t = i / d, c = i - t * d;
    sK[t * dp + c] = kvb[(long)t * 2 * C + c];
    sV[t * dp + c] = kvb[(long)t * 2 * C + C + c];
  }
  for (int c = tid; c < d; c += NT) sq[c] = q[(long)b * C + hh * d + c];
  __syncthreads();
  float mx = -INFINITY;
  for (int t = tid; t < T; t += NT) {
    float s = 0.f;
    for (int c = 0; c < d; ++c) s += sq[c] * sK[t * dp + c];
    s *= scale;
    sp[t] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int t = tid; t < T; t += NT) {
    const float e = expf(sp[t] - mx);
    sp[t] = e;
    sum += e;
  }
  sum = block_sum(sum, red);
  const float inv = 1.f / sum;
  for (int t = tid; t < T; t += NT) {
    const float p = sp[t] * inv;
    sp[t] = p;
    P[(long)blockIdx.x * T + t] = p;
  }
  __syncthreads();
  for (int c = tid; c < d; c += NT) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += sp[t] * sV[t * dp + c];
    a[(long)b * C + hh * d + c] = acc;
  }
}

// adjoint of the above for the upstream gradient da [B][C]:
//   dp_t = da . v_t;  ds_t = p_t (dp_t - sum_u p_u dp_u) scale;  dq = sum_t ds_t k_t;  dK_t = ds_t q;  dV_t = p_t da
// dq [B][C], dkv [B * T][2C] (every element written)
__global__ __launch_bounds__(NT) void cls_attn1_bwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, const float* __restrict__ P,
                                                           const float* __restrict__ da, float* __restrict__ dq, float* __restrict__ dkv, int T,
                                                           int C, int heads, int d, float scale) {
  extern __shared__ float sm[];
  const int dp = d + 1;
  float* sK = sm;
  float* sV = sK + (size_t)T * dp;
  float* sq = sV + (size_t)T * dp;
  float* sda = sq + d;
  float* sp = sda + d;
  float* sds = sp + T;
  float* red = sds + T;
  const int b = blockIdx.x / heads, hh = blockIdx.x - b * heads, tid = threadIdx.x;
  const float* kvb = kv + (long)b * T * 2 * C + hh * d;
  for (int i = tid; i < T * d; i += NT) {
    const int t = i / d, c = i - t * d;
    sK[t * dp + c] = kvb[(long)t * 2 * C + c];
    sV[t * dp + c] = kvb[(long)t * 2 * C + C + c];
  }
  for (int c = tid; c < d; c += NT) {
    sq[c] = q[(long)b * C + hh * d + c];
    sda[c] = da[(long)b * C + hh * d + c];
  }
  for (int t = tid; t < T; t += NT) sp[t] = P[(long)blockIdx.x * T + t];
  __syncthreads();
  float dot = 0.f;
  for (int t = tid; t < T; t += NT) {
    float s = 0.f;
    for (int c = 0; c < d; ++c) s += sda[c] * sV[t * dp + c];
    sds[t] = s;
    dot += sp[t] * s;
  }
  dot = block_sum(dot, red);
  for (int t = tid; t < T; t += NT) sds[t] = sp[t] * (sds[t] - dot) * scale;
  __syncthreads();
  float* dkvb = dkv + (long)b * T * 2 * C + hh * d;
  for (int i = tid; i < T * d; i += NT) {
    const int t = i / d, c = i - t * d;
    dkvb[(long)t * 2 * C + c] = sds[t] * sq[c];
    dkvb[(long)t * 2 * C + C + c] = sp[t] * sda[c];
  }
  for (int c = tid; c < d; c += NT) {
    float acc = 0.f;
    for (int t = 0; t < T; ++t) acc += sds[t] * sK[t * dp + c];
    dq[(long)b * C + hh * d + c] = acc;
  }
}

// One workgroup per sample: lse[b] = max + log(sum exp(l - max)) of lg [B][ldl]; logp[b] = l[y_b] - lse[b] (NaN for a y outside [0, out));
// copies the row to logits [B][out] and keeps y for the backward.  The maximum is subtracted first: logits near +-100 do not overflow.
__global__ __launch_bounds__(NT) void cls_lse_kernel(const float* __restrict__ lg, int ldl, const int64_t* __restrict__ y, float* __restrict__ logits,
                                                     float* __restrict__ logp, float* __restrict__ lse, int64_t* __restrict__ ykeep, int out) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* row = lg + (long)b * ldl;
  float mx = -INFINITY;
  for (int j = tid; j < out; j += NT) {
    const float v = row[j];
    mx = fmaxf(mx, v);
    if (logits) logits[(long)b * out + j] = v;
  }
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int j = tid; j < out; j += NT) sum += expf(row[j] - mx);
  sum = block_sum(sum, red);
  if (tid == 0) {
    const float l = mx + logf(sum);
    const int64_t yy = y[b];
    lse[b] = l;
    ykeep[b] = yy;
    if (logp) logp[b] = (yy >= 0 && yy < out) ? row[yy] - l : NAN;
  }
}

// dlg[b][j] = scale (onehot(y_b)[j] - softmax(lg[b])[j]) for j < out, 0 for the pad columns [out, outP)
__global__ __launch_bounds__(NT) void cls_seed_kernel(const float* __restrict__ lg, const float* __restrict__ lse, const int64_t* __restrict__ ykeep,
                                                      float* __restrict__ dlg, int B, int out, int outP, float scale) {
  const long total = (long)B * outP;
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int b = (int)(i / outP), j = (int)(i - (long)b * outP);
    float v = 0.f;
    if (j < out) v = scale * ((ykeep[b] == (int64_t)j ? 1.f : 0.f) - expf(lg[i] - lse[b]));
    dlg[i] = v;
  }
}

// cwT[c][j] = cw[j][c] for j < out, 0 for the pad columns: the backward GEMM's operand (its K = outP must be a multiple of 4)
__global__ __launch_bounds__(NT) void cls_pack_cwT_kernel(const float* __restrict__ cw, float* __restrict__ cwT, int out, int outP, int C) {
  const long total = (long)C * outP;
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const int c = (int)(i / outP), j = (int)(i - (long)c * outP);
    cwT[i] = j < out ? cw[(long)j * C + c] : 0.f;
  }
}

__global__ __launch_bounds__(NT) void cls_accumulate_kernel(float* __restrict__ g, const float* __restrict__ d, long n4) {
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long)gridDim.x * NT) {
    cgd_f32x4 a = ((cgd_f32x4*)g)[i];
    const cgd_f32x4 v = ((const cgd_f32x4*)d)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += v[k];
    ((cgd_f32x4*)g)[i] = a;
  }
}

size_t r4(size_t n) { return (n + 3) & ~(size_t)3; }

// the scratch block: every region starts 16-byte aligned
struct PoolBufs {
  float *tok, *q, *kv, *P, *a, *lg, *lse, *dlg, *da, *dq, *dkv, *dtok, *dq0;
  int64_t* ykeep;
  size_t total;
};
PoolBufs carve(const AttnPoolShape& sh, float* base) {
  const size_t B = sh.B, T = sh.S2 + 1, C = sh.C, heads = sh.C / sh.d, outP = r4(sh.out);
  PoolBufs o;
  size_t off = 0;
  auto take = [&](size_t n) {
    float* p = base ? base + off : nullptr;
    off += r4(n);
    return p;
  };
  o.tok = take(B * T * C);
  o.q = take(B * C);
  o.kv = take(B * T * 2 * C);
  o.P = take(B * heads * T);
  o.a = take(B * C);
  o.lg = take(B * outP);
  o.lse = take(B);
  o.ykeep = (int64_t*)take(2 * B);
  o.dlg = take(B * outP);
  o.da = take(B * C);
  o.dq = take(B * C);
  o.dkv = take(B * T * 2 * C);
  o.dtok = take(B * T * C);
  o.dq0 = take(B * C);
  o.total = off;
  return o;
}

int check_shape(cgd_ctx* ctx, const AttnPoolShape& sh) {
  if (sh.B <= 0 || sh.B > 65535 || sh.S2 <= 0 || sh.C <= 0 || sh.d <= 0 || sh.out <= 0) CGD_FAIL(ctx, "attnpool: empty shape");
  if (!cgd_attnpool_supported(sh.S2, sh.C, sh.d, sh.out))
    CGD_FAIL(ctx, "attnpool: C must be a multiple of 4 and of the head width, and K and V of one head ((S*S + 1) x d floats each) must fit 64 KB of LDS");
  return 0;
}

}  // namespace

bool cgd_attnpool_supported(int S2, int C, int d, int out) {
  if (S2 <= 0 || C <= 0 || d <= 0 || out <= 0 || (C & 3) || C % d) return false;
  if ((long)S2 + 1 > (1 << 20) || d > (1 << 14)) return false;
  return (attn1_lds_floats(S2 + 1, d) + 4) * sizeof(float) <= kAttnLdsMax;
}

size_t cgd_attnpool_scratch_floats(const AttnPoolShape& sh) { return carve(sh, nullptr).total; }

int cgd_attnpool_pack_cwT(cgd_ctx* ctx, const float* cw, float* cwT, int out, int C, hipStream_t s) {
  const int outP = (int)r4(out);
  CGD_LAUNCH(cls_pack_cwT_kernel, dim3(grid_for((long)C * outP)), dim3(NT), 0, s, cw, cwT, out, outP, C);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_launch_accumulate(cgd_ctx* ctx, float* g, const float* d, long n, hipStream_t s) {
  if (n <= 0 || (n & 3) || ((uintptr_t)g & 15) || ((uintptr_t)d & 15)) CGD_FAIL(ctx, "accumulate: n must be a positive multiple of 4, pointers 16-byte aligned");
  CGD_LAUNCH(cls_accumulate_kernel, dim3(grid_for(n / 4)), dim3(NT), 0, s, g, d, n / 4);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_attnpool_fwd(cgd_ctx* ctx, const AttnPoolShape& sh, const AttnPoolWeights& w, const float* h, int ldh, const int64_t* y, float* pooled,
                     float* logits, float* logp, float* scratch, hipStream_t s) {
  CGD_TRY(check_shape(ctx, sh));
  if (!h || !y || !scratch || ldh < sh.C || ((uintptr_t)scratch & 15)) CGD_FAIL(ctx, "attnpool: h, y and a 16-byte aligned scratch are required");
  const PoolBufs b = carve(sh, scratch);
  const int B = sh.B, S2 = sh.S2, T = S2 + 1, C = sh.C, d = sh.d, heads = C / d, out = sh.out, outP = (int)r4(out);
  CGD_TRY(cgd_sync_pending(ctx, s));  // h may still lie in split-K slices of its producer
  CGD_LAUNCH(cls_tokens_fwd_kernel, dim3(cdiv(C, 64), B), dim3(NT), 0, s, h, ldh, w.posT, b.tok, S2, C);
  // q of token 0 only (row b * T of the token matrix); K and V of every token
  GemmParams gq = lin(b.tok, T * C, w.qkvw, C, b.q, C, w.qkvb, nullptr, 0, B, C);
  gq.weight = sh.weight;
  CGD_TRY(cgd_launch_gemm(ctx, gq, s));
  GemmParams gkv = lin(b.tok, C, w.qkvw + (size_t)C * C, C, b.kv, 2 * C, w.qkvb + C, nullptr, 0, (long)B * T, 2 * C);
  gkv.weight = sh.weight;
  CGD_TRY(cgd_launch_gemm(ctx, gkv, s));
  const size_t lds = attn1_lds_floats(T, d) * sizeof(float);
  CGD_LAUNCH(cls_attn1_fwd_kernel, dim3(B * heads), dim3(NT), lds, s, b.q, b.kv, b.P, b.a, T, C, heads, d, 1.f / sqrtf((float)d));
  GemmParams gc = lin(b.a, C, w.cw, C, b.lg, outP, w.cb, nullptr, 0, B, out);
  gc.weight = sh.weight;
  CGD_TRY(cgd_launch_gemm(ctx, gc, s));
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(cls_lse_kernel, dim3(B), dim3(NT), 0, s, b.lg, outP, y, logits, logp, b.lse, b.ykeep, out);
  if (pooled) CGD_HIP(ctx, hipMemcpyAsync(pooled, b.a, (size_t)B * C * sizeof(float), hipMemcpyDeviceToDevice, s));
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

int cgd_attnpool_bwd(cgd_ctx* ctx, const AttnPoolShape& sh, const AttnPoolWeights& w, float scale, float* dh, int lddh, float* scratch,
                     hipStream_t s) {
  CGD_TRY(check_shape(ctx, sh));
  if (!dh || !scratch || lddh < sh.C || (lddh & 3) || ((uintptr_t)dh & 15) || ((uintptr_t)scratch & 15))
    CGD_FAIL(ctx, "attnpool: dh (16-byte aligned, row stride a multiple of 4) and the forward's scratch are required");
  const PoolBufs b = carve(sh, scratch);
  const int B = sh.B, S2 = sh.S2, T = S2 + 1, C = sh.C, d = sh.d, heads = C / d, out = sh.out, outP = (int)r4(out);
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(cls_seed_kernel, dim3(grid_for((long)B * outP)), dim3(NT), 0, s, b.lg, b.lse, b.ykeep, b.dlg, B, out, outP, scale);
  // da = dlogits c_proj.weight
  GemmParams gc = lin(b.dlg, outP, w.cwT, outP, b.da, C, nullptr, nullptr, 0, B, C);
  gc.weight = sh.weight;
  CGD_TRY(cgd_launch_gemm(ctx, gc, s));
  CGD_TRY(cgd_sync_pending(ctx, s));
  const size_t lds = attn1_lds_floats(T, d) * sizeof(float);
  CGD_LAUNCH(cls_attn1_bwd_kernel, dim3(B * heads), dim3(NT), lds, s, b.q, b.kv, b.P, b.da, b.dq, b.dkv, T, C, heads, d, 1.f / sqrtf((float)d));
  // token gradients: K / V part of every token (columns C .. 3C of qkv_proj.weight^T), q part of token 0 (columns 0 .. C)
  GemmParams gkv = lin(b.dkv, 2 * C, w.qkvwT + C, 2 * C, b.dtok, C, nullptr, nullptr, 0, (long)B * T, C);
  gkv.ldb = 3 * C;
  gkv.weight = sh.weight;
  CGD_TRY(cgd_launch_gemm(ctx, gkv, s));
  GemmParams gq = lin(b.dq, C, w.qkvwT, C, b.dq0, C, nullptr, nullptr, 0, B, C);
  gq.ldb = 3 * C;
  gq.weight = sh.weight;
  CGD_TRY(cgd_launch_gemm(ctx, gq, s));
  CGD_TRY(cgd_sync_pending(ctx, s));
  cgd_chanstats_invalidate(ctx, dh, (long)B * S2, lddh, C);
  CGD_LAUNCH(cls_tokens_bwd_kernel, dim3(grid_for((long)B * S2 * (C / 4))), dim3(NT), 0, s, b.dtok, b.dq0, dh, lddh, B, S2, C / 4);
  CGD_HIP(ctx, hipGetLastError());
  return 0;
}

// ---- op-level entry points (tests, benchmarks): the weights as a checkpoint holds them; the transposed copies are packed behind the pass
// scratch on every forward call --------------------------------------------------------------------------------------------------------
namespace {
struct OpLayout {
  AttnPoolShape sh;
  size_t pass, posT, qkvwT, cwT, total;
};
OpLayout op_layout(int B, int S, int C, int d, int out) {
  OpLayout L;
  L.sh = AttnPoolShape{B, S * S, C, d, out, 0};
  const size_t T = (size_t)S * S + 1;
  L.pass = cgd_attnpool_scratch_floats(L.sh);
  L.posT = L.pass;
  L.qkvwT = L.posT + r4(T * C);
  L.cwT = L.qkvwT + r4((size_t)3 * C * C);
  L.total = L.cwT + r4((size_t)C * r4(out));
  return L;
}
bool op_args_ok(int B, int S, int C, int d, int out) {
  return B > 0 && B <= 65535 && S > 0 && S <= 1024 && C > 0 && d > 0 && out > 0 && cgd_attnpool_supported(S * S, C, d, out);
}
}  // namespace

extern "C" {
int64_t cgd_op_attnpool_scratch_floats(int B, int S, int C, int d, int out) {
  if (!op_args_ok(B, S, C, d, out)) return -2;
  return (int64_t)op_layout(B, S, C, d, out).total;
}
int cgd_op_attnpool_fwd(cgd_ctx* ctx, const float* h, const float* pos, const float* qkv_w, const float* qkv_b, const float* c_w, const float* c_b,
                        const int64_t* y, float* pooled, float* logits, float* logp, float* scratch, int B, int S, int C, int d, int out,
                        void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  if (!op_args_ok(B, S, C, d, out)) CGD_FAIL(ctx, "attnpool: unsupported shape");
  if (!h || !pos || !qkv_w || !qkv_b || !c_w || !c_b || !y || !scratch || ((uintptr_t)scratch & 15)) CGD_FAIL(ctx, "attnpool: missing or misaligned buffer");
  hipStream_t s = (hipStream_t)stream;
  const OpLayout L = op_layout(B, S, C, d, out);
  const int T = S * S + 1;
  CGD_TRY(cgd_launch_transpose(ctx, pos, T, 0, scratch + L.posT, C, 0, C, T, 1, s));
  CGD_TRY(cgd_launch_transpose(ctx, qkv_w, C, 0, scratch + L.qkvwT, 3 * C, 0, 3 * C, C, 1, s));
  CGD_TRY(cgd_attnpool_pack_cwT(ctx, c_w, scratch + L.cwT, out, C, s));
  const AttnPoolWeights w{scratch + L.posT, qkv_w, qkv_b, scratch + L.qkvwT, c_w, c_b, scratch + L.cwT};
  CGD_TRY(cgd_attnpool_fwd(ctx, L.sh, w, h, C, y, pooled, logits, logp, scratch, s));
  return cgd_flush_pending(ctx, s);
}
int cgd_op_attnpool_bwd(cgd_ctx* ctx, const float* qkv_w, const float* qkv_b, const float* c_w, const float* c_b, float scale, float* dh, float* scratch,
                        int B, int S, int C, int d, int out, void* stream) {
  if (!ctx) return -3;
  DeviceScope dev_scope(ctx);
  if (!op_args_ok(B, S, C, d, out)) CGD_FAIL(ctx, "attnpool: unsupported shape");
  if (!qkv_w || !qkv_b || !c_w || !c_b || !dh || !scratch) CGD_FAIL(ctx, "attnpool: missing buffer");
  hipStream_t s = (hipStream_t)stream;
  const OpLayout L = op_layout(B, S, C, d, out);
  const AttnPoolWeights w{scratch + L.posT, qkv_w, qkv_b, scratch + L.qkvwT, c_w, c_b, scratch + L.cwT};
  CGD_TRY(cgd_attnpool_bwd(ctx, L.sh, w, scale, dh, C, scratch, s));
  return cgd_flush_pending(ctx, s);
}
}  // extern "C"
