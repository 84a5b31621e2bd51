// CLIP text tower (clip.model.CLIP.encode_text) forward on MI355X.
//
// Replaces the `clip` package's text transformer behind encode_text_prompt (cgd/clip_util.py; the reference's clip_util.py:104-108,
// reached for every text prompt from cgd/cgd.py).  Setup-time work, forward only:
//   x = token_embedding[tok] + positional_embedding                (text_tokens_kernel)
//   `layers` pre-LN residual blocks, the image tower's ResidualAttentionBlock (ClipBlock, net.h) with a CAUSAL attention mask
//   (clip.model.CLIP.build_attention_mask: key j > query i excluded; every attention kernel family honours AttnShape::causal)
//   row of each sequence at argmax(tok[n]) (the end-of-text token, the first maximal id)   (text_eot_kernel)
//   ln_final on those N rows only (LayerNorm is per row, so gathering first is exact) -> @ text_projection
// One set of layer buffers is reused by every layer: nothing is kept for a backward pass.
#include "../../include/cgd_mi355x.h"
#include "net.h"

namespace {

// x[n][t][:] = emb[tok[n][t]][:] + pos[t][:]; an id outside [0, vocab) reads nothing and makes its row NaN (the Python wrapper rejects such ids)
__global__ __launch_bounds__(256) void text_tokens_kernel(const int64_t* __restrict__ tok, const float* __restrict__ emb, const float* __restrict__ pos,
                                                          float* __restrict__ x, int T, int W, int64_t vocab) {
  const long row = blockIdx.x;
  const int t = (int)(row % T);
  const int64_t id = tok[row];
  const bool ok = id >= 0 && id < vocab;
  const float* __restrict__ e = emb + (ok ? id : 0) * (int64_t)W;
  const float* __restrict__ p = pos + (long)t * W;
  float* __restrict__ o = x + row * W;
  for (int c = threadIdx.x; c < W; c += 256) o[c] = ok ? e[c] + p[c] : NAN;
}

// out[n][:] = x[n][argmax_t tok[n][t]][:], the FIRST maximal index (torch.argmax, CLIP's end-of-text convention); one wavefront per sequence
__global__ __launch_bounds__(64) void text_eot_kernel(const int64_t* __restrict__ tok, const float* __restrict__ x, float* __restrict__ out, int T, int W) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const int64_t* __restrict__ tk = tok + (long)n * T;
  int64_t best = tk[0];
  int bi = 0;
  for (int t = lane; t < T; t += 64) {  // t ascending: a strict > keeps this lane's first maximum
    const int64_t v = tk[t];
    if (v > best) {
      best = v;
      bi = t;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int64_t ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  const float* __restrict__ src = x + ((long)n * T + bi) * W;
  for (int c = lane; c < W; c += 64) out[(long)n * W + c] = src[c];
}

struct TextTower : NetBase {
  cgd_text_config cfg;
  int T = 0, W = 0;
  std::vector<ClipBlock> layers;
  float *tokemb = 0, *pos = 0, *lnf_g = 0, *lnf_b = 0, *proj = 0, *projT = 0;
  ClipActs act;  // one set of layer buffers (forward only); xa / xb carry the residual stream from layer to layer
  DevBuf xa, xb, eot, eotn, st_f;

  int build();
  int finalize(hipStream_t s);
  int forward(const int64_t* tok, int N, float* emb, hipStream_t s);
};

int TextTower::build() {
  T = cfg.context_length;
  W = cfg.width;
  if (T < 1 || cfg.vocab_size < 1 || cfg.layers < 0 || cfg.out_dim < 1 || W < 1 || cfg.heads < 1) CGD_FAIL(ctx, "text: bad configuration");
  if (W % cfg.heads || (W / cfg.heads) % 4) CGD_FAIL(ctx, "text: bad head configuration");
  add_param("token_embedding.weight", (int64_t)cfg.vocab_size * W);
  add_param("positional_embedding", (int64_t)T * W);
  layers.resize(cfg.layers);
  for (int l = 0; l < cfg.layers; ++l) layers[l].add_params(*this, "transformer.resblocks." + std::to_string(l), W, cfg.heads);
  add_param("ln_final.weight", W);
  add_param("ln_final.bias", W);
  add_param("text_projection", (int64_t)W * cfg.out_dim);
  return 0;
}

int TextTower::finalize(hipStream_t s) {
  CGD_TRY(check_all_set());
  tokemb = P("token_embedding.weight"); pos = P("positional_embedding");
  lnf_g = P("ln_final.weight"); lnf_b = P("ln_final.bias");
  proj = P("text_projection");
  // emb = x @ text_projection: the GEMM's B operand is [N = out_dim][K = W]
  CGD_TRY(transpose_weight(proj, &projT, W, cfg.out_dim, s));
  for (ClipBlock& l : layers) l.lookup(*this);
  CGD_HIP(ctx, hipStreamSynchronize(s));
  finalized = true;
  return 0;
}

int TextTower::forward(const int64_t* tok, int N, float* emb, hipStream_t s) {
  if (!finalized) CGD_FAIL(ctx, "text: finalize() has not been called after the last set_param");
  if (N < 1) CGD_FAIL(ctx, "text: N must be >= 1");
  const long rows = (long)N * T;
  CGD_TRY(ensure(xa, rows * W)); CGD_TRY(ensure(xb, rows * W));
  CGD_TRY(ensure(eot, (size_t)N * W)); CGD_TRY(ensure(eotn, (size_t)N * W)); CGD_TRY(ensure(st_f, (size_t)N * 2));
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(text_tokens_kernel, dim3((unsigned)rows), dim3(256), 0, s, tok, tokemb, pos, xa.p, T, W, (int64_t)cfg.vocab_size);
  CGD_HIP(ctx, hipGetLastError());
  float* x = xa.p;
  float* xo = xb.p;
  for (const ClipBlock& l : layers) {
    CGD_TRY(clip_block_fwd(*this, l, act, x, xo, N, T, true, s));
    std::swap(x, xo);
  }
  CGD_TRY(cgd_sync_pending(ctx, s));  // the gather reads the residual stream: a deferred split-K reduction must have landed
  CGD_LAUNCH(text_eot_kernel, dim3(N), dim3(64), 0, s, tok, x, eot.p, T, W);
  CGD_HIP(ctx, hipGetLastError());
  CGD_TRY(cgd_launch_ln_fwd(ctx, eot.p, W, eotn.p, W, N, W, lnf_g, lnf_b, 1e-5f, st_f.p, s));
  CGD_TRY(cgd_launch_gemm(ctx, lin(eotn.p, W, projT, W, emb, cfg.out_dim, nullptr, nullptr, 0, N, cfg.out_dim), s));
  return 0;
}

}  // namespace

struct cgd_text {
  TextTower net;
};

extern "C" {
int cgd_text_create(cgd_ctx* ctx, const cgd_text_config* cfg, cgd_text** out) { return net_create(ctx, out, cfg); }
// host-only: OpenAI top-level names
int cgd_text_manifest(const cgd_text_config* cfg, void (*cb)(const char*, int64_t, void*), void* user) { return net_manifest<TextTower>(cb, user, cfg); }
void cgd_text_destroy(cgd_text* t) { net_destroy(t); }
int cgd_text_num_params(cgd_text* t) { return net_num_params(t); }
int cgd_text_param_info(cgd_text* t, int i, char* buf, int len, int64_t* numel) { return net_param_info(t, i, buf, len, numel); }
int cgd_text_set_param(cgd_text* t, const char* name, const float* data, int64_t numel) { return net_set_param(t, name, data, numel); }
int cgd_text_finalize(cgd_text* t) { return net_finalize(t); }
int cgd_text_set_activation(cgd_text* t, int act) { return t ? clip_set_activation(t->net.ctx, t->net.layers, act) : -3; }
int cgd_text_forward(cgd_text* t, const int64_t* tokens, int N, float* emb, void* stream) {
  if (!tokens || !emb) return -3;
  return net_pass(t, stream, [&](hipStream_t s) { return t->net.forward(tokens, N, emb, s); });
}
}
