// CLIP text tower (clip.model.CLIP.encode_text) forward on MI355X.
//
// Replaces the `clip` package's text transformer behind encode_text_prompt (cgd/clip_util.py; the reference's clip_util.py:104-108,
// reached for every text prompt from cgd/cgd.py).  Setup-time work, forward only:
//   x = token_embedding[tok] + positional_embedding                (text_tokens_kernel)
//   `layers` pre-LN residual blocks, the image tower's ResidualAttentionBlock with a CAUSAL attention mask
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

struct TextLayer {
  std::string pre;
  float *ln1g = 0, *ln1b = 0, *inw = 0, *inb = 0, *ow = 0, *ob = 0;
  float *ln2g = 0, *ln2b = 0, *fcw = 0, *fcb = 0, *pjw = 0, *pjb = 0;
};

struct TextTower : NetBase {
  cgd_text_config cfg;
  int T = 0, W = 0;
  std::vector<TextLayer> layers;
  float *tokemb = 0, *pos = 0, *lnf_g = 0, *lnf_b = 0, *proj = 0, *projT = 0;
  // one set of layer buffers (forward only); xa / xb carry the residual stream from layer to layer
  DevBuf xa, xb, st1, y, qkv, qkvT, probs, a, x1, st2, y2, u, ga, eot, eotn, st_f;

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
  for (int l = 0; l < cfg.layers; ++l) {
    const std::string p = "transformer.resblocks." + std::to_string(l);
    layers[l].pre = p;
    add_param(p + ".ln_1.weight", W);
    add_param(p + ".ln_1.bias", W);
    add_param(p + ".attn.in_proj_weight", (int64_t)3 * W * W);
    add_param(p + ".attn.in_proj_bias", 3 * W);
    add_param(p + ".attn.out_proj.weight", (int64_t)W * W);
    add_param(p + ".attn.out_proj.bias", W);
    add_param(p + ".ln_2.weight", W);
    add_param(p + ".ln_2.bias", W);
    add_param(p + ".mlp.c_fc.weight", (int64_t)4 * W * W);
    add_param(p + ".mlp.c_fc.bias", 4 * W);
    add_param(p + ".mlp.c_proj.weight", (int64_t)4 * W * W);
    add_param(p + ".mlp.c_proj.bias", W);
  }
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
  if (!projT) CGD_TRY(alloc(&projT, (size_t)W * cfg.out_dim));
  CGD_TRY(cgd_launch_transpose(ctx, proj, cfg.out_dim, 0, projT, W, 0, W, cfg.out_dim, 1, s));
  for (TextLayer& l : layers) {
    const std::string& p = l.pre;
    l.ln1g = P(p + ".ln_1.weight"); l.ln1b = P(p + ".ln_1.bias");
    l.inw = P(p + ".attn.in_proj_weight"); l.inb = P(p + ".attn.in_proj_bias");
    l.ow = P(p + ".attn.out_proj.weight"); l.ob = P(p + ".attn.out_proj.bias");
    l.ln2g = P(p + ".ln_2.weight"); l.ln2b = P(p + ".ln_2.bias");
    l.fcw = P(p + ".mlp.c_fc.weight"); l.fcb = P(p + ".mlp.c_fc.bias");
    l.pjw = P(p + ".mlp.c_proj.weight"); l.pjb = P(p + ".mlp.c_proj.bias");
  }
  CGD_HIP(ctx, hipStreamSynchronize(s));
  finalized = true;
  return 0;
}

// nn.Linear y = A W^T + bias (+ R): B = the torch weight [out][in] as uploaded
static GemmParams lin(const float* A, int lda, const float* Wt, int K, float* C, int ldc, const float* bias, const float* R, int ldr, long M, int Nn,
                      int defer = 0) {
  GemmParams p;
  p.defer = defer;  // 1: the next kernel reading C is a LayerNorm that sums split-K slices itself (norm.hip)
  p.A = A; p.lda = lda; p.B = Wt; p.ldb = K; p.C = C; p.ldc = ldc; p.bias = bias; p.R = R; p.ldr = ldr;
  p.weight = 1;
  p.M = (int)M; p.N = Nn; p.K = K;
  return p;
}

int TextTower::forward(const int64_t* tok, int N, float* emb, hipStream_t s) {
  if (!finalized) CGD_FAIL(ctx, "text: finalize() has not been called after the last set_param");
  if (N < 1) CGD_FAIL(ctx, "text: N must be >= 1");
  const long rows = (long)N * T;
  const int H = cfg.heads, d = W / H;
  const int ldq = 3 * W, ldo = W;  // the row strides of qkv and of the attention output, used both to size the scratch and for the launch
  const AttnShape sh{N, H, T, d, W, 0, 1};
  CGD_TRY(ensure(xa, rows * W)); CGD_TRY(ensure(xb, rows * W));
  CGD_TRY(ensure(st1, rows * 2)); CGD_TRY(ensure(st2, rows * 2));
  CGD_TRY(ensure(y, rows * W)); CGD_TRY(ensure(qkv, rows * ldq)); CGD_TRY(ensure(a, rows * ldo));
  CGD_TRY(ensure(x1, rows * W)); CGD_TRY(ensure(y2, rows * W)); CGD_TRY(ensure(u, rows * 4 * W)); CGD_TRY(ensure(ga, rows * 4 * W));
  CGD_TRY(ensure(qkvT, cgd_attn_buf_floats(ctx, sh, ldq, ldo, 0))); CGD_TRY(ensure(probs, cgd_attn_buf_floats(ctx, sh, ldq, ldo, 1)));
  CGD_TRY(ensure(eot, (size_t)N * W)); CGD_TRY(ensure(eotn, (size_t)N * W)); CGD_TRY(ensure(st_f, (size_t)N * 2));
  CGD_TRY(cgd_sync_pending(ctx, s));
  CGD_LAUNCH(text_tokens_kernel, dim3((unsigned)rows), dim3(256), 0, s, tok, tokemb, pos, xa.p, T, W, (int64_t)cfg.vocab_size);
  CGD_HIP(ctx, hipGetLastError());
  float* x = xa.p;
  float* xo = xb.p;
  for (TextLayer& l : layers) {
    CGD_TRY(cgd_launch_ln_fwd(ctx, x, W, y.p, W, (int)rows, W, l.ln1g, l.ln1b, 1e-5f, st1.p, s));
    CGD_TRY(cgd_launch_gemm(ctx, lin(y.p, W, l.inw, W, qkv.p, ldq, l.inb, nullptr, 0, rows, 3 * W), s));
    AttnBufs bf{qkvT.p, probs.p, nullptr, nullptr, nullptr};
    CGD_TRY(cgd_attn_fwd(ctx, sh, qkv.p, ldq, a.p, ldo, bf, s));
    CGD_TRY(cgd_launch_gemm(ctx, lin(a.p, ldo, l.ow, W, x1.p, W, l.ob, x, W, rows, W, 1), s));
    CGD_TRY(cgd_launch_ln_fwd(ctx, x1.p, W, y2.p, W, (int)rows, W, l.ln2g, l.ln2b, 1e-5f, st2.p, s));
    {
      // c_fc + QuickGELU (fused into the GEMM's epilogue where the weight GEMM kernel takes the launch in one slice)
      GemmParams fc = lin(y2.p, W, l.fcw, W, u.p, 4 * W, l.fcb, nullptr, 0, rows, 4 * W);
      if (cgd_gemm_fuses_act(ctx, fc)) {
        fc.act_out = ga.p; fc.ld_act = 4 * W; fc.act = 2;
        CGD_TRY(cgd_launch_gemm(ctx, fc, s));
      } else {
        CGD_TRY(cgd_launch_gemm(ctx, fc, s));
        CGD_TRY(cgd_launch_act_fwd(ctx, u.p, ga.p, rows * 4 * W, 2, s));
      }
    }
    CGD_TRY(cgd_launch_gemm(ctx, lin(ga.p, 4 * W, l.pjw, 4 * W, xo, W, l.pjb, x1.p, W, rows, W, 1), s));
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
int cgd_text_create(cgd_ctx* ctx, const cgd_text_config* cfg, cgd_text** out) {
  if (!ctx || !cfg || !out) return -3;
  cgd_text* t = new cgd_text();
  t->net.ctx = ctx;
  t->net.cfg = *cfg;
  if (t->net.build() != 0) {
    delete t;
    return -2;
  }
  *out = t;
  return 0;
}
// host-only: parameter manifest (OpenAI top-level names, element counts); no GPU, no context
int cgd_text_manifest(const cgd_text_config* cfg, void (*cb)(const char*, int64_t, void*), void* user) {
  if (!cfg) return -3;
  cgd_ctx host;
  TextTower net;
  net.ctx = &host;
  net.cfg = *cfg;
  if (net.build() != 0) return -2;
  if (cb)
    for (const ParamSpec& p : net.params) cb(p.name.c_str(), p.numel, user);
  return (int)net.params.size();
}
void cgd_text_destroy(cgd_text* t) {
  if (t) cgd_frag_cache_clear(t->net.ctx);
  delete t;
}
int cgd_text_num_params(cgd_text* t) {
  if (!t) return -3;
  DeviceScope dev_scope(t->net.ctx);
  return (int)t->net.params.size();
}
int cgd_text_param_info(cgd_text* t, int i, char* buf, int len, int64_t* numel) {
  if (!t) return -3;
  DeviceScope dev_scope(t->net.ctx);
  if (i < 0 || i >= (int)t->net.params.size()) return -1;
  snprintf(buf, len, "%s", t->net.params[i].name.c_str());
  if (numel) *numel = t->net.params[i].numel;
  return 0;
}
int cgd_text_set_param(cgd_text* t, const char* name, const float* data, int64_t numel) {
  if (!t) return -3;
  DeviceScope dev_scope(t->net.ctx);
  cgd_frag_cache_clear(t->net.ctx);
  return t->net.set_param(name, data, numel);
}
int cgd_text_finalize(cgd_text* t) {
  if (!t) return -3;
  DeviceScope dev_scope(t->net.ctx);
  cgd_frag_cache_clear(t->net.ctx);
  return t->net.finalize(nullptr);
}
int cgd_text_forward(cgd_text* t, const int64_t* tokens, int N, float* emb, void* stream) {
  if (!t || !tokens || !emb) return -3;
  DeviceScope dev_scope(t->net.ctx);
  if (const int rc = t->net.forward(tokens, N, emb, (hipStream_t)stream)) {
    t->net.ctx->pending.valid = false;  // failed pass: its deferred slices must not be reduced into a stale tensor later
    return rc;
  }
  return cgd_flush_pending(t->net.ctx, (hipStream_t)stream);
}
}
