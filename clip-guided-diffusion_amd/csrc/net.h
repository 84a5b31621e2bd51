// Shared plumbing of the network handles (UNet, ViT, CLIP text, CLIP ResNet, LPIPS): named parameter store, device buffers that are
// allocated once and reused by every later step (no allocation in the hot loop), weight packing helpers, attention scratch sized by the
// launch that uses it, the handle C ABI written once, and CLIP's residual attention block (image and text tower).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "kernels.h"

struct DevBuf {
  float* p = nullptr;
  size_t n = 0;
};

// view of an activation: rows x C with row stride ld
struct TV {
  float* p = nullptr;
  int ld = 0;
  int C = 0;
};

struct ParamSpec {
  std::string name;
  int64_t numel = 0;
  float* dev = nullptr;
  bool set = false;
};

// attention scratch (AttnBufs' members): NetBase::attn_fwd / attn_bwd size it with exactly the (shape, strides) they launch with, so it always
// fits the kernel family cgd_attn_fwd / cgd_attn_bwd pick for that call (flash: row statistics + a copy of O instead of T x T probabilities)
struct AttnScratch {
  DevBuf qkvT, P, Pt, dP, dAt;
};

struct NetBase {
  // false: the handle leaves the context's frag cache alone (LPIPS: its convs use their own pre-packed Bpk copies, and clearing the cache would
  // evict the packed weights of the context's other nets)
  static constexpr bool uses_frag_cache = true;
  cgd_ctx* ctx = nullptr;
  std::vector<ParamSpec> params;
  std::map<std::string, int> index;
  std::vector<void*> allocs;
  bool finalized = false;

  ~NetBase() {
    for (void* p : allocs) (void)hipFree(p);
  }
  int add_param(const std::string& name, int64_t numel) {
    index[name] = (int)params.size();
    ParamSpec s;
    s.name = name;
    s.numel = numel;
    params.push_back(s);
    return (int)params.size() - 1;
  }
  float* P(const std::string& name) {
    auto it = index.find(name);
    return it == index.end() ? nullptr : params[it->second].dev;
  }
  int alloc(float** out, size_t n) {
    void* p = nullptr;
    CGD_HIP(ctx, hipMalloc(&p, (n ? n : 1) * sizeof(float)));
    ++ctx->device_allocs;
    allocs.push_back(p);
    *out = (float*)p;
    return 0;
  }
  int ensure(DevBuf& b, size_t n) {
    if (n == 0 || (b.n >= n && b.p)) return 0;
    // grow-only; the old block stays registered and is released with the handle
    CGD_TRY(alloc(&b.p, n));
    b.n = n;
    return 0;
  }
  int set_param(const char* name, const float* data, int64_t numel) {
    auto it = index.find(name);
    if (it == index.end()) CGD_FAIL(ctx, std::string("unknown parameter: ") + name);
    ParamSpec& s = params[it->second];
    if (s.numel != numel)
      CGD_FAIL(ctx, std::string("parameter ") + name + ": expected " + std::to_string(s.numel) + " elements, got " + std::to_string(numel));
    if (!s.dev) CGD_TRY(alloc(&s.dev, (size_t)numel));
    CGD_HIP(ctx, hipMemcpy(s.dev, data, (size_t)numel * sizeof(float), hipMemcpyDefault));
    s.set = true;
    finalized = false;
    return 0;
  }
  int check_all_set() {
    for (auto& s : params)
      if (!s.set) CGD_FAIL(ctx, "parameter not set: " + s.name);
    return 0;
  }
  // wt = w^T for a weight w [rows][cols] (wt [cols][rows]: the backward's operand), allocated on the first call
  int transpose_weight(const float* w, float** wt, int rows, int cols, hipStream_t s) {
    if (!*wt) CGD_TRY(alloc(wt, (size_t)rows * cols));
    return cgd_launch_transpose(ctx, w, cols, 0, *wt, rows, 0, rows, cols, 1, s);
  }
  int attn_fwd(AttnScratch& b, const AttnShape& sh, const float* qkv, int ldq, float* out, int ldo, hipStream_t s) {
    CGD_TRY(ensure(b.qkvT, cgd_attn_buf_floats(ctx, sh, ldq, ldo, 0)));
    CGD_TRY(ensure(b.P, cgd_attn_buf_floats(ctx, sh, ldq, ldo, 1)));
    return cgd_attn_fwd(ctx, sh, qkv, ldq, out, ldo, AttnBufs{b.qkvT.p, b.P.p, nullptr, nullptr, nullptr}, s);
  }
  // after attn_fwd on the same scratch; a dout stride that selects another family than the forward's fails in cgd_attn_bwd
  int attn_bwd(AttnScratch& b, const AttnShape& sh, const float* qkv, int ldq, const float* dout, int lddo, float* dqkv, int lddq, hipStream_t s) {
    CGD_TRY(ensure(b.Pt, cgd_attn_buf_floats(ctx, sh, ldq, lddo, 2)));
    CGD_TRY(ensure(b.dP, cgd_attn_buf_floats(ctx, sh, ldq, lddo, 3)));
    CGD_TRY(ensure(b.dAt, cgd_attn_buf_floats(ctx, sh, ldq, lddo, 4)));
    return cgd_attn_bwd(ctx, sh, qkv, ldq, dout, lddo, dqkv, lddq, AttnBufs{b.qkvT.p, b.P.p, b.Pt.p, b.dP.p, b.dAt.p}, s);
  }
};

// nn.Linear y = A W^T + bias (+ R): B = the torch weight [out][in] as uploaded, a persistent (packed-at-load) weight
static inline GemmParams lin(const float* A, int lda, const float* Wt, int K, float* C, int ldc, const float* bias, const float* R, int ldr,
                             long M, int Nn, int defer = 0) {
  GemmParams p;
  p.defer = defer;  // 1: the next kernel reading C is a LayerNorm that sums split-K slices itself (norm.hip)
  p.A = A; p.lda = lda; p.B = Wt; p.ldb = K; p.C = C; p.ldc = ldc; p.bias = bias; p.R = R; p.ldr = ldr;
  p.weight = 1;
  p.M = (int)M; p.N = Nn; p.K = K;
  return p;
}

// ---- CLIP's ResidualAttentionBlock (clip.model), shared by the image tower (vit.hip) and the text tower (text.hip):
//   x1 = x + out_proj(MHA(ln_1(x))),  x_out = x1 + c_proj(act(c_fc(ln_2(x1)))), act = QuickGELU or GELU
struct ClipBlock {
  std::string pre;  // parameter prefix, "transformer.resblocks.{l}"
  int W = 0, heads = 0;
  int act = 2;  // activation between c_fc and c_proj: 2 QuickGELU (OpenAI's towers), 3 exact GELU (open_clip's); cgd_vit_set_activation / cgd_text_set_activation
  float eps = 1e-5f;  // of both LayerNorms (CLIP's; the depth net's timm blocks use 1e-6)
  std::string names[12];  // the twelve parameters in the order of the pointers below (CLIP's names, or timm's for the depth net's backbone)
  float *ln1g = 0, *ln1b = 0, *inw = 0, *inb = 0, *ow = 0, *ob = 0;
  float *ln2g = 0, *ln2b = 0, *fcw = 0, *fcb = 0, *pjw = 0, *pjb = 0;
  // build(): registers the twelve parameters; timm: under timm's VisionTransformer block names (norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2:
  // the same tensors in the same layouts)
  void add_params(NetBase& net, const std::string& prefix, int width, int nheads, bool timm = false);
  void lookup(NetBase& net);                                                        // finalize(): their device pointers
};
// the forward activations of one block (the image tower keeps one set per layer for its backward pass, the text tower reuses one set)
struct ClipActs {
  DevBuf st1, y, qkv, a, x1, st2, y2, u, ga;
  AttnScratch att;
};
// the towers' cgd_*_set_activation: any time after create
template <class Blocks>
int clip_set_activation(cgd_ctx* ctx, Blocks& blocks, int act) {
  if (act != 2 && act != 3) CGD_FAIL(ctx, "set_activation: act must be 2 (QuickGELU) or 3 (GELU)");
  for (auto& b : blocks) b.act = act;
  return 0;
}
// x [N*T][W] -> xo [N*T][W] (xo != x); causal: key j > query i is masked (the text tower)
int clip_block_fwd(NetBase& net, const ClipBlock& b, ClipActs& t, const float* x, float* xo, int N, int T, bool causal, hipStream_t s);

// ---- the handle C ABI, written once: every family's extern "C" entry points (include/cgd_mi355x.h) forward to these.  H is the opaque
// handle struct, whose member `net` is the family's NetBase; cfg: the family's configuration (none for LPIPS).
template <class H, class... Cfg>
int net_create(cgd_ctx* ctx, H** out, const Cfg*... cfg) {
  if (!ctx || !out || ((!cfg) || ...)) return -3;
  H* h = new H();
  h->net.ctx = ctx;
  ((h->net.cfg = *cfg), ...);
  if (h->net.build() != 0) {
    delete h;
    return -2;
  }
  *out = h;
  return 0;
}
// host-only: parameter manifest of a configuration (names, element counts); no GPU, no context
template <class Net, class... Cfg>
int net_manifest(void (*cb)(const char*, int64_t, void*), void* user, const Cfg*... cfg) {
  if (((!cfg) || ...)) return -3;
  cgd_ctx host;  // plain host object: build() only records names and shapes
  Net net;
  net.ctx = &host;
  ((net.cfg = *cfg), ...);
  if (net.build() != 0) return -2;
  if (cb)
    for (const ParamSpec& p : net.params) cb(p.name.c_str(), p.numel, user);
  return (int)net.params.size();
}
template <class H>
void net_destroy(H* h) {
  if (h && h->net.uses_frag_cache) cgd_frag_cache_clear(h->net.ctx);  // packed copies are keyed by weight pointers that die with the net
  delete h;
}
template <class H>
int net_num_params(H* h) {
  if (!h) return -3;
  DeviceScope dev_scope(h->net.ctx);
  return (int)h->net.params.size();
}
template <class H>
int net_param_info(H* h, int i, char* buf, int len, int64_t* numel) {
  if (!h) return -3;
  DeviceScope dev_scope(h->net.ctx);
  if (i < 0 || i >= (int)h->net.params.size()) return -1;
  snprintf(buf, len, "%s", h->net.params[i].name.c_str());
  if (numel) *numel = h->net.params[i].numel;
  return 0;
}
template <class H>
int net_set_param(H* h, const char* name, const float* data, int64_t numel) {
  if (!h) return -3;
  DeviceScope dev_scope(h->net.ctx);
  if (h->net.uses_frag_cache) cgd_frag_cache_clear(h->net.ctx);
  return h->net.set_param(name, data, numel);
}
template <class H>
int net_finalize(H* h) {
  if (!h) return -3;
  DeviceScope dev_scope(h->net.ctx);
  if (h->net.uses_frag_cache) cgd_frag_cache_clear(h->net.ctx);
  return h->net.finalize(nullptr);
}
// one forward / backward pass: pass(stream) runs it on the handle's device; nothing it deferred may outlive the call
template <class H, class F>
int net_pass(H* h, void* stream, F&& pass) {
  if (!h) return -3;
  DeviceScope dev_scope(h->net.ctx);
  if (const int rc = pass((hipStream_t)stream)) {
    h->net.ctx->pending.valid = false;  // failed pass: its deferred slices must not be reduced into a stale tensor later
    return rc;
  }
  return cgd_flush_pending(h->net.ctx, (hipStream_t)stream);
}

// one-time weight packing (device side)
// w [Co][Ci][3][3] -> fwd  [Co][(ky*3+kx)*Ci + ci]
// w [Co][Ci][3][3] -> dgrad [Ci][(ky*3+kx)*Co + co] = w[co][ci][2-ky][2-kx]
int cgd_pack_conv3x3(cgd_ctx* ctx, const float* w, float* wf, float* wd, int Co, int Ci, hipStream_t s);
