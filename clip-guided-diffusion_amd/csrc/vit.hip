// CLIP image tower (clip.model.VisionTransformer) forward and backward-to-input on MI355X.
//
// Replaces clip_model.encode_image(clip_in) (/root/reference/cgd/cgd.py:194; model loaded at
// /root/reference/cgd/clip_util.py:59-66) and the CLIP leg of th.autograd.grad(loss, x) (cgd.py:228).
// patch conv (kernel = stride = patch, no bias) = GEMM over im2col rows; 12/24 pre-LN residual blocks:
// LN(fp32) -> packed in_proj -> MHA (softmax(QK^T/sqrt(64))V) -> out_proj ; LN -> c_fc -> QuickGELU -> c_proj;
// ln_post(cls) @ proj.  Only d/d(image) is needed: each linear's backward is the same GEMM kernel on a
// transposed copy of the weight packed at load.
#include <memory>

#include "../../include/cgd_mi355x.h"
#include "net.h"

// ---- ClipBlock (net.h): also the text tower's block
void ClipBlock::add_params(NetBase& net, const std::string& prefix, int width, int nheads, bool timm) {
  pre = prefix;
  W = width;
  heads = nheads;
  static const char* const clip_names[12] = {".ln_1.weight", ".ln_1.bias", ".attn.in_proj_weight", ".attn.in_proj_bias", ".attn.out_proj.weight",
                                             ".attn.out_proj.bias", ".ln_2.weight", ".ln_2.bias", ".mlp.c_fc.weight", ".mlp.c_fc.bias",
                                             ".mlp.c_proj.weight", ".mlp.c_proj.bias"};
  static const char* const timm_names[12] = {".norm1.weight", ".norm1.bias", ".attn.qkv.weight", ".attn.qkv.bias", ".attn.proj.weight", ".attn.proj.bias",
                                             ".norm2.weight", ".norm2.bias", ".mlp.fc1.weight", ".mlp.fc1.bias", ".mlp.fc2.weight", ".mlp.fc2.bias"};
  const int64_t w = W;
  const int64_t numel[12] = {w, w, 3 * w * w, 3 * w, w * w, w, w, w, 4 * w * w, 4 * w, 4 * w * w, w};
  for (int i = 0; i < 12; ++i) {
    names[i] = pre + (timm ? timm_names : clip_names)[i];
    net.add_param(names[i], numel[i]);
  }
}

void ClipBlock::lookup(NetBase& net) {
  float** const dst[12] = {&ln1g, &ln1b, &inw, &inb, &ow, &ob, &ln2g, &ln2b, &fcw, &fcb, &pjw, &pjb};
  for (int i = 0; i < 12; ++i) *dst[i] = net.P(names[i]);
}

int clip_block_fwd(NetBase& net, const ClipBlock& b, ClipActs& t, const float* x, float* xo, int N, int T, bool causal, hipStream_t s) {
  cgd_ctx* ctx = net.ctx;
  const int W = b.W;
  const long rows = (long)N * T;
  CGD_TRY(net.ensure(t.st1, rows * 2)); CGD_TRY(net.ensure(t.st2, rows * 2));
  CGD_TRY(net.ensure(t.y, rows * W)); CGD_TRY(net.ensure(t.qkv, rows * 3 * W)); CGD_TRY(net.ensure(t.a, rows * W));
  CGD_TRY(net.ensure(t.x1, rows * W)); CGD_TRY(net.ensure(t.y2, rows * W)); CGD_TRY(net.ensure(t.u, rows * 4 * W));
  CGD_TRY(net.ensure(t.ga, rows * 4 * W));
  CGD_TRY(cgd_launch_ln_fwd(ctx, x, W, t.y.p, W, (int)rows, W, b.ln1g, b.ln1b, b.eps, t.st1.p, s));
  CGD_TRY(cgd_launch_gemm(ctx, lin(t.y.p, W, b.inw, W, t.qkv.p, 3 * W, b.inb, nullptr, 0, rows, 3 * W), s));
  const AttnShape sh{N, b.heads, T, W / b.heads, W, 0, causal ? 1 : 0};
  CGD_TRY(net.attn_fwd(t.att, sh, t.qkv.p, 3 * W, t.a.p, W, s));
  CGD_TRY(cgd_launch_gemm(ctx, lin(t.a.p, W, b.ow, W, t.x1.p, W, b.ob, x, W, rows, W, 1), s));
  CGD_TRY(cgd_launch_ln_fwd(ctx, t.x1.p, W, t.y2.p, W, (int)rows, W, b.ln2g, b.ln2b, b.eps, t.st2.p, s));
  {
    // c_fc + QuickGELU / GELU (b.act): the activation runs in the GEMM's epilogue where hgemm2 takes the launch in one slice (u is kept
    // for the image tower's backward pass, ga feeds c_proj); otherwise the separate elementwise kernel
    GemmParams fc = lin(t.y2.p, W, b.fcw, W, t.u.p, 4 * W, b.fcb, nullptr, 0, rows, 4 * W);
    if (cgd_gemm_fuses_act(ctx, fc)) {
      fc.act_out = t.ga.p; fc.ld_act = 4 * W; fc.act = b.act;
      CGD_TRY(cgd_launch_gemm(ctx, fc, s));
    } else {
      CGD_TRY(cgd_launch_gemm(ctx, fc, s));
      CGD_TRY(cgd_launch_act_fwd(ctx, t.u.p, t.ga.p, rows * 4 * W, b.act, s));
    }
  }
  return cgd_launch_gemm(ctx, lin(t.ga.p, 4 * W, b.pjw, 4 * W, xo, W, b.pjb, t.x1.p, W, rows, W, 1), s);
}

namespace {

struct Layer : ClipBlock {
  float *inwT = 0, *owT = 0, *fcwT = 0, *pjwT = 0;
  ClipActs f;                                        // forward
  DevBuf xo;
  DevBuf dga, du, dy2, dx1, da, dqkv, dy, dx;        // backward
};

struct ViT : NetBase {
  cgd_vit_config cfg;
  int g = 0, L = 0, W = 0, PP = 0;
  std::vector<Layer> layers;
  float *convw = 0, *convwT = 0, *cls = 0, *pos = 0, *lnpre_g = 0, *lnpre_b = 0, *lnpost_g = 0, *lnpost_b = 0, *proj = 0, *projT = 0;
  int N = 0, layout = 0;
  bool have_fwd = false;
  int fwd_prec = 0;  // precision mode the saved activations of the last forward were computed under
  DevBuf cols, pe, tok, st_pre, x0, st_post, clsn, dclsn, dxl, dtok, dcols;

  int build();
  int finalize(hipStream_t s);
  int forward(const float* img, int layout, int N, float* emb, hipStream_t s);
  int dgrad(const float* demb, float* dimg, hipStream_t s);
};

int ViT::build() {
  g = cfg.resolution / cfg.patch;
  L = g * g + 1;
  W = cfg.width;
  PP = 3 * cfg.patch * cfg.patch;
  if (cfg.resolution % cfg.patch) CGD_FAIL(ctx, "vit: resolution must be a multiple of the patch size");
  if (W % cfg.heads || (W / cfg.heads) % 4) CGD_FAIL(ctx, "vit: bad head configuration");
  add_param("conv1.weight", (int64_t)W * PP);
  add_param("class_embedding", W);
  add_param("positional_embedding", (int64_t)L * W);
  add_param("ln_pre.weight", W);
  add_param("ln_pre.bias", W);
  layers.resize(cfg.layers);
  for (int l = 0; l < cfg.layers; ++l) layers[l].add_params(*this, "transformer.resblocks." + std::to_string(l), W, cfg.heads);
  add_param("ln_post.weight", W);
  add_param("ln_post.bias", W);
  add_param("proj", (int64_t)W * cfg.out_dim);
  return 0;
}

int ViT::finalize(hipStream_t s) {
  CGD_TRY(check_all_set());
  convw = P("conv1.weight"); cls = P("class_embedding"); pos = P("positional_embedding");
  lnpre_g = P("ln_pre.weight"); lnpre_b = P("ln_pre.bias");
  lnpost_g = P("ln_post.weight"); lnpost_b = P("ln_post.bias");
  proj = P("proj");
  CGD_TRY(transpose_weight(convw, &convwT, W, PP, s));
  CGD_TRY(transpose_weight(proj, &projT, W, cfg.out_dim, s));
  for (Layer& l : layers) {
    l.lookup(*this);
    CGD_TRY(transpose_weight(l.inw, &l.inwT, 3 * W, W, s));
    CGD_TRY(transpose_weight(l.ow, &l.owT, W, W, s));
    CGD_TRY(transpose_weight(l.fcw, &l.fcwT, 4 * W, W, s));
    CGD_TRY(transpose_weight(l.pjw, &l.pjwT, W, 4 * W, s));
  }
  CGD_HIP(ctx, hipStreamSynchronize(s));
  finalized = true;
  have_fwd = false;  // the saved activations belong to the previous weights
  return 0;
}

int ViT::forward(const float* img, int lay, int Nn, float* emb, hipStream_t s) {
  if (!finalized) CGD_FAIL(ctx, "vit: finalize() has not been called after the last set_param");
  N = Nn; layout = lay; have_fwd = false;
  fwd_prec = ctx->precision;
  const long rows = (long)N * L;
  const float* colp = img;
  if (layout == 0) {
    CGD_TRY(ensure(cols, (size_t)N * g * g * PP));
    CGD_TRY(cgd_launch_patchify(ctx, img, cols.p, N, cfg.resolution, cfg.patch, s));
    colp = cols.p;
  }
  CGD_TRY(ensure(pe, (size_t)N * g * g * W));
  CGD_TRY(ensure(tok, rows * W));
  CGD_TRY(ensure(x0, rows * W));
  CGD_TRY(ensure(st_pre, rows * 2));
  CGD_TRY(cgd_launch_gemm(ctx, lin(colp, PP, convw, PP, pe.p, W, nullptr, nullptr, 0, (long)N * g * g, W), s));
  CGD_TRY(cgd_launch_vit_tokens(ctx, pe.p, cls, pos, tok.p, N, L, W, s));
  CGD_TRY(cgd_launch_ln_fwd(ctx, tok.p, W, x0.p, W, (int)rows, W, lnpre_g, lnpre_b, 1e-5f, st_pre.p, s));
  const float* x = x0.p;
  for (Layer& l : layers) {
    CGD_TRY(ensure(l.xo, rows * W));
    CGD_TRY(clip_block_fwd(*this, l, l.f, x, l.xo.p, N, L, false, s));
    x = l.xo.p;
  }
  CGD_TRY(ensure(st_post, (size_t)N * 2));
  CGD_TRY(ensure(clsn, (size_t)N * W));
  CGD_TRY(cgd_launch_ln_fwd(ctx, x, L * W, clsn.p, W, N, W, lnpost_g, lnpost_b, 1e-5f, st_post.p, s));
  CGD_TRY(cgd_launch_gemm(ctx, lin(clsn.p, W, projT, W, emb, cfg.out_dim, nullptr, nullptr, 0, N, cfg.out_dim), s));
  have_fwd = true;
  return 0;
}

int ViT::dgrad(const float* demb, float* dimg, hipStream_t s) {
  if (!finalized) CGD_FAIL(ctx, "vit: finalize() has not been called after the last set_param");
  if (!have_fwd) CGD_FAIL(ctx, "vit: dgrad() needs a preceding forward()");
  // the saved activations and the attention scratch belong to the mode the forward ran under: refused here, before any launch
  if (fwd_prec != ctx->precision) CGD_FAIL(ctx, "vit: dgrad() under another precision mode than its forward()");
  const long rows = (long)N * L;
  const int H = cfg.heads, d = W / H;
  CGD_TRY(ensure(dclsn, (size_t)N * W));
  CGD_TRY(ensure(dxl, rows * W));
  // emb = clsn @ proj  ->  d clsn = demb @ proj^T : B = proj [W][out] is already [N=W][K=out]
  CGD_TRY(cgd_launch_gemm(ctx, lin(demb, cfg.out_dim, proj, cfg.out_dim, dclsn.p, W, nullptr, nullptr, 0, N, W), s));
  CGD_TRY(cgd_launch_fill(ctx, dxl.p, rows * W, 0.f, s));
  const float* xlast = layers.empty() ? x0.p : layers.back().xo.p;
  CGD_TRY(cgd_launch_ln_bwd(ctx, xlast, L * W, dclsn.p, W, dxl.p, L * W, nullptr, 0, N, W, lnpost_g, st_post.p, s));
  const float* dcur = dxl.p;
  for (int li = (int)layers.size() - 1; li >= 0; --li) {
    Layer& l = layers[li];
    const float* xin = li == 0 ? x0.p : layers[li - 1].xo.p;
    CGD_TRY(ensure(l.dga, rows * 4 * W)); CGD_TRY(ensure(l.du, rows * 4 * W)); CGD_TRY(ensure(l.dy2, rows * W));
    CGD_TRY(ensure(l.dx1, rows * W)); CGD_TRY(ensure(l.da, rows * W)); CGD_TRY(ensure(l.dqkv, rows * 3 * W));
    CGD_TRY(ensure(l.dy, rows * W)); CGD_TRY(ensure(l.dx, rows * W));
    // MLP
    {
      // d(c_proj) and the backward of the activation: du = (dcur @ W_proj) * gelu'(u), fused like the forward
      GemmParams pj = lin(dcur, W, l.pjwT, W, l.dga.p, 4 * W, nullptr, nullptr, 0, rows, 4 * W);
      if (cgd_gemm_fuses_act(ctx, pj)) {
        pj.C = l.du.p;
        pj.act_in = l.f.u.p; pj.ld_act = 4 * W; pj.act = l.act;
        CGD_TRY(cgd_launch_gemm(ctx, pj, s));
      } else {
        CGD_TRY(cgd_launch_gemm(ctx, pj, s));
        CGD_TRY(cgd_launch_act_bwd(ctx, l.f.u.p, l.dga.p, l.du.p, rows * 4 * W, l.act, s));
      }
    }
    CGD_TRY(cgd_launch_gemm(ctx, lin(l.du.p, 4 * W, l.fcwT, 4 * W, l.dy2.p, W, nullptr, nullptr, 0, rows, W, 1), s));
    CGD_TRY(cgd_launch_ln_bwd(ctx, l.f.x1.p, W, l.dy2.p, W, l.dx1.p, W, dcur, W, (int)rows, W, l.ln2g, l.f.st2.p, s));
    // attention
    CGD_TRY(cgd_launch_gemm(ctx, lin(l.dx1.p, W, l.owT, W, l.da.p, W, nullptr, nullptr, 0, rows, W), s));
    CGD_TRY(attn_bwd(l.f.att, AttnShape{N, H, L, d, W, 0, 0}, l.f.qkv.p, 3 * W, l.da.p, W, l.dqkv.p, 3 * W, s));
    CGD_TRY(cgd_launch_gemm(ctx, lin(l.dqkv.p, 3 * W, l.inwT, 3 * W, l.dy.p, W, nullptr, nullptr, 0, rows, W, 1), s));
    CGD_TRY(cgd_launch_ln_bwd(ctx, xin, W, l.dy.p, W, l.dx.p, W, l.dx1.p, W, (int)rows, W, l.ln1g, l.f.st1.p, s));
    dcur = l.dx.p;
  }
  CGD_TRY(ensure(dtok, rows * W));
  CGD_TRY(cgd_launch_ln_bwd(ctx, tok.p, W, dcur, W, dtok.p, W, nullptr, 0, (int)rows, W, lnpre_g, st_pre.p, s));
  // patch rows (token 0 is the class token): d cols[n] = dtok[n][1:] @ conv1.weight  (B = convwT [PP][W])
  float* dc = dimg;
  if (layout == 0) {
    CGD_TRY(ensure(dcols, (size_t)N * g * g * PP));
    dc = dcols.p;
  }
  // one weight GEMM over all N * L token rows whose epilogue drops the class-token row of every image (GemmParams::skip_group) where
  // the weight GEMM kernel takes the shape in one slice; otherwise N batched (L - 1)-row GEMMs on the generic kernel (patch 14: 588
  // columns are not a multiple of 32)
  GemmParams one = lin(dtok.p, W, convwT, W, dc, PP, nullptr, nullptr, 0, rows, PP);
  one.no_split = 1;
  if (cgd_gemm_fuses_act(ctx, one)) {
    one.skip_group = L;
    CGD_TRY(cgd_launch_gemm(ctx, one, s));
  } else {
    GemmParams p;
    p.A = dtok.p + W; p.lda = W; p.B = convwT; p.ldb = W; p.C = dc; p.ldc = PP; p.M = g * g; p.N = PP; p.K = W;
    p.nbatch = N; p.bdiv = 1; p.sA1 = (long)L * W; p.sC1 = (long)g * g * PP;
    CGD_TRY(cgd_launch_gemm(ctx, p, s));
  }
  if (layout == 0) CGD_TRY(cgd_launch_unpatchify(ctx, dcols.p, dimg, N, cfg.resolution, cfg.patch, s));
  return 0;
}

}  // namespace

struct cgd_vit {
  ViT net;
};

extern "C" {
int cgd_vit_create(cgd_ctx* ctx, const cgd_vit_config* cfg, cgd_vit** out) { return net_create(ctx, out, cfg); }
// host-only: OpenAI `visual.*` names without the prefix
int cgd_vit_manifest(const cgd_vit_config* cfg, void (*cb)(const char*, int64_t, void*), void* user) { return net_manifest<ViT>(cb, user, cfg); }
void cgd_vit_destroy(cgd_vit* v) { net_destroy(v); }
int cgd_vit_num_params(cgd_vit* v) { return net_num_params(v); }
int cgd_vit_param_info(cgd_vit* v, int i, char* buf, int len, int64_t* numel) { return net_param_info(v, i, buf, len, numel); }
int cgd_vit_set_param(cgd_vit* v, const char* name, const float* data, int64_t numel) { return net_set_param(v, name, data, numel); }
int cgd_vit_finalize(cgd_vit* v) { return net_finalize(v); }
int cgd_vit_set_activation(cgd_vit* v, int act) {
  if (!v) return -3;
  v->net.have_fwd = false;  // a dgrad after the switch needs a forward that ran with it
  return clip_set_activation(v->net.ctx, v->net.layers, act);
}
int cgd_vit_forward(cgd_vit* v, const float* img, int layout, int N, float* emb, void* stream) {
  return net_pass(v, stream, [&](hipStream_t s) { return v->net.forward(img, layout, N, emb, s); });
}
int cgd_vit_dgrad(cgd_vit* v, const float* d_emb, float* d_img, void* stream) {
  return net_pass(v, stream, [&](hipStream_t s) { return v->net.dgrad(d_emb, d_img, s); });
}
}
