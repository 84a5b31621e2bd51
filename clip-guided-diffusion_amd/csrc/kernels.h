// Host launchers of the non-GEMM kernels (internal).  All tensors fp32; activations NHWC / token-major with an
// explicit row stride so that channel slices of concat buffers can be read and written in place.
#pragma once
#include "common.h"

// ---- norm.hip ---------------------------------------------------------------------------------------------
size_t cgd_gn_scratch_floats(int B, int HW, int C);
// y = act(GN(x)*gamma+beta [*(1+scale)+shift]);  film = [B][ldfilm] rows (scale | shift, 2C used) or null;  act: 0 none, 1 SiLU.
// `scratch` (cgd_gn_scratch_floats) keeps the statistics and folded coefficients for the backward pass.
int cgd_launch_gn_fwd(cgd_ctx* ctx, const float* x, int ldx, float* y, int ldy, int B, int HW, int C, const float* gamma,
                      const float* beta, const float* film, int ldfilm, int act, float eps, float* scratch, hipStream_t s);
// y == nullptr: statistics and folded coefficients only; cgd_gn_ab() then locates the compact {a, b} pairs [B][C][2] with which
// the consumer applies y = act(x * a + b) itself (the halo conv kernel while it stages its input: the normalised tensor is never
// written).
const float* cgd_gn_ab(const float* scratch, int B, int HW, int C);
// the full folded coefficients {a, b, gcoef = gamma (1 + scale), mean} per (sample, channel) of a finished forward pass: what a dgrad conv's
// epilogue needs to take the norm's backward sums itself (GemmParams::gnb_coef)
const float* cgd_gn_coef(const float* scratch, int B, int HW, int C);
size_t cgd_gn_stats_offset(int B, int HW, int C);  // float offset of the {mean, rstd} pairs [B][32][2] inside the scratch
// dx = dGN/dx (dz) (+ add) (+ add2);  needs the forward's scratch.  add / add2: residual-path and skip-connection gradients
// that meet at this tensor (both optional, own row strides).
int cgd_launch_gn_bwd(cgd_ctx* ctx, const float* x, int ldx, const float* dz, int lddz, float* dx, int lddx, const float* add,
                      int ldadd, int B, int HW, int C, int act, float* scratch, hipStream_t s, const float* add2 = nullptr,
                      int ldadd2 = 0);
// The same for a GroupNorm + SiLU whose `add` operand is the weight GEMM `sk` (C = dx, same pixels: a ResBlock's 1x1 skip dgrad): ONE launch of
// that GEMM whose epilogue applies the norm's backward (GemmParams::gnf_*) instead of the GEMM, its dx write, the read-back and the apply pass.
// Only when the norm's backward sums come from epilogue records of the conv that produced dz and the GEMM kernel takes the operands
// (cgd_gemm_fuses_gnb); otherwise *done = false, nothing is launched and the caller runs the two launches.
int cgd_launch_gn_bwd_skip_gemm(cgd_ctx* ctx, GemmParams sk, const float* x, int ldx, const float* dz, int lddz, const float* add2, int ldadd2,
                                int B, int HW, int C, float* scratch, hipStream_t s, bool* done);
int cgd_launch_ln_fwd(cgd_ctx* ctx, const float* x, int ldx, float* y, int ldy, int rows, int C, const float* gamma,
                      const float* beta, float eps, float* stats, hipStream_t s);
int cgd_launch_ln_bwd(cgd_ctx* ctx, const float* x, int ldx, const float* dy, int lddy, float* dx, int lddx, const float* add,
                      int ldadd, int rows, int C, const float* gamma, const float* stats, hipStream_t s);

// ---- elem.hip ---------------------------------------------------------------------------------------------
// out[b,y,x,:] = scale * sum_{2x2} in[b,2y+i,2x+j,:] (+ add)
int cgd_launch_pool2x2(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, const float* add, int ldadd, int B, int Ho,
                       int Wo, int C, float scale, hipStream_t s);
// out[b,y,x,:] = scale * in[b,y/2,x/2,:] (+ add)
// two resamplings of equal shape in one launch: up = 0: 2 x 2 sums * scale, 1: nearest 2x * scale (elem.hip resample2x_pair_kernel)
int cgd_launch_resample2x_pair(cgd_ctx* ctx, int up, const float* in0, int ldi0, float* out0, int ldo0, const float* in1, int ldi1, float* out1,
                               int ldo1, int B, int Ho, int Wo, int C, float scale, hipStream_t s);
int cgd_launch_upsample2x(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, const float* add, int ldadd, int B, int Ho,
                          int Wo, int C, float scale, hipStream_t s);
// out = a (+ b), 2-D with row strides
int cgd_launch_copy2d(cgd_ctx* ctx, const float* a, int lda, const float* b, int ldb, float* out, int ldo, long rows, int C,
                      hipStream_t s);
// out[:, 0:Ca] = a, out[:, Ca:Ca+Cb] = b
int cgd_launch_concat2(cgd_ctx* ctx, const float* a, int lda, int Ca, const float* b, int ldb, int Cb, float* out, int ldo, long rows,
                       hipStream_t s);
// act: 1 SiLU, 2 QuickGELU, 3 exact (erf) GELU; any other code fails.   fwd: y = act(x);  bwd: dx = dy * act'(x)
int cgd_launch_act_fwd(cgd_ctx* ctx, const float* x, float* y, long n, int act, hipStream_t s);
int cgd_launch_act_bwd(cgd_ctx* ctx, const float* x, const float* dy, float* dx, long n, int act, hipStream_t s);
// batched transpose: out[z][c][r] = in[z][r][c]  (in: [R][ldi], out: [Cc][ldo]); pad columns r in [R, ldo) are zeroed
int cgd_launch_transpose(cgd_ctx* ctx, const float* in, int ldi, long si, float* out, int ldo, long so, int R, int Cc, int nb,
                         hipStream_t s);
// timestep embedding: out[b][0:half] = cos(t*freqs), out[b][half:] = sin(t*freqs); freqs = host-computed table [dim/2]
int cgd_launch_timestep_embedding(cgd_ctx* ctx, const float* t, const float* freqs, float* out, int B, int dim, hipStream_t s);
// out[b][:] += table[idx[b]][:]
int cgd_launch_embedding_add(cgd_ctx* ctx, const float* table, const int64_t* idx, float* out, int B, int dim, hipStream_t s);
// ViT token assembly: tok[n][0] = cls + pos[0]; tok[n][1+i] = patch[n][i] + pos[1+i]
int cgd_launch_vit_tokens(cgd_ctx* ctx, const float* patch, const float* cls, const float* pos, float* tok, int N, int L, int W,
                          hipStream_t s);
// im2col for the ViT patch conv (NCHW image -> [N*g*g][3*P*P]) and its adjoint
int cgd_launch_patchify(cgd_ctx* ctx, const float* img, float* cols, int N, int res, int P, hipStream_t s);
int cgd_launch_unpatchify(cgd_ctx* ctx, const float* cols, float* img, int N, int res, int P, hipStream_t s);
int cgd_launch_fill(cgd_ctx* ctx, float* p, long n, float v, hipStream_t s);
// h[b * HW + i][c] += e[b * lde + c]: a per-(sample, channel) vector added to every pixel, in place (the additive timestep embedding of a
// classic ResBlock); C, ldh and lde multiples of 4, h and e 16-byte aligned
int cgd_launch_add_chan(cgd_ctx* ctx, float* h, int ldh, const float* e, int lde, int B, int HW, int C, hipStream_t s);

// ---- sconv.hip: 3x3 convolution of stride 2, padding 1 (the classic UNet's Downsample) and its backward to the input ---------------------
// nullptr when the launchers below run the problem, else the reason they refuse it (host only).  ld_in: row stride of the gathered operand (x, or
// dy when dgrad), ld_out: of the written one (y / dx), ldadd: of the backward's add operand (0 = none); B, H, W: the input's
const char* cgd_sconv_refusal(int dgrad, int ld_in, int ld_out, int ldadd, int B, int H, int W, int Cin, int Cout);
// wf / wd: the two copies cgd_pack_conv3x3 leaves (net.h)
int cgd_launch_sconv_fwd(cgd_ctx* ctx, const float* x, int ldx, const float* wf, const float* bias, float* y, int ldy, int B, int H, int W, int Cin,
                         int Cout, hipStream_t s);
// dx (B, H, W, Cin) = conv^T dy (+ add): one launch, the pixel parity taken from the workgroup index; deterministic
int cgd_launch_sconv_dgrad(cgd_ctx* ctx, const float* dy, int lddy, const float* wd, float* dx, int lddx, const float* add, int ldadd, int B, int H,
                           int W, int Cin, int Cout, hipStream_t s);

// ---- attn.hip ---------------------------------------------------------------------------------------------
// in-place row softmax over the first T columns of [rows][ld]; columns [T, ld) are set to 0
int cgd_launch_softmax_rows(cgd_ctx* ctx, float* S, long rows, int T, int ld, hipStream_t s);
// in-place dS = P * (dP - rowsum(dP*P)) on dP
int cgd_launch_softmax_bwd_rows(cgd_ctx* ctx, const float* P, float* dP, long rows, int T, int ld, hipStream_t s);

struct AttnShape {
  int nb;      // independent sequences (batch)
  int heads;   // heads per sequence
  int T;       // tokens
  int d;       // head dim
  int C;       // = heads*d
  int legacy;  // 1: per-head [q|k|v] interleave (QKVAttentionLegacy); 0: [Q all heads | K | V]
  int causal;  // 1: key j > query i is masked (the CLIP text tower); forward only, cgd_attn_bwd refuses it
};
struct AttnBufs {     // all owned by the caller, sized by cgd_attn_buf_floats
  float* qkvT;        // [nb][3C][Tp]
  float* P;           // [nb*heads][T][Tp]   (saved for backward)
  float* Pt;          // [nb*heads][T][Tp]   (backward temp, also dS^T)
  float* dP;          // [nb*heads][T][Tp]
  float* dAt;         // [nb][C][Tp]
};
static inline int attn_tp(int T) { return (T + 3) & ~3; }
// floats of AttnBufs member `which` (0 qkvT, 1 P, 2 Pt, 3 dP, 4 dAt) for the kernel family the context runs this shape on (0 = not touched)
size_t cgd_attn_buf_floats(const cgd_ctx* ctx, const AttnShape& sh, int ldq, int ldo, int which);
// qkv: [nb*T][3C] token-major (row stride ldq);  out: [nb*T][C] (row stride ldo)
int cgd_attn_fwd(cgd_ctx* ctx, const AttnShape& sh, const float* qkv, int ldq, float* out, int ldo, const AttnBufs& bufs,
                 hipStream_t s);
// dout: [nb*T][C];  dqkv: [nb*T][3C] (fully overwritten)
int cgd_attn_bwd(cgd_ctx* ctx, const AttnShape& sh, const float* qkv, int ldq, const float* dout, int lddo, float* dqkv, int lddq,
                 const AttnBufs& bufs, hipStream_t s);

// attn_flash.hip (round 5): d = 64 or 80, T > 32 in bf16x3 contexts (T > 64 only at CGD_ATTN_FLASH=1); P is never materialised, bufs.P holds the row statistics (LSE | D),
// bufs.qkvT a copy of O for the backward's D = rowsum(dO * O).  qo / ko / vo / step: column offsets of head 0 and the per-head step
// (sh.causal: the causal instantiation)
int cgd_attn_flash_fwd(cgd_ctx* ctx, const AttnShape& sh, const float* qkv, int ldq, float* out, int ldo, const AttnBufs& bufs, long qo,
                       long ko, long vo, long step, hipStream_t s);
int cgd_attn_flash_bwd(cgd_ctx* ctx, const AttnShape& sh, const float* qkv, int ldq, const float* dout, int lddo, float* dqkv, int lddq,
                       const AttnBufs& bufs, long qo, long ko, long vo, long step, hipStream_t s);

// ---- guidance.hip -----------------------------------------------------------------------------------------
struct CutoutGeom {
  int oy, ox, h, w;  // crop origin and (possibly truncated) extent
};
// out layout 0: NCHW (cutn*B, 3, cs, cs), index = cut*B + b;  layout 1: ViT patch rows [(cut*B+b)*g*g + gy*g+gx][3*P*P]
int cgd_launch_cutouts_fwd(cgd_ctx* ctx, const float* x_in /*B,3,H,W in [-1,1]*/, const int* coords /*dev [cutn][4]*/,
                           float* out, int B, int H, int W, int cutn, int cs, int layout, int P, hipStream_t s);
// G[b,c,y,x] (+)= sum over cutouts of pooled-gradient scatter; dout has the forward's layout
int cgd_launch_cutouts_bwd(cgd_ctx* ctx, const float* dout, const int* coords, float* G /*B,3,H,W*/, int B, int H, int W, int cutn,
                           int cs, int layout, int P, int accumulate, hipStream_t s);
// cutaug.hip: cutouts with the `use_augs` augmentations between crop and pool (params: device float [cutn][16], the record of
// include/cgd_mi355x.h; noise: device float or null, noise_off: device int64 [cutn] offsets of each cutout's four (B,3,h,w) planes)
int cgd_launch_cutouts_aug_fwd(cgd_ctx* ctx, const float* x_in, const int* coords, const float* params, const float* noise,
                               const int64_t* noise_off, float* out, int B, int H, int W, int cutn, int cs, int layout, int P,
                               hipStream_t s);
// G[b,c,y,x] (+)= adjoint of the above (noise does not enter); scratch: cgd_cutouts_aug_scratch(B, H, W, cutn) floats
int cgd_launch_cutouts_aug_bwd(cgd_ctx* ctx, const float* dout, const int* coords, const float* params, float* G, float* scratch, int B,
                               int H, int W, int cutn, int cs, int layout, int P, int accumulate, hipStream_t s);
size_t cgd_cutouts_aug_scratch(int B, int H, int W, int cutn);
// host: per output pixel of an h x w crop, the affine nearest source index (-1: fill) and the perspective's 4 taps / weights
int cgd_aug_sample_map(const float* params, int h, int w, int32_t* affine_src, int32_t* persp_idx, float* persp_w);
// cutresize.hip: cutouts through the antialiased cubic resize (flags: device int32 [cutn], bit 0 luma before the resize, bit 1 flip along
// W after it); scratch: cgd_cutouts_resize_scratch(B, H, W, cutn) floats
int cgd_launch_cutouts_resize_fwd(cgd_ctx* ctx, const float* x_in, const int* coords, const int* flags, float* out, int B, int H, int W,
                                  int cutn, int cs, int layout, int P, hipStream_t s);
int cgd_launch_cutouts_resize_bwd(cgd_ctx* ctx, const float* dout, const int* coords, const int* flags, float* G, float* scratch, int B,
                                  int H, int W, int cutn, int cs, int layout, int P, int accumulate, hipStream_t s);
size_t cgd_cutouts_resize_scratch(int B, int H, int W, int cutn);
// host: weights [m][taps], first taps [m] and the tap count of an n -> m resize, from the routine the kernels run
int cgd_resize_weights(int n, int m, float* w, int32_t* left, int* taps);
// mask.hip: the merge of masked sampling after a sampler update (include/cgd_mi355x.h: cgd_masked_merge); sample and x0 (or null) are merged
// in place, x_re (with n_re, or both null) receives the merged sample taken back up one level
struct cgd_mask_coef;
int cgd_launch_masked_merge(cgd_ctx* ctx, float* sample, float* x0, const float* init, const float* mask, const float* n_known,
                            const float* n_re, float* x_re, int B, int H, int W, int init_batch, int mask_batch, int mask_channels,
                            const cgd_mask_coef& k, hipStream_t s);
// ilvr.hip: the low-frequency refinement of ILVR after a sampler update (include/cgd_mi355x.h: cgd_ilvr_refine); sample and x0 (or null) are
// refined in place; scratch: cgd_ilvr_scratch(B, H, W, factor, x0 != null) floats (0 for a shape or factor the launcher refuses)
int cgd_launch_ilvr_refine(cgd_ctx* ctx, float* sample, float* x0, const float* ref, const float* noise, float* scratch, int B, int H, int W,
                           int ref_batch, int factor, float sa, float sb, hipStream_t s);
long cgd_ilvr_scratch(int B, int H, int W, int factor, int with_x0);
// warp.hip: what 2D animation runs between two frames (include/cgd_mi355x.h: cgd_frame_warp, cgd_channel_stats, cgd_color_match).  The
// arguments are judged before the context is needed: a refused call returns -2 even with a null context, an accepted one -3 without one
struct cgd_warp;
int cgd_launch_frame_warp(cgd_ctx* ctx, const float* src, float* dst, int B, int C, int H, int W, const cgd_warp* w, hipStream_t s);
int cgd_launch_channel_stats(cgd_ctx* ctx, const float* x, float* stats, int B, int C, int H, int W, hipStream_t s);
int cgd_launch_color_match(cgd_ctx* ctx, float* x, const float* stats_x, const float* stats_ref, int ref_batch, float amount, int clamp, int B,
                           int C, int H, int W, hipStream_t s);
// warp3d.hip: the perspective warp of 3D animation (cgd_frame_warp3d); judged like the launchers of warp.hip, -2 before -3.  An identity
// camera goes to cgd_launch_frame_warp with the identity matrix
struct cgd_camera;
int cgd_launch_frame_warp3d(cgd_ctx* ctx, const float* src, float* dst, const float* depth, int depth_batch, int B, int C, int H, int W,
                            const cgd_camera* cam, hipStream_t s);
// depth.hip: the launcher behind cgd_op_resize_cubic (include/cgd_mi355x.h), for flow.hip's pyramid; needs a context
int cgd_launch_resize_cubic(cgd_ctx* ctx, const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, float a, float b, float lo,
                            int clamp_lo, hipStream_t s);
// window.hip: the adjoint pair of windowed sampling (include/cgd_mi355x.h: cgd_window_gather / cgd_window_merge); oy [ny], ox [nx]: host arrays of
// window origins; ay [ny][S], ax [nx][S]: device weight tables, both or neither (null = ones)
int cgd_launch_window_gather(cgd_ctx* ctx, const float* full, float* win, const int* oy, int ny, const int* ox, int nx, const float* ay,
                             const float* ax, int B, int C, int H, int W, int S, int wrap, hipStream_t s);
int cgd_launch_window_merge(cgd_ctx* ctx, const float* win, float* full, const int* oy, int ny, const int* ox, int nx, const float* ay,
                            const float* ax, int B, int C, int H, int W, int S, int wrap, int accumulate, hipStream_t s);
// invert.hip: the update of one DDIM inversion step (include/cgd_mi355x.h: cgd_ddim_reverse_update); eps is read in place from the model's
// 6-channel output, x0 and noise_out (with init) may be null
struct cgd_reverse_coef;
int cgd_launch_ddim_reverse_update(cgd_ctx* ctx, const float* x, const float* out6, const float* init, float* x_next, float* x0,
                                   float* noise_out, int B, int H, int W, int init_batch, const cgd_reverse_coef& k, hipStream_t s);
// spherical-distance loss and its gradient w.r.t. the cutout embeddings
//   emb [cutn*B][D] (row = cut*B + b), targets [P][D], weights [B][P] (dense per-sample prompt weights, see
//   host-side broadcast rules), loss_part: per-(cut,b) partial losses [cutn*B] (already * scale / cutn)
int cgd_launch_spherical_loss(cgd_ctx* ctx, const float* emb, const float* targets, const float* weights, float* demb,
                              float* loss_part, int cutn, int B, int P, int D, float scale, hipStream_t s);

// ---- classifier.hip: the head of the noisy ImageNet classifier (guided_diffusion.unet.AttentionPool2d + log-softmax-select) -------------
// h [B * S2][C] NHWC rows (the SiLU(GroupNorm) output) -> tokens [mean | h_0 .. h_{S2-1}] + positional embedding (T = S2 + 1) -> qkv_proj ->
// attention of token 0's query over all T keys per head (new order: [Q all heads | K | V]) -> c_proj -> logits -> log-softmax-select.
struct AttnPoolShape {
  int B, S2, C, d, out;  // samples, spatial positions, channels, head width (heads = C / d), classes
  int weight;            // 1: the weights are persistent (a network handle's): the GEMM launcher may cache packed copies of them
};
struct AttnPoolWeights {
  const float* posT;   // [T][C]: positional_embedding [C][T] transposed
  const float* qkvw;   // [3C][C]
  const float* qkvb;   // [3C]
  const float* qkvwT;  // [C][3C]
  const float* cw;     // [out][C]
  const float* cb;     // [out]
  const float* cwT;    // [C][outP], outP = out rounded up to 4, pad columns zero (cgd_attnpool_pack_cwT)
};
// floats of the scratch of one call shape (activations kept for the backward + the backward's temporaries)
size_t cgd_attnpool_scratch_floats(const AttnPoolShape& sh);
// the largest (T, d) the single-query attention kernels keep in LDS
bool cgd_attnpool_supported(int S2, int C, int d, int out);
int cgd_attnpool_pack_cwT(cgd_ctx* ctx, const float* cw, float* cwT, int out, int C, hipStream_t s);
// y [B] class ids; logits [B][out] or null; logp [B] or null (logp[b] = log_softmax(logits[b])[y[b]]); pooled [B][C] or null: the attention
// output of token 0 in front of c_proj
int cgd_attnpool_fwd(cgd_ctx* ctx, const AttnPoolShape& sh, const AttnPoolWeights& w, const float* h, int ldh, const int64_t* y, float* pooled,
                     float* logits, float* logp, float* scratch, hipStream_t s);
// dh [B * S2][C] (row stride lddh) = scale * d(sum_b logp[b]) / dh of the forward that filled `scratch`
int cgd_attnpool_bwd(cgd_ctx* ctx, const AttnPoolShape& sh, const AttnPoolWeights& w, float scale, float* dh, int lddh, float* scratch,
                     hipStream_t s);
// g += d (n floats, n a multiple of 4, 16-byte aligned)
int cgd_launch_accumulate(cgd_ctx* ctx, float* g, const float* d, long n, hipStream_t s);

// ---- gram.hip: per-sample Gram matrices of tall-skinny activations (the VGG style loss) ---------------------------------------------
// A [B * N][C] fp32 rows (row stride lda >= C, a multiple of 4; 16-byte aligned), C in {64, 128, 256, 512}, any N >= 1; exact fp32 products whatever the
// context precision; the slab partials live in the context's split-K workspace.
//   Gs == nullptr: out [B][C][C] = scale * A_b^T A_b
//   else         : out [B][C][C] = gk * (scale * A_b^T A_b - Gs) and lpart[b * lstride + i] = lw * (partial sums of (scale * A_b^T A_b - Gs)^2),
//                  i < cgd_gram_loss_parts(C)
int cgd_gram_loss_parts(int C);
int cgd_launch_gram(cgd_ctx* ctx, const float* A, int lda, int B, int N, int C, float scale, float* out, const float* Gs, float gk, float lw,
                    float* lpart, long lstride, hipStream_t s);
