/* libcgd_mi355x — C ABI of the MI355X-native CLIP-guided diffusion sampling step.
 *
 * The reference (afiaka87/clip-guided-diffusion) is pure Python and has NO native boundary; the per-timestep
 * hot path is reached through two Python callables handed to the sampler:
 *     model(x, timesteps, y)            /root/reference/cgd/cgd.py:251  (guided_diffusion UNetModel)
 *     cond_fn(x, t, out, y=None)        /root/reference/cgd/cgd.py:151-239, :255
 * and the sampler update of guided_diffusion's p_sample_with_grad / ddim_sample_with_grad selected at
 * /root/reference/cgd/cgd.py:242-245.  This header is the boundary a maintainer binds with ctypes
 * (INTEGRATION.md shows the stub); each entry point cites the reference code it replaces.
 *
 * Conventions: every pointer is a DEVICE pointer to fp32 unless stated; the caller (PyTorch-ROCm) owns all
 * I/O buffers; the library owns packed weights, saved activations and workspaces inside its handles; all work
 * is enqueued on the caller's stream (`stream` = hipStream_t, e.g. torch.cuda.current_stream().cuda_stream);
 * no hidden synchronisation; functions return 0 on success, non-zero on error and never throw —
 * cgd_last_error() returns the message.  Handles are single-threaded, one per GPU.
 */
#ifndef CGD_MI355X_H
#define CGD_MI355X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cgd_ctx cgd_ctx;
typedef struct cgd_unet cgd_unet;
typedef struct cgd_vit cgd_vit;

/* MFMA contraction precision (fp32 storage everywhere): 0 = fp32-input MFMA (exact), 1 = bf16x3 split
 * (~fp32 accuracy, default), 2 = single bf16 product (the reference's CUDA path runs the nets in fp16). */
enum { CGD_F32 = 0, CGD_BF16X3 = 1, CGD_BF16 = 2 };

int cgd_ctx_create(cgd_ctx** out, int device);
void cgd_ctx_destroy(cgd_ctx* ctx);
const char* cgd_last_error(cgd_ctx* ctx);
int cgd_set_precision(cgd_ctx* ctx, int mode);
int cgd_get_precision(cgd_ctx* ctx);
/* read-only: device allocations made since context creation on behalf of network passes (activation buffers and weight copies of every handle,
 * the packed-weight cache, the conv-epilogue record buffers).  A handle that has seen its largest shape must leave it unchanged. */
int64_t cgd_ctx_device_allocs(cgd_ctx* ctx);
const char* cgd_version(void);
/* tuning knob: GEMM tile codes for the automatic selection (64, 128, 256 = 256x128, 257 = 128x256; +1000 = 2-deep prefetch) */
int cgd_set_tiles(cgd_ctx* ctx, int large_tile, int small_tile);
/* tuning knob: weight GEMM kernel (hgemm.hip): mode 0 off / 1 auto, smallest M, 64-column chunks per split-K slice (0 = keep) */
int cgd_set_hgemm(cgd_ctx* ctx, int mode, int min_m, int min_chunks);
/* HIP-event timing of the profiled launches on their own stream (measurement only; bench.py roofline / hbm legs).
 * cgd_profile_read: out[3k .. 3k+2] = {summed ms, algorithmic work, launches} of kind k: 0 = igemm_kernel / hgemm_kernel launches
 * incl. their split-K reduce [FLOP], 1 = hconv2_kernel launches alone [FLOP], 2 = GroupNorm forward / backward ops, all launches
 * of one norm [algorithmic HBM bytes], 3 = wconv_kernel launches alone (the dominant kernel) [FLOP], 4 = kconv_kernel launches alone
 * (the weight-streaming conv kernel of the <= 32x32-pixel maps) [FLOP], 5 = the wconv_kernel launches that carry a GroupNorm-backward
 * epilogue (a subset of kind 3) [FLOP]: 3 * cgd_profile_kinds() = 18 doubles; synchronises the device and resets. */
int cgd_profile(cgd_ctx* ctx, int enable);
int cgd_profile_read(cgd_ctx* ctx, double* out18);
/* number of kinds k above (the buffer of cgd_profile_read holds 3 * cgd_profile_kinds() doubles) */
int cgd_profile_kinds(void);
/* measurement: process-wide counters since the library was loaded: out2[0] = kernel launches, out2[1] = split-K reduce launches
 * among them (bench.py: launches_per_step / splitk_reduce_per_step) */
int cgd_launch_counts(unsigned long long* out2);

/* ---- UNet epsilon/sigma predictor: replaces guided_diffusion.unet.UNetModel built at
 *      /root/reference/cgd/script_util.py:316 from /root/reference/data/diffusion_model_flags.py ---- */
typedef struct cgd_unet_config {
  int image_size;
  int model_channels;
  int num_res_blocks;
  int n_mult;
  float channel_mult[8];
  int n_att;
  int attention_ds[8];     /* downsample rates that carry attention (image_size // attention_resolution) */
  int num_classes;         /* 0 = unconditional */
  int num_heads;
  int num_head_channels;   /* -1: use num_heads */
  int use_new_attention_order;
  int in_channels;         /* 3, or 6: a super-resolution UNet, x (3) + the upsampled low-resolution image (3) */
  int out_channels;        /* 6 (learn_sigma) */
  /* The classic architecture of improved-diffusion / guided-diffusion's defaults.  0 for both is the architecture of the published
   * guided-diffusion checkpoints, and what a zero-initialised struct gets. */
  int classic_resample;    /* 1: resblock_updown = False, conv_resample = True: Downsample is a 3x3 conv of stride 2 (input_blocks.K.0.op),
                              Upsample nearest 2x + a 3x3 conv (output_blocks.K.J.conv) */
  int additive_emb;        /* 1: use_scale_shift_norm = False: the timestep embedding is added to conv1's output (emb_layers.1 has cout rows) */
} cgd_unet_config;

/* host-only (no GPU, no context): the parameter manifest of a configuration — cb(name, numel, user) per parameter in upload order,
 * returns the count (negative: invalid configuration).  The same for the other networks below.  Used by the CPU tests of checkpoint
 * ingestion (names and shapes of all published checkpoints against the oracle networks). */
typedef void (*cgd_manifest_cb)(const char* name, int64_t numel, void* user);
int cgd_unet_manifest(const cgd_unet_config* cfg, cgd_manifest_cb cb, void* user);
int cgd_unet_create(cgd_ctx* ctx, const cgd_unet_config* cfg, cgd_unet** out);
void cgd_unet_destroy(cgd_unet* u);
/* parameter ingestion, names = upstream state-dict keys (model.load_state_dict at script_util.py:317);
 * `data` may be a host or device pointer.
 * Streams (this and every other cgd_*_set_param / cgd_*_finalize below): they take no stream, run on the NULL stream and are
 * host-synchronous — the copy and the packing are complete on return.  The null stream is not ordered with streams created
 * non-blocking (every PyTorch stream is), so a device `data` must be COMPLETE before set_param is called — synchronise the stream
 * that produced it, a dtype conversion enqueued just before included — and no pass of the handle may be in flight on any stream
 * between the first set_param and the return of finalize.  (nets._Net.load_state_dict drains the caller's current stream once
 * before its first set_param.) */
int cgd_unet_num_params(cgd_unet* u);
int cgd_unet_param_info(cgd_unet* u, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_unet_set_param(cgd_unet* u, const char* name, const float* data, int64_t numel);
int cgd_unet_finalize(cgd_unet* u); /* pack fwd + dgrad (rotated/transposed) weight layouts */
/* model(x, timesteps, y): x (B,3,H,W) NCHW, timesteps (B) fp32 (already mapped/rescaled), y (B) int64 or NULL
 * -> out (B,6,H,W) NCHW.  Keeps the activations the backward pass needs. */
int cgd_unet_forward(cgd_unet* u, const float* x, const float* timesteps, const int64_t* y, float* out, int B, int H, int W,
                     void* stream);
/* Round 6: the embedding head of model(x, t, y) — timestep embedding, time_embed MLP, class embedding, ALL FiLM projections — depends on (t, y)
 * only.  cgd_unet_embed computes it into one of two buffers (slot 0 / 1) on `stream`; cgd_unet_forward_slot is cgd_unet_forward reading that
 * buffer.  The sampler runs embed for step n + 1 on a side stream while step n computes (eight small dependent launches off the critical path).
 * The caller orders embed(slot) -> forward_slot(slot) -> next embed(slot) with events; embed calls are stream-ordered among themselves; call it
 * only between whole passes of the context (between a forward and its dgrad is fine), never inside one and never from another host thread. */
int cgd_unet_embed(cgd_unet* u, const float* timesteps, const int64_t* y, int B, int slot, void* stream);
int cgd_unet_forward_slot(cgd_unet* u, const float* x, int slot, float* out, int B, int H, int W, void* stream);
/* d(sum(out * g_out))/dx of the LAST forward: replaces the UNet leg of th.autograd.grad(loss, x), cgd.py:228 */
int cgd_unet_dgrad(cgd_unet* u, const float* g_out, float* g_x, void* stream);
/* Super-resolution handles (in_channels 6; guided-diffusion's SuperResModel): the low-resolution image low (B_low,3,h,w) NCHW in [-1,1],
 * B_low 1 or the batch of the later forwards, is copied (stream-ordered) into a buffer the handle owns and conditions every later
 * cgd_unet_forward / cgd_unet_forward_slot until it is replaced: those take x (B,3,H,W) as on a 3-channel handle, upsample the image
 * bilinearly to (H, W) and run the stem on cat([x, upsampled]) in one launch (cgd_op_sr_stem); they fail when no image is set or
 * B_low is neither 1 nor B.  cgd_unet_dgrad still returns (B,3,H,W): only d/dx exists.  Refused on a 3-channel handle. */
int cgd_unet_set_low_res(cgd_unet* u, const float* low, int B_low, int h, int w, void* stream);

/* ---- CLIP image tower (VisionTransformer): replaces clip_model.encode_image, cgd/cgd.py:194 ---- */
typedef struct cgd_vit_config {
  int resolution, patch, width, layers, heads, out_dim;
} cgd_vit_config;
int cgd_vit_manifest(const cgd_vit_config* cfg, cgd_manifest_cb cb, void* user);
int cgd_vit_create(cgd_ctx* ctx, const cgd_vit_config* cfg, cgd_vit** out);
void cgd_vit_destroy(cgd_vit* v);
int cgd_vit_num_params(cgd_vit* v);
int cgd_vit_param_info(cgd_vit* v, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_vit_set_param(cgd_vit* v, const char* name, const float* data, int64_t numel);
int cgd_vit_finalize(cgd_vit* v);
/* activation between c_fc and c_proj of every block: 2 QuickGELU x sigmoid(1.702 x) (the default: OpenAI's checkpoints), 3 exact GELU
 * 0.5 x (1 + erf(x / sqrt 2)) (the open_clip / LAION checkpoints).  Any time after create; another value returns -2 (cgd_last_error). */
int cgd_vit_set_activation(cgd_vit* v, int act);
/* layout 0: img (N,3,res,res) NCHW; layout 1: patch rows [N*g*g][3*patch*patch] (what cgd_cutouts_fwd layout 1 writes) */
int cgd_vit_forward(cgd_vit* v, const float* img, int layout, int N, float* emb /* (N,out_dim) */, void* stream);
int cgd_vit_dgrad(cgd_vit* v, const float* d_emb, float* d_img /* same layout as the forward input */, void* stream);

/* ---- CLIP text tower (clip.model.CLIP.encode_text): token embedding + positional embedding, `layers` pre-LN residual blocks with CAUSAL
 *      self-attention, ln_final on the end-of-text row of each sequence (the first maximal token id, CLIP's EOT convention), @ text_projection.
 *      Replaces the `clip` package's text transformer behind encode_text_prompt (cgd/clip_util.py).  Forward only; runs in the context's
 *      precision mode.  Parameter names are the OpenAI top-level keys: token_embedding.weight, positional_embedding,
 *      transformer.resblocks.{l}.* (the image tower's block names), ln_final.{weight,bias}, text_projection (W x out_dim, x @ text_projection). ---- */
typedef struct cgd_text cgd_text;
typedef struct cgd_text_config {
  int context_length, vocab_size, width, layers, heads, out_dim;
} cgd_text_config;
int cgd_text_manifest(const cgd_text_config* cfg, cgd_manifest_cb cb, void* user);
int cgd_text_create(cgd_ctx* ctx, const cgd_text_config* cfg, cgd_text** out);
void cgd_text_destroy(cgd_text* t);
int cgd_text_num_params(cgd_text* t);
int cgd_text_param_info(cgd_text* t, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_text_set_param(cgd_text* t, const char* name, const float* data, int64_t numel);
int cgd_text_finalize(cgd_text* t);
int cgd_text_set_activation(cgd_text* t, int act); /* as cgd_vit_set_activation */
/* tokens: DEVICE int64 (N, context_length), ids in [0, vocab_size) (an id outside that range reads nothing and makes its row NaN);
 * emb: (N, out_dim) */
int cgd_text_forward(cgd_text* t, const int64_t* tokens, int N, float* emb, void* stream);

/* ---- CLIP image tower, ModifiedResNet variant (RN50 / RN101; clip_util.py:17): same role as the ViT tower.  Parameters use
 *      the OpenAI `visual.*` names including the BatchNorm running statistics (folded into the convolutions by finalize).
 *      img: (N,3,res,res) NCHW, CLIP-normalised. ---- */
typedef struct cgd_rn cgd_rn;
typedef struct cgd_rn_config {
  int resolution, width, layers[4], out_dim, heads;
} cgd_rn_config;
int cgd_rn_manifest(const cgd_rn_config* cfg, cgd_manifest_cb cb, void* user);
int cgd_rn_create(cgd_ctx* ctx, const cgd_rn_config* cfg, cgd_rn** out);
void cgd_rn_destroy(cgd_rn* v);
int cgd_rn_num_params(cgd_rn* v);
int cgd_rn_param_info(cgd_rn* v, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_rn_set_param(cgd_rn* v, const char* name, const float* data, int64_t numel);
int cgd_rn_finalize(cgd_rn* v);
int cgd_rn_forward(cgd_rn* v, const float* img, int N, float* emb /* (N,out_dim) */, void* stream);
int cgd_rn_dgrad(cgd_rn* v, const float* d_emb, float* d_img /* (N,3,res,res) */, void* stream);
/* Test support, not on the product path (no reference counterpart): mask replay.  The post-ReLU activations saved by the last
 * forward (call order: stem relu1..3, then relu1, relu2, relu3 of every Bottleneck; [3P] clip/model.py ModifiedResNet) can be
 * overwritten with the oracle's ([rows][channels] NHWC rows on the device), so that cgd_rn_dgrad takes the oracle's ReLU masks and
 * the rest of the backward chain is graded at the literal tolerance (tests/parity_checks.py check_resnet_mask_replay). */
int cgd_rn_debug_relu_count(cgd_rn* v);
int cgd_rn_debug_relu_info(cgd_rn* v, int index, int64_t* rows, int* channels);
int cgd_rn_debug_relu_set(cgd_rn* v, int index, const float* src, void* stream);

/* ---- LPIPS-VGG16 init loss: replaces lpips.LPIPS(net='vgg') (cgd/cgd.py:147-148) and `lpips_vgg(x_in, init_tensor)` with its
 *      backward to x_in (cgd.py:220-224,228).  Parameters use the package's names (net.slice{k}.{idx}.weight|bias,
 *      lin{k}.model.1.weight).  set_reference: the fixed second argument (init image, (B,3,H,W) NCHW in [-1,1], H and W
 *      multiples of 16).  loss_grad: loss[b] = lpips(x_b, ref_b);  g (B,3,H,W) (+)= grad_scale * d(sum_b loss_b)/dx. ---- */
typedef struct cgd_lpips cgd_lpips;
int cgd_lpips_manifest(cgd_manifest_cb cb, void* user);
int cgd_lpips_create(cgd_ctx* ctx, cgd_lpips** out);
void cgd_lpips_destroy(cgd_lpips* v);
int cgd_lpips_num_params(cgd_lpips* v);
int cgd_lpips_param_info(cgd_lpips* v, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_lpips_set_param(cgd_lpips* v, const char* name, const float* data, int64_t numel);
int cgd_lpips_finalize(cgd_lpips* v);
int cgd_lpips_set_reference(cgd_lpips* v, const float* ref_nchw, int B, int H, int W, void* stream);
int cgd_lpips_loss_grad(cgd_lpips* v, const float* x_nchw, float grad_scale, float* loss /* [B] */, float* g_nchw, int accumulate,
                        void* stream);
/* Test support, not on the product path: mask replay.  acts = 13 device pointers (post-ReLU activations conv1_1 .. conv5_3 of the
 * image the NEXT cgd_lpips_loss_grad call is given, [B*h_l*w_l][cout_l] NHWC rows) or NULL to switch it off: the trunk pass of that
 * call continues from these activations, so taps, ReLU masks and max-pool arg-max are the caller's (the oracle's). */
int cgd_lpips_debug_replay(cgd_lpips* v, const float* const* acts);
/* VGG Gram-matrix style term on the same trunk (Gatys et al.; Johnson et al.).  For tap k of sample b, A_k = the post-ReLU activation [N_k][C_k]
 * (N_k = H_k W_k; C_k = 64, 128, 256, 512, 512):
 *   G_k(x)[b] = A_k^T A_k / (C_k N_k),   L_style[b] = sum_k lambda_k |G_k(x)[b] - G_k(style)|_F^2.
 * set_style: ONE style image (1,3,Hs,Ws) NCHW in [-1,1], Hs and Ws multiples of 16 but otherwise free (a Gram matrix does not depend on the frame);
 * lambda[5] >= 0, a tap with lambda 0 is skipped everywhere.  A reference set by cgd_lpips_set_reference stays intact.
 * style_loss_grad: one trunk forward, both heads, one trunk backward: x (B,3,H,W);  style_loss[b] = L_style[b];
 * g (B,3,H,W) (+)= lpips_grad_scale * d(sum_b lpips_b)/dx + style_grad_scale * d(sum_b L_style[b])/dx.  lpips_loss [B] or NULL: NULL gives the style
 * term alone and needs no reference; otherwise (B, H, W) must be the reference's.  g may not alias x.  cgd_lpips_debug_replay applies to this call too. */
int cgd_lpips_set_style(cgd_lpips* v, const float* style_nchw, int Hs, int Ws, const float* lambda /* [5] */, void* stream);
int cgd_lpips_style_loss_grad(cgd_lpips* v, const float* x_nchw, int B, int H, int W, float lpips_grad_scale, float style_grad_scale,
                              float* lpips_loss /* [B] or NULL */, float* style_loss /* [B] */, float* g_nchw, int accumulate, void* stream);

/* ---- Secondary diffusion model (SecondaryDiffusionImageNet2 of Katherine Crowson's CLIP-guided diffusion notebooks / Disco Diffusion): a
 *      small convolutional denoiser that predicts the clean image for the guidance losses, so that their gradient returns to x through ~50
 *      GFLOP of 3x3 convolutions instead of through the UNet (no reference counterpart: the reference differentiates the UNet).
 *      Parameters use the module's state-dict names (net.0.0.weight ... net.4.bias, timestep_embed.weight [8][1]).  x (B,3,H,W) NCHW, H and W
 *      multiples of 32 (anything else fails, -2, before any launch); t (B) device fp32 in [0,1]: the model's own time, atan2(sigma, alpha) 2/pi.
 *        forward:       pred = x cos(t pi/2) - v sin(t pi/2), v = net(cat(x, Fourier planes of t)); keeps the activations for dgrad
 *        forward_blend: the same, and x_in = pred fac + x (1 - fac) in the head's launch
 *        dgrad:         dx (B,3,H,W) = d(sum(v * dv_seed))/dx of the LAST forward; dv_seed (B,3,H,W).  The caller chains pred and x_in
 *                       (cgd_secondary_combine).  Fails (-2) without a forward since the last finalize / failed forward.
 *      The trunk always runs on exact-fp32 products (as LPIPS). ---- */
typedef struct cgd_secondary cgd_secondary;
int cgd_secondary_manifest(cgd_manifest_cb cb, void* user);
int cgd_secondary_create(cgd_ctx* ctx, cgd_secondary** out);
void cgd_secondary_destroy(cgd_secondary* v);
int cgd_secondary_num_params(cgd_secondary* v);
int cgd_secondary_param_info(cgd_secondary* v, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_secondary_set_param(cgd_secondary* v, const char* name, const float* data, int64_t numel);
int cgd_secondary_finalize(cgd_secondary* v);
int cgd_secondary_forward(cgd_secondary* v, const float* x, const float* t, int B, int H, int W, float* pred, void* stream);
int cgd_secondary_forward_blend(cgd_secondary* v, const float* x, const float* t, int B, int H, int W, float fac, float* pred, float* x_in,
                                void* stream);
int cgd_secondary_dgrad(cgd_secondary* v, const float* dv_seed, float* dx, void* stream);
/* Test support, not on the product path: mask replay.  acts = 23 device pointers (post-ReLU activations of the 23 ConvBlocks in execution
 * order, [B*h_l*w_l][cout_l] dense NHWC rows, for the input the following forward calls are given) or NULL to switch it off: each forward
 * continues from these activations, so the ReLU masks of its dgrad are the caller's (the oracle's). */
int cgd_secondary_debug_replay(cgd_secondary* v, const float* const* acts);
/* the head alone (what forward / forward_blend launch last): v, x, pred, x_in (or NULL) (B,3,H,W), 16-byte aligned */
int cgd_secondary_head(cgd_ctx* ctx, const float* v, const float* x, const float* t, float fac, float* pred, float* x_in, int B, int H, int W,
                       void* stream);
/* The secondary-path counterpart of cgd_guidance_combine.  g_in = dL/dx_in of the CLIP / LPIPS legs (or NULL); the tv and saturation terms
 * are taken on x_in, the range term on pred.  With G_in = g_in + tv + sat and G_pred = fac G_in + range:
 *   g_direct = (1 - fac) G_in + alpha G_pred  (dL/dx not through the net);  seed3 = -sigma G_pred  (dL/dv, the seed of cgd_secondary_dgrad);
 * loss_part [cgd_guidance_part_blocks][3] = partial (tv, range, sat) losses.  cgd_grad_finish / cgd_scalars take it from there. */
int cgd_secondary_combine(cgd_ctx* ctx, const float* g_in, const float* x_in, const float* pred, float* g_direct, float* seed3,
                          float* loss_part, int B, int H, int W, float fac, float alpha, float sigma, float tv_scale, float range_scale,
                          float sat_scale, void* stream);
/* single ops of the secondary model, exported for parity tests.  pack: NCHW x + the 16 Fourier planes [cos f | sin f], f = 2 pi t[b]
 * embed_weight[j] -> NHWC rows [B*H*W][32] (channels 0..2 x, 3..18 the planes, 19..31 zero).  bilinear_up2x (align_corners = False):
 * adjoint 0: in [B][Hi][Wi] rows of C channels at stride ldi -> out [B][2Hi][2Wi] rows at stride ldo; adjoint 1: in = gradient of the
 * (2Hi, 2Wi) map at stride ldi -> out = gradient of the (Hi, Wi) map at stride ldo (gather form).  C and the strides multiples of 4,
 * pointers 16-byte aligned, or the call fails (-2) before anything is launched. */
int cgd_op_secondary_pack(cgd_ctx* ctx, const float* x, const float* t, const float* embed_weight, float* out, int B, int H, int W,
                          void* stream);
int cgd_op_bilinear_up2x(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, int B, int Hi, int Wi, int C, int adjoint,
                         void* stream);

/* ---- DPT-Large (MiDaS v3: dpt_large-midas-2f21e586.pt), the depth network of 3D animation; forward only (csrc/depth.hip).  Parameter names
 *      are the checkpoint's own (pretrained.model.*, pretrained.act_postprocess{1..4}.*, scratch.*); the groups the forward does not use
 *      (pretrained.model.norm / head, scratch.refinenet4.resConfUnit1) are not part of the manifest.  DPT-Large is
 *      {16, 1024, 24, 16, {5, 11, 17, 23}, 24, 256, {256, 512, 1024, 1024}}.  create refuses (-2) what the kernels cannot run: channel counts
 *      that are no multiples of 32, a head dim other than 64 or 80, hooks that are not increasing block indices.
 *   set_pos_embed   the position embedding [(1 + gh gw)][width] (class row first; host or device memory) of a token grid other than the
 *                   native one, resized by the caller (bilinear, align_corners = False, on the grid part); kept per grid.
 *   forward         img (B,3,H,W) NCHW fp32, already normalised, H and W multiples of 32 -> inv_depth (B,1,H,W) and / or
 *                   depth = max((offset - inv_depth) / scale, floor) (either may be NULL, not both).  Anything else fails (-2) before any
 *                   launch, as does a grid without a position embedding.
 *   debug_map       test support: the reassembled map of tap k = 0..3 of the last forward (in front of layer{k+1}_rn) as dense NHWC rows;
 *                   out3 = {height, width, channels}; out == NULL only reports the shape. */
typedef struct cgd_depth cgd_depth;
typedef struct cgd_depth_config {
  int patch, width, layers, heads, hooks[4], native_grid, features, reassemble_channels[4];
} cgd_depth_config;
int cgd_depth_manifest(const cgd_depth_config* cfg, cgd_manifest_cb cb, void* user);
int cgd_depth_create(cgd_ctx* ctx, const cgd_depth_config* cfg, cgd_depth** out);
void cgd_depth_destroy(cgd_depth* v);
int cgd_depth_num_params(cgd_depth* v);
int cgd_depth_param_info(cgd_depth* v, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_depth_set_param(cgd_depth* v, const char* name, const float* data, int64_t numel);
int cgd_depth_finalize(cgd_depth* v);
int cgd_depth_set_pos_embed(cgd_depth* v, int gh, int gw, const float* data);
int cgd_depth_forward(cgd_depth* v, const float* img, int B, int H, int W, float offset, float scale, float floor, float* inv_depth,
                      float* depth, void* stream);
int cgd_depth_debug_map(cgd_depth* v, int k, float* out, int* out3, void* stream);
/* measurement support (benchmarks/depth_step.py): after_backbone != 0 makes every later forward return behind the last hooked block, writing
 * no output; 0 restores the whole forward */
int cgd_depth_debug_stop(cgd_depth* v, int after_backbone);
/* single ops of the depth network, exported for parity tests.  All work on NHWC rows (C and the row strides multiples of 4, pointers 16-byte
 * aligned) unless stated otherwise and fail (-2) before anything is launched when an argument breaks a rule.
 *   relu_rows         out = relu(in) on [rows][C] views (out may be in)
 *   bilinear_up2x_ac  align_corners = True: in [B][Hi][Wi] -> out [B][2Hi][2Wi] (+ add, of out's shape, or NULL); output o reads the source
 *                     position o (n - 1) / (2n - 1); n = 1 is a copy
 *   conv_transpose    ConvTranspose2d with kernel = stride = k in {2, 4}: w [Cin][Cout][k][k] as torch stores it, bias [Cout] or NULL, Cin and
 *                     Cout multiples of 32; wpack (Cin Cout k k floats) and g (B H W Cout k k floats) are scratch
 *   depth_readout     DPT's ProjectReadout: tok [B (L + 1)][W] (class token first), w [W][2W], bias [W] -> out [B L][W] =
 *                     GELU(w [tok_i | cls] + bias); tmp (B (L + 1) W floats) and clsv (B W floats) are scratch; W a multiple of 32
 *   depth_head_tail   x [rows][32] (stride ldx) -> inv_depth[r] = relu(bias[0] + sum_c w[c] act(x[r][c])), act = ReLU when relu_in;
 *                     depth[r] = max((offset - inv_depth[r]) / scale, floor); either output may be NULL
 *   resize_cubic      `planes` dense (Hi, Wi) planes -> (Ho, Wo): out = a * resize(in) + b (clamp_lo: max(., lo) of that) with the antialiased cubic weights of the resized
 *                     cutouts, the taps outside the image read at the nearest edge pixel; one launch, gather form; an identical size copies
 *                     (bit-identical for a = 1, b = 0); at most an 8-fold reduction per axis */
int cgd_op_relu_rows(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, int64_t rows, int C, void* stream);
int cgd_op_bilinear_up2x_ac(cgd_ctx* ctx, const float* in, int ldi, float* out, int ldo, const float* add, int ldadd, int B, int Hi, int Wi,
                            int C, void* stream);
int cgd_op_conv_transpose(cgd_ctx* ctx, const float* x, int ldx, const float* w, const float* bias, float* out, int ldo, float* wpack,
                          float* g, int B, int H, int W, int Cin, int Cout, int k, void* stream);
int cgd_op_depth_readout(cgd_ctx* ctx, const float* tok, const float* w, const float* bias, float* out, float* tmp, float* clsv, int B,
                         int L, int W, void* stream);
int cgd_op_depth_head_tail(cgd_ctx* ctx, const float* x, int ldx, const float* w, const float* bias, float* inv_depth, float* depth,
                           int64_t rows, int relu_in, float offset, float scale, float floor, void* stream);
int cgd_op_resize_cubic(cgd_ctx* ctx, const float* in, float* out, int planes, int Hi, int Wi, int Ho, int Wo, float a, float b,
                        float lo, int clamp_lo, void* stream);

/* ---- Noisy ImageNet classifier of guided-diffusion (EncoderUNetModel with pool="attention": 64x64_classifier.pt ... 512x512_classifier.pt):
 *      the encoder half of the ADM UNet (time_embed, input_blocks, middle_block: same ResBlocks and legacy-order AttentionBlocks, no label_emb,
 *      no output blocks), then out.0 (GroupNorm32) -> SiLU -> out.2 (AttentionPool2d: positional_embedding (C, S*S+1), qkv_proj, c_proj; new
 *      attention order, token 0 kept), S = image_size / 2^(n_mult-1), heads = C / num_head_channels.  Classifier guidance adds
 *      scale * d(sum_b log p(y_b | x_b, t_b))/dx to the guidance gradient.  Parameters use the module's state-dict names.
 *        forward: x (B,3,H,W) NCHW with H = W = image_size (anything else fails, -2, before any launch), timesteps (B) fp32, y (B) int64 ->
 *                 logits (B,out_channels) (or NULL) and, if logp != NULL, logp[b] = log_softmax(logits[b])[y[b]] (NaN for a y outside the
 *                 classes); keeps the activations for dgrad
 *        dgrad:   g_x (B,3,H,W) (+)= scale * d(sum_b logp[b])/dx of the LAST forward; accumulate 0 / 1
 *      A configuration the conv kernels or the pool kernels cannot run is refused at create (-2). ---- */
typedef struct cgd_classifier cgd_classifier;
typedef struct cgd_classifier_config {
  int image_size;
  int model_channels;
  int num_res_blocks;
  int n_mult;
  float channel_mult[8];
  int n_att;
  int attention_ds[8];
  int num_head_channels;
  int out_channels;        /* 1000 */
} cgd_classifier_config;
int cgd_classifier_manifest(const cgd_classifier_config* cfg, cgd_manifest_cb cb, void* user);
int cgd_classifier_create(cgd_ctx* ctx, const cgd_classifier_config* cfg, cgd_classifier** out);
void cgd_classifier_destroy(cgd_classifier* c);
int cgd_classifier_num_params(cgd_classifier* c);
int cgd_classifier_param_info(cgd_classifier* c, int index, char* name_buf, int buf_len, int64_t* numel);
int cgd_classifier_set_param(cgd_classifier* c, const char* name, const float* data, int64_t numel);
int cgd_classifier_finalize(cgd_classifier* c);
int cgd_classifier_forward(cgd_classifier* c, const float* x, const float* timesteps, const int64_t* y, float* logits, float* logp, int B, int H,
                           int W, void* stream);
int cgd_classifier_dgrad(cgd_classifier* c, float scale, float* g_x, int accumulate, void* stream);
/* The classifier's head alone, exported for parity tests and benchmarks.  h [B*S*S][C] dense NHWC rows (the SiLU(GroupNorm) output), the four
 * parameters as the checkpoint holds them, y (B) int64 -> pooled [B][C] (token 0 of the attention output in front of c_proj; or NULL),
 * logits [B][out] (or NULL), logp [B] (or NULL).  scratch: cgd_op_attnpool_scratch_floats floats, 16-byte aligned; it keeps what the backward
 * needs.  bwd: dh [B*S*S][C] = scale * d(sum_b logp[b])/dh of the forward that filled `scratch` (same weights, same shape). */
int64_t cgd_op_attnpool_scratch_floats(int B, int S, int C, int d, int out);
int cgd_op_attnpool_fwd(cgd_ctx* ctx, const float* h, const float* pos, const float* qkv_w, const float* qkv_b, const float* c_w, const float* c_b,
                        const int64_t* y, float* pooled, float* logits, float* logp, float* scratch, int B, int S, int C, int d, int out,
                        void* stream);
int cgd_op_attnpool_bwd(cgd_ctx* ctx, const float* qkv_w, const float* qkv_b, const float* c_w, const float* c_b, float scale, float* dh,
                        float* scratch, int B, int S, int C, int d, int out, void* stream);

/* ---- cutouts: replaces MakeCutouts.forward (cgd/modules.py:50-66) + x.add(1).div(2) (cgd.py:190) + CLIP_NORMALIZE
 *      (clip_util.py:45).  coords: device int32 [cutn][4] = (oy, ox, h, w) of each (possibly truncated) crop. ---- */
int cgd_cutouts_fwd(cgd_ctx* ctx, const float* x_in, const int32_t* coords, float* out, int B, int H, int W, int cutn, int cut_size,
                    int layout, int patch, void* stream);
int cgd_cutouts_bwd(cgd_ctx* ctx, const float* d_out, const int32_t* coords, float* g_in, int B, int H, int W, int cutn,
                    int cut_size, int layout, int patch, int accumulate, void* stream);

/* ---- augmented cutouts (`use_augs`, the reference's modules.py:13-24 between the crop and the pool): per cutout k and sample b, in [0,1]
 *      space, z1 = flip((x_in crop + 1) / 2) + n1; z2 = nearest affine(z1) + n2; z3 = (bilinear perspective(z2) or z2) + n3;
 *      z4 = (3-channel grayscale(z3) or z3) + n4; out = (adaptive_avg_pool(z4, cut_size) - mean) / std, layouts as cgd_cutouts_fwd.
 *      Resampling fills 0 in [0,1] space; source coordinates follow grid_sample(align_corners=False) in float32 (nearest: half to even).
 *      params: device float [cutn][16] per cutout:
 *        [0] flip (1: flip along W)   [1] float32(cos a)   [2] float32(sin a)   [3] tx   [4] ty   (a = rotation angle, clockwise)
 *        [5] perspective (1: on)      [6..13] float32 homography coefficients c0..c7 (output pixel centre -> input, as torchvision's
 *                                             perspective coefficients)       [14] grayscale (1: on)   [15] unused (0)
 *      noise: device float or NULL (no noise); noise_off: device int64 [cutn], float offset into `noise` of cutout k's four
 *      consecutive (B,3,h,w) planes n1..n4 (h, w = the crop's extent).  The adjoint is deterministic (gather form, no atomics) and
 *      needs `scratch` of cgd_cutouts_aug_scratch_floats(B, H, W, cutn) floats. ---- */
int cgd_cutouts_aug_fwd(cgd_ctx* ctx, const float* x_in, const int32_t* coords, const float* params, const float* noise,
                        const int64_t* noise_off, float* out, int B, int H, int W, int cutn, int cut_size, int layout, int patch,
                        void* stream);
int cgd_cutouts_aug_bwd(cgd_ctx* ctx, const float* d_out, const int32_t* coords, const float* params, float* g_in, float* scratch, int B,
                        int H, int W, int cutn, int cut_size, int layout, int patch, int accumulate, void* stream);
int64_t cgd_cutouts_aug_scratch_floats(int B, int H, int W, int cutn); /* host-only */
/* host-only, test support: for every output pixel p = i*w + j of an h x w crop with the HOST record `params` (16 floats), the affine's
 * nearest source index affine_src[p] (-1: fill) and the perspective's bilinear taps persp_idx[4p..4p+3] (nw, ne, sw, se; -1: fill) and
 * weights persp_w[4p..4p+3] (0 for a fill tap), whatever the record's flags say */
int cgd_op_aug_sample_map(const float* params, int h, int w, int32_t* affine_src, int32_t* persp_idx, float* persp_w);

/* ---- resized cutouts (the overview + inner cut scheme of the CLIP-guided-diffusion notebooks): per cutout k and sample b, in [0,1] space,
 *      z = (x_in[b, :, oy:oy+h, ox:ox+w] + 1) / 2; z = 3-channel grayscale(z) if flags[k] & 1 (ITU-R 601-2 luma, as the augmented cutouts);
 *      r = Wy z Wx^T per channel; r = flip along W (r) if flags[k] & 2; out = (r - mean) / std, layouts as cgd_cutouts_fwd.
 *      W (m x n, m = cut_size, n = the crop's extent along the axis, s = m / n) is ResizeRight's antialiased cubic resize with zero padding:
 *      centre c_o = ((2o+1) n - m) / (2m); k(d) = cubic(d), support S = 4 for s >= 1, k(d) = s cubic(s d), S = 4n / m for s < 1;
 *      T = ceil(S) taps j = left_o .. left_o + T - 1, left_o = ceil(c_o - S / 2); w_oj = k(c_o - j) / sum of k over all T taps (a zero
 *      sum divides by 1).  Taps outside [0, n) read zero (black in [0,1] space), whatever the image holds beyond the box, and the weights
 *      are not renormalised over the taps inside: rows at the box border sum to less than 1.  m == n is the identity.  left_o, T and the tap
 *      distances are integer arithmetic, the cubic polynomial float32.
 *      coords as above, every box with h, w >= 1 inside the image (the table lives on the device: callers check it before the upload; a
 *      box that is not reads nothing, gives a NaN row and no gradient); flags: device int32 [cutn].  Host-checkable arguments (sizes,
 *      cut_size not a multiple of patch in layout 1, an image whose weight rows do not fit the LDS) fail with -2 before any launch.
 *      The adjoint is deterministic (gather form, no atomics) and needs `scratch` of cgd_cutouts_resize_scratch_floats(B, H, W, cutn)
 *      floats; accumulate as in cgd_cutouts_bwd. ---- */
int cgd_cutouts_resize_fwd(cgd_ctx* ctx, const float* x_in, const int32_t* coords, const int32_t* flags, float* out, int B, int H, int W,
                           int cutn, int cut_size, int layout, int patch, void* stream);
int cgd_cutouts_resize_bwd(cgd_ctx* ctx, const float* d_out, const int32_t* coords, const int32_t* flags, float* g_in, float* scratch, int B,
                           int H, int W, int cutn, int cut_size, int layout, int patch, int accumulate, void* stream);
int64_t cgd_cutouts_resize_scratch_floats(int B, int H, int W, int cutn); /* host-only */
/* host-only, test support: the weights of an n -> m resize from the routine the kernels run: *taps = T; w [m][T] and left [m] when both are
 * given (both NULL: only *taps, to size them) */
int cgd_cutouts_resize_weights(int n, int m, float* w, int32_t* left, int* taps);

/* ---- losses.spherical_dist_loss (cgd/losses.py:10-14) weighted as at cgd.py:196-204, with its gradient.
 *      emb (cutn*B, D) row = cut*B+b; targets_n (P, D) L2-normalised; weights (B, P) dense per-sample prompt
 *      weights; d_emb (cutn*B, D); loss_part (cutn*B) partial losses (sum = 'CLIP Loss'). ---- */
int cgd_spherical_loss(cgd_ctx* ctx, const float* emb, const float* targets_n, const float* weights, float* d_emb, float* loss_part,
                       int cutn, int B, int P, int D, float clip_guidance_scale, void* stream);

/* ---- directional CLIP loss of a prompt-pair edit, with its gradient.  emb (cutn*B, D) row = cut*B+b: the generated image;
 *      src_emb (cutn*Bs, D), Bs = 1 or B, row = cut*Bs + (Bs == 1 ? 0 : b): the source image through the same cutout (no gradient);
 *      dirs_n (P, D) L2-normalised text directions; weights (B, P) dense, zero columns are skipped.  With e^ = e / max(|e|, 1e-12),
 *      s^ likewise, delta = e^ - s^, n = |delta| and cos_p = delta . d_p / n (0 when n <= 1e-6: such a row has no gradient),
 *      loss_part[cut*B+b] = c sum_p w_bp (1 - cos_p), c = clip_guidance_scale / cutn, and d_emb (cutn*B, D) is set to (accumulate 0) or
 *      increased by (accumulate 1: the spherical launch of the same step wrote it) d loss_part / d emb.  D > 2048, Bs other than 1 or B,
 *      a count below 1 or a null pointer fail with -2 before any launch. ---- */
int cgd_directional_loss(cgd_ctx* ctx, const float* emb, const float* src_emb, const float* dirs_n, const float* weights, float* d_emb,
                         float* loss_part, int cutn, int B, int Bs, int P, int D, float clip_guidance_scale, int accumulate, void* stream);

/* ---- region prompts: both losses with every prompt weighted by its mask's share of the row's cutout.
 *      A region is an 8-bit mask m of the frame's size H x W (the size of x; offsets and windows included), 255 inside and 0 outside.  Its
 *      summed-area table S is (H+1, W+1) int32: row 0 and column 0 are zero, S[y][x] = sum of m over rows < y and columns < x.  sat holds the
 *      R tables one after the other.  geo is the step's cutout table as the cutters upload it: only its first cutn rows (oy, ox, h, w) are read.
 *      For the box of cut k and table r
 *          cov[k, r] = (S[oy+h][ox+w] - S[oy][ox+w] - S[oy+h][ox] + S[oy][ox]) / (255 h w)
 *      with the numerator in integer arithmetic (exact) and one float32 division; cov = 0 when h w == 0.  A corner outside the frame is clamped
 *      to it (callers upload boxes inside the frame; the clamp only keeps the reads inside the table).  region_of (P) int32 names prompt p's
 *      table, or -1 for "everywhere" (cov = 1); power (P) float32 > 0.  The effective weight of row cut * B + b is
 *          w_eff[cut, b, p] = weights[b, p] * cov[cut, region_of[p]] ** power[p]
 *      (the power is not evaluated when it is exactly 1), and everything else is as in the plain entries: c = clip_guidance_scale / cutn,
 *      the layout of the partials, accumulate, and the n <= 1e-6 rule of the directional loss.
 *      Skipping: a column with w_eff == 0 is skipped and its target / direction row is not read, exactly as a zero weight is in the plain
 *      entries.  A row whose every column is skipped has loss 0 and gradient bits all zero; under accumulate = 1 it is left untouched.  There
 *      is no renormalisation per cutout: a cut that sees no region contributes nothing.
 *      One launch of one wavefront per embedding row, as the plain entries; the coverage is computed in the kernel, once per prompt.
 *      region_of_host is the caller's host copy of region_of.  A null pointer, R < 1, a region_of_host entry outside [-1, R), D > 2048, a
 *      count below 1, or a frame with 255 H W >= 2^31 (the table is int32) fail with -2 before any launch. ---- */
int cgd_spherical_loss_regions(cgd_ctx* ctx, const float* emb, const float* targets_n, const float* weights, float* d_emb, float* loss_part,
                               int cutn, int B, int P, int D, float clip_guidance_scale, const int32_t* sat, const int32_t* region_of,
                               const int32_t* region_of_host, const float* power, const int32_t* geo, int R, int H, int W, void* stream);
int cgd_directional_loss_regions(cgd_ctx* ctx, const float* emb, const float* src_emb, const float* dirs_n, const float* weights, float* d_emb,
                                 float* loss_part, int cutn, int B, int Bs, int P, int D, float clip_guidance_scale, int accumulate,
                                 const int32_t* sat, const int32_t* region_of, const int32_t* region_of_host, const float* power,
                                 const int32_t* geo, int R, int H, int W, void* stream);
/* test and benchmark support: out (cutn, P) = cov[k, region_of[p]] ** power[p] from the device function the two losses use (1 where
 * region_of[p] is -1); the same -2 cases */
int cgd_op_region_coverage(cgd_ctx* ctx, const int32_t* sat, const int32_t* region_of, const int32_t* region_of_host, const float* power,
                           const int32_t* geo, float* out, int cutn, int P, int R, int H, int W, void* stream);

/* ---- aesthetic-predictor guidance (the LAION aesthetic predictors on the CLIP image embedding), with its gradient.  emb (cutn*B, D)
 *      row = cut*B+b; head (D + 1): the predictor collapsed to one vector a (D) followed by its bias beta.  With e^ = e / max(|e|, 1e-12),
 *      s = a . e^ + beta (the predicted score of the cutout) and c = scale / cutn:
 *          loss_part[cut*B+b] = -c s        score[cut*B+b] = s  (score may be NULL: it is then not written)
 *      and d_emb (cutn*B, D) is set to (accumulate 0: every element is written) or increased by (accumulate 1: the spherical or directional
 *      launch of the same step wrote it; one float addition per element) d loss_part / d emb = -c (a - (a . e^) e^) / max(|e|, 1e-12).
 *      A row of exact zeros has s = beta and no gradient: zero bits under accumulate 0, left untouched under accumulate 1.  scale may be
 *      negative (steers away from what the predictor rates highly).  One wavefront per row, reductions in a fixed order: repeated calls are
 *      bit-identical.  D > 2048, a count below 1, or a null emb, head, d_emb or loss_part fail with -2 before any launch
 *      (and before the context is needed: without one a well-formed call returns -3). ---- */
int cgd_aesthetic_loss(cgd_ctx* ctx, const float* emb, const float* head, float* d_emb, float* loss_part, float* score, int cutn, int B,
                       int D, float scale, int accumulate, void* stream);

/* per-timestep scalars of the (respaced) diffusion process, float64 tables evaluated on the host */
typedef struct cgd_step_coef {
  float sqrt_recip;             /* sqrt(1/abar_t)                                  */
  float sqrt_recipm1;           /* sqrt(1/abar_t - 1)                              */
  float coef1, coef2;           /* posterior_mean_coef1/2                          */
  float min_log, max_log;       /* posterior_log_variance_clipped[t], log(beta_t)  */
  float fac;                    /* sqrt(1-abar)[current_timestep] (cgd.py:177)     */
  float sqrt_one_minus_ab;      /* sqrt(1-abar_t)            (DDIM)                */
  float sqrt_ab_prev;           /* sqrt(abar_{t-1})          (DDIM)                */
  float sqrt_one_minus_ab_prev; /* sqrt(1-abar_{t-1})        (DDIM, eta=0)         */
  int nonzero;                  /* t != 0                                          */
} cgd_step_coef;

/* p_mean_variance tail (epsilon-pred, LEARNED_RANGE, clip_denoised=False) + blend x_in (cgd.py:177-179) */
int cgd_pmv_blend(cgd_ctx* ctx, const float* x, const float* model_out6, float* pred_xstart, float* mean, float* log_variance,
                  float* x_in, int B, int H, int W, const cgd_step_coef* k, void* stream);
/* number of per-block partial entries the two kernels below write */
int cgd_guidance_part_blocks(int B, int H, int W);
/* tv_loss / range_loss / saturation gradients (losses.py:5-7,17-22; cgd.py:201-218) chained through the blend and
 * x0 = a*x - b*eps:  g_direct (B,3,H,W) = dL/dx not through the UNet; seed6 (B,6,H,W) = dL/d(model_out);
 * loss_part [blocks][3] = partial (tv, range, sat) losses.  g_clip_in = dL_clip/dx_in from cgd_cutouts_bwd or NULL. */
int cgd_guidance_combine(cgd_ctx* ctx, const float* g_clip_in, const float* x_in, const float* pred_xstart, float* g_direct,
                         float* seed6, float* loss_part, int B, int H, int W, const cgd_step_coef* k, float tv_scale,
                         float range_scale, float sat_scale, void* stream);
/* g = -(g_direct + g_unet) (cgd.py:228); g_part [blocks][2] = partial (sum g, sum g^2) */
int cgd_grad_finish(cgd_ctx* ctx, const float* g_direct, const float* g_unet, float* g, float* g_part, int B, int H, int W,
                    void* stream);
/* scalars[8] = {CLIP, TV, Range, Sat, Total loss, Magnitude, Grad mean, magnitude clamp factor} (log keys of cgd.py:208-233) */
int cgd_scalars(cgd_ctx* ctx, const float* clip_part, int n_clip, const float* loss_part, const float* g_part, int B, int H, int W,
                int use_magnitude, float* scalars, void* stream);
/* mode 0: p_sample_with_grad + condition_mean_with_grad; mode 1: ddim_sample_with_grad + condition_score_with_grad (eta 0).
 * g may be NULL (no guidance); scalars (from cgd_scalars) carries the magnitude clamp factor, or NULL. */
int cgd_sample_update(cgd_ctx* ctx, const float* x, const float* pred_xstart, const float* mean, const float* log_variance,
                      const float* g, const float* noise, const float* scalars, float* sample, float* pred_xstart_out, int B, int H,
                      int W, const cgd_step_coef* k, int mode, void* stream);

/* ---- multistep samplers: PLMS (guided_diffusion's plms_sample, pseudo linear multistep of Liu et al., ICLR 2022) and DDIM with
 *      eta > 0 (ddim_sample_with_grad's sigma term).  One call = the whole update after one guided evaluation at (x_eval, k):
 *        eps0 = (a x_eval - pred_xstart) / b ; eps1 = eps0 - sqrt(1-abar) g ; x0c = a x_eval - b eps1 ; eps = (a x_eval - x0c) / b
 *      (a = sqrt_recip, b = sqrt_recipm1 of k; g scaled by scalars[7] when scalars is given, as in cgd_sample_update), then per phase:
 *        0 Adams-Bashforth: eps_out = eps; eps' = AB_order(eps, eps_hist[0] (newest), eps_hist[1], eps_hist[2]) with the weights
 *          1 | (3, -1)/2 | (23, -16, 5)/12 | (55, -59, 37, -9)/24; x0' = a x - b eps'; mean = sqrt(abar_prev) x0' + sqrt(1-abar_prev) eps';
 *          sample = t != 0 ? mean : x0c; pred_xstart_out = pred_xstart (the unconditioned prediction)
 *        1 start-step predictor: eps_out = eps; sample = sqrt(abar_prev) x0c + sqrt(1-abar_prev) eps (the input of the corrector's
 *          evaluation at t-1); pred_xstart_out = pred_xstart
 *        2 start-step corrector (the evaluation ran at x_eval = the predictor, k = coefficients of t-1): eps' = (eps_hist[0] + eps) / 2,
 *          then mean as in phase 0 from x with k_step (coefficients of t, t != 0 required) -> sample; eps_out and pred_xstart_out unused
 *        3 DDIM with eta: sample = sqrt(abar_prev) x0c + dir eps + [t != 0] sigma noise; pred_xstart_out = pred_xstart
 *      x_eval may be NULL (= x) and k_step NULL (= k) except in phase 2.  Returns -2 (cgd_last_error) for a phase outside 0..3, an order
 *      outside 1..4 in phase 0, or a missing buffer the phase needs. ---- */
typedef struct cgd_multistep {
  int phase;   /* 0 Adams-Bashforth, 1 start predictor, 2 start corrector, 3 DDIM with eta                          */
  int order;   /* phase 0: terms combined, 1..4 (this evaluation's eps and order-1 history entries)               */
  float sigma; /* phase 3: eta sqrt((1-abar_prev)/(1-abar)) sqrt(1 - abar/abar_prev)                                */
  float dir;   /* phase 3: sqrt(1 - abar_prev - sigma^2), the coefficient of eps in the mean                        */
} cgd_multistep;
int cgd_multistep_update(cgd_ctx* ctx, const float* x, const float* x_eval, const float* pred_xstart, const float* g,
                         const float* scalars, const float* noise, const float* const eps_hist[3], float* eps_out, float* sample,
                         float* pred_xstart_out, int B, int H, int W, const cgd_step_coef* k, const cgd_step_coef* k_step,
                         const cgd_multistep* m, void* stream);

/* ---- DPM-Solver++(2M) (Lu et al., 2022: data prediction, multistep; deterministic and SDE): the whole update after one guided evaluation
 *      at (x, k), from level t to level t-1, in one launch.  With x0c the guided pred_xstart exactly as in cgd_multistep_update,
 *        eps0 = (a x - pred_xstart) / b ; eps1 = eps0 - sqrt(1-abar) g ; x0c = a x - b eps1
 *      (a = sqrt_recip, b = sqrt_recipm1 of k; g scaled by scalars[7] when scalars is given; g may be NULL):
 *        D               = c_r != 0 ? x0c + c_r (x0c - x0_hist) : x0c          (x0_hist: the x0c_out of the step before)
 *        sample          = t != 0 ? c_x x + c_d D (+ c_n noise when c_n != 0) : x0c     (a select: nothing is multiplied at the clean end)
 *        x0c_out         = x0c                                                 (the next step's x0_hist)
 *        pred_xstart_out = pred_xstart                                         (the unconditioned prediction)
 *      alpha = sqrt(abar), sigma = sqrt(1-abar), lambda = log(alpha / sigma), h = lambda_{t-1} - lambda_t, eta = 0 (ODE) or > 0 (SDE):
 *        c_x = sigma_{t-1} / sigma_t e^(-eta h) ; c_d = -alpha_{t-1} expm1(-(1 + eta) h) ; c_n = sigma_{t-1} sqrt(-expm1(-2 eta h)) ;
 *        c_r = h / (2 h_last), h_last = lambda_t - lambda_{t+1}, for a second-order step, 0 for a first-order one
 *      (first order: DDIM with the same eta for eta in {0, 1}); at t == 0, where h is infinite: c_x = 0, c_d = 1, c_n = c_r = 0.
 *      x, pred_xstart, g, noise, x0_hist and the outputs: (B,3,H,W).  x, pred_xstart and sample are required; x0c_out and pred_xstart_out
 *      may be NULL and are then not written; x0_hist is read only when c_r != 0, noise only when c_n != 0 and t != 0.  Any
 *      4-byte-aligned pointers and any H * W are accepted (16-byte accesses when every pointer is 16-byte aligned and 4 | H * W).
 *      Returns -2 (cgd_last_error), before any launch, for a non-positive size, a missing required buffer, c_r != 0 without x0_hist,
 *      c_n != 0 at t != 0 without noise, or an output that aliases x or another output. ---- */
typedef struct cgd_dpmpp {
  float c_x; /* coefficient of x                                                         */
  float c_d; /* coefficient of D, the (extrapolated) guided pred_xstart                  */
  float c_r; /* second order: h / (2 h_last), the weight of x0c - x0_hist in D; else 0   */
  float c_n; /* SDE: coefficient of the step noise; 0 for the deterministic solver       */
} cgd_dpmpp;
int cgd_dpmpp_update(cgd_ctx* ctx, const float* x, const float* pred_xstart, const float* g, const float* scalars, const float* noise,
                     const float* x0_hist, float* x0c_out, float* sample, float* pred_xstart_out, int B, int H, int W,
                     const cgd_step_coef* k, const cgd_dpmpp* d, void* stream);

/* ---- dynamic thresholding of the guided pred_xstart under DPM-Solver++ (Saharia et al., 2022; Lu et al., 2022).  Per sample b, with
 *      a_b = |x0c_b| flattened to n = 3 H W values (|-0| = +0) and v_j the j-th smallest of them:
 *        q_b = v_k + (v_{k+1} - v_k) frac      (torch.quantile's 'linear' rule: pos = p (n - 1), k = floor(pos), frac = pos - k, computed by
 *                                               the host in float64; k + 1 is clamped to n - 1)
 *        s_b = min(max(q_b, floor), cap)       (floor = 1 and cap = +inf: dynamic thresholding; cap == floor: the static clip to +-cap)
 *        x0t = clamp(x0c, -s_b, s_b) / s_b     (a true division)
 *      and x0t takes x0c's place in cgd_dpmpp_update: D = c_r != 0 ? x0t + c_r (x0t - x0_hist) : x0t; sample = t != 0 ? c_x x + c_d D
 *      (+ c_n noise) : x0t; x0c_out = x0t (so x0_hist is the x0t of the step before); pred_xstart_out = pred_xstart.
 *      v_k and v_{k+1} are exact: radix selection on the bit patterns with the sign cleared, integer histograms per workgroup, partial counts
 *      in `scratch` summed in a fixed order by the next launch, no synchronisation between workgroups inside a launch; the same bits on every
 *      run.  A row that holds a non-finite value does not fault and does not disturb the other rows; its own result is unspecified.
 *      cgd_abs_quantile_scratch_bytes: bytes of `scratch` for B rows of n values (host only; -1 for a non-positive size or n > 2^31 - 1);
 *      cgd_abs_quantile_slice: the values one workgroup counts (a row runs on ceil(n / slice) workgroups).
 *      cgd_op_abs_quantile: the selection on a plain array v [B][n]; out3 [B][3] = {v_k, v_{k+1}, s}.  Five launches.
 *      cgd_dpmpp_threshold: the first launch computes x0c from x, pred_xstart, g and scalars exactly as cgd_dpmpp_update does and WRITES it
 *      to x0c (B,3,H,W); the later launches and cgd_dpmpp_update_thr read that buffer, so the selected and the clamped values are the same
 *      bits.  thr3 [B][3] = {v_k, v_{k+1}, s}.  With cap == floor every s_b is cap: one launch writes x0c and thr3 = {0, 0, cap}, nothing is
 *      selected and scratch may be NULL.  x0c may not alias x, pred_xstart or g.
 *      cgd_dpmpp_update_thr: cgd_dpmpp_update with x0c read from the buffer and s_b from thr3[b * 3 + 2] in device memory (the host never
 *      reads it); one launch.  The same optional buffers and aliasing rules as cgd_dpmpp_update; in addition x0c may not alias any output.
 *      Any 4-byte-aligned pointers and any sizes are accepted (16-byte accesses when every pointer is 16-byte aligned and 4 | n, 4 | H * W).
 *      All return -2 (cgd_last_error), before any launch, for a non-positive size, k outside [0, n), frac outside [0, 1], cap < floor, a
 *      missing required buffer or missing scratch, or an aliased output. ---- */
int64_t cgd_abs_quantile_scratch_bytes(int B, int64_t n);
int cgd_abs_quantile_slice(void);
int cgd_op_abs_quantile(cgd_ctx* ctx, const float* v, int B, int64_t n, int64_t k, float frac, float floor, float cap, float* out3,
                        void* scratch, void* stream);
int cgd_dpmpp_threshold(cgd_ctx* ctx, const float* x, const float* pred_xstart, const float* g, const float* scalars, float* x0c, int B,
                        int H, int W, const cgd_step_coef* k_coef, int64_t k, float frac, float floor, float cap, float* thr3, void* scratch,
                        void* stream);
int cgd_dpmpp_update_thr(cgd_ctx* ctx, const float* x, const float* pred_xstart, const float* x0c, const float* thr3, const float* noise,
                         const float* x0_hist, float* x0c_out, float* sample, float* pred_xstart_out, int B, int H, int W,
                         const cgd_step_coef* k_coef, const cgd_dpmpp* d, void* stream);

/* ---- masked sampling (inpainting / outpainting of an init image): the merge after a sampler update at step index t, in one launch.
 *      The update left `sample` (the state at level t-1) and `pred_xstart`; with m = mask (1 regenerate, 0 keep the init image):
 *        known       = sqrt(abar_prev) init + sqrt(1 - abar_prev) n_known   (two rounded products and a rounded sum, not fused)
 *        sample      = m == 0 ? known : m == 1 ? sample      : m sample      + (1 - m) known
 *        pred_xstart = m == 0 ? init  : m == 1 ? pred_xstart : m pred_xstart + (1 - m) init
 *      both in place.  The endpoints are selects: where m == 0 nothing of sample / pred_xstart reaches the output, non-finite values
 *      included; where m == 1 the two keep their bits.  With n_re and x_re the launch also writes the merged sample taken back up one
 *      level (RePaint's resampling with jump length 1): x_re = renoise_x sample + renoise_n n_re.
 *      sample, pred_xstart, n_known, n_re, x_re: (B,3,H,W); init: (init_batch,3,H,W), init_batch 1 or B; mask: (mask_batch,
 *      mask_channels,H,W), mask_batch 1 or B, mask_channels 1 or 3.  pred_xstart may be NULL; n_known only when
 *      sqrt_one_minus_ab_prev == 0 (t == 0); n_re and x_re are both given or both NULL.  `flags` names the optional buffers that are
 *      passed and must agree with the pointers.  Any 4-byte-aligned pointers and any H * W are accepted (16-byte accesses when every
 *      pointer is 16-byte aligned and 4 | H * W).  Returns -2 (cgd_last_error) for a missing buffer, flags that disagree with the
 *      pointers, a broadcast extent other than the ones above, or a non-positive size. ---- */
enum { CGD_MASK_PRED_XSTART = 1, CGD_MASK_N_KNOWN = 2, CGD_MASK_RENOISE = 4 };
typedef struct cgd_mask_coef {
  float sqrt_ab_prev;           /* sqrt(abar_{t-1}): the init image's share of the known region                 */
  float sqrt_one_minus_ab_prev; /* sqrt(1 - abar_{t-1}): the share of n_known (0 at t == 0)                     */
  float renoise_x;              /* sqrt(abar_t / abar_{t-1}): x_{t-1}'s share of the re-noised x_t               */
  float renoise_n;              /* sqrt(1 - abar_t / abar_{t-1}): the share of n_re                              */
  int flags;                    /* CGD_MASK_PRED_XSTART | CGD_MASK_N_KNOWN | CGD_MASK_RENOISE: buffers passed   */
} cgd_mask_coef;
int cgd_masked_merge(cgd_ctx* ctx, float* sample, float* pred_xstart, const float* init, const float* mask, const float* n_known,
                     const float* n_re, float* x_re, int B, int H, int W, int init_batch, int mask_batch, int mask_channels,
                     const cgd_mask_coef* k, void* stream);

/* ---- ILVR (Choi et al., 2021): sampling conditioned on the low frequencies of a reference image; the refinement after a sampler update
 *      at step index t, in two launches whatever B.  Per axis of extent n and factor N, D is the (n/N, n) antialiased cubic down-resize
 *      and U the (n, n/N) cubic up-resize of cgd_cutouts_resize_weights (ResizeRight, pad_mode='constant': taps outside the extent read
 *      zero, rows are not renormalised), P = U D and phi(z) = P_H z P_W^T per plane.  The update left `sample` (the state at level t-1)
 *      and `pred_xstart`:
 *        known        = sa ref + sb noise            (sa = sqrt(abar_{t-1}), sb = sqrt(1 - abar_{t-1}); two rounded products and a
 *                                                     rounded sum, not fused)
 *        sample      += phi(known - sample)
 *        pred_xstart += phi(ref   - pred_xstart)
 *      both in place; a correction that is exactly zero leaves the bits of its pixel alone.  Gather form, fixed summation order: the
 *      same bits on every run.  sample, pred_xstart, noise: (B,3,H,W); ref: (ref_batch,3,H,W), ref_batch 1 or B; scratch:
 *      cgd_ilvr_scratch_floats(B, H, W, factor, pred_xstart != NULL) floats (0 for a shape or factor that is refused).  pred_xstart
 *      may be NULL; noise only when sb == 0 (t == 0; it is not read then).  Any 4-byte-aligned pointers are accepted.  Returns -2
 *      (cgd_last_error), before any launch, for a missing sample, ref or scratch, a factor that is not a power of two in [2, 64] or
 *      does not divide H and W, a ref_batch other than 1 or B, a missing noise with sb != 0, or a non-positive size. ---- */
long cgd_ilvr_scratch_floats(int B, int H, int W, int factor, int with_pred_xstart);
int cgd_ilvr_refine(cgd_ctx* ctx, float* sample, float* pred_xstart, const float* ref, const float* noise, float* scratch, int B, int H,
                    int W, int ref_batch, int factor, float sa, float sb, void* stream);

/* ---- 2D animation (Disco Diffusion's 2D mode, Deforum): frame k starts from frame k - 1, zoomed, rotated and shifted.  What runs once per
 *      frame, each in one launch; NCHW fp32, any C.
 *      cgd_frame_warp: affine resampling.  For destination pixel (x, y) the source position is
 *        sx = m0 x + m1 y + m2,  sy = m3 x + m4 y + m5        (the INVERSE map, built by the host; pixel centres sit on integers)
 *      computed, floored and split into integer and fractional parts in fp64; the fractions then become fp32, weights and sums are fp32.
 *      interp 0: bilinear, taps floor, floor + 1.  interp 1: bicubic, Keys kernel with a = -0.75 (OpenCV's INTER_CUBIC, torch's bicubic; not
 *      the a = -0.5 of the cutout resize), taps floor - 1 .. floor + 2.  Separable: the x taps of a row are summed in ascending order, then
 *      the row results in ascending y.  border, applied to every tap index on its own: 0 wrap (i mod n, also for negative i), 1 reflect
 *      without repeating the edge (period 2 (n - 1): OpenCV's REFLECT_101, torch's reflection with align_corners=True; a side of length 1
 *      gives index 0), 2 replicate (clamp).  clamp 1: the result is clamped to [-1, 1] after interpolation (bicubic overshoots).  At a
 *      fraction of 0 the weights are exactly 1 and 0: the identity and integer shifts copy bits.
 *      cgd_channel_stats: stats (B,C,2) = (mean, population standard deviation) of every plane; the sums of x and x^2 are fp64, in a fixed
 *      order, one workgroup per plane.
 *      cgd_color_match, in place: x <- x + amount ((mu_ref + (x - mu_x) r) - x), r = sigma_ref / sigma_x and r = 1 where sigma_x < 1e-6 (a
 *      flat plane stays flat); stats_x (B,C,2) and stats_ref (ref_batch,C,2) as cgd_channel_stats writes them, ref_batch 1 or B, amount in
 *      [0, 1] (0 leaves the bits alone), clamp 1 = clamp the result to [-1, 1].
 *      Gather form, no atomics, no scratch buffer: the same bits on every run.  Plane offsets are 64-bit.  Any 4-byte-aligned pointers
 *      are accepted.  dst must not alias src.  Each returns -2 (cgd_last_error), before any launch, for a null pointer, src == dst, a
 *      non-positive size, H W >= 2^31, an unknown interp or border, a non-finite matrix entry, a matrix that maps a frame corner beyond
 *      +-2^30 (the integer tap indices then cannot overflow), a ref_batch other than 1 or B, or an amount outside [0, 1].  The arguments
 *      are judged before the context is looked at: a refused call returns -2 with a NULL context too, an accepted one -3. ---- */
typedef struct cgd_warp {
  double m[6];
  int interp; /* 0 bilinear, 1 bicubic */
  int border; /* 0 wrap, 1 reflect, 2 replicate */
  int clamp;  /* 1: clamp the result to [-1, 1] */
} cgd_warp;
int cgd_frame_warp(cgd_ctx* ctx, const float* src, float* dst, int B, int C, int H, int W, const cgd_warp* warp, void* stream);
int cgd_channel_stats(cgd_ctx* ctx, const float* x, float* stats, int B, int C, int H, int W, void* stream);
int cgd_color_match(cgd_ctx* ctx, float* x, const float* stats_x, const float* stats_ref, int ref_batch, float amount, int clamp, int B, int C,
                    int H, int W, void* stream);

/* ---- 3D animation (Disco Diffusion's 3D mode, Deforum): frame k starts from frame k - 1 as a pinhole camera sees it after moving, with a
 *      depth for every pixel (parallax).  One launch; NCHW fp32, any C.
 *      Camera axes: x right, y down, z into the screen; pixel centres sit on integers; (cx, cy) is the principal point and f the focal
 *      length in pixels.  A source position q of depth z > 0 is the point X = z ((qx - cx) / f, (qy - cy) / f, 1); the motion between two
 *      frames is X' = R X + T (R row-major); X' is seen at (cx, cy) + f (X'x, X'y) / X'z.  cgd_frame_warp3d gathers: destination pixel p reads
 *      the source at G(p, z), the exact inverse of that map for a source point of depth z,
 *        r = ((px - cx) / f, (py - cy) / f, 1),  a = R^T r with a_z <- max(a_z, 1e-6),  b = R^T T,
 *        lambda = max((z + b_z) / a_z, near),  Xs = lambda a - b,  G = (cx + f Xs_x / z, cy + f Xs_y / z)
 *      all in fp64.  depth NULL: z = max(z0, near) everywhere (a homography).  depth (depth_batch, 1, H, W), depth_batch 1 or B, in the units
 *      of z0: the depth belongs to the unknown source pixel and is resolved by `iters` fixed-point steps s_0 = p,
 *      s_{k+1} = G(p, max(D(s_k), near)); D(s) is bilinear with a replicate border, taps and weights in fp64, exactly the stored value at an
 *      integer position; a NaN depth reads as near.  The final position is clamped to +-2^30, then floored, split and sampled exactly as
 *      cgd_frame_warp samples (interp, border, clamp as there, the same summation order).  A camera with R = I and T = 0 exactly copies
 *      bits, with or without a depth map.  Gather form, no atomics, no scratch buffer: the same bits on every run.  Plane offsets are
 *      64-bit.  Returns -2 (cgd_last_error), before any launch and before the context is looked at, for a null src, dst or cam, a dst that
 *      overlaps src or depth, a pointer that is not 4-byte aligned, a non-positive size, H W >= 2^31, an unknown interp or border, iters
 *      outside 1..4, a non-finite camera entry, f, z0 or near <= 0, max |R R^T - I| > 1e-9 or det R < 0, or a depth_batch other than 1 or
 *      B when depth is given; an accepted call returns -3 with a NULL context. ---- */
typedef struct cgd_camera {
  double R[9], T[3], f, cx, cy, z0, near;
  int iters;  /* fixed-point steps of the depth lookup, 1..4 (not used without a depth map) */
  int interp; /* 0 bilinear, 1 bicubic */
  int border; /* 0 wrap, 1 reflect, 2 replicate */
  int clamp;  /* 1: clamp the result to [-1, 1] */
} cgd_camera;
int cgd_frame_warp3d(cgd_ctx* ctx, const float* src, float* dst, const float* depth, int depth_batch, int B, int C, int H, int W,
                     const cgd_camera* cam, void* stream);

/* ---- video mode (Disco Diffusion's video input and Warp notebooks, Deforum's hybrid video): frame k starts from the stylised frame k - 1,
 *      moved the way the clip moved.  Dense pyramidal Lucas-Kanade optical flow in the PATCH form (each pixel moves its whole window by its
 *      own flow) and the warp that follows a flow (csrc/flow.hip).  NCHW fp32; pixel centres sit on integers.
 *      A flow is (B, 2, H, W): channel 0 the x displacement in pixels, channel 1 the y displacement.  cgd_flow_estimate(tmpl, img) writes F
 *      with img(p + F(p)) ~ tmpl(p); tmpl and img are (B, C, H, W), C 3 (luminance Y = (0.2989 R + 0.587 G) + 0.114 B in fp32) or 1.
 *      Pyramid: level 0 is Y, level l + 1 the antialiased cubic resize (cgd_op_resize_cubic's launcher) of level l to
 *      (ceil(H_l / 2), ceil(W_l / 2)), both frames and the whole batch as 2B planes in one launch.  cgd_flow_levels: the largest L <= levels
 *      whose coarsest level has a shorter side of at least 2 radius + 1, at least 1 (0 for arguments that are refused).  The coarsest level
 *      starts from zero; a finer level (Hf, Wf) reads the coarser flow (Hc, Wc) bilinearly at ((x + 0.5) Wc / Wf - 0.5,
 *      (y + 0.5) Hc / Hf - 0.5), fp64 coordinates, taps and weights, replicate border, times Wf / Wc (x) or Hf / Hc (y), rounded to fp32.
 *      One iteration at pixel p with flow u, over the window q = p + (dx, dy), |dx|, |dy| <= radius, q inside the frame, ascending dy then
 *      ascending dx: b the template level, bx, by its central differences divided by 2 (replicate border); s = q + u in fp64 counts when
 *      0 <= sx <= W - 1 and 0 <= sy <= H - 1 and contributes to nothing otherwise; a(s) bilinear, split in fp64 with fp32 weights as
 *      cgd_frame_warp splits; e = b(q) - a(s); fp32 sums Gxx = lambda + sum bx^2, Gyy = lambda + sum by^2, Gxy = sum bx by,
 *      rx = sum bx e, ry = sum by e; det = Gxx Gyy - Gxy^2, du = (Gyy rx - Gxy ry) / det, dv = (Gxx ry - Gxy rx) / det; a non-finite
 *      step is zero, a step longer than max_step is scaled to that length; u += (du, dv).  All `iters` iterations of a level run in one
 *      launch (a pixel reads only its own flow); an estimate is about 2 L launches.  Fixed summation order, no atomics: the same bits on
 *      every run.  scratch: cgd_flow_scratch_floats(B, H, W, levels, radius) floats (0 for arguments that are refused).
 *      cgd_op_flow_level (test support): one level on given planes b, a (B, H, W); coarse (B, 2, Hc, Wc) or NULL (start from zero); flow
 *      (B, 2, H, W) is written only.
 *      cgd_frame_warp_flow, one launch, gather form:  dst(p) = w S(p + F(p)) + (1 - w) fallback(p),  w = blend m(p).  S samples src
 *      (B, C, H, W) exactly as cgd_frame_warp does (interp, border, clamp, summation order; position p + (double)F(p) clamped to +-2^30).
 *      m = 1 without flow_back.  With flow_back (the flow of the opposite direction) Fb is read bilinearly at s = p + F(p) (fp64 taps,
 *      replicate border) and m = 0 when s lies outside [0, W - 1] x [0, H - 1], when Fb(s) is not finite, or unless
 *      |F + Fb|^2 <= alpha (|F|^2 + |Fb|^2) + beta, in fp64 (the forward-backward check of Sundaram et al., 2010; usual values
 *      alpha 0.01, beta 0.5).  A non-finite F reads as zero flow with m = 0.  w == 1 stores the sample's bits (zero flow with blend 1
 *      copies src), w == 0 the fallback's.  fallback (B, C, H, W) may be NULL only with blend == 1 and no flow_back; the sample is then
 *      stored whatever m.  mask_out (B, 1, H, W), optional, receives m.  flow and flow_back are (flow_batch, 2, H, W), flow_batch 1 or B.
 *      The arguments are judged before the context is looked at: a refused call returns -2 (cgd_last_error), an accepted one -3 with a
 *      NULL context.  Refused: a null or not 4-byte-aligned pointer, a non-positive size, H W >= 2^31, C not 1 or 3 (estimate), radius
 *      outside 1..7, iters outside 1..16, levels outside 1..8, a lambda or max_step that is not finite and positive, a flow that aliases
 *      an input, more than 32767 samples, H W >= 2^30 when more than one pyramid level would run (the resize's limit); for the warp also an unknown interp or border, a flow_batch other than 1 or B, blend outside [0, 1], a negative or
 *      non-finite alpha or beta, and a dst or mask_out that overlaps an input. ---- */
typedef struct cgd_flow_params {
  int levels, iters, radius; /* defaults 4, 4, 4 */
  float lambda, max_step;    /* defaults 1e-3, 1 */
} cgd_flow_params;
typedef struct cgd_warp_flow {
  float blend, alpha, beta; /* defaults 1, 0.01, 0.5 */
  int interp;               /* 0 bilinear, 1 bicubic */
  int border;               /* 0 wrap, 1 reflect, 2 replicate */
  int clamp;                /* 1: clamp the sample to [-1, 1] */
} cgd_warp_flow;
int cgd_flow_levels(int H, int W, int levels, int radius);
long cgd_flow_scratch_floats(int B, int H, int W, int levels, int radius);
int cgd_flow_estimate(cgd_ctx* ctx, const float* tmpl, const float* img, float* flow, float* scratch, int B, int C, int H, int W,
                      const cgd_flow_params* params, void* stream);
int cgd_op_flow_level(cgd_ctx* ctx, const float* b, const float* a, const float* coarse, int Hc, int Wc, float* flow, int B, int H, int W,
                      const cgd_flow_params* params, void* stream);
int cgd_frame_warp_flow(cgd_ctx* ctx, const float* src, const float* flow, const float* flow_back, const float* fallback, float* dst,
                        float* mask_out, int flow_batch, int B, int C, int H, int W, const cgd_warp_flow* settings, void* stream);

/* ---- windowed sampling (MultiDiffusion, Bar-Tal et al., 2023): the frame is cut into overlapping S x S windows of the model's trained size, the
 *      model runs on all windows as one batch, and the window outputs are averaged into one prediction for the frame.  An adjoint pair, one
 *      launch each whatever B, C and the window count:
 *        gather  win[b,k,c,u,v]   = ay[ky][u] ax[kx][v] full[b,c,(oy[ky]+u) mod H,(ox[kx]+v) mod W]                 k = ky nx + kx
 *        merge   full[b,c,y,x] (+)= sum_ky sum_kx ay[ky][u] ax[kx][v] win[b,k,c,u,v]      over the windows that cover (y,x):
 *                                                                                        u = (y - oy[ky]) mod H < S, v = (x - ox[kx]) mod W < S
 *      full: (B,C,H,W) fp32 NCHW; win: (B nW,C,S,S), nW = ny nx, row b nW + k.  oy [ny], ox [nx]: window origins per axis, HOST arrays (read
 *      during the call, at most 16 per axis); the window grid is their outer product.  wrap: bit 0 lets windows run over the right edge and
 *      continue at x = 0, bit 1 the same for the bottom edge.  ay [ny][S], ax [nx][S]: device tables of per-axis weights, both or neither;
 *      NULL means ones, and the gather is then a copy that keeps every bit.  The merge is in gather form: one thread owns its output elements
 *      and sums the covering windows in a fixed order (ky ascending outside, kx ascending inside), no atomics, the same bits on every run;
 *      accumulate != 0 adds the sum to what `full` holds.  Any 4-byte-aligned pointers are accepted (16-byte accesses when full, win and the
 *      tables are 16-byte aligned).  Both return -2 (cgd_last_error), before any launch, unless: S, H, W and every origin are multiples of 8;
 *      S <= H and S <= W; 1 <= ny, nx <= 16; every origin lies in [0, extent), and o + S <= extent on an axis that does not wrap; every pixel
 *      is covered by at least one window; H W and S S are below 2^31; the sizes are positive and full, win, oy, ox are given. ---- */
int cgd_window_gather(cgd_ctx* ctx, const float* full, float* win, const int* oy, int ny, const int* ox, int nx, const float* ay, const float* ax,
                      int B, int C, int H, int W, int S, int wrap, void* stream);
int cgd_window_merge(cgd_ctx* ctx, const float* win, float* full, const int* oy, int ny, const int* ox, int nx, const float* ay, const float* ax,
                     int B, int C, int H, int W, int S, int wrap, int accumulate, void* stream);

/* ---- DDIM inversion of an init image (guided_diffusion's ddim_reverse_sample, unguided, clip_denoised=False): the update of one inversion
 *      step, from level t up to level t+1 along the deterministic DDIM ODE, in one launch after the UNet forward:
 *        eps         = model_out6[:, 0:3]                 (read in place: plane b * 6 + c; the variance planes 3..5 are never touched)
 *        pred_xstart = sqrt_recip x - sqrt_recipm1 eps
 *        x_next      = sqrt_ab_next pred_xstart + sqrt_one_minus_ab_next eps
 *        noise_out   = (x_next - sqrt_ab_next init) inv_sqrt_one_minus_ab_next     (the tensor that q_samples init to x_next at level t+1)
 *      eps is the model's output, not upstream's (sqrt_recip x - pred_xstart) / sqrt_recipm1: equal in exact arithmetic, but that form
 *      divides by sqrt_recipm1 ~ 0.01 at t = 0 and costs an fp32 round trip 2e-4.
 *      x, x_next, pred_xstart, noise_out: (B,3,H,W); model_out6: (B,6,H,W); init: (init_batch,3,H,W), init_batch 1 or B.  x_next is
 *      required; no output may alias x and the outputs must be distinct buffers; pred_xstart and noise_out may be NULL; noise_out needs init, and init is read only for noise_out.
 *      Any 4-byte-aligned pointers and any H * W are accepted (16-byte accesses when every pointer is 16-byte aligned and 4 | H * W).
 *      Returns -2 (cgd_last_error), before any launch, for a non-positive size, a missing required buffer, an output that aliases x or another output, noise_out without
 *      init, an init batch other than 1 or B, or noise_out where sqrt_one_minus_ab_next (or its inverse) is 0: abar_next = 1, no noise at that level. ---- */
typedef struct cgd_reverse_coef {
  float sqrt_recip;                 /* sqrt(1/abar_t)                                                        */
  float sqrt_recipm1;               /* sqrt(1/abar_t - 1)                                                    */
  float sqrt_ab_next;               /* sqrt(abar_{t+1}) (0 at the last index)                                */
  float sqrt_one_minus_ab_next;     /* sqrt(1 - abar_{t+1})                                                  */
  float inv_sqrt_one_minus_ab_next; /* 1 / sqrt(1 - abar_{t+1}), or 0 where it is undefined                  */
} cgd_reverse_coef;
int cgd_ddim_reverse_update(cgd_ctx* ctx, const float* x, const float* model_out6, const float* init, float* x_next, float* pred_xstart,
                            float* noise_out, int B, int H, int W, int init_batch, const cgd_reverse_coef* k, void* stream);

/* ---- single ops, exported for parity tests and for user-supplied cond_fn plumbing ---- */
/* C[M][N] = alpha * A[M][K] B[N][K]^T (+bias[N]) (+R[M][N]); conv3x3: A is NHWC (Bn,H,W,Cin), B = [N][9*Cin].
 * force_tile: 0 auto, 64 / 128 / 256 / 257 (+1000: two-deep prefetch) igemm tiles, 513 weight GEMM kernel (B re-packed per call),
 * 514 the same with the packed copy cached by B's pointer (B must persist; micro-benchmarks), 518 the few-row weight GEMM kernel (5 <= M rows, K
 * split inside the workgroup, one slice; the cached fragment copy of THIS B pointer is dropped first, other weights of the context stay), 519 the
 * same with the copy cached by B's pointer (B must persist; micro-benchmarks).  A forced 518 / 519 asks only what the kernel can run, not the
 * CGD_KGEMM policy knobs.  splitk: >= 1 slices (1 = automatic), -1 = one slice, never split automatically. */
int cgd_op_gemm(cgd_ctx* ctx, const float* A, int lda, const float* B, int ldb, float* C, int ldc, const float* bias, const float* R,
                int ldr, int M, int N, int K, float alpha, int force_tile, int splitk, void* stream);
/* cgd_op_gemm with the two switches the networks' linears set (test support, like cgd_op_conv3x3_ex).  weight = 1: B is a persistent weight, the
 * weight GEMM kernel caches its fragment copy by B's pointer (B must then keep its content for the life of the context).  defer = 1: a launch that
 * splits K leaves its slices in the context workspace; see cgd_op_conv3x3_ex for who sums them. */
int cgd_op_gemm_ex(cgd_ctx* ctx, const float* A, int lda, const float* B, int ldb, float* C, int ldc, const float* bias, const float* R,
                   int ldr, int M, int N, int K, float alpha, int force_tile, int splitk, int weight, int defer, void* stream);
/* host only, reads nothing on the device and changes nothing: the deferred split-K reduction the context still holds,
 * out5 = {valid, slices, rows, columns, row stride of the output}; all zero when nothing is pending.  With out2[1] of cgd_launch_counts a test can
 * tell whether a reader summed the slices itself (counter unchanged, nothing pending afterwards) or a reduce launch ran (counter + 1). */
int cgd_op_pending(cgd_ctx* ctx, int64_t out5[5]);
/* G[b] = scale * A_b^T A_b for A [B * N][C] (row stride lda >= C, a multiple of 4; 16-byte aligned), C in {64, 128, 256, 512}, any N >= 1: the tall-skinny
 * contraction of the style loss (csrc/gram.hip).  Exact fp32 products whatever the context precision; bit-identical from run to run. */
int cgd_op_gram(cgd_ctx* ctx, const float* A, int lda, int B, int N, int C, float scale, float* G_out /* [B][C][C] */, void* stream);
/* dx[M][N] = A[M][K] W[N][K]^T (+ add[M][N]) + the backward of a GroupNorm + SiLU over the same M = B * HW rows: dz silu'(x a + b) A1 - (x - mean) A2 - A3
 * per element, coef = [B][N][4] {a, b, unused, mean}, bcoef = [B][N][4] {A1, A2, A3, unused} (what cgd_op_gn_bwd computes internally).  One launch of
 * the weight GEMM kernel (W re-packed per call) whose epilogue applies the norm: a ResBlock's 1x1 skip dgrad and GN1's backward.  bf16x3 contexts only;
 * K % 64 == 0, N % 32 == 0, every row stride a multiple of 4, operands 16-byte aligned, HW % 128 == 0 or B == 1: anything else is an error. */
int cgd_op_gemm_gn_bwd(cgd_ctx* ctx, const float* A, int lda, const float* W, int ldw, float* dx, int lddx, const float* x, int ldx,
                       const float* dz, int lddz, const float* add, int ldadd, const float* coef, const float* bcoef, int B, int HW, int N, int K,
                       void* stream);
/* host-only (no GPU, no context): 1 if cgd_op_gemm_gn_bwd runs a problem with these strides on a context of this precision mode, 0 if it returns an
 * error (the same predicate).  x_misalign: byte offset of x from a 16-byte boundary; ldadd = 0: no `add` operand. */
int cgd_op_gemm_gn_bwd_accepts(int precision, int lda, int ldw, int lddx, int ldx, int lddz, int ldadd, int x_misalign, int B, int HW, int N, int K);
/* w_packed: [Cout][9*Cin] fp32 (generic kernel); w_frag (optional): the same weights in MFMA-fragment order, bf16 hi/lo planes,
 * produced by cgd_op_pack_conv3x3_frag from the torch layout [Co][Ci][3][3] (dgrad=1: rotated/transposed) — enables the
 * halo-staged kernel (force_tile 512 or automatic for large images) */
int cgd_op_pack_conv3x3_frag(cgd_ctx* ctx, const float* w_torch, float* out /* Co*Ci*9 floats of storage */, int Co, int Ci, int dgrad,
                             void* stream);
/* host-only (no GPU, no context): the launcher's choice for a GEMM (conv = 0: C[M][N] over K, weight = 1 when B is a persistent
 * weight) or a conv3x3 (conv = 1: M = B*H*W pixels, N = Cout) with the default knobs: out4 = {kernel: 0 igemm_kernel, 1 hconv2_kernel,
 * 2 hgemm_kernel; tile code; split-K slices; workgroups of the main launch}.  CPU tests of the dispatch policy use it. */
int cgd_op_plan(int conv, int M, int N, int K, int H, int W, int Cin, int weight, int precision, int num_cu, int* out4);
/* host-only, cgd_op_plan for a 3x3 conv [Bn][H][W][Cin] -> Cout with what the UNet's ResBlocks set besides the shape: hconv_var = the tile variant
 * bits of cgd_set_hconv; stats = 1: the launch is asked for forward GroupNorm records of its output; gnb = 1: for the backward sums of a norm (a
 * dgrad conv).  out5 = {kernel, tile code, split-K slices, workgroups, pixels per workgroup tile of hconv2_kernel (0 on the other kernels)}. */
int cgd_op_plan_conv(int Bn, int H, int W, int Cin, int Cout, int precision, int num_cu, int hconv_var, int stats, int gnb, int* out5);
/* tuning knob: mode & 15 = 0 off / 1 auto (M >= min_m); mode >> 4 = tile variant bits (0: 8x16 pixels, 1: 16x16, 2: 16x16 below 16384
 * pixels, 4: wavefront sub-tile 64 pixels x 64 channels instead of the default 128 x 32, 8: the unsplit 4x16-pixel x 128-channel tile (all
 * of K in one workgroup) wherever the context is bf16x3 and Cout a multiple of 128, not only where the launcher picks it by itself: tests and
 * benchmarks; other problems keep their tile) */
int cgd_set_hconv(cgd_ctx* ctx, int mode, int min_m);
int cgd_op_conv3x3(cgd_ctx* ctx, const float* x_nhwc, int ldx, const float* w_packed, const float* w_frag, float* y_nhwc, int ldy,
                   const float* bias, const float* R, int ldr, int Bn, int H, int W, int Cin, int Cout, int upsample_input, int force_tile,
                   int splitk, void* stream);
/* cgd_op_conv3x3 with the add-ons the UNet's ResBlocks switch on (test support, like cgd_op_conv3x3_wino_ex below).  gn_ab: per-(sample,
 * channel) pairs {a, b} [Bn][Cin][2]; the conv then runs on SiLU(x * a + b), applied in the patch staging (halo conv kernels only: any other
 * route is refused).  defer = 1: a launch that splits K leaves its slices in the context workspace (unless CGD_DEFER=0).  The next entry of the
 * context sums them: a cgd_op_gn_fwd (x) / cgd_op_gn_bwd (dz) / cgd_op_ln_fwd (x) / cgd_op_ln_bwd (dy) on exactly this tensor (pointer, rows,
 * columns, row stride, stream) at load time, writing the finished tensor back as it goes (cgd_op_ln_bwd and the register-cached single-launch cgd_op_gn_bwd keep dy / dz in
 * registers and do NOT write it back: that buffer then never holds the finished tensor; the LayerNorms
 * only at C = 256 / 512 / 768 / 1024, the single-launch GroupNorms only with CGD_DEFER >= 2); a norm that does not match, and every GEMM / conv,
 * pooling / upsampling, activation, attention and Gram entry, runs the reduce launch first, on the producer's stream.  stats, gnb_x, gnb_ldx, gnb_scratch: as in
 * cgd_op_conv3x3_wino_ex. */
int cgd_op_conv3x3_ex(cgd_ctx* ctx, const float* x_nhwc, int ldx, const float* w_packed, const float* w_frag, float* y_nhwc, int ldy,
                      const float* bias, const float* R, int ldr, const float* gn_ab, int Bn, int H, int W, int Cin, int Cout,
                      int upsample_input, int force_tile, int splitk, int defer, int stats, const float* gnb_x, int gnb_ldx,
                      const float* gnb_scratch, void* stream);
/* Winograd F(2,3)-along-W variant of the halo conv (wconv.hip; H a multiple of 8, W of 16; bf16x3 products, or — round 6 — exact fp32 products
 * in precision-0 contexts: wconv_kernel<..., F32> on v_mfma_f32_32x32x2_f32): w_wino = the torch weights transformed and packed by
 * cgd_op_pack_conv3x3_wino (Co*Ci*12 floats of storage) FOR THE CONTEXT'S CURRENT PRECISION MODE (fp32 values or bf16 hi / lo planes: pack and
 * run under the same mode; the UNet repacks its copies when the mode changes).  gn_ab (optional): per-(sample, channel) pairs
 * {a, b} [Bn][Cin][2]; the kernel then convolves SiLU(x * a + b) (the fused GroupNorm of the UNet's ResBlocks).
 * cgd_set_wino: mode 1 (default) = the UNet's 3x3 convs of >= min_m (default 16384) pixels run on this kernel, 0 = off, 2 / 3 = 16- / 8-row
 * tiles everywhere; set BEFORE cgd_unet_finalize, which packs the transformed weights (environment CGD_WINO="<mode>[,min_m]"). */
int cgd_op_pack_conv3x3_wino(cgd_ctx* ctx, const float* w_torch, float* out, int Co, int Ci, int dgrad, void* stream);
int cgd_op_conv3x3_wino(cgd_ctx* ctx, const float* x_nhwc, int ldx, const float* w_wino, float* y_nhwc, int ldy, const float* bias,
                        const float* R, int ldr, const float* gn_ab, int Bn, int H, int W, int Cin, int Cout, int upsample_input,
                        void* stream);
int cgd_set_wino(cgd_ctx* ctx, int mode, int min_m);
/* Round 5, test support for the conv-epilogue GroupNorm records: cgd_op_conv3x3_wino with the add-ons the UNet's
 * ResBlocks switch on.  stats = 1: the epilogue also takes per-(8 x 16-pixel half tile, channel) statistics of y for the cgd_op_gn_fwd that
 * reads y next (same pointer / row stride / rows; y may be a channel slice of a wider concat buffer).  gnb_x (+ gnb_ldx, gnb_scratch =
 * the scratch of the FORWARD cgd_op_gn_fwd over gnb_x with act = 1): y is the upstream gradient dz of that GroupNorm + SiLU and the
 * epilogue also takes the norm's backward sums, which the cgd_op_gn_bwd called on (gnb_x, y) then merges instead of sweeping x and dz.
 * Records belong to the current pass: cgd_op_new_pass starts the next one (what cgd_unet_forward / cgd_unet_dgrad do), after which no
 * earlier record can be served; a launch that rewrites y without taking records kills y's records too. */
int cgd_op_conv3x3_wino_ex(cgd_ctx* ctx, const float* x_nhwc, int ldx, const float* w_wino, float* y_nhwc, int ldy, const float* bias,
                           const float* R, int ldr, const float* gn_ab, int Bn, int H, int W, int Cin, int Cout, int upsample_input,
                           int stats, const float* gnb_x, int gnb_ldx, const float* gnb_scratch, void* stream);
/* 3x3 convolution of stride 2, padding 1 (csrc/sconv.hip: the classic UNet's Downsample) and its backward to the input, as implicit GEMMs on MFMA
 * in the context's precision mode.  NHWC fp32 rows with a row stride; w_torch [Cout][Cin][3][3] as uploaded, packed per call (test and benchmark
 * entries: the UNet packs once at finalize).
 *   cgd_op_conv3x3_s2:       y (B, H/2, W/2, Cout) = conv(x (B, H, W, Cin)) + bias (bias may be NULL)
 *   cgd_op_conv3x3_s2_dgrad: dx (B, H, W, Cin) = conv^T(dy (B, H/2, W/2, Cout)) (+ add, same shape as dx, may be NULL); B, H, W are the INPUT's.
 *                            A gather per input-pixel parity (1, 2, 2 and 4 taps), one launch, no atomics: bit-identical from run to run.
 * Refused (-2, cgd_last_error): odd H or W, Cin or Cout not a positive multiple of 32, a row stride below its channel count or not a multiple of 4,
 * an operand of 2^31 bytes or more (32-bit byte offsets), a pointer that is not 16-byte aligned.
 * cgd_op_conv3x3_s2_accepts: host-only (no GPU, no context), 1 if the entries run a problem of these strides and shape, 0 if they refuse it (the
 * same predicate, pointers aside).  dgrad = 0: ld_in = ldx, ld_out = ldy; dgrad = 1: ld_in = lddy, ld_out = lddx; ldadd = 0: no add operand. */
int cgd_op_conv3x3_s2(cgd_ctx* ctx, const float* x_nhwc, int ldx, const float* w_torch, const float* bias, float* y_nhwc, int ldy, int B, int H,
                      int W, int Cin, int Cout, void* stream);
int cgd_op_conv3x3_s2_dgrad(cgd_ctx* ctx, const float* dy_nhwc, int lddy, const float* w_torch, float* dx_nhwc, int lddx, const float* add,
                            int ldadd, int B, int H, int W, int Cin, int Cout, void* stream);
int cgd_op_conv3x3_s2_accepts(int dgrad, int ld_in, int ld_out, int ldadd, int B, int H, int W, int Cin, int Cout);
/* host-only (no GPU, no context; test support, as cgd_op_attn_plan): the launcher's tile and split-K choice for the forward (dgrad = 0) or the backward
 * (dgrad = 1) of a dense problem on a device of num_cu compute units with the context's fixed 256 MiB workspace; B, H, W: the INPUT's.
 * out4 = {tile rows (128 | 64), tile columns (64 | 32), split-K slices, workgroups of the main launch (the backward's grid is rounded up to whole
 * groups of 8 tiles x 4 parity classes; the surplus workgroups return at once)}.  -2 where cgd_op_conv3x3_s2_accepts refuses the problem. */
int cgd_op_plan_conv_s2(int dgrad, int B, int H, int W, int Cin, int Cout, int num_cu, int* out4);
/* The same two on weights the caller packed once (what the UNet's Downsample runs per step; benchmarks time these, so that no per-call weight
 * pack is inside the figure): w_fwd [Cout][9 Cin] with column (ky * 3 + kx) * Cin + ci, w_dgrad [Cin][9 Cout] with column
 * ((2 - ky) * 3 + (2 - kx)) * Cout + co = w[co][ci][ky][kx] (ops.pack_conv3x3 gives both). */
int cgd_op_conv3x3_s2_packed(cgd_ctx* ctx, const float* x_nhwc, int ldx, const float* w_fwd, const float* bias, float* y_nhwc, int ldy, int B,
                             int H, int W, int Cin, int Cout, void* stream);
int cgd_op_conv3x3_s2_dgrad_packed(cgd_ctx* ctx, const float* dy_nhwc, int lddy, const float* w_dgrad, float* dx_nhwc, int lddx,
                                   const float* add, int ldadd, int B, int H, int W, int Cin, int Cout, void* stream);
int cgd_op_new_pass(cgd_ctx* ctx);
/* number of GroupNorm launches since context creation that MERGED conv-epilogue records (forward statistics + backward sums) instead of
 * sweeping their input: lets a test assert which path a cgd_op_gn_fwd / cgd_op_gn_bwd call took */
int64_t cgd_op_gn_record_merges(cgd_ctx* ctx);
/* test support: copies the live records of the current pass for tensor y (`rows` rows of C floats at row stride ldy, written on `stream`), as ONE conv
 * launch left them, to the device buffer out (cap floats): [rows / *pixels][C][2], kind 0 = (mean, M2) of the *pixels values of every (tile, channel),
 * kind 1 = the backward sums (gcoef sum du, gcoef sum du (x - mean)); *pixels = 0 and nothing copied when the tensor has none */
int cgd_op_gn_records(cgd_ctx* ctx, const float* y, int ldy, int64_t rows, int C, int kind, float* out, int64_t cap, int* pixels, void* stream);
/* host-only: float offset of the per-(sample, group) statistics {mean, rstd} [B][32][2] inside a cgd_op_gn_fwd scratch buffer (tests compare
 * them with float64 group statistics) */
int64_t cgd_op_gn_stats_offset(int B, int HW, int C);
/* host-only (no GPU, no context): the software pipeline of wconv_kernel's patch staging inside one 24-step channel chunk, nb = 4 (16-row
 * tiles) or 2 (8-row tiles): out7 = {task whose 4 pixel loads are issued at step q, tasks whose transform piece 1 ... 6 runs at step
 * q}, -1 = none; task k lives in register slot k & 1.  CPU tests check that no slot is reloaded while its task is still live. */
int cgd_op_wconv_schedule(int nb, int q, int* out7);
/* box calibration (bench.py `box_calibration`): a register-resident v_mfma_f32_32x32x16_bf16 loop, one wavefront per SIMD
 * on every CU, `iters` x 12 MFMAs per wavefront: no memory traffic, so its rate is what the box's clock / power state gives the matrix pipes.
 * flop_out (optional, host): the FLOP of the launch; time it with events on `stream`. */
int cgd_op_mfma_peak(cgd_ctx* ctx, int iters, double* flop_out, void* stream);
int cgd_op_conv_in(cgd_ctx* ctx, const float* x_nchw, const float* w, const float* bias, float* y_nhwc, int Bn, int H, int W, int Cin,
                   int Cout, void* stream);
int cgd_op_conv_thin_out(cgd_ctx* ctx, const float* x_nhwc, int ldx, const float* w, const float* bias, float* y_nchw, int Bn, int H,
                         int W, int Cin, int Cout, void* stream);
/* The conditioned stem of the super-resolution UNets in one launch (csrc/superres.hip):
 *   y = conv3x3(cat([x, bilinear(low -> H x W)], channels), w, bias)      (SuperResModel.forward + input_blocks.0.0)
 * x (B,3,H,W) NCHW; low (B_low,3,h,w) NCHW with B_low 1 (shared by the batch) or B, any h, w >= 1; wpacked [Cout][3][3][6] as
 * cgd_pack_conv3x3 leaves it; bias [Cout] or NULL; y NHWC rows of stride ldy (0 = Cout).  Cout a multiple of 4, at most 256.  The
 * interpolation is F.interpolate(mode="bilinear", align_corners=False) with integer tap geometry; the zero padding is that of the
 * concatenated tensor.  No (B,6,H,W) tensor is formed. */
int cgd_op_sr_stem(cgd_ctx* ctx, const float* x, const float* low, int B_low, int h, int w, const float* wpacked, const float* bias, float* y,
                   int ldy, int B, int H, int W, int Cout, void* stream);
int64_t cgd_op_gn_scratch_floats(int B, int HW, int C);
/* GroupNorm over 32 groups: C a multiple of 32 and <= 4096, forward row strides (ldx, ldy) multiples of 4.  Up to 1024 pixels per sample (the
 * default single-launch size)
 * any pointer and, in the backward, any stride is taken (odd strides / 16-byte misaligned views run on scalar accesses);
 * above that the kernels run on 16-byte accesses: every row stride must be a multiple of 4 and x / y / dz / dx / add 16-byte aligned, or
 * the call fails (CGD_FAIL) before anything is launched. */
int cgd_op_gn_fwd(cgd_ctx* ctx, const float* x, int ldx, float* y, int ldy, int B, int HW, int C, const float* gamma,
                  const float* beta, const float* film, int act, float eps, float* scratch, void* stream);
int cgd_op_gn_bwd(cgd_ctx* ctx, const float* x, int ldx, const float* dz, int lddz, float* dx, int lddx, const float* add, int ldadd,
                  int B, int HW, int C, int act, float* scratch, void* stream);
int cgd_op_ln_fwd(cgd_ctx* ctx, const float* x, float* y, int rows, int C, const float* gamma, const float* beta, float eps,
                  float* stats, void* stream);
int cgd_op_ln_bwd(cgd_ctx* ctx, const float* x, const float* dy, float* dx, int rows, int C, const float* gamma, const float* stats,
                  void* stream);
/* pool2x2 / upsample2x: (Ho, Wo) = the OUTPUT map, the input is (2 Ho, 2 Wo) / (Ho / 2, Wo / 2).  B, Ho, Wo, C positive, C a multiple of 4, in / out
 * 16-byte aligned and, for upsample2x, Ho and Wo even, or the call fails before anything is launched */
int cgd_op_pool2x2(cgd_ctx* ctx, const float* in, float* out, int B, int Ho, int Wo, int C, float scale, void* stream);
int cgd_op_upsample2x(cgd_ctx* ctx, const float* in, float* out, int B, int Ho, int Wo, int C, float scale, void* stream);
/* act: 1 SiLU, 2 QuickGELU, 3 exact (erf) GELU; any other code fails (-2).  dy null: out = act(x); else out = dy * act'(x) */
int cgd_op_act(cgd_ctx* ctx, const float* x, const float* dy, float* out, int64_t n, int act, void* stream);
/* upper bound over all kernel families (the GEMM path's T x T probabilities); the networks size their own scratch per family (flash: row statistics) */
int64_t cgd_op_attn_buf_floats(int nb, int heads, int T, int d, int which);
/* test support (like cgd_op_gemm_ex / cgd_op_pending), host only: the floats of buffer `which` that the networks allocate for this call on THIS
 * context, i.e. the size of the kernel family the context would run it on now (row strides 3 heads d and heads d): flash keeps a copy of O in
 * bufs[0] and LSE | D, 2 nb heads 32 ceil(T / 32) floats, in bufs[1]; attn_s64_* only P; attn_mid_* no Pt / dAt; 0 = the family does not touch the
 * buffer (the forward of every family leaves bufs[2..4] alone: the networks hand it NULL there).  -1 for a NULL context or a non-positive shape.
 * The buffers carry state from a forward to its backward only. */
int64_t cgd_op_attn_buf_floats_ctx(cgd_ctx* ctx, int nb, int heads, int T, int d, int legacy, int causal, int which);
int cgd_op_attn_fwd(cgd_ctx* ctx, const float* qkv, float* out, int nb, int heads, int T, int d, int legacy, float* bufs[5],
                    void* stream);
int cgd_op_attn_bwd(cgd_ctx* ctx, const float* qkv, const float* dout, float* dqkv, int nb, int heads, int T, int d, int legacy,
                    float* bufs[5], void* stream);
/* cgd_op_attn_fwd with a causal mask (key j > query i excluded; [Q all heads | K | V] rows): every kernel family honours it.  There is no causal
 * backward: cgd_op_attn_bwd fails (-2) on the buffers of a causal forward. */
int cgd_op_attn_fwd_causal(cgd_ctx* ctx, const float* qkv, float* out, int nb, int heads, int T, int d, float* bufs[5], void* stream);
/* host-only (no GPU, no context): the kernel family cgd_op_attn_fwd / _bwd (and the UNet / ViT towers) pick for one attention shape.  ldq / ldo =
 * row strides of qkv and of out / dout in floats; precision as in cgd_ctx_create; attn_flash = the CGD_ATTN_FLASH knob (0..3), < 0 = its default.
 * out2 = {family: 0 batched GEMMs + row softmax (any head dim), 1 attn_s64_* (d = 64, T <= 64), 2 attn_mid_* (d = 64, T > 64, probabilities
 * materialised), 3 attn_flash_* (row statistics only); kernel launches of the backward of a fused family (0 for family 0)}.  The forward and the
 * backward of a call use the same family: the backward fails (-2, cgd_last_error) rather than fall back when dqkv's rows are not 16-byte aligned,
 * or when the forward that filled the buffers ran another family (a different dout stride, a precision change between the passes).
 * The plan is that of a FRESH context: CGD_ATTN_X3 / CGD_ATTN_FLASH of the environment are not read (pass attn_flash explicitly). */
int cgd_op_attn_plan(int T, int d, int ldq, int ldo, int precision, int attn_flash, int* out2);

#ifdef __cplusplus
}
#endif
#endif
