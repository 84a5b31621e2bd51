"""Handles of the two device networks behind the C ABI.

`UNet` mirrors the callable the reference hands to the sampler, `model(x, timesteps, y)`
(/root/reference/cgd/cgd.py:251, built by /root/reference/cgd/script_util.py:281-324); `ClipImageTower`
mirrors `clip_model.encode_image` + `.visual.input_resolution` (/root/reference/cgd/clip_util.py:59-66,
/root/reference/cgd/cgd.py:194).  Both add `dgrad`, the hand-derived backward-to-input that replaces
`th.autograd.grad(loss, x)` (cgd.py:228).  `ClipTextTower` mirrors `clip_model.encode_text` (prompt encoding, forward only).
"""
import ctypes as C

import torch as th

from . import lib as L

DEFAULT_CHANNEL_MULT = {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4), 64: (1, 2, 3, 4)}

VIT_CONFIGS = {
    # name: (resolution, patch, width, layers, heads, out_dim)   (clip/model.py)
    "ViT-B/32": (224, 32, 768, 12, 12, 512),
    "ViT-B/16": (224, 16, 768, 12, 12, 512),
    "ViT-L/14": (224, 14, 1024, 24, 16, 768),
}

TEXT_CONFIGS = {
    # name: (context_length, vocab_size, width, layers, heads, out_dim) of the text tower of each published CLIP model
    # (clip/model.py build_model: width = ln_final.weight.shape[0], heads = width // 64, out_dim = text_projection.shape[1])
    "ViT-B/16": (77, 49408, 512, 12, 8, 512),
    "ViT-B/32": (77, 49408, 512, 12, 8, 512),
    "RN50": (77, 49408, 512, 12, 8, 1024),
    "RN101": (77, 49408, 512, 12, 8, 512),
    "RN50x4": (77, 49408, 640, 12, 10, 640),
    "RN50x16": (77, 49408, 768, 12, 12, 768),
    "ViT-L/14": (77, 49408, 768, 12, 12, 768),
}


OPENCLIP_CONFIGS = {
    # open_clip (LAION) ViT architectures, dash-spelled as open_clip spells them (OpenAI's names are slash-spelled: no collision):
    # name: (image tower (resolution, patch, width, layers, heads, out_dim), text tower (context_length, vocab_size, width, layers, heads, out_dim)).
    # Written from memory of open_clip's model configs; loading a checkpoint cross-checks every dimension a shape reveals (cgd.clip_util).
    # All four were trained with the exact GELU; "<name>-quickgelu" (open_clip's own suffix) selects QuickGELU.  ViT-H-14: head dim 80.
    "ViT-B-32": ((224, 32, 768, 12, 12, 512), (77, 49408, 512, 12, 8, 512)),
    "ViT-B-16": ((224, 16, 768, 12, 12, 512), (77, 49408, 512, 12, 8, 512)),
    "ViT-L-14": ((224, 14, 1024, 24, 16, 768), (77, 49408, 768, 12, 12, 768)),
    "ViT-H-14": ((224, 14, 1280, 32, 16, 1024), (77, 49408, 1024, 24, 16, 1024)),
}

ACTIVATIONS = {"quick_gelu": 2, "gelu": 3}  # the codes of cgd_vit_set_activation / cgd_text_set_activation / cgd_op_act


def openclip_arch(name):
    """'ViT-H-14' -> ('ViT-H-14', 'gelu'); 'ViT-B-32-quickgelu' -> ('ViT-B-32', 'quick_gelu'); anything else -> None."""
    base, act = (name[:-len("-quickgelu")], "quick_gelu") if name.endswith("-quickgelu") else (name, "gelu")
    return (base, act) if base in OPENCLIP_CONFIGS else None


def _activation_code(activation):
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}, got {activation!r}")
    return ACTIVATIONS[activation]


class _Net:
    _prefix = None

    def _fn(self, name):
        return getattr(self.ctx.lib, f"cgd_{self._prefix}_{name}")

    def param_specs(self):
        n = self._fn("num_params")(self.h)
        buf = C.create_string_buffer(256)
        numel = C.c_int64()
        out = []
        for i in range(n):
            self.ctx.check(self._fn("param_info")(self.h, i, buf, 256, C.byref(numel)))
            out.append((buf.value.decode(), numel.value))
        return out

    def load_state_dict(self, sd, prefix=""):
        """Upload every parameter (fp32) and pack the forward / dgrad weight layouts.  Safe on any stream: cgd_*_set_param and
        cgd_*_finalize run on the null stream, which a created (non-blocking) stream does not order with, so the current stream of the
        context's device is drained once before the first upload — the conversions to fp32 enqueued here, whatever produced a device
        state dict on that stream, and a pass of this handle that is still in flight."""
        staged = []
        for name, numel in self.param_specs():
            key = prefix + name
            if key not in sd:
                raise KeyError(f"missing parameter {key}")
            t = sd[key].detach().to(dtype=th.float32).contiguous()
            if t.numel() != numel:
                raise ValueError(f"{key}: expected {numel} elements, got {t.numel()}")
            staged.append((name, t, numel))
        th.cuda.current_stream(self.ctx.device).synchronize()
        for name, t, numel in staged:
            self.ctx.check(self._fn("set_param")(self.h, name.encode(), t.data_ptr(), numel))
        self.ctx.check(self._fn("finalize")(self.h))
        return self

    def _adopt(self, h):
        self.h = h
        self.ctx._nets.add(self)  # the context closes its networks before it goes away (their handles point into it)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):  # after Context.close() the native side is already gone
                self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UNet(_Net):
    _prefix = "unet"

    def __init__(self, ctx, image_size, model_channels, num_res_blocks, attention_resolutions="32,16,8", channel_mult=None,
                 num_classes=None, num_heads=4, num_head_channels=-1, use_new_attention_order=False, in_channels=3,
                 out_channels=6, resblock_updown=True, use_scale_shift_norm=True):
        self.ctx = ctx
        cfg = self.make_config(image_size, model_channels, num_res_blocks, attention_resolutions, channel_mult, num_classes, num_heads,
                               num_head_channels, use_new_attention_order, in_channels, out_channels, resblock_updown, use_scale_shift_norm)
        self.cfg = cfg
        self.num_classes = num_classes
        self.in_channels = in_channels
        self.out_channels = out_channels
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_unet_create(ctx.h, C.byref(cfg), C.byref(h)))
        self._adopt(h)

    @staticmethod
    def make_config(image_size, model_channels, num_res_blocks, attention_resolutions="32,16,8", channel_mult=None, num_classes=None,
                    num_heads=4, num_head_channels=-1, use_new_attention_order=False, in_channels=3, out_channels=6, resblock_updown=True,
                    use_scale_shift_norm=True):
        """guided_diffusion's create_model arguments -> the C struct (host-only: also feeds cgd_unet_manifest in the CPU tests).
        resblock_updown=False: Downsample / Upsample are convs (conv_resample=True); use_scale_shift_norm=False: the timestep embedding is
        added to conv1's output instead of modulating the second norm.  The defaults are the published guided-diffusion checkpoints'."""
        if channel_mult is None:
            channel_mult = DEFAULT_CHANNEL_MULT[image_size]
        att = [image_size // int(r) for r in str(attention_resolutions).split(",") if r.strip()]  # "": attention in the middle block only
        cfg = L.UNetConfig()
        cfg.image_size, cfg.model_channels, cfg.num_res_blocks = image_size, model_channels, num_res_blocks
        cfg.n_mult = len(channel_mult)
        for i, m in enumerate(channel_mult):
            cfg.channel_mult[i] = float(m)
        cfg.n_att = len(att)
        for i, a in enumerate(att):
            cfg.attention_ds[i] = a
        cfg.num_classes = int(num_classes or 0)
        cfg.num_heads, cfg.num_head_channels = num_heads, num_head_channels
        cfg.use_new_attention_order = int(bool(use_new_attention_order))
        cfg.in_channels, cfg.out_channels = in_channels, out_channels
        cfg.classic_resample = int(not resblock_updown)
        cfg.additive_emb = int(not use_scale_shift_norm)
        return cfg

    def set_low_res(self, low_res):
        """Super-resolution handles (in_channels=6; guided-diffusion's SuperResModel): the low-resolution image, (1 or B,3,h,w) in [-1,1],
        that conditions every later forward until it is replaced.  The forward upsamples it bilinearly to x's frame and feeds
        cat([x, upsampled]) to the stem, in one launch; x stays (B,3,H,W) and dgrad returns (B,3,H,W).  The handle keeps its own copy."""
        if not th.is_tensor(low_res) or low_res.dim() != 4 or low_res.shape[1] != 3 or 0 in low_res.shape:
            raise ValueError(f"low_res must be (1 or B, 3, h, w), got {tuple(low_res.shape) if th.is_tensor(low_res) else type(low_res).__name__}")
        low = low_res.detach().to(device=f"cuda:{self.ctx.device}", dtype=th.float32).contiguous()
        n, _, h, w = low.shape
        self.ctx.check(self.ctx.lib.cgd_unet_set_low_res(self.h, low.data_ptr(), n, h, w, self.ctx.stream()))
        self._keep_low = low  # the copy is enqueued on the stream: the source outlives it here
        return self

    def forward(self, x, timesteps, y=None, out=None):
        """x (B,3,H,W) fp32 NCHW on the GPU; timesteps (B,) (any dtype; converted to fp32); y (B,) int64."""
        B, _, H, W = x.shape
        x = x.contiguous().float()
        t = timesteps.to(device=x.device, dtype=th.float32).contiguous()
        if y is not None:
            y = y.to(device=x.device, dtype=th.int64).contiguous()
        if out is None:
            out = th.empty((B, self.out_channels, H, W), device=x.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_unet_forward(self.h, x.data_ptr(), t.data_ptr(), L.ptr(y), out.data_ptr(), B, H, W,
                                                     self.ctx.stream()))
        self._keep = (x, t, y)  # inputs must outlive the enqueued work
        return out

    def embed(self, timesteps, y, slot):
        """The (t, y)-only head of model(x, t, y) — time / class embedding and all FiLM projections — into buffer `slot` (0 / 1), on the current
        stream.  `forward_slot` then runs the rest; the sampler uses the pair to take the head off the step's critical path."""
        t = timesteps.to(dtype=th.float32).contiguous()
        if y is not None:
            y = y.to(dtype=th.int64).contiguous()
        self.ctx.check(self.ctx.lib.cgd_unet_embed(self.h, t.data_ptr(), L.ptr(y), int(t.shape[0]), int(slot), self.ctx.stream()))
        if not hasattr(self, "_keep_emb"):
            self._keep_emb = {}
        self._keep_emb[int(slot)] = (t, y)  # inputs must outlive the enqueued work

    def forward_slot(self, x, slot, out=None):
        """model(x, t, y) with the embedding head already computed by embed(t, y, slot)."""
        B, _, H, W = x.shape
        x = x.contiguous().float()
        if out is None:
            out = th.empty((B, self.out_channels, H, W), device=x.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_unet_forward_slot(self.h, x.data_ptr(), int(slot), out.data_ptr(), B, H, W, self.ctx.stream()))
        self._keep = (x,)
        return out

    def __call__(self, x, timesteps, y=None, out=None):
        """model(x, timesteps, y) as the sampler and user cond_fns call it: an autograd node when `x` requires grad."""
        if x.requires_grad and th.is_grad_enabled():
            return UNetFunction.apply(x, self, timesteps, y)
        return self.forward(x, timesteps, y, out)

    def dgrad(self, g_out, g_x=None):
        """d(sum(out*g_out))/dx for the last forward."""
        g_out = g_out.contiguous().float()
        B, _, H, W = g_out.shape
        if g_x is None:
            g_x = th.empty((B, 3, H, W), device=g_out.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_unet_dgrad(self.h, g_out.data_ptr(), g_x.data_ptr(), self.ctx.stream()))
        self._keep_g = g_out
        return g_x


class UNetFunction(th.autograd.Function):
    """model(x, ts, y) as an autograd node: backward = cgd_unet_dgrad of the LAST forward (only d/dx exists)."""

    @staticmethod
    def forward(ctx, x, unet, ts, y):
        ctx.unet = unet
        return unet.forward(x.detach(), ts, y)

    @staticmethod
    def backward(ctx, g):
        return ctx.unet.dgrad(g.contiguous()), None, None, None


class WindowedUNet:
    """Windowed sampling (MultiDiffusion, Bar-Tal et al., 2023) as a model wrapper: a frame larger than the checkpoint's trained size is cut
    into overlapping windows of that size (windows.WindowPlan: `stride` apart, the last one flush with the edge; `wrap` in '', 'x', 'y',
    'xy' lets them run over the right / bottom edge and continue at 0, which makes the frame tile along that axis).  `forward` gathers the
    windows of `x` (cgd_window_gather), runs the wrapped net on all of them as one batch and averages the window outputs, all channels alike,
    into one prediction for the frame (cgd_window_merge with the plan's weights: the plain average, or sin^2 weights with `feather`);
    `dgrad` runs the adjoints in reverse, so it is the exact gradient of `forward`.  Same surface as `UNet` where the sampler and
    ClipGuidance use it (ctx, forward, __call__, dgrad, num_classes, in_channels, out_channels; other attributes are the wrapped net's), but
    no embed / forward_slot: the embedding head cannot run ahead of a windowed forward.  All windows go through one forward, because dgrad
    differentiates the handle's last forward; a frame whose windows do not fit in memory raises the ordinary out-of-memory error."""

    def __init__(self, unet, stride, wrap="", feather=False, window=None):
        from . import windows
        if getattr(unet, "in_channels", 3) != 3:
            raise ValueError("windowed sampling wraps a 3-channel UNet: super-resolution on windows is not built")
        size = int(unet.cfg.image_size)
        if window is not None and int(window) != size:
            raise ValueError(f"the window side is the wrapped net's image_size {size}, got {window!r}")
        if wrap not in windows.WRAPS:
            raise ValueError(f"wrap must be one of {sorted(windows.WRAPS)}, got {wrap!r}")
        windows.window_origins(size, size, stride)  # refuses a stride that is no positive multiple of 8 or exceeds the window
        self.unet, self.ctx = unet, unet.ctx
        self.window, self.stride, self.wrap, self.feather = size, int(stride), wrap, bool(feather)
        self.num_classes, self.in_channels, self.out_channels = unet.num_classes, unet.in_channels, unet.out_channels
        self._plans = {}
        self._last = None  # the plan and batch of the last forward: dgrad differentiates that one

    def __getattr__(self, name):  # only what the wrapper does not define itself
        if name in ("embed", "forward_slot", "unet"):
            raise AttributeError(name)
        return getattr(self.unet, name)

    def set_low_res(self, low_res):
        raise ValueError("windowed sampling does not take a low-resolution condition: super-resolution on windows is not built")

    def plan(self, H, W):
        """The window plan of an (H, W) frame, tables on the device; cached per shape."""
        from . import windows
        p = self._plans.get((H, W))
        if p is None:
            p = self._plans[(H, W)] = windows.WindowPlan(H, W, self.window, self.stride, self.wrap, self.feather).to(f"cuda:{self.ctx.device}")
            p.c_oy, p.c_ox = (C.c_int * p.ny)(*p.oy), (C.c_int * p.nx)(*p.ox)
            p.bufs = {}  # the window batches of this frame shape, by (role, B, channels)
        return p

    def _gather(self, p, full, win, weighted):
        B, Cn = full.shape[:2]
        self.ctx.check(self.ctx.lib.cgd_window_gather(self.ctx.h, full.data_ptr(), win.data_ptr(), p.c_oy, p.ny, p.c_ox, p.nx,
                                                      p.ay.data_ptr() if weighted else None, p.ax.data_ptr() if weighted else None,
                                                      B, Cn, p.H, p.W, p.S, p.wrap, self.ctx.stream()))

    def _merge(self, p, win, full, weighted):
        B, Cn = full.shape[:2]
        self.ctx.check(self.ctx.lib.cgd_window_merge(self.ctx.h, win.data_ptr(), full.data_ptr(), p.c_oy, p.ny, p.c_ox, p.nx,
                                                     p.ay.data_ptr() if weighted else None, p.ax.data_ptr() if weighted else None,
                                                     B, Cn, p.H, p.W, p.S, p.wrap, 0, self.ctx.stream()))

    def _buf(self, p, name, B, Cn, dev):
        t = p.bufs.get((name, B, Cn))
        if t is None or t.device != dev:
            t = p.bufs[(name, B, Cn)] = th.empty((B * p.n, Cn, p.S, p.S), device=dev, dtype=th.float32)
        return t

    def forward(self, x, timesteps, y=None, out=None):
        """x (B,3,H,W) fp32 NCHW on the GPU, H and W multiples of 8 and at least the window side; timesteps (B,), y (B,) as for UNet.forward:
        every window of sample b runs at timesteps[b] and y[b]."""
        B, _, H, W = x.shape
        x = x.contiguous().float()
        p = self.plan(H, W)
        xw = self._buf(p, "x", B, 3, x.device)
        self._gather(p, x, xw, False)
        t = timesteps.to(device=x.device, dtype=th.float32).repeat_interleave(p.n)
        if y is not None:
            y = y.to(device=x.device, dtype=th.int64).repeat_interleave(p.n)
        ow = self.unet.forward(xw, t, y, out=self._buf(p, "out", B, self.out_channels, x.device))
        if out is None:
            out = th.empty((B, self.out_channels, H, W), device=x.device, dtype=th.float32)
        self._merge(p, ow, out, True)
        self._last, self._keep = (p, B), x  # inputs must outlive the enqueued work
        return out

    def __call__(self, x, timesteps, y=None, out=None):
        """model(x, timesteps, y): an autograd node (UNetFunction, over this wrapper's forward / dgrad) when `x` requires grad."""
        if x.requires_grad and th.is_grad_enabled():
            return UNetFunction.apply(x, self, timesteps, y)
        return self.forward(x, timesteps, y, out)

    def dgrad(self, g_out, g_x=None):
        """d(sum(out*g_out))/dx for the last forward: the merge's adjoint (a weighted gather), the wrapped net's dgrad on all windows, the
        gather's adjoint (an unweighted merge)."""
        if self._last is None:
            raise RuntimeError("WindowedUNet.dgrad: no forward to differentiate")
        p, B = self._last
        g_out = g_out.contiguous().float()
        if tuple(g_out.shape) != (B, self.out_channels, p.H, p.W):
            raise ValueError(f"g_out must have the last forward's output shape {(B, self.out_channels, p.H, p.W)}, got {tuple(g_out.shape)}")
        gw = self._buf(p, "g_out", B, self.out_channels, g_out.device)
        self._gather(p, g_out, gw, True)
        gxw = self.unet.dgrad(gw, self._buf(p, "g_x", B, 3, g_out.device))
        if g_x is None:
            g_x = th.empty((B, 3, p.H, p.W), device=g_out.device, dtype=th.float32)
        self._merge(p, gxw, g_x, False)
        self._keep_g = g_out
        return g_x


class ClipImageTower(_Net):
    _prefix = "vit"

    def __init__(self, ctx, name="ViT-B/32", config=None, activation="quick_gelu"):
        """activation: "quick_gelu" (OpenAI's checkpoints) or "gelu" (the exact GELU of the open_clip / LAION checkpoints)."""
        self.ctx = ctx
        act = _activation_code(activation)
        res, patch, width, layers, heads, out = config or VIT_CONFIGS[name]
        cfg = L.ViTConfig(res, patch, width, layers, heads, out)
        self.cfg = cfg
        self.input_resolution = res
        self.patch, self.out_dim = patch, out
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_vit_create(ctx.h, C.byref(cfg), C.byref(h)))
        self._adopt(h)
        self.activation = activation
        if act != ACTIVATIONS["quick_gelu"]:
            ctx.check(ctx.lib.cgd_vit_set_activation(h, act))
        self._layout = 0
        self._n = 0

    def load_clip_state_dict(self, sd):
        """Accepts an OpenAI CLIP state dict (keys `visual.*`) or a bare visual-tower dict."""
        prefix = "visual." if any(k.startswith("visual.") for k in sd) else ""
        return self.load_state_dict(sd, prefix)

    def encode_image(self, img, layout=0, n=None, out=None):
        """layout 0: (N,3,res,res) NCHW already CLIP-normalised; layout 1: patch rows from cutouts_fwd."""
        img = img.contiguous().float()
        N = img.shape[0] if layout == 0 else int(n)
        if out is None:
            out = th.empty((N, self.out_dim), device=img.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_vit_forward(self.h, img.data_ptr(), layout, N, out.data_ptr(), self.ctx.stream()))
        self._layout, self._n, self._keep = layout, N, img
        return out

    def dgrad(self, d_emb, d_img=None):
        d_emb = d_emb.contiguous().float()
        if d_img is None:
            d_img = th.empty_like(self._keep)
        self.ctx.check(self.ctx.lib.cgd_vit_dgrad(self.h, d_emb.data_ptr(), d_img.data_ptr(), self.ctx.stream()))
        self._keep_g = d_emb
        return d_img


class EncodeImageFunction(th.autograd.Function):
    """tower.encode_image as an autograd node; backward = the tower's hand-derived backward-to-image of its LAST forward."""

    @staticmethod
    def forward(ctx, image, tower):
        ctx.tower, ctx.in_shape = tower, tuple(image.shape)
        return tower.encode_image(image.detach().float().contiguous())

    @staticmethod
    def backward(ctx, d_emb):
        return ctx.tower.dgrad(d_emb.float().contiguous()).view(ctx.in_shape), None


class ClipTextTower(_Net):
    """`clip_model.encode_text(tokens)` (clip.model.CLIP.encode_text) on the device: forward only, in the context's precision mode."""
    _prefix = "text"

    def __init__(self, ctx, name="ViT-B/32", config=None, activation="quick_gelu"):
        self.ctx = ctx
        act = _activation_code(activation)
        T, vocab, width, layers, heads, out = config or TEXT_CONFIGS[name]
        self.cfg = L.TextConfig(T, vocab, width, layers, heads, out)
        self.context_length, self.vocab_size, self.width, self.out_dim = T, vocab, width, out
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_text_create(ctx.h, C.byref(self.cfg), C.byref(h)))
        self._adopt(h)
        self.activation = activation
        if act != ACTIVATIONS["quick_gelu"]:
            ctx.check(ctx.lib.cgd_text_set_activation(h, act))

    def load_clip_state_dict(self, sd):
        """An OpenAI CLIP state dict: the text tower's keys are top-level (`visual.*` and `logit_scale` are not read)."""
        return self.load_state_dict(sd)

    def encode_text(self, tokens, out=None):
        """tokens (N, context_length) integer ids in [0, vocab_size) -> (N, out_dim) fp32."""
        if tokens.dim() != 2 or tokens.shape[1] != self.context_length:
            raise ValueError(f"tokens must be (N, {self.context_length}), got {tuple(tokens.shape)}")
        if tokens.is_floating_point() or tokens.is_complex() or tokens.dtype == th.bool:
            raise ValueError(f"tokens must be integer ids, got {tokens.dtype}")
        if tokens.shape[0] == 0:
            raise ValueError("tokens: empty batch")
        lo, hi = int(tokens.min()), int(tokens.max())
        if lo < 0 or hi >= self.vocab_size:
            raise ValueError(f"token ids must lie in [0, {self.vocab_size}), got [{lo}, {hi}]")
        tok = tokens.to(device=f"cuda:{self.ctx.device}", dtype=th.int64).contiguous()
        if out is None:
            out = th.empty((tok.shape[0], self.out_dim), device=tok.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_text_forward(self.h, tok.data_ptr(), tok.shape[0], out.data_ptr(), self.ctx.stream()))
        self._keep = tok  # the launch reads it asynchronously
        return out


RN_CONFIGS = {
    # name: (resolution, width, layers, out_dim, heads)   (clip/model.py ModifiedResNet)
    "RN50": (224, 64, (3, 4, 6, 3), 1024, 32),
    "RN101": (224, 64, (3, 4, 23, 3), 512, 32),
    "RN50x4": (288, 80, (4, 6, 10, 6), 640, 40),    # widths 40 / 80 are zero-padded to 64 / 96 channels on the device
    "RN50x16": (384, 96, (6, 8, 18, 8), 768, 48),
}


class ClipResNetTower(_Net):
    """CLIP ModifiedResNet image tower (RN50 / RN101): `encode_image` + `dgrad`, same role as `ClipImageTower`.  `patch` is 0:
    the cutout kernel hands it plain (N,3,res,res) images (layout 0)."""
    _prefix = "rn"
    patch = 0

    def __init__(self, ctx, name="RN50", config=None):
        self.ctx = ctx
        res, width, layers, out, heads = config or RN_CONFIGS[name]
        cfg = self.make_config(res, width, layers, out, heads)
        self.cfg = cfg
        self.input_resolution, self.out_dim = res, out
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_rn_create(ctx.h, C.byref(cfg), C.byref(h)))
        self._adopt(h)

    @staticmethod
    def make_config(res, width, layers, out, heads):
        cfg = L.RNConfig()
        cfg.resolution, cfg.width, cfg.out_dim, cfg.heads = res, width, out, heads
        for i, v in enumerate(layers):
            cfg.layers[i] = v
        return cfg

    def load_clip_state_dict(self, sd):
        prefix = "visual." if any(k.startswith("visual.") for k in sd) else ""
        return self.load_state_dict(sd, prefix)

    def encode_image(self, img, layout=0, n=None, out=None):
        assert layout == 0, "the ResNet tower takes NCHW images"
        img = img.contiguous().float()
        N = img.shape[0]
        if out is None:
            out = th.empty((N, self.out_dim), device=img.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_rn_forward(self.h, img.data_ptr(), N, out.data_ptr(), self.ctx.stream()))
        self._keep = img
        return out

    def dgrad(self, d_emb, d_img=None):
        d_emb = d_emb.contiguous().float()
        if d_img is None:
            d_img = th.empty_like(self._keep)
        self.ctx.check(self.ctx.lib.cgd_rn_dgrad(self.h, d_emb.data_ptr(), d_img.data_ptr(), self.ctx.stream()))
        self._keep_g = d_emb
        return d_img


class LpipsVGG(_Net):
    """`lpips.LPIPS(net='vgg')` against a fixed reference image (/root/reference/cgd/cgd.py:147-148,220-224): value per sample and
    gradient w.r.t. the first argument.  `load_state_dict` takes the package's keys (`net.slice{k}.{idx}.*`, `lin{k}.model.1.weight`)."""
    _prefix = "lpips"

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_lpips_create(ctx.h, C.byref(h)))
        self._adopt(h)
        self._ref = None

    def set_reference(self, ref):
        """ref (B,3,H,W) in [-1,1] (the init image); H, W multiples of 16."""
        ref = ref.contiguous().float()
        B, _, H, W = ref.shape
        self.ctx.check(self.ctx.lib.cgd_lpips_set_reference(self.h, ref.data_ptr(), B, H, W, self.ctx.stream()))
        self._ref = ref
        return self

    def loss_grad(self, x, grad_scale=1.0, g=None, accumulate=False, loss=None):
        """Returns (loss (B,), g (B,3,H,W)) with g (+)= grad_scale * d(sum loss)/dx."""
        x = x.contiguous().float()
        assert self._ref is not None and tuple(x.shape) == tuple(self._ref.shape), "set_reference first (same shape)"
        if g is None:
            g = th.zeros_like(x) if accumulate else th.empty_like(x)
        if loss is None:
            loss = th.empty(x.shape[0], device=x.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_lpips_loss_grad(self.h, x.data_ptr(), float(grad_scale), loss.data_ptr(), g.data_ptr(),
                                                       int(bool(accumulate)), self.ctx.stream()))
        self._keep = x
        return loss, g

    def set_style(self, img, weights=(1, 1, 1, 1, 0)):
        """img (1,3,Hs,Ws) or (3,Hs,Ws) in [-1,1], the ONE style image; Hs, Ws multiples of 16, otherwise free.  weights: lambda_k of the five taps
        (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3) in L_style = sum_k lambda_k |G_k(x) - G_k(style)|_F^2, G_k = A_k^T A_k / (C_k N_k); a tap with weight 0
        is skipped everywhere.  A reference set by `set_reference` stays intact."""
        img = img.contiguous().float()
        if img.dim() == 3:
            img = img[None]
        if img.dim() != 4 or img.shape[0] != 1 or img.shape[1] != 3:
            raise ValueError(f"style image must be (1,3,H,W), got {tuple(img.shape)}")
        weights = tuple(float(w) for w in weights)
        if len(weights) != 5:
            raise ValueError("style weights: one per tap, five in all")
        lam = (C.c_float * 5)(*weights)
        self.ctx.check(self.ctx.lib.cgd_lpips_set_style(self.h, img.data_ptr(), img.shape[2], img.shape[3], lam, self.ctx.stream()))
        self._style = True
        return self

    def style_loss_grad(self, x, style_scale=1.0, lpips_scale=None, g=None, accumulate=False, style_loss=None, lpips_loss=None):
        """One trunk pass for both terms.  Returns (style_loss (B,), lpips_loss (B,) or None, g (B,3,H,W)) with
        g (+)= style_scale * d(sum style_loss)/dx [+ lpips_scale * d(sum lpips_loss)/dx].  lpips_scale=None: the style term alone (no reference needed)."""
        x = x.contiguous().float()
        assert getattr(self, "_style", False), "set_style first"
        if lpips_scale is not None:
            assert self._ref is not None and tuple(x.shape) == tuple(self._ref.shape), "set_reference first (same shape)"
        B, _, H, W = x.shape
        if g is None:
            g = th.zeros_like(x) if accumulate else th.empty_like(x)
        if style_loss is None:
            style_loss = th.empty(B, device=x.device, dtype=th.float32)
        if lpips_scale is not None and lpips_loss is None:
            lpips_loss = th.empty(B, device=x.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_lpips_style_loss_grad(
            self.h, x.data_ptr(), B, H, W, float(lpips_scale or 0.0), float(style_scale), lpips_loss.data_ptr() if lpips_scale is not None else None,
            style_loss.data_ptr(), g.data_ptr(), int(bool(accumulate)), self.ctx.stream()))
        self._keep = x
        return style_loss, (lpips_loss if lpips_scale is not None else None), g


class SecondaryModel(_Net):
    """The secondary diffusion model (SecondaryDiffusionImageNet2 of Katherine Crowson's CLIP-guided diffusion notebooks, also shipped with
    Disco Diffusion): a small convolutional denoiser whose prediction of the clean image stands in for the UNet's in the guidance losses, so
    that their gradient returns to `x` through this net instead of through the UNet.  `load_state_dict` takes the module's own keys
    (`net.0.0.weight` ... `net.4.bias`, `timestep_embed.weight`): the published secondary_model_imagenet_2.pth loads by name.  H and W must be
    multiples of 32."""
    _prefix = "secondary"

    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_secondary_create(ctx.h, C.byref(h)))
        self._adopt(h)
        self.dgrad_calls = 0

    @staticmethod
    def model_time(alpha, sigma):
        """The model's time t in [0, 1] of a noise level: x_t = alpha x_0 + sigma eps with alpha = cos(t pi / 2), sigma = sin(t pi / 2)."""
        import math
        return math.atan2(float(sigma), float(alpha)) * 2.0 / math.pi

    def forward(self, x, t, fac=None, pred=None, x_in=None):
        """x (B,3,H,W) fp32 NCHW on the GPU, t (B,) the model's time -> pred; with `fac` also x_in = pred fac + x (1 - fac), from the same
        launch: returns (pred, x_in)."""
        x = x.contiguous().float()
        B, _, H, W = x.shape
        t = t.to(device=x.device, dtype=th.float32).contiguous()
        if pred is None:
            pred = th.empty_like(x)
        if fac is None:
            self.ctx.check(self.ctx.lib.cgd_secondary_forward(self.h, x.data_ptr(), t.data_ptr(), B, H, W, pred.data_ptr(), self.ctx.stream()))
            self._keep = (x, t)  # inputs must outlive the enqueued work
            return pred
        if x_in is None:
            x_in = th.empty_like(x)
        self.ctx.check(self.ctx.lib.cgd_secondary_forward_blend(self.h, x.data_ptr(), t.data_ptr(), B, H, W, float(fac), pred.data_ptr(),
                                                                x_in.data_ptr(), self.ctx.stream()))
        self._keep = (x, t)
        return pred, x_in

    def dgrad(self, dv, dx=None):
        """d(sum(v * dv))/dx of the last forward, v = the net's raw output (pred = x alpha - v sigma)."""
        dv = dv.contiguous().float()
        if dx is None:
            dx = th.empty_like(dv)
        self.ctx.check(self.ctx.lib.cgd_secondary_dgrad(self.h, dv.data_ptr(), dx.data_ptr(), self.ctx.stream()))
        self._keep_g = dv
        self.dgrad_calls += 1
        return dx

    def debug_replay(self, acts):
        """Test support (cgd_secondary_debug_replay): 23 post-ReLU activations as dense NHWC rows on the device, or None to switch it off."""
        if acts is None:
            self._replay = None
            self.ctx.check(self.ctx.lib.cgd_secondary_debug_replay(self.h, None))
            return
        self._replay = [a.contiguous().float() for a in acts]
        arr = (C.c_void_p * len(self._replay))(*[a.data_ptr() for a in self._replay])
        assert len(self._replay) == 23
        self.ctx.check(self.ctx.lib.cgd_secondary_debug_replay(self.h, arr))


def collapse_aesthetic_state_dict(sd):
    """A published aesthetic-predictor checkpoint -> the (D + 1,) float64 host vector (a, beta) with score = a . normalize(e) + beta.  Two
    formats, written from memory of the upstream repositories and therefore cross-checked shape by shape here:
      LAION-AI/aesthetic-predictor (sa_0_4_vit_b_32_linear.pth, ..._b_16_..., ..._l_14_...): the state dict of nn.Linear(D, 1), `weight` (1, D)
        and `bias` (1,);
      improved-aesthetic-predictor (sac+logos+ava1-l14-linearMSE.pth and siblings): `layers.{0,2,4,6,7}.weight` / `.bias` of the chain
        768 -> 1024 -> 128 -> 64 -> 16 -> 1 with only dropout in between, which is the identity at inference: no active non-linearity.
    The rule is the general one, not the key list: the 2-D `*.weight` tensors in key order must chain (each one's input width is the one
    before's output width) from some D down to 1, every one with a `*.bias` of its output width (or none); the chain is collapsed in float64,
    a = W_n ... W_1 and beta chained likewise.  A {'state_dict': ...} wrapper and `module.` prefixes are removed.  ValueError names what does
    not fit; any tensor that is neither such a weight nor its bias is refused too (a layer this rule would drop silently)."""
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    if not isinstance(sd, dict):
        raise ValueError(f"aesthetic head: expected a state dict, got {type(sd).__name__}")
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items() if isinstance(v, th.Tensor)}
    names = [k for k in sd if (k == "weight" or k.endswith(".weight")) and sd[k].dim() == 2]
    if not names:
        raise ValueError(f"aesthetic head: no 2-D '*.weight' tensor among {sorted(sd)[:8]}")
    used = set(names)
    a, beta = None, None
    for k in names:
        w = sd[k].detach().double().cpu()
        bias_key = k[:-len("weight")] + "bias"
        b = sd.get(bias_key)
        if b is not None:
            used.add(bias_key)
            b = b.detach().double().cpu().flatten()
            if b.numel() != w.shape[0]:
                raise ValueError(f"aesthetic head: '{bias_key}' has {b.numel()} elements, '{k}' has {w.shape[0]} outputs")
        else:
            b = th.zeros(w.shape[0], dtype=th.float64)
        if a is None:
            a, beta = w, b
        else:
            if w.shape[1] != a.shape[0]:
                raise ValueError(f"aesthetic head: broken chain, '{k}' takes {w.shape[1]} inputs but the layer before it gives {a.shape[0]}")
            a, beta = w @ a, w @ beta + b
    if a.shape[0] != 1:
        raise ValueError(f"aesthetic head: the chain ends in {a.shape[0]} outputs, not in 1 score")
    extra = sorted(set(sd) - used)
    if extra:
        raise ValueError(f"aesthetic head: tensors that are no linear layer of the chain: {extra[:8]}")
    return th.cat([a.flatten(), beta.flatten()])


class AestheticHead:
    """An aesthetic predictor on a tower's image embeddings as the guidance uses it (csrc/aesthetic.hip): `vec`, one (dim + 1,) fp32 device
    tensor holding a (dim) and then beta, score = a . normalize(e) + beta.  Built from a checkpoint's state dict (`from_state_dict`, the two
    formats of collapse_aesthetic_state_dict) or loaded like a network handle (param_specs / load_state_dict with the one entry 'head':
    shard.load_broadcast then reads on rank 0 and broadcasts)."""

    def __init__(self, dim, device="cuda"):
        self.dim, self.device, self.vec = int(dim), device, None
        if self.dim < 1:
            raise ValueError(f"aesthetic head: dim must be positive, got {dim}")

    def param_specs(self):
        return [("head", self.dim + 1)]

    def load_state_dict(self, sd, prefix=""):
        v = sd[prefix + "head"].flatten()
        if v.numel() != self.dim + 1:
            raise ValueError(f"aesthetic head: {v.numel()} values for dim {self.dim} (expected dim + 1)")
        self.vec = v.to(device=self.device, dtype=th.float32).contiguous()
        return self

    @classmethod
    def from_state_dict(cls, sd, device="cuda"):
        v = collapse_aesthetic_state_dict(sd)
        return cls(v.numel() - 1, device).load_state_dict({"head": v})


CLASSIFIER_CONFIGS = {
    # guided-diffusion's create_classifier defaults by image size (64x64_classifier.pt ... 512x512_classifier.pt): width 128, depth 2 (4 at
    # 64x64), attention at resolutions 32,16,8, 64-channel heads, the UNet's channel_mult by size, 1000 classes.  Written from the published
    # source; loading a checkpoint cross-checks every dimension a shape reveals (cgd.clip_util.classifier_config_from_state_dict).
    size: dict(image_size=size, model_channels=128, num_res_blocks=4 if size == 64 else 2, attention_resolutions="32,16,8",
               channel_mult=DEFAULT_CHANNEL_MULT[size], num_head_channels=64, out_channels=1000)
    for size in (64, 128, 256, 512)
}


class NoisyClassifier(_Net):
    """guided-diffusion's noise-aware ImageNet classifier (`EncoderUNetModel`, pool="attention"): `forward` gives the logits and
    log p(y | x_t, t), `dgrad` the gradient of sum_b log p(y_b | x_b, t_b) w.r.t. x — classifier guidance.  `load_state_dict` takes the
    module's own keys (`time_embed.*`, `input_blocks.*`, `middle_block.*`, `out.0.*`, `out.2.*`)."""
    _prefix = "classifier"

    def __init__(self, ctx, image_size, model_channels=128, num_res_blocks=2, attention_resolutions="32,16,8", channel_mult=None,
                 num_head_channels=64, out_channels=1000):
        self.ctx = ctx
        self.cfg = self.make_config(image_size, model_channels, num_res_blocks, attention_resolutions, channel_mult, num_head_channels,
                                    out_channels)
        self.image_size, self.out_channels = image_size, out_channels
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_classifier_create(ctx.h, C.byref(self.cfg), C.byref(h)))
        self._adopt(h)
        self.dgrad_calls = 0

    @staticmethod
    def make_config(image_size, model_channels=128, num_res_blocks=2, attention_resolutions="32,16,8", channel_mult=None,
                    num_head_channels=64, out_channels=1000):
        """guided_diffusion's create_classifier arguments -> the C struct (host-only: also feeds cgd_classifier_manifest)."""
        if channel_mult is None:
            channel_mult = DEFAULT_CHANNEL_MULT[image_size]
        att = [image_size // int(r) for r in str(attention_resolutions).split(",")]
        if len(channel_mult) > 8 or len(att) > 8:
            raise ValueError("classifier: at most 8 levels and 8 attention resolutions")
        cfg = L.ClassifierConfig()
        cfg.image_size, cfg.model_channels, cfg.num_res_blocks = image_size, model_channels, num_res_blocks
        cfg.n_mult = len(channel_mult)
        for i, m in enumerate(channel_mult):
            cfg.channel_mult[i] = float(m)
        cfg.n_att = len(att)
        for i, a in enumerate(att):
            cfg.attention_ds[i] = a
        cfg.num_head_channels, cfg.out_channels = num_head_channels, out_channels
        return cfg

    def forward(self, x, timesteps, y, logits=None, logp=None):
        """x (B,3,S,S) fp32 NCHW on the GPU, S = image_size; timesteps (B,) (converted to fp32); y (B,) class ids.
        Returns (logits (B,out_channels), logp (B,)) with logp[b] = log_softmax(logits[b])[y[b]]."""
        B, _, H, W = x.shape
        x = x.contiguous().float()
        t = timesteps.to(device=x.device, dtype=th.float32).contiguous()
        y = y.to(device=x.device, dtype=th.int64).contiguous()
        if logits is None:
            logits = th.empty((B, self.out_channels), device=x.device, dtype=th.float32)
        if logp is None:
            logp = th.empty((B,), device=x.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_classifier_forward(self.h, x.data_ptr(), t.data_ptr(), y.data_ptr(), logits.data_ptr(), logp.data_ptr(),
                                                           B, H, W, self.ctx.stream()))
        self._keep = (x, t, y)  # inputs must outlive the enqueued work
        return logits, logp

    def dgrad(self, scale=1.0, g=None, accumulate=False):
        """g (+)= scale * d(sum_b logp[b])/dx of the last forward."""
        if g is None:
            x = self._keep[0]
            g = th.zeros_like(x) if accumulate else th.empty_like(x)
        assert g.is_contiguous() and g.dtype == th.float32, "g must be a contiguous fp32 tensor of x's shape"
        self.ctx.check(self.ctx.lib.cgd_classifier_dgrad(self.h, float(scale), g.data_ptr(), int(bool(accumulate)), self.ctx.stream()))
        self.dgrad_calls += 1
        return g


DEPTH_CONFIGS = {
    # name: the fields of cgd_depth_config.  DPT-Large (MiDaS v3, dpt_large-midas-2f21e586.pt): timm's vit_large_patch16_384 with hooks behind
    # blocks 5, 11, 17, 23, trained at a 24 x 24 token grid.  Written from memory of isl-org/DPT; loading a checkpoint cross-checks every shape.
    "dpt_large": dict(patch=16, width=1024, layers=24, heads=16, hooks=(5, 11, 17, 23), native_grid=24, features=256,
                      reassemble_channels=(256, 512, 1024, 1024)),
}
DEPTH_CHECKPOINTS = {"dpt_large-midas-2f21e586.pt": "dpt_large"}
# groups of the published file that the forward does not use
DEPTH_IGNORED_PREFIXES = ("pretrained.model.norm.", "pretrained.model.head.", "scratch.refinenet4.resConfUnit1.")


def depth_config(config):
    """A name of DEPTH_CONFIGS, or a dict of its fields -> (lib.DepthConfig, the dict)."""
    if isinstance(config, str):
        if config not in DEPTH_CONFIGS:
            raise ValueError(f"depth config must be one of {sorted(DEPTH_CONFIGS)} or a dict of its fields, got {config!r}")
        config = DEPTH_CONFIGS[config]
    d = dict(config)
    if len(d["hooks"]) != 4 or len(d["reassemble_channels"]) != 4:
        raise ValueError("depth config: four hooks and four reassemble_channels")
    cfg = L.DepthConfig()
    cfg.patch, cfg.width, cfg.layers, cfg.heads = d["patch"], d["width"], d["layers"], d["heads"]
    cfg.native_grid, cfg.features = d["native_grid"], d["features"]
    for i in range(4):
        cfg.hooks[i] = d["hooks"][i]
        cfg.reassemble_channels[i] = d["reassemble_channels"][i]
    return cfg, d


def depth_param_shapes(config):
    """{key: shape} of every tensor of the published DPT checkpoint layout that the forward uses, for a configuration (host only).  The key
    table is written from memory of isl-org/DPT and timm: no checkpoint was available to check it against."""
    _, d = depth_config(config)
    W, P, F, ng = d["width"], d["patch"], d["features"], d["native_grid"]
    m, out = "pretrained.model.", {}
    out[m + "patch_embed.proj.weight"], out[m + "patch_embed.proj.bias"] = (W, 3, P, P), (W,)
    out[m + "cls_token"], out[m + "pos_embed"] = (1, 1, W), (1, 1 + ng * ng, W)
    for l in range(d["layers"]):
        b = f"{m}blocks.{l}."
        for name, shape in (("norm1", None), ("attn.qkv", (3 * W, W)), ("attn.proj", (W, W)), ("norm2", None), ("mlp.fc1", (4 * W, W)),
                            ("mlp.fc2", (W, 4 * W))):
            out[b + name + ".weight"] = shape or (W,)
            out[b + name + ".bias"] = (shape[0],) if shape else (W,)
    for k, c in enumerate(d["reassemble_channels"]):
        a = f"pretrained.act_postprocess{k + 1}."
        out[a + "0.project.0.weight"], out[a + "0.project.0.bias"] = (W, 2 * W), (W,)
        out[a + "3.weight"], out[a + "3.bias"] = (c, W, 1, 1), (c,)
        ks = {0: 4, 1: 2, 3: 3}.get(k)  # ConvTranspose2d k = s = 4 / 2, Identity, Conv2d 3x3 stride 2
        if ks:
            out[a + "4.weight"], out[a + "4.bias"] = (c, c, ks, ks), (c,)
        out[f"scratch.layer{k + 1}_rn.weight"] = (F, c, 3, 3)
    for k in range(4):
        r = f"scratch.refinenet{k + 1}."
        for unit in ((1, 2) if k < 3 else (2,)):
            for conv in (1, 2):
                out[f"{r}resConfUnit{unit}.conv{conv}.weight"], out[f"{r}resConfUnit{unit}.conv{conv}.bias"] = (F, F, 3, 3), (F,)
        out[r + "out_conv.weight"], out[r + "out_conv.bias"] = (F, F, 1, 1), (F,)
    out["scratch.output_conv.0.weight"], out["scratch.output_conv.0.bias"] = (F // 2, F, 3, 3), (F // 2,)
    out["scratch.output_conv.2.weight"], out["scratch.output_conv.2.bias"] = (32, F // 2, 3, 3), (32,)
    out["scratch.output_conv.4.weight"], out["scratch.output_conv.4.bias"] = (1, 32, 1, 1), (1,)
    return out


def depth_net_size(H, W, size=384):
    """The size the depth net runs a (H, W) frame at: the short side goes to `size`, both sides to the nearest multiple of 32 (at least 32)."""
    import math
    s = size / min(H, W)
    return tuple(max(32, 32 * int(math.floor(side * s / 32 + 0.5))) for side in (H, W))


def depth_resize_pos_embed(pos, native_grid, gh, gw):
    """pos_embed (1, 1 + n n, W) -> the rows (1 + gh gw, W) of a (gh, gw) token grid: the grid part resized bilinearly (align_corners=False),
    the class row kept; the native grid comes back unchanged."""
    pos = pos.reshape(1 + native_grid * native_grid, -1).float()
    if (gh, gw) == (native_grid, native_grid):
        return pos
    grid = pos[1:].reshape(1, native_grid, native_grid, -1).permute(0, 3, 1, 2)
    grid = th.nn.functional.interpolate(grid, size=(gh, gw), mode="bilinear", align_corners=False)
    return th.cat([pos[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, -1)])


class DepthNet(_Net):
    """DPT-Large (MiDaS v3, Ranftl et al., "Vision Transformers for Dense Prediction"), forward only: the depth network of 3D animation.
    `load_state_dict` takes the published dpt_large-midas-2f21e586.pt by its own keys (depth_param_shapes; every shape is cross-checked, a
    missing key or a wrong shape is a ValueError naming it; `pretrained.model.norm.*`, `pretrained.model.head.*` and
    `scratch.refinenet4.resConfUnit1.*` are ignored).  The key table is written from memory: no checkpoint was available to check it against.

    The object is the callable `animate(depth=...)` takes: `net(frame)` with frame (B, 3, H, W) in [0, 1] on the GPU returns (B, 1, H, W)
    fp32, finite and at least `floor`.  The frame goes to depth_net_size(H, W, size) through the antialiased cubic resize (edge-replicating),
    normalised to [-1, 1] in the same launch; the net's inverse depth becomes depth = max((offset - inv_depth) / scale, floor) at net size
    (50 and 19 are Deforum's constants as remembered: typical MiDaS output lands near the flat default 1.0), and the same resize takes it back
    to (H, W), clamped at `floor` again because the cubic overshoots."""
    _prefix = "depth"

    def __init__(self, ctx, config="dpt_large", size=384, offset=50.0, scale=19.0, floor=0.05):
        self.ctx = ctx
        self.cfg, self.config = depth_config(config)
        self.size, self.offset, self.scale, self.floor = int(size), float(offset), float(scale), float(floor)
        if self.size < 32 or not self.scale != 0 or not self.floor > 0:
            raise ValueError(f"DepthNet: size >= 32, scale != 0 and floor > 0 are required, got {size}, {scale}, {floor}")
        h = C.c_void_p()
        ctx.check(ctx.lib.cgd_depth_create(ctx.h, C.byref(self.cfg), C.byref(h)))
        self._adopt(h)
        self._pos, self._grids = None, set()

    def load_state_dict(self, sd, prefix=""):
        shapes = depth_param_shapes(self.config)
        for key, shape in shapes.items():
            if prefix + key not in sd:
                raise ValueError(f"depth checkpoint: missing key {prefix + key}")
            if tuple(sd[prefix + key].shape) != tuple(shape):
                raise ValueError(f"depth checkpoint: {prefix + key} has shape {tuple(sd[prefix + key].shape)}, expected {tuple(shape)}")
        self._pos = sd[prefix + "pretrained.model.pos_embed"].detach().float().cpu()
        self._grids = set()
        return super().load_state_dict(sd, prefix)

    def _ensure_grid(self, gh, gw):
        ng = self.config["native_grid"]
        if (gh, gw) == (ng, ng) or (gh, gw) in self._grids:
            return
        if self._pos is None:
            raise RuntimeError("DepthNet: load_state_dict first")
        rows = depth_resize_pos_embed(self._pos, ng, gh, gw).contiguous()
        th.cuda.current_stream(self.ctx.device).synchronize()  # (the upload is a blocking copy outside the stream's order)
        self.ctx.check(self.ctx.lib.cgd_depth_set_pos_embed(self.h, gh, gw, rows.data_ptr()))
        self._grids.add((gh, gw))

    def forward(self, img, want="inv_depth"):
        """img (B, 3, h, w) fp32 NCHW on the GPU, already normalised to [-1, 1], h and w multiples of 32 -> inv_depth (B, 1, h, w), or with
        want="depth" the mapped depth, or with want="both" the pair."""
        img = img.contiguous().float()
        B, _, h, w = img.shape
        if h % 32 or w % 32:
            raise ValueError(f"DepthNet: the net runs at multiples of 32, got {h} x {w}")
        p = self.config["patch"]
        self._ensure_grid(h // p, w // p)
        inv = th.empty((B, 1, h, w), device=img.device, dtype=th.float32) if want in ("inv_depth", "both") else None
        dep = th.empty((B, 1, h, w), device=img.device, dtype=th.float32) if want in ("depth", "both") else None
        self.ctx.check(self.ctx.lib.cgd_depth_forward(self.h, img.data_ptr(), B, h, w, self.offset, self.scale, self.floor,
                                                      None if inv is None else inv.data_ptr(), None if dep is None else dep.data_ptr(),
                                                      self.ctx.stream()))
        self._keep = img  # inputs must outlive the enqueued work
        return (inv, dep) if want == "both" else (inv if dep is None else dep)

    def debug_map(self, k):
        """Test support: the reassembled map of tap k = 0..3 of the last forward, (B, c_k, h_k, w_k)."""
        out3 = (C.c_int * 3)()
        self.ctx.check(self.ctx.lib.cgd_depth_debug_map(self.h, k, None, out3, self.ctx.stream()))
        B = self._keep.shape[0]
        t = th.empty((B, out3[0], out3[1], out3[2]), device=self._keep.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_depth_debug_map(self.h, k, t.data_ptr(), out3, self.ctx.stream()))
        return t.permute(0, 3, 1, 2)

    def __call__(self, frame):
        from . import ops
        if frame.dim() != 4 or frame.shape[1] != 3:
            raise ValueError(f"DepthNet: expected a (B, 3, H, W) frame, got {tuple(frame.shape)}")
        frame = frame.contiguous().float()
        B, _, H, W = frame.shape
        h, w = depth_net_size(H, W, self.size)
        img = ops.resize_cubic(self.ctx, frame, h, w, a=2.0, b=-1.0)  # (x - 0.5) / 0.5 in the resize's launch
        dep = self.forward(img, want="depth")
        return ops.resize_cubic(self.ctx, dep, H, W, lo=self.floor)


def manifest(kind, cfg=None):
    """[(name, numel)] of a network configuration from the library's host-only manifest functions (no GPU, no context)."""
    out = []
    cb = L.MANIFEST_CB(lambda name, numel, user: out.append((name.decode(), int(numel))))
    lib = L.load()
    n = getattr(lib, f"cgd_{kind}_manifest")(cb, None) if kind in ("lpips", "secondary") else getattr(lib, f"cgd_{kind}_manifest")(C.byref(cfg), cb, None)
    if n < 0:
        raise ValueError(f"{kind}: invalid configuration (status {n})")
    return out
