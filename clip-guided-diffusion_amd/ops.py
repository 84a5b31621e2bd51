"""Single-op wrappers over the C ABI on PyTorch-ROCm tensors (device memory + stream plumbing only).

Used by the parity tests and available to a user-supplied cond_fn.  Activations are NHWC / token-major fp32.

Every operand is checked before any C call (ValueError otherwise): fp32, on the GPU, and in a layout the ABI can express.  Where the
ABI takes a row stride (GEMM operands, conv inputs and residuals, GroupNorm operands) a view is accepted if its last dimension is
dense and its leading dimensions collapse to one row stride -- a channel slice of an NHWC concat buffer, say -- and that stride is
what the C call receives.  Every other operand must be contiguous.
"""
import ctypes as C

import torch as th

from . import lib as L

_DEVICE_TYPE = "cuda"  # where every operand must live: the kernels dereference raw device pointers


def _s():
    return L.stream_ptr()


def _check(t, name):
    if not isinstance(t, th.Tensor):
        raise ValueError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if t.device.type != _DEVICE_TYPE:
        raise ValueError(f"{name}: expected a GPU tensor, got one on {t.device}")
    if t.dtype != th.float32:
        raise ValueError(f"{name}: expected float32, got {t.dtype}")


def _dense(t, name):
    """Device pointer of a contiguous fp32 GPU tensor (None passes through)."""
    if t is None:
        return None
    _check(t, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor, got shape {tuple(t.shape)} strides {t.stride()}")
    return t.data_ptr()


def _rows(t, name):
    """(device pointer, row stride) of an fp32 GPU tensor read as rows of its last dimension: the last dimension must be dense and
    the leading dimensions must collapse to one row stride, no smaller than the row.  None gives (None, 0)."""
    if t is None:
        return None, 0
    _check(t, name)
    if t.dim() == 0:
        raise ValueError(f"{name}: expected at least one dimension")
    shape, strides = tuple(t.shape), t.stride()
    width = shape[-1]
    if width > 1 and strides[-1] != 1:
        raise ValueError(f"{name}: the last dimension must be dense, got strides {strides}")
    lead = [(n, s) for n, s in zip(shape[:-1], strides[:-1]) if n != 1]  # size-1 dimensions carry no layout
    ld = lead[-1][1] if lead else width
    expect = ld
    for n, s in reversed(lead):
        if s != expect:
            raise ValueError(f"{name}: leading dimensions do not collapse to one row stride (shape {shape}, strides {strides})")
        expect *= n
    if lead and ld < width:
        raise ValueError(f"{name}: row stride {ld} is smaller than the row width {width}")
    return t.data_ptr(), ld


def pack_conv3x3(w):
    """torch conv weight [Co][Ci][3][3] -> (forward [Co][9*Ci], dgrad [Ci][9*Co]) packed layouts."""
    co, ci = w.shape[:2]
    wf = w.permute(0, 2, 3, 1).reshape(co, 9 * ci).contiguous()
    wd = w.flip(2, 3).permute(1, 2, 3, 0).reshape(ci, 9 * co).contiguous()
    return wf, wd


def gemm(ctx, A, B, bias=None, R=None, alpha=1.0, force_tile=0, splitk=1, out=None):
    """C[M,N] = alpha * A[M,K] @ B[N,K]^T (+bias) (+R); A, B, R and `out` may be row-strided views"""
    M, K = A.shape
    N = B.shape[0]
    pa, lda = _rows(A, "A")
    pb, ldb = _rows(B, "B")
    pbias = _dense(bias, "bias")
    pr, ldr = _rows(R, "R")
    if out is None:
        out = th.empty((M, N), device=A.device, dtype=th.float32)
    pc, ldc = _rows(out, "out")
    ctx.check(ctx.lib.cgd_op_gemm(ctx.h, pa, lda, pb, ldb, pc, ldc, pbias, pr, ldr, M, N, K, float(alpha), force_tile, splitk, _s()))
    return out


def gemm_ex(ctx, A, B, bias=None, R=None, alpha=1.0, force_tile=0, splitk=1, weight=False, defer=False, out=None):
    """gemm() with the two switches of the networks' linears: `weight` (B is a persistent weight: its packed copy is cached by pointer) and
    `defer` (a launch that splits K leaves its slices to the norm that reads `out` next; `pending(ctx)` shows them)."""
    M, K = A.shape
    N = B.shape[0]
    pa, lda = _rows(A, "A")
    pb, ldb = _rows(B, "B")
    pbias = _dense(bias, "bias")
    pr, ldr = _rows(R, "R")
    if out is None:
        out = th.empty((M, N), device=A.device, dtype=th.float32)
    pc, ldc = _rows(out, "out")
    ctx.check(ctx.lib.cgd_op_gemm_ex(ctx.h, pa, lda, pb, ldb, pc, ldc, pbias, pr, ldr, M, N, K, float(alpha), force_tile, splitk, int(bool(weight)),
                                     int(bool(defer)), _s()))
    return out


def pending(ctx):
    """The deferred split-K reduction the context still holds: {valid, slices, rows, cols, ldc} (host state only, all zero when none)."""
    out = (C.c_int64 * 5)()
    ctx.check(ctx.lib.cgd_op_pending(ctx.h, out))
    return dict(zip(("valid", "slices", "rows", "cols", "ldc"), (int(v) for v in out)))


def gemm_gn_bwd(ctx, A, W, x, dz, coef, bcoef, add=None, out=None):
    """dx[B,HW,N] = A[B,HW,K] @ W[N,K]^T (+add) + GroupNorm+SiLU backward of (x, dz) with the per-(sample, channel) tables coef [B,N,4] =
    {a, b, -, mean} and bcoef [B,N,4] = {A1, A2, A3, -}, in one launch.  A, W, x, dz, add and `out` may be row-strided views."""
    B, HW, K = A.shape
    N = W.shape[0]
    pa, lda = _rows(A, "A")
    pw, ldw = _rows(W, "W")
    px, ldx = _rows(x, "x")
    pdz, lddz = _rows(dz, "dz")
    padd, ldadd = _rows(add, "add")
    pc, pbc = _dense(coef, "coef"), _dense(bcoef, "bcoef")
    if out is None:
        out = th.empty((B, HW, N), device=A.device, dtype=th.float32)
    po, ldo = _rows(out, "out")
    ctx.check(ctx.lib.cgd_op_gemm_gn_bwd(ctx.h, pa, lda, pw, ldw, po, ldo, px, ldx, pdz, lddz, padd, ldadd, pc, pbc, B, HW, N, K, _s()))
    return out


def pack_conv3x3_frag(ctx, w, dgrad=False):
    """torch conv weight [Co][Ci][3][3] (on the GPU) -> MFMA-fragment-order bf16 hi/lo planes for the halo conv kernel."""
    co, ci = w.shape[:2]
    wc = w.contiguous().float()
    pw = _dense(wc, "w")
    out = th.empty(co * ci * 9, device=w.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_pack_conv3x3_frag(ctx.h, pw, out.data_ptr(), co, ci, int(dgrad), _s()))
    return out


def conv3x3(ctx, x_nhwc, w_packed, bias=None, R=None, upsample_input=False, force_tile=0, splitk=1, w_frag=None):
    """x (B,H,W,Cin) NHWC (H,W = OUTPUT size; with upsample_input the tensor holds (B,H/2,W/2,Cin)); x and R may be channel slices."""
    Bn, Hs, Ws, Cin = x_nhwc.shape
    H, W = (Hs * 2, Ws * 2) if upsample_input else (Hs, Ws)
    Cout = w_packed.shape[0]
    px, ldx = _rows(x_nhwc, "x")
    pw, pfrag, pbias = _dense(w_packed, "w_packed"), _dense(w_frag, "w_frag"), _dense(bias, "bias")
    pr, ldr = _rows(R, "R")
    y = th.empty((Bn, H, W, Cout), device=x_nhwc.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_conv3x3(ctx.h, px, ldx, pw, pfrag, y.data_ptr(), Cout, pbias, pr, ldr, Bn, H, W, Cin, Cout, int(upsample_input),
                                     force_tile, splitk, _s()))
    return y


def conv3x3_s2(ctx, x_nhwc, w, bias=None, out=None, packed=False):
    """conv2d(stride=2, padding=1) of x (B,H,W,Cin) NHWC with the torch weight w [Cout][Cin][3][3] -> (B,H/2,W/2,Cout); x and `out` may be
    channel slices.  packed: w is pack_conv3x3(w)[0], [Cout][9 Cin], packed once by the caller (no per-call pack launch)."""
    Bn, H, W, Cin = x_nhwc.shape
    Cout = w.shape[0]
    px, ldx = _rows(x_nhwc, "x")
    pw, pbias = _dense(w, "w"), _dense(bias, "bias")
    if out is None:
        out = th.empty((Bn, H // 2, W // 2, Cout), device=x_nhwc.device, dtype=th.float32)
    py, ldy = _rows(out, "out")
    fn = ctx.lib.cgd_op_conv3x3_s2_packed if packed else ctx.lib.cgd_op_conv3x3_s2
    ctx.check(fn(ctx.h, px, ldx, pw, pbias, py, ldy, Bn, H, W, Cin, Cout, _s()))
    return out


def conv3x3_s2_dgrad(ctx, dy_nhwc, w, add=None, out=None, packed=False):
    """The input gradient of conv3x3_s2: dy (B,Ho,Wo,Cout) -> dx (B,2Ho,2Wo,Cin) (+ add, dx's shape); dy, add and `out` may be channel slices.
    packed: w is pack_conv3x3(w)[1], [Cin][9 Cout], packed once by the caller."""
    Bn, Ho, Wo, Cout = dy_nhwc.shape
    Cin = w.shape[0] if packed else w.shape[1]
    pdy, lddy = _rows(dy_nhwc, "dy")
    pw = _dense(w, "w")
    padd, ldadd = _rows(add, "add")
    if out is None:
        out = th.empty((Bn, 2 * Ho, 2 * Wo, Cin), device=dy_nhwc.device, dtype=th.float32)
    pdx, lddx = _rows(out, "out")
    fn = ctx.lib.cgd_op_conv3x3_s2_dgrad_packed if packed else ctx.lib.cgd_op_conv3x3_s2_dgrad
    ctx.check(fn(ctx.h, pdy, lddy, pw, pdx, lddx, padd, ldadd, Bn, 2 * Ho, 2 * Wo, Cin, Cout, _s()))
    return out


def pack_conv3x3_wino(ctx, w, dgrad=False):
    """torch conv weight [Co][Ci][3][3] (on the GPU) -> Winograd F(2,3)-transformed bf16 hi/lo fragments for wconv.hip."""
    co, ci = w.shape[:2]
    wc = w.contiguous().float()
    pw = _dense(wc, "w")
    out = th.empty(co * ci * 12, device=w.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_pack_conv3x3_wino(ctx.h, pw, out.data_ptr(), co, ci, int(dgrad), _s()))
    return out


def conv3x3_wino(ctx, x_nhwc, w_wino, cout, bias=None, R=None, upsample_input=False, gn_ab=None):
    """The Winograd halo conv kernel on x (B,H,W,Cin) NHWC (H, W multiples of 16); gn_ab (B,Cin,2): convolve SiLU(x * a + b).
    x and R may be channel slices."""
    Bn, Hs, Ws, Cin = x_nhwc.shape
    H, W = (Hs * 2, Ws * 2) if upsample_input else (Hs, Ws)
    px, ldx = _rows(x_nhwc, "x")
    pw, pbias, pab = _dense(w_wino, "w_wino"), _dense(bias, "bias"), _dense(gn_ab, "gn_ab")
    pr, ldr = _rows(R, "R")
    y = th.empty((Bn, H, W, cout), device=x_nhwc.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_conv3x3_wino(ctx.h, px, ldx, pw, y.data_ptr(), cout, pbias, pr, ldr, pab, Bn, H, W, Cin, cout, int(upsample_input),
                                          _s()))
    return y


def conv_in(ctx, x_nchw, w_packed, bias, cout):
    Bn, Cin, H, W = x_nchw.shape
    px, pw, pbias = _dense(x_nchw, "x"), _dense(w_packed, "w_packed"), _dense(bias, "bias")
    y = th.empty((Bn, H, W, cout), device=x_nchw.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_conv_in(ctx.h, px, pw, pbias, y.data_ptr(), Bn, H, W, Cin, cout, _s()))
    return y


def sr_stem(ctx, x_nchw, low, w_packed, bias=None, out=None):
    """The conditioned stem of the super-resolution UNets in one launch: conv3x3(cat([x, bilinear(low -> H x W)], 1), w, bias).
    x (B,3,H,W) and low (1 or B,3,h,w) NCHW, contiguous (offset views are fine); w_packed [Cout, 54] as pack_conv3x3 leaves the
    [Cout,6,3,3] weight; `out` (B,H,W,Cout) NHWC may be a channel slice.  No (B,6,H,W) tensor is formed."""
    if x_nchw.dim() != 4 or x_nchw.shape[1] != 3:
        raise ValueError(f"x: expected (B,3,H,W), got {tuple(x_nchw.shape)}")
    Bn, _, H, W = x_nchw.shape
    if low.dim() != 4 or low.shape[1] != 3 or low.shape[0] not in (1, Bn) or 0 in low.shape:
        raise ValueError(f"low: expected (1 or {Bn},3,h,w), got {tuple(low.shape)}")
    if w_packed.dim() != 2 or w_packed.shape[1] != 54:
        raise ValueError(f"w_packed: expected [Cout, 54], got {tuple(w_packed.shape)}")
    cout = w_packed.shape[0]
    px, pl, pw, pbias = _dense(x_nchw, "x"), _dense(low, "low"), _dense(w_packed, "w_packed"), _dense(bias, "bias")
    if out is None:
        out = th.empty((Bn, H, W, cout), device=x_nchw.device, dtype=th.float32)
    elif tuple(out.shape) != (Bn, H, W, cout):
        raise ValueError(f"out: expected {(Bn, H, W, cout)}, got {tuple(out.shape)}")
    po, ldo = _rows(out, "out")
    ctx.check(ctx.lib.cgd_op_sr_stem(ctx.h, px, pl, low.shape[0], low.shape[2], low.shape[3], pw, pbias, po, ldo, Bn, H, W, cout, _s()))
    return out


def conv_thin_out(ctx, x_nhwc, w_packed, bias, cout):
    """x (B,H,W,Cin) NHWC, may be a channel slice -> y (B,cout,H,W) NCHW"""
    Bn, H, W, Cin = x_nhwc.shape
    px, ldx = _rows(x_nhwc, "x")
    pw, pbias = _dense(w_packed, "w_packed"), _dense(bias, "bias")
    y = th.empty((Bn, cout, H, W), device=x_nhwc.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_conv_thin_out(ctx.h, px, ldx, pw, pbias, y.data_ptr(), Bn, H, W, Cin, cout, _s()))
    return y


def gn_scratch(ctx, B, HW, C, device):
    n = ctx.lib.cgd_op_gn_scratch_floats(B, HW, C)
    return th.empty(n, device=device, dtype=th.float32)


def groupnorm_fwd(ctx, x, gamma, beta, film=None, act=1, eps=1e-5, scratch=None):
    """x (B,HW,C) NHWC-flattened, may be a channel slice.  Returns (y, scratch) — scratch feeds groupnorm_bwd."""
    B, HW, Cc = x.shape
    px, ldx = _rows(x, "x")
    pg, pb, pf = _dense(gamma, "gamma"), _dense(beta, "beta"), _dense(film, "film")
    if scratch is None:
        scratch = gn_scratch(ctx, B, HW, Cc, x.device)
    ps = _dense(scratch, "scratch")
    y = th.empty((B, HW, Cc), device=x.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_gn_fwd(ctx.h, px, ldx, y.data_ptr(), Cc, B, HW, Cc, pg, pb, pf, act, eps, ps, _s()))
    return y, scratch


def groupnorm_bwd(ctx, x, dz, scratch, act=1, add=None):
    """x, dz and add (B,HW,C) may be channel slices"""
    B, HW, Cc = x.shape
    px, ldx = _rows(x, "x")
    pdz, lddz = _rows(dz, "dz")
    padd, ldadd = _rows(add, "add")
    ps = _dense(scratch, "scratch")
    dx = th.empty((B, HW, Cc), device=x.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_gn_bwd(ctx.h, px, ldx, pdz, lddz, dx.data_ptr(), Cc, padd, ldadd, B, HW, Cc, act, ps, _s()))
    return dx


def layernorm_fwd(ctx, x, gamma, beta, eps=1e-5):
    rows, Cc = x.shape
    px, pg, pb = _dense(x, "x"), _dense(gamma, "gamma"), _dense(beta, "beta")
    y = th.empty((rows, Cc), device=x.device, dtype=th.float32)
    stats = th.empty((rows, 2), device=x.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_ln_fwd(ctx.h, px, y.data_ptr(), rows, Cc, pg, pb, eps, stats.data_ptr(), _s()))
    return y, stats


def layernorm_bwd(ctx, x, dy, gamma, stats):
    rows, Cc = x.shape
    px, pdy, pg, pst = _dense(x, "x"), _dense(dy, "dy"), _dense(gamma, "gamma"), _dense(stats, "stats")
    dx = th.empty((rows, Cc), device=x.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_ln_bwd(ctx.h, px, pdy, dx.data_ptr(), rows, Cc, pg, pst, _s()))
    return dx


def pool2x2(ctx, x_nhwc, scale=0.25):
    B, H, W, Cc = x_nhwc.shape
    px = _dense(x_nhwc, "x")
    y = th.empty((B, H // 2, W // 2, Cc), device=x_nhwc.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_pool2x2(ctx.h, px, y.data_ptr(), B, H // 2, W // 2, Cc, scale, _s()))
    return y


def upsample2x(ctx, x_nhwc, scale=1.0):
    B, H, W, Cc = x_nhwc.shape
    px = _dense(x_nhwc, "x")
    y = th.empty((B, H * 2, W * 2, Cc), device=x_nhwc.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_upsample2x(ctx.h, px, y.data_ptr(), B, H * 2, W * 2, Cc, scale, _s()))
    return y


def act(ctx, x, kind, dy=None):
    """kind 1 SiLU, 2 QuickGELU, 3 exact (erf) GELU; with dy returns dy * act'(x)."""
    px, pdy = _dense(x, "x"), _dense(dy, "dy")
    if dy is not None and dy.numel() != x.numel():
        raise ValueError(f"dy: {dy.numel()} elements, x has {x.numel()}")
    out = th.empty(x.shape, device=x.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_op_act(ctx.h, px, pdy, out.data_ptr(), x.numel(), kind, _s()))
    return out


def _nchw(t, name):
    ptr = _dense(t, name)
    if t.dim() != 4:
        raise ValueError(f"{name}: expected (B, C, H, W), got shape {tuple(t.shape)}")
    return ptr


def frame_warp(ctx, src, matrix, interp="bicubic", border="wrap", clamp=False, out=None):
    """Affine resampling of src (B,C,H,W) in one launch (cgd_frame_warp): `matrix` holds the six entries of the INVERSE map, destination
    pixel (x, y) reads the source at (m0 x + m1 y + m2, m3 x + m4 y + m5); interp 'bilinear' / 'bicubic' (a = -0.75), border 'wrap' /
    'reflect' / 'replicate', clamp: to [-1, 1] after interpolation.  `out` must not alias `src`."""
    ps = _nchw(src, "src")
    if interp not in L.WARP_INTERP or border not in L.WARP_BORDER:
        raise ValueError(f"interp must be one of {sorted(L.WARP_INTERP)} and border one of {sorted(L.WARP_BORDER)}, got {interp!r} and {border!r}")
    m = [float(v) for v in matrix]
    if len(m) != 6:
        raise ValueError(f"matrix: expected 6 entries, got {len(m)}")
    if out is None:
        out = th.empty_like(src)
    po = _nchw(out, "out")
    if tuple(out.shape) != tuple(src.shape):
        raise ValueError(f"out: shape {tuple(out.shape)}, src has {tuple(src.shape)}")
    B, Cn, H, W = src.shape
    w = L.Warp((C.c_double * 6)(*m), L.WARP_INTERP[interp], L.WARP_BORDER[border], int(bool(clamp)))
    ctx.check(ctx.lib.cgd_frame_warp(ctx.h, ps, po, B, Cn, H, W, C.byref(w), _s()))
    return out


def frame_warp3d(ctx, src, camera, depth=None, interp="bicubic", border="wrap", clamp=False, iters=1, out=None):
    """Perspective resampling of src (B,C,H,W) in one launch (cgd_frame_warp3d): `camera` is what animate.camera returns (R, T, f, cx, cy, z0,
    near: the motion X' = R X + T of a pinhole camera between two frames); `depth` None (flat, at camera.z0) or (1 or B, 1, H, W) in the units
    of z0, resolved at the source pixel by `iters` in 1..4 fixed-point steps; interp, border, clamp as in frame_warp.  `out` must not alias
    `src` or `depth`."""
    ps = _nchw(src, "src")
    if interp not in L.WARP_INTERP or border not in L.WARP_BORDER:
        raise ValueError(f"interp must be one of {sorted(L.WARP_INTERP)} and border one of {sorted(L.WARP_BORDER)}, got {interp!r} and {border!r}")
    R, T = [float(v) for v in camera.R], [float(v) for v in camera.T]
    if len(R) != 9 or len(T) != 3:
        raise ValueError(f"camera: expected 9 entries of R and 3 of T, got {len(R)} and {len(T)}")
    if isinstance(iters, bool) or int(iters) != iters:
        raise ValueError(f"iters must be an integer, got {iters!r}")
    B, Cn, H, W = src.shape
    pd = None
    if depth is not None:
        pd = _nchw(depth, "depth")
        if tuple(depth.shape[1:]) != (1, H, W) or depth.shape[0] not in (1, B):
            raise ValueError(f"depth: expected (1 or {B}, 1, {H}, {W}), got {tuple(depth.shape)}")
        if depth.device != src.device:
            raise ValueError(f"depth is on {depth.device}, src on {src.device}")
    if out is None:
        out = th.empty_like(src)
    po = _nchw(out, "out")
    if tuple(out.shape) != tuple(src.shape):
        raise ValueError(f"out: shape {tuple(out.shape)}, src has {tuple(src.shape)}")
    cam = L.Camera((C.c_double * 9)(*R), (C.c_double * 3)(*T), float(camera.f), float(camera.cx), float(camera.cy), float(camera.z0),
                   float(camera.near), int(iters), L.WARP_INTERP[interp], L.WARP_BORDER[border], int(bool(clamp)))
    ctx.check(ctx.lib.cgd_frame_warp3d(ctx.h, ps, po, pd, 0 if depth is None else int(depth.shape[0]), B, Cn, H, W, C.byref(cam), _s()))
    return out


def _flow_params(levels, iters, radius, lam, max_step):
    for name, v in (("levels", levels), ("iters", iters), ("radius", radius)):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"{name} must be an integer, got {v!r}")
    return L.FlowParams(int(levels), int(iters), int(radius), float(lam), float(max_step))


def flow_estimate(ctx, tmpl, img, levels=4, iters=4, radius=4, lam=1e-3, max_step=1.0, out=None):
    """Dense pyramidal Lucas-Kanade flow F (B,2,H,W) with img(p + F(p)) ~ tmpl(p) (cgd_flow_estimate): channel 0 the x displacement in
    pixels, channel 1 the y displacement; tmpl and img are (B,C,H,W) with C 3 (luminance) or 1.  `levels` pyramid levels at the most
    (cgd_flow_levels), `iters` iterations per level, windows of (2 radius + 1)^2 pixels, regulariser `lam`, steps of at most `max_step`
    pixels.  The scratch is the context's, one buffer per (device, size).  `out` must not alias an input."""
    pt, pi = _nchw(tmpl, "tmpl"), _nchw(img, "img")
    if tuple(img.shape) != tuple(tmpl.shape) or img.device != tmpl.device:
        raise ValueError(f"img: shape {tuple(img.shape)} on {img.device}, tmpl has {tuple(tmpl.shape)} on {tmpl.device}")
    B, Cn, H, W = tmpl.shape
    p = _flow_params(levels, iters, radius, lam, max_step)
    if out is None:
        out = th.empty((B, 2, H, W), device=tmpl.device, dtype=th.float32)
    po = _nchw(out, "out")
    if tuple(out.shape) != (B, 2, H, W):
        raise ValueError(f"out: expected shape {(B, 2, H, W)}, got {tuple(out.shape)}")
    n = int(ctx.lib.cgd_flow_scratch_floats(B, H, W, p.levels, p.radius))
    cache = ctx.__dict__.setdefault("_flow_scratch", {})
    key = (tmpl.device, n)
    if key not in cache:
        cache[key] = th.empty(max(n, 1), device=tmpl.device, dtype=th.float32)
    ctx.check(ctx.lib.cgd_flow_estimate(ctx.h, pt, pi, po, cache[key].data_ptr(), B, Cn, H, W, C.byref(p), _s()))
    return out


def flow_level(ctx, b, a, coarse=None, iters=4, radius=4, lam=1e-3, max_step=1.0, out=None):
    """One pyramid level of flow_estimate on given planes (cgd_op_flow_level, test support): b, a (B,H,W) template and image level, `coarse`
    None (start from zero) or the coarser level's flow (B,2,Hc,Wc); returns the level's flow (B,2,H,W)."""
    pb, pa, pc = _dense(b, "b"), _dense(a, "a"), _dense(coarse, "coarse")
    if b.dim() != 3 or tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"b and a: expected one shape (B, H, W), got {tuple(b.shape)} and {tuple(a.shape)}")
    B, H, W = b.shape
    Hc = Wc = 0
    if coarse is not None:
        if coarse.dim() != 4 or tuple(coarse.shape[:2]) != (B, 2):
            raise ValueError(f"coarse: expected ({B}, 2, Hc, Wc), got {tuple(coarse.shape)}")
        Hc, Wc = coarse.shape[2:]
    p = _flow_params(1, iters, radius, lam, max_step)
    if out is None:
        out = th.empty((B, 2, H, W), device=b.device, dtype=th.float32)
    po = _nchw(out, "out")
    if tuple(out.shape) != (B, 2, H, W):
        raise ValueError(f"out: expected shape {(B, 2, H, W)}, got {tuple(out.shape)}")
    ctx.check(ctx.lib.cgd_op_flow_level(ctx.h, pb, pa, pc, Hc, Wc, po, B, H, W, C.byref(p), _s()))
    return out


def frame_warp_flow(ctx, src, flow, flow_back=None, fallback=None, blend=1.0, alpha=0.01, beta=0.5, interp="bicubic", border="replicate",
                    clamp=False, out=None, mask_out=None):
    """out(p) = w S(p + flow(p)) + (1 - w) fallback(p), w = blend m(p), in one launch (cgd_frame_warp_flow): S samples src (B,C,H,W) as
    frame_warp does (interp, border, clamp); `flow` (1 or B, 2, H, W) in pixels, x first.  m = 1 without `flow_back`; with it (the flow of
    the opposite direction, same shape) m = 0 where p + flow(p) leaves the frame or the forward-backward check
    |F + Fb|^2 <= alpha (|F|^2 + |Fb|^2) + beta fails.  `fallback` (B,C,H,W) may be None only with blend == 1 and no flow_back.
    `mask_out` (B,1,H,W) receives m.  `out` and `mask_out` must not alias an input."""
    ps = _nchw(src, "src")
    if interp not in L.WARP_INTERP or border not in L.WARP_BORDER:
        raise ValueError(f"interp must be one of {sorted(L.WARP_INTERP)} and border one of {sorted(L.WARP_BORDER)}, got {interp!r} and {border!r}")
    B, Cn, H, W = src.shape
    pf = _nchw(flow, "flow")
    if tuple(flow.shape[1:]) != (2, H, W) or flow.shape[0] not in (1, B):
        raise ValueError(f"flow: expected (1 or {B}, 2, {H}, {W}), got {tuple(flow.shape)}")
    pb = pfb = pm = None
    if flow_back is not None:
        pb = _nchw(flow_back, "flow_back")
        if tuple(flow_back.shape) != tuple(flow.shape):
            raise ValueError(f"flow_back: shape {tuple(flow_back.shape)}, flow has {tuple(flow.shape)}")
    if fallback is not None:
        pfb = _nchw(fallback, "fallback")
        if tuple(fallback.shape) != tuple(src.shape):
            raise ValueError(f"fallback: shape {tuple(fallback.shape)}, src has {tuple(src.shape)}")
    if out is None:
        out = th.empty_like(src)
    po = _nchw(out, "out")
    if tuple(out.shape) != tuple(src.shape):
        raise ValueError(f"out: shape {tuple(out.shape)}, src has {tuple(src.shape)}")
    if mask_out is not None:
        pm = _nchw(mask_out, "mask_out")
        if tuple(mask_out.shape) != (B, 1, H, W):
            raise ValueError(f"mask_out: expected shape {(B, 1, H, W)}, got {tuple(mask_out.shape)}")
    for name, t in (("flow", flow), ("flow_back", flow_back), ("fallback", fallback), ("out", out), ("mask_out", mask_out)):
        if t is not None and t.device != src.device:
            raise ValueError(f"{name} is on {t.device}, src on {src.device}")
    w = L.WarpFlow(float(blend), float(alpha), float(beta), L.WARP_INTERP[interp], L.WARP_BORDER[border], int(bool(clamp)))
    ctx.check(ctx.lib.cgd_frame_warp_flow(ctx.h, ps, pf, pb, pfb, po, pm, int(flow.shape[0]), B, Cn, H, W, C.byref(w), _s()))
    return out


def resize_cubic(ctx, x, Ho, Wo, a=1.0, b=0.0, lo=None, out=None):
    """a * resize(x) + b of x (B,C,H,W) to (B,C,Ho,Wo) in one launch (cgd_op_resize_cubic): the antialiased cubic weights of the resized
    cutouts, the taps outside the image read at the nearest edge pixel; `lo`: the result is clamped from below.  An identical size copies."""
    px = _nchw(x, "x")
    B, Cn, H, W = x.shape
    if out is None:
        out = th.empty((B, Cn, int(Ho), int(Wo)), device=x.device, dtype=th.float32)
    po = _dense(out, "out")
    if tuple(out.shape) != (B, Cn, int(Ho), int(Wo)):
        raise ValueError(f"out: expected shape {(B, Cn, int(Ho), int(Wo))}, got {tuple(out.shape)}")
    ctx.check(ctx.lib.cgd_op_resize_cubic(ctx.h, px, po, B * Cn, H, W, int(Ho), int(Wo), float(a), float(b), float(lo or 0.0), int(lo is not None),
                                          _s()))
    return out


def channel_stats(ctx, x, out=None):
    """(B,C,2): mean and population standard deviation of every plane of x (B,C,H,W), sums in fp64 (cgd_channel_stats)."""
    px = _nchw(x, "x")
    B, Cn, H, W = x.shape
    if out is None:
        out = th.empty((B, Cn, 2), device=x.device, dtype=th.float32)
    po = _dense(out, "out")
    if tuple(out.shape) != (B, Cn, 2):
        raise ValueError(f"out: expected shape {(B, Cn, 2)}, got {tuple(out.shape)}")
    ctx.check(ctx.lib.cgd_channel_stats(ctx.h, px, po, B, Cn, H, W, _s()))
    return out


def color_match(ctx, x, stats_ref, amount=1.0, clamp=False, stats_x=None):
    """In place: every plane of x (B,C,H,W) is moved toward the mean and standard deviation `stats_ref` (1 or B, C, 2) by `amount` in
    [0, 1] (cgd_color_match); `stats_x`: channel_stats(x) (taken here when None).  Returns x."""
    px = _nchw(x, "x")
    B, Cn, H, W = x.shape
    if stats_x is None:
        stats_x = channel_stats(ctx, x)
    psx, psr = _dense(stats_x, "stats_x"), _dense(stats_ref, "stats_ref")
    if tuple(stats_x.shape) != (B, Cn, 2) or stats_ref.dim() != 3 or tuple(stats_ref.shape[1:]) != (Cn, 2):
        raise ValueError(f"stats_x must be {(B, Cn, 2)} and stats_ref (1 or {B}, {Cn}, 2), got {tuple(stats_x.shape)} and {tuple(stats_ref.shape)}")
    ctx.check(ctx.lib.cgd_color_match(ctx.h, px, psx, psr, int(stats_ref.shape[0]), float(amount), int(bool(clamp)), B, Cn, H, W, _s()))
    return x


class Attention:
    """QKV attention on token-major qkv (nb*T, 3C); keeps the buffers the backward needs."""

    def __init__(self, ctx, nb, heads, T, d, legacy, device):
        self.ctx, self.nb, self.heads, self.T, self.d, self.legacy = ctx, nb, heads, T, d, int(legacy)
        self.bufs = [th.zeros(ctx.lib.cgd_op_attn_buf_floats(nb, heads, T, d, w), device=device, dtype=th.float32) for w in range(5)]
        self._arr = (C.c_void_p * 5)(*[b.data_ptr() for b in self.bufs])

    def forward(self, qkv):
        Cc = self.heads * self.d
        pq = _dense(qkv, "qkv")
        out = th.empty((self.nb * self.T, Cc), device=qkv.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_op_attn_fwd(self.ctx.h, pq, out.data_ptr(), self.nb, self.heads, self.T, self.d,
                                                    self.legacy, self._arr, _s()))
        return out

    def forward_causal(self, qkv):
        """The forward with key j > query i masked (the CLIP text tower; [Q | K | V] rows only, no backward)."""
        if self.legacy:
            raise ValueError("causal attention takes the [Q all heads | K | V] row layout (legacy=0)")
        Cc = self.heads * self.d
        pq = _dense(qkv, "qkv")
        out = th.empty((self.nb * self.T, Cc), device=qkv.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_op_attn_fwd_causal(self.ctx.h, pq, out.data_ptr(), self.nb, self.heads, self.T, self.d,
                                                           self._arr, _s()))
        return out

    def backward(self, qkv, dout):
        pq, pd = _dense(qkv, "qkv"), _dense(dout, "dout")
        dqkv = th.empty(qkv.shape, device=qkv.device, dtype=th.float32)
        self.ctx.check(self.ctx.lib.cgd_op_attn_bwd(self.ctx.h, pq, pd, dqkv.data_ptr(), self.nb, self.heads,
                                                    self.T, self.d, self.legacy, self._arr, _s()))
        return dqkv
