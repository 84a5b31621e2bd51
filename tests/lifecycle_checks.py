"""Network handles across call SEQUENCES (tests/test_gpu_lifecycle.py, benchmarks/gpu_diag.py): every other network check creates a fresh
context and a fresh handle, uploads once and runs one forward + one backward, so the state a handle keeps between calls — grow-only activation
buffers and the pointers stashed into them, lazily packed weight copies (the context's fragment cache, the Winograd copies, transposed
weights), the two FiLM slots, the saved shape, deferred split-K slices, the conv-epilogue record serial, the attention family per scratch
buffer, the LPIPS reference features — is only ever exercised from its initial value.

Every pass of every sequence here is judged twice:
  1. against the oracle at the strict criterion of `parity_checks.rec` (unit-peak backward seeds; `relu-flips` for the input gradient of the
     ReLU towers, as everywhere else);
  2. bit for bit (`th.equal`) against the SAME call on a fresh handle in a fresh context: the kernels use no atomics and the launch plan is
     a function of (shape, knobs), so a handle with a history must reproduce the fresh handle exactly.  A `_flag` record per tensor.
Oracle and fresh-handle results are computed once per (network, weight seed, shape, input variant[, precision]) and cached in this module.

The walk tables at the top are what tests/test_lifecycle_host.py checks on the CPU (each "grow" step grows every buffer, 128 x 128 crosses
the Winograd threshold, 32 x 48 runs its lower levels on the implicit GEMM with deferred split-K slices, 32 x 64 reaches the weight-streaming
conv kernel on non-square maps): edit them there too.
"""
import math

import torch as th

from tests import parity_checks as pc
from tests.parity_checks import DEV, _flag, g, rec, rec_flips, unit_seed

# ---- scenario tables (shared with the CPU tier) ------------------------------------------------------------------------------------------
UNET_CASE = "mini"
# (B, H, W) per step; step k uses input variant k (its own x, t, y and backward seed)
# (why two non-square steps: at 32 x 48 the lower levels are 16 x 24 and 8 x 12, whose widths the halo
# kernels do not take, so those convs run on the implicit GEMM with 9 deferred split-K slices and NO conv of that step reaches the weight-streaming
# kernel; 32 x 64 is the non-square step whose 16 x 32 and 8 x 16 levels do — tests/test_lifecycle_host.py asserts both from the launch plan)
UNET_WALK = [(1, 64, 64), (2, 128, 128), (1, 64, 64), (2, 32, 48), (1, 128, 128), (2, 128, 128), (2, 32, 64)]
UNET_WALK_GROWS = [1]          # steps larger than everything before them, in every per-buffer element count
UNET_WALK_SHRINKS = [2, 3, 4, 6]  # steps smaller than the largest shape seen before them
UNET_WALK_F32 = UNET_WALK[:3]
CFG64_WALK = [(1, 64, 64), (2, 64, 64), (1, 64, 64)]
# eight passes after UNET_WALK, alternating smaller and equal shapes: nothing may be allocated (the largest shape is UNET_WALK[1])
UNET_WARM = [(1, 64, 64), (2, 128, 128), (2, 32, 48), (2, 128, 128), (1, 128, 128), (2, 128, 128), (1, 64, 64), (2, 128, 128)]
UNET_LARGER = (3, 128, 128)    # ... and this one must allocate: the counter is live
T_VALUES = [0.0, 999.0, 417.5, 3.0, 250.25, 998.0, 1.5]  # sample b of variant v gets T_VALUES[(v + b) % 7]: 0, 999 and fractional values
VIT_NAME = "ViT-B/32"
VIT_WALK = [(3, 0), (16, 1), (1, 0), (16, 0)]  # (N, layout): 0 = NCHW images, 1 = the cutout kernel's patch rows with n=
VIT_WARM = [(1, 0), (16, 1), (3, 0), (16, 0), (8, 1), (16, 1), (1, 1), (16, 0)]
VIT_LARGER = (17, 0)
TEXT_CFG = (77, 49408, 512, 12, 8, 512)  # the ViT-B/32 text tower
TEXT_WALK = [1, 4, 2]
RN_CFG = (64, 64, (1, 1, 1, 1), 128, 32)  # the tiny ModifiedResNet of test_gpu_parity.py
RN_WALK = [2, 5, 1]
LPIPS_WALK = [(2, 64, 64), (1, 96, 128), (2, 64, 64)]
SEEDS = {"unet": (1234, 4242), "vit": (4321, 999), "text": (11, 12), "rn": (2468, 1357), "lpips": (777, 778)}  # weight seeds 1 / 2 per family

_ORACLE_NETS, _ORACLE, _FRESH = {}, {}, {}


def _ctx(precision=1):
    return pc._ctx(precision)


def _oracle_net(kind, seed, case=None):
    key = (kind, case, seed)
    if key not in _ORACLE_NETS:
        if kind == "unet":
            net = pc.oracle_unet(case, seed)
        elif kind == "vit":
            net = pc.oracle_vit(VIT_NAME, seed)
        elif kind == "text":
            from tests import text_ref
            net = text_ref.synthetic_init_(text_ref.ClipTextModel(*TEXT_CFG), seed=seed).eval()
        elif kind == "rn":
            net = pc.oracle_resnet("tiny", RN_CFG, seed)
        else:
            net = pc.oracle_lpips(seed)
        _ORACLE_NETS[key] = net
    return _ORACLE_NETS[key]


def _sd(kind, net):
    return pc.lpips_sd(net) if kind == "lpips" else pc.device_sd(net)


def _new_handle(ctx, kind, case=None):
    from cgd_amd import nets
    if kind == "unet":
        return nets.UNet(ctx, **pc.UNET_CASES[case])
    if kind == "vit":
        return nets.ClipImageTower(ctx, VIT_NAME)
    if kind == "text":
        return nets.ClipTextTower(ctx, config=TEXT_CFG)
    if kind == "rn":
        return nets.ClipResNetTower(ctx, "tiny", RN_CFG)
    return nets.LpipsVGG(ctx)


def _load(dev, kind, seed, case=None):
    sd = _sd(kind, _oracle_net(kind, seed, case))
    if kind in ("vit", "rn", "text"):
        dev.load_clip_state_dict(sd)
    else:
        dev.load_state_dict(sd)
    return dev


def _handle(ctx, kind, seed, case=None):
    return _load(_new_handle(ctx, kind, case), kind, seed, case)


# ---- one call per family: inputs, oracle, device ---------------------------------------------------------------------------------------
class UNetCall:
    kind, flips = "unet", False

    def __init__(self, B, H, W, v, case=UNET_CASE):
        self.case, self.key = case, (case, B, H, W, v)
        nc = pc.UNET_CASES[case].get("num_classes")
        self.x = th.randn(B, 3, H, W, generator=g(600 + v))
        self.t = th.tensor([T_VALUES[(v + b) % len(T_VALUES)] for b in range(B)])
        self.y = th.randint(0, nc, (B,), generator=g(610 + v)) if nc else None
        self.gout = th.randn(B, 6, H, W, generator=g(620 + v))
        self.gout[:, 3:] = 0  # the guidance only seeds the epsilon channels
        self.tag = f"unet[{case} B{B} {H}x{W} v{v}]"

    def oracle(self, seed):
        ref = _oracle_net("unet", seed, self.case)
        xr = self.x.clone().requires_grad_()
        o = ref(xr, self.t, self.y)
        (o * self.gout).sum().backward()
        sd = unit_seed(xr.grad)
        return {"fwd": o.detach(), "bwd": xr.grad * sd, "sd": sd}

    def forward(self, dev, out=None):
        return dev.forward(self.x.to(DEV), self.t.to(DEV), None if self.y is None else self.y.to(DEV), out=out)

    def dgrad(self, dev, sd, g_x=None):
        return dev.dgrad((self.gout * sd).to(DEV), g_x)


class VitCall:
    kind, flips, case = "vit", False, None

    def __init__(self, N, layout=0, v=0):
        self.N, self.layout, self.key = N, layout, (N, v)  # the layout is a property of the call, not of the result: same oracle
        self.img = th.randn(N, 3, 224, 224, generator=g(700 + v))
        self.de = th.randn(N, 512, generator=g(710 + v))
        self.tag = f"vit[{VIT_NAME} N{N} layout{layout} v{v}]"

    @staticmethod
    def rows(img, patch=32):
        """(N,3,R,R) -> the cutout kernel's patch rows [N * g * g][3 * patch * patch]"""
        N, gs = img.shape[0], img.shape[2] // patch
        return img.reshape(N, 3, gs, patch, gs, patch).permute(0, 2, 4, 1, 3, 5).reshape(N * gs * gs, -1).contiguous()

    def oracle(self, seed):
        ref = _oracle_net("vit", seed)
        ir = self.img.clone().requires_grad_()
        e = ref.encode_image(ir)
        (e * self.de).sum().backward()
        sd = unit_seed(ir.grad)
        return {"fwd": e.detach(), "bwd": ir.grad * sd, "sd": sd}

    def forward(self, dev, out=None):
        if self.layout == 0:
            return dev.encode_image(self.img.to(DEV), out=out)
        return dev.encode_image(self.rows(self.img).to(DEV), layout=1, n=self.N, out=out)

    def grad_shape(self):
        return (self.N, 3, 224, 224) if self.layout == 0 else (self.N * 49, 3 * 32 * 32)

    def dgrad(self, dev, sd, g_x=None):
        d = dev.dgrad((self.de * sd).to(DEV), g_x)
        if self.layout == 0:
            return d
        gs = 224 // 32  # patch rows back to NCHW: compared with the same oracle gradient
        return d.reshape(self.N, gs, gs, 3, 32, 32).permute(0, 3, 1, 4, 2, 5).reshape(self.N, 3, 224, 224)


class RnCall:
    kind, flips, case = "rn", True, None

    def __init__(self, N, v=0):
        self.key = (N, v)
        self.img = th.randn(N, 3, RN_CFG[0], RN_CFG[0], generator=g(750 + v))
        self.de = th.randn(N, RN_CFG[3], generator=g(760 + v))
        self.tag = f"resnet[tiny N{N} v{v}]"

    def oracle(self, seed):
        ref = _oracle_net("rn", seed)
        ir = self.img.double().requires_grad_()
        e = ref.encode_image(ir)
        (e * self.de.double()).sum().backward()
        sd = unit_seed(ir.grad)
        return {"fwd": e.detach().float(), "bwd": (ir.grad * sd).float(), "sd": sd}

    def forward(self, dev, out=None):
        return dev.encode_image(self.img.to(DEV), out=out)

    def dgrad(self, dev, sd, g_x=None):
        return dev.dgrad((self.de * sd).to(DEV), g_x)


class TextCall:
    kind, flips, case = "text", False, None

    def __init__(self, N, v=0):
        from tests import text_ref
        self.key = (N, v)
        lengths = [77, 5, 40, 2, 13, 77, 64, 21][:N]
        self.tok = text_ref.random_tokens(N, 77, TEXT_CFG[1], lengths, seed=40 + v)
        self.tag = f"text[ViT-B/32 N{N} v{v}]"

    def oracle(self, seed):
        with th.no_grad():
            return {"fwd": _oracle_net("text", seed).encode_text(self.tok), "bwd": None, "sd": 1.0}

    def forward(self, dev, out=None):
        return dev.encode_text(self.tok.to(DEV), out=out)

    dgrad = None  # forward only


class LpipsCall:
    """set_reference(ref) + loss_grad(x): `fwd` is the per-sample loss, `bwd` the gradient at unit peak"""
    kind, flips, case = "lpips", False, None  # graded strictly, as parity_checks.check_lpips grades it

    def __init__(self, B, H, W, v=0):
        self.key = (B, H, W, v)
        # the inputs of parity_checks.check_lpips (variant 0 = its generators 70 / 71): the gradient is discontinuous in the activations (ReLU masks,
        # max-pool arg-max) and the suite grades it strictly on those inputs; other draws can flip one mask on a FRESH handle too (measured at
        # (1, 96, 128) with generators 770 / 780: one element off by 1.05e-3 of the peak, bit-equal to the fresh handle) — not what this tier is about
        self.ref = th.rand(B, 3, H, W, generator=g(70 + v)) * 2 - 1
        self.x = (self.ref + 0.3 * th.randn(B, 3, H, W, generator=g(71 + v))).clamp(-1.2, 1.2)
        self.tag = f"lpips[B{B} {H}x{W} v{v}]"

    def oracle(self, seed):
        orc = _oracle_net("lpips", seed)
        xr = self.x.double().requires_grad_()
        val = orc(xr, self.ref.double()).flatten()
        val.sum().backward()
        sd = unit_seed(xr.grad)
        return {"fwd": val.detach().float(), "bwd": (xr.grad * sd).float(), "sd": sd}

    def set_reference(self, dev):
        dev.set_reference(self.ref.to(DEV))

    def loss_grad(self, dev, sd):
        # loss and g start as NaN sentinels: a call that wrote nothing cannot pass on what an earlier identical call left in recycled memory
        return dev.loss_grad(self.x.to(DEV), grad_scale=sd, g=_nan_like(tuple(self.x.shape)), loss=_nan_like((self.x.shape[0],)))

    def run(self, dev, sd):
        self.set_reference(dev)
        return self.loss_grad(dev, sd)


def oracle(call, seed):
    key = (call.kind, seed) + call.key
    if key not in _ORACLE:
        _ORACLE[key] = call.oracle(seed)
    return _ORACLE[key]


def run_pass(call, dev, seed):
    """forward + backward of `call` on `dev` -> (fwd, bwd) on the CPU"""
    sd = oracle(call, seed)["sd"]
    if call.kind == "lpips":
        loss, gx = call.run(dev, sd)
        th.cuda.synchronize()
        return loss.cpu(), gx.cpu()
    # outputs start as NaN sentinels (`rec` fails on a non-finite result): the warm passes repeat the inputs of earlier steps, and torch's allocator
    # may hand a new output the memory of the earlier identical result — a pass that silently wrote nothing must not compare equal
    ora = oracle(call, seed)
    o = call.forward(dev, out=_nan_like(tuple(ora["fwd"].shape)))
    gx = None
    if call.dgrad is not None:
        gshape = call.grad_shape() if hasattr(call, "grad_shape") else tuple(ora["bwd"].shape)
        gx = call.dgrad(dev, sd, _nan_like(gshape))
    th.cuda.synchronize()
    return o.cpu(), None if gx is None else gx.cpu()


def fresh(call, seed, precision=1):
    """the same call on a fresh handle in a fresh context (cached)"""
    key = (call.kind, seed, precision, getattr(call, "layout", 0)) + call.key
    if key not in _FRESH:
        ctx = _ctx(precision)
        dev = _handle(ctx, call.kind, seed, call.case)
        _FRESH[key] = run_pass(call, dev, seed)
        dev.close()
        ctx.close()
    return _FRESH[key]


def judge(recs, where, call, seed, got, precision=1, bitwise=True):
    """the two verdicts on one pass: strict (relu-flips for the ReLU towers' gradient) against the oracle, bit-equal to a fresh handle"""
    fwd, bwd = got
    ora = oracle(call, seed)
    tag = f"{where}: {call.tag} w{seed} p{precision}"
    recs.append(rec(f"{tag} forward", fwd, ora["fwd"]))
    if bwd is not None:
        recs.append((rec_flips if call.flips else rec)(f"{tag} dgrad", bwd, ora["bwd"]))
    if bitwise:
        f_fwd, f_bwd = fresh(call, seed, precision)
        recs.append(_flag(f"{tag} forward bit-equal to a fresh handle", th.equal(fwd, f_fwd)))
        if bwd is not None:
            recs.append(_flag(f"{tag} dgrad bit-equal to a fresh handle", th.equal(bwd, f_bwd)))
    return recs


def walk(recs, where, dev, calls, seed, precision=1):
    for k, call in enumerate(calls):
        judge(recs, f"{where} step {k}", call, seed, run_pass(call, dev, seed), precision)
    return recs


def allocs(ctx):
    return int(ctx.lib.cgd_ctx_device_allocs(ctx.h))


def _refusal(fn):
    """the message of the CgdError `fn` raises ('' when it does not raise)"""
    from cgd_amd import lib
    try:
        fn()
    except lib.CgdError as e:
        return str(e)
    th.cuda.synchronize()
    return ""


def _nan_like(shape):
    return th.full(shape, float("nan"), device=DEV)


def _untouched(t):
    th.cuda.synchronize()
    return bool(th.isnan(t).all().item())


def unet_calls(table, case=UNET_CASE, v0=0):
    return [UNetCall(B, H, W, v0 + k, case) for k, (B, H, W) in enumerate(table)]


# ---- 1. shape walks + 8. no allocation once warm ------------------------------------------------------------------------------------------
def check_unet_shape_walk(precision=1):
    """One `mini` handle through UNET_WALK (precision 0: its first three steps).  The step to 128 x 128 grows every buffer (stale `dst` / `cats` /
    `hs` / `head_in` views, ChanStatsEntry records keyed by the old pointers), crosses wino_min_m (Winograd copies packed mid-life) and takes
    GroupNorm epilogue records per sample; the way back runs on buffers that are too large; 32 x 48 is non-square with widths the halo
    kernels refuse on its lower levels (implicit GEMM, deferred split-K slices), 32 x 64 the non-square step of the weight-streaming conv kernel.
    At precision 1 the walk is followed by UNET_WARM, during which the context must not allocate, and UNET_LARGER, which must."""
    ctx = _ctx(precision)
    seed = SEEDS["unet"][0]
    dev = _handle(ctx, "unet", seed, UNET_CASE)
    table = UNET_WALK if precision == 1 else UNET_WALK_F32
    recs = walk([], f"unet walk p{precision}", dev, unet_calls(table), seed, precision)
    if precision == 1:
        a0 = allocs(ctx)
        for k, (B, H, W) in enumerate(UNET_WARM):
            call = UNetCall(B, H, W, UNET_WALK.index((B, H, W)))  # the variants of the walk: oracle and fresh results are cached
            judge(recs, f"unet warm pass {k}", call, seed, run_pass(call, dev, seed), precision)
        recs.append(_flag(f"unet warm: no device allocation in 8 passes after the largest shape ({allocs(ctx) - a0} made)", allocs(ctx) == a0))
        big = UNetCall(*UNET_LARGER, 7)
        judge(recs, "unet larger batch", big, seed, run_pass(big, dev, seed), precision)
        recs.append(_flag("unet warm: the allocation counter moves when a larger shape arrives", allocs(ctx) > a0))
    return recs


def check_unet_cfg64_walk():
    """cfg64 (the 64 x 64 checkpoint configuration: attention at 32^2 / 16^2 / 8^2) B1 -> B2 -> B1: AttnBlock scratch grows."""
    ctx = _ctx(1)
    dev = _handle(ctx, "unet", 1234, "cfg64")
    return walk([], "unet cfg64 walk", dev, unet_calls(CFG64_WALK, "cfg64"), 1234)


def check_tower_walks():
    """7. batch walks of the four other families, each on one handle; the ViT walk covers both image layouts and is followed by the warm /
    larger allocation check."""
    recs = []
    ctx = _ctx(1)
    vit = _handle(ctx, "vit", SEEDS["vit"][0])
    a_cold = allocs(ctx)
    walk(recs, "vit walk", vit, [VitCall(N, lay) for (N, lay) in VIT_WALK], SEEDS["vit"][0])
    a0 = allocs(ctx)
    recs.append(_flag("vit walk: per-layer activations grew during the walk", a0 > a_cold))
    for k, (N, lay) in enumerate(VIT_WARM):
        call = VitCall(N, lay)
        judge(recs, f"vit warm pass {k}", call, SEEDS["vit"][0], run_pass(call, vit, SEEDS["vit"][0]))
    recs.append(_flag(f"vit warm: no device allocation in 8 passes after the largest batch ({allocs(ctx) - a0} made)", allocs(ctx) == a0))
    big = VitCall(*VIT_LARGER)
    judge(recs, "vit larger batch", big, SEEDS["vit"][0], run_pass(big, vit, SEEDS["vit"][0]))
    recs.append(_flag("vit warm: the allocation counter moves when a larger batch arrives", allocs(ctx) > a0))
    vit.close()
    walk(recs, "text walk", _handle(ctx, "text", SEEDS["text"][0]), [TextCall(n) for n in TEXT_WALK], SEEDS["text"][0])
    walk(recs, "resnet walk", _handle(ctx, "rn", SEEDS["rn"][0]), [RnCall(n) for n in RN_WALK], SEEDS["rn"][0])
    lp = _handle(ctx, "lpips", SEEDS["lpips"][0])
    walk(recs, "lpips walk", lp, [LpipsCall(*s) for s in LPIPS_WALK], SEEDS["lpips"][0])
    # loss_grad with an x of another shape than the reference: the C entry point takes no shape (it runs at the reference's), so the wrapper
    # (nets.LpipsVGG.loss_grad) refuses the call before it reaches the library
    other = LpipsCall(1, 96, 128)
    gbuf, lbuf = _nan_like((1, 3, 96, 128)), _nan_like((1,))
    try:
        lp.loss_grad(other.x.to(DEV), g=gbuf, loss=lbuf)
        msg = ""
    except AssertionError as e:
        msg = str(e)
    recs.append(_flag("lpips: loss_grad with x of another shape than the reference is refused by the wrapper", "same shape" in msg))
    recs.append(_flag("lpips: ... and leaves g and loss untouched", _untouched(gbuf) and _untouched(lbuf)))
    last = LpipsCall(*LPIPS_WALK[-1])
    sd = oracle(last, SEEDS["lpips"][0])["sd"]
    loss, gx = last.loss_grad(lp, sd)  # the reference of the walk's last step is still in place
    judge(recs, "lpips after the refused call", last, SEEDS["lpips"][0], (loss.cpu(), gx.cpu()))
    return recs


# ---- 2. order of passes ------------------------------------------------------------------------------------------------------------------
def _order(recs, where, dev, A, Bc, seed, bad_forward, good_after):
    oa, ob = oracle(A, seed), oracle(Bc, seed)
    # forward(A), forward(B), dgrad: the gradient of B
    A.forward(dev)
    fb = Bc.forward(dev).clone()
    gb = Bc.dgrad(dev, ob["sd"]).clone()
    judge(recs, f"{where} forward(A) forward(B) dgrad", Bc, seed, (fb.cpu(), gb.cpu()))
    # forward(A), dgrad, dgrad with another seed, dgrad with the first seed again: each is right
    fa = A.forward(dev).clone()
    g1 = A.dgrad(dev, oa["sd"]).clone()
    g2 = A.dgrad(dev, -0.5 * oa["sd"]).clone()
    g3 = A.dgrad(dev, oa["sd"]).clone()
    judge(recs, f"{where} forward(A) dgrad", A, seed, (fa.cpu(), g1.cpu()))
    recs.append((rec_flips if A.flips else rec)(f"{where} second dgrad of the same forward, seed x -0.5", g2.cpu(), -0.5 * oa["bwd"]))
    recs.append(_flag(f"{where} third dgrad of the same forward, first seed again: bit-equal to the first", th.equal(g3, g1)))
    # a refused forward between a good forward and its dgrad
    fa = A.forward(dev).clone()
    msg = _refusal(bad_forward)
    recs.append(_flag(f"{where} the bad forward is refused with a message ({msg[:60]!r})", bool(msg)))
    gx = _nan_like(tuple(oa["bwd"].shape))
    msg2 = _refusal(lambda: A.dgrad(dev, oa["sd"], gx))
    if msg2:  # a refusal: with a message, g_x untouched
        recs.append(_flag(f"{where} dgrad after the refused forward refuses and leaves g_x untouched", _untouched(gx)))
    else:     # or bit for bit the gradient of the last successful forward
        recs.append(_flag(f"{where} dgrad after the refused forward = the gradient of the last successful forward, bit for bit", th.equal(gx, g1)))
    judge(recs, f"{where} after the refused forward", good_after, seed, run_pass(good_after, dev, seed))
    return recs


def check_pass_order():
    recs = []
    ctx = _ctx(1)
    seed = SEEDS["unet"][0]
    unet = _handle(ctx, "unet", seed, UNET_CASE)
    A, Bc = UNetCall(1, 64, 64, 0), UNetCall(2, 32, 48, 3)
    bad = th.zeros(1, 3, 66, 64, device=DEV)  # mini has three levels: H must be a multiple of 4 — refused by UNet::forward before anything is launched
    obuf = _nan_like((1, 6, 66, 64))
    _order(recs, "unet order:", unet, A, Bc, seed, lambda: unet.forward(bad, A.t.to(DEV), A.y.to(DEV), out=obuf), UNetCall(1, 64, 64, 2))
    recs.append(_flag("unet order: the refused forward wrote nothing", _untouched(obuf)))
    unet.close()
    vs = SEEDS["vit"][0]
    vit = _handle(ctx, "vit", vs)
    VA, VB = VitCall(3), VitCall(1)
    # the image tower refuses a forward between set_param and finalize; the refusal case of the UNet (a shape) has no counterpart: N is free
    name, numel = vit.param_specs()[0]
    w0 = _sd("vit", _oracle_net("vit", vs))["visual." + name].contiguous()

    def bad_vit():
        ctx.check(ctx.lib.cgd_vit_set_param(vit.h, name.encode(), w0.data_ptr(), numel))
        VB.forward(vit)

    # (the refused forward leaves the handle un-finalized: dgrad must refuse too, and finalize + forward must bring it back)
    _order(recs, "vit order:", vit, VA, VB, vs, bad_vit, _Refinalized(vit, VitCall(3), ctx))
    return recs


class _Refinalized:
    """a call whose forward finalizes the handle first (same weights): the way back from a set_param without finalize"""

    def __init__(self, dev, call, ctx):
        self._dev, self._call, self._ctx = dev, call, ctx
        for k in ("kind", "flips", "case", "key", "tag", "oracle", "dgrad"):
            setattr(self, k, getattr(call, k))

    def forward(self, dev, out=None):
        self._ctx.check(self._ctx.lib.cgd_vit_finalize(dev.h))
        return self._call.forward(dev, out=out)


# ---- 3. weight re-upload ------------------------------------------------------------------------------------------------------------------
def _call_of(kind):
    return {"unet": lambda: UNetCall(1, 128, 128, 4), "vit": lambda: VitCall(3), "text": lambda: TextCall(4), "rn": lambda: RnCall(2),
            "lpips": lambda: LpipsCall(2, 64, 64)}[kind]()


def check_reupload(kind):
    """Weights of seed 1, a pass, weights of seed 2 into the SAME handle, a pass: strict against the seed-2 oracle and bit-equal to a fresh seed-2
    handle (UNet at 128 x 128: Winograd copies and fragment-cache entries of seed 1 exist; transposed weights are refilled, not reallocated).  Then
    one set_param without finalize: every pass entry refuses with the finalize message and writes nothing."""
    recs = []
    ctx = _ctx(1)
    s1, s2 = SEEDS[kind]
    case = UNET_CASE if kind == "unet" else None
    dev = _handle(ctx, kind, s1, case)
    call = _call_of(kind)
    judge(recs, f"{kind} re-upload: seed 1", call, s1, run_pass(call, dev, s1))
    if kind == "unet":
        dev.embed(call.t.to(DEV), call.y.to(DEV), 1)  # FiLM projections of the seed-1 weights in slot 1
    _load(dev, kind, s2, case)
    if kind == "unet":  # ... which UNet::finalize invalidates: forward_slot refuses before any launch
        obuf = _nan_like(tuple(oracle(call, s2)["fwd"].shape))
        msg = _refusal(lambda: dev.forward_slot(call.x.to(DEV), 1, out=obuf))
        recs.append(_flag("unet re-upload: forward_slot on an embedding of the previous weights is refused and writes nothing",
                          "preceding embed()" in msg and _untouched(obuf)))
    if kind in ("unet", "vit", "rn"):  # new weights: the activations of the last forward are not theirs
        gx = _nan_like(tuple(oracle(call, s2)["bwd"].shape))
        msg = _refusal(lambda: call.dgrad(dev, 1.0, gx))
        recs.append(_flag(f"{kind} re-upload: dgrad of a forward under the previous weights is refused ({msg[-50:]!r})", "forward" in msg and _untouched(gx)))
    if kind == "lpips":  # ... and neither are the reference features (Lpips::finalize drops them)
        gx, lbuf = _nan_like(tuple(call.x.shape)), _nan_like((call.x.shape[0],))
        msg = _refusal(lambda: dev.loss_grad(call.x.to(DEV), g=gx, loss=lbuf))
        recs.append(_flag(f"lpips re-upload: loss_grad against the previous weights' reference is refused ({msg[-40:]!r})",
                          "no reference" in msg and _untouched(gx) and _untouched(lbuf)))
    judge(recs, f"{kind} re-upload: seed 2 in the same handle", call, s2, run_pass(call, dev, s2))
    # one tensor without finalize
    name, numel = dev.param_specs()[1]
    t = th.zeros(numel, device=DEV)
    ctx.check(dev._fn("set_param")(dev.h, name.encode(), t.data_ptr(), numel))
    word = "finalize"
    if kind == "lpips":
        gx, lbuf = _nan_like(tuple(call.x.shape)), _nan_like((call.x.shape[0],))
        m1 = _refusal(lambda: dev.loss_grad(call.x.to(DEV), g=gx, loss=lbuf))
        m2 = _refusal(lambda: call.set_reference(dev))
        recs.append(_flag(f"lpips: passes between set_param and finalize refuse ({m1[-30:]!r})", word in m1 and word in m2 and _untouched(gx) and _untouched(lbuf)))
    else:
        fshape = tuple(oracle(call, s2)["fwd"].shape)
        obuf = _nan_like(fshape)
        if kind == "unet":
            m1 = _refusal(lambda: dev.forward(call.x.to(DEV), call.t.to(DEV), call.y.to(DEV), out=obuf))
        elif kind == "text":
            m1 = _refusal(lambda: dev.encode_text(call.tok.to(DEV), out=obuf))
        else:
            m1 = _refusal(lambda: dev.encode_image(call.img.to(DEV), out=obuf))
        recs.append(_flag(f"{kind}: forward between set_param and finalize refuses and writes nothing ({m1[-40:]!r})", word in m1 and _untouched(obuf)))
        if call.dgrad is not None:
            gx = _nan_like(tuple(oracle(call, s2)["bwd"].shape))
            m2 = _refusal(lambda: call.dgrad(dev, 1.0, gx))
            recs.append(_flag(f"{kind}: dgrad between set_param and finalize refuses and writes nothing ({m2[-40:]!r})", word in m2 and _untouched(gx)))
    # back: the full seed-2 upload again
    _load(dev, kind, s2, case)
    judge(recs, f"{kind} re-upload: after the refused passes", call, s2, run_pass(call, dev, s2))
    return recs


# ---- 4. embedding slots -------------------------------------------------------------------------------------------------------------------
def check_embed_slots():
    recs = []
    ctx = _ctx(1)
    seed = SEEDS["unet"][0]
    dev = _handle(ctx, "unet", seed, UNET_CASE)
    c1, c2 = UNetCall(1, 64, 64, 0), UNetCall(2, 64, 64, 8)
    dev.embed(c1.t.to(DEV), c1.y.to(DEV), 0)
    dev.embed(c2.t.to(DEV), c2.y.to(DEV), 1)
    for slot, call in ((0, c2), (1, c1)):  # the other batch size
        obuf = _nan_like((call.x.shape[0], 6, 64, 64))
        msg = _refusal(lambda: dev.forward_slot(call.x.to(DEV), slot, out=obuf))
        recs.append(_flag(f"embed slots: forward_slot({slot}) with the other batch size refuses and writes nothing", "same batch size" in msg and _untouched(obuf)))
    # four alternating-slot steps, distinct t, the batch changes between steps 2 and 3; the next step's embed runs before this step's forward
    steps = [UNetCall(1, 64, 64, 0), UNetCall(1, 64, 64, 2), UNetCall(2, 64, 64, 8), UNetCall(2, 64, 64, 9)]
    dev.embed(steps[0].t.to(DEV), steps[0].y.to(DEV), 0)
    for k, call in enumerate(steps):
        if k + 1 < len(steps):
            nxt = steps[k + 1]
            dev.embed(nxt.t.to(DEV), nxt.y.to(DEV), (k + 1) & 1)
        o = dev.forward_slot(call.x.to(DEV), k & 1).clone()
        gx = call.dgrad(dev, oracle(call, seed)["sd"]).clone()
        th.cuda.synchronize()
        judge(recs, f"embed slots step {k} (slot {k & 1}) = plain forward(x, t, y)", call, seed, (o.cpu(), gx.cpu()))
    return recs


# ---- 5. several handles in one context ----------------------------------------------------------------------------------------------------
def check_shared_context():
    recs = []
    ctx = _ctx(1)
    su, (sv1, sv2), st, sr, sl = SEEDS["unet"][0], SEEDS["vit"], SEEDS["text"][0], SEEDS["rn"][0], SEEDS["lpips"][0]
    unet, vit1, vit2 = _handle(ctx, "unet", su, UNET_CASE), _handle(ctx, "vit", sv1), _handle(ctx, "vit", sv2)
    text, rn, lp = _handle(ctx, "text", st), _handle(ctx, "rn", sr), _handle(ctx, "lpips", sl)
    cu, cv, ct, cr, cl = UNetCall(1, 128, 128, 4), VitCall(3), TextCall(4), RnCall(2), LpipsCall(2, 64, 64)
    # all forwards, then the backwards in another order
    fu, fv1, fv2, ft, fr = cu.forward(unet), cv.forward(vit1), cv.forward(vit2), ct.forward(text), cr.forward(rn)
    cl.set_reference(lp)
    gr = cr.dgrad(rn, oracle(cr, sr)["sd"])
    ll, gl = cl.loss_grad(lp, oracle(cl, sl)["sd"])
    gv2 = cv.dgrad(vit2, oracle(cv, sv2)["sd"])
    gu = cu.dgrad(unet, oracle(cu, su)["sd"])
    gv1 = cv.dgrad(vit1, oracle(cv, sv1)["sd"])
    th.cuda.synchronize()
    for call, seed, got in ((cu, su, (fu, gu)), (cv, sv1, (fv1, gv1)), (cv, sv2, (fv2, gv2)), (ct, st, (ft, None)), (cr, sr, (fr, gr)), (cl, sl, (ll, gl))):
        judge(recs, "shared context, interleaved", call, seed, tuple(None if t is None else t.cpu() for t in got))
    # destroy one ViT tower between the other's forward and dgrad (its destroy clears the shared fragment cache)
    f1 = cv.forward(vit1).clone()
    vit2.close()
    g1 = cv.dgrad(vit1, oracle(cv, sv1)["sd"]).clone()
    th.cuda.synchronize()
    judge(recs, "shared context, other tower destroyed between forward and dgrad", cv, sv1, (f1.cpu(), g1.cpu()))
    judge(recs, "shared context, next pass after the destroy", cv, sv1, run_pass(cv, vit1, sv1))
    # destroy the UNet between an LPIPS set_reference / loss_grad pair and the next loss_grad (clears chanstats and the cache; LPIPS uses neither)
    cl.set_reference(lp)
    l1, gx1 = cl.loss_grad(lp, oracle(cl, sl)["sd"])
    l1, gx1 = l1.clone(), gx1.clone()
    unet.close()
    l2, gx2 = cl.loss_grad(lp, oracle(cl, sl)["sd"])
    th.cuda.synchronize()
    judge(recs, "shared context, lpips after the UNet's destroy", cl, sl, (l2.cpu(), gx2.cpu()))
    recs.append(_flag("shared context: lpips loss_grad unchanged by the UNet's destroy", th.equal(l1, l2) and th.equal(gx1, gx2)))
    # a new tower with new weights after the destroys: its allocations may be recycled ones
    vit3 = _handle(ctx, "vit", sv2)
    judge(recs, "shared context, tower created after the destroys", cv, sv2, run_pass(cv, vit3, sv2))
    unet2 = _handle(ctx, "unet", SEEDS["unet"][1], UNET_CASE)
    judge(recs, "shared context, UNet created after the destroys", cu, SEEDS["unet"][1], run_pass(cu, unet2, SEEDS["unet"][1]))
    judge(recs, "shared context, surviving tower at the end", cv, sv1, run_pass(cv, vit1, sv1))
    return recs


# ---- 6. precision switch on a live context ------------------------------------------------------------------------------------------------
def check_precision_switch():
    recs = []
    ctx = _ctx(1)
    su, sv = SEEDS["unet"][0], SEEDS["vit"][0]
    unet, vit = _handle(ctx, "unet", su, UNET_CASE), _handle(ctx, "vit", sv)
    cu, cv = UNetCall(1, 128, 128, 4), VitCall(3)
    for p in (1, 0, 1):  # whole passes under each mode (the UNet's Winograd copies are repacked at every switch)
        ctx.set_precision(p)
        judge(recs, f"precision switch -> {p}", cu, su, run_pass(cu, unet, su), p)
        judge(recs, f"precision switch -> {p}", cv, sv, run_pass(cv, vit, sv), p)
    # a switch between forward and dgrad: UNet::dgrad / ViT::dgrad refuse before any launch (the saved activations, the attention scratch and
    # the Winograd copies belong to the forward's mode); back under the forward's mode the gradient is the fresh handle's
    for name, dev, call, seed in (("unet", unet, cu, su), ("vit", vit, cv, sv)):
        f = call.forward(dev).clone()
        ctx.set_precision(0)
        gx = _nan_like(tuple(oracle(call, seed)["bwd"].shape))
        msg = _refusal(lambda: call.dgrad(dev, oracle(call, seed)["sd"], gx))
        recs.append(_flag(f"precision switch: {name} dgrad under another mode than its forward refuses, g_x untouched ({msg[-45:]!r})",
                          "precision mode" in msg and _untouched(gx)))
        ctx.set_precision(1)
        gx = call.dgrad(dev, oracle(call, seed)["sd"]).clone()
        th.cuda.synchronize()
        judge(recs, f"precision switch: {name} dgrad back under the forward's mode", call, seed, (f.cpu(), gx.cpu()))
    return recs


# ---- the classic architecture (conv resampling, additive embedding) through the same sequences ------------------------------------------------
CLASSIC_CASE = "classic_narrow"
CLASSIC_WALK = [(1, 64, 64), (2, 128, 128), (1, 64, 64), (2, 32, 64), (1, 128, 128), (2, 128, 128)]
CLASSIC_WARM = [(1, 64, 64), (2, 32, 64), (2, 128, 128), (1, 128, 128)]


def check_classic_walk():
    """One handle of the narrow community structure through CLASSIC_WALK at precision 1: Downsample / Upsample own grow-only buffers (`out`, `dx`,
    `d1`), views stashed into the concat buffers (`dst`) and the B, H, W the forward saved for the backward; the step to 128 x 128 grows them all,
    the way back runs on buffers that are too large, 32 x 64 is non-square with a 1 x 2 bottom map.  Then CLASSIC_WARM, during which the context
    must not allocate."""
    ctx = _ctx(1)
    seed = SEEDS["unet"][0]
    dev = _handle(ctx, "unet", seed, CLASSIC_CASE)
    recs = walk([], "classic walk", dev, unet_calls(CLASSIC_WALK, CLASSIC_CASE), seed)
    a0 = allocs(ctx)
    for k, (B, H, W) in enumerate(CLASSIC_WARM):
        call = UNetCall(B, H, W, CLASSIC_WALK.index((B, H, W)), CLASSIC_CASE)
        judge(recs, f"classic warm pass {k}", call, seed, run_pass(call, dev, seed))
    recs.append(_flag(f"classic warm: no device allocation in {len(CLASSIC_WARM)} passes after the largest shape ({allocs(ctx) - a0} made)", allocs(ctx) == a0))
    dev.close()
    return recs


def check_classic_order_reupload_and_precision():
    """forward(A) forward(B) dgrad, three dgrads of one forward, a forward refused for its frame (48 x 48 is no multiple of 32) between a forward
    and its dgrad; weights of seed 2 into the handle that ran seed 1 (the packed stride-2 conv weights are refilled); precision 1 -> 0 -> 1"""
    recs = []
    ctx = _ctx(1)
    s1, s2 = SEEDS["unet"]
    dev = _handle(ctx, "unet", s1, CLASSIC_CASE)
    A, Bc = UNetCall(1, 64, 64, 0, CLASSIC_CASE), UNetCall(2, 32, 64, 3, CLASSIC_CASE)
    bad, obuf = th.zeros(1, 3, 48, 48, device=DEV), _nan_like((1, 6, 48, 48))
    _order(recs, "classic order:", dev, A, Bc, s1, lambda: dev.forward(bad, A.t.to(DEV), None, out=obuf), UNetCall(1, 64, 64, 2, CLASSIC_CASE))
    recs.append(_flag("classic order: the refused forward wrote nothing", _untouched(obuf)))
    _load(dev, "unet", s2, CLASSIC_CASE)
    judge(recs, "classic re-upload: seed 2 into the handle that ran seed 1", A, s2, run_pass(A, dev, s2))
    _load(dev, "unet", s1, CLASSIC_CASE)
    for p in (1, 0, 1):
        ctx.set_precision(p)
        judge(recs, f"classic precision switch -> {p}", A, s1, run_pass(A, dev, s1), p)
    dev.close()
    return recs


def check_classic_shared_context():
    """a classic and a published-architecture handle interleaved in one context: forward(classic), forward(mini), dgrad(classic), dgrad(mini), twice
    (the split-K workspace, `ctx->pending`, the GroupNorm record pool and the packed-weight scratch are the context's)"""
    recs = []
    ctx = _ctx(1)
    seed = SEEDS["unet"][0]
    classic, mini = _handle(ctx, "unet", seed, CLASSIC_CASE), _handle(ctx, "unet", seed, UNET_CASE)
    for k, (cc, cm) in enumerate(((UNetCall(1, 64, 64, 0, CLASSIC_CASE), UNetCall(1, 64, 64, 0)), (UNetCall(2, 32, 64, 3, CLASSIC_CASE), UNetCall(2, 32, 64, 6)))):
        fc = cc.forward(classic).clone()
        fm = cm.forward(mini).clone()
        gc = cc.dgrad(classic, oracle(cc, seed)["sd"]).clone()
        gm = cm.dgrad(mini, oracle(cm, seed)["sd"]).clone()
        th.cuda.synchronize()
        judge(recs, f"classic + mini interleaved, round {k}", cc, seed, (fc.cpu(), gc.cpu()))
        judge(recs, f"classic + mini interleaved, round {k}", cm, seed, (fm.cpu(), gm.cpu()))
    classic.close()
    mini.close()
    return recs


# ---- 9. two sampler runs on the same objects ----------------------------------------------------------------------------------------------
def check_two_runs():
    """The `mini` scene of step_checks.py, two guided steps at 64 x 64, then another scene (64 x 96, other prompt weights, other cutn) on the same
    context, network handles and sampler: the second run is judged by `compare` against the oracle, and its x_{t-1}, g and loss scalars are
    bit-equal to those of the second scene run on fresh objects."""
    from tests import step_checks as sc

    def snap(it):
        out = []
        for o, guid, legs in it:
            out.append(({k: v.clone() for k, v in o.items() if th.is_tensor(v)}, sc._FrozenLog(guid.log()), legs))
        return out

    first = sc.Scenario("mini", steps=2, hw=(64, 64))
    second = dict(steps=2, hw=(64, 96), cutn=6, P=2, weights=[0.7, 0.3])
    snap(first.run_device(1))
    s2 = sc.Scenario("mini", **second)
    reused = snap(s2.run_device(1, reuse=first.dev_objs))
    recs = sc.compare(s2, 1, s2.run_oracle(), iter(reused))
    s3 = sc.Scenario("mini", **second)
    clean = snap(s3.run_device(1))
    for k, ((o_r, log_r, legs_r), (o_c, log_c, legs_c)) in enumerate(zip(reused, clean)):
        recs.append(_flag(f"two runs: step {k} x_(t-1) bit-equal to a run on fresh objects", th.equal(o_r["sample"], o_c["sample"])))
        recs.append(_flag(f"two runs: step {k} g bit-equal to a run on fresh objects", legs_r is not None and th.equal(legs_r["g"], legs_c["g"])))
        same = all(log_r.log()[key] == log_c.log()[key] or (math.isnan(log_r.log()[key]) and math.isnan(log_c.log()[key])) for key in log_c.log())
        recs.append(_flag(f"two runs: step {k} loss scalars equal to a run on fresh objects", same and len(log_c.log()) > 0))
    return recs


def unet_buffer_counts(case, B, H, W):
    """Host-only: element counts of the buffer classes a UNet handle sizes by (B, H, W), derived from the configuration — the embedding head (B rows),
    per level the activations (B * h * w * channels) and, where the level carries attention, the qkv rows and an upper bound of the attention scratch
    (B * heads * T * T probabilities)."""
    kw = pc.UNET_CASES[case]
    from cgd_amd import nets
    mult = kw.get("channel_mult") or nets.DEFAULT_CHANNEL_MULT[kw["image_size"]]
    att = [kw["image_size"] // int(r) for r in str(kw["attention_resolutions"]).split(",")]
    mc = kw["model_channels"]
    out = {"embedding head": B * 4 * mc}
    for lvl, m in enumerate(mult):
        h, w, ch = H >> lvl, W >> lvl, int(m * mc)
        out[f"level {lvl} activations"] = B * h * w * ch
        out[f"level {lvl} concat"] = B * h * w * 2 * ch
        if (1 << lvl) in att:
            heads = ch // kw["num_head_channels"] if kw.get("num_head_channels", -1) != -1 else kw.get("num_heads", 4)
            out[f"level {lvl} qkv"] = B * h * w * 3 * ch
            out[f"level {lvl} attention scratch"] = B * heads * (h * w) ** 2
    return out


def classic_resample_counts(case, B, H, W):
    """Host-only: element counts of the grow-only buffers of the classic architecture's resampling modules (unet.hip Downsample / Upsample), from the
    configuration: the Downsample under level l reads B x h x w x ch (`dx`) and writes a quarter of it (`out`); the Upsample above level l + 1
    reads B x (h / 2) x (w / 2) x ch' (`dx`) and writes four times that (`out`, and `d1`, the conv's gradient at the high resolution)"""
    kw = pc.UNET_CASES[case]
    mult, mc = kw["channel_mult"], kw["model_channels"]
    out = {}
    for lvl in range(len(mult) - 1):
        h, w = H >> lvl, W >> lvl
        ch, chu = int(mult[lvl] * mc), int(mult[lvl + 1] * mc)
        out[f"Downsample {lvl} dx"] = B * h * w * ch
        out[f"Downsample {lvl} out"] = B * (h // 2) * (w // 2) * ch
        out[f"Upsample {lvl + 1} dx"] = B * (h // 2) * (w // 2) * chu
        out[f"Upsample {lvl + 1} out"] = out[f"Upsample {lvl + 1} d1"] = B * h * w * chu
    return out


GROUPS = {
    "unet_walk": [lambda: check_unet_shape_walk(1), lambda: check_unet_shape_walk(0), check_unet_cfg64_walk],
    "order": [check_pass_order],
    "reupload": [lambda k=k: check_reupload(k) for k in ("unet", "vit", "text", "rn", "lpips")],
    "slots": [check_embed_slots],
    "shared": [check_shared_context],
    "precision": [check_precision_switch],
    "towers": [check_tower_walks],
    "two_runs": [check_two_runs],
    "classic": [check_classic_walk, check_classic_order_reupload_and_precision, check_classic_shared_context],
}
