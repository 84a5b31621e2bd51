"""GPU tests (pytest -m gpu) of the super-resolution path: the conditioned stem op (csrc/superres.hip) against the float64 restatement
(tests/superres_ref.py), a 6-channel UNet handle against the oracle UNet wrapped as guided-diffusion's SuperResModel (forward and
dgrad), the handle across call sequences, and one guided p_sample / DDIM step with model_kwargs = {"y", "low_res"} against the oracle
diffusion.  Tolerance: the project's, literally, |a - b| <= 1e-4 + 1e-3 |ref| for every element (parity_checks.rec)."""
import pytest
import torch as th
import torch.nn.functional as F

from tests import parity_checks as pc
from tests import step_checks as sc
from tests import superres_ref as sr
from tests.parity_checks import DEV, g, rec

pytestmark = pytest.mark.gpu

# image 32, 32 channels, mult (1, 2), one ResBlock per level, attention at 16x16, class-conditional, a 6-channel stem
SR_CASE = dict(image_size=32, model_channels=32, num_res_blocks=1, attention_resolutions="16", channel_mult=(1, 2), num_classes=10,
               num_head_channels=32, in_channels=6)
FRAME, LOW = (32, 40), (8, 10)


def _assert_all(recs):
    bad = [r for r in recs if not r["ok"]]
    assert not bad, "; ".join(f"{r['name']} [{r['criterion']}]: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e}"
                              + (" VACUOUS" if r.get("vacuous") else "") for r in bad)
    assert all(r["criterion"] == "strict" for r in recs)


class SuperResModel(th.nn.Module):
    """guided_diffusion.unet.SuperResModel over the oracle UNet: model(x, t, y, low_res) = unet(cat([x, bilinear(low_res)], 1), t, y).
    `low_res` may also be held by the module (the oracle loops of tests/step_checks.py build their own model_kwargs)."""

    def __init__(self, unet, low_res=None):
        super().__init__()
        self.unet, self.low_res = unet, low_res

    def forward(self, x, timesteps, y=None, low_res=None):
        low = self.low_res if low_res is None else low_res
        up = F.interpolate(low, x.shape[2:], mode="bilinear")
        if up.shape[0] == 1 and x.shape[0] > 1:
            up = up.expand(x.shape[0], -1, -1, -1)
        return self.unet(th.cat([x, up], dim=1), timesteps, y)

    def state_dict(self, *a, **k):  # the checkpoint's keys: the wrapper adds none
        return self.unet.state_dict(*a, **k)


# ---- op level ---------------------------------------------------------------------------------------------------------------------------
#            B  frame     low      B_low Cout
OP_CASES = {"a": (2, (32, 32), (8, 8), 2, 32),      # integer ratio, one tile column, a low-res image per sample
            "b": (2, (9, 70), (5, 7), 1, 192),      # rows no multiple of the tile height, columns across a 64-column tile, non-integer ratios, broadcast
            "c": (1, (6, 66), (1, 1), 1, 32),       # the one-pixel low-res image
            "d": (1, (9, 70), (9, 70), 1, 192)}     # ratio 1: the conditioning passes through exactly


def _op_operands(case):
    B, hw, lhw, B_low, cout = OP_CASES[case]
    x = th.randn(B, 3, *hw, generator=g(70))
    low = th.rand(B_low, 3, *lhw, generator=g(71)) * 2 - 1
    w = (th.rand(cout, 6, 3, 3, generator=g(72)) * 2 - 1) * (3.0 / 54) ** 0.5
    bias = th.randn(cout, generator=g(73)) * 0.02
    return x, low, w, bias


@pytest.fixture(scope="module")
def op_refs():
    """the float64 references, computed once and shared"""
    return {case: sr.sr_stem(*_op_operands(case)) for case in OP_CASES}


@pytest.mark.parametrize("case", sorted(OP_CASES))
def test_sr_stem_against_the_restatement(case, op_refs):
    from cgd_amd import ops
    ctx = pc._ctx(1)
    x, low, w, bias = _op_operands(case)
    wf = ops.pack_conv3x3(w.to(DEV))[0]
    got = ops.sr_stem(ctx, x.to(DEV), low.to(DEV), wf, bias.to(DEV))
    th.cuda.synchronize()
    _assert_all([rec(f"sr_stem[{case}]", got, op_refs[case])])
    if case == "d":  # and without a bias the centre tap alone copies the conditioning plane bit for bit
        w1 = th.zeros(4, 6, 3, 3)
        for c in range(3):
            w1[c, 3 + c, 1, 1] = 1.0
        got = ops.sr_stem(ctx, x.to(DEV), low.to(DEV), ops.pack_conv3x3(w1.to(DEV))[0])
        assert th.equal(got[0, :, :, :3].cpu(), low[0].permute(1, 2, 0))


@pytest.mark.parametrize("c0,pad", [(4, 8), (1, 5)])  # 16-byte aligned rows (vector stores) and misaligned ones (scalar stores)
def test_sr_stem_on_offset_views_with_a_wider_row_stride(c0, pad, op_refs):
    from cgd_amd import ops
    ctx = pc._ctx(1)
    x, low, w, bias = _op_operands("b")
    B, _, H, W = x.shape
    cout = w.shape[0]

    def offset_view(t, off):  # the tensor as a contiguous view that starts `off` floats into a larger buffer
        buf = th.full((t.numel() + off + 3,), float("nan"), device=DEV)
        buf[off:off + t.numel()] = t.reshape(-1).to(DEV)
        return buf[off:off + t.numel()].view(t.shape)

    ld = cout + pad
    ybuf = th.full((B, H, W, ld), -77.0, device=DEV)
    out = ybuf[..., c0:c0 + cout]
    ops.sr_stem(ctx, offset_view(x, 3), offset_view(low, 1), ops.pack_conv3x3(w.to(DEV))[0], offset_view(bias, 2), out=out)
    th.cuda.synchronize()
    _assert_all([rec(f"sr_stem[b, views, ldy {ld}, offset {c0}]", out, op_refs["b"])])
    assert bool((ybuf[..., :c0] == -77.0).all()) and bool((ybuf[..., c0 + cout:] == -77.0).all())  # nothing outside the slice is written


def test_sr_stem_refusals():
    from cgd_amd import lib as L
    from cgd_amd import ops
    ctx = pc._ctx(1)
    x, low = th.zeros(2, 3, 8, 8, device=DEV), th.zeros(3, 3, 2, 2, device=DEV)
    with pytest.raises(ValueError):
        ops.sr_stem(ctx, x, low, th.zeros(32, 54, device=DEV))  # a low-res batch that is neither 1 nor B
    with pytest.raises(ValueError):
        ops.sr_stem(ctx, x, low[:1], th.zeros(32, 27, device=DEV))  # a 3-channel weight
    with pytest.raises(L.CgdError, match="multiple of 4"):
        ops.sr_stem(ctx, x, low[:1], th.zeros(30, 54, device=DEV))
    with pytest.raises(L.CgdError, match="at most 256"):
        ops.sr_stem(ctx, x, low[:1], th.zeros(260, 54, device=DEV))


# ---- net level ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sr_net():
    """oracle UNet (6-channel stem, synthetic init), inputs on a 32x40 frame with an 8x10 low-res image, and the reference forward /
    dgrad through the SuperResModel wrapper: computed once, read-only"""
    from oracle.unet import UNetModel, synthetic_init_
    unet = synthetic_init_(UNetModel(**SR_CASE), seed=1234).eval()
    for p in unet.parameters():
        p.requires_grad_(False)
    B, (H, W) = 2, FRAME
    ins = dict(x=th.randn(B, 3, H, W, generator=g(60)), t=th.tensor([417.0] * B), y=th.randint(0, 10, (B,), generator=g(61)),
               low_a=th.rand(B, 3, *LOW, generator=g(63)) * 2 - 1, low_b=th.rand(1, 3, *LOW, generator=g(64)) * 2 - 1)
    gout = th.randn(B, 6, H, W, generator=g(62))
    gout[:, 3:] = 0  # the guidance only seeds the epsilon channels
    model = SuperResModel(unet)
    refs = {}
    for key in ("low_a", "low_b"):
        xr = ins["x"].clone().requires_grad_()
        o = model(xr, ins["t"], ins["y"], low_res=ins[key])
        (o * gout).sum().backward()
        refs[key] = (o.detach(), xr.grad.clone())
    return unet, ins, gout, refs


def _device_net(ctx, unet):
    from cgd_amd import nets
    return nets.UNet(ctx, **SR_CASE).load_state_dict(pc.device_sd(unet))


def _dev_inputs(ins):
    return ins["x"].to(DEV), ins["t"].to(DEV), ins["y"].to(DEV)


@pytest.mark.parametrize("precision", [0, 1])
def test_six_channel_unet_forward_and_dgrad(precision, sr_net):
    unet, ins, gout, refs = sr_net
    dev = _device_net(pc._ctx(precision), unet)
    assert dev.in_channels == 6
    o_ref, g_ref = refs["low_a"]
    dev.set_low_res(ins["low_a"])  # a CPU tensor: the handle copies it to its device
    od = dev.forward(*_dev_inputs(ins))
    seed = pc.unit_seed(g_ref)
    gx = dev.dgrad((gout * seed).to(DEV))
    th.cuda.synchronize()
    assert tuple(gx.shape) == (2, 3) + FRAME  # only d/dx exists: no gradient planes for the conditioning
    tag = f"sr unet[p{precision} B2 {FRAME[0]}x{FRAME[1]} low {LOW[0]}x{LOW[1]}]"
    _assert_all([rec(f"{tag} forward", od, o_ref), rec(f"{tag} dgrad", gx, g_ref * seed)])


def test_call_sequences(sr_net):
    from cgd_amd import lib as L
    unet, ins, gout, refs = sr_net
    ctx = pc._ctx(1)
    dev = _device_net(ctx, unet)
    x, t, y = _dev_inputs(ins)
    # no image yet
    with pytest.raises(L.CgdError, match="set_low_res"):
        dev.forward(x, t, y)
    # set A, forward; set B (batch 1, shared), forward: the second result is a fresh handle's with B, bit for bit
    dev.set_low_res(ins["low_a"].to(DEV))
    o_a = dev.forward(x, t, y).clone()
    dev.set_low_res(ins["low_b"].to(DEV))
    o_b = dev.forward(x, t, y).clone()
    fresh = _device_net(ctx, unet)
    fresh.set_low_res(ins["low_b"].to(DEV))
    o_f = fresh.forward(x, t, y)
    th.cuda.synchronize()
    assert th.equal(o_b, o_f) and not th.equal(o_a, o_b)
    _assert_all([rec("sr unet: forward after set A", o_a, refs["low_a"][0]), rec("sr unet: forward after set B", o_b, refs["low_b"][0])])
    # the caller's tensor need not outlive the call: overwrite it, the handle's copy conditions the next forward
    tmp = ins["low_b"].to(DEV).clone()
    dev.set_low_res(tmp)
    tmp.fill_(9.0)
    o_b2 = dev.forward(x, t, y)
    th.cuda.synchronize()
    assert th.equal(o_b2, o_b)
    # dgrad after forward_slot
    dev.embed(t, y, 1)
    o_s = dev.forward_slot(x, 1)
    o_ref, g_ref = refs["low_b"]
    seed = pc.unit_seed(g_ref)
    gx = dev.dgrad((gout * seed).to(DEV))
    th.cuda.synchronize()
    assert th.equal(o_s, o_b)
    _assert_all([rec("sr unet: dgrad after forward_slot", gx, g_ref * seed)])
    # another frame size, same low-res image (batch 1): 16x16 from the 8x10 image
    xs = th.randn(1, 3, 16, 16, generator=g(65))
    ref = SuperResModel(unet)(xs, ins["t"][:1], ins["y"][:1], low_res=ins["low_b"])
    o_small = dev.forward(xs.to(DEV), t[:1], y[:1])
    th.cuda.synchronize()
    _assert_all([rec("sr unet: forward at 16x16 with the same low-res image", o_small, ref)])
    # a low-res batch that is neither 1 nor B
    dev.set_low_res(th.zeros(3, 3, *LOW))
    with pytest.raises(L.CgdError, match="must be 1 or equal"):
        dev.forward(x, t, y)
    with pytest.raises(L.CgdError, match="must be 1 or equal"):
        dev.embed(t, y, 0) or dev.forward_slot(x, 0)
    with pytest.raises(ValueError):
        dev.set_low_res(th.zeros(2, 4, *LOW))
    # a 3-channel handle refuses the image
    from cgd_amd import nets
    plain = nets.UNet(ctx, **dict(SR_CASE, in_channels=3))
    with pytest.raises(L.CgdError, match="in_channels 6"):
        plain.set_low_res(ins["low_b"])


# ---- one guided step ------------------------------------------------------------------------------------------------------------------
class SuperResScenario(sc.Scenario):
    """tests/step_checks.py's scenario on the 6-channel case: the oracle model is the SuperResModel wrapper (holding low_res, since the
    oracle loop builds its own model_kwargs); the device loops get model_kwargs = {"y", "low_res"}."""

    def __init__(self, **kw):
        pc.UNET_CASES.setdefault("sr_mini", SR_CASE)
        super().__init__("sr_mini", hw=FRAME, **kw)
        self.low = th.rand(1, 3, *LOW, generator=g(66)) * 2 - 1
        self.ref_unet = SuperResModel(self.ref_unet, self.low).eval()
        self.set_calls = 0

    def _make_device(self, precision):
        ctx, unet, clip, clip2, lp, smp = super()._make_device(precision)
        low = self.low.to(DEV)
        plain_set = unet.set_low_res

        def counting_set(t):
            self.set_calls += 1
            return plain_set(t)

        unet.set_low_res = counting_set
        for name in ("p_sample_loop_progressive", "ddim_sample_loop_progressive"):
            plain = getattr(smp, name)
            setattr(smp, name, lambda *a, _plain=plain, model_kwargs=None, **k: _plain(*a, model_kwargs=dict(model_kwargs or {}, low_res=low), **k))
        return ctx, unet, clip, clip2, lp, smp


@pytest.mark.parametrize("ddim", [False, True])
def test_one_guided_step_with_low_res(ddim):
    scen = SuperResScenario(ddim=ddim, steps=1)
    recs = sc.compare(scen, 1, scen.run_oracle(), scen.run_device(1))
    _assert_all(recs)
    assert scen.set_calls == 1
