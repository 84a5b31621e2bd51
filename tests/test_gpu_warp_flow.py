"""GPU tests of the flow-guided warp of csrc/flow.hip through cgd_amd.ops.frame_warp_flow: against the float64 restatement
(tests/flow_ref.py: warp_flow) on every pixel over interp x border, on the shapes of tests/test_gpu_warp3d.py; zero flow copies bits; a
constant integer flow is ops.frame_warp of that shift, bit for bit; blend 0, 0.5 and 1; the consistency mask equals the restatement's
exactly, on flow pairs built so that no pixel's test value lies within 1e-3 of its threshold (asserted); mask_out; the clamp; the refusals.
Tolerance: parity_checks.rec (|a - b| <= 1e-4 + 1e-3 |ref|).  Every case runs on plain allocations and once more on pointers offset by
one float."""
import pytest
import torch as th

from tests import flow_ref as F
from tests import parity_checks as pc
from tests import warp_ref as R
from tests.test_gpu_masked import _dev
from tests.test_gpu_warp3d import OFFSETS, SHAPES, _assert_all, _src

pytestmark = pytest.mark.gpu

DEV = pc.DEV


@pytest.fixture(scope="module")
def rig():
    from cgd_amd import lib, ops
    return lib.Context(0, 1), ops


def _flows(shape, per_sample):
    """name -> (1 or B, 2, H, W) fp32: a smooth field of a few pixels, and a wide one (up to 2.6 frame widths: several periods of wrap and
    reflect); no y motion on a frame of height 1"""
    B, _, H, W = shape
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float32), th.arange(W, dtype=th.float32), indexing="ij")
    vy = 0.0 if H == 1 else 1.0
    out = {"smooth": [], "wide": []}
    for b in range(B if per_sample else 1):
        out["smooth"].append(th.stack([2.3 * th.sin(0.31 * xs + 0.7 * b) * th.cos(0.17 * ys) + 0.4, vy * (1.9 * th.cos(0.23 * xs - 0.5 * b) + 0.3 * th.sin(0.4 * ys))]))
        out["wide"].append(th.stack([2.6 * W * th.sin(0.11 * xs + 0.05 * ys + b), vy * 1.7 * H * th.cos(0.07 * xs - 0.13 * ys)]))
    return {k: th.stack(v) for k, v in out.items()}


def _fallback(shape):
    th.manual_seed(1 + sum(shape))
    return th.randn(shape) * 0.5


def _warp(rig, src, flow, back=None, fallback=None, want_mask=False, offset=False, **kw):
    ctx, ops = rig
    d_src, d_flow, d_back, d_fb = (_dev(t, offset) for t in (src, flow, back, fallback))
    d_out = _dev(th.full(src.shape, float("nan")), offset)
    d_mask = _dev(th.full((src.shape[0], 1) + tuple(src.shape[2:]), float("nan")), offset) if want_mask else None
    ops.frame_warp_flow(ctx, d_src, d_flow, flow_back=d_back, fallback=d_fb, out=d_out, mask_out=d_mask, **kw)
    th.cuda.synchronize()
    for dev, host in ((d_src, src), (d_flow, flow), (d_back, back), (d_fb, fallback)):  # the inputs are only read
        assert host is None or th.equal(dev.cpu().view(th.int32), host.view(th.int32))
    return (d_out.cpu(), d_mask.cpu()) if want_mask else d_out.cpu()


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_flow_copies_the_bits(rig, shape):
    src = _src(shape)
    for fbatch in {1, shape[0]}:
        zero = th.zeros(fbatch, 2, *shape[2:])
        for offset in OFFSETS:
            for interp in R.INTERPS:
                for border in R.BORDERS:
                    got = _warp(rig, src, zero, interp=interp, border=border, offset=offset)
                    assert th.equal(got.view(th.int32), src.view(th.int32)), (interp, border, offset)
        got = _warp(rig, src, zero, back=zero, fallback=_fallback(shape), blend=1.0)  # consistent everywhere: w = 1
        assert th.equal(got.view(th.int32), src.view(th.int32))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("interp", R.INTERPS)
@pytest.mark.parametrize("border", R.BORDERS)
def test_warp_matches_fp64_on_every_pixel(rig, shape, interp, border):
    src, fb = _src(shape), _fallback(shape)
    recs = []
    for per_sample in (False, True):
        for fname, flow in _flows(shape, per_sample).items():
            for blend, fallback in ((1.0, None), (0.5, fb)):
                want, _, _ = F.warp_flow(src, flow, None, fallback, blend=blend, interp=interp, border=border)  # once, for both offsets
                for offset in OFFSETS:
                    got = _warp(rig, src, flow, fallback=fallback, blend=blend, interp=interp, border=border, offset=offset)
                    recs.append(pc.rec(f"{fname}, per sample {per_sample}, blend {blend} (offset {int(offset)})", got, want))
    _assert_all(recs)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_constant_integer_flow_is_frame_warp_of_that_shift(rig, shape):
    ctx, ops = rig
    src = _src(shape)
    H, W = shape[2:]
    for fx, fy in ((3, 0 if H == 1 else -2), (-W - 1, 0), (0, 0 if H == 1 else 2 * H + 1)):
        flow = th.stack([th.full((H, W), float(fx)), th.full((H, W), float(fy))])[None]
        for interp in R.INTERPS:
            for border in R.BORDERS:
                want = ops.frame_warp(ctx, src.to(DEV), (1, 0, fx, 0, 1, fy), interp=interp, border=border).cpu()
                for offset in OFFSETS:
                    got = _warp(rig, src, flow, interp=interp, border=border, offset=offset)
                    assert th.equal(got.view(th.int32), want.view(th.int32)), (fx, fy, interp, border, offset)


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_blend_0_half_and_1(rig, shape):
    src, fb = _src(shape), _fallback(shape)
    flow = _flows(shape, True)["smooth"]
    free = _warp(rig, src, flow)
    for offset in OFFSETS:
        assert th.equal(_warp(rig, src, flow, fallback=fb, blend=0.0, offset=offset).view(th.int32), fb.view(th.int32))  # the fallback's bits
        assert th.equal(_warp(rig, src, flow, fallback=fb, blend=1.0, offset=offset).view(th.int32), free.view(th.int32))  # the sample's bits
    half = _warp(rig, src, flow, fallback=fb, blend=0.5)
    _assert_all([pc.rec("blend 0.5", half, F.warp_flow(src, flow, None, fb, blend=0.5)[0]),
                 pc.rec("blend 0.5 is the mean", half, 0.5 * free.double() + 0.5 * fb.double())])


def _pairs(shape):
    """name -> (flow, flow_back, share of m = 1 expected at least, at most): a consistent pair, one with an occluding patch in the backward
    flow, one whose flow leaves the frame on most pixels; constant flows with fractions of 1 / 4, so that every position and every
    interpolated backward flow is exact"""
    B, _, H, W = shape
    vy = 0.0 if H == 1 else 1.0
    fx, fy = 2.5, -1.25 * vy

    def const(x, y, n=B):
        return th.stack([th.full((H, W), float(x)), th.full((H, W), float(y))])[None].repeat(n, 1, 1, 1)

    back = const(-fx, -fy)
    patched = back.clone()
    patched[:, 0, H // 4:max(H // 4 + 1, H // 2), W // 3:2 * W // 3] += 4.0
    nan = const(fx, fy)
    nan[0, 0, 0, 1] = float("nan")
    nan[-1, 1, -1, 2] = float("inf")
    return {"consistent": (const(fx, fy), back, 0.5, 1.0), "occluding patch": (const(fx, fy), patched, 0.1, 0.95),
            "leaves the frame": (const(0.75 * W, 0.0), const(-0.75 * W, 0.0), 0.1, 0.3), "one flow for the batch": (const(fx, fy, 1), patched[:1], 0.1, 0.95),
            "non-finite flow": (nan, back, 0.4, 1.0)}


@pytest.mark.parametrize("shape", SHAPES)
def test_consistency_mask_is_the_restatements_exactly(rig, shape):
    src, fb = _src(shape), _fallback(shape)
    recs = []
    for name, (flow, back, lo, hi) in _pairs(shape).items():
        want, m, margin = F.warp_flow(src, flow, back, fb, blend=0.75, interp="bilinear", border="reflect")
        assert margin >= 1e-3, (name, margin)  # no pixel's test value near its threshold
        assert lo <= float(m.mean()) <= hi, (name, float(m.mean()))
        for offset in OFFSETS:
            got, mask = _warp(rig, src, flow, back, fb, want_mask=True, blend=0.75, interp="bilinear", border="reflect", offset=offset)
            assert th.equal(mask.double(), m), (name, offset, int((mask.double() != m).sum()))
            assert th.equal(got[(m == 0).expand_as(got)].view(th.int32), fb[(m == 0).expand_as(fb)].view(th.int32))  # untrusted: the fallback's bits
            recs.append(pc.rec(f"{name} (offset {int(offset)})", got, want))
    _assert_all(recs)


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_mask_out_without_flow_back_and_looser_checks(rig, shape):
    src, fb = _src(shape), _fallback(shape)
    flow, patched, _, _ = _pairs(shape)["occluding patch"]
    _, mask = _warp(rig, src, flow, fallback=fb, want_mask=True)
    assert bool((mask == 1).all())  # m = 1 without flow_back
    nan = _pairs(shape)["non-finite flow"][0]
    got, mask = _warp(rig, src, nan, want_mask=True, interp="bilinear")
    assert float(mask.sum()) == mask.numel() - 2 and mask[0, 0, 0, 1] == 0 and mask[-1, 0, -1, 2] == 0
    assert got[0, 0, 0, 1] == src[0, 0, 0, 1] and bool(th.isfinite(got).all())  # no fallback: a non-finite flow reads as zero flow
    for alpha, beta in ((0.01, 0.5), (0.0, 0.0), (0.0, 17.0), (4.0, 0.5)):  # beta 17 accepts the patch's 4 px, alpha 4 everything
        _, m, margin = F.warp_flow(src, flow, patched, fb, alpha=alpha, beta=beta)
        # (0, 0) has no margin by construction: lhs <= 0 only where F + Fb cancels.  It is kept because the comparison is exact on both sides:
        # every flow value and every bilinear weight of Fb is a multiple of 1 / 4, so F + Fb and its square are exact in fp64, and the
        # kernel runs this check in fp64 with contraction off, as the restatement does
        assert margin >= 1e-3 or (alpha, beta) == (0.0, 0.0)
        _, mask = _warp(rig, src, flow, patched, fb, want_mask=True, alpha=alpha, beta=beta)
        assert th.equal(mask.double(), m), (alpha, beta)
        if (alpha, beta) == (0.0, 0.0):  # lhs <= 0 only where the pair cancels, which it does exactly (quarters) outside the patch
            assert 0 < float(m.mean()) < 1


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_clamp_is_the_clamp_of_the_sample_and_runs_repeat(rig, shape):
    src, fb = _src(shape) * 1.5, _fallback(shape) * 4
    flow = _flows(shape, True)["smooth"]
    for interp in R.INTERPS:
        for border in R.BORDERS:
            free = _warp(rig, src, flow, interp=interp, border=border)
            again = _warp(rig, src, flow, interp=interp, border=border, offset=True)
            assert th.equal(free.view(th.int32), again.view(th.int32)) and float(free.abs().max()) > 1
            assert th.equal(_warp(rig, src, flow, interp=interp, border=border, clamp=True), free.clamp(-1, 1))
            got = _warp(rig, src, flow, fallback=fb, blend=0.5, interp=interp, border=border, clamp=True)  # the fallback is not clamped
            _assert_all([pc.rec(f"clamp with fallback {interp} {border}", got, F.warp_flow(src, flow, None, fb, 0.5, interp=interp, border=border, clamp=True)[0])])
            assert float(got.abs().max()) > 1


def test_wrapper_refuses_what_the_abi_cannot_express(rig):
    ctx, ops = rig
    x = th.zeros(2, 3, 8, 8, device=DEV)
    f = th.zeros(2, 2, 8, 8, device=DEV)
    fb = th.zeros(2, 3, 8, 8, device=DEV)
    m = th.zeros(2, 1, 8, 8, device=DEV)
    assert tuple(ops.frame_warp_flow(ctx, x, f, flow_back=f.clone(), fallback=fb, blend=0.5, mask_out=m).shape) == (2, 3, 8, 8)
    assert tuple(ops.frame_warp_flow(ctx, x, f[:1]).shape) == (2, 3, 8, 8)
    for kw in (dict(interp="nearest"), dict(border="zeros"), dict(flow_back=f[:1]), dict(flow_back=f.double()), dict(fallback=fb[:1]),
               dict(fallback=fb.cpu()), dict(mask_out=m[:1]), dict(mask_out=th.zeros(2, 3, 8, 8, device=DEV)), dict(out=th.zeros(2, 3, 8, 4, device=DEV)),
               dict(out=x.cpu()), dict(out=x.double())):
        with pytest.raises(ValueError):
            ops.frame_warp_flow(ctx, x, f, **kw)
    for bad in (f.cpu(), f.double(), f[:, :1], f[0], th.zeros(3, 2, 8, 8, device=DEV), f.transpose(2, 3), th.zeros(2, 2, 8, 4, device=DEV)):
        with pytest.raises(ValueError):
            ops.frame_warp_flow(ctx, x, bad)
    for bad in (x.cpu(), x.double(), x[0], x.transpose(2, 3)):
        with pytest.raises(ValueError):
            ops.frame_warp_flow(ctx, bad, f)
    with pytest.raises(RuntimeError, match="dst must not alias"):
        ops.frame_warp_flow(ctx, x, f, out=x)
    with pytest.raises(RuntimeError, match="dst must not alias"):
        ops.frame_warp_flow(ctx, x, f, fallback=fb, out=fb)
    with pytest.raises(RuntimeError, match="mask_out must not alias"):
        ops.frame_warp_flow(ctx, x, f, mask_out=f.view(-1)[:128].view(2, 1, 8, 8))
    with pytest.raises(RuntimeError, match="fallback is required"):
        ops.frame_warp_flow(ctx, x, f, blend=0.5)
    with pytest.raises(RuntimeError, match="fallback is required"):
        ops.frame_warp_flow(ctx, x, f, flow_back=f.clone())
    for kw, why in ((dict(blend=1.5), "blend"), (dict(blend=-0.1), "blend"), (dict(alpha=-1.0), "alpha"), (dict(beta=float("nan")), "beta")):
        with pytest.raises(RuntimeError, match=why):
            ops.frame_warp_flow(ctx, x, f, fallback=fb, **kw)
