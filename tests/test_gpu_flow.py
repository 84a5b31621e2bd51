"""GPU tests of the flow estimator of csrc/flow.hip through cgd_amd.ops.flow_level and ops.flow_estimate, against the float64 restatement
(tests/flow_ref.py): one pyramid level with one iteration and with four, started from zero and from a coarser flow, and the whole estimate.
Tolerance: parity_checks.rec's, |a - b| <= 1e-4 + 1e-3 |ref|.  A window sample that sits on the validity boundary (0 <= s <= size - 1) may
fall the other way when the flow before it was summed in fp32, so at most 0.5 % of a case's pixels may lie outside that bound; the largest
miss is printed and none may exceed max_step.  That cap is a condition on the inputs: the float32 restatement of the reference must stay
inside it on every case (asserted in the fixture, on the CPU).  Every case runs on plain allocations and once more on pointers offset by
one float.  Also: identical frames give exactly zero flow, two runs give the same bits, the inputs are only read, and on the 64 x 96 scenes
the device flow meets the accuracy conditions of tests/test_flow_host.py."""
import pytest
import torch as th

from tests import flow_ref as F
from tests import parity_checks as pc
from tests.test_gpu_masked import _dev

pytestmark = pytest.mark.gpu

DEV = pc.DEV
OFFSETS = [False, True]
CAP = 0.005
# name -> (B, C, H, W), radius, levels, one motion per sample, texture seed
CASES = {
    "24x40": ((1, 3, 24, 40), 3, 3, [(1.3, -0.8)], 2),
    "33x47": ((2, 3, 33, 47), 4, 4, [(1.6, 0.9), (-0.7, 1.2, 2.0, 0.98)], 4),
    "17x33": ((1, 1, 17, 33), 4, 4, [(-0.9, 0.6)], 5),
    "1x16": ((1, 1, 1, 16), 4, 4, [(0.6, 0.0)], 6),
    "64x96 shift": ((1, 3, 64, 96), 4, 4, [(2.3, -1.7)], 1),
    "64x96 rotation": ((1, 3, 64, 96), 4, 4, [(0.8, -0.5, 3.0, 1.03)], 1),
}
ACCURACY = {"64x96 shift": 0.98, "64x96 rotation": 0.90}


def _outside(got, ref):
    """share of the pixels with a flow component outside the tolerance, and the largest difference"""
    diff = (got.double().cpu() - ref.double()).abs()
    return float((diff > pc.ATOL + pc.RTOL * ref.double().abs()).any(dim=1).double().mean()), float(diff.max())


@pytest.fixture(scope="module")
def cases():
    """per case: the frames, the analytic flow, the float64 reference of the estimate and of its levels; made once, only read"""
    out = {}
    for name, (shape, radius, levels, motions, seed) in CASES.items():
        B, Cn, H, W = shape
        parts = [F.scene(H, W, m, seed + 3 * b, channels=Cn) for b, m in enumerate(motions)]
        tmpl, img, want = (th.cat([p[i] for p in parts]) for i in range(3))
        assert tuple(tmpl.shape) == shape
        kw = dict(levels_=levels, radius=radius)
        ref = F.estimate(tmpl, img, **kw)
        share, worst = _outside(F.estimate(tmpl, img, dtype=th.float32, **kw), ref)
        assert share <= CAP and worst <= 1.0, (name, share, worst)  # the condition on the inputs
        L = F.levels(H, W, levels, radius)
        pyr = [p.float() for p in F.pyramid(th.cat([F.luminance(tmpl), F.luminance(img)]), L)]
        out[name] = dict(tmpl=tmpl, img=img, want=want, ref=ref, L=L, pyr=pyr, radius=radius, levels=levels, B=B)
    return out


@pytest.fixture(scope="module")
def rig():
    from cgd_amd import lib, ops
    return lib.Context(0, 1), ops


def _estimate(rig, c, offset=False, tmpl=None, img=None):
    ctx, ops = rig
    tmpl, img = c["tmpl"] if tmpl is None else tmpl, c["img"] if img is None else img
    d_t, d_i = _dev(tmpl, offset), _dev(img, offset)
    d_out = _dev(th.full((tmpl.shape[0], 2) + tuple(tmpl.shape[2:]), float("nan")), offset)
    ops.flow_estimate(ctx, d_t, d_i, levels=c["levels"], radius=c["radius"], out=d_out)
    th.cuda.synchronize()
    assert th.equal(d_t.cpu(), tmpl) and th.equal(d_i.cpu(), img)  # the frames are only read
    return d_out.cpu()


def _check(name, got, ref, max_step=1.0):
    share, worst = _outside(got, ref)
    print(f"{name}: {100 * share:.3f} % of the pixels outside 1e-4 + 1e-3 |ref|, largest difference {worst:.3e}")
    assert bool(th.isfinite(got).all()) and share <= CAP and worst <= max_step, (name, share, worst)


@pytest.mark.parametrize("name", list(CASES))
def test_estimate_matches_the_reference(rig, cases, name):
    c = cases[name]
    assert rig[0].lib.cgd_flow_levels(*c["tmpl"].shape[2:], c["levels"], c["radius"]) == c["L"]
    for offset in OFFSETS:
        got = _estimate(rig, c, offset)
        _check(f"{name} (offset {int(offset)})", got, c["ref"])
        if name == "1x16":
            assert c["L"] == 1 and bool((got[:, 1] == 0).all())  # one row: no y difference, dv stays 0


@pytest.mark.parametrize("name", ["24x40", "33x47", "17x33", "1x16"])
@pytest.mark.parametrize("iters", [1, 4])
def test_one_level_matches_the_reference(rig, cases, name, iters):
    ctx, ops = rig
    c = cases[name]
    B, pyr, radius = c["B"], c["pyr"], c["radius"]
    runs = [(0 if c["L"] == 1 else 1, None)]  # the coarsest start: from zero (on level 1 where there is one: smaller motion)
    if c["L"] > 1:
        coarse = F.level(pyr[1][:B], pyr[1][B:], None, 4, radius)
        runs.append((0, coarse))
    for lvl, coarse in runs:
        b, a = pyr[lvl][:B].contiguous(), pyr[lvl][B:].contiguous()
        ref = F.level(b, a, coarse, iters, radius)
        for offset in OFFSETS:
            d_b, d_a, d_c = _dev(b, offset), _dev(a, offset), _dev(coarse, offset)
            d_out = _dev(th.full(ref.shape, float("nan")), offset)
            ops.flow_level(ctx, d_b, d_a, coarse=d_c, iters=iters, radius=radius, out=d_out)
            th.cuda.synchronize()
            assert th.equal(d_b.cpu(), b) and th.equal(d_a.cpu(), a) and (coarse is None or th.equal(d_c.cpu(), coarse))
            _check(f"{name} level {lvl}, {iters} iterations, coarse {coarse is not None} (offset {int(offset)})", d_out.cpu(), ref)
            if iters == 1 and coarse is None:  # one step is no longer than max_step
                assert float(d_out.cpu().pow(2).sum(dim=1).sqrt().max()) <= 1.0 + 1e-6


@pytest.mark.parametrize("name", ["24x40", "33x47", "1x16", "64x96 shift"])
def test_identical_frames_give_exactly_zero_flow_and_runs_repeat(rig, cases, name):
    c = cases[name]
    for offset in OFFSETS:
        zero = _estimate(rig, c, offset, img=c["tmpl"].clone())
        assert bool((zero == 0).all()), name
    first, again = _estimate(rig, c), _estimate(rig, c, offset=True)
    assert th.equal(first.view(th.int32), again.view(th.int32))
    assert th.equal(first.view(th.int32), _estimate(rig, c).view(th.int32))


@pytest.mark.parametrize("name", list(ACCURACY))
def test_device_flow_meets_the_accuracy_conditions(rig, cases, name):
    c = cases[name]
    share, worst = F.share_within(_estimate(rig, c), c["want"])
    print(f"{name}: {100 * share:.2f} % within 0.25 px of the analytic flow, max error {worst:.3f} px")
    assert share >= ACCURACY[name]


def test_wrapper_refuses_what_the_abi_cannot_express(rig):
    ctx, ops = rig
    x, y = th.zeros(1, 3, 16, 24, device=DEV), th.zeros(1, 3, 16, 24, device=DEV)
    assert tuple(ops.flow_estimate(ctx, x, y).shape) == (1, 2, 16, 24)
    for kw in (dict(levels=1.5), dict(iters=True), dict(out=th.zeros(1, 2, 16, 16, device=DEV)), dict(out=th.zeros(1, 2, 16, 24))):
        with pytest.raises(ValueError):
            ops.flow_estimate(ctx, x, y, **kw)
    for bad in (y.cpu(), y.double(), y[:, :, :8], y[0], y.transpose(2, 3)):
        with pytest.raises(ValueError):
            ops.flow_estimate(ctx, x, bad)
    with pytest.raises(RuntimeError, match="C must be 1 or 3"):
        ops.flow_estimate(ctx, x[:, :2].contiguous(), y[:, :2].contiguous())
    for kw, why in ((dict(radius=8), "radius"), (dict(iters=17), "iters"), (dict(levels=9), "levels"), (dict(lam=0.0), "lambda"),
                    (dict(max_step=float("inf")), "max_step")):
        with pytest.raises(RuntimeError, match=why):
            ops.flow_estimate(ctx, x, y, **kw)
    with pytest.raises(RuntimeError, match="alias"):
        ops.flow_estimate(ctx, x, y, out=x[:, :2])
