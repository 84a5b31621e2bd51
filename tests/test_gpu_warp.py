"""GPU tests of csrc/warp.hip through cgd_amd.ops: cgd_frame_warp against the float64 restatement (tests/warp_ref.py) and its exactness rules
(the identity and integer wrap shifts copy bits), cgd_channel_stats / cgd_color_match against theirs.  Tolerance: parity_checks.rec
(|a - b| <= 1e-4 + 1e-3 |ref|); an emulation of fp32 weights on fp64 coordinates stays within 5e-6 of the restatement at peak 3.5.  Every
case runs on plain allocations and once more on pointers offset by one float."""
import pytest
import torch as th

from tests import parity_checks as pc
from tests import warp_ref as R
from tests.test_gpu_masked import _dev

pytestmark = pytest.mark.gpu

DEV = pc.DEV
SHAPES = [(2, 3, 24, 40), (1, 3, 17, 33), (1, 1, 1, 9), (1, 3, 64, 64)]
OFFSETS = [False, True]


@pytest.fixture(scope="module")
def rig():
    from cgd_amd import animate, lib, ops
    return lib.Context(0, 1), ops, animate


def _src(shape):
    th.manual_seed(sum(shape))
    return th.randn(shape)


def _warp(rig, src, m, interp, border, clamp=False, offset=False):
    ctx, ops, _ = rig
    d_src, d_out = _dev(src, offset), _dev(th.full(src.shape, float("nan")), offset)
    ops.frame_warp(ctx, d_src, m, interp=interp, border=border, clamp=clamp, out=d_out)
    th.cuda.synchronize()
    assert th.equal(d_src.cpu(), src)  # the source is only read
    return d_out.cpu()


def _assert_all(recs):
    for r in recs:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3e}")
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


def _motions(animate, H, W):
    """zoom 0.5 / 1.3 / 2, angles 17 and 180 degrees, shifts of +-(3 W + 0.25, 2 H - 0.5): several periods of wrap and reflect, negative
    coordinates"""
    sx, sy = 3 * W + 0.25, 2 * H - 0.5
    return {"zoom 0.5, 17 deg, +shift": animate.motion_matrix(0.5, 17.0, sx, sy, H, W),
            "zoom 1.3, 180 deg, -shift": animate.motion_matrix(1.3, 180.0, -sx, -sy, H, W),
            "zoom 2, 17 deg, -shift": animate.motion_matrix(2.0, 17.0, -sx, -sy, H, W),
            "zoom 1.3, 17 deg": animate.motion_matrix(1.3, 17.0, 0.0, 0.0, H, W),
            "180 deg": animate.motion_matrix(1.0, 180.0, 0.0, 0.0, H, W),
            "+shift": animate.motion_matrix(1.0, 0.0, sx, sy, H, W),
            "-shift": animate.motion_matrix(1.0, 0.0, -sx, -sy, H, W)}


# ---- the warp ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_identity_copies_the_bits(rig, shape):
    src = _src(shape)
    for offset in OFFSETS:
        for interp in R.INTERPS:
            for border in R.BORDERS:
                assert th.equal(_warp(rig, src, (1, 0, 0, 0, 1, 0), interp, border, offset=offset), src), (interp, border, offset)


@pytest.mark.parametrize("shape", SHAPES)
def test_integer_shifts_under_wrap_are_rolls(rig, shape):
    _, _, animate = rig
    src = _src(shape)
    H, W = shape[2:]
    for tx, ty in ((1, 0), (-30, 5), (3 * W + 7, -2 * H - 3)):  # the last: more than three frame widths
        for offset in OFFSETS:
            for interp in R.INTERPS:
                got = _warp(rig, src, animate.motion_matrix(1.0, 0.0, tx, ty, H, W), interp, "wrap", offset=offset)
                assert th.equal(got, th.roll(src, (ty, tx), dims=(2, 3))), (tx, ty, interp, offset)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("interp", R.INTERPS)
@pytest.mark.parametrize("border", R.BORDERS)
def test_warp_matches_fp64(rig, shape, interp, border):
    _, _, animate = rig
    src = _src(shape)
    recs = []
    for name, m in _motions(animate, *shape[2:]).items():
        want = R.warp_fp64(src, m, interp, border)  # once, for both pointer offsets
        for offset in OFFSETS:
            recs.append(pc.rec(f"{name} (offset {int(offset)})", _warp(rig, src, m, interp, border, offset=offset), want))
    _assert_all(recs)


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_clamp_is_the_clamp_of_the_unclamped_result_and_runs_repeat(rig, shape):
    _, _, animate = rig
    src = _src(shape) * 1.5
    m = animate.motion_matrix(1.3, 17.0, 2.25, -1.5, *shape[2:])
    for interp in R.INTERPS:
        for border in R.BORDERS:
            free = _warp(rig, src, m, interp, border)
            again = _warp(rig, src, m, interp, border)
            assert th.equal(free, again) and float(free.abs().max()) > 1
            assert th.equal(_warp(rig, src, m, interp, border, clamp=True), free.clamp(-1, 1))


def test_plane_offsets_are_64_bit(rig):
    """33 planes of 8192 x 8192: the last planes start beyond 2^31 elements.  A wrap shift of every plane against torch.roll of that plane."""
    ctx, ops, animate = rig
    shape = (1, 33, 8192, 8192)
    src = th.empty(shape, device=DEV)
    for p in (0, 31, 32):
        src[0, p].normal_()
    out = ops.frame_warp(ctx, src, animate.motion_matrix(1.0, 0.0, -5.0, 3.0, 8192, 8192), interp="bilinear", border="wrap")
    for p in (0, 31, 32):
        assert th.equal(out[0, p], th.roll(src[0, p], (3, -5), dims=(0, 1))), p
    stats = ops.channel_stats(ctx, src[:, 31:33].contiguous())
    want = th.stack([src[0, 31:33].double().mean(dim=(1, 2)), src[0, 31:33].double().var(dim=(1, 2), unbiased=False).sqrt()], dim=-1)[None]
    _assert_all([pc.rec("stats of a 2^26-pixel plane", stats, want)])


def test_wrapper_refuses_what_the_abi_cannot_express(rig):
    ctx, ops, _ = rig
    x = th.zeros(1, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.frame_warp(ctx, x, (1, 0, 0, 0, 1, 0), interp="nearest")
    with pytest.raises(ValueError):
        ops.frame_warp(ctx, x, (1, 0, 0, 0, 1))
    with pytest.raises(ValueError):
        ops.frame_warp(ctx, x.cpu(), (1, 0, 0, 0, 1, 0))
    with pytest.raises(RuntimeError, match="alias"):
        ops.frame_warp(ctx, x, (1, 0, 0, 0, 1, 0), out=x)
    with pytest.raises(RuntimeError, match="2\\^30"):
        ops.frame_warp(ctx, x, (1, 0, 2.0 ** 31, 0, 1, 0))
    with pytest.raises(RuntimeError, match="amount"):
        ops.color_match(ctx, x, th.zeros(1, 3, 2, device=DEV), amount=1.5)


# ---- colour -----------------------------------------------------------------------------------------------------------------------------
def _colour_case(shape):
    th.manual_seed(7 + sum(shape))
    B, C = shape[:2]
    x = th.randn(shape) * (0.2 + 0.1 * th.arange(1, B * C + 1).view(B, C, 1, 1)) + 0.15 * th.arange(-1, B * C - 1).view(B, C, 1, 1) + 0.07
    ref = th.randn(shape) * 0.5 - 0.1
    return x, ref


@pytest.mark.parametrize("shape", SHAPES)
def test_stats_match_fp64(rig, shape):
    ctx, ops, _ = rig
    x, _ = _colour_case(shape)
    want = R.stats_fp64(x)
    recs = []
    for offset in OFFSETS:
        out = _dev(th.full((shape[0], shape[1], 2), float("nan")), offset)
        ops.channel_stats(ctx, _dev(x, offset), out=out)
        recs.append(pc.rec(f"stats (offset {int(offset)})", out.cpu(), want))
        assert th.equal(out.cpu(), ops.channel_stats(ctx, _dev(x, False)).cpu())  # the same bits wherever the operands lie
    _assert_all(recs)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ref_batch", ["one", "B"])
def test_color_match_matches_fp64(rig, shape, ref_batch):
    ctx, ops, _ = rig
    x, ref = _colour_case(shape)
    if ref_batch == "one":
        ref = ref[:1]
    sx = ops.channel_stats(ctx, x.to(DEV))
    sr = ops.channel_stats(ctx, ref.to(DEV))
    recs = []
    for offset in OFFSETS:
        d_sx, d_sr = _dev(sx.cpu(), offset), _dev(sr.cpu(), offset)
        for amount in (0.0, 0.5, 1.0):
            d_x = _dev(x, offset)
            assert ops.color_match(ctx, d_x, d_sr, amount=amount, stats_x=d_sx) is d_x
            got = d_x.cpu()
            recs.append(pc.rec(f"amount {amount} (offset {int(offset)})", got, R.color_match_fp64(x, sx, sr, amount)))
            if amount == 0.0:
                assert th.equal(got.view(th.int32), x.view(th.int32))  # the bits are left alone
            if amount == 1.0 and shape[2] * shape[3] > 1:  # the output has the reference's statistics
                recs.append(pc.rec(f"stats after amount 1 (offset {int(offset)})", ops.channel_stats(ctx, d_x.contiguous()).cpu(),
                                   sr.cpu().double().expand(shape[0], -1, -1)))
            d_c = _dev(x * 3, offset)
            ops.color_match(ctx, d_c, d_sr, amount=amount, clamp=True, stats_x=d_sx)
            recs.append(pc.rec(f"clamped, amount {amount} (offset {int(offset)})", d_c.cpu(), R.color_match_fp64(x * 3, sx, sr, amount, clamp=True)))
    _assert_all(recs)


def test_a_constant_plane_stays_constant_and_finite(rig):
    ctx, ops, _ = rig
    x = th.full((2, 3, 17, 33), 0.25, device=DEV)
    x[1] = -0.75
    ref = th.randn(1, 3, 17, 33, device=DEV) * 0.5 + 0.3
    sr = ops.channel_stats(ctx, ref)
    sx = ops.channel_stats(ctx, x)
    assert float(sx[..., 1].abs().max()) < 1e-6 and th.equal(sx[..., 0].cpu(), th.tensor([[0.25] * 3, [-0.75] * 3]))
    for amount in (0.5, 1.0):
        out = ops.color_match(ctx, x.clone(), sr, amount=amount, stats_x=sx).cpu()
        assert th.isfinite(out).all()
        assert th.equal(out, out[:, :, :1, :1].expand_as(out))
        want = x.cpu()[:, :, :1, :1].double() + amount * (sr.cpu()[..., 0].double().view(1, 3, 1, 1) - x.cpu()[:, :, :1, :1].double())
        _assert_all([pc.rec(f"flat planes, amount {amount}", out[:, :, :1, :1], want)])
