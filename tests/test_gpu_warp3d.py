"""GPU tests of csrc/warp3d.hip through cgd_amd.ops.frame_warp3d: against the float64 restatement (tests/warp3d_ref.py) on every pixel, the
identity camera's bit copy, agreement with the 2D kernel where a flat depth makes the camera an affine map, the clamp, repeatability, and the
wrapper's refusals.  Tolerance: parity_checks.rec (|a - b| <= 1e-4 + 1e-3 |ref|).  Every case runs on plain allocations and once more on
pointers offset by one float.  The frames of height 1 get a narrow field of view, so that a 30 degree yaw keeps every ray in front of the
camera (f = (H / 2) / tan(fov / 2) is 1.4 pixels at H = 1 and fov 40)."""
import math

import pytest
import torch as th

from tests import parity_checks as pc
from tests import warp3d_ref as R3
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


def _depth(shape, per_sample):
    """smooth, in [0.6, 1.6]; (1 or B, 1, H, W)"""
    B, _, H, W = shape
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float32), th.arange(W, dtype=th.float32), indexing="ij")
    maps = [1.1 + 0.5 * th.sin(0.37 * xs + 0.9 * b) * th.cos(0.23 * ys - 0.4 * b) for b in range(B if per_sample else 1)]
    d = th.stack(maps)[:, None]
    assert float(d.min()) >= 0.6 and float(d.max()) <= 1.6
    return d


def _fov(shape):
    return 5.0 if shape[2] == 1 else 40.0


def _cameras(animate, shape):
    """a few degrees about every axis with all three translations; a 30 degree yaw; a translation_x of 3.3 frame widths at depth 1 (2 to
    5.5 widths over the depth map: several periods of wrap and reflect)"""
    H, W = shape[2:]
    fov = _fov(shape)
    f = (H / 2.0) / math.tan(math.radians(fov) / 2.0)
    return {"mixed": animate.camera(3.0, -2.0, 10.0, 1.0, 2.0, 3.0, fov, H, W),
            "yaw 30": animate.camera(0.0, 0.0, 0.0, 0.0, 30.0, 0.0, fov, H, W),
            "wide tx": animate.camera(3.3 * W * 200.0 / f, 0.5, 0.0, 0.0, 0.0, 0.0, fov, H, W)}


def _warp(rig, src, cam, depth=None, iters=1, interp="bicubic", border="wrap", clamp=False, offset=False):
    ctx, ops, _ = rig
    d_src, d_depth, d_out = _dev(src, offset), _dev(depth, offset), _dev(th.full(src.shape, float("nan")), offset)
    ops.frame_warp3d(ctx, d_src, cam, depth=d_depth, interp=interp, border=border, clamp=clamp, iters=iters, out=d_out)
    th.cuda.synchronize()
    assert th.equal(d_src.cpu(), src) and (depth is None or th.equal(d_depth.cpu(), depth))  # the source and the depth are only read
    return d_out.cpu()


def _assert_all(recs):
    for r in recs:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3e}")
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


def _depth_cases(shape):
    """(name, depth, iters): flat, one map for the batch and one per sample, resolved in 1 and 3 steps"""
    one, per = _depth(shape, False), _depth(shape, True)
    return [("flat", None, 1), ("map 1, 1 step", one, 1), ("map 1, 3 steps", one, 3), ("map B, 1 step", per, 1), ("map B, 3 steps", per, 3)]


@pytest.mark.parametrize("shape", SHAPES)
def test_identity_camera_copies_the_bits(rig, shape):
    _, _, animate = rig
    src = _src(shape)
    cam = animate.camera(0, 0, 0, 0, 0, 0, 40, *shape[2:])
    for depth in (None, _depth(shape, False), _depth(shape, True)):
        for offset in OFFSETS:
            for interp in R.INTERPS:
                for border in R.BORDERS:
                    got = _warp(rig, src, cam, depth, 3, interp, border, offset=offset)
                    assert th.equal(got.view(th.int32), src.view(th.int32)), (interp, border, offset, depth is None)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("interp", R.INTERPS)
@pytest.mark.parametrize("border", R.BORDERS)
def test_warp3d_matches_fp64_on_every_pixel(rig, shape, interp, border):
    _, _, animate = rig
    src = _src(shape)
    recs = []
    for cname, cam in _cameras(animate, shape).items():
        for dname, depth, iters in _depth_cases(shape):
            want, clamped = R3.warp3d_fp64(src, cam, depth, iters, interp, border)  # once, for both pointer offsets
            assert clamped == 0, (cname, dname, clamped)  # every ray in front of the camera, every source point beyond the near plane
            for offset in OFFSETS:
                recs.append(pc.rec(f"{cname}, {dname} (offset {int(offset)})", _warp(rig, src, cam, depth, iters, interp, border, offset=offset), want))
    _assert_all(recs)


@pytest.mark.parametrize("shape", SHAPES)
def test_flying_past_the_scene_clamps_as_the_restatement_does(rig, shape):
    """translation_z / 200 = 2 lies beyond every depth (<= 1.6): lambda meets the near plane on every pixel; a ray that a 100 degree yaw puts
    behind the camera meets the a_z clamp."""
    _, _, animate = rig
    src = _src(shape)
    H, W = shape[2:]
    recs = []
    for cname, cam in (("past", animate.camera(1.0, -1.0, 400.0, 1.0, 2.0, 3.0, _fov(shape), H, W)),
                       ("behind", animate.camera(0.0, 0.0, 0.0, 0.0, 100.0, 0.0, _fov(shape), H, W))):
        for dname, depth, iters in _depth_cases(shape)[:3]:
            for interp in R.INTERPS:
                for border in R.BORDERS:
                    want, clamped = R3.warp3d_fp64(src, cam, depth, iters, interp, border)
                    assert clamped == H * W if cname == "past" else 0 < clamped < H * W, (cname, dname, clamped)
                    recs.append(pc.rec(f"{cname}, {dname}, {interp}, {border}", _warp(rig, src, cam, depth, iters, interp, border), want))
    _assert_all(recs)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("interp", R.INTERPS)
def test_flat_in_plane_cameras_agree_with_the_2d_kernel(rig, shape, interp):
    ctx, ops, animate = rig
    src = _src(shape)
    H, W = shape[2:]
    fov = _fov(shape)
    f = (H / 2.0) / math.tan(math.radians(fov) / 2.0)
    cases = []
    for z0 in (1.0, 2.5):
        cases += [(f"rz 17, z0 {z0}", animate.camera(0, 0, 0, 0, 0, 17.0, fov, H, W, z0=z0), animate.motion_matrix(1.0, 17.0, 0.0, 0.0, H, W)),
                  (f"tz 40, z0 {z0}", animate.camera(0, 0, 40.0, 0, 0, 0, fov, H, W, z0=z0), animate.motion_matrix(z0 / (z0 - 0.2), 0.0, 0.0, 0.0, H, W)),
                  (f"tx 30, z0 {z0}", animate.camera(30.0, 0, 0, 0, 0, 0, fov, H, W, z0=z0), animate.motion_matrix(1.0, 0.0, f * 0.15 / z0, 0.0, H, W))]
    recs = []
    for name, cam, matrix in cases:
        for border in R.BORDERS:
            want = ops.frame_warp(ctx, src.to(DEV), matrix, interp=interp, border=border).cpu()
            for offset in OFFSETS:
                recs.append(pc.rec(f"{name}, {border} (offset {int(offset)})", _warp(rig, src, cam, None, 1, interp, border, offset=offset), want))
    _assert_all(recs)


@pytest.mark.parametrize("shape", SHAPES[:2])
def test_clamp_is_the_clamp_of_the_unclamped_result_and_runs_repeat(rig, shape):
    _, _, animate = rig
    src = _src(shape) * 1.5
    cam = _cameras(animate, shape)["mixed"]
    for depth, iters in ((None, 1), (_depth(shape, True), 3)):
        for interp in R.INTERPS:
            for border in R.BORDERS:
                free = _warp(rig, src, cam, depth, iters, interp, border)
                again = _warp(rig, src, cam, depth, iters, interp, border, offset=True)
                assert th.equal(free.view(th.int32), again.view(th.int32)) and float(free.abs().max()) > 1
                assert th.equal(_warp(rig, src, cam, depth, iters, interp, border, clamp=True), free.clamp(-1, 1))


def test_wrapper_refuses_what_the_abi_cannot_express(rig):
    ctx, ops, animate = rig
    x = th.zeros(2, 1, 8, 8, device=DEV)
    d = th.ones(2, 1, 8, 8, device=DEV)
    cam = animate.camera(1, 2, 3, 1, 2, 3, 40, 8, 8)
    assert tuple(ops.frame_warp3d(ctx, x, cam, depth=d, iters=4).shape) == (2, 1, 8, 8)
    for kw in (dict(interp="nearest"), dict(border="zeros"), dict(iters=1.5), dict(iters=True), dict(depth=d[:, :, :4]), dict(depth=d[:, 0]),
               dict(depth=th.ones(3, 1, 8, 8, device=DEV)), dict(depth=th.ones(2, 2, 8, 8, device=DEV)), dict(depth=d.double()), dict(depth=d.cpu()),
               dict(depth=d.transpose(2, 3)), dict(out=th.zeros(2, 1, 8, 4, device=DEV)), dict(out=x.cpu()), dict(out=x.double())):
        with pytest.raises(ValueError):
            ops.frame_warp3d(ctx, x, cam, **kw)
    for bad in (x.cpu(), x.double(), x[0], x.transpose(2, 3)):
        with pytest.raises(ValueError):
            ops.frame_warp3d(ctx, bad, cam)
    with pytest.raises(ValueError):
        ops.frame_warp3d(ctx, x, cam._replace(R=cam.R[:8]))
    with pytest.raises(RuntimeError, match="alias src"):
        ops.frame_warp3d(ctx, x, cam, out=x)
    with pytest.raises(RuntimeError, match="alias depth"):
        ops.frame_warp3d(ctx, x, cam, depth=d, out=d)
    with pytest.raises(RuntimeError, match="iters"):
        ops.frame_warp3d(ctx, x, cam, depth=d, iters=5)
    with pytest.raises(RuntimeError, match="rotation"):
        ops.frame_warp3d(ctx, x, cam._replace(R=(2.0,) + cam.R[1:]))
    with pytest.raises(RuntimeError, match="positive"):
        ops.frame_warp3d(ctx, x, cam._replace(near=0.0))
