"""GPU test of the animation driver's 3D mode (cgd_amd/animate.py) on the smallest scene of tests/test_gpu_animate.py: synthetic weights,
64 x 64, eight `ddim` steps, three frames, a callable depth.  Device against device, bit for bit: the init image of every later frame is
ops.frame_warp3d of the frame before, with the depth the callable returned for that frame's pred_xstart; the PNGs land where 2D mode puts
them.  What the kernel computes is checked in tests/test_gpu_warp3d.py."""
import os

import pytest
import torch as th

from tests.test_gpu_animate import FRAMES, SKIP, _kw, _Recording

pytestmark = pytest.mark.gpu

MOTION = dict(translation_x="0:(0),2:(20)", translation_y=-6.0, translation_z="0:(0),2:(12)", rotation_3d_x=0.5, rotation_3d_y="0:(0),2:(2)",
              rotation_3d_z=-1.0, fov=50.0)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("animate3d")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
        mp.chdir(tmp)
        from cgd_amd import animate as an
        rec = _Recording(mp)
        seen = []

        def depth_fn(x0):
            seen.append(x0.detach().clone())
            return 0.6 + x0.mean(dim=1, keepdim=True)  # (B,1,H,W) in [0.6, 1.6]

        items = list(an.animate(FRAMES, mode="3d", depth=depth_fn, depth_iters=2, near=0.1, frames_skip=SKIP, frames_scale=1500,
                                border="reflect", interp="bilinear", **MOTION, **_kw(tmp, "fly")))
        th.cuda.synchronize()
        return dict(items=items, runs=rec.take(), seen=seen, tmp=tmp)


def test_later_frames_start_from_frame_warp3d_of_the_frame_before(scene):
    from cgd_amd import animate as an
    from cgd_amd import lib, ops
    runs, seen = scene["runs"], scene["seen"]
    assert len(runs) == FRAMES and len(seen) == FRAMES - 1
    assert runs[0][0] is None and runs[0][1] == 0 and runs[0][4] == 8
    ctx = lib.Context(0, 1)
    tracks = {k: an.keyframes(v, FRAMES) for k, v in MOTION.items()}
    for k in (1, 2):
        init, skip, sample, x0, steps = runs[k]
        assert skip == 4 and steps == 4 and th.isfinite(sample).all()
        prev_sample, prev_x0 = runs[k - 1][2], runs[k - 1][3]
        assert tuple(seen[k - 1].shape) == (2, 3, 64, 64) and seen[k - 1].is_cuda
        assert float(seen[k - 1].min()) >= 0 and float(seen[k - 1].max()) <= 1
        assert th.equal(seen[k - 1], (prev_x0.clamp(-1, 1) + 1) / 2)
        cam = an.camera(tracks["translation_x"][k], tracks["translation_y"][k], tracks["translation_z"][k], tracks["rotation_3d_x"][k],
                        tracks["rotation_3d_y"][k], tracks["rotation_3d_z"][k], tracks["fov"][k], 64, 64, near=0.1)
        depth = (0.6 + seen[k - 1].mean(dim=1, keepdim=True)).contiguous()
        want = ops.frame_warp3d(ctx, prev_sample, cam, depth=depth, interp="bilinear", border="reflect", clamp=True, iters=2)
        assert th.equal(init, want), k
        assert float(init.abs().max()) <= 1.0 and not th.equal(init, prev_sample.clamp(-1, 1))  # the camera moved


def test_pngs_land_where_2d_mode_puts_them(scene):
    root = scene["tmp"] / "fly"
    assert [(k, b, os.path.relpath(p, root)) for k, b, p in scene["items"]] == [
        (k, b, os.path.join("Loose_seal", f"{b:02}", f"{k:04}.png")) for k in range(FRAMES) for b in (0, 1)]
    assert all(os.path.isfile(p) for _, _, p in scene["items"])
