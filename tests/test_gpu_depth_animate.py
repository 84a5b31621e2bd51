"""The depth network in the animation driver's 3D mode, on the smallest scene of tests/test_gpu_animate3d.py (synthetic weights, 64 x 64, eight
`ddim` steps), two frames: a DepthNet passed as `depth=` is the callable animate already knows, and `--depth_model` builds one."""
import os

import pytest
import torch as th

from tests.test_gpu_animate import SKIP, _kw, _Recording

pytestmark = pytest.mark.gpu

TINY = dict(patch=16, width=128, layers=4, heads=2, hooks=(0, 1, 2, 3), native_grid=2, features=32, reassemble_channels=(32, 64, 128, 128))
MOTION = dict(translation_z=40.0, translation_x=6.0, fov=50.0)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("depth_animate")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
        mp.chdir(tmp)
        from cgd_amd import animate as an
        from cgd_amd import lib, nets, synthetic
        ctx = lib.Context(0, 1)
        # constants that put the synthetic net's O(1) inverse depth across the mapping: depths between the floor and about 1.5
        net = nets.DepthNet(ctx, TINY, size=64, offset=3.0, scale=2.0, floor=0.2).load_state_dict(synthetic.depth_state_dict(TINY, seed=3))
        rec = _Recording(mp)
        kw = dict(mode="3d", frames_skip=SKIP, frames_scale=1500, border="reflect", interp="bilinear", **MOTION)
        list(an.animate(2, depth=net, **kw, **_kw(tmp, "net")))
        direct = rec.take()
        seen = []

        def wrapped(x):
            seen.append(x.detach().clone())
            return net(x)

        list(an.animate(2, depth=wrapped, **kw, **_kw(tmp, "fn")))
        th.cuda.synchronize()
        return dict(direct=direct, wrapped=rec.take(), seen=seen, net=net, ctx=ctx, tmp=tmp)


def test_a_depth_net_is_the_callable_animate_takes(scene):
    from cgd_amd import animate as an
    from cgd_amd import ops
    direct, wrapped = scene["direct"], scene["wrapped"]
    assert len(direct) == 2 and len(wrapped) == 2 and len(scene["seen"]) == 1
    for a, b in zip(direct, wrapped):
        assert (a[0] is None) == (b[0] is None) and (a[0] is None or th.equal(a[0], b[0]))
        assert th.equal(a[2], b[2]) and th.equal(a[3], b[3])  # the last sample and pred_xstart of both frames, bit for bit
    # the init image of frame 1 is the warp by the net's depth, and not the flat-depth warp
    depth = scene["net"](scene["seen"][0])
    assert tuple(depth.shape) == (2, 1, 64, 64) and float(depth.min()) >= 0.2 and float(depth.max() - depth.min()) > 0.05
    cam = an.camera(MOTION["translation_x"], 0.0, MOTION["translation_z"], 0.0, 0.0, 0.0, MOTION["fov"], 64, 64, near=0.05)
    prev = direct[0][2]
    want = ops.frame_warp3d(scene["ctx"], prev, cam, depth=depth, interp="bilinear", border="reflect", clamp=True, iters=1)
    flat = ops.frame_warp3d(scene["ctx"], prev, cam, depth=None, interp="bilinear", border="reflect", clamp=True, iters=1)
    assert th.equal(direct[1][0], want) and not th.equal(direct[1][0], flat)


def test_depth_model_on_the_command_line_builds_a_net_and_completes(scene, capsys):
    from cgd_amd import animate as an
    from cgd_amd import nets
    tmp = scene["tmp"]
    built = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
        mp.chdir(tmp)
        plain = an.load_depth_model
        mp.setattr(an, "load_depth_model", lambda ctx, spec: built.append(plain(ctx, spec)) or built[-1])
        an.main(["--frames", "2", "--mode", "3d", "--translation_z", "30", "--frames_skip", str(SKIP), "--frames_scale", "0",
                 "--depth_model", "dpt_large-midas-2f21e586.pt:size=64:offset=3:scale=2", "--",
                 "--prompts", "Loose seal.", "--image_size", "64", "--batch_size", "1", "--num_cutouts", "2", "--timestep_respacing", "ddim8",
                 "--prefix", str(tmp / "cli"), "--checkpoints_dir", str(tmp / "ckpt"), "--quiet", "--device", "cuda"])
    assert len(built) == 1 and isinstance(built[0], nets.DepthNet)
    assert (built[0].size, built[0].offset, built[0].scale, built[0].config["layers"]) == (64, 3.0, 2.0, 24)
    lines = [ln.split("\t") for ln in capsys.readouterr().out.strip().splitlines() if ln.count("\t") == 2]
    assert [ln[0] for ln in lines] == ["0", "1"] and all(os.path.isfile(ln[2]) for ln in lines)
