"""GPU test of the animation driver's video mode (cgd_amd/animate.py) on the smallest scene of tests/test_gpu_animate.py: synthetic weights,
64 x 64, eight `ddim` steps, three frames.  The clip is the test's own: PNGs of a smooth texture shifted by a few pixels per frame.  Device
against device, bit for bit: frame 0 starts from the clip's frame 0; frame k starts from ops.frame_warp_flow of the previous sample along
ops.flow_estimate(clip_k, clip_{k-1}), with the clip's frame k as the fallback, with and without the consistency check; the PNGs land
where 2D mode puts them.  What the kernels compute is checked in tests/test_gpu_flow.py and tests/test_gpu_warp_flow.py."""
import os

import numpy as np
import pytest
import torch as th

from tests import flow_ref as F
from tests.test_gpu_animate import FRAMES, SKIP, _kw, _Recording

pytestmark = pytest.mark.gpu

SHIFT = (2.0, -1.0)  # pixels per frame
RUNS = {"plain": dict(flow_blend=0.999, color_match=0.5, border="replicate", interp="bicubic"),
        "checked": dict(flow_blend=0.8, check_consistency=True, flow_levels=3, flow_iters=2, flow_radius=3, border="reflect", interp="bilinear")}


def _write_clip(folder):
    from PIL import Image
    os.makedirs(folder)
    ys, xs = th.meshgrid(th.arange(64, dtype=th.float64), th.arange(64, dtype=th.float64), indexing="ij")
    paths = []
    for k in range(FRAMES):
        rgb = th.stack([F.texture(xs - SHIFT[0] * k, ys - SHIFT[1] * k, seed=11 + c, max_freq=0.5) for c in range(3)], dim=-1)
        arr = ((rgb / 3 + 0.5).clamp(0, 1) * 255).round().to(th.uint8).numpy()
        paths.append(os.path.join(folder, f"{k:03}.png"))
        Image.fromarray(arr).save(paths[-1])
    return paths


def _load(path, B):
    """as the init image is loaded"""
    from PIL import Image
    pil = Image.open(path).convert("RGB").resize((64, 64))
    return th.from_numpy(np.array(pil)).float().div(255).permute(2, 0, 1).to("cuda").unsqueeze(0).mul(2).sub(1).expand(B, -1, -1, -1).contiguous()


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("animate_video")
    paths = _write_clip(str(tmp / "clip"))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
        mp.chdir(tmp)
        from cgd_amd import animate as an
        rec = _Recording(mp)
        s = dict(tmp=tmp, paths=paths)
        sources = {"plain": str(tmp / "clip"), "checked": str(tmp / "clip" / "*.png")}  # a directory and a glob
        for name, kw in RUNS.items():
            s[name + "_items"] = list(an.animate(FRAMES, mode="video", video_frames=sources[name], frames_skip=SKIP, frames_scale=1500, **kw,
                                                 **_kw(tmp, name)))
            s[name] = rec.take()
        th.cuda.synchronize()
    return s


@pytest.mark.parametrize("name", list(RUNS))
def test_frame_0_starts_from_the_clips_first_frame(scene, name):
    runs = scene[name]
    assert len(runs) == FRAMES
    init, skip, sample, _, steps = runs[0]
    assert skip == 4 and steps == 4 and th.isfinite(sample).all()
    assert th.equal(init, _load(scene["paths"][0], 2))


@pytest.mark.parametrize("name", list(RUNS))
def test_later_frames_start_from_the_previous_sample_moved_along_the_clips_flow(scene, name):
    from cgd_amd import lib, ops
    runs, kw = scene[name], RUNS[name]
    ctx = lib.Context(0, 1)
    flow_kw = dict(levels=kw.get("flow_levels", 4), iters=kw.get("flow_iters", 4), radius=kw.get("flow_radius", 4))
    stats0 = ops.channel_stats(ctx, runs[0][2])
    for k in (1, 2):
        init, skip, sample, _, steps = runs[k]
        assert skip == 4 and steps == 4 and th.isfinite(sample).all()
        now, before = _load(scene["paths"][k], 2), _load(scene["paths"][k - 1], 2)
        flow = ops.flow_estimate(ctx, now[:1], before[:1], **flow_kw)
        back = ops.flow_estimate(ctx, before[:1], now[:1], **flow_kw) if kw.get("check_consistency") else None
        want = ops.frame_warp_flow(ctx, runs[k - 1][2], flow, flow_back=back, fallback=now, blend=kw["flow_blend"], interp=kw["interp"],
                                   border=kw["border"], clamp=True)
        if kw.get("color_match"):
            ops.color_match(ctx, want, stats0, amount=kw["color_match"], clamp=True)
        assert th.equal(init, want), (name, k)
        assert float(init.abs().max()) <= 1.0 and not th.equal(init, runs[k - 1][2].clamp(-1, 1))  # the clip moved
        # the flow the driver followed is the clip's motion: the previous frame is read SHIFT behind
        inner = flow[0, :, 12:-12, 12:-12].cpu()
        assert abs(float(inner[0].median()) + SHIFT[0]) < 0.25 and abs(float(inner[1].median()) + SHIFT[1]) < 0.25


def test_pngs_land_where_2d_mode_puts_them(scene):
    for name in RUNS:
        root = scene["tmp"] / name
        assert [(k, b, os.path.relpath(p, root)) for k, b, p in scene[name + "_items"]] == [
            (k, b, os.path.join("Loose_seal", f"{b:02}", f"{k:04}.png")) for k in range(FRAMES) for b in (0, 1)]
        assert all(os.path.isfile(p) for _, _, p in scene[name + "_items"])
