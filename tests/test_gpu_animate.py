"""GPU test of the animation driver (cgd_amd/animate.py) on the synthetic-weights 64 x 64 scene of the drop-in test of tests/test_gpu_ilvr.py:
eight `ddim` steps, three frames.  Frame 0 against the plain generator, the later frames against a chain built by hand from the public pieces,
the PNG names, a prompt switch, and how often the loaders run.  The comparisons are device against device, bit for bit: what the pieces compute
is checked where they are tested (tests/test_gpu_warp.py, the sampler's and the guidance's own files); here only that the driver strings them
together as documented."""
import os

import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

FRAMES, SEED, SKIP = 3, 7, 0.5
MOTION = dict(zoom="0:(1.0),2:(1.08)", angle=3.0, translation_x="0:(0),2:(5)", translation_y=-1.5)


def _kw(tmp, name, **extra):
    return dict(prompts=["Loose seal."], image_size=64, batch_size=2, num_cutouts=2, timestep_respacing="ddim8", seed=SEED,
                prefix_path=str(tmp / name), checkpoints_dir=str(tmp / "ckpt"), save_frequency=1, progress=False, device="cuda", **extra)


class _Recording:
    """every run of the ddim loop: (init_image, skip_timesteps, the last yielded sample and pred_xstart)"""

    def __init__(self, mp):
        from cgd_amd import sampler
        self.runs = runs = []
        plain = sampler.GuidedSampler.ddim_sample_loop_progressive

        def recording(self, *a, **kw):
            init = kw.get("init_image")
            rec = [None if init is None else init.detach().clone(), kw.get("skip_timesteps"), None, None, 0]
            runs.append(rec)
            for out in plain(self, *a, **kw):
                rec[2], rec[3], rec[4] = out["sample"].detach().clone(), out["pred_xstart"].detach().clone(), rec[4] + 1
                yield out

        mp.setattr(sampler.GuidedSampler, "ddim_sample_loop_progressive", recording)

    def take(self):
        out = list(self.runs)
        del self.runs[:]
        return out


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Every run of the file, made once: the plain generator, animate without motion, with motion and colour matching, with a prompt switch
    on top, and the two chains by hand."""
    tmp = tmp_path_factory.mktemp("animate")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
        mp.chdir(tmp)
        from cgd import cgd as entry
        from cgd import clip_util, script_util
        from cgd_amd import animate as an
        from cgd_amd import ops
        rec = _Recording(mp)
        loads = {"unet": 0, "clip": 0, "lpips": 0}
        for mod, name, key in ((script_util, "load_guided_diffusion", "unet"), (clip_util, "load_clip", "clip"), (script_util, "load_lpips", "lpips")):
            def counted(*a, _f=getattr(mod, name), _k=key, **k):
                loads[_k] += 1
                return _f(*a, **k)
            mp.setattr(mod, name, counted)
        s = {}
        s["plain_items"] = list(entry.clip_guided_diffusion(**_kw(tmp, "plain")))
        s["plain"], s["plain_loads"] = rec.take(), dict(loads)
        before = dict(loads)
        s["still_items"] = list(an.animate(FRAMES, frames_skip=SKIP, frames_scale=1500, **_kw(tmp, "still")))
        s["still"], s["still_loads"] = rec.take(), {k: loads[k] - before[k] for k in loads}
        s["moving_items"] = list(an.animate(FRAMES, frames_skip=SKIP, frames_scale=1500, color_match=0.5, border="reflect", interp="bilinear",
                                            **MOTION, **_kw(tmp, "moving")))
        s["moving"] = rec.take()
        s["switch_items"] = list(an.animate(FRAMES, frames_skip=SKIP, frames_scale=1500, color_match=0.5, border="reflect", interp="bilinear",
                                            prompts_at={1: ["A harbour at dusk.:2", "fog"]}, **MOTION, **_kw(tmp, "switch")))
        s["switch"] = rec.take()

        def by_hand(name, color, border, interp, motion):
            run = entry.prepare_run(**_kw(tmp, name), lpips_for_later=True)
            ctx = run.model.ctx
            tracks = [an.keyframes(motion.get(k, d), FRAMES) for k, d in (("zoom", 1.0), ("angle", 0.0), ("translation_x", 0.0), ("translation_y", 0.0))]
            skip, prev, stats0 = round(SKIP * run.diffusion.num_timesteps), None, None
            for k in range(FRAMES):
                init = None
                if k:
                    th.manual_seed(SEED + k)
                    init = ops.frame_warp(ctx, prev, an.motion_matrix(*(t[k] for t in tracks), 64, 64), interp=interp, border=border, clamp=True)
                    if color:
                        ops.color_match(ctx, init, stats0, amount=color, clamp=True)
                    run.cond_fn.set_init(init, 1500)
                for out in (run.samples(init_image=init, skip_timesteps=skip) if k else run.samples()):
                    run.cond_fn.current_timestep -= 1
                prev = out["sample"].detach().clone()
                if k == 0 and color:
                    stats0 = ops.channel_stats(ctx, prev)
            return rec.take()

        s["still_by_hand"] = by_hand("hand0", 0.0, "wrap", "bicubic", {})
        s["moving_by_hand"] = by_hand("hand1", 0.5, "reflect", "bilinear", MOTION)
        s["tmp"] = tmp
        th.cuda.synchronize()
    return s


def test_frame_0_is_the_plain_generators_last_frame(scene):
    (_, skip, sample, x0, steps), = scene["plain"]
    assert steps == 8 and skip == 0
    for name in ("still", "moving", "switch"):
        init0, skip0, sample0, x00, steps0 = scene[name][0]
        assert init0 is None and skip0 == 0 and steps0 == 8
        assert th.equal(sample0, sample) and th.equal(x00, x0), name  # (a prompt switch at frame 1 leaves frame 0's bits alone)
    from PIL import Image
    last = {b: p for b, p in scene["plain_items"] if os.path.basename(p) == "0007.png"}
    first = {b: p for k, b, p in scene["still_items"] if k == 0}
    assert sorted(last) == sorted(first) == [0, 1]
    for b in (0, 1):
        assert np.array_equal(np.array(Image.open(last[b])), np.array(Image.open(first[b])))


@pytest.mark.parametrize("name", ["still", "moving"])
def test_later_frames_are_the_chain_built_by_hand(scene, name):
    """Device against device: animate's frames 1 and 2 against ops.frame_warp of the previous `sample`, ops.color_match, cond_fn.set_init
    and the sampler loop with init_image= / skip_timesteps=, under the same seeds."""
    mine, hand = scene[name], scene[name + "_by_hand"]
    assert len(mine) == len(hand) == FRAMES
    for k in (1, 2):
        assert mine[k][1] == hand[k][1] == 4 and mine[k][4] == hand[k][4] == 4
        for i in (0, 2, 3):
            assert th.isfinite(mine[k][i]).all() and th.equal(mine[k][i], hand[k][i]), (k, i)
        assert tuple(mine[k][0].shape) == (2, 3, 64, 64) and float(mine[k][0].abs().max()) <= 1.0  # the warped state, clamped
    if name == "still":  # no motion: the init image of frame k is the clamped final sample of frame k - 1
        assert th.equal(mine[1][0], mine[0][2].clamp(-1, 1))
    else:
        assert not th.equal(mine[1][0], scene["still"][1][0])


def test_pngs_are_named_by_frame(scene):
    for name in ("still", "moving", "switch"):
        items, root = scene[name + "_items"], scene["tmp"] / name
        assert [(k, b, os.path.relpath(p, root)) for k, b, p in items] == [
            (k, b, os.path.join("Loose_seal", f"{b:02}", f"{k:04}.png")) for k in range(FRAMES) for b in (0, 1)]
        assert all(os.path.isfile(p) for _, _, p in items)


def test_a_prompt_switch_changes_the_frames_from_its_keyframe_on(scene):
    a, b = scene["moving"], scene["switch"]
    assert th.equal(a[1][0], b[1][0])  # frame 1 starts from the same warped frame 0 ...
    assert not th.equal(a[1][2], b[1][2]) and not th.equal(a[2][2], b[2][2])  # ... and goes elsewhere
    assert all(th.isfinite(r[2]).all() for r in b)


def test_networks_are_loaded_once_per_animation(scene):
    """Three frames call the loaders as often as the one run of the plain generator does (its prompt encoder asks clip_util.load_clip, which
    caches, once more per prompt), plus the LPIPS handle for the later frames: nothing is built per frame."""
    assert scene["plain_loads"] == {"unet": 1, "clip": 2, "lpips": 0}
    assert scene["still_loads"] == {"unet": 1, "clip": 2, "lpips": 1}
