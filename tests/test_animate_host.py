"""Host side of 2D animation (cgd_amd/animate.py, csrc/warp.hip): the float64 restatement of the warp (tests/warp_ref.py) against torch's
grid_sample and numpy's roll, the keyframe parser, the motion matrix and its conventions, animate's refusals before any load, the argument
refusals of the three new exports (no context, no GPU), ClipGuidance.set_init / set_targets, and animate's call sequence on recording
fakes.  No GPU."""
import ctypes as C
import math
import os
import types

import numpy as np
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import animate as an
from cgd_amd import guidance as dg
from cgd_amd import lib as L
from tests import warp_ref as R


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", R.INTERPS)
@pytest.mark.parametrize("border,padding", [("replicate", "border"), ("reflect", "reflection")])
def test_restatement_matches_grid_sample(interp, border, padding):
    th.manual_seed(0)
    B, H, W = 2, 13, 21
    src = th.randn(B, 3, H, W, dtype=th.float64)
    m = an.motion_matrix(1.3, 17.0, 7.3, -25.6, H, W)
    want = th.nn.functional.grid_sample(src, R.grid_sample_matrix(m, H, W).expand(B, -1, -1, -1), mode=interp, padding_mode=padding,
                                        align_corners=True)
    err = float((R.warp_fp64(src, m, interp, border) - want).abs().max())
    print(f"{interp} {border}: |restatement - grid_sample| {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("interp", R.INTERPS)
def test_restatement_integer_wrap_shift_is_a_roll(interp):
    th.manual_seed(1)
    src = th.randn(1, 2, 9, 14, dtype=th.float64)
    for tx, ty in ((3, 0), (-30, 5), (47, -19)):
        got = R.warp_fp64(src, an.motion_matrix(1.0, 0.0, tx, ty, 9, 14), interp, "wrap")
        assert np.array_equal(got.numpy(), np.roll(src.numpy(), (ty, tx), axis=(2, 3)))


def test_restatement_borders_and_a_side_of_one():
    i = th.arange(-9, 10)
    assert R.border_index(i, 4, "wrap").tolist() == [(v % 4) for v in range(-9, 10)]
    assert R.border_index(i, 4, "replicate").tolist() == [min(max(v, 0), 3) for v in range(-9, 10)]
    assert R.border_index(th.arange(-7, 8), 4, "reflect").tolist() == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]
    assert R.border_index(i, 1, "reflect").tolist() == [0] * 19
    w = R.cubic_weights(th.tensor([0.0, 0.5], dtype=th.float64))
    assert [float(t[0]) for t in w] == [0.0, 1.0, 0.0, 0.0]
    assert [float(t[1]) for t in w] == pytest.approx([-0.09375, 0.59375, 0.59375, -0.09375], abs=1e-15)


def test_restatement_of_the_colour_transfer():
    th.manual_seed(2)
    x, ref = th.randn(2, 3, 5, 7).double() * 0.4 + 0.2, th.randn(1, 3, 5, 7).double()
    sx, sr = R.stats_fp64(x), R.stats_fp64(ref)
    assert th.equal(R.color_match_fp64(x, sx, sr, 0.0), x)
    full = R.color_match_fp64(x, sx, sr, 1.0)
    assert float((R.stats_fp64(full) - sr.expand(2, -1, -1)).abs().max()) <= 1e-12
    half = R.color_match_fp64(x, sx, sr, 0.5)
    assert float((half - (x + full) / 2).abs().max()) <= 1e-12
    flat = th.full((1, 3, 4, 4), 0.25, dtype=th.float64)
    out = R.color_match_fp64(flat, R.stats_fp64(flat), sr, 1.0)
    assert th.isfinite(out).all() and float((out - sr[0, :, 0].view(1, 3, 1, 1)).abs().max()) <= 1e-15


# ---- keyframes ------------------------------------------------------------------------------------------------------------------------
def test_keyframes_interpolate_and_hold():
    v = an.keyframes("10:(1.0), 30:(1.04), 90:(1.0)", 100)
    assert len(v) == 100 and v[:11] == [1.0] * 11 and v[30] == 1.04 and v[90:] == [1.0] * 10
    assert v[20] == pytest.approx(1.02, abs=1e-15) and v[60] == pytest.approx(1.02, abs=1e-15) and v[15] == pytest.approx(1.01, abs=1e-15)
    assert an.keyframes("0:(0),60:(2)", 4) == pytest.approx([0.0, 1 / 30, 2 / 30, 3 / 30])
    assert an.keyframes(" 5 : ( -40 ) ", 3) == [-40.0] * 3  # one key holds everywhere
    assert an.keyframes("30:(2), 0:(1)", 31)[15] == pytest.approx(1.5)  # keys in any order
    for bare in (1.02, 3, "1.02", " -4e-1 "):
        assert an.keyframes(bare, 5) == [float(bare)] * 5


@pytest.mark.parametrize("bad", ["", "  ", "abc", "0:1.0", "0:(1.0", "0(1.0)", "0:(1.0),", "0:(1.0) 3:(2)", "0:(1.0), 0:(2)", "-1:(2)", "1.5:(2)",
                                 "0:(x)", "0:(nan)", "0:(inf)", "a:(1)", "0:()", "0:((1))", "nan", True, None])
def test_keyframes_refuse_malformed_text(bad):
    with pytest.raises(ValueError):
        an.keyframes(bad, 10)


def test_keyframes_refuse_an_empty_clip():
    with pytest.raises(ValueError):
        an.keyframes("0:(1)", 0)


# ---- the motion matrix ----------------------------------------------------------------------------------------------------------------
def _apply(m, x, y):
    return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]


@pytest.mark.parametrize("args", [(1.3, 17.0, 7.3, -25.6, 13, 21), (0.5, -200.0, -3.0, 0.25, 64, 64), (2.0, 90.0, 0.0, 0.0, 1, 9)])
def test_forward_after_inverse_is_the_identity(args):
    inv, fwd = an.motion_matrix(*args), an.forward_matrix(*args)
    for p in ((0.0, 0.0), (20.0, 0.0), (3.5, 11.25), (-40.0, 100.0)):
        q = _apply(fwd, *_apply(inv, *p))
        r = _apply(inv, *_apply(fwd, *p))
        assert max(abs(q[0] - p[0]), abs(q[1] - p[1]), abs(r[0] - p[0]), abs(r[1] - p[1])) <= 1e-12


def test_motion_conventions():
    assert an.motion_matrix(1.0, 0.0, 0.0, 0.0, 24, 40) == (1.0, -0.0, 0.0, 0.0, 1.0, 0.0)
    # tx = 3 alone: dst[x] = src[x - 3] (content moves right); ty = 2: content moves down
    assert an.motion_matrix(1.0, 0.0, 3.0, 0.0, 24, 40) == (1.0, -0.0, -3.0, 0.0, 1.0, 0.0)
    assert an.motion_matrix(1.0, 0.0, 0.0, 2.0, 24, 40) == (1.0, -0.0, 0.0, 0.0, 1.0, -2.0)
    src = th.arange(40.0).view(1, 1, 1, 40).expand(1, 1, 24, 40)
    out = R.warp_fp64(src, an.motion_matrix(1.0, 0.0, 3.0, 0.0, 24, 40), "bilinear", "wrap")
    assert out[0, 0, 0, 10] == 7.0
    # zoom 2 maps the geometric centre to itself and halves distances in the inverse
    m = an.motion_matrix(2.0, 0.0, 0.0, 0.0, 24, 40)
    cx, cy = 19.5, 11.5
    assert _apply(m, cx, cy) == pytest.approx((cx, cy), abs=1e-12)
    assert _apply(m, cx + 8, cy - 6) == pytest.approx((cx + 4, cy - 3), abs=1e-12)
    # 90 degrees on a square frame: the right edge's midpoint goes to the top edge's midpoint (counter-clockwise on the screen)
    fwd = an.forward_matrix(1.0, 90.0, 0.0, 0.0, 33, 33)
    assert _apply(fwd, 32.0, 16.0) == pytest.approx((16.0, 0.0), abs=1e-12)
    inv = an.motion_matrix(1.0, 90.0, 0.0, 0.0, 33, 33)
    assert _apply(inv, 16.0, 0.0) == pytest.approx((32.0, 16.0), abs=1e-12)
    # 180 degrees about the geometric centre permutes the pixels of an even frame
    inv = an.motion_matrix(1.0, 180.0, 0.0, 0.0, 24, 40)
    assert _apply(inv, 0.0, 0.0) == pytest.approx((39.0, 23.0), abs=1e-12)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            an.motion_matrix(bad, 0.0, 0.0, 0.0, 8, 8)


def test_prompts_at_cli_values():
    assert an.parse_prompts_at(["40=a city at night|a skyline:0.5", " 3 =x"]) == {40: ["a city at night", "a skyline:0.5"], 3: ["x"]}
    for bad in (["a city"], ["x=a city"], ["4="], ["4=a", "4=b"], ["-1=a"]):
        with pytest.raises(ValueError):
            an.parse_prompts_at(bad)
    a = an.build_parser().parse_args(["--frames", "3", "--zoom", "0:(1.02)", "--fixed_seed", "--prompts_at", "1=a", "--prompts_at", "2=b"])
    assert a.frames == 3 and a.zoom == "0:(1.02)" and a.border == "wrap" and a.interp == "bicubic" and a.frames_skip == 0.6
    assert a.frames_scale == 1500 and a.color_match == 0.0 and a.fixed_seed and a.prompts_at == ["1=a", "2=b"]


# ---- refusals of the driver -------------------------------------------------------------------------------------------------------------
def test_animate_refuses_before_anything_is_loaded(monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util
    from cgd_amd import shard

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    for mod, name in ((clip_util, "load_clip"), (clip_util, "encode_text_prompt"), (script_util, "download_guided_diffusion"),
                      (script_util, "load_guided_diffusion"), (script_util, "load_lpips"), (mine, "ClipGuidance")):
        monkeypatch.setattr(mod, name, no_load)
    base = dict(prompts=["a cat"], device="cuda", timestep_respacing="ddim10")
    for frames, kw in ((3, dict(init_image="a.png::m.png")), (3, dict(init_image="invert=a.png")), (3, dict(init_image="upsample=a.png")),
                       (3, dict(init_image="ilvr8=a.png")), (3, dict(prompts=["a cat=>a dog"], init_image="a.png")),
                       (3, dict(prompts_at={1: ["a cat=>a dog"]})), (3, dict(use_augs=True)), (0, {}), (-2, {}), (2.5, {}),
                       (3, dict(frames_skip=1.0)), (3, dict(frames_skip=-0.1)), (3, dict(frames_skip=0.96)), (3, dict(border="zeros")),
                       (3, dict(interp="nearest")), (3, dict(color_match=1.5)), (3, dict(zoom="0:(1),2:(0)")), (3, dict(angle="0:1")),
                       (3, dict(prompts=["a cat@@0,0,0.5,1"], prompts_at={1: ["a dog"]})), (3, dict(prompts_at={1: []})),
                       (3, dict(prompts_at={-1: ["x"]}))):
        with pytest.raises(ValueError):
            next(an.animate(frames, **{**base, **kw}))
    monkeypatch.setattr(shard, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="one process"):
        next(an.animate(3, **base))


# ---- the C ABI's refusals (judged before the context: no GPU needed) ---------------------------------------------------------------------
def _warp(m=(1, 0, 0, 0, 1, 0), interp=1, border=0, clamp=0):
    return L.Warp((C.c_double * 6)(*m), interp, border, clamp)


def test_frame_warp_refuses_bad_arguments_without_a_context():
    h = L.load()
    ok = dict(src=64, dst=4096, B=1, C=3, H=8, W=8, w=_warp())

    def call(**kw):
        a = {**ok, **kw}
        return h.cgd_frame_warp(None, a["src"], a["dst"], a["B"], a["C"], a["H"], a["W"], None if a["w"] is None else C.byref(a["w"]), None)

    assert call() == -3  # nothing to refuse: the missing context is what is left
    inf, nan = float("inf"), float("nan")
    for kw in (dict(src=None), dict(dst=None), dict(w=None), dict(dst=64), dict(src=66), dict(B=0), dict(C=-1), dict(H=0), dict(W=0),
               dict(H=1 << 16, W=1 << 15), dict(w=_warp(interp=2)), dict(w=_warp(interp=-1)), dict(w=_warp(border=3)), dict(w=_warp(border=-1)),
               dict(w=_warp(m=(1, 0, nan, 0, 1, 0))), dict(w=_warp(m=(inf, 0, 0, 0, 1, 0))), dict(w=_warp(m=(1, 0, 0, 0, 1, -inf))),
               dict(w=_warp(m=(1, 0, 2.0 ** 30 + 1, 0, 1, 0))), dict(w=_warp(m=(1, 0, 0, 0, 1, -(2.0 ** 30) - 1))),
               dict(w=_warp(m=(2.0 ** 28, 0, 0, 0, 1, 0))), dict(w=_warp(m=(1, 0, 0, -(2.0 ** 28), 0, 0)))):
        assert call(**kw) == -2, kw
    assert call(w=_warp(m=(1, 0, 2.0 ** 30 - 7, 0, 1, 0))) == -3  # the far corner lands on 2^30 exactly: accepted
    assert call(H=1 << 16, W=(1 << 15) - 1) == -3


def test_colour_kernels_refuse_bad_arguments_without_a_context():
    h = L.load()
    assert h.cgd_channel_stats(None, 64, 4096, 1, 3, 8, 8, None) == -3
    for args in ((None, 4096, 1, 3, 8, 8), (64, None, 1, 3, 8, 8), (64, 4096, 0, 3, 8, 8), (64, 4096, 1, 3, 8, 0), (64, 4098, 1, 3, 8, 8),
                 (64, 4096, 1, 3, 1 << 16, 1 << 15)):
        assert h.cgd_channel_stats(None, *args, None) == -2, args
    ok = dict(x=64, sx=4096, sr=8192, rb=1, amount=0.5, clamp=0, B=2, C=3, H=8, W=8)

    def call(**kw):
        a = {**ok, **kw}
        return h.cgd_color_match(None, a["x"], a["sx"], a["sr"], a["rb"], a["amount"], a["clamp"], a["B"], a["C"], a["H"], a["W"], None)

    assert call() == -3 and call(rb=2) == -3 and call(amount=0.0) == -3 and call(amount=1.0) == -3
    for kw in (dict(x=None), dict(sx=None), dict(sr=None), dict(rb=3), dict(rb=0), dict(amount=-0.01), dict(amount=1.01), dict(amount=float("nan")),
               dict(B=0), dict(H=-1), dict(x=65), dict(H=1 << 16, W=1 << 15)):
        assert call(**kw) == -2, kw
    for name in ("cgd_frame_warp", "cgd_channel_stats", "cgd_color_match"):
        assert name in L.EXPORTED_SYMBOLS
    assert C.sizeof(L.Warp) == 64


# ---- ClipGuidance between runs ------------------------------------------------------------------------------------------------------------
def test_set_init_replaces_the_lpips_reference_and_set_targets_the_prompts():
    from tests.test_direction_host import _Recorder
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    refs = []
    lp = types.SimpleNamespace(set_reference=lambda t: refs.append(t.clone()),
                               loss_grad=lambda x_in, grad_scale, g, accumulate, loss: (refs.append(grad_scale) or loss, g))
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(2, 16), [0.5, 0.5], 4, lpips=lp)
    assert guid.lpips is None  # no init image yet: the term is off and the handle is only kept
    x = th.zeros(2, 3, 32, 48)

    def step():
        guid.current_timestep, guid.coords_tape, guid.calls = 49, [[(0, 0, 32)] * 4], 0
        guid.native(x, x.clone(), x.clone(), coef=None)

    step()
    assert not refs
    a, b = th.full((1, 3, 32, 48), 0.25), th.full((2, 3, 32, 48), -0.5)
    guid.set_init(a, 1500)
    step()
    step()
    assert len(refs) == 3 and th.equal(refs[0], a.expand(2, -1, -1, -1)) and refs[1:] == [1500.0, 1500.0]  # one set_reference, two steps
    guid.set_init(b, 700)
    step()
    assert len(refs) == 5 and th.equal(refs[3], b) and refs[4] == 700.0
    guid.set_init(None, 0)
    step()
    assert len(refs) == 5 and guid.lpips is None
    with pytest.raises(ValueError):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(2, 16), [0.5, 0.5], 4).set_init(a, 1.0)
    # prompts: the weight matrix is rebuilt for the new list
    del r.calls[:]
    step()
    assert r.args("cgd_spherical_loss")[0][8] == 2 and tuple(guid._wm[2].shape) == (2, 2)
    e = th.randn(1, 16)
    guid.set_targets(e, [1.0])
    del r.calls[:]
    step()
    assert r.args("cgd_spherical_loss")[0][8] == 1 and th.equal(guid._wm[2], th.ones(2, 1))
    assert th.allclose(guid.targets_n, th.nn.functional.normalize(e, dim=-1))
    with pytest.raises(ValueError):
        guid.set_targets(e, [1.0, 2.0])


# ---- the driver on recording fakes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed_seed", [False, True])
def test_animate_call_sequence_with_fake_device_objects(tmp_path, monkeypatch, fixed_seed):
    from cgd import cgd as mine
    from cgd import clip_util, script_util
    from cgd_amd import ops
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    events = []

    class FakeTorch:  # torch, minus the device placement (there is no GPU here)
        def __getattr__(self, k):
            return getattr(th, k)

        @staticmethod
        def tensor(data, device=None, **kw):
            return th.tensor(data, **kw)

        @staticmethod
        def zeros(shape, device=None, **kw):
            return th.zeros(shape, **kw)

    monkeypatch.setattr(mine, "th", FakeTorch())
    real_seed = th.manual_seed
    monkeypatch.setattr(th, "manual_seed", lambda seed: events.append(("seed", seed)) or real_seed(seed))
    tower = types.SimpleNamespace(ctx="ctx", input_resolution=16, out_dim=8, patch=8)
    monkeypatch.setattr(clip_util, "load_clip", lambda name, device: events.append(("load_clip", name)) or (types.SimpleNamespace(tower=tower), 16))
    monkeypatch.setattr(clip_util, "encode_text_prompt",
                        lambda txt, w, name, device: events.append(("encode", txt)) or (th.full((1, 8), float(len(txt))), w))

    class FakeDiffusion:
        num_timesteps = 10

        def ddim_sample_loop_progressive(self, model, shape, **kw):
            events.append(("loop", shape, kw["skip_timesteps"], None if kw["init_image"] is None else kw["init_image"].clone()))
            n = len([e for e in events if e[0] == "loop"])
            for i in range(self.num_timesteps - kw["skip_timesteps"]):
                yield {"sample": th.full(shape, 0.125 * n), "pred_xstart": th.full(shape, -1.0 + 0.25 * n)}

        p_sample_loop_progressive = ddim_sample_loop_progressive

    monkeypatch.setattr(script_util, "load_guided_diffusion",
                        lambda **kw: events.append(("load_unet",)) or (types.SimpleNamespace(ctx="ctx"), FakeDiffusion()))
    monkeypatch.setattr(script_util, "load_lpips", lambda *a, **k: events.append(("load_lpips",)) or "lpips")

    class FakeGuidance:
        def __init__(self, ctx, unet, towers, diffusion, target_embeds, weights, num_cutouts, **kw):
            events.append(("guidance", kw["lpips"], kw["init_tensor"], kw["init_scale"]))
            self.current_timestep, self.last_ran = None, True

        def set_init(self, init, scale):
            events.append(("set_init", init.clone(), scale, self.current_timestep))

        def set_targets(self, embeds, weights):
            events.append(("set_targets", [e.clone() for e in embeds], weights.tolist()))

    monkeypatch.setattr(mine, "ClipGuidance", FakeGuidance)
    monkeypatch.setattr(script_util, "stage_images", lambda x: types.SimpleNamespace(get=lambda: script_util.to_uint8_hwc(x)))

    def fake_warp(ctx, src, matrix, interp, border, clamp):
        events.append(("warp", ctx, src.clone(), tuple(matrix), interp, border, clamp))
        return src + 1.0

    def fake_stats(ctx, x):
        events.append(("stats", x.clone()))
        return th.zeros(x.shape[0], 3, 2)

    def fake_match(ctx, x, stats_ref, amount, clamp):
        events.append(("match", amount, clamp))
        return x.add_(0.5)

    monkeypatch.setattr(ops, "frame_warp", fake_warp)
    monkeypatch.setattr(ops, "channel_stats", fake_stats)
    monkeypatch.setattr(ops, "color_match", fake_match)
    items = list(an.animate(3, zoom="0:(1.0),2:(1.5)", angle=0.0, translation_x="0:(0),2:(4)", translation_y=0, border="reflect",
                            interp="bilinear", frames_skip=0.6, frames_scale=1500, color_match=0.25, fixed_seed=fixed_seed,
                            prompts_at={1: ["fog:2", "a boat"], 2: ["a boat"]}, prompts=["a boat"], image_size=128, batch_size=2,
                            num_cutouts=4, timestep_respacing="ddim10", seed=11, prefix_path=str(tmp_path / "out"),
                            checkpoints_dir=str(tmp_path / "ck"), device="cuda", progress=False, width_offset=16))
    kinds = [e[0] for e in events]
    # one build of the networks and of the guidance; the LPIPS handle is loaded for the later frames although frame 0 has no init image
    assert kinds.count("load_clip") == kinds.count("load_unet") == kinds.count("load_lpips") == kinds.count("guidance") == 1
    assert [e for e in events if e[0] == "guidance"][0][1:] == ("lpips", None, 0)
    # every distinct text is encoded once
    assert [e[1] for e in events if e[0] == "encode"] == ["a boat", "fog"]
    tg = [e for e in events if e[0] == "set_targets"]
    assert len(tg) == 2 and tg[0][2] == pytest.approx([2 / 3, 1 / 3]) and tg[1][2] == [1.0]
    assert tg[0][1][0][:, 0].tolist() == [3.0, 6.0] and tg[1][1][0][:, 0].tolist() == [6.0]
    assert [e[1] for e in events if e[0] == "seed"] == ([11, 11, 11] if fixed_seed else [11, 12, 13])
    # frame 0: the plain run; frames 1, 2: the warped, colour-matched previous sample as init image, 6 of the 10 steps skipped
    loops = [e for e in events if e[0] == "loop"]
    assert [(e[1], e[2]) for e in loops] == [((2, 3, 128, 144), 0), ((2, 3, 128, 144), 6), ((2, 3, 128, 144), 6)] and loops[0][3] is None
    warps, inits = [e for e in events if e[0] == "warp"], [e for e in events if e[0] == "set_init"]
    assert len(warps) == len(inits) == 2 and kinds.count("stats") == 1 and [e[1:] for e in events if e[0] == "match"] == [(0.25, True)] * 2
    assert th.equal(warps[0][2], th.full((2, 3, 128, 144), 0.125)) and th.equal(warps[1][2], th.full((2, 3, 128, 144), 0.25))
    assert all(w[1] == "ctx" and w[4:] == ("bilinear", "reflect", True) for w in warps)
    assert warps[0][3] == an.motion_matrix(1.25, 0.0, 2.0, 0.0, 128, 144) and warps[1][3] == an.motion_matrix(1.5, 0.0, 4.0, 0.0, 128, 144)
    for k in (0, 1):
        assert th.equal(inits[k][1], th.full((2, 3, 128, 144), 0.125 * (k + 1) + 1.5)) and inits[k][2] == 1500 and th.equal(loops[k + 1][3], inits[k][1])
    # order within a frame: seed, warp, match, set_init, loop
    at = kinds.index("warp")
    assert kinds[at - 1] == "seed" and kinds[at:at + 4] == ["warp", "match", "set_init", "loop"]
    # one PNG per frame and sample, named by the frame
    assert [(k, b, os.path.relpath(p, tmp_path / "out")) for k, b, p in items] == [
        (k, b, os.path.join("a_boat", f"{b:02}", f"{k:04}.png")) for k in range(3) for b in (0, 1)]
    assert all(os.path.isfile(p) for _, _, p in items)
    from PIL import Image
    assert [int(np.array(Image.open(p))[0, 0, 0]) for _, b, p in items if b == 0] == [31, 63, 95]  # the last pred_xstart of every run

    # frames_scale 0: no LPIPS load, and set_init switches the term off
    del events[:]
    seen = []
    FakeGuidance.set_init = lambda self, init, scale: seen.append((init, scale))
    list(an.animate(2, frames_scale=0, prompts=["a boat"], image_size=128, timestep_respacing="ddim10", prefix_path=str(tmp_path / "o2"),
                    checkpoints_dir=str(tmp_path / "ck"), device="cuda", progress=False))
    assert "load_lpips" not in [e[0] for e in events] and seen == [(None, 0)] and "match" not in [e[0] for e in events]
