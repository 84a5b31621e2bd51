"""Host-side tests of video mode (csrc/flow.hip, cgd_amd/animate.py): the float64 restatement of the flow (tests/flow_ref.py) on its own
against analytic motions, its float32 restatement against it, the level rule and the refusals of the C entries through the library without a
context, the listing of a clip's frames, and every refusal of the driver before anything is loaded.  No GPU."""
import ctypes as C
import os

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import animate as an
from cgd_amd import lib as L
from tests import flow_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFT = dict(motion=(2.3, -1.7), seed=0)                 # at least 98 % of all pixels within 0.25 px
ROTATION = dict(motion=(0.8, -0.5, 3.0, 1.03), seed=3)   # 3 degrees, zoom 1.03, a shift: at least 90 %


@pytest.fixture(scope="module")
def scenes():
    """the two 64 x 96 scenes and their float64 reference flows, made once and only read"""
    out = {}
    for name, s in (("shift", SHIFT), ("rotation", ROTATION)):
        tmpl, img, want = F.scene(64, 96, s["motion"], s["seed"])
        out[name] = (tmpl, img, want, F.estimate(tmpl, img))
    return out


def test_reference_recovers_a_shift(scenes):
    _, _, want, flow = scenes["shift"]
    share, worst = F.share_within(flow, want)
    print(f"shift (2.3, -1.7): {100 * share:.2f} % within 0.25 px, max error {worst:.3f} px")
    assert share >= 0.98


def test_reference_recovers_a_rotation_with_zoom_and_shift(scenes):
    _, _, want, flow = scenes["rotation"]
    share, worst = F.share_within(flow, want)
    print(f"3 degrees, zoom 1.03, shift (0.8, -0.5): {100 * share:.2f} % within 0.25 px, max error {worst:.3f} px")
    assert share >= 0.90


def test_identical_frames_give_exactly_zero_flow(scenes):
    tmpl = scenes["shift"][0]
    for dtype in (th.float64, th.float32):
        flow = F.estimate(tmpl, tmpl.clone(), dtype=dtype)
        assert tuple(flow.shape) == (1, 2, 64, 96) and flow.dtype == th.float32 and bool((flow == 0).all())


@pytest.mark.parametrize("name", ["shift", "rotation"])
def test_float32_restatement_stays_inside_the_cap(scenes, name):
    """what the GPU tests rely on when they allow 0.5 % of a case's pixels outside |a - b| <= 1e-4 + 1e-3 |ref|: on these inputs fp32 sums and
    fp32 step arithmetic move no more pixels than that"""
    tmpl, img, _, ref = scenes[name]
    got = F.estimate(tmpl, img, dtype=th.float32)
    diff = (got.double() - ref.double()).abs()
    outside = float((diff > 1e-4 + 1e-3 * ref.double().abs()).any(dim=1).double().mean())
    print(f"{name}: {100 * outside:.3f} % outside, largest difference {float(diff.max()):.3e}")
    assert outside <= 0.005 and float(diff.max()) <= 1.0


def test_one_level_is_what_estimate_runs_per_level(scenes):
    tmpl, img, _, ref = scenes["shift"]
    assert F.levels(64, 96, 4, 4) == 3  # 8 x 12 would be short of the 9-pixel window
    pyr = F.pyramid(th.cat([F.luminance(tmpl), F.luminance(img)]), 3)
    assert [tuple(p.shape[1:]) for p in pyr] == [(64, 96), (32, 48), (16, 24)]
    flow = None
    for p in reversed(pyr):
        flow = F.level(p[:1], p[1:], flow)
    assert th.equal(flow, ref)
    start = F.start_flow(th.ones(1, 2, 8, 12), 16, 24)
    assert th.equal(start, th.full((1, 2, 16, 24), 2.0))  # a constant flow doubles with the frame
    odd = F.start_flow(th.stack([th.full((1, 9, 17), 1.0), th.full((1, 9, 17), -1.0)], dim=1), 17, 33)
    assert th.allclose(odd[:, 0], th.full((1, 17, 33), 33 / 17)) and th.allclose(odd[:, 1], th.full((1, 17, 33), -17 / 9))


def test_level_rule_of_the_library_is_the_restatements():
    h = L.load()
    # 64 x 96, radius 4: 8 x 12 is short of 9 -> three levels; radius 3 keeps four; a 1 x 16 frame keeps one
    assert h.cgd_flow_levels(64, 96, 4, 4) == 3 and h.cgd_flow_levels(64, 96, 4, 3) == 4 and h.cgd_flow_levels(1, 16, 4, 4) == 1
    assert h.cgd_flow_levels(24, 40, 3, 3) == 2 and h.cgd_flow_levels(33, 47, 4, 4) == 3 and h.cgd_flow_levels(17, 33, 4, 4) == 2
    # sizes are halved upward: 65 -> 33 -> 17 -> 9 keeps a fourth level, 64 -> 32 -> 16 -> 8 does not
    assert h.cgd_flow_levels(65, 65, 8, 4) == 4 and h.cgd_flow_levels(64, 64, 8, 4) == 3 and h.cgd_flow_levels(512, 512, 4, 4) == 4
    for H in (1, 7, 9, 17, 18, 33, 64, 100, 513):
        for W in (1, 16, 35, 36, 96, 257):
            for levels in (1, 2, 4, 8):
                for radius in (1, 4, 7):
                    assert h.cgd_flow_levels(H, W, levels, radius) == F.levels(H, W, levels, radius), (H, W, levels, radius)
                    assert h.cgd_flow_scratch_floats(2, H, W, levels, radius) == F.scratch_floats(2, H, W, levels, radius)
    for bad in ((0, 8, 4, 4), (8, 0, 4, 4), (8, 8, 0, 4), (8, 8, 9, 4), (8, 8, 4, 0), (8, 8, 4, 8)):
        assert h.cgd_flow_levels(*bad) == 0 and h.cgd_flow_scratch_floats(1, *bad) == 0
    assert h.cgd_flow_scratch_floats(0, 8, 8, 4, 4) == 0 and h.cgd_flow_scratch_floats(1, 1 << 16, 1 << 15, 4, 4) == 0


def _params(levels=4, iters=4, radius=4, lam=1e-3, max_step=1.0):
    return L.FlowParams(levels, iters, radius, lam, max_step)


def test_flow_entries_refuse_bad_arguments_without_a_context():
    h = L.load()
    inf, nan = float("inf"), float("nan")
    ok = dict(tmpl=1 << 20, img=2 << 20, flow=3 << 20, scratch=8 << 20, B=2, C=3, H=16, W=24, p=_params())

    def estimate(**kw):
        a = {**ok, **kw}
        return h.cgd_flow_estimate(None, a["tmpl"], a["img"], a["flow"], a["scratch"], a["B"], a["C"], a["H"], a["W"],
                                   None if a["p"] is None else C.byref(a["p"]), None)

    assert estimate() == -3 and estimate(C=1) == -3 and estimate(p=_params(8, 16, 7, 1e-9, 100.0)) == -3 and estimate(p=_params(1, 1, 1)) == -3
    big = dict(H=1 << 16, W=(1 << 15) - 1, B=1, C=1, tmpl=1 << 40, img=2 << 40, flow=3 << 40, scratch=4 << 40)
    assert estimate(**big, p=_params(levels=1)) == -3 and estimate(**big) == -2  # from 2^30 pixels the pyramid's resize is out: one level only
    assert estimate(**dict(big, H=1 << 15), p=_params(levels=8)) == -3  # below 2^30 every level runs
    bad_params = [_params(levels=0), _params(levels=9), _params(iters=0), _params(iters=17), _params(radius=0), _params(radius=8),
                  _params(lam=0.0), _params(lam=-1e-3), _params(lam=nan), _params(lam=inf), _params(max_step=0.0), _params(max_step=-1.0),
                  _params(max_step=nan), _params(max_step=inf)]
    for kw in [dict(tmpl=None), dict(img=None), dict(flow=None), dict(scratch=None), dict(p=None),
               dict(tmpl=(1 << 20) + 2), dict(img=(2 << 20) + 1), dict(flow=(3 << 20) + 3), dict(scratch=(8 << 20) + 2),
               dict(B=0), dict(H=0), dict(W=-1), dict(H=1 << 16, W=1 << 15, B=1), dict(C=2), dict(C=4), dict(C=0),
               dict(flow=1 << 20), dict(flow=2 << 20), dict(flow=(1 << 20) + 4 * 2303), dict(flow=(2 << 20) - 4)] + [dict(p=p) for p in bad_params]:
        assert estimate(**kw) == -2, kw

    lv = dict(b=1 << 20, a=2 << 20, coarse=4 << 20, Hc=8, Wc=12, flow=3 << 20, B=2, H=16, W=24, p=_params())

    def level(**kw):
        a = {**lv, **kw}
        return h.cgd_op_flow_level(None, a["b"], a["a"], a["coarse"], a["Hc"], a["Wc"], a["flow"], a["B"], a["H"], a["W"],
                                   None if a["p"] is None else C.byref(a["p"]), None)

    assert level() == -3 and level(coarse=None, Hc=0, Wc=0) == -3
    for kw in [dict(b=None), dict(a=None), dict(flow=None), dict(p=None), dict(b=(1 << 20) + 1), dict(coarse=(4 << 20) + 2), dict(flow=(3 << 20) + 1),
               dict(B=0), dict(H=0), dict(W=0), dict(Hc=0), dict(Wc=-3), dict(flow=1 << 20), dict(flow=2 << 20), dict(flow=4 << 20),
               dict(flow=(2 << 20) + 4 * 767)] + [dict(p=p) for p in bad_params]:
        assert level(**kw) == -2, kw


def _settings(blend=1.0, alpha=0.01, beta=0.5, interp=1, border=2, clamp=0):
    return L.WarpFlow(blend, alpha, beta, interp, border, clamp)


def test_frame_warp_flow_refuses_bad_arguments_without_a_context():
    h = L.load()
    inf, nan = float("inf"), float("nan")
    ok = dict(src=1 << 20, flow=2 << 20, back=3 << 20, fb=4 << 20, dst=5 << 20, mask=6 << 20, fbatch=2, B=2, C=3, H=8, W=8, w=_settings())

    def call(**kw):
        a = {**ok, **kw}
        return h.cgd_frame_warp_flow(None, a["src"], a["flow"], a["back"], a["fb"], a["dst"], a["mask"], a["fbatch"], a["B"], a["C"], a["H"],
                                     a["W"], None if a["w"] is None else C.byref(a["w"]), None)

    assert call() == -3 and call(fbatch=1) == -3 and call(back=None, mask=None) == -3 and call(back=None, fb=None) == -3
    assert call(w=_settings(0.0, 0.0, 0.0, 0, 0, 1)) == -3 and call(w=_settings(0.5, 3.0, 100.0, 1, 1, 1)) == -3
    for kw in [dict(src=None), dict(flow=None), dict(dst=None), dict(w=None),
               dict(src=(1 << 20) + 2), dict(flow=(2 << 20) + 1), dict(back=(3 << 20) + 3), dict(fb=(4 << 20) + 2), dict(dst=(5 << 20) + 1),
               dict(mask=(6 << 20) + 2), dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(H=1 << 16, W=1 << 15, B=1, fbatch=1),
               dict(fbatch=0), dict(fbatch=3), dict(w=_settings(interp=2)), dict(w=_settings(interp=-1)), dict(w=_settings(border=3)),
               dict(w=_settings(border=-1)), dict(w=_settings(blend=-0.1)), dict(w=_settings(blend=1.5)), dict(w=_settings(blend=nan)),
               dict(w=_settings(alpha=-0.01)), dict(w=_settings(alpha=nan)), dict(w=_settings(alpha=inf)), dict(w=_settings(beta=-1.0)),
               dict(w=_settings(beta=nan)), dict(w=_settings(beta=inf)),
               dict(fb=None), dict(fb=None, back=None, w=_settings(blend=0.999)),  # no fallback: only with blend 1 and no flow_back
               dict(dst=1 << 20), dict(dst=2 << 20), dict(dst=3 << 20), dict(dst=4 << 20), dict(dst=(1 << 20) + 4 * 383), dict(dst=(2 << 20) - 4),
               dict(mask=1 << 20), dict(mask=2 << 20), dict(mask=5 << 20), dict(mask=(5 << 20) + 4 * 383)]:
        assert call(**kw) == -2, kw


def test_header_declares_and_library_exports_the_symbols():
    text = open(os.path.join(ROOT, "include", "cgd_mi355x.h")).read()
    for name in ("cgd_flow_levels", "cgd_flow_scratch_floats", "cgd_flow_estimate", "cgd_op_flow_level", "cgd_frame_warp_flow"):
        assert f" {name}(" in text and name in L.EXPORTED_SYMBOLS and hasattr(L.load(), name)
    assert "typedef struct cgd_flow_params {" in text and "typedef struct cgd_warp_flow {" in text
    assert C.sizeof(L.FlowParams) == 20 and [n for n, _ in L.FlowParams._fields_] == ["levels", "iters", "radius", "lam", "max_step"]
    assert C.sizeof(L.WarpFlow) == 24 and [n for n, _ in L.WarpFlow._fields_] == ["blend", "alpha", "beta", "interp", "border", "clamp"]
    build = open(os.path.join(ROOT, "clip-guided-diffusion_amd", "csrc", "build.sh")).read()
    assert " flow " in build


# ---- the clip ---------------------------------------------------------------------------------------------------------------------------
def test_frames_are_listed_in_name_order(tmp_path):
    d = tmp_path / "clip"
    d.mkdir()
    for name in ("0010.png", "0002.png", "0001.PNG", "notes.txt", "0003.jpg", "thumbs.db"):
        (d / name).write_bytes(b"")
    assert [os.path.basename(p) for p in an.list_video_frames(str(d))] == ["0001.PNG", "0002.png", "0003.jpg", "0010.png"]
    assert [os.path.basename(p) for p in an.list_video_frames(d)] == ["0001.PNG", "0002.png", "0003.jpg", "0010.png"]  # a path object
    assert [os.path.basename(p) for p in an.list_video_frames(str(d / "*.png"))] == ["0002.png", "0010.png"]
    assert an.list_video_frames(str(d / "*.gif")) == []
    given = [str(d / "0010.png"), str(d / "0001.PNG")]
    assert an.list_video_frames(given) == given and an.list_video_frames(tuple(given)) == given  # a list keeps its order
    t = th.zeros(3, 3, 8, 8)
    assert an.list_video_frames(t) is t
    for bad in (None, th.zeros(3, 1, 8, 8), th.zeros(3, 8, 8)):
        with pytest.raises(ValueError):
            an.list_video_frames(bad)


def test_a_frame_is_opened_and_resized_as_an_init_image_is(tmp_path):
    import numpy as np
    from PIL import Image
    rgb = (np.arange(12 * 20 * 3) % 251).astype(np.uint8).reshape(12, 20, 3)
    Image.fromarray(rgb).save(tmp_path / "a.png")
    got = an._video_frame([str(tmp_path / "a.png")], 0, 2, 12, 20, "cpu")
    assert tuple(got.shape) == (2, 3, 12, 20) and got.is_contiguous()
    want = th.from_numpy(rgb).float().div(255).permute(2, 0, 1).mul(2).sub(1)
    assert th.equal(got[0], want) and th.equal(got[1], want)
    small = an._video_frame([str(tmp_path / "a.png")], 0, 1, 6, 10, "cpu")
    pil = Image.open(tmp_path / "a.png").convert("RGB").resize((10, 6))
    assert th.equal(small[0], th.from_numpy(np.array(pil)).float().div(255).permute(2, 0, 1).mul(2).sub(1))
    clip = th.rand(3, 3, 12, 20) * 2 - 1
    assert th.equal(an._video_frame(clip, 2, 2, 12, 20, "cpu"), clip[2:3].expand(2, -1, -1, -1))
    with pytest.raises(ValueError, match="frames are"):
        an._video_frame(clip, 0, 1, 16, 16, "cpu")


# ---- refusals of the driver ---------------------------------------------------------------------------------------------------------------
def test_animate_refuses_video_arguments_before_anything_is_loaded(tmp_path, monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    for mod, name in ((clip_util, "load_clip"), (clip_util, "encode_text_prompt"), (script_util, "download_guided_diffusion"),
                      (script_util, "load_guided_diffusion"), (script_util, "load_lpips"), (mine, "ClipGuidance")):
        monkeypatch.setattr(mod, name, no_load)
    base = dict(prompts=["a cat"], device="cuda", timestep_respacing="ddim10")
    clip = th.zeros(3, 3, 64, 64)
    d = tmp_path / "clip"
    d.mkdir()
    for name in ("a.png", "b.png"):
        (d / name).write_bytes(b"")
    video = dict(mode="video", video_frames=clip)
    flat = th.ones(1, 1, 8, 8)
    cases = [
        # video mode takes no typed-in motion and no depth
        dict(video, zoom=1.02), dict(video, zoom="0:(1),2:(1.1)"), dict(video, angle=2), dict(video, translation_x=1), dict(video, translation_y="1:(3)"),
        dict(video, translation_z=1), dict(video, rotation_3d_x=1), dict(video, rotation_3d_y=-1), dict(video, rotation_3d_z=0.5), dict(video, fov=50),
        dict(video, depth=flat), dict(video, depth=lambda x: flat), dict(video, depth_iters=2), dict(video, near=0.1),
        dict(video, depth_model="dpt_large-midas-2f21e586.pt"),
        # the other modes take no video argument
        dict(video_frames=clip), dict(video_frames=str(d)), dict(flow_blend=0.9), dict(check_consistency=True), dict(flow_levels=3), dict(flow_iters=2),
        dict(flow_radius=5), dict(mode="3d", video_frames=clip), dict(mode="3d", check_consistency=True), dict(mode="2d", flow_blend=1.0),
        # frame 0 is the clip's
        dict(video, init_image="a.png"),
        # the clip: missing, too short, empty, of the wrong kind
        dict(mode="video"), dict(mode="video", video_frames=th.zeros(2, 3, 64, 64)), dict(mode="video", video_frames=str(d)),
        dict(mode="video", video_frames=str(d / "*.jpg")), dict(mode="video", video_frames=[]), dict(mode="video", video_frames=th.zeros(3, 1, 64, 64)),
        dict(mode="video", video_frames=str(tmp_path / "nowhere")),
        # the flow's settings
        dict(video, flow_blend=-0.1), dict(video, flow_blend=1.01), dict(video, flow_blend=float("nan")), dict(video, flow_levels=0),
        dict(video, flow_levels=9), dict(video, flow_levels=2.0), dict(video, flow_iters=0), dict(video, flow_iters=17), dict(video, flow_iters=True),
        dict(video, flow_radius=0), dict(video, flow_radius=8),
        # what the other modes refuse, video mode refuses
        dict(video, use_augs=True), dict(video, init_image="a.png::m.png"), dict(video, init_image="invert=a.png"),
        dict(video, init_image="upsample=a.png"), dict(video, init_image="ilvr8=a.png"), dict(video, prompts=["a cat=>a dog"]),
        dict(video, frames_skip=1.0), dict(video, border="zeros"), dict(video, interp="nearest"), dict(video, color_match=2),
    ]
    for kw in cases:
        with pytest.raises(ValueError):
            next(an.animate(3, **{**base, **kw}))
    with pytest.raises(ValueError):
        next(an.animate(0, **base, **video))
    with pytest.raises(ValueError, match="the clip has 3 frames"):
        next(an.animate(4, **base, **video))
    with pytest.raises(ValueError, match="zoom, fov: not with mode='video'"):
        next(an.animate(3, zoom=1.1, fov=60, **base, **video))
    with pytest.raises(ValueError, match="flow_blend, check_consistency: only with mode='video'"):
        next(an.animate(3, flow_blend=0.5, check_consistency=True, **base))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    from cgd_amd import shard
    if shard.world()[1] > 1:  # a sharded run
        with pytest.raises(ValueError, match="one process"):
            next(an.animate(3, **base, **video))


def test_cli_flags():
    a = an.build_parser().parse_args(["--frames", "3"])
    assert (a.mode, a.video_frames, a.flow_blend, a.check_consistency, a.flow_levels, a.flow_iters, a.flow_radius) == ("2d", None, 0.999, False, 4, 4, 4)
    a = an.build_parser().parse_args(["--frames", "3", "--mode", "video", "--video_frames", "clip/*.png", "--flow_blend", "0.9", "--check_consistency",
                                      "--flow_levels", "3", "--flow_iters", "2", "--flow_radius", "5"])
    assert (a.mode, a.video_frames, a.flow_blend, a.check_consistency, a.flow_levels, a.flow_iters, a.flow_radius) == (
        "video", "clip/*.png", 0.9, True, 3, 2, 5)
