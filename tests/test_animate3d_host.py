"""Host side of 3D animation (cgd_amd/animate.py, csrc/warp3d.hip): the camera's conventions, project / unproject as a round trip, the
float64 restatement (tests/warp3d_ref.py) against torch's grid_sample, the argument refusals of cgd_frame_warp3d (no context, no GPU), the
header and the export, animate's refusals before any load, the new command-line flags, and the driver's call sequence on recording fakes in
both modes.  No GPU."""
import ctypes as C
import math
import os
import sys
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import animate as an
from cgd_amd import lib as L
from tests import warp3d_ref as R3
from tests import warp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 40


def _cam(tx=0.0, ty=0.0, tz=0.0, rx=0.0, ry=0.0, rz=0.0, fov=40.0, h=H, w=W, **kw):
    return an.camera(tx, ty, tz, rx, ry, rz, fov, h, w, **kw)


# ---- the camera -----------------------------------------------------------------------------------------------------------------------
def test_camera_fields_and_refusals():
    c = _cam()
    assert c.R == (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0) and c.T == (0.0, 0.0, 0.0)
    assert all(math.copysign(1.0, v) == 1.0 for v in c.R + c.T)  # no negative zeros: the identity camera is the identity to the bit
    assert (c.cx, c.cy, c.z0, c.near) == (19.5, 11.5, 1.0, 0.05) and c.f == pytest.approx(12 / math.tan(math.radians(20)), rel=1e-15)
    assert _cam(tx=4, ty=-6, tz=10).T == (0.02, -0.03, -0.05)
    c = _cam(rx=11, ry=-23, rz=35)
    rows = [c.R[0:3], c.R[3:6], c.R[6:9]]
    for i in range(3):
        for j in range(3):
            assert sum(a * b for a, b in zip(rows[i], rows[j])) == pytest.approx(float(i == j), abs=1e-15)
    for bad in (dict(fov=0), dict(fov=180), dict(fov=-3), dict(fov=float("nan")), dict(tx=float("inf")), dict(rz=float("nan")), dict(z0=0),
                dict(near=0), dict(near=-1), dict(h=0)):
        with pytest.raises(ValueError):
            _cam(**bad)


def test_conventions_on_the_screen():
    cx, cy = 19.5, 11.5
    f = _cam().f
    # rotation_3d_z = 17 degrees is the 2D mode's angle = 17: the backward maps agree
    m = an.motion_matrix(1, 17, 0, 0, H, W)
    c = _cam(rz=17)
    for p in ((0.0, 0.0), (39.0, 23.0), (7.25, 19.5), (-12.0, 40.0)):
        for z in (0.5, 1.0, 3.0):
            s = an.unproject(c, p, z)
            assert abs(s[0] - (m[0] * p[0] + m[1] * p[1] + m[2])) <= 1e-9 and abs(s[1] - (m[3] * p[0] + m[4] * p[1] + m[5])) <= 1e-9
    # translation_x > 0 moves the content right by f tx / 200 / z pixels: near things faster
    for z in (0.5, 1.0, 3.0):
        q = an.project(_cam(tx=30), (10.0, 5.0), z)
        assert q[0] - 10.0 == pytest.approx(f * 30 / 200 / z, abs=1e-9) and q[1] == pytest.approx(5.0, abs=1e-9)
        q = an.project(_cam(ty=30), (10.0, 5.0), z)  # translation_y > 0: down
        assert q[1] - 5.0 == pytest.approx(f * 30 / 200 / z, abs=1e-9) and q[0] == pytest.approx(10.0, abs=1e-9)
    # translation_z > 0 flies forward: at flat depth z0 a magnification of z0 / (z0 - tz / 200) about the centre
    for z0, tz in ((1.0, 40.0), (2.0, -60.0), (0.5, 20.0)):
        q = an.project(_cam(tz=tz), (cx + 8, cy - 6), z0)
        mag = z0 / (z0 - tz / 200)
        assert q == pytest.approx((cx + 8 * mag, cy - 6 * mag), abs=1e-9)
        assert an.project(_cam(tz=tz), (cx, cy), z0) == pytest.approx((cx, cy), abs=1e-12)
    assert an.project(_cam(tz=40), (cx + 8, cy), 1.0)[0] > cx + 8  # forward magnifies
    # rotation_3d_y > 0: the camera turns right, the content moves left; rotation_3d_x > 0: the camera tilts up, the content moves down
    q = an.project(_cam(ry=5), (cx, cy), 1.0)
    assert q[0] == pytest.approx(cx - f * math.tan(math.radians(5)), abs=1e-9) and q[1] == pytest.approx(cy, abs=1e-12)
    q = an.project(_cam(rx=5), (cx, cy), 1.0)
    assert q[1] == pytest.approx(cy + f * math.tan(math.radians(5)), abs=1e-9) and q[0] == pytest.approx(cx, abs=1e-12)
    # rotation_3d_z > 0 turns the picture counter-clockwise: the right edge's midpoint goes up
    assert an.project(_cam(rz=90, h=33, w=33), (32.0, 16.0), 1.0) == pytest.approx((16.0, 0.0), abs=1e-9)


CAMERAS = [dict(), dict(tx=30), dict(tz=40), dict(rz=17), dict(tx=3, ty=-2, tz=10, rx=1, ry=2, rz=3), dict(ry=30), dict(rx=-12, tz=-25, fov=75),
           dict(tx=-80, ty=15, tz=60, rx=4, ry=-6, rz=170, fov=20)]


@pytest.mark.parametrize("motion", CAMERAS)
def test_project_after_unproject_is_the_identity(motion):
    c = _cam(**motion)
    for z in (0.5, 1.0, 3.0):
        for p in ((0.0, 0.0), (39.0, 23.0), (7.25, 19.5), (19.5, 11.5), (33.0, 2.0)):
            q = an.project(c, an.unproject(c, p, z), z)
            assert max(abs(q[0] - p[0]), abs(q[1] - p[1])) <= 1e-9, (motion, z, p, q)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restatement_positions_are_unproject():
    c = _cam(tx=3, ty=-2, tz=10, rx=1, ry=2, rz=3)
    sx, sy, clamped = R3.positions(c, H, W)
    assert clamped == 0 and tuple(sx.shape) == (1, H, W)
    for x, y in ((0, 0), (39, 23), (7, 19)):
        assert (float(sx[0, y, x]), float(sy[0, y, x])) == pytest.approx(an.unproject(c, (float(x), float(y)), 1.0), abs=1e-12)
    # a depth map: one step uses the destination pixel's own depth; an integer position reads the stored value
    D = th.linspace(0.6, 1.6, H * W, dtype=th.float64).view(1, 1, H, W)
    sx, sy, _ = R3.positions(c, H, W, D, iters=1)
    assert (float(sx[0, 19, 7]), float(sy[0, 19, 7])) == pytest.approx(an.unproject(c, (7.0, 19.0), float(D[0, 0, 19, 7])), abs=1e-12)
    grid = th.tensor([3.0, -5.0, 7.5, 100.0], dtype=th.float64)
    assert R3.depth_at(D[0, 0], grid, th.full_like(grid, 2.0)).tolist() == pytest.approx(
        [float(D[0, 0, 2, 3]), float(D[0, 0, 2, 0]), float(D[0, 0, 2, 7] + D[0, 0, 2, 8]) / 2, float(D[0, 0, 2, 39])], abs=1e-15)
    assert float(R3.depth_at(D[0, 0], th.tensor([3.0], dtype=th.float64), th.tensor([2.0], dtype=th.float64))) == float(D[0, 0, 2, 3])
    # flying past the scene: lambda meets the near plane, and the restatement says so
    assert R3.positions(_cam(tz=300), H, W)[2] == H * W


@pytest.mark.parametrize("interp", R.INTERPS)
@pytest.mark.parametrize("border,padding", [("replicate", "border"), ("reflect", "reflection")])
def test_flat_restatement_matches_grid_sample(interp, border, padding):
    th.manual_seed(0)
    B, h, w = 2, 13, 21
    src = th.randn(B, 3, h, w, dtype=th.float64)
    c = an.camera(25, -40, 30, 2, -3, 17, 40, h, w)
    sx, sy, clamped = R3.positions(c, h, w)
    assert clamped == 0
    want = th.nn.functional.grid_sample(src, R3.grid_sample_grid(sx, sy, h, w).expand(B, -1, -1, -1), mode=interp, padding_mode=padding,
                                        align_corners=True)
    err = float((R3.sample_fp64(src, sx, sy, interp, border) - want).abs().max())
    print(f"{interp} {border}: |restatement - grid_sample| {err:.3e}")
    assert err <= 1e-12


def test_flat_restatement_of_an_in_plane_camera_is_the_2d_restatement():
    th.manual_seed(1)
    src = th.randn(1, 2, H, W, dtype=th.float64)
    got, clamped = R3.warp3d_fp64(src, _cam(rz=17), interp="bicubic", border="wrap")
    assert clamped == 0
    assert float((got - R.warp_fp64(src, an.motion_matrix(1, 17, 0, 0, H, W), "bicubic", "wrap")).abs().max()) <= 1e-9


# ---- the C ABI's refusals (judged before the context: no GPU needed) ---------------------------------------------------------------------
def _abi_cam(R=(1, 0, 0, 0, 1, 0, 0, 0, 1), T=(0.1, 0, 0), f=20.0, cx=3.5, cy=3.5, z0=1.0, near=0.05, iters=1, interp=1, border=0, clamp=0):
    return L.Camera((C.c_double * 9)(*R), (C.c_double * 3)(*T), f, cx, cy, z0, near, iters, interp, border, clamp)


def test_frame_warp3d_refuses_bad_arguments_without_a_context():
    h = L.load()
    ok = dict(src=64, dst=4096, depth=8192, db=1, B=2, C=3, H=8, W=8, cam=_abi_cam())

    def call(**kw):
        a = {**ok, **kw}
        return h.cgd_frame_warp3d(None, a["src"], a["dst"], a["depth"], a["db"], a["B"], a["C"], a["H"], a["W"],
                                  None if a["cam"] is None else C.byref(a["cam"]), None)

    inf, nan = float("inf"), float("nan")
    c17, s17 = math.cos(math.radians(17)), math.sin(math.radians(17))
    # nothing to refuse: the missing context is what is left
    assert call() == -3 and call(db=2) == -3 and call(depth=None, db=0) == -3 and call(depth=None, db=7) == -3
    assert call(cam=_abi_cam(R=(c17, s17, 0, -s17, c17, 0, 0, 0, 1), iters=4, interp=0, border=2, clamp=1)) == -3
    assert call(cam=_abi_cam(T=(0, 0, 0))) == -3  # the identity camera, too
    assert call(H=1 << 16, W=(1 << 15) - 1, B=1, C=1, depth=None, dst=1 << 40) == -3
    for kw in (dict(src=None), dict(dst=None), dict(cam=None),
               dict(dst=64), dict(dst=8192), dict(dst=64 + 4 * 100), dict(dst=8192 - 4), dict(src=4096 + 4 * 383),  # dst over src or depth
               dict(src=66), dict(dst=4097), dict(depth=8194),
               dict(B=0), dict(C=-1), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15, depth=None, dst=1 << 40),
               dict(cam=_abi_cam(interp=2)), dict(cam=_abi_cam(interp=-1)), dict(cam=_abi_cam(border=3)), dict(cam=_abi_cam(border=-1)),
               dict(cam=_abi_cam(iters=0)), dict(cam=_abi_cam(iters=5)),
               dict(cam=_abi_cam(R=(1, 0, 0, 0, nan, 0, 0, 0, 1))), dict(cam=_abi_cam(T=(0, inf, 0))), dict(cam=_abi_cam(f=nan)),
               dict(cam=_abi_cam(cx=inf)), dict(cam=_abi_cam(cy=-inf)), dict(cam=_abi_cam(z0=nan)), dict(cam=_abi_cam(near=inf)),
               dict(cam=_abi_cam(f=0.0)), dict(cam=_abi_cam(f=-20.0)), dict(cam=_abi_cam(z0=0.0)), dict(cam=_abi_cam(z0=-1.0)),
               dict(cam=_abi_cam(near=0.0)), dict(cam=_abi_cam(near=-0.05)),
               dict(cam=_abi_cam(R=(1, 0, 0, 0, 1 + 1e-8, 0, 0, 0, 1))), dict(cam=_abi_cam(R=(1, 1e-8, 0, 0, 1, 0, 0, 0, 1))),
               dict(cam=_abi_cam(R=(2, 0, 0, 0, 0.5, 0, 0, 0, 1))), dict(cam=_abi_cam(R=(1, 0, 0, 0, 1, 0, 0, 0, -1))),  # a mirror
               dict(cam=_abi_cam(R=(0,) * 9)),
               dict(db=0), dict(db=3), dict(db=-1)):
        assert call(**kw) == -2, kw
    assert call(cam=_abi_cam(R=(1, 1e-10, 0, 0, 1, 0, 0, 0, 1))) == -3  # inside the 1e-9 of the orthonormality test


def test_header_declares_and_library_exports_the_symbol():
    text = open(os.path.join(ROOT, "include", "cgd_mi355x.h")).read()
    assert "int cgd_frame_warp3d(cgd_ctx* ctx, const float* src, float* dst, const float* depth, int depth_batch, int B, int C, int H, int W," in text
    assert "typedef struct cgd_camera {" in text and "double R[9], T[3], f, cx, cy, z0, near;" in text
    assert "cgd_frame_warp3d" in L.EXPORTED_SYMBOLS and hasattr(L.load(), "cgd_frame_warp3d")
    assert C.sizeof(L.Camera) == 17 * 8 + 4 * 4
    assert [n for n, _ in L.Camera._fields_] == ["R", "T", "f", "cx", "cy", "z0", "near", "iters", "interp", "border", "clamp"]


# ---- refusals of the driver -------------------------------------------------------------------------------------------------------------
def test_animate_refuses_mode_arguments_before_anything_is_loaded(monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    for mod, name in ((clip_util, "load_clip"), (clip_util, "encode_text_prompt"), (script_util, "download_guided_diffusion"),
                      (script_util, "load_guided_diffusion"), (script_util, "load_lpips"), (mine, "ClipGuidance")):
        monkeypatch.setattr(mod, name, no_load)
    base = dict(prompts=["a cat"], device="cuda", timestep_respacing="ddim10")
    flat = th.ones(1, 1, 8, 8)
    for kw in (dict(mode="4d"), dict(mode=None), dict(mode="3D"),
               # 3D mode takes no zoom / angle
               dict(mode="3d", zoom=1.02), dict(mode="3d", zoom="0:(1),2:(1.1)"), dict(mode="3d", angle=2), dict(mode="3d", angle="1:(3)"),
               # 2D mode (the default) takes no 3D-only argument
               dict(translation_z=1), dict(rotation_3d_x="0:(0),2:(1)"), dict(rotation_3d_y=-1), dict(rotation_3d_z=0.5), dict(fov=50),
               dict(depth=flat), dict(depth=lambda x: flat), dict(depth_iters=2), dict(near=0.1), dict(mode="2d", translation_z=1),
               dict(mode="3d", depth_iters=0), dict(mode="3d", depth_iters=5), dict(mode="3d", depth_iters=1.5), dict(mode="3d", depth_iters=True),
               dict(mode="3d", fov=0), dict(mode="3d", fov=180), dict(mode="3d", fov="0:(40),2:(200)"), dict(mode="3d", fov="0:(-10),1:(40)"),
               dict(mode="3d", near=0), dict(mode="3d", near=float("nan")), dict(mode="3d", translation_z="0:1"),
               dict(mode="3d", depth="midas"), dict(mode="3d", depth=th.ones(8, 8, 8)),
               # what 2D mode refuses, 3D mode refuses
               dict(mode="3d", use_augs=True), dict(mode="3d", init_image="a.png::m.png"), dict(mode="3d", frames_skip=1.0)):
        with pytest.raises(ValueError):
            next(an.animate(3, **{**base, **kw}))
    with pytest.raises(ValueError, match="translation_z.*rotation_3d_z"):
        next(an.animate(3, mode="3d", zoom=1.1, **base))
    with pytest.raises(ValueError, match="rotation_3d_y, fov: only with mode='3d'"):
        next(an.animate(3, rotation_3d_y=1, fov=60, **base))


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_flags(tmp_path, monkeypatch):
    a = an.build_parser().parse_args(["--frames", "3"])
    assert (a.mode, a.translation_z, a.rotation_3d_x, a.rotation_3d_y, a.rotation_3d_z, a.fov, a.depth_fn, a.depth_iters, a.near) == (
        "2d", "0", "0", "0", "0", "40", None, 1, 0.05)
    a = an.build_parser().parse_args(["--frames", "9", "--mode", "3d", "--translation_z", "0:(4)", "--rotation_3d_x", "-1", "--rotation_3d_y",
                                      "0:(0),8:(2)", "--rotation_3d_z", "0.25", "--fov", "55", "--depth_fn", "my_depth:estimate", "--depth_iters",
                                      "3", "--near", "0.1", "--translation_x", "2"])
    assert (a.mode, a.translation_z, a.rotation_3d_x, a.rotation_3d_y, a.rotation_3d_z, a.fov, a.depth_fn, a.depth_iters, a.near) == (
        "3d", "0:(4)", "-1", "0:(0),8:(2)", "0.25", "55", "my_depth:estimate", 3, 0.1)
    assert a.translation_x == "2" and a.zoom == "1.0" and a.angle == "0"
    with pytest.raises(SystemExit):
        an.build_parser().parse_args(["--frames", "3", "--mode", "4d"])
    # the flags of 2D mode parse as they did
    a = an.build_parser().parse_args(["--frames", "3", "--zoom", "0:(1.02)", "--fixed_seed", "--prompts_at", "1=a", "--prompts_at", "2=b"])
    assert a.frames == 3 and a.zoom == "0:(1.02)" and a.border == "wrap" and a.interp == "bicubic" and a.frames_skip == 0.6
    assert a.frames_scale == 1500 and a.color_match == 0.0 and a.fixed_seed and a.prompts_at == ["1=a", "2=b"]
    assert (a.angle, a.translation_x, a.translation_y) == ("0", "0", "0")
    # --depth_fn MODULE:FUNCTION
    (tmp_path / "my_depth_mod.py").write_text("def estimate(x):\n    return x[:, :1] * 0 + 1\n\nNOT_A_FUNCTION = 3\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    fn = an.load_depth_fn("my_depth_mod:estimate")
    assert callable(fn) and fn.__name__ == "estimate" and an.load_depth_fn(None) is None
    for bad in ("my_depth_mod", "my_depth_mod:", ":estimate", "my_depth_mod:NOT_A_FUNCTION", "my_depth_mod:missing"):
        with pytest.raises(ValueError):
            an.load_depth_fn(bad)
    sys.modules.pop("my_depth_mod", None)


# ---- the driver on recording fakes --------------------------------------------------------------------------------------------------------
SHAPE = (2, 3, 128, 144)


def _fakes(monkeypatch, tmp_path, events):
    """The fake device objects of tests/test_animate_host.py's sequence test, with ops.frame_warp3d recorded as well."""
    from cgd import cgd as mine
    from cgd import clip_util, script_util
    from cgd_amd import ops
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)

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

    def fake_warp3d(ctx, src, camera, depth, interp, border, clamp, iters):
        events.append(("warp3d", ctx, src.clone(), camera, depth, interp, border, clamp, iters))
        return src + 2.0

    def fake_stats(ctx, x):
        events.append(("stats", x.clone()))
        return th.zeros(x.shape[0], 3, 2)

    def fake_match(ctx, x, stats_ref, amount, clamp):
        events.append(("match", amount, clamp))
        return x.add_(0.5)

    monkeypatch.setattr(ops, "frame_warp", fake_warp)
    monkeypatch.setattr(ops, "frame_warp3d", fake_warp3d)
    monkeypatch.setattr(ops, "channel_stats", fake_stats)
    monkeypatch.setattr(ops, "color_match", fake_match)


def _run_kw(tmp_path, name):
    return dict(prompts=["a boat"], image_size=128, batch_size=2, num_cutouts=4, timestep_respacing="ddim10", seed=11,
                prefix_path=str(tmp_path / name), checkpoints_dir=str(tmp_path / "ck"), device="cuda", progress=False, width_offset=16)


def test_3d_mode_calls_frame_warp3d_once_per_later_frame_with_the_callables_depth(tmp_path, monkeypatch):
    events = []
    _fakes(monkeypatch, tmp_path, events)
    asked = []

    def depth_fn(x0):
        asked.append(x0.clone())
        events.append(("depth",))
        return th.full((2, 1, 128, 144), 1.0 + len(asked), dtype=th.float64)  # any float type: the driver hands fp32 to the kernel

    items = list(an.animate(3, mode="3d", translation_x="0:(0),2:(4)", translation_y=-3, translation_z="0:(0),2:(10)", rotation_3d_x=1,
                            rotation_3d_y="0:(0),2:(2)", rotation_3d_z=-0.5, fov="0:(40),2:(60)", depth=depth_fn, depth_iters=3, near=0.1,
                            border="reflect", interp="bilinear", frames_skip=0.6, frames_scale=1500, color_match=0.25, **_run_kw(tmp_path, "out")))
    kinds = [e[0] for e in events]
    assert "warp" not in kinds and kinds.count("warp3d") == 2 and kinds.count("depth") == 2
    assert kinds.count("load_clip") == kinds.count("load_unet") == kinds.count("load_lpips") == kinds.count("guidance") == 1
    warps, inits, loops = ([e for e in events if e[0] == k] for k in ("warp3d", "set_init", "loop"))
    # the previous frame's last sample is warped; the callable saw its last pred_xstart, as (B,3,H,W) in [0, 1]
    assert th.equal(warps[0][2], th.full(SHAPE, 0.125)) and th.equal(warps[1][2], th.full(SHAPE, 0.25))
    assert th.equal(asked[0], th.full(SHAPE, 0.125)) and th.equal(asked[1], th.full(SHAPE, 0.25))  # (-0.75 + 1) / 2, (-0.5 + 1) / 2
    for k, w in enumerate(warps):
        assert w[1] == "ctx" and w[5:] == ("bilinear", "reflect", True, 3)
        assert w[4].dtype == th.float32 and th.equal(w[4], th.full((2, 1, 128, 144), 2.0 + k))
    assert warps[0][3] == an.camera(2.0, -3.0, 5.0, 1.0, 1.0, -0.5, 50.0, 128, 144, near=0.1)
    assert warps[1][3] == an.camera(4.0, -3.0, 10.0, 1.0, 2.0, -0.5, 60.0, 128, 144, near=0.1)
    # the rest of the frame step is the 2D mode's: colour match, set_init, the loop from the warped frame with 6 of 10 steps skipped
    assert [e[1:] for e in events if e[0] == "match"] == [(0.25, True)] * 2 and kinds.count("stats") == 1
    assert [(e[1], e[2]) for e in loops] == [(SHAPE, 0), (SHAPE, 6), (SHAPE, 6)] and loops[0][3] is None
    for k in (0, 1):
        assert th.equal(inits[k][1], th.full(SHAPE, 0.125 * (k + 1) + 2.5)) and inits[k][2] == 1500 and th.equal(loops[k + 1][3], inits[k][1])
    assert [e[1] for e in events if e[0] == "seed"] == [11, 12, 13]
    at = kinds.index("warp3d")
    assert kinds[at - 2:at + 4] == ["seed", "depth", "warp3d", "match", "set_init", "loop"]
    assert [(k, b, os.path.relpath(p, tmp_path / "out")) for k, b, p in items] == [
        (k, b, os.path.join("a_boat", f"{b:02}", f"{k:04}.png")) for k in range(3) for b in (0, 1)]
    assert all(os.path.isfile(p) for _, _, p in items)

    # flat depth, and a tensor given once: no callable is asked, the kernel gets None / the tensor
    for depth, want in ((None, None), (th.full((128, 144), 0.75), th.full((1, 1, 128, 144), 0.75))):
        del events[:]
        list(an.animate(2, mode="3d", translation_z=8, depth=depth, **_run_kw(tmp_path, "o2")))
        (w,) = [e for e in events if e[0] == "warp3d"]
        assert (w[4] is None) if want is None else th.equal(w[4], want)
        assert w[3] == an.camera(0.0, 0.0, 8.0, 0.0, 0.0, 0.0, 40.0, 128, 144) and w[5:] == ("bicubic", "wrap", True, 1)
        assert "warp" not in [e[0] for e in events]


def test_default_mode_makes_the_calls_it_made(tmp_path, monkeypatch):
    events = []
    _fakes(monkeypatch, tmp_path, events)
    kw = dict(zoom="0:(1.0),2:(1.5)", angle=0.0, translation_x="0:(0),2:(4)", translation_y=0, border="reflect", interp="bilinear",
              frames_skip=0.6, frames_scale=1500, color_match=0.25)
    list(an.animate(3, **kw, **_run_kw(tmp_path, "a")))
    first = [e[0] for e in events]
    assert "warp3d" not in first and first.count("warp") == 2
    warps = [e for e in events if e[0] == "warp"]
    assert warps[0][3] == an.motion_matrix(1.25, 0.0, 2.0, 0.0, 128, 144) and warps[1][3] == an.motion_matrix(1.5, 0.0, 4.0, 0.0, 128, 144)
    assert all(w[1] == "ctx" and w[4:] == ("bilinear", "reflect", True) for w in warps)
    per_frame = ["seed", "warp", "match", "set_init", "loop"]
    assert first[first.index("loop"):] == ["loop", "stats"] + per_frame * 2
    del events[:]
    list(an.animate(3, mode="2d", translation_z=0, rotation_3d_x="0:(0)", fov=40, depth=None, depth_iters=1, near=0.05, **kw, **_run_kw(tmp_path, "b")))
    assert [e[0] for e in events] == first  # the defaults, spelled out, change nothing


@pytest.mark.parametrize("bad,why", [(lambda x: th.ones(2, 1, 64, 144), "shape"), (lambda x: th.ones(3, 1, 128, 144), "shape"),
                                     (lambda x: th.ones(2, 3, 128, 144), "shape"), (lambda x: None, "tensor"),
                                     (lambda x: th.full((2, 1, 128, 144), float("nan")), "finite"),
                                     (lambda x: th.ones(1, 1, 128, 144).index_fill_(3, th.tensor([5]), float("inf")), "finite"),
                                     (lambda x: th.zeros(2, 1, 128, 144), "positive"), (lambda x: -th.ones(128, 144), "positive")])
def test_a_bad_depth_raises_naming_the_frame(tmp_path, monkeypatch, bad, why):
    events = []
    _fakes(monkeypatch, tmp_path, events)
    calls = []

    def depth_fn(x0):
        calls.append(1)
        return th.ones(2, 1, 128, 144) if len(calls) == 1 else bad(x0)

    with pytest.raises(ValueError, match=f"frame 2.*{why}"):
        list(an.animate(3, mode="3d", translation_z=5, depth=depth_fn, **_run_kw(tmp_path, "bad")))
    assert [e[0] for e in events].count("warp3d") == 1  # frame 1 went through
    # a tensor given once is judged when the frame size is known, as frame 0's
    with pytest.raises(ValueError, match="frame 0.*shape"):
        list(an.animate(3, mode="3d", translation_z=5, depth=th.ones(1, 1, 64, 64), **_run_kw(tmp_path, "bad2")))
