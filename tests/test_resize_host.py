"""Host side of the resized cutouts (csrc/cutresize.hip): the float64 restatement (tests/resize_ref.py) against ResizeRight's own outputs
(tests/golden/reference_resize.npz), the kernels' weight routine through its host-only entry against the restatement, the draws, flags and
schedule of MakeCutoutsResized, the `cuts=` value of --clip_model, and ClipGuidance's launch order with a recording library.  No GPU needed."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import guidance as dg
from cgd_amd import lib
from tests import resize_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_resize.npz")
CASES = ["40_16", "23_16", "9_16", "16_16", "17_32", "37_32", "24x40_16"]


@pytest.fixture(scope="module")
def fx():
    return np.load(GOLDEN)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_resize_right(fx, case):
    x, y = th.as_tensor(fx[f"x_{case}"]), th.as_tensor(fx[f"y_{case}"])
    assert x.dtype == th.float64 and x.shape[:2] == (2, 3)
    m = y.shape[-1]
    grid = float((R.resize(x, m, m, reference_grid=True) - y).abs().max())
    exact = float((R.resize(x, m, m) - y).abs().max())
    print(f"{case}: |reference_grid - ResizeRight| {grid:.3e}, |exact - ResizeRight| {exact:.3e}")
    assert grid <= 1e-12
    assert exact <= 5e-4  # ResizeRight's float32 grid against exact geometry: recorded above, not a property of the kernels


def test_restatement_gradient_matches_resize_right_autograd(fx):
    x = th.as_tensor(fx["x_23_16"]).requires_grad_()
    d = th.as_tensor(fx["d_23_16"])
    g, = th.autograd.grad((R.resize(x, 16, 16, reference_grid=True) * d).sum(), x)
    assert float((g - th.as_tensor(fx["g_23_16"])).abs().max()) <= 1e-12


def test_border_rows_are_not_renormalised():
    for (n, m), want in {(37, 224): 0.60, (9, 16): 0.83, (40, 16): 0.93}.items():
        assert abs(R.matrix(n, m).sum(1).min() - want) < 0.005, (n, m)
    assert np.array_equal(R.matrix(16, 16), np.eye(16))


def host_weights(n, m):
    handle = lib.load()
    t = C.c_int(0)
    assert handle.cgd_cutouts_resize_weights(n, m, None, None, C.byref(t)) == 0
    w = np.empty((m, t.value), np.float32)
    left = np.empty(m, np.int32)
    assert handle.cgd_cutouts_resize_weights(n, m, w.ctypes.data, left.ctypes.data, C.byref(t)) == 0
    return left, t.value, w


@pytest.mark.parametrize("n,m", [(40, 16), (23, 16), (9, 16), (16, 16), (17, 32), (37, 32), (24, 16), (256, 224), (225, 224), (512, 224),
                                 (300, 224), (64, 224), (37, 224)])
def test_kernel_weight_routine_matches_the_exact_restatement(n, m):
    left, T, w = host_weights(n, m)
    left_ref, T_ref, w_ref = R.taps_exact(n, m)
    assert T == T_ref and np.array_equal(left, left_ref)
    err = np.abs(w - w_ref).max()
    print(f"{n}->{m}: T {T}, max weight error {err:.3e}")
    assert err <= 2e-6
    if m == n:  # identity: one unit tap per row
        assert all(w[o, o - left[o]] == 1.0 and np.count_nonzero(w[o]) == 1 for o in range(m))
    # the package's CPU restatement is the same operator
    assert float((dg.resize_matrix(n, m, th.float64) - th.as_tensor(R.matrix(n, m))).abs().max()) <= 1e-14


def test_weight_entry_rejects_bad_arguments():
    handle = lib.load()
    t = C.c_int(0)
    assert handle.cgd_cutouts_resize_weights(8, 4, None, None, None) == -3
    assert handle.cgd_cutouts_resize_weights(0, 4, None, None, C.byref(t)) == -2
    assert handle.cgd_cutouts_resize_weights(8, 0, None, None, C.byref(t)) == -2
    buf = (C.c_int32 * 4)()
    assert handle.cgd_cutouts_resize_weights(8, 4, None, buf, C.byref(t)) == -3
    assert handle.cgd_cutouts_resize_fwd(None, None, None, None, None, 1, 8, 8, 1, 4, 0, 0, None) == -3
    assert handle.cgd_cutouts_resize_bwd(None, None, None, None, None, None, 1, 8, 8, 1, 4, 0, 0, 0, None) == -3
    assert handle.cgd_cutouts_resize_scratch_floats(2, 64, 48, 5) == 5 * 2 * 3 * 64 * 48
    assert handle.cgd_cutouts_resize_scratch_floats(0, 64, 48, 5) == 0


# ---- MakeCutoutsResized ----------------------------------------------------------------------------------------------------------
def expected_inner(W, H, cs, count, pow_):
    """Hand-written draw order: size, ox, oy per cut on the global CPU generator."""
    out = []
    for _ in range(count):
        size = int(th.rand([]) ** pow_ * (min(H, W) - min(H, W, cs)) + min(H, W, cs))
        ox = th.randint(0, W - size + 1, ()).item()
        oy = th.randint(0, H - size + 1, ()).item()
        out.append((ox, oy, size, size))
    return out


def test_draw_order_and_flags():
    W, H, cs = 56, 40, 16
    mk = dg.MakeCutoutsResized(cs, overview=4, inner=12)
    th.manual_seed(5)
    recs = mk.draw(W, H)
    state = th.get_rng_state()
    th.manual_seed(5)
    inner = expected_inner(W, H, cs, 12, 0.5)
    assert th.equal(th.get_rng_state(), state)  # three draws per inner cut, none for the overview cuts
    assert recs[:4] == [(0, 0, W, H, 0), (0, 0, W, H, 1), (0, 0, W, H, 2), (0, 0, W, H, 3)]  # plain, gray, flip, gray + flip
    assert [r[:4] for r in recs[4:]] == inner
    assert [r[4] for r in recs[4:]] == [1, 1, 1] + [0] * 9  # i <= int(0.2 * 12) = 2
    assert all(cs <= r[2] <= min(W, H) and r[0] + r[2] <= W and r[1] + r[3] <= H for r in recs[4:])
    assert len({r[2] for r in recs[4:]}) > 3
    # fewer / more overview cuts
    assert [r[4] for r in dg.MakeCutoutsResized(cs, 2, 0).draw(W, H)] == [0, 1]
    assert [r[4] for r in dg.MakeCutoutsResized(cs, 6, 0).draw(W, H)] == [0] * 6
    # an image smaller than the cut size: every inner cut is the largest square
    assert all(r[2] == 12 for r in dg.MakeCutoutsResized(16, 0, 3).draw(12, 20))
    with pytest.raises(ValueError):
        dg.MakeCutoutsResized(cs, 0, 0)


def test_schedule_and_cache():
    mk = dg.MakeCutoutsResized(16, overview=1, inner=6, schedule=[(0.4, 4, 2), (0.7, 2, 4)])
    assert mk.counts(0.0) == (4, 2) and mk.counts(0.39) == (4, 2) and mk.counts(0.4) == (2, 4) and mk.counts(0.69) == (2, 4)
    assert mk.counts(0.7) == (1, 6) and mk.counts(1.0) == (1, 6)
    assert dg.MakeCutoutsResized(16, 3, 5).counts(0.2) == (3, 5)
    th.manual_seed(2)
    mk.cache_coordinates(48, 48)
    assert len(mk.cached_coords) == 6
    state = th.get_rng_state()
    a = mk.draw(48, 48, use_cache=True, num_cutouts_override=(4, 2))
    b = mk.draw(48, 48, use_cache=True, num_cutouts_override=(1, 6))
    assert th.equal(th.get_rng_state(), state)  # cached: no draw
    assert [r[:4] for r in a[4:]] == mk.cached_coords[:2] and [r[:4] for r in b[1:]] == mk.cached_coords
    assert [r[4] for r in a] == [0, 1, 2, 3, 1, 0] and [r[4] for r in b] == [0, 1, 1, 0, 0, 0, 0]
    assert len(mk.draw(48, 48, num_cutouts_override=3)) == 3


def test_forward_on_cpu_is_the_restatement_with_autograd():
    x = th.rand(2, 3, 40, 56, generator=th.Generator().manual_seed(1)).requires_grad_()
    mk = dg.MakeCutoutsResized(16, overview=4, inner=3)
    th.manual_seed(8)
    out = mk(x)
    assert out.shape == (7 * 2, 3, 16, 16) and out.requires_grad
    ref = R.cutouts(x.detach().double(), mk.last_coords, 16)
    assert float((out.detach().double() - ref).abs().max()) <= 1e-5
    out.sum().backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0


def test_resize_table_layout_and_refusals():
    recs = [(0, 0, 48, 40, 3), (5, 6, 16, 16, 1), (2, 3, 20, 20, 0), (1, 1, 9, 9, 0), (0, 0, 8, 8, 2)]
    table = dg.resize_table(recs, 40, 48)
    assert table[:5] == [(0, 0, 40, 48), (6, 5, 16, 16), (3, 2, 20, 20), (1, 1, 9, 9), (0, 0, 8, 8)]
    assert table[5:] == [(3, 1, 0, 0), (2, 0, 0, 0)]
    for bad in [(0, 0, 0, 8, 0), (0, 0, 8, 0, 0), (41, 0, 8, 8, 0), (0, 33, 8, 8, 0), (-1, 0, 8, 8, 0)]:
        with pytest.raises(ValueError):
            dg.resize_table([bad], 40, 48)


# ---- the `cuts=` value ------------------------------------------------------------------------------------------------------------
def test_cuts_value_parsing_and_refusals():
    from cgd import clip_util
    assert clip_util.split_cuts("ViT-B/32") == ("ViT-B/32", None)
    assert clip_util.split_cuts("ViT-B/32+cuts=4:12") == ("ViT-B/32", (4, 12, None))
    assert clip_util.split_cuts("cuts=2:6/0:16 + RN50+secondary=f.pth") == ("RN50+secondary=f.pth", (0, 16, [(0.4, 2, 6)]))
    for bad in ("ViT-B/32+cuts=4", "ViT-B/32+cuts=4:x", "ViT-B/32+cuts=", "ViT-B/32+cuts=-1:4", "ViT-B/32+cuts=0:0", "ViT-B/32+cuts=1:2/3:4/5:6",
                "ViT-B/32+cuts=1:2+cuts=3:4", "cuts=4:12", "cuts=4:12+secondary=f.pth", "ViT-B/32+cuts=4:12:1"):
        with pytest.raises(ValueError):
            clip_util.split_cuts(bad)
    with pytest.raises(ValueError):
        clip_util.split_cuts("ViT-B/32+cuts=4:12", progressive_cutout=True)
    with pytest.raises(ValueError):
        clip_util.split_cuts("ViT-B/32+cuts=4:12", use_augs=True)
    mk = clip_util.MakeCutoutsResized(224, *clip_util.split_cuts("ViT-B/32+cuts=2:6/0:16")[1][:2], schedule=[(0.4, 2, 6)])
    assert mk.counts(0.1) == (2, 6) and mk.counts(0.5) == (0, 16)


def test_generator_refuses_before_anything_is_loaded(monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    monkeypatch.setattr(clip_util, "load_clip", no_load)
    monkeypatch.setattr(script_util, "download_guided_diffusion", no_load)
    for kw in (dict(clip_model_name="ViT-B/32+cuts=4"), dict(clip_model_name="cuts=4:12"),
               dict(clip_model_name="ViT-B/32+cuts=4:12", progressive_cutout=True)):
        with pytest.raises(ValueError):
            next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", **kw))
    assert "cuts=OV:IN" in mine.build_parser().format_help()


# ---- ClipGuidance with a recording library --------------------------------------------------------------------------------------
def test_guidance_launch_order_and_cut_count_with_a_recording_library():
    calls = []

    class FakeLib:
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, args))
                return {"cgd_guidance_part_blocks": 32, "cgd_cutouts_resize_scratch_floats": 7}.get(name, 0)
            return fn

    ctx = types.SimpleNamespace(lib=FakeLib(), h=1, check=lambda rc: None, stream=lambda: 0)

    class Tower:
        def __init__(self, name, res, patch, dim):
            self.name, self.input_resolution, self.patch, self.out_dim = name, res, patch, dim

        def encode_image(self, img, layout=0, n=None, out=None):
            calls.append((f"{self.name}.encode_image", (layout, n, tuple(img.shape))))
            return out

        def dgrad(self, d_emb, d_img=None):
            calls.append((f"{self.name}.dgrad", (tuple(d_emb.shape),)))
            return d_img

    unet = types.SimpleNamespace(dgrad=lambda seed, out: out)
    diffusion = types.SimpleNamespace(num_timesteps=50)
    vit, rn = Tower("vit", 32, 8, 16), Tower("rn", 64, 0, 24)
    B, H, W = 2, 32, 48
    mk = dg.MakeCutoutsResized(32, overview=1, inner=4, schedule=[(0.4, 4, 2)])
    guid = dg.ClipGuidance(ctx, unet, [vit, rn], diffusion, [th.randn(2, 16), th.randn(2, 24)], [1.0, -0.25], 16, make_cutouts=mk)
    x = th.zeros(B, 3, H, W)
    for timestep, cutn in ((49, 6), (20, 5)):  # 2 % done: 4 + 2 cuts; 60 % done: 1 + 4
        del calls[:]
        guid.current_timestep = timestep
        th.manual_seed(3)
        guid.native(x, x.clone(), x.clone(), coef=None)
        names = [c[0] for c in calls]
        leg = ["cgd_cutouts_resize_fwd", "{}.encode_image", "cgd_spherical_loss", "{}.dgrad", "cgd_cutouts_resize_bwd"]
        assert names == ["cgd_cutouts_resize_scratch_floats"] + [n.format("vit") for n in leg] + [n.format("rn") for n in leg] + [
            "cgd_guidance_part_blocks", "cgd_guidance_combine", "cgd_grad_finish", "cgd_scalars"]
        by = {n: [c[1] for c in calls if c[0] == n] for n in set(names)}
        fwd, bwd = by["cgd_cutouts_resize_fwd"], by["cgd_cutouts_resize_bwd"]
        assert fwd[0][5:12] == (B, H, W, cutn, 32, 1, 8) and fwd[1][5:12] == (B, H, W, cutn, 64, 0, 0)  # each tower's own cut size
        assert fwd[0][2] == fwd[1][2] == bwd[0][2] and fwd[0][3] == fwd[0][2] + 16 * cutn == bwd[1][3]  # one table: boxes, then flags
        assert [c[-2] for c in bwd] == [0, 1] and bwd[0][6:13] == (B, H, W, cutn, 32, 1, 8)
        assert by["vit.encode_image"] == [(1, cutn * B, (cutn * B * 16, 3 * 64))] and by["rn.encode_image"] == [(0, cutn * B, (cutn * B, 3, 64, 64))]
        assert [c[6] for c in by["cgd_spherical_loss"]] == [cutn, cutn]  # the mean over cuts uses the step's count
        assert by["cgd_scalars"][0][2] == 2 * cutn * B
        recs = mk.last_coords
        assert len(recs) == cutn and [r[4] for r in recs[:4 if cutn == 6 else 1]] == ([0, 1, 2, 3] if cutn == 6 else [0])
    with pytest.raises(ValueError):
        dg.ClipGuidance(ctx, unet, [vit], diffusion, [th.randn(2, 16)], [1.0, -0.25], 16, make_cutouts=mk, progressive_cutout=True)
