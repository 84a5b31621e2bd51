"""CPU tests of windowed sampling: the planner (cgd_amd/windows.py: window origins, normalised weight tables) against its two rules and
against the restatement of tests/window_ref.py, the adjointness of that restatement's gather / merge pair, the '+windows=' suffix parser
and what it and the generator refuse before anything is loaded, the torch reference module, and the C ABI's new entries."""
import os
import re

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd.script_util import split_threshold, split_windows
from cgd_amd import lib as L
from cgd_amd import windows
from tests import window_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (L, S, stride, wrap) -> origins: the flush-last rule, the wrap rule, and a wrapped axis of the window's own length
ORIGIN_CASES = [((40, 16, 16, False), [0, 16, 24]), ((32, 16, 8, True), [0, 8, 16, 24]), ((16, 16, 8, True), [0, 8])]
# frames (H, W, S, stride, wrap) of the op-level GPU tests plus the model-level ones
PLANS = [(40, 24, 16, 16, ""), (32, 32, 16, 8, "xy"), (16, 32, 16, 8, "y"), (48, 64, 32, 16, ""), (32, 64, 32, 16, "x")]


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,expect", ORIGIN_CASES)
def test_window_origins_follow_the_flush_last_and_the_wrap_rule(case, expect):
    assert windows.window_origins(*case) == expect
    assert wr.origins(*case) == expect


def test_window_origins_more_cases_and_refusals():
    assert windows.window_origins(16, 16, 8) == [0]                       # the frame is the window
    assert windows.window_origins(256, 256, 128, True) == [0, 128]         # ... and wraps: two rolled copies
    assert windows.window_origins(512, 256, 128) == [0, 128, 256]
    assert windows.window_origins(1024, 256, 128) == [0, 128, 256, 384, 512, 640, 768]
    assert windows.window_origins(72, 32, 24) == [0, 24, 40]               # the last stride is shortened, never lengthened
    for H, W, S, stride, wrap in PLANS:
        assert windows.window_origins(H, S, stride, "y" in wrap) == wr.origins(H, S, stride, "y" in wrap)
        assert windows.window_origins(W, S, stride, "x" in wrap) == wr.origins(W, S, stride, "x" in wrap)
    bad = [(40, 16, 12, False), (40, 16, 0, False), (40, 16, -8, False), (40, 16, 8.0, False),  # the stride: a positive multiple of 8
           (44, 16, 8, False), (40, 12, 8, False),                                                # ... and so are L and S
           (8, 16, 8, False),                                                                     # a window larger than the axis
           (40, 16, 24, False),                                                                   # a stride that leaves gaps
           (40, 16, 16, True),                                                                    # wrap: the stride does not divide L
           (8 * 17, 8, 8, True), (8 * 18, 8, 8, False)]                                           # more than 16 windows
    for case in bad:
        with pytest.raises(ValueError):
            windows.window_origins(*case)
    assert len(windows.window_origins(8 * 16, 8, 8, True)) == 16


@pytest.mark.parametrize("profile", windows.PROFILES)
def test_tables_are_a_partition_of_unity_in_fp32(profile):
    """The fp32 tables, summed in fp64 over the windows that cover a pixel, give 1 per axis and (their products) per pixel of the frame.
    Bound: every entry is an fp64 value in (0, 1] rounded to fp32, a relative error of at most 2^-24; the entries over a pixel sum to 1, so
    an axis sum is off by at most 2^-24 and a product of two axis sums by 2^-23 (+ 2^-48): 2 ulp of fp32 at 1, 'a few ulp'."""
    for H, W, S, stride, wrap in PLANS:
        plan = windows.WindowPlan(H, W, S, stride, wrap, feather=profile == "feather")
        assert plan.ay.dtype == th.float32 and tuple(plan.ay.shape) == (plan.ny, S) and tuple(plan.ax.shape) == (plan.nx, S)
        assert (plan.ay > 0).all() and (plan.ax > 0).all() and plan.n == plan.ny * plan.nx
        ones = th.ones(plan.n, 1, S, S, dtype=th.float64)
        for tab, orig, Lx in ((plan.ay, plan.oy, H), (plan.ax, plan.ox, W)):
            total = th.zeros(Lx, dtype=th.float64)
            for k, o in enumerate(orig):
                total[(o + th.arange(S)) % Lx] += tab[k].double()
            assert float((total - 1).abs().max()) <= 2.0 ** -24, (H, W, wrap, profile)
            assert float((tab.double() - wr.tables(orig, Lx, S, profile)).abs().max()) <= 2.0 ** -24  # the restatement, rounded
        frame = wr.merge(ones, plan.oy, plan.ox, H, W, plan.ay.double(), plan.ax.double())
        assert float((frame - 1).abs().max()) <= 2.0 ** -23 + 2.0 ** -40, (H, W, wrap, profile)
    with pytest.raises(ValueError):
        windows.window_tables([0, 8], 24, 16, "gauss")


def test_uniform_tables_are_reciprocal_cover_counts_and_feather_vanishes_toward_covered_edges():
    a = windows.window_tables([0, 16, 24], 40, 16)
    assert th.equal(a[0], th.ones(16)) and th.equal(a[1], th.cat([th.ones(8), th.full((8,), 0.5)]))
    assert th.equal(a[2], th.cat([th.full((8,), 0.5), th.ones(8)]))
    f = windows.window_tables([0, 8, 16, 24], 32, 16, "feather")
    assert th.allclose(f, f[0].expand(4, 16)) and float(f[0, 0]) < 0.02 and float(f[0, 7]) > 0.5  # every window alike under wrap
    one = windows.window_tables([0], 16, 16, "feather")
    assert th.equal(one, th.ones(1, 16))  # a lone window carries the whole weight whatever the profile


# ---- the restatement's pair is adjoint -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_gather_and_merge_are_adjoint_in_fp64(weighted):
    gen = th.Generator().manual_seed(5)
    for H, W, S, stride, wrap in PLANS[:3]:
        oy, ox = wr.origins(H, S, stride, "y" in wrap), wr.origins(W, S, stride, "x" in wrap)
        ay, ax = (wr.tables(oy, H, S, "feather"), wr.tables(ox, W, S, "feather")) if weighted else (None, None)
        for B, C in ((1, 3), (2, 6)):
            f = th.randn(B, C, H, W, generator=gen, dtype=th.float64)
            w = th.randn(B * len(oy) * len(ox), C, S, S, generator=gen, dtype=th.float64)
            lhs = (wr.merge(w, oy, ox, H, W, ay, ax) * f).sum()
            rhs = (w * wr.gather(f, oy, ox, S, ay, ax)).sum()
            scale = (w.abs().sum() * f.abs().max()).item()
            assert abs(float(lhs - rhs)) <= 1e-14 * scale
            assert abs(float(lhs)) > 1e-3  # not a comparison of zeros
        if weighted:  # merge(gather(x)) with the normalised weights on the merge alone gives x back
            back = wr.merge(wr.gather(f, oy, ox, S), oy, ox, H, W, ay, ax)
            assert float((back - f).abs().max()) <= 1e-14


# ---- the '+windows=' suffix ------------------------------------------------------------------------------------------------------------
def test_split_windows_parses_every_accepted_form():
    for plain in ("250", "ddim50", "plms25", "dpm20+thr=0.995:1.5"):
        assert split_windows(plain) == (plain, None)
        assert split_windows(plain, 256, 0, 256) == (plain, None)
    assert split_windows("250+windows=128") == ("250", (128, "", False))
    assert split_windows("ddim50+windows=64:wrapx") == ("ddim50", (64, "x", False))
    assert split_windows("plms25+windows=8:wrapy") == ("plms25", (8, "y", False))
    assert split_windows("1000+windows=256:wrap") == ("1000", (256, "xy", False))
    assert split_windows("250+windows=128:feather") == ("250", (128, "", True))
    assert split_windows("250+windows=128:wrapx:feather") == ("250", (128, "x", True))
    assert split_windows("250+windows=128:wrapx", 256, 0, 256) == ("250", (128, "x", False))
    assert split_windows("250+windows=128:wrap", 256, 0, 0) == ("250", (128, "xy", False))  # the frame is the window, rolled
    assert split_windows("250+windows=96:wrapy", 256, 128, 8, "a.png::m.png", "ViT-B/32+secondary=s.pth") == ("250", (96, "y", False))
    assert split_windows("250+windows=128", 256, 0, 256, "ilvr8=a.png") == ("250", (128, "", False))
    # the last suffix: what is left still carries '+thr=' for split_threshold
    spec, win = split_windows("dpm20+thr=0.995:1.5+windows=128:wrapx:feather", 256, 0, 256)
    assert spec == "dpm20+thr=0.995:1.5" and win == (128, "x", True)
    assert split_threshold(spec) == ("dpm20", (0.995, 1.5))


@pytest.mark.parametrize("bad", ["250+windows=", "250+windows=abc", "250+windows=128:", "250+windows=128:wrapz", "250+windows=128:feather:wrapx",
                                 "250+windows=128:wrapx:wrapy", "250+windows=128:wrapx:feather:feather", "250+windows=12.5", "+windows=128",
                                 "250+windows=-8", "250+windows=0", "250+windows=12", "250+windows=100"])
def test_split_windows_refuses_malformed_suffixes_and_strides(bad):
    with pytest.raises(ValueError):
        split_windows(bad)


@pytest.mark.parametrize("value,kw", [
    ("250+windows=264", {}),                                              # a stride larger than image_size
    ("250+windows=128", dict(width_offset=100)),                          # a frame side that is no multiple of 8
    ("250+windows=128", dict(height_offset=4)),
    ("250+windows=96:wrapx", dict(width_offset=256)),                     # wrap on an axis the stride does not divide (512 % 96)
    ("250+windows=96:wrapy", dict(width_offset=32)),                      # ... (256 % 96), the other axis does not help
    ("250+windows=96:wrap", dict(height_offset=128)),
    ("250+windows=128", dict(init_image="upsample=a.png")),
    ("250+windows=128", dict(init_image="upsample=a.png::m.png")),
    ("ddim50+windows=128", dict(init_image="invert=a.png")),
    ("250+windows=128", dict(clip_model_name="ViT-B/32+classifier=c.pt:3")),
])
def test_windows_refusals_before_anything_is_loaded(tmp_path, value, kw):
    with pytest.raises(ValueError):
        split_windows(value, 256, kw.get("height_offset", 0), kw.get("width_offset", 0), kw.get("init_image"), kw.get("clip_model_name", ""))
    from cgd.cgd import clip_guided_diffusion
    with pytest.raises(ValueError):
        next(clip_guided_diffusion(prompts=["x"], image_size=256, timestep_respacing=value, device="cuda", checkpoints_dir=str(tmp_path / "none"),
                                   prefix_path=str(tmp_path / "out"), **kw))
    assert not (tmp_path / "none").exists() and not (tmp_path / "out").exists()


def test_the_respace_help_names_the_suffix():
    from cgd.cgd import build_parser
    text = build_parser().format_help()
    assert "+windows=STRIDE" in text and "wrapx" in text and "feather" in text


# ---- the reference module -------------------------------------------------------------------------------------------------------------
def test_windowed_ref_with_one_window_covering_the_frame_is_the_bare_module():
    from tests import parity_checks as pc
    unet = pc.oracle_unet("mini")
    gen = th.Generator().manual_seed(3)
    x, t, y = th.randn(2, 3, 32, 32, generator=gen), th.tensor([417.0, 20.0]), th.tensor([3, 7])
    bare = unet(x, t, y)
    for feather in (False, True):
        ref = wr.WindowedRef(unet, 32, 16, "", feather)
        assert ref.plan(32, 32)[:2] == ([0], [0]) and ref.num_classes == 10
        assert th.equal(ref(x, t, y), bare)


def test_windowed_ref_averages_window_outputs_of_a_toy_model():
    """a model that returns its input on six channels: the average of the windows is the frame itself; and one that returns the window's
    own row coordinate: the frame then holds the weighted mean of the coordinates its covering windows give a pixel"""
    class Echo(th.nn.Module):
        def forward(self, x, ts, y=None):
            return th.cat([x, x * ts.view(-1, 1, 1, 1)], 1)

    x = th.randn(2, 3, 40, 24, generator=th.Generator().manual_seed(1), dtype=th.float64)
    ts = th.tensor([2.0, -1.0], dtype=th.float64)
    for wrap, feather in (("", False), ("", True)):
        out = wr.WindowedRef(Echo(), 16, 16, wrap, feather)(x, ts)
        assert float((out[:, :3] - x).abs().max()) <= 1e-14 and float((out[:, 3:] - x * ts.view(-1, 1, 1, 1)).abs().max()) <= 1e-14

    class Rows(th.nn.Module):
        def forward(self, x, ts, y=None):
            return th.arange(16.0, dtype=x.dtype).view(1, 1, 16, 1).expand(x.shape[0], 1, 16, 16)

    out = wr.WindowedRef(Rows(), 16, 16)(x[:1, :1], ts[:1])  # H = 40: windows at rows 0, 16 and 24
    col = out[0, 0, :, 0]
    r = th.arange(16.0, dtype=th.float64)
    # rows 0..15: window 0 alone; 16..23: window 1 alone (its rows 0..7); 24..31: windows 1 (rows 8..15) and 2 (rows 0..7); 32..39: window 2
    expect = th.cat([r, r[:8], (r[8:] + r[:8]) / 2, r[8:]])
    assert float((col - expect).abs().max()) <= 1e-14


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_window_pair():
    handle = L.load()
    for name in ("cgd_window_gather", "cgd_window_merge"):
        assert hasattr(handle, name) and name in L.EXPORTED_SYMBOLS
    code = open(os.path.join(ROOT, "include", "cgd_mi355x.h")).read()
    assert re.search(r"\bint\s+cgd_window_gather\s*\(", code) and re.search(r"\bint\s+cgd_window_merge\s*\(", code)
    assert len(L._SIGS["cgd_window_merge"][1]) == len(L._SIGS["cgd_window_gather"][1]) + 1  # the accumulate flag
