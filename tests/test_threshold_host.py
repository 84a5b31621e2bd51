"""CPU tests of dynamic thresholding under DPM-Solver++ sampling: the rank arithmetic of cgd_amd.diffusion against torch.quantile, the
'+thr=' suffix of the respacing value, the argument checks and the call sequence of `GuidedSampler.dpmpp_sample_loop_progressive` with a
recording fake library (no GPU), and the restatement (tests/threshold_ref.py) against tests/dpm_ref.py where nothing is thresholded."""
import math
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from cgd_amd import guidance as dg
from tests import dpm_ref, threshold_ref
from tests.test_plms_host import ToyModel, toy_cond_fn


# ---- rank arithmetic -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(1, 0.3), (1, 1.0), (2, 0.5), (7, 1.0), (101, 0.5), (101, 0.37), (1000, 0.995), (997, 0.995), (4096, 1e-9),
                                 (5, 0.25), (3 * 64 * 64, 0.995)])
def test_threshold_rank_is_torch_quantiles_linear_rule(n, p):
    k, frac = dd.SpacedDiffusion.threshold_rank(p, n)
    assert isinstance(k, int) and 0 <= k <= n - 1 and 0.0 <= frac < 1.0
    assert (k, frac) == threshold_ref.rank(p, n)
    if p == 1.0:
        assert (k, frac) == (n - 1, 0.0)
    if (n, p) in ((101, 0.5), (5, 0.25)):  # pos is an integer
        assert frac == 0.0 and k == round(p * (n - 1))
    rows = th.randn(4, n, generator=th.Generator().manual_seed(n), dtype=th.float64).abs()
    v = th.sort(rows, dim=1).values
    mine = v[:, k] + (v[:, min(k + 1, n - 1)] - v[:, k]) * frac
    assert th.allclose(mine, th.quantile(rows, p, dim=1), rtol=1e-12, atol=1e-15)


def test_threshold_rank_refusals():
    for bad in (0.0, -0.1, 1.0001, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError):
            dd.SpacedDiffusion.threshold_rank(bad, 10)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError):
            dd.SpacedDiffusion.threshold_rank(0.5, bad)


# ---- the respacing suffix ------------------------------------------------------------------------------------------------------------
def test_split_threshold_parses_and_refuses():
    from cgd import script_util
    assert script_util.split_threshold("dpm20") == ("dpm20", None)
    assert script_util.split_threshold("ddim50") == ("ddim50", None) and script_util.split_threshold("250") == ("250", None)
    assert script_util.split_threshold(1000) == ("1000", None)
    assert script_util.split_threshold("dpm20+thr=0.995") == ("dpm20", (0.995, None))
    assert script_util.split_threshold("dpmsde20+thr=0.995:1.5") == ("dpmsde20", (0.995, 1.5))
    assert script_util.split_threshold("dpm8+thr=1:1") == ("dpm8", (1.0, 1.0))
    for other in ("ddim20+thr=0.995", "plms20+thr=0.9", "250+thr=0.9", "+thr=0.9"):
        with pytest.raises(ValueError, match="dpmN"):
            script_util.split_threshold(other)
    for bad in ("dpm20+thr=", "dpm20+thr=abc", "dpm20+thr=0.9:", "dpm20+thr=0.9:1:2", "dpm20+thr=0", "dpm20+thr=1.5", "dpm20+thr=-0.5",
                "dpm20+thr=nan", "dpm20+thr=0.9:0.5", "dpm20+thr=0.9:nan"):
        with pytest.raises(ValueError):
            script_util.split_threshold(bad)


def test_generator_refuses_the_suffix_on_other_spacings_before_loading_anything():
    from cgd import cgd as mine
    for spec in ("ddim8+thr=0.995", "plms8+thr=0.995", "100+thr=0.995"):
        with pytest.raises(ValueError, match="dpmN"):
            next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", timestep_respacing=spec))


def test_cli_help_names_the_suffix():
    import re
    from cgd import cgd as mine
    text = re.sub(r"\s+", " ", mine.build_parser().format_help())
    assert "+thr=" in text and "dpm20+thr=0.995" in text


@pytest.mark.parametrize("spec,expect", [("dpm10+thr=0.995", (2, 0.0, 0.995)), ("dpmsde10+thr=0.9:1.5", (2, 1.0, (0.9, 1.5))), ("dpm10", (2, 0.0, None))])
def test_dropin_generator_strips_the_suffix_and_passes_the_option(spec, expect, tmp_path, monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    used, seen_spec = [], []

    class FakeTorch:
        def __getattr__(self, k):
            return getattr(th, k)

        @staticmethod
        def tensor(data, device=None, **kw):
            return th.tensor(data, **kw)

        @staticmethod
        def zeros(shape, device=None, **kw):
            return th.zeros(shape, **kw)

    monkeypatch.setattr(mine, "th", FakeTorch())
    tower = types.SimpleNamespace(ctx="ctx", input_resolution=16, out_dim=8, patch=8)
    monkeypatch.setattr(clip_util, "load_clip", lambda name, device: (types.SimpleNamespace(tower=tower), 16))
    monkeypatch.setattr(clip_util, "encode_text_prompt", lambda txt, w, name, device: (th.ones(1, 8), w))

    def loop(model, shape, order=None, eta=None, **kw):
        used.append((order, eta, kw.get("threshold"), "threshold" in kw))
        for i in range(3):
            yield {"sample": th.zeros(shape), "pred_xstart": th.zeros(shape)}

    diffusion = types.SimpleNamespace(num_timesteps=3, dpmpp_sample_loop_progressive=loop)

    def load(**kw):
        seen_spec.append(kw["timestep_respacing"])
        return types.SimpleNamespace(ctx="ctx"), diffusion

    monkeypatch.setattr(script_util, "load_guided_diffusion", load)

    class FakeGuidance:
        def __init__(self, *a, **kw):
            self.scalars, self.current_timestep, self.last_ran = th.zeros(8), None, True

        def snapshot(self):
            return 0

        def log(self, snap):
            return {"CLIP Loss": 0.0}

    monkeypatch.setattr(mine, "ClipGuidance", FakeGuidance)
    monkeypatch.setattr(script_util, "stage_images", lambda x: types.SimpleNamespace(get=lambda: script_util.to_uint8_hwc(x)))
    items = list(mine.clip_guided_diffusion(prompts=["a"], image_size=64, timestep_respacing=spec, prefix_path=str(tmp_path / "out"),
                                            checkpoints_dir=str(tmp_path / "ck"), device="cuda", progress=False, save_frequency=1))
    assert len(items) == 3 and seen_spec == [spec.split("+")[0]]  # the tables never see the suffix
    assert used == [expect + (expect[2] is not None,)]  # without the suffix the keyword is not passed at all


# ---- host logic of the device sampler ------------------------------------------------------------------------------------------------
SCRATCH_BYTES = 4096


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return SCRATCH_BYTES if name == "cgd_abs_quantile_scratch_bytes" else 0
        return fn


def _rig(spec="dpm10"):
    from cgd_amd import sampler
    lib = Recorder()
    ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", spec, False))
    guid = object.__new__(dg.ClipGuidance)
    guid.use_magnitude, guid.scalars, guid.current_timestep = False, th.zeros(8), smp.num_timesteps - 1
    guid.native = lambda x, x0, x_in, coef: th.ones_like(x)
    model = types.SimpleNamespace(forward=lambda x, ts, y, out=None: out, num_classes=5)
    return smp, guid, model, lib.calls


SHAPE = (2, 3, 4, 6)


def _run(smp, guid, model, **kw):
    gen = smp.dpmpp_sample_loop_progressive(model, SHAPE, clip_denoised=False, cond_fn=guid, model_kwargs={"y": th.zeros(2, dtype=th.long)},
                                            device="cpu", randomize_class=True, cond_fn_with_grad=True, **kw)
    outs = []
    for out in gen:
        outs.append(out)
        guid.current_timestep -= 1
    return outs


def _shape_of(call):
    """everything of a recorded call that is not an address: names, sizes, coefficient values"""
    name, args = call
    out = [name]
    for a in args:
        if hasattr(a, "_fields_"):
            out.append(tuple(getattr(a, f[0]) for f in a._fields_))
        elif isinstance(a, int) and a > 4096:
            out.append("ptr")
        else:
            out.append(a)
    return out


def test_threshold_none_issues_exactly_the_calls_of_a_run_without_the_keyword():
    runs = []
    for kw in ({}, {"threshold": None}):
        for eta in (0.0, 1.0):
            smp, guid, model, calls = _rig()
            th.manual_seed(5)
            _run(smp, guid, model, order=2, eta=eta, **kw)
            runs.append([_shape_of(c) for c in calls])
            assert {n for n, _ in calls} == {"cgd_pmv_blend", "cgd_dpmpp_update"}
    assert runs[0] == runs[2] and runs[1] == runs[3]


# args of cgd_dpmpp_threshold: ctx, x, x0, g, scalars, x0c, B, H, W, k_coef, k, frac, floor, cap, thr3, scratch, stream
# args of cgd_dpmpp_update_thr: ctx, x, x0, x0c, thr3, noise, x0_hist, x0c_out, sample, x0_out, B, H, W, k_coef, d, stream
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_set_threshold_issues_the_selection_then_the_thresholded_update(eta):
    smp, guid, model, calls = _rig()
    tab, N = smp.tables, smp.num_timesteps
    outs = _run(smp, guid, model, order=2, eta=eta, threshold=0.995)
    names = [n for n, _ in calls if n != "cgd_pmv_blend"]
    assert names == ["cgd_abs_quantile_scratch_bytes"] + ["cgd_dpmpp_threshold", "cgd_dpmpp_update_thr"] * N  # the scratch is sized once
    assert [a for n, a in calls if n == "cgd_abs_quantile_scratch_bytes"] == [(2, 72)]
    sel = [a for n, a in calls if n == "cgd_dpmpp_threshold"]
    ups = [a for n, a in calls if n == "cgd_dpmpp_update_thr"]
    k, frac = tab.threshold_rank(0.995, 72)
    prev, written = None, set()
    for step, (s, u) in enumerate(zip(sel, ups)):
        i = N - 1 - step
        eff = 1 if (step == 0 or i == 0) else 2
        assert s[1] == u[1] and s[2] == u[2] and s[5] == u[3] and s[14] == u[4]  # the same x, pred_xstart, x0c buffer and thr3
        assert s[6:9] == (2, 4, 6) and u[10:13] == (2, 4, 6)
        assert s[10:14] == (k, frac, 1.0, math.inf) and s[15] is not None
        assert (s[5], s[14], s[15]) == (sel[0][5], sel[0][14], sel[0][15])  # allocated once per loop
        assert s[9].sqrt_recip == u[13].sqrt_recip == pytest.approx(tab.sqrt_recip_alphas_cumprod[i], rel=1e-6)
        d = u[14]
        assert (d.c_x, d.c_d, d.c_r, d.c_n) == pytest.approx(tab.dpmpp_coef_f64(i, eff, eta), rel=1e-6, abs=1e-12)
        # the history rotates by pointer exactly as without thresholding
        assert u[1] == (outs[step - 1]["sample"].data_ptr() if step else u[1])
        assert u[6] == (prev if eff == 2 else None)
        assert (u[7] is not None) == (i > 1)
        assert u[7] is None or u[7] not in (prev, u[1], u[8], u[3])
        assert u[8] == outs[step]["sample"].data_ptr() and u[9] == outs[step]["pred_xstart"].data_ptr()
        assert (u[5] is not None) == bool(eta)
        prev = u[7]
        written.add(u[7])
    assert len(written - {None}) == 2


def test_cap_one_issues_no_selection():
    smp, guid, model, calls = _rig()
    _run(smp, guid, model, order=2, threshold=(0.995, 1.0))
    names = [n for n, _ in calls if n != "cgd_pmv_blend"]
    assert names == ["cgd_dpmpp_threshold", "cgd_dpmpp_update_thr"] * smp.num_timesteps  # no scratch is sized
    for n, a in calls:
        if n == "cgd_dpmpp_threshold":
            assert a[12:14] == (1.0, 1.0) and a[15] is None  # cap == floor and no scratch: the library runs one launch and selects nothing


def test_masked_run_merges_after_the_thresholded_update():
    smp, guid, model, calls = _rig()
    mask = th.zeros(1, 1, 4, 6)
    mask[..., :3] = 1.0
    _run(smp, guid, model, threshold=(0.9, 2.0), noise=th.randn(SHAPE), init_image=th.rand(SHAPE), mask=mask)
    names = [n for n, _ in calls if n not in ("cgd_pmv_blend", "cgd_abs_quantile_scratch_bytes")]
    assert names == ["cgd_dpmpp_threshold", "cgd_dpmpp_update_thr", "cgd_masked_merge"] * 10
    ups = [a for n, a in calls if n == "cgd_dpmpp_update_thr"]
    merges = [a for n, a in calls if n == "cgd_masked_merge"]
    assert all(m[1] == u[8] and m[2] == u[9] for u, m in zip(ups, merges))
    assert all(a[13] == 2.0 for n, a in calls if n == "cgd_dpmpp_threshold")


def test_loop_argument_validation():
    smp, guid, model, _ = _rig()
    kw = dict(clip_denoised=False, cond_fn=guid, cond_fn_with_grad=True)
    for bad in (True, False, 0, 0.0, -0.5, 1.5, float("nan"), "0.9", (0.9,), (0.9, 1.5, 2.0), (0.9, 0.5), (0.9, float("nan")), (True, 2.0),
                (0.9, True), (0.9, "2"), (1.5, 2.0), [0.9, 0.99]):
        with pytest.raises(ValueError):
            smp.dpmpp_sample_loop_progressive(model, SHAPE, threshold=bad, **kw)
    for good in (None, 1, 1.0, 0.5, (0.5, 1), (0.5, 1.0), (1.0, math.inf), [0.9, 1.5]):
        smp.dpmpp_sample_loop_progressive(model, SHAPE, threshold=good, **kw)  # a generator: nothing runs
    with pytest.raises(NotImplementedError):  # the guard on the unguided prediction's clip stays
        smp.dpmpp_sample_loop_progressive(model, SHAPE, clip_denoised=True, cond_fn=guid, cond_fn_with_grad=True, threshold=0.9)
    for name in ("ddim_sample_loop_progressive", "plms_sample_loop_progressive", "p_sample_loop_progressive"):
        with pytest.raises(TypeError):  # the other loops do not take the option
            getattr(smp, name)(model, SHAPE, threshold=0.9, **kw)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _toy_tape(shape, scale, steps):
    gen = th.Generator().manual_seed(3)
    return {"x_T": scale * th.randn(shape, generator=gen), "noise": [scale * th.randn(shape, generator=gen) for _ in range(steps)],
            "y": [th.randint(0, 3, (shape[0],), generator=gen) for _ in range(steps)]}


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_restatement_without_excursions_is_dpm_ref_bit_for_bit(eta):
    """every |x0c| <= 1 and a huge cap: s = 1, and clamp and / 1 are exact.  The scene: the last six levels from a small init image (at
    the noisy end the toy's pred_xstart is O(100) whatever the state)"""
    shape = (2, 3, 4, 5)
    kw = dict(clip_denoised=False, model_kwargs={"y": th.zeros(2, dtype=th.long)}, device="cpu", randomize_class=True, cond_fn_with_grad=True,
              order=2, eta=eta, tape=_toy_tape(shape, 0.1, 10), skip_timesteps=4,
              init_image=0.2 * th.randn(shape, generator=th.Generator().manual_seed(8)))
    plain = dpm_ref.create_dpm_diffusion(1000, "linear", "dpm10")
    thr = threshold_ref.create_threshold_diffusion(1000, "linear", "dpm10", threshold=(0.995, 1e30))
    a = list(plain.dpmpp_sample_loop_progressive(ToyModel(), shape, cond_fn=toy_cond_fn([]), **kw))
    b = list(thr.dpmpp_sample_loop_progressive(ToyModel(), shape, cond_fn=toy_cond_fn([]), **kw))
    assert len(a) == len(b) == 6 and len(thr.seen_scales) == 6
    assert max(float(e.max()) for e in thr.seen_excess) <= 1.0, "the scene is meant to stay inside [-1, 1]"
    assert all(th.equal(s, th.ones(2, dtype=th.float64)) for s in thr.seen_scales)
    for p, q in zip(a, b):
        assert th.equal(p["sample"], q["sample"]) and th.equal(p["pred_xstart"], q["pred_xstart"])


def test_restatement_thresholds_where_the_prediction_leaves_the_range():
    shape = (2, 3, 4, 5)
    kw = dict(clip_denoised=False, model_kwargs={"y": th.zeros(2, dtype=th.long)}, device="cpu", randomize_class=True, cond_fn_with_grad=True,
              order=2, eta=0.0, tape=_toy_tape(shape, 1.0, 10))
    plain = dpm_ref.create_dpm_diffusion(1000, "linear", "dpm10")
    a = list(plain.dpmpp_sample_loop_progressive(ToyModel(), shape, cond_fn=toy_cond_fn([]), **kw))
    for threshold in (1.0, (0.9, 1.5), (0.9, 1.0)):
        thr = threshold_ref.create_threshold_diffusion(1000, "linear", "dpm10", threshold=threshold)
        b = list(thr.dpmpp_sample_loop_progressive(ToyModel(), shape, cond_fn=toy_cond_fn([]), **kw))
        assert max(float(e.max()) for e in thr.seen_excess) > 1.0
        cap = threshold[1] if isinstance(threshold, tuple) else math.inf
        assert all(float(s.min()) >= 1.0 and float(s.max()) <= cap for s in thr.seen_scales)
        assert not th.allclose(a[-1]["sample"], b[-1]["sample"], rtol=1e-3, atol=1e-4)
        if threshold == 1.0:  # rescaled by the maximum: the last sample, a thresholded prediction, lies in [-1, 1]
            assert float(b[-1]["sample"].abs().max()) <= 1.0
        # the rule itself, on the first evaluation's guided prediction: s is the p-quantile of |x0c| per sample, clipped to [1, cap]
    x = th.randn(3, 3, 8, 8, generator=th.Generator().manual_seed(1)) * 2
    x0t, s = threshold_ref.threshold(x, 0.9, 2.5)
    want = th.quantile(x.abs().flatten(1).double(), 0.9, dim=1).clamp(1.0, 2.5)
    assert th.allclose(s.double(), want, rtol=1e-6) and float(x0t.abs().max()) <= 1.0
    assert th.equal(x0t, (th.maximum(th.minimum(x, s.view(-1, 1, 1, 1)), -s.view(-1, 1, 1, 1)) / s.view(-1, 1, 1, 1)))


def test_library_binding_header_and_build_list_declare_the_entries():
    import os
    from cgd_amd import lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cgd_mi355x.h")).read()
    for name in ("cgd_abs_quantile_scratch_bytes", "cgd_abs_quantile_slice", "cgd_op_abs_quantile", "cgd_dpmpp_threshold", "cgd_dpmpp_update_thr"):
        assert name in L.EXPORTED_SYMBOLS and f" {name}(" in header
    assert " threshold " in open(os.path.join(root, "clip-guided-diffusion_amd", "csrc", "build.sh")).read()
