"""CPU tests of ILVR: the low-pass operator of the restatement (tests/ilvr_ref.py) against the vendored ResizeRight's fixture, the
'ilvrN[@U]=IMAGE' parser, what the loops refuse, the host's call sequence (driven with a recording fake library, no GPU), the restatement
on a toy model, and the C ABI's new entries."""
import os
import re
import types

import numpy as np
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd.script_util import check_init_ilvr, ilvr_stop, split_init_ilvr
from cgd_amd import diffusion as dd
from cgd_amd import lib as L
from oracle import diffusion as od
from tests import ilvr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(32, 32, 2), (32, 32, 8), (24, 40, 4), (64, 64, 32), (16, 16, 16)]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_ilvr.npz"))


# ---- the operator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N", CASES)
def test_lowpass_matrix_reproduces_resize_right(fixture, H, W, N):
    x, y = th.from_numpy(fixture[f"x_{H}x{W}_{N}"]), th.from_numpy(fixture[f"y_{H}x{W}_{N}"])
    assert x.dtype == th.float64 and tuple(x.shape) == (2, 3, H, W)
    got = ilvr_ref.lowpass_matrix(H, N) @ x @ ilvr_ref.lowpass_matrix(W, N).T
    assert float((got - y).abs().max()) <= 1e-12
    assert float(y.abs().max()) > 1e-2  # the comparison is not one of zeros


def test_lowpass_rows_taper_at_the_border_and_sum_to_one_inside():
    P = ilvr_ref.lowpass_matrix(64, 4)
    sums = P.sum(1)
    assert sums.dtype == th.float64 and abs(float(sums[32]) - 1.0) < 1e-12
    assert 0.4 < float(sums[0]) < 0.8 and 0.4 < float(sums[-1]) < 0.8  # constant padding: the correction tapers at the border
    with pytest.raises(ValueError):
        ilvr_ref.lowpass_matrix(30, 4)


def test_refine_fp64_replaces_the_low_band_only():
    gen = th.Generator().manual_seed(0)
    s, x0, ref, n = (th.randn(2, 3, 32, 32, generator=gen) for _ in range(4))
    out_s, out_x0 = ilvr_ref.refine_fp64(0.8, 0.6, s, x0, ref[:1], n, 4)
    known = 0.8 * ref[:1].double() + 0.6 * n.double()
    assert th.allclose(out_s, s.double() + ilvr_ref.lowpass(known - s.double(), 4), atol=1e-13)
    assert th.allclose(out_x0, x0.double() + ilvr_ref.lowpass(ref[:1].double() - x0.double(), 4), atol=1e-13)
    assert ilvr_ref.refine_fp64(1.0, 0.0, s, None, ref, None, 4)[1] is None


# ---- the ilvrN[@U]=IMAGE value -----------------------------------------------------------------------------------------------------
def test_init_image_value_without_the_prefix_is_the_image():
    for value in ("photos/a.png", "ilvr8.png", "https://example.org/ilvr8=a.png", "invert=a.png"):
        assert split_init_ilvr(value) == (value, None)
        assert check_init_ilvr(value, 64) is None
    assert check_init_ilvr(None, 64) is None and check_init_ilvr("a.png::m.png", 64) is None


def test_init_image_value_with_the_prefix_gives_factor_and_fraction():
    assert split_init_ilvr("ilvr8=a.png") == ("a.png", (8, 1.0))
    assert split_init_ilvr("ilvr16@0.8=https://example.org/a.png") == ("https://example.org/a.png", (16, 0.8))
    assert split_init_ilvr("ilvr64@1=a=b.png") == ("a=b.png", (64, 1.0))
    assert check_init_ilvr("ilvr8@0.5=a.png", 64, 8, 16) == (8, 0.5)


@pytest.mark.parametrize("bad", ["ilvr=a.png", "ilvrx=a.png", "ilvr3=a.png", "ilvr1=a.png", "ilvr128=a.png", "ilvr8@=a.png", "ilvr8@x=a.png",
                                 "ilvr8@0=a.png", "ilvr8@1.5=a.png", "ilvr8@-0.5=a.png", "ilvr8="])
def test_malformed_ilvr_values_are_refused(bad):
    with pytest.raises(ValueError):
        split_init_ilvr(bad)


@pytest.mark.parametrize("bad", ["ilvr8=a.png::m.png", "ilvr8=invert=a.png", "invert=ilvr8=a.png", "ilvr8=upsample=a.png",
                                 "upsample=ilvr8=a.png"])
def test_ilvr_with_a_mask_inversion_or_upsampling_is_refused(bad):
    with pytest.raises(ValueError):
        check_init_ilvr(bad, 256)


def test_a_factor_that_does_not_divide_the_frame_is_refused():
    assert check_init_ilvr("ilvr64=a.png", 64) == (64, 1.0)
    for ho, wo in ((32, 0), (0, 32), (8, 8)):
        with pytest.raises(ValueError):
            check_init_ilvr("ilvr64=a.png", 64, ho, wo)


def test_the_generator_refuses_bad_ilvr_values_before_anything_is_loaded(tmp_path):
    from cgd.cgd import clip_guided_diffusion
    for value, kw in (("ilvr8=a.png::m.png", {}), ("ilvr8=invert=a.png", {}), ("ilvr32=a.png", {"height_offset": 16}), ("ilvr5=a.png", {})):
        with pytest.raises(ValueError):
            next(clip_guided_diffusion(prompts=["x"], image_size=64, init_image=value, device="cuda", checkpoints_dir=str(tmp_path / "none"),
                                       prefix_path=str(tmp_path / "out"), **kw))
    assert not (tmp_path / "none").exists() and not (tmp_path / "out").exists()


def test_stop_index_of_a_fraction():
    assert [ilvr_stop(u, 10) for u in (1.0, 0.9, 0.8, 0.7, 0.5, 0.05)] == [0, 1, 2, 3, 5, 10]
    assert ilvr_stop(0.8, 250) == 50 and ilvr_stop(0.333, 1000) == 667


def test_cli_help_names_the_form():
    from cgd import cgd as mine
    assert "ilvrN=IMAGE" in mine._CLI_SPEC and "ilvrN@U=IMAGE" in mine._CLI_SPEC
    assert "ilvrN=IMAGE" in " ".join(mine.build_parser().format_help().split())


# ---- host logic with a recording fake library -------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _rig(spec="ddim10"):
    from cgd_amd import sampler
    lib = Recorder()
    ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", spec, False))
    model = types.SimpleNamespace(forward=lambda x, ts, y, out=None: out)
    return smp, lib, model


SHAPE = (2, 3, 8, 12)
KW = dict(clip_denoised=False, device="cpu")
UPDATES = ("cgd_sample_update", "cgd_sample_update", "cgd_multistep_update", "cgd_dpmpp_update")


def _loops(smp):
    return (smp.p_sample_loop_progressive, smp.ddim_sample_loop_progressive, smp.plms_sample_loop_progressive,
            smp.dpmpp_sample_loop_progressive)


def _names(lib):
    return [n for n, _ in lib.calls if n != "cgd_ilvr_scratch_floats"]


def test_loops_refuse_ilvr_with_a_mask_or_resampling():
    smp, lib, model = _rig()
    ref = th.zeros(1, 3, 8, 12)
    for loop in _loops(smp):
        with pytest.raises(ValueError):
            loop(model, SHAPE, init_image=th.zeros(SHAPE), mask=th.ones(1, 1, 8, 12), ilvr=(ref, 4), **KW)
        with pytest.raises(ValueError):
            loop(model, SHAPE, resamples=2, ilvr=(ref, 4), **KW)
    assert not lib.calls


@pytest.mark.parametrize("bad", [
    lambda r: (r, 3), lambda r: (r, 1), lambda r: (r, 128), lambda r: (r, 4.0), lambda r: (r, True), lambda r: (r, 8),  # 8 does not divide 12
    lambda r: (r[0], 4), lambda r: (th.zeros(3, 3, 8, 12), 4), lambda r: (th.zeros(1, 1, 8, 12), 4), lambda r: (th.zeros(1, 3, 8, 8), 4),
    lambda r: (None, 4), lambda r: (r, 4, -1), lambda r: (r, 4, 11), lambda r: (r, 4, 1.0), lambda r: (r,), lambda r: r])
def test_loops_refuse_bad_factors_shapes_and_stop_indices(bad):
    smp, lib, model = _rig()
    for loop in _loops(smp):
        with pytest.raises(ValueError):
            loop(model, SHAPE, ilvr=bad(th.zeros(1, 3, 8, 12)), **KW)
    assert not lib.calls


def test_a_loop_without_ilvr_issues_the_parents_call_sequence():
    for kind, update in enumerate(UPDATES):
        smp, lib, model = _rig()
        assert len(list(_loops(smp)[kind](model, SHAPE, **KW))) == 10
        names = [n for n, _ in lib.calls]
        if kind == 2:  # order 2: the start step evaluates twice
            assert names == ["cgd_pmv_blend", update] * 11
        else:
            assert names == ["cgd_pmv_blend", update] * 10


@pytest.mark.parametrize("stop", [0, 4, 10])
def test_a_loop_with_ilvr_refines_after_every_update_at_or_above_stop_and_never_below(stop):
    ref = th.zeros(1, 3, 8, 12)
    for kind, update in enumerate(UPDATES):
        smp, lib, model = _rig()
        outs = list(_loops(smp)[kind](model, SHAPE, ilvr=(ref, 4, stop), **KW))
        assert len(outs) == 10
        assert [n for n, _ in lib.calls].count("cgd_ilvr_scratch_floats") == 1  # the scratch is sized once per loop
        assert lib.calls[0] == ("cgd_ilvr_scratch_floats", (2, 8, 12, 4, 1))
        names = _names(lib)
        want = []
        for i in range(9, -1, -1):
            if kind == 2 and i == 9:  # the PLMS start step: predictor (refined), second evaluation, corrector
                want += ["cgd_pmv_blend", update] + ["cgd_ilvr_refine"] * (i >= stop)
            want += ["cgd_pmv_blend", update] + ["cgd_ilvr_refine"] * (i >= stop)
        assert names == want
        refines = [a for n, a in lib.calls if n == "cgd_ilvr_refine"]
        if stop == 10:
            assert not refines
            continue
        # args: ctx, sample, pred_xstart, ref, noise, scratch, B, H, W, ref_batch, factor, sa, sb, stream
        assert all(a[6:11] == (2, 8, 12, 1, 4) for a in refines)
        assert len({a[5] for a in refines}) == 1 and len({a[3] for a in refines}) == 1  # one scratch, one reference
        tab = smp.tables
        levels = [i for i in range(9, stop - 1, -1)]
        if kind == 2:
            levels = [9] + levels
        for a, i in zip(refines, levels):
            k = tab.mask_coef(i)
            assert (a[11], a[12]) == (k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev)
            assert (a[4] is None) == (i == 0)
        if stop == 0:
            assert (refines[-1][11], refines[-1][12]) == (1.0, 0.0)  # i == 0: the reference itself
        if kind == 2:
            assert refines[0][2] is None and refines[1][2] is not None  # the predictor has no pred_xstart
        if kind in (1, 2, 3):  # deterministic: the loop's initial noise throughout
            assert len({a[4] for a in refines if a[4] is not None}) == 1
        # the update's outputs are what is refined
        ups = [a for n, a in lib.calls if n == update]
        out_idx = {"cgd_sample_update": (8, 9), "cgd_multistep_update": (9, 10), "cgd_dpmpp_update": (8, 9)}[update]
        last = ups[len(refines) - 1]  # (the PLMS start step has two updates and two refinements)
        assert refines[-1][1] == last[out_idx[0]] and refines[-1][2] == last[out_idx[1]]


def test_a_reference_of_the_batch_is_passed_with_its_batch():
    smp, lib, model = _rig()
    list(smp.ddim_sample_loop_progressive(model, SHAPE, ilvr=(th.zeros(SHAPE), 2), **KW))
    assert all(a[9] == 2 and a[10] == 2 for n, a in lib.calls if n == "cgd_ilvr_refine")


def test_a_sharded_loop_cuts_a_reference_of_the_global_batch_to_its_rows():
    smp, lib, model = _rig()
    smp.shard = ([1, 3], 4)
    ref = th.arange(4.0).view(4, 1, 1, 1).expand(4, 3, 8, 12).contiguous()
    list(smp.ddim_sample_loop_progressive(model, SHAPE, ilvr=(ref, 4, 9), **KW))
    (args,) = [a for n, a in lib.calls if n == "cgd_ilvr_refine"]
    assert args[9] == 2  # this rank's two rows


def test_a_deterministic_loop_with_ilvr_adds_no_random_draw():
    ref = th.zeros(1, 3, 8, 12)
    for kind, kw in ((1, {}), (2, {}), (3, {})):
        ends = []
        for extra in ({}, {"ilvr": (ref, 4)}):
            smp, _, model = _rig()
            th.manual_seed(9)
            list(_loops(smp)[kind](model, SHAPE, **extra, **kw, **KW))
            ends.append(th.rand(1))
        assert th.equal(*ends)


def test_a_stochastic_loop_draws_once_per_refinement_after_the_steps_own_noise():
    ref = th.zeros(1, 3, 8, 12)
    smp, lib, model = _rig()
    th.manual_seed(5)
    list(smp.p_sample_loop_progressive(model, SHAPE, ilvr=(ref, 4, 6), **KW))
    after = th.rand(1)
    th.manual_seed(5)
    th.randn(SHAPE)
    for i in range(9, -1, -1):
        th.randn(SHAPE)
        if i >= 6:
            th.randn(SHAPE)
    assert th.equal(after, th.rand(1))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
class ToyModel(th.nn.Module):
    def __init__(self):
        super().__init__()
        self.abar = th.from_numpy(od.GaussianDiffusion(od.get_named_beta_schedule("linear", 1000)).alphas_cumprod).float()

    def forward(self, x, ts, y=None):
        c = (1 - self.abar[ts.long()]).sqrt().view(-1, 1, 1, 1)
        return th.cat([c * x + 0.1 * th.tanh(x), th.tanh(x)], dim=1)


def _toy_tape(n, shape, seed=3):
    gen = th.Generator().manual_seed(seed)
    mk = lambda: th.randn(shape, generator=gen)  # noqa: E731
    return {"x_T": mk(), "noise": [mk() for _ in range(n)], "ilvr_noise": [mk() for _ in range(n)],
            "y": [th.zeros(shape[0], dtype=th.long)] * n}


@pytest.mark.parametrize("kind", ["p", "ddim", "plms", "dpm"])
def test_restatement_with_stop_at_the_number_of_timesteps_is_the_plain_loop(kind):
    ref = ilvr_ref.create_ilvr_diffusion(1000, "linear", "ddim10")
    shape = (2, 3, 8, 8)
    tape, image = _toy_tape(10, shape), th.tanh(th.randn(shape, generator=th.Generator().manual_seed(1)))
    model = ToyModel()
    got = list(ref.ilvr_loop(kind, model, shape, image, 4, tape, stop=10, skip_timesteps=3, init_image=image))
    loop = {"p": ref.p_sample_loop_progressive, "ddim": ref.ddim_sample_loop_progressive, "plms": ref.plms_sample_loop_progressive,
            "dpm": ref.dpmpp_sample_loop_progressive}[kind]
    want = list(loop(model, shape, clip_denoised=False, device="cpu", skip_timesteps=3, init_image=image, tape=tape))
    assert len(got) == len(want) == 7
    for a, b in zip(got, want):
        assert th.equal(a["sample"], b["sample"]) and th.equal(a["pred_xstart"], b["pred_xstart"])
    # ... and with stop = 0 it is not
    other = list(ref.ilvr_loop(kind, model, shape, image, 4, tape, stop=0, skip_timesteps=3, init_image=image))
    assert not th.equal(other[0]["sample"], want[0]["sample"])


def test_restatement_refines_the_first_update_with_the_first_taped_draw():
    ref = ilvr_ref.create_ilvr_diffusion(1000, "linear", "ddim10")
    shape = (1, 3, 8, 8)
    tape, image = _toy_tape(10, shape), th.tanh(th.randn(shape, generator=th.Generator().manual_seed(1)))
    outs = list(ref.ilvr_loop("p", ToyModel(), shape, image, 4, tape))
    assert len(outs) == 10
    # the reference is noised to level 8 (abar_prev of index 9)
    abp = float(ref.alphas_cumprod_prev[9])
    with th.no_grad():
        plain = ref.p_sample_with_grad(ToyModel(), tape["x_T"], th.tensor([9]), clip_denoised=False, noise=tape["noise"][0])
    want_s, _ = ilvr_ref.refine_fp64(abp ** 0.5, (1 - abp) ** 0.5, plain["sample"], None, image, tape["ilvr_noise"][0], 4)
    assert th.allclose(outs[0]["sample"].double(), want_s, atol=1e-6)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_refinement_and_the_header_declares_it():
    handle = L.load()
    for name in ("cgd_ilvr_refine", "cgd_ilvr_scratch_floats"):
        assert hasattr(handle, name) and name in L.EXPORTED_SYMBOLS
    src = open(os.path.join(ROOT, "include", "cgd_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+cgd_ilvr_refine\s*\(", code) and re.search(r"\blong\s+cgd_ilvr_scratch_floats\s*\(", code)
    # the scratch: one low-resolution image per pair; 0 for what the launcher refuses
    f = handle.cgd_ilvr_scratch_floats
    assert f(2, 24, 40, 4, 0) == 2 * 3 * 6 * 10 and f(2, 24, 40, 4, 1) == 2 * 2 * 3 * 6 * 10
    assert f(1, 256, 256, 32, 1) == 2 * 3 * 8 * 8
    assert f(2, 24, 40, 3, 0) == 0 and f(2, 24, 40, 16, 0) == 0 and f(0, 24, 40, 4, 0) == 0 and f(1, 256, 256, 128, 0) == 0
