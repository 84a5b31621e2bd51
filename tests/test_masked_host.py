"""CPU tests of masked sampling: the IMAGE::MASK parser, the merge coefficients, what the loops refuse, the host's call sequence (driven
with a recording fake library, no GPU), the restatement (tests/masked_ref.py) on a toy model, and the C ABI's new entry."""
import math
import os
import re
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from cgd_amd import lib as L
from oracle import diffusion as od
from tests import masked_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the IMAGE::MASK value ---------------------------------------------------------------------------------------------------------
def test_init_image_value_without_separator_is_the_image():
    from cgd import script_util
    assert script_util.split_init_mask("photos/a.png") == ("photos/a.png", None)
    # the '://' of a URL is no separator
    assert script_util.split_init_mask("https://example.org/a.png") == ("https://example.org/a.png", None)


def test_init_image_value_splits_at_the_last_separator():
    from cgd import script_util
    assert script_util.split_init_mask("a.png::m.png") == ("a.png", "m.png")
    assert script_util.split_init_mask("https://example.org/a.png::https://example.org/m.png") == \
        ("https://example.org/a.png", "https://example.org/m.png")
    assert script_util.split_init_mask("odd::name.png::m.png") == ("odd::name.png", "m.png")


@pytest.mark.parametrize("bad", ["a.png::", "::m.png", "::"])
def test_init_image_value_with_an_empty_part_is_refused(bad):
    from cgd import script_util
    with pytest.raises(ValueError):
        script_util.split_init_mask(bad)


def test_cli_help_names_the_mask():
    from cgd import cgd as mine
    assert "IMAGE::MASK" in mine._CLI_SPEC
    assert "IMAGE::MASK" in mine.build_parser().format_help()


# ---- coefficients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_mask_coefficients_match_float64_closed_forms(schedule):
    tab = dd.create_gaussian_diffusion(1000, schedule, "50", False)
    ref = od.create_gaussian_diffusion(1000, schedule, "50", False)
    N = tab.num_timesteps
    for i in (0, 1, N - 1):
        k = tab.mask_coef(i)
        abp = 1.0 if i == 0 else float(ref.alphas_cumprod[i - 1])
        alpha = 1.0 - float(ref.betas[i])  # abar[i] / abar_prev[i]
        for got, want in ((k.sqrt_ab_prev, math.sqrt(abp)), (k.sqrt_one_minus_ab_prev, math.sqrt(1 - abp)),
                          (k.renoise_x, math.sqrt(alpha)), (k.renoise_n, math.sqrt(1 - alpha))):
            assert got == pytest.approx(want, rel=2e-7, abs=1e-9)  # float32 rounding of the float64 value
        assert k.flags == 0
    k0 = tab.mask_coef(0)
    assert k0.sqrt_ab_prev == 1.0 and k0.sqrt_one_minus_ab_prev == 0.0


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


SHAPE = (2, 3, 4, 6)
KW = dict(clip_denoised=False, device="cpu")


def _loops(smp):
    return (smp.p_sample_loop_progressive, smp.ddim_sample_loop_progressive, smp.plms_sample_loop_progressive)


def test_loops_refuse_a_mask_without_an_init_image():
    smp, lib, model = _rig()
    for loop in _loops(smp):
        with pytest.raises(ValueError):
            loop(model, SHAPE, mask=th.ones(1, 1, 4, 6), **KW)
    assert not lib.calls


@pytest.mark.parametrize("mask_shape", [(4, 6), (3, 1, 4, 6), (1, 2, 4, 6), (1, 1, 4, 5), (1, 1, 6, 4)])
def test_loops_refuse_bad_mask_shapes(mask_shape):
    smp, _, model = _rig()
    for loop in _loops(smp):
        with pytest.raises(ValueError):
            loop(model, SHAPE, init_image=th.zeros(SHAPE), mask=th.ones(mask_shape), **KW)


def test_loops_refuse_bad_init_shapes_and_mask_values():
    smp, _, model = _rig()
    for loop in _loops(smp):
        with pytest.raises(ValueError):
            loop(model, SHAPE, init_image=th.zeros(3, 3, 4, 6), mask=th.ones(1, 1, 4, 6), **KW)
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError):
                loop(model, SHAPE, init_image=th.zeros(SHAPE), mask=th.full((1, 1, 4, 6), bad), **KW)


def test_resamples_below_one_and_resampling_under_plms_are_refused():
    smp, _, model = _rig()
    init, mask = th.zeros(SHAPE), th.ones(1, 1, 4, 6)
    for loop in _loops(smp):
        for bad in (0, -1, 1.5, True):
            with pytest.raises(ValueError):
                loop(model, SHAPE, init_image=init, mask=mask, resamples=bad, **KW)
    with pytest.raises(ValueError):
        smp.plms_sample_loop_progressive(model, SHAPE, init_image=init, mask=mask, resamples=2, **KW)
    for loop in _loops(smp)[:2]:  # the repeats re-run the merge: nothing to repeat without a mask
        with pytest.raises(ValueError):
            loop(model, SHAPE, resamples=2, **KW)


def test_a_masked_loop_merges_after_every_update_and_an_unmasked_one_never():
    init, mask = th.zeros(1, 3, 4, 6), th.ones(2, 1, 4, 6)
    for kind, update in ((0, "cgd_sample_update"), (1, "cgd_sample_update"), (2, "cgd_multistep_update")):
        smp, lib, model = _rig()
        plain = list(_loops(smp)[kind](model, SHAPE, init_image=th.zeros(SHAPE), **KW))
        assert len(plain) == 10 and not [n for n, _ in lib.calls if n == "cgd_masked_merge"]
        n_plain = len(lib.calls)
        del lib.calls[:]
        outs = list(_loops(smp)[kind](model, SHAPE, init_image=init, mask=mask, **KW))
        names = [n for n, _ in lib.calls]
        assert len(outs) == 10
        if kind == 2:  # order 2: the start step merges its predictor (no pred_xstart) and its result
            assert names[:6] == ["cgd_pmv_blend", update, "cgd_masked_merge", "cgd_pmv_blend", update, "cgd_masked_merge"]
            assert names[6:] == ["cgd_pmv_blend", update, "cgd_masked_merge"] * 9 and len(names) == n_plain + 11
        else:
            assert names == ["cgd_pmv_blend", update, "cgd_masked_merge"] * 10
        merges = [a for n, a in lib.calls if n == "cgd_masked_merge"]
        # args: ctx, sample, pred_xstart, init, mask, n_known, n_re, x_re, B, H, W, init_batch, mask_batch, mask_channels, k, stream
        assert all(a[8:14] == (2, 4, 6, 1, 2, 1) and a[6] is None and a[7] is None for a in merges)
        last = merges[-1]
        assert last[5] is None and last[14].flags == L.MASK_PRED_XSTART and last[14].sqrt_ab_prev == 1.0  # i == 0: known = init
        first = merges[0]
        assert first[5] is not None and first[14].flags & L.MASK_N_KNOWN
        if kind == 2:
            assert first[2] is None and first[14].flags == L.MASK_N_KNOWN and merges[1][14].flags == L.MASK_PRED_XSTART | L.MASK_N_KNOWN
            assert len({a[5] for a in merges[:-1]}) == 1  # deterministic loop: the same noise tensor (the loop's initial one) throughout
        if kind == 1:
            assert len({a[5] for a in merges[:-1]}) == 1
        # the update's outputs are what is merged
        ups = [a for n, a in lib.calls if n == update]
        out_idx = (9, 10) if update == "cgd_multistep_update" else (8, 9)
        assert merges[-1][1] == ups[-1][out_idx[0]] and merges[-1][2] == ups[-1][out_idx[1]]


def test_resampling_repeats_every_step_but_the_last_and_yields_once_per_step():
    smp, lib, model = _rig()
    th.manual_seed(5)
    outs = list(smp.p_sample_loop_progressive(model, SHAPE, init_image=th.zeros(SHAPE), mask=th.ones(1, 3, 4, 6), resamples=3, **KW))
    after = th.rand(1)
    assert len(outs) == 10
    merges = [a for n, a in lib.calls if n == "cgd_masked_merge"]
    assert len(merges) == 9 * 3 + 1
    again = [a[6] is not None for a in merges]
    assert again == [True, True, False] * 9 + [False]
    assert all((a[7] is not None) == (a[6] is not None) and bool(a[14].flags & L.MASK_RENOISE) == (a[6] is not None) for a in merges)
    # a repeat starts from the re-noised state the merge wrote (sample update args: ctx, x, ...)
    ups = [a for n, a in lib.calls if n == "cgd_sample_update"]
    assert ups[1][1] == merges[0][7] and ups[2][1] == merges[1][7] and ups[3][1] == merges[2][1]
    # draws: x_T, then per evaluation the step noise and the known region's noise, and one re-noise draw per repeat
    th.manual_seed(5)
    th.randn(SHAPE)
    for rep in again:
        th.randn(SHAPE), th.randn(SHAPE)
        if rep:
            th.randn(SHAPE)
    assert th.equal(after, th.rand(1))


def test_a_deterministic_masked_loop_adds_no_random_draw():
    init, mask = th.zeros(SHAPE), th.ones(1, 1, 4, 6)
    ends = []
    for kw in ({}, {"init_image": init, "mask": mask}):
        smp, _, model = _rig()
        th.manual_seed(9)
        list(smp.ddim_sample_loop_progressive(model, SHAPE, **kw, **KW))
        ends.append(th.rand(1))
    assert th.equal(*ends)


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
    return {"x_T": mk(), "noise": [mk() for _ in range(n)], "known_noise": [mk() for _ in range(n)], "renoise": [mk() for _ in range(n)],
            "y": [th.zeros(shape[0], dtype=th.long)] * n}


@pytest.mark.parametrize("kind", ["p", "ddim", "plms"])
def test_restatement_with_an_all_ones_mask_is_the_unmasked_loop(kind):
    ref = masked_ref.create_masked_diffusion(1000, "linear", "ddim10")
    shape = (2, 3, 4, 5)
    tape, init = _toy_tape(10, shape), th.tanh(th.randn(shape, generator=th.Generator().manual_seed(1)))
    model = ToyModel()
    got = list(ref.masked_loop(kind, model, shape, init, th.ones(1, 1, 4, 5), tape, skip_timesteps=3))
    if kind == "plms":
        want = list(ref.plms_sample_loop_progressive(model, shape, clip_denoised=False, device="cpu", skip_timesteps=3, init_image=init, tape=tape))
    else:
        loop = ref.p_sample_loop_progressive if kind == "p" else ref.ddim_sample_loop_progressive
        want = list(loop(model, shape, clip_denoised=False, device="cpu", skip_timesteps=3, init_image=init, tape=tape))
    assert len(got) == len(want) == 7
    for a, b in zip(got, want):
        assert th.equal(a["sample"], b["sample"]) and th.equal(a["pred_xstart"], b["pred_xstart"])


def test_restatement_keeps_the_init_image_where_the_mask_is_zero_and_resamples():
    ref = masked_ref.create_masked_diffusion(1000, "linear", "ddim10")
    shape = (1, 3, 4, 5)
    tape, init = _toy_tape(30, shape), th.tanh(th.randn(shape, generator=th.Generator().manual_seed(1)))
    mask = masked_ref.make_mask((1, 1, 4, 5), seed=2)
    seen = []

    class Counting(ToyModel):
        def forward(self, x, ts, y=None):
            seen.append(int(ts[0]))
            return super().forward(x, ts, y)

    outs = list(ref.masked_loop("p", Counting(), shape, init, mask, tape, skip_timesteps=6, resamples=2))
    tm = ref.timestep_map
    assert len(outs) == 4 and seen == [tm[3], tm[3], tm[2], tm[2], tm[1], tm[1], tm[0]]
    keep = (mask == 0).expand(shape)
    assert th.equal(outs[-1]["sample"][keep], init[keep]) and th.equal(outs[-1]["pred_xstart"][keep], init[keep])
    abp = float(ref.alphas_cumprod_prev[3])
    want = (abp ** 0.5) * init + ((1 - abp) ** 0.5) * tape["known_noise"][1]  # the second merge of step index 3 is the one yielded
    assert th.equal(outs[0]["sample"][keep], want[keep])
    with pytest.raises(ValueError):
        list(ref.masked_loop("plms", ToyModel(), shape, init, mask, tape, resamples=2))


def test_fp64_merge_selects_at_the_mask_endpoints():
    k = dd.create_gaussian_diffusion(1000, "linear", "50", False).mask_coef(20)
    m = th.tensor([0.0, 1.0, 0.25]).view(1, 1, 1, 3)
    s = th.tensor([float("inf"), 2.0, 4.0]).view(1, 1, 1, 3).expand(1, 3, 1, 3)
    x0 = th.tensor([float("nan"), 3.0, 8.0]).view(1, 1, 1, 3).expand(1, 3, 1, 3)
    init, n = th.full((1, 3, 1, 3), 0.5), th.full((1, 3, 1, 3), -1.0)
    out_s, out_x0, x_re = masked_ref.merge_fp64(k, s, x0, init, m, n, n_re=th.ones(1, 3, 1, 3))
    known = k.sqrt_ab_prev * 0.5 - k.sqrt_one_minus_ab_prev
    assert out_s[0, 0, 0].tolist() == pytest.approx([known, 2.0, 0.25 * 4.0 + 0.75 * known])
    assert out_x0[0, 0, 0].tolist() == pytest.approx([0.5, 3.0, 0.25 * 8.0 + 0.75 * 0.5])
    assert th.allclose(x_re, k.renoise_x * out_s + k.renoise_n)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_merge_and_the_header_declares_it():
    handle = L.load()
    assert hasattr(handle, "cgd_masked_merge") and "cgd_masked_merge" in L.EXPORTED_SYMBOLS
    src = open(os.path.join(ROOT, "include", "cgd_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+cgd_masked_merge\s*\(", code) and re.search(r"\}\s*cgd_mask_coef\s*;", code)
    # the ctypes mirror has the header's fields, in order
    body = re.search(r"typedef struct cgd_mask_coef \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"(?:float|int)\s+(\w+)\s*;", body) == [f for f, _ in L.MaskCoef._fields_]
    assert (L.MASK_PRED_XSTART, L.MASK_N_KNOWN, L.MASK_RENOISE) == (1, 2, 4)
    assert re.search(r"CGD_MASK_PRED_XSTART = 1, CGD_MASK_N_KNOWN = 2, CGD_MASK_RENOISE = 4", code)
