"""CPU tests of DDIM inversion: the step coefficients, the restatement (tests/invert_ref.py) on a round trip in float64, the implied noise
in float32, the `invert=` prefix of the init-image value, what the loop and the generator refuse, the host's call sequence (driven with a
recording fake library, no GPU), and the C ABI's new entry."""
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
from tests import invert_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- coefficients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule,spec", [("linear", "50"), ("linear", "ddim50"), ("cosine", "50")])
def test_reverse_coefficients_match_float64_closed_forms(schedule, spec):
    tab = dd.create_gaussian_diffusion(1000, schedule, spec, False)
    ref = od.create_gaussian_diffusion(1000, schedule, spec, False)
    N = tab.num_timesteps
    assert N == 50
    for i in (0, 1, 20, N - 2, N - 1):
        k = tab.reverse_coef(i)
        ab = float(ref.alphas_cumprod[i])
        abn = float(ref.alphas_cumprod_next[i])
        assert abn == (float(ref.alphas_cumprod[i + 1]) if i + 1 < N else 0.0)
        for got, want in ((k.sqrt_recip, math.sqrt(1 / ab)), (k.sqrt_recipm1, math.sqrt(1 / ab - 1)), (k.sqrt_ab_next, math.sqrt(abn)),
                          (k.sqrt_one_minus_ab_next, math.sqrt(1 - abn)), (k.inv_sqrt_one_minus_ab_next, 1 / math.sqrt(1 - abn))):
            assert got == pytest.approx(want, rel=2e-7, abs=1e-9)  # float32 rounding of the float64 value
        if i + 1 < N:
            # the level an inversion step reaches is the level the sampling step of index i + 1 starts from
            up = tab.step_coef(i + 1)
            assert k.sqrt_one_minus_ab_next == up.sqrt_one_minus_ab
            assert k.sqrt_ab_next == pytest.approx(1 / up.sqrt_recip, rel=2e-7)
        if i + 2 < N:  # ... and the level the sampling step of index i + 2 arrives at
            assert k.sqrt_ab_next == tab.step_coef(i + 2).sqrt_ab_prev and \
                k.sqrt_one_minus_ab_next == tab.step_coef(i + 2).sqrt_one_minus_ab_prev
    last = tab.reverse_coef(N - 1)
    assert last.sqrt_ab_next == 0.0 and last.sqrt_one_minus_ab_next == 1.0 and last.inv_sqrt_one_minus_ab_next == 1.0


def test_the_inverse_root_is_zero_where_it_is_undefined():
    tab = dd.create_gaussian_diffusion(1000, "linear", "50", False)
    tab.alphas_cumprod_next = tab.alphas_cumprod_next.copy()
    tab.alphas_cumprod_next[3] = 1.0  # no schedule has this; the struct's rule for it is 0, which the kernel refuses with noise_out
    k = tab.reverse_coef(3)
    assert k.sqrt_one_minus_ab_next == 0.0 and k.inv_sqrt_one_minus_ab_next == 0.0


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
class ConstEps(th.nn.Module):
    """a model whose eps is one fixed random tensor, whatever the input (channels 3..5: the variance head, zeros)"""

    def __init__(self, shape, dtype, seed=11):
        super().__init__()
        self.eps = th.randn(shape, generator=th.Generator().manual_seed(seed), dtype=th.float64).to(dtype)
        self.seen = []

    def forward(self, x, ts, y=None):
        self.seen.append(int(ts[0]))
        return th.cat([self.eps, th.zeros_like(self.eps)], dim=1)


@pytest.mark.parametrize("skip", [0, 25])
def test_restatement_round_trip_in_float64(skip):
    """reverse_loop up to level t0, then the oracle's unguided eta-0 DDIM steps back down, both in float64 (invert_ref.float64_tables: the
    oracle's own code with its table entries left unrounded).  With a constant eps every step is an affine map and the step down from
    level i + 1 is the exact inverse of the step up from level i, so what remains is rounding: 1e-9 is 4e6 float64 unit roundoffs over
    at most 2 x 49 steps whose coefficients stay below 160.  The float32 prototype of upstream's re-derived eps lost 2e-4 here.
    The state entering step index 0 is the image; that step's pred_xstart is not (the level offset)."""
    shape = (2, 3, 5, 7)
    ref = invert_ref.create_invert_diffusion(1000, "linear", "ddim50")
    image = th.tanh(th.randn(shape, generator=th.Generator().manual_seed(1), dtype=th.float64))
    model = ConstEps(shape, th.float64)
    t0 = ref.num_timesteps - 1 - skip
    with invert_ref.float64_tables():
        ups = list(ref.reverse_loop(model, image, skip_timesteps=skip))
        assert len(ups) == t0 and model.seen == [ref.timestep_map[i] for i in range(t0)]
        assert [sorted(o) for o in ups[:-1]] == [["pred_xstart", "sample"]] * (t0 - 1) and sorted(ups[-1]) == ["noise", "pred_xstart", "sample"]
        latent, noise = ups[-1]["sample"], ups[-1]["noise"]
        assert latent.dtype == th.float64
        x = latent
        for i in range(t0, 0, -1):
            t = th.tensor([i] * shape[0])
            x = ref.ddim_sample_with_grad(model, x, t, clip_denoised=False, cond_fn=None, model_kwargs={}, eta=0.0,
                                          noise=th.zeros_like(x))["sample"]
        err = (x - image).abs().max().item()
        print(f"round trip ddim50 skip {skip}: max |state entering step 0 - image| = {err:.3e}")
        assert err <= 1e-9
        # the level offset: step index 0 sees the image as a level-0 state and predicts sqrt_recip[0] image - sqrt_recipm1[0] eps
        t = th.zeros(shape[0], dtype=th.long)
        x0 = ref.ddim_sample_with_grad(model, x, t, clip_denoised=False, cond_fn=None, model_kwargs={}, eta=0.0,
                                       noise=th.zeros_like(x))["pred_xstart"]
        a, b = float(ref.sqrt_recip_alphas_cumprod[0]), float(ref.sqrt_recipm1_alphas_cumprod[0])
        assert (x0 - (a * image - b * model.eps)).abs().max().item() <= 1e-9
        assert (x0 - image + b * model.eps).abs().max().item() <= (a - 1) * image.abs().max().item() + 1e-9
        assert (x0 - image).abs().max().item() > 0.5 * b * model.eps.abs().max().item() > 1e-3
        # the implied noise q_samples the image to the latent
        assert (ref.q_sample(image, th.tensor([t0] * shape[0]), noise) - latent).abs().max().item() <= 1e-12 * (1 + latent.abs().max().item())


@pytest.mark.parametrize("spec", ["ddim50", "ddim20", "1000"])
def test_implied_noise_reproduces_the_latent_in_float32(spec):
    """noise = (latent - sa init) / sb, then sa init + sb noise, all float32: fl(sa init) is the same number both times and cancels; what is
    left are the roundings of the difference, the quotient, the product sb noise and the final sum, (3 |latent - sa init| + |latent|) 2^-24
    to first order, inside the bound 8 2^-24 (|latent| + |init|) asserted elementwise.  The same bound holds the start state of a sampling
    loop to the latent in tests/test_gpu_invert.py."""
    shape = (1, 3, 6, 10)
    ref = invert_ref.create_invert_diffusion(1000, "linear", spec)
    N = ref.num_timesteps
    image = th.tanh(th.randn(shape, generator=th.Generator().manual_seed(2)))
    model = ConstEps(shape, th.float32)
    worst = 0.0
    for skip in (0, N // 2):
        t0 = N - 1 - skip
        out = None
        for out in ref.reverse_loop(model, image, skip_timesteps=skip):
            pass
        latent, noise = out["sample"], out["noise"]
        assert latent.dtype == th.float32 and noise.dtype == th.float32
        again = ref.q_sample(image, th.tensor([t0]), noise)
        bound = 8 * 2.0 ** -24 * (latent.abs() + image.abs())
        ratio = ((again - latent).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (spec, skip, ratio)
    print(f"implied noise {spec}: worst |q_sample - latent| / bound = {worst:.3f}")


# ---- the invert= prefix ------------------------------------------------------------------------------------------------------------
def test_init_image_value_without_the_prefix_is_the_image():
    from cgd import script_util
    for v in ("photos/a.png", "https://example.org/a.png", "inverted.png", "a=invert=b.png"):
        assert script_util.split_init_invert(v) == (v, False)


def test_init_image_value_with_the_prefix_composes_with_the_mask():
    from cgd import script_util

    def parse(value):
        image, mask = script_util.split_init_mask(value)
        return script_util.split_init_invert(image) + (mask,)

    assert script_util.split_init_invert("invert=a.png") == ("a.png", True)
    assert parse("a.png") == ("a.png", False, None)
    assert parse("invert=a.png") == ("a.png", True, None)
    assert parse("invert=a.png::m.png") == ("a.png", True, "m.png")
    assert parse("a.png::m.png") == ("a.png", False, "m.png")
    assert parse("invert=https://example.org/a.png") == ("https://example.org/a.png", True, None)
    assert parse("invert=https://example.org/a.png::https://example.org/m.png") == \
        ("https://example.org/a.png", True, "https://example.org/m.png")
    assert parse("a.png::invert=m.png") == ("a.png", False, "invert=m.png")  # the prefix belongs to the image part only
    assert script_util.split_init_mask("invert=a.png::m.png") == ("invert=a.png", "m.png")  # split_init_mask is as it was


def test_a_bare_prefix_is_refused():
    from cgd import script_util
    with pytest.raises(ValueError):
        script_util.split_init_invert("invert=")
    with pytest.raises(ValueError):
        script_util.split_init_invert(script_util.split_init_mask("invert=::m.png")[0])


def test_cli_help_names_the_prefix():
    from cgd import cgd as mine
    assert "invert=IMAGE" in mine._CLI_SPEC and "invert=IMAGE::MASK" in mine._CLI_SPEC
    assert "invert=IMAGE" in re.sub(r"\s+", " ", mine.build_parser().format_help())


@pytest.mark.parametrize("respacing", ["250", "1000", "25,25"])
def test_generator_refuses_the_prefix_without_a_deterministic_sampler(respacing):
    from cgd import cgd as mine
    for value in ("invert=a.png", "invert=a.png::m.png"):
        with pytest.raises(ValueError, match=r"(?s)ddim.*plms"):
            next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", init_image=value, timestep_respacing=respacing))


@pytest.mark.parametrize("offsets", [dict(height_offset=64), dict(width_offset=-64)])
def test_generator_refuses_the_prefix_with_a_size_offset(offsets):
    from cgd import cgd as mine
    with pytest.raises(ValueError, match="offset"):
        next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", init_image="invert=a.png", timestep_respacing="ddim50", **offsets))


def test_generator_refuses_a_bare_prefix():
    from cgd import cgd as mine
    with pytest.raises(ValueError, match="invert=IMAGE"):
        next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", init_image="invert=", timestep_respacing="ddim50"))


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
    seen = []

    def forward(x, ts, y, out=None):
        seen.append((x.data_ptr(), ts.tolist(), y))
        return out

    return smp, lib, types.SimpleNamespace(forward=forward), seen


SHAPE = (2, 3, 4, 6)


def test_inversion_refuses_clipping_short_schedules_and_bad_images():
    smp, lib, model, _ = _rig()
    image = th.zeros(SHAPE)
    with pytest.raises(NotImplementedError):
        smp.ddim_reverse_sample_loop_progressive(model, image, clip_denoised=True, device="cpu")
    for skip in (9, 10, 50):  # t0 = 10 - 1 - skip < 1
        with pytest.raises(ValueError):
            smp.ddim_reverse_sample_loop_progressive(model, image, device="cpu", skip_timesteps=skip)
        with pytest.raises(ValueError):
            smp.ddim_invert(model, image, device="cpu", skip_timesteps=skip)
    with pytest.raises(ValueError):
        smp.ddim_reverse_sample_loop_progressive(model, image, device="cpu", skip_timesteps=-1)
    for bad in (th.zeros(3, 4, 6), th.zeros(2, 1, 4, 6), th.zeros(2, 6, 4, 6), th.zeros(2, 3, 4), th.zeros(0, 3, 4, 6), [[0.0]]):
        with pytest.raises(ValueError):
            smp.ddim_reverse_sample_loop_progressive(model, bad, device="cpu")
    assert not lib.calls
    assert len(list(smp.ddim_reverse_sample_loop_progressive(model, image, device="cpu", skip_timesteps=8))) == 1  # t0 == 1 runs


@pytest.mark.parametrize("skip", [0, 4])
def test_inversion_runs_indices_upwards_with_one_launch_each_and_draws_nothing(skip, monkeypatch):
    smp, lib, model, seen = _rig()
    tab = smp.tables
    t0 = 10 - 1 - skip
    image = th.tanh(th.randn(SHAPE, generator=th.Generator().manual_seed(4)))
    y = th.tensor([3, 5])

    def no_draw(*a, **k):
        raise AssertionError("the inversion draws nothing")

    th.manual_seed(9)
    with monkeypatch.context() as m:
        for name in ("randn", "randn_like", "randint", "rand", "rand_like", "normal"):
            m.setattr(th, name, no_draw)
        outs = list(smp.ddim_reverse_sample_loop_progressive(model, image, model_kwargs={"y": y}, device="cpu", skip_timesteps=skip))
    after = th.rand(1)
    th.manual_seed(9)
    assert th.equal(after, th.rand(1))  # the global stream is where it was
    assert len(outs) == t0
    assert [n for n, _ in lib.calls] == ["cgd_ddim_reverse_update"] * t0
    # args: ctx, x, out6, init, x_next, pred_xstart, noise_out, B, H, W, init_batch, k, stream
    calls = [a for _, a in lib.calls]
    for i, (a, out, (x_ptr, ts, y_seen)) in enumerate(zip(calls, outs, seen)):
        last = i == t0 - 1
        want = tab.reverse_coef(i)
        assert [getattr(a[11], f) for f, _ in L.ReverseCoef._fields_] == [getattr(want, f) for f, _ in L.ReverseCoef._fields_]
        assert ts == [float(tab.timestep_map[i])] * 2 and y_seen is y  # the model timestep of index i, y as given
        assert a[7:11] == (2, 4, 6, 2)
        assert a[1] == x_ptr and a[4] == out["sample"].data_ptr() and a[5] == out["pred_xstart"].data_ptr() and a[4] != a[1]
        assert (a[3] is not None) == last and (a[6] is not None) == last and ("noise" in out) == last
        if i:
            assert a[1] == calls[i - 1][4]  # the state of step i is what step i - 1 wrote
    assert calls[-1][6] == outs[-1]["noise"].data_ptr()
    assert len({a[2] for a in calls}) == 1  # one model-output buffer, read in place


def test_ddim_invert_returns_the_last_state_and_its_noise():
    smp, lib, model, _ = _rig()
    latent, noise = smp.ddim_invert(model, th.zeros(SHAPE), device="cpu", skip_timesteps=3)
    last = lib.calls[-1][1]
    assert len(lib.calls) == 6 and latent.data_ptr() == last[4] and noise.data_ptr() == last[6]
    assert tuple(latent.shape) == tuple(noise.shape) == SHAPE


def test_the_sampling_loops_are_as_they_were():
    """the inversion is an addition: a plain DDIM run issues the launches it issued before and never the new one"""
    smp, lib, model, _ = _rig()
    model.forward = lambda x, ts, y, out=None: out
    assert len(list(smp.ddim_sample_loop_progressive(model, SHAPE, clip_denoised=False, device="cpu"))) == 10
    assert [n for n, _ in lib.calls] == ["cgd_pmv_blend", "cgd_sample_update"] * 10


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_reverse_update_and_the_header_declares_it():
    handle = L.load()
    assert hasattr(handle, "cgd_ddim_reverse_update") and "cgd_ddim_reverse_update" in L.EXPORTED_SYMBOLS
    src = open(os.path.join(ROOT, "include", "cgd_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+cgd_ddim_reverse_update\s*\(", code) and re.search(r"\}\s*cgd_reverse_coef\s*;", code)
    body = re.search(r"typedef struct cgd_reverse_coef \{(.*?)\}", code, flags=re.S).group(1)
    assert re.findall(r"float\s+(\w+)\s*;", body) == [f for f, _ in L.ReverseCoef._fields_]
    assert [f for f, _ in L.ReverseCoef._fields_] == ["sqrt_recip", "sqrt_recipm1", "sqrt_ab_next", "sqrt_one_minus_ab_next",
                                                      "inv_sqrt_one_minus_ab_next"]


def test_a_null_context_or_coefficient_pointer_is_rejected():
    handle = L.load()
    assert handle.cgd_ddim_reverse_update(None, None, None, None, None, None, None, 1, 8, 8, 1, None, None) == -3
    assert handle.cgd_ddim_reverse_update(None, None, None, None, None, None, None, 1, 8, 8, 1, L.ReverseCoef(), None) == -3
