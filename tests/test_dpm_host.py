"""CPU tests of DPM-Solver++(2M) sampling on the logSNR-uniform spacing 'dpmN': the spacing and the step coefficients of
cgd_amd.diffusion, the restatement (tests/dpm_ref.py) against the oracle's DDIM step and against the closed form of a Gaussian toy, and the
host logic of `GuidedSampler.dpmpp_sample_loop_progressive` and of the drop-in generator, driven with a recording fake library (no GPU)."""
import math
import types

import numpy as np
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from cgd_amd import guidance as dg
from oracle import diffusion as od
from tests import dpm_ref
from tests.test_plms_host import ToyModel, toy_cond_fn


# ---- spacing -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,levels", [(10, 10), (20, 20), (25, 25), (50, 49), (100, 94)])
def test_logsnr_spacing_level_counts_on_the_linear_schedule(n, levels):
    betas = dd.named_beta_schedule("linear", 1000)
    kept = dd.space_timesteps(1000, f"dpm{n}", betas=betas)
    assert len(kept) == levels and kept == dpm_ref.logsnr_timesteps(od.get_named_beta_schedule("linear", 1000), n)
    assert dd.space_timesteps(1000, f"dpmsde{n}", betas=betas) == kept
    tab = dd.create_gaussian_diffusion(1000, "linear", f"dpm{n}")
    assert tab.num_timesteps == levels and tab.timestep_map == sorted(kept)
    assert dd.create_gaussian_diffusion(1000, "linear", f"dpmsde{n}").timestep_map == tab.timestep_map


@pytest.mark.parametrize("schedule", ["linear", "cosine"])
@pytest.mark.parametrize("n", [2, 3, 8, 20, 50, 250])
def test_logsnr_spacing_holds_both_ends_and_is_uniform_in_lambda(schedule, n):
    tab = dd.create_gaussian_diffusion(1000, schedule, f"dpm{n}")
    tmap = tab.timestep_map
    assert tmap[0] == 0 and tmap[-1] == 999 and 2 <= len(tmap) <= n
    assert all(a < b for a, b in zip(tmap, tmap[1:]))
    assert tmap == sorted(dpm_ref.logsnr_timesteps(od.get_named_beta_schedule(schedule, 1000), n))
    # every kept level is the nearest timestep to one of the uniform targets: no target is further from its level than from any other timestep
    base = np.cumprod(1.0 - dd.named_beta_schedule(schedule, 1000))
    lam = 0.5 * np.log(base / (1.0 - base))
    assert np.allclose(tab.alphas_cumprod, base[tmap], rtol=1e-12)
    for target in np.linspace(lam[0], lam[-1], n):
        assert np.abs(lam[tmap] - target).min() == np.abs(lam - target).min()


def test_logsnr_spacing_refusals_and_untouched_specs():
    betas = dd.named_beta_schedule("linear", 1000)
    for spec in ("dpm1", "dpm0", "dpmsde1"):
        with pytest.raises(ValueError):
            dd.space_timesteps(1000, spec, betas=betas)
        with pytest.raises(ValueError):
            dd.create_gaussian_diffusion(1000, "linear", spec)
    for spec in ("dpm20", "dpmsde20"):
        with pytest.raises(ValueError, match="betas"):
            dd.space_timesteps(1000, spec)
    with pytest.raises(ValueError):
        dd.space_timesteps(1000, "dpm20", betas=betas[:500])
    for spec in ("ddim10", "ddim50", "ddim250", "plms25", "250", "25,25", "10,15,20"):
        ora = od.space_timesteps(1000, spec.replace("plms", "ddim"))
        assert dd.space_timesteps(1000, spec) == ora == dd.space_timesteps(1000, spec, betas=betas)


# ---- coefficients --------------------------------------------------------------------------------------------------------------------
SPECS = [("linear", "dpm20"), ("cosine", "dpm20"), ("linear", "ddim50"), ("linear", "dpm8")]


@pytest.mark.parametrize("schedule,spec", SPECS)
def test_eta0_identity_and_the_restatement(schedule, spec):
    tab = dd.create_gaussian_diffusion(1000, schedule, spec)
    ref = dpm_ref.create_dpm_diffusion(1000, schedule, spec)
    assert ref.timestep_map == tab.timestep_map
    for i in range(1, tab.num_timesteps):
        for order in (1, 2):
            if order == 2 and i == tab.num_timesteps - 1:
                with pytest.raises(ValueError):
                    tab.dpmpp_coef_f64(i, 2, 0.0)
                continue
            for eta in (0.0, 0.5, 1.0):
                c = tab.dpmpp_coef_f64(i, order, eta)
                assert c == pytest.approx(ref.step_coefs(i, order, eta), rel=1e-12, abs=1e-15)
                k = tab.dpmpp_coef(i, order, eta)
                assert (k.c_x, k.c_d, k.c_r, k.c_n) == pytest.approx(c, rel=1e-6, abs=1e-12)
            c_x, c_d, c_r, c_n = tab.dpmpp_coef_f64(i, order, 0.0)
            assert c_d == pytest.approx(math.sqrt(tab.alphas_cumprod_prev[i]) - c_x * math.sqrt(tab.alphas_cumprod[i]), rel=1e-12, abs=1e-14)
            assert c_n == 0.0 and (c_r > 0.0) == (order == 2)
    if (schedule, spec) == ("linear", "dpm20"):  # uniform in lambda up to the rounding to timesteps: the extrapolation weight stays near 1/2
        inner = [tab.dpmpp_coef_f64(i, 2, 0.0)[2] for i in range(3, tab.num_timesteps - 1)]
        assert 0.3 < min(inner) and max(inner) < 0.8


@pytest.mark.parametrize("schedule,spec", SPECS)
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_order1_is_the_oracles_ddim_step(schedule, spec, eta):
    """mean = sqrt(abar_prev) x0 + sqrt(1 - abar_prev - sigma^2) eps with eps = (x - alpha x0) / sigma_t, noise scale sigma: the
    coefficients of x, x0 and the noise from the oracle's float64 tables"""
    tab = dd.create_gaussian_diffusion(1000, schedule, spec)
    ora = dpm_ref.create_dpm_diffusion(1000, schedule, spec)  # an oracle SpacedDiffusion on the kept timesteps
    for i in range(1, tab.num_timesteps):
        ab, abp = ora.alphas_cumprod[i], ora.alphas_cumprod_prev[i]
        sigma = eta * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
        dirc = math.sqrt(1 - abp - sigma ** 2)
        want = (dirc / math.sqrt(1 - ab), math.sqrt(abp) - dirc * math.sqrt(ab) / math.sqrt(1 - ab), 0.0, sigma)
        assert tab.dpmpp_coef_f64(i, 1, eta) == pytest.approx(want, rel=1e-12, abs=1e-12)
        assert ora.step_coefs(i, 1, eta) == pytest.approx(want, rel=1e-12, abs=1e-12)


def test_coefficients_at_the_clean_end_and_bad_arguments():
    tab = dd.create_gaussian_diffusion(1000, "linear", "dpm20")
    for order, eta in ((1, 0.0), (2, 0.0), (2, 1.0), (1, 3.0)):
        assert tab.dpmpp_coef_f64(0, order, eta) == (0.0, 1.0, 0.0, 0.0)
        k = tab.dpmpp_coef(0, order, eta)
        assert (k.c_x, k.c_d, k.c_r, k.c_n) == (0.0, 1.0, 0.0, 0.0)
    assert dpm_ref.coefs(0.9, 1.0, 0.5, 2, 1.0) == (0.0, 1.0, 0.0, 0.0)
    for order in (0, 3, "2"):
        with pytest.raises(ValueError):
            tab.dpmpp_coef(5, order, 0.0)
    with pytest.raises(ValueError):
        tab.dpmpp_coef(5, 2, -0.5)


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_restatement_order1_runs_the_oracles_ddim_loop(eta):
    """whole loops on the toy network with a guidance function: order 1 with eta in {0, 1} against ddim_sample_with_grad"""
    import functools
    ref = dpm_ref.create_dpm_diffusion(1000, "linear", "ddim10")
    ora = od.create_gaussian_diffusion(1000, "linear", "ddim10")
    gen = th.Generator().manual_seed(3)
    shape = (2, 3, 4, 5)
    tape = {"x_T": th.randn(shape, generator=gen), "noise": [th.randn(shape, generator=gen) for _ in range(10)],
            "y": [th.randint(0, 3, (2,), generator=gen) for _ in range(10)]}
    kw = dict(clip_denoised=False, model_kwargs={"y": th.zeros(2, dtype=th.long)}, device="cpu", randomize_class=True, cond_fn_with_grad=True)
    m1, c1, m2, c2 = ToyModel(), [], ToyModel(), []
    a = list(ref.dpmpp_sample_loop_progressive(m1, shape, cond_fn=toy_cond_fn(c1), order=1, eta=eta, tape=tape, **kw))
    b = list(ora._loop(functools.partial(ora.ddim_sample_with_grad, eta=eta), m2, shape, None, False, toy_cond_fn(c2), kw["model_kwargs"],
                       "cpu", 0, None, True, tape))
    assert m1.seen == m2.seen and c1 == c2 and len(a) == len(b) == 10
    assert th.equal(a[0]["pred_xstart"], b[0]["pred_xstart"])  # the same evaluation; later ones see states that differ by rounding
    for p, d in zip(a, b):
        assert th.allclose(p["sample"], d["sample"], rtol=1e-5, atol=1e-5)
        assert th.allclose(p["pred_xstart"], d["pred_xstart"], rtol=1e-5, atol=1e-5)


# ---- convergence on the Gaussian toy -------------------------------------------------------------------------------------------------
def test_toy_second_order_on_dpm20_beats_first_order_on_ddim100():
    e2, e1 = dpm_ref.toy_error("dpm20", 2), dpm_ref.toy_error("ddim100", 1)
    print(f"toy max error: order 2 on dpm20 {e2:.4f}, order 1 on ddim100 {e1:.4f}")
    assert e2 < e1
    assert e2 == pytest.approx(0.028, abs=2e-3) and e1 == pytest.approx(0.055, abs=2e-3)  # the figures of DESIGN.md's table


def test_toy_orders_of_convergence():
    e = {(spec, o): dpm_ref.toy_error(spec, o) for spec in ("ddim250", "ddim500") for o in (1, 2)}
    r1, r2 = e["ddim250", 1] / e["ddim500", 1], e["ddim250", 2] / e["ddim500", 2]
    print(f"toy error ratio ddim250 / ddim500: order 1 {r1:.2f}, order 2 {r2:.2f}")
    assert r2 >= 3.0 and r1 < 2.5


def test_toy_stride_spacing_gains_nothing_at_20_levels():
    """the finding that ties the solver to its spacing: on 'ddim20' the second order is no better than the first"""
    assert dpm_ref.toy_error("ddim20", 2) > 0.9 * dpm_ref.toy_error("ddim20", 1)
    assert dpm_ref.toy_error("dpm20", 2) < 0.2 * dpm_ref.toy_error("dpm20", 1)


# ---- host logic of the device sampler ------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _native_rig(spec="dpm10"):
    from cgd_amd import sampler
    lib = Recorder()
    events = lib.calls
    ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", spec, False))
    guid = object.__new__(dg.ClipGuidance)
    guid.use_magnitude, guid.scalars, guid.current_timestep = False, th.zeros(8), smp.num_timesteps - 1

    def native(x, x0, x_in, coef):
        events.append(("cond_fn", guid.current_timestep))
        return th.ones_like(x)

    guid.native = native

    def forward(x, ts, y, out=None):
        events.append(("forward", float(ts[0])))
        return out

    model = types.SimpleNamespace(forward=forward, num_classes=5)
    draws = []
    plain = smp._draw_like

    def draw(x):
        events.append(("draw", None))
        draws.append(plain(x))
        return draws[-1]

    smp._draw_like = draw
    return smp, guid, model, events, draws


def _run_native(smp, guid, model, **kw):
    gen = smp.dpmpp_sample_loop_progressive(model, (1, 3, 4, 6), clip_denoised=False, cond_fn=guid,
                                            model_kwargs={"y": th.zeros(1, dtype=th.long)}, device="cpu", randomize_class=True,
                                            cond_fn_with_grad=True, **kw)
    outs = []
    for out in gen:
        outs.append(out)
        guid.current_timestep -= 1
    return outs


# args of cgd_dpmpp_update: ctx, x, x0, g, scalars, noise, x0_hist, x0c_out, sample, x0_out, B, H, W, k, d, stream
X, NOISE, HIST, X0C, SAMPLE, K, D = 1, 5, 6, 7, 8, 13, 14


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_native_call_sequence_orders_history_and_draws(eta):
    smp, guid, model, events, draws = _native_rig()
    tab = smp.tables
    N = tab.num_timesteps
    assert N == 10
    th.manual_seed(11)
    outs = _run_native(smp, guid, model, order=2, eta=eta)
    after = th.rand(1)
    assert len(outs) == N
    # per step: one forward at the level's model timestep, the blend, (the noise draw,) cond_fn, one update
    per_step = ["forward", "cgd_pmv_blend"] + (["draw"] if eta else []) + ["cond_fn", "cgd_dpmpp_update"]
    assert [n for n, _ in events] == per_step * N
    assert [a for n, a in events if n == "forward"] == [float(tab.timestep_map[i]) for i in range(N - 1, -1, -1)]
    assert [a for n, a in events if n == "cond_fn"] == list(range(N - 1, -1, -1))
    ups = [a for n, a in events if n == "cgd_dpmpp_update"]
    prev = None
    written = set()
    for step, u in enumerate(ups):
        i = N - 1 - step
        eff = 1 if (step == 0 or i == 0) else 2  # no history on the first step; lower order final
        want = tab.dpmpp_coef_f64(i, eff, eta)
        d = u[D]
        assert (d.c_x, d.c_d, d.c_r, d.c_n) == pytest.approx(want, rel=1e-6, abs=1e-12)
        assert (d.c_r != 0.0) == (eff == 2)
        assert u[K].nonzero == int(i != 0) and u[K].sqrt_recip == pytest.approx(tab.sqrt_recip_alphas_cumprod[i], rel=1e-6)
        # the state fed in is the sample of the step before; the history read is the entry the step before wrote
        assert u[X] == (outs[step - 1]["sample"].data_ptr() if step else u[X])
        assert u[HIST] == (prev if eff == 2 else None)
        assert (u[X0C] is not None) == (i > 1)  # nothing reads the entries of step indices 1 and 0
        assert u[X0C] is None or u[X0C] not in (prev, u[X], u[SAMPLE])
        assert u[SAMPLE] == outs[step]["sample"].data_ptr() and u[9] == outs[step]["pred_xstart"].data_ptr()
        assert (u[NOISE] is not None) == bool(eta)
        if eta:
            assert u[NOISE] == draws[step].data_ptr()  # the draw of this evaluation, taken before cond_fn
        prev = u[X0C]
        written.add(u[X0C])
    assert len(written - {None}) == 2  # two buffers rotate by pointer, nothing is copied
    assert len(draws) == (N if eta else 0)
    # the generator saw x_T, then per step the class labels (and the step noise): nothing else
    th.manual_seed(11)
    th.randn(1, 3, 4, 6)
    for _ in range(N):
        th.randint(0, 5, (1,))
        if eta:
            th.randn(1, 3, 4, 6)
    assert th.equal(after, th.rand(1))


def test_native_order1_never_reads_or_writes_history():
    smp, guid, model, events, _ = _native_rig()
    outs = _run_native(smp, guid, model, order=1)
    ups = [a for n, a in events if n == "cgd_dpmpp_update"]
    assert len(outs) == len(ups) == 10
    assert all(u[HIST] is None and u[X0C] is None and u[D].c_r == 0.0 and u[NOISE] is None for u in ups)


def test_tape_replay_reads_the_step_noise_per_evaluation_only_with_eta():
    shape = (1, 3, 4, 6)
    gen = th.Generator().manual_seed(5)
    for eta in (0.0, 0.7):
        smp, guid, model, events, draws = _native_rig()
        smp.tape = {"x_T": th.randn(shape, generator=gen), "y": [th.zeros(1, dtype=th.long)] * 10,
                    "noise": [th.randn(shape, generator=gen) for _ in range(10)] if eta else []}
        _run_native(smp, guid, model, eta=eta, skip_timesteps=3, init_image=th.zeros(shape))
        ups = [a for n, a in events if n == "cgd_dpmpp_update"]
        assert len(ups) == 7 and not draws
        assert ups[0][D].c_r == 0.0 and all(u[D].c_r != 0.0 for u in ups[1:-1]) and ups[-1][D].c_r == 0.0
        assert all((u[NOISE] is not None) == bool(eta) for u in ups)


def test_masked_run_merges_after_every_update_and_keeps_the_initial_noise_at_eta0():
    shape = (1, 3, 4, 6)
    mask = th.zeros(1, 1, 4, 6)
    mask[..., :3] = 1.0
    init = th.rand(shape)
    for eta in (0.0, 1.0):
        smp, guid, model, events, draws = _native_rig()
        x_T = th.randn(shape)
        _run_native(smp, guid, model, eta=eta, noise=x_T, init_image=init, mask=mask)
        names = [n for n, _ in events if n.startswith("cgd_") and n != "cgd_pmv_blend"]
        assert names == ["cgd_dpmpp_update", "cgd_masked_merge"] * 10
        merges = [a for n, a in events if n == "cgd_masked_merge"]
        ups = [a for n, a in events if n == "cgd_dpmpp_update"]
        for step, (u, m) in enumerate(zip(ups, merges)):
            assert m[1] == u[SAMPLE] and m[2] == u[9]  # merged in place; the history entry (u[X0C]) is not touched
            last = step == 9
            if eta:
                assert len(draws) == 20 and (m[5] is None if last else m[5] == draws[2 * step + 1].data_ptr())
            else:
                assert not draws and (m[5] is None if last else m[5] == x_T.data_ptr())
    with pytest.raises(ValueError, match="DDIM"):
        smp.dpmpp_sample_loop_progressive(model, shape, clip_denoised=False, cond_fn=guid, cond_fn_with_grad=True, init_image=init,
                                          mask=mask, resamples=2)
    with pytest.raises(ValueError):
        smp.dpmpp_sample_loop_progressive(model, shape, clip_denoised=False, cond_fn=guid, cond_fn_with_grad=True, mask=mask)


def test_refusals():
    smp, guid, model, _, _ = _native_rig()
    kw = dict(clip_denoised=False, cond_fn=guid, cond_fn_with_grad=True)
    for bad in (0, 3, 2.0, "2", True, None):
        with pytest.raises(ValueError):
            smp.dpmpp_sample_loop_progressive(model, (1, 3, 4, 6), order=bad, **kw)
    for bad in (-0.1, float("nan"), "1", None, True):
        with pytest.raises(ValueError):
            smp.dpmpp_sample_loop_progressive(model, (1, 3, 4, 6), eta=bad, **kw)
    with pytest.raises(ValueError):
        smp.dpmpp_sample_loop_progressive(model, (1, 3, 4, 6), resamples=2, **kw)
    with pytest.raises(NotImplementedError):
        smp.dpmpp_sample_loop_progressive(model, (1, 3, 4, 6), clip_denoised=True, cond_fn=guid, cond_fn_with_grad=True)
    with pytest.raises(NotImplementedError):
        smp.dpmpp_sample_loop_progressive(model, (1, 3, 4, 6), clip_denoised=False, cond_fn=guid, cond_fn_with_grad=False)


def test_generic_cond_fn_path_runs_one_evaluation_per_step():
    from cgd_amd import sampler
    lib = Recorder()
    ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "dpm10", False))
    seen = []

    def model(x, ts, y):
        return th.cat([0.5 * x, th.zeros_like(x)], dim=1)

    def cond_fn(x, t, out, y=None):
        seen.append(int(t[0]))
        return -th.autograd.grad(out["pred_xstart"].sum(), x)[0]

    outs = list(smp.dpmpp_sample_loop_progressive(model, (1, 3, 4, 4), clip_denoised=False, cond_fn=cond_fn, device="cpu",
                                                  cond_fn_with_grad=True, eta=1.0))
    assert len(outs) == 10 and seen == list(range(9, -1, -1))
    assert [n for n, _ in lib.calls] == ["cgd_dpmpp_update"] * 10
    assert all(a[3] is not None and a[NOISE] is not None for _, a in lib.calls)  # cond_fn's gradient and the step noise reach the launch


def test_existing_loops_issue_the_launches_they_issued():
    from cgd_amd import sampler
    for name, want in (("p_sample_loop_progressive", "cgd_sample_update"), ("ddim_sample_loop_progressive", "cgd_sample_update"),
                       ("plms_sample_loop_progressive", "cgd_multistep_update")):
        lib = Recorder()
        ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
        smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "ddim10", False))
        model = types.SimpleNamespace(forward=lambda x, ts, y, out=None: out)
        list(getattr(smp, name)(model, (1, 3, 4, 4), clip_denoised=False, device="cpu"))
        assert {n for n, _ in lib.calls} == {"cgd_pmv_blend", want}


# ---- the drop-in generator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,expect", [("dpm10", ("dpm", 2, 0.0)), ("dpmsde10", ("dpm", 2, 1.0)), ("plms10", ("plms", 2, None)),
                                         ("ddim10", ("ddim", None, None)), ("10", ("p", None, None))])
def test_dropin_generator_routes_respacing_to_its_loop(spec, expect, tmp_path, monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    used = []

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

    def fake_loop(kind):
        def loop(model, shape, order=None, eta=None, **kw):
            used.append((kind, order, eta))
            for i in range(3):
                yield {"sample": th.zeros(shape), "pred_xstart": th.zeros(shape)}
        return loop

    diffusion = types.SimpleNamespace(num_timesteps=3, p_sample_loop_progressive=fake_loop("p"),
                                      ddim_sample_loop_progressive=fake_loop("ddim"), plms_sample_loop_progressive=fake_loop("plms"),
                                      dpmpp_sample_loop_progressive=fake_loop("dpm"))
    seen_spec = []

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
    assert used == [expect] and len(items) == 3 and seen_spec == [spec]  # the tables are built from the same spec


def test_inverted_init_images_go_with_dpm_but_not_with_dpmsde():
    from cgd import cgd as mine
    for value in ("invert=a.png", "invert=a.png::m.png"):
        with pytest.raises(ValueError, match=r"(?s)ddim.*plms.*dpmsde"):
            next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", init_image=value, timestep_respacing="dpmsde20"))
        # 'dpm20' passes the sampler check: the next refusal of the same prologue is the one about the size offset
        with pytest.raises(ValueError, match="offset"):
            next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", init_image=value, timestep_respacing="dpm20", height_offset=64))


def test_cli_help_names_dpm_and_keeps_plms():
    import re
    from cgd import cgd as mine
    assert "dpm20" in mine._CLI_SPEC and "dpmsde" in mine._CLI_SPEC and "plms50" in mine._CLI_SPEC
    text = re.sub(r"\s+", " ", mine.build_parser().format_help())
    assert "dpm20" in text and "plms50" in text


def test_library_binding_and_header_declare_the_entry():
    import os
    from cgd_amd import lib as L
    assert "cgd_dpmpp_update" in L.EXPORTED_SYMBOLS
    assert [f[0] for f in L.Dpmpp._fields_] == ["c_x", "c_d", "c_r", "c_n"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "cgd_mi355x.h")).read()
    assert "int cgd_dpmpp_update(" in header and "} cgd_dpmpp;" in header
    assert " dpm " in open(os.path.join(root, "clip-guided-diffusion_amd", "csrc", "build.sh")).read()
