"""CPU tests of PLMS sampling and DDIM with eta > 0: the restatement (tests/plms_ref.py) against the oracle, and the host logic of
`GuidedSampler.plms_sample_loop_progressive` / `ddim_sample_loop_progressive(eta=...)` and of the drop-in generator, driven with a
recording fake library (no GPU)."""
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from cgd_amd import guidance as dg
from oracle import diffusion as od
from tests import plms_ref


# ---- the restatement --------------------------------------------------------------------------------------------------------
class ToyModel(th.nn.Module):
    """eps-prediction toy with a learned-range head that roughly predicts the noise of x (so that pred_xstart stays O(1) along the
    trajectory); records the (original) timesteps it is evaluated at"""
    num_classes = 3

    def __init__(self):
        super().__init__()
        self.w = th.nn.Parameter(th.tensor(0.1))
        self.abar = th.from_numpy(od.GaussianDiffusion(od.get_named_beta_schedule("linear", 1000)).alphas_cumprod).float()
        self.seen = []

    def forward(self, x, ts, y=None):
        self.seen.append(int(ts[0]))
        c = (1 - self.abar[ts.long()]).sqrt().view(-1, 1, 1, 1)
        return th.cat([c * x + self.w * th.tanh(x), th.tanh(x)], dim=1)


def toy_cond_fn(calls):
    def cond_fn(x, t, out, y=None):
        calls.append(int(t[0]))
        return -th.autograd.grad((out["pred_xstart"] ** 2).sum(), x)[0] * 0.05
    return cond_fn


def _toy_run(diff, loop, order=None, **kw):
    model, calls = ToyModel(), []
    gen = th.Generator().manual_seed(3)
    shape = (2, 3, 4, 5)
    tape = {"x_T": th.randn(shape, generator=gen), "noise": [th.randn(shape, generator=gen) for _ in range(diff.num_timesteps)],
            "y": [th.randint(0, 3, (2,), generator=gen) for _ in range(diff.num_timesteps)]}
    extra = {} if order is None else {"order": order}
    outs = list(loop(model, shape, clip_denoised=False, cond_fn=toy_cond_fn(calls), model_kwargs={"y": th.zeros(2, dtype=th.long)},
                     device="cpu", randomize_class=True, cond_fn_with_grad=True, tape=tape, **extra, **kw))
    return outs, model.seen, calls


def test_restatement_order1_is_ddim_eta0():
    ref = plms_ref.create_plms_diffusion(1000, "linear", "plms10")
    ora = od.create_gaussian_diffusion(1000, "linear", "ddim10")
    p_outs, p_seen, p_calls = _toy_run(ref, ref.plms_sample_loop_progressive, order=1)
    d_outs, d_seen, d_calls = _toy_run(ora, ora.ddim_sample_loop_progressive)
    assert p_seen == d_seen and p_calls == d_calls and len(p_outs) == len(d_outs) == 10
    for p, d in zip(p_outs, d_outs):
        assert th.allclose(p["sample"], d["sample"], rtol=1e-5, atol=1e-5)
        assert th.equal(p["pred_xstart"], d["pred_xstart"])


@pytest.mark.parametrize("order", [2, 3, 4])
def test_restatement_counts_evaluations_calls_and_timesteps(order):
    ref = plms_ref.create_plms_diffusion(1000, "linear", "plms10")
    outs, seen, calls = _toy_run(ref, ref.plms_sample_loop_progressive, order=order)
    # 10 steps, 11 evaluations: the start step also evaluates at t - 1 (its model timestep: the respaced map of t - 1)
    assert len(outs) == 10 and ref.evaluations == 11
    assert calls == [9, 8] + list(range(8, -1, -1))
    assert seen == [ref.timestep_map[t] for t in calls]
    assert all(len(o["old_eps"]) <= order - 1 for o in outs)
    assert all(th.isfinite(o["sample"]).all() for o in outs)


def test_restatement_refuses_bad_orders_and_one_step_schedules():
    ref = plms_ref.create_plms_diffusion(1000, "linear", "plms10")
    for bad in (0, 5, 2.0, True):
        with pytest.raises(ValueError):
            ref.plms_sample_loop_progressive(ToyModel(), (1, 3, 4, 4), clip_denoised=False, order=bad)
    with pytest.raises(ValueError):
        ref.plms_sample_loop_progressive(ToyModel(), (1, 3, 4, 4), clip_denoised=False, skip_timesteps=9, order=2)


@pytest.mark.parametrize("n", ["10", "25", "50", "250"])
def test_plms_spacing_equals_ddim_spacing(n):
    assert dd.space_timesteps(1000, "plms" + n) == dd.space_timesteps(1000, "ddim" + n) == od.space_timesteps(1000, "ddim" + n)
    assert plms_ref.space_timesteps(1000, "plms" + n) == od.space_timesteps(1000, "ddim" + n)
    a, b = dd.create_gaussian_diffusion(1000, "linear", "plms" + n), dd.create_gaussian_diffusion(1000, "linear", "ddim" + n)
    assert a.timestep_map == b.timestep_map and (a.alphas_cumprod == b.alphas_cumprod).all()


# ---- host logic of the device sampler ------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _native_rig(spec="plms10"):
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
    smp._draw_like = lambda x: pytest.fail("PLMS draws no per-step noise")
    return smp, guid, model, events


def _run_native(smp, guid, model, **kw):
    gen = smp.plms_sample_loop_progressive(model, (1, 3, 4, 6), clip_denoised=False, cond_fn=guid,
                                           model_kwargs={"y": th.zeros(1, dtype=th.long)}, device="cpu", randomize_class=True,
                                           cond_fn_with_grad=True, **kw)
    outs = []
    for out in gen:  # the drop-in generator's closure counter: one decrement per yielded sample
        outs.append(out)
        guid.current_timestep -= 1
    return outs


@pytest.mark.parametrize("order", [2, 4])
def test_plms_native_call_sequence_phases_and_history(order):
    smp, guid, model, events = _native_rig()
    th.manual_seed(11)
    outs = _run_native(smp, guid, model, order=order)
    after = th.rand(1)
    assert len(outs) == 10
    # no random draw but x_T and the per-step class labels
    th.manual_seed(11)
    th.randn(1, 3, 4, 6)
    for _ in range(10):
        th.randint(0, 5, (1,))
    expect_next = th.rand(1)
    # the calls grouped by step: a step ends with the update that writes its sample (phase 0, or 2 on the start step)
    steps, cur = [], {"forward": [], "cond": [], "updates": []}
    for name, arg in events:
        if name == "forward":
            cur["forward"].append(arg)
        elif name == "cond_fn":
            cur["cond"].append(arg)
        elif name == "cgd_multistep_update":
            cur["updates"].append(arg)
            if arg[16].phase in (0, 2):
                steps.append(cur)
                cur = {"forward": [], "cond": [], "updates": []}
        elif name != "cgd_pmv_blend":
            pytest.fail(f"unexpected library call {name}")
    assert len(steps) == 10 and cur == {"forward": [], "cond": [], "updates": []}
    tmap = smp.tables.timestep_map
    # the start step: two forwards (t = 9 and t = 8) and two cond_fn calls seeing the same closure counter, then one of each per step
    first = steps[0]
    assert first["forward"] == [float(tmap[9]), float(tmap[8])] and first["cond"] == [9, 9]
    assert [len(s["forward"]) for s in steps] == [2] + [1] * 9 and [s["cond"] for s in steps[1:]] == [[k] for k in range(8, -1, -1)]
    # phases, orders and history pointers of cgd_multistep_update (args: ctx, x, x_eval, x0, g, scalars, noise, hist, eps_out, sample,
    # x0_out, B, H, W, k, k_step, m, stream)
    p1, p2 = first["updates"]
    assert p1[16].phase == 1 and p1[8] is not None and p1[2] is None and p1[6] is None
    assert p2[16].phase == 2 and p2[7][0] == p1[8] and p2[2] == p1[9] and p2[8] is None and p2[10] is None
    assert p2[14].sqrt_recip == pytest.approx(smp.tables.sqrt_recip_alphas_cumprod[8], rel=1e-6)
    assert p2[15].sqrt_recip == pytest.approx(smp.tables.sqrt_recip_alphas_cumprod[9], rel=1e-6)
    hist = [p1[8]]
    ptrs = {p1[8]}
    for n, s in enumerate(steps[1:], start=1):
        (u,) = s["updates"]
        m = u[16]
        assert m.phase == 0 and m.order == min(order, len(hist) + 1)
        newest_first = hist[::-1]
        assert [u[7][j] for j in range(m.order - 1)] == newest_first[:m.order - 1]
        assert u[8] not in hist and u[6] is None
        hist.append(u[8])
        ptrs.add(u[8])
        if len(hist) >= order:
            hist.pop(0)
    assert len(ptrs) == order  # the history rotates through `order` buffers by pointer
    assert th.equal(after, expect_next)


def test_plms_order1_is_adams_bashforth_only():
    smp, guid, model, events = _native_rig()
    _run_native(smp, guid, model, order=1)
    ups = [a for n, a in events if n == "cgd_multistep_update"]
    assert len(ups) == 10 and all(a[16].phase == 0 and a[16].order == 1 for a in ups)
    assert sum(n == "forward" for n, _ in events) == 10


def test_plms_refuses_bad_orders_and_one_step_schedules():
    smp, guid, model, _ = _native_rig()
    for bad in (0, 5, 2.0, "2", True):
        with pytest.raises(ValueError):
            smp.plms_sample_loop_progressive(model, (1, 3, 4, 6), clip_denoised=False, cond_fn=guid, cond_fn_with_grad=True, order=bad)
    with pytest.raises(ValueError):
        smp.plms_sample_loop_progressive(model, (1, 3, 4, 6), clip_denoised=False, cond_fn=guid, cond_fn_with_grad=True,
                                         skip_timesteps=9, order=2)
    one, guid1, model1, _ = _native_rig("1")
    with pytest.raises(ValueError):
        one.plms_sample_loop_progressive(model1, (1, 3, 4, 6), clip_denoised=False, cond_fn=guid1, cond_fn_with_grad=True)
    assert len(_run_native(one, guid1, model1, order=1)) == 1
    with pytest.raises(NotImplementedError):
        smp.plms_sample_loop_progressive(model, (1, 3, 4, 6), clip_denoised=True, cond_fn=guid, cond_fn_with_grad=True)


def test_plms_generic_cond_fn_path_runs_two_evaluations_on_the_start_step(monkeypatch):
    from cgd_amd import sampler
    lib = Recorder()
    ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "plms10", False))
    seen = []

    def model(x, ts, y):
        return th.cat([0.5 * x, th.zeros_like(x)], dim=1)

    def cond_fn(x, t, out, y=None):
        seen.append(int(t[0]))
        return -th.autograd.grad(out["pred_xstart"].sum(), x)[0]

    outs = list(smp.plms_sample_loop_progressive(model, (1, 3, 4, 4), clip_denoised=False, cond_fn=cond_fn, device="cpu",
                                                 cond_fn_with_grad=True, order=3))
    assert len(outs) == 10 and seen == [9, 8] + list(range(8, -1, -1))
    phases = [a[16].phase for n, a in lib.calls if n == "cgd_multistep_update"]
    assert phases == [1, 2] + [0] * 9 and all(n == "cgd_multistep_update" for n, _ in lib.calls)


def test_ddim_eta_routes_to_the_multistep_entry():
    import math
    from cgd_amd import sampler
    for eta in (0.0, 0.5):
        lib = Recorder()
        ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
        smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "ddim10", False))
        model = types.SimpleNamespace(forward=lambda x, ts, y, out=None: out)
        outs = list(smp.ddim_sample_loop_progressive(model, (1, 3, 4, 4), clip_denoised=False, device="cpu", eta=eta))
        assert len(outs) == 10
        names = [n for n, _ in lib.calls]
        if eta == 0.0:
            assert names == ["cgd_pmv_blend", "cgd_sample_update"] * 10
            assert all(a[-2] == 1 for n, a in lib.calls if n == "cgd_sample_update")
        else:
            assert names == ["cgd_pmv_blend", "cgd_multistep_update"] * 10
            tb = smp.tables
            for step, (n, a) in enumerate(c for c in lib.calls if c[0] == "cgd_multistep_update"):
                i = 9 - step
                ab, abp = tb.alphas_cumprod[i], tb.alphas_cumprod_prev[i]
                sigma = eta * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
                m = a[16]
                assert m.phase == 3 and m.sigma == pytest.approx(sigma, rel=1e-6, abs=1e-12)
                assert m.dir == pytest.approx(math.sqrt(1 - abp - sigma ** 2), rel=1e-6, abs=1e-12)
                assert a[6] is not None  # this loop's per-step noise draw
    with pytest.raises(ValueError):
        smp.ddim_sample_loop_progressive(model, (1, 3, 4, 4), clip_denoised=False, device="cpu", eta=-0.1)


# ---- the drop-in generator -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,expect", [("plms10", ("plms", 2)), ("ddim10", ("ddim", None)), ("10", ("p", None))])
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
        def loop(model, shape, order=None, **kw):
            used.append((kind, order))
            for i in range(3):
                yield {"sample": th.zeros(shape), "pred_xstart": th.zeros(shape)}
        return loop

    diffusion = types.SimpleNamespace(num_timesteps=3, p_sample_loop_progressive=fake_loop("p"),
                                      ddim_sample_loop_progressive=fake_loop("ddim"), plms_sample_loop_progressive=fake_loop("plms"))
    monkeypatch.setattr(script_util, "load_guided_diffusion", lambda **kw: (types.SimpleNamespace(ctx="ctx"), diffusion))

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
    assert used == [expect] and len(items) == 3


def test_cli_help_names_plms():
    from cgd import cgd as mine
    assert "plms50" in mine._CLI_SPEC
