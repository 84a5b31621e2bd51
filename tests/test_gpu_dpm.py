"""GPU tests of DPM-Solver++(2M) sampling: cgd_dpmpp_update against fp64 torch and against the neighbouring update kernels, and whole
trajectories of the native sampler against the restatement (tests/dpm_ref.py) on the mini scene of tests/step_checks.py, spaced 'dpm8',
with a replayed tape (x_T, class ids, step noise, noise of the kept region, and cutout coordinates per cond_fn call)."""
import itertools
import math
import os

import pytest
import torch as th

from tests import dpm_ref
from tests import parity_checks as pc
from tests import step_checks

pytestmark = pytest.mark.gpu

DEV = pc.DEV
SHAPES = {"aligned": (2, 3, 24, 40), "odd": (1, 3, 5, 7)}  # 'odd': 4 does not divide H * W, and every pointer sits 4 bytes off 16


def _assert_all(recs):
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


# ---- op level --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def op_rig():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    return L.Context(0, 1), dd.create_gaussian_diffusion(1000, "linear", "dpm50", False), L


def _tensor(shape, gen=None, fill=None):
    """a contiguous tensor of `shape`; for the 'odd' shape it starts one float into its allocation (a 4-byte-offset pointer)"""
    n = math.prod(shape)
    off = 1 if shape == SHAPES["odd"] else 0
    flat = th.empty(n + off + 3, device=DEV)
    view = flat[off:off + n].view(shape)
    view.copy_(th.randn(shape, generator=gen)) if fill is None else view.fill_(fill)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


def _inputs(shape, seed, with_g, with_scal):
    gen = th.Generator().manual_seed(seed)
    x, x0, noise, hist = (_tensor(shape, gen) for _ in range(4))
    g = _tensor(shape, gen) if with_g else None
    scal = th.tensor([0, 0, 0, 0, 0, 0, 0, 0.37]).float().to(DEV) if with_scal else None
    return x, x0, g, scal, noise, hist


def _ref_update(x, x0, g, fct, noise, hist, k, d):
    """fp64 restatement of cgd_dpmpp_update (include/cgd_mi355x.h) with the float32 coefficients the kernel sees"""
    dbl = lambda t: None if t is None else t.double().cpu()  # noqa: E731
    x, x0, g, noise, hist = dbl(x), dbl(x0), dbl(g), dbl(noise), dbl(hist)
    a, b, s1 = float(k.sqrt_recip), float(k.sqrt_recipm1), float(k.sqrt_one_minus_ab)
    e = (a * x - x0) / b - s1 * (g * fct if g is not None else 0.0)
    x0c = a * x - b * e
    dd_ = x0c + float(d.c_r) * (x0c - hist) if d.c_r != 0 else x0c
    if not k.nonzero:
        return x0c, x0c, x0
    s = float(d.c_x) * x + float(d.c_d) * dd_
    if d.c_n != 0:
        s = s + float(d.c_n) * noise
    return s, x0c, x0


def _launch(rig, shape, t, order, eta, with_g, with_scal, outputs=(True, True)):
    ctx, tab, L = rig
    x, x0, g, scal, noise, hist = _inputs(shape, 1000 * t + 100 * order + int(10 * eta) + with_g + 2 * with_scal, with_g, with_scal)
    k, d = tab.step_coef(t, 3), tab.dpmpp_coef(t, order, eta)
    sample = _tensor(shape, fill=float("nan"))
    x0c_out = _tensor(shape, fill=float("nan")) if outputs[0] else None
    x0_out = _tensor(shape, fill=float("nan")) if outputs[1] else None
    # unused inputs are not passed at all: a launch that read them would fault on NULL, not pass by luck
    ctx.check(ctx.lib.cgd_dpmpp_update(ctx.h, x.data_ptr(), x0.data_ptr(), L.ptr(g), L.ptr(scal), noise.data_ptr() if d.c_n and t else None,
                                       hist.data_ptr() if d.c_r else None, L.ptr(x0c_out), sample.data_ptr(), L.ptr(x0_out),
                                       shape[0], shape[2], shape[3], k, d, ctx.stream()))
    th.cuda.synchronize()
    ref = _ref_update(x, x0, g, 0.37 if with_scal else 1.0, noise, hist, k, d)
    return (sample, x0c_out, x0_out), ref, (x, x0, g, scal, noise, hist, k, d)


@pytest.mark.parametrize("name", list(SHAPES))
def test_update_matches_fp64(op_rig, name):
    recs = []
    for t, order, eta, (with_g, with_scal) in itertools.product((20, 0), (1, 2), (0.0, 1.0), ((False, False), (True, False), (True, True))):
        outs, ref, (*_, d) = _launch(op_rig, SHAPES[name], t, order, eta, with_g, with_scal)
        assert (d.c_r != 0) == (order == 2 and t != 0) and (d.c_n != 0) == (eta != 0 and t != 0)
        tag = f"dpmpp {name} t{t} order{order} eta{eta:g} g{int(with_g)} clamp{int(with_scal)}"
        for what, got, want in zip(("sample", "x0c", "pred_xstart"), outs, ref):
            assert th.isfinite(got).all(), f"{tag} {what}: an element was not written"
            recs.append(pc.rec(f"{tag} {what}", got, want))
        assert th.equal(outs[2].cpu(), ref[2].float())  # a copy, bit for bit
    _assert_all(recs)


@pytest.mark.parametrize("name", list(SHAPES))
def test_outputs_that_are_not_asked_for_are_not_written(op_rig, name):
    """one NaN arena holds the three outputs with guard floats between them: every element of a passed output is written, the arena around
    them and the slot of an omitted output stay NaN"""
    ctx, tab, L = op_rig
    shape = SHAPES[name]
    n = math.prod(shape)
    step = n + 8  # 32 guard bytes: keeps the 16-byte alignment class of the first slot
    off = 1 if name == "odd" else 0
    x, x0, g, scal, noise, hist = _inputs(shape, 7, True, False)
    k, d = tab.step_coef(20, 3), tab.dpmpp_coef(20, 2, 1.0)
    for passed in ((True, True), (True, False), (False, True), (False, False)):
        arena = th.full((3 * step + 8,), float("nan"), device=DEV)
        slots = [arena[4 + off + j * step:4 + off + j * step + n].view(shape) for j in range(3)]
        sample, x0c_out, x0_out = slots[0], slots[1] if passed[0] else None, slots[2] if passed[1] else None
        ctx.check(ctx.lib.cgd_dpmpp_update(ctx.h, x.data_ptr(), x0.data_ptr(), g.data_ptr(), None, noise.data_ptr(), hist.data_ptr(),
                                           L.ptr(x0c_out), sample.data_ptr(), L.ptr(x0_out), shape[0], shape[2], shape[3], k, d, ctx.stream()))
        th.cuda.synchronize()
        written = th.isfinite(arena)
        expect = th.zeros_like(written)
        for j, on in enumerate((True,) + passed):
            if on:
                expect[4 + off + j * step:4 + off + j * step + n] = True
        assert th.equal(written, expect), passed


@pytest.mark.parametrize("name", list(SHAPES))
def test_clean_end_sample_is_the_multistep_updates_bit_for_bit(op_rig, name):
    import ctypes as C
    ctx, tab, L = op_rig
    shape = SHAPES[name]
    for with_g, with_scal in ((False, False), (True, False), (True, True)):
        (sample, _, _), _, (x, x0, g, scal, noise, hist, k, d) = _launch(op_rig, shape, 0, 2, 1.0, with_g, with_scal)
        other, x0_o, eps_o = (_tensor(shape, fill=float("nan")) for _ in range(3))
        ctx.check(ctx.lib.cgd_multistep_update(ctx.h, x.data_ptr(), None, x0.data_ptr(), L.ptr(g), L.ptr(scal), None,
                                               (C.c_void_p * 3)(None, None, None), eps_o.data_ptr(), other.data_ptr(), x0_o.data_ptr(),
                                               shape[0], shape[2], shape[3], k, None, L.Multistep(0, 1, 0.0, 0.0), ctx.stream()))
        th.cuda.synchronize()
        assert th.isfinite(sample).all() and th.equal(sample, other), (name, with_g, with_scal)


def test_order1_matches_the_ddim_updates(op_rig):
    """eta = 0 against cgd_sample_update mode 1, eta = 1 against cgd_multistep_update phase 3 with eta = 1, on the same inputs"""
    ctx, tab, L = op_rig
    shape = SHAPES["aligned"]
    recs = []
    for t, (with_g, with_scal) in itertools.product((20, 3, 0), ((False, False), (True, True))):
        for eta in (0.0, 1.0):
            (sample, _, x0_out), _, (x, x0, g, scal, noise, hist, k, d) = _launch(op_rig, shape, t, 1, eta, with_g, with_scal)
            other, x0_o = th.full_like(x, float("nan")), th.full_like(x, float("nan"))
            if eta == 0.0:
                junk = th.zeros_like(x)  # mean / log-variance / noise: mode 1 does not read them
                ctx.check(ctx.lib.cgd_sample_update(ctx.h, x.data_ptr(), x0.data_ptr(), junk.data_ptr(), junk.data_ptr(), L.ptr(g),
                                                    junk.data_ptr(), L.ptr(scal), other.data_ptr(), x0_o.data_ptr(), shape[0], shape[2],
                                                    shape[3], k, 1, ctx.stream()))
            else:
                ab, abp = tab.alphas_cumprod[t], tab.alphas_cumprod_prev[t]
                sigma = math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
                m = L.Multistep(3, 0, sigma, math.sqrt(max(0.0, 1 - abp - sigma * sigma)))
                ctx.check(ctx.lib.cgd_multistep_update(ctx.h, x.data_ptr(), None, x0.data_ptr(), L.ptr(g), L.ptr(scal), noise.data_ptr(),
                                                       None, None, other.data_ptr(), x0_o.data_ptr(), shape[0], shape[2], shape[3], k, None,
                                                       m, ctx.stream()))
            th.cuda.synchronize()
            tag = f"dpmpp order 1 eta{eta:g} t{t} g{int(with_g)} vs ddim"
            recs.append(pc.rec(f"{tag} sample", sample, other))
            assert th.equal(x0_out, x0_o)
    _assert_all(recs)


def test_bad_arguments_are_refused(op_rig):
    ctx, tab, L = op_rig
    bufs = [th.zeros(1, 3, 8, 8, device=DEV) for _ in range(8)]
    x, x0, g, noise, hist, x0c, sample, x0o = (b.data_ptr() for b in bufs)
    k1, k0 = tab.step_coef(5), tab.step_coef(0)
    ode, sde = tab.dpmpp_coef(5, 2, 0.0), tab.dpmpp_coef(5, 1, 1.0)

    def call(x=x, x0=x0, noise=noise, hist=hist, x0c=x0c, sample=sample, x0o=x0o, B=1, H=8, W=8, k=k1, d=ode):
        return ctx.lib.cgd_dpmpp_update(ctx.h, x, x0, g, None, noise, hist, x0c, sample, x0o, B, H, W, k, d, ctx.stream())

    assert call() == 0 and call(d=sde) == 0 and call(x0c=None, x0o=None) == 0
    assert call(d=sde, noise=None, k=k0) == 0  # at t == 0 nothing reads the noise
    bad = [dict(x=None), dict(x0=None), dict(sample=None),  # a missing required buffer
           dict(hist=None), dict(d=sde, noise=None),  # c_r != 0 without the history, c_n != 0 at t != 0 without the noise
           dict(B=0), dict(H=0), dict(W=-1),  # non-positive sizes
           dict(sample=x), dict(x0c=x), dict(x0o=x), dict(x0c=sample), dict(x0o=sample), dict(x0o=x0c)]  # aliasing outputs
    for kw in bad:
        assert call(**kw) == -2 and ctx.lib.cgd_last_error(ctx.h), kw
    th.cuda.synchronize()


# ---- trajectories ------------------------------------------------------------------------------------------------------------------------
SPEC, STEPS = "dpm8", 5


@pytest.fixture(scope="module")
def scene():
    """the mini scene of tests/step_checks.py re-spaced to 'dpm8': the last five levels (indices 4 .. 0: a first step without history,
    three second-order steps, the first-order step to the clean image), one tape entry of cutout coordinates per cond_fn call"""
    from cgd_amd import diffusion as dd
    from oracle import guidance as og
    sc = step_checks.Scenario("mini", ddim=True, steps=STEPS)
    N = dd.create_gaussian_diffusion(1000, sc.schedule, SPEC).num_timesteps
    assert N == 8
    sc.spec, sc.N, sc.t_first = SPEC, N, STEPS - 1
    sc.skip, sc.counter0 = N - STEPS, STEPS - 1
    gen = th.Generator().manual_seed(4321)
    sc.tape["coords"] = [og.generate_coords(sc.H, sc.W, sc.cutn, sc.res, 1.0, generator=gen) for _ in range(STEPS)]
    sc.tape["known_noise"] = [th.randn(sc.B, 3, sc.H, sc.W, generator=gen) for _ in range(STEPS)]
    sc.mask = th.zeros(1, 1, sc.H, sc.W)
    sc.mask[..., : sc.W // 2] = 1.0  # the left half is regenerated, the right half kept
    return sc


def _mkw(sc, dev):
    return {"y": th.zeros(sc.B, dtype=th.long, device=dev)} if sc.kw.get("num_classes") else {}


def _oracle(sc, order, eta, user_cond=None, mask=None):
    og = sc.og
    diff = dpm_ref.create_dpm_diffusion(1000, sc.schedule, sc.spec, sc.rescale)
    cgs, tvs, rs = sc.scales
    if user_cond is None:
        cond, st = og.make_cond_fn(diffusion=diff, clip_model=sc.ref_clip, make_cutouts=og.MakeCutouts(sc.res, sc.cutn),
                                   target_embeds=sc.targets, weights=sc.w, num_cutouts=sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                                   range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude, coords_tape=sc.tape["coords"])
    else:
        cond, st = user_cond("cpu"), {}
    mkw = _mkw(sc, "cpu")
    gen = diff.dpmpp_sample_loop_progressive(sc.ref_unet, (sc.B, 3, sc.H, sc.W), clip_denoised=False, cond_fn=cond, model_kwargs=dict(mkw),
                                             skip_timesteps=sc.skip, init_image=sc.x0_star.expand(sc.B, -1, -1, -1),
                                             randomize_class=bool(mkw), order=order, eta=eta, tape=sc.tape, mask=mask)
    st["current_timestep"] = sc.counter0
    out = []
    for o in gen:
        st["current_timestep"] -= 1
        out.append((o["sample"].clone(), o["pred_xstart"].clone(), dict(st.get("log", {}))))
    return out


def _device(sc, order, eta, user_cond=None, mask=None):
    from cgd_amd import diffusion as dd
    from cgd_amd import guidance as dg
    from cgd_amd import lib, nets, sampler
    ctx = lib.Context(0, 1)
    unet = nets.UNet(ctx, **sc.kw)
    unet.load_state_dict({k: v.to(DEV) for k, v in sc.ref_unet.state_dict().items()})
    clip = nets.ClipImageTower(ctx, config=sc.vit_cfg)
    clip.load_clip_state_dict({k: v.to(DEV) for k, v in sc.ref_clip.state_dict().items()})
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, sc.schedule, sc.spec, sc.rescale))
    smp.tape = sc.tape
    cgs, tvs, rs = sc.scales
    if user_cond is None:
        cond = dg.ClipGuidance(ctx, unet, clip, smp, sc.targets.to(DEV), sc.w, sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                               range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude)
        cond.coords_tape = sc.tape["coords"]
        cond.current_timestep = sc.counter0
    else:
        cond = user_cond(DEV)
    mkw = _mkw(sc, DEV)
    gen = smp.dpmpp_sample_loop_progressive(unet, (sc.B, 3, sc.H, sc.W), clip_denoised=False, cond_fn=cond, model_kwargs=mkw, device=DEV,
                                            skip_timesteps=sc.skip, init_image=sc.x0_star.expand(sc.B, -1, -1, -1).to(DEV),
                                            randomize_class=bool(mkw), cond_fn_with_grad=True, order=order, eta=eta,
                                            **({} if mask is None else {"mask": mask.to(DEV)}))
    out = []
    for o in gen:
        th.cuda.synchronize()
        out.append((o["sample"].cpu(), o["pred_xstart"].cpu(), cond.log() if user_cond is None else {}))
        if user_cond is None:
            cond.current_timestep -= 1
    if user_cond is None:
        assert cond.calls == STEPS, "one cond_fn call per step"
    return out


def _compare(tag, d_out, o_out):
    recs = []
    assert len(d_out) == len(o_out) == STEPS
    for k, ((ds, dx, dl), (os_, ox, ol)) in enumerate(zip(d_out, o_out)):
        recs.append(pc.rec(f"{tag} step{k} sample", ds, os_))
        recs.append(pc.rec(f"{tag} step{k} pred_xstart", dx, ox))
        for key in ("CLIP Loss", "TV Loss", "Range Loss", "Total Loss"):
            if key in ol:
                recs.append(pc.rec(f"{tag} step{k} {key}", th.tensor([dl[key]]), th.tensor([ol[key]]), allow_small=True))
    return recs


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_trajectory_order2_native_guidance(scene, eta):
    _assert_all(_compare(f"dpmpp 2M eta {eta:g} mini", _device(scene, 2, eta), _oracle(scene, 2, eta)))


def test_trajectory_order2_under_a_half_image_mask(scene):
    d_out = _device(scene, 2, 0.0, mask=scene.mask)
    _assert_all(_compare("dpmpp 2M masked mini", d_out, _oracle(scene, 2, 0.0, mask=scene.mask)))
    # the kept half of the last sample and of its pred_xstart is the init image, bit for bit
    keep = scene.W // 2
    init = scene.x0_star.expand(scene.B, -1, -1, -1)
    assert th.equal(d_out[-1][0][..., keep:], init[..., keep:]) and th.equal(d_out[-1][1][..., keep:], init[..., keep:])
    assert not th.equal(d_out[-1][0][..., :keep], init[..., :keep])


def test_trajectory_generic_cond_fn_through_autograd(scene):
    """a user cond_fn (not ClipGuidance) runs through autograd over the UNet node on the device, under DPM-Solver++"""
    target = scene.x0_star

    def user_cond(dev):
        tgt = target.to(dev)

        def cond_fn(x, t, out, y=None):
            loss = 0.1 * ((out["pred_xstart"] - tgt) ** 2).sum()
            return -th.autograd.grad(loss, x)[0]
        return cond_fn

    _assert_all(_compare("dpmpp 2M generic", _device(scene, 2, 0.0, user_cond=user_cond), _oracle(scene, 2, 0.0, user_cond=user_cond)))


def test_dropin_generator_dpm_synthetic_weights(tmp_path, monkeypatch):
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion
    from cgd_amd import diffusion as dd
    from cgd_amd import sampler
    levels = dd.create_gaussian_diffusion(1000, "linear", "dpm8").num_timesteps
    seen = []
    plain = sampler.GuidedSampler.dpmpp_sample_loop_progressive

    def recording(self, *a, **kw):
        seen.append((kw.get("order"), kw.get("eta"), self.num_timesteps, []))
        for out in plain(self, *a, **kw):
            seen[-1][3].append(out["sample"].detach().clone())
            yield out

    monkeypatch.setattr(sampler.GuidedSampler, "dpmpp_sample_loop_progressive", recording)
    items = list(clip_guided_diffusion(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=2, timestep_respacing="dpm8",
                                       seed=7, prefix_path=str(tmp_path / "out"), checkpoints_dir=str(tmp_path / "ckpt"),
                                       save_frequency=1, progress=False, device="cuda"))
    assert len(items) == levels and all(os.path.isfile(p) for _, p in items)
    assert [s[:3] for s in seen] == [(2, 0.0, levels)] and len(seen[0][3]) == levels
    assert all(th.isfinite(s).all() for s in seen[0][3])
