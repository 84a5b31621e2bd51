"""GPU tests of PLMS sampling and DDIM with eta > 0: cgd_multistep_update against fp64 torch, and whole trajectories of the native
sampler against the restatement (tests/plms_ref.py) / the oracle's `ddim_sample_with_grad`, on the scenes of tests/step_checks.py with a
replayed tape (x_T, class ids, step noise, and cutout coordinates per cond_fn CALL: a PLMS start step calls cond_fn twice)."""
import functools
import itertools
import os

import pytest
import torch as th

from tests import parity_checks as pc
from tests import plms_ref
from tests import step_checks

pytestmark = pytest.mark.gpu

DEV = pc.DEV
AB = plms_ref.AB_WEIGHTS


def _assert_all(recs):
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


# ---- op level ----------------------------------------------------------------------------------------------------------------------
def _ref_update(phase, order, x, xe, x0, g, fct, noise, hist, k, ks, sigma, dirc):
    """fp64 restatement of cgd_multistep_update (include/cgd_mi355x.h) with the float32 coefficients the kernel sees"""
    d = lambda t: None if t is None else t.double().cpu()  # noqa: E731
    x, xe, x0, noise = d(x), d(xe), d(x0), d(noise)
    hist = [d(h) for h in hist]
    a, b, s1 = float(k.sqrt_recip), float(k.sqrt_recipm1), float(k.sqrt_one_minus_ab)
    gv = d(g) * fct if g is not None else 0.0
    e = (a * xe - x0) / b - s1 * gv
    x0c = a * xe - b * e
    eps = (a * xe - x0c) / b
    if phase == 3:
        s = x0c * float(k.sqrt_ab_prev) + dirc * eps
        return (s + sigma * noise if k.nonzero else s), x0, None
    if phase == 1:
        return x0c * float(k.sqrt_ab_prev) + float(k.sqrt_one_minus_ab_prev) * eps, x0, eps
    if phase == 2:
        ep, xs = (hist[0] + eps) / 2, x
    else:
        ep, xs = sum(w * t for w, t in zip(AB[order], [eps] + hist)), xe
    x0p = float(ks.sqrt_recip) * xs - float(ks.sqrt_recipm1) * ep
    mean = x0p * float(ks.sqrt_ab_prev) + float(ks.sqrt_one_minus_ab_prev) * ep
    return (mean if ks.nonzero else x0c), (x0 if phase == 0 else None), (eps if phase == 0 else None)


@pytest.fixture(scope="module")
def op_rig():
    import ctypes as C
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    ctx = L.Context(0, 1)
    tab = dd.create_gaussian_diffusion(1000, "linear", "plms50", False)
    return ctx, tab, L, C


def _launch(rig, phase, order, t, with_g, with_scal, sigma=0.0, dirc=0.0, B=2, H=24, W=40):
    ctx, tab, L, C = rig
    gen = th.Generator().manual_seed(100 * phase + 10 * order + t + with_g + 2 * with_scal)
    mk = lambda: th.randn(B, 3, H, W, generator=gen).to(DEV)  # noqa: E731
    x, x0, noise = mk(), mk(), mk()
    xe = mk() if phase == 2 else x
    g = mk() if with_g else None
    scal = th.tensor([0, 0, 0, 0, 0, 0, 0, 0.37]).float().to(DEV) if with_scal else None
    hist = [mk() for _ in range(3)]
    k = tab.step_coef(t - 1 if phase == 2 else t, 3)
    ks = tab.step_coef(t, 3)
    sample, x0_out, eps_out = (th.full_like(x, float("nan")) for _ in range(3))
    hp = (C.c_void_p * 3)(*[h.data_ptr() for h in hist])
    ctx.check(ctx.lib.cgd_multistep_update(ctx.h, x.data_ptr(), xe.data_ptr() if phase == 2 else None, x0.data_ptr(), L.ptr(g),
                                           L.ptr(scal), noise.data_ptr() if phase == 3 else None, hp, eps_out.data_ptr(),
                                           sample.data_ptr(), x0_out.data_ptr(), B, H, W, k, ks if phase == 2 else None,
                                           L.Multistep(phase, order, sigma, dirc), ctx.stream()))
    th.cuda.synchronize()
    ref = _ref_update(phase, order, x, xe, x0, g, 0.37 if with_scal else 1.0, noise if phase == 3 else None, hist, k,
                      ks if phase == 2 else k, sigma, dirc)
    tag = f"phase{phase} order{order} t{t} g{int(with_g)} clamp{int(with_scal)}"
    recs = [pc.rec(f"{tag} sample", sample, ref[0])]
    if ref[1] is not None:
        recs.append(pc.rec(f"{tag} pred_xstart", x0_out, ref[1]))
    if ref[2] is not None:
        recs.append(pc.rec(f"{tag} eps", eps_out, ref[2]))
    if phase == 2:  # the corrector writes neither eps nor pred_xstart
        assert th.isnan(eps_out).all() and th.isnan(x0_out).all()
    return recs


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_adams_bashforth_update_matches_fp64(op_rig, order):
    recs = []
    for t, with_g, with_scal in itertools.product((20, 0), (False, True), (False, True)):
        if with_scal and not with_g:
            continue
        recs += _launch(op_rig, 0, order, t, with_g, with_scal)
    _assert_all(recs)


def test_start_step_predictor_and_corrector_match_fp64(op_rig):
    recs = []
    for phase, (with_g, with_scal) in itertools.product((1, 2), ((False, False), (True, False), (True, True))):
        recs += _launch(op_rig, phase, 0, 20, with_g, with_scal)
    recs += _launch(op_rig, 2, 0, 1, True, True)  # corrector at t - 1 = 0
    _assert_all(recs)


def test_ddim_eta_update_matches_fp64(op_rig):
    import math
    tab = op_rig[1]
    recs = []
    for t, with_g, with_scal in ((20, True, True), (20, False, False), (0, True, False)):
        ab, abp = tab.alphas_cumprod[t], tab.alphas_cumprod_prev[t]
        sigma = 0.5 * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
        recs += _launch(op_rig, 3, 0, t, with_g, with_scal, sigma=sigma, dirc=math.sqrt(1 - abp - sigma ** 2))
    _assert_all(recs)


def test_bad_phase_order_and_start_step_at_t0_are_refused(op_rig):
    import ctypes as C
    from cgd_amd import lib as L
    ctx, tab = op_rig[0], op_rig[1]
    x = th.zeros(1, 3, 8, 8, device=DEV)
    hp = (C.c_void_p * 3)(x.data_ptr(), x.data_ptr(), x.data_ptr())
    for phase, order, k_step in ((4, 1, None), (-1, 1, None), (0, 0, None), (0, 5, None), (2, 0, tab.step_coef(0))):
        rc = ctx.lib.cgd_multistep_update(ctx.h, x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, None, hp, x.data_ptr(),
                                          x.data_ptr(), x.data_ptr(), 1, 8, 8, tab.step_coef(1), k_step, L.Multistep(phase, order, 0.0, 0.0),
                                          ctx.stream())
        assert rc == -2 and ctx.lib.cgd_last_error(ctx.h)
    # an order-3 update without its second history entry
    hp1 = (C.c_void_p * 3)(x.data_ptr(), None, None)
    assert ctx.lib.cgd_multistep_update(ctx.h, x.data_ptr(), None, x.data_ptr(), None, None, None, hp1, x.data_ptr(), x.data_ptr(),
                                        x.data_ptr(), 1, 8, 8, tab.step_coef(1), None, L.Multistep(0, 3, 0.0, 0.0), ctx.stream()) == -2


# ---- trajectories --------------------------------------------------------------------------------------------------------------------
def _scene(case="mini", steps=5, calls=None, **kw):
    """a step_checks scene with the spacing of 'ddimN' (= 'plmsN') and one tape entry of cutout coordinates per cond_fn call"""
    from oracle import guidance as og
    sc = step_checks.Scenario(case, ddim=True, steps=steps, **kw)
    if calls is not None:
        gen = th.Generator().manual_seed(4321)
        sc.tape["coords"] = [og.generate_coords(sc.H, sc.W, sc.cutn, sc.res, 1.0, generator=gen) for _ in range(calls)]
    return sc


def _mkw(sc, dev):
    return {"y": th.zeros(sc.B, dtype=th.long, device=dev)} if sc.kw.get("num_classes") else {}


def _oracle(sc, kind, order=2, eta=0.0, user_cond=None):
    og = sc.og
    diff = plms_ref.create_plms_diffusion(1000, sc.schedule, sc.spec, sc.rescale)
    cgs, tvs, rs = sc.scales
    if user_cond is None:
        cond, st = og.make_cond_fn(diffusion=diff, clip_model=sc.ref_clip, make_cutouts=og.MakeCutouts(sc.res, sc.cutn),
                                   target_embeds=sc.targets, weights=sc.w, num_cutouts=sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                                   range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude, coords_tape=sc.tape["coords"])
    else:
        cond, st = user_cond("cpu"), {}
    shape, mkw = (sc.B, 3, sc.H, sc.W), _mkw(sc, "cpu")
    init = sc.x0_star.expand(sc.B, -1, -1, -1)
    if kind == "plms":
        gen = diff.plms_sample_loop_progressive(sc.ref_unet, shape, clip_denoised=False, cond_fn=cond, model_kwargs=dict(mkw), device="cpu",
                                                skip_timesteps=sc.skip, init_image=init, randomize_class=bool(mkw), cond_fn_with_grad=True,
                                                order=order, tape=sc.tape)
    else:
        gen = diff._loop(functools.partial(diff.ddim_sample_with_grad, eta=eta), sc.ref_unet, shape, None, False, cond, dict(mkw), "cpu",
                         sc.skip, init, bool(mkw), sc.tape)
    st["current_timestep"] = sc.counter0
    out = []
    for o in itertools.islice(gen, sc.steps):
        st["current_timestep"] -= 1
        out.append((o["sample"].clone(), o["pred_xstart"].clone(), dict(st.get("log", {}))))
    return out


def _device(sc, kind, order=2, eta=0.0, user_cond=None, precision=1):
    from cgd_amd import diffusion as dd
    from cgd_amd import guidance as dg
    from cgd_amd import lib, nets, sampler
    ctx = lib.Context(0, precision)
    unet = nets.UNet(ctx, **sc.kw)
    unet.load_state_dict({k: v.to(DEV) for k, v in sc.ref_unet.state_dict().items()})
    clip = nets.ClipImageTower(ctx, sc.vit_name) if sc.vit_name else nets.ClipImageTower(ctx, config=sc.vit_cfg)
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
    shape, mkw = (sc.B, 3, sc.H, sc.W), _mkw(sc, DEV)
    kw = dict(clip_denoised=False, cond_fn=cond, model_kwargs=mkw, device=DEV, skip_timesteps=sc.skip,
              init_image=sc.x0_star.expand(sc.B, -1, -1, -1).to(DEV), randomize_class=bool(mkw), cond_fn_with_grad=True)
    gen = smp.plms_sample_loop_progressive(unet, shape, order=order, **kw) if kind == "plms" else \
        smp.ddim_sample_loop_progressive(unet, shape, eta=eta, **kw)
    out = []
    for o in itertools.islice(gen, sc.steps):
        th.cuda.synchronize()
        out.append((o["sample"].cpu(), o["pred_xstart"].cpu(), cond.log() if user_cond is None else {}))
        if user_cond is None:
            cond.current_timestep -= 1
    if user_cond is None:
        assert cond.calls == len(sc.tape["coords"]), "one tape entry of coordinates per cond_fn call"
    return out


def _compare(sc, tag, d_out, o_out):
    recs = []
    assert len(d_out) == len(o_out) == sc.steps
    for k, ((ds, dx, dl), (os_, ox, ol)) in enumerate(zip(d_out, o_out)):
        recs.append(pc.rec(f"{tag} step{k} sample", ds, os_))
        recs.append(pc.rec(f"{tag} step{k} pred_xstart", dx, ox))
        for key in ("CLIP Loss", "TV Loss", "Range Loss", "Total Loss"):
            if key in ol:
                recs.append(pc.rec(f"{tag} step{k} {key}", th.tensor([dl[key]]), th.tensor([ol[key]]), allow_small=True))
    return recs


@pytest.mark.parametrize("order", [2, 4])
def test_plms_trajectory_native_guidance_mini(order):
    sc = _scene("mini", steps=5, calls=6)
    _assert_all(_compare(sc, f"plms order {order} mini", _device(sc, "plms", order), _oracle(sc, "plms", order)))


def test_plms_order1_trajectory_mini():
    sc = _scene("mini", steps=4, calls=4)
    _assert_all(_compare(sc, "plms order 1 mini", _device(sc, "plms", 1), _oracle(sc, "plms", 1)))


def test_plms_trajectory_headline_shape():
    sc = _scene("cfg256", steps=3, calls=4, vit_name="ViT-B/32", cutn=16, respacing="250", scales=(1000.0, 150.0, 50.0), head_scale=1.0)
    _assert_all(_compare(sc, "plms order 2 headline", _device(sc, "plms", 2), _oracle(sc, "plms", 2)))


def test_plms_trajectory_generic_cond_fn_through_autograd():
    """a user cond_fn (not ClipGuidance) runs through autograd over the UNet node on the device, under PLMS"""
    sc = _scene("mini", steps=4)
    target = sc.x0_star

    def user_cond(dev):
        tgt = target.to(dev)

        def cond_fn(x, t, out, y=None):
            loss = 0.1 * ((out["pred_xstart"] - tgt) ** 2).sum()
            return -th.autograd.grad(loss, x)[0]
        return cond_fn

    _assert_all(_compare(sc, "plms order 3 generic", _device(sc, "plms", 3, user_cond=user_cond),
                         _oracle(sc, "plms", 3, user_cond=user_cond)))


def test_ddim_eta_trajectory_against_the_oracle():
    sc = _scene("mini", steps=4)
    _assert_all(_compare(sc, "ddim eta 0.5 mini", _device(sc, "ddim", eta=0.5), _oracle(sc, "ddim", eta=0.5)))


def test_dropin_generator_plms_synthetic_weights(tmp_path, monkeypatch):
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion
    from cgd_amd import sampler
    seen = []
    plain = sampler.GuidedSampler.plms_sample_loop_progressive

    def recording(self, *a, **kw):
        seen.append((kw.get("order"), []))
        for out in plain(self, *a, **kw):
            seen[-1][1].append(out["sample"].detach().clone())
            yield out

    monkeypatch.setattr(sampler.GuidedSampler, "plms_sample_loop_progressive", recording)
    runs = []
    for r in range(2):
        items = list(clip_guided_diffusion(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=2, timestep_respacing="plms8",
                                           seed=7, prefix_path=str(tmp_path / f"out{r}"), checkpoints_dir=str(tmp_path / "ckpt"),
                                           save_frequency=1, progress=False, device="cuda"))
        assert len(items) == 8 and all(os.path.isfile(p) for _, p in items)
        runs.append(items)
    assert [o for o, _ in seen] == [2, 2] and [len(s) for _, s in seen] == [8, 8]
    for a, b in zip(seen[0][1], seen[1][1]):
        assert th.isfinite(a).all() and th.equal(a, b)
