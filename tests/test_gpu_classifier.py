"""The noisy ImageNet classifier and classifier guidance on the GPU, through the C ABI, against tests/classifier_ref.py (fp32, CPU, autograd).

Criterion: tests/parity_checks.py's records at the literal |a - b| <= 1e-4 + 1e-3 |ref|, strict (the net has no ReLU); every backward pass is
seeded so that the reference gradient has unit peak (`unit_seed`)."""
import ctypes as C
import functools

import pytest
import torch as th

from tests import classifier_ref as cr
from tests import parity_checks as pc
from tests.parity_checks import DEV, g, rec

pytestmark = pytest.mark.gpu


def _assert_ok(records):
    for r in records:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e} "
              f"[{r['criterion']}] strict={r['ok_strict']}")
    bad = [r for r in records if not r["ok"]]
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _ctx():
    return pc._ctx(1)


def _rows(a):
    """(B,C,S,S) -> dense NHWC rows [B*S*S][C]"""
    return a.permute(0, 2, 3, 1).reshape(-1, a.shape[1]).contiguous()


# ---- the head alone ---------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = {
    # the published head: 8 heads of 64 over 65 tokens, 1000 classes; two samples with different labels
    "published": dict(B=2, C=512, S=8, d=64, out=1000, y=(3, 997)),
    # odd key count (17) that fills no whole wavefront, 32-wide heads, a class count that is no multiple of anything
    "small": dict(B=3, C=128, S=4, d=32, out=7, y=(0, 6, 2)),
}


@functools.lru_cache(maxsize=None)
def _head_case(name, peak=None):
    """One CPU forward + backward of AttentionPool2d + log-softmax-select on seeded weights; `peak`: c_proj scaled so that the logits peak there."""
    k = HEAD_SHAPES[name]
    B, Cc, S, d, out = k["B"], k["C"], k["S"], k["d"], k["out"]
    gen = g(700 + Cc)
    pool = cr.AttentionPool2d(S, Cc, d, out)
    with th.no_grad():
        pool.positional_embedding.copy_(th.randn(Cc, S * S + 1, generator=gen) / Cc ** 0.5)
        pool.qkv_proj.weight.copy_(th.randn(3 * Cc, Cc, 1, generator=gen) * 2.0 / Cc ** 0.5)
        pool.qkv_proj.bias.copy_(th.randn(3 * Cc, generator=gen) * 0.1)
        pool.c_proj.weight.copy_(th.randn(out, Cc, 1, generator=gen) * 4.0 / Cc ** 0.5)
        pool.c_proj.bias.copy_(th.randn(out, generator=gen) * 0.1)
    for p in pool.parameters():
        p.requires_grad_(False)
    h = th.randn(B, Cc, S, S, generator=gen)
    if peak is not None:
        with th.no_grad():
            f = peak / pool(h).abs().max().item()
            pool.c_proj.weight.mul_(f)
            pool.c_proj.bias.mul_(f)
    y = th.tensor(k["y"])
    hr = h.clone().requires_grad_()
    logits = pool(hr)
    logp = cr.logp_of(logits, y)
    logp.sum().backward()
    with th.no_grad():
        pooled = pool.pooled(h)
    return dict(k, pool=pool, h=h, yt=y, pooled=pooled, logits=logits.detach(), logp=logp.detach(), dh=hr.grad)


def _run_head(case):
    ctx = _ctx()
    s = ctx.stream()
    B, Cc, S, d, out = case["B"], case["C"], case["S"], case["d"], case["out"]
    pool = case["pool"]
    n = ctx.lib.cgd_op_attnpool_scratch_floats(B, S, Cc, d, out)
    assert n > 0
    scratch = th.empty(n, device=DEV)
    w = [t.detach().reshape(-1).contiguous().to(DEV) for t in (pool.positional_embedding, pool.qkv_proj.weight, pool.qkv_proj.bias,
                                                               pool.c_proj.weight, pool.c_proj.bias)]
    hd, yd = _rows(case["h"]).to(DEV), case["yt"].to(DEV)
    pooled, logits, logp = th.empty(B, Cc, device=DEV), th.empty(B, out, device=DEV), th.empty(B, device=DEV)
    ctx.check(ctx.lib.cgd_op_attnpool_fwd(ctx.h, hd.data_ptr(), w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(),
                                          w[4].data_ptr(), yd.data_ptr(), pooled.data_ptr(), logits.data_ptr(), logp.data_ptr(),
                                          scratch.data_ptr(), B, S, Cc, d, out, s))
    seed = pc.unit_seed(case["dh"])
    dh = th.full((B * S * S, Cc), float("nan"), device=DEV)
    ctx.check(ctx.lib.cgd_op_attnpool_bwd(ctx.h, w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(), w[4].data_ptr(), seed, dh.data_ptr(),
                                          scratch.data_ptr(), B, S, Cc, d, out, s))
    th.cuda.synchronize()
    return pooled, logits, logp, dh, seed


@pytest.mark.parametrize("name", sorted(HEAD_SHAPES))
def test_head_against_the_reference(name):
    case = _head_case(name)
    pooled, logits, logp, dh, seed = _run_head(case)
    tag = f"attnpool[{name}]"
    _assert_ok([rec(f"{tag} pooled", pooled, case["pooled"]), rec(f"{tag} logits", logits, case["logits"]),
                rec(f"{tag} logp", logp, case["logp"]), rec(f"{tag} dh", dh, _rows(case["dh"]) * seed)])


@pytest.mark.parametrize("name", sorted(HEAD_SHAPES))
def test_head_with_logits_near_100_does_not_overflow(name):
    """exp(100) overflows fp32: a log-softmax without the maximum subtracted returns inf / nan here."""
    case = _head_case(name, peak=100.0)
    assert 99.0 < case["logits"].abs().max().item() < 101.0
    _, logits, logp, dh, seed = _run_head(case)
    assert bool(th.isfinite(logp).all()) and bool(th.isfinite(dh).all())
    tag = f"attnpool[{name}, logits near 100]"
    # logp is the record the large-logit case is about and stays strict.  The logits themselves peak at 100 here: the fp32 rounding of c_proj's
    # C-term sums grows with that peak (elements near zero carry the absolute error of the large ones), so they are graded in units of the peak
    _assert_ok([rec(f"{tag} logits", logits, case["logits"], unit_peak="c_proj scaled so that the logits peak near 100"),
                rec(f"{tag} logp", logp, case["logp"]), rec(f"{tag} dh", dh, _rows(case["dh"]) * seed)])


# ---- the whole net ----------------------------------------------------------------------------------------------------------------------
NET_INPUTS = {
    "clsA": dict(t=(417.0,), y=(7,)),
    "clsB": dict(t=(417.0, 12.5), y=(2, 5)),  # per-sample timesteps (one fractional), different labels
}


@functools.lru_cache(maxsize=None)
def _net_pair(name):
    """(CPU reference, device net) of a mini configuration on the same seeded weights; shared by the tests, never modified."""
    from cgd_amd import nets, synthetic
    kw = cr.MINI[name]
    sd = synthetic.classifier_state_dict(dict(kw), seed=8642)
    ref = cr.build(sd, **kw)
    dev = nets.NoisyClassifier(_ctx(), **kw)
    dev.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    return ref, dev


@functools.lru_cache(maxsize=None)
def _net_reference(name, B=None):
    """One CPU forward + backward: logits, logp and d(sum logp)/dx with its unit-peak factor."""
    ref, _ = _net_pair(name)
    kw, inp = cr.MINI[name], NET_INPUTS[name]
    B = B or len(inp["t"])
    S = kw["image_size"]
    x = th.randn(len(inp["t"]), 3, S, S, generator=g(710 + S))[:B].contiguous()
    t, y = th.tensor(inp["t"][:B]), th.tensor(inp["y"][:B])
    xr = x.clone().requires_grad_()
    logits = ref(xr, t)
    logp = cr.logp_of(logits, y)
    logp.sum().backward()
    return dict(x=x, t=t, y=y, logits=logits.detach(), logp=logp.detach(), dx=xr.grad, seed=pc.unit_seed(xr.grad))


@pytest.mark.parametrize("name", sorted(cr.MINI))
def test_net_against_the_reference(name):
    _, dev = _net_pair(name)
    r = _net_reference(name)
    logits, logp = dev.forward(r["x"].to(DEV), r["t"].to(DEV), r["y"].to(DEV))
    dx = dev.dgrad(r["seed"])
    th.cuda.synchronize()
    tag = f"classifier[{name}]"
    _assert_ok([rec(f"{tag} logits", logits, r["logits"]), rec(f"{tag} logp", logp, r["logp"]), rec(f"{tag} dx", dx, r["dx"] * r["seed"])])


def test_call_sequence_on_one_handle():
    """B = 2, B = 1, B = 2 again on one handle: every dgrad belongs to the last forward; accumulate adds; a handle that has seen each shape
    allocates nothing."""
    ctx = _ctx()
    _, dev = _net_pair("clsB")
    out, allocs = [], None
    for n, B in enumerate((2, 1, 2)):
        r = _net_reference("clsB", B)
        logits, logp = dev.forward(r["x"].to(DEV), r["t"].to(DEV), r["y"].to(DEV))
        dx = dev.dgrad(r["seed"])
        th.cuda.synchronize()
        out += [rec(f"sequence {n} B{B} logits", logits, r["logits"]), rec(f"sequence {n} B{B} logp", logp, r["logp"]),
                rec(f"sequence {n} B{B} dx", dx, r["dx"] * r["seed"])]
        if n == 1:
            allocs = ctx.lib.cgd_ctx_device_allocs(ctx.h)
    acc = th.zeros_like(dx)
    dev.dgrad(r["seed"], acc, accumulate=True)
    dev.dgrad(r["seed"], acc, accumulate=True)
    th.cuda.synchronize()
    out.append(rec("sequence accumulate twice", acc, 2 * r["dx"] * r["seed"]))
    assert ctx.lib.cgd_ctx_device_allocs(ctx.h) == allocs, "a handle that has seen each shape allocates nothing"
    _assert_ok(out)


def test_refusals_come_before_any_launch():
    from cgd_amd.lib import CgdError
    ctx = _ctx()
    _, dev = _net_pair("clsB")
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    with pytest.raises(CgdError, match="image_size"):
        dev.forward(th.zeros(1, 3, 32, 32, device=DEV), th.zeros(1, device=DEV), th.zeros(1, dtype=th.int64, device=DEV))
    with pytest.raises(CgdError, match="preceding forward"):
        dev.dgrad(1.0, th.zeros(1, 3, 32, 32, device=DEV))
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before


# ---- classifier guidance: one guided step ---------------------------------------------------------------------------------------------------
CLS, STEP_I, CUTN = 7, 12, 4


@functools.lru_cache(maxsize=None)
def _step_setup():
    """The mini UNet (32x32, 10 classes) with synthetic weights, a synthetic ViT-B/32 tower, the clsA classifier (32x32, 10 classes), one
    taped set of cutout boxes and the reference d logp / dx at the step's x and model timestep."""
    from cgd_amd import diffusion, nets, synthetic
    from oracle import guidance as og
    ctx = _ctx()
    _, dev_vit = pc.build_vit_pair(ctx, "ViT-B/32")
    unet = nets.UNet(ctx, **pc.UNET_CASES["mini"])
    unet.load_state_dict(synthetic.synthetic_state_dict(unet, seed=1234, device=DEV))
    sec = nets.SecondaryModel(ctx)
    sec.load_state_dict({k: v.to(DEV) for k, v in synthetic.secondary_state_dict(seed=9753).items()})
    ref_cls, dev_cls = _net_pair("clsA")
    tables = diffusion.create_gaussian_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="50")
    gen = g(720)
    B, H, W = 1, 32, 32
    x = th.randn(B, 3, H, W, generator=gen) * 0.8
    coords = og.generate_coords(H, W, CUTN, 224, 1.0, generator=gen)
    targets = [th.randn(1, 512, generator=g(721)).to(DEV)]
    ts = th.full((B,), float(tables.model_timestep(STEP_I)))
    xr = x.clone().requires_grad_()
    logp = cr.logp_of(ref_cls(xr, ts), th.full((B,), CLS))
    logp.sum().backward()
    return dict(ctx=ctx, vit=dev_vit, unet=unet, sec=sec, cls=dev_cls, tables=tables, x=x, coords=coords, targets=targets, ts=ts,
                logp=logp.detach(), dlogp=xr.grad)


def _guided(st, secondary=False, use_magnitude=False, **cls_kw):
    """One ClipGuidance.native call at step STEP_I on the taped boxes -> (g, log, cond)."""
    from cgd_amd import guidance
    from tests import step_checks
    ctx, tables, unet = st["ctx"], st["tables"], st["unet"]
    B, _, H, W = st["x"].shape
    cgs, tvs, rs = step_checks.default_scales(H, W)
    sampler = type("D", (), {"tables": tables, "num_timesteps": tables.num_timesteps, "step_coef": lambda self, a, b=None: tables.step_coef(a, b)})()
    kw = dict(clip_guidance_scale=cgs, tv_scale=tvs, range_scale=rs, use_magnitude=use_magnitude)
    if secondary:
        kw["secondary"] = st["sec"]
    cond = guidance.ClipGuidance(ctx, unet, [st["vit"]], sampler, st["targets"], th.tensor([1.0]), CUTN, **kw, **cls_kw)
    cond.current_timestep = STEP_I
    cond.coords_tape = [st["coords"]]
    coef = tables.step_coef(STEP_I, STEP_I)
    xd, ts = st["x"].to(DEV), st["ts"].to(DEV)
    out6 = unet.forward(xd, ts, th.full((B,), CLS, device=DEV))
    x0, mean, logvar, xin = (th.empty_like(xd) for _ in range(4))
    ctx.check(ctx.lib.cgd_pmv_blend(ctx.h, xd.data_ptr(), out6.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), xin.data_ptr(),
                                    B, H, W, coef, ctx.stream()))
    g_dev = cond.native(xd, x0, xin, coef, ts=ts) if cls_kw else cond.native(xd, x0, xin, coef)
    th.cuda.synchronize()
    return g_dev.clone(), cond.log(), cond


OLD_KEYS = ["CLIP Loss", "Range Loss", "TV Loss", "Total Loss", "Grad"]


@pytest.mark.parametrize("secondary", [False, True], ids=["unet", "secondary"])
def test_guidance_adds_scale_times_dlogp(secondary):
    st = _step_setup()
    g0, log0, _ = _guided(st, secondary)
    assert list(log0) == OLD_KEYS
    u = pc.unit_seed(st["dlogp"])
    print(f"peaks: g without classifier {g0.abs().max().item():.3e}, d logp/dx {st['dlogp'].abs().max().item():.3e}")
    out = []
    for scale in (1.0, 2.5):
        gc, logc, cond = _guided(st, secondary, classifier=st["cls"], classifier_scale=scale, classifier_class=CLS)
        tag = f"guidance[{'secondary' if secondary else 'unet'}, scale {scale}]"
        out.append(rec(f"{tag} g(classifier) - g(no classifier)", (gc - g0) * (u / scale), st["dlogp"] * u))
        out.append(rec(f"{tag} logp", cond.classifier_logp, st["logp"]))
        want = -scale * st["logp"].sum().item()
        out.append(rec(f"{tag} log Classifier Loss", th.tensor([logc["Classifier Loss"]]), th.tensor([want])))
        out.append(rec(f"{tag} log Total Loss", th.tensor([logc["Total Loss"]]), th.tensor([log0["Total Loss"] + want])))
        assert list(logc) == ["CLIP Loss", "Range Loss", "TV Loss", "Total Loss", "Classifier Loss", "Grad"]
    _assert_ok(out)


def test_magnitude_clamp_sees_the_summed_gradient():
    st = _step_setup()
    gp, _, _ = _guided(st, classifier=st["cls"], classifier_scale=2.5, classifier_class=CLS)
    gm, logm, cond = _guided(st, use_magnitude=True, classifier=st["cls"], classifier_scale=2.5, classifier_class=CLS)
    assert th.equal(gp, gm), "the clamp is a factor beside g (scalars[7]), not a change of g"
    rms = gm.double().pow(2).mean().sqrt().float().view(1)
    _assert_ok([rec("scalars[5] = rms of the summed gradient", cond.scalars[5:6], rms), rec("log Magnitude", th.tensor([logm["Magnitude"]]), rms)])


def test_without_a_classifier_nothing_changes():
    st = _step_setup()
    g_old, log_old, c_old = _guided(st)
    g_new, log_new, c_new = _guided(st, classifier=None, classifier_scale=3.0, classifier_class=None)
    assert th.equal(g_old, g_new) and log_old == log_new and list(log_new) == OLD_KEYS
    assert sorted(c_old._buf) == sorted(c_new._buf) and not any(k.startswith("cls_") for k in c_new._buf)


# ---- four steps of a loop -----------------------------------------------------------------------------------------------------------------
def _loop(st, name, spec, classifier):
    from cgd_amd import diffusion, guidance, sampler
    from tests import step_checks
    ctx = st["ctx"]
    smp = sampler.GuidedSampler(ctx, diffusion.create_gaussian_diffusion(1000, "linear", spec, False))
    assert smp.num_timesteps >= 4
    cgs, tvs, rs = step_checks.default_scales(32, 32)
    kw = dict(classifier=st["cls"], classifier_scale=2.0, classifier_class=CLS) if classifier else {}
    cond = guidance.ClipGuidance(ctx, st["unet"], [st["vit"]], smp, st["targets"], th.tensor([1.0]), CUTN, clip_guidance_scale=cgs, tv_scale=tvs,
                                 range_scale=rs, **kw)
    cond.current_timestep = smp.num_timesteps - 1
    th.manual_seed(730)
    seen_y, frames = [], []
    mkw = {"y": th.full((1,), CLS, device=DEV)}
    loop = getattr(smp, name)
    for o in loop(st["unet"], (1, 3, 32, 32), clip_denoised=False, cond_fn=cond, model_kwargs=mkw, device=DEV, randomize_class=False,
                  cond_fn_with_grad=True):
        seen_y.append(int(mkw["y"][0]))
        frames.append(o["sample"].clone())
        cond.current_timestep -= 1
        if len(frames) == 4:
            break
    th.cuda.synchronize()
    assert cond.calls == 4 and seen_y == [CLS] * 4
    if classifier:
        assert "Classifier Loss" in cond.log()
    return th.stack(frames).cpu()


@pytest.mark.parametrize("name,spec", [("p_sample_loop_progressive", "8"), ("dpmpp_sample_loop_progressive", "dpm8")])
def test_four_steps_of_a_loop_with_the_classifier(name, spec):
    st = _step_setup()
    a = _loop(st, name, spec, True)
    b = _loop(st, name, spec, True)
    plain = _loop(st, name, spec, False)
    assert bool(th.isfinite(a).all()) and th.equal(a, b), "finite and reproducible from the seed"
    assert not th.equal(a[-1], plain[-1]), "the classifier term moves the sample"
