"""CPU tests of tests/tail_ref.py (the float64 references and input recipes of tests/test_gpu_tail.py) and of the reference helpers the
cutout cases of tests/parity_checks.py add: each against the oracle's own functions, so that no helper runs for the first time on a GPU."""
import itertools

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from oracle import diffusion as od
from oracle import guidance as og
from tests import parity_checks as pc
from tests import tail_ref as tr



@pytest.fixture(scope="module")
def tab():
    return dd.create_gaussian_diffusion(*tr.SCHEDULE)


@pytest.fixture(scope="module")
def oracle():
    return od.create_gaussian_diffusion(*tr.SCHEDULE)


def _close(a, b, tol=1e-9):
    a, b = th.as_tensor(a).double(), th.as_tensor(b).double()
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def test_schedule_has_the_stated_ends(tab):
    assert tab.num_timesteps == 250
    last, first = tab.step_coef(tr.STEPS["last"], tr.STEPS["last"]), tab.step_coef(0, 0)
    assert 150 < last.sqrt_recip < 165 and 1 - last.fac < 1e-4 and last.nonzero == 1
    assert first.nonzero == 0 and abs(first.fac - 0.01) < 1e-3
    assert [tr.blocks(*s) for s in tr.SHAPES] == [1, 1, 1, 23, 1024, 1024]
    assert tr.blocks(1, 40, 48) == 23 and 1 * 3 * 296 * 300 > 262144 and (3 * 296 * 300) % 256


@pytest.mark.parametrize("step", sorted(tr.STEPS))
def test_pmv_blend_matches_the_oracle_p_mean_variance(tab, oracle, step):
    i = tr.STEPS[step]
    k = tab.step_coef(i, i)
    x, out6 = tr.pmv_inputs((2, 24, 40), i, k)
    x0, mean, lv, x_in = tr.pmv_blend(x, out6, k)
    o = oracle.p_mean_variance(lambda xx, t: out6.double(), x.double(), th.full((2,), i, dtype=th.long), clip_denoised=False)
    # the oracle extracts float32 coefficients as the kernel does, but multiplies in the tensor's dtype (float64 here)
    _close(x0, o["pred_xstart"], 1e-6)
    _close(mean, o["mean"], 1e-6)
    _close(lv, o["log_variance"], 1e-6)
    fac = float(tab.sqrt_one_minus_alphas_cumprod[i])
    _close(x_in, o["pred_xstart"] * fac + x.double() * (1 - fac), 1e-6)
    assert x0.abs().max() < 8, "the recipe keeps pred_xstart O(1) although a x and b eps are up to 157 times larger"
    assert lv.max() > max(k.min_log, k.max_log) and lv.min() < min(k.min_log, k.max_log), "frac extrapolates on both sides"
    for t in (x0, mean, lv, x_in):
        assert t.abs().max().item() >= pc.MIN_PEAK


@pytest.mark.parametrize("step,setting", list(itertools.product(sorted(tr.STEPS), sorted(tr.SETTINGS))))
def test_combine_reference_is_the_gradient_of_the_oracle_losses_through_a_toy_model(tab, step, setting):
    """dL/dx of the full composition x -> eps(x) = M x (a toy linear model) -> x0 = a x - b eps -> x_in -> losses equals
    g_direct + M^T seed_eps of the reference, and the loss values are the oracle's."""
    i = tr.STEPS[step]
    k = tab.step_coef(i, i)
    c = tr.coef(k)
    tv, rng, sat, with_clip = tr.SETTINGS[setting]
    scales = (tv * tr.SCALES[0], rng * tr.SCALES[1], sat * tr.SCALES[2])
    x_in, x0, g_clip = tr.combine_inputs((2, 6, 5), i)
    g_clip = g_clip if with_clip else None
    g_direct, seed_eps, losses = tr.guidance_combine(g_clip, x_in, x0, k, *scales)
    x, eps = tr.combine_leaves(x_in, x0, k)
    # eps(x) = m * (x rolled along W) + c0 with c0 chosen so that eps(x) is the recovered eps at this x
    m = 0.3
    c0 = eps - m * x.roll(1, dims=3)
    xr = x.clone().requires_grad_()
    eps_x = m * xr.roll(1, dims=3) + c0
    x0_x = c["sqrt_recip"] * xr - c["sqrt_recipm1"] * eps_x
    x_in_x = x0_x * c["fac"] + xr * (1 - c["fac"])
    loss = og.tv_loss(x_in_x).sum() * scales[0] + og.range_loss(x0_x).sum() * scales[1]
    loss = loss + th.abs(x_in_x - x_in_x.clamp(min=-1, max=1)).mean().sum() * scales[2]
    if with_clip:
        loss = loss + (g_clip.double() * x_in_x).sum()
    want = th.autograd.grad(loss, xr)[0]
    got = g_direct + m * seed_eps.roll(-1, dims=3)
    _close(got, want, 1e-7)
    _close(losses, th.stack([og.tv_loss(x_in.double()).sum() * scales[0], og.range_loss(x0.double()).sum() * scales[1],
                             (x_in.double() - x_in.double().clamp(-1, 1)).abs().mean() * scales[2]]), 1e-6)


def test_combine_edge_closed_form_agrees_with_autograd_away_from_the_kinks(tab):
    k = tab.step_coef(125, 125)
    x_in, x0, _ = tr.combine_inputs((2, 4, 3), 125)
    gd, se, losses = tr.guidance_combine(None, x_in, x0, k, 0.0, 50.0, 30.0)
    gd2, se2, l2 = tr.combine_edge_closed_form(x_in, x0, k, 50.0, 30.0)
    _close(gd2, gd)
    _close(se2, se)
    _close(l2, losses[1:])
    # at the kinks: zero contribution at exactly +-1, the sign and 2^-23 just beyond
    xe, x0e = tr.combine_edge_inputs()
    assert xe.shape == x0e.shape == (1, 3, 5, 5) and len({(a, b) for a, b in zip(xe.flatten().tolist(), x0e.flatten().tolist())}) == 25
    gd, se, _ = tr.combine_edge_closed_form(xe, x0e, k, 50.0, 0.0)
    inside = x0e.abs() <= 1
    assert (se[inside] == 0).all() and (gd[inside] == 0).all() and (se[~inside] != 0).all()
    assert th.equal(th.sign(se[~inside]), -th.sign(x0e[~inside]).double())
    _close(se[~inside].abs(), th.full_like(se[~inside], tr.coef(k)["sqrt_recipm1"] * 50.0 * 2 * 2.0 ** -23 / 75), 1e-12)
    gd, se, _ = tr.combine_edge_closed_form(xe, x0e, k, 0.0, 30.0)
    inside = xe.abs() <= 1
    assert (gd[inside] == 0).all() and th.equal(th.sign(gd[~inside]), th.sign(xe[~inside]).double())


def test_grad_finish_and_scalars_references():
    gd, gu = tr.finish_inputs((2, 24, 40))
    g, s1, s2, sa = tr.grad_finish(gd, gu)
    _close(g, -(gd.double() + gu.double()))
    assert tr.grad_finish(gd, None)[0].equal(-gd.double())
    assert g.abs().max() >= pc.MIN_PEAK and sa > 100 * s1.abs()
    total = g.numel()
    for use_mag, scale in itertools.product((0, 1), (0.01, 0.4)):
        gs = g * scale / g.pow(2).mean().sqrt()
        part = th.stack([gs.sum(), gs.pow(2).sum()]).reshape(1, 2)
        sc = tr.scalars(th.tensor([2.0, 3.0]), th.tensor([[1.0, 2.0, 4.0]]), part, total, use_mag)
        # the oracle's cond_fn: mag = g.square().mean().sqrt(); g = g * mag.clamp(max=0.05) / mag; log["Grad"] = g.mean()
        mag = gs.square().mean().sqrt()
        gc = gs * mag.clamp(max=0.05) / mag if use_mag else gs
        _close(sc, th.stack([th.tensor(5.0).double(), th.tensor(1.0).double(), th.tensor(2.0).double(), th.tensor(4.0).double(),
                             th.tensor(12.0).double(), mag, gc.mean(), gc.pow(2).mean().sqrt() / mag]), 1e-12)
        assert abs(sc[5].item() - scale) < 1e-12 and abs(sc[7].item() - (0.125 if use_mag and scale == 0.4 else 1.0)) < 1e-12
    for n_clip, nblk, mag in itertools.product((1, 7, 300), (1, 23, 1024), (0.01, 0.4)):
        cp, lp, gp = tr.scalars_inputs(n_clip, nblk, 256 * nblk, mag)
        sc = tr.scalars(cp, lp, gp, 256 * nblk, 1)
        assert cp.shape == (n_clip,) and lp.shape == (nblk, 3) and gp.shape == (nblk, 2)
        assert abs(sc[5].item() / mag - 1) < 1e-6 and (sc[:6] > 0).all() and sc[7] >= 0.125 - 1e-6  # graded as ratios to these


@pytest.mark.parametrize("step", sorted(tr.STEPS))
def test_sample_update_references_match_the_oracle_steps(tab, oracle, step):
    """p_sample_with_grad / ddim_sample_with_grad of the oracle, driven with a model that returns the eps-hat and variance channel the
    reference's inputs imply and a cond_fn that returns the given g"""
    i = tr.STEPS[step]
    k = tab.step_coef(i, i)
    c = tr.coef(k)
    shape = (2, 6, 5)
    t = th.full((2,), i, dtype=th.long)
    for with_g, fct in ((False, 1.0), (True, 1.0), (True, 0.37)):
        # mode 1: the oracle recomputes pred_xstart from (x, eps-hat): give it the eps-hat of the recipe's (x, x0)
        inp = tr.update_inputs(shape, 1, i, k)
        x, x0 = inp["x"].double(), inp["x0"].double()
        eps = (c["sqrt_recip"] * x - x0) / c["sqrt_recipm1"]
        model = lambda xx, tt: th.cat([eps, th.zeros_like(eps)], dim=1)  # noqa: E731
        cond = (lambda xx, tt, p, **kw: inp["g"].double() * fct) if with_g else None
        o = oracle.ddim_sample_with_grad(model, x, t, clip_denoised=False, cond_fn=cond, noise=inp["noise"].double())
        s, p = tr.sample_update(1, inp["x"], inp["x0"], None, None, inp["g"] if with_g else None, None, fct, k)
        amp = max(1.0, c["sqrt_recip"] * 8)  # the oracle's x0-hat = a x - b eps in float64 with float32 coefficients
        _close(s, o["sample"], 1e-6 * amp)
        _close(p, o["pred_xstart"], 1e-6 * amp)
        assert s.abs().max() >= pc.MIN_PEAK and th.isfinite(s).all()
        # mode 0: mean and log-variance are inputs; the oracle's p_sample_with_grad composes them as the reference does
        inp = tr.update_inputs(shape, 0, i, k)
        assert inp["logvar"].min() >= min(k.min_log, k.max_log) - 1e-5 and inp["logvar"].max() <= max(k.min_log, k.max_log) + 1e-5
        mean, lv = inp["mean"].double(), inp["logvar"].double()
        gv = inp["g"].double() * fct if with_g else 0.0
        want = mean + th.exp(lv) * gv + (0.0 if i == 0 else th.exp(0.5 * lv) * inp["noise"].double())
        s, p = tr.sample_update(0, None, inp["x0"], inp["mean"], inp["logvar"], inp["g"] if with_g else None, inp["noise"], fct, k)
        _close(s, want, 1e-12)
        assert p.equal(inp["x0"].double()) and s.abs().max() >= pc.MIN_PEAK
        if i == 0:
            s2, _ = tr.sample_update(0, None, inp["x0"], inp["mean"], inp["logvar"], inp["g"] if with_g else None, None, fct, k)
            assert s2.equal(s)


def test_p_sample_with_grad_composition_is_the_mode0_formula(oracle):
    """mode 0 restates oracle/diffusion.py p_sample_with_grad + condition_mean_with_grad once: mean + variance g + [t != 0] exp(log_variance / 2) noise"""
    gen = th.Generator().manual_seed(0)
    x = th.randn(1, 3, 4, 4, generator=gen).double()
    out6 = th.randn(1, 6, 4, 4, generator=gen).double()
    g, noise = th.randn(1, 3, 4, 4, generator=gen).double(), th.randn(1, 3, 4, 4, generator=gen).double()
    for i in (0, 125):
        t = th.full((1,), i, dtype=th.long)
        p = oracle.p_mean_variance(lambda xx, tt: out6, x, t, clip_denoised=False)
        o = oracle.p_sample_with_grad(lambda xx, tt: out6, x, t, clip_denoised=False, cond_fn=lambda xx, tt, pp, **kw: g, noise=noise)

        class K:
            nonzero = int(i != 0)
            sqrt_recip = sqrt_recipm1 = coef1 = coef2 = min_log = max_log = fac = sqrt_one_minus_ab = sqrt_ab_prev = sqrt_one_minus_ab_prev = 0.0
        s, x0 = tr.sample_update(0, None, p["pred_xstart"], p["mean"], p["log_variance"], g, noise, 1.0, K)
        _close(s, o["sample"], 1e-6)  # condition_mean_with_grad casts mean and g to float32
        _close(x0, o["pred_xstart"], 1e-12)


@pytest.mark.parametrize("shape", tr.SHAPES)
def test_every_recipe_gives_references_above_the_vacuous_peak(tab, shape):
    for step, i in tr.STEPS.items():
        k = tab.step_coef(i, i)
        for t in tr.pmv_blend(*tr.pmv_inputs(shape, i, k), k):
            assert t.abs().max().item() >= pc.MIN_PEAK
        x_in, x0, g_clip = tr.combine_inputs(shape, i)
        if x_in.numel() > 1000:
            assert 0.3 < (x_in.abs() > 1).float().mean().item() < 0.5 and 0.3 < (x0.abs() > 1).float().mean().item() < 0.5
        for name, (tv, rng, sat, with_clip) in tr.SETTINGS.items():
            gd, se, losses = tr.guidance_combine(g_clip if with_clip else None, x_in, x0, k, tv * tr.SCALES[0], rng * tr.SCALES[1],
                                                 sat * tr.SCALES[2])
            assert gd.abs().max() > 0 and se.abs().max() > 0, "unit_seed needs a non-zero leg"
            for on, v in zip((tv, rng, sat), losses):
                assert (v.item() >= pc.MIN_PEAK) if on else (v.item() == 0.0), (shape, step, name, losses)
        for mode in (0, 1):
            inp = tr.update_inputs(shape, mode, i, k)
            s, _ = tr.sample_update(mode, inp.get("x"), inp["x0"], inp.get("mean"), inp.get("logvar"), inp["g"], inp["noise"], 0.37, k)
            assert s.abs().max().item() >= pc.MIN_PEAK and th.isfinite(s).all()
    g = tr.grad_finish(*tr.finish_inputs(shape))[0]
    assert g.abs().max().item() >= pc.MIN_PEAK


# ---- reference helpers of the cutout cases in tests/parity_checks.py ---------------------------------------------------------------------
def test_grouped_cutout_reference_equals_the_oracle_make_cutouts():
    x = th.randn(2, 3, 24, 20, generator=pc.g(1)).double().requires_grad_()
    for coords, cs in ((pc.CUTOUT_EXTENT_COORDS, 8), ([(k % 9, (3 * k) % 11, 4 + k % 5) for k in range(40)], 4)):
        want = og.MakeCutouts(cs, len(coords))(x, coords=coords)
        got = pc.pool_cutouts_grouped(x, coords, cs)
        assert got.shape == want.shape and th.equal(got, want)
        dy = th.randn(want.shape, generator=pc.g(2)).double()
        _close(th.autograd.grad((got * dy).sum(), x)[0], th.autograd.grad((want * dy).sum(), x)[0], 1e-13)  # another order of summation


def test_cutout_edge_cases_have_the_stated_geometry():
    cases = {c[:6]: c for c in pc.cutout_edge_cases()}
    B, H, W, cutn, cs, patch, coords = cases[(2, 24, 20, 6, 8, 4)]
    ext = [(min(s, H - oy), min(s, W - ox)) for ox, oy, s in coords]
    assert ext[2:4] == [(1, 1), (2, 3)] and ext[0][0] == 1 and ext[0][1] > 1 and ext[1][1] == 1 and ext[1][0] > 1
    assert ext[4] == (24, 20) and ext[5] == (7, 7)
    B, H, W, cutn, cs, patch, coords = cases[(4, 16, 16, 5462, 4, 2)]
    assert B * 3 * cutn == 65544 and 65535 // (B * 3) == cutn - 1 and len(coords) == cutn
    for B, H, W, cutn, cs, patch, coords in cases.values():
        assert len(coords) == cutn and (patch == 0 or cs % patch == 0)
        assert all(0 <= ox < W and 0 <= oy < H and s >= 1 for ox, oy, s in coords)
        mx = max(H, W)  # the launchers' own ranges: these cases are meant to run, not to be refused
        assert mx * mx * cs < 2 ** 32 and (cs + 1) * mx * cs < 2 ** 32 and cs ** 3 < 2 ** 32 and H * W * W < 2 ** 32 and B * 3 <= 65535
    assert {(14, 224), (14, 336), (0, 448)} <= {(c[5], c[4]) for c in cases.values()} and {256, 257} <= {c[3] for c in cases.values()}
