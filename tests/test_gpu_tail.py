"""GPU tests of the step-tail kernels every sampler shares (csrc/guidance.hip: cgd_pmv_blend, cgd_guidance_combine, cgd_grad_finish,
cgd_scalars, cgd_sample_update), each alone through the C ABI against the float64 references of tests/tail_ref.py.

Shapes (tail_ref.SHAPES) are the smallest that reach each path: one partial block with dead lanes, a TV stencil without a vertical / a
horizontal neighbour, H != W with row, plane and sample borders, and two shapes above the 1024-block cap of the grid-stride launches (a
ragged one and the batch-2 production shape).  Steps: a middle one, index 0 and the last index of the 250-step linear schedule (a = 157).
Gradients are graded at unit peak of their own reference (`unit_seed`), so the TV, range and saturation terms are each graded alone.
Where a result is a difference of terms 157 times larger it carries step_checks' named criterion `cancelling-legs` (atol counted in units
of max(1, max|a x|)); the strict verdict is reported beside it."""
import itertools

import pytest
import torch as th

from tests import parity_checks as pc
from tests import tail_ref as tr

pytestmark = pytest.mark.gpu

DEV = pc.DEV
NAN = float("nan")
SHAPE_IDS = ["x".join(map(str, s)) for s in tr.SHAPES]


def _assert_all(recs):
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


@pytest.fixture(scope="module")
def rig():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    return L.Context(0, 1), dd.create_gaussian_diffusion(*tr.SCHEDULE), L


def _coef(tab, step):
    return tab.step_coef(tr.STEPS[step], tr.STEPS[step])


def _nan(*shape):
    return th.full(shape, NAN, device=DEV)


def _dev(t):
    return None if t is None else t.to(DEV)


def _rec_cancel(name, got, ref, leg_peak):
    """`cancelling-legs`: |got - ref| <= atol max(1, peak of the cancelling leg) + rtol |ref|"""
    r = pc.rec(name, got, ref)
    scale = max(1.0, leg_peak)
    r.update(criterion="cancelling-legs", ok=pc.rec(name, got, ref, atol=pc.ATOL * scale)["ok"],
             reason=f"difference of two terms of peak {scale:.3g} (a x and b eps); atol counted in units of that peak (strict verdict in ok_strict)")
    return r


def _rec_sum(name, got, ref, sum_abs):
    """a cancelling sum: within 1e-4 of the sum of magnitudes (a float32 tree of this depth errs by ~1e-6 of it)"""
    return pc.rec(name, th.as_tensor(got).double().reshape(1) / sum_abs, th.as_tensor(ref).double().reshape(1) / sum_abs, rtol=0.0, allow_small=True)


def _partials(part, nblk, width):
    """the device's per-block partial array, pre-filled with NaN and 3 floats longer than it should be written -> (blocks, width) float64"""
    p = part.double().cpu()
    assert th.isnan(p[nblk * width:]).all(), "the kernel wrote past its last block's partial"
    assert not th.isnan(p[:nblk * width]).any(), "fewer blocks wrote a partial than cgd_guidance_part_blocks reports"
    return p[:nblk * width].reshape(nblk, width)


# ---- cgd_pmv_blend ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", tr.SHAPES, ids=SHAPE_IDS)
def test_pmv_blend_matches_fp64(rig, shape):
    ctx, tab, L = rig
    B, H, W = shape
    recs = []
    for step in tr.STEPS:
        k = _coef(tab, step)
        x, out6 = tr.pmv_inputs(shape, tr.STEPS[step], k)
        outs = [_nan(B, 3, H, W) for _ in range(4)]
        xd, od = x.to(DEV), out6.to(DEV)
        ctx.check(ctx.lib.cgd_pmv_blend(ctx.h, xd.data_ptr(), od.data_ptr(), *[o.data_ptr() for o in outs], B, H, W, k, ctx.stream()))
        th.cuda.synchronize()
        leg = (float(k.sqrt_recip) * x.double()).abs().max().item()
        for name, got, ref in zip(("pred_xstart", "mean", "log_variance", "x_in"), outs, tr.pmv_blend(x, out6, k)):
            tag = f"pmv_blend {SHAPE_IDS[tr.SHAPES.index(shape)]} {step} {name}"
            if step == "last" and name in ("pred_xstart", "x_in"):
                recs.append(_rec_cancel(tag, got, ref, leg))
            else:
                recs.append(pc.rec(tag, got, ref))
    _assert_all(recs)


# ---- cgd_guidance_combine ----------------------------------------------------------------------------------------------------------------
def _combine(rig, shape, k, g_clip, x_in, x0, scales):
    ctx, tab, L = rig
    B, H, W = shape
    nblk = ctx.lib.cgd_guidance_part_blocks(B, H, W)
    assert nblk == tr.blocks(B, H, W)
    gdir, seed6, part = _nan(B, 3, H, W), _nan(B, 6, H, W), _nan(nblk * 3 + 3)
    gc, xi, xz = _dev(g_clip), x_in.to(DEV), x0.to(DEV)
    ctx.check(ctx.lib.cgd_guidance_combine(ctx.h, L.ptr(gc), xi.data_ptr(), xz.data_ptr(), gdir.data_ptr(), seed6.data_ptr(), part.data_ptr(),
                                           B, H, W, k, *scales, ctx.stream()))
    th.cuda.synchronize()
    return gdir.double().cpu(), seed6.double().cpu(), _partials(part, nblk, 3), part


def _grade_combine(tag, recs, gdir, seed6, lsum, g_direct, seed_eps, losses, on):
    assert (seed6[:, 3:] == 0).all(), f"{tag}: the variance half of the seed must be exactly zero"
    for name, got, ref in (("g_direct", gdir, g_direct), ("seed_eps", seed6[:, :3], seed_eps)):
        sd = pc.unit_seed(ref)
        recs.append(pc.rec(f"{tag} {name} (unit peak)", got * sd, ref * sd))
    for j, name in enumerate(("TV", "range", "saturation")):
        if on[j]:
            recs.append(pc.rec(f"{tag} {name} loss [rtol 1e-3, atol 0]", lsum[j].reshape(1), losses[j].reshape(1), atol=0.0, allow_small=True))
        else:
            assert lsum[j].item() == 0.0, f"{tag}: {name} loss with a zero scale"


@pytest.mark.parametrize("shape", tr.SHAPES, ids=SHAPE_IDS)
def test_guidance_combine_each_term_alone_matches_fp64_autograd(rig, shape):
    tab = rig[1]
    recs = []
    for step in tr.STEPS:
        k = _coef(tab, step)
        x_in, x0, g_clip = tr.combine_inputs(shape, tr.STEPS[step])
        for setting, (tv, rng, sat, with_clip) in tr.SETTINGS.items():
            scales = (tv * tr.SCALES[0], rng * tr.SCALES[1], sat * tr.SCALES[2])
            gc = g_clip if with_clip else None
            gdir, seed6, lpart, _ = _combine(rig, shape, k, gc, x_in, x0, scales)
            g_direct, seed_eps, losses = tr.guidance_combine(gc, x_in, x0, k, *scales)
            _grade_combine(f"combine {SHAPE_IDS[tr.SHAPES.index(shape)]} {step} {setting}", recs, gdir, seed6, lpart.sum(0), g_direct, seed_eps,
                           losses, (tv, rng, sat))
    _assert_all(recs)


def test_guidance_combine_at_the_clamp_kinks(rig):
    """exactly +-1, +-(1 + 2^-23) and 0 in x_in and x0: no saturation / range contribution at exactly +-1, sign and magnitude just beyond"""
    tab = rig[1]
    x_in, x0 = tr.combine_edge_inputs()
    recs = []
    for step, (rs, ss) in itertools.product(("mid", "last"), ((50.0, 0.0), (0.0, 30.0), (50.0, 30.0))):
        k = _coef(tab, step)
        gdir, seed6, lpart, _ = _combine(rig, (1, 5, 5), k, None, x_in, x0, (0.0, rs, ss))
        g_direct, seed_eps, losses = tr.combine_edge_closed_form(x_in, x0, k, rs, ss)
        dead = (x0.abs() <= 1) if ss == 0 else ((x_in.abs() <= 1) if rs == 0 else (x0.abs() <= 1) & (x_in.abs() <= 1))
        assert (gdir[dead] == 0).all() and (seed6[:, :3][dead] == 0).all() and (gdir[~dead] != 0).all()
        _grade_combine(f"combine kinks {step} range {rs:g} sat {ss:g}", recs, gdir, seed6, lpart.sum(0), g_direct, seed_eps,
                       th.cat([th.zeros(1, dtype=th.float64), losses]), (0, rs != 0, ss != 0))
    _assert_all(recs)


# ---- cgd_grad_finish ------------------------------------------------------------------------------------------------------------------
def _finish(rig, shape, gd, gu):
    ctx, tab, L = rig
    B, H, W = shape
    nblk = tr.blocks(B, H, W)
    g, part = _nan(B, 3, H, W), _nan(nblk * 2 + 3)
    gdd, gud = gd.to(DEV), _dev(gu)
    ctx.check(ctx.lib.cgd_grad_finish(ctx.h, gdd.data_ptr(), L.ptr(gud), g.data_ptr(), part.data_ptr(), B, H, W, ctx.stream()))
    th.cuda.synchronize()
    return g, _partials(part, nblk, 2), part


@pytest.mark.parametrize("shape", tr.SHAPES, ids=SHAPE_IDS)
def test_grad_finish_matches_fp64(rig, shape):
    gd, gu = tr.finish_inputs(shape)
    recs = []
    for with_unet in (True, False):
        g, gpart, _ = _finish(rig, shape, gd, gu if with_unet else None)
        ref, s1, s2, sa = tr.grad_finish(gd, gu if with_unet else None)
        tag = f"grad_finish {SHAPE_IDS[tr.SHAPES.index(shape)]} g_unet {int(with_unet)}"
        recs.append(pc.rec(f"{tag} g", g, ref))
        recs.append(pc.rec(f"{tag} sum g^2 [rtol 1e-3, atol 0]", gpart[:, 1].sum().reshape(1), s2.reshape(1), atol=0.0))
        recs.append(_rec_sum(f"{tag} sum g / sum |g|", gpart[:, 0].sum(), s1, sa))
    _assert_all(recs)


# ---- cgd_scalars ----------------------------------------------------------------------------------------------------------------------
SCALAR_NAMES = ("CLIP", "TV", "range", "saturation", "total", "magnitude", "grad mean", "clamp factor")


def _scalars(rig, shape, clip_part, lpart_dev, gpart_dev, use_mag):
    ctx = rig[0]
    B, H, W = shape
    out = _nan(8)
    cp = clip_part.to(DEV)
    ctx.check(ctx.lib.cgd_scalars(ctx.h, cp.data_ptr(), cp.numel(), lpart_dev.data_ptr(), gpart_dev.data_ptr(), B, H, W, use_mag, out.data_ptr(),
                                  ctx.stream()))
    th.cuda.synchronize()
    return out.double().cpu()


def _grade_scalars(tag, recs, got, ref, mean_unit):
    keep = [j for j in range(8) if j != 6]
    recs.append(pc.rec(f"{tag} {[SCALAR_NAMES[j] for j in keep]} / reference", got[keep] / ref[keep], th.ones(7, dtype=th.float64)))
    recs.append(pc.rec(f"{tag} grad mean, in units of mean |g| x clamp factor", got[6:7] / mean_unit, ref[6:7] / mean_unit, rtol=0.0, allow_small=True))


@pytest.mark.parametrize("shape", [(1, 5, 7), (1, 40, 48), (1, 296, 300)], ids=["1-block", "23-blocks", "1024-blocks"])
def test_scalars_matches_fp64(rig, shape):
    """block counts 1, 23 and 1024 x CLIP partial counts 1, 7 and 300 (both beyond the 256-thread stride) x use_magnitude x a magnitude on
    either side of the 0.05 clamp; fed synthetic partial arrays and the device's own (cgd_guidance_combine / cgd_grad_finish outputs)"""
    tab = rig[1]
    B, H, W = shape
    nblk, total = tr.blocks(*shape), B * 3 * H * W
    assert nblk == {7: 1, 48: 23, 300: 1024}[W]
    recs = []
    # the device's own loss partials, and its gradient partials of a g of the wanted magnitude
    x_in, x0, g_clip = tr.combine_inputs(shape, 125)
    lpart_dev = _combine(rig, shape, _coef(tab, "mid"), g_clip, x_in, x0, tr.SCALES)[3]
    gd, gu = tr.finish_inputs(shape)
    rms = tr.grad_finish(gd, gu)[0].pow(2).mean().sqrt().item()
    for n_clip, use_mag, mag in itertools.product((1, 7, 300), (0, 1), (0.01, 0.4)):
        tag = f"scalars {nblk} blocks n_clip {n_clip} use_magnitude {use_mag} magnitude {mag:g}"
        clip_part, lp, gp = tr.scalars_inputs(n_clip, nblk, total, mag)
        # synthetic partials
        fct = min(mag, 0.05) / mag if use_mag else 1.0
        ref = tr.scalars(clip_part, lp, gp, total, use_mag)
        got = _scalars(rig, shape, clip_part, lp.to(DEV), gp.to(DEV), use_mag)
        _grade_scalars(tag + " [synthetic]", recs, got, ref, gp[:, 0].double().abs().sum().item() / total * fct)
        # the device's own
        gds, gus = (gd.double() * mag / rms).float(), (gu.double() * mag / rms).float()
        g, _, gpart_dev = _finish(rig, shape, gds, gus)
        ref = tr.scalars(clip_part, lpart_dev[:nblk * 3].cpu(), gpart_dev[:nblk * 2].cpu(), total, use_mag)
        got = _scalars(rig, shape, clip_part, lpart_dev, gpart_dev, use_mag)
        _grade_scalars(tag + " [device partials]", recs, got, ref, g.double().abs().sum().item() / total * fct)
        assert abs(ref[5].item() / mag - 1) < 1e-3 and abs(ref[7].item() - fct) < 1e-3 * fct, "the inputs set the magnitude the case names"
        if mag < 0.05 or not use_mag:
            assert got[7].item() == 1.0, f"{tag}: the clamp factor below 0.05 is exactly 1"
    _assert_all(recs)


# ---- cgd_sample_update ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["p_sample", "ddim"])
@pytest.mark.parametrize("shape", tr.SHAPES, ids=SHAPE_IDS)
def test_sample_update_matches_fp64(rig, shape, mode):
    """the inputs a mode does not use (x in mode 0; mean, log-variance and noise in mode 1; noise at index 0) are NaN-filled: a finite
    output proves that they are not read"""
    ctx, tab, L = rig
    B, H, W = shape
    recs = []
    for step, (with_g, clamp) in itertools.product(tr.STEPS, ((False, False), (True, False), (True, True))):
        k = _coef(tab, step)
        inp = tr.update_inputs(shape, mode, tr.STEPS[step], k)
        use_noise = mode == 0 and step != "first"
        dev = {n: (_dev(inp[n]) if n in inp and (n != "noise" or use_noise) else _nan(B, 3, H, W)) for n in ("x", "x0", "mean", "logvar", "noise")}
        g = inp["g"] if with_g else None
        gdev = _dev(g)
        scal = th.tensor([0, 0, 0, 0, 0, 0, 0, 0.37]).float().to(DEV) if clamp else None
        sample, x0_out = _nan(B, 3, H, W), _nan(B, 3, H, W)
        ctx.check(ctx.lib.cgd_sample_update(ctx.h, dev["x"].data_ptr(), dev["x0"].data_ptr(), dev["mean"].data_ptr(), dev["logvar"].data_ptr(),
                                            L.ptr(gdev), dev["noise"].data_ptr(), L.ptr(scal), sample.data_ptr(), x0_out.data_ptr(), B, H, W, k,
                                            mode, ctx.stream()))
        th.cuda.synchronize()
        ref, _ = tr.sample_update(mode, inp.get("x"), inp["x0"], inp.get("mean"), inp.get("logvar"), g, inp["noise"] if use_noise else None,
                                  0.37 if clamp else 1.0, k)
        tag = f"sample_update mode {mode} {SHAPE_IDS[tr.SHAPES.index(shape)]} {step} g {int(with_g)} clamp {int(clamp)}"
        if mode == 1 and step == "last":
            recs.append(_rec_cancel(f"{tag} sample", sample, ref, (float(k.sqrt_recip) * inp["x"].double()).abs().max().item()))
        else:
            recs.append(pc.rec(f"{tag} sample", sample, ref))
        assert th.equal(x0_out.cpu(), inp["x0"]), f"{tag}: pred_xstart_out is the unconditioned input, bit for bit"
    _assert_all(recs)
