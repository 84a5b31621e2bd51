"""Resized cutouts (csrc/cutresize.hip) on the GPU: forward and adjoint against the float64 restatement (tests/resize_ref.py) at the literal
bound |a - b| <= 1e-4 + 1e-3 |ref|, the adjoint identity, a bit-reproducible backward, accumulate, MakeCutoutsResized as an autograd node,
ClipGuidance's CLIP leg against its torch leg, and a two-step ddim run whose schedule changes the cut count between the steps."""
import functools

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import guidance as dg
from tests import resize_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
MEAN = th.tensor(dg.CLIP_MEAN, dtype=th.float64).view(1, 3, 1, 1)
STD = th.tensor(dg.CLIP_STD, dtype=th.float64).view(1, 3, 1, 1)


@pytest.fixture(scope="module")
def ctx():
    from cgd_amd import lib
    return lib.Context(0, 1)


def close(name, got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    err = (got - ref).abs()
    print(f"{name}: max |diff| {float(err.max()):.3e}, peak |ref| {float(ref.abs().max()):.3e}")
    assert th.isfinite(got).all()
    assert bool((err <= 1e-4 + 1e-3 * ref.abs()).all()), name


def close_with_ties(name, got, ref):
    """the bound tests/test_gpu_cutaug.py puts on quantities behind a CLIP tower: the literal inequality for all but 1e-4 of the elements"""
    bad = ((got - ref).abs() > 1e-4 + 1e-3 * ref.abs())
    n = int(bad.sum())
    print(f"{name}: {n} of {ref.numel()} elements outside, max |diff| {float((got - ref).abs().max()):.3e}")
    assert th.isfinite(got).all()
    assert n <= 1e-4 * ref.numel(), (name, n, ref.numel())


def to_patch_rows(img, P):
    N, C, cs, _ = img.shape
    g = cs // P
    return img.view(N, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N * g * g, C * P * P)


# (B, H, W, cs, layout, patch) and the cuts (ox, oy, w, h, flags): one overview of each flag combination, an upscaled inner cut (gray) and a
# cut touching the bottom-right border.  Overviews downscale (anisotropically on the 40 x 56 image); the border cut is the identity
# (extent == cs) in the first and third case and a downscale in the second.
CASES = {
    "48-16": ((1, 48, 48, 16, 0, 0), [(0, 0, 48, 48, f) for f in range(4)] + [(7, 11, 9, 9, 1), (32, 32, 16, 16, 0)]),
    "40x56-32": ((2, 40, 56, 32, 1, 16), [(0, 0, 56, 40, f) for f in range(4)] + [(3, 5, 20, 20, 1), (20, 4, 36, 36, 2)]),
    "256-224": ((1, 256, 256, 224, 1, 32), [(0, 0, 256, 256, f) for f in range(4)] + [(30, 50, 100, 100, 1), (32, 32, 224, 224, 0)]),
}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """input, cotangent and the float64 reference forward / gradient of a case, computed once"""
    (B, H, W, cs, layout, patch), recs = CASES[name]
    gen = th.Generator().manual_seed(len(name) + H)
    x = th.rand(B, 3, H, W, generator=gen, dtype=th.float64) * 2 - 1
    y = th.randn(len(recs) * B, 3, cs, cs, generator=gen, dtype=th.float64)
    xr = x.clone().requires_grad_()
    ref = (R.cutouts((xr + 1) / 2, recs, cs) - MEAN) / STD
    g, = th.autograd.grad((ref * y).sum(), xr)
    return x, y, ref.detach(), g


def table_of(recs, H, W):
    return th.tensor(dg.resize_table(recs, H, W), dtype=th.int32, device=DEV)


def native_fwd(ctx, x, recs, cs, layout, patch):
    B, _, H, W = x.shape
    n = len(recs)
    tab = table_of(recs, H, W)
    out = th.empty((n * B * (cs // patch) ** 2, 3 * patch * patch) if layout else (n * B, 3, cs, cs), device=DEV)
    ctx.check(ctx.lib.cgd_cutouts_resize_fwd(ctx.h, x.data_ptr(), tab.data_ptr(), tab.data_ptr() + 16 * n, out.data_ptr(), B, H, W, n, cs,
                                             layout, patch, ctx.stream()))
    return out


def native_bwd(ctx, d, recs, shape, cs, layout, patch, g, accumulate):
    B, _, H, W = shape
    n = len(recs)
    tab = table_of(recs, H, W)
    scratch = th.empty(ctx.lib.cgd_cutouts_resize_scratch_floats(B, H, W, n), device=DEV)
    ctx.check(ctx.lib.cgd_cutouts_resize_bwd(ctx.h, d.data_ptr(), tab.data_ptr(), tab.data_ptr() + 16 * n, g.data_ptr(), scratch.data_ptr(),
                                             B, H, W, n, cs, layout, patch, int(accumulate), ctx.stream()))
    return g


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_the_exact_restatement(ctx, name):
    (B, H, W, cs, layout, patch), recs = CASES[name]
    x, _, ref, _ = case_data(name)
    got = native_fwd(ctx, x.float().to(DEV), recs, cs, layout, patch)
    close(f"fwd {name}", got, to_patch_rows(ref, patch) if layout else ref)


@pytest.mark.parametrize("name", list(CASES))
def test_backward_matches_autograd_is_deterministic_and_accumulates(ctx, name):
    (B, H, W, cs, layout, patch), recs = CASES[name]
    x, y, _, want = case_data(name)
    d = (to_patch_rows(y, patch) if layout else y).float().contiguous().to(DEV)
    g1 = native_bwd(ctx, d, recs, x.shape, cs, layout, patch, th.full(x.shape, 0.25, device=DEV), True)
    g2 = native_bwd(ctx, d, recs, x.shape, cs, layout, patch, th.full(x.shape, float("nan"), device=DEV), False)
    g3 = native_bwd(ctx, d, recs, x.shape, cs, layout, patch, th.empty(x.shape, device=DEV), False)
    assert th.equal(g2, g3)
    assert float((g1 - (g2 + 0.25)).abs().max()) <= 1e-6 * max(1.0, float(g2.abs().max()))
    close(f"bwd {name}", g2, want)


@pytest.mark.parametrize("name", ["40x56-32", "256-224"])
def test_adjoint_identity(ctx, name):
    (B, H, W, cs, layout, patch), recs = CASES[name]
    x = case_data(name)[0].float().to(DEV)
    fx = native_fwd(ctx, x, recs, cs, layout, patch)
    f0 = native_fwd(ctx, th.zeros_like(x), recs, cs, layout, patch)  # the operator is affine: (x + 1) / 2 and the normalisation
    y = th.randn(fx.shape, generator=th.Generator(device=DEV).manual_seed(2), device=DEV)
    g = native_bwd(ctx, y, recs, x.shape, cs, layout, patch, th.empty_like(x), False)
    lhs = float(((fx - f0).double() * y.double()).sum())
    rhs = float((x.double() * g.double()).sum())
    print(f"adjoint identity {name}: {lhs:.9e} vs {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


def test_host_checkable_arguments_fail_before_any_launch(ctx):
    from cgd_amd.lib import CgdError
    x = th.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(CgdError, match="multiple of the patch"):
        native_fwd(ctx, x, [(0, 0, 32, 32, 0)], 24, 1, 16)
    with pytest.raises(CgdError, match="multiple of the patch"):
        native_bwd(ctx, th.zeros(4, 768, device=DEV), [(0, 0, 32, 32, 0)], x.shape, 24, 1, 16, th.empty_like(x), False)
    for bad in [(0, 0, 0, 8, 0), (30, 0, 8, 8, 0), (0, 25, 8, 8, 0)]:
        with pytest.raises(ValueError):
            native_fwd(ctx, x, [bad], 16, 0, 0)


def test_make_cutouts_resized_on_the_gpu(ctx):
    B, H, W, cs = 2, 40, 56, 16
    x = th.rand(B, 3, H, W, generator=th.Generator().manual_seed(4)).to(DEV)
    outs = []
    for native in (True, False):
        th.manual_seed(6)
        mk = dg.MakeCutoutsResized(cs, overview=4, inner=3, ctx=ctx)
        xr = x.clone().requires_grad_()
        out = mk(xr) if native else mk.resized(xr, mk.draw(W, H))
        assert out.shape == (7 * B, 3, cs, cs) and out.requires_grad
        w = th.linspace(-1, 1, out.numel(), device=DEV).view_as(out)
        g, = th.autograd.grad((out * w).sum(), xr)
        outs.append((out.detach(), g))
    close("MakeCutoutsResized fwd", outs[0][0], outs[1][0])
    close("MakeCutoutsResized bwd", outs[0][1], outs[1][1])
    with th.no_grad():
        th.manual_seed(6)
        plain = dg.MakeCutoutsResized(cs, overview=4, inner=3, ctx=ctx)(x)
    assert th.equal(plain, outs[0][0])


def _guidance(ctx, names, mk):
    from cgd_amd import nets, synthetic
    towers, targets = [], []
    for k, name in enumerate(names):
        if name in nets.VIT_CONFIGS:
            t = nets.ClipImageTower(ctx, name)
            t.load_state_dict(synthetic.synthetic_state_dict(t, seed=4321))
        else:
            t = nets.ClipResNetTower(ctx, name)
            t.load_state_dict(synthetic.resnet_state_dict(t, seed=2468))
        towers.append(t)
        targets.append(th.randn(2, t.out_dim, generator=th.Generator(device=DEV).manual_seed(11 + k), device=DEV))
    return dg.ClipGuidance(ctx, None, towers, None, targets, [1.0, 0.5], mk.cutn, make_cutouts=mk)


@pytest.mark.parametrize("names", [("ViT-B/32",), ("RN50",)])
def test_clip_leg_matches_the_torch_leg(ctx, names):
    """ClipGuidance's resized CLIP leg, native against _clip_leg_torch on the same records: d(CLIP loss)/dx_in (accumulated onto a
    non-zero gclip), the CLIP loss and the tower's embeddings."""
    B, H, W = 1, 256, 256
    mk = dg.MakeCutoutsResized(224, overview=4, inner=4, ctx=ctx)
    guid = _guidance(ctx, names, mk)
    x_in = th.tanh(th.randn(B, 3, H, W, generator=th.Generator(device=DEV).manual_seed(3), device=DEV))
    th.manual_seed(1)
    recs = mk.draw(W, H)
    cutn = len(recs)
    wm = dg.prompt_weight_matrix(th.tensor([1.0, 0.5]), B, DEV)
    res = {}
    for leg in ("native", "torch"):
        gclip = th.full((B, 3, H, W), 0.5, device=DEV)
        part = th.empty(len(names) * cutn * B, device=DEV)
        fn = guid._clip_leg if leg == "native" else guid._clip_leg_torch
        fn(x_in, dg._CutLaunch(ctx.lib, recs, table_of(recs, H, W), resized=True), wm, None, gclip, part, 1)
        th.cuda.synchronize()
        res[leg] = (gclip - 0.5, float(part.double().sum()), guid.emb.clone())
    (g_n, l_n, e_n), (g_t, l_t, e_t) = res["native"], res["torch"]
    print(f"{names}: CLIP loss native {l_n:.6f} torch {l_t:.6f}; |g| peak {float(g_t.abs().max()):.3e}")
    assert abs(l_n - l_t) <= 1e-4 + 1e-3 * abs(l_t)
    close_with_ties("emb", e_n, e_t)
    close_with_ties("g_clip_in", g_n, g_t)


def test_two_ddim_steps_with_a_schedule_that_changes_the_cut_count(ctx):
    """GuidedSampler's ddim loop with a MakeCutoutsResized whose schedule gives 4 + 2 cuts on the first step and 1 + 3 on the second: the
    counts reach the launches (half of the run is done at the first step, all of it at the second) and the steps are finite."""
    import itertools

    from cgd_amd import diffusion, nets, sampler, synthetic
    from tests import parity_checks as pc
    from tests import step_checks
    unet = nets.UNet(ctx, **pc.UNET_CASES["mini"])
    unet.load_state_dict(synthetic.synthetic_state_dict(unet, seed=1234, device=DEV))
    tower = nets.ClipImageTower(ctx, config=step_checks.MINI_VIT)
    tower.load_state_dict(synthetic.synthetic_state_dict(tower, seed=4321))
    tables = diffusion.create_gaussian_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="ddim2")
    B, H, W = 1, 32, 48
    target = th.randn(1, tower.out_dim, generator=th.Generator(device=DEV).manual_seed(9), device=DEV)

    def run():
        smp = sampler.GuidedSampler(ctx, tables)
        mk = dg.MakeCutoutsResized(tower.input_resolution, overview=1, inner=3, schedule=[(0.75, 4, 2)], ctx=ctx)
        guid = dg.ClipGuidance(ctx, unet, tower, smp, target, [1.0], 16, clip_guidance_scale=100.0, tv_scale=1.0, range_scale=1.0,
                               make_cutouts=mk)
        th.manual_seed(21)
        th.cuda.manual_seed(21)
        loop = smp.ddim_sample_loop_progressive(unet, (B, 3, H, W), clip_denoised=False, cond_fn=guid, device=DEV, cond_fn_with_grad=True,
                                                model_kwargs={"y": th.zeros(B, dtype=th.long, device=DEV)})
        guid.current_timestep = smp.num_timesteps - 1
        counts, outs = [], []
        for out in itertools.islice(loop, 2):
            th.cuda.synchronize()
            counts.append([r[4] for r in mk.last_coords])
            outs.append((out["sample"].clone(), guid.log()["CLIP Loss"]))
            guid.current_timestep -= 1
        return counts, outs

    counts, outs = run()
    assert [len(c) for c in counts] == [6, 4] and counts[0][:4] == [0, 1, 2, 3] and counts[1][0] == 0
    for sample, loss in outs:
        assert th.isfinite(sample).all() and loss == loss and loss > 0
