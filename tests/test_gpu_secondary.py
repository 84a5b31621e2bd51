"""The secondary-model guidance path on the GPU, through the C ABI, against tests/secondary_ref.py (fp32, CPU, autograd).

Criterion: tests/parity_checks.py's records at the literal |a - b| <= 1e-4 + 1e-3 |ref| — strict on pred, on every op kernel and on dx with
the ReLU masks replayed from the CPU run; the free-running dx is a record under the existing named `relu-flips` criterion with its strict
verdict reported beside it (as check_resnet / check_lpips_mask_replay do).  Shapes: 32x32 batch 1 (the bottom map is 1x1: the first
upsample is all border clamps) and 64x96 batch 2 (non-square, per-sample t, slice strides)."""
import functools
import math

import pytest
import torch as th
import torch.nn.functional as F

from tests import parity_checks as pc
from tests import secondary_ref
from tests.parity_checks import DEV, g, rec, rec_flips

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 32), (2, 64, 96)]


def _assert_ok(records):
    for r in records:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e} "
              f"[{r['criterion']}] strict={r['ok_strict']}")
    bad = [r for r in records if not r["ok"]]
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _pair():
    """(context, CPU reference, device net) on the same seeded weights; shared by the tests, never modified."""
    from cgd_amd import nets, synthetic
    ctx = pc._ctx(1)
    sd = synthetic.secondary_state_dict(seed=9753)
    ref = secondary_ref.build(sd)
    dev = nets.SecondaryModel(ctx)
    dev.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    return ctx, ref, dev


@functools.lru_cache(maxsize=None)
def _reference(B, H, W):
    """One CPU forward + backward per shape: inputs, pred, the unit-peak seed on v, dx and the 23 post-ReLU activations."""
    _, ref, _ = _pair()
    x = th.randn(B, 3, H, W, generator=g(300 + H))
    t = th.tensor([0.37, 0.81][:B])
    xr = x.clone().requires_grad_()
    with secondary_ref.CaptureRelu(ref) as cap:
        v = ref.v(xr, t)
    dv = th.randn(B, 3, H, W, generator=g(301 + W))
    (v * dv).sum().backward()
    scale = pc.unit_seed(xr.grad)
    with th.no_grad():
        pred = ref(x, t)
    return {"x": x, "t": t, "pred": pred, "dv": dv * scale, "dx": xr.grad * scale, "acts": [pc._nhwc_rows(a) for a in cap.acts]}


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_pred_and_dx_against_the_reference(B, H, W):
    ctx, _, dev = _pair()
    r = _reference(B, H, W)
    assert len(r["acts"]) == 23
    tag = f"secondary B{B} {H}x{W}"
    x, t, dv = r["x"].to(DEV), r["t"].to(DEV), r["dv"].to(DEV)
    pred = dev.forward(x, t)
    dx_free = dev.dgrad(dv)
    th.cuda.synchronize()
    out = [rec(f"{tag} pred", pred, r["pred"]), rec_flips(f"{tag} dx (device masks)", dx_free, r["dx"])]
    dev.debug_replay([a.to(DEV) for a in r["acts"]])
    try:
        pred_r = dev.forward(x, t)
        dx = dev.dgrad(dv)
        th.cuda.synchronize()
    finally:
        dev.debug_replay(None)
    out += [rec(f"{tag} pred (replayed activations)", pred_r, r["pred"]), rec(f"{tag} dx (reference masks)", dx, r["dx"])]
    _assert_ok(out)


def test_refusals_come_before_any_launch():
    from cgd_amd.lib import CgdError
    ctx, _, dev = _pair()
    import ctypes as C
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    with pytest.raises(CgdError, match="multiples of 32"):
        dev.forward(th.zeros(1, 3, 48, 64, device=DEV), th.zeros(1, device=DEV))
    with pytest.raises(CgdError, match="without a forward"):
        dev.dgrad(th.zeros(1, 3, 48, 64, device=DEV))  # the failed forward left nothing to differentiate
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before


def test_lifecycle_two_batch_sizes_on_one_handle():
    """Consecutive calls at different batch sizes and shapes on one handle: each answers for its own input, a dgrad belongs to the last
    forward, and a warm handle allocates nothing."""
    ctx, _, dev = _pair()
    out = []
    for (B, H, W) in [SHAPES[1], SHAPES[0], SHAPES[1]]:
        r = _reference(B, H, W)
        pred = dev.forward(r["x"].to(DEV), r["t"].to(DEV))
        out.append(rec(f"lifecycle pred B{B} {H}x{W}", pred, r["pred"]))
        out.append(rec_flips(f"lifecycle dx B{B} {H}x{W}", dev.dgrad(r["dv"].to(DEV)), r["dx"]))
    allocs = ctx.lib.cgd_ctx_device_allocs(ctx.h)
    r = _reference(*SHAPES[0])
    pred, xin = dev.forward(r["x"].to(DEV), r["t"].to(DEV), fac=0.25)
    dev.dgrad(r["dv"].to(DEV))
    th.cuda.synchronize()
    assert ctx.lib.cgd_ctx_device_allocs(ctx.h) == allocs, "a handle that has seen its largest shape allocates nothing"
    out.append(rec("lifecycle blend pred", pred, r["pred"]))
    out.append(rec("lifecycle blend x_in", xin, r["pred"] * 0.25 + r["x"] * 0.75))
    _assert_ok(out)


# ---- op kernels against torch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hi,Wi,C,ld_small,ld_big", [(1, 1, 1, 256, 256, 512), (2, 3, 5, 64, 68, 128), (1, 17, 9, 8, 8, 8)])
def test_bilinear_upsample_and_adjoint(B, Hi, Wi, C, ld_small, ld_big):
    """Forward and gather-form adjoint on channel slices (row strides wider than C, the slice not at column 0)."""
    ctx = _pair()[0]
    s = ctx.stream()
    a = th.randn(B, Hi, Wi, C, generator=g(310))
    d = th.randn(B, 2 * Hi, 2 * Wi, C, generator=g(311))
    ar = a.permute(0, 3, 1, 2).clone().requires_grad_()
    up = F.interpolate(ar, scale_factor=2, mode="bilinear", align_corners=False)
    (up * d.permute(0, 3, 1, 2)).sum().backward()
    off_s, off_b = ld_small - C, ld_big - C
    small = th.full((B * Hi * Wi, ld_small), 7.0, device=DEV)
    big = th.full((B * 4 * Hi * Wi, ld_big), 7.0, device=DEV)
    small[:, off_s:] = a.reshape(-1, C).to(DEV)
    ctx.check(ctx.lib.cgd_op_bilinear_up2x(ctx.h, small.data_ptr() + 4 * off_s, ld_small, big.data_ptr() + 4 * off_b, ld_big, B, Hi, Wi, C, 0, s))
    out = [rec("bilinear x2 forward", big[:, off_b:].cpu().view(B, 2 * Hi, 2 * Wi, C), up.detach().permute(0, 2, 3, 1))]
    assert bool((big[:, :off_b] == 7.0).all()), "columns outside the slice are untouched"
    big[:, off_b:] = d.reshape(-1, C).to(DEV)
    small.fill_(7.0)
    ctx.check(ctx.lib.cgd_op_bilinear_up2x(ctx.h, big.data_ptr() + 4 * off_b, ld_big, small.data_ptr() + 4 * off_s, ld_small, B, Hi, Wi, C, 1, s))
    out.append(rec("bilinear x2 adjoint", small[:, off_s:].cpu().view(B, Hi, Wi, C), ar.grad.permute(0, 2, 3, 1)))
    assert bool((small[:, :off_s] == 7.0).all())
    _assert_ok(out)


@pytest.mark.parametrize("B,Ho,Wo,C", [(1, 1, 1, 256), (2, 3, 5, 64)])
def test_average_pool_and_adjoint(B, Ho, Wo, C):
    """AvgPool2d(2) and its adjoint as the net runs them: the library's 2x2 pooling / nearest upsample kernels with scale 1/4."""
    ctx = _pair()[0]
    a = th.randn(B, 2 * Ho, 2 * Wo, C, generator=g(320))
    d = th.randn(B, Ho, Wo, C, generator=g(321))
    ar = a.permute(0, 3, 1, 2).clone().requires_grad_()
    p = F.avg_pool2d(ar, 2)
    (p * d.permute(0, 3, 1, 2)).sum().backward()
    from cgd_amd import ops
    got = ops.pool2x2(ctx, a.to(DEV), 0.25)
    gad = ops.upsample2x(ctx, d.to(DEV), 0.25)
    _assert_ok([rec("avg pool forward", got.view(B, Ho, Wo, C), p.detach().permute(0, 2, 3, 1)),
                rec("avg pool adjoint", gad.view(B, 2 * Ho, 2 * Wo, C), ar.grad.permute(0, 2, 3, 1))])


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_pack_and_head(B, H, W):
    ctx, ref, _ = _pair()
    s = ctx.stream()
    r = _reference(B, H, W)
    x, t = r["x"], r["t"]
    emb = ref.timestep_embed(t[:, None])
    want = th.zeros(B, H, W, 32)
    want[..., :3] = x.permute(0, 2, 3, 1)
    want[..., 3:19] = emb[:, None, None, :]
    packed = th.full((B * H * W, 32), 7.0, device=DEV)
    xd, td, wd = x.to(DEV), t.to(DEV), ref.timestep_embed.weight.detach().reshape(-1).to(DEV)
    ctx.check(ctx.lib.cgd_op_secondary_pack(ctx.h, xd.data_ptr(), td.data_ptr(), wd.data_ptr(), packed.data_ptr(), B, H, W, s))
    out = [rec("pack", packed.cpu().view(B, H, W, 32)[..., :19], want[..., :19])]
    assert bool((packed[:, 19:] == 0).all()), "the padded channels are exact zeros"
    v = th.randn(B, 3, H, W, generator=g(330))
    fac = 0.3
    al, sg = th.cos(t * math.pi / 2)[:, None, None, None], th.sin(t * math.pi / 2)[:, None, None, None]
    pred_ref = x * al - v * sg
    pred, xin = th.empty(B, 3, H, W, device=DEV), th.empty(B, 3, H, W, device=DEV)
    vd = v.to(DEV)
    ctx.check(ctx.lib.cgd_secondary_head(ctx.h, vd.data_ptr(), xd.data_ptr(), td.data_ptr(), fac, pred.data_ptr(), xin.data_ptr(), B, H, W, s))
    out += [rec("head pred", pred, pred_ref), rec("head x_in", xin, pred_ref * fac + x * (1 - fac))]
    _assert_ok(out)


@pytest.mark.parametrize("B,H,W,sat", [(1, 32, 32, 0.0), (2, 64, 96, 3.0)])
def test_combine_against_autograd(B, H, W, sat):
    from oracle import guidance as og
    ctx = _pair()[0]
    s = ctx.stream()
    fac, alpha, sigma = 0.6, 0.8, 0.6
    tvs, rs = 40.0, 30.0
    x = th.randn(B, 3, H, W, generator=g(340)).requires_grad_()
    v = th.randn(B, 3, H, W, generator=g(341)).requires_grad_()
    gin = th.randn(B, 3, H, W, generator=g(342)) * 1e-2
    pred = x * alpha - v * sigma
    x_in = pred * fac + x * (1 - fac)
    tv_l, rng_l = og.tv_loss(x_in).sum() * tvs, og.range_loss(pred).sum() * rs
    sat_l = th.abs(x_in - x_in.clamp(min=-1, max=1)).mean().sum() * sat
    loss = (x_in * gin).sum() + tv_l + rng_l + sat_l
    # the direct part is dL/dx with v held fixed; the seed is dL/dv
    dx_ref, dv_ref = th.autograd.grad(loss, [x, v])
    nblk = ctx.lib.cgd_guidance_part_blocks(B, H, W)
    gdir, seed, part = th.empty(B, 3, H, W, device=DEV), th.empty(B, 3, H, W, device=DEV), th.empty(nblk, 3, device=DEV)
    gd, xd, pd = gin.to(DEV), x_in.detach().to(DEV), pred.detach().to(DEV)
    ctx.check(ctx.lib.cgd_secondary_combine(ctx.h, gd.data_ptr(), xd.data_ptr(), pd.data_ptr(), gdir.data_ptr(), seed.data_ptr(), part.data_ptr(),
                                            B, H, W, fac, alpha, sigma, tvs, rs, sat, s))
    sums = part.double().sum(0).cpu()
    out = [rec("combine direct part", gdir, dx_ref), rec("combine seed", seed, dv_ref),
           rec("combine tv loss", sums[0:1], tv_l.detach().double().view(1)), rec("combine range loss", sums[1:2], rng_l.detach().double().view(1))]
    if sat:
        out.append(rec("combine saturation loss", sums[2:3], sat_l.detach().double().view(1)))
    _assert_ok(out)


# ---- one guided step --------------------------------------------------------------------------------------------------------------
class _CountingUNet:
    """The UNet handle as ClipGuidance sees it, with a call counter on dgrad."""

    def __init__(self, unet):
        self.unet, self.dgrad_calls = unet, 0

    def dgrad(self, *a, **k):
        self.dgrad_calls += 1
        return self.unet.dgrad(*a, **k)

    def __getattr__(self, name):
        return getattr(self.unet, name)


@functools.lru_cache(maxsize=None)
def _step_nets():
    from cgd_amd import nets, synthetic
    ctx = _pair()[0]
    ref_vit, dev_vit = pc.build_vit_pair(ctx, "ViT-B/32")
    unet = nets.UNet(ctx, **pc.UNET_CASES["mini"])
    unet.load_state_dict(synthetic.synthetic_state_dict(unet, seed=1234, device=DEV))
    return ref_vit, dev_vit, unet


@pytest.mark.parametrize("variant", ["plain", "sat+magnitude+two towers"])
def test_guided_step_matches_the_reference_and_skips_the_unet_backward(variant):
    """One guided step at 64x64, synthetic ViT-B/32 (+ a second small tower), synthetic UNet, cutn 4, taped coordinates: g and the logged
    scalars against secondary_ref.guided_step; unet.dgrad is never called."""
    from cgd_amd import diffusion, guidance, nets
    from oracle import clip_vit as ocv
    from oracle import guidance as og
    from tests import step_checks
    ctx, ref, dev = _pair()
    ref_vit, dev_vit, unet = _step_nets()
    full = variant != "plain"
    B, H, W, cutn = 1, 64, 64, 4
    tables = diffusion.create_gaussian_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="50")
    i = 12
    gen = g(350)
    x = th.randn(B, 3, H, W, generator=gen) * 0.8
    coords = og.generate_coords(H, W, cutn, 224, 1.0, generator=gen)
    targets = [th.randn(1, 512, generator=g(351))]
    o_models, o_cutters, towers = [ref_vit], [og.MakeCutouts(224, cutn)], [dev_vit]
    if full:
        cfg2 = (32, 8, 64, 1, 1, 48)
        ref2 = ocv.ClipImageModel.__new__(ocv.ClipImageModel)
        th.nn.Module.__init__(ref2)
        ref2.visual = ocv.VisionTransformer(*cfg2)
        ocv.synthetic_init_(ref2, seed=999).eval()
        for p in ref2.parameters():
            p.requires_grad_(False)
        dev2 = nets.ClipImageTower(ctx, config=cfg2)
        dev2.load_clip_state_dict(pc.device_sd(ref2))
        o_models.append(ref2); o_cutters.append(og.MakeCutouts(32, cutn)); towers.append(dev2)
        targets.append(th.randn(1, 48, generator=g(352)))
    cgs, tvs, rs = step_checks.default_scales(H, W)
    sat = 2.0 if full else 0.0
    w = th.tensor([1.0])
    g_ref, st = secondary_ref.guided_step(ref, x, tables, i, clip_model=o_models, make_cutouts=o_cutters, target_embeds=targets, weights=w,
                                          num_cutouts=cutn, clip_guidance_scale=cgs, tv_scale=tvs, range_scale=rs, sat_scale=sat,
                                          use_magnitude=full, coords_tape=[coords])
    counting = _CountingUNet(unet)
    sampler = type("D", (), {"tables": tables, "num_timesteps": tables.num_timesteps, "step_coef": lambda self, a, b=None: tables.step_coef(a, b)})()
    cond = guidance.ClipGuidance(ctx, counting, towers, sampler, [t.to(DEV) for t in targets], w, cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                                 range_scale=rs, sat_scale=sat, use_magnitude=full, secondary=dev)
    cond.current_timestep = i
    cond.coords_tape = [coords]
    calls0 = dev.dgrad_calls
    xd = x.to(DEV)
    coef = tables.step_coef(i, i)
    junk = th.full_like(xd, float("nan"))  # the UNet's pred_xstart / blend must not enter the guidance losses
    g_dev = cond.native(xd, junk, junk, coef)
    th.cuda.synchronize()
    assert counting.dgrad_calls == 0, "the UNet backward pass must not run on the secondary path"
    assert dev.dgrad_calls == calls0 + 1
    log_d, log_r = cond.log(), st["log"]
    out = [rec(f"step[{variant}] pred", cond._buf["sec_pred"], st["pred"]), rec(f"step[{variant}] x_in", cond._buf["sec_xin"], st["x_in"]),
           rec(f"step[{variant}] g_clip_in", cond._buf["gclip"], st["legs"]["g_clip_in"]),
           rec_flips(f"step[{variant}] g (device masks)", g_dev, st["legs"]["g_raw"])]
    keys = ["CLIP Loss", "Range Loss", "TV Loss", "Total Loss"] + (["Saturation Loss", "Magnitude"] if full else [])
    for k in keys:
        out.append(rec(f"step[{variant}] log {k}", th.tensor([log_d[k]]), th.tensor([log_r[k]]), allow_small=True))
    # with the reference's masks the whole gradient is graded at the literal tolerance
    with secondary_ref.CaptureRelu(ref) as cap:
        with th.no_grad():
            ref(x, th.full((B,), secondary_ref.model_time(*[float(tbl[i]) for tbl in (tables.sqrt_alphas_cumprod, tables.sqrt_one_minus_alphas_cumprod)]),
                           dtype=th.float32))
    dev.debug_replay([pc._nhwc_rows(a).to(DEV) for a in cap.acts])
    try:
        cond.coords_tape, cond.calls = [coords], 0
        g_rep = cond.native(xd, junk, junk, coef)
        th.cuda.synchronize()
    finally:
        dev.debug_replay(None)
    scale = pc.unit_seed(st["legs"]["g_raw"])
    out.append(rec(f"step[{variant}] g (reference masks)", g_rep * scale, st["legs"]["g_raw"] * scale))
    if full:
        out.append(rec(f"step[{variant}] clamped g", (g_rep * cond.scalars[7]) * scale, g_ref * scale))
    _assert_ok(out)
