"""VGG Gram-matrix style loss on the GPU against the fp64 reference of tests/style_ref.py: the Gram contraction (cgd_op_gram), the loss head
(cgd_lpips_set_style / cgd_lpips_style_loss_grad) alone and together with the LPIPS term, one guided step and the drop-in generator.
Records are parity_checks.rec's, at the project's literal |a - b| <= 1e-4 + 1e-3 |ref|; gradients are brought to unit peak with unit_seed."""
import ctypes as C
import functools
import os

import pytest
import torch as th

from tests import parity_checks as pc
from tests import step_checks as sc
from tests import style_ref
from tests.parity_checks import DEV, _CaptureRelu, _ctx, _nhwc_rows, rec, unit_seed

pytestmark = pytest.mark.gpu


def _assert_all(recs, allowed=("strict",)):
    for r in recs:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']} [{r['criterion']}]: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e}")
    bad = [r for r in recs if not r["ok"]]
    assert not bad, "; ".join(f"{r['name']} [{r['criterion']}]: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e}"
                              + (" VACUOUS" if r.get("vacuous") else "") for r in bad)
    assert all(r["criterion"] in allowed for r in recs), [r["name"] for r in recs if r["criterion"] not in allowed]


# ---- the contraction ---------------------------------------------------------------------------------------------------------------------
# N below one slab (a slab holds 16384 / C rows), N no multiple of a slab, several slabs, every C (and with it every tile count); B = 2 with
# different samples: a slab that crossed the sample boundary would mix them
GRAM_CASES = [(1, 1, 64, 0), (2, 16, 512, 0), (1, 48, 512, 0), (2, 192, 256, 0), (1, 4096, 64, 0), (2, 3072, 128, 0), (2, 192, 256, 64)]


def _gram(ctx, a, B, N, Cc, lda, scale):
    out = th.full((B, Cc, Cc), float("nan"), device=DEV)
    ctx.check(ctx.lib.cgd_op_gram(ctx.h, a.data_ptr(), lda, B, N, Cc, scale, out.data_ptr(), ctx.stream()))
    th.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", [0, 1])
def test_gram_contraction_against_fp64(precision):
    ctx = _ctx(precision)
    recs = []
    for (B, N, Cc, pad) in GRAM_CASES:
        lda = Cc + pad
        rows = th.relu(th.randn(B * N, lda, generator=pc.g(60 + Cc + N)))
        a = rows[:, :Cc]
        dev_rows = rows.to(DEV)
        if pad:
            dev_rows[:, Cc:] = float("nan")  # the columns beyond C are never read
        scale = 1.0 / N  # outputs O(1)
        ref = th.einsum("bni,bnj->bij", a.double().view(B, N, Cc), a.double().view(B, N, Cc)) * scale
        got = _gram(ctx, dev_rows, B, N, Cc, lda, scale)
        recs.append(rec(f"gram[p{precision}] B{B} N{N} C{Cc} lda{lda}", got, ref.float()))
        again = _gram(ctx, dev_rows, B, N, Cc, lda, scale)
        assert th.equal(got, again), f"gram B{B} N{N} C{Cc}: two calls differ"
        assert th.equal(got, got.transpose(1, 2)), f"gram B{B} N{N} C{Cc}: not exactly symmetric"
    _assert_all(recs)


def test_gram_refuses_what_it_cannot_run():
    ctx = _ctx(1)
    a = th.zeros(64, 96, device=DEV)
    out = th.zeros(1, 96, 96, device=DEV)
    for (lda, Cc, N) in [(96, 96, 64), (62, 64, 64), (66, 64, 62), (64, 64, 0)]:
        assert ctx.lib.cgd_op_gram(ctx.h, a.data_ptr(), lda, 1, N, Cc, 1.0, out.data_ptr(), ctx.stream()) != 0


# ---- the loss head -----------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(2, 64, 64, 48, 80), (1, 96, 128, 64, 64)]


@functools.lru_cache(maxsize=None)
def _head_case(B, H, W, Hs, Ws, weights=style_ref.DEFAULT_WEIGHTS):
    """Inputs, the fp64 reference (loss, gradient) and the oracle's activations of one shape: computed once, shared, never modified."""
    orc = pc.oracle_lpips()
    style = th.rand(1, 3, Hs, Ws, generator=pc.g(80)) * 2 - 1
    x = th.tanh(th.randn(B, 3, H, W, generator=pc.g(81)))
    with _CaptureRelu() as cap:
        loss, grad, rel = style_ref.style_loss_and_grad(orc, x.double(), style.double(), weights)
    acts = [a for a in cap.acts[13:26]]  # calls 0..12 are the style image's trunk pass, 13..25 the pass over x
    return dict(orc=orc, style=style, x=x, loss=loss, grad=grad, rel=rel, acts=acts)


def _device_net(ctx, orc):
    from cgd_amd import nets
    return nets.LpipsVGG(ctx).load_state_dict(pc.lpips_sd(orc))


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_style_loss_and_gradient(shape):
    B, H, W, Hs, Ws = shape
    case = _head_case(*shape)
    # the loss is no difference of near-equal numbers: |G - G_s|_F / |G_s|_F of the reference at every tap
    print("relative Gram distances per tap:", ["%.3f" % r for r in case["rel"]])
    assert min(case["rel"]) >= 0.1, case["rel"]
    ctx = _ctx(1)
    net = _device_net(ctx, case["orc"])
    net.set_style(case["style"].to(DEV))
    gs = unit_seed(case["grad"])
    xd = case["x"].to(DEV)
    tag = f"style B{B} {H}x{W} style {Hs}x{Ws}"
    recs = []
    # the device's own ReLU masks
    loss, _, gx = net.style_loss_grad(xd, style_scale=gs)
    th.cuda.synchronize()
    recs.append(rec(f"{tag} loss", loss, case["loss"].float()))
    recs.append(rec(f"{tag} grad", gx, (case["grad"] * gs).float()))
    # the oracle's masks and arg-max (mask replay): the strict check of the backward chain
    acts = [_nhwc_rows(a) for a in case["acts"]]
    table = (C.c_void_p * 13)(*[a.data_ptr() for a in acts])
    ctx.check(ctx.lib.cgd_lpips_debug_replay(net.h, table))
    try:
        loss_r, _, gx_r = net.style_loss_grad(xd, style_scale=gs)
        th.cuda.synchronize()
    finally:
        ctx.check(ctx.lib.cgd_lpips_debug_replay(net.h, None))
    recs.append(rec(f"{tag} loss (oracle masks)", loss_r, case["loss"].float()))
    recs.append(rec(f"{tag} grad (oracle masks)", gx_r, (case["grad"] * gs).float()))
    base = th.randn(B, 3, H, W, generator=pc.g(82))
    _, _, gacc = net.style_loss_grad(xd, style_scale=gs, g=base.to(DEV).clone(), accumulate=True)
    recs.append(rec(f"{tag} grad accumulate", gacc, (case["grad"] * gs).float() + base))
    _assert_all(recs)


def test_style_tap_weights_and_skipped_taps():
    """lambda = (0, 0, 1, 0, 2): the weights are applied, and a tap with weight 0 launches nothing (fewer launches than the default weights
    although relu5_3 joins)."""
    shape = HEAD_SHAPES[0]
    weights = (0.0, 0.0, 1.0, 0.0, 2.0)
    case = _head_case(*shape, weights=weights)
    ctx = _ctx(1)
    net = _device_net(ctx, case["orc"])
    xd = case["x"].to(DEV)
    gs = unit_seed(case["grad"])
    net.set_style(case["style"].to(DEV), weights)
    n0 = _launches(ctx)
    loss, _, gx = net.style_loss_grad(xd, style_scale=gs)
    n_two = _launches(ctx) - n0
    th.cuda.synchronize()
    _assert_all([rec("style lambda (0,0,1,0,2) loss", loss, case["loss"].float()),
                 rec("style lambda (0,0,1,0,2) grad", gx, (case["grad"] * gs).float())])
    net.set_style(case["style"].to(DEV), (1, 1, 1, 1, 1))
    n0 = _launches(ctx)
    net.style_loss_grad(xd, style_scale=gs)
    n_five = _launches(ctx) - n0
    # per active tap: the slab kernel, the finish and the backward GEMM
    assert n_five - n_two >= 3 * 3, (n_two, n_five)


def _launches(ctx):
    out = (C.c_uint64 * 2)()
    ctx.check(ctx.lib.cgd_launch_counts(out))
    return int(out[0])


def test_style_call_needs_a_style_and_refuses_aliasing():
    ctx = _ctx(1)
    net = _device_net(ctx, pc.oracle_lpips())
    x = th.zeros(1, 3, 32, 32, device=DEV)
    loss = th.zeros(1, device=DEV)
    g = th.zeros_like(x)
    call = lambda gp: ctx.lib.cgd_lpips_style_loss_grad(net.h, x.data_ptr(), 1, 32, 32, 0.0, 1.0, None, loss.data_ptr(), gp, 0, ctx.stream())  # noqa: E731
    assert call(g.data_ptr()) != 0
    with pytest.raises(RuntimeError, match="style"):
        ctx.check(call(g.data_ptr()))
    net.set_style(th.zeros(1, 3, 32, 48, device=DEV) + 0.1)
    assert call(x.data_ptr()) != 0  # g aliases x
    assert call(g.data_ptr()) == 0
    # with lpips_loss, a reference is needed
    lp = th.zeros(1, device=DEV)
    assert ctx.lib.cgd_lpips_style_loss_grad(net.h, x.data_ptr(), 1, 32, 32, 1.0, 1.0, lp.data_ptr(), loss.data_ptr(), g.data_ptr(), 0, ctx.stream()) != 0
    th.cuda.synchronize()


# ---- both terms in one call --------------------------------------------------------------------------------------------------------------
def test_combined_call_shares_the_trunk():
    B, H, W, Hs, Ws = HEAD_SHAPES[0]
    case = _head_case(B, H, W, Hs, Ws)
    orc = case["orc"]
    ctx = _ctx(1)
    net = _device_net(ctx, orc)
    xd = case["x"].to(DEV)
    ref_img = th.rand(B, 3, H, W, generator=pc.g(83)) * 2 - 1
    # fp64 reference of the LPIPS term
    xr = case["x"].double().requires_grad_()
    lp_ref = orc(xr, ref_img.double()).flatten()
    lp_ref.sum().backward()
    g_lp, g_st = xr.grad, case["grad"]
    s_lp, s_st = unit_seed(g_lp), unit_seed(g_st)  # both legs at unit peak, so that neither drowns in the other
    net.set_reference(ref_img.to(DEV))
    # before any style is set
    n0 = _launches(ctx)
    lp_before, g_before = net.loss_grad(xd, grad_scale=s_lp)
    n_lpips = _launches(ctx) - n0
    lp_before, g_before = lp_before.clone(), g_before.clone()
    net.set_style(case["style"].to(DEV))
    n0 = _launches(ctx)
    st_alone, _, g_style = net.style_loss_grad(xd, style_scale=s_st)
    n_style = _launches(ctx) - n0
    st_alone, g_style = st_alone.clone(), g_style.clone()
    n0 = _launches(ctx)
    st_both, lp_both, g_both = net.style_loss_grad(xd, style_scale=s_st, lpips_scale=s_lp)
    n_both = _launches(ctx) - n0
    th.cuda.synchronize()
    print(f"launches: LPIPS alone {n_lpips}, style alone {n_style}, combined {n_both}")
    recs = [rec("combined: lpips loss", lp_both, lp_ref.detach().float()),
            rec("combined: style loss", st_both, case["loss"].float()),
            rec("combined: gradient == sum of the two references", g_both, (g_lp * s_lp + g_st * s_st).float())]
    _assert_all(recs)
    assert th.equal(lp_both, lp_before), "the LPIPS loss of the combined call differs from loss_grad's"
    assert th.equal(st_both, st_alone), "the style loss of the combined call differs from the style-only call's"
    # the combined gradient against the sum of the two separate device gradients (one trunk backward of the summed cotangents)
    _assert_all([rec("combined: gradient == separate device gradients, summed", g_both, g_before + g_style)])
    # the 13 trunk convolutions forward and the 13 backward run once
    assert n_both <= n_lpips + n_style - 26, (n_lpips, n_style, n_both)
    # and loss_grad is untouched by all of it, bit for bit
    lp_after, g_after = net.loss_grad(xd, grad_scale=s_lp)
    th.cuda.synchronize()
    assert th.equal(lp_after, lp_before) and th.equal(g_after, g_before)


# ---- one guided step -----------------------------------------------------------------------------------------------------------------------
STYLE_SCALE = 10.0  # the style leg of g then has about the peak of the LPIPS leg at init_scale 1000 (synthetic weights, 32 x 32)


class StyleScenario(sc.Scenario):
    """step_checks.Scenario with the style term on both sides.  The oracle's cond_fn adds `lpips_model(x_in, init).sum() * init_scale`: its LPIPS
    module is wrapped (style_ref.LpipsPlusStyle) so that this expression is init_scale * lpips + STYLE_SCALE * L_style — with `lpips_on` False
    only the style term, which the oracle then logs under 'Init VGG Loss'.  The device gets the real scales."""

    def __init__(self, lpips_on, **kw):
        super().__init__("mini", init_scale=1000.0, **kw)
        self.lpips_on = lpips_on
        self.style_cpu = th.rand(1, 3, 48, 32, generator=pc.g(84)) * 2 - 1
        self.o_plain = self.o_lp
        self.o_lp = style_ref.LpipsPlusStyle(self.o_plain, self.style_cpu, lpips_weight=1.0 if lpips_on else 0.0,
                                             style_weight=STYLE_SCALE / self.init_scale)

    def _run_device(self, ctx, dev_unet, dev_clip, dev_clip2, d_lp, smp):
        from cgd_amd import guidance as dg
        B, H, W = self.B, self.H, self.W
        cgs, tvs, rs = self.scales
        guid = dg.ClipGuidance(ctx, dev_unet, dev_clip, smp, self.targets.to(DEV), self.w, self.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                               range_scale=rs, lpips=d_lp, init_tensor=self.init_cpu.to(DEV) if self.lpips_on else None,
                               init_scale=self.init_scale if self.lpips_on else 0.0, style_tensor=self.style_cpu.to(DEV),
                               style_scale=STYLE_SCALE)
        guid.coords_tape = self.tape["coords"]
        smp.tape = self.tape
        dmkw = {"y": th.zeros(B, dtype=th.long, device=DEV)} if self.kw.get("num_classes") else {}
        d_gen = smp.p_sample_loop_progressive(dev_unet, (B, 3, H, W), clip_denoised=False, cond_fn=guid, model_kwargs=dmkw, device=DEV,
                                              skip_timesteps=self.skip, init_image=self.x0_star.expand(B, -1, -1, -1).to(DEV),
                                              randomize_class=bool(dmkw), cond_fn_with_grad=True)
        guid.current_timestep = self.counter0
        import itertools
        for out in itertools.islice(d_gen, self.steps):
            th.cuda.synchronize()
            bufs = guid._buf
            legs = {"g": bufs["g"].clone(), "g_clip_in": bufs["gclip"].clone(), "g_direct": bufs["gdir"].clone(),
                    "seed_eps": bufs["seed6"][:, :3].clone(), "seed_var": bufs["seed6"][:, 3:].clone(), "g_unet": bufs["gunet"].clone()}
            lg = guid.log()
            assert "Style Loss" in lg and ("Init VGG Loss" in lg) == self.lpips_on, sorted(lg)
            self.logs.append(dict(lg))
            merged = dict(lg)  # the oracle logs both terms under the one key it has
            merged["Init VGG Loss"] = lg["Style Loss"] + lg.get("Init VGG Loss", 0.0)
            yield out, sc._FrozenLog(merged), legs
            guid.current_timestep -= 1


@pytest.mark.parametrize("lpips_on", [True, False], ids=["with-lpips", "style-only"])
def test_guided_step_with_style_term(lpips_on):
    s = StyleScenario(lpips_on, steps=2, B=2)
    s.logs = []
    # the records test_gpu_step.py::test_init_image_lpips_term grades, by the same criteria
    _assert_all(sc.compare(s, 1, s.run_oracle(), s.run_device(1)), allowed=("strict", "relu-flips"))
    assert len(s.logs) == 2 and all(lg["Style Loss"] > 0 for lg in s.logs)


# ---- the drop-in generator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prompt", [True, False], ids=["with-prompt", "style-only"])
def test_dropin_generator_with_style_image(with_prompt, tmp_path, monkeypatch, capsys):
    import numpy as np
    from PIL import Image
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(1)
    Image.fromarray(rng.integers(0, 255, (80, 96, 3), dtype=np.uint8)).save(tmp_path / "style.png")
    from cgd.cgd import clip_guided_diffusion
    gen = clip_guided_diffusion(prompts=["Loose seal."] if with_prompt else [], image_prompts=[f"style={tmp_path / 'style.png'}:50"], image_size=64,
                                batch_size=1, num_cutouts=2, timestep_respacing="5", noise_schedule="cosine", prefix_path=str(tmp_path / "out"),
                                checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=True, device="cuda")
    items = list(gen)
    assert [b for b, _ in items] == [0] * 5 and all(os.path.isfile(p) for _, p in items)
    frame = np.asarray(Image.open(items[-1][1]))
    assert frame.shape == (64, 64, 3) and frame.dtype == np.uint8
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Style Loss" in ln]
    assert len(lines) == 5
