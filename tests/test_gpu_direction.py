"""The directional CLIP loss on the GPU.  Op level: cgd_directional_loss (csrc/direction.hip) through the C ABI against the float64 reference
(tests/direction_ref.py) at the literal |a - b| <= 1e-4 + 1e-3 |ref|; on the stressed value set each row's gradient is first multiplied by
|e_r| n_r (it is homogeneous of degree -1 in both) and the tensor brought to unit peak.  Step level: ClipGuidance.native with direction prompts
against the same step with the CLIP leg restated in torch ops and autograd (_clip_leg_torch), and one short run of the drop-in generator."""
import ctypes as C
import functools
import math
import os

import pytest
import torch as th

from tests import direction_ref as R
from tests import parity_checks as pc
from tests.parity_checks import DEV, g, rec

pytestmark = pytest.mark.gpu

PAD = 5  # the outputs are allocated this many floats too long


@functools.lru_cache(maxsize=None)
def _ctx():
    return pc._ctx(1)


def _assert_ok(records):
    for r in records:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e} "
              f"[{r['criterion']}] strict={r['ok_strict']}")
    bad = [r for r in records if not r["ok"]]
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _case(shape, kind="ordinary", seed=0):
    """inputs and the float64 reference of a case, computed once and never modified"""
    e, s, d, w = R.make_case(shape, kind, seed)
    loss, grad, n = R.loss_and_grad(e, s, d, w, shape[0], shape[1])
    return dict(e=e, s=s, d=d, w=w, loss=loss, grad=grad, n=n)


def run(e, s, d, w, shape, accumulate=0, prefill=float("nan"), scale=R.SCALE, check=True):
    """-> (d_emb (N, D), loss_part (N,), the two padding tails, return code)"""
    ctx = _ctx()
    cutn, B, Bs, P, D = shape
    N = cutn * B
    ed, sd, dd, wd = (t.float().contiguous().to(DEV) for t in (e, s, d, w))
    demb = th.full((N * D + PAD,), float("nan"), device=DEV)
    if isinstance(prefill, th.Tensor):
        demb[:N * D] = prefill.to(DEV).reshape(-1)
    else:
        demb[:N * D] = prefill
    part = th.full((N + PAD,), float("nan"), device=DEV)
    rc = ctx.lib.cgd_directional_loss(ctx.h, ed.data_ptr(), sd.data_ptr(), dd.data_ptr(), wd.data_ptr(), demb.data_ptr(), part.data_ptr(),
                                      cutn, B, Bs, P, D, scale, accumulate, ctx.stream())
    if check:
        ctx.check(rc)
    th.cuda.synchronize()
    return demb[:N * D].view(N, D).cpu(), part[:N].cpu(), (demb[N * D:].cpu(), part[N:].cpu()), rc


def grade(tag, got_g, got_l, c, scaled):
    ok_l, use_l = R.within(got_l.double().sum().view(1), c["loss"].sum().view(1))
    if scaled:
        f = R.degree_scale(c["e"], c["n"])
        a, b = R.unit_peak(got_g.double() * f, c["grad"] * f)
    else:
        a, b = got_g.double(), c["grad"]
    ok_g, use_g = R.within(a, b)
    print(f"{tag}: loss sum {float(got_l.double().sum()):.6f} (ref {float(c['loss'].sum()):.6f}), use of the bound: loss {use_l:.4f}, "
          f"gradient {use_g:.4f} ({'scaled by |e| n, unit peak' if scaled else 'as it stands'}; peak |ref| {float(b.abs().max()):.3e})")
    assert float(b.abs().max()) >= 100 * 1e-4, "a reference this small would pass on atol alone"
    assert ok_l and ok_g, tag
    # every row's own partial loss too
    assert R.within(got_l, c["loss"])[0], tag


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ordinary_values_against_the_reference(shape):
    c = _case(shape)
    got_g, got_l, tails, _ = run(c["e"], c["s"], c["d"], c["w"], shape)
    grade(f"directional {shape} ordinary", got_g, got_l, c, scaled=False)
    assert all(bool(th.isnan(t).all()) and t.numel() == PAD for t in tails), "the padding behind the outputs was written"


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stressed_values_against_the_reference(shape, seed):
    c = _case(shape, "stressed", seed)
    got_g, got_l, tails, _ = run(c["e"], c["s"], c["d"], c["w"], shape)
    grade(f"directional {shape} stressed/{seed}", got_g, got_l, c, scaled=True)
    assert all(bool(th.isnan(t).all()) for t in tails)


def test_row_without_a_direction_has_the_full_loss_and_a_zero_gradient():
    shape = R.SHAPES[0]
    cutn, B = shape[:2]
    c = _case(shape)
    e = c["e"].clone()
    e[3] = 2 * R.source_rows(c["s"], cutn, B)[3]  # e^ == s^ bit for bit: delta is exactly zero
    loss, grad, n = R.loss_and_grad(e, c["s"], c["d"], c["w"], cutn, B)
    assert float(n[3]) <= 1e-6
    got_g, got_l, _, _ = run(e, c["s"], c["d"], c["w"], shape)
    want = R.SCALE / cutn * float(c["w"][3 % B].double().sum())
    assert abs(float(got_l[3]) - want) <= 1e-4 + 1e-3 * abs(want)
    assert not got_g[3].view(th.int32).any(), "gradient bits of the row must all be zero"
    assert R.within(got_g, grad)[0] and R.within(got_l, loss)[0]
    # accumulate leaves such a row as it is
    pre = th.randn(got_g.shape, generator=g(5))
    acc_g, _, _, _ = run(e, c["s"], c["d"], c["w"], shape, accumulate=1, prefill=pre)
    assert th.equal(acc_g[3], pre[3])


def test_zero_weight_column_is_skipped():
    shape = R.SHAPES[2]  # P = 3
    cutn, B = shape[:2]
    c = _case(shape)
    w = c["w"].clone()
    w[:, 1] = 0
    d = c["d"].clone()
    loss, grad, _ = R.loss_and_grad(c["e"], c["s"], d, w, cutn, B)
    got_g, got_l, _, _ = run(c["e"], c["s"], d, w, shape)
    assert R.within(got_g, grad)[0] and R.within(got_l, loss)[0]
    d[1] = float("nan")  # a skipped column is not read into the result
    nan_g, nan_l, _, _ = run(c["e"], c["s"], d, w, shape)
    assert th.equal(nan_g, got_g) and th.equal(nan_l, got_l)


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_accumulate_adds_onto_a_filled_gradient_and_runs_are_bit_identical(shape):
    c = _case(shape)
    a_g, a_l, _, _ = run(c["e"], c["s"], c["d"], c["w"], shape)
    b_g, b_l, _, _ = run(c["e"], c["s"], c["d"], c["w"], shape, prefill=7.0)  # accumulate 0 overwrites
    assert th.equal(a_g, b_g) and th.equal(a_l, b_l)
    pre = th.randn(a_g.shape, generator=g(6)) * float(a_g.abs().max())
    acc_g, acc_l, tails, _ = run(c["e"], c["s"], c["d"], c["w"], shape, accumulate=1, prefill=pre)
    assert th.equal(acc_g, pre + a_g) and th.equal(acc_l, a_l)  # one float addition per element
    assert all(bool(th.isnan(t).all()) for t in tails)


def test_shared_source_equals_the_repeated_source():
    shape = R.SHAPES[0]
    cutn, B, _, P, D = shape
    c = _case(shape)
    a = run(c["e"], c["s"], c["d"], c["w"], shape)
    b = run(c["e"], c["s"].repeat_interleave(B, dim=0), c["d"], c["w"], (cutn, B, B, P, D))
    assert th.equal(a[0], b[0]) and th.equal(a[1], b[1])


def test_refusals_write_nothing():
    ctx = _ctx()
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    for shape, msg in (((1, 1, 1, 1, 2049), b"embedding dim"), ((2, 3, 2, 1, 64), b"source batch")):
        cutn, B, Bs, P, D = shape
        e, s, d, w = th.randn(cutn * B, D), th.randn(cutn * Bs, D), th.nn.functional.normalize(th.randn(P, D), dim=1), th.ones(B, P)
        got_g, got_l, tails, rc = run(e, s, d, w, shape, check=False)
        assert rc == -2 and msg in ctx.lib.cgd_last_error(ctx.h)
        assert bool(th.isnan(got_g).all()) and bool(th.isnan(got_l).all()) and all(bool(th.isnan(t).all()) for t in tails)
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before


# ---- one guided step ------------------------------------------------------------------------------------------------------------------------
STEP_I, CUTN, HW = 12, 4, 64
TAPE = [(0, 0, 64), (5, 9, 40), (20, 3, 44), (29, 30, 34)]  # (ox, oy, size): the whole frame and three inner crops


@functools.lru_cache(maxsize=None)
def _step_setup():
    """mini UNet at 64 x 64 and a ViT-B/32 tower on seeded weights, a small second tower, x_t, the source image, targets and directions"""
    from cgd_amd import diffusion, nets, synthetic
    from tests import step_checks
    ctx = _ctx()
    _, vit = pc.build_vit_pair(ctx, "ViT-B/32")
    vit2 = nets.ClipImageTower(ctx, config=step_checks.MINI_VIT)
    vit2.load_state_dict(synthetic.synthetic_state_dict(vit2, seed=999))
    unet = nets.UNet(ctx, **pc.UNET_CASES["mini"])
    unet.load_state_dict(synthetic.synthetic_state_dict(unet, seed=1234, device=DEV))
    tables = diffusion.create_gaussian_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="50")
    gen = g(740)
    B = 2
    x = th.randn(B, 3, HW, HW, generator=gen) * 0.8
    source = th.tanh(th.randn(1, 3, HW, HW, generator=gen))
    dims = (vit.out_dim, vit2.out_dim)
    targets = [th.randn(1, D, generator=gen).to(DEV) for D in dims]
    dirs = [th.randn(1, D, generator=gen).to(DEV) for D in dims]
    return dict(ctx=ctx, towers=[vit, vit2], unet=unet, tables=tables, x=x, source=source.to(DEV), targets=targets, dirs=dirs)


def _guided(st, leg="native", towers=1, with_target=True, cutter=None, tape=None, calls=1, **kw):
    """`calls` ClipGuidance.native calls at step STEP_I on the same inputs -> (g, d loss / d x_in, log, launches of the last call) of the last one"""
    from cgd_amd import guidance
    from tests import step_checks
    ctx, tables, unet = st["ctx"], st["tables"], st["unet"]
    B = st["x"].shape[0]
    cgs, tvs, rs = step_checks.default_scales(HW, HW)
    sampler = type("D", (), {"tables": tables, "num_timesteps": tables.num_timesteps, "step_coef": lambda self, a, b=None: tables.step_coef(a, b)})()
    cond = guidance.ClipGuidance(ctx, unet, st["towers"][:towers], sampler, [t for t in st["targets"][:towers]] if with_target else None,
                                 th.tensor([0.6]) if with_target else None, CUTN, clip_guidance_scale=cgs, tv_scale=tvs, range_scale=rs,
                                 direction_embeds=st["dirs"][:towers], direction_weights=th.tensor([0.4] if with_target else [1.0]),
                                 direction_source=st["source"], make_cutouts=cutter, **kw)
    if leg == "torch":
        cond._clip_leg = cond._clip_leg_torch
    cond.current_timestep = STEP_I
    cond.coords_tape = [tape or TAPE] * calls
    coef = tables.step_coef(STEP_I, STEP_I)
    xd = st["x"].to(DEV)
    ts = th.full((B,), float(tables.model_timestep(STEP_I)), device=DEV)
    counts = (C.c_uint64 * 2)()
    for _ in range(calls):
        out6 = unet.forward(xd, ts, th.full((B,), 7, device=DEV))
        x0, mean, logvar, xin = (th.empty_like(xd) for _ in range(4))
        ctx.check(ctx.lib.cgd_pmv_blend(ctx.h, xd.data_ptr(), out6.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), xin.data_ptr(),
                                        B, HW, HW, coef, ctx.stream()))
        ctx.lib.cgd_launch_counts(counts)
        before = counts[0]
        g_dev = cond.native(xd, x0, xin, coef)
        ctx.lib.cgd_launch_counts(counts)
        th.cuda.synchronize()
    return g_dev.clone(), cond._buf["gclip"].clone(), cond.log(), counts[0] - before


def _compare(tag, native, torch_):
    (g_n, c_n, log_n, _), (g_t, c_t, log_t, _) = native, torch_
    out = []
    for name, a, b in (("g", g_n, g_t), ("g_clip_in", c_n, c_t)):
        sd = pc.unit_seed(b)
        out.append(rec(f"{tag} {name} (unit peak)", a * sd, b * sd))
        out.append(rec(f"{tag} {name}", a, b, allow_small=True))
    for key in ("CLIP Loss", "Direction Loss", "TV Loss", "Range Loss", "Total Loss"):
        out.append(rec(f"{tag} {key}", th.tensor([log_n[key]]), th.tensor([log_t[key]]), allow_small=True))
    assert math.isfinite(log_n["Direction Loss"]) and log_n["Direction Loss"] != 0
    _assert_ok(out)


@pytest.mark.parametrize("case", ["target+direction", "direction only", "two towers"])
def test_guided_step_matches_the_torch_leg(case):
    st = _step_setup()
    kw = dict(towers=2 if case == "two towers" else 1, with_target=case != "direction only")
    native, torch_ = _guided(st, "native", **kw), _guided(st, "torch", **kw)
    _compare(f"direction step[{case}]", native, torch_)
    log = native[2]
    if case == "direction only":
        assert abs(log["Direction Loss"] - log["CLIP Loss"]) <= 1e-5 * abs(log["CLIP Loss"])
    else:
        assert list(log) == ["CLIP Loss", "Range Loss", "TV Loss", "Direction Loss", "Total Loss", "Grad"]


def test_guided_step_with_the_resized_cutter_matches_the_torch_leg():
    from cgd_amd import guidance
    st = _step_setup()
    mk = guidance.MakeCutoutsResized(224, overview=1, inner=3, ctx=st["ctx"])
    # (ox, oy, w, h, flags): the overview, then a gray, a mirrored and a non-square inner cut; the flags apply to both images
    recs = [(0, 0, HW, HW, 0), (3, 5, 40, 40, guidance.RESIZE_GRAY), (20, 4, 36, 36, guidance.RESIZE_FLIP), (10, 20, 44, 30, 0)]
    native = _guided(st, "native", cutter=mk, tape=recs)
    torch_ = _guided(st, "torch", cutter=mk, tape=recs)
    _compare("direction step[cuts=1:3]", native, torch_)


def test_cached_cutouts_reuse_the_source_embeddings_bit_for_bit():
    st = _step_setup()
    g_u, c_u, log_u, n_u = _guided(st)
    g_c, c_c, log_c, n_c = _guided(st, calls=2, cached_cutouts=True)
    assert th.equal(g_u, g_c) and th.equal(c_u, c_c) and log_u == log_c
    print(f"launches of a step: {n_u} with the source forward, {n_c} on kept source embeddings")
    assert 0 < n_c < n_u


def test_without_direction_prompts_the_step_is_unchanged():
    """the same guided step through ClipGuidance with and without the (unset) keywords: same bits, same buffers, same launch count"""
    from cgd_amd import guidance
    from tests import step_checks
    st = _step_setup()
    ctx, tables, unet = st["ctx"], st["tables"], st["unet"]
    cgs, tvs, rs = step_checks.default_scales(HW, HW)
    sampler = type("D", (), {"tables": tables, "num_timesteps": tables.num_timesteps})()
    coef = tables.step_coef(STEP_I, STEP_I)
    xd = st["x"].to(DEV)
    out = []
    for kw in ({}, dict(direction_embeds=None, direction_weights=None, direction_source=None)):
        cond = guidance.ClipGuidance(ctx, unet, st["towers"][:1], sampler, st["targets"][:1], th.tensor([1.0]), CUTN, clip_guidance_scale=cgs,
                                     tv_scale=tvs, range_scale=rs, **kw)
        cond.current_timestep, cond.coords_tape = STEP_I, [TAPE]
        out6 = unet.forward(xd, th.full((2,), float(tables.model_timestep(STEP_I)), device=DEV), th.full((2,), 7, device=DEV))
        x0, mean, logvar, xin = (th.empty_like(xd) for _ in range(4))
        ctx.check(ctx.lib.cgd_pmv_blend(ctx.h, xd.data_ptr(), out6.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), xin.data_ptr(),
                                        2, HW, HW, coef, ctx.stream()))
        g_dev = cond.native(xd, x0, xin, coef)
        th.cuda.synchronize()
        out.append((g_dev.clone(), cond.log(), sorted(cond._buf)))
    assert th.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and out[0][2] == out[1][2]
    assert list(out[0][1]) == ["CLIP Loss", "Range Loss", "TV Loss", "Total Loss", "Grad"] and not any(k.startswith("src_") for k in out[0][2])


# ---- the drop-in generator ------------------------------------------------------------------------------------------------------------------
def test_dropin_generator_with_a_direction_prompt(tmp_path, monkeypatch, capsys):
    import numpy as np
    from PIL import Image
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (80, 96, 3), dtype=np.uint8)).save(tmp_path / "init.png")
    from cgd.cgd import clip_guided_diffusion
    items = list(clip_guided_diffusion(prompts=["a photo of a cat=>a photo of a dog:1.5", "a garden:0.5"], image_size=64, batch_size=1,
                                       num_cutouts=2, timestep_respacing="ddim6", skip_timesteps=3, prefix_path=str(tmp_path / "out"),
                                       checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=True, device="cuda",
                                       init_image=str(tmp_path / "init.png")))
    assert [b for b, _ in items] == [0, 0, 0] and all(os.path.isfile(p) for _, p in items)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Direction Loss" in ln]
    assert len(lines) == 3
    for ln in lines:
        vals = dict(kv.split(": ") for kv in ln.split("\t"))
        assert math.isfinite(float(vals["Direction Loss"])) and math.isfinite(float(vals["CLIP Loss"])) and float(vals["Direction Loss"]) != 0
