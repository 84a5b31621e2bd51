"""Aesthetic-predictor guidance on the GPU.  Op level: cgd_aesthetic_loss (csrc/aesthetic.hip) through the C ABI against the float64 reference
(tests/aesthetic_ref.py) at the literal |a - b| <= 1e-4 + 1e-3 |ref|; on the stressed value set each row's gradient is first multiplied by
|e_r| (it is homogeneous of degree -1) and the tensor brought to unit peak.  Step level: ClipGuidance.native with aesthetic heads against the
same step with the CLIP leg restated in torch ops and autograd (_clip_leg_torch), and two short runs of the drop-in generator."""
import ctypes as C
import functools
import math
import os

import pytest
import torch as th

from tests import aesthetic_ref as R
from tests import parity_checks as pc
from tests.parity_checks import DEV, g, rec

pytestmark = pytest.mark.gpu

PAD = 5  # the outputs are allocated this many floats too long


def _sid(s):
    return "x".join(map(str, s))


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
    e, head = R.make_case(shape, kind, seed)
    loss, grad, score = R.loss_grad_score(e, head, shape[0], shape[1])
    return dict(e=e, head=head, loss=loss, grad=grad, score=score)


def run(e, head, shape, accumulate=0, prefill=float("nan"), scale=R.SCALE, check=True, with_score=True, null_head=False):
    """-> (d_emb (N, D), loss_part (N,), score (N,), the three padding tails, return code)"""
    ctx = _ctx()
    cutn, B, D = shape
    N = max(cutn, 1) * B  # (a refused cutn = 0 still gets outputs to look at)
    ed, hd = e.float().contiguous().to(DEV), head.float().contiguous().to(DEV)
    demb = th.full((N * D + PAD,), float("nan"), device=DEV)
    if isinstance(prefill, th.Tensor):
        demb[:N * D] = prefill.to(DEV).reshape(-1)
    else:
        demb[:N * D] = prefill
    part = th.full((N + PAD,), float("nan"), device=DEV)
    score = th.full((N + PAD,), float("nan"), device=DEV)
    rc = ctx.lib.cgd_aesthetic_loss(ctx.h, ed.data_ptr(), None if null_head else hd.data_ptr(), demb.data_ptr(), part.data_ptr(),
                                    score.data_ptr() if with_score else None, cutn, B, D, scale, accumulate, ctx.stream())
    if check:
        ctx.check(rc)
    th.cuda.synchronize()
    return demb[:N * D].view(N, D).cpu(), part[:N].cpu(), score[:N].cpu(), (demb[N * D:].cpu(), part[N:].cpu(), score[N:].cpu()), rc


def _untouched(tails):
    return all(bool(th.isnan(t).all()) and t.numel() == PAD for t in tails)


def grade(tag, got_g, got_l, got_s, c, shape, scaled):
    cutn, B, D = shape
    ok_l, use_l = R.within(got_l.double().sum().view(1), c["loss"].sum().view(1))
    ok_p, use_p = R.within(got_l, c["loss"])
    ok_s, use_s = R.within(got_s, c["score"])
    if scaled:
        a, b, peak = R.graded_gradient(got_g, c["grad"], c["e"], c["head"], cutn)
        if D == 1:  # the unit sphere in one dimension is two points: there is no gradient, and the reference says so
            assert peak == 0.0
        else:
            assert float(b.abs().max()) == 1.0 and peak >= 100 * 1e-4, "a reference this small would pass on atol alone"
    else:
        a, b = got_g.double(), c["grad"]
    ok_g, use_g = R.within(a, b)
    print(f"{tag}: loss sum {float(got_l.double().sum()):.6f} (ref {float(c['loss'].sum()):.6f}), use of the bound: loss sum {use_l:.4f}, "
          f"partials {use_p:.4f}, score {use_s:.4f}, gradient {use_g:.4f} ({'scaled by |e|, unit peak' if scaled else 'as it stands'}; "
          f"peak |ref| {float(c['grad'].abs().max()):.3e})")
    assert ok_l and ok_p and ok_s and ok_g, tag


# ---- the op ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_ordinary_values_against_the_reference(shape):
    c = _case(shape)
    got_g, got_l, got_s, tails, _ = run(c["e"], c["head"], shape)
    grade(f"aesthetic {shape} ordinary", got_g, got_l, got_s, c, shape, scaled=False)
    assert _untouched(tails), "the padding behind the outputs was written"


@pytest.mark.parametrize("seed", R.SEEDS["stressed"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=_sid)
def test_stressed_values_against_the_reference(shape, seed):
    c = _case(shape, "stressed", seed)
    got_g, got_l, got_s, tails, _ = run(c["e"], c["head"], shape)
    grade(f"aesthetic {shape} stressed/{seed}", got_g, got_l, got_s, c, shape, scaled=True)
    assert _untouched(tails), "the padding behind the outputs was written"


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[4]], ids=_sid)
def test_null_score_gives_the_same_bits(shape):
    c = _case(shape)
    a_g, a_l, _, _, _ = run(c["e"], c["head"], shape)
    b_g, b_l, b_s, tails, _ = run(c["e"], c["head"], shape, with_score=False)
    assert th.equal(a_g, b_g) and th.equal(a_l, b_l)
    assert bool(th.isnan(b_s).all()) and _untouched(tails)  # (the buffer that was not handed over)


def test_zero_row_has_the_bias_term_and_no_gradient():
    shape = R.SHAPES[0]
    cutn, B, D = shape
    c = _case(shape)
    e = c["e"].clone()
    e[3] = 0
    loss, grad, score = R.loss_grad_score(e, c["head"], cutn, B)
    got_g, got_l, got_s, _, _ = run(e, c["head"], shape)
    beta = float(c["head"][-1])
    want = th.tensor(-R.SCALE / cutn, dtype=th.float32) * c["head"][-1]  # -c beta, one float32 product: a . e^ is exactly zero
    assert float(got_s[3]) == beta and float(got_l[3]) == float(want)
    assert not got_g[3].view(th.int32).any(), "gradient bits of the row must all be zero"
    assert R.within(got_g, grad)[0] and R.within(got_l, loss)[0] and R.within(got_s, score)[0]
    # accumulate leaves such a row as it is
    pre = th.randn(got_g.shape, generator=g(5))
    acc_g, acc_l, _, _, _ = run(e, c["head"], shape, accumulate=1, prefill=pre)
    assert th.equal(acc_g[3], pre[3]) and th.equal(acc_l, got_l)
    assert th.equal(acc_g[:3], pre[:3] + got_g[:3]) and th.equal(acc_g[4:], pre[4:] + got_g[4:])


@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[4], R.SHAPES[5]], ids=_sid)
def test_accumulate_adds_onto_a_filled_gradient_and_runs_are_bit_identical(shape):
    c = _case(shape)
    a_g, a_l, a_s, _, _ = run(c["e"], c["head"], shape)
    r_g, r_l, r_s, _, _ = run(c["e"], c["head"], shape)
    assert th.equal(a_g, r_g) and th.equal(a_l, r_l) and th.equal(a_s, r_s)  # two runs
    b_g, b_l, b_s, _, _ = run(c["e"], c["head"], shape, prefill=7.0)  # accumulate 0 overwrites
    assert th.equal(a_g, b_g) and th.equal(a_l, b_l) and th.equal(a_s, b_s)
    pre = th.randn(a_g.shape, generator=g(6)) * max(float(a_g.abs().max()), 1.0)
    acc_g, acc_l, acc_s, tails, _ = run(c["e"], c["head"], shape, accumulate=1, prefill=pre)
    assert th.equal(acc_g, pre + a_g) and th.equal(acc_l, a_l) and th.equal(acc_s, a_s)  # one float addition per element
    assert _untouched(tails)


@pytest.mark.parametrize("shape", [R.SHAPES[2], R.SHAPES[3]], ids=_sid)
def test_negative_scale_is_the_exact_negation(shape):
    c = _case(shape, "stressed", 1)
    p_g, p_l, p_s, _, _ = run(c["e"], c["head"], shape)
    n_g, n_l, n_s, _, _ = run(c["e"], c["head"], shape, scale=-R.SCALE)
    assert th.equal(n_g, -p_g) and th.equal(n_l, -p_l) and th.equal(n_s, p_s)
    assert bool((p_g != 0).any()) and bool((p_l != 0).all())


def test_refusals_write_nothing():
    ctx = _ctx()
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    for shape, kw, msg in (((1, 1, 2049), {}, b"embedding dim"), ((0, 2, 64), {}, b"must be positive"),
                           ((2, 2, 64), dict(null_head=True), b"null pointer")):
        cutn, B, D = shape
        e, head = th.randn(max(cutn, 1) * B, D), th.randn(D + 1)
        got_g, got_l, got_s, tails, rc = run(e, head, shape, check=False, **kw)  # (cutn = 0: outputs sized for one cut)
        assert rc == -2 and msg in ctx.lib.cgd_last_error(ctx.h), (rc, ctx.lib.cgd_last_error(ctx.h))
        assert got_g.numel() and bool(th.isnan(got_g).all()) and bool(th.isnan(got_l).all()) and bool(th.isnan(got_s).all()) and _untouched(tails)
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before


# ---- one guided step ------------------------------------------------------------------------------------------------------------------------
STEP_I, CUTN, HW = 12, 4, 64
TAPE = [(0, 0, 64), (5, 9, 40), (20, 3, 44), (29, 30, 34)]  # (ox, oy, size): the whole frame and three inner crops
AES_SCALE = 300.0


@functools.lru_cache(maxsize=None)
def _step_setup():
    """mini UNet at 64 x 64 and a ViT-B/32 tower on seeded weights, a small second tower, x_t, a source image, targets, directions and heads"""
    from cgd_amd import diffusion, nets, synthetic
    from tests import step_checks
    ctx = _ctx()
    _, vit = pc.build_vit_pair(ctx, "ViT-B/32")
    vit2 = nets.ClipImageTower(ctx, config=step_checks.MINI_VIT)
    vit2.load_state_dict(synthetic.synthetic_state_dict(vit2, seed=999))
    unet = nets.UNet(ctx, **pc.UNET_CASES["mini"])
    unet.load_state_dict(synthetic.synthetic_state_dict(unet, seed=1234, device=DEV))
    tables = diffusion.create_gaussian_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="50")
    gen = g(741)
    B = 2
    x = th.randn(B, 3, HW, HW, generator=gen) * 0.8
    source = th.tanh(th.randn(1, 3, HW, HW, generator=gen))
    dims = (vit.out_dim, vit2.out_dim)
    targets = [th.randn(1, D, generator=gen).to(DEV) for D in dims]
    dirs = [th.randn(1, D, generator=gen).to(DEV) for D in dims]
    heads = [nets.AestheticHead(D, DEV).load_state_dict(synthetic.aesthetic_head(D)) for D in dims]
    return dict(ctx=ctx, towers=[vit, vit2], unet=unet, tables=tables, x=x, source=source.to(DEV), targets=targets, dirs=dirs, heads=heads)


def _guided(st, leg="native", towers=1, with_target=True, with_direction=False, heads="all", cutter=None, tape=None, **kw):
    """one ClipGuidance.native call at step STEP_I -> (g, d loss / d x_in, log, launches of the call, the guidance object)"""
    from cgd_amd import guidance
    from tests import step_checks
    ctx, tables, unet = st["ctx"], st["tables"], st["unet"]
    B = st["x"].shape[0]
    cgs, tvs, rs = step_checks.default_scales(HW, HW)
    sampler = type("D", (), {"tables": tables, "num_timesteps": tables.num_timesteps, "step_coef": lambda self, a, b=None: tables.step_coef(a, b)})()
    if with_direction:
        kw.update(direction_embeds=st["dirs"][:towers], direction_weights=th.tensor([0.4] if with_target else [1.0]), direction_source=st["source"])
    if heads == "all":
        kw.update(aesthetic_heads=st["heads"][:towers], aesthetic_scale=AES_SCALE)
    elif heads == "second":
        kw.update(aesthetic_heads=[None, st["heads"][1]], aesthetic_scale=[0.0, AES_SCALE])
    cond = guidance.ClipGuidance(ctx, unet, st["towers"][:towers], sampler, [t for t in st["targets"][:towers]] if with_target else None,
                                 th.tensor([0.6] if with_direction else [1.0]) if with_target else None, CUTN, clip_guidance_scale=cgs,
                                 tv_scale=tvs, range_scale=rs, make_cutouts=cutter, **kw)
    if leg == "torch":
        cond._clip_leg = cond._clip_leg_torch
    cond.current_timestep = STEP_I
    cond.coords_tape = [tape or TAPE]
    coef = tables.step_coef(STEP_I, STEP_I)
    xd = st["x"].to(DEV)
    ts = th.full((B,), float(tables.model_timestep(STEP_I)), device=DEV)
    counts = (C.c_uint64 * 2)()
    out6 = unet.forward(xd, ts, th.full((B,), 7, device=DEV))
    x0, mean, logvar, xin = (th.empty_like(xd) for _ in range(4))
    ctx.check(ctx.lib.cgd_pmv_blend(ctx.h, xd.data_ptr(), out6.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), xin.data_ptr(),
                                    B, HW, HW, coef, ctx.stream()))
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    g_dev = cond.native(xd, x0, xin, coef)
    ctx.lib.cgd_launch_counts(counts)
    th.cuda.synchronize()
    return g_dev.clone(), cond._buf["gclip"].clone(), cond.log(), counts[0] - before, cond


def _compare(tag, native, torch_):
    (g_n, c_n, log_n, _, _), (g_t, c_t, log_t, _, _) = native, torch_
    out = []
    for name, a, b in (("g", g_n, g_t), ("g_clip_in", c_n, c_t)):
        sd = pc.unit_seed(b)
        out.append(rec(f"{tag} {name} (unit peak)", a * sd, b * sd))
        out.append(rec(f"{tag} {name}", a, b, allow_small=True))
    for key in ("CLIP Loss", "Aesthetic Loss", "Aesthetic Score", "TV Loss", "Range Loss", "Total Loss"):
        out.append(rec(f"{tag} {key}", th.tensor([log_n[key]]), th.tensor([log_t[key]]), allow_small=True))
    assert math.isfinite(log_n["Aesthetic Loss"]) and log_n["Aesthetic Loss"] != 0 and math.isfinite(log_n["Aesthetic Score"])
    _assert_ok(out)


STEP_CASES = {
    "target+head": dict(),
    "head only": dict(with_target=False),
    "two towers, head on the second": dict(towers=2, heads="second"),
    "target+direction+head": dict(with_direction=True),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_guided_step_matches_the_torch_leg(case):
    st = _step_setup()
    kw = STEP_CASES[case]
    native, torch_ = _guided(st, "native", **kw), _guided(st, "torch", **kw)
    _compare(f"aesthetic step[{case}]", native, torch_)
    log, cond = native[2], native[4]
    if case == "head only":
        assert abs(log["Aesthetic Loss"] - log["CLIP Loss"]) <= 1e-5 * abs(log["CLIP Loss"])
        assert list(log) == ["CLIP Loss", "Range Loss", "TV Loss", "Aesthetic Loss", "Aesthetic Score", "Total Loss", "Grad"]
    if case == "target+direction+head":
        assert cond._clip_kinds() == 3
        assert list(log) == ["CLIP Loss", "Range Loss", "TV Loss", "Direction Loss", "Aesthetic Loss", "Aesthetic Score", "Total Loss", "Grad"]
    if case == "two towers, head on the second":
        part = cond.clip_part.view(2, 2, -1)
        assert not part[0, 1].view(th.int32).any() and bool(part[1, 1].any())  # zeros in the aesthetic rows of the tower without a head
    # the logged term is -scale * sum_b mean_cut s, the logged score the mean of s: one head, so the two agree
    B = st["x"].shape[0]
    assert abs(log["Aesthetic Loss"] + AES_SCALE * B * log["Aesthetic Score"]) <= 1e-4 * abs(log["Aesthetic Loss"])


def test_guided_step_with_the_resized_cutter_matches_the_torch_leg():
    from cgd_amd import guidance
    st = _step_setup()
    mk = guidance.MakeCutoutsResized(224, overview=1, inner=3, ctx=st["ctx"])
    # (ox, oy, w, h, flags): the overview, then a gray, a mirrored and a non-square inner cut
    recs = [(0, 0, HW, HW, 0), (3, 5, 40, 40, guidance.RESIZE_GRAY), (20, 4, 36, 36, guidance.RESIZE_FLIP), (10, 20, 44, 30, 0)]
    native = _guided(st, "native", cutter=mk, tape=recs)
    torch_ = _guided(st, "torch", cutter=mk, tape=recs)
    _compare("aesthetic step[cuts=1:3]", native, torch_)


def test_launch_count_grows_by_the_number_of_towers_with_a_head():
    st = _step_setup()
    n = {name: _guided(st, towers=2, heads=name)[3] for name in ("none", "second", "all")}
    print(f"launches of a two-tower step: {n}")
    assert n["second"] == n["none"] + 1 and n["all"] == n["none"] + 2
    one = {name: _guided(st, towers=1, heads=name)[3] for name in ("none", "all")}
    assert one["all"] == one["none"] + 1


def test_without_the_keywords_the_step_is_unchanged():
    """the same guided step through ClipGuidance without the keywords and with them unset: same bits, same buffers, same launch count, same log keys"""
    st = _step_setup()
    out = []
    for kw in (dict(heads="none"), dict(heads="none", aesthetic_heads=None, aesthetic_scale=0.0),
               dict(heads="none", aesthetic_heads=st["heads"][:1], aesthetic_scale=0.0)):
        g_dev, gclip, log, launches, cond = _guided(st, **kw)
        out.append((g_dev, gclip, log, launches, sorted(cond._buf)))
    for other in out[1:]:
        assert th.equal(out[0][0], other[0]) and th.equal(out[0][1], other[1]) and out[0][2:] == other[2:]
    assert list(out[0][2]) == ["CLIP Loss", "Range Loss", "TV Loss", "Total Loss", "Grad"] and "aes_score" not in out[0][4]


# ---- the drop-in generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_augs", [False, True], ids=["plain", "use_augs"])
def test_dropin_generator_with_an_aesthetic_head(tmp_path, monkeypatch, capsys, use_augs):
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion
    assert not os.path.exists("none.pth")
    items = list(clip_guided_diffusion(prompts=["a garden"], image_size=64, batch_size=1, num_cutouts=2, timestep_respacing="ddim6",
                                       clip_model_name="ViT-B/32+aesthetic=none.pth:300", prefix_path=str(tmp_path / "out"),
                                       checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=True, device="cuda", use_augs=use_augs))
    assert [b for b, _ in items] == [0] * 6 and all(os.path.isfile(p) for _, p in items)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "Aesthetic Loss" in ln]
    assert len(lines) == 6
    for ln in lines:
        vals = dict(kv.split(": ") for kv in ln.split("\t"))
        assert math.isfinite(float(vals["Aesthetic Loss"])) and float(vals["Aesthetic Loss"]) != 0 and math.isfinite(float(vals["CLIP Loss"]))
