"""Host side of the aesthetic-predictor guidance (csrc/aesthetic.hip, nets.AestheticHead, clip_util.split_aesthetic): the float64 reference
(tests/aesthetic_ref.py) against torch's autograd, the condition on the shared cases that lets the GPU tests' bound measure the kernel, the
collapse of the published head formats, the `aesthetic=FILE:SCALE` entry, the declared symbol, the entry's refusals without a context, and
ClipGuidance's argument checks and call sequence on recording stubs.  No GPU."""
import itertools
import math
import re

import pytest
import torch as th
import torch.nn.functional as F

import cgd_amd  # noqa: F401
from cgd_amd import guidance as dg
from cgd_amd import lib as L
from cgd_amd import nets, synthetic
from tests import aesthetic_ref as R
from tests.test_direction_host import _Recorder

CASES = [(shape, kind, seed) for shape in R.SHAPES for kind in R.KINDS for seed in R.SEEDS[kind]]


def _id(case):
    return "x".join(map(str, case[0])) + f"-{case[1]}{case[2]}"


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_reference_equals_float64_autograd_of_the_normalize_formulation(case):
    shape, kind, seed = case
    cutn, B, D = shape
    e, head = R.make_case(shape, kind, seed)
    assert bool((e.norm(dim=1) > 0).all())
    er = e.double().requires_grad_()
    h = head.double()
    score = F.normalize(er, dim=-1) @ h[:-1] + h[-1]
    loss = score.view(cutn, B).mean(0).sum() * -R.SCALE
    g, = th.autograd.grad(loss, er)
    ref_l, ref_g, ref_s = R.loss_grad_score(e, head, cutn, B)
    assert th.allclose(ref_s, score.detach(), rtol=1e-13, atol=0)
    assert abs(float(ref_l.sum()) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    # the gradient times |e_r| is c (a - (a . e^) e^), of size c max|a|; at D = 1 both sides are zero up to the rounding of e^
    norm = e.double().norm(dim=1, keepdim=True)
    assert float(((ref_g - g) * norm).abs().max()) <= 1e-12 * R.SCALE / cutn * float(h[:-1].abs().max())


def test_reference_zero_row_has_the_bias_score_and_no_gradient():
    shape = R.SHAPES[0]
    e, head = R.make_case(shape)
    e[3] = 0
    l, g, s = R.loss_grad_score(e, head, shape[0], shape[1])
    assert float(s[3]) == float(head[-1].double()) and not g[3].any() and float(l[3]) == -R.SCALE / shape[0] * float(head[-1].double())
    # a negative scale is the exact negation
    l2, g2, s2 = R.loss_grad_score(e, head, shape[0], shape[1], -R.SCALE)
    assert th.equal(l2, -l) and th.equal(g2, -g) and th.equal(s2, s)


def _float32_other_order(e, head, cutn, scale=R.SCALE):
    """the kernel's formulas in float32 on the CPU, every sum over D taken over a fixed permutation of the elements in chunks of 7"""
    D = e.shape[1]
    perm = th.randperm(D, generator=th.Generator().manual_seed(D))
    e, a, beta = e.float()[:, perm], head.float()[:-1][perm], head.float()[-1]

    def total(t):
        return th.stack([c.sum(1) for c in t.split(7, dim=1)], 1).sum(1)

    inv = 1.0 / total(e * e).sqrt().clamp_min(1e-12)
    eh = e * inv[:, None]
    dot = total(eh * a)
    c = th.tensor(scale / cutn, dtype=th.float32)
    grad = th.empty_like(e)
    grad[:, perm] = -c * (a[None, :] - dot[:, None] * eh) * inv[:, None]
    return -c * (dot + beta), grad, dot + beta


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_shared_cases_leave_three_quarters_of_the_bound_to_the_kernel(case):
    """float32 in another summation order against the float64 reference: at most 0.25 of |a - b| <= 1e-4 + 1e-3 |ref| on every row's partial
    loss, on the loss sum, on the score and on the gradient as the GPU test grades it (as it stands on ordinary values; times |e_r| and at
    unit peak on stressed ones).  beta is chosen in make_case so that a . e^ and beta cannot cancel."""
    shape, kind, seed = case
    cutn, B, D = shape
    e, head = R.make_case(shape, kind, seed)
    ref_l, ref_g, ref_s = R.loss_grad_score(e, head, cutn, B)
    got_l, got_g, got_s = _float32_other_order(e, head, cutn)
    uses = {"partials": R.within(got_l, ref_l)[1], "sum": R.within(got_l.double().sum().view(1), ref_l.sum().view(1))[1],
            "score": R.within(got_s, ref_s)[1]}
    if kind == "stressed":
        a, b, peak = R.graded_gradient(got_g, ref_g, e, head, cutn)
        assert D == 1 or peak > 0
        uses["gradient"] = R.within(a, b)[1]
    else:
        uses["gradient"] = R.within(got_g, ref_g)[1]
    print(_id(case), {k: round(v, 5) for k, v in uses.items()})
    assert max(uses.values()) <= 0.25, uses


def test_case_builder_reaches_the_stated_regimes():
    seen = set()
    for seed in R.SEEDS["stressed"]:
        e, head = R.make_case(R.SHAPES[0], "stressed", seed)
        norms = e.double().norm(dim=1)
        seen |= {(r, round(math.log10(float(n)))) for r, n in enumerate(norms)}
        a = head[:-1].abs()
        assert float(a.max() / a.min()) >= 1e3 and float(a.max()) <= 100.0 and float(a.min()) >= 0.01
    assert seen == set(itertools.product(range(8), (-3, 0, 3)))
    e, head = R.make_case(R.SHAPES[0])
    assert bool(((e.norm(dim=1) > 7.9) & (e.norm(dim=1) < 12.1)).all())
    assert [s for s in R.SHAPES if s[2] == 2048 or s[2] == 65 or s[2] == 1] == [(1, 1, 2048), (5, 2, 65), (2, 2, 1)]


# ---- the published formats ---------------------------------------------------------------------------------------------------------------
def _improved(dims=(768, 1024, 128, 64, 16, 1), seed=0):
    """the improved predictor's nn.Sequential as upstream builds it: Linear / Dropout pairs, the last two Linears back to back"""
    th.manual_seed(seed)
    layers = []
    for i, (m, n) in enumerate(zip(dims[:-1], dims[1:])):
        layers.append(th.nn.Linear(m, n))
        if i < len(dims) - 3:
            layers.append(th.nn.Dropout(0.2 if i == 0 else 0.1))
    return th.nn.Sequential(*layers).double().eval()


def test_collapse_of_the_five_layer_chain_equals_the_eval_mode_module():
    net = _improved()
    sd = {"layers." + k: v for k, v in net.state_dict().items()}
    assert [k for k in sd if k.endswith("weight")] == [f"layers.{i}.weight" for i in (0, 2, 4, 6, 7)]
    vec = nets.collapse_aesthetic_state_dict(sd)
    assert vec.dtype == th.float64 and vec.numel() == 769
    x = th.randn(9, 768, dtype=th.float64, generator=th.Generator().manual_seed(1))
    want = net(x).flatten().detach()
    got = x @ vec[:-1] + vec[-1]
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # wrapped, with DataParallel prefixes and an epoch counter; float32 tensors collapse in float64 all the same
    wrapped = {"state_dict": {"module." + k: v.float() for k, v in sd.items()}, "epoch": 3}
    vec32 = nets.collapse_aesthetic_state_dict(wrapped)
    assert vec32.dtype == th.float64 and float((vec32 - vec).abs().max()) <= 1e-5 * float(vec.abs().max())
    head = nets.AestheticHead.from_state_dict(sd, device="cpu")
    assert head.dim == 768 and head.vec.dtype == th.float32 and tuple(head.vec.shape) == (769,)


@pytest.mark.parametrize("dim", [512, 768])
def test_the_linear_format_loads(dim):
    lin = th.nn.Linear(dim, 1)
    sd = lin.state_dict()
    assert tuple(sd["weight"].shape) == (1, dim) and tuple(sd["bias"].shape) == (1,)
    head = nets.AestheticHead.from_state_dict(sd, device="cpu")
    assert head.dim == dim and th.equal(head.vec[:-1], sd["weight"][0]) and th.equal(head.vec[-1:], sd["bias"])
    assert head.param_specs() == [("head", dim + 1)]


def test_malformed_heads_are_refused_by_name():
    ok = {"layers." + k: v for k, v in _improved((32, 16, 8, 4, 2, 1)).state_dict().items()}
    nets.collapse_aesthetic_state_dict(ok)
    with pytest.raises(ValueError, match="ends in 2 outputs"):
        nets.collapse_aesthetic_state_dict({k: v for k, v in ok.items() if not k.startswith("layers.7.")})
    broken = dict(ok)
    broken["layers.4.weight"] = th.zeros(4, 9, dtype=th.float64)
    with pytest.raises(ValueError, match="broken chain.*layers.4.weight"):
        nets.collapse_aesthetic_state_dict(broken)
    with pytest.raises(ValueError, match="layers.2.bias"):
        nets.collapse_aesthetic_state_dict({**ok, "layers.2.bias": th.zeros(5)})
    with pytest.raises(ValueError, match="bn.running_mean"):
        nets.collapse_aesthetic_state_dict({**ok, "bn.running_mean": th.zeros(5)})
    with pytest.raises(ValueError, match="no 2-D"):
        nets.collapse_aesthetic_state_dict({"bias": th.zeros(1)})
    with pytest.raises(ValueError, match="state dict"):
        nets.collapse_aesthetic_state_dict([1, 2])
    with pytest.raises(ValueError, match="dim \\+ 1"):
        nets.AestheticHead(8, "cpu").load_state_dict({"head": th.zeros(8)})


def test_loader_refuses_a_head_of_another_width_and_a_missing_file(tmp_path, monkeypatch):
    from cgd import clip_util
    monkeypatch.delenv("CGD_SYNTHETIC_WEIGHTS", raising=False)
    ctx = type("Ctx", (), {"device": 0})()
    th.save(th.nn.Linear(768, 1).state_dict(), tmp_path / "l14.pth")
    with pytest.raises(ValueError, match="768-wide.*ViT-B/32 gives 512"):
        clip_util.load_aesthetic(ctx, str(tmp_path / "l14.pth"), "cuda", 512, "ViT-B/32")
    with pytest.raises(FileNotFoundError, match="none.pth"):
        clip_util.load_aesthetic(ctx, str(tmp_path / "none.pth"), "cuda", 512)
    sd = synthetic.aesthetic_head(640)
    assert tuple(sd["head"].shape) == (641,) and th.equal(sd["head"], synthetic.aesthetic_head(640)["head"]) and float(sd["head"][-1]) == 5.0


# ---- the `aesthetic=FILE:SCALE` entry -----------------------------------------------------------------------------------------------------
def test_split_aesthetic_binds_to_the_tower_before_it():
    from cgd.clip_util import split_aesthetic
    assert split_aesthetic("ViT-L/14+aesthetic=sa_0_4_vit_l_14_linear.pth:500+ViT-B/32") == (
        "ViT-L/14+ViT-B/32", [("sa_0_4_vit_l_14_linear.pth", 500.0), None])
    assert split_aesthetic("ViT-B/32+ViT-B/16+aesthetic=b16.pth:-3e2") == ("ViT-B/32+ViT-B/16", [None, ("b16.pth", -300.0)])
    assert split_aesthetic("ViT-B/32+aesthetic=a.pth:1+ViT-B/16+aesthetic=b.pth:2") == ("ViT-B/32+ViT-B/16", [("a.pth", 1.0), ("b.pth", 2.0)])
    # entries that are no towers do not count; FILE keeps its own colons (split at the last one)
    assert split_aesthetic("ViT-B/32+cuts=4:12+aesthetic=C:/heads/a.pth:0.5+secondary=s.pth") == (
        "ViT-B/32+cuts=4:12+secondary=s.pth", [("C:/heads/a.pth", 0.5)])
    assert split_aesthetic(" ViT-B/32 + aesthetic = a.pth : 7 ") == ("ViT-B/32", [("a.pth", 7.0)])
    # lists without the entry pass through unchanged
    for plain in ("ViT-B/32", "RN50+ViT-L/14", "ViT-B/32+secondary=s.pth+cuts=2:3", "ViT-B-32=laion.pt+classifier=c.pt:207:2"):
        names, heads = split_aesthetic(plain)
        assert names is plain and heads == [None] * (2 if plain.startswith("RN50") else 1)


@pytest.mark.parametrize("bad, match", [
    ("aesthetic=a.pth:300", "tower before it"), ("aesthetic=a.pth:300+ViT-B/32", "tower before it"),
    ("cuts=4:4+aesthetic=a.pth:300+ViT-B/32", "tower before it"),
    ("ViT-B/32+aesthetic=:300", "checkpoint path"), ("ViT-B/32+aesthetic=", "checkpoint path"), ("ViT-B/32+aesthetic= :3", "checkpoint path"),
    ("ViT-B/32+aesthetic=a.pth", "SCALE"), ("ViT-B/32+aesthetic=a.pth:", "SCALE"), ("ViT-B/32+aesthetic=a.pth:big", "SCALE"),
    ("ViT-B/32+aesthetic=a.pth:nan", "finite non-zero"), ("ViT-B/32+aesthetic=a.pth:inf", "finite non-zero"),
    ("ViT-B/32+aesthetic=a.pth:-inf", "finite non-zero"), ("ViT-B/32+aesthetic=a.pth:0", "finite non-zero"),
    ("ViT-B/32+aesthetic=a.pth:0.0", "finite non-zero"),
    ("ViT-B/32+aesthetic=a.pth:1+aesthetic=b.pth:2", "two 'aesthetic=' entries on one tower"),
    ("ViT-B/32+aesthetic=a.pth:1+cuts=1:1+aesthetic=b.pth:2", "two 'aesthetic=' entries on one tower"),
    # the improved predictor's own name is cut at its '+': both errors say what to do
    ("ViT-L/14+aesthetic=sac+logos+ava1-l14-linearMSE.pth:1", "renamed or symlinked"),
    ("ViT-L/14+aesthetic=sac:2+logos+ava1-l14-linearMSE.pth", "'logos' behind an 'aesthetic=' entry.*renamed or symlinked"),
])
def test_split_aesthetic_refusals(bad, match):
    from cgd.clip_util import split_aesthetic
    with pytest.raises(ValueError, match=match):
        split_aesthetic(bad)


def test_generator_refuses_before_anything_is_loaded(monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    monkeypatch.setattr(clip_util, "load_clip", no_load)
    monkeypatch.setattr(clip_util, "load_aesthetic", no_load)
    monkeypatch.setattr(script_util, "download_guided_diffusion", no_load)
    for name in ("aesthetic=a.pth:300", "ViT-B/32+aesthetic=a.pth", "ViT-B/32+aesthetic=a.pth:0", "ViT-B/32+aesthetic=:5",
                 "ViT-B/32+aesthetic=a.pth:1+aesthetic=b.pth:2", "ViT-B/32+aesthetic=a.pth:nan"):
        with pytest.raises(ValueError, match="aesthetic"):
            next(mine.clip_guided_diffusion(device="cuda", prompts=["a cat"], clip_model_name=name))
    text = " ".join(mine.build_parser().format_help().split())
    assert "A+aesthetic=FILE:SCALE" in text and "renamed or symlinked" in text


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_signature_table_has_it():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgd_mi355x.h")).read()
    m = re.search(r"int cgd_aesthetic_loss\(([^;]*)\);", header)
    assert m, "include/cgd_mi355x.h does not declare cgd_aesthetic_loss"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert params == ["cgd_ctx* ctx", "const float* emb", "const float* head", "float* d_emb", "float* loss_part", "float* score", "int cutn",
                      "int B", "int D", "float scale", "int accumulate", "void* stream"]
    import ctypes as C
    res, args = L._SIGS["cgd_aesthetic_loss"]
    assert res is C.c_int32 or res is C.c_int
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    assert args == [vp] * 6 + [i32, i32, i32, f32, i32, vp]
    assert "cgd_aesthetic_loss" in L.EXPORTED_SYMBOLS


def test_entry_refuses_bad_arguments_without_a_context():
    h = L.load()
    ok = dict(emb=64, head=4096, demb=8192, part=12288, score=16384, cutn=4, B=2, D=512, scale=500.0, acc=0)

    def call(**kw):
        a = {**ok, **kw}
        return h.cgd_aesthetic_loss(None, a["emb"], a["head"], a["demb"], a["part"], a["score"], a["cutn"], a["B"], a["D"], a["scale"], a["acc"], None)

    assert call() == -3 and call(score=None) == -3 and call(D=2048) == -3 and call(scale=-1.0) == -3 and call(acc=1) == -3  # nothing to refuse
    for kw in (dict(D=2049), dict(D=0), dict(D=-4), dict(cutn=0), dict(cutn=-1), dict(B=0), dict(emb=None), dict(head=None), dict(demb=None),
               dict(part=None), dict(cutn=1 << 16, B=1 << 15)):
        assert call(**kw) == -2, kw


# ---- ClipGuidance on recording stubs ----------------------------------------------------------------------------------------------------
B, H, W = 2, 32, 48
TAIL = ["cgd_guidance_part_blocks", "cgd_guidance_combine", "unet.dgrad", "cgd_grad_finish", "cgd_scalars"]


def _head(dim, seed=0):
    return nets.AestheticHead(dim, "cpu").load_state_dict(synthetic.aesthetic_head(dim, seed))


def _run(guid, cutn=6):
    guid.current_timestep, guid.coords_tape = 49, [[(0, 0, 32)] * cutn]
    x = th.zeros(B, 3, H, W)
    return guid.native(x, x.clone(), x.clone(), coef=None)


def test_call_sequence_with_a_target_and_a_head():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    head = _head(16)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 6, aesthetic_heads=head, aesthetic_scale=300.0)
    _run(guid)
    assert r.names() == ["cgd_cutouts_fwd", "vit.encode_image", "cgd_spherical_loss", "cgd_aesthetic_loss", "vit.dgrad", "cgd_cutouts_bwd"] + TAIL
    N = 6 * B
    sph, aes = r.args("cgd_spherical_loss")[0], r.args("cgd_aesthetic_loss")[0]
    # (h, emb, head, d_emb, loss_part, score, cutn, B, D, scale, accumulate, stream): onto the spherical gradient, rows behind the spherical ones
    assert aes[1] == sph[1] and aes[3] == sph[4] and aes[4] - sph[5] == 4 * N and aes[6:11] == (6, B, 16, 300.0, 1)
    assert aes[2] == guid.aes_list[0][0].data_ptr() and aes[5] == guid.aes_score.data_ptr() and tuple(guid.aes_score.shape) == (1, N)
    assert r.args("cgd_scalars")[0][2] == 2 * N and guid.clip_part.numel() == 2 * N
    assert list(guid.log()) == ["CLIP Loss", "Range Loss", "TV Loss", "Aesthetic Loss", "Aesthetic Score", "Total Loss", "Grad"]


def test_call_sequence_with_a_head_only():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, None, None, 6, aesthetic_heads=[_head(16)], aesthetic_scale=[-2.0])
    _run(guid)
    assert r.names() == ["cgd_cutouts_fwd", "vit.encode_image", "cgd_aesthetic_loss", "vit.dgrad", "cgd_cutouts_bwd"] + TAIL
    aes = r.args("cgd_aesthetic_loss")[0]
    assert aes[6:11] == (6, B, 16, -2.0, 0) and aes[4] == guid.clip_part.data_ptr()  # nothing wrote d_emb before: accumulate 0
    assert r.args("cgd_scalars")[0][2] == 6 * B and not guid.no_clip


def test_call_sequence_with_directions_and_a_head_on_the_second_of_two_towers():
    r = _Recorder()
    vit, rn = r.tower("vit", 32, 8, 16), r.tower("rn", 64, 0, 24)
    guid = dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, [th.randn(1, 16), th.randn(1, 24)], [0.5], 6,
                           direction_embeds=[th.randn(1, 16), th.randn(1, 24)], direction_weights=[0.75], direction_source=th.zeros(1, 3, H, W),
                           aesthetic_heads=[None, _head(24)], aesthetic_scale=[0.0, 40.0])
    _run(guid)

    def leg(t, head):
        return ["cgd_cutouts_fwd", f"{t}.encode_image"] * 2 + ["cgd_spherical_loss", "cgd_directional_loss"] + (
            ["cgd_aesthetic_loss"] if head else []) + [f"{t}.dgrad", "cgd_cutouts_bwd"]

    assert r.names() == leg("vit", False) + leg("rn", True) + TAIL
    N = 6 * B
    sph, drc, aes = r.args("cgd_spherical_loss"), r.args("cgd_directional_loss"), r.args("cgd_aesthetic_loss")
    base = sph[0][5]
    # three kinds of rows per tower: spherical, directional, aesthetic; the tower without a head has zeros in its aesthetic rows
    assert [s[5] - base for s in sph] == [0, 4 * 3 * N] and [d[6] - base for d in drc] == [4 * N, 4 * 4 * N] and aes[0][4] - base == 4 * 5 * N
    assert aes[0][6:11] == (6, B, 24, 40.0, 1) and guid.clip_part.numel() == 2 * 3 * N
    assert not guid.clip_part[2 * N:3 * N].any()
    assert list(guid.log()) == ["CLIP Loss", "Range Loss", "TV Loss", "Direction Loss", "Aesthetic Loss", "Aesthetic Score", "Total Loss", "Grad"]
    # the directional share is still the directional rows, not the last ones
    guid.clip_part.zero_()
    guid.clip_part[N:2 * N] = 1.0
    guid.clip_part[5 * N:] = 2.0
    guid.aes_score.fill_(6.5)
    log = guid.log()
    assert log["Direction Loss"] == N and log["Aesthetic Loss"] == 2 * N and log["Aesthetic Score"] == 6.5


def test_heads_only_and_none_on_the_first_tower_skips_that_tower():
    r = _Recorder()
    vit, rn = r.tower("vit", 32, 8, 16), r.tower("rn", 64, 0, 24)
    guid = dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, None, None, 6, aesthetic_heads=[None, _head(24)], aesthetic_scale=5.0)
    _run(guid)
    assert r.names() == ["cgd_cutouts_fwd", "rn.encode_image", "cgd_aesthetic_loss", "rn.dgrad", "cgd_cutouts_bwd"] + TAIL
    assert r.args("cgd_cutouts_bwd")[0][-2] == 0 and not guid.clip_part[:6 * B].any()  # the first tower that runs overwrites gclip


def test_argument_checks_of_the_class():
    r = _Recorder()
    vit, rn = r.tower("vit", 32, 8, 16), r.tower("rn", 64, 0, 24)
    t16, t24 = th.randn(1, 16), th.randn(1, 24)
    with pytest.raises(ValueError, match="1 aesthetic heads for 2 CLIP towers"):
        dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, [t16, t24], [1.0], 4, aesthetic_heads=[_head(16)], aesthetic_scale=1.0)
    with pytest.raises(ValueError, match="3 aesthetic scales for 2 heads"):
        dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, [t16, t24], [1.0], 4, aesthetic_heads=[_head(16), None], aesthetic_scale=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="tower 1 is for 16-wide embeddings, the tower gives 24"):
        dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, [t16, t24], [1.0], 4, aesthetic_heads=[_head(16), _head(16)], aesthetic_scale=1.0)
    with pytest.raises(ValueError, match="finite"):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, t16, [1.0], 4, aesthetic_heads=_head(16), aesthetic_scale=float("nan"))
    with pytest.raises(ValueError, match="no target embeddings"):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, None, None, 4, aesthetic_heads=_head(16), aesthetic_scale=0.0)
    with pytest.raises(ValueError, match="loaded"):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, t16, [1.0], 4, aesthetic_heads=nets.AestheticHead(16, "cpu"), aesthetic_scale=2.0)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, t16, [1.0], 4, aesthetic_heads=_head(16), aesthetic_scale=2.0)
    assert guid.aes_list[0][1] == 2.0 and guid._clip_kinds() == 2
    assert not r.calls  # every refusal came before any launch


def test_scale_zero_and_unset_keywords_leave_the_step_as_it_is():
    seqs = []
    for kw in ({}, dict(aesthetic_heads=None, aesthetic_scale=0.0), dict(aesthetic_heads="head", aesthetic_scale=0.0),
               dict(aesthetic_heads=["head"], aesthetic_scale=[0])):
        r = _Recorder()
        vit = r.tower("vit", 32, 8, 16)
        kw = {k: (_head(16) if v == "head" else [_head(16)] if v == ["head"] else v) for k, v in kw.items()}
        guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(2, 16), [1.0, 0.5], 6, **kw)
        _run(guid)
        assert guid.aes_list is None and guid._clip_kinds() == 1 and guid.aes_score is None
        assert r.names() == ["cgd_cutouts_fwd", "vit.encode_image", "cgd_spherical_loss", "vit.dgrad", "cgd_cutouts_bwd"] + TAIL
        assert r.args("cgd_scalars")[0][2] == 6 * B
        assert list(guid.log()) == ["CLIP Loss", "Range Loss", "TV Loss", "Total Loss", "Grad"]
        seqs.append(sorted(guid._buf))
    assert all(s == seqs[0] for s in seqs) and "aes_score" not in seqs[0]
