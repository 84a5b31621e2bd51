"""open_clip (LAION) ViT support on the device: the exact GELU (activation code 3) as an op, in the towers and in a guided step, and the fused
attention kernels at head dim 80 (ViT-H-14).  References are float64 on the CPU; the criterion is parity_checks.rec, |a - b| <= 1e-4 + 1e-3 |ref|
for every element, gradients at unit peak (unit_seed) as check_attn / check_vit judge theirs."""
import ctypes as C
import functools
import math

import pytest
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from tests import parity_checks as pc
from tests import step_checks, text_ref
from tests import value_regime_checks as vr

pytestmark = pytest.mark.gpu


def _report(recs):
    print("\n".join(f"{'OK  ' if r['ok'] else 'FAIL'} {r['name']}: abs {r['err_abs']:.3e} rel-to-peak {r['err_rel']:.3e} peak {r['ref_max']:.3e}"
                    for r in recs))


def _assert_all(recs):
    _report(recs)
    bad = [r["name"] for r in recs if not r["ok"]]
    assert not bad, bad


def _gelu_case(u, dy):
    ur = u.double().requires_grad_()
    y = F.gelu(ur)  # the erf form
    (gr,) = th.autograd.grad((y * dy.double()).sum(), ur)
    return y.detach(), gr


def test_act3_is_the_exact_gelu():
    from cgd_amd import lib, ops
    ctx = pc._ctx(1)
    recs = []
    v = th.randn(1000, generator=pc.g(31)) * 3
    dy = th.randn(1000, generator=pc.g(32))
    y, gr = _gelu_case(v, dy)
    recs.append(pc.rec("act3 fwd randn * 3", ops.act(ctx, v.to(pc.DEV), 3), y.float()))
    recs.append(pc.rec("act3 bwd randn * 3", ops.act(ctx, v.to(pc.DEV), 3, dy.to(pc.DEV)), gr.float()))
    # the MLP-input range of the trained-network value regimes: the grid of value_regime_checks.act_grid (|u| up to 150, tiny and zero arguments)
    u = vr.act_grid(1)
    du = th.randn(u.numel(), generator=pc.g(441)).abs() + 0.5
    y, gr = _gelu_case(u, du)
    recs.append(pc.rec("act3 fwd on the MLP-input grid", ops.act(ctx, u.to(pc.DEV), 3), y.float()))
    recs.append(pc.rec("act3 bwd on the MLP-input grid", ops.act(ctx, u.to(pc.DEV), 3, du.to(pc.DEV)), gr.float()))
    _assert_all(recs)
    for bad in (0, 4, -1, 17):  # an unknown code fails: it used to run SiLU
        with pytest.raises(lib.CgdError):
            ops.act(ctx, v.to(pc.DEV), bad)
        with pytest.raises(lib.CgdError):
            ops.act(ctx, v.to(pc.DEV), bad, dy.to(pc.DEV))


D80_SHAPES = [(2, 2, 257, 80, 0), (1, 16, 257, 80, 0), (1, 3, 100, 80, 0), (1, 2, 72, 80, 0), (1, 2, 50, 80, 0), (1, 2, 577, 80, 0), (1, 2, 256, 80, 1),
              (1, 4, 257, 64, 0)]  # the last: d = 64 unchanged, as a control


def _family(lib_, T, d, heads, precision):
    out2 = (C.c_int * 2)()
    assert lib_.cgd_op_attn_plan(T, d, 3 * heads * d, heads * d, precision, -1, out2) == 0
    return out2[0]


@pytest.mark.parametrize("precision", [0, 1])
def test_attention_head_dim_80(precision):
    from cgd_amd import ops
    ctx = pc._ctx(precision)
    recs = []
    for (nb, heads, T, d, legacy) in D80_SHAPES:
        fam = _family(ctx.lib, T, d, heads, precision)
        assert fam == (3 if precision == 1 else (2 if d == 64 else 0)), (T, d, fam)
        Cc = heads * d
        qkv = th.randn(nb * T, 3 * Cc, generator=pc.g(40))
        dout = th.randn(nb * T, Cc, generator=pc.g(41))
        qr = qkv.double().requires_grad_()
        ref = pc._attn_ref(qr, nb, heads, T, d, legacy)
        (ref * dout.double()).sum().backward()
        at = ops.Attention(ctx, nb, heads, T, d, legacy, pc.DEV)
        got = at.forward(qkv.to(pc.DEV))
        tag = f"[p{precision} family {fam}] nb{nb} h{heads} T{T} d{d} legacy{legacy}"
        recs.append(pc.rec("attn fwd" + tag, got, ref.float()))
        sd = pc.unit_seed(qr.grad)
        dq = at.backward(qkv.to(pc.DEV), (dout * sd).to(pc.DEV))
        recs.append(pc.rec("attn bwd" + tag, dq, (qr.grad * sd).float()))
    _assert_all(recs)


@pytest.mark.parametrize("precision", [0, 1])
def test_causal_attention_head_dim_80(precision):
    from cgd_amd import ops
    ctx = pc._ctx(precision)
    nb, heads, T, d = 2, 2, 77, 80
    qkv = th.randn(nb * T, 3 * heads * d, generator=pc.g(77))
    x = qkv.double().view(nb, T, 3, heads, d).permute(2, 0, 3, 1, 4)
    s = x[0] @ x[1].transpose(-1, -2) / math.sqrt(d)
    s = s.masked_fill(th.ones(T, T, dtype=th.bool).triu(1), float("-inf"))
    ref = (th.softmax(s, -1) @ x[2]).permute(0, 2, 1, 3).reshape(nb * T, heads * d)
    got = ops.Attention(ctx, nb, heads, T, d, 0, pc.DEV).forward_causal(qkv.to(pc.DEV))
    fam = _family(ctx.lib, T, d, heads, precision)
    assert fam == (3 if precision == 1 else 0)
    _assert_all([pc.rec(f"causal attn[p{precision} family {fam}] nb{nb} h{heads} T{T} d{d}", got, ref.float())])
    assert th.allclose(got[:1].cpu(), qkv[:1, 2 * heads * d:].float(), rtol=1e-2, atol=1e-2)  # query 0 sees key 0 only


VIT_CFG = (224, 14, 160, 2, 2, 64)  # 257 tokens, two heads of 80


def _gelu_vit(seed=4321):
    from oracle import clip_vit as ocv
    ref = ocv.ClipImageModel.__new__(ocv.ClipImageModel)
    nn.Module.__init__(ref)
    ref.visual = ocv.VisionTransformer(*VIT_CFG)
    ocv.synthetic_init_(ref, seed=seed).eval()
    for blk in ref.visual.transformer.resblocks:
        blk.mlp.gelu = nn.GELU()
    for p in ref.parameters():
        p.requires_grad_(False)
    return ref


def _vit_recs(ctx, ref, activation, tag, N=3):
    from cgd_amd import nets
    dev = nets.ClipImageTower(ctx, config=VIT_CFG, activation=activation)
    dev.load_clip_state_dict({k: v.to(pc.DEV) for k, v in ref.state_dict().items()})
    img = th.randn(N, 3, 224, 224, generator=pc.g(70))
    de = th.randn(N, VIT_CFG[5], generator=pc.g(71))
    r64 = _gelu_vit().double()
    ir = img.double().requires_grad_()
    e = r64.visual(ir)
    (e * de.double()).sum().backward()
    sd = pc.unit_seed(ir.grad)
    ed = dev.encode_image(img.to(pc.DEV))
    di = dev.dgrad((de * sd).to(pc.DEV))
    th.cuda.synchronize()
    return [pc.rec(f"{tag} forward", ed, e.detach().float()), pc.rec(f"{tag} dgrad", di, (ir.grad * sd).float())]


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("precision", [0, 1])
def test_gelu_image_tower(precision, fuse, monkeypatch):
    monkeypatch.setenv("CGD_FUSE_ACT", str(fuse))  # read when the context is created: the activation in the GEMM epilogues, or as its own kernel
    ctx = pc._ctx(precision)
    ref = _gelu_vit()
    _assert_all(_vit_recs(ctx, ref, "gelu", f"gelu vit[p{precision} fuse{fuse}]"))
    # the same weights through QuickGELU must NOT pass: the switch does something
    wrong = _vit_recs(ctx, ref, "quick_gelu", f"quick_gelu on gelu weights[p{precision} fuse{fuse}]")
    _report(wrong)
    assert not wrong[0]["ok"] and not wrong[1]["ok"]


@pytest.mark.parametrize("precision", [0, 1])
def test_gelu_text_tower(precision):
    from cgd_amd import nets
    ctx = pc._ctx(precision)
    cfg = (77, 1000, 160, 2, 2, 64)  # two heads of 80, causal, 77 tokens
    ref = text_ref.synthetic_init_(text_ref.ClipTextModel(*cfg), seed=13).eval()
    for blk in ref.transformer.resblocks:
        blk.mlp.gelu = nn.GELU()
    dev = nets.ClipTextTower(ctx, config=cfg, activation="gelu")
    dev.load_clip_state_dict({k: v.to(pc.DEV) for k, v in ref.state_dict().items()})
    quick = nets.ClipTextTower(ctx, config=cfg)
    quick.load_clip_state_dict({k: v.to(pc.DEV) for k, v in ref.state_dict().items()})
    tok = text_ref.random_tokens(4, 77, cfg[1], [77, 5, 40, 13], seed=5)
    with th.no_grad():
        e = ref.double().encode_text(tok)
    got, other = dev.encode_text(tok.to(pc.DEV)), quick.encode_text(tok.to(pc.DEV))
    th.cuda.synchronize()
    _assert_all([pc.rec(f"gelu text[p{precision}]", got, e.float())])
    assert not pc.rec("quick_gelu on gelu weights", other, e.float())["ok"]


def test_setters_refuse_other_codes():
    from cgd_amd import lib, nets
    ctx = pc._ctx(1)
    vit = nets.ClipImageTower(ctx, config=(32, 8, 64, 1, 1, 48))
    txt = nets.ClipTextTower(ctx, config=(77, 100, 64, 1, 1, 48))
    for h, fn in ((vit.h, ctx.lib.cgd_vit_set_activation), (txt.h, ctx.lib.cgd_text_set_activation)):
        assert fn(h, 3) == 0 and fn(h, 2) == 0
        for bad in (0, 1, 4):
            assert fn(h, bad) == -2
            assert b"act" in ctx.lib.cgd_last_error(ctx.h)
    with pytest.raises(ValueError):
        nets.ClipImageTower(ctx, config=(32, 8, 64, 1, 1, 48), activation="relu")
    assert lib.CgdError  # (imported for the symbol check above)


def test_guided_step_on_a_gelu_tower(monkeypatch):
    """One ClipGuidance step, the way tests/step_checks.py builds its scenes, with an exact-GELU CLIP tower of head dim 80 (50 tokens: the
    fused d = 80 attention kernels) on both sides."""
    from cgd_amd import nets
    sc = step_checks.Scenario("mini", steps=1, vit_cfg=(56, 8, 160, 2, 2, 64))
    for blk in sc.ref_clip.visual.transformer.resblocks:
        blk.mlp.gelu = nn.GELU()
    monkeypatch.setattr(nets, "ClipImageTower", functools.partial(nets.ClipImageTower, activation="gelu"))
    recs = step_checks.compare(sc, 1, sc.run_oracle(), sc.run_device(1))
    _assert_all(recs)
