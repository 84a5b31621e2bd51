"""CPU side of the value-regime family (tests/value_regime_checks.py): every magnitude in the case table is what the admissibility ladder gives
(fp32 PyTorch within 0.25 of the bound against float64; bf16x3 emulation of the attention products within 1.0), every case is admissible at its
magnitude, and every case IS in the regime it names.  Prints one line per case: magnitude, fp32 fraction, emulation fraction."""
import math

import pytest
import torch as th

from tests import value_regime_checks as vr


def _line(*a):
    print(" ".join(str(x) for x in a))


def _attn_all(cls, regime, gain=None):
    out = []
    for causal in (False, True):
        for sh in (vr.ATTN_CAUSAL_SHAPES if causal else vr.ATTN_SHAPES):
            f32, emu = vr.attn_fractions(sh, regime, gain, causal, emulate=cls == "x3")
            out.append((sh, causal, f32, emu))
    return out


def _attn_admissible(cls, regime, gain=None):
    return all(f <= vr.FP32_SHARE and (e is None or e <= vr.EMU_SHARE) for _, _, f, e in _attn_all(cls, regime, gain))


@pytest.mark.parametrize("cls", ["f32", "x3"])
def test_attention_gain_is_the_ladders_choice(cls):
    assert vr.choose(vr.GAIN_LADDER, lambda s: _attn_admissible(cls, "gain", s)) == vr.ATTN_GAIN[cls]


@pytest.mark.parametrize("cls", ["f32", "x3"])
@pytest.mark.parametrize("regime", vr.ATTN_REGIMES)
def test_attention_cases_are_admissible(cls, regime):
    gain = vr.ATTN_GAIN[cls] if regime == "gain" else None
    for sh, causal, f32, emu in _attn_all(cls, regime, gain):
        _line(f"attention[{cls}]", "causal" if causal else "", sh, regime, "" if gain is None else f"gain {gain}", f"fp32 {f32:.3f}",
              "" if emu is None else f"bf16x3 emulation {emu:.3f}")
        assert f32 <= vr.FP32_SHARE and (emu is None or emu <= vr.EMU_SHARE)


@pytest.mark.parametrize("cls", ["f32", "x3"])
def test_attention_gain_case_at_one_head_of_512_channels_is_admissible(cls):
    for sh in vr.ATTN_GAIN_ONLY:
        f32, emu = vr.attn_fractions(sh, "gain", vr.ATTN_GAIN[cls], False, emulate=cls == "x3")
        _line(f"attention[{cls}]", sh, f"gain {vr.ATTN_GAIN[cls]} (gain case only)", f"fp32 {f32:.3f}", "" if emu is None else f"bf16x3 emulation {emu:.3f}")
        assert f32 <= vr.FP32_SHARE and (emu is None or emu <= vr.EMU_SHARE)
        assert vr.attn_class(1, {}, sh[3]) == "x3" and vr.attn_class(1, {"CGD_ATTN_X3": "0"}, sh[3]) == "x3" and vr.attn_class(0, {}, sh[3]) == "f32"


def test_attention_cases_left_out_of_bf16x3_contexts_do_fail_the_emulation():
    for shape, regime, kind in vr.ATTN_X3_LEFT_OUT:
        c = vr.attn_case(shape, regime)
        dout, gr, sd = c["bwd"][kind]
        _, ge = vr.attn_emulate_x3(c["q"], c["k"], c["v"], vr._heads(dout, shape))
        worst = max(vr.frac(a * sd, b * sd) for a, b in zip(ge, vr.attn_unpack_grad(gr, shape)))
        _line("left out of bf16x3 contexts:", shape, regime, kind, f"bf16x3 emulation {worst:.3f}")
        assert worst > vr.EMU_SHARE


@pytest.mark.parametrize("causal", [False, True])
def test_attention_cases_are_in_their_regime(causal):
    for sh in (vr.ATTN_CAUSAL_SHAPES if causal else vr.ATTN_SHAPES):
        nb, heads, T, d, _ = sh
        # logits of 15 and more; peaked (at least half the rows one-hot to 0.9) where ATTN_PEAKED says so
        for cls in ("f32", "x3"):
            q, k, v, _ = vr.attn_qkv(sh, "gain", vr.ATTN_GAIN[cls], causal)
            s, p = vr.attn_probs(q, k, causal)
            assert s[th.isfinite(s)].abs().max() >= 15, (sh, cls)
            if "gain" in vr.ATTN_PEAKED[cls]:
                assert (p.max(-1).values >= 0.9).double().mean() >= 0.5, (sh, cls)
        q, k, v, dom = vr.attn_qkv(sh, "planted", None, causal)
        s, p = vr.attn_probs(q, k, causal)
        top2 = s.topk(2, dim=-1)
        rows = th.arange(1 if causal else 0, T)  # (causal row 0 has one key)
        assert bool((top2.indices[..., 0] == dom)[..., rows].all()), sh
        margin = (top2.values[..., 0] - top2.values[..., 1])[..., rows]
        assert margin.min() >= 15 or (causal and (margin >= 15).double().mean() >= 0.9), (sh, margin.min())
        assert (p.max(-1).values >= 0.9).double().mean() >= 0.5
        if not causal:  # key 0, the last valid key and a key in each of the flash forward's four key partitions (where T has them)
            pos = vr.planted_positions(T)
            assert pos[:2] == [0, T - 1] and {(x // 32) % 4 for x in pos} >= set(range(min(4, (T + 31) // 32)))
            assert set(dom.tolist()) == set(pos)
        for regime, sign in (("ascending", 1), ("descending", -1)):
            q, k, v, _ = vr.attn_qkv(sh, regime, None, causal)
            plant = (q[..., :1, :vr.NRES].double() @ k[..., :vr.NRES].double().transpose(-1, -2))[..., 0, :] / math.sqrt(d)
            step = plant[..., 32::32] - plant[..., :-32:32]
            assert bool((sign * step > 1).all()), (sh, regime)  # every 32-key block moves the planted term by more than 1
        q, k, v, _ = vr.attn_qkv(sh, "offset", None, causal)
        off = (q[..., :vr.NRES].double() @ k[..., :vr.NRES].double().transpose(-1, -2)) / math.sqrt(d)  # the planted part of the logits
        assert 100 <= off.min() == off.max() <= 200, (sh, off.min(), off.max())  # one common term, beyond the 88.7 where __expf overflows
        for t in (q, k):  # the term is built from values bf16 holds exactly
            assert th.equal(t[..., :vr.NRES].bfloat16().float(), t[..., :vr.NRES])
        q, k, v, _ = vr.attn_qkv(sh, "identical", None, causal)
        _, p = vr.attn_probs(q, k, causal)
        expect = 1.0 / (th.arange(T) + 1.0).double() if causal else th.full((T,), 1.0 / T, dtype=th.float64)
        live = th.ones(T, T, dtype=th.bool).tril() if causal else th.ones(T, T, dtype=th.bool)
        assert th.allclose(p[..., live], expect[:, None].expand(T, T)[live], rtol=1e-9, atol=0), sh


def test_groupnorm_cases():
    pick = vr.choose(vr.OUTLIER_LADDER, lambda o: all(vr.gn_fraction(sh, rg, o) <= vr.FP32_SHARE for sh in vr.GN_SHAPES
                                                      for rg in vr.GN_OUTLIER_REGIMES))
    assert pick == vr.GN_OUTLIER
    assert vr.choose(vr.GN_MEAN_LADDER, lambda m: all(vr.gn_fraction(sh, "mean", m) <= vr.FP32_SHARE for sh in vr.GN_SHAPES)) == vr.GN_MEAN
    for sh, rg, mag in vr.gn_cases():
        f32 = vr.gn_fraction(sh, rg, mag)
        _line("groupnorm", sh, rg, "" if mag is None else f"magnitude {mag:g}", f"fp32 {f32:.3f}")
        assert f32 <= vr.FP32_SHARE
        B, HW, C, _, _, path = sh
        cpg = C // 32
        x = vr.gn_input(sh, rg, mag)
        xg = x.double().reshape(B, HW, 32, cpg)
        if rg in ("outlier-first-pixel", "outlier-first-channel"):
            for grp in range(0, 32, 2):
                p, c = vr.gn_shift_index(sh, grp)
                big = xg[:, :, grp].abs() == mag
                assert bool(big[:, p].all() if rg == "outlier-first-pixel" else big[:, p:p + 8, 0].all())
                assert int(big.sum()) == B * (cpg if rg == "outlier-first-pixel" else 8)
        elif rg.startswith("outlier"):  # the outlier sits at the documented shift element of its kernel (or, the control, does not)
            for grp in range(0, 32, 2):
                p, c = vr.gn_shift_index(sh, grp)
                assert (p, c) == ((3 * vr.gn_pick_chunk(HW, B), grp * cpg) if path == "chunked" else (0, grp * cpg))
                assert p % vr.gn_pick_chunk(HW, B) == 0 and p < HW
                at_shift = bool((x[:, p, c].abs() == mag).all())
                assert at_shift == (rg == "outlier-at-shift")
                assert int((xg[:, :, grp].abs() == mag).sum()) == B  # one outlier per (sample, group) ...
                assert int((xg[:, :, grp + 1].abs() > 10).sum()) == 0  # ... ordinary groups beside them
        elif rg in ("mean", "mean1e3-stats"):
            assert abs(xg.mean().item()) / xg.std().item() >= 0.9 * mag
        elif rg == "constant":
            var = xg.permute(0, 2, 1, 3).reshape(B, 32, -1).var(-1, unbiased=False)
            assert bool((var[:, [0, 1, 5]] == 0).all()) and bool((var[:, [2, 3, 4]] > 0.5).all())
        elif rg == "sigma1e-3":
            assert 0.5e-3 < xg.std().item() < 2e-3
    assert {sh[5] for sh in vr.GN_SHAPES} == {"cached", "streaming", "scalar", "scalar-streaming", "chunked"}


def test_groupnorm_shapes_select_the_kernels_they_name():
    """norm.hip launch_gn_small_fwd: float4 accesses iff 4 | channels per group; the slab is register-cached iff HW <= 8 * (1024 >> lg)"""
    for B, HW, C, _, _, path in vr.GN_SHAPES:
        cpg = C // 32
        v4 = cpg % 4 == 0
        cq = cpg // 4 if v4 else cpg
        lg = max(cq - 1, 0).bit_length()
        cached = HW <= 8 * (1024 >> lg)
        want = "chunked" if HW > 1024 else {(True, True): "cached", (True, False): "streaming", (False, True): "scalar",
                                            (False, False): "scalar-streaming"}[(v4, cached)]
        assert want == path, (B, HW, C, want, path)


def test_layernorm_cases():
    pick = vr.choose(vr.OUTLIER_LADDER, lambda o: all(vr.ln_fraction(sh, "outlier-channels", o) <= vr.FP32_SHARE for sh in vr.LN_SHAPES))
    assert pick == vr.LN_OUTLIER
    for sh, rg, mag in vr.ln_cases():
        f32 = vr.ln_fraction(sh, rg, mag)
        _line("layernorm", sh, rg, "" if mag is None else f"magnitude {mag:g}", f"fp32 {f32:.3f}")
        assert f32 <= vr.FP32_SHARE
        x = vr.ln_input(sh, rg, mag)
        if rg == "outlier-channels":
            big = (x.abs() >= 100 * 1.5).sum(-1)
            assert bool((big == 3).all())
        elif rg == "row-offset":
            assert (x.mean(-1).abs() / x.std(-1)).max() >= 30
        else:
            assert int((x.var(-1, unbiased=False) == 0).sum()) == 2


def test_activation_cases():
    for kind, k in vr.ACT_KINDS.items():
        f32 = vr.act_fraction(kind)
        u = vr.act_grid(kind)
        _line("activation kind", kind, f"|k u| up to {(k * u.abs()).max():.0f}", f"fp32 {f32:.4f}")
        assert f32 <= vr.FP32_SHARE
        ku = (k * u.double())
        for side in (1, -1):  # both sides of the __expf overflow, on both signs
            assert bool(((side * ku > 80) & (side * ku < 88.7)).any()) and bool((side * ku > 88.7).any())
        for v in (0.0, 1e-30, -1e-30, 1e-6, -1e-6):
            assert bool((u == th.tensor(v, dtype=th.float32)).any())
        for v in vr.ACT_KU:
            assert bool(((ku.abs() - v).abs() < 1e-3).any())


def test_spherical_loss_cases():
    import torch.nn.functional as F
    for sh in vr.SPH_SHAPES:
        f32 = vr.sph_fraction(sh)
        _line("spherical loss", sh, vr.SPH_ROWS, f"fp32 {f32:.4f}")
        assert f32 <= vr.FP32_SHARE
        cutn, B, P, D = sh
        emb, tg = vr.sph_input(sh)
        e = emb.double().view(cutn, B, D)
        dist = (F.normalize(e, dim=-1) - F.normalize(tg[0].double(), dim=-1)).norm(dim=-1)
        assert th.allclose(dist[0], th.tensor(0.05).double(), rtol=1e-3) and th.allclose(dist[1], th.tensor(1.95).double(), rtol=1e-3)
        assert th.allclose(e[2].norm(dim=-1), th.tensor(1e-3).double(), rtol=1e-4) and th.allclose(e[3].norm(dim=-1), th.tensor(1e3).double(), rtol=1e-4)
        assert bool(((dist[4:] > 1.2) & (dist[4:] < 1.6)).all())


def test_fused_groupnorm_silu_conv_staging_cases():
    for sh in vr.WSTAGE_SHAPES:
        f32, emu = vr.wstage_fractions(sh)
        u = vr.wstage_case(sh)["u"]
        _line("wconv fused GroupNorm + SiLU input", sh, f"u in [{u.min():.0f}, {u.max():.0f}]", f"fp32 {f32:.3f}", f"bf16x3 emulation {emu:.3f}")
        assert f32 <= vr.FP32_SHARE and emu <= vr.EMU_SHARE
        assert u.min() <= -vr.WSTAGE_SPAN and u.max() >= vr.WSTAGE_SPAN and 0.3 < vr.wstage_case(sh)["y"].std() < 3


@pytest.mark.parametrize("net", ["unet", "vit"])
def test_trained_like_network_gain_is_the_ladders_choice(net):
    """fp32 oracle against the float64 oracle, forward and input gradient; bf16x3 contexts are capped by the op-level emulation's gain"""
    fr = {}

    def ok(s):
        fr[s] = vr.net_fraction(net, s)
        return fr[s] <= vr.FP32_SHARE

    pick = vr.choose(vr.GAIN_LADDER, ok)
    _line(f"trained-like {net}:", " ".join(f"gain {s}: fp32 {f:.3f}" for s, f in fr.items()), "-> exact fp32", pick, ", bf16x3", min(pick, vr.ATTN_GAIN["x3"]))
    assert vr.NET_GAIN[net] == {"f32": pick, "x3": min(pick, vr.ATTN_GAIN["x3"])}


def test_trained_like_networks_reach_the_fused_forms():
    """the planted pre-activations are where the comments say, and the library's own launch plan puts the launches behind them on the kernels
    that fuse the activation (bf16x3 context, default knobs)"""
    import cgd_amd  # noqa: F401
    from cgd_amd import lib
    plans = vr.net_plans(lib.load())
    _line("launch plans [kernel, tile, slices, workgroups]:", plans)
    for k in ("vit c_fc", "vit c_proj backward"):
        assert plans[k][0] == 2 and plans[k][2] == 1, plans  # hgemm2, one slice: cgd_gemm_fuses_act
    assert plans["unet 64-channel conv, first level"][:2] == [1, 512] and vr.UNET_HW ** 2 >= 4096  # hconv2 at >= fuse_gn_min_m pixels
    assert plans["unet 128-channel conv, second level"][:2] == [1, 516]  # kconv: staged only under UNET_FUSE_ALL
    pre = vr.net_preacts("vit")
    for n, u in pre.items():
        ku = 1.702 * u[..., :4]
        _line("vit", n, "1.702 u of the planted columns:", [round(v, 1) for v in ku.mean((0, 1)).tolist()])
        assert bool((ku[..., 0] > 88.7).all()) and bool((ku[..., 1] < -88.7).all()) and bool((ku[..., 2].abs() > 50).all()) and bool((ku[..., 3].abs() > 50).all())
    pre = vr.net_preacts("unet")
    te = pre["time_embed.0"][0]
    _line("unet time_embed.0 planted outputs:", [round(v, 1) for v in te[[2, 7, 11]].tolist()])
    assert te[2] > 88.7 and te[7] < -88.7 and te[11] > 50
    gn = pre["first ResBlock norm"][0, [1, 9]]
    _line("unet first ResBlock norm, planted channels: u in", [round(gn.min().item(), 1), round(gn.max().item(), 1)])
    assert gn.min() <= -60 and gn.max() >= 60
