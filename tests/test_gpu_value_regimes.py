"""Op kernels on trained-network value ranges (pytest -m gpu): peaked / shifted / uniform softmaxes on every attention kernel selection,
GroupNorm and LayerNorm with outliers (also where the kernels take their variance shift from), |mean| >> sigma and constant groups, the
activations on both sides of the __expf overflow, the spherical loss near 0 and near pi — against float64 at the strict criterion of
test_gpu_parity.py (tests/value_regime_checks.py holds the case tables and the admissibility rule that sets each magnitude)."""
import pytest

from tests import value_regime_checks as vr
from tests.test_gpu_parity import _assert_all

pytestmark = pytest.mark.gpu


def _strict(recs):
    assert recs and not any(r.get("vacuous") for r in recs), [r["name"] for r in recs if r.get("vacuous")]
    for r in recs:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3e}")
    _assert_all(recs, allowed=("strict",))


@pytest.mark.parametrize("name,precision,envd", vr.ATTN_CONTEXTS, ids=[c[0].replace(" ", "-") for c in vr.ATTN_CONTEXTS])
def test_attention_value_regimes(name, precision, envd):
    """logit gain, planted dominant keys, monotone logits across key blocks, a common offset beyond exp's range, identical keys; forward, causal
    forward, backward with random and dominant-value-aligned seeds; every kernel selection test_gpu_parity.py grades"""
    _strict(vr.check_attn_regimes(name, precision, envd))


def test_groupnorm_value_regimes():
    _strict(vr.check_gn_regimes())


def test_layernorm_value_regimes():
    _strict(vr.check_ln_regimes())


def test_activation_value_regimes():
    _strict(vr.check_act_regimes())


def test_spherical_loss_value_regimes():
    _strict(vr.check_sph_regimes())


def test_fused_groupnorm_silu_conv_staging_value_regimes():
    _strict(vr.check_wstage_regimes())


@pytest.mark.parametrize("net,precision", [("unet", 0), ("unet", 1), ("vit", 0), ("vit", 1)])
def test_trained_like_network_value_regimes(net, precision):
    """ViT-B/32 (8 images: 400 token rows) and the `mini` UNet at 64 x 64 with trained-like synthetic weights (value_regime_checks.trained_like_),
    forward and input gradient against the FLOAT64 oracle."""
    recs, _ = vr.check_net_regimes(net, precision)
    _strict(recs)


def test_trained_like_unet_stages_groupnorm_silu_in_the_halo_convs():
    """The planted gamma / beta of the first ResBlock norm reach the conv kernels' staging loops, read back from the launch profile: with
    CGD_FUSE_GN=0 every GroupNorm materialises its output (8 bytes per element); the default context stages the >= 4096-pixel convs on hconv2 (fewer
    GroupNorm bytes, hconv2 launches); with the minimum lowered the <= 32 x 32 maps are staged by kconv too (fewer bytes again, kconv launches).
    All three are graded against the float64 oracle."""
    prof = {}
    for name, envd in (("off", {"CGD_FUSE_GN": "0"}), ("default", None), ("all", vr.UNET_FUSE_ALL)):
        recs, prof[name] = vr.check_net_regimes("unet", 1, envd)
        _strict(recs)
        print(name, "launches per kind", [p[2] for p in prof[name]], "GroupNorm bytes", prof[name][2][1])
    gn = {k: v[2][1] for k, v in prof.items()}
    assert gn["all"] < gn["default"] < gn["off"], gn
    assert prof["default"][1][2] >= 1 and prof["all"][4][2] >= 1, prof  # hconv2 launches, kconv launches


def test_trained_like_vit_runs_the_fused_quickgelu_gemms():
    """cgd_gemm_fuses_act (vit.hip) holds when the launcher's plan for the GEMM is hgemm2 in one slice: asked of the library itself"""
    import cgd_amd  # noqa: F401
    from cgd_amd import lib
    plans = vr.net_plans(lib.load())
    assert plans["vit c_fc"][0] == 2 and plans["vit c_fc"][2] == 1 and plans["vit c_proj backward"][0] == 2 and plans["vit c_proj backward"][2] == 1, plans
