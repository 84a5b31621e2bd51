"""CPU tests of the VGG Gram-matrix style loss: the closed-form tap gradient against autograd (fp64), the 'style=FILE[:SCALE]' value of
--image_prompts, and the C ABI's new entries."""
import os
import re

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib as L
from tests import style_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    from oracle import lpips_vgg as olp
    return olp.synthetic_init_(olp.LpipsVGG()).double().eval()


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def test_closed_form_tap_gradient_equals_autograd_per_tap():
    """dL/dA_k = lambda_k 4 / (C_k N_k) A_k (G_k - G_k(style)) against fp64 autograd of the loss w.r.t. each tap, per tap, with unequal
    weights and a style image of another size than the input."""
    orc = _oracle()
    g = th.Generator().manual_seed(5)
    style = (th.rand(1, 3, 48, 32, generator=g) * 2 - 1).double()
    x = th.tanh(th.randn(2, 3, 32, 48, generator=g)).double()
    weights = (1.0, 0.5, 2.0, 1.5, 0.25)
    grams = style_ref.style_grams(orc, style)
    with th.no_grad():
        taps = [t.clone().requires_grad_() for t in orc.features(x)]
    style_ref.tap_losses(taps, grams, weights).sum().backward()
    for k in range(5):
        want = taps[k].grad
        got = style_ref.closed_form_tap_grad(taps[k].detach(), grams[k], weights[k])
        assert want.abs().max() > 0
        assert (got - want).abs().max() <= 1e-12 * want.abs().max(), (k, float((got - want).abs().max()), float(want.abs().max()))


def test_gram_shapes_self_loss_and_zero_weight_taps():
    orc = _oracle()
    g = th.Generator().manual_seed(6)
    style = (th.rand(1, 3, 32, 32, generator=g) * 2 - 1).double()
    grams = style_ref.style_grams(orc, style)
    assert [tuple(m.shape) for m in grams] == [(64, 64), (128, 128), (256, 256), (512, 512), (512, 512)]
    # the loss of the style image itself is zero; a tap with weight 0 adds nothing
    x = th.tanh(th.randn(1, 3, 32, 32, generator=g)).double()
    with th.no_grad():
        assert float(style_ref.style_loss(orc, style, grams).abs().max()) == 0.0
        full = style_ref.style_loss(orc, x, grams, (1, 1, 1, 1, 1))
        part = style_ref.style_loss(orc, x, grams, (1, 1, 1, 1, 0))
        only4 = style_ref.style_loss(orc, x, grams, (0, 0, 0, 0, 1))
    assert th.allclose(full, part + only4, rtol=1e-12, atol=0)


# ---- the 'style=FILE[:SCALE]' value ----------------------------------------------------------------------------------------------------
def test_style_entry_is_split_off_the_image_prompts():
    from cgd import script_util
    assert script_util.split_style_prompts(["a.png:2", "style=a.png:3000", "b.png"]) == (["a.png:2", "b.png"], ("a.png", 3000.0))
    assert script_util.split_style_prompts(["style=dir/van gogh.png"]) == ([], ("dir/van gogh.png", 1.0))
    assert script_util.split_style_prompts(["style=https://example.org/s.png:2.5"]) == ([], ("https://example.org/s.png", 2.5))
    assert script_util.split_style_prompts(["style=https://example.org/s.png"]) == ([], ("https://example.org/s.png", 1.0))
    assert script_util.split_style_prompts(["a.png"]) == (["a.png"], None)
    assert script_util.split_style_prompts([]) == ([], None)
    assert script_util.split_style_prompts(["style=a.png:3000"], 256, 320) == ([], ("a.png", 3000.0))


@pytest.mark.parametrize("bad", [["style="], ["style=:3"], ["style=a.png:0"], ["style=a.png:-2"], ["style=a.png:nan"],
                                 ["style=a.png:1", "style=b.png:1"], ["style=a.png", "x.png", "style=a.png"]])
def test_malformed_style_entries_are_refused(bad):
    from cgd import script_util
    with pytest.raises(ValueError):
        script_util.split_style_prompts(bad)


def test_style_entry_needs_frame_sides_that_are_multiples_of_16():
    from cgd import script_util
    with pytest.raises(ValueError, match="multiples of 16"):
        script_util.split_style_prompts(["style=a.png"], 256, 264)
    assert script_util.split_style_prompts(["a.png"], 256, 264) == (["a.png"], None)  # only a style entry asks for it


def test_generator_refuses_a_malformed_style_entry_before_anything_is_loaded(tmp_path):
    from cgd import cgd
    for bad in (["style="], ["style=a.png:0"], ["style=a.png", "style=b.png"]):
        gen = cgd.clip_guided_diffusion(prompts=["a cat"], image_prompts=bad, device="cuda", checkpoints_dir=str(tmp_path / "none"),
                                        prefix_path=tmp_path / "out")
        with pytest.raises(ValueError, match="style="):
            next(gen)
        assert not (tmp_path / "none").exists() and not (tmp_path / "out").exists()


def test_style_entry_stays_out_of_the_weight_rules():
    """The zero-sum check of the direction prompts counts prompt weights only: a style entry's SCALE is no prompt weight."""
    from cgd import script_util
    prompts = ["a cat=>a dog:1", "a house:-1"]
    with pytest.raises(RuntimeError, match="sum to 0"):
        script_util.direction_prompts(prompts, [], init_image="i.png")
    with pytest.raises(RuntimeError, match="sum to 0"):  # SCALE 5 does not rescue a zero sum ...
        script_util.direction_prompts(prompts, ["style=s.png:5"], init_image="i.png")
    ok = ["a cat=>a dog:1", "a house:-0.5"]
    assert script_util.direction_prompts(ok, ["style=s.png:-0.5"], init_image="i.png")[0] == ("a cat", "a dog")  # ... nor cause one
    # and a style file whose name holds '=>' is no malformed direction prompt
    assert script_util.direction_prompts(ok, ["style=a=>b.png:2"], init_image="i.png")[1] is None


def test_guidance_normalises_prompt_weights_without_the_style_scale():
    """ClipGuidance takes the style scale beside the prompt weights, never among them (host logic only: no launch is made here)."""
    import types
    from cgd_amd import guidance as dg
    tower = types.SimpleNamespace(out_dim=8, input_resolution=32, patch=8)
    diffusion = types.SimpleNamespace(num_timesteps=10)
    handle = object()
    style = th.zeros(1, 3, 32, 32)
    guid = dg.ClipGuidance(None, None, tower, diffusion, th.randn(2, 8), [0.75, 0.25], 4, lpips=handle, style_tensor=style, style_scale=3000.0)
    assert guid.weights.tolist() == [0.75, 0.25] and guid.style is handle and guid.style_scale == 3000.0 and guid.lpips is None
    assert guid.style_weights == (1, 1, 1, 1, 0) and not guid.no_clip
    only = dg.ClipGuidance(None, None, tower, diffusion, None, None, 4, lpips=handle, style_tensor=style, style_scale=2.0)
    assert only.no_clip and only.weights.numel() == 0 and only.targets_list[0].shape == (0, 8)
    plain = dg.ClipGuidance(None, None, tower, diffusion, th.randn(2, 8), [0.75, 0.25], 4)
    assert plain.style is None and not plain.no_clip
    with pytest.raises(ValueError, match="lpips"):
        dg.ClipGuidance(None, None, tower, diffusion, th.randn(2, 8), [1.0, 1.0], 4, style_tensor=style, style_scale=1.0)
    with pytest.raises(ValueError, match="positive"):
        dg.ClipGuidance(None, None, tower, diffusion, th.randn(2, 8), [1.0, 1.0], 4, lpips=handle, style_tensor=style, style_scale=-1.0)
    with pytest.raises(ValueError, match="target embeddings"):
        dg.ClipGuidance(None, None, tower, diffusion, None, None, 4)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("cgd_op_gram", "cgd_lpips_set_style", "cgd_lpips_style_loss_grad")


def test_header_declares_and_library_exports_the_new_symbols():
    src = open(os.path.join(ROOT, "include", "cgd_mi355x.h")).read()
    handle = L.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/cgd_mi355x.h"
        assert hasattr(handle, name), f"{name} is not exported"
        assert name in L._SIGS, f"{name} has no ctypes signature in lib.py"


def test_null_handles_are_rejected():
    handle = L.load()
    assert handle.cgd_lpips_set_style(None, None, 16, 16, None, None) == -3
    assert handle.cgd_lpips_style_loss_grad(None, None, 1, 16, 16, 1.0, 1.0, None, None, None, 0, None) == -3
    assert handle.cgd_op_gram(None, None, 64, 1, 1, 64, 1.0, None, None) == -3
