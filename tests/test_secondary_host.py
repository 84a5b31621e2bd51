"""Host side of the secondary-model guidance path (no GPU): the library's parameter manifest against the PyTorch restatement, the
`secondary=FILE` entry of the CLIP model list and its refusals, and the model-time mapping."""
import math

import numpy as np
import pytest

import cgd_amd  # noqa: F401
from cgd_amd import lib, nets
from tests import secondary_ref


def test_manifest_names_and_sizes_equal_the_reference_state_dict():
    want = {k: v.numel() for k, v in secondary_ref.SecondaryDiffusionImageNet2().state_dict().items()}
    got = nets.manifest("secondary")
    assert len(got) == len(dict(got)) == 2 * 24 + 1, "24 convolutions (weight + bias) and the Fourier frequencies, each listed once"
    assert dict(got) == want
    assert dict(got)["timestep_embed.weight"] == 8 and dict(got)["net.0.0.weight"] == 64 * 19 * 9 and dict(got)["net.4.weight"] == 3 * 64 * 9
    assert "net.2.main.3.main.3.main.3.main.3.main.4.0.weight" in dict(got)


def test_synthetic_state_dict_covers_the_manifest_and_loads_into_the_reference():
    from cgd_amd import synthetic
    sd = synthetic.secondary_state_dict(seed=5)
    assert {k: v.numel() for k, v in sd.items()} == dict(nets.manifest("secondary"))
    net = secondary_ref.build(sd)
    assert float(net.timestep_embed.weight.abs().max()) > 0
    sd2 = synthetic.secondary_state_dict(seed=5)
    assert all((sd[k] == sd2[k]).all() for k in sd), "seeded: the same weights on every rank and run"


def test_null_handles_are_rejected():
    handle = lib.load()
    assert handle.cgd_secondary_num_params(None) == -3
    assert handle.cgd_secondary_finalize(None) == -3
    handle.cgd_secondary_destroy(None)  # no-op
    assert handle.cgd_secondary_forward(None, None, None, 1, 32, 32, None, None) == -3
    assert handle.cgd_secondary_forward_blend(None, None, None, 1, 32, 32, 0.5, None, None, None) == -3
    assert handle.cgd_secondary_dgrad(None, None, None, None) == -3
    assert handle.cgd_secondary_debug_replay(None, None) == -3
    assert handle.cgd_secondary_head(None, None, None, None, 0.5, None, None, 1, 32, 32, None) == -3
    assert handle.cgd_secondary_combine(None, None, None, None, None, None, None, 1, 32, 32, 0.5, 0.8, 0.6, 1.0, 1.0, 0.0, None) == -3
    assert handle.cgd_op_secondary_pack(None, None, None, None, None, 1, 32, 32, None) == -3
    assert handle.cgd_op_bilinear_up2x(None, None, 4, None, 4, 1, 1, 1, 4, 0, None) == -3


def test_secondary_entry_of_the_clip_model_list():
    from cgd import clip_util
    assert clip_util.split_secondary("ViT-B/32") == (["ViT-B/32"], None)
    assert clip_util.split_secondary("RN50+ViT-L/14") == (["RN50", "ViT-L/14"], None)
    assert clip_util.split_secondary("ViT-B/32+secondary=ckpt/secondary_model_imagenet_2.pth") == (["ViT-B/32"], "ckpt/secondary_model_imagenet_2.pth")
    # position and spacing do not matter; it counts as no tower; ARCH=FILE entries stay tower entries
    assert clip_util.split_secondary(" secondary = s.pth + ViT-H-14=h.pt + RN50 ", 256) == (["ViT-H-14=h.pt", "RN50"], "s.pth")
    assert clip_util.split_secondary("ViT-B/32+secondary=s.pth", 256, 64, 32) == (["ViT-B/32"], "s.pth")
    # without a secondary model the image size is not its business
    assert clip_util.split_secondary("ViT-B/32", 250, 3, 5) == (["ViT-B/32"], None)


@pytest.mark.parametrize("name", ["secondary=s.pth", " secondary=s.pth ", "secondary=a.pth+secondary=b.pth", "ViT-B/32+secondary=", "+secondary=s.pth"])
def test_secondary_entry_refusals(name):
    from cgd import clip_util
    with pytest.raises(ValueError):
        clip_util.split_secondary(name, 256)


@pytest.mark.parametrize("size,ho,wo", [(250, 0, 0), (256, 16, 0), (256, 0, 48), (128, 1, 0)])
def test_image_size_that_is_no_multiple_of_32_is_refused(size, ho, wo):
    from cgd import clip_util
    with pytest.raises(ValueError, match="multiple of 32"):
        clip_util.split_secondary("ViT-B/32+secondary=s.pth", size, ho, wo)


def test_generator_refuses_before_anything_is_loaded(monkeypatch):
    """Both refusals come out of clip_guided_diffusion before a checkpoint, a CLIP tower or a context is touched."""
    from cgd import cgd as mine
    from cgd import clip_util, script_util

    def boom(*a, **k):
        raise AssertionError("something was loaded before the refusal")

    for mod, fn in ((clip_util, "load_clip"), (clip_util, "load_secondary"), (script_util, "load_guided_diffusion"),
                    (script_util, "download_guided_diffusion"), (script_util, "get_context")):
        monkeypatch.setattr(mod, fn, boom)
    with pytest.raises(ValueError, match="CLIP tower"):
        next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", clip_model_name="secondary=s.pth", image_size=256))
    with pytest.raises(ValueError, match="multiple of 32"):
        next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", clip_model_name="ViT-B/32+secondary=s.pth", image_size=256, height_offset=8))


def test_model_time_mapping_against_float64():
    """t = atan2(sigma, alpha) 2/pi, from the table row fac comes from: cos(t pi/2) = alpha and sin(t pi/2) = sigma to float64 rounding."""
    from cgd_amd import diffusion, guidance
    for schedule, spec in (("linear", "1000"), ("cosine", "ddim50"), ("linear", "25")):
        tables = diffusion.create_gaussian_diffusion(steps=1000, noise_schedule=schedule, timestep_respacing=spec)
        cg = guidance.ClipGuidance.__new__(guidance.ClipGuidance)
        cg.diffusion = tables
        for i in (0, 1, tables.num_timesteps // 2, tables.num_timesteps - 1):
            cg.current_timestep = i
            alpha, sigma, t = cg.secondary_level()
            a64, s64 = np.float64(tables.sqrt_alphas_cumprod[i]), np.float64(tables.sqrt_one_minus_alphas_cumprod[i])
            assert alpha == float(a64) and sigma == float(s64)
            assert t == secondary_ref.model_time(float(a64), float(s64)) == nets.SecondaryModel.model_time(a64, s64)
            assert 0.0 <= t <= 1.0
            assert abs(math.cos(t * math.pi / 2) - a64) < 1e-14 and abs(math.sin(t * math.pi / 2) - s64) < 1e-14
            # the same row as fac
            assert np.float32(sigma) == np.float32(tables.step_coef(i, i).fac)
    assert nets.SecondaryModel.model_time(1.0, 0.0) == 0.0 and nets.SecondaryModel.model_time(0.0, 1.0) == 1.0
