"""UNet hyper-parameters of the published guided-diffusion checkpoints, keyed like the reference's
DIFFUSION_LOOKUP['cond'|'uncond'][image_size] (/root/reference/data/diffusion_model_flags.py:1-120): a spec table —
it fixes every layer shape the HIP kernels must cover.  Built from a shared base plus per-checkpoint deltas."""

_OPENAI = "https://openaipublic.blob.core.windows.net/diffusion/jul-2021/"
_BASE = dict(diffusion_steps=1000, learn_sigma=True, noise_schedule="linear", num_channels=256, num_res_blocks=2,
             resblock_updown=True, use_fp16=True, use_scale_shift_norm=True)


def _entry(url, cond, size, **delta):
    flags = dict(_BASE, class_cond=cond, image_size=size, attention_resolutions="32,16,8")
    flags.update(delta)
    return {"url": url, "filename": url.rsplit("/", 1)[-1], "model_flags": flags}


_BIG = dict(attention_resolutions="32, 16, 8", rescale_timesteps=True, timestep_respacing="1000", num_head_channels=64)

DIFFUSION_LOOKUP = {
    "cond": {
        64: _entry(_OPENAI + "64x64_diffusion.pt", True, 64, dropout=0.1, noise_schedule="cosine", num_channels=192,
                   num_head_channels=64, num_res_blocks=3, use_new_attention_order=True),
        128: _entry(_OPENAI + "128x128_diffusion.pt", True, 128, num_heads=4),
        256: _entry(_OPENAI + "256x256_diffusion.pt", True, 256, num_head_channels=64),
        512: _entry(_OPENAI + "512x512_diffusion.pt", True, 512, **_BIG),
    },
    "uncond": {
        256: _entry(_OPENAI + "256x256_diffusion_uncond.pt", False, 256, num_head_channels=64),
        512: _entry("https://the-eye.eu/public/AI/models/512x512_diffusion_unconditional_ImageNet/"
                    "512x512_diffusion_uncond_finetune_008100.pt", False, 512, **_BIG),
    },
}


def _upsampler(large, small, **delta):
    url = _OPENAI + f"{small}_{large}_upsampler.pt"
    flags = dict(_BASE, class_cond=True, large_size=large, small_size=small, num_channels=192, channel_mult=(1, 1, 2, 2, 4, 4))
    flags.update(delta)
    return {"url": url, "filename": url.rsplit("/", 1)[-1], "model_flags": flags}


# guided-diffusion's super-resolution checkpoints (SuperResModel: a UNet with a 6-channel stem that reads x_t and the bilinearly upsampled
# low-resolution image), keyed by large_size.  A table of its own: DIFFUSION_LOOKUP mirrors the reference's table, which has no upsamplers.
# Written from memory of upstream's README flags and sr_create_model (channel_mult (1,1,2,2,4,4) at both sizes; the attention downsample
# rates are large_size // resolution).  No checkpoint was at hand to confirm it: script_util.check_upsampler_state_dict compares every
# shape of a loaded state dict with the manifest these flags give, and refuses a mismatch by name.
UPSAMPLER_LOOKUP = {
    256: _upsampler(256, 64, attention_resolutions="32,16,8", num_heads=4),
    512: _upsampler(512, 128, attention_resolutions="32,16", num_head_channels=64),
}

def _community(filename, **delta):
    # the classic architecture: conv down / upsampling (resblock_updown False) and, for most fine-tunes, additive timestep embeddings
    flags = dict(_BASE, class_cond=False, image_size=256, num_channels=128, num_res_blocks=2, attention_resolutions="16", num_heads=1,
                 num_head_channels=-1, resblock_updown=False, use_scale_shift_norm=False, use_new_attention_order=False)
    flags.update(delta)
    return {"filename": filename, "model_flags": flags}


# Community fine-tunes trained from improved-diffusion / guided-diffusion DEFAULTS, selected with '+model=FILE' on --timestep_respacing
# (script_util.split_model), keyed by file basename.  A hit supplies what no tensor shape shows: the head count.  Written from memory of the
# flags Disco Diffusion sets for these files; no checkpoint was at hand to confirm them, so only entries that can be stated with confidence
# are listed, and script_util.load_community_model compares every shape of a loaded state dict with the manifest these flags give and
# refuses a mismatch by name (as for UPSAMPLER_LOOKUP).  Other files load with '+model=FILE:heads=N' or ':head_channels=N'.
COMMUNITY_LOOKUP = {
    name: _community(name) for name in (
        "256x256_openai_comics_faces_by_alex_spirin_084000.pt",
        "pixel_art_diffusion_hard_256.pt",
        "pixel_art_diffusion_soft_256.pt",
    )
}

# upstream guided_diffusion.script_util.model_and_diffusion_defaults()
MODEL_AND_DIFFUSION_DEFAULTS = dict(
    image_size=64, num_channels=128, num_res_blocks=2, num_heads=4, num_heads_upsample=-1, num_head_channels=-1,
    attention_resolutions="16,8", channel_mult="", dropout=0.0, class_cond=False, use_checkpoint=False, use_scale_shift_norm=True,
    resblock_updown=False, use_fp16=False, use_new_attention_order=False, learn_sigma=False, diffusion_steps=1000,
    noise_schedule="linear", timestep_respacing="", use_kl=False, predict_xstart=False, rescale_timesteps=False,
    rescale_learned_sigmas=False)
