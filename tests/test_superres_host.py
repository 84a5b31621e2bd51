"""CPU tests of the super-resolution path: the float64 restatement of the conditioned stem (tests/superres_ref.py) against what upstream
runs in float32, the 6-channel parameter manifests against the oracle UNet, the `upsample=IMAGE` value of --init_image with its
refusals, the upsampler flag table, the state-dict cross-check, and the sampler's `low_res` plumbing with a recording library.  No GPU."""
import types

import pytest
import torch as th
import torch.nn.functional as F

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from cgd_amd import lib as L
from cgd_amd import nets
from tests import superres_ref as sr

RTOL, ATOL = 1e-3, 1e-4  # the project's literal tolerance (tests/parity_checks.py)

# (low h, low w) -> (frame H, frame W): integer and non-integer ratios, the published 64 -> 256 and 128 -> 512, a non-square frame,
# an upsample along one axis only, the one-pixel image, and equal sizes
SHAPES = [((8, 8), (32, 32)), ((5, 7), (9, 70)), ((64, 64), (256, 256)), ((128, 128), (512, 512)), ((64, 72), (256, 288)),
          ((3, 3), (7, 130)), ((1, 1), (6, 66)), ((9, 70), (9, 70))]


def _stem_weights(cout=32, seed=3):
    """fan-in scaled like the oracle's synthetic init"""
    g = th.Generator().manual_seed(seed)
    bound = (3.0 / 54) ** 0.5
    return (th.rand(cout, 6, 3, 3, generator=g) * 2 - 1) * bound, th.randn(cout, generator=g) * 0.02


@pytest.mark.parametrize("low_hw,hw", SHAPES)
def test_restatement_agrees_with_torch_interpolate_and_conv(low_hw, hw):
    g = th.Generator().manual_seed(11)
    low = th.rand(2, 3, *low_hw, generator=g) * 2 - 1
    x = th.randn(2, 3, *hw, generator=g)
    # the operator: float32 F.interpolate against the integer-geometry matrices in float64.  Values in [-1, 1] and convex weights: the
    # float32 result carries the rounding of two source coordinates, four products and three sums, a few ulp of 1.0 (1.2e-7 each):
    # 2e-6 is 16 of them
    up64 = sr.bilinear(low, *hw)
    up32 = F.interpolate(low, hw, mode="bilinear")
    assert (up32.double() - up64).abs().max().item() <= 2e-6
    if low_hw == hw:
        assert th.equal(up64, low.double())  # ratio 1: the conditioning passes through exactly
    w, b = _stem_weights()
    ref = sr.sr_stem(x, low, w, b)
    got = sr.sr_stem_torch32(x, low, w, b).double()
    assert ref.shape == (2, hw[0], hw[1], 32)
    assert bool(((got - ref).abs() <= ATOL + RTOL * ref.abs()).all())


def test_restatement_pads_the_concatenated_tensor_and_clamps_the_interpolation():
    """the two border rules on neighbouring pixels: with a constant low-res image the upsampled planes are that constant up to the
    frame's edge (clamped, not faded), and the stem's output at a corner pixel misses exactly the taps that fall outside the frame"""
    low = th.full((1, 3, 2, 2), 0.5)
    up = sr.bilinear(low, 6, 10)
    assert th.equal(up, th.full((1, 3, 6, 10), 0.5, dtype=th.float64))
    x = th.zeros(1, 3, 6, 10)
    w = th.zeros(4, 6, 3, 3)
    w[:, 3:] = 1.0
    y = sr.sr_stem(x, low, w)  # every output counts the in-frame taps of the three conditioning planes
    assert y[0, 0, 0, 0].item() == pytest.approx(3 * 4 * 0.5) and y[0, 0, 5, 0].item() == pytest.approx(3 * 6 * 0.5)
    assert y[0, 2, 5, 0].item() == pytest.approx(3 * 9 * 0.5)
    # a batch-1 image is shared by the batch
    assert sr.sr_input(th.zeros(3, 3, 6, 10), low).shape == (3, 6, 6, 10)


# ---- manifests and the flag table ---------------------------------------------------------------------------------------------------
def _upsampler_kwargs(size):
    from cgd import script_util
    return script_util.upsampler_unet_kwargs(script_util.upsampler_config(size))


@pytest.mark.parametrize("size", [256, 512])
def test_six_channel_manifest_matches_the_oracle_unet(size):
    """fails on a library whose UNet handle pins in_channels to 3: the manifest returns an error there"""
    from oracle import unet as ou
    kw = _upsampler_kwargs(size)
    assert kw["in_channels"] == 6 and kw["image_size"] == size and kw["channel_mult"] == (1, 1, 2, 2, 4, 4) and kw["model_channels"] == 192
    got = nets.manifest("unet", nets.UNet.make_config(**kw))
    with th.device("meta"):
        ref = {k: v.numel() for k, v in ou.UNetModel(**kw).state_dict().items()}
    assert dict(got) == ref and [k for k, _ in got] == list(ref)  # names, element counts and the upload order
    assert dict(got)["input_blocks.0.0.weight"] == 192 * 6 * 9
    heads = {256: dict(num_heads=4, num_head_channels=-1, attention_resolutions="32,16,8"),
             512: dict(num_heads=4, num_head_channels=64, attention_resolutions="32,16")}[size]
    assert {k: kw[k] for k in heads} == heads and kw["num_classes"] == 1000 and kw["out_channels"] == 6


def test_three_channel_manifest_is_unchanged_and_other_widths_are_refused():
    from cgd import script_util
    kw = script_util.unet_kwargs(script_util.model_config(256, True))
    got = dict(nets.manifest("unet", nets.UNet.make_config(**kw)))
    assert got["input_blocks.0.0.weight"] == 256 * 3 * 9 and sum(got.values()) == 553838086  # the published 256x256 checkpoint's size
    for bad in (0, 4, 9):
        with pytest.raises(ValueError):
            nets.manifest("unet", nets.UNet.make_config(**dict(kw, in_channels=bad)))


def test_upsampler_lookup_entries():
    from cgd import model_flags, script_util
    assert sorted(model_flags.UPSAMPLER_LOOKUP) == [256, 512]
    assert set(model_flags.DIFFUSION_LOOKUP) == {"cond", "uncond"}  # the reference's table stays as it is
    for size, small, name in ((256, 64, "64_256_upsampler.pt"), (512, 128, "128_512_upsampler.pt")):
        entry = model_flags.UPSAMPLER_LOOKUP[size]
        flags = entry["model_flags"]
        assert entry["filename"] == name and entry["url"].endswith("/" + name)
        assert (flags["large_size"], flags["small_size"]) == (size, small) and size == 4 * small
        assert flags["class_cond"] and flags["learn_sigma"] and flags["noise_schedule"] == "linear" and flags["diffusion_steps"] == 1000
        assert flags["num_channels"] == 192 and flags["num_res_blocks"] == 2 and flags["resblock_updown"] and flags["use_scale_shift_norm"]
        cfg = script_util.upsampler_config(size, timestep_respacing="ddim25")
        assert cfg["timestep_respacing"] == "ddim25" and cfg["diffusion_steps"] == 1000 and not cfg["rescale_timesteps"]
        assert nets.manifest("unet", nets.UNet.make_config(**script_util.upsampler_unet_kwargs(cfg)))  # a valid configuration


def test_state_dict_cross_check_names_the_first_mismatch():
    from cgd import script_util
    kw = dict(image_size=32, model_channels=32, num_res_blocks=1, attention_resolutions="16", channel_mult=(1, 2), num_classes=4,
              in_channels=6)
    specs = nets.manifest("unet", nets.UNet.make_config(**kw))
    from oracle import unet as ou
    sd = ou.UNetModel(**kw).state_dict()
    script_util.check_upsampler_state_dict(sd, specs)
    with pytest.raises(ValueError, match="lacks"):
        script_util.check_upsampler_state_dict({k: v for k, v in sd.items() if k != "out.2.bias"}, specs)
    with pytest.raises(ValueError, match="does not expect"):
        script_util.check_upsampler_state_dict(dict(sd, extra=th.zeros(1)), specs)
    with pytest.raises(ValueError, match="middle_block.1.qkv.weight"):
        script_util.check_upsampler_state_dict(dict(sd, **{"middle_block.1.qkv.weight": th.zeros(5)}), specs)
    three = ou.UNetModel(**dict(kw, in_channels=3)).state_dict()
    with pytest.raises(ValueError, match="input_blocks.0.0.weight"):
        script_util.check_upsampler_state_dict(three, specs)
    with pytest.raises(ValueError, match=r"\[ch0, 6, 3, 3\]"):  # the right element count in the wrong shape
        script_util.check_upsampler_state_dict(dict(sd, **{"input_blocks.0.0.weight": th.zeros(32, 3, 6, 3)}), specs)


# ---- 'upsample=IMAGE' ---------------------------------------------------------------------------------------------------------------
def test_split_init_upsample():
    from cgd import script_util as su
    assert su.split_init_upsample("upsample=a.png") == ("a.png", True)
    assert su.split_init_upsample("a.png") == ("a.png", False)
    assert su.split_init_upsample("dir/upsample=a.png") == ("dir/upsample=a.png", False)
    assert su.split_init_upsample("upsample=https://host/a.png") == ("https://host/a.png", True)
    with pytest.raises(ValueError, match="upsample=IMAGE"):
        su.split_init_upsample("upsample=")
    # next to the mask and the inversion prefix: 'upsample=IMAGE::MASK'
    image, mask = su.split_init_mask("upsample=a.png::m.png")
    assert (su.split_init_upsample(image), mask) == (("a.png", True), "m.png")
    assert su.check_init_upsample("upsample=a.png::m.png", 256, True) and su.check_init_upsample("upsample=a.png", 512, True)
    assert not su.check_init_upsample("a.png", 128, False) and not su.check_init_upsample("invert=a.png", 128, True)
    assert not su.check_init_upsample(None, 256, True) and not su.check_init_upsample("", 256, True)


@pytest.mark.parametrize("kw,match", [
    (dict(init_image="upsample=a.png", image_size=128), "image_size 256 or 512"),
    (dict(init_image="upsample=a.png", image_size=64), "image_size 256 or 512"),
    (dict(init_image="upsample=a.png", image_size=256, class_cond=False), "uncond"),
    (dict(init_image="upsample=invert=a.png", image_size=256, timestep_respacing="ddim50"), "cannot be combined"),
    (dict(init_image="invert=upsample=a.png", image_size=256, timestep_respacing="ddim50"), "cannot be combined"),
    (dict(init_image="invert=upsample=a.png::m.png", image_size=512, timestep_respacing="ddim50"), "cannot be combined"),
    (dict(init_image="upsample=", image_size=256), "upsample=IMAGE"),
])
def test_generator_refuses_before_anything_is_loaded(kw, match, monkeypatch):
    from cgd import cgd as mine
    from cgd import script_util

    def no_load(*a, **k):
        raise AssertionError("refused too late: something was being loaded")

    for name in ("download_guided_diffusion", "download_upsampler", "load_guided_diffusion", "load_upsampler", "fetch"):
        monkeypatch.setattr(script_util, name, no_load)
    monkeypatch.setattr(mine.clip_util, "load_clip", no_load)
    with pytest.raises(ValueError, match=match):
        next(mine.clip_guided_diffusion(prompts=["x"], device="cuda", **kw))


def test_cli_help_mentions_upsample_and_the_flag_set_is_what_it_was():
    from cgd import cgd as mine
    parser = mine.build_parser()
    init = next(a for a in parser._actions if a.dest == "init_image")
    assert "upsample=IMAGE" in init.help
    assert not any("upsample" in a.dest or "low_res" in a.dest for a in parser._actions)  # no new flag


def test_cond_fn_accepts_and_ignores_low_res():
    import inspect
    from cgd_amd.guidance import ClipGuidance
    p = inspect.signature(ClipGuidance.__call__).parameters
    assert list(p)[:5] == ["self", "x", "t", "out", "y"] and p["low_res"].default is None


# ---- sampler plumbing with a recording library --------------------------------------------------------------------------------------
class Recorder:
    def __init__(self, events):
        self.calls = events

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _rig(spec, with_setter=True):
    from cgd_amd import sampler
    events = []
    lib = Recorder(events)
    ctx = types.SimpleNamespace(lib=lib, h=1, check=lambda rc: None, device=0, stream=lambda: 0)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", spec, False))

    def forward(x, ts, y, out=None):
        events.append(("forward", (x.shape[0],)))
        return out

    model = types.SimpleNamespace(forward=forward, num_classes=5)
    if with_setter:
        model.set_low_res = lambda low: events.append(("set_low_res", (low,)))
    return smp, model, events


SHAPE = (2, 3, 4, 8)
LOOPS = {
    "p_sample": ("10", lambda smp, m, **kw: smp.p_sample_loop_progressive(m, SHAPE, clip_denoised=False, device="cpu", **kw)),
    "ddim": ("ddim10", lambda smp, m, **kw: smp.ddim_sample_loop_progressive(m, SHAPE, clip_denoised=False, device="cpu", **kw)),
    "plms": ("ddim10", lambda smp, m, **kw: smp.plms_sample_loop_progressive(m, SHAPE, clip_denoised=False, device="cpu", **kw)),
    "dpmpp": ("dpm10", lambda smp, m, **kw: smp.dpmpp_sample_loop_progressive(m, SHAPE, clip_denoised=False, device="cpu", **kw)),
    "reverse": ("ddim10", lambda smp, m, **kw: smp.ddim_reverse_sample_loop_progressive(m, th.zeros(SHAPE), device="cpu", **kw)),
}


@pytest.mark.parametrize("loop", sorted(LOOPS))
def test_low_res_is_set_once_per_loop_before_the_first_forward(loop):
    spec, run = LOOPS[loop]
    smp, model, events = _rig(spec)
    low = th.rand(2, 3, 1, 2)
    outs = list(run(smp, model, model_kwargs={"y": th.zeros(2, dtype=th.long), "low_res": low}))
    assert len(outs) >= 9
    names = [n for n, _ in events]
    assert names[0] == "set_low_res" and names.count("set_low_res") == 1 and names.count("forward") >= 9
    assert events[0][1][0] is low  # the tensor as given: the handle copies it
    # the launches of the loop are what they are without low_res
    smp0, model0, events0 = _rig(spec, with_setter=False)
    list(run(smp0, model0, model_kwargs={"y": th.zeros(2, dtype=th.long)}))
    assert names[1:] == [n for n, _ in events0]


@pytest.mark.parametrize("loop", sorted(LOOPS))
def test_without_low_res_the_call_sequence_is_what_it_was(loop):
    spec, run = LOOPS[loop]
    smp, model, events = _rig(spec)  # a super-resolution model without the keyword: nothing is set
    list(run(smp, model, model_kwargs={"y": th.zeros(2, dtype=th.long)}))
    names = [n for n, _ in events]
    assert "set_low_res" not in names
    per_step = {"p_sample": ["forward", "cgd_pmv_blend", "cgd_sample_update"], "ddim": ["forward", "cgd_pmv_blend", "cgd_sample_update"],
                "dpmpp": ["forward", "cgd_pmv_blend", "cgd_dpmpp_update"], "reverse": ["forward", "cgd_ddim_reverse_update"]}
    if loop == "plms":  # the start step evaluates twice: predictor and corrector, one update launch each
        assert names == ["forward", "cgd_pmv_blend", "cgd_multistep_update"] * 11
    else:
        assert names == per_step[loop] * (9 if loop == "reverse" else 10)


def test_low_res_needs_a_model_that_takes_it():
    smp, model, events = _rig("ddim10", with_setter=False)
    with pytest.raises(ValueError, match="super-resolution model"):
        list(smp.ddim_sample_loop_progressive(model, SHAPE, clip_denoised=False, device="cpu", model_kwargs={"low_res": th.zeros(1, 3, 1, 2)}))
    assert not events


@pytest.mark.parametrize("rows", [[1], [0, 2]])
def test_under_sharding_a_rank_passes_its_own_rows(rows):
    smp, model, events = _rig("ddim10")
    smp.shard = (rows, 3)
    low = th.arange(3.0).view(3, 1, 1, 1).expand(3, 3, 1, 2).contiguous()
    shape = (len(rows), 3, 4, 8)
    list(smp.ddim_sample_loop_progressive(model, shape, clip_denoised=False, device="cpu", model_kwargs={"low_res": low}))
    assert events[0][0] == "set_low_res" and [n for n, _ in events].count("set_low_res") == 1
    assert th.equal(events[0][1][0], low[rows])
    # one image for the whole batch stays one image
    smp, model, events = _rig("ddim10")
    smp.shard = (rows, 3)
    list(smp.ddim_sample_loop_progressive(model, shape, clip_denoised=False, device="cpu", model_kwargs={"low_res": low[:1]}))
    assert th.equal(events[0][1][0], low[:1])


def test_low_res_reaches_a_python_cond_fn_in_the_model_kwargs():
    """upstream hands **model_kwargs to cond_fn: a user cond_fn sees low_res beside y"""
    smp, model, events = _rig("ddim10")
    seen = []

    def cond_fn(x, t, out, y=None, low_res=None):
        seen.append((y, low_res))
        return th.zeros_like(x)

    class Model:
        num_classes = 5
        set_low_res = staticmethod(model.set_low_res)

        def __call__(self, x, ts, y):
            return th.zeros(x.shape[0], 6, *x.shape[2:]) + 0 * x.sum()

    low, y = th.zeros(1, 3, 1, 2), th.zeros(2, dtype=th.long)
    next(smp.ddim_sample_loop_progressive(Model(), SHAPE, clip_denoised=False, device="cpu", cond_fn=cond_fn, cond_fn_with_grad=True,
                                          model_kwargs={"y": y, "low_res": low}))
    assert len(seen) == 1 and seen[0][0] is y and seen[0][1] is low


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entries_and_rejects_null_handles():
    handle = L.load()
    for name in ("cgd_op_sr_stem", "cgd_unet_set_low_res"):
        assert hasattr(handle, name) and name in L.EXPORTED_SYMBOLS
    assert handle.cgd_op_sr_stem(None, None, None, 1, 8, 8, None, None, None, 0, 1, 32, 32, 32, None) == -3
    assert handle.cgd_unet_set_low_res(None, None, 1, 8, 8, None) == -3
