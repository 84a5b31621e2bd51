"""Host-side checks of the classic UNet architecture (conv down / upsampling, additive timestep embeddings): the reference module against the
trusted oracle, the library's parameter manifests against the reference's state dicts, the stride-2 conv's accept predicate, the flags read
from a state dict's shapes, the '+model=' suffix and the community table.  No GPU."""
import ctypes as C

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib as L
from cgd_amd import nets
from cgd_amd.cgd import script_util
from cgd_amd.cgd.model_flags import COMMUNITY_LOOKUP, DIFFUSION_LOOKUP, UPSAMPLER_LOOKUP
from oracle import unet as oracle_unet
from tests import classic_unet_ref as R


def test_reference_with_both_switches_on_is_the_oracle_network():
    """the anchor: on one state dict, ClassicUNetModel(resblock_updown=True, use_scale_shift_norm=True) computes oracle/unet.py's outputs"""
    cfg = dict(R.TINY, num_classes=10)
    a = oracle_unet.synthetic_init_(oracle_unet.UNetModel(**cfg), seed=5)
    b = R.ClassicUNetModel(**cfg)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    g = th.Generator().manual_seed(3)
    x, t, y = th.randn(2, 3, 32, 32, generator=g), th.tensor([7.0, 420.0]), th.tensor([3, 9])
    with th.no_grad():
        assert th.equal(a(x, t, y), b(x, t, y))


@pytest.mark.parametrize("updown,film", R.FLAG_COMBOS)
@pytest.mark.parametrize("cfg", [R.TINY, R.COMICS], ids=["tiny", "comics_faces"])
def test_manifest_equals_the_reference_state_dict(cfg, updown, film):
    with th.device("meta"):
        ref = R.ClassicUNetModel(**cfg, resblock_updown=updown, use_scale_shift_norm=film)
    want = [(k, v.numel()) for k, v in ref.state_dict().items()]
    got = nets.manifest("unet", nets.UNet.make_config(**cfg, resblock_updown=updown, use_scale_shift_norm=film))
    assert got == want
    if not updown:
        assert any(n.endswith(".0.op.weight") for n, _ in got) and any(n.endswith(".conv.weight") and n.startswith("output_blocks") for n, _ in got)


def test_zeroed_new_fields_give_the_old_manifest():
    """a caller that builds the struct without the two new fields (memset, or lib.UNetConfig() and the old assignments) gets the published
    architecture: the manifest of oracle/unet.py's network, names, order and sizes"""
    kw = dict(image_size=64, model_channels=64, num_res_blocks=1, attention_resolutions="32", channel_mult=(1, 2), num_classes=1000, num_heads=4)
    via_make = nets.UNet.make_config(**kw)
    assert (via_make.classic_resample, via_make.additive_emb) == (0, 0)
    raw = L.UNetConfig()
    C.memset(C.byref(raw), 0, C.sizeof(raw))
    raw.image_size, raw.model_channels, raw.num_res_blocks, raw.n_mult = 64, 64, 1, 2
    raw.channel_mult[0], raw.channel_mult[1] = 1.0, 2.0
    raw.n_att, raw.num_classes, raw.num_heads, raw.num_head_channels = 1, 1000, 4, -1
    raw.attention_ds[0] = 2
    raw.in_channels, raw.out_channels = 3, 6
    assert bytes(raw) == bytes(via_make)
    with th.device("meta"):
        want = [(k, v.numel()) for k, v in oracle_unet.UNetModel(**kw).state_dict().items()]
    assert nets.manifest("unet", raw) == want == nets.manifest("unet", via_make)
    bad = nets.UNet.make_config(**kw)
    bad.classic_resample = 2
    with pytest.raises(ValueError):
        nets.manifest("unet", bad)


def test_stride2_conv_accepts_what_it_documents():
    acc = L.load().cgd_op_conv3x3_s2_accepts
    # (dgrad, ld_in, ld_out, ldadd, B, H, W, Cin, Cout)
    assert acc(0, 128, 128, 0, 1, 2, 2, 128, 128) == 1
    assert acc(0, 96, 160, 0, 1, 4, 6, 96, 160) == 1
    assert acc(0, 192, 160, 0, 3, 6, 10, 128, 128) == 1
    assert acc(1, 160, 192, 0, 3, 6, 10, 128, 128) == 1 and acc(1, 160, 192, 132, 3, 6, 10, 128, 128) == 1
    assert acc(0, 128, 128, 0, 1, 256, 256, 128, 128) == 1 and acc(0, 512, 512, 0, 7, 16, 16, 512, 512) == 1
    for H, W in ((3, 4), (4, 5), (1, 2), (0, 4)):
        assert acc(0, 32, 32, 0, 1, H, W, 32, 32) == 0, (H, W)
    for ci, co in ((48, 32), (32, 16), (0, 32), (32, -32), (100, 100)):
        assert acc(0, max(ci, 4), max(co, 4), 0, 1, 4, 4, ci, co) == 0, (ci, co)
    assert acc(0, 130, 128, 0, 1, 4, 4, 128, 128) == 0 and acc(0, 128, 129, 0, 1, 4, 4, 128, 128) == 0  # strides that are no multiples of 4
    assert acc(1, 128, 128, 130, 1, 4, 4, 128, 128) == 0
    assert acc(0, 64, 128, 0, 1, 4, 4, 128, 128) == 0 and acc(1, 128, 128, 64, 1, 4, 4, 128, 128) == 0  # a stride below its channel count
    assert acc(0, 128, 128, 0, 0, 4, 4, 128, 128) == 0
    # byte extents: x of exactly 2^31 bytes is refused, one row of pixels less runs; likewise the written operand and `add`
    assert acc(0, 128, 128, 0, 1, 2048, 2048, 128, 128) == 0  # 2048 * 2048 * 128 * 4 = 2^31
    assert acc(0, 128, 128, 0, 1, 2048, 2046, 128, 128) == 1
    assert acc(1, 128, 128, 0, 1, 2048, 2048, 128, 128) == 0 and acc(1, 128, 128, 0, 1, 2046, 2048, 128, 128) == 1
    # 512 rows: the last one starts at 511 * ld * 4 bytes, below 2^31 at ld = 2^20 and beyond it at ld = 2^20 + 4096
    far = (1 << 20) + 4096
    assert acc(1, 32, 32, far, 1, 16, 32, 32, 32) == 0 and acc(1, 32, 32, 1 << 20, 1, 16, 32, 32, 32) == 1
    assert acc(0, far, 32, 0, 1, 16, 32, 32, 32) == 0 and acc(0, 1 << 20, 32, 0, 1, 16, 32, 32, 32) == 1
    assert acc(0, 32, (1 << 22) + (1 << 16), 0, 1, 16, 32, 32, 32) == 0 and acc(0, 32, 1 << 22, 0, 1, 16, 32, 32, 32) == 1  # (128 rows of y)
    assert acc(0, 8192, 8192, 0, 1, 2, 2, 8192, 8192) == 0  # the weight: 9 * 8192^2 * 4 bytes


def _meta_state_dict(**kw):
    with th.device("meta"):
        return R.ClassicUNetModel(**kw).state_dict()


def _published():
    """(name, the flags of the table, image size, the reference's constructor arguments)"""
    out = []
    for cond in DIFFUSION_LOOKUP:
        for size, info in DIFFUSION_LOOKUP[cond].items():
            cfg = script_util.model_config(size, cond == "cond")
            out.append((info["filename"], cfg, size, script_util.unet_kwargs(cfg)))
    for size, info in UPSAMPLER_LOOKUP.items():
        cfg = script_util.upsampler_config(size)
        out.append((info["filename"], cfg, size, script_util.upsampler_unet_kwargs(cfg)))
    for name, info in COMMUNITY_LOOKUP.items():
        cfg = script_util.community_flags((name, None, None, False), info["model_flags"]["image_size"], info["model_flags"]["class_cond"])
        out.append((name, cfg, cfg["image_size"], script_util.community_unet_kwargs(cfg)))
    return out


@pytest.mark.parametrize("name,cfg,size,kw", _published(), ids=[p[0] for p in _published()])
def test_flags_round_trip_through_a_state_dict(name, cfg, size, kw):
    kw = dict(kw)
    kw.setdefault("resblock_updown", cfg["resblock_updown"])
    kw.setdefault("use_scale_shift_norm", cfg["use_scale_shift_norm"])
    sd = _meta_state_dict(**kw)
    assert [(k, v.numel()) for k, v in sd.items()] == nets.manifest("unet", nets.UNet.make_config(**kw))
    got = script_util.unet_flags_from_state_dict(sd, size)
    assert got["num_channels"] == cfg["num_channels"] and got["num_res_blocks"] == cfg["num_res_blocks"]
    assert got["attention_resolutions"] == cfg["attention_resolutions"].replace(" ", "")
    assert tuple(got["channel_mult"]) == tuple(kw["channel_mult"] or nets.DEFAULT_CHANNEL_MULT[size])
    for key in ("resblock_updown", "use_scale_shift_norm", "class_cond", "learn_sigma"):
        assert got[key] == cfg[key], key
    assert got["in_channels"] == kw.get("in_channels", 3) and got["image_size"] == size


def test_community_table_holds_the_three_known_fine_tunes():
    for name in ("256x256_openai_comics_faces_by_alex_spirin_084000.pt", "pixel_art_diffusion_hard_256.pt", "pixel_art_diffusion_soft_256.pt"):
        f = COMMUNITY_LOOKUP[name]["model_flags"]
        assert (f["image_size"], f["num_channels"], f["num_res_blocks"], f["attention_resolutions"], f["num_heads"]) == (256, 128, 2, "16", 1)
        assert (f["use_scale_shift_norm"], f["resblock_updown"], f["learn_sigma"], f["noise_schedule"], f["class_cond"]) == (False, False, True, "linear", False)
        kw = script_util.community_unet_kwargs(script_util.community_flags((name, None, None, False), 256, False))
        assert kw == dict(R.COMICS, channel_mult=(1, 1, 2, 2, 4, 4), num_classes=None, num_head_channels=-1, use_new_attention_order=False,
                          out_channels=6, resblock_updown=False, use_scale_shift_norm=False)


def test_a_corrupted_state_dict_is_refused_by_the_name_of_its_tensor():
    kw = dict(R.TINY, resblock_updown=False, use_scale_shift_norm=False)
    good = dict(_meta_state_dict(**kw))
    flags = script_util.unet_flags_from_state_dict(good, 32)
    assert (flags["resblock_updown"], flags["use_scale_shift_norm"], flags["attention_resolutions"], flags["channel_mult"]) == (False, False, "16", (1, 2))

    def broken(name, shape=None):
        sd = dict(good)
        if shape is None:
            del sd[name]
        else:
            sd[name] = th.empty(shape, device="meta")
        return sd

    cases = [("time_embed.0.weight", None), ("time_embed.0.weight", (200, 64)), ("out.2.weight", (3, 64, 3, 3)), ("out.2.weight", (5, 64, 3, 3)),
             ("input_blocks.0.0.weight", (64, 4, 3, 3)), ("input_blocks.1.0.emb_layers.1.weight", (96, 256)),
             ("input_blocks.2.0.op.weight", (64, 32, 3, 3)), ("input_blocks.3.0.in_layers.2.weight", (96, 64, 3, 3)),
             ("input_blocks.1.0.in_layers.2.weight", None)]
    for name, shape in cases:
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            script_util.unet_flags_from_state_dict(broken(name, shape), 32)
    with pytest.raises(ValueError, match="learn_sigma"):
        script_util.unet_flags_from_state_dict(broken("out.2.weight", (3, 64, 3, 3)), 32)
    # a state dict that contradicts its table entry, a conditioning that disagrees, a missing head count
    name = "pixel_art_diffusion_hard_256.pt"
    with pytest.raises(ValueError, match="num_channels"):
        script_util.community_flags((name, None, None, False), 256, False, sd=_meta_state_dict(**dict(R.COMICS, model_channels=64, resblock_updown=False, use_scale_shift_norm=False)))
    with pytest.raises(ValueError, match="uncond"):
        script_util.community_flags((name, None, None, False), 256, True)
    with pytest.raises(ValueError, match="256 x 256"):
        script_util.community_flags((name, None, None, False), 128, False)
    with pytest.raises(ValueError, match="heads=N"):
        script_util.community_flags(("mine.pt", None, None, False), 32, False, sd=good)
    f = script_util.community_flags(("mine.pt", None, 32, True), 32, False, sd=good)
    assert (f["num_head_channels"], f["use_new_attention_order"], f["num_channels"], f["resblock_updown"]) == (32, True, 64, False)
    with pytest.raises(ValueError, match="expect"):
        script_util.check_state_dict({k: v for k, v in good.items() if k != "out.0.bias"}, nets.manifest("unet", nets.UNet.make_config(**kw)), "mine.pt")


def test_model_suffix_parser():
    sm = script_util.split_model
    assert sm("ddim100") == ("ddim100", None)
    assert sm("ddim100+model=a/b.pt") == ("ddim100", ("a/b.pt", None, None, False))
    assert sm("250+model=m.pt:heads=4") == ("250", ("m.pt", 4, None, False))
    assert sm("plms50+model=m.pt:head_channels=64:new_order") == ("plms50", ("m.pt", None, 64, True))
    assert sm("250+model=m.pt:new_order:heads=1") == ("250", ("m.pt", 1, None, True))
    # in combination: '+model=' comes off first, the others keep their own rules on what remains
    rest, spec = sm("dpm20+thr=0.995:1.5+windows=64:wrapx+model=pixel_art_diffusion_hard_256.pt")
    assert spec == ("pixel_art_diffusion_hard_256.pt", None, None, False)
    rest, win = script_util.split_windows(rest, 256, 0, 64)
    assert win == (64, "x", False) and script_util.split_threshold(rest) == ("dpm20", (0.995, 1.5))
    for bad in ("+model=m.pt", "250+model=", "250+model=:heads=4", "250+model=m.pt:heads=0", "250+model=m.pt:heads=x", "250+model=m.pt:heads=2:head_channels=64",
                "250+model=m.pt:heads=2:heads=2", "250+model=m.pt:order", "250+model=m.pt:new_order:new_order", "250+model=m.pt:heads=",
                "250+model=m.pt+windows=64", "250+model=m.pt+thr=0.9", "250+model=a.pt+model=b.pt"):
        with pytest.raises(ValueError, match=r"\+model="):
            sm(bad)
    # before anything is loaded: an unknown file without a head count, a known one at the wrong conditioning, 'upsample=' next to it
    with pytest.raises(ValueError, match="heads=N"):
        script_util.check_model(("mine.pt", None, None, False), 256, False)
    script_util.check_model(("dir/pixel_art_diffusion_soft_256.pt", None, None, False), 256, False)
    with pytest.raises(ValueError, match="uncond"):
        script_util.check_model(("pixel_art_diffusion_soft_256.pt", None, None, False), 256, True)
    with pytest.raises(ValueError, match="upsample="):
        script_util.check_model(("pixel_art_diffusion_soft_256.pt", None, None, False), 256, False, "upsample=a.png")


def test_synthetic_weights_take_table_names_only(monkeypatch):
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    with pytest.raises(ValueError, match="known checkpoints"):
        script_util.check_model(("mine.pt", 4, None, False), 256, False)
    script_util.check_model(("pixel_art_diffusion_hard_256.pt", None, None, False), 256, False)


def test_animate_plan_check_takes_a_model_spacing():
    """the animation driver counts its steps from the spacing without its suffixes: '+model=' comes off there too, alone and behind
    '+thr=' / '+windows='"""
    from cgd_amd import animate as an
    for spacing in ("ddim100+model=pixel_art_diffusion_hard_256.pt", "dpm20+thr=0.995+windows=128:wrapx+model=mine.pt:heads=4:new_order"):
        frames, plan = an._check(3, "wrap", "bicubic", 0.6, 1500, 0.0, None, dict(timestep_respacing=spacing, prompts=["a"]))
        assert frames == 3 and plan == {}
    with pytest.raises(ValueError, match=r"\+model="):
        an._check(3, "wrap", "bicubic", 0.6, 1500, 0.0, None, dict(timestep_respacing="ddim100+model=", prompts=["a"]))
    with pytest.raises(ValueError, match="frames_skip"):  # the step count is that of the spacing: 0.95 * 10 rounds to all 10 steps
        an._check(3, "wrap", "bicubic", 0.95, 1500, 0.0, None, dict(timestep_respacing="ddim10+model=mine.pt:heads=1", prompts=["a"]))


def test_checkpoints_without_down_path_attention_with_other_class_counts_and_in_wrappers():
    # no attention level on the way down: attention_resolutions "" round-trips into a valid configuration (the middle block still attends)
    kw = dict(R.TINY, attention_resolutions="", resblock_updown=False, use_scale_shift_norm=False)
    with th.device("meta"):
        ref = R.ClassicUNetModel(**dict(kw, attention_resolutions="1"))  # (the reference takes resolutions as numbers: 32 // 1 is no level's rate)
    sd = dict(ref.state_dict())
    flags = script_util.unet_flags_from_state_dict(sd, 32)
    assert flags["attention_resolutions"] == ""
    f = script_util.community_flags(("mine.pt", 1, None, False), 32, False, sd=sd)
    assert [(k, v.numel()) for k, v in sd.items()] == nets.manifest("unet", nets.UNet.make_config(**script_util.community_unet_kwargs(f)))
    # the class count is read from label_emb.weight, and a malformed one is refused by name
    with th.device("meta"):
        sd = dict(R.ClassicUNetModel(**dict(R.TINY, num_classes=10)).state_dict())
    f = script_util.community_flags(("mine.pt", 1, None, False), 32, True, sd=sd)
    assert f["num_classes"] == 10 and script_util.community_unet_kwargs(f)["num_classes"] == 10
    with pytest.raises(ValueError, match=r"label_emb\.weight"):
        script_util.unet_flags_from_state_dict(dict(sd, **{"label_emb.weight": th.empty(10, 100, device="meta")}), 32)
    # wrappers of training scripts are opened; what is no state dict is refused by name
    assert script_util.unwrap_state_dict({"state_dict": sd, "step": 7}) is sd and script_util.unwrap_state_dict({"model": sd}) is sd
    assert script_util.unwrap_state_dict(sd) is sd
    with pytest.raises(ValueError, match="'step'"):
        script_util.unwrap_state_dict(dict(sd, step=7), "mine.pt")
    with pytest.raises(ValueError, match="not a state dict"):
        script_util.unwrap_state_dict([1, 2], "mine.pt")
