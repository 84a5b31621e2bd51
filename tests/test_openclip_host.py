"""open_clip (LAION) ViT checkpoints without a GPU: `--clip_model` name parsing, the loader's configuration inference on synthetic state dicts
built from the library's own parameter manifests, the attention dispatch plan at head dim 80 and the two activation setters' symbols."""
import ctypes as C

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd import clip_util, script_util
from cgd_amd import lib, nets

ARCHS = sorted(nets.OPENCLIP_CONFIGS)

# the table of the issue, restated here so that an edit of nets.OPENCLIP_CONFIGS cannot pass unnoticed
TABLE = {
    "ViT-B-32": ((224, 32, 768, 12, 12, 512), (77, 49408, 512, 12, 8, 512)),
    "ViT-B-16": ((224, 16, 768, 12, 12, 512), (77, 49408, 512, 12, 8, 512)),
    "ViT-L-14": ((224, 14, 1024, 24, 16, 768), (77, 49408, 768, 12, 12, 768)),
    "ViT-H-14": ((224, 14, 1280, 32, 16, 1024), (77, 49408, 1024, 24, 16, 1024)),
}


def test_config_table():
    assert nets.OPENCLIP_CONFIGS == TABLE
    assert nets.ACTIVATIONS == {"quick_gelu": 2, "gelu": 3}
    assert not set(nets.OPENCLIP_CONFIGS) & (set(nets.VIT_CONFIGS) | set(nets.RN_CONFIGS) | set(clip_util.CLIP_MODEL_URLS))


def test_name_parsing():
    p = clip_util.parse_clip_model_name
    for arch in ARCHS:
        assert p(arch) == (arch, "gelu", None)
        assert p(arch + "-quickgelu") == (arch, "quick_gelu", None)
        assert p(f"{arch}=/ckpts/laion2b.pt") == (arch, "gelu", "/ckpts/laion2b.pt")
        assert p(f"{arch}-quickgelu=/a=b/c.pt") == (arch, "quick_gelu", "/a=b/c.pt")  # only the first '=' separates
    # OpenAI names and plain paths: untouched, QuickGELU
    for name in list(clip_util.CLIP_MODEL_URLS) + ["/ckpts/ViT-B-32.pt", "model.pt", "/odd=dir/x.pt", "ViT-g-14", "ViT-g-14=/x.pt"]:
        assert p(name) == (None, "quick_gelu", name)
    with pytest.raises(ValueError):
        p("ViT-H-14=")
    # the 'A+B' split of cgd.clip_guided_diffusion happens before: every part parses on its own
    parts = [n.strip() for n in "ViT-B/32 + ViT-H-14=/c/h.pt+ViT-B-16-quickgelu".split("+")]
    assert [p(n) for n in parts] == [(None, "quick_gelu", "ViT-B/32"), ("ViT-H-14", "gelu", "/c/h.pt"), ("ViT-B-16", "quick_gelu", None)]


def test_cli_help_names_the_syntax_and_keeps_the_contract():
    from cgd import cgd as cgd_mod
    line = [ln for ln in cgd_mod._CLI_SPEC.splitlines() if ln.startswith("--clip_model")]
    assert len(line) == 1
    spec, text = (s.strip() for s in line[0].split("|", 1))
    assert spec == "--clip_model -clip str ViT-B/32"
    assert "ARCH=" in text and "ViT-H-14" in text and "A+B" in text


def _meta_state_dict(arch, vit_cfg=None, text_cfg=None, mlp_ratio=4):
    """An open_clip-style state dict of meta tensors (shapes only: ViT-H-14 would be 2.5 GB) from the library's manifests"""
    vit_cfg, text_cfg = vit_cfg or TABLE[arch][0], text_cfg or TABLE[arch][1]
    res, patch, width, layers, heads, out = vit_cfg
    T, vocab, tw, tl, th_, tout = text_cfg

    def shape(name, numel, w, cfg):
        leaf = name.rsplit(".", 1)[-1]
        if name == "conv1.weight":
            return (w, 3, patch, patch)
        if name == "proj":
            return (w, out)
        if name == "text_projection":
            return (tw, tout)
        if name == "token_embedding.weight":
            return (vocab, tw)
        if name == "positional_embedding":
            return (numel // w, w)
        if name.endswith("in_proj_weight"):
            return (3 * w, w)
        if name.endswith("out_proj.weight"):
            return (w, w)
        if name.endswith("c_fc.weight"):
            return (mlp_ratio * w, (4 * w * w) // (mlp_ratio * w))
        if name.endswith("c_proj.weight"):
            return ((4 * w * w) // (mlp_ratio * w), mlp_ratio * w)
        assert leaf in ("weight", "bias", "in_proj_bias", "class_embedding"), name
        return (numel,)

    sd = {}
    for name, numel in nets.manifest("vit", lib.ViTConfig(*vit_cfg)):
        sd["visual." + name] = th.empty(shape(name, numel, width, vit_cfg), device="meta")
    for name, numel in nets.manifest("text", lib.TextConfig(*text_cfg)):
        sd[name] = th.empty(shape(name, numel, tw, text_cfg), device="meta")
    sd["logit_scale"] = th.empty((), device="meta")
    sd["attn_mask"] = th.empty(T, T, device="meta")
    return sd


def _wrap(sd, how):
    if how == "module":
        return {"module." + k: v for k, v in sd.items()}
    if how == "state_dict":
        return {"epoch": 32, "name": "run", "state_dict": {"module." + k: v for k, v in sd.items()}}
    return sd


@pytest.mark.parametrize("arch,how", [("ViT-B-32", "plain"), ("ViT-B-16", "module"), ("ViT-L-14", "state_dict"), ("ViT-H-14", "state_dict"),
                                      ("ViT-H-14", "plain")])
def test_configurations_from_a_state_dict_equal_the_table(arch, how):
    sd, vit, text = clip_util.openclip_configs_from_state_dict(arch, _wrap(_meta_state_dict(arch), how))
    assert (vit, text) == TABLE[arch]
    assert all(isinstance(v, th.Tensor) for v in sd.values()) and "visual.proj" in sd and "text_projection" in sd
    assert not any(k.startswith("module.") for k in sd) and "epoch" not in sd
    # every parameter the towers ask for is there under its manifest name
    for name, _ in nets.manifest("vit", lib.ViTConfig(*vit)):
        assert "visual." + name in sd
    for name, _ in nets.manifest("text", lib.TextConfig(*text)):
        assert name in sd and clip_util._is_text_key(name)
    assert not clip_util._is_text_key("logit_scale") and not clip_util._is_text_key("attn_mask")


class _FakeTower:
    made = []

    def __init__(self, ctx, name=None, config=None, activation="quick_gelu"):
        self.kind, self.config, self.activation = type(self).__name__, tuple(config), activation
        self.input_resolution, self.out_dim = config[0], config[5]
        _FakeTower.made.append(self)

    def load_state_dict(self, sd, prefix=""):
        self.keys = sorted(sd)
        return self


class _FakeImage(_FakeTower):
    pass


class _FakeText(_FakeTower):
    pass


@pytest.fixture
def fake_towers(monkeypatch):
    """load_clip with the device taken away: the tower constructors record what they are handed"""
    class Ctx:
        device = 0
    _FakeTower.made = []
    monkeypatch.setattr(script_util, "get_context", lambda device: Ctx())
    monkeypatch.setattr(nets, "ClipImageTower", _FakeImage)
    monkeypatch.setattr(nets, "ClipTextTower", _FakeText)
    monkeypatch.delenv("CGD_SYNTHETIC_WEIGHTS", raising=False)
    clip_util.load_clip.cache_clear()
    yield _FakeTower.made
    clip_util.load_clip.cache_clear()


def _small_state_dict(vit_cfg, text_cfg):
    """real (tiny-valued) tensors for th.save: zeros of the manifest shapes"""
    return {k: th.zeros(v.shape) for k, v in _meta_state_dict(None, vit_cfg, text_cfg).items()}


def test_load_clip_hands_vit_h_14_its_16_heads(fake_towers, tmp_path, monkeypatch):
    """A ViT-H-14-shaped checkpoint file (width 1280, so width // 64 = 20; one layer per tower instead of 32 / 24 keeps the file small, and the table
    is narrowed to the file's depth so that the cross-check passes) loaded as ViT-H-14: both towers get 16 heads and the exact GELU."""
    vit_cfg, text_cfg = (224, 14, 1280, 1, 16, 1024), (77, 64, 128, 1, 16, 1024)  # (a small text tower keeps the file small)
    monkeypatch.setitem(nets.OPENCLIP_CONFIGS, "ViT-H-14", (vit_cfg, text_cfg))
    path = tmp_path / "h14.pt"
    th.save({"state_dict": {"module." + k: v for k, v in _small_state_dict(vit_cfg, text_cfg).items()}}, path)
    model, size = clip_util.load_clip(f"ViT-H-14={path}", "cuda")
    image, text = fake_towers
    assert (image.kind, image.config, image.activation) == ("_FakeImage", vit_cfg, "gelu")
    assert (text.kind, text.config, text.activation) == ("_FakeText", text_cfg, "gelu")
    assert image.config[4] == 16 and 1280 // 64 == 20
    assert size == 224 and model.text_model is text
    assert all(k.startswith("visual.") for k in image.keys) and "logit_scale" not in text.keys and "attn_mask" not in text.keys


def test_load_clip_quickgelu_suffix_and_plain_paths(fake_towers, tmp_path, monkeypatch):
    vit_cfg, text_cfg = (224, 32, 768, 1, 12, 512), (77, 64, 512, 1, 8, 512)
    monkeypatch.setitem(nets.OPENCLIP_CONFIGS, "ViT-B-32", (vit_cfg, text_cfg))
    path = tmp_path / "b32.pt"
    th.save(_small_state_dict(vit_cfg, text_cfg), path)
    clip_util.load_clip(f"ViT-B-32-quickgelu={path}", "cuda")
    assert [t.activation for t in fake_towers] == ["quick_gelu", "quick_gelu"]
    del fake_towers[:]
    monkeypatch.setattr(clip_util, "_clip_importable", lambda: False)
    clip_util.load_clip(str(path), "cuda")  # a plain path: OpenAI's inference, as before (heads = width // 64, QuickGELU)
    assert [(t.config[4], t.activation) for t in fake_towers] == [(12, "quick_gelu"), (8, "quick_gelu")]
    with pytest.raises(FileNotFoundError):
        clip_util.load_clip("ViT-B-32", "cuda")  # an architecture without a file needs CGD_SYNTHETIC_WEIGHTS=1
    with pytest.raises(FileNotFoundError):
        clip_util.load_clip(f"ViT-B-32={tmp_path / 'absent.pt'}", "cuda")


def test_shape_mismatch_names_the_dimension():
    sd = _meta_state_dict("ViT-L-14")
    with pytest.raises(ValueError, match="image tower has width 1024"):
        clip_util.openclip_configs_from_state_dict("ViT-H-14", sd)
    with pytest.raises(ValueError, match="patch 14"):
        clip_util.openclip_configs_from_state_dict("ViT-B-16", _meta_state_dict("ViT-L-14", vit_cfg=(224, 14, 768, 12, 12, 512),
                                                                                 text_cfg=TABLE["ViT-B-16"][1]))
    with pytest.raises(ValueError, match="text tower has layers 12"):
        clip_util.openclip_configs_from_state_dict("ViT-H-14", _meta_state_dict("ViT-H-14", text_cfg=(77, 49408, 1024, 12, 16, 1024)))


def test_non_4x_mlp_is_refused():
    # ViT-g-14's image tower: width 1408, MLP 6144 (ratio 48 / 11); here the same idea at ratio 2 on a table architecture
    sd = _meta_state_dict("ViT-B-32", mlp_ratio=2)
    with pytest.raises(NotImplementedError, match="4 x width"):
        clip_util.openclip_configs_from_state_dict("ViT-B-32", sd)


def _plan(handle, T, d, heads=16, precision=1, flash=-1):
    out = (C.c_int * 2)()
    assert handle.cgd_op_attn_plan(T, d, 3 * heads * d, heads * d, precision, flash, out) == 0
    return tuple(out)


def test_attention_plan_head_dim_80():
    handle = lib.load()
    GENERIC, FLASH = 0, 3
    for T in (50, 72, 257, 577):
        assert _plan(handle, T, 80) == (FLASH, 2), T  # dq + dkv at every T: the one-workgroup backward is d = 64 only
        assert _plan(handle, T, 80, precision=0)[0] == GENERIC, T
    assert _plan(handle, 16, 80)[0] == GENERIC and _plan(handle, 32, 80)[0] == GENERIC
    assert _plan(handle, 50, 80, flash=1)[0] == GENERIC and _plan(handle, 257, 80, flash=1) == (FLASH, 2)
    assert _plan(handle, 257, 80, flash=0)[0] == GENERIC
    out = (C.c_int * 2)()
    assert handle.cgd_op_attn_plan(257, 80, 3 * 16 * 80 + 2, 16 * 80, 1, -1, out) == 0 and out[0] == GENERIC  # misaligned rows
    # the neighbours keep their families
    assert _plan(handle, 257, 64) == (FLASH, 2) and _plan(handle, 50, 64) == (FLASH, 1) and _plan(handle, 257, 96)[0] == GENERIC


def test_activation_setters_are_exported_and_refuse_null():
    handle = lib.load()
    for name in ("cgd_vit_set_activation", "cgd_text_set_activation"):
        assert name in lib.EXPORTED_SYMBOLS
        fn = getattr(handle, name)
        assert fn(None, 3) == -3
    with pytest.raises(ValueError, match="activation"):
        nets._activation_code("relu")
