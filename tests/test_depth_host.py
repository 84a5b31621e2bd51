"""Host side of the depth network (CPU, `not gpu`): the manifest of DPT-Large against the key table, the loader's refusals, the net-size rule, the
position-embedding resize, the reference's RCU and edge-replicating resize, and `--depth_model` parsing with its refusals."""
import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

import cgd_amd  # noqa: F401
from cgd_amd import animate as an
from cgd_amd import lib as L
from cgd_amd import nets
from tests import depth_ref as R

TINY = dict(patch=16, width=128, layers=4, heads=2, hooks=(0, 1, 2, 3), native_grid=2, features=32, reassemble_channels=(32, 64, 128, 128))


def test_manifest_of_dpt_large_is_the_published_key_set():
    cfg, _ = nets.depth_config("dpt_large")
    got = dict(nets.manifest("depth", cfg))
    shapes = nets.depth_param_shapes("dpt_large")
    assert set(got) == set(shapes)
    for k, shape in shapes.items():
        assert got[k] == int(np.prod(shape)), k
    # spot checks of the table itself, as the published file has them
    W = 1024
    assert shapes["pretrained.model.pos_embed"] == (1, 577, W) and shapes["pretrained.model.patch_embed.proj.weight"] == (W, 3, 16, 16)
    assert shapes["pretrained.model.blocks.23.attn.qkv.weight"] == (3 * W, W) and shapes["pretrained.model.blocks.0.mlp.fc2.weight"] == (W, 4 * W)
    assert shapes["pretrained.act_postprocess1.4.weight"] == (256, 256, 4, 4) and shapes["pretrained.act_postprocess2.4.weight"] == (512, 512, 2, 2)
    assert "pretrained.act_postprocess3.4.weight" not in shapes and shapes["pretrained.act_postprocess4.4.weight"] == (1024, 1024, 3, 3)
    assert shapes["pretrained.act_postprocess4.0.project.0.weight"] == (W, 2 * W) and shapes["scratch.layer3_rn.weight"] == (256, 1024, 3, 3)
    assert "scratch.layer1_rn.bias" not in shapes and "scratch.refinenet4.resConfUnit1.conv1.weight" not in shapes
    assert shapes["scratch.refinenet4.resConfUnit2.conv2.bias"] == (256,) and shapes["scratch.refinenet1.out_conv.weight"] == (256, 256, 1, 1)
    assert shapes["scratch.output_conv.0.weight"] == (128, 256, 3, 3) and shapes["scratch.output_conv.4.weight"] == (1, 32, 1, 1)
    assert not any(k.startswith(nets.DEPTH_IGNORED_PREFIXES) for k in shapes)
    assert len(shapes) == 4 + 24 * 12 + (6 + 6 + 4 + 6) + 4 + (3 * 10 + 6) + 6


@pytest.mark.parametrize("bad", [dict(width=100), dict(width=96, heads=1), dict(heads=4), dict(features=48), dict(reassemble_channels=(32, 64, 100, 128)),
                                 dict(hooks=(0, 1, 3, 2)), dict(hooks=(0, 1, 2, 4)), dict(layers=0)])
def test_manifest_refuses_what_the_kernels_cannot_run(bad):
    cfg, _ = nets.depth_config({**TINY, **bad})
    assert L.load().cgd_depth_manifest(cfg, L.MANIFEST_CB(lambda *a: None), None) == -2


class _Probe(nets.DepthNet):
    """load_state_dict's checks without a GPU: the upload is replaced by a record of the keys it would read"""

    def __init__(self, config):
        self.cfg, self.config = nets.depth_config(config)
        self.read = None

    def param_specs(self):
        return nets.manifest("depth", self.cfg)

    def __del__(self):
        pass


def test_load_state_dict_names_missing_keys_and_wrong_shapes(monkeypatch):
    from cgd_amd import synthetic
    sd = synthetic.depth_state_dict(TINY, seed=1)
    assert {k: tuple(v.shape) for k, v in sd.items()} == nets.depth_param_shapes(TINY)
    seen = {}
    monkeypatch.setattr(nets._Net, "load_state_dict", lambda self, d, prefix="": seen.update(keys=[n for n, _ in self.param_specs()]) or self)
    # the three unused groups are ignored, present or not
    extra = {**sd, "pretrained.model.norm.weight": th.zeros(128), "pretrained.model.head.weight": th.zeros(1000, 128),
             "scratch.refinenet4.resConfUnit1.conv1.weight": th.zeros(32, 32, 3, 3)}
    _Probe(TINY).load_state_dict(extra)
    assert set(seen["keys"]) == set(sd)
    for key in ("pretrained.model.blocks.2.attn.qkv.bias", "pretrained.act_postprocess1.4.weight", "scratch.output_conv.4.bias"):
        with pytest.raises(ValueError, match="missing key " + key.replace(".", r"\.")):
            _Probe(TINY).load_state_dict({k: v for k, v in sd.items() if k != key})
    for key, shape in (("pretrained.model.pos_embed", (1, 4, 128)), ("scratch.layer2_rn.weight", (32, 64, 1, 1)),
                       ("pretrained.act_postprocess2.4.weight", (64, 64, 4, 4)), ("pretrained.model.cls_token", (128,))):
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + " has shape"):
            _Probe(TINY).load_state_dict({**sd, key: th.zeros(shape)})


def test_net_size_rule():
    for fn in (nets.depth_net_size, R.net_size):
        assert fn(256, 256) == (384, 384) and fn(512, 512) == (384, 384)
        assert fn(256, 384) == (384, 576) and fn(64, 512) == (384, 3072) and fn(32, 32) == (384, 384)
        assert fn(48, 80, 64) == (64, 96) and fn(100, 30, 16) == (64, 32)  # halves round up, never below 32


def test_pos_embed_resize():
    th.manual_seed(0)
    pos = th.randn(1, 1 + 9, 8)
    for fn in (nets.depth_resize_pos_embed, R.resize_pos_embed):
        assert th.equal(fn(pos, 3, 3, 3), pos[0])
        for gh, gw in ((2, 5), (6, 3), (1, 1)):
            got = fn(pos, 3, gh, gw)
            ref = F.interpolate(pos[0, 1:].reshape(1, 3, 3, 8).permute(0, 3, 1, 2), size=(gh, gw), mode="bilinear", align_corners=False)
            assert got.shape == (1 + gh * gw, 8) and th.equal(got[0], pos[0, 0])
            assert th.equal(got[1:], ref.permute(0, 2, 3, 1).reshape(gh * gw, 8))


def test_reference_rcu_keeps_the_unrectified_residual():
    th.manual_seed(1)
    x = -th.rand(1, 4, 5, 5) - 0.1  # all negative: relu(x) = 0, so the conv branch is a constant and a rectified residual would be 0
    sd = {"u.conv1.weight": th.randn(4, 4, 3, 3), "u.conv1.bias": th.randn(4), "u.conv2.weight": th.randn(4, 4, 3, 3), "u.conv2.bias": th.randn(4)}
    branch = F.conv2d(F.relu(F.conv2d(th.zeros_like(x), sd["u.conv1.weight"], sd["u.conv1.bias"], padding=1)), sd["u.conv2.weight"],
                      sd["u.conv2.bias"], padding=1)
    assert th.allclose(R.rcu(x, sd, "u"), branch + x, atol=1e-6) and not th.allclose(R.rcu(x, sd, "u"), branch, atol=1e-3)


@pytest.mark.parametrize("n,m", [(256, 384), (384, 256), (64, 32), (96, 160), (5, 32), (7, 7)])
def test_edge_replicating_resize_rows_sum_to_one(n, m):
    if n == m:
        x = th.randn(2, n, n)
        assert th.equal(R.resize_edge(x, n, n), x)
        return
    M = R.edge_matrix(n, m)
    assert M.shape == (m, n) and np.abs(M.sum(1) - 1).max() < 1e-12
    # a constant image stays constant up to the border, which zero padding would not give
    assert th.allclose(R.resize_edge(th.full((1, n, n), 0.7, dtype=th.float64), m, m), th.full((1, m, m), 0.7, dtype=th.float64), atol=1e-12)
    # the library's own weight rows, folded the same way, agree
    import ctypes as C
    h = L.load()
    T = C.c_int()
    w = np.zeros((m, 64), np.float32)
    left = np.zeros(m, np.int32)
    assert h.cgd_cutouts_resize_weights(n, m, w.ctypes.data, left.ctypes.data, C.byref(T)) == 0
    Mk = np.zeros((m, n))
    wk = w.reshape(-1)[:m * T.value].reshape(m, T.value)
    for o in range(m):
        for t in range(T.value):
            Mk[o, min(max(int(left[o]) + t, 0), n - 1)] += wk[o, t]
    assert np.abs(Mk - M).max() < 1e-6


def test_depth_mapping():
    inv = th.tensor([0.0, 12.0, 50.0, 80.0])
    assert th.allclose(R.depth_map(inv), th.tensor([50 / 19, 2.0, 0.05, 0.05]))


def test_depth_model_parsing():
    assert an.parse_depth_model(None) is None
    assert an.parse_depth_model("dpt_large-midas-2f21e586.pt") == ("dpt_large-midas-2f21e586.pt", {})
    assert an.parse_depth_model("w/dpt.pt:size=256:scale=10:offset=40.5") == ("w/dpt.pt", {"size": 256, "scale": 10.0, "offset": 40.5})
    for bad in ("", ":size=3", "f.pt:size", "f.pt:size=abc", "f.pt:floor=1", "f.pt:size=64:size=96", "f.pt:size=16", "f.pt:scale=0", "f.pt:offset=nan"):
        with pytest.raises(ValueError, match="depth_model"):
            an.parse_depth_model(bad)
    a = an.build_parser().parse_args(["--frames", "3", "--mode", "3d", "--depth_model", "x.pt:size=64"])
    assert a.depth_model == "x.pt:size=64" and an.build_parser().parse_args(["--frames", "3"]).depth_model is None


def test_depth_model_refusals_come_before_anything_is_loaded(monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util
    from cgd_amd import shard

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    for mod, name in ((clip_util, "load_clip"), (clip_util, "encode_text_prompt"), (script_util, "download_guided_diffusion"),
                      (script_util, "load_guided_diffusion"), (script_util, "load_lpips"), (mine, "ClipGuidance"), (an, "load_depth_model")):
        monkeypatch.setattr(mod, name, no_load)
    base = dict(prompts=["a cat"], device="cuda", timestep_respacing="ddim10")
    with pytest.raises(ValueError, match="depth_model: only with mode='3d'"):
        next(an.animate(3, depth_model="dpt_large-midas-2f21e586.pt", **base))
    with pytest.raises(ValueError, match="depth_model and depth"):
        next(an.animate(3, mode="3d", depth_model="dpt_large-midas-2f21e586.pt", depth=lambda x: x[:, :1], **base))
    with pytest.raises(ValueError, match="depth_model"):
        next(an.animate(3, mode="3d", depth_model="f.pt:size=abc", **base))
    monkeypatch.setattr(shard, "world", lambda: (0, 2))
    with pytest.raises(ValueError):
        next(an.animate(3, mode="3d", depth_model="dpt_large-midas-2f21e586.pt", **base))
