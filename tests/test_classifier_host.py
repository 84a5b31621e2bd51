"""Host side of the noisy classifier (no GPU): parameter manifests against tests/classifier_ref.py, checkpoint-shape inference, the
`classifier=FILE:CLASS[:SCALE]` entry of --clip_model, error codes of the C ABI, and the reference's own identities."""
import ctypes as C

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd import clip_util
from cgd_amd import lib, nets
from tests import classifier_ref as cr

CONFIGS = {**{f"{s}x{s}": kw for s, kw in nets.CLASSIFIER_CONFIGS.items()}, **cr.MINI}


def _meta_state_dict(kw):
    with th.device("meta"):
        return cr.EncoderUNetModel(**kw).state_dict()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_manifest_lists_the_reference_state_dict_in_upload_order(name):
    kw = CONFIGS[name]
    ref = _meta_state_dict(kw)
    got = nets.manifest("classifier", nets.NoisyClassifier.make_config(**kw))
    assert [k for k, _ in got] == list(ref)
    assert dict(got) == {k: v.numel() for k, v in ref.items()}
    S = kw["image_size"] >> (len(kw["channel_mult"]) - 1)
    assert tuple(ref["out.2.positional_embedding"].shape)[1] == S * S + 1


def test_published_sizes_share_the_head():
    for size, kw in nets.CLASSIFIER_CONFIGS.items():
        sd = _meta_state_dict(kw)
        assert tuple(sd["out.2.positional_embedding"].shape) == (512, 65), size
        assert tuple(sd["out.2.c_proj.weight"].shape) == (1000, 512, 1), size
    assert nets.CLASSIFIER_CONFIGS[64]["num_res_blocks"] == 4 and nets.CLASSIFIER_CONFIGS[256]["num_res_blocks"] == 2


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_config_from_state_dict_round_trips(name):
    kw = CONFIGS[name]
    sd = {("module." + k): v for k, v in _meta_state_dict(kw).items()}
    clean, got = clip_util.classifier_config_from_state_dict({"state_dict": sd, "epoch": 3}, num_head_channels=kw["num_head_channels"])
    assert set(clean) == {k[len("module."):] for k in sd}
    want = dict(kw, channel_mult=tuple(float(m) for m in kw["channel_mult"]))
    got = dict(got, channel_mult=tuple(float(m) for m in got["channel_mult"]))
    assert got == want
    # ... and the inferred configuration asks the library for exactly the checkpoint's tensors
    assert dict(nets.manifest("classifier", nets.NoisyClassifier.make_config(**got))) == {k: v.numel() for k, v in clean.items()}


def test_config_from_state_dict_refuses_damaged_checkpoints():
    kw = nets.CLASSIFIER_CONFIGS[256]
    good = dict(_meta_state_dict(kw))
    bad = dict(good)
    bad["out.2.positional_embedding"] = th.empty(512, 64, device="meta")  # 64 positions: not S*S + 1
    with pytest.raises(ValueError, match=r"S\*S \+ 1"):
        clip_util.classifier_config_from_state_dict(bad)
    # a missing level: the three blocks of level 1 (two ResBlocks and the `down` block) are gone, the rest keeps its numbers
    bad = {k: v for k, v in good.items() if k.split(".")[:2] not in (["input_blocks", "4"], ["input_blocks", "5"], ["input_blocks", "6"])}
    with pytest.raises(ValueError, match="level is missing"):
        clip_util.classifier_config_from_state_dict(bad)
    # ... also when the remaining blocks are renumbered
    renum = {}
    for k, v in bad.items():
        p = k.split(".")
        if p[0] == "input_blocks" and int(p[1]) > 6:
            p[1] = str(int(p[1]) - 3)
        renum[".".join(p)] = v
    with pytest.raises(ValueError):
        clip_util.classifier_config_from_state_dict(renum)
    # a wrong width: a 96-wide net of the 256x256 layout
    with pytest.raises(ValueError, match="model_channels"):
        clip_util.classifier_config_from_state_dict(_meta_state_dict(dict(kw, model_channels=96, num_head_channels=32)))
    with pytest.raises(ValueError, match="diffusion UNet"):
        clip_util.classifier_config_from_state_dict(dict(good, **{"label_emb.weight": th.empty(1000, 512, device="meta")}))


def test_split_classifier_parses_and_refuses_before_any_load(tmp_path):
    sc = clip_util.split_classifier
    assert sc("ViT-B/32") == ("ViT-B/32", None)
    assert sc("ViT-B/32+classifier=FILE:3") == ("ViT-B/32", ("FILE", 3, 1.0))
    assert sc("ViT-B/32+classifier=FILE:3:2.5") == ("ViT-B/32", ("FILE", 3, 2.5))
    assert sc("ViT-B/32+classifier=C:/models/256x256_classifier.pt:207") == ("ViT-B/32", ("C:/models/256x256_classifier.pt", 207, 1.0))
    assert sc("ViT-B/32+classifier=host:dir/f.pt:207:0.5") == ("ViT-B/32", ("host:dir/f.pt", 207, 0.5))
    missing = str(tmp_path / "never_opened.pt")  # refusals never touch the file: it does not exist
    for bad in (f"ViT-B/32+classifier={missing}", f"ViT-B/32+classifier={missing}:", f"ViT-B/32+classifier={missing}:dog",
                f"ViT-B/32+classifier={missing}:2.5", f"ViT-B/32+classifier={missing}:3:0", f"ViT-B/32+classifier={missing}:3:-1",
                f"ViT-B/32+classifier={missing}:-3", f"ViT-B/32+classifier={missing}:3:nan", "ViT-B/32+classifier=:3",
                f"classifier={missing}:3", f"ViT-B/32+classifier={missing}:3+classifier={missing}:4"):
        with pytest.raises(ValueError):
            sc(bad)
    for off in ((64, 0), (0, 64)):
        with pytest.raises(ValueError, match="offset"):
            sc(f"ViT-B/32+classifier={missing}:3", *off)
    # composes with the other value entries in either order
    for spec in (f"ViT-B/32+secondary=S.pth+cuts=4:12+classifier={missing}:3:2", f"classifier={missing}:3:2+cuts=4:12+ViT-B/32+secondary=S.pth"):
        rest, found = sc(spec)
        assert found == (missing, 3, 2.0)
        rest, cuts = clip_util.split_cuts(rest)
        names, secondary = clip_util.split_secondary(rest, 256)
        assert names == ["ViT-B/32"] and secondary == "S.pth" and cuts[:2] == (4, 12)


def test_generator_refuses_a_bad_classifier_entry_before_any_load(tmp_path):
    from cgd import cgd as mine
    missing = str(tmp_path / "never_opened.pt")
    with pytest.raises(ValueError, match="CLASS"):
        next(mine.clip_guided_diffusion(prompts=["x"], clip_model_name=f"ViT-B/32+classifier={missing}", device="cuda:0"))
    with pytest.raises(ValueError, match="offset"):
        next(mine.clip_guided_diffusion(prompts=["x"], clip_model_name=f"ViT-B/32+classifier={missing}:3", height_offset=64, device="cuda:0"))


def _cfg(**over):
    kw = dict(cr.MINI["clsB"])
    kw.update(over)
    return nets.NoisyClassifier.make_config(**kw)


def test_null_handles_and_bad_configurations_return_errors():
    h = lib.load()
    assert h.cgd_classifier_num_params(None) == -3 and h.cgd_classifier_finalize(None) == -3
    assert h.cgd_classifier_forward(None, None, None, None, None, None, 1, 16, 16, None) == -3
    assert h.cgd_classifier_dgrad(None, 1.0, None, 0, None) == -3
    assert h.cgd_classifier_set_param(None, b"x", None, 0) == -3
    h.cgd_classifier_destroy(None)  # no-op
    assert h.cgd_classifier_manifest(None, lib.MANIFEST_CB(lambda *a: None), None) == -3
    out = C.c_void_p()
    assert h.cgd_classifier_create(None, C.byref(_cfg()), C.byref(out)) == -3
    assert h.cgd_op_attnpool_fwd(None, *([None] * 11), 1, 4, 128, 32, 7, None) == -3
    assert h.cgd_op_attnpool_bwd(None, None, None, None, None, 1.0, None, None, 1, 4, 128, 32, 7, None) == -3
    assert h.cgd_op_attnpool_scratch_floats(1, 4, 128, 32, 7) > 0
    assert h.cgd_op_attnpool_scratch_floats(0, 4, 128, 32, 7) == -2
    assert h.cgd_op_attnpool_scratch_floats(1, 4, 128, 48, 7) == -2     # 128 channels are no whole number of 48-wide heads
    assert h.cgd_op_attnpool_scratch_floats(1, 32, 512, 64, 1000) == -2  # 1025 keys of one head do not fit the LDS
    assert nets.manifest("classifier", _cfg())
    empty = _cfg()
    empty.n_mult = 0
    for bad in (empty, _cfg(model_channels=48), _cfg(out_channels=0), _cfg(out_channels=-5), _cfg(num_head_channels=0),
                _cfg(num_head_channels=48), _cfg(image_size=18), _cfg(num_res_blocks=0)):
        with pytest.raises(ValueError):
            nets.manifest("classifier", bad)


def test_reference_identities():
    """d logp / d logits = onehot - softmax; the pool's gradient gives every spatial position 1 / (S*S) of token 0's gradient."""
    g = th.Generator().manual_seed(5)
    logits = th.randn(3, 7, generator=g, requires_grad=True)
    y = th.tensor([0, 6, 2])
    cr.logp_of(logits, y).sum().backward()
    want = th.nn.functional.one_hot(y, 7).float() - th.softmax(logits.detach(), -1)
    assert th.allclose(logits.grad, want, atol=1e-6)
    pool = cr.AttentionPool2d(4, 64, 32, 5)
    h = th.randn(2, 64, 4, 4, generator=g, requires_grad=True)
    tok = pool.tokens(h)
    tok.retain_grad()
    cr.logp_of(pool.c_proj(pool.attend(pool.qkv_proj(tok)))[:, :, 0], th.tensor([1, 4])).sum().backward()
    via_mean = tok.grad[:, :, :1] / 16
    assert th.allclose(h.grad.reshape(2, 64, 16), tok.grad[:, :, 1:] + via_mean, atol=1e-6)
    assert via_mean.abs().max() > 0
