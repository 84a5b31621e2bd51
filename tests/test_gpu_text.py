"""The CLIP text tower on the GPU: causal attention of every kernel family against a float64 reference, the full-size towers against the
CPU restatement (tests/text_ref.py), and prompt encoding through the drop-in without the `clip` package."""
import ctypes as C
import math
import sys

import pytest
import torch as th

from tests import parity_checks as pc
from tests import text_ref

pytestmark = pytest.mark.gpu

# precision 2 (one bf16 product per MFMA): bounds on max |a - b| / max |ref|, about twice what was measured on an MI355X:
# the ViT-B/32 text tower 6.0e-3 / 6.6e-3 / 6.9e-3 at N = 1 / 3 / 8; the batched-GEMM attention family 3.5e-3 at worst (its contractions are
# the bf16 GEMM's; the fused families compute exact fp32 products in precision 2 and are held to the literal tolerance)
BF16_TOWER_BOUND = 1.5e-2
BF16_ATTN_GEMM_BOUND = 1e-2


def _assert_all(recs):
    bad = [r for r in recs if not r["ok"]]
    assert not bad, "; ".join(f"{r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e}" for r in bad)


def _causal_ref(qkv, nb, heads, T, d):
    """float64 softmax(q k^T / sqrt(d) + causal mask) v on [Q all heads | K | V] rows."""
    C_ = heads * d
    x = qkv.double().view(nb, T, 3, heads, d).permute(2, 0, 3, 1, 4)  # (3, nb, heads, T, d)
    q, k, v = x[0], x[1], x[2]
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    s = s.masked_fill(th.ones(T, T, dtype=th.bool).triu(1), float("-inf"))
    return (th.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(nb * T, C_)


def _family(lib, T, d, heads, precision):
    out2 = (C.c_int * 2)()
    assert lib.cgd_op_attn_plan(T, d, 3 * heads * d, heads * d, precision, -1, out2) == 0
    return out2[0]


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_causal_attention_every_family(precision):
    import cgd_amd  # noqa: F401
    from cgd_amd import lib, ops
    ctx = lib.Context(0, precision)
    recs, families = [], set()
    for T in (8, 33, 64, 77, 128, 257):
        for nb, heads, d in ((2, 3, 64), (1, 8, 64), (3, 2, 32)):
            fam = _family(ctx.lib, T, d, heads, precision)
            families.add(fam)
            qkv = th.randn(nb * T, 3 * heads * d, generator=pc.g(T + 7 * heads + d))
            ref = _causal_ref(qkv, nb, heads, T, d)
            at = ops.Attention(ctx, nb, heads, T, d, 0, pc.DEV)
            got = at.forward_causal(qkv.to(pc.DEV))
            name = f"causal attn[p{precision} family {fam}] nb{nb} h{heads} T{T} d{d}"
            if precision == 2 and fam == 0:
                r = pc.rec(name, got, ref.float())
                r["ok"] = bool(th.isfinite(got).all()) and r["err_rel"] <= BF16_ATTN_GEMM_BOUND
                recs.append(r)
            else:
                recs.append(pc.rec(name, got, ref.float()))
            # the first key row only sees itself: a non-causal result would differ there (guards against a silently ignored mask)
            assert th.allclose(got[:1, :heads * d].cpu(), qkv[:1, 2 * heads * d:].float(), rtol=1e-2, atol=1e-2)
            # no causal backward: the buffers of a causal forward are refused, never read as if they were non-causal
            with pytest.raises(lib.CgdError, match="causal"):
                at.backward(qkv.to(pc.DEV), th.randn(nb * T, heads * d, device=pc.DEV))
    print("\n".join(f"{r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e}" for r in recs))
    _assert_all(recs)
    expect = {0, 1, 3} if precision == 1 else {0, 1, 2}  # bf16x3: T <= 32 s64, T > 32 flash; else s64 / mid; d = 32: batched GEMMs
    assert expect <= families, families


def _tower_pair(ctx, cfg, seed):
    from cgd_amd import nets
    ref = text_ref.synthetic_init_(text_ref.ClipTextModel(*cfg), seed=seed).eval()
    dev = nets.ClipTextTower(ctx, config=cfg)
    dev.load_clip_state_dict({k: v.to(pc.DEV) for k, v in ref.state_dict().items()})
    return ref, dev


def _prompts(n, vocab, seed):
    """n sequences of mixed length; one is 77 tokens long (end-of-text at position 76), one holds the end-of-text id twice (the first counts)"""
    lengths = [77, 5, 40, 2, 13, 77, 64, 21][:n] if n > 1 else [77]
    tok = text_ref.random_tokens(n, 77, vocab, lengths, seed=seed)
    if n > 1:
        tok[1, 3] = vocab - 1  # an end-of-text id in the middle of a (truncated-like) sequence
    return tok


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_text_tower_vit_b32_full_size(precision):
    import cgd_amd  # noqa: F401
    from cgd_amd import lib
    ctx = lib.Context(0, precision)
    cfg = text_ref.TEXT_CONFIGS["ViT-B/32"]
    ref, dev = _tower_pair(ctx, cfg, seed=11)
    recs = []
    for n in (1, 3, 8):
        tok = _prompts(n, cfg[1], seed=n)
        with th.no_grad():
            e = ref.encode_text(tok)
        got = dev.encode_text(tok.to(pc.DEV))
        th.cuda.synchronize()
        r = pc.rec(f"text[ViT-B/32 p{precision} N{n}]", got, e)
        if precision == 2:
            r["ok"] = bool(th.isfinite(got).all()) and r["err_rel"] <= BF16_TOWER_BOUND
        recs.append(r)
    print("\n".join(f"{r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e}" for r in recs))
    _assert_all(recs)


@pytest.mark.parametrize("width,heads,out", [(640, 10, 640), (768, 12, 768)])
def test_text_tower_wider_configs(width, heads, out):
    import cgd_amd  # noqa: F401
    from cgd_amd import lib
    ctx = lib.Context(0, 1)
    cfg = (77, 49408, width, 3, heads, out)  # RN50x4 / RN50x16 / ViT-L/14 widths, 3 of their 12 layers
    ref, dev = _tower_pair(ctx, cfg, seed=width)
    tok = _prompts(4, cfg[1], seed=5)
    with th.no_grad():
        e = ref.encode_text(tok)
    _assert_all([pc.rec(f"text[W{width} H{heads}]", dev.encode_text(tok.to(pc.DEV)), e)])


def test_text_tower_rejects_out_of_range_ids():
    import cgd_amd  # noqa: F401
    from cgd_amd import lib
    ctx = lib.Context(0, 1)
    _, dev = _tower_pair(ctx, (77, 1000, 128, 1, 2, 64), seed=3)
    tok = text_ref.random_tokens(2, 77, 1000, [10, 77])
    for bad in (1000, -1, 1 << 40):
        t = tok.clone()
        t[1, 4] = bad
        with pytest.raises(ValueError):
            dev.encode_text(t.to(pc.DEV))
    assert th.isfinite(dev.encode_text(tok.to(pc.DEV))).all()


def _full_archive(tmp_path, merges_len):
    """A full synthetic CLIP archive (fp16 state dict with image- and text-tower keys, like clip.load's checkpoint) whose vocabulary matches
    a synthetic BPE file: 512 byte symbols + merges + start / end."""
    from oracle import clip_vit as ocv
    vis = ocv.synthetic_init_(ocv.VisionTransformer(64, 16, 128, 2, 2, 512))
    txt = text_ref.synthetic_init_(text_ref.ClipTextModel(77, 512 + merges_len + 2, 512, 2, 8, 512), seed=99)
    sd = {"visual." + k: v for k, v in vis.state_dict().items()}
    sd.update(txt.state_dict())
    sd["logit_scale"] = th.tensor(4.6052)
    sd = {k: v.detach().half() for k, v in sd.items()}
    path = str(tmp_path / "clip_full.pt")
    th.save(sd, path)
    txt.load_state_dict({k: v.float() for k, v in sd.items() if not k.startswith("visual.") and k != "logit_scale"})
    return path, txt.eval()


def test_encode_text_prompt_native_without_clip(tmp_path, monkeypatch):
    import cgd_amd  # noqa: F401
    from cgd import clip_util
    from cgd_amd import tokenizer
    from tests.test_text_host import CORPUS, learn_merges, write_bpe
    merges = learn_merges(CORPUS, 150)
    bpe = write_bpe(str(tmp_path / tokenizer.BPE_FILENAME), merges)
    monkeypatch.setenv("CGD_CLIP_BPE", bpe)
    monkeypatch.setitem(sys.modules, "clip", None)  # `import clip` raises ImportError
    monkeypatch.setattr(clip_util, "_synthetic_text_embedding", lambda *a, **k: pytest.fail("hash fallback used"))
    path, ref = _full_archive(tmp_path, len(merges))
    clip_util.load_clip.cache_clear()
    try:
        model, _ = clip_util.load_clip(path, "cuda")
        assert model.native_text
        for prompt in ("an owl in a misty forest", "a fox", " ".join(["owl"] * 70)):
            emb, w = clip_util.encode_text_prompt(prompt, 0.5, path, "cuda")
            assert w == 0.5 and emb.shape == (1, 512)
            tok = tokenizer.tokenize(prompt, tokenizer=tokenizer.SimpleTokenizer(bpe))
            with th.no_grad():
                e = ref.encode_text(tok)
            _assert_all([pc.rec(f"encode_text_prompt {prompt[:20]!r}", emb, e)])
    finally:
        clip_util.load_clip.cache_clear()


def test_generator_runs_with_native_text_prompts(tmp_path, monkeypatch):
    import itertools
    import cgd_amd  # noqa: F401
    from cgd import clip_util
    from cgd.cgd import clip_guided_diffusion
    from cgd_amd import tokenizer
    from tests.test_text_host import CORPUS, learn_merges, write_bpe
    merges = learn_merges(CORPUS, 150)
    monkeypatch.setenv("CGD_CLIP_BPE", write_bpe(str(tmp_path / tokenizer.BPE_FILENAME), merges))
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")  # the diffusion model: seeded weights (the CLIP archive is the file written here)
    monkeypatch.setitem(sys.modules, "clip", None)
    monkeypatch.setattr(clip_util, "_synthetic_text_embedding", lambda *a, **k: pytest.fail("hash fallback used"))
    monkeypatch.chdir(tmp_path)
    path, _ = _full_archive(tmp_path, len(merges))
    clip_util.load_clip.cache_clear()
    try:
        gen = clip_guided_diffusion(prompts=["an owl in a misty forest", "a fox:0.5"], image_size=64, batch_size=1, num_cutouts=2,
                                    timestep_respacing="25", clip_model_name=path, prefix_path=str(tmp_path / "out"),
                                    checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=False, device="cuda")
        items = list(itertools.islice(gen, 2))
        assert len(items) == 2
        for _, p in items:
            assert p.endswith(".png")
    finally:
        clip_util.load_clip.cache_clear()
