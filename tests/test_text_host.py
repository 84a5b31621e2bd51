"""CPU checks of the CLIP text tower's host side: the fp32 restatement (tests/text_ref.py) against an independent implementation, published
parameter counts, the library's host-only parameter manifest, the tokenizer against transformers' CLIP tokenizer, and the drop-in's
configuration inference."""
import collections
import gzip
import json

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib, nets, tokenizer
from tests import text_ref

CORPUS = ("an owl in a misty forest at dawn, oil painting", "a fox jumping over the lazy dog", "portrait of an old sailor, dramatic lighting",
          "the city skyline at night; neon reflections on wet streets", "a bowl of fruit: apples, pears & grapes", "watercolor owl",
          "it's a beautiful day, isn't it?", "trending on artstation 4k", "a red cube on a blue sphere", "foggy mountains")


def _map_to_hf(sd, layers, W):
    m = {"text_model.embeddings.token_embedding.weight": sd["token_embedding.weight"],
         "text_model.embeddings.position_embedding.weight": sd["positional_embedding"],
         "text_model.final_layer_norm.weight": sd["ln_final.weight"], "text_model.final_layer_norm.bias": sd["ln_final.bias"],
         "text_projection.weight": sd["text_projection"].T.contiguous()}
    for l in range(layers):
        p, q = f"transformer.resblocks.{l}.", f"text_model.encoder.layers.{l}."
        w, b = sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"]
        for i, n in enumerate(("q_proj", "k_proj", "v_proj")):
            m[q + f"self_attn.{n}.weight"], m[q + f"self_attn.{n}.bias"] = w[i * W:(i + 1) * W], b[i * W:(i + 1) * W]
        m[q + "self_attn.out_proj.weight"], m[q + "self_attn.out_proj.bias"] = sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"]
        m[q + "layer_norm1.weight"], m[q + "layer_norm1.bias"] = sd[p + "ln_1.weight"], sd[p + "ln_1.bias"]
        m[q + "layer_norm2.weight"], m[q + "layer_norm2.bias"] = sd[p + "ln_2.weight"], sd[p + "ln_2.bias"]
        m[q + "mlp.fc1.weight"], m[q + "mlp.fc1.bias"] = sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"]
        m[q + "mlp.fc2.weight"], m[q + "mlp.fc2.bias"] = sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"]
    return m


def test_text_ref_matches_hf_clip_text_model():
    tr = pytest.importorskip("transformers")
    T, V, W, L, H, D = 16, 300, 128, 2, 2, 64
    # eos_token_id = 2: transformers' pooling at input_ids.argmax(-1), CLIP's own end-of-text convention
    cfg = tr.CLIPTextConfig(vocab_size=V, hidden_size=W, intermediate_size=4 * W, num_hidden_layers=L, num_attention_heads=H,
                            max_position_embeddings=T, projection_dim=D, hidden_act="quick_gelu", eos_token_id=2)
    hf = tr.CLIPTextModelWithProjection(cfg).eval()
    ours = text_ref.synthetic_init_(text_ref.ClipTextModel(T, V, W, L, H, D)).eval()
    missing, unexpected = hf.load_state_dict(_map_to_hf(ours.state_dict(), L, W), strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    tok = text_ref.random_tokens(3, T, V, [16, 5, 9], seed=1)
    with th.no_grad():
        a, b = ours.encode_text(tok), hf(input_ids=tok).text_embeds
    assert th.allclose(a, b, rtol=1e-4, atol=1e-5), (a - b).abs().max()
    # the mask matters: the same tower without it gives another embedding for the short prompts
    for blk in ours.transformer.resblocks:
        blk.attn_mask = th.zeros_like(blk.attn_mask)
    with th.no_grad():
        assert not th.allclose(ours.encode_text(tok)[1:], b[1:], rtol=1e-3, atol=1e-3)


def test_vit_b32_text_tower_parameter_count():
    # published ViT-B/32 CLIP total 151,277,313 = 87,849,216 (image tower) + 63,428,096 (text tower) + 1 (logit_scale)
    assert sum(p.numel() for p in text_ref.build("ViT-B/32").parameters()) == 63_428_096 == 151_277_313 - 87_849_216 - 1
    assert sum(k for _, k in nets.manifest("text", lib.TextConfig(*nets.TEXT_CONFIGS["ViT-B/32"]))) == 63_428_096


@pytest.mark.parametrize("name", sorted(text_ref.TEXT_CONFIGS))
def test_text_manifest_equals_restatement_state_dict(name):
    assert nets.TEXT_CONFIGS[name] == text_ref.TEXT_CONFIGS[name]
    man = nets.manifest("text", lib.TextConfig(*nets.TEXT_CONFIGS[name]))
    ref = [(k, v.numel()) for k, v in text_ref.build(name).state_dict().items()]
    assert sorted(man) == sorted(ref)


def test_text_manifest_rejects_bad_configurations():
    with pytest.raises(ValueError):
        nets.manifest("text", lib.TextConfig(77, 49408, 500, 12, 8, 512))  # head dim 62.5
    with pytest.raises(ValueError):
        nets.manifest("text", lib.TextConfig(0, 49408, 512, 12, 8, 512))


@pytest.mark.parametrize("name", sorted(text_ref.TEXT_CONFIGS))
def test_text_config_round_trips_through_state_dict(name):
    from cgd import clip_util
    with th.device("meta"):
        sd = text_ref.build(name).state_dict()
    sd["visual.proj"] = th.empty(768, 512, device="meta")  # image-tower keys next to the text keys, like a full CLIP archive
    sd["visual.transformer.resblocks.0.attn.in_proj_weight"] = th.empty(1, device="meta")
    sd["logit_scale"] = th.empty((), device="meta")
    assert clip_util._text_config_from_state_dict(sd) == text_ref.TEXT_CONFIGS[name]
    assert sorted(k for k in sd if clip_util._is_text_key(k)) == sorted(text_ref.build(name).state_dict())


# ---- tokenizer ------------------------------------------------------------------------------------------------------------------------
def learn_merges(corpus, n_merges):
    """A small BPE merges table learnt from `corpus` (standard BPE training: repeatedly merge the most frequent adjacent pair, ties broken
    by the pair itself), on CLIP's pre-tokenised, byte-encoded words with the end-of-word marker."""
    b2u = tokenizer.bytes_to_unicode()
    words = collections.Counter()
    for text in corpus:
        for piece in tokenizer._PATTERN.findall(tokenizer._clean(text)):
            chars = [b2u[b] for b in piece.encode("utf-8")]
            words[tuple(chars[:-1] + [chars[-1] + "</w>"])] += 1
    merges = []
    for _ in range(n_merges):
        pairs = collections.Counter()
        for w, c in words.items():
            for p in zip(w, w[1:]):
                pairs[p] += c
        if not pairs:
            break
        best = max(pairs.items(), key=lambda kv: (kv[1], kv[0]))[0]
        merges.append(best)
        new = collections.Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1])
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            new[tuple(out)] += c
        words = new
    return merges


def write_bpe(path, merges):
    with gzip.open(path, "wt", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "".join(f"{a} {b}\n" for a, b in merges))
    return path


@pytest.fixture
def synthetic_bpe(tmp_path):
    merges = learn_merges(CORPUS, 150)
    assert len(merges) == 150
    return write_bpe(str(tmp_path / tokenizer.BPE_FILENAME), merges), merges


def test_tokenizer_matches_transformers(synthetic_bpe):
    tr = pytest.importorskip("transformers")
    path, merges = synthetic_bpe
    ours = tokenizer.SimpleTokenizer(path)
    chars = list(tokenizer.bytes_to_unicode().values())
    vocab = chars + [c + "</w>" for c in chars] + [a + b for a, b in merges] + ["<|startoftext|>", "<|endoftext|>"]
    assert len(set(vocab)) == len(vocab) == 512 + 150 + 2
    hf = tr.CLIPTokenizer(vocab=json.loads(json.dumps({t: i for i, t in enumerate(vocab)})), merges=[(a, b) for a, b in merges])
    prompts = list(CORPUS) + ["An  OWL\tin the   FOREST", "unseen words: zebra quokka 1234 !!", "a&amp;b &lt;tag&gt;", "x", "", "mixed-Case & punctuation..."]
    for p in prompts:
        a = ours.encode(p)
        b = hf(p.replace("&amp;", "&").replace("&lt;", "<").replace("&gt;", ">"), add_special_tokens=False)["input_ids"]
        assert a == b, (p, a, b)
    tok = tokenizer.tokenize(prompts, tokenizer=ours)
    assert tok.dtype == th.int64 and tok.shape == (len(prompts), 77)
    for row, p in zip(tok, prompts):
        ids = hf(p.replace("&amp;", "&").replace("&lt;", "<").replace("&gt;", ">"))["input_ids"]  # <|startoftext|> ... <|endoftext|>
        assert row[:len(ids)].tolist() == ids and not row[len(ids):].any()
        assert int(row.argmax()) == len(ids) - 1  # the end-of-text token is the first maximal id


def test_tokenize_overflow_and_truncate(synthetic_bpe):
    path, _ = synthetic_bpe
    tk = tokenizer.SimpleTokenizer(path)
    long = " ".join(["owl"] * 80)
    with pytest.raises(RuntimeError, match="too long for context length 77"):
        tokenizer.tokenize(long, tokenizer=tk)
    t = tokenizer.tokenize([long, "owl"], truncate=True, tokenizer=tk)
    ids = [tk.sot] + tk.encode(long) + [tk.eot]
    assert t[0, :76].tolist() == ids[:76] and int(t[0, 76]) == tk.eot
    assert t[1, :3].tolist() == [tk.sot] + tk.encode("owl") + [tk.eot] and not t[1, 3:].any()
    exact = " ".join(["owl"] * 75)  # 75 ids + start + end = 77: fits without truncation
    assert len(tk.encode(exact)) == 75 and int(tokenizer.tokenize(exact, tokenizer=tk)[0, 76]) == tk.eot


def test_bpe_file_lookup(tmp_path, monkeypatch, synthetic_bpe):
    path, _ = synthetic_bpe
    monkeypatch.delenv("CGD_CLIP_BPE", raising=False)
    with pytest.raises(FileNotFoundError) as e:
        tokenizer.bpe_path(str(tmp_path / "nowhere"))
    assert "CGD_CLIP_BPE" in str(e.value) and str(tmp_path / "nowhere" / "clip" / tokenizer.BPE_FILENAME) in str(e.value)
    (tmp_path / "ck" / "clip").mkdir(parents=True)
    dst = tmp_path / "ck" / "clip" / tokenizer.BPE_FILENAME
    dst.write_bytes(open(path, "rb").read())
    assert tokenizer.bpe_path(str(tmp_path / "ck")) == str(dst)
    monkeypatch.setenv("CGD_CLIP_BPE", path)
    assert tokenizer.bpe_path(str(tmp_path / "nowhere")) == path


def test_text_tower_rejects_bad_tokens_before_the_device():
    """The id range check runs in Python before any launch (the kernel itself never reads outside the table)."""
    tower = nets.ClipTextTower.__new__(nets.ClipTextTower)  # no context: the checks come first
    tower.context_length, tower.vocab_size = 8, 100
    for bad in (th.zeros(2, 7, dtype=th.int64), th.zeros(8, dtype=th.int64), th.zeros(2, 8), th.zeros(0, 8, dtype=th.int64),
                th.full((1, 8), 100, dtype=th.int64), th.full((1, 8), -1, dtype=th.int32)):
        with pytest.raises(ValueError):
            tower.encode_text(bad)
