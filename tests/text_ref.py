"""CPU fp32 restatement of the CLIP text tower, `clip.model.CLIP.encode_text`.  TEST INFRASTRUCTURE ONLY.

token_embedding(text) + positional_embedding -> `layers` pre-LN residual attention blocks (the image tower's block, with the causal mask of
`CLIP.build_attention_mask`: -inf above the diagonal) -> ln_final -> the row of each sequence at text.argmax(-1) (the end-of-text token)
@ text_projection.  Parameter names equal the OpenAI top-level keys of a CLIP state dict.  Pinned against an independently written
implementation of the same architecture (transformers.CLIPTextModelWithProjection) in tests/test_text_host.py.
"""
import torch as th
import torch.nn as nn

from oracle import clip_vit

TEXT_CONFIGS = {
    # name: (context_length, vocab_size, width, layers, heads, out_dim)   (published CLIP checkpoints)
    "RN50": (77, 49408, 512, 12, 8, 1024),
    "RN101": (77, 49408, 512, 12, 8, 512),
    "RN50x4": (77, 49408, 640, 12, 10, 640),
    "RN50x16": (77, 49408, 768, 12, 12, 768),
    "ViT-B/32": (77, 49408, 512, 12, 8, 512),
    "ViT-B/16": (77, 49408, 512, 12, 8, 512),
    "ViT-L/14": (77, 49408, 768, 12, 12, 768),
}


class CausalBlock(clip_vit.ResidualAttentionBlock):
    def __init__(self, d_model, n_head, context_length):
        super().__init__(d_model, n_head)
        self.register_buffer("attn_mask", th.full((context_length, context_length), float("-inf")).triu_(1), persistent=False)

    def forward(self, x):  # x: (L, N, D)
        y = self.ln_1(x)
        x = x + self.attn(y, y, y, need_weights=False, attn_mask=self.attn_mask)[0]
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads, context_length):
        super().__init__()
        self.resblocks = nn.Sequential(*[CausalBlock(width, heads, context_length) for _ in range(layers)])

    def forward(self, x):
        return self.resblocks(x)


class ClipTextModel(nn.Module):
    def __init__(self, context_length=77, vocab_size=49408, width=512, layers=12, heads=8, out_dim=512):
        super().__init__()
        self.context_length = context_length
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(th.empty(context_length, width))
        self.transformer = Transformer(width, layers, heads, context_length)
        self.ln_final = clip_vit.LayerNorm(width)
        self.text_projection = nn.Parameter(th.empty(width, out_dim))

    def encode_text(self, text):
        x = self.token_embedding(text) + self.positional_embedding
        x = self.transformer(x.permute(1, 0, 2)).permute(1, 0, 2)
        x = self.ln_final(x)
        return x[th.arange(x.shape[0]), text.argmax(dim=-1)] @ self.text_projection

    forward = encode_text


def build(name):
    return ClipTextModel(*TEXT_CONFIGS[name])


def synthetic_init_(model, seed=8642):
    """Seeded synthetic weights with CLIP's initialisation scales (no checkpoints on disk, no network)."""
    g = th.Generator().manual_seed(seed)
    width = model.ln_final.weight.shape[0]
    with th.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")):
                p.copy_(1.0 + 0.02 * th.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.02 * th.randn(p.shape, generator=g))
            elif name == "token_embedding.weight":
                p.copy_(0.02 * th.randn(p.shape, generator=g))
            elif name == "positional_embedding":
                p.copy_(0.01 * th.randn(p.shape, generator=g))
            elif name == "text_projection":
                p.copy_(width ** -0.5 * th.randn(p.shape, generator=g))
            else:
                p.copy_(p[0].numel() ** -0.5 * th.randn(p.shape, generator=g))
    return model


def random_tokens(n, context_length, vocab_size, lengths, seed=0):
    """(n, context_length) int64 like clip.tokenize: start token vocab-2, `lengths[i]` ids in total including start / end, end token vocab-1
    (the maximal id: the end-of-text row), zero padding."""
    g = th.Generator().manual_seed(seed)
    tok = th.zeros(n, context_length, dtype=th.int64)
    for i, length in enumerate(lengths):
        tok[i, 0] = vocab_size - 2
        tok[i, 1:length - 1] = th.randint(0, vocab_size - 2, (length - 2,), generator=g)
        tok[i, length - 1] = vocab_size - 1
    return tok
