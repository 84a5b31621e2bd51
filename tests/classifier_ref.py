"""CPU reference (fp32, autograd) of guided-diffusion's noisy ImageNet classifier: `EncoderUNetModel` with pool="attention", assembled from
the oracle UNet's own ResBlock / AttentionBlock / GroupNorm32 / timestep_embedding, plus `AttentionPool2d` written out from the published
source.  Its `state_dict()` names are the names the library's manifest must list."""
import math

import torch as th
import torch.nn as nn

from oracle.unet import AttentionBlock, GroupNorm32, ResBlock, TimestepEmbedSequential, default_channel_mult, timestep_embedding

# the two small configurations of the GPU tests (keyword arguments of EncoderUNetModel and of nets.NoisyClassifier alike)
MINI = {
    # final map 8x8: T = 65 tokens as in production; attention at two levels, one 64-wide head at the first of them
    "clsA": dict(image_size=32, model_channels=64, num_res_blocks=1, attention_resolutions="16,8", channel_mult=(1, 2, 2), num_head_channels=64,
                 out_channels=10),
    # final map 4x4: T = 17 (an odd key count below one wavefront), 32-wide heads, 7 classes, depth 2
    "clsB": dict(image_size=16, model_channels=32, num_res_blocks=2, attention_resolutions="4", channel_mult=(1, 2, 4), num_head_channels=32,
                 out_channels=7),
}


class AttentionPool2d(nn.Module):
    """guided_diffusion.unet.AttentionPool2d (adapted there from CLIP): tokens = [mean | positions] + positional embedding, qkv_proj, the NEW
    attention order (q, k, v = chunk(3, dim=1), then heads; each operand scaled by d^-1/4), c_proj, token 0."""

    def __init__(self, spacial_dim, embed_dim, num_heads_channels, output_dim=None):
        super().__init__()
        self.positional_embedding = nn.Parameter(th.randn(embed_dim, spacial_dim ** 2 + 1) / embed_dim ** 0.5)
        self.qkv_proj = nn.Conv1d(embed_dim, 3 * embed_dim, 1)
        self.c_proj = nn.Conv1d(embed_dim, output_dim or embed_dim, 1)
        self.num_heads = embed_dim // num_heads_channels

    def tokens(self, x):
        b, c = x.shape[:2]
        x = x.reshape(b, c, -1)
        x = th.cat([x.mean(dim=-1, keepdim=True), x], dim=-1)
        return x + self.positional_embedding[None, :, :].to(x.dtype)

    def attend(self, qkv):
        bs, width, length = qkv.shape
        ch = width // (3 * self.num_heads)
        q, k, v = qkv.chunk(3, dim=1)
        scale = 1 / math.sqrt(math.sqrt(ch))
        weight = th.einsum("bct,bcs->bts", (q * scale).view(bs * self.num_heads, ch, length), (k * scale).view(bs * self.num_heads, ch, length))
        weight = th.softmax(weight.float(), dim=-1).type(weight.dtype)
        a = th.einsum("bts,bcs->bct", weight, v.reshape(bs * self.num_heads, ch, length))
        return a.reshape(bs, -1, length)

    def pooled(self, x):
        """token 0 of the attention output, in front of c_proj: (B, C)"""
        return self.attend(self.qkv_proj(self.tokens(x)))[:, :, 0]

    def forward(self, x):
        return self.c_proj(self.attend(self.qkv_proj(self.tokens(x))))[:, :, 0]


class EncoderUNetModel(nn.Module):
    """guided_diffusion.unet.EncoderUNetModel as create_classifier builds it: use_scale_shift_norm, resblock_updown, legacy attention order,
    pool="attention"."""

    def __init__(self, image_size, model_channels=128, num_res_blocks=2, attention_resolutions="32,16,8", channel_mult=None,
                 num_head_channels=64, out_channels=1000, in_channels=3):
        super().__init__()
        if channel_mult is None:
            channel_mult = default_channel_mult(image_size)
        attention_ds = [image_size // int(r) for r in str(attention_resolutions).split(",")]
        self.model_channels = model_channels
        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.SiLU(), nn.Linear(ted, ted))
        ch = int(channel_mult[0] * model_channels)
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(nn.Conv2d(in_channels, ch, 3, padding=1))])
        ds = 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, ted, int(mult * model_channels))]
                ch = int(mult * model_channels)
                if ds in attention_ds:
                    layers.append(AttentionBlock(ch, num_head_channels=num_head_channels))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(ResBlock(ch, ted, ch, down=True)))
                ds *= 2
        self.middle_block = TimestepEmbedSequential(ResBlock(ch, ted, ch), AttentionBlock(ch, num_head_channels=num_head_channels),
                                                    ResBlock(ch, ted, ch))
        self.out = nn.Sequential(GroupNorm32(32, ch), nn.SiLU(), AttentionPool2d(image_size // ds, ch, num_head_channels, out_channels))

    def features(self, x, timesteps):
        """the input of the pool: SiLU(GroupNorm(middle_block output)), (B, C, S, S)"""
        emb = self.time_embed(timestep_embedding(timesteps, self.model_channels))
        h = x
        for m in self.input_blocks:
            h = m(h, emb)
        h = self.middle_block(h, emb)
        return self.out[1](self.out[0](h))

    def forward(self, x, timesteps):
        return self.out[2](self.features(x, timesteps))


def logp_of(logits, y):
    """log p(y | .) per sample: log_softmax(logits)[range(B), y], as guided-diffusion's classifier cond_fn selects it"""
    return th.log_softmax(logits, dim=-1)[th.arange(logits.shape[0]), y.view(-1)]


def build(sd, **kw):
    """The reference net of a configuration on a given state dict (fp32, eval, no parameter gradients)."""
    net = EncoderUNetModel(**kw)
    net.load_state_dict({k: v.detach().cpu().float().view_as(net.state_dict()[k]) for k, v in sd.items()})
    net.eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net
