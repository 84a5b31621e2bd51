"""CPU reference of guided-diffusion's UNetModel with the two architecture switches the community checkpoints use.  TEST INFRASTRUCTURE ONLY.

    resblock_updown=False      Downsample = Conv2d(ch, ch, 3, stride=2, padding=1) under the key `op`; Upsample = nearest 2x, then
                               Conv2d(ch, ch, 3, padding=1) under the key `conv` (upstream conv_resample=True)
    use_scale_shift_norm=False h = conv1(SiLU(GN1(x))) + emb_layers(emb)[:, :, None, None]; then GN2 -> SiLU -> conv2

With both switches True this is oracle/unet.py's network, key for key (tests/test_classic_unet_host.py asserts equal outputs on one state
dict), which anchors the new reference to the trusted one.  The norms, the attention block and the timestep embedding ARE oracle/unet.py's.
Written from the published architecture of openai/improved-diffusion and openai/guided-diffusion (unet.py: ResBlock, Downsample, Upsample).
"""
import torch as th
import torch.nn as nn
import torch.nn.functional as F

from oracle.unet import AttentionBlock, GroupNorm32, Resample, default_channel_mult, synthetic_init_, timestep_embedding  # noqa: F401


class Downsample(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.op = nn.Conv2d(channels, channels, 3, stride=2, padding=1)

    def forward(self, x):
        return self.op(x)


class Upsample(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)

    def forward(self, x):
        return self.conv(F.interpolate(x, scale_factor=2, mode="nearest"))


class ResBlock(nn.Module):
    def __init__(self, channels, emb_channels, out_channels, up=False, down=False, use_scale_shift_norm=True):
        super().__init__()
        self.film = use_scale_shift_norm
        self.in_layers = nn.Sequential(GroupNorm32(32, channels), nn.SiLU(), nn.Conv2d(channels, out_channels, 3, padding=1))
        self.updown = up or down
        if self.updown:
            self.h_upd = Resample(up)
            self.x_upd = Resample(up)
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, 2 * out_channels if self.film else out_channels))
        self.out_layers = nn.Sequential(GroupNorm32(32, out_channels), nn.SiLU(), nn.Dropout(0.0),
                                        nn.Conv2d(out_channels, out_channels, 3, padding=1))
        self.skip_connection = nn.Identity() if out_channels == channels else nn.Conv2d(channels, out_channels, 1)

    def forward(self, x, emb):
        if self.updown:
            h = self.in_layers[1](self.in_layers[0](x))
            h = self.h_upd(h)
            x = self.x_upd(x)
            h = self.in_layers[2](h)
        else:
            h = self.in_layers(x)
        e = self.emb_layers(emb)[..., None, None]
        if self.film:
            scale, shift = th.chunk(e, 2, dim=1)
            h = self.out_layers[0](h) * (1 + scale) + shift
            h = self.out_layers[3](self.out_layers[2](self.out_layers[1](h)))
        else:
            h = self.out_layers(h + e)
        return self.skip_connection(x) + h


class Seq(nn.Sequential):
    def forward(self, x, emb):
        for layer in self:
            x = layer(x, emb) if isinstance(layer, ResBlock) else layer(x)
        return x


class ClassicUNetModel(nn.Module):
    def __init__(self, image_size, model_channels, num_res_blocks, attention_resolutions="32,16,8", channel_mult=None, num_classes=None,
                 num_heads=4, num_head_channels=-1, use_new_attention_order=False, in_channels=3, out_channels=6, resblock_updown=True,
                 use_scale_shift_norm=True):
        super().__init__()
        if channel_mult is None:
            channel_mult = default_channel_mult(image_size)
        attention_ds = [image_size // int(r) for r in str(attention_resolutions).split(",")]
        self.model_channels, self.num_classes = model_channels, num_classes
        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.SiLU(), nn.Linear(ted, ted))
        if num_classes is not None:
            self.label_emb = nn.Embedding(num_classes, ted)
        att = dict(num_heads=num_heads, num_head_channels=num_head_channels, use_new_attention_order=use_new_attention_order)
        rb = dict(use_scale_shift_norm=use_scale_shift_norm)

        ch = input_ch = int(channel_mult[0] * model_channels)
        self.input_blocks = nn.ModuleList([Seq(nn.Conv2d(in_channels, ch, 3, padding=1))])
        chans = [ch]
        ds = 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, ted, int(mult * model_channels), **rb)]
                ch = int(mult * model_channels)
                if ds in attention_ds:
                    layers.append(AttentionBlock(ch, **att))
                self.input_blocks.append(Seq(*layers))
                chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(Seq(ResBlock(ch, ted, ch, down=True, **rb) if resblock_updown else Downsample(ch)))
                chans.append(ch)
                ds *= 2
        self.middle_block = Seq(ResBlock(ch, ted, ch, **rb), AttentionBlock(ch, **att), ResBlock(ch, ted, ch, **rb))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [ResBlock(ch + ich, ted, int(model_channels * mult), **rb)]
                ch = int(model_channels * mult)
                if ds in attention_ds:
                    layers.append(AttentionBlock(ch, **att))
                if level and i == num_res_blocks:
                    layers.append(ResBlock(ch, ted, ch, up=True, **rb) if resblock_updown else Upsample(ch))
                    ds //= 2
                self.output_blocks.append(Seq(*layers))
        self.out = nn.Sequential(GroupNorm32(32, ch), nn.SiLU(), nn.Conv2d(input_ch, out_channels, 3, padding=1))

    def forward(self, x, timesteps, y=None):
        emb = self.time_embed(timestep_embedding(timesteps, self.model_channels))
        if self.num_classes is not None:
            emb = emb + self.label_emb(y)
        hs = []
        h = x
        for m in self.input_blocks:
            h = m(h, emb)
            hs.append(h)
        h = self.middle_block(h, emb)
        for m in self.output_blocks:
            h = th.cat([h, hs.pop()], dim=1)
            h = m(h, emb)
        return self.out(h)


FLAG_COMBOS = [(True, True), (True, False), (False, True), (False, False)]  # (resblock_updown, use_scale_shift_norm)
TINY = dict(image_size=32, model_channels=64, num_res_blocks=1, attention_resolutions="16", channel_mult=(1, 2), num_heads=1)
# the comics-faces / pixel-art configuration (cgd.model_flags.COMMUNITY_LOOKUP)
COMICS = dict(image_size=256, model_channels=128, num_res_blocks=2, attention_resolutions="16", num_heads=1)
# the STRUCTURE of that configuration at a quarter of its width: six levels, five Downsamples and Upsamples, two ResBlocks per level, one-head
# attention where the map is 1 / 16 of the frame (128 channels here, 512 in the checkpoints); frames must be multiples of 32
NARROW = dict(COMICS, model_channels=32, channel_mult=(1, 1, 2, 2, 4, 4))
CASES = {"tiny": TINY, "narrow": NARROW, "comics": COMICS}
