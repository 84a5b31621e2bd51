"""PyTorch restatement of the secondary diffusion model (fp32, CPU, autograd) and of the guidance step that uses it: the references of
tests/test_secondary_host.py and tests/test_gpu_secondary.py.

`SecondaryDiffusionImageNet2` is the module of Katherine Crowson's CLIP-guided diffusion notebooks (also shipped with Disco Diffusion),
written out from its published description: c = 64, cs = [64, 128, 128, 256, 256, 512], ConvBlock = Conv2d(3x3, padding 1) + ReLU,
AvgPool2d(2) down, bilinear x2 (align_corners=False) up, SkipBlock(main) = cat([main(x), x], dim=1), a 16-value Fourier embedding of t as
constant planes behind the 3 image channels, and pred = x cos(t pi/2) - v sin(t pi/2).  Its `state_dict()` names are the parameter names the
library's manifest must list.
"""
import math

import torch as th
from torch import nn


class ConvBlock(nn.Sequential):
    def __init__(self, c_in, c_out):
        super().__init__(nn.Conv2d(c_in, c_out, 3, padding=1), nn.ReLU(inplace=False))


class SkipBlock(nn.Module):
    def __init__(self, main):
        super().__init__()
        self.main = nn.Sequential(*main)

    def forward(self, x):
        return th.cat([self.main(x), x], dim=1)


class FourierFeatures(nn.Module):
    def __init__(self, in_features, out_features, std=1.0):
        super().__init__()
        assert out_features % 2 == 0
        self.weight = nn.Parameter(th.randn([out_features // 2, in_features]) * std)

    def forward(self, inp):
        f = 2 * math.pi * inp @ self.weight.T
        return th.cat([f.cos(), f.sin()], dim=-1)


class SecondaryDiffusionImageNet2(nn.Module):
    def __init__(self):
        super().__init__()
        c = 64
        cs = [c, c * 2, c * 2, c * 4, c * 4, c * 8]
        self.timestep_embed = FourierFeatures(1, 16)
        down = lambda: nn.AvgPool2d(2)  # noqa: E731
        up = lambda: nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)  # noqa: E731
        self.net = nn.Sequential(
            ConvBlock(3 + 16, cs[0]), ConvBlock(cs[0], cs[0]),
            SkipBlock([down(), ConvBlock(cs[0], cs[1]), ConvBlock(cs[1], cs[1]),
                       SkipBlock([down(), ConvBlock(cs[1], cs[2]), ConvBlock(cs[2], cs[2]),
                                  SkipBlock([down(), ConvBlock(cs[2], cs[3]), ConvBlock(cs[3], cs[3]),
                                             SkipBlock([down(), ConvBlock(cs[3], cs[4]), ConvBlock(cs[4], cs[4]),
                                                        SkipBlock([down(), ConvBlock(cs[4], cs[5]), ConvBlock(cs[5], cs[5]),
                                                                   ConvBlock(cs[5], cs[5]), ConvBlock(cs[5], cs[4]), up()]),
                                                        ConvBlock(cs[4] * 2, cs[4]), ConvBlock(cs[4], cs[3]), up()]),
                                             ConvBlock(cs[3] * 2, cs[3]), ConvBlock(cs[3], cs[2]), up()]),
                                  ConvBlock(cs[2] * 2, cs[2]), ConvBlock(cs[2], cs[1]), up()]),
                       ConvBlock(cs[1] * 2, cs[1]), ConvBlock(cs[1], cs[0]), up()]),
            ConvBlock(cs[0] * 2, cs[0]), nn.Conv2d(cs[0], 3, 3, padding=1))

    def v(self, x, t):
        emb = self.timestep_embed(t[:, None])
        planes = emb[:, :, None, None].expand(-1, -1, x.shape[2], x.shape[3])
        return self.net(th.cat([x, planes], dim=1))

    def forward(self, x, t):
        """x (B,3,H,W), t (B,) in [0,1] -> pred"""
        v = self.v(x, t)
        alpha, sigma = th.cos(t * math.pi / 2), th.sin(t * math.pi / 2)
        return x * alpha[:, None, None, None] - v * sigma[:, None, None, None]


def build(sd=None):
    """The module in eval mode with frozen parameters, optionally loaded from a state dict (flat tensors are reshaped by name)."""
    net = SecondaryDiffusionImageNet2().eval()
    if sd is not None:
        own = net.state_dict()
        net.load_state_dict({k: sd[k].detach().float().cpu().reshape(own[k].shape) for k in own})
    for p in net.parameters():
        p.requires_grad_(False)
    return net


class CaptureRelu:
    """Records the output of every ReLU of the module in execution order (the 23 post-ReLU activations a mask replay hands to the device)."""

    def __init__(self, net):
        self.net, self.acts, self.hooks = net, [], []

    def __enter__(self):
        for m in self.net.modules():
            if isinstance(m, nn.ReLU):
                self.hooks.append(m.register_forward_hook(lambda mod, inp, out: self.acts.append(out.detach())))
        return self

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()


def model_time(alpha, sigma):
    """float64: the model's time of a noise level (alpha, sigma) = (cos(t pi/2), sin(t pi/2))"""
    return math.atan2(sigma, alpha) * 2.0 / math.pi


def guided_step(net, x, diffusion, current_timestep, **cond_kwargs):
    """Guidance with the secondary model, by autograd: pred = net(x, t) at t = atan2(sigma_i, alpha_i) 2/pi of table row
    i = current_timestep, handed to the oracle's cond_fn (oracle/guidance.py, the restatement of the reference's closure) as
    out['pred_xstart']: x_in = pred fac + x (1 - fac) with fac = sigma_i, CLIP / tv / saturation on x_in, range on pred, g = -dL/dx through
    the secondary net (then the magnitude clamp).  -> (g, state) with state['log'], state['legs'] (incl. 'g_raw' before the clamp)."""
    from oracle import guidance as og
    i = current_timestep
    alpha, sigma = float(diffusion.sqrt_alphas_cumprod[i]), float(diffusion.sqrt_one_minus_alphas_cumprod[i])
    cond_fn, st = og.make_cond_fn(diffusion=diffusion, **cond_kwargs)
    st["current_timestep"] = i
    st["diag"] = True
    with th.enable_grad():
        xr = x.detach().float().requires_grad_()
        t = th.full((x.shape[0],), model_time(alpha, sigma), dtype=th.float32)
        pred = net(xr, t)
        g = cond_fn(xr, th.full((x.shape[0],), i, dtype=th.long), {"pred_xstart": pred})
    st["pred"] = pred.detach()
    return g.detach(), st
