"""fp64 reference of the VGG Gram-matrix style loss (TEST INFRASTRUCTURE ONLY): Gram matrices, the loss and its gradient by autograd through
`oracle.lpips_vgg.LpipsVGG.features`, which is imported and left as it is.

For tap k of sample b, A_k = the post-ReLU activation [N_k][C_k] of the LPIPS trunk on the scaled input (N_k = H_k W_k; C_k = 64, 128, 256, 512, 512):
    G_k(x)[b]    = A_k^T A_k / (C_k N_k)
    L_style[b]   = sum_k lambda_k |G_k(x)[b] - G_k(style)|_F^2
    dL[b] / dA_k = lambda_k 4 / (C_k N_k) A_k (G_k(x)[b] - G_k(style))
"""
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 0.0)


def gram(a):
    """(B,C,H,W) tap -> (B,C,C): A^T A / (C N) with A the [N][C] pixel rows of each sample."""
    B, C, H, W = a.shape
    f = a.reshape(B, C, H * W)
    return f @ f.transpose(1, 2) / (C * H * W)


def style_grams(orc, style):
    """The five G_k(style) of ONE style image (1,3,Hs,Ws), each (C_k, C_k), detached."""
    assert style.shape[0] == 1
    with th.no_grad():
        return [gram(t)[0] for t in orc.features(style)]


def tap_losses(taps, grams_s, weights=DEFAULT_WEIGHTS):
    """(B,) = sum_k lambda_k |G_k - G_k(style)|_F^2 from a list of the five taps."""
    total = 0
    for k, lam in enumerate(weights):
        if lam:
            total = total + lam * (gram(taps[k]) - grams_s[k]).pow(2).sum(dim=(1, 2))
    return total


def style_loss(orc, x, grams_s, weights=DEFAULT_WEIGHTS):
    return tap_losses(orc.features(x), grams_s, weights)


def style_loss_and_grad(orc, x, style, weights=DEFAULT_WEIGHTS):
    """(loss (B,), d(sum_b loss)/dx, rel) in the dtype of x (use fp64); rel: per tap, the smallest |G_k(x)[b] - G_k(style)|_F / |G_k(style)|_F over
    the batch, which says whether the loss is a difference of near-equal numbers."""
    gs = style_grams(orc, style)
    xr = x.detach().clone().requires_grad_()
    taps = orc.features(xr)
    loss = tap_losses(taps, gs, weights)
    loss.sum().backward()
    with th.no_grad():
        rel = [float(((gram(t) - g).flatten(1).norm(dim=1) / g.norm()).min()) for t, g in zip(taps, gs)]
    return loss.detach(), xr.grad.detach(), rel


def closed_form_tap_grad(a, gram_s, lam):
    """dL/dA_k of the module docstring for a tap a (B,C,H,W), as a (B,C,H,W) tensor."""
    B, C, H, W = a.shape
    d = gram(a) - gram_s  # (B,C,C), symmetric
    return lam * 4.0 / (C * H * W) * (d @ a.reshape(B, C, H * W)).reshape(B, C, H, W)


class LpipsPlusStyle(th.nn.Module):
    """Stands in for the oracle's LPIPS module in `oracle.guidance.make_cond_fn`, which computes `lpips_model(x_in, init).sum() * init_scale`:
    returns lpips_weight * lpips(in0, in1) + style_weight * L_style(in0) per sample, shaped like the module's output (B,1,1,1).  With
    init_scale = S on the oracle's side, lpips_weight = init_scale / S and style_weight = style_scale / S add both terms at their own scales."""

    def __init__(self, orc, style, weights=DEFAULT_WEIGHTS, lpips_weight=1.0, style_weight=1.0):
        super().__init__()
        self.orc, self.weights, self.lpips_weight, self.style_weight = orc, tuple(weights), float(lpips_weight), float(style_weight)
        self.grams = style_grams(orc, style.to(next(orc.parameters()).dtype))

    def lpips_state_dict(self):
        return self.orc.lpips_state_dict()

    def forward(self, in0, in1):
        taps = self.orc.features(in0)
        val = self.style_weight * tap_losses(taps, self.grams, self.weights).view(-1, 1, 1, 1)
        if self.lpips_weight:
            f1 = self.orc.features(in1)
            for k in range(5):
                d = (self.orc.normalize_tensor(taps[k]) - self.orc.normalize_tensor(f1[k])) ** 2
                val = val + self.lpips_weight * self.orc.lins[k](d).mean(dim=(2, 3), keepdim=True)
        return val
