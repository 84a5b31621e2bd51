"""Restatement of dynamic thresholding of the guided pred_xstart under DPM-Solver++(2M) (Saharia et al., 2022, "dynamic thresholding"; Lu et
al., 2022), on top of tests/dpm_ref.py.  TEST INFRASTRUCTURE ONLY.

Per evaluation, with x0c the guided pred_xstart and, per sample, a = |x0c| flattened to n values, v_j its j-th smallest (torch.sort):

    pos = p (n - 1), k = floor(pos), frac = pos - k      (float64; frac rounded to float32, as the device receives it)
    q   = v_k + (v_{k+1} - v_k) frac                     (k + 1 clamped to n - 1; torch.quantile's 'linear' rule)
    s   = min(max(q, 1), cap)
    x0t = clamp(x0c, -s, s) / s

and x0t takes x0c's place in the update and in the history; the yielded pred_xstart stays the unguided one.  Coefficients are float64.
"""
import math

import numpy as np
import torch as th

from oracle import diffusion as od
from tests import dpm_ref


def rank(p, n):
    pos = float(p) * (n - 1)
    k = min(int(math.floor(pos)), n - 1)
    return k, pos - k


def row_scale(a_sorted, p, cap=math.inf, floor=1.0):
    """s of one sample from its sorted absolute values (any float dtype), evaluated in float64"""
    n = a_sorted.numel()
    k, frac = rank(p, n)
    vk, vk1 = float(a_sorted[k]), float(a_sorted[min(k + 1, n - 1)])
    q = vk + (vk1 - vk) * float(np.float32(frac))
    return min(max(q, floor), cap)


def scales(x0c, p, cap=math.inf):
    """(B,) float64 scales of a (B, ...) tensor"""
    flat = x0c.detach().abs().flatten(1)
    return th.tensor([row_scale(th.sort(r).values, p, cap) for r in flat], dtype=th.float64)


def threshold(x0c, p, cap=math.inf):
    """-> (x0t in x0c's dtype, the scales)"""
    s = scales(x0c, p, cap).to(x0c.dtype).view(-1, *([1] * (x0c.dim() - 1)))
    return th.maximum(th.minimum(x0c, s), -s) / s, s.flatten()


class ThresholdDiffusion(dpm_ref.DPMDiffusion):
    threshold = None  # None or (p, cap)

    def dpmpp_sample(self, model, x, t, cond_fn=None, model_kwargs=None, order=2, eta=0.0, noise=None, hist=None):
        if self.threshold is None:
            return super().dpmpp_sample(model, x, t, cond_fn, model_kwargs, order, eta, noise, hist)
        i = int(t[0])
        _, x0c, x0 = self.guided_eval(model, x, t, cond_fn, model_kwargs)
        x0t, s = threshold(x0c, *self.threshold)
        self.seen_scales.append(s.double())
        self.seen_excess.append(x0c.abs().flatten(1).max(dim=1).values.double())
        eff = 2 if (order == 2 and hist is not None and i > 0) else 1
        c_x, c_d, c_r, c_n = self.step_coefs(i, eff, eta)
        d = x0t + c_r * (x0t - hist) if eff == 2 else x0t
        sample = x0t
        if i > 0:
            sample = c_x * x + c_d * d
            if c_n:
                sample = sample + c_n * noise
        return {"sample": sample, "pred_xstart": x0, "x0c": x0t}


def create_threshold_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="", rescale_timesteps=False, threshold=None):
    """`threshold`: None, p or (p, cap).  The object records the scales of every evaluation in `seen_scales` ((B,) per step)."""
    betas = od.get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    diff = ThresholdDiffusion(dpm_ref.space_timesteps(steps, timestep_respacing, betas), betas, rescale_timesteps=rescale_timesteps)
    if threshold is not None:
        diff.threshold = tuple(threshold) if isinstance(threshold, (tuple, list)) else (threshold, math.inf)
    diff.seen_scales, diff.seen_excess = [], []
    return diff
