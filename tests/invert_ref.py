"""Restatement of DDIM inversion (guided_diffusion's `ddim_reverse_sample` / `ddim_reverse_sample_loop`: the deterministic DDIM ODE run
upwards from an image) on top of the CPU oracle.  TEST INFRASTRUCTURE ONLY.

One step at index i takes the state from level i to level i + 1 (unguided, clip_denoised=False):

    eps         = the model's output, channels 0..2
    pred_xstart = sqrt_recip[i] x - sqrt_recipm1[i] eps                      (the oracle's p_mean_variance)
    x_next      = sqrt(abar_next[i]) pred_xstart + sqrt(1 - abar_next[i]) eps

eps is taken from the model.  Upstream re-derives it from pred_xstart, (sqrt_recip x - pred_xstart) / sqrt_recipm1: the same number in exact
arithmetic, divided by sqrt_recipm1[0] ~ 0.01 in floating point.  The loop runs indices 0 .. t0 - 1, t0 = num_timesteps - 1 - skip_timesteps,
and the clean image is treated as the state at level 0 (upstream's one-level offset).  `implied_noise` is the tensor for which
q_sample(image, t0, noise) == latent, so that the oracle's sampling loops start from the latent when given `noise=noise, init_image=image,
skip_timesteps=skip`.
"""
import contextlib

import torch as th

from oracle import diffusion as od
from tests import masked_ref


@contextlib.contextmanager
def float64_tables():
    """The oracle's `_extract` rounds every table entry to float32 (the reference's dtype).  Inside this context it keeps them float64, so
    that the oracle's own steps, given float64 states and a float64 model, run in float64 throughout."""
    plain = od._extract

    def extract64(arr, t, shape):
        res = th.from_numpy(arr).to(t.device)[t].double()
        while res.dim() < len(shape):
            res = res[..., None]
        return res.expand(shape)

    od._extract = extract64
    try:
        yield
    finally:
        od._extract = plain


class InvertDiffusion(masked_ref.MaskedDiffusion):
    def ddim_reverse_sample(self, model, x, t, model_kwargs=None):
        """-> {"sample": the state at level t + 1, "pred_xstart"}"""
        seen = {}

        def keeping(x_, ts, **kw):
            out = model(x_, ts, **kw)
            seen["eps"] = out[:, :3]
            return out

        with th.no_grad():
            x0 = self.p_mean_variance(keeping, x, t, clip_denoised=False, model_kwargs=model_kwargs)["pred_xstart"]
        eps = seen["eps"]  # the model's own, not re-derived from pred_xstart
        abn = od._extract(self.alphas_cumprod_next, t, x.shape)
        return {"sample": th.sqrt(abn) * x0 + th.sqrt(1 - abn) * eps, "pred_xstart": x0}

    def reverse_loop(self, model, image, model_kwargs=None, skip_timesteps=0):
        """yields {"sample", "pred_xstart"} per index 0 .. t0 - 1; the last one also carries "noise" """
        t0 = self.num_timesteps - 1 - skip_timesteps
        if t0 < 1:
            raise ValueError("nothing to invert")
        x = image
        for i in range(t0):
            t = th.tensor([i] * image.shape[0], dtype=th.long)
            out = self.ddim_reverse_sample(model, x, t, model_kwargs=dict(model_kwargs or {}))
            if i == t0 - 1:
                out["noise"] = self.implied_noise(image, out["sample"], t0)
            yield out
            x = out["sample"]

    def implied_noise(self, image, latent, t0):
        """the noise for which q_sample(image, t0, noise) == latent: q_sample's two table entries, inverted"""
        t = th.tensor([t0] * latent.shape[0], dtype=th.long)
        return (latent - od._extract(self.sqrt_alphas_cumprod, t, latent.shape) * image) / \
            od._extract(self.sqrt_one_minus_alphas_cumprod, t, latent.shape)


def create_invert_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="", rescale_timesteps=False):
    from tests import plms_ref
    betas = od.get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return InvertDiffusion(plms_ref.space_timesteps(steps, timestep_respacing), betas, rescale_timesteps=rescale_timesteps)


def reverse_update_fp64(coef, x, out6, init=None):
    """fp64 restatement of cgd_ddim_reverse_update (include/cgd_mi355x.h) with the float32 coefficients the kernel sees.
    -> (x_next, pred_xstart, noise_out or None); only channels 0..2 of out6 are read; init broadcasts over the batch."""
    x, eps = x.double().cpu(), out6[:, :3].double().cpu()
    x0 = float(coef.sqrt_recip) * x - float(coef.sqrt_recipm1) * eps
    xn = float(coef.sqrt_ab_next) * x0 + float(coef.sqrt_one_minus_ab_next) * eps
    noise = None
    if init is not None:
        noise = (xn - float(coef.sqrt_ab_next) * init.double().cpu().expand_as(xn)) / float(coef.sqrt_one_minus_ab_next)
    return xn, x0, noise
