"""Restatement of DPM-Solver++(2M) sampling (Lu et al., 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic
Models": data prediction, multistep, second order; deterministic and SDE form) and of the logSNR-uniform spacing 'dpmN', on top of the CPU
oracle.  TEST INFRASTRUCTURE ONLY.

With alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma), one step takes the state from level i to level i - 1
('prev'), h = lambda_prev - lambda_i, x0c = the guided pred_xstart of the evaluation at (x, i) (ddim_sample_with_grad's
condition_score_with_grad, as tests/plms_ref.py):

    D      = x0c + h / (2 h_last) (x0c - x0c of the step before)        second order; D = x0c at first order
    sample = sigma_prev / sigma_i e^(-eta h) x - alpha_prev expm1(-(1 + eta) h) D + sigma_prev sqrt(-expm1(-2 eta h)) noise

eta = 0 is DPM-Solver++(2M), eta = 1 SDE-DPM-Solver++(2M).  The first executed step has no history and step index 0 ends at the clean image
(h infinite; 'lower order final'): both run at first order, and step index 0 returns x0c.  The yielded pred_xstart is the unconditioned
one, as in the oracle's DDIM step.  All coefficient arithmetic is float64.
"""
import math

import numpy as np
import torch as th

from oracle import diffusion as od
from tests import masked_ref


def lam(ab):
    return 0.5 * math.log(ab / (1.0 - ab))


def logsnr_timesteps(betas, count):
    """at most `count` timesteps, the nearest ones to `count` targets uniform in lambda between the ends of the schedule (ties: lower t)"""
    if count < 2:
        raise ValueError("a logSNR-uniform spacing needs at least 2 levels")
    ab = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    lams = 0.5 * (np.log(ab) - np.log1p(-ab))
    kept = set()
    for target in np.linspace(lams[0], lams[-1], count):
        dist = np.abs(lams - target)
        kept.add(min(range(len(lams)), key=lambda t: (dist[t], t)))
    return kept


def space_timesteps(num_timesteps, spec, betas=None):
    """oracle spacing, plus 'plmsN' (= 'ddimN') and 'dpmN' / 'dpmsdeN' (logSNR-uniform, needs betas)"""
    if isinstance(spec, str) and spec.startswith("dpm"):
        if betas is None:
            raise ValueError("'dpmN' needs the base schedule")
        return logsnr_timesteps(betas, int(spec[6:] if spec.startswith("dpmsde") else spec[3:]))
    if isinstance(spec, str) and spec.startswith("plms"):
        spec = "ddim" + spec[4:]
    return od.space_timesteps(num_timesteps, spec)


def coefs(ab, ab_prev, ab_up, order, eta):
    """(c_x, c_d, c_r, c_n) of the step from abar = ab down to ab_prev (1.0: the clean image); ab_up: abar of the level the step before
    started from (used at order 2)"""
    if ab_prev >= 1.0:
        return 0.0, 1.0, 0.0, 0.0
    h = lam(ab_prev) - lam(ab)
    c_r = h / (2.0 * (lam(ab) - lam(ab_up))) if order == 2 else 0.0
    return (math.sqrt((1.0 - ab_prev) / (1.0 - ab)) * math.exp(-eta * h), -math.sqrt(ab_prev) * math.expm1(-(1.0 + eta) * h), c_r,
            math.sqrt(1.0 - ab_prev) * math.sqrt(max(0.0, -math.expm1(-2.0 * eta * h))))


def solve(denoiser, x, abars, order, eta=0.0, noises=None):
    """The solver on bare arrays (float64): `abars` = abar of the levels, clean end first (as alphas_cumprod); starts from x at the last
    level, ends with the step to the clean image.  denoiser(x, abar) -> pred_xstart."""
    hist = None
    n = len(abars)
    for k, i in enumerate(range(n - 1, -1, -1)):
        x0 = denoiser(x, abars[i])
        eff = 2 if (order == 2 and hist is not None and i > 0) else 1
        c_x, c_d, c_r, c_n = coefs(abars[i], abars[i - 1] if i > 0 else 1.0, abars[i + 1] if eff == 2 else None, eff, eta)
        d = x0 + c_r * (x0 - hist) if eff == 2 else x0
        x = c_x * x + c_d * d + (c_n * noises[k] if c_n else 0.0) if i > 0 else x0
        hist = x0
    return x


class DPMDiffusion(masked_ref.MaskedDiffusion):
    def step_coefs(self, i, order, eta):
        return coefs(self.alphas_cumprod[i], self.alphas_cumprod_prev[i] if i > 0 else 1.0,
                     self.alphas_cumprod[i + 1] if order == 2 else None, order, eta)

    def dpmpp_sample(self, model, x, t, cond_fn=None, model_kwargs=None, order=2, eta=0.0, noise=None, hist=None):
        """-> {'sample', 'pred_xstart' (unconditioned), 'x0c' (the history entry)}; `hist`: x0c of the step before or None"""
        i = int(t[0])
        _, x0c, x0 = self.guided_eval(model, x, t, cond_fn, model_kwargs)
        eff = 2 if (order == 2 and hist is not None and i > 0) else 1
        c_x, c_d, c_r, c_n = self.step_coefs(i, eff, eta)
        d = x0c + c_r * (x0c - hist) if eff == 2 else x0c
        sample = x0c
        if i > 0:
            sample = c_x * x + c_d * d
            if c_n:
                sample = sample + c_n * noise
        return {"sample": sample, "pred_xstart": x0, "x0c": x0c}

    def dpmpp_sample_loop_progressive(self, model, shape, clip_denoised=False, cond_fn=None, model_kwargs=None, device=None,
                                      skip_timesteps=0, init_image=None, randomize_class=False, cond_fn_with_grad=True, order=2,
                                      eta=0.0, tape=None, mask=None):
        """`tape`: x_T, y (per step), noise (per evaluation, read only for eta > 0), known_noise (per merge, masked with eta > 0).
        `mask`: every update is followed by the merge of tests/masked_ref.py; the history stays as evaluated."""
        if order not in (1, 2) or isinstance(order, bool):
            raise ValueError(f"order must be 1 or 2: {order!r}")
        if not eta >= 0:
            raise ValueError("eta must be >= 0")
        assert not clip_denoised and cond_fn_with_grad
        B = shape[0]
        x_T = tape["x_T"]
        indices = list(range(self.num_timesteps - skip_timesteps))[::-1]
        img = x_T
        if skip_timesteps and init_image is None:
            init_image = th.zeros_like(img)
        if init_image is not None:
            img = self.q_sample(init_image, th.tensor([indices[0]] * B), x_T)
        model_kwargs = dict(model_kwargs or {})
        hist = None
        for n, i in enumerate(indices):
            t = th.tensor([i] * B, dtype=th.long)
            if randomize_class and "y" in model_kwargs:
                model_kwargs["y"] = tape["y"][n]
            with th.no_grad():
                out = self.dpmpp_sample(model, img, t, cond_fn, model_kwargs, order, eta, tape["noise"][n] if eta else None, hist)
            hist = out.pop("x0c")
            if mask is not None:
                out["sample"], out["pred_xstart"] = self.merge(i, out["sample"], out["pred_xstart"], init_image, mask,
                                                               tape["known_noise"][n] if eta else x_T)
            yield out
            img = out["sample"]


def create_dpm_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="", rescale_timesteps=False):
    betas = od.get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return DPMDiffusion(space_timesteps(steps, timestep_respacing, betas), betas, rescale_timesteps=rescale_timesteps)


# ---- the Gaussian toy: data N(mu, s^2), the exact posterior-mean denoiser, the probability-flow ODE in closed form --------------------
def toy_denoiser(mu, s):
    def den(x, ab):
        return mu + math.sqrt(ab) * s * s / (ab * s * s + 1.0 - ab) * (x - math.sqrt(ab) * mu)
    return den


def toy_truth(x_T, abars, mu, s):
    """The clean end of the probability-flow ODE through x_T: along it (x_t - alpha_t mu) / sqrt(alpha_t^2 s^2 + sigma_t^2) is constant, and
    at alpha = 1, sigma = 0 the state is mu + s times that constant"""
    z = (x_T - math.sqrt(abars[-1]) * mu) / math.sqrt(abars[-1] * s * s + 1.0 - abars[-1])
    return mu + s * z


def toy_error(spec, order, mu=0.3, s=0.5, draws=4096, seed=0):
    """max |solver - truth| over `draws` start states, on the linear schedule of 1000 steps spaced by `spec`"""
    betas = od.get_named_beta_schedule("linear", 1000)
    ab = np.cumprod(1.0 - betas)
    abars = [float(ab[t]) for t in sorted(space_timesteps(1000, spec, betas))]
    x_T = np.random.default_rng(seed).standard_normal(draws)
    return float(np.abs(solve(toy_denoiser(mu, s), x_T, abars, order) - toy_truth(x_T, abars, mu, s)).max())
