"""Restatement of masked sampling (inpainting / outpainting of an init image; the resampling of RePaint, Lugmayr et al., CVPR 2022, with
jump length 1) on top of the CPU oracle and tests/plms_ref.py.  TEST INFRASTRUCTURE ONLY.

After every update of step index i (which leaves `sample`, the state at level i - 1, and `pred_xstart`):

    known       = sqrt(abar_prev[i]) init + sqrt(1 - abar_prev[i]) n_known          (init itself at i = 0)
    sample      = m sample      + (1 - m) known
    pred_xstart = m pred_xstart + (1 - m) init

with the mask's endpoints as selects (m == 0: known / init whatever sample holds; m == 1: untouched).  n_known is a fresh draw per merge
in the stochastic loops (p_sample, DDIM with eta > 0; `tape['known_noise']`, one entry per merge) and the loop's initial noise (`tape['x_T']`)
in the deterministic ones (DDIM eta = 0, PLMS).  With `resamples = r` every step index i > 0 runs r times: after each of the first r - 1
merges  x_i = sqrt(abar[i] / abar_prev[i]) x_{i-1} + sqrt(1 - abar[i] / abar_prev[i]) n_re  (`tape['renoise']`) and the step runs again on
the next entry of `tape['noise']` (one per evaluation).  The loops yield once per step index.
"""
import functools

import torch as th

from tests import plms_ref


def select_merge(m, a, b):
    """m a + (1 - m) b with the endpoints as selects"""
    return th.where(m == 0, b, th.where(m == 1, a, m * a + (1 - m) * b))


def merge_fp64(coef, sample, pred_xstart, init, mask, n_known, n_re=None):
    """fp64 restatement of cgd_masked_merge (include/cgd_mi355x.h) with the float32 coefficients the kernel sees.
    -> (sample, pred_xstart or None, x_re or None); init and mask broadcast over batch / channels."""
    d = lambda t: None if t is None else t.double().cpu()  # noqa: E731
    sample, pred_xstart, init, mask, n_known, n_re = d(sample), d(pred_xstart), d(init), d(mask), d(n_known), d(n_re)
    known = float(coef.sqrt_ab_prev) * init
    if n_known is not None:
        known = known + float(coef.sqrt_one_minus_ab_prev) * n_known
    m = mask.expand_as(sample)
    s = select_merge(m, sample, known.expand_as(sample))
    x0 = None if pred_xstart is None else select_merge(m, pred_xstart, init.expand_as(sample))
    x_re = None if n_re is None else float(coef.renoise_x) * s + float(coef.renoise_n) * n_re
    return s, x0, x_re


class MaskedDiffusion(plms_ref.PLMSDiffusion):
    def merge(self, i, sample, pred_xstart, init, mask, n_known):
        abp = float(self.alphas_cumprod_prev[i])
        known = init if i == 0 else (abp ** 0.5) * init + ((1 - abp) ** 0.5) * n_known
        m = mask.expand_as(sample)
        return select_merge(m, sample, known.expand_as(sample)), \
            None if pred_xstart is None else select_merge(m, pred_xstart, init.expand_as(sample))

    def masked_plms_sample(self, model, x, t, i, init, mask, x_T, cond_fn, model_kwargs, order, old_eps):
        """plms_ref.PLMSDiffusion.plms_sample with the start step's predictor merged before the second evaluation and the step's
        result merged at the end; the eps history stays as evaluated"""
        from oracle import diffusion as od
        ab_prev = od._extract(self.alphas_cumprod_prev, t, x.shape)
        eps, x0c, x0 = self.guided_eval(model, x, t, cond_fn, model_kwargs)
        if order > 1 and old_eps is None:
            old_eps = [eps]
            pred = x0c * th.sqrt(ab_prev) + th.sqrt(1 - ab_prev) * eps
            pred, _ = self.merge(i, pred, None, init, mask, x_T)
            eps_2, _, _ = self.guided_eval(model, pred, t - 1, cond_fn, model_kwargs)
            eps_prime = (eps + eps_2) / 2
        else:
            old_eps = list(old_eps or []) + [eps]
            k = min(order, len(old_eps))
            eps_prime = sum(w * e for w, e in zip(plms_ref.AB_WEIGHTS[k], old_eps[::-1]))
        if len(old_eps) >= order:
            old_eps.pop(0)
        x0p = (od._extract(self.sqrt_recip_alphas_cumprod, t, x.shape) * x
               - od._extract(self.sqrt_recipm1_alphas_cumprod, t, x.shape) * eps_prime)
        mean = x0p * th.sqrt(ab_prev) + th.sqrt(1 - ab_prev) * eps_prime
        sample = mean if i != 0 else x0c
        sample, x0 = self.merge(i, sample, x0, init, mask, x_T)
        return {"sample": sample, "pred_xstart": x0}, old_eps

    def masked_loop(self, kind, model, shape, init_image, mask, tape, cond_fn=None, model_kwargs=None, skip_timesteps=0,
                    randomize_class=False, eta=0.0, order=2, resamples=1):
        """kind: 'p' | 'ddim' | 'plms'.  `tape`: x_T, y and noise as in the oracle loops (noise: one entry per evaluation), plus
        'known_noise' (one per merge of a stochastic loop) and 'renoise' (one per repeat)."""
        if kind == "plms":
            plms_ref.check_order(order)
            if resamples != 1:
                raise ValueError("PLMS cannot resample")
        stochastic = kind == "p" or (kind == "ddim" and eta > 0)
        step_fn = self.p_sample_with_grad if kind == "p" else functools.partial(self.ddim_sample_with_grad, eta=eta)
        B = shape[0]
        x_T = tape["x_T"]
        indices = list(range(self.num_timesteps - skip_timesteps))[::-1]
        img = self.q_sample(init_image, th.tensor([indices[0]] * B), x_T)
        model_kwargs = dict(model_kwargs or {})
        evals = merges = repeats = 0
        old_eps = None
        for n, i in enumerate(indices):
            t = th.tensor([i] * B, dtype=th.long)
            if randomize_class and "y" in model_kwargs:
                model_kwargs["y"] = tape["y"][n]
            if kind == "plms":
                with th.no_grad():
                    out, old_eps = self.masked_plms_sample(model, img, t, i, init_image, mask, x_T, cond_fn, model_kwargs, order, old_eps)
                yield out
                img = out["sample"]
                continue
            for r in range(resamples if i > 0 else 1):
                with th.no_grad():
                    out = step_fn(model, img, t, clip_denoised=False, cond_fn=cond_fn, model_kwargs=model_kwargs, noise=tape["noise"][evals])
                evals += 1
                n_known = x_T
                if stochastic:
                    n_known = tape["known_noise"][merges]
                    merges += 1
                sample, x0 = self.merge(i, out["sample"], out["pred_xstart"], init_image, mask, n_known)
                if r + 1 < (resamples if i > 0 else 1):
                    a = float(self.alphas_cumprod[i] / self.alphas_cumprod_prev[i])
                    img = (a ** 0.5) * sample + ((1 - a) ** 0.5) * tape["renoise"][repeats]
                    repeats += 1
            yield {"sample": sample, "pred_xstart": x0}
            img = sample


def create_masked_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="", rescale_timesteps=False):
    from oracle import diffusion as od
    betas = od.get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return MaskedDiffusion(plms_ref.space_timesteps(steps, timestep_respacing), betas, rescale_timesteps=rescale_timesteps)


def make_mask(shape, seed=0, ones=0.4, blend=0.3):
    """A mask with `ones` of its pixels at exactly 1, `blend` strictly inside (0, 1) and the rest at exactly 0, scattered"""
    gen = th.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    order = th.randperm(n, generator=gen)
    m = th.zeros(n)
    n1, nb = round(ones * n), round(blend * n)
    m[order[:n1]] = 1.0
    m[order[n1:n1 + nb]] = 0.1 + 0.8 * th.rand(nb, generator=gen)
    return m.view(shape)
