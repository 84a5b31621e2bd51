"""Restatement of ILVR (Choi et al., 2021, "ILVR: Conditioning Method for Denoising Diffusion Probabilistic Models") on top of the CPU
oracle, tests/plms_ref.py and tests/dpm_ref.py.  TEST INFRASTRUCTURE ONLY.

Per axis of extent n and factor N, D = resize_matrix(n, n / N) (the antialiased cubic down-resize) and U = resize_matrix(n / N, n) (the
cubic up-resize), both ResizeRight with pad_mode='constant'; P = U D and phi_N(z) = P_H z P_W^T per plane.  After every update of a step
index i >= stop (which leaves `sample`, the state at level i - 1, and `pred_xstart`):

    known        = sqrt(abar_prev[i]) ref + sqrt(1 - abar_prev[i]) n          (ref itself at i = 0)
    sample      += phi_N(known - sample)
    pred_xstart += phi_N(ref   - pred_xstart)

n is a fresh draw per refinement in the stochastic loops (p_sample, DDIM and DPM-Solver++ with eta > 0; `tape['ilvr_noise']`, one entry
per refinement) and the loop's initial noise (`tape['x_T']`) in the deterministic ones.  The refinement's arithmetic is float64.
"""
import functools

import torch as th

from tests import dpm_ref, plms_ref


@functools.lru_cache(maxsize=None)
def lowpass_matrix(n, N):
    """P = U D of an extent n and a factor N, float64 (n, n)"""
    from cgd_amd.guidance import resize_matrix
    if n % N:
        raise ValueError(f"the factor {N} does not divide {n}")
    return resize_matrix(n // N, n, dtype=th.float64) @ resize_matrix(n, n // N, dtype=th.float64)


def lowpass(z, N):
    """phi_N of (..., H, W) in float64"""
    z = z.double()
    return lowpass_matrix(z.shape[-2], N) @ z @ lowpass_matrix(z.shape[-1], N).T


def refine_fp64(sa, sb, sample, pred_xstart, ref, noise, N):
    """fp64 restatement of cgd_ilvr_refine (include/cgd_mi355x.h) with the float32 coefficients the kernel sees.
    -> (sample, pred_xstart or None); ref broadcasts over the batch; noise None: known = sa ref."""
    d = lambda t: None if t is None else t.double().cpu()  # noqa: E731
    sample, pred_xstart, ref, noise = d(sample), d(pred_xstart), d(ref), d(noise)
    known = float(sa) * ref
    if noise is not None:
        known = known + float(sb) * noise
    s = sample + lowpass(known.expand_as(sample) - sample, N)
    x0 = None if pred_xstart is None else pred_xstart + lowpass(ref.expand_as(pred_xstart) - pred_xstart, N)
    return s, x0


class IlvrDiffusion(dpm_ref.DPMDiffusion):
    def refine(self, i, sample, pred_xstart, ref, n, N, stop):
        if i < stop:
            return sample, pred_xstart
        abp = float(self.alphas_cumprod_prev[i])
        sa, sb = (1.0, 0.0) if i == 0 else (abp ** 0.5, (1 - abp) ** 0.5)
        s, x0 = refine_fp64(sa, sb, sample, pred_xstart, ref, None if i == 0 else n, N)
        return s.to(sample.dtype), None if x0 is None else x0.to(pred_xstart.dtype)

    def ilvr_plms_sample(self, model, x, t, i, ref, N, stop, x_T, cond_fn, model_kwargs, order, old_eps):
        """plms_ref.PLMSDiffusion.plms_sample with the start step's predictor refined before the second evaluation and the step's
        result refined at the end; the eps history stays as evaluated"""
        from oracle import diffusion as od
        ab_prev = od._extract(self.alphas_cumprod_prev, t, x.shape)
        eps, x0c, x0 = self.guided_eval(model, x, t, cond_fn, model_kwargs)
        if order > 1 and old_eps is None:
            old_eps = [eps]
            pred = x0c * th.sqrt(ab_prev) + th.sqrt(1 - ab_prev) * eps
            pred, _ = self.refine(i, pred, None, ref, x_T, N, stop)
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
        sample, x0 = self.refine(i, sample, x0, ref, x_T, N, stop)
        return {"sample": sample, "pred_xstart": x0}, old_eps

    def ilvr_loop(self, kind, model, shape, ref, N, tape, stop=0, cond_fn=None, model_kwargs=None, skip_timesteps=0, init_image=None,
                  randomize_class=False, eta=0.0, order=2):
        """kind: 'p' | 'ddim' | 'plms' | 'dpm'.  `tape`: x_T, y and noise as in the oracle loops (noise: one entry per evaluation, read
        where the loop draws a step noise), plus 'ilvr_noise' (one per refinement of a stochastic loop)."""
        if kind == "plms":
            plms_ref.check_order(order)
        stochastic = kind == "p" or (kind in ("ddim", "dpm") and eta > 0)
        step_fn = self.p_sample_with_grad if kind == "p" else functools.partial(self.ddim_sample_with_grad, eta=eta)
        B = shape[0]
        x_T = tape["x_T"]
        indices = list(range(self.num_timesteps - skip_timesteps))[::-1]
        img = x_T
        if skip_timesteps and init_image is None:
            init_image = th.zeros_like(img)
        if init_image is not None:
            img = self.q_sample(init_image, th.tensor([indices[0]] * B), x_T)
        model_kwargs = dict(model_kwargs or {})
        refinements = 0
        old_eps = hist = None
        for n, i in enumerate(indices):
            t = th.tensor([i] * B, dtype=th.long)
            if randomize_class and "y" in model_kwargs:
                model_kwargs["y"] = tape["y"][n]
            if kind == "plms":
                with th.no_grad():
                    out, old_eps = self.ilvr_plms_sample(model, img, t, i, ref, N, stop, x_T, cond_fn, model_kwargs, order, old_eps)
                yield out
                img = out["sample"]
                continue
            with th.no_grad():
                if kind == "dpm":
                    out = self.dpmpp_sample(model, img, t, cond_fn, model_kwargs, order, eta, tape["noise"][n] if eta else None, hist)
                    hist = out.pop("x0c")
                else:
                    out = step_fn(model, img, t, clip_denoised=False, cond_fn=cond_fn, model_kwargs=model_kwargs, noise=tape["noise"][n])
            noise = x_T
            if stochastic and i >= stop:
                noise = tape["ilvr_noise"][refinements]
                refinements += 1
            sample, x0 = self.refine(i, out["sample"], out["pred_xstart"], ref, noise, N, stop)
            yield {"sample": sample, "pred_xstart": x0}
            img = sample


def create_ilvr_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="", rescale_timesteps=False):
    from oracle import diffusion as od
    betas = od.get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return IlvrDiffusion(dpm_ref.space_timesteps(steps, timestep_respacing, betas), betas, rescale_timesteps=rescale_timesteps)
