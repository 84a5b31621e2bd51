"""Restatement of PLMS sampling (pseudo linear multistep, Liu et al., ICLR 2022, "Pseudo Numerical Methods for Diffusion Models on
Manifolds") as the guided_diffusion fork's `plms_sample` / `plms_sample_loop_progressive` run it, on top of the CPU oracle.
TEST INFRASTRUCTURE ONLY.

The fork's source is not available offline: this file restates the specification the device sampler implements.  One guided
evaluation at (x, t) is `ddim_sample_with_grad`'s (p_mean_variance, condition_score_with_grad), and its eps is re-derived from the
conditioned pred_xstart.  The first step of an order > 1 run is pseudo improved Euler (a second evaluation at the predictor and
t - 1), every other step Adams-Bashforth over the last `order` eps.  No per-step noise; pred_xstart yielded is the unconditioned one.
"""
import torch as th

from oracle import diffusion as od

AB_WEIGHTS = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


def space_timesteps(num_timesteps, spec):
    """oracle spacing, with 'plmsN' spaced exactly like 'ddimN'"""
    if isinstance(spec, str) and spec.startswith("plms"):
        spec = "ddim" + spec[4:]
    return od.space_timesteps(num_timesteps, spec)


def check_order(order):
    if isinstance(order, bool) or not isinstance(order, int) or not 1 <= order <= 4:
        raise ValueError(f"order is invalid (should be int from 1-4): {order!r}")


class PLMSDiffusion(od.SpacedDiffusion):
    evaluations = 0  # guided evaluations (UNet forwards) so far

    def guided_eval(self, model, x, t, cond_fn=None, model_kwargs=None):
        """-> (eps, conditioned pred_xstart, unconditioned pred_xstart) of one guided evaluation at (x, t)"""
        self.evaluations += 1
        with th.enable_grad():
            x = x.detach().requires_grad_()
            out_orig = self.p_mean_variance(model, x, t, clip_denoised=False, model_kwargs=model_kwargs)
            out = self.condition_score_with_grad(cond_fn, out_orig, x, t, model_kwargs) if cond_fn is not None else out_orig
        x = x.detach()
        x0c = out["pred_xstart"].detach()
        return self._eps_from_xstart(x, t, x0c), x0c, out_orig["pred_xstart"].detach()

    def plms_sample(self, model, x, t, cond_fn=None, model_kwargs=None, order=2, old_eps=None):
        check_order(order)
        ab_prev = od._extract(self.alphas_cumprod_prev, t, x.shape)
        eps, x0c, x0 = self.guided_eval(model, x, t, cond_fn, model_kwargs)
        if order > 1 and old_eps is None:
            # pseudo improved Euler
            old_eps = [eps]
            pred = x0c * th.sqrt(ab_prev) + th.sqrt(1 - ab_prev) * eps
            eps_2, _, _ = self.guided_eval(model, pred, t - 1, cond_fn, model_kwargs)
            eps_prime = (eps + eps_2) / 2
        else:
            # Adams-Bashforth
            old_eps = list(old_eps or []) + [eps]
            k = min(order, len(old_eps))
            eps_prime = sum(w * e for w, e in zip(AB_WEIGHTS[k], old_eps[::-1]))
        if len(old_eps) >= order:
            old_eps.pop(0)
        x0p = (od._extract(self.sqrt_recip_alphas_cumprod, t, x.shape) * x
               - od._extract(self.sqrt_recipm1_alphas_cumprod, t, x.shape) * eps_prime)
        mean = x0p * th.sqrt(ab_prev) + th.sqrt(1 - ab_prev) * eps_prime
        nonzero = (t != 0).float().view(-1, *([1] * (x.dim() - 1)))
        sample = mean * nonzero + x0c * (1 - nonzero)
        return {"sample": sample, "pred_xstart": x0, "old_eps": old_eps}

    def plms_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, cond_fn=None, model_kwargs=None,
                                     device=None, progress=False, skip_timesteps=0, init_image=None, randomize_class=False,
                                     cond_fn_with_grad=True, order=2, tape=None):
        """`tape` as in the oracle loops; its per-step noise is not used (PLMS draws none)."""
        check_order(order)
        if order > 1 and self.num_timesteps - skip_timesteps < 2:
            raise ValueError("a one-step schedule with order > 1 would evaluate at t = -1")
        state = {"old_eps": None}

        def step(model_, x, t, clip_denoised=True, cond_fn=None, model_kwargs=None, noise=None):
            out = self.plms_sample(model_, x, t, cond_fn=cond_fn, model_kwargs=model_kwargs, order=order, old_eps=state["old_eps"])
            state["old_eps"] = out["old_eps"]
            return out

        return self._loop(step, model, shape, noise, clip_denoised, cond_fn, model_kwargs, device, skip_timesteps, init_image,
                          randomize_class, tape)


def create_plms_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="", rescale_timesteps=False):
    betas = od.get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return PLMSDiffusion(space_timesteps(steps, timestep_respacing), betas, rescale_timesteps=rescale_timesteps)
