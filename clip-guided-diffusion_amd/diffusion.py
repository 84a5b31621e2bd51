"""Host side of the (respaced) Gaussian diffusion process: float64 schedule tables and per-step scalars.

Mirrors the interface of guided_diffusion's `SpacedDiffusion` that the reference touches —
`create_model_and_diffusion(...)` at /root/reference/cgd/script_util.py:316, `diffusion.num_timesteps` and
`diffusion.sqrt_one_minus_alphas_cumprod` at /root/reference/cgd/cgd.py:154,177, and the two progressive loops
selected at /root/reference/cgd/cgd.py:242-262 (implemented in sampler.py on top of these tables).
All per-pixel arithmetic of a step runs in HIP kernels (csrc/guidance.hip); only O(T) scalar tables live here.
"""
import math

import numpy as np

from . import lib as L


def named_beta_schedule(name, steps):
    if name == "linear":
        s = 1000.0 / steps
        return np.linspace(s * 1e-4, s * 2e-2, steps, dtype=np.float64)
    if name == "cosine":
        def abar(u):
            return math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2
        return np.asarray([min(1.0 - abar((i + 1) / steps) / abar(i / steps), 0.999) for i in range(steps)], dtype=np.float64)
    raise NotImplementedError(f"unknown beta schedule: {name}")


def logsnr_timesteps(betas, count):
    """The timesteps of 'dpmN': `count` targets uniform in lambda = log(alpha / sigma) = 0.5 log(abar / (1 - abar)) between the two ends of
    the base schedule, each replaced by the nearest timestep (ties go to the lower one).  The distinct picks are kept: always 0 and
    T - 1, and fewer than `count` where the schedule is coarser in lambda than the targets (49 of 50 on the linear schedule of 1000)."""
    if count < 2:
        raise ValueError(f"a logSNR-uniform spacing needs at least 2 levels (the two ends of the schedule), got {count}")
    ab = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    lam = 0.5 * np.log(ab / (1.0 - ab))
    return {int(np.argmin(np.abs(lam - target))) for target in np.linspace(lam[0], lam[-1], count)}


def space_timesteps(num_timesteps, spec, betas=None):
    """'ddimN' (and 'plmsN', spaced the same way) -> fixed integer stride with exactly N steps; 'dpmN' / 'dpmsdeN' -> at most N timesteps
    uniform in logSNR (logsnr_timesteps; needs the base schedule `betas`); 'a,b,c' -> per-section even spacing (rounded)."""
    if isinstance(spec, str):
        if spec.startswith("dpm"):
            if betas is None:
                raise ValueError(f"timestep spacing {spec!r} is uniform in logSNR and needs the base schedule: pass betas=")
            if len(betas) != num_timesteps:
                raise ValueError(f"betas has {len(betas)} entries for {num_timesteps} timesteps")
            return logsnr_timesteps(betas, int(spec[6 if spec.startswith("dpmsde") else 3:]))
        if spec.startswith(("ddim", "plms")):
            want = int(spec[4:])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        spec = [int(v) for v in spec.split(",")]
    base, extra = divmod(num_timesteps, len(spec))
    kept, start = [], 0
    for sec, count in enumerate(spec):
        size = base + (1 if sec < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1.0 if count <= 1 else (size - 1) / (count - 1)
        kept += _walk(start, stride, count)
        start += size
    return set(kept)


def _walk(start, stride, count):
    # accumulate like upstream (cur += frac) so that rounding of the running sum matches
    out, cur = [], 0.0
    for _ in range(count):
        out.append(start + round(cur))
        cur += stride
    return out


class SpacedDiffusion:
    """epsilon-prediction / LEARNED_RANGE process restricted to `use_timesteps` of a base schedule."""

    def __init__(self, use_timesteps, betas, rescale_timesteps=False):
        base_ab = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(betas)
        self.rescale_timesteps = bool(rescale_timesteps)
        self.timestep_map, new_betas, last = [], [], 1.0
        for i, ab in enumerate(base_ab):
            if i in self.use_timesteps:
                new_betas.append(1.0 - ab / last)
                last = ab
                self.timestep_map.append(i)
        b = self.betas = np.asarray(new_betas, dtype=np.float64)
        self.num_timesteps = len(b)
        a = 1.0 - b
        ab = self.alphas_cumprod = np.cumprod(a)
        abp = self.alphas_cumprod_prev = np.append(1.0, ab[:-1])
        self.alphas_cumprod_next = np.append(ab[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(ab)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - ab)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / ab)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / ab - 1.0)
        pv = self.posterior_variance = b * (1.0 - abp) / (1.0 - ab)
        self.posterior_log_variance_clipped = np.log(np.append(pv[1], pv[1:])) if len(pv) > 1 else np.log(np.maximum(pv, 1e-20))
        self.posterior_mean_coef1 = b * np.sqrt(abp) / (1.0 - ab)
        self.posterior_mean_coef2 = (1.0 - abp) * np.sqrt(a) / (1.0 - ab)

    def model_timestep(self, i):
        """What the UNet sees for respaced index i (the reference's _WrappedModel)."""
        t = float(self.timestep_map[i])
        if self.rescale_timesteps:
            t = t * (1000.0 / self.original_num_steps)
        return t

    def step_coef(self, i, fac_index=None):
        k = L.StepCoef()
        k.sqrt_recip = self.sqrt_recip_alphas_cumprod[i]
        k.sqrt_recipm1 = self.sqrt_recipm1_alphas_cumprod[i]
        k.coef1 = self.posterior_mean_coef1[i]
        k.coef2 = self.posterior_mean_coef2[i]
        k.min_log = self.posterior_log_variance_clipped[i]
        k.max_log = math.log(self.betas[i])
        k.fac = 0.0 if fac_index is None else self.sqrt_one_minus_alphas_cumprod[fac_index]
        k.sqrt_one_minus_ab = math.sqrt(1.0 - self.alphas_cumprod[i])
        k.sqrt_ab_prev = math.sqrt(self.alphas_cumprod_prev[i])
        k.sqrt_one_minus_ab_prev = math.sqrt(1.0 - self.alphas_cumprod_prev[i])
        k.nonzero = int(i != 0)
        return k

    def dpmpp_coef_f64(self, i, order, eta=0.0):
        """(c_x, c_d, c_r, c_n) of the DPM-Solver++ step from level i to level i - 1 (Lu et al., 2022; data prediction, multistep), float64:
            sample = c_x x + c_d D + c_n noise,  D = x0c + c_r (x0c - x0c of the step before)
        with alpha = sqrt(abar), sigma = sqrt(1 - abar), lambda = log(alpha / sigma), 'prev' = level i - 1, h = lambda_prev - lambda_i:
            c_x = sigma_prev / sigma_i e^(-eta h),  c_d = -alpha_prev expm1(-(1 + eta) h),  c_n = sigma_prev sqrt(-expm1(-2 eta h)),
            c_r = h / (2 h_last), h_last = lambda_i - lambda_(i+1), for order 2; 0 for order 1.
        eta = 0 is the deterministic solver (order 1: DDIM), eta = 1 the SDE solver (order 1: DDIM with eta = 1).  At i = 0 the step ends
        at the clean image, h is infinite and the values are their limits: c_x = 0, c_d = 1, c_n = c_r = 0 (lower order final)."""
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order!r}")
        if not eta >= 0.0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        if i == 0:
            return 0.0, 1.0, 0.0, 0.0
        ab, abp = self.alphas_cumprod[i], self.alphas_cumprod_prev[i]

        def lam(v):
            return 0.5 * math.log(v / (1.0 - v))

        h = lam(abp) - lam(ab)
        c_r = 0.0
        if order == 2:
            if i + 1 >= self.num_timesteps:
                raise ValueError("a second-order step needs the step before it: the first index of the schedule has none")
            c_r = h / (2.0 * (lam(ab) - lam(self.alphas_cumprod[i + 1])))
        return (math.sqrt((1.0 - abp) / (1.0 - ab)) * math.exp(-eta * h), -math.sqrt(abp) * math.expm1(-(1.0 + eta) * h), c_r,
                math.sqrt(1.0 - abp) * math.sqrt(-math.expm1(-2.0 * eta * h)) if eta else 0.0)

    def dpmpp_coef(self, i, order, eta=0.0):
        """dpmpp_coef_f64 as the cgd_dpmpp struct of cgd_dpmpp_update (csrc/dpm.hip)."""
        k = L.Dpmpp()
        k.c_x, k.c_d, k.c_r, k.c_n = self.dpmpp_coef_f64(i, order, eta)
        return k

    @staticmethod
    def threshold_rank(p, n):
        """(k, frac) of the p-quantile of n values under torch.quantile's 'linear' rule, float64: pos = p (n - 1), k = floor(pos),
        frac = pos - k, so that the quantile is v_k + (v_{k+1} - v_k) frac with v_j the j-th smallest value (k + 1 clamped to n - 1).
        What cgd_dpmpp_threshold takes (csrc/threshold.hip); p in (0, 1], p = 1 is the maximum."""
        if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 < p <= 1.0:
            raise ValueError(f"the quantile p must be a number in (0, 1], got {p!r}")
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"n must be an int >= 1, got {n!r}")
        pos = float(p) * (n - 1)
        k = min(int(math.floor(pos)), n - 1)
        return k, pos - k

    def mask_coef(self, i):
        """Coefficients of the masked-sampling merge after the update of step index i (sampler.py, csrc/mask.hip): the known region
        lives at level i - 1, known = sqrt(abar_prev) init + sqrt(1 - abar_prev) noise (the init image itself at i = 0), and a
        resampling repeat goes back up with x_i = sqrt(abar / abar_prev) x_{i-1} + sqrt(1 - abar / abar_prev) noise."""
        k = L.MaskCoef()
        ab, abp = self.alphas_cumprod[i], self.alphas_cumprod_prev[i]
        k.sqrt_ab_prev = math.sqrt(abp)
        k.sqrt_one_minus_ab_prev = math.sqrt(1.0 - abp)
        k.renoise_x = math.sqrt(ab / abp)
        k.renoise_n = math.sqrt(1.0 - ab / abp)
        k.flags = 0
        return k

    def reverse_coef(self, i):
        """Coefficients of the DDIM inversion step at index i (sampler.py, csrc/invert.hip), which takes the state from level i up to level
        i + 1: pred_xstart = sqrt_recip x - sqrt_recipm1 eps, x_next = sqrt(abar_next) pred_xstart + sqrt(1 - abar_next) eps.  abar_next of
        the last index is 0 (x_next = eps there; the inversion loop stops one index earlier).  The inverse of sqrt(1 - abar_next) is 0
        where that root is 0, i.e. where the next level carries no noise and none can be implied."""
        k = L.ReverseCoef()
        abn = self.alphas_cumprod_next[i]
        k.sqrt_recip = self.sqrt_recip_alphas_cumprod[i]
        k.sqrt_recipm1 = self.sqrt_recipm1_alphas_cumprod[i]
        k.sqrt_ab_next = math.sqrt(abn)
        k.sqrt_one_minus_ab_next = math.sqrt(1.0 - abn)
        k.inv_sqrt_one_minus_ab_next = 1.0 / math.sqrt(1.0 - abn) if abn < 1.0 else 0.0
        return k


def create_gaussian_diffusion(steps=1000, noise_schedule="linear", timestep_respacing="", rescale_timesteps=False):
    betas = named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    return SpacedDiffusion(space_timesteps(steps, timestep_respacing, betas=betas), betas, rescale_timesteps=rescale_timesteps)
