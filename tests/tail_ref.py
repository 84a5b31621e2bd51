"""float64 references of the guided-step tail kernels of csrc/guidance.hip (cgd_pmv_blend, cgd_guidance_combine, cgd_grad_finish,
cgd_scalars, cgd_sample_update) and the input recipes of tests/test_gpu_tail.py.  Plain torch, no device code: tests/test_tail_host.py
runs every helper here on the CPU (against the oracle's own functions), so none of them executes for the first time next to a kernel.

The step coefficients are taken as the float32 values the kernel sees (the fields of the ctypes `StepCoef`), `1 - fac` from the float32
`fac`; everything else is float64."""
import torch as th

from oracle import guidance as og

# (B, H, W): one partial block with dead lanes | no vertical / no horizontal TV neighbour | H != W, six planes | above 262144 elements:
# 1024 capped blocks, a second element for some threads, total not a multiple of 256 | the batch-2 production shape (whole strides)
SHAPES = [(1, 5, 7), (3, 1, 9), (1, 9, 1), (2, 24, 40), (1, 296, 300), (2, 256, 256)]
SCHEDULE = (1000, "linear", "250", False)
STEPS = {"mid": 125, "first": 0, "last": 249}  # respaced indices: a middle step, nonzero == 0, a = 157 with fac = 1 - 2e-5
SCALES = (150.0, 50.0, 30.0)  # tv, range, saturation
# cgd_guidance_combine settings: (tv, range, sat, with g_clip)
SETTINGS = {"tv": (1, 0, 0, False), "range": (0, 1, 0, False), "sat": (0, 0, 1, False), "all": (1, 1, 1, False), "all+clip": (1, 1, 1, True)}


def coef(k):
    """the float32 fields of a StepCoef as Python floats (exact)"""
    return {name: float(getattr(k, name)) for name in ("sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "min_log", "max_log", "fac",
                                                       "sqrt_one_minus_ab", "sqrt_ab_prev", "sqrt_one_minus_ab_prev")}


def blocks(B, H, W):
    """workgroups of 256 threads of the grid-stride kernels (capped at 1024): what cgd_guidance_part_blocks must return"""
    return min((B * 3 * H * W + 255) // 256, 1024)


def _d(t):
    return None if t is None else t.detach().double().cpu()


def _gen(*key):
    return th.Generator().manual_seed(sum(int(v) * 1009 ** i for i, v in enumerate(key)) % (2 ** 31))


# ---- references --------------------------------------------------------------------------------------------------------------------
def pmv_blend(x, out6, k):
    """p_mean_variance (epsilon prediction, learned range) + x_in = pred_xstart fac + x (1 - fac) -> pred_xstart, mean, log_variance, x_in"""
    c = coef(k)
    x, out6 = _d(x), _d(out6)
    eps, v = out6[:, :3], out6[:, 3:]
    frac = (v + 1) / 2
    log_var = frac * c["max_log"] + (1 - frac) * c["min_log"]
    x0 = c["sqrt_recip"] * x - c["sqrt_recipm1"] * eps
    mean = c["coef1"] * x0 + c["coef2"] * x
    return x0, mean, log_var, x0 * c["fac"] + x * (1 - c["fac"])


def combine_leaves(x_in, x0, k):
    """the (x, eps) in float64 of which the float32 test inputs are x0 = a x - b eps and x_in = fac x0 + (1 - fac) x"""
    c = coef(k)
    x_in, x0 = _d(x_in), _d(x0)
    x = (x_in - c["fac"] * x0) / (1 - c["fac"])
    return x, (c["sqrt_recip"] * x - x0) / c["sqrt_recipm1"]


def combine_loss(x, eps, g_clip, k, tv_scale, range_scale, sat_scale):
    """L(x, eps) of the guidance legs that do not pass through CLIP, with the oracle's loss functions -> (L, tv, range, sat, x_in, x0)"""
    c = coef(k)
    x0 = c["sqrt_recip"] * x - c["sqrt_recipm1"] * eps
    x_in = c["fac"] * x0 + (1 - c["fac"]) * x
    tv = tv_scale * og.tv_loss(x_in).sum()
    rng = range_scale * og.range_loss(x0).sum()
    sat = sat_scale * (x_in - x_in.clamp(-1, 1)).abs().mean()
    total = tv + rng + sat
    if g_clip is not None:
        total = total + (_d(g_clip) * x_in).sum()
    return total, tv, rng, sat, x_in, x0


def guidance_combine(g_clip, x_in, x0, k, tv_scale, range_scale, sat_scale):
    """by autograd -> g_direct = dL/dx, seed_eps = dL/deps, (tv, range, sat) loss values"""
    x, eps = combine_leaves(x_in, x0, k)
    x.requires_grad_()
    eps.requires_grad_()
    total, tv, rng, sat, x_in_r, x0_r = combine_loss(x, eps, g_clip, k, tv_scale, range_scale, sat_scale)
    # the rebuilt tensors equal the kernel's inputs to float64 rounding: no element may have changed sides of a clamp kink on the way
    for r, t in ((x_in_r, _d(x_in)), (x0_r, _d(x0))):
        assert th.equal((r.detach() > 1), (t > 1)) and th.equal((r.detach() < -1), (t < -1)), "a test input sits on a clamp kink"
    g_direct, seed_eps = th.autograd.grad(total, [x, eps])
    return g_direct, seed_eps, th.stack([tv, rng, sat]).detach()


def combine_edge_closed_form(x_in, x0, k, range_scale, sat_scale):
    """closed form without the TV term, for inputs AT the clamp kinks (sign(0) = 0 there) -> g_direct, seed_eps, (range, sat) losses"""
    c = coef(k)
    x_in, x0 = _d(x_in), _d(x0)
    B, n = x_in.shape[0], x_in[0].numel()
    over, ro = x_in - x_in.clamp(-1, 1), x0 - x0.clamp(-1, 1)
    g_in = sat_scale * th.sign(over) / (n * B)
    g_x0 = c["fac"] * g_in + range_scale * 2 * ro / n
    return ((1 - c["fac"]) * g_in + c["sqrt_recip"] * g_x0, -c["sqrt_recipm1"] * g_x0,
            th.stack([range_scale * ro.pow(2).sum() / n, sat_scale * over.abs().sum() / (n * B)]))


def grad_finish(g_direct, g_unet):
    """g = -(g_direct + g_unet) -> g, sum g, sum g^2, sum |g|"""
    g = -(_d(g_direct) + (_d(g_unet) if g_unet is not None else 0.0))
    return g, g.sum(), g.pow(2).sum(), g.abs().sum()


def scalars(clip_part, loss_part, g_part, total, use_magnitude):
    """[clip, tv, range, sat, total loss, magnitude = rms g, grad mean after the clamp, clamp factor min(mag, 0.05) / mag]"""
    clip, (tv, rng, sat) = _d(clip_part).sum(), _d(loss_part).reshape(-1, 3).sum(0)
    s1, s2 = _d(g_part).reshape(-1, 2).sum(0)
    mag = (s2 / total).sqrt()
    fct = mag.clamp(max=0.05) / mag if use_magnitude else th.ones((), dtype=th.float64)
    return th.stack([clip, tv, rng, sat, clip + tv + rng + sat, mag, s1 / total * fct, fct])


def sample_update(mode, x, x0, mean, logvar, g, noise, fct, k):
    """mode 0: p_sample_with_grad (mean + variance g, + noise unless t == 0); mode 1: condition_score_with_grad + DDIM, eta = 0.
    -> sample, pred_xstart (the unconditioned input in both modes)"""
    c = coef(k)
    gv = _d(g) * fct if g is not None else 0.0
    if mode == 0:
        mean, logvar = _d(mean), _d(logvar)
        s = mean + th.exp(logvar) * gv
        if k.nonzero:
            s = s + th.exp(0.5 * logvar) * _d(noise)
        return s, _d(x0)
    x, x0 = _d(x), _d(x0)
    a, b = c["sqrt_recip"], c["sqrt_recipm1"]
    eps = (a * x - x0) / b - c["sqrt_one_minus_ab"] * gv
    x0c = a * x - b * eps
    eps2 = (a * x - x0c) / b
    return x0c * c["sqrt_ab_prev"] + c["sqrt_one_minus_ab_prev"] * eps2, x0


# ---- input recipes (float32, CPU) -------------------------------------------------------------------------------------------------------
def pmv_inputs(shape, step, k):
    """x = q_sample of an O(1) image, eps-hat consistent with an O(1) pred_xstart (so that a x - b eps cancels as on a real step), variance
    channel in [-1.5, 1.5] (frac extrapolates on both sides)"""
    B, H, W = shape
    gen = _gen(1, step, B, H, W)
    c = coef(k)
    a, b = c["sqrt_recip"], c["sqrt_recipm1"]
    x0s = 1.2 * th.randn(B, 3, H, W, generator=gen)
    x = (x0s + b * th.randn(B, 3, H, W, generator=gen)) / a
    eps = (a * x - 1.2 * th.randn(B, 3, H, W, generator=gen)) / b
    v = th.rand(B, 3, H, W, generator=gen) * 3 - 1.5
    return x.float(), th.cat([eps, v], dim=1).float().contiguous()


def combine_inputs(shape, step):
    """x_in, x0 ~ 1.2 randn (about 40 % of the elements outside [-1, 1]) and a random g_clip"""
    B, H, W = shape
    gen = _gen(2, step, B, H, W)
    return tuple((s * th.randn(B, 3, H, W, generator=gen)).float() for s in (1.2, 1.2, 1.0))


def combine_edge_inputs():
    """exactly +-1, +-(1 + 2^-23) and 0 in both x_in and x0, every pair of the five values"""
    e = 2.0 ** -23
    vals = th.tensor([1.0, -1.0, 1.0 + e, -1.0 - e, 0.0])
    x_in = vals.repeat(15)[:75].reshape(1, 3, 5, 5).float().contiguous()
    x0 = vals.repeat_interleave(5).repeat(3).reshape(1, 3, 5, 5).float().contiguous()
    return x_in, x0


def finish_inputs(shape):
    B, H, W = shape
    gen = _gen(3, B, H, W)
    return tuple(th.randn(B, 3, H, W, generator=gen).float() for _ in range(2))


def scalars_inputs(n_clip, nblk, total, magnitude):
    """synthetic partial arrays: positive losses, a cancelling sum of g, and sum g^2 = magnitude^2 total"""
    gen = _gen(4, n_clip, nblk)
    clip_part = (th.rand(n_clip, generator=gen) + 0.5).float()
    loss_part = (th.rand(nblk, 3, generator=gen) + 0.1).float()
    s2 = th.rand(nblk, generator=gen).double() + 0.5
    s2 = s2 / s2.sum() * magnitude ** 2 * total
    g_part = th.stack([th.randn(nblk, generator=gen).double() * magnitude * 16, s2], dim=1).float().contiguous()
    return clip_part, loss_part, g_part


def update_inputs(shape, mode, step, k):
    """mode 0: mean, logvar in the step's learned range; mode 1: x = q_sample of an O(1) image with an O(1) pred_xstart.  Both: g, noise."""
    B, H, W = shape
    gen = _gen(5, mode, step, B, H, W)
    c = coef(k)
    mk = lambda: th.randn(B, 3, H, W, generator=gen)  # noqa: E731
    x0 = 1.2 * mk()
    out = {"x0": x0.float(), "g": mk().float(), "noise": mk().float()}
    if mode == 0:
        out["mean"] = mk().float()
        out["logvar"] = (c["min_log"] + (c["max_log"] - c["min_log"]) * th.rand(B, 3, H, W, generator=gen)).float()
    else:
        out["x"] = ((x0 + c["sqrt_recipm1"] * mk()) / c["sqrt_recip"]).float()
    return out
