"""Guided sampling loops on the MI355X: the replacement of guided_diffusion's
`p_sample_loop_progressive` / `ddim_sample_loop_progressive` (+ `p_sample_with_grad`, `ddim_sample_with_grad`,
`condition_mean_with_grad`, `condition_score_with_grad`) as the reference calls them at
/root/reference/cgd/cgd.py:242-262 (same keyword arguments, same yielded dicts {"sample", "pred_xstart"}).

Per step: UNet forward (C ABI) -> p_mean_variance tail + blend (HIP) -> noise draw -> cond_fn -> update (HIP).
With a `ClipGuidance` cond_fn everything stays native; any other Python callable gets the reference semantics
through autograd Functions whose forward/backward call the same C ABI (`UNetFunction`).
PLMS (`plms_sample_loop_progressive`, from the fork's history) and DDIM with eta > 0 reuse the same guided evaluation and finish
it with one cgd_multistep_update launch per evaluation; PLMS draws no per-step noise.
Masked sampling (`mask=`, with an init image: 1 regenerates, 0 keeps) adds one cgd_masked_merge launch after every update, which puts the
init image, noised to the level the update produced, back into the kept region; `resamples=r` repeats every step r times (RePaint with
jump length 1).  Without a mask nothing of it runs.
ILVR (`ilvr=(ref, factor[, stop])`; Choi et al., 2021) conditions sampling on the low frequencies of a reference image: where the masked
merge sits, cgd_ilvr_refine (two launches, csrc/ilvr.hip) replaces the low-frequency band of the state by that of the reference noised to
the level the update produced, at step indices >= stop.  Without `ilvr` nothing of it runs.
DPM-Solver++(2M) (`dpmpp_sample_loop_progressive`, Lu et al., 2022; eta = 0 the ODE solver, eta > 0 the SDE solver) runs on the levels of
'dpmN' (uniform in logSNR, diffusion.logsnr_timesteps): one guided evaluation per step and one cgd_dpmpp_update launch, which combines the
evaluation's guided pred_xstart with the one of the step before; the two history buffers rotate by pointer.  With `threshold=` the guided
pred_xstart is thresholded dynamically first (per sample: clamped to its own quantile of absolute values and rescaled): cgd_dpmpp_threshold
selects the quantile on the device (csrc/threshold.hip) and cgd_dpmpp_update_thr updates (csrc/dpm.hip); without it nothing of that runs.
DDIM inversion (`ddim_reverse_sample_loop_progressive`, `ddim_invert`; guided_diffusion's ddim_reverse_sample) runs the deterministic DDIM ODE
upwards from an image: per step one UNet forward and one cgd_ddim_reverse_update launch.  `ddim_invert` returns the latent and the noise that
q_samples the image to it, so every loop above starts from the latent when called with `noise=noise, init_image=image, skip_timesteps=s`.
"""
import collections
import ctypes as C
import math
import os

import torch as th

from . import lib as L
from .guidance import ClipGuidance
from .nets import UNetFunction  # noqa: F401  (re-exported: the autograd node of model(x, ts, y))


def _timestep_table(tables, steps, B, device):
    """model timesteps of step indices 0 .. steps - 1 on the device (one row per step, B columns): no per-step fill kernel"""
    return th.tensor([float(tables.model_timestep(k)) for k in range(steps)], dtype=th.float32, device=device).view(-1, 1).repeat(1, B).contiguous()


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


class EmbedAhead:
    """Runs the (t, y)-only head of model(x, t, y) — timestep / class embedding, the FiLM projections of every ResBlock: eight small dependent
    launches, ~0.15 ms with their dispatch latencies — for step n + 1 on a side stream while step n computes.  Two FiLM
    buffers (slot = n & 1); events order embed(slot) -> forward(slot) -> the next embed(slot).  Only for the native paths (no cond_fn, or
    ClipGuidance), batches of <= 4 rows (the head's GEMMs are GEMVs then and touch no shared split-K workspace).  Random draws keep the
    reference's order: they are issued by the host in program order whatever stream executes them.
    MEASURED NEGATIVE, therefore opt-in (CGD_EMBED_AHEAD=1; 2 = the same choreography with the "side" stream being the main stream, the control
    of the A/B): profiles/r6_ab_embed_ahead.txt — 18.65 -> 19.29 ms per step.  A second active HIP stream costs every launch of the step (~0.7 us
    x 874) far more than the eight small launches it takes off the critical path."""

    @staticmethod
    def create(sampler, model, cond_fn, img, indices):
        mode = os.environ.get("CGD_EMBED_AHEAD", "0")
        if mode not in ("1", "2") or not hasattr(model, "embed") or img.shape[0] > 4 or len(indices) < 2:
            return None
        if cond_fn is not None and not isinstance(cond_fn, ClipGuidance):
            return None
        return EmbedAhead(sampler, img.device, img.shape[0], indices)

    def __init__(self, sampler, dev, B, indices):
        self.dev, self.indices = dev, indices
        self.side = th.cuda.current_stream(dev) if os.environ.get("CGD_EMBED_AHEAD") == "2" else th.cuda.Stream(device=dev)
        self.ev_emb = [th.cuda.Event(), th.cuda.Event()]
        self.ev_fwd = [th.cuda.Event(), th.cuda.Event()]
        self.fwd_seen = [False, False]
        self.n = 0  # the step whose forward comes next
        main = th.cuda.current_stream(dev)
        # model timesteps of the whole schedule, built on the main stream: the side stream waits for it once
        self.tt = _timestep_table(sampler.tables, sampler.num_timesteps, B, dev)
        ready = th.cuda.Event()
        ready.record(main)
        self.side.wait_event(ready)
        self._keep = []

    def side_stream(self):
        return th.cuda.stream(self.side)

    def launch(self, model, n, y):
        """embedding head of step n into slot n & 1 on the side stream"""
        slot = n & 1
        with th.cuda.stream(self.side):
            if self.fwd_seen[slot]:
                self.side.wait_event(self.ev_fwd[slot])  # the forward that read this slot last (step n - 2) is done
            if y is not None:
                y = y.to(self.dev)
                y.record_stream(self.side) if y.is_cuda else None
            model.embed(self.tt[self.indices[n]], y, slot)
            self.ev_emb[slot].record(self.side)
        self._keep = [y]

    def forward(self, model, x, out):
        slot = self.n & 1
        main = th.cuda.current_stream(self.dev)
        main.wait_event(self.ev_emb[slot])
        o = model.forward_slot(x, slot, out=out)
        self.ev_fwd[slot].record(main)
        self.fwd_seen[slot] = True
        self.n += 1
        return o


class _Run:
    """State of one loop call: the model, cond_fn and model_kwargs, the work buffers of the evaluation (allocated once, for the loop's
    shape), the model-timestep table, the optional EmbedAhead (the loop may drop it), the post-update rewrite (None, _Mask or _Ilvr), one
    keep-alive slot for what the last update's launches read."""
    Eval = collections.namedtuple("Eval", "x0 mean logvar g scal noise coef ts fac_index n_known")  # what `evaluate` hands to the update

    def __init__(self, sampler, model, cond_fn, model_kwargs, img, rewrite=None):
        self.sampler, self.model, self.cond_fn, self.model_kwargs, self.rewrite = sampler, model, cond_fn, model_kwargs, rewrite
        self.native = isinstance(cond_fn, ClipGuidance)
        (B, _, H, W), dev = img.shape, img.device
        self.dims = (B, H, W)
        self.x0, self.mean, self.logvar, self.xin = (th.empty((B, 3, H, W), device=dev, dtype=th.float32) for _ in range(4))
        # the generic plugin path calls model(x, ts, y), which allocates its own output
        self.out6 = th.empty((B, 6, H, W), device=dev, dtype=th.float32) if (cond_fn is None or self.native) else None
        self.ts = _timestep_table(sampler.tables, sampler.num_timesteps, B, dev)
        self.ahead = self.keep = None

    def evaluate(self, x, i, noise, draw_noise=True, n_known=None):
        """One guided evaluation at (x, i): UNet forward -> p_mean_variance tail + blend -> (noise draw) -> cond_fn.  Returns the pieces
        the update kernels read; nothing of the update itself.  `n_known` is passed through, except True (a rewrite in a stochastic
        loop): the noise of the kept region is drawn right after the step's own."""
        smp, model, cond_fn, native = self.sampler, self.model, self.cond_fn, self.native
        ctx, lib = smp.ctx, smp.ctx.lib
        B, _, H, W = x.shape
        fac_index = cond_fn.fac_index() if native else None
        coef = smp.tables.step_coef(i, fac_index)
        ts, y = self.ts[i], self.model_kwargs.get("y")
        x0, mean, logvar, xin, scal = self.x0, self.mean, self.logvar, self.xin, None
        if cond_fn is None or native:
            if self.ahead is not None:
                # the embedding head of this step ran ahead on the side stream (EmbedAhead): wait for it, run the rest of the model
                out6 = self.ahead.forward(model, x, self.out6)
            else:
                out6 = model.forward(x, ts, y, out=self.out6)
            ctx.check(lib.cgd_pmv_blend(ctx.h, x.data_ptr(), out6.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(),
                                        xin.data_ptr(), B, H, W, coef, ctx.stream()))
            if noise is None and draw_noise:
                noise = smp._draw_like(x)  # drawn before cond_fn, as in p_sample_with_grad
            n_known = smp._draw_like(x) if n_known is True else n_known
            if native:
                cond_fn.step_ts = ts  # the model timesteps this forward received: a classifier term is evaluated at them
            g = cond_fn.native(x, x0, xin, coef) if native else None
            scal = cond_fn.scalars if (native and g is not None and cond_fn.use_magnitude) else None
        else:
            # generic plugin path: reference semantics via autograd over the C-ABI UNet node
            with th.enable_grad():
                xr = x.detach().requires_grad_()
                out6 = model(xr, ts, y)  # autograd node over cgd_unet_forward / cgd_unet_dgrad (nets.UNetFunction)
                eps, v = out6[:, :3], out6[:, 3:]
                frac = (v + 1) / 2
                lv = frac * coef.max_log + (1 - frac) * coef.min_log
                p0 = coef.sqrt_recip * xr - coef.sqrt_recipm1 * eps
                mu = coef.coef1 * p0 + coef.coef2 * xr
                if noise is None and draw_noise:
                    noise = smp._draw_like(x)
                n_known = smp._draw_like(x) if n_known is True else n_known
                t_idx = th.full((B,), i, device=x.device, dtype=th.long)
                p = {"mean": mu, "variance": th.exp(lv), "log_variance": lv, "pred_xstart": p0}
                g = cond_fn(xr, t_idx, p, **self.model_kwargs)
            g = g.detach().float().contiguous()
            x0.copy_(p0.detach()); mean.copy_(mu.detach()); logvar.copy_(lv.detach())
        return self.Eval(x0, mean, logvar, g, scal, noise, coef, ts, fac_index, n_known)


class _Rewrite:
    """What `mask=` and `ilvr=` put after every update: a region of the new state (the mask's kept region, ILVR's low-frequency band) is
    replaced by that of an image (the init image, the reference) noised to the level the update produced.  Two operations: `noise` before
    the step's evaluation, `apply` after its update; subclasses launch."""
    stop = 0  # step indices below it are left alone (ILVR's stop index)

    def __init__(self, sampler, x_T, stochastic):
        self.sampler, self.x_T, self.stochastic = sampler, x_T.contiguous(), stochastic
        self.used, self.keep = 0, None  # tape entries taken; what the last launch read

    def noise(self, x, i):
        """-> the noise of the image for the next `apply`, or True for the evaluation to draw it: the loop's initial noise in the
        deterministic loops (the tensor that q_sampled the init image at the first index: the region follows one trajectory and nothing is
        drawn); in the stochastic loops the tape's next entry, or a fresh draw that the evaluation takes right after the step's own noise.
        Below the stop index, where nothing is rewritten, nothing is drawn."""
        if i < self.stop:
            return None
        if not self.stochastic:
            return self.x_T
        if self.sampler.tape is None:
            return True
        self.used += 1
        return self.sampler.tape[self.tape_key][self.used - 1].to(x.device).float().contiguous()

    def apply(self, i, sample, x0_out, n, again=False):
        """After the update of step index i: `sample` (the state at level i - 1) and `x0_out` (or None) are rewritten in place, with the
        image noised by `n`.  `again` (masks only): this step index runs once more, the re-noised state is returned; otherwise None."""
        if i < self.stop:
            return None
        k = self.sampler.tables.mask_coef(i)
        return self.launch(k, sample, x0_out, n if k.sqrt_one_minus_ab_prev != 0.0 else None, again)  # i == 0: the image itself, no noise


class _Mask(_Rewrite):
    """cgd_masked_merge: the init image goes back into the kept region (mask 0).  With `again` the same launch writes the merged sample
    taken back up to level i (resamples > 1), with the tape's next 'renoise' entry or a fresh draw."""
    tape_key = "known_noise"

    def __init__(self, sampler, x_T, stochastic, init, mask):
        super().__init__(sampler, x_T, stochastic)
        self.init, self.mask = (t.to(x_T.device).float().contiguous() for t in (init, mask))
        self.renoised = 0  # entries of the tape's 'renoise' taken

    def launch(self, k, sample, x0_out, n_known, again):
        smp, ctx = self.sampler, self.sampler.ctx
        B, _, H, W = sample.shape
        n_re = x_re = None
        if again:
            n_re = smp._draw_like(sample) if smp.tape is None else smp.tape["renoise"][self.renoised].to(sample.device).float().contiguous()
            self.renoised += 1
            x_re = th.empty_like(sample)
        k.flags = (L.MASK_PRED_XSTART if x0_out is not None else 0) | (L.MASK_N_KNOWN if n_known is not None else 0) | \
            (L.MASK_RENOISE if n_re is not None else 0)
        init, mask = self.init, self.mask
        ctx.check(ctx.lib.cgd_masked_merge(ctx.h, sample.data_ptr(), L.ptr(x0_out), init.data_ptr(), mask.data_ptr(), L.ptr(n_known),
                                           L.ptr(n_re), L.ptr(x_re), B, H, W, init.shape[0], mask.shape[0], mask.shape[1], k, ctx.stream()))
        self.keep = (n_known, n_re)
        return x_re


class _Ilvr(_Rewrite):
    """cgd_ilvr_refine at step indices >= stop: the low-frequency band of the state becomes that of the reference noised to the state's
    level, the one of pred_xstart that of the reference.  The scratch of the two launches lives as long as the loop."""
    tape_key = "ilvr_noise"

    def __init__(self, sampler, x_T, stochastic, ref, factor, stop):
        super().__init__(sampler, x_T, stochastic)
        if sampler.shard is not None and ref.shape[0] == sampler.shard[1] and ref.shape[0] != 1:
            ref = ref[sampler.shard[0]]  # a reference of the global batch: this rank's rows
        self.ref, self.factor, self.stop = ref.to(x_T.device).float().contiguous(), factor, stop
        floats = sampler.ctx.lib.cgd_ilvr_scratch_floats(x_T.shape[0], x_T.shape[2], x_T.shape[3], factor, 1)
        self.scratch = th.empty(int(floats), device=x_T.device, dtype=th.float32)

    def launch(self, k, sample, x0_out, n, again):
        ctx, ref = self.sampler.ctx, self.ref
        B, _, H, W = sample.shape
        ctx.check(ctx.lib.cgd_ilvr_refine(ctx.h, sample.data_ptr(), L.ptr(x0_out), ref.data_ptr(), L.ptr(n), self.scratch.data_ptr(),
                                          B, H, W, ref.shape[0], self.factor, k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev, ctx.stream()))
        self.keep = (n,)


class _Stepper:
    """The update rule of one loop.  `step` is what the loop calls: rewrite noise -> guided evaluation -> `update` (the subclass's launches,
    which returns what they read, to be kept alive) -> rewrite."""
    draws_noise = False  # whether every evaluation takes a per-step noise: a fresh draw, or the replay tape's next entry
    stochastic = False  # whether that noise enters the state, so that a rewrite noises its image afresh per step too
    one_evaluation = True  # per step, which EmbedAhead's one-embedding-per-step choreography assumes

    def step(self, run, x, i, noise, again=False):
        """One step at (x, i) -> ({"sample", "pred_xstart"}, the re-noised state when the step index runs `again`, else None)"""
        ev = run.evaluate(x, i, noise, self.draws_noise, run.rewrite.noise(x, i) if run.rewrite is not None else None)
        sample, x0_out = th.empty_like(x), th.empty_like(x)
        run.keep = self.update(run, x, i, ev, sample, x0_out)
        x_re = run.rewrite.apply(i, sample, x0_out, ev.n_known, again) if run.rewrite is not None else None
        return {"sample": sample, "pred_xstart": x0_out}, x_re


class _Ancestral(_Stepper):
    """p_sample, or DDIM with `eta`.  DDIM with eta > 0 runs its update through cgd_multistep_update (phase 3); eta == 0 keeps
    cgd_sample_update mode 1, which takes a noise tensor (a draw, or the tape's entry) that its update does not use: the loop stays
    deterministic and a rewrite follows the loop's initial noise."""
    draws_noise = True

    def __init__(self, ddim=False, eta=0.0):
        self.mode, self.eta, self.stochastic = (1 if ddim else 0), eta, not ddim or bool(eta)  # mode: cgd_sample_update's

    def update(self, run, x, i, ev, sample, x0_out):
        tables, ctx = run.sampler.tables, run.sampler.ctx
        if self.eta:
            ab, abp = float(tables.alphas_cumprod[i]), float(tables.alphas_cumprod_prev[i])
            sigma = self.eta * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
            m = L.Multistep(3, 0, sigma, math.sqrt(max(0.0, 1 - abp - sigma * sigma)))
            ctx.check(ctx.lib.cgd_multistep_update(ctx.h, x.data_ptr(), None, ev.x0.data_ptr(), L.ptr(ev.g), L.ptr(ev.scal), ev.noise.data_ptr(),
                                                   None, None, sample.data_ptr(), x0_out.data_ptr(), *run.dims, ev.coef, None, m, ctx.stream()))
        else:
            ctx.check(ctx.lib.cgd_sample_update(ctx.h, x.data_ptr(), ev.x0.data_ptr(), ev.mean.data_ptr(), ev.logvar.data_ptr(), L.ptr(ev.g),
                                                ev.noise.data_ptr(), L.ptr(ev.scal), sample.data_ptr(), x0_out.data_ptr(), *run.dims, ev.coef,
                                                self.mode, ctx.stream()))
        return ev.noise, ev.g, ev.ts


class _Plms(_Stepper):
    """PLMS (plms_sample of the guided_diffusion fork); draws no noise.  `old_eps`: history buffers (oldest first), `free`: spare buffers.
    The history rotates by pointer: the buffer dropped from the front is the next step's eps_out.  Under a rewrite the start step's
    predictor (level i - 1, the input of the second evaluation) is rewritten before that evaluation, and every step's result afterwards;
    the eps history stays as evaluated."""
    one_evaluation = False  # the start step evaluates twice

    def __init__(self, order):
        self.order, self.old_eps, self.free = order, [], []

    def update(self, run, x, i, ev, sample, x0_out):
        tables, ctx, lib = run.sampler.tables, run.sampler.ctx, run.sampler.ctx.lib
        order, old, g, s = self.order, self.old_eps, ev.g, ctx.stream()
        eps_new = self.free.pop() if self.free else th.empty_like(x)
        if order > 1 and not old:
            # start step, pseudo improved Euler: predictor at t, a second guided evaluation at (predictor, t-1), corrector
            xp = th.empty_like(x)  # once per loop: the history is never empty again
            ctx.check(lib.cgd_multistep_update(ctx.h, x.data_ptr(), None, ev.x0.data_ptr(), L.ptr(g), L.ptr(ev.scal), None, None,
                                               eps_new.data_ptr(), xp.data_ptr(), x0_out.data_ptr(), *run.dims, ev.coef, None,
                                               L.Multistep(1, 0, 0.0, 0.0), s))
            old.append(eps_new)
            if run.rewrite is not None:
                run.rewrite.apply(i, xp, None, ev.n_known)
            ev2 = run.evaluate(xp, i - 1, None, False)
            hist = (C.c_void_p * 3)(eps_new.data_ptr(), None, None)
            k_t = tables.step_coef(i, ev.fac_index)
            ctx.check(lib.cgd_multistep_update(ctx.h, x.data_ptr(), xp.data_ptr(), ev2.x0.data_ptr(), L.ptr(ev2.g), L.ptr(ev2.scal), None,
                                               hist, None, sample.data_ptr(), None, *run.dims, ev2.coef, k_t, L.Multistep(2, 0, 0.0, 0.0), s))
            keep = (g, ev2.g, ev.ts, ev2.ts, xp)
        else:
            # Adams-Bashforth of min(order, history + 1) terms, the newest history entry first
            prev = [old[-1 - j].data_ptr() if j < len(old) else None for j in range(3)]
            ctx.check(lib.cgd_multistep_update(ctx.h, x.data_ptr(), None, ev.x0.data_ptr(), L.ptr(g), L.ptr(ev.scal), None,
                                               (C.c_void_p * 3)(*prev), eps_new.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), *run.dims,
                                               ev.coef, None, L.Multistep(0, min(order, len(old) + 1), 0.0, 0.0), s))
            old.append(eps_new)
            keep = (g, ev.ts)
        if len(old) >= order:
            self.free.append(old.pop(0))
        return keep


class _Dpmpp(_Stepper):
    """DPM-Solver++(2M).  `hist`: the guided pred_xstart of the step before (None on the first step, which therefore runs at order 1),
    `free`: the spare buffer.  The history rotates by pointer: the entry the launch has read is the buffer the next launch writes.  Step
    index 0 runs at order 1 (diffusion.dpmpp_coef) and nothing reads the entry of step index 1 or 0, so those are not written.  Under a
    rewrite the history stays as evaluated.
    `threshold` (p, cap): cgd_dpmpp_threshold writes the guided pred_xstart to a buffer and selects the sample's scale s on the device,
    cgd_dpmpp_update_thr clamps, rescales and updates.  The buffer, the (B, 3) result and the selection's scratch (`thr`) are allocated once."""

    def __init__(self, order, eta, threshold):
        self.order, self.eta, self.threshold, self.hist, self.free, self.thr = order, eta, threshold, None, [], None
        self.draws_noise = self.stochastic = bool(eta)  # eta > 0: the SDE solver

    def update(self, run, x, i, ev, sample, x0_out):
        tables, ctx, lib = run.sampler.tables, run.sampler.ctx, run.sampler.ctx.lib
        (B, H, W), noise, g, hist = run.dims, ev.noise, ev.g, self.hist
        d = tables.dpmpp_coef(i, 2 if (self.order == 2 and hist is not None) else 1, self.eta)
        x0c = (self.free.pop() if self.free else th.empty_like(x)) if (self.order == 2 and i > 1) else None
        tail = (L.ptr(noise), L.ptr(hist) if d.c_r else None, L.ptr(x0c), sample.data_ptr(), x0_out.data_ptr(), B, H, W, ev.coef, d, ctx.stream())
        if self.threshold is not None:
            p, cap = self.threshold
            if self.thr is None:
                n = 3 * H * W
                # cap == 1: every scale is 1 (the static clip), nothing is selected and no scratch is needed
                scratch = th.empty(int(lib.cgd_abs_quantile_scratch_bytes(B, n)), dtype=th.uint8, device=x.device) if cap > 1.0 else None
                self.thr = (th.empty_like(x), th.empty((B, 3), dtype=th.float32, device=x.device), scratch, tables.threshold_rank(p, n))
            raw, thr3, scratch, (rank, frac) = self.thr
            ctx.check(lib.cgd_dpmpp_threshold(ctx.h, x.data_ptr(), ev.x0.data_ptr(), L.ptr(g), L.ptr(ev.scal), raw.data_ptr(), B, H, W,
                                              ev.coef, rank, frac, 1.0, cap, thr3.data_ptr(), L.ptr(scratch), ctx.stream()))
            ctx.check(lib.cgd_dpmpp_update_thr(ctx.h, x.data_ptr(), ev.x0.data_ptr(), raw.data_ptr(), thr3.data_ptr(), *tail))
        else:
            ctx.check(lib.cgd_dpmpp_update(ctx.h, x.data_ptr(), ev.x0.data_ptr(), L.ptr(g), L.ptr(ev.scal), *tail))
        if hist is not None:
            self.free.append(hist)
        self.hist = x0c
        return noise, g, ev.ts


class GuidedSampler:
    """`diffusion` object handed to the drop-in generator: owns the host tables (diffusion.SpacedDiffusion) and
    runs the progressive loops on one GPU."""

    def __init__(self, ctx, tables):
        self.ctx = ctx
        self.tables = tables
        self.num_timesteps = tables.num_timesteps
        self.sqrt_one_minus_alphas_cumprod = tables.sqrt_one_minus_alphas_cumprod
        self.timestep_map = tables.timestep_map
        self.tape = None  # optional {'x_T','noise':[...],'y':[...]} replay (tests)
        # multi-GPU sharding: (indices of the global batch this rank owns, global batch size).  Every rank draws
        # the GLOBAL (B,3,H,W) tensors from the same seed, exactly like the batched reference run, and keeps its slice, and there is
        # no per-step collective.  The samples equal those of the batched run (up to the tile / split-K choices of a different batch
        # size) EXCEPT with `use_magnitude`: its RMS clamp (cgd.py:229-232) is taken over the rank's own samples, not over the
        # global batch — a documented deviation for batch > 1; `sat_scale` is normalised by the global batch.
        self.shard = None

    def step_coef(self, i, fac_index=None):
        return self.tables.step_coef(i, fac_index)

    def _draw_like(self, x):
        """randn_like(x); with sharding the global batch is drawn and this rank's rows are kept."""
        if self.shard is None:
            return th.randn_like(x)
        idx, gb = self.shard
        return th.randn((gb,) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)[idx].contiguous()

    def _set_low_res(self, model, model_kwargs):
        """Super-resolution sampling (upstream's super_res_sample puts the image into model_kwargs["low_res"]): once per loop, before the
        first forward, the image goes to the model's handle, which conditions every forward of the loop on it.  Under sharding a
        low_res of the global batch is cut to this rank's rows.  Without "low_res" nothing happens."""
        low = model_kwargs.get("low_res") if model_kwargs else None
        if low is None:
            return
        if not hasattr(model, "set_low_res"):
            raise ValueError('model_kwargs["low_res"] needs a super-resolution model (nets.UNet(in_channels=6): set_low_res)')
        if self.shard is not None and low.shape[0] == self.shard[1] and low.shape[0] != 1:
            low = low[self.shard[0]]
        model.set_low_res(low)

    @staticmethod
    def _check_mask(shape, init_image, mask, resamples, plms=False):
        if not _is_int(resamples) or resamples < 1:
            raise ValueError(f"resamples must be an int >= 1, got {resamples!r}")
        if resamples > 1 and plms:
            raise ValueError("PLMS cannot resample: its eps history would mix noise levels (use the p_sample or DDIM loop)")
        if mask is None:
            if resamples > 1:
                raise ValueError("resamples > 1 needs a mask: the repeats re-run the merge of masked sampling")
            return
        if init_image is None:
            raise ValueError("a mask needs an init image: the kept region is taken from it")
        B, H, W = shape[0], shape[2], shape[3]
        if init_image.dim() != 4 or init_image.shape[0] not in (1, B) or tuple(init_image.shape[1:]) != (3, H, W):
            raise ValueError(f"init_image must be (1 or {B}, 3, {H}, {W}) under a mask, got {tuple(init_image.shape)}")
        if mask.dim() != 4 or mask.shape[0] not in (1, B) or mask.shape[1] not in (1, 3) or tuple(mask.shape[2:]) != (H, W):
            raise ValueError(f"mask must be (1 or {B}, 1 or 3, {H}, {W}), got {tuple(mask.shape)}")
        lo, hi = float(mask.min()), float(mask.max())
        if not (lo >= 0.0 and hi <= 1.0):
            raise ValueError(f"mask values must lie in [0, 1] (1 regenerates, 0 keeps), got [{lo}, {hi}]")

    def _check_ilvr(self, shape, ilvr, mask, resamples):
        """None | (ref, factor) | (ref, factor, stop) -> None | (ref, factor, stop); refusals before anything runs"""
        if ilvr is None:
            return None
        if mask is not None:
            raise ValueError("ilvr and mask cannot be combined: both rewrite the state after every update")
        if _is_int(resamples) and resamples > 1:
            raise ValueError("ilvr cannot resample: resamples > 1 repeats the merge of masked sampling")
        if not isinstance(ilvr, (tuple, list)) or len(ilvr) not in (2, 3):
            raise ValueError("ilvr must be (ref, factor) or (ref, factor, stop)")
        ref, factor = ilvr[0], ilvr[1]
        stop = ilvr[2] if len(ilvr) == 3 else 0
        B, H, W = shape[0], shape[2], shape[3]
        if not _is_int(factor) or not 2 <= factor <= 64 or factor & (factor - 1):
            raise ValueError(f"the ilvr factor must be a power of two in [2, 64], got {factor!r}")
        if H % factor or W % factor:
            raise ValueError(f"the ilvr factor {factor} does not divide the {H} x {W} frame")
        if not th.is_tensor(ref) or ref.dim() != 4 or tuple(ref.shape[1:]) != (3, H, W):
            raise ValueError(f"the ilvr reference must be (1 or {B}, 3, {H}, {W})")
        gb = self.shard[1] if self.shard is not None else B
        if ref.shape[0] not in (1, B, gb):
            raise ValueError(f"the ilvr reference must be (1 or {B}, 3, {H}, {W}), got {tuple(ref.shape)}")
        if not _is_int(stop) or not 0 <= stop <= self.num_timesteps:
            raise ValueError(f"the ilvr stop index must be an int in [0, {self.num_timesteps}], got {stop!r}")
        return ref, factor, stop

    # ---- loops ------------------------------------------------------------------------------------------
    @staticmethod
    def _check_guards(clip_denoised, cond_fn, cond_fn_with_grad):
        if clip_denoised:
            raise NotImplementedError("the reference samples with clip_denoised=False (cgd.py:253)")
        if cond_fn is not None and not cond_fn_with_grad:
            raise NotImplementedError("the reference passes cond_fn_with_grad=True (cgd.py:260)")

    def _loop(self, stepper, model, shape, *, noise, cond_fn, model_kwargs, device, progress, skip_timesteps, init_image, randomize_class,
              mask=None, resamples=1, ilvr=None):
        """The loop of every sampler; `stepper` is its update rule (_Ancestral, _Plms, _Dpmpp).  The arguments arrive checked by the public
        loops, `ilvr` as the (ref, factor, stop) of _check_ilvr."""
        device = th.device(device or f"cuda:{self.ctx.device}")
        tape = self.tape
        if noise is not None:
            img = noise.to(device).float()
        elif tape is not None:
            img = tape["x_T"].to(device).float()
        elif self.shard is not None:
            idx, gb = self.shard
            assert shape[0] == len(idx), "shape[0] must be this rank's share of the global batch"
            img = th.randn(gb, *shape[1:], device=device)[idx]
        else:
            img = th.randn(*shape, device=device)
        if skip_timesteps and init_image is None:
            init_image = th.zeros_like(img)
        # a rewrite's x_T is img as it is here: in a loop that is not stochastic its image keeps the loop's initial noise
        rewrite = _Mask(self, img, stepper.stochastic, init_image, mask) if mask is not None else None
        if ilvr is not None:
            rewrite = _Ilvr(self, img, stepper.stochastic, *ilvr)
        indices = list(range(self.num_timesteps - skip_timesteps))[::-1]
        if init_image is not None:
            img = float(self.tables.sqrt_alphas_cumprod[indices[0]]) * init_image.to(device).float() + \
                float(self.tables.sqrt_one_minus_alphas_cumprod[indices[0]]) * img
        model_kwargs = dict(model_kwargs or {})
        self._set_low_res(model, model_kwargs)
        it = indices
        if progress:
            from tqdm.auto import tqdm
            it = tqdm(indices)
        img = img.contiguous()
        run = _Run(self, model, cond_fn, model_kwargs, img, rewrite)

        def draw_y(n):
            """step n's class labels under `randomize_class` — same draws, in the same order of the generator, as the reference loop"""
            if tape is not None:
                return tape["y"][n].to(device)
            if self.shard is not None:
                return th.randint(0, model.num_classes, (self.shard[1],), device=device)[self.shard[0]]
            return th.randint(0, model.num_classes, model_kwargs["y"].shape, device=device)

        rand_y = bool(randomize_class and "y" in model_kwargs)
        # EmbedAhead's one-embedding-per-step choreography applies neither to PLMS, whose start step evaluates the model twice, nor to
        # the repeated evaluations of resamples > 1
        ahead = run.ahead = EmbedAhead.create(self, model, cond_fn, img, indices) if (stepper.one_evaluation and resamples == 1) else None
        evals = 0  # evaluations so far: the tape's step noise is consumed per evaluation
        for n, i in enumerate(it):
            if rand_y and (ahead is None or n == 0):
                model_kwargs["y"] = draw_y(n)
            if ahead is not None and n == 0:
                ahead.launch(model, 0, model_kwargs.get("y"))
            # masked sampling with resamples = r: step index i > 0 runs r times; after each of the first r - 1 merges the state goes back
            # up one level (written by the merge's launch, returned by the step) and the step runs again.  One yield per step index.
            repeats = resamples if (rewrite is not None and i > 0) else 1
            for r in range(repeats):
                step_noise = tape["noise"][evals].to(device).float().contiguous() if (tape is not None and stepper.draws_noise) else None
                evals += 1
                with th.no_grad():
                    out, img = stepper.step(run, img, i, step_noise, r + 1 < repeats)  # img: the re-noised state while the index repeats
            if ahead is not None and tape is not None and rand_y and n + 1 >= len(tape["y"]):
                ahead = run.ahead = None  # a replay tape shorter than the schedule (tests that run a few steps): the remaining steps run in line
            if ahead is not None and n + 1 < len(indices):
                # step n is enqueued: now (host order = the reference's order of random draws: after this step's noise) draw the next step's
                # labels and run its embedding head on the side stream, where it overlaps this step's kernels
                with ahead.side_stream():
                    if rand_y:
                        model_kwargs["y"] = draw_y(n + 1)
                    ahead.launch(model, n + 1, model_kwargs.get("y"))
            yield out
            img = out["sample"]

    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                  model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                                  randomize_class=False, cond_fn_with_grad=False, mask=None, resamples=1, ilvr=None):
        """`mask` ((1 or B, 1 or 3, H, W) in [0, 1], with `init_image`): masked sampling, 1 regenerates and 0 keeps the init image;
        `resamples`: how often every step index > 0 runs (RePaint with jump length 1).
        `ilvr`: None, (ref, factor) or (ref, factor, stop): ILVR, after every update of a step index >= stop (default 0) the low-frequency
        band of the state (the antialiased cubic resize down by `factor`, a power of two in [2, 64] that divides H and W, and back up)
        is replaced by that of `ref` ((1 or B, 3, H, W) in [-1, 1]) noised to the level the update produced, with a fresh draw per
        refinement.  Not together with `mask` or `resamples` > 1."""
        ilvr = self._check_ilvr(shape, ilvr, mask, resamples)
        self._check_mask(shape, init_image, mask, resamples)
        self._check_guards(clip_denoised, cond_fn, cond_fn_with_grad)
        return self._loop(_Ancestral(), model, shape, noise=noise, cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, progress=progress,
                          skip_timesteps=skip_timesteps, init_image=init_image, randomize_class=randomize_class, mask=mask, resamples=resamples,
                          ilvr=ilvr)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, eta=0.0, skip_timesteps=0, init_image=None,
                                     randomize_class=False, cond_fn_with_grad=False, mask=None, resamples=1, ilvr=None):
        """eta == 0 (what the reference passes): cgd_sample_update mode 1.  eta > 0: ddim_sample_with_grad's sigma term with the
        per-step noise draw of this loop, through cgd_multistep_update.  `mask`, `resamples`: as in p_sample_loop_progressive; with
        eta == 0 the kept region is noised with the loop's initial noise throughout and a masked run stays deterministic.  `ilvr`: as in
        p_sample_loop_progressive; with eta == 0 the reference is noised with the loop's initial noise and nothing is drawn."""
        eta = float(eta)
        if not eta >= 0.0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        ilvr = self._check_ilvr(shape, ilvr, mask, resamples)
        self._check_mask(shape, init_image, mask, resamples)
        self._check_guards(clip_denoised, cond_fn, cond_fn_with_grad)
        return self._loop(_Ancestral(True, eta), model, shape, noise=noise, cond_fn=cond_fn, model_kwargs=model_kwargs, device=device,
                          progress=progress, skip_timesteps=skip_timesteps, init_image=init_image, randomize_class=randomize_class, mask=mask,
                          resamples=resamples, ilvr=ilvr)

    def plms_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                     model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                                     randomize_class=False, cond_fn_with_grad=False, order=2, mask=None, resamples=1, ilvr=None):
        """PLMS (pseudo linear multistep, Liu et al., ICLR 2022) as the guided_diffusion fork's `plms_sample_loop_progressive`:
        a first step of pseudo improved Euler (two guided evaluations, at t and at t-1) when order > 1, Adams-Bashforth of up to
        `order` eps terms afterwards.  No per-step noise.  A schedule of a single step with order > 1 would evaluate at t = -1 and is
        refused (the fork indexes its tables with -1 there).  `mask`: masked sampling as in p_sample_loop_progressive, the kept region
        noised with the loop's initial noise; `resamples` > 1 is refused (the eps history would mix noise levels).  `ilvr`: as in
        ddim_sample_loop_progressive with eta == 0; the start step's predictor is refined before its second evaluation, the eps history
        stays as evaluated."""
        if not _is_int(order) or not 1 <= order <= 4:
            raise ValueError(f"order is invalid (should be int from 1-4): {order!r}")
        self._check_guards(clip_denoised, cond_fn, cond_fn_with_grad)
        if order > 1 and self.num_timesteps - skip_timesteps < 2:
            raise ValueError(f"PLMS of order {order} needs at least two timesteps: its first step also evaluates at t - 1")
        ilvr = self._check_ilvr(shape, ilvr, mask, resamples)
        self._check_mask(shape, init_image, mask, resamples, plms=True)
        return self._loop(_Plms(order), model, shape, noise=noise, cond_fn=cond_fn, model_kwargs=model_kwargs, device=device, progress=progress,
                          skip_timesteps=skip_timesteps, init_image=init_image, randomize_class=randomize_class, mask=mask, ilvr=ilvr)

    def dpmpp_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                                      model_kwargs=None, device=None, progress=False, skip_timesteps=0, init_image=None,
                                      randomize_class=False, cond_fn_with_grad=False, order=2, eta=0.0, mask=None, resamples=1, threshold=None,
                                      ilvr=None):
        """DPM-Solver++(2M) (Lu et al., 2022: data prediction, multistep): one guided evaluation per step; the update extrapolates the guided
        pred_xstart with the one of the step before (`order` 2; the first step and step index 0 run at order 1; `order` 1 is DDIM with the
        same eta for eta in {0, 1}).  eta == 0: the deterministic solver, no per-step noise.  eta > 0: the SDE solver (eta = 1 is
        SDE-DPM-Solver++(2M)), one noise draw per evaluation before cond_fn, as in DDIM with eta.  Meant for tables spaced uniformly in
        logSNR (timestep_respacing 'dpmN'); on the integer-stride levels of 'ddimN' the second order gains nothing below about 50 steps
        (DESIGN.md).  `mask`: masked sampling as in ddim_sample_loop_progressive (eta == 0: the kept region is noised with the loop's
        initial noise); `resamples` > 1 is refused: a resampled history would mix noise levels.  `ilvr`: as in
        ddim_sample_loop_progressive (a fresh draw per refinement with eta > 0); the pred_xstart history stays as evaluated.
        `threshold`: None, p, or (p, cap): dynamic thresholding of the guided pred_xstart (Saharia et al., 2022).  Per sample, s = the
        p-quantile of |guided pred_xstart| (p in (0, 1]; torch.quantile's 'linear' rule, selected exactly on the device), raised to at least 1
        and lowered to at most `cap` (>= 1; none when not given); the prediction is clamped to [-s, s] and divided by s before the update, and
        the history holds the thresholded predictions.  cap = 1 is the static clip of the guided prediction to [-1, 1].  With order 1 this
        is thresholded DDIM.  The yielded pred_xstart stays the unguided prediction."""
        if not _is_int(order) or order not in (1, 2):
            raise ValueError(f"order is invalid (should be 1 or 2): {order!r}")
        if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not eta >= 0.0:
            raise ValueError(f"eta must be a number >= 0, got {eta!r}")
        self._check_guards(clip_denoised, cond_fn, cond_fn_with_grad)
        if _is_int(resamples) and resamples > 1:
            raise ValueError("DPM-Solver++ cannot resample: its pred_xstart history would mix noise levels (use the DDIM loop, "
                             "ddim_sample_loop_progressive, for resamples > 1)")
        ilvr = self._check_ilvr(shape, ilvr, mask, resamples)
        self._check_mask(shape, init_image, mask, resamples)
        return self._loop(_Dpmpp(order, float(eta), self._check_threshold(threshold)), model, shape, noise=noise, cond_fn=cond_fn,
                          model_kwargs=model_kwargs, device=device, progress=progress, skip_timesteps=skip_timesteps, init_image=init_image,
                          randomize_class=randomize_class, mask=mask, ilvr=ilvr)

    @staticmethod
    def _check_threshold(threshold):
        """None | p | (p, cap) -> None | (p, cap) as floats, cap = inf when not given"""
        if threshold is None:
            return None
        p, cap = threshold if isinstance(threshold, (tuple, list)) and len(threshold) == 2 else (threshold, math.inf)
        for v in (p, cap):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"threshold must be None, p or (p, cap) with numbers, got {threshold!r}")
        if not 0.0 < p <= 1.0:
            raise ValueError(f"threshold: the quantile p must lie in (0, 1], got {p!r}")
        if not cap >= 1.0:
            raise ValueError(f"threshold: cap must be >= 1 (1 is the static clip to [-1, 1]), got {cap!r}")
        return float(p), float(cap)

    # ---- DDIM inversion ---------------------------------------------------------------------------------
    def ddim_reverse_sample_loop_progressive(self, model, image, clip_denoised=False, model_kwargs=None, device=None, progress=False,
                                             skip_timesteps=0):
        """guided_diffusion's `ddim_reverse_sample_loop`, progressive: the deterministic DDIM ODE (eta 0) upwards from `image` ((B,3,H,W)
        in [-1, 1]), step indices 0 .. t0 - 1 with t0 = num_timesteps - 1 - skip_timesteps, so that the last state sits at level t0, the
        first index of a sampling loop called with the same `skip_timesteps`.  Per step: model.forward at the index's model timestep and
        one cgd_ddim_reverse_update launch; eps is the model's output (csrc/invert.hip).  Yields {"sample", "pred_xstart"} per step; the
        last yield also carries "noise", the tensor for which q_sample(image, t0, noise) == sample.  Unguided; `y` is taken from
        `model_kwargs` as given; nothing random is drawn.
        Level offset (upstream's, kept): the clean image is treated as the state at level 0, although a state at level 0 carries
        1 - abar_0 of noise.  A sampling run from the latent therefore reproduces the image as the state ENTERING step index 0, not as that
        step's pred_xstart, which differs from it by sqrt_recipm1[0] eps."""
        if clip_denoised:
            raise NotImplementedError("DDIM inversion runs with clip_denoised=False: clamping pred_xstart breaks the ODE the sampling loops "
                                      "run back down (the reference samples with clip_denoised=False, cgd.py:253)")
        if not _is_int(skip_timesteps) or skip_timesteps < 0:
            raise ValueError(f"skip_timesteps must be an int >= 0, got {skip_timesteps!r}")
        t0 = self.num_timesteps - 1 - skip_timesteps
        if t0 < 1:
            raise ValueError(f"DDIM inversion needs at least one step below level num_timesteps - 1 - skip_timesteps = {t0}: "
                             f"{self.num_timesteps} timesteps, {skip_timesteps} skipped")
        if not th.is_tensor(image) or image.dim() != 4 or image.shape[1] != 3 or 0 in image.shape:
            raise ValueError(f"image must be (B, 3, H, W), got {tuple(image.shape) if th.is_tensor(image) else type(image).__name__}")
        return self._reverse_loop(model, image, dict(model_kwargs or {}), th.device(device or f"cuda:{self.ctx.device}"), progress, t0)

    def _reverse_loop(self, model, image, model_kwargs, device, progress, t0):
        ctx, lib = self.ctx, self.ctx.lib
        init = image.to(device).float().contiguous()
        B, _, H, W = init.shape
        self._set_low_res(model, model_kwargs)
        tt = _timestep_table(self.tables, t0, B, device)
        y = model_kwargs.get("y")
        out6 = th.empty((B, 6, H, W), device=device, dtype=th.float32)
        it = range(t0)
        if progress:
            from tqdm.auto import tqdm
            it = tqdm(it, desc="DDIM inversion")
        x = init
        for i in it:
            last = i == t0 - 1
            with th.no_grad():
                o6 = model.forward(x, tt[i], y, out=out6)
                x_next, x0 = th.empty_like(init), th.empty_like(init)
                noise = th.empty_like(init) if last else None
                ctx.check(lib.cgd_ddim_reverse_update(ctx.h, x.data_ptr(), o6.data_ptr(), init.data_ptr() if last else None,
                                                      x_next.data_ptr(), x0.data_ptr(), L.ptr(noise), B, H, W, B,
                                                      self.tables.reverse_coef(i), ctx.stream()))
            out = {"sample": x_next, "pred_xstart": x0}
            if last:
                out["noise"] = noise
            yield out
            x = x_next

    def ddim_invert(self, model, image, clip_denoised=False, model_kwargs=None, device=None, progress=False, skip_timesteps=0):
        """Drains ddim_reverse_sample_loop_progressive -> (latent, noise): the state at level t0 = num_timesteps - 1 - skip_timesteps and
        the tensor for which q_sample(image, t0, noise) == latent.  Any sampling loop of this class, masked or not, sharded or not, starts
        from the latent when called with `noise=noise, init_image=image, skip_timesteps=skip_timesteps`; under a mask the deterministic
        loops re-noise the kept region with that same tensor, consistent with the start state.  Reconstructing the image needs the class
        fixed over the run (an unconditional model, or randomize_class=False with the `y` given here)."""
        out = None
        for out in self.ddim_reverse_sample_loop_progressive(model, image, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                                             device=device, progress=progress, skip_timesteps=skip_timesteps):
            pass
        return out["sample"], out["noise"]
