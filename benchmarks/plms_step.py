"""Wall time of whole guided sampling runs with PLMS against the p_sample schedule at the headline shape (bench.py config 2: 256x256,
cutn 16, CLIP ViT-B/32, batch 1, synthetic weights), in one process:

  respace-250  p_sample_loop_progressive over the 250-step schedule (what `-respace 250` runs)
  plms50       plms_sample_loop_progressive(order=2) over 'plms50' (what `-respace plms50` runs: 51 guided evaluations)

Each mode runs --runs full trajectories from x_T after one untimed warm-up run; wall clock around work that ends in a device
synchronise.  Then the microseconds per launch of cgd_multistep_update (PLMS order 4, and DDIM eta) against cgd_sample_update mode 1
at the same shape, from HIP events.  Prints one JSON line.  Usage: python benchmarks/plms_step.py [--runs 3]"""
import argparse
import ctypes as C
import json
import statistics

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=500)
    ap.add_argument("--launch-repeats", type=int, default=5)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    from cgd_amd import sampler
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp250, guid, _) = steplib.setup()
    smp_plms = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "plms50", False))
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}

    def run(mode):
        smp = smp250 if mode == "respace-250" else smp_plms
        guid.diffusion = smp
        guid.current_timestep = smp.num_timesteps - 1
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
        gen = smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw) if mode == "respace-250" else \
            smp.plms_sample_loop_progressive(unet, (1, 3, H, W), order=2, **kw)
        t, n, out = steplib.drain(gen, guid)
        return t, n, bool(th.isfinite(out["sample"]).all())

    modes = ["respace-250", "plms50"]
    res = steplib.alternate(modes, run, args.runs)
    times = {m: [t for t, _, _ in v] for m, v in res.items()}
    steps, finite = {m: v[-1][1] for m, v in res.items()}, {m: v[-1][2] for m, v in res.items()}

    # per-launch cost of the updates at the headline shape
    x, x0, g, noise = (th.randn(1, 3, H, W, device=dev) for _ in range(4))
    mean, logvar = th.randn_like(x), th.randn_like(x) * 0.1 - 5
    hist = [th.randn_like(x) for _ in range(3)]
    eps_out, sample, x0_out = th.empty_like(x), th.empty_like(x), th.empty_like(x)
    scal = th.ones(8, device=dev)
    k = smp_plms.tables.step_coef(25, 25)
    hp = (C.c_void_p * 3)(*[h.data_ptr() for h in hist])

    def sample_update():
        ctx.check(ctx.lib.cgd_sample_update(ctx.h, x.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), g.data_ptr(),
                                            noise.data_ptr(), scal.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, k, 1,
                                            ctx.stream()))

    def multistep(phase, order, sigma=0.0, dirc=0.0):
        m = L.Multistep(phase, order, sigma, dirc)

        def fn():
            ctx.check(ctx.lib.cgd_multistep_update(ctx.h, x.data_ptr(), None, x0.data_ptr(), g.data_ptr(), scal.data_ptr(), noise.data_ptr(),
                                                   hp, eps_out.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, k, None, m,
                                                   ctx.stream()))
        return fn

    launch_us = steplib.per_launch({"cgd_sample_update_mode1": sample_update, "cgd_multistep_update_plms_order4": multistep(0, 4),
                                    "cgd_multistep_update_plms_order2": multistep(0, 2),
                                    "cgd_multistep_update_ddim_eta": multistep(3, 0, 0.1, 0.9)}, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in times.items()}
    print(json.dumps({"what": "seconds per full guided sampling run, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, synthetic "
                              f"weights), median of {args.runs} runs", "s_per_run": {m: round(v, 3) for m, v in med.items()},
                      "runs_s": {m: [round(t, 3) for t in v] for m, v in times.items()}, "steps_yielded": steps, "finite": finite,
                      "ms_per_yielded_step": {m: round(med[m] / steps[m] * 1e3, 3) for m in modes},
                      "plms50_over_respace250": round(med["plms50"] / med["respace-250"], 4),
                      "update_launch_us": {n: steplib.stats(v) for n, v in launch_us.items()}, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
