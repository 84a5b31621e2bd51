"""Wall time of whole guided sampling runs with DPM-Solver++(2M) on the logSNR-uniform spacing against PLMS and the p_sample schedule at
the headline shape (bench.py config 2: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights), in one process:

  respace-250  p_sample_loop_progressive over the 250-step schedule (what `-respace 250` runs)
  plms50       plms_sample_loop_progressive(order=2) over 'plms50' (what `-respace plms50` runs: 51 guided evaluations)
  dpm20        dpmpp_sample_loop_progressive(order=2, eta=0) over 'dpm20' (what `-respace dpm20` runs: 20 guided evaluations)

Each mode runs --runs full trajectories from x_T after one untimed warm-up run; wall clock around work that ends in a device
synchronise.  Then the microseconds per launch of cgd_dpmpp_update (second order, eta = 0 and eta = 1) against cgd_sample_update mode 1
at the same shape, from HIP events, --launch-repeats times each in turn.  Synthetic weights: the runs time the work, they say nothing
about image quality.  Prints one JSON line.  Usage: python benchmarks/dpm_step.py [--runs 3]"""
import argparse
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
    from cgd_amd import sampler
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp250, guid, _) = steplib.setup()
    smps = {"respace-250": smp250,
            "plms50": sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "plms50", False)),
            "dpm20": sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "dpm20", False))}
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}

    def run(mode):
        smp = smps[mode]
        guid.diffusion = smp
        guid.current_timestep = smp.num_timesteps - 1
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
        if mode == "respace-250":
            gen = smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw)
        elif mode == "plms50":
            gen = smp.plms_sample_loop_progressive(unet, (1, 3, H, W), order=2, **kw)
        else:
            gen = smp.dpmpp_sample_loop_progressive(unet, (1, 3, H, W), order=2, eta=0.0, **kw)
        t, n, out = steplib.drain(gen, guid)
        return t, n, bool(th.isfinite(out["sample"]).all())

    modes = list(smps)
    res = steplib.alternate(modes, run, args.runs)
    times = {m: [t for t, _, _ in v] for m, v in res.items()}
    steps, finite = {m: v[-1][1] for m, v in res.items()}, {m: v[-1][2] for m, v in res.items()}

    # per-launch cost of the updates at the headline shape
    x, x0, g, noise, hist = (th.randn(1, 3, H, W, device=dev) for _ in range(5))
    mean, logvar = th.randn_like(x), th.randn_like(x) * 0.1 - 5
    x0c, sample, x0_out = th.empty_like(x), th.empty_like(x), th.empty_like(x)
    scal = th.ones(8, device=dev)
    tab = smps["dpm20"].tables
    k = tab.step_coef(10, 10)

    def sample_update():
        ctx.check(ctx.lib.cgd_sample_update(ctx.h, x.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), g.data_ptr(),
                                            noise.data_ptr(), scal.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, k, 1,
                                            ctx.stream()))

    def dpmpp(eta):
        d = tab.dpmpp_coef(10, 2, eta)

        def fn():
            ctx.check(ctx.lib.cgd_dpmpp_update(ctx.h, x.data_ptr(), x0.data_ptr(), g.data_ptr(), scal.data_ptr(), noise.data_ptr(),
                                               hist.data_ptr(), x0c.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, k, d,
                                               ctx.stream()))
        return fn

    fns = {"cgd_sample_update_mode1": sample_update, "cgd_dpmpp_update_2m_eta0": dpmpp(0.0), "cgd_dpmpp_update_2m_eta1": dpmpp(1.0)}
    launch = steplib.per_launch(fns, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in times.items()}
    print(json.dumps({"what": "seconds per full guided sampling run, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, synthetic "
                              f"weights), median of {args.runs} runs", "s_per_run": {m: round(v, 3) for m, v in med.items()},
                      "runs_s": {m: [round(t, 3) for t in v] for m, v in times.items()}, "steps_yielded": steps, "finite": finite,
                      "ms_per_yielded_step": {m: round(med[m] / steps[m] * 1e3, 3) for m in modes},
                      "dpm20_over_respace250": round(med["dpm20"] / med["respace-250"], 4),
                      "dpm20_over_plms50": round(med["dpm20"] / med["plms50"], 4),
                      "update_launch_us": {n: steplib.stats(v) for n, v in launch.items()}, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
