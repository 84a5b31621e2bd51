"""Cost of dynamic thresholding under DPM-Solver++(2M) at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP ViT-B/32, batch 1,
synthetic weights), in one process:

  dpm20        dpmpp_sample_loop_progressive(order=2, eta=0) over 'dpm20' (what `-respace dpm20` runs)
  dpm20+thr    the same with threshold=0.995 (what `-respace dpm20+thr=0.995` runs)

The two modes alternate, --runs full trajectories each after one untimed warm-up run; wall clock around work that ends in a device
synchronise; the library's launch counter gives the launches per step of each.  Then the microseconds of the selection alone
(cgd_op_abs_quantile, p = 0.995: five launches) at n = 196608 and 786432 (3 x 256^2 and 3 x 512^2), B = 1 and 4, and of
cgd_dpmpp_threshold + cgd_dpmpp_update_thr against cgd_dpmpp_update at the headline shape, from HIP events, --launch-repeats times each in
turn.  Synthetic weights: the runs time the work, they say nothing about image quality.  Prints one JSON line.
Usage: python benchmarks/threshold_step.py [--runs 3]"""
import argparse
import json
import math
import statistics

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=200)
    ap.add_argument("--launch-repeats", type=int, default=5)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import diffusion as dd
    from cgd_amd import sampler
    dev = steplib.DEV
    cfg, ctx, (unet, towers, _, guid, _) = steplib.setup()
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", "dpm20", False))
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}

    def launches():
        return steplib.launch_count(ctx)

    def run(mode):
        guid.diffusion = smp
        guid.current_timestep = smp.num_timesteps - 1
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
        gen = smp.dpmpp_sample_loop_progressive(unet, (1, 3, H, W), order=2, eta=0.0, **({"threshold": 0.995} if mode == "dpm20+thr" else {}), **kw)
        l0 = launches()
        t, n, out = steplib.drain(gen, guid)
        return t, n, bool(th.isfinite(out["sample"]).all()), launches() - l0

    modes = ["dpm20", "dpm20+thr"]
    res = steplib.alternate(modes, run, args.runs)
    times = {m: [v[0] for v in r] for m, r in res.items()}
    steps, finite, lcount = ({m: r[-1][j] for m, r in res.items()} for j in (1, 2, 3))

    tab = smp.tables
    fns = {}
    keep = []
    for n in (3 * 256 * 256, 3 * 512 * 512):
        for B in (1, 4):
            v = th.randn(B, n, device=dev)
            out3 = th.empty(B, 3, device=dev)
            scratch = th.empty(int(ctx.lib.cgd_abs_quantile_scratch_bytes(B, n)), dtype=th.uint8, device=dev)
            k, frac = tab.threshold_rank(0.995, n)
            keep.append((v, out3, scratch))

            def select(v=v, out3=out3, scratch=scratch, B=B, n=n, k=k, frac=frac):
                ctx.check(ctx.lib.cgd_op_abs_quantile(ctx.h, v.data_ptr(), B, n, k, frac, 1.0, math.inf, out3.data_ptr(), scratch.data_ptr(),
                                                      ctx.stream()))
            fns[f"abs_quantile_n{n}_B{B}"] = select

    x, x0, g, noise, hist = (th.randn(1, 3, H, W, device=dev) for _ in range(5))
    raw, x0c, sample, x0_out = (th.empty_like(x) for _ in range(4))
    scal, thr3 = th.ones(8, device=dev), th.empty(1, 3, device=dev)
    n = 3 * H * W
    scratch = th.empty(int(ctx.lib.cgd_abs_quantile_scratch_bytes(1, n)), dtype=th.uint8, device=dev)
    kc, d = tab.step_coef(10, 10), tab.dpmpp_coef(10, 2, 0.0)
    k, frac = tab.threshold_rank(0.995, n)

    def plain():
        ctx.check(ctx.lib.cgd_dpmpp_update(ctx.h, x.data_ptr(), x0.data_ptr(), g.data_ptr(), scal.data_ptr(), None, hist.data_ptr(),
                                           x0c.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, kc, d, ctx.stream()))

    def thresholded():
        ctx.check(ctx.lib.cgd_dpmpp_threshold(ctx.h, x.data_ptr(), x0.data_ptr(), g.data_ptr(), scal.data_ptr(), raw.data_ptr(), 1, H, W, kc, k,
                                              frac, 1.0, math.inf, thr3.data_ptr(), scratch.data_ptr(), ctx.stream()))
        ctx.check(ctx.lib.cgd_dpmpp_update_thr(ctx.h, x.data_ptr(), x0.data_ptr(), raw.data_ptr(), thr3.data_ptr(), None, hist.data_ptr(),
                                               x0c.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, kc, d, ctx.stream()))

    fns["cgd_dpmpp_update_2m_eta0"] = plain
    fns["cgd_dpmpp_threshold_plus_update_thr"] = thresholded
    l0 = launches()
    thresholded()
    thr_launches = launches() - l0
    call = steplib.per_launch(fns, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in times.items()}
    ms = {m: med[m] / steps[m] * 1e3 for m in modes}
    print(json.dumps({"what": "DPM-Solver++(2M) on 'dpm20' with and without threshold=0.995, bench.py config 2 (256x256, cutn 16, ViT-B/32, "
                              f"batch 1, synthetic weights), alternating, median of {args.runs} runs",
                      "s_per_run": {m: round(v, 4) for m, v in med.items()}, "runs_s": {m: [round(t, 4) for t in v] for m, v in times.items()},
                      "steps_yielded": steps, "finite": finite, "ms_per_step": {m: round(v, 4) for m, v in ms.items()},
                      "thr_over_plain": round(med["dpm20+thr"] / med["dpm20"], 5),
                      "launches_per_run": lcount, "added_launches_per_step": (lcount["dpm20+thr"] - lcount["dpm20"]) / steps["dpm20"],
                      "launches_of_threshold_plus_update_thr": thr_launches,
                      "call_us": {name: steplib.stats(v) for name, v in call.items()}, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
