"""Cost of ILVR at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights), in one process:

  launch    microseconds per cgd_ilvr_refine call (its two launches, sample and pred_xstart pair) for the factors 4, 8 and 32, next to
            cgd_masked_merge in the same run, from HIP events.  The refinement moves about seven plane sets of B * 3 * H * W floats (the
            down pass reads ref, noise, sample and ref, pred_xstart; the up pass reads and writes sample and pred_xstart), the merge about
            four: the merge is the yardstick of the launches.
  plain     the first --steps steps of p_sample_loop_progressive over the 250-step schedule from an init image
  ilvr8     the same with ilvr=(init image, 8): one cgd_ilvr_refine per step

The plain and ilvr8 runs alternate, --runs of each after one untimed warm-up run; wall clock around work that ends in a device
synchronise; launch counts from the library's counter.  Prints one JSON line.  Usage: python benchmarks/ilvr_step.py [--runs 5] [--steps 40]"""
import argparse
import json
import statistics

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--launch-iters", type=int, default=500)
    ap.add_argument("--launch-repeats", type=int, default=5)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import lib as L
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, _) = steplib.setup()
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    gen = th.Generator().manual_seed(5)
    init = th.tanh(th.randn(1, 3, H, W, generator=gen)).to(dev)

    def run(mode):
        guid.current_timestep = smp.num_timesteps - 1
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True,
                  init_image=init)
        if mode == "ilvr8":
            kw["ilvr"] = (init, 8)
        n0 = steplib.launch_count(ctx)
        t, n, out = steplib.drain(smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw), guid, steps=args.steps)
        return t / n, (steplib.launch_count(ctx) - n0) / n, bool(th.isfinite(out["sample"]).all())

    res = steplib.alternate(["plain", "ilvr8"], run, args.runs)
    ms = {m: [1e3 * v[0] for v in r] for m, r in res.items()}
    launches = {m: r[-1][1] for m, r in res.items()}
    finite = {m: all(v[2] for v in r) for m, r in res.items()}

    # per-call cost at the headline shape
    sample, x0, noise = (th.randn(1, 3, H, W, device=dev) for _ in range(3))
    mask = th.zeros(1, 1, H, W, device=dev)
    mask[..., W // 2:] = 1.0
    k = smp.tables.mask_coef(125)

    def merge():
        mk = smp.tables.mask_coef(125)
        mk.flags = L.MASK_PRED_XSTART | L.MASK_N_KNOWN
        ctx.check(ctx.lib.cgd_masked_merge(ctx.h, sample.data_ptr(), x0.data_ptr(), init.data_ptr(), mask.data_ptr(), noise.data_ptr(), None,
                                           None, 1, H, W, 1, 1, 1, mk, ctx.stream()))

    def refine(N, with_x0=True):
        scratch = th.empty(int(ctx.lib.cgd_ilvr_scratch_floats(1, H, W, N, 1)), device=dev)

        def fn():
            ctx.check(ctx.lib.cgd_ilvr_refine(ctx.h, sample.data_ptr(), x0.data_ptr() if with_x0 else None, init.data_ptr(), noise.data_ptr(),
                                              scratch.data_ptr(), 1, H, W, 1, N, k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev, ctx.stream()))
        return fn

    fns = {"cgd_masked_merge": merge}
    fns.update({f"cgd_ilvr_refine_N{N}": refine(N) for N in (4, 8, 32)})
    fns["cgd_ilvr_refine_N8_sample_only"] = refine(8, False)
    launch_us = steplib.per_launch(fns, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in ms.items()}
    print(json.dumps({"what": "milliseconds per guided p_sample step from an init image, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, "
                              f"synthetic weights, -respace 250), first {args.steps} steps, median of {args.runs} alternating runs",
                      "ms_per_step": {m: round(v, 3) for m, v in med.items()}, "runs_ms": {m: [round(t, 3) for t in v] for m, v in ms.items()},
                      "launches_per_step": launches, "finite": finite, "ilvr8_minus_plain_ms": round(med["ilvr8"] - med["plain"], 4),
                      "call_us": {n: steplib.stats(v) for n, v in launch_us.items()}, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
