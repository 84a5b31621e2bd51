"""Cost of masked sampling at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights), in one
process:

  launch      microseconds per launch of cgd_masked_merge (with and without the re-noise output) next to cgd_sample_update mode 0, from
              HIP events
  unmasked    p_sample_loop_progressive over the 250-step schedule from an init image (what `-respace 250 -init a.png` runs)
  masked      the same with a half-image mask (`-init a.png::m.png`): one more launch per evaluation
  resamples2  the masked run with resamples=2 (one run): every step index but the last evaluates twice

The unmasked and masked runs alternate, --runs of each after one untimed warm-up run; wall clock around work that ends in a device
synchronise.  Prints one JSON line.  Usage: python benchmarks/masked_step.py [--runs 3]"""
import argparse
import json
import statistics

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=500)
    ap.add_argument("--launch-repeats", type=int, default=5)
    ap.add_argument("--no-resamples", action="store_true", help="skip the resamples=2 run")
    args = ap.parse_args()
    import torch as th
    from cgd_amd import lib as L
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, _) = steplib.setup()
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    gen = th.Generator().manual_seed(5)
    init = th.tanh(th.randn(1, 3, H, W, generator=gen)).to(dev)
    mask = th.zeros(1, 1, H, W, device=dev)
    mask[..., W // 2:] = 1.0

    def run(mode):
        guid.current_timestep = smp.num_timesteps - 1
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True,
                  init_image=init)
        if mode != "unmasked":
            kw["mask"] = mask
        if mode == "resamples2":
            kw["resamples"] = 2
        it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw)
        t, n, out = steplib.drain(it, guid)
        kept = bool(th.equal(out["pred_xstart"][..., :W // 2], init[..., :W // 2]))
        return t, n, bool(th.isfinite(out["sample"]).all()), kept

    modes = ["unmasked", "masked"]
    res = steplib.alternate(modes, run, args.runs)
    times = {m: [v[0] for v in r] for m, r in res.items()}
    steps, finite, kept = ({m: r[-1][j] for m, r in res.items()} for j in (1, 2, 3))
    if not args.no_resamples:
        th.manual_seed(2000)
        t, n, ok, kp = run("resamples2")
        times["resamples2"], steps["resamples2"], finite["resamples2"], kept["resamples2"] = [t], n, ok, kp

    # per-launch cost at the headline shape
    x, x0, mean, g, noise, n_re = (th.randn(1, 3, H, W, device=dev) for _ in range(6))
    logvar = th.randn_like(x) * 0.1 - 5
    sample, x0_out, x_re = th.empty_like(x), th.empty_like(x), th.empty_like(x)
    scal = th.ones(8, device=dev)
    k = smp.tables.step_coef(125, 125)

    def sample_update():
        ctx.check(ctx.lib.cgd_sample_update(ctx.h, x.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), g.data_ptr(),
                                            noise.data_ptr(), scal.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), 1, H, W, k, 0,
                                            ctx.stream()))

    def merge(renoise):
        mk = smp.tables.mask_coef(125)
        mk.flags = L.MASK_PRED_XSTART | L.MASK_N_KNOWN | (L.MASK_RENOISE if renoise else 0)

        def fn():
            ctx.check(ctx.lib.cgd_masked_merge(ctx.h, sample.data_ptr(), x0_out.data_ptr(), init.data_ptr(), mask.data_ptr(),
                                               noise.data_ptr(), n_re.data_ptr() if renoise else None,
                                               x_re.data_ptr() if renoise else None, 1, H, W, 1, 1, 1, mk, ctx.stream()))
        return fn

    sample.copy_(x)
    x0_out.copy_(x0)
    launch_us = steplib.per_launch({"cgd_sample_update_mode0": sample_update, "cgd_masked_merge": merge(False),
                                    "cgd_masked_merge_renoise": merge(True)}, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in times.items()}
    print(json.dumps({"what": "seconds per full guided p_sample run from an init image, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, "
                              f"synthetic weights, -respace 250), median of {args.runs} alternating runs (resamples2: one run)",
                      "s_per_run": {m: round(v, 3) for m, v in med.items()}, "runs_s": {m: [round(t, 3) for t in v] for m, v in times.items()},
                      "steps_yielded": steps, "finite": finite, "kept_half_is_init": kept,
                      "masked_over_unmasked": round(med["masked"] / med["unmasked"], 4),
                      "launch_us": {n: steplib.stats(v) for n, v in launch_us.items()}, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
