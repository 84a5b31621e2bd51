"""Cost of windowed sampling (nets.WindowedUNet, '+windows=') on a 256x512 frame with the networks of bench.py config 2 (256x256 UNet, cutn 16,
CLIP ViT-B/32, batch 1, synthetic weights), in one process:

  whole     the first --steps steps of p_sample_loop_progressive over the 250-step schedule, the whole frame through the UNet in one
            forward (what --width_offset 256 alone does)
  windows   the same frame with the UNet wrapped at stride 128: three 256x256 windows per evaluation, one batched forward / dgrad
  launch    microseconds per cgd_window_gather / cgd_window_merge call for that plan at C = 3 and C = 6, with and without the weight tables,
            next to the same data movement in torch (slicing + cat for the gather, zeros + index_add_ along W for the merge), from HIP events

The whole and windows runs alternate, --runs of each after one untimed warm-up run; wall clock around work that ends in a device
synchronise; launch counts from the library's counter.  Prints one JSON line.  Usage: python benchmarks/window_step.py [--runs 5] [--steps 20]"""
import argparse
import json
import statistics

import steplib

HW, STRIDE = (256, 512), 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--launch-iters", type=int, default=500)
    ap.add_argument("--launch-repeats", type=int, default=5)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import guidance as dg
    from cgd_amd import nets
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, _) = steplib.setup(hw=HW)
    H, W = HW
    wunet = nets.WindowedUNet(unet, STRIDE)
    gen = th.Generator().manual_seed(99)
    targets = [th.randn(cfg["P"], t.out_dim, generator=gen).to(dev) for t in towers]
    guid_w = dg.ClipGuidance(ctx, wunet, towers, smp, targets, th.ones(cfg["P"]) / cfg["P"], cfg["cutn"], clip_guidance_scale=1000.0, tv_scale=150.0,
                             range_scale=50.0)
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}

    def run(mode):
        model, cond = (wunet, guid_w) if mode == "windows" else (unet, guid)
        cond.current_timestep = smp.num_timesteps - 1
        kw = dict(clip_denoised=False, cond_fn=cond, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
        n0 = steplib.launch_count(ctx)
        t, n, out = steplib.drain(smp.p_sample_loop_progressive(model, (1, 3, H, W), **kw), cond, steps=args.steps)
        return t / n, (steplib.launch_count(ctx) - n0) / n, bool(th.isfinite(out["sample"]).all())

    res = steplib.alternate(["whole", "windows"], run, args.runs)
    ms = {m: [1e3 * v[0] for v in r] for m, r in res.items()}
    launches = {m: r[-1][1] for m, r in res.items()}
    finite = {m: all(v[2] for v in r) for m, r in res.items()}

    # the two kernels alone, for the plan of the runs above
    p = wunet.plan(H, W)
    S, n = p.S, p.n
    fns = {}
    for Cn in (3, 6):
        full, win = th.randn(1, Cn, H, W, device=dev), th.randn(n, Cn, S, S, device=dev)
        cols = th.cat([o + th.arange(S, device=dev) for o in p.ox])

        def gather(weighted, full=full, win=win, Cn=Cn):
            return lambda: wunet._gather(p, full, win, weighted)

        def merge(weighted, full=full, win=win, Cn=Cn):
            return lambda: wunet._merge(p, win, full, weighted)

        def torch_gather(full=full):
            return lambda: th.cat([full[..., o:o + S] for o in p.ox])

        def torch_merge(win=win, Cn=Cn, cols=cols):
            # (n, C, S, S) -> (1, C, H, n * S), added into the frame's columns: what the unweighted merge computes (ny = 1 in this plan)
            return lambda: th.zeros(1, Cn, H, W, device=dev).index_add_(3, cols, win.permute(1, 2, 0, 3).reshape(1, Cn, S, n * S))

        fns.update({f"cgd_window_gather_C{Cn}": gather(False), f"cgd_window_gather_C{Cn}_weighted": gather(True),
                    f"cgd_window_merge_C{Cn}": merge(False), f"cgd_window_merge_C{Cn}_weighted": merge(True),
                    f"torch_slices_cat_C{Cn}": torch_gather(), f"torch_index_add_C{Cn}": torch_merge()})
    assert p.ny == 1
    launch_us = steplib.per_launch(fns, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in ms.items()}
    print(json.dumps({"what": f"milliseconds per guided p_sample step on a {H}x{W} frame, networks of bench.py config 2 (256x256 UNet, cutn 16, "
                              f"ViT-B/32, batch 1, synthetic weights, -respace 250), first {args.steps} steps, median of {args.runs} alternating "
                              f"runs; windows: stride {STRIDE}, {n} windows",
                      "ms_per_step": {m: round(v, 3) for m, v in med.items()}, "runs_ms": {m: [round(t, 3) for t in v] for m, v in ms.items()},
                      "launches_per_step": launches, "finite": finite, "windows_over_whole": round(med["windows"] / med["whole"], 4),
                      "call_us": {k: steplib.stats(v) for k, v in launch_us.items()}, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
