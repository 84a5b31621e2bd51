"""Cost of the resized cutouts (`cuts=4:12`) per guided step at the headline shape (bench.py config 2: 256x256, CLIP ViT-B/32, batch 1,
respace 250, p_sample, synthetic weights), in one process with one seed:

  resized   ClipGuidance._clip_leg with MakeCutoutsResized(224, overview=4, inner=12) (the cutresize kernels), 16 cuts
  pooled    the plain guided step with 16 pooled cutouts (the default path, unchanged)

The two modes alternate in rounds of --steps timed steps (after --warmup steps each), wall clock around work that ends in a device
synchronise.  Then the microseconds per launch of cgd_cutouts_resize_fwd / _bwd and of cgd_cutouts_aug_fwd / _bwd at the same shape
(16 cuts of a 256x256 image into ViT-B/32 patch rows), from HIP events.
Prints one JSON line.  Usage: python benchmarks/resize_cutouts_step.py [--steps 40] [--warmup 5] [--rounds 3]"""
import argparse
import json
import statistics
import time

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=200)
    ap.add_argument("--launch-repeats", type=int, default=5)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import guidance as dg
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, x0_star) = steplib.setup()
    H, W = cfg["hw"]
    N, start = smp.num_timesteps, cfg["start"]
    pooled_mk = guid.make_cutouts
    resized_mk = dg.MakeCutoutsResized(towers[0].input_resolution, overview=4, inner=12, ctx=ctx)

    def trajectory():
        while True:
            gen = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=guid,
                                                model_kwargs={"y": th.zeros(1, dtype=th.long, device=dev)}, device=dev,
                                                skip_timesteps=N - 1 - start, init_image=x0_star, randomize_class=True, cond_fn_with_grad=True)
            guid.current_timestep = start
            for out in gen:
                guid.current_timestep -= 1
                yield out

    modes = {"resized": resized_mk, "pooled": pooled_mk}
    th.manual_seed(1000)
    steps = trajectory()
    times = {m: [] for m in modes}
    for r in range(args.rounds):
        for mode, mk in modes.items():
            guid.make_cutouts = mk
            for _ in range(args.warmup):
                next(steps)
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = next(steps)
            th.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) / args.steps * 1e3)
            assert bool(th.isfinite(out["sample"]).all()), mode
    guid.make_cutouts = pooled_mk

    # per-launch cost at the headline cutout shape: ViT-B/32 patch rows, 16 cuts of a 256x256 image
    cs, patch, cutn, B = 224, 32, 16, 1
    x = th.tanh(th.randn(B, 3, H, W, device=dev))
    th.manual_seed(3)
    recs = resized_mk.draw(W, H)
    table = th.tensor(dg.resize_table(recs, H, W), dtype=th.int32, device=dev)
    clip_in = th.empty(cutn * B * (cs // patch) ** 2, 3 * patch * patch, device=dev)
    g = th.empty_like(x)
    rs_scratch = th.empty(ctx.lib.cgd_cutouts_resize_scratch_floats(B, H, W, cutn), device=dev)
    coords = dg.generate_coords(H, W, cutn, cs, 1.0)
    aug = dg._AugLaunch(ctx.lib, coords, B, H, W, x.device)
    noise = th.randn(sum(4 * 3 * B * h * w for _, _, h, w in aug.geo_list), device=dev) * dg.AUG_NOISE_STD
    offs, o = [], 0
    for _, _, h, w in aug.geo_list:
        offs.append(o)
        o += 4 * 3 * B * h * w
    off = th.tensor(offs, dtype=th.int64, device=dev)
    aug_scratch = th.empty(ctx.lib.cgd_cutouts_aug_scratch_floats(B, H, W, cutn), device=dev)

    def rs_fwd():
        ctx.check(ctx.lib.cgd_cutouts_resize_fwd(ctx.h, x.data_ptr(), table.data_ptr(), table.data_ptr() + 16 * cutn, clip_in.data_ptr(), B, H,
                                                 W, cutn, cs, 1, patch, ctx.stream()))

    def rs_bwd():
        ctx.check(ctx.lib.cgd_cutouts_resize_bwd(ctx.h, clip_in.data_ptr(), table.data_ptr(), table.data_ptr() + 16 * cutn, g.data_ptr(),
                                                 rs_scratch.data_ptr(), B, H, W, cutn, cs, 1, patch, 0, ctx.stream()))

    def aug_fwd():
        ctx.check(ctx.lib.cgd_cutouts_aug_fwd(ctx.h, x.data_ptr(), aug.geo.data_ptr(), aug.params.data_ptr(), noise.data_ptr(), off.data_ptr(),
                                              clip_in.data_ptr(), B, H, W, cutn, cs, 1, patch, ctx.stream()))

    def aug_bwd():
        ctx.check(ctx.lib.cgd_cutouts_aug_bwd(ctx.h, clip_in.data_ptr(), aug.geo.data_ptr(), aug.params.data_ptr(), g.data_ptr(),
                                              aug_scratch.data_ptr(), B, H, W, cutn, cs, 1, patch, 0, ctx.stream()))

    us = steplib.per_launch({"cutouts_resize_fwd_us": rs_fwd, "cutouts_resize_bwd_us": rs_bwd, "cutouts_aug_fwd_us": aug_fwd,
                             "cutouts_aug_bwd_us": aug_bwd}, args.launch_iters, args.launch_repeats)
    launches = {name: steplib.stats(v) for name, v in us.items()}
    med = {m: statistics.median(v) for m, v in times.items()}
    print(json.dumps({"what": "ms per guided step, bench.py config 2 (256x256, 16 cuts, ViT-B/32, batch 1, respace 250, p_sample), "
                              f"median of {args.rounds} rounds x {args.steps} steps",
                      "ms_per_step": {m: round(v, 3) for m, v in med.items()},
                      "rounds_ms": {m: [round(t, 3) for t in v] for m, v in times.items()},
                      "resized_over_pooled_ms": round(med["resized"] - med["pooled"], 3),
                      **launches, "inner_sizes": sorted(r[2] for r in recs[4:]), "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
