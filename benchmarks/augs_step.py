"""Cost of `use_augs=True` per guided step at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP ViT-B/32, batch 1,
respace 250, p_sample, synthetic weights), in one process with one seed:

  augs-native  ClipGuidance._clip_leg with use_augs cutouts (the cutaug kernels)
  augs-torch   the same leg through _clip_leg_torch (crop / augment / pool in torch ops with autograd)
  augs-off     the plain guided step (the floor)

The three modes alternate in rounds of --steps timed steps (after --warmup steps each), wall clock around work that ends in a device
synchronise.  Then the microseconds per launch of cgd_cutouts_aug_fwd / _bwd at the headline cutout shape, from HIP events.
Prints one JSON line.  Usage: python benchmarks/augs_step.py [--steps 40] [--warmup 5] [--rounds 3]"""
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
    plain_mk = guid.make_cutouts
    aug_mk = dg.MakeCutouts(towers[0].input_resolution, cfg["cutn"], use_augs=True, ctx=ctx)

    def trajectory():
        while True:
            gen = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=guid,
                                                model_kwargs={"y": th.zeros(1, dtype=th.long, device=dev)}, device=dev,
                                                skip_timesteps=N - 1 - start, init_image=x0_star, randomize_class=True, cond_fn_with_grad=True)
            guid.current_timestep = start
            for out in gen:
                guid.current_timestep -= 1
                yield out

    def set_mode(mode):
        guid.make_cutouts = plain_mk if mode == "augs-off" else aug_mk
        if mode == "augs-torch":
            guid._clip_leg = guid._clip_leg_torch
        else:
            guid.__dict__.pop("_clip_leg", None)

    modes = ["augs-native", "augs-torch", "augs-off"]
    th.manual_seed(1000)
    steps = trajectory()
    times = {m: [] for m in modes}
    for r in range(args.rounds):
        for mode in modes:
            set_mode(mode)
            for _ in range(args.warmup):
                next(steps)
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = next(steps)
            th.cuda.synchronize()
            times[mode].append((time.perf_counter() - t0) / args.steps * 1e3)
            assert bool(th.isfinite(out["sample"]).all()), mode
    set_mode("augs-native")

    # per-launch cost of the kernels at the headline cutout shape (ViT-B/32 patch rows, noise on, 16 crops of a 256x256 image)
    cs, patch, cutn, B = 224, 32, cfg["cutn"], 1
    x = th.tanh(th.randn(B, 3, H, W, device=dev))
    th.manual_seed(3)
    coords = dg.generate_coords(H, W, cutn, cs, 1.0)
    aug = dg._AugLaunch(ctx.lib, coords, B, H, W, x.device)
    clip_in = th.empty(cutn * B * (cs // patch) ** 2, 3 * patch * patch, device=dev)
    aug.forward(ctx, x, clip_in, cs, 1, patch)  # draws this launch's noise once; the timed launches reuse the last group's inputs
    noise = th.randn(sum(4 * 3 * B * h * w for _, _, h, w in aug.geo_list), device=dev) * dg.AUG_NOISE_STD
    offs, o = [], 0
    for _, _, h, w in aug.geo_list:
        offs.append(o)
        o += 4 * 3 * B * h * w
    off = th.tensor(offs, dtype=th.int64, device=dev)
    g = th.empty_like(x)
    scratch = th.empty(ctx.lib.cgd_cutouts_aug_scratch_floats(B, H, W, cutn), device=dev)

    def fwd():
        ctx.check(ctx.lib.cgd_cutouts_aug_fwd(ctx.h, x.data_ptr(), aug.geo.data_ptr(), aug.params.data_ptr(), noise.data_ptr(), off.data_ptr(),
                                              clip_in.data_ptr(), B, H, W, cutn, cs, 1, patch, ctx.stream()))

    def bwd():
        ctx.check(ctx.lib.cgd_cutouts_aug_bwd(ctx.h, clip_in.data_ptr(), aug.geo.data_ptr(), aug.params.data_ptr(), g.data_ptr(),
                                              scratch.data_ptr(), B, H, W, cutn, cs, 1, patch, 0, ctx.stream()))

    us = steplib.per_launch({"fwd": fwd, "bwd": bwd}, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in times.items()}
    print(json.dumps({"what": "ms per guided step, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, respace 250, p_sample), "
                              f"median of {args.rounds} rounds x {args.steps} steps",
                      "ms_per_step": {m: round(v, 3) for m, v in med.items()},
                      "rounds_ms": {m: [round(t, 3) for t in v] for m, v in times.items()},
                      "augs_native_over_off_ms": round(med["augs-native"] - med["augs-off"], 3),
                      "augs_torch_over_off_ms": round(med["augs-torch"] - med["augs-off"], 3),
                      "cutouts_aug_fwd_us": steplib.stats(us["fwd"]), "cutouts_aug_bwd_us": steplib.stats(us["bwd"]),
                      "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
