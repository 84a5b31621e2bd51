"""Cost of a guided step with region prompts ('TEXT@@REGION', the `_regions` loss entries of csrc/guidance.hip and csrc/direction.hip) at the
headline shape (bench.py config 2's networks: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights, respace 250, p_sample), in one
process:

  plain_ms        milliseconds per guided step with two prompts that act on the whole frame
  regions_ms      the same loop with the same two prompts confined to the left and the right half of the frame ('0,0,0.5,1' and '0.5,0,1,1'):
                  the same launches through the other loss entry, which reads four table entries per prompt and row
  launches        kernel launches per guided step of both paths; they must be equal (the script fails otherwise)
  loss_us         each `_regions` launch alone against its plain entry at (cutn 16, B 1, P 1, D 512), from HIP events around --iters
                  back-to-back calls, and cgd_op_region_coverage beside them

Every figure is the median of --repeats measurements (the paths taken alternately, after one untimed warm-up each) with their minimum and
maximum beside it.  Prints one JSON line.  Usage: python benchmarks/region_step.py [--repeats 5] [--steps 40]"""
import argparse
import json

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import guidance as dg
    from cgd_amd import regions
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup()
    H, W = cfg["hw"]
    gen = th.Generator().manual_seed(99)
    targets = [th.randn(2, t.out_dim, generator=gen).to(dev) for t in towers]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    start = cfg["start"]
    skip = smp.num_timesteps - 1 - start
    plan = regions.plan_from_specs([("0,0,0.5,1", 1.0), ("0.5,0,1,1", 1.0)], H, W, dev)

    def make(with_regions):
        return dg.ClipGuidance(ctx, unet, towers, smp, targets, [0.5, 0.5], cfg["cutn"], clip_guidance_scale=1000.0, tv_scale=150.0,
                               range_scale=50.0, regions=plan if with_regions else None)

    conds = {"plain": make(False), "regions": make(True)}
    per_step, finite = {}, {}

    def guided(name):
        cond = conds[name]
        cond.current_timestep = start
        it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=cond, model_kwargs=dict(y), device=dev,
                                           skip_timesteps=skip, init_image=image, randomize_class=False, cond_fn_with_grad=True)
        n0 = steplib.launch_count(ctx)
        t, n, out = steplib.drain(it, cond, args.steps)
        per_step[name], finite[name] = (steplib.launch_count(ctx) - n0) / n, bool(th.isfinite(out["sample"]).all())
        return t / n * 1e3

    ms = steplib.alternate(list(conds), guided, args.repeats)
    if per_step["plain"] != per_step["regions"]:
        raise SystemExit(f"launches per step differ: {per_step}")

    cutn, B, P, D = cfg["cutn"], 1, 1, towers[0].out_dim
    g = th.Generator(device=dev).manual_seed(5)
    emb, src = (th.randn(cutn * B, D, device=dev, generator=g) for _ in range(2))
    d_n = th.nn.functional.normalize(th.randn(P, D, device=dev, generator=g), dim=-1)
    w = th.ones(B, P, device=dev)
    demb, part, cov = th.empty(cutn * B, D, device=dev), th.empty(cutn * B, device=dev), th.empty(cutn, P, device=dev)
    th.manual_seed(11)
    geo = th.tensor(dg.crop_geometry(dg.generate_coords(H, W, cutn, towers[0].input_resolution, 1.0), H, W), dtype=th.int32, device=dev)
    one = plan.columns([0])
    lib, s = ctx.lib, ctx.stream()
    e, sp, dn, wp, de, pa = (t.data_ptr() for t in (emb, src, d_n, w, demb, part))

    def directional():
        ctx.check(lib.cgd_directional_loss(ctx.h, e, sp, dn, wp, de, pa, cutn, B, 1, P, D, 1000.0, 0, s))

    def directional_regions():
        ctx.check(lib.cgd_directional_loss_regions(ctx.h, e, sp, dn, wp, de, pa, cutn, B, 1, P, D, 1000.0, 0, *one.args(geo), s))

    def spherical():
        ctx.check(lib.cgd_spherical_loss(ctx.h, e, dn, wp, de, pa, cutn, B, P, D, 1000.0, s))

    def spherical_regions():
        ctx.check(lib.cgd_spherical_loss_regions(ctx.h, e, dn, wp, de, pa, cutn, B, P, D, 1000.0, *one.args(geo), s))

    def coverage():
        a = one.args(geo)
        ctx.check(lib.cgd_op_region_coverage(ctx.h, *a[:5], cov.data_ptr(), cutn, P, *a[5:], s))

    loss = steplib.per_launch({"cgd_spherical_loss": spherical, "cgd_spherical_loss_regions": spherical_regions,
                               "cgd_directional_loss": directional, "cgd_directional_loss_regions": directional_regions,
                               "cgd_op_region_coverage": coverage}, args.iters, args.repeats)
    stat = steplib.stats
    med = {n: stat(v, 3) for n, v in ms.items()}
    spread = max(v["max"] - v["min"] for v in med.values())
    print(json.dumps({"what": "guided step with two prompts, on the whole frame / on the left and right half, at 256x256, cutn 16, batch 1, "
                              f"synthetic weights, bench.py config 2's networks; median / min / max of {args.repeats} alternating repeats of "
                              f"{args.steps} steps",
                      "ms_per_step": med,
                      "regions_minus_plain_ms": round(med["regions"]["median"] - med["plain"]["median"], 3), "spread_of_the_repeats_ms": round(spread, 3),
                      "loss_us (back-to-back calls)": {n: stat(v, 1) for n, v in loss.items()},
                      "launches_per_step": per_step, "finite": finite, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
