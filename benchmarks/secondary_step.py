"""Cost of a guided step with and without the secondary model at the headline shape (bench.py config 2's networks: 256x256, cutn 16, CLIP
ViT-B/32, batch 1, synthetic weights, respace 250, p_sample), in one process:

  plain_ms       milliseconds per guided step, the guidance gradient through the UNet's backward pass (the path of a run without `secondary=`)
  secondary_ms   the same loop with the secondary model: no UNet backward pass
  trunk_us       the secondary net alone, from HIP events around --trunk-iters back-to-back calls: forward (pack, 23 ConvBlocks, head) and dgrad
  launches       kernel launches per guided step of the two paths

Every figure is the median of --repeats measurements (the two paths taken alternately, after one untimed warm-up each) with their minimum and
maximum beside it.  Prints one JSON line.  Usage: python benchmarks/secondary_step.py [--repeats 5] [--steps 40]"""
import argparse
import json

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--trunk-iters", type=int, default=20)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import nets, synthetic
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup()
    sec = nets.SecondaryModel(ctx).load_state_dict(synthetic.secondary_state_dict(device=dev))
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    start = cfg["start"]
    skip = smp.num_timesteps - 1 - start

    def guided(secondary):
        guid.secondary = secondary
        guid.current_timestep = start
        th.manual_seed(1000)
        it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev,
                                           skip_timesteps=skip, init_image=image, randomize_class=False, cond_fn_with_grad=True)
        n0 = steplib.launch_count(ctx)
        t, n, out = steplib.drain(it, guid, args.steps)
        return t / n * 1e3, (steplib.launch_count(ctx) - n0) / n, bool(th.isfinite(out["sample"]).all())

    guided(None)
    guided(sec)
    ms = {"plain": [], "secondary": []}
    per_step, finite = {}, {}
    for _ in range(args.repeats):
        for name, net in (("plain", None), ("secondary", sec)):
            t, per_step[name], finite[name] = guided(net)
            ms[name].append(t)
    guid.secondary = None

    x = th.randn(1, 3, H, W, device=dev)
    tt = th.full((1,), 0.5, device=dev)
    dv = th.randn(1, 3, H, W, device=dev)
    pred, dx = th.empty_like(x), th.empty_like(x)

    fns = {"forward": lambda: sec.forward(x, tt, pred=pred), "dgrad": lambda: sec.dgrad(dv, dx)}
    trunk = steplib.per_launch(fns, args.trunk_iters, args.repeats)
    stat = steplib.stats

    print(json.dumps({"what": "guided step with / without the secondary model at 256x256, batch 1, synthetic weights, bench.py config 2's networks; "
                              f"median / min / max of {args.repeats} alternating repeats of {args.steps} steps",
                      "plain_ms_per_step": stat(ms["plain"], 3), "secondary_ms_per_step": stat(ms["secondary"], 3),
                      "trunk_us": {n: stat(v, 1) for n, v in trunk.items()}, "launches_per_step": per_step, "finite": finite,
                      "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
