"""Cost of a guided step with a direction prompt ('SOURCE=>TARGET', the directional CLIP loss of csrc/direction.hip) at the headline shape
(bench.py config 2's networks: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights, respace 250, p_sample), in one process:

  plain_ms        milliseconds per guided step without a direction prompt (the path of a run that does not ask for one)
  direction_ms    the same loop with one direction prompt beside the target prompt: the source image's cutouts and one more tower forward
                  of cutn images per step, and the loss launch
  cached_ms       the same with cached_cutouts: the boxes never change, so the source embeddings are computed on the first step only
                  (the plain path with cached_cutouts is timed beside it: cached boxes change the plain step too)
  loss_us         cgd_directional_loss alone at (cutn 16, B 1, P 1, D 512), from HIP events around --iters back-to-back calls, with
                  cgd_spherical_loss at the same shape beside it
  launches        kernel launches per guided step of every path

Every figure is the median of --repeats measurements (the paths taken alternately, after one untimed warm-up each) with their minimum and
maximum beside it.  Prints one JSON line.  Usage: python benchmarks/direction_step.py [--repeats 5] [--steps 40]"""
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
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup()
    H, W = cfg["hw"]
    gen = th.Generator().manual_seed(98)
    dirs = [th.randn(1, t.out_dim, generator=gen).to(dev) for t in towers]
    source = th.tanh(th.randn(1, 3, H, W, generator=gen)).to(dev)
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    start = cfg["start"]
    skip = smp.num_timesteps - 1 - start

    def make(direction, cached):
        kw = dict(direction_embeds=dirs, direction_weights=[1.0], direction_source=source) if direction else {}
        c = dg.ClipGuidance(ctx, unet, towers, smp, guid.targets_list, guid.weights, cfg["cutn"], clip_guidance_scale=1000.0, tv_scale=150.0,
                            range_scale=50.0, cached_cutouts=cached, **kw)
        if cached:
            th.manual_seed(7)
            c.make_cutouts.cache_coordinates(H, W)
        return c

    conds = {"plain": guid, "direction": make(True, False), "plain_cached": make(False, True), "direction_cached": make(True, True)}
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

    cutn, B, P, D = cfg["cutn"], 1, 1, towers[0].out_dim
    g = th.Generator(device=dev).manual_seed(5)
    emb, src = (th.randn(cutn * B, D, device=dev, generator=g) for _ in range(2))
    d_n = th.nn.functional.normalize(th.randn(P, D, device=dev, generator=g), dim=-1)
    w = th.ones(B, P, device=dev)
    demb, part = th.empty(cutn * B, D, device=dev), th.empty(cutn * B, device=dev)
    lib, s = ctx.lib, ctx.stream()

    def directional():
        ctx.check(lib.cgd_directional_loss(ctx.h, emb.data_ptr(), src.data_ptr(), d_n.data_ptr(), w.data_ptr(), demb.data_ptr(), part.data_ptr(),
                                           cutn, B, 1, P, D, 1000.0, 0, s))

    def spherical():
        ctx.check(lib.cgd_spherical_loss(ctx.h, emb.data_ptr(), d_n.data_ptr(), w.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B, P, D,
                                         1000.0, s))

    loss = steplib.per_launch({"cgd_directional_loss": directional, "cgd_spherical_loss": spherical}, args.iters, args.repeats)
    stat = steplib.stats
    print(json.dumps({"what": "guided step with / without one direction prompt at 256x256, cutn 16, batch 1, synthetic weights, bench.py config 2's "
                              f"networks; median / min / max of {args.repeats} alternating repeats of {args.steps} steps",
                      "ms_per_step": {n: stat(v, 3) for n, v in ms.items()},
                      "loss_us (back-to-back calls)": {n: stat(v, 1) for n, v in loss.items()},
                      "launches_per_step": per_step, "finite": finite, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
