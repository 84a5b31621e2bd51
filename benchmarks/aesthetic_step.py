"""Cost of a guided step with an aesthetic head ('A+aesthetic=FILE:SCALE', the aesthetic-predictor loss of csrc/aesthetic.hip) at the headline
shape (bench.py config 2's networks: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights, respace 250, p_sample), in one process:

  plain_ms        milliseconds per guided step without a head (the path of a run that does not ask for one)
  aesthetic_ms    the same loop with a seeded head on the tower beside the target prompt: one more launch per step
  loss_us         cgd_aesthetic_loss alone at (cutn 16, B 1) and D = 512 / 768 / 1024, from HIP events around --iters back-to-back calls, with
                  cgd_spherical_loss (P 1) at the same shapes beside it
  launches        kernel launches per guided step of both paths (expected: +1 per tower with a head)

Every figure is the median of --repeats measurements (the paths taken alternately, after one untimed warm-up each) with their minimum and
maximum beside it.  Prints one JSON line.  Usage: python benchmarks/aesthetic_step.py [--repeats 5] [--steps 40]"""
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
    from cgd_amd import nets, synthetic
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup()
    H, W = cfg["hw"]
    heads = [nets.AestheticHead(t.out_dim, dev).load_state_dict(synthetic.aesthetic_head(t.out_dim)) for t in towers]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    start = cfg["start"]
    skip = smp.num_timesteps - 1 - start
    with_head = dg.ClipGuidance(ctx, unet, towers, smp, guid.targets_list, guid.weights, cfg["cutn"], clip_guidance_scale=1000.0, tv_scale=150.0,
                                range_scale=50.0, aesthetic_heads=heads, aesthetic_scale=300.0)
    conds = {"plain": guid, "aesthetic": with_head}
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
    log = with_head.log()

    cutn, B, P = cfg["cutn"], 1, 1
    lib, s = ctx.lib, ctx.stream()
    g = th.Generator(device=dev).manual_seed(5)
    fns, keep = {}, []
    for D in (512, 768, 1024):
        emb = th.randn(cutn * B, D, device=dev, generator=g)
        head = synthetic.aesthetic_head(D)["head"].to(dev)
        tgt = th.nn.functional.normalize(th.randn(P, D, device=dev, generator=g), dim=-1)
        w = th.ones(B, P, device=dev)
        demb, part, score = th.empty(cutn * B, D, device=dev), th.empty(cutn * B, device=dev), th.empty(cutn * B, device=dev)
        keep.append((emb, head, tgt, w, demb, part, score))

        def aesthetic(emb=emb, head=head, demb=demb, part=part, score=score, D=D):
            ctx.check(lib.cgd_aesthetic_loss(ctx.h, emb.data_ptr(), head.data_ptr(), demb.data_ptr(), part.data_ptr(), score.data_ptr(), cutn, B, D,
                                             300.0, 0, s))

        def spherical(emb=emb, tgt=tgt, w=w, demb=demb, part=part, D=D):
            ctx.check(lib.cgd_spherical_loss(ctx.h, emb.data_ptr(), tgt.data_ptr(), w.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B, P, D,
                                             1000.0, s))

        fns[f"cgd_aesthetic_loss D={D}"], fns[f"cgd_spherical_loss D={D}"] = aesthetic, spherical
    loss = steplib.per_launch(fns, args.iters, args.repeats)
    stat = steplib.stats
    print(json.dumps({"what": "guided step with / without an aesthetic head at 256x256, cutn 16, batch 1, synthetic weights, bench.py config 2's "
                              f"networks; median / min / max of {args.repeats} alternating repeats of {args.steps} steps",
                      "ms_per_step": {n: stat(v, 3) for n, v in ms.items()},
                      "loss_us (back-to-back calls)": {n: stat(v, 1) for n, v in loss.items()},
                      "launches_per_step": per_step, "finite": finite,
                      "last step's log": {k: round(v, 4) for k, v in log.items() if k.startswith(("CLIP", "Aesthetic"))},
                      "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
