"""Cost of a guided step with and without classifier guidance at the headline shape (bench.py config 2's networks: 256x256, cutn 16, CLIP
ViT-B/32, batch 1, synthetic weights, respace 250, p_sample; the 256x256 noisy classifier, synthetic weights), in one process:

  plain_ms        milliseconds per guided step without a classifier (the path of a run without `classifier=`)
  classifier_ms   the same loop with the classifier term: one classifier forward and one backward-to-input more per step
  net_us          the classifier alone, from HIP events around --net-iters back-to-back calls: forward and dgrad
  head_us         its head alone (AttentionPool2d + log-softmax-select at C = 512, S = 8, 1000 classes): forward and backward
  launches        kernel launches per guided step of the two paths

Every figure is the median of --repeats measurements (the two paths taken alternately, after one untimed warm-up each) with their minimum and
maximum beside it.  Prints one JSON line.  Usage: python benchmarks/classifier_step.py [--repeats 5] [--steps 40]"""
import argparse
import json

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--net-iters", type=int, default=20)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import nets, synthetic
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup()
    H, W = cfg["hw"]
    cls = nets.NoisyClassifier(ctx, **nets.CLASSIFIER_CONFIGS[H])
    cls.load_state_dict(synthetic.classifier_state_dict(cls.cfg, device=dev))
    y = {"y": th.full((1,), 207, dtype=th.long, device=dev)}
    start = cfg["start"]
    skip = smp.num_timesteps - 1 - start
    guid.classifier_scale, guid.classifier_class = 1.0, 207

    def guided(classifier):
        guid.classifier = classifier
        guid.current_timestep = start
        th.manual_seed(1000)
        it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev,
                                           skip_timesteps=skip, init_image=image, randomize_class=False, cond_fn_with_grad=True)
        n0 = steplib.launch_count(ctx)
        t, n, out = steplib.drain(it, guid, args.steps)
        return t / n * 1e3, (steplib.launch_count(ctx) - n0) / n, bool(th.isfinite(out["sample"]).all())

    guided(None)
    guided(cls)
    ms = {"plain": [], "classifier": []}
    per_step, finite = {}, {}
    for _ in range(args.repeats):
        for name, net in (("plain", None), ("classifier", cls)):
            t, per_step[name], finite[name] = guided(net)
            ms[name].append(t)
    guid.classifier = None

    x = th.randn(1, 3, H, W, device=dev)
    tt = th.full((1,), 417.0, device=dev)
    yy = y["y"]
    logits, logp, dx = th.empty(1, cls.out_channels, device=dev), th.empty(1, device=dev), th.empty_like(x)
    net = steplib.per_launch({"forward": lambda: cls.forward(x, tt, yy, logits=logits, logp=logp), "dgrad": lambda: cls.dgrad(1.0, dx)},
                             args.net_iters, args.repeats)

    B, S, C, d, out = 1, 8, 512, 64, cls.out_channels
    lib, s = ctx.lib, ctx.stream()
    scratch = th.empty(lib.cgd_op_attnpool_scratch_floats(B, S, C, d, out), device=dev)
    g = th.Generator(device=dev).manual_seed(5)
    h = th.randn(B * S * S, C, device=dev, generator=g)
    pos, qw, qb = (th.randn(n, device=dev, generator=g) * C ** -0.5 for n in (C * (S * S + 1), 3 * C * C, 3 * C))
    cw, cb = (th.randn(n, device=dev, generator=g) * C ** -0.5 for n in (out * C, out))
    dh = th.empty_like(h)

    def head_fwd():
        ctx.check(lib.cgd_op_attnpool_fwd(ctx.h, h.data_ptr(), pos.data_ptr(), qw.data_ptr(), qb.data_ptr(), cw.data_ptr(), cb.data_ptr(),
                                          yy.data_ptr(), None, logits.data_ptr(), logp.data_ptr(), scratch.data_ptr(), B, S, C, d, out, s))

    def head_bwd():
        ctx.check(lib.cgd_op_attnpool_bwd(ctx.h, qw.data_ptr(), qb.data_ptr(), cw.data_ptr(), cb.data_ptr(), 1.0, dh.data_ptr(),
                                          scratch.data_ptr(), B, S, C, d, out, s))

    head_fwd()
    head = steplib.per_launch({"forward": head_fwd, "backward": head_bwd}, args.net_iters, args.repeats)
    stat = steplib.stats

    print(json.dumps({"what": "guided step with / without classifier guidance at 256x256, batch 1, synthetic weights, bench.py config 2's networks; "
                              f"median / min / max of {args.repeats} alternating repeats of {args.steps} steps",
                      "plain_ms_per_step": stat(ms["plain"], 3), "classifier_ms_per_step": stat(ms["classifier"], 3),
                      "net_us": {n: stat(v, 1) for n, v in net.items()},
                      "head_us (op entry points: they also pack the transposed weights on every forward)": {n: stat(v, 1) for n, v in head.items()},
                      "launches_per_step": per_step, "finite": finite, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
