"""Cost of a guided step with the VGG Gram-matrix style term (csrc/gram.hip, the style head of csrc/lpips.hip) at the headline shape
(bench.py config 2's networks: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic weights, respace 250, p_sample), in one process:

  neither_ms      milliseconds per guided step without an init image and without a style image
  lpips_ms        the same loop with the LPIPS-VGG16 init term (init_scale 1000)
  style_ms        with the style term alone: one VGG16 trunk pass forward and backward plus the style head.  --style_scale is small (default
                  0.01) on purpose: the loss is quartic in the activations, and with seeded random weights a scale that matters drives the
                  sample to infinity within the 40 steps; a step on non-finite data is no measurement (its kernels draw less power and run
                  faster).  The cost of the term does not depend on the scale; `finite` and `style_loss` in the output say the run was sound
  both_ms         with both: one combined call, the trunk pass is shared
  gram_us         cgd_op_gram alone at the five tap shapes (N, C) of a 256x256 frame, from HIP events around --iters back-to-back calls,
                  torch.matmul(A.T, A) on the same tensors beside it, and each as a multiple of the time an HBM read of A takes at the
                  6.3 TB/s a streaming copy reaches on this part (back-to-back calls on one tensor find A in the 256 MB Infinity Cache, so a
                  multiple below 1 is possible and says nothing about a cold call)
  launches        kernel launches per guided step of every path

Every figure is the median of --repeats measurements (the paths taken alternately, after one untimed warm-up each) with their minimum and
maximum beside it.  Prints one JSON line.  Usage: python benchmarks/style_step.py [--repeats 5] [--steps 40]"""
import argparse
import json

import steplib

HBM_BYTES_PER_S = 6.3e12
TAP_SHAPES = [(65536, 64), (16384, 128), (4096, 256), (1024, 512), (256, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--style_scale", type=float, default=0.01)
    args = ap.parse_args()
    import torch as th
    from cgd_amd import guidance as dg
    from cgd_amd import nets, synthetic
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup()
    H, W = cfg["hw"]
    gen = th.Generator().manual_seed(97)
    style = (th.rand(1, 3, H, W, generator=gen) * 2 - 1).to(dev)
    init = th.tanh(th.randn(1, 3, H, W, generator=gen)).to(dev)
    vgg = nets.LpipsVGG(ctx).load_state_dict(synthetic.lpips_state_dict(device=dev))
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    start = cfg["start"]
    skip = smp.num_timesteps - 1 - start

    def make(lpips, styled):
        kw = dict(lpips=vgg) if (lpips or styled) else {}
        if lpips:
            kw.update(init_tensor=init, init_scale=1000.0)
        if styled:
            kw.update(style_tensor=style, style_scale=args.style_scale)
        return dg.ClipGuidance(ctx, unet, towers, smp, guid.targets_list, guid.weights, cfg["cutn"], clip_guidance_scale=1000.0, tv_scale=150.0,
                               range_scale=50.0, **kw)

    conds = {"neither": guid, "lpips": make(True, False), "style": make(False, True), "both": make(True, True)}
    per_step, finite, style_loss = {}, {}, {}

    def guided(name):
        cond = conds[name]
        cond.current_timestep = start
        it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=cond, model_kwargs=dict(y), device=dev,
                                           skip_timesteps=skip, init_image=image, randomize_class=False, cond_fn_with_grad=True)
        n0 = steplib.launch_count(ctx)
        t, n, out = steplib.drain(it, cond, args.steps)
        per_step[name], finite[name] = (steplib.launch_count(ctx) - n0) / n, bool(th.isfinite(out["sample"]).all())
        if cond.style is not None:
            style_loss[name] = cond.log()["Style Loss"]
        return t / n * 1e3

    ms = steplib.alternate(list(conds), guided, args.repeats)

    lib, s = ctx.lib, ctx.stream()
    g = th.Generator(device=dev).manual_seed(5)
    fns, read_us = {}, {}
    for (N, Cc) in TAP_SHAPES:
        a = th.relu(th.randn(N, Cc, device=dev, generator=g))
        out = th.empty(Cc, Cc, device=dev)
        scale = 1.0 / (N * Cc)
        fns[f"cgd_op_gram {N}x{Cc}"] = lambda a=a, out=out, N=N, Cc=Cc, scale=scale: ctx.check(
            lib.cgd_op_gram(ctx.h, a.data_ptr(), Cc, 1, N, Cc, scale, out.data_ptr(), s))
        fns[f"torch.matmul {N}x{Cc}"] = lambda a=a, out=out: th.matmul(a.t(), a, out=out)
        read_us[f"{N}x{Cc}"] = N * Cc * 4 / HBM_BYTES_PER_S * 1e6
    us = steplib.per_launch(fns, args.iters, args.repeats)
    stat = steplib.stats
    gram = {}
    for (N, Cc) in TAP_SHAPES:
        key = f"{N}x{Cc}"
        ours, torch_ = stat(us[f"cgd_op_gram {key}"], 1), stat(us[f"torch.matmul {key}"], 1)
        gram[key] = {"cgd_op_gram_us": ours, "torch_matmul_us": torch_, "hbm_read_of_A_us": round(read_us[key], 2),
                     "cgd_op_gram_over_hbm_read": round(ours["median"] / read_us[key], 1),
                     "torch_matmul_over_hbm_read": round(torch_["median"] / read_us[key], 1)}
    print(json.dumps({"what": "guided step without / with the LPIPS init term and the VGG Gram-matrix style term at 256x256, cutn 16, batch 1, "
                              f"synthetic weights, bench.py config 2's networks; median / min / max of {args.repeats} alternating repeats of "
                              f"{args.steps} steps",
                      "ms_per_step": {n: stat(v, 3) for n, v in ms.items()},
                      "gram_us (back-to-back calls, A [N][C] fp32, two launches per cgd_op_gram call)": gram,
                      "launches_per_step": per_step, "finite": finite, "style_loss (last step, scaled)": style_loss, "style_scale": args.style_scale, "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
