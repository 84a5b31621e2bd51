"""Cost of super-resolution sampling at batch 1, synthetic weights, in one process:

  step_ms         milliseconds per guided step (cutn 16, CLIP ViT-B/32, respace 250, p_sample) on a 256x256 frame: the 64 -> 256 upsampler
                  (192 channels, 6-channel stem, low-res image 64x64 in model_kwargs["low_res"]) against the 256x256 base model (bench.py config 2)
  launches        kernel launches per guided step of the two
  stem_us         the conditioned stem alone at (256x256, low 64x64, Cout 192) and (512x512, low 128x128, Cout 192): the fused launch
                  (cgd_op_sr_stem) against the unfused composition -- F.interpolate(bilinear) + cat into a (1,6,H,W) tensor, then cgd_op_conv_in
                  with Cin = 6 as the library dispatches it (im2col + weight padding + MFMA GEMM)

Every figure is the median of --repeats measurements taken alternately (after an untimed warm-up of each) with minimum and maximum.
Prints one JSON line.  `--plan` (no GPU needed) prints instead which kernel every conv and attention level of the two upsampler
configurations dispatches to, from the library's host-only planners.
Usage: python benchmarks/upsample_step.py [--repeats 5] [--steps 40] [--stem-iters 50] | --plan"""
import argparse
import ctypes
import json

import steplib


def upsampler_kwargs(size):
    from cgd import script_util
    return script_util.upsampler_unet_kwargs(script_util.upsampler_config(size))


def plan(size):
    """[(level resolution, width, conv kernel / tile / split-K of a width -> width 3x3 conv, attention family or None)] at batch 1"""
    from cgd_amd import lib as L
    lib = L.load()
    kw = upsampler_kwargs(size)
    att = [size // int(r) for r in kw["attention_resolutions"].split(",")]
    conv_names = {0: "igemm", 1: "hconv2 / wconv (515) / kconv (516)", 2: "hgemm"}
    fam = {0: "batched GEMMs + row softmax", 1: "attn_s64", 2: "attn_mid", 3: "attn_flash"}
    rows = []
    for level, mult in enumerate(kw["channel_mult"]):
        res, width = size >> level, int(mult * kw["model_channels"])
        out5 = (ctypes.c_int * 5)()
        rc = lib.cgd_op_plan_conv(1, res, res, width, width, 1, 256, 0, 1, 0, out5)
        a = None
        if (1 << level) in att:
            d = width // kw["num_heads"] if kw["num_head_channels"] == -1 else kw["num_head_channels"]
            out2 = (ctypes.c_int * 2)()
            lib.cgd_op_attn_plan(res * res, d, 3 * width, width, 1, -1, out2)
            a = {"heads": width // d, "head_dim": d, "tokens": res * res, "family": fam[out2[0]]}
        rows.append({"resolution": res, "width": width, "conv3x3": {"rc": rc, "kernel": conv_names.get(out5[0], out5[0]), "tile": out5[1],
                                                                   "splitk": out5[2], "workgroups": out5[3]}, "attention": a})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--stem-iters", type=int, default=50)
    ap.add_argument("--plan", action="store_true")
    args = ap.parse_args()
    import cgd_amd  # noqa: F401
    if args.plan:
        print(json.dumps({"what": "dispatch of the two upsampler configurations at batch 1, bf16x3, 256 CUs (host-only planners)",
                          "64_256": plan(256), "128_512": plan(512)}))
        return
    import torch as th
    import torch.nn.functional as F
    from cgd_amd import ops
    dev = steplib.DEV
    sets = {"base256": steplib.setup(), "upsampler64_256": steplib.setup(unet=upsampler_kwargs(256))}
    low = th.tanh(th.randn(1, 3, 64, 64, generator=th.Generator().manual_seed(5))).to(dev)

    def guided(name):
        cfg, ctx, (unet, towers, smp, guid, image) = sets[name]
        H, W = cfg["hw"]
        start = cfg["start"]
        guid.current_timestep = start
        th.manual_seed(1000)
        mk = {"y": th.zeros(1, dtype=th.long, device=dev)}
        if name != "base256":
            mk["low_res"] = low
        it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=guid, model_kwargs=mk, device=dev,
                                           skip_timesteps=smp.num_timesteps - 1 - start, init_image=image, randomize_class=True,
                                           cond_fn_with_grad=True)
        n0 = steplib.launch_count(ctx)
        t, n, out = steplib.drain(it, guid, args.steps)
        return t / n * 1e3, (steplib.launch_count(ctx) - n0) / n, bool(th.isfinite(out["sample"]).all())

    for name in sets:
        guided(name)
    ms, per_step, finite = {n: [] for n in sets}, {}, {}
    for _ in range(args.repeats):
        for name in sets:
            t, per_step[name], finite[name] = guided(name)
            ms[name].append(t)

    ctx = sets["base256"][1]
    stem = {}
    for (H, lh) in ((256, 64), (512, 128)):
        g = th.Generator(device=dev).manual_seed(7)
        x = th.randn(1, 3, H, H, device=dev, generator=g)
        lo = th.rand(1, 3, lh, lh, device=dev, generator=g) * 2 - 1
        w = (th.rand(192, 6, 3, 3, device=dev, generator=g) * 2 - 1) * (3.0 / 54) ** 0.5
        bias = th.randn(192, device=dev, generator=g) * 0.02
        wf = ops.pack_conv3x3(w)[0]
        y = th.empty(1, H, H, 192, device=dev)

        def fused():
            ops.sr_stem(ctx, x, lo, wf, bias, out=y)

        def unfused():
            x6 = th.cat([x, F.interpolate(lo, (H, H), mode="bilinear")], 1)
            return ops.conv_in(ctx, x6, wf, bias, 192)

        fused()
        err = float((y - unfused()).abs().max())
        us = steplib.per_launch({"fused": fused, "unfused": unfused}, args.stem_iters, args.repeats)
        stem[f"{H}x{H} low {lh}x{lh} Cout 192"] = {**{n: steplib.stats(v, 1) for n, v in us.items()}, "max_abs_diff": err}

    print(json.dumps({"what": "super-resolution sampling at batch 1, synthetic weights; median / min / max of "
                              f"{args.repeats} alternating repeats ({args.steps} steps; {args.stem_iters} back-to-back stem calls)",
                      "step_ms": {n: steplib.stats(v, 3) for n, v in ms.items()}, "launches_per_step": per_step, "finite": finite,
                      "stem_us (unfused = torch interpolate + cat, then conv_in Cin 6; its output allocation included)": stem,
                      "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
