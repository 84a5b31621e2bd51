"""Cost of the classic UNet architecture (conv down / upsampling, additive timestep embeddings) at batch 1, synthetic weights:

  (a) step_ms / launches   one guided step (cutn 16, CLIP ViT-B/32, respace 250, p_sample) with the comics-faces configuration (256 x 256,
                           128 channels, 2 res blocks, attention at 16 x 16 with one head; cgd.model_flags.COMMUNITY_LOOKUP) beside the
                           published 256 x 256 unconditional model, and the kernel launches per step of the two
  (b) sconv_us             the stride-2 conv and its dgrad at that model's five downsample shapes, on weights packed once outside the timed
                           loop as the UNet runs them (cgd_op_conv3x3_s2_packed / _dgrad_packed; on the small maps the figure includes the
                           split-K reduce launch), and the per-call-pack entries cgd_op_conv3x3_s2 / _dgrad beside them ("*_with_pack"), against
                             torch:        F.conv2d(stride=2) on channels-last tensors and torch.nn.grad.conv2d_input (reported, not gated)
                             composition:  what the library offered before: cgd_op_conv3x3 at full resolution + a strided copy (forward), a
                                           strided scatter into zeros + cgd_op_conv3x3 on the rotated weights (backward): four times the products
  (c) headline             the guided step of the published 256 x 256 class-conditional model (bench.py config 2) on this tree and on the
                           tree given with --parent-root (a checkout of the parent commit with its library built), one process per
                           measurement, alternating; "not measured" without --parent-root

Every figure is the median of --repeats measurements taken alternately (after an untimed warm-up of each) with minimum and maximum.
Prints one JSON line.
Usage: python benchmarks/classic_step.py [--repeats 5] [--steps 40] [--op-iters 50] [--parent-root DIR] [--skip a,b,c]"""
import argparse
import json
import os
import subprocess
import sys

import steplib

COMICS = dict(image_size=256, model_channels=128, num_res_blocks=2, attention_resolutions="16", num_classes=None, num_heads=1,
              resblock_updown=False, use_scale_shift_norm=False)
UNCOND256 = dict(image_size=256, model_channels=256, num_res_blocks=2, attention_resolutions="32,16,8", num_classes=None, num_head_channels=64)
DOWN_SHAPES = [(256, 128), (128, 128), (64, 256), (32, 256), (16, 512)]  # (input side, channels) of the comics-faces model's five Downsamples

# one measurement of the headline step in a process of its own: argv = tree root, steps, repeats -> one JSON line
WORKER = r"""
import json, os, statistics, sys
root, steps, repeats = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
sys.path.insert(0, os.path.join(root, "benchmarks")); sys.path.insert(0, root)
os.chdir(root)
import steplib, torch as th
cfg, ctx, (unet, towers, smp, guid, image) = steplib.setup()
def guided():
    H, W = cfg["hw"]; start = cfg["start"]; guid.current_timestep = start; th.manual_seed(1000)
    it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=guid, model_kwargs={"y": th.zeros(1, dtype=th.long, device=steplib.DEV)},
                                       device=steplib.DEV, skip_timesteps=smp.num_timesteps - 1 - start, init_image=image, randomize_class=True, cond_fn_with_grad=True)
    n0 = steplib.launch_count(ctx); t, n, out = steplib.drain(it, guid, steps)
    return t / n * 1e3, (steplib.launch_count(ctx) - n0) / n
guided()
ms = [guided() for _ in range(repeats)]
print(json.dumps({"ms": statistics.median(m for m, _ in ms), "launches": ms[-1][1]}))
"""


def guided_steps(args):
    import torch as th
    dev = steplib.DEV
    sets = {"uncond256": steplib.setup(unet=UNCOND256), "comics_faces": steplib.setup(unet=COMICS)}

    def guided(name):
        cfg, ctx, (unet, towers, smp, guid, image) = sets[name]
        H, W = cfg["hw"]
        start = cfg["start"]
        guid.current_timestep = start
        th.manual_seed(1000)
        it = smp.p_sample_loop_progressive(unet, (1, 3, H, W), clip_denoised=False, cond_fn=guid, model_kwargs={}, device=dev,
                                           skip_timesteps=smp.num_timesteps - 1 - start, init_image=image, randomize_class=False,
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
    return {"step_ms": {n: steplib.stats(v, 3) for n, v in ms.items()}, "launches_per_step": per_step, "finite": finite}


def sconv_ops(args):
    import torch as th
    import torch.nn.functional as F
    import cgd_amd  # noqa: F401
    from cgd_amd import lib as L
    from cgd_amd import ops
    dev = steplib.DEV
    ctx = L.Context(0, 1)
    res = {}
    for (S, Cn) in DOWN_SHAPES:
        g = th.Generator(device=dev).manual_seed(7)
        x = th.randn(1, S, S, Cn, device=dev, generator=g)
        dy = th.randn(1, S // 2, S // 2, Cn, device=dev, generator=g)
        w = (th.rand(Cn, Cn, 3, 3, device=dev, generator=g) * 2 - 1) * (3.0 / (9 * Cn)) ** 0.5
        bias = th.randn(Cn, device=dev, generator=g) * 0.02
        wf, wd = (t.to(dev) for t in ops.pack_conv3x3(w.cpu()))
        wfrag, wdfrag = ops.pack_conv3x3_frag(ctx, w, dgrad=False), ops.pack_conv3x3_frag(ctx, w, dgrad=True)
        y, dx = th.empty(1, S // 2, S // 2, Cn, device=dev), th.empty(1, S, S, Cn, device=dev)
        stuffed = th.zeros(1, S, S, Cn, device=dev)
        x_cl, w_cl = x.permute(0, 3, 1, 2), w.contiguous(memory_format=th.channels_last)  # NCHW views of channels-last storage
        dy_cl = dy.permute(0, 3, 1, 2)

        fns = {
            "fwd": lambda: ops.conv3x3_s2(ctx, x, wf, bias, out=y, packed=True),
            "fwd_with_pack": lambda: ops.conv3x3_s2(ctx, x, w, bias, out=y),
            "fwd_composition": lambda: ops.conv3x3(ctx, x, wf, bias, w_frag=wfrag)[:, ::2, ::2].contiguous(),
            "fwd_torch": lambda: F.conv2d(x_cl, w_cl, bias, stride=2, padding=1),
            "dgrad": lambda: ops.conv3x3_s2_dgrad(ctx, dy, wd, out=dx, packed=True),
            "dgrad_with_pack": lambda: ops.conv3x3_s2_dgrad(ctx, dy, w, out=dx),
            "dgrad_composition": lambda: (stuffed[:, ::2, ::2].copy_(dy), ops.conv3x3(ctx, stuffed, wd, w_frag=wdfrag))[1],
            "dgrad_torch": lambda: th.nn.grad.conv2d_input(x_cl.shape, w_cl, dy_cl, stride=2, padding=1),
        }
        n0 = steplib.launch_count(ctx)
        fns["fwd"]()
        n1 = steplib.launch_count(ctx)
        fns["dgrad"]()
        launches = {"fwd": n1 - n0, "dgrad": steplib.launch_count(ctx) - n1}
        err = {"fwd_vs_composition": float((fns["fwd"]() - fns["fwd_composition"]()).abs().max()),
               "dgrad_vs_composition": float((fns["dgrad"]() - fns["dgrad_composition"]()).abs().max())}
        us = steplib.per_launch(fns, args.op_iters, args.repeats)
        res[f"{S}x{S}x{Cn} -> {S // 2}x{S // 2}"] = {**{n: steplib.stats(v, 1) for n, v in us.items()}, "max_abs_diff": err, "launches": launches,
                                                     "gflop": round(2 * (S // 2) ** 2 * Cn * Cn * 9 / 1e9, 3)}
    return res


def headline(args):
    if not args.parent_root:
        return "not measured (no --parent-root)"
    here = steplib.ROOT
    runs = {"parent": [], "this": []}
    launches = {}
    for _ in range(args.pairs):
        for name, root in (("parent", os.path.abspath(args.parent_root)), ("this", here)):
            r = subprocess.run([sys.executable, "-c", WORKER, root, str(args.steps), str(args.repeats)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                return f"not measured ({name} worker failed: {r.stderr[-300:]})"
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            runs[name].append(rec["ms"])
            launches[name] = rec["launches"]
    return {"step_ms": {n: steplib.stats(v, 3) for n, v in runs.items()}, "launches_per_step": launches,
            "pairs": [round(b - a, 3) for a, b in zip(runs["parent"], runs["this"])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--parent-root", default="")
    ap.add_argument("--skip", default="")
    args = ap.parse_args()
    skip = set(args.skip.split(",")) if args.skip else set()
    import torch as th
    out = {"what": f"classic UNet architecture at batch 1, synthetic weights; median / min / max of {args.repeats} alternating repeats "
                   f"({args.steps} steps; {args.op_iters} back-to-back op calls)"}
    # (c) first: its processes must not share the GPU with this one's networks
    out["headline_step (bench.py config 2; one process per measurement, parent and this tree alternating)"] = \
        "skipped" if "c" in skip else headline(args)
    out["sconv_us (composition = cgd_op_conv3x3 at full resolution + strided copy / strided scatter; torch = conv2d(stride=2), channels last)"] = \
        "skipped" if "b" in skip else sconv_ops(args)
    out["guided_step"] = "skipped" if "a" in skip else guided_steps(args)
    out["device"] = th.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
