"""Cost and accuracy of the native depth network (nets.DepthNet, csrc/depth.hip): DPT-Large on synthetic weights, in one process:

  call        per call of the net on a 256x256 and on a 512x512 frame (batch 1; the net runs at 384x384 for both): microseconds from HIP events
              and kernel launches, split into the resize to net size, the backbone (patch GEMM, 24 blocks), the decoder (readout, reassemble,
              fusion, head: the whole forward minus the backbone) and the resize back
  frame_k     one 3D animation frame k > 0 at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP ViT-B/32, batch 1, -respace 250,
              frames_skip 0.6: 100 steps run) with the depth from the net against the same frame with flat depth; medians of --runs
              alternating runs after one untimed warm-up of each
  error       the largest deviation of the full 24-layer net at 384x384 from tests/depth_ref.py on the same weights (the reference in fp32,
              which is what the tests use, and in fp64; the net in the bf16x3 mode and in the exact-fp32 mode): max |a - b| of inv_depth, the
              largest |a - b| / (1e-4 + 1e-3 |ref|) and the share of pixels above 1, beside the fp32 reference's own distance from the
              fp64 one (--no-error skips it)

Prints one JSON line.  Usage: python benchmarks/depth_step.py [--runs 3]"""
import argparse
import json
import statistics
import time

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=20)
    ap.add_argument("--launch-repeats", type=int, default=5)
    ap.add_argument("--no-error", action="store_true")
    ap.add_argument("--no-frame", action="store_true")
    args = ap.parse_args()
    import torch as th
    from cgd_amd import animate, nets, ops, synthetic
    dev = steplib.DEV
    if args.no_frame:
        import cgd_amd  # noqa: F401
        from cgd_amd import lib as L
        ctx = L.Context(0, 1)
    else:
        cfg, ctx, (unet, towers, smp, guid, _) = steplib.setup()
    sd = synthetic.depth_state_dict("dpt_large")
    net = nets.DepthNet(ctx, "dpt_large").load_state_dict(sd)
    lib = ctx.lib

    # ---- per call: time and launches of the four parts
    fns, launches, keep = {}, {}, []
    for n in (256, 512):
        frame = th.rand(1, 3, n, n, device=dev)
        h, w = nets.depth_net_size(n, n, net.size)
        img = ops.resize_cubic(ctx, frame, h, w, a=2.0, b=-1.0)
        dep = net.forward(img, want="depth")
        back = th.empty(1, 1, n, n, device=dev)
        keep.append((frame, img, dep, back))

        def backbone(img=img):
            lib.cgd_depth_debug_stop(net.h, 1)
            net.forward(img, want="depth")
            lib.cgd_depth_debug_stop(net.h, 0)

        parts = {f"resize_in_{n}": lambda frame=frame, img=img, h=h, w=w: ops.resize_cubic(ctx, frame, h, w, a=2.0, b=-1.0, out=img),
                 f"backbone_{n}": backbone,
                 f"forward_{n}": lambda img=img: net.forward(img, want="depth"),
                 f"resize_out_{n}": lambda dep=dep, back=back, n=n: ops.resize_cubic(ctx, dep, n, n, lo=net.floor, out=back),
                 f"call_{n}": lambda frame=frame: net(frame)}
        for name, fn in parts.items():
            fn()
            c0 = steplib.launch_count(ctx)
            fn()
            launches[name] = steplib.launch_count(ctx) - c0
        fns.update(parts)
    call_us = {k: steplib.stats(v) for k, v in steplib.per_launch(fns, args.launch_iters, args.launch_repeats).items()}
    for n in (256, 512):
        call_us[f"decoder_{n}"] = {"median": round(call_us[f"forward_{n}"]["median"] - call_us[f"backbone_{n}"]["median"], 2)}
        launches[f"decoder_{n}"] = launches[f"forward_{n}"] - launches[f"backbone_{n}"]
    out = {"what": "DPT-Large (synthetic weights, bf16x3) per call on a 256x256 and a 512x512 frame (net 384x384), batch 1: microseconds (HIP events, "
                   f"{args.launch_iters} calls back to back, {args.launch_repeats} rounds) and kernel launches per part; decoder = forward - backbone",
           "call_us": call_us, "launches": launches, "device": th.cuda.get_device_name(0)}

    # ---- a 3D frame k > 0 with the net against flat depth
    if not args.no_frame:
        H, W = cfg["hw"]
        y = {"y": th.zeros(1, dtype=th.long, device=dev)}
        lpips = nets.LpipsVGG(ctx).load_state_dict(synthetic.lpips_state_dict(device=dev))
        skip = round(0.6 * smp.num_timesteps)
        cam = animate.camera(2.0, -1.0, 4.0, 0.3, 0.5, 2.0, 40.0, H, W)
        prev = th.tanh(th.randn(1, 3, H, W, generator=th.Generator().manual_seed(5))).to(dev)
        stats0 = ops.channel_stats(ctx, prev)

        def run(mode):
            kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
            th.cuda.synchronize()
            t0 = time.perf_counter()
            depth = net((prev.clamp(-1, 1) + 1) / 2) if mode == "frame_k_net" else None
            init = ops.frame_warp3d(ctx, prev, cam, depth=depth, interp="bicubic", border="wrap", clamp=True, iters=1)
            ops.color_match(ctx, init, stats0, amount=1.0, clamp=True)
            guid.set_init(init, 1500, lpips=lpips)
            kw.update(init_image=init, skip_timesteps=skip)
            guid.current_timestep = smp.num_timesteps - 1
            _, nsteps, res = steplib.drain(smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw), guid)
            return time.perf_counter() - t0, nsteps, bool(th.isfinite(res["sample"]).all())

        res = steplib.alternate(["frame_k_flat", "frame_k_net"], run, args.runs)
        sec = {m: [v[0] for v in r] for m, r in res.items()}
        out["seconds_per_frame"] = {m: round(statistics.median(v), 3) for m, v in sec.items()}
        out["runs_s"] = {m: [round(t, 3) for t in v] for m, v in sec.items()}
        out["steps"] = {m: r[-1][1] for m, r in res.items()}
        out["finite"] = {m: all(v[2] for v in r) for m, r in res.items()}

    # ---- the full net against the CPU reference
    if not args.no_error:
        from tests import depth_ref
        img = th.randn(1, 3, 384, 384, generator=th.Generator().manual_seed(9)).clamp(-1, 1)
        with th.no_grad():
            ref32 = depth_ref.forward(nets.DEPTH_CONFIGS["dpt_large"], sd, img)[0].double()
            ref64 = depth_ref.forward(nets.DEPTH_CONFIGS["dpt_large"], sd, img, dtype=th.float64)[0]

        def judge(got, ref):
            diff = (got.double() - ref).abs()
            return {"max_abs": float(diff.max()), "worst_over_bound": float((diff / (1e-4 + 1e-3 * ref.abs())).max()),
                    "share_over_bound": float((diff > 1e-4 + 1e-3 * ref.abs()).double().mean())}

        out["error_384"] = {"ref_peak": float(ref32.abs().max()), "ref_positive_share": float((ref32 > 0).double().mean()),
                            "bf16x3_vs_ref_fp32": judge(net.forward(img.to(dev)).cpu(), ref32),
                            "bf16x3_vs_ref_fp64": judge(net.forward(img.to(dev)).cpu(), ref64), "ref_fp32_vs_ref_fp64": judge(ref32, ref64)}
        ctx.set_precision("f32")
        out["error_384"]["f32_vs_ref_fp64"] = judge(net.forward(img.to(dev)).cpu(), ref64)
        ctx.set_precision("bf16x3")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
