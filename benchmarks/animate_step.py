"""Cost of 2D animation (cgd_amd/animate.py) at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP ViT-B/32, batch 1, synthetic
weights), in one process:

  call      microseconds per call, from HIP events, of cgd_frame_warp (bilinear and bicubic, wrap border, at 256x256 and 512x512, B 1, C 3), of
            cgd_channel_stats and cgd_color_match at the same sizes, and of the same bilinear / bicubic warp through torch's affine_grid +
            grid_sample (reflection border: grid_sample has no wrap) for comparison
  frame0    one full frame: all 250 steps of p_sample_loop_progressive (-respace 250)
  frame_k   one frame k > 0 as the driver makes it: cgd_frame_warp of the previous state, cgd_color_match, ClipGuidance.set_init with the
            LPIPS term at scale 1500, then the loop from the warped frame with frames_skip 0.6 (150 of the 250 steps skipped, 100 run)

frame0 and frame_k alternate, --runs of each after one untimed warm-up of each; wall clock around work that ends in a device synchronise.
Prints one JSON line.  Usage: python benchmarks/animate_step.py [--runs 3]"""
import argparse
import ctypes
import json
import statistics

import steplib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=500)
    ap.add_argument("--launch-repeats", type=int, default=5)
    args = ap.parse_args()
    import torch as th
    import torch.nn.functional as F
    from cgd_amd import animate, nets, ops, synthetic
    from cgd_amd import lib as L
    dev = steplib.DEV
    cfg, ctx, (unet, towers, smp, guid, _) = steplib.setup()
    H, W = cfg["hw"]
    y = {"y": th.zeros(1, dtype=th.long, device=dev)}
    lpips = nets.LpipsVGG(ctx).load_state_dict(synthetic.lpips_state_dict(device=dev))
    skip = round(0.6 * smp.num_timesteps)
    matrix = animate.motion_matrix(1.02, 2.0, 1.5, -0.5, H, W)
    state = {"prev": th.tanh(th.randn(1, 3, H, W, generator=th.Generator().manual_seed(5))).to(dev)}
    stats0 = ops.channel_stats(ctx, state["prev"])

    def run(mode):
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
        th.cuda.synchronize()
        if mode == "frame_k":
            init = ops.frame_warp(ctx, state["prev"], matrix, interp="bicubic", border="wrap", clamp=True)
            ops.color_match(ctx, init, stats0, amount=1.0, clamp=True)
            guid.set_init(init, 1500, lpips=lpips)
            kw.update(init_image=init, skip_timesteps=skip)
        else:
            guid.set_init(None, 0)
        guid.current_timestep = smp.num_timesteps - 1
        t, n, out = steplib.drain(smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw), guid)
        return t, n, bool(th.isfinite(out["sample"]).all())

    res = steplib.alternate(["frame0", "frame_k"], run, args.runs)
    sec = {m: [v[0] for v in r] for m, r in res.items()}
    steps = {m: r[-1][1] for m, r in res.items()}
    finite = {m: all(v[2] for v in r) for m, r in res.items()}

    fns, keep = {}, []  # (keep: the tensors whose pointers the closures hold)
    for n in (256, 512):
        src = th.randn(1, 3, n, n, device=dev)
        dst, st = th.empty_like(src), th.empty(1, 3, 2, device=dev)
        m = animate.motion_matrix(1.02, 2.0, 1.5, -0.5, n, n)
        ref = ops.channel_stats(ctx, th.randn(1, 3, n, n, device=dev))
        theta = th.tensor([[m[0], m[1], 0.0], [m[3], m[4], 0.0]], device=dev).unsqueeze(0)  # same scale and angle, no shift
        # the C entries themselves, as ilvr_step.py calls them: the checks of the ops wrappers cost the host as much as a launch costs the GPU
        lib, h, s_ = ctx.lib, ctx.h, ctx.stream()
        for code, interp in enumerate(("bilinear", "bicubic")):
            w = L.Warp((ctypes.c_double * 6)(*m), code, L.WARP_BORDER["wrap"], 0)
            fns[f"cgd_frame_warp_{interp}_{n}"] = (lambda s=src.data_ptr(), d=dst.data_ptr(), w=w, n=n:
                                                   lib.cgd_frame_warp(h, s, d, 1, 3, n, n, ctypes.byref(w), s_))
            fns[f"grid_sample_{interp}_{n}"] = (lambda s=src, t=theta, i=interp: F.grid_sample(
                s, F.affine_grid(t, list(s.shape), align_corners=True), mode=i, padding_mode="reflection", align_corners=True))
        fns[f"cgd_channel_stats_{n}"] = lambda s=src.data_ptr(), o=st.data_ptr(), n=n: lib.cgd_channel_stats(h, s, o, 1, 3, n, n, s_)
        fns[f"cgd_color_match_{n}"] = (lambda d=dst.data_ptr(), o=st.data_ptr(), r=ref.data_ptr(), n=n:
                                       lib.cgd_color_match(h, d, o, r, 1, 1.0, 0, 1, 3, n, n, s_))
        keep.append((src, dst, st, ref))
    call_us = steplib.per_launch(fns, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in sec.items()}
    print(json.dumps({"what": "seconds per animation frame, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, synthetic weights, -respace 250): "
                              f"frame0 = all 250 steps, frame_k = warp + colour match + {steps['frame_k']} steps (frames_skip 0.6) with the LPIPS term; "
                              f"median of {args.runs} alternating runs",
                      "seconds_per_frame": {m: round(v, 3) for m, v in med.items()}, "runs_s": {m: [round(t, 3) for t in v] for m, v in sec.items()},
                      "steps": steps, "finite": finite, "call_us": {n: steplib.stats(v) for n, v in call_us.items()},
                      "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
