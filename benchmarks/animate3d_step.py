"""Cost of 3D animation (cgd_amd/animate.py, mode="3d") beside 2D mode, at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP
ViT-B/32, batch 1, synthetic weights), in one process:

  call        microseconds per call, from HIP events, at 256x256 and 512x512, B 1, C 3, wrap border, bilinear and bicubic, of
                cgd_frame_warp3d   flat depth; a depth map resolved in 1 and in 3 fixed-point steps
                cgd_frame_warp     the affine 2D warp at the same shape
                torch              grid_sample on a grid built in torch (fp32) from cgd_frame_warp3d's formulas, the grid's construction
                                   included (flat, and the depth map in 1 and 3 steps, its lookups grid_sample calls of their own;
                                   reflection border: grid_sample has no wrap)
  frame_k_2d  one frame k > 0 as the driver makes it in 2D mode: cgd_frame_warp of the previous state, cgd_color_match, ClipGuidance.set_init
              with the LPIPS term at scale 1500, then the loop from the warped frame with frames_skip 0.6 (100 of the 250 steps run)
  frame_k_3d  the same with cgd_frame_warp3d (a fixed depth map, one step) in the warp's place

frame_k_2d and frame_k_3d alternate, --runs of each after one untimed warm-up of each; wall clock around work that ends in a device
synchronise.  The per-call figures are medians over --launch-repeats rounds in which the calls take turns.  Prints one JSON line.
Usage: python benchmarks/animate3d_step.py [--runs 3]"""
import argparse
import ctypes
import json
import statistics

import steplib


def torch_warp3d(F, th, src, cam, depth, iters, interp):
    """cgd_frame_warp3d's formulas in torch ops on src's device, fp32: the grid, then grid_sample"""
    _, _, H, W = src.shape
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float32, device=src.device), th.arange(W, dtype=th.float32, device=src.device), indexing="ij")
    R, T = cam.R, cam.T
    b = [R[i] * T[0] + R[3 + i] * T[1] + R[6 + i] * T[2] for i in range(3)]
    rx, ry = (xs - cam.cx) / cam.f, (ys - cam.cy) / cam.f
    ax, ay = R[0] * rx + R[3] * ry + R[6], R[1] * rx + R[4] * ry + R[7]
    az = (R[2] * rx + R[5] * ry + R[8]).clamp(min=1e-6)

    def grid(sx, sy):
        return th.stack([sx * (2 / (W - 1)) - 1, sy * (2 / (H - 1)) - 1], dim=-1).unsqueeze(0)

    sx, sy = xs, ys
    for _ in range(iters if depth is not None else 1):
        if depth is None:
            z = max(cam.z0, cam.near)
        else:
            z = F.grid_sample(depth, grid(sx, sy), mode="bilinear", padding_mode="border", align_corners=True)[0, 0].clamp(min=cam.near)
        lam = ((z + b[2]) / az).clamp(min=cam.near)
        sx, sy = cam.cx + cam.f * (lam * ax - b[0]) / z, cam.cy + cam.f * (lam * ay - b[1]) / z
    return F.grid_sample(src, grid(sx, sy), mode=interp, padding_mode="reflection", align_corners=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=300)
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

    def smooth_depth(n, m):
        ys, xs = th.meshgrid(th.arange(n, dtype=th.float32), th.arange(m, dtype=th.float32), indexing="ij")
        return (1.1 + 0.5 * th.sin(xs * (9.0 / m)) * th.cos(ys * (7.0 / n)))[None, None].to(dev).contiguous()

    matrix = animate.motion_matrix(1.02, 2.0, 1.5, -0.5, H, W)
    cam = animate.camera(2.0, -1.0, 4.0, 0.3, 0.5, 2.0, 40.0, H, W)
    depth = smooth_depth(H, W)
    state = {"prev": th.tanh(th.randn(1, 3, H, W, generator=th.Generator().manual_seed(5))).to(dev)}
    stats0 = ops.channel_stats(ctx, state["prev"])

    def run(mode):
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
        th.cuda.synchronize()
        if mode == "frame_k_3d":
            init = ops.frame_warp3d(ctx, state["prev"], cam, depth=depth, interp="bicubic", border="wrap", clamp=True, iters=1)
        else:
            init = ops.frame_warp(ctx, state["prev"], matrix, interp="bicubic", border="wrap", clamp=True)
        ops.color_match(ctx, init, stats0, amount=1.0, clamp=True)
        guid.set_init(init, 1500, lpips=lpips)
        kw.update(init_image=init, skip_timesteps=skip)
        guid.current_timestep = smp.num_timesteps - 1
        t, n, out = steplib.drain(smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw), guid)
        return t, n, bool(th.isfinite(out["sample"]).all())

    res = steplib.alternate(["frame_k_2d", "frame_k_3d"], run, args.runs)
    sec = {m: [v[0] for v in r] for m, r in res.items()}
    steps = {m: r[-1][1] for m, r in res.items()}
    finite = {m: all(v[2] for v in r) for m, r in res.items()}

    fns, keep = {}, []  # (keep: the tensors whose pointers the closures hold)
    lib, h, s_ = ctx.lib, ctx.h, ctx.stream()
    for n in (256, 512):
        src = th.randn(1, 3, n, n, device=dev)
        dst, dmap = th.empty_like(src), smooth_depth(n, n)
        m = animate.motion_matrix(1.02, 2.0, 1.5, -0.5, n, n)
        c = animate.camera(2.0, -1.0, 4.0, 0.3, 0.5, 2.0, 40.0, n, n)
        # the C entries themselves, as animate_step.py calls them: the checks of the ops wrappers cost the host as much as a launch costs the GPU
        for code, interp in enumerate(("bilinear", "bicubic")):
            w = L.Warp((ctypes.c_double * 6)(*m), code, L.WARP_BORDER["wrap"], 0)
            fns[f"cgd_frame_warp_{interp}_{n}"] = (lambda s=src.data_ptr(), d=dst.data_ptr(), w=w, n=n:
                                                   lib.cgd_frame_warp(h, s, d, 1, 3, n, n, ctypes.byref(w), s_))
            for name, dp, iters in (("flat", None, 1), ("depth_1", dmap.data_ptr(), 1), ("depth_3", dmap.data_ptr(), 3)):
                k = L.Camera((ctypes.c_double * 9)(*c.R), (ctypes.c_double * 3)(*c.T), c.f, c.cx, c.cy, c.z0, c.near, iters, code,
                             L.WARP_BORDER["wrap"], 0)
                fns[f"cgd_frame_warp3d_{name}_{interp}_{n}"] = (lambda s=src.data_ptr(), d=dst.data_ptr(), dp=dp, k=k, n=n:
                                                                lib.cgd_frame_warp3d(h, s, d, dp, 1, 1, 3, n, n, ctypes.byref(k), s_))
                fns[f"torch_{name}_{interp}_{n}"] = (lambda s=src, c=c, dm=(None if dp is None else dmap), it=iters, i=interp:
                                                     torch_warp3d(F, th, s, c, dm, it, i))
        keep.append((src, dst, dmap))
    for name, fn in fns.items():  # every C entry accepts its arguments
        rc = fn()
        assert not isinstance(rc, int) or rc == 0, (name, rc)
    call_us = steplib.per_launch(fns, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in sec.items()}
    print(json.dumps({"what": "seconds per animation frame k > 0, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, synthetic weights, -respace 250): "
                              f"warp + colour match + {steps['frame_k_3d']} steps (frames_skip 0.6) with the LPIPS term, 2D warp against 3D warp "
                              f"(depth map, 1 step); median of {args.runs} alternating runs",
                      "seconds_per_frame": {m: round(v, 3) for m, v in med.items()}, "runs_s": {m: [round(t, 3) for t in v] for m, v in sec.items()},
                      "steps": steps, "finite": finite, "call_us": {n: steplib.stats(v) for n, v in call_us.items()},
                      "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
