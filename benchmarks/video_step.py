"""Cost of video mode (cgd_amd/animate.py, mode="video") beside 2D mode, at the headline shape (bench.py config 2: 256x256, cutn 16, CLIP
ViT-B/32, batch 1, synthetic weights), in one process:

  call        microseconds per call, from HIP events, at 256x256 and 512x512, B 1, C 3, of
                cgd_flow_estimate      the defaults (4 levels, 4 iterations, radius 4): luminance, pyramid and every level
                cgd_op_flow_level      the finest level alone, started from a coarser flow
                torch_flow             the same algorithm composed from torch ops on the GPU, fp32: antialiased bicubic interpolate for the
                                       pyramid, unfold for the template windows, one grid_sample over all 81 window offsets per iteration
                torch_flow_level       its finest level alone
                cgd_frame_warp_flow    bicubic, replicate border, with a fallback; without and with the consistency check
                torch_warp_flow        grid_sample on base grid + flow (the check: a second grid_sample of the backward flow and a blend)
  frame_k_2d  one frame k > 0 as the driver makes it in 2D mode: cgd_frame_warp of the previous state, cgd_color_match, ClipGuidance.set_init
              with the LPIPS term at scale 1500, then the loop from the warped frame with frames_skip 0.6 (100 of the 250 steps run)
  frame_k_video, frame_k_video_checked
              the same with ops.flow_estimate (two of them under check_consistency) and ops.frame_warp_flow in the warp's place; the two clip
              frames are already on the GPU

The three frame modes alternate, --runs of each after one untimed warm-up of each; wall clock around work that ends in a device synchronise;
launches_per_frame counts the library's kernel launches of one frame.  The per-call figures are medians over --launch-repeats rounds in
which the calls take turns.  Prints one JSON line.
Usage: python benchmarks/video_step.py [--runs 3]"""
import argparse
import ctypes
import json
import math
import statistics

import steplib


def torch_level(F, th, b, a, flow, iters=4, R=4, lam=1e-3, max_step=1.0):
    """one level of the patch-form Lucas-Kanade flow on (1,1,H,W) planes, from `flow` (1,2,H,W), in torch ops"""
    _, _, H, W = b.shape
    k = 2 * R + 1
    bp = F.pad(b, (1, 1, 1, 1), mode="replicate")
    bx, by = (bp[..., 1:-1, 2:] - bp[..., 1:-1, :-2]) * 0.5, (bp[..., 2:, 1:-1] - bp[..., :-2, 1:-1]) * 0.5
    ub, ux, uy = (F.unfold(t, k, padding=R)[0] for t in (b, bx, by))  # (k k, H W), dy-major like the kernel's loop
    inside = F.unfold(th.ones_like(b), k, padding=R)[0] > 0
    d = th.arange(-R, R + 1, dtype=th.float32, device=b.device)
    dy, dx = (t.reshape(-1, 1) for t in th.meshgrid(d, d, indexing="ij"))
    ys, xs = (t.reshape(1, -1) for t in th.meshgrid(th.arange(H, dtype=th.float32, device=b.device),
                                                     th.arange(W, dtype=th.float32, device=b.device), indexing="ij"))
    u, v = flow[0, 0].reshape(1, -1).clone(), flow[0, 1].reshape(1, -1).clone()
    for _ in range(iters):
        sx, sy = xs + dx + u, ys + dy + v
        valid = (inside & (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)).float()
        grid = th.stack([sx * (2 / max(W - 1, 1)) - 1, sy * (2 / max(H - 1, 1)) - 1], dim=-1)[None]
        av = F.grid_sample(a, grid, mode="bilinear", padding_mode="border", align_corners=True)[0, 0]
        gx, gy = ux * valid, uy * valid
        e = ub - av
        gxx, gyy, gxy = lam + (gx * gx).sum(0), lam + (gy * gy).sum(0), (gx * gy).sum(0)
        rx, ry = (gx * e).sum(0), (gy * e).sum(0)
        det = gxx * gyy - gxy * gxy
        du, dv = (gyy * rx - gxy * ry) / det, (gxx * ry - gxy * rx) / det
        length = (du * du + dv * dv).sqrt().clamp(min=1e-30)
        scale = (max_step / length).clamp(max=1.0)
        u, v = u + th.nan_to_num(du * scale), v + th.nan_to_num(dv * scale)
    return th.stack([u.reshape(H, W), v.reshape(H, W)])[None]


def torch_flow(F, th, tmpl, img, levels=4, iters=4, R=4):
    """the whole estimate in torch ops: luminance, antialiased bicubic pyramid, levels from the coarsest down"""
    luma = th.tensor([0.2989, 0.587, 0.114], device=tmpl.device).view(1, 3, 1, 1)
    pyr = [th.cat([(tmpl * luma).sum(1, keepdim=True), (img * luma).sum(1, keepdim=True)])]
    for _ in range(1, levels):
        h, w = pyr[-1].shape[2:]
        if min((h + 1) // 2, (w + 1) // 2) < 2 * R + 1:
            break
        pyr.append(F.interpolate(pyr[-1], size=((h + 1) // 2, (w + 1) // 2), mode="bicubic", antialias=True, align_corners=False))
    flow = None
    for p in reversed(pyr):
        h, w = p.shape[2:]
        if flow is None:
            flow = th.zeros(1, 2, h, w, device=p.device)
        else:
            sy, sx = h / flow.shape[2], w / flow.shape[3]
            flow = F.interpolate(flow, size=(h, w), mode="bilinear", align_corners=False) * th.tensor([sx, sy], device=p.device).view(1, 2, 1, 1)
        flow = torch_level(F, th, p[:1], p[1:], flow, iters, R)
    return flow


def torch_warp_flow(F, th, src, flow, back, fallback, blend, alpha=0.01, beta=0.5):
    _, _, H, W = src.shape
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float32, device=src.device), th.arange(W, dtype=th.float32, device=src.device), indexing="ij")
    sx, sy = xs + flow[0, 0], ys + flow[0, 1]
    grid = th.stack([sx * (2 / (W - 1)) - 1, sy * (2 / (H - 1)) - 1], dim=-1)[None]
    out = F.grid_sample(src, grid, mode="bicubic", padding_mode="border", align_corners=True).clamp(-1, 1)
    w = blend
    if back is not None:
        fb = F.grid_sample(back, grid, mode="bilinear", padding_mode="border", align_corners=True)
        lhs = (flow + fb).pow(2).sum(1, keepdim=True)
        rhs = alpha * (flow.pow(2).sum(1, keepdim=True) + fb.pow(2).sum(1, keepdim=True)) + beta
        ok = (lhs <= rhs) & ((sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1))[None, None]
        w = blend * ok.float()
    return w * out + (1 - w) * fallback


def clip_frames(th, n, dev, shift=(2.3, -1.7)):
    """two (1,3,n,n) frames of a smooth texture, the second shifted"""
    ys, xs = th.meshgrid(th.arange(n, dtype=th.float32, device=dev), th.arange(n, dtype=th.float32, device=dev), indexing="ij")
    g = th.Generator().manual_seed(3)
    freq, ang, ph = th.rand(24, generator=g) * 0.7 + 0.1, th.rand(24, generator=g) * 2 * math.pi, th.rand(72, generator=g) * 2 * math.pi

    def frame(ox, oy):
        out = []
        for c in range(3):
            t = sum(th.sin(float(freq[i]) * (math.cos(float(ang[i])) * (xs - ox) + math.sin(float(ang[i])) * (ys - oy)) + float(ph[24 * c + i]))
                    for i in range(24))
            out.append(t / 8)
        return th.stack(out)[None].clamp(-1, 1).contiguous()

    return frame(0.0, 0.0), frame(*shift)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launch-iters", type=int, default=50)
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
    before, now = clip_frames(th, H, dev)
    state = {"prev": th.tanh(th.randn(1, 3, H, W, generator=th.Generator().manual_seed(5))).to(dev)}
    stats0 = ops.channel_stats(ctx, state["prev"])
    launches = {}

    def run(mode):
        kw = dict(clip_denoised=False, cond_fn=guid, model_kwargs=dict(y), device=dev, randomize_class=True, cond_fn_with_grad=True)
        th.cuda.synchronize()
        n0 = steplib.launch_count(ctx)
        if mode == "frame_k_2d":
            init = ops.frame_warp(ctx, state["prev"], matrix, interp="bicubic", border="replicate", clamp=True)
        else:
            flow = ops.flow_estimate(ctx, now, before)
            back = ops.flow_estimate(ctx, before, now) if mode == "frame_k_video_checked" else None
            init = ops.frame_warp_flow(ctx, state["prev"], flow, flow_back=back, fallback=now, blend=0.999, interp="bicubic", border="replicate",
                                       clamp=True)
        n1 = steplib.launch_count(ctx)
        ops.color_match(ctx, init, stats0, amount=1.0, clamp=True)
        guid.set_init(init, 1500, lpips=lpips)
        kw.update(init_image=init, skip_timesteps=skip)
        guid.current_timestep = smp.num_timesteps - 1
        t, n, out = steplib.drain(smp.p_sample_loop_progressive(unet, (1, 3, H, W), **kw), guid)
        launches[mode] = {"frame": steplib.launch_count(ctx) - n0, "motion": n1 - n0}
        return t, n, bool(th.isfinite(out["sample"]).all())

    modes = ["frame_k_2d", "frame_k_video", "frame_k_video_checked"]
    res = steplib.alternate(modes, run, args.runs)
    sec = {m: [v[0] for v in r] for m, r in res.items()}
    steps = {m: r[-1][1] for m, r in res.items()}
    finite = {m: all(v[2] for v in r) for m, r in res.items()}

    fns, keep = {}, []  # (keep: the tensors whose pointers the closures hold)
    lib, h, s_ = ctx.lib, ctx.h, ctx.stream()
    p = L.FlowParams(4, 4, 4, 1e-3, 1.0)
    for n in (256, 512):
        a, b = clip_frames(th, n, dev)
        flow, back = ops.flow_estimate(ctx, b, a), ops.flow_estimate(ctx, a, b)
        err = float((flow[0, :, 16:-16, 16:-16] - th.tensor([-2.3, 1.7], device=dev).view(2, 1, 1)).abs().median())
        terr = float((torch_flow(F, th, b, a)[0, :, 16:-16, 16:-16] - th.tensor([-2.3, 1.7], device=dev).view(2, 1, 1)).abs().median())
        assert err < 0.1 and terr < 0.1, (n, err, terr)  # both estimators find the shift
        scratch = th.empty(lib.cgd_flow_scratch_floats(1, n, n, 4, 4), device=dev)
        out = th.empty_like(flow)
        luma = th.tensor([0.2989, 0.587, 0.114], device=dev).view(1, 3, 1, 1)
        pb, pa = (b * luma).sum(1).contiguous(), (a * luma).sum(1).contiguous()
        coarse = F.interpolate(flow, size=(n // 2, n // 2), mode="bilinear", align_corners=False).mul(0.5).contiguous()
        src, fb, dst = th.randn(1, 3, n, n, device=dev).clamp(-1, 1), b, th.empty(1, 3, n, n, device=dev)
        fns[f"cgd_flow_estimate_{n}"] = (lambda t=b.data_ptr(), i=a.data_ptr(), o=out.data_ptr(), sc=scratch.data_ptr(), n=n:
                                         lib.cgd_flow_estimate(h, t, i, o, sc, 1, 3, n, n, ctypes.byref(p), s_))
        fns[f"cgd_op_flow_level_{n}"] = (lambda t=pb.data_ptr(), i=pa.data_ptr(), c=coarse.data_ptr(), o=out.data_ptr(), n=n:
                                         lib.cgd_op_flow_level(h, t, i, c, n // 2, n // 2, o, 1, n, n, ctypes.byref(p), s_))
        fns[f"torch_flow_{n}"] = lambda t=b, i=a: torch_flow(F, th, t, i)
        fns[f"torch_flow_level_{n}"] = (lambda t=pb[None], i=pa[None], c=coarse, n=n:
                                        torch_level(F, th, t, i, F.interpolate(c, size=(n, n), mode="bilinear", align_corners=False) * 2))
        for name, bk in (("", None), ("_checked", back)):
            w = L.WarpFlow(0.999, 0.01, 0.5, 1, 2, 1)
            fns[f"cgd_frame_warp_flow{name}_{n}"] = (lambda s=src.data_ptr(), f=flow.data_ptr(), k=(None if bk is None else bk.data_ptr()), fb=fb.data_ptr(),
                                                     d=dst.data_ptr(), w=w, n=n:
                                                     lib.cgd_frame_warp_flow(h, s, f, k, fb, d, None, 1, 1, 3, n, n, ctypes.byref(w), s_))
            fns[f"torch_warp_flow{name}_{n}"] = lambda s=src, f=flow, k=bk, fb=fb: torch_warp_flow(F, th, s, f, k, fb, 0.999)
        keep.append((a, b, flow, back, scratch, out, pb, pa, coarse, src, dst))
    for name, fn in fns.items():  # every C entry accepts its arguments
        rc = fn()
        assert not isinstance(rc, int) or rc == 0, (name, rc)
    call_us = steplib.per_launch(fns, args.launch_iters, args.launch_repeats)
    med = {m: statistics.median(v) for m, v in sec.items()}
    print(json.dumps({"what": "seconds per animation frame k > 0, bench.py config 2 (256x256, cutn 16, ViT-B/32, batch 1, synthetic weights, -respace 250): "
                              f"warp + colour match + {steps['frame_k_video']} steps (frames_skip 0.6) with the LPIPS term, 2D warp against flow "
                              f"estimate + flow warp, without and with the consistency check; median of {args.runs} alternating runs",
                      "seconds_per_frame": {m: round(v, 3) for m, v in med.items()}, "runs_s": {m: [round(t, 3) for t in v] for m, v in sec.items()},
                      "steps": steps, "finite": finite, "launches_per_frame": launches, "call_us": {n: steplib.stats(v) for n, v in call_us.items()},
                      "device": th.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
