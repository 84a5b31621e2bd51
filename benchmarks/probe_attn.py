"""Probe: the fused attention kernels on the UNet's three attention shapes (T = 1024 / 256 / 64 at 8 / 16 / 16 heads of 64) and the
ViT-B/32 shape (16 x 50 tokens, 12 heads), forward + backward, timed with HIP events; a target for rocprofv3 --pmc passes
(benchmarks/pmc_probe.sh).  Usage: python benchmarks/probe_attn.py [iters] [--shape nb,heads,T,d,legacy ...] [--repeats R]
[--tower ARCH N]

--shape replaces the default shapes (e.g. --shape 16,16,257,80,0: open_clip ViT-H-14 at cutn 16).  --repeats R times every entry R times and
prints the median with the spread (min .. max) of those runs: an A/B between two builds is a difference only beyond that spread.
--tower ARCH N times forward + dgrad of a synthetic-weight open_clip image tower (cgd_amd.nets.OPENCLIP_CONFIGS) on N images the same way."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

import cgd_amd  # noqa: E402,F401
from cgd_amd import lib, nets, ops, synthetic  # noqa: E402

DEFAULT_SHAPES = [(1, 8, 1024, 64, 1), (1, 16, 256, 64, 1), (1, 16, 64, 64, 1), (16, 12, 50, 64, 0)]


def timed_us(fn, iters, repeats):
    """[microseconds per call] of `repeats` runs of `iters` back-to-back calls (HIP events), after three warm-up calls"""
    for _ in range(3):
        fn()
    th.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        th.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / iters)
    return out


def show(us):
    med = statistics.median(us)
    return f"{med:8.1f} us" + (f"  (min {min(us):.1f} .. max {max(us):.1f} over {len(us)} runs)" if len(us) > 1 else "")


def main(argv):
    iters, repeats, shapes, tower = 20, 1, [], None
    args = list(argv)
    while args:
        a = args.pop(0)
        if a == "--shape":
            shapes.append(tuple(int(v) for v in args.pop(0).split(",")))
        elif a == "--repeats":
            repeats = int(args.pop(0))
        elif a == "--tower":
            tower = (args.pop(0), int(args.pop(0)))
        else:
            iters = int(a)
    ctx = lib.Context(0, 1)
    for (nb, heads, T, d, legacy) in (shapes or ([] if tower else DEFAULT_SHAPES)):
        C = heads * d
        qkv = th.randn(nb * T, 3 * C, device="cuda")
        dout = th.randn(nb * T, C, device="cuda")
        at = ops.Attention(ctx, nb, heads, T, d, legacy=bool(legacy), device="cuda")
        total = 0.0
        for name, fn in (("fwd", lambda: at.forward(qkv)), ("bwd", lambda: at.backward(qkv, dout))):
            if name == "bwd":
                at.forward(qkv)
            us = timed_us(fn, iters, repeats)
            med = statistics.median(us)
            total += med
            flop = (4.0 if name == "fwd" else 10.0) * nb * heads * T * T * d
            print(f"attn {name} nb{nb} h{heads} T{T} d{d}: {show(us)}  {flop / med / 1e6:7.1f} TFLOP/s", flush=True)
        print(f"attn fwd+bwd nb{nb} h{heads} T{T} d{d}: {total:8.1f} us (sum of the medians)", flush=True)
    if tower:
        arch, N = tower
        cfg = nets.OPENCLIP_CONFIGS[arch][0]
        net = nets.ClipImageTower(ctx, config=cfg, activation="gelu")
        net.load_state_dict(synthetic.synthetic_state_dict(net, seed=4321, device="cuda"))
        img = th.randn(N, 3, cfg[0], cfg[0], device="cuda")
        demb = th.randn(N, cfg[5], device="cuda")

        def step():
            net.encode_image(img)
            net.dgrad(demb)

        print(f"tower {arch} N{N} forward + dgrad: {show(timed_us(step, max(1, iters // 4), repeats))}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
