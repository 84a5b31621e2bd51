"""Op-level A/B of the 64x64-level 3x3 convs: hconv2_kernel in two split-K slices followed by the GroupNorm statistics sweep that sums the
slices (what the UNet runs there: gn_stats_partial_kernel + gn_stats_final_kernel) against the unsplit 4x16-pixel x 128-channel tile (cgd_set_hconv
variant bit 3), alone and followed by the GroupNorm statistics of its output (a merge of epilogue records where the launch leaves them, a sweep
otherwise).  Alternating runs on one device; median [min .. max] in microseconds per launch (pair).
Usage: python benchmarks/bench_hconv_unsplit.py [rounds] [json]   -> table on stdout; every run's figure to the file `json` if one is named."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch as th  # noqa: E402

import cgd_amd  # noqa: E402,F401
from cgd_amd import lib as L  # noqa: E402
from cgd_amd import ops  # noqa: E402

H = W = 64
SHAPES = [(512, 512), (768, 512), (1024, 512)]  # (K channels in, N channels out) of BASELINE config 2's 64x64 level
N_ITER = 20


def timed(fn):
    e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N_ITER):
        fn()
    e1.record()
    th.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / N_ITER


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    json_path = sys.argv[2] if len(sys.argv) > 2 else None
    ctx = L.Context(0, 1)
    lib = ctx.lib
    res = []
    fmt = lambda v: f"{statistics.median(v):6.1f} [{min(v):5.1f} .. {max(v):5.1f}]"  # noqa: E731
    print(f"{'case':<26s}{'A: 2 slices + stats sweep':>28s}{'B: unsplit conv alone':>28s}{'B + stats of its output':>28s}", flush=True)
    for (K, N) in SHAPES:
        for dgrad in (0, 1):
            for gn in (0, 1):
                x = th.randn(1, H, W, K, device="cuda")
                wt = th.randn(*((K, N) if dgrad else (N, K)), 3, 3, device="cuda") * 0.02
                wf, wd = ops.pack_conv3x3(wt)
                wp = wd if dgrad else wf
                wfrag = ops.pack_conv3x3_frag(ctx, wt, dgrad=bool(dgrad))
                bias = th.randn(N, device="cuda")
                ab = th.stack([1 + 0.1 * th.randn(K, device="cuda"), 0.1 * th.randn(K, device="cuda")], -1).contiguous()
                y = th.empty(1, H * W, N, device="cuda")
                gamma, beta = th.ones(N, device="cuda"), th.zeros(N, device="cuda")
                scr = ops.gn_scratch(ctx, 1, H * W, N, "cuda")
                pab = ab.data_ptr() if gn else None

                def conv(defer, stats):
                    ctx.check(lib.cgd_op_conv3x3_ex(ctx.h, x.data_ptr(), K, wp.data_ptr(), wfrag.data_ptr(), y.data_ptr(), N, bias.data_ptr(), None, 0,
                                                    pab, 1, H, W, K, N, 0, 512, 1, defer, stats, None, 0, None, L.stream_ptr()))

                def gstats():
                    ctx.check(lib.cgd_op_gn_fwd(ctx.h, y.data_ptr(), N, None, 0, 1, H * W, N, gamma.data_ptr(), beta.data_ptr(), None, 1, 1e-5,
                                                scr.data_ptr(), L.stream_ptr()))

                def pair_a():
                    conv(1, 0)
                    gstats()

                def pair_b():
                    conv(0, 1)
                    gstats()

                ta, tb, tbp = [], [], []
                for r in range(rounds + 1):
                    ctx.check(lib.cgd_set_hconv(ctx.h, 1, 256))
                    a = timed(pair_a)
                    ctx.check(lib.cgd_set_hconv(ctx.h, 1 + 16 * 8, 256))
                    b = timed(lambda: conv(0, 0))
                    bp = timed(pair_b)
                    if r:  # round 0 warms up
                        ta.append(a)
                        tb.append(b)
                        tbp.append(bp)
                ctx.check(lib.cgd_set_hconv(ctx.h, 1, 256))
                name = f"{K:>4d}->{N} {'dgrad' if dgrad else 'fwd  '} {'gn' if gn else 'plain'}"
                print(f"{name:<26s}{fmt(ta):>28s}{fmt(tb):>28s}{fmt(tbp):>28s}", flush=True)
                res.append({"K": K, "N": N, "dgrad": dgrad, "gn": gn, "a_pair_us": ta, "b_conv_us": tb, "b_pair_us": tbp})
    if json_path:
        with open(json_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
