"""What the benchmarks/*_step.py scripts share: the networks of bench.py config 2 on cuda:0, timed draining of a sampling generator,
alternating runs over modes, per-launch timing from HIP events, and the median / min / max of a list.  Each script keeps its modes, its
launch closures and its JSON keys.  Seeding: every mode's warm-up run starts from seed 1000 and every timed run of round r from 2000 + r,
so the modes of one round see the same draws."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def setup(**cfg_changes):
    """-> (cfg, ctx, (unet, towers, sampler, guidance, image)): bench.CONFIGS[2] with `cfg_changes`, built on cuda:0"""
    import bench
    import cgd_amd  # noqa: F401
    from cgd_amd import lib as L
    cfg = dict(bench.CONFIGS[2], **cfg_changes)
    ctx = L.Context(0, 1)
    return cfg, ctx, bench.build_device(ctx, cfg, DEV)


def launch_count(ctx):
    """kernel launches of the library so far"""
    import ctypes
    c = (ctypes.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(c)
    return int(c[0])


def drain(gen, guid, steps=None):
    """Runs the sampling generator to its end (or `steps` yields), stepping guid.current_timestep down, between two device synchronises.
    -> (seconds, steps yielded, last output)"""
    import torch as th
    th.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    for out in gen:
        guid.current_timestep -= 1
        n += 1
        if n == steps:
            break
    th.cuda.synchronize()
    return time.perf_counter() - t0, n, out


def alternate(modes, run, runs):
    """One untimed warm-up run per mode (buffers, first touch of the kernels), then `runs` rounds over the modes in turn.
    -> {mode: [run(mode) of every round]}"""
    import torch as th
    for m in modes:
        th.manual_seed(1000)
        run(m)
    res = {m: [] for m in modes}
    for r in range(runs):
        for m in modes:
            th.manual_seed(2000 + r)
            res[m].append(run(m))
    return res


def per_launch(fns, iters, repeats):
    """{name: fn} -> {name: [microseconds per call, one figure per repeat]}: 20 warm-up calls each, then the fns in turn, `repeats` times
    (so that a drift of the clocks lands on all of them), HIP events around `iters` back-to-back calls."""
    import torch as th
    for fn in fns.values():
        for _ in range(20):
            fn()
    us = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            e0, e1 = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) / iters * 1e3)
    return us


def stats(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}
