"""Plan coverage of the community checkpoints' network (CPU, `not gpu`), in the style of tests/plan_dump.py: the float reference of the real
COMMUNITY_LOOKUP flags (tests/classic_unet_ref.COMICS, conv resampling, additive embedding) runs on the meta device at 256 x 256, B = 1, with
hooks that record every contraction launch, forward and backward to the input; the launchers' host-only plan entries say what each one runs:
    3x3 conv                cgd_op_plan_conv  (kernel, tile code, slices), with the input upsampled or not (Upsample.conv)
    1x1 conv / linear       cgd_op_plan       (kernel, tile code, slices)
    Downsample              cgd_op_plan_conv_s2 (tile rows, slices), forward and backward
    attention               cgd_op_attn_plan  (family) and the head dim
Each launch is reduced to its CLASS, and every class must appear in a row of a GPU table (the shape-edge table, test_gpu_sconv.py's shapes) or
in the launch plan of a network case of tests/test_gpu_classic_unet.py at its own frame (the narrow structure at 32 x 32, 64 x 96, 128 x 128 and
the real flags at 128 x 128), so that no kernel x tile x split combination the checkpoints run at their native frame goes ungraded.

Restated, not read back: the 3x3 convs are planned without the GroupNorm-record requests (stats, gnb) the ResBlocks add; both only move a launch
between tiles of the same kernel."""
import ctypes as C
from collections import defaultdict

import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib as L
from tests import classic_unet_ref as R
from tests import shape_edge_checks as se

NUM_CU = 256
CONV_NAME = {512: "hconv2", 515: "wconv", 516: "kconv"}


def record(cfg, B, H, W):
    """[(kind, ...)] of every contraction the reference executes, in call order (meta device: nothing is computed)"""
    recs = []

    def hook(mod, inp, out):
        x = inp[0]
        if isinstance(mod, R.Downsample):
            recs.append(("sconv", x.shape[0], x.shape[2], x.shape[3], x.shape[1], out.shape[1]))
        elif isinstance(mod, R.Upsample):
            recs.append(("conv3x3", x.shape[0], out.shape[2], out.shape[3], x.shape[1], out.shape[1], 1))
        elif isinstance(mod, R.AttentionBlock):
            heads = mod.num_heads
            recs.append(("attn", x.shape[0], heads, x.shape[2] * x.shape[3], x.shape[1] // heads))
        elif isinstance(mod, th.nn.Conv2d) and mod.kernel_size == (3, 3):
            if mod.stride == (1, 1) and not getattr(mod, "_resample_owned", False):
                recs.append(("conv3x3", x.shape[0], out.shape[2], out.shape[3], mod.in_channels, mod.out_channels, 0))
        elif isinstance(mod, (th.nn.Conv2d, th.nn.Conv1d)):
            recs.append(("gemm", out.numel() // mod.out_channels, mod.out_channels, mod.in_channels))
        elif isinstance(mod, th.nn.Linear):
            recs.append(("gemm", x.numel() // mod.in_features, mod.out_features, mod.in_features))

    with th.device("meta"):
        net = R.ClassicUNetModel(**cfg, resblock_updown=False, use_scale_shift_norm=False).eval()
    for m in net.modules():
        if isinstance(m, R.Upsample):
            m.conv._resample_owned = True  # (recorded by its owner, with the upsampled-input flag)
    kinds = (R.Downsample, R.Upsample, R.AttentionBlock, th.nn.Conv2d, th.nn.Conv1d, th.nn.Linear)
    hs = [m.register_forward_hook(hook) for m in net.modules() if isinstance(m, kinds)]
    with th.no_grad(), th.device("meta"):
        net(th.empty(B, 3, H, W), th.zeros(B))
    for h in hs:
        h.remove()
    return recs


def classes_of(recs, precision=1):
    """{class: [launch, ...]} over the forward and the backward-to-input launch of every record"""
    h = L.load()
    out = defaultdict(list)
    for r in recs:
        kind = r[0]
        for bwd in (0, 1):
            if kind == "sconv":
                _, B, H, W, Ci, Co = r
                o = (C.c_int * 4)()
                assert h.cgd_op_plan_conv_s2(bwd, B, H, W, Ci, Co, NUM_CU, o) == 0, r
                out[("sconv", "bwd" if bwd else "fwd", f"{o[0]}x{o[1]}", "split" if o[2] > 1 else "one slice")].append((r, tuple(o)))
            elif kind == "conv3x3":
                _, B, H, W, Ci, Co, ups = r
                if bwd and ups:
                    continue  # (the gradient of an upsampled-input conv is a plain conv followed by the pooling kernel)
                if min(Ci, Co) < 32:  # the stem (3 channels in) and the output conv (6 out) have kernels of their own and no plan entry
                    out[("conv_in" if Ci < 32 else "conv_thin_out", "bwd" if bwd else "fwd")].append((r, ()))
                    continue
                o = (C.c_int * 5)()
                ci, co = (Co, Ci) if bwd else (Ci, Co)
                assert h.cgd_op_plan_conv(B, H, W, ci, co, precision, NUM_CU, 0, 0, 0, o) == 0, r
                name = CONV_NAME.get(o[1], f"igemm{o[1]}") if o[0] == 1 or o[1] in CONV_NAME else f"igemm{o[1]}"
                out[("conv3x3", name, "split" if o[2] > 1 else "one slice", "upsampled input" if ups and not bwd else "plain input")].append((r, tuple(o)))
            elif kind == "gemm":
                _, M, N, K = r
                n_, k_ = (K, N) if bwd else (N, K)
                o = (C.c_int * 4)()
                assert h.cgd_op_plan(0, M, n_, k_, 0, 0, 0, 1, precision, NUM_CU, o) == 0, r
                out[("gemm", f"tile{o[1]}", "split" if o[2] > 1 else "one slice")].append((r, tuple(o)))
            elif not bwd:
                _, nb, heads, T, d = r
                o = (C.c_int * 2)()
                assert h.cgd_op_attn_plan(T, d, 3 * heads * d, heads * d, precision, -1, o) == 0, r
                out[("attn", ("generic", "s64", "mid", "flash")[o[0]], f"d{d}")].append((r, tuple(o)))
    return out


def table_classes():
    """{class: where} of the GPU tables' rows in a bf16x3 context (the forced tile codes of the shape-edge table, its stride-2 conv and attention
    rows, the shapes of tests/test_gpu_sconv.py)"""
    from tests import test_gpu_sconv as ts
    cov = {}

    def put(cls, where):
        cov.setdefault(cls, where)

    for row in se.TABLE:
        s = row.spec
        if row.verdict != "run" or not any(se.CONTEXTS[ck][0] == 1 for ck in row.ctxs):
            continue
        where = f"shape edges: {row.name}"
        sk = "split" if s.get("sk", 1) > 1 else "one slice"
        if row.op == "gemm" and s["tile"]:
            put(("gemm", f"tile{s['tile']}", sk), where)
        elif row.op == "conv" and s["tile"] in CONV_NAME and not s["dgrad"]:
            put(("conv3x3", CONV_NAME[s["tile"]], sk, "upsampled input" if s["ups"] else "plain input"), where)
        elif row.op == "conv" and s["tile"] in CONV_NAME:
            put(("conv3x3", CONV_NAME[s["tile"]], sk, "plain input"), where)
        elif row.op == "wino":
            put(("conv3x3", "wconv", "one slice", "upsampled input" if s["ups"] else "plain input"), where)
        elif row.op == "sconv":
            p = se.sconv_plan(s["dgrad"], s["B"], s["H"], s["W"], s["Ci"], s["Co"])
            put(("sconv", "bwd" if s["dgrad"] else "fwd", f"{p['bm']}x{p['bn']}", "split" if p["sk"] > 1 else "one slice"), where)
        elif row.op == "attn" and not s["causal"]:
            fam = se.attn_family(s["T"], s["d"], "p1")
            put(("attn", ("generic", "s64", "mid", "flash")[fam], f"d{s['d']}"), where)
    for (B, H, W, Ci, Co, _, _) in ts.SHAPES + [(1, 258, 258, 96, 96, 0, 0)]:
        for dgrad in (0, 1):
            p = se.sconv_plan(dgrad, B, H, W, Ci, Co)
            put(("sconv", "bwd" if dgrad else "fwd", f"{p['bm']}x{p['bn']}", "split" if p["sk"] > 1 else "one slice"), f"test_gpu_sconv.py: B{B} {H}x{W} {Ci}->{Co}")
    return cov


# the network cases of tests/test_gpu_classic_unet.py at precision 1, each at its own frame
NETWORK_CASES = [("narrow", 2, 32, 32), ("narrow", 2, 64, 96), ("narrow", 1, 128, 128), ("comics", 1, 128, 128)]


def network_classes():
    cov = {}
    for case, B, H, W in NETWORK_CASES:
        for cls in classes_of(record(R.CASES[case], B, H, W)):
            cov.setdefault(cls, f"network case: {case} B{B} {H}x{W}")
    return cov


def test_every_launch_class_of_the_community_net_at_256_is_graded_somewhere():
    want = classes_of(record(R.COMICS, 1, 256, 256))
    tables, nets = table_classes(), network_classes()
    uncovered = []
    for cls in sorted(want):
        where = tables.get(cls) or nets.get(cls)
        r, o = want[cls][0]
        print(f"{' / '.join(cls):<58s} {len(want[cls]):>3d} launches, e.g. {r} -> {o}: {where or 'NOT COVERED'}")
        if not where:
            uncovered.append(cls)
    assert not uncovered, uncovered


def test_the_recorder_sees_the_structure_of_the_checkpoints():
    recs = record(R.COMICS, 1, 256, 256)
    downs = [r for r in recs if r[0] == "sconv"]
    assert [(r[2], r[4]) for r in downs] == [(256, 128), (128, 128), (64, 256), (32, 256), (16, 512)]
    attn = [r for r in recs if r[0] == "attn"]
    # one head of 512 channels over the 16 x 16 map (five blocks) and, in the middle block, over the 8 x 8 map
    assert [r[1:] for r in attn] == [(1, 1, 256, 512)] * 2 + [(1, 1, 64, 512)] + [(1, 1, 256, 512)] * 3
    assert sum(1 for r in recs if r[0] == "conv3x3" and r[6]) == 5
    half = [r for r in record(R.COMICS, 1, 128, 128) if r[0] == "attn"]
    assert {r[1:] for r in half} == {(1, 1, 64, 512), (1, 1, 16, 512)}
