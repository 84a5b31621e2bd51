"""Scratch and saved state at their exact size, guarded and poisoned (tests/test_gpu_scratch.py, tests/test_scratch_host.py).

Every other GPU tier grades OPERANDS.  This one grades the buffers the kernels own between and inside calls: the scratch a caller sizes with
a `*_scratch_floats` / `*_buf_floats` / `*_scratch_bytes` query, the state a forward leaves for its backward, and the partial / result
buffers whose size the header states.  Per case:
- allocation: every such buffer is a `Scratch`: a 1-D `strided_checks.Guarded` view of EXACTLY the floats the size query returns for that
  call's own arguments, with as many guard floats on either side (at least 4096).  A buffer whose query returns 0 is a pointer into the
  middle of a poisoned 8193-float arena that must stay whole; where the networks hand a kernel NULL (the attention forward's Pt / dP / dAt)
  the case hands it NULL.  No buffer is ever smaller than its query says: an overrun shows as a damaged guard, never as a fault;
- two runs: view and guards are filled with the quiet-NaN bits 0x7FC0BEEF, then with the finite 1.0e6 (a stale read that a fmaxf or a select
  swallows shows as a bit difference between the runs).  A forward / backward pair is poisoned once, before the forward;
- verdicts per run, all four required for every row: every guard bit-intact (`guards`), every output strict against the float64 / oracle
  reference the entry's own test uses (`parity`: `rec`, the literal 1e-4 + 1e-3 |ref|, backward seeds at unit peak), outputs bit-equal
  between the runs (`rerun`), and the kernel family or route the row claims (`route`: the sizes the context reports, cgd_op_attn_plan, the
  launch profile).
Operands keep the Guarded treatment of the shape-edge runners.  One TABLE drives the GPU file and the host file; `closed_form` restates every
size query in plain integer arithmetic."""
import contextlib
import ctypes as C
import functools
import math
import struct
from collections import namedtuple

import torch as th
import torch.nn.functional as F

from tests import shape_edge_checks as se
from tests.parity_checks import DEV, _ctx, _flag, g, rec, unit_seed
from tests.strided_checks import GAP, HALO, OUT_BITS, Guarded, _conv_ref, _gn_ref, _routes, _s

POISON_NAN_BITS = 0x7FC0BEEF
POISON_FINITE = 1.0e6
POISON_FINITE_BITS = struct.unpack("<i", struct.pack("<f", POISON_FINITE))[0]
POISON_BITS = (POISON_NAN_BITS, POISON_FINITE_BITS)
MIN_GUARD = 4096
VERDICTS = {"guards", "parity", "rerun", "route"}

CONTEXTS = dict(se.CONTEXTS, p1_flash3=(1, {"CGD_ATTN_FLASH": "3"}))
ATTN_CTXS = se.ATTN_CTXS

Row = namedtuple("Row", "fam op name ctxs spec")
Out = namedtuple("Out", "label G ref poison cols allow_small grade", defaults=(True, None, False, True))


def ceil_div(a, b):
    return -(-a // b)


class Scratch:
    """`n` floats, exactly, inside a guarded allocation: n guard floats on either side, at least MIN_GUARD, the view 16-byte aligned.
    n = 0: a pointer into the middle of a 2 * MIN_GUARD + 1 float arena, all of which must stay as poisoned."""

    def __init__(self, n, name="scratch", device=DEV):
        self.n, self.name = int(n), name
        assert self.n >= 0, (name, n)
        if self.n:
            gr = max(1, ceil_div(MIN_GUARD, self.n))
            self.G = Guarded((self.n,), guard_rows=gr, off=(-gr * self.n) % 4, device=device)
        else:
            self.G = Guarded((1,), guard_rows=MIN_GUARD, device=device)
        self.guard = (self.G.buf.numel() - max(self.n, 1)) // 2

    @property
    def ptr(self):
        return self.G.ptr

    @property
    def view(self):
        return self.G.view

    def poison(self, k):
        if k == 0:
            self.G.poison(POISON_NAN_BITS)
        else:
            self.G.buf.fill_(POISON_FINITE)

    def intact(self, k):
        return self.G.intact(POISON_BITS[k], whole=self.n == 0)


def bits_equal(a, b):
    return th.equal(a.contiguous().view(th.int32), b.contiguous().view(th.int32))


def _tag(recs, row, verdict):
    return [dict(r, row=row.name, verdict=verdict) for r in recs]


def protocol(row, scratches, inputs, outputs, launch, route, extra=()):
    """The two poisoned runs of one row.  scratches [Scratch]; inputs [(Guarded, values)], reloaded before each run (in / out operands are
    listed here AND as an Out with poison=False); outputs [Out]; launch() -> launches per profiled kind, runs the row's whole call
    sequence (forward, then backward) once; route (text, predicate on the counts); extra: further route flags [(text, bool)]."""
    recs, runs = [], []
    for k in range(2):
        for s in scratches:
            s.poison(k)
        for G, t in inputs:
            G.load(t, GAP[k])
        for o in outputs:
            if o.poison and isinstance(o.G, Guarded):
                o.G.poison(OUT_BITS[k])
        counts = launch()
        th.cuda.synchronize() if th.cuda.is_available() else None
        got = [o.G.view.clone() for o in outputs]
        runs.append(got)
        par = []
        for o, t in zip(outputs, got):
            if not o.grade:
                continue
            a, b = (t, o.ref) if o.cols is None else (t[:, o.cols.to(t.device)], o.ref[:, o.cols])
            par.append(rec(f"{row.name} {o.label} (run {k})", a, b, allow_small=o.allow_small))
        recs += _tag(par, row, "parity")
        recs += _tag([_flag(f"{row.name}: guards of {s.name} [{s.n} floats, {s.guard} guard floats a side] intact (run {k})", s.intact(k))
                      for s in scratches], row, "guards")
        recs += _tag([_flag(f"{row.name} {o.label}: nothing written outside the view (run {k})",
                            o.G.intact(OUT_BITS[k]) if o.poison else o.G.intact(struct.unpack("<i", struct.pack("<f", GAP[k]))[0]))
                      for o in outputs if isinstance(o.G, Guarded)], row, "guards")
        if k == 0:
            desc, pred = route
            recs += _tag([_flag(f"{row.name}: route {desc} (launches per kind {counts})", pred(counts))]
                         + [_flag(f"{row.name}: {text}", ok) for text, ok in extra], row, "route")
    recs += _tag([_flag(f"{row.name}: outputs bit-equal between the NaN-poisoned and the 1e6-poisoned run",
                        all(bits_equal(a, b) for a, b in zip(*runs)))], row, "rerun")
    return recs


NO_CONV = ("no conv kernel", lambda c: all(c[j] == 0 for j in HALO))
NO_KIND = ("no profiled kind", lambda c: sum(c) == 0)
GN_KIND = ("groupnorm, no GEMM", lambda c: c[2] >= 1 and c[0] == 0)


def profiled(ctx, fn):
    return lambda: _routes(ctx, fn)


# ---- closed forms of the size queries (plain integers; the host file compares them with the library at every row) ------------------------
def attn_tp(T):
    return (T + 3) & ~3


def attn_family_of(T, d, prec, env):
    """restatement of attn.hip attn_select for a dense op-level call: 0 generic, 1 s64, 2 mid, 3 flash"""
    x3 = prec == 1 and env.get("CGD_ATTN_X3", "1") != "0"
    flash = int(env.get("CGD_ATTN_FLASH", "3"))
    if x3 and d in (64, 80) and ((T > 64 and flash >= 1) or (32 < T <= 64 and flash >= 2)):
        return 3
    if d == 64:
        return 1 if T <= 64 else 2
    return 0


def attn_sizes(fam, nb, heads, T, d):
    """floats of (qkvT, P, Pt, dP, dAt) per kernel family (attn.hip cgd_attn_buf_floats)"""
    Tp, Cc = attn_tp(T), heads * d
    probs = nb * heads * T * Tp
    if fam == 3:
        return [nb * T * Cc, 2 * nb * heads * 32 * ceil_div(T, 32), 0, 0, 0]
    if fam == 1:
        return [0, probs, 0, 0, 0]
    if fam == 2:
        return [nb * 3 * Cc * Tp, probs, 0, probs, 0]
    return [nb * 3 * Cc * Tp, probs, probs, probs, nb * Cc * Tp]


def attn_upper(nb, heads, T, d):
    Tp, Cc = attn_tp(T), heads * d
    return [nb * 3 * Cc * Tp] + [nb * heads * T * Tp] * 3 + [nb * Cc * Tp]


def gn_nchunk(B, HW):
    return ceil_div(HW, se.gn_chunk(HW, B))


def gn_sizes(B, HW, Cc):
    """part | stats | coef | bcoef | ab (norm.hip gn_layout): total, and the float offsets of stats, coef and ab"""
    part = B * gn_nchunk(B, HW) * 64
    return dict(total=part + B * 64 + B * Cc * 8 + B * Cc * 2, stats=part, coef=part + B * 64, ab=part + B * 64 + B * Cc * 8)


def r4(n):
    return (n + 3) & ~3


def attnpool_size(B, S, Cc, d, out):
    T, heads, outP = S * S + 1, Cc // d, r4(out)
    regions = [B * T * Cc, B * Cc, B * T * 2 * Cc, B * heads * T, B * Cc, B * outP, B, 2 * B, B * outP, B * Cc, B * Cc, B * T * 2 * Cc, B * T * Cc,
               B * Cc]
    return sum(r4(n) for n in regions) + r4(T * Cc) + r4(3 * Cc * Cc) + r4(Cc * outP)


def rows_per_launch(B, cutn):
    return min(max(cutn, 1), 65535 // B)


def cutaug_size(B, H, W, cutn):
    return 2 * rows_per_launch(B, cutn) * B * 3 * H * W if min(B, H, W, cutn) > 0 else 0


def cutresize_size(B, H, W, cutn):
    return rows_per_launch(B, cutn) * B * 3 * H * W if min(B, H, W, cutn) > 0 and B <= 65535 else 0


def ilvr_size(B, H, W, N, with_x0):
    ok = 2 <= N <= 64 and N & (N - 1) == 0 and H % N == 0 and W % N == 0
    return (2 if with_x0 else 1) * B * 3 * (H // N) * (W // N) if ok else 0


QUANTILE_SLICE = 4096


def quantile_bytes(B, n):
    S = ceil_div(n, QUANTILE_SLICE)
    return 4 * (2 * B * S * 256 + 6 * B + B * S)


def part_blocks(B, H, W):
    return min(ceil_div(B * 3 * H * W, 256), 1024)


def cutout_bounds_ok(kind, B, H, W, cutn, cs):
    """restatement of check_shape of cutaug.hip (:334) / cutresize.hip (:235) for layout 0"""
    lim = 2 ** 31 - 1
    if min(B, H, W, cs) <= 0 or cutn < 0 or B > 65535:
        return False
    both = B * 3 * H * W <= lim and cs * cs * 3 * B * max(cutn, 1) <= lim
    if kind == "aug":
        return both and (cs + 1) * max(H, W) <= lim and cutn * B * 3 * H * W <= lim and H * W * 8 <= lim  # (GA_SUB = 8)
    return both and 8 * cs * max(H, W, cs) <= lim and H * W * 8 <= lim  # (RS_GATHER_SUB = 8)


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
BIG_CUT = dict(B=3, H=4, W=4, cutn=21846, cs=2)  # 65535 // 3 = 21845 rows per launch: two runs of 21845 + 1 cutouts


def _attn_rows():
    rows = []

    def add(nb, heads, T, d, legacy, causal=0, ctxs=ATTN_CTXS):
        name = f"attn{' causal' if causal else ''} nb{nb} h{heads} T{T} d{d} legacy{legacy}" + (" flash3" if ctxs == ("p1_flash3",) else "")
        rows.append(Row("attn", "attn", name, ctxs, dict(nb=nb, heads=heads, T=T, d=d, legacy=legacy, causal=causal)))

    for T in (1, 7, 31, 32, 33, 63, 64, 65, 96, 97, 129):
        for (nb, heads) in ((1, 1), (2, 3)):
            for legacy in (0, 1):
                add(nb, heads, T, 64, legacy)
    for T in (33, 65):
        add(2, 3, T, 80, 0)
    for i, d in enumerate((32, 128)):
        for T in (5, 65):
            add(2, 2, T, d, i & 1)  # the generic family: all five buffers
    for T in (33, 65):
        add(2, 3, T, 64, 0, causal=1)
    for T in (255, 256, 257):  # one head of 512 channels (the classic architecture's community checkpoints at 256 x 256): generic, all five buffers
        for nb in (1, 2):
            for legacy in (0, 1):
                add(nb, 1, T, 512, legacy)
    for T in (33, 64):  # the one-workgroup backward: statistics rows of Tq = 64
        add(2, 3, T, 64, 0, ctxs=("p1_flash3",))
    return rows


def _norm_rows():
    rows = []

    def gn(B, HW, Cc, bwd=1):
        k = se.gn_kernel(HW, Cc)
        fam = "chunked" if k == "chunked" else "-".join(k)
        rows.append(Row("gn", "gn", f"gn B{B} HW{HW} C{Cc} [{fam}]" + ("" if bwd else " fwd only"), ("p1",), dict(B=B, HW=HW, C=Cc, bwd=bwd)))

    gn(1, 64, 64)  # the issue's shapes, named by what norm.hip runs on them
    gn(1, 1152, 64)
    gn(1, 64, 96)
    gn(2, 1050, 64)  # chunk 8: 132 chunks, the last one holds 2 pixels
    gn(1, 64, 128)  # float4, register-cached
    gn(1, 257, 4096)  # float4, streaming
    gn(1, 524288, 32, bwd=0)  # exactly 2048 chunks of 256 pixels
    rows.append(Row("gn", "gn_ab", "gn statistics only -> gn_ab of cgd_op_conv3x3_ex (hconv2) B1 16x16 C64", ("p1",), dict(B=1, H=16, W=16, C=64, Co=64)))
    rows.append(Row("gn", "gn_gnb", "gn forward -> gnb_scratch of the Winograd dgrad conv -> gn backward merges B1 64x64 C64", ("p1",),
                    dict(B=1, H=64, W=64, C=64)))
    for r in (1, 5, 50):
        for Cc in (256, 768, 520):
            rows.append(Row("ln", "ln", f"ln {r}x{Cc}", ("p1",), dict(rows=r, C=Cc)))
    return rows


HEADS = {
    "published": dict(B=2, C=512, S=8, d=64, out=1000, y=(3, 997)),
    "small": dict(B=3, C=128, S=4, d=32, out=7, y=(0, 6, 2)),
    "out5": dict(B=1, C=64, S=2, d=32, out=5, y=(4,)),  # out no multiple of 4: the rounded-up regions of the carve
}
RESIZE_RECS = [(0, 0, 56, 40, f) for f in range(4)] + [(3, 5, 20, 20, 1), (20, 4, 36, 36, 2)]  # test_gpu_resize_cutouts.py "40x56-32"


def _other_rows():
    rows = [Row("attnpool", "attnpool", f"attnpool {k}", ("p1",), dict(head=k)) for k in HEADS]
    for kind, ordinary in (("aug", dict(B=2, H=80, W=112, cutn=9, cs=64, layout=1, patch=16)),
                           ("resize", dict(B=2, H=40, W=56, cutn=len(RESIZE_RECS), cs=32, layout=1, patch=16))):
        for acc in (0, 1):
            rows.append(Row("cut" + kind, "cut", f"cutouts_{kind} B2 ordinary acc{acc}", ("p1",), dict(ordinary, kind=kind, acc=acc, big=0)))
            rows.append(Row("cut" + kind, "cut", f"cutouts_{kind} B3 4x4 cutn21846 cs2 (two runs) acc{acc}", ("p1",),
                            dict(BIG_CUT, kind=kind, acc=acc, big=1, layout=0, patch=0)))
    for (shape, N) in (((2, 3, 24, 40), 2), ((2, 3, 24, 40), 4), ((1, 3, 128, 64), 64)):
        for with_x0 in (1, 0):
            for ref_b in sorted({1, shape[0]}):
                rows.append(Row("ilvr", "ilvr", f"ilvr {shape[0]}x{shape[2]}x{shape[3]} N{N} x0{with_x0} ref{ref_b}", ("p1",),
                                dict(B=shape[0], H=shape[2], W=shape[3], N=N, x0=with_x0, ref_b=ref_b)))
    for n in (4095, 4096, 4097, 2 * 4096 + 1):
        for mis in (0, 1):
            rows.append(Row("quantile", "quantile", f"abs_quantile B3 n{n} {'misaligned' if mis else 'aligned'}", ("p1",), dict(B=3, n=n, mis=mis)))
    # cgd_dpmpp_threshold selects over n = 3 H W values: 4096 and 4097 are no multiples of 3.  1365 / 1366 pixels put n either side of one
    # slice, 2731 gives 2 * 4096 + 1, 4096 pixels three whole slices on the vector path
    for HW in (1365, 1366, 2731, 4096):
        for mis in (0, 1):
            rows.append(Row("quantile", "threshold", f"dpmpp_threshold B3 n{3 * HW} {'misaligned' if mis else 'aligned'}", ("p1",),
                            dict(B=3, H=1, W=HW, mis=mis)))
    for shape in ((1, 5, 7), (1, 40, 48), (1, 296, 300)):
        rows.append(Row("partials", "tail", "step tail {}x{}x{}".format(*shape), ("p1",), dict(B=shape[0], H=shape[1], W=shape[2])))
        rows.append(Row("partials", "secondary", "secondary_combine {}x{}x{}".format(*shape), ("p1",), dict(B=shape[0], H=shape[1], W=shape[2])))
    rows.append(Row("partials", "records", "gn_records of the unsplit hconv2 tile B2 32x64 32->128", ("p1",), dict(B=2, H=32, W=64, Ci=32, Co=128)))
    for D in (1, 64, 65, 2048):
        rows.append(Row("partials", "spherical", f"spherical loss cutn3 B2 P2 D{D}", ("p1",), dict(cutn=3, B=2, P=2, D=D)))
        rows.append(Row("partials", "directional", f"directional loss cutn3 B2 Bs1 P2 D{D}", ("p1",), dict(cutn=3, B=2, Bs=1, P=2, D=D)))
    return rows


TABLE = _attn_rows() + _norm_rows() + _other_rows()
GROUPS = sorted({(r.fam, ck) for r in TABLE for ck in r.ctxs})


def rows_of(fam, ck):
    return [r for r in TABLE if r.fam == fam and ck in r.ctxs]


def closed_form(row, ck="p1"):
    """{buffer: floats} of every queried buffer of a row, from the restatements above"""
    s = row.spec
    if row.op == "attn":
        fam = attn_family_of(s["T"], s["d"], *CONTEXTS[ck])
        return dict(zip(("qkvT", "P", "Pt", "dP", "dAt"), attn_sizes(fam, s["nb"], s["heads"], s["T"], s["d"])))
    if row.op == "gn":
        return dict(scratch=gn_sizes(s["B"], s["HW"], s["C"])["total"])
    if row.op in ("gn_ab", "gn_gnb"):
        return dict(scratch=gn_sizes(s["B"], s["H"] * s["W"], s["C"])["total"])
    if row.op == "ln":
        return dict(stats=2 * s["rows"])
    if row.op == "attnpool":
        h = HEADS[s["head"]]
        return dict(scratch=attnpool_size(h["B"], h["S"], h["C"], h["d"], h["out"]))
    if row.op == "cut":
        return dict(scratch=(cutaug_size if s["kind"] == "aug" else cutresize_size)(s["B"], s["H"], s["W"], s["cutn"]))
    if row.op == "ilvr":
        return dict(scratch=ilvr_size(s["B"], s["H"], s["W"], s["N"], s["x0"]))
    if row.op == "quantile":
        return dict(scratch=quantile_bytes(s["B"], s["n"]) // 4, out3=3 * s["B"])
    if row.op == "threshold":
        return dict(scratch=quantile_bytes(s["B"], 3 * s["H"] * s["W"]) // 4, thr3=3 * s["B"])
    if row.op == "tail":
        nb = part_blocks(s["B"], s["H"], s["W"])
        return dict(loss_part=3 * nb, g_part=2 * nb, scalars=8)
    if row.op == "secondary":
        return dict(loss_part=3 * part_blocks(s["B"], s["H"], s["W"]))
    if row.op in ("spherical", "directional"):
        return dict(loss_part=s["cutn"] * s["B"])
    if row.op == "records":  # one (mean, M2) pair per (64-pixel tile, channel)
        return dict(records=s["B"] * s["H"] * s["W"] // 64 * s["Co"] * 2)
    raise KeyError(row.op)


def queried(lib, row, ctx=None):
    """{buffer: floats} as the library reports them; attention needs the context (the family is the context's choice), header-stated sizes
    (LayerNorm statistics, loss partials per row, out3 / thr3, the scalars block) have no query and are not listed"""
    s = row.spec
    if row.op == "attn":
        return {nm: int(lib.cgd_op_attn_buf_floats_ctx(ctx.h, s["nb"], s["heads"], s["T"], s["d"], s["legacy"], s["causal"], i))
                for i, nm in enumerate(("qkvT", "P", "Pt", "dP", "dAt"))}
    if row.op == "gn":
        return dict(scratch=int(lib.cgd_op_gn_scratch_floats(s["B"], s["HW"], s["C"])))
    if row.op in ("gn_ab", "gn_gnb"):
        return dict(scratch=int(lib.cgd_op_gn_scratch_floats(s["B"], s["H"] * s["W"], s["C"])))
    if row.op == "attnpool":
        h = HEADS[s["head"]]
        return dict(scratch=int(lib.cgd_op_attnpool_scratch_floats(h["B"], h["S"], h["C"], h["d"], h["out"])))
    if row.op == "cut":
        fn = lib.cgd_cutouts_aug_scratch_floats if s["kind"] == "aug" else lib.cgd_cutouts_resize_scratch_floats
        return dict(scratch=int(fn(s["B"], s["H"], s["W"], s["cutn"])))
    if row.op == "ilvr":
        return dict(scratch=int(lib.cgd_ilvr_scratch_floats(s["B"], s["H"], s["W"], s["N"], s["x0"])))
    if row.op in ("quantile", "threshold"):
        n = s["n"] if row.op == "quantile" else 3 * s["H"] * s["W"]
        nbytes = int(lib.cgd_abs_quantile_scratch_bytes(s["B"], n))
        assert nbytes % 4 == 0
        return dict(scratch=nbytes // 4)
    if row.op in ("tail", "secondary"):
        nb = int(lib.cgd_guidance_part_blocks(s["B"], s["H"], s["W"]))
        return dict(loss_part=3 * nb, g_part=2 * nb) if row.op == "tail" else dict(loss_part=3 * nb)
    return {}


def sizes_for(ctx, row, ck):
    """the exact sizes a runner allocates: the library's answer where there is a query, the header's text otherwise; the route verdict
    carries the comparison with the closed form"""
    want = closed_form(row, ck)
    got = dict(want, **queried(ctx.lib, row, ctx))
    return got, (f"sizes {got} = the closed form", got == want)


# ---- references shared by the GPU runners and the host file ---------------------------------------------------------------------------------
def _r(shape, seed, scale=1.0):
    return scale * th.randn(*shape, generator=g(seed))


@functools.lru_cache(maxsize=None)
def head_case(name):
    """tests/test_gpu_classifier.py `_head_case` for a shape of HEADS: one CPU forward + backward of AttentionPool2d + log-softmax-select"""
    from tests import classifier_ref as cr
    k = HEADS[name]
    B, Cc, S, d, out = k["B"], k["C"], k["S"], k["d"], k["out"]
    gen = g(700 + Cc)
    pool = cr.AttentionPool2d(S, Cc, d, out)
    with th.no_grad():
        pool.positional_embedding.copy_(th.randn(Cc, S * S + 1, generator=gen) / Cc ** 0.5)
        pool.qkv_proj.weight.copy_(th.randn(3 * Cc, Cc, 1, generator=gen) * 2.0 / Cc ** 0.5)
        pool.qkv_proj.bias.copy_(th.randn(3 * Cc, generator=gen) * 0.1)
        pool.c_proj.weight.copy_(th.randn(out, Cc, 1, generator=gen) * 4.0 / Cc ** 0.5)
        pool.c_proj.bias.copy_(th.randn(out, generator=gen) * 0.1)
    for p in pool.parameters():
        p.requires_grad_(False)
    h = th.randn(B, Cc, S, S, generator=gen)
    y = th.tensor(k["y"])
    hr = h.clone().requires_grad_()
    logits = pool(hr)
    logp = cr.logp_of(logits, y)
    logp.sum().backward()
    with th.no_grad():
        pooled = pool.pooled(h)
    rows = lambda a: a.permute(0, 2, 3, 1).reshape(-1, a.shape[1]).contiguous()  # noqa: E731
    return dict(k, pool=pool, h=rows(h), yt=y, pooled=pooled, logits=logits.detach(), logp=logp.detach(), dh=rows(hr.grad))


def big_cut_boxes(cutn, H, W, cs):
    """(ox, oy, size) of the multi-run row: every size from cs to the frame and every offset, cycled"""
    out = []
    for k in range(cutn):
        size = cs + k % (min(H, W) - cs + 1)
        out.append(((k // 3) % (W - size + 1), (k // 7) % (H - size + 1), size))
    return out


def to_patch_rows(img, P):
    N, Cc, cs, _ = img.shape
    q = cs // P
    return img.reshape(N, Cc, q, P, q, P).permute(0, 2, 4, 1, 3, 5).reshape(N * q * q, Cc * P * P)


@contextlib.contextmanager
def _no_aug_noise():
    from cgd_amd import guidance as dg
    old, dg.AUG_NOISE_STD = dg.AUG_NOISE_STD, 0.0
    try:
        yield
    finally:
        dg.AUG_NOISE_STD = old


IDENTITY_AUG = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0] + [0.0] * 8 + [0.0, 0.0]


@functools.lru_cache(maxsize=None)
def cut_case(kind, big):
    """inputs, tables and references of a cutout row: x (B,3,H,W) in [-1, 1], the cotangent dy at unit-peak gradient, the pre-fill of the
    accumulating adjoint; `geo` int32 table, `par` the 16-float records (aug) -> forward reference, adjoint reference.
    ordinary aug: the torch restatement (guidance.MakeCutouts.augmented, fp32 on the CPU, whose nearest picks the kernels reproduce exactly:
    tests/test_cutaug_host.py) with the parameter draws of seed 7; ordinary resize: tests/resize_ref.py in float64; the multi-run row: identity
    augmentation / plain boxes, the reference computed once per distinct box and indexed."""
    from cgd_amd import guidance as dg
    from tests import resize_ref as R
    mean, std = (th.tensor(c, dtype=th.float64).view(1, 3, 1, 1) for c in (dg.CLIP_MEAN, dg.CLIP_STD))
    if big:
        B, H, W, cutn, cs = (BIG_CUT[k] for k in ("B", "H", "W", "cutn", "cs"))
        boxes = big_cut_boxes(cutn, H, W, cs)
        gen = g(880 + (kind == "aug"))
        x = th.rand(B, 3, H, W, generator=gen) * 2 - 1
        dy = th.randn(cutn * B, 3, cs, cs, generator=gen)
        keys = sorted(set(boxes))
        index = th.tensor([keys.index(b) for b in boxes])
        xr = x.double().requires_grad_()
        x01 = (xr + 1) / 2
        if kind == "aug":
            per = [F.adaptive_avg_pool2d(x01[:, :, oy:oy + sz, ox:ox + sz], cs) for (ox, oy, sz) in keys]
            geo = th.tensor(dg.crop_geometry(boxes, H, W), dtype=th.int32)
            par = th.tensor([IDENTITY_AUG] * cutn, dtype=th.float32)
        else:
            recs = [(ox, oy, sz, sz, 0) for (ox, oy, sz) in boxes]
            per = [R.cutouts(x01, [(ox, oy, sz, sz, 0)], cs) for (ox, oy, sz) in keys]
            geo, par = th.tensor(dg.resize_table(recs, H, W), dtype=th.int32), None
        per = (th.stack(per) - mean) / std  # (keys, B, 3, cs, cs)
        fwd = per[index].reshape(cutn * B, 3, cs, cs)
        dsum = th.zeros(len(keys), B, 3, cs, cs, dtype=th.float64).index_add_(0, index, dy.double().reshape(cutn, B, 3, cs, cs))
        gref, = th.autograd.grad((per * dsum).sum(), xr)
        layout, patch = 0, 0
    elif kind == "aug":
        B, H, W, cutn, cs, layout, patch = 2, 80, 112, 9, 64, 1, 16
        gen = g(109)
        x = th.rand(B, 3, H, W, generator=gen) * 2 - 1
        th.manual_seed(109)
        boxes = dg.generate_coords(H, W, cutn, cs, 1.0)
        th.manual_seed(7)
        geo = th.tensor(dg.crop_geometry(boxes, H, W), dtype=th.int32)
        par = th.tensor([dg.draw_aug_params(h, w).record() for (_, _, h, w) in dg.crop_geometry(boxes, H, W)], dtype=th.float32)
        with _no_aug_noise():
            th.manual_seed(7)
            xr = x.clone().requires_grad_()
            cut = dg.MakeCutouts(cs, cutn, use_augs=True).augmented(xr.add(1).div(2), boxes)
        fwd = (cut - mean.float()) / std.float()
        dy = th.randn(cutn * B, 3, cs, cs, generator=gen)
        gref, = th.autograd.grad((fwd * dy).sum(), xr)
        fwd = fwd.detach()
    else:
        B, H, W, cs, layout, patch = 2, 40, 56, 32, 1, 16
        cutn = len(RESIZE_RECS)
        gen = g(56)
        x = th.rand(B, 3, H, W, generator=gen) * 2 - 1
        dy = th.randn(cutn * B, 3, cs, cs, generator=gen)
        xr = x.double().requires_grad_()
        fwd = (R.cutouts((xr + 1) / 2, RESIZE_RECS, cs) - mean) / std
        gref, = th.autograd.grad((fwd * dy.double()).sum(), xr)
        geo, par = th.tensor(dg.resize_table(RESIZE_RECS, H, W), dtype=th.int32), None
    sd = unit_seed(gref)
    pre = 0.5 * th.randn(B, 3, H, W, generator=g(54))
    fwd, dyo = fwd.detach().double(), (dy * sd).float()
    if layout:
        fwd, dyo = to_patch_rows(fwd, patch), to_patch_rows(dyo, patch).contiguous()
    return dict(B=B, H=H, W=W, cutn=cutn, cs=cs, layout=layout, patch=patch, x=x.float(), dy=dyo, pre=pre, geo=geo, par=par, fwd=fwd,
                grad=gref.double() * sd)


@functools.lru_cache(maxsize=None)
def spherical_case(cutn, B, P, D):
    """cgd_spherical_loss against oracle.guidance.spherical_dist_loss in float64 (parity_checks._spherical_case), per row"""
    from oracle import guidance as og
    emb, tg = _r((cutn * B, D), 52), _r((P, D), 53)
    wm = (th.eye(B) * 0.7 if B == P else th.tensor([1.0, 0.5, -0.3][:P]).view(1, P).expand(B, P)).contiguous().float()
    er = emb.double().requires_grad_()
    d = og.spherical_dist_loss(er.view(cutn, B, 1, D), tg.double().view(1, 1, P, D))  # (cutn, B, P)
    part = (d * wm.double().view(1, B, P)).sum(2) * (1000.0 / cutn)
    grad, = th.autograd.grad(part.sum(), er)
    return emb, F.normalize(tg, dim=-1), wm, part.detach().reshape(-1), grad


# ---- GPU runners ---------------------------------------------------------------------------------------------------------------------------
def make_ctx(ck):
    prec, env = CONTEXTS[ck]
    with se._environ(env):
        return _ctx(prec)


def _dev(*ts):
    out = [None if t is None else t.to(DEV) for t in ts]
    return out if len(out) > 1 else out[0]


def _plain(t, label, ref, **kw):
    """an output that is not a Guarded view of a strided operand: a dense tensor inside a Guarded of its own"""
    return Out(label, Guarded(tuple(t), None, 0, 4), ref, **kw)


def run_attn(ctx, row, ck):
    s = row.spec
    nb, heads, T, d, legacy, causal = (s[k] for k in ("nb", "heads", "T", "d", "legacy", "causal"))
    qkv, dout, ref, dref = se.attn_data(nb, heads, T, d, legacy, causal)
    Cc, lib = heads * d, ctx.lib
    prec, env = CONTEXTS[ck]
    fam = attn_family_of(T, d, prec, env)
    sizes, size_flag = sizes_for(ctx, row, ck)
    plan = (C.c_int * 2)()
    # (the plan is that of a fresh context and does not read CGD_ATTN_X3: with the bf16x3 products off the choice is that of precision 0)
    assert lib.cgd_op_attn_plan(T, d, 3 * Cc, Cc, prec if env.get("CGD_ATTN_X3", "1") != "0" else 0, int(env.get("CGD_ATTN_FLASH", "-1")), plan) == 0
    upper = [int(lib.cgd_op_attn_buf_floats(nb, heads, T, d, i)) for i in range(5)]
    names = ("qkvT", "P", "Pt", "dP", "dAt")
    extra = [size_flag, (f"cgd_op_attn_plan family {plan[0]} = the claimed family {fam}", plan[0] == fam),
             (f"per-family sizes within the upper bound {upper}", all(sizes[n] <= u for n, u in zip(names, upper)))]
    bufs = [Scratch(sizes[n], n) for n in names]
    fwd_arr = (C.c_void_p * 5)(bufs[0].ptr, bufs[1].ptr, None, None, None)  # the networks hand the forward NULL for Pt / dP / dAt
    bwd_arr = (C.c_void_p * 5)(*[b.ptr for b in bufs])
    Q, O = Guarded((nb * T, 3 * Cc), None, 0, 4), Guarded((nb * T, Cc), None, 0, 4)
    DO, DQ = Guarded((nb * T, Cc), None, 0, 4), Guarded((nb * T, 3 * Cc), None, 0, 4)
    route = se.ROUTES["attn_generic" if fam == 0 else "attn_fused"]

    def seq():
        if causal:
            ctx.check(lib.cgd_op_attn_fwd_causal(ctx.h, Q.ptr, O.ptr, nb, heads, T, d, fwd_arr, _s()))
            return
        ctx.check(lib.cgd_op_attn_fwd(ctx.h, Q.ptr, O.ptr, nb, heads, T, d, legacy, fwd_arr, _s()))
        ctx.check(lib.cgd_op_attn_bwd(ctx.h, Q.ptr, DO.ptr, DQ.ptr, nb, heads, T, d, legacy, bwd_arr, _s()))

    ins, outs = [(Q, qkv)], [Out("out", O, ref)]
    if not causal:
        ins.append((DO, dout))
        cols = se.attn_cols(heads, d, legacy)
        # (at T = 1 the softmax is constant: dq and dk are identically zero, as in the shape-edge tier)
        outs += [Out(nm, DQ, dref, cols=idx, allow_small=T == 1 and nm in ("dq", "dk")) for nm, idx in zip(("dq", "dk", "dv"), cols)]
    return protocol(row, bufs, ins, outs, profiled(ctx, seq), route, extra)


def run_gn(ctx, row, ck):
    s = row.spec
    B, HW, Cc, bwd = s["B"], s["HW"], s["C"], s["bwd"]
    lib = ctx.lib
    big = HW > 4096
    ldx, ldy, lddz, lddx, ldadd = (Cc,) * 5 if big else (Cc + 8, Cc + 4, Cc + 12, Cc + 4, Cc + 8)
    x, gamma, beta, film, yref, dz, add, dxref = se.gn_data(B, HW, Cc, bwd)
    gd, bd, fd = _dev(gamma, beta, film)
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr = Scratch(sizes["scratch"], "gn scratch")
    X, Y = Guarded((B, HW, Cc), ldx, 0 if big else 4), Guarded((B, HW, Cc), ldy, 0)
    ins, outs = [(X, x)], [Out("y", Y, yref)]
    if bwd:
        DZ, DX, AD = Guarded((B, HW, Cc), lddz, 4), Guarded((B, HW, Cc), lddx, 0), Guarded((B, HW, Cc), ldadd, 4)
        ins += [(DZ, dz), (AD, add)]
        outs.append(Out("dx", DX, dxref))

    def seq():
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        ctx.check(lib.cgd_op_gn_fwd(ctx.h, X.ptr, ldx, Y.ptr, ldy, B, HW, Cc, gd.data_ptr(), bd.data_ptr(), fd.data_ptr(), 1, 1e-5, scr.ptr, _s()))
        if bwd:
            ctx.check(lib.cgd_op_gn_bwd(ctx.h, X.ptr, ldx, DZ.ptr, lddz, DX.ptr, lddx, AD.ptr, ldadd, B, HW, Cc, 1, scr.ptr, _s()))

    k = se.gn_kernel(HW, Cc)
    extra = [size_flag, (f"norm.hip runs this shape on {k} ({gn_nchunk(B, HW)} chunks of {se.gn_chunk(HW, B)} pixels in the scratch layout)", True)]
    return protocol(row, [scr], ins, outs, profiled(ctx, seq), GN_KIND, extra)


def run_gn_ab(ctx, row, ck):
    """a statistics-only forward (y = NULL) leaves the folded {a, b} pairs at the end of its scratch; cgd_op_conv3x3_ex convolves
    SiLU(x a + b) from there on the halo kernel.  The conv result is graded against the float64 conv of the float64 norm."""
    from cgd_amd import ops
    s = row.spec
    B, H, W, Cc, Co = s["B"], s["H"], s["W"], s["C"], s["Co"]
    HW, lib = H * W, ctx.lib
    x = _r((B, H, W, Cc), 120) * 2 + 0.7
    gamma, beta = 1 + 0.1 * _r((Cc,), 121), 0.1 * _r((Cc,), 122)
    w, b = _r((Co, Cc, 3, 3), 123) / math.sqrt(9 * Cc), _r((Co,), 124, 0.3)
    xg = x.double().reshape(B, HW, 32, Cc // 32)
    mean = xg.mean(dim=(1, 3))
    rstd = (xg.var(dim=(1, 3), unbiased=False) + 1e-5).rsqrt()
    a = rstd.repeat_interleave(Cc // 32, dim=1) * gamma.double()
    ab = th.stack([a, beta.double() - mean.repeat_interleave(Cc // 32, dim=1) * a], dim=2)  # (B, C, 2)
    ref = _conv_ref(x, w, b, 0, None, ab)
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr = Scratch(sizes["scratch"], "gn scratch")
    ab_off = gn_sizes(B, HW, Cc)["ab"]
    wf, _ = ops.pack_conv3x3(w)
    wt, bd, gd, btd = _dev(wf, b, gamma, beta)
    wfrag = ops.pack_conv3x3_frag(ctx, w.to(DEV))
    ldx, ldy = Cc + 8, Co + 8
    X, Y = Guarded((B, H, W, Cc), ldx, 4), Guarded((B, H, W, Co), ldy, 4)

    def seq():
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        ctx.check(lib.cgd_op_gn_fwd(ctx.h, X.ptr, ldx, None, 4, B, HW, Cc, gd.data_ptr(), btd.data_ptr(), None, 1, 1e-5, scr.ptr, _s()))
        ctx.check(lib.cgd_op_conv3x3_ex(ctx.h, X.ptr, ldx, wt.data_ptr(), wfrag.data_ptr(), Y.ptr, ldy, bd.data_ptr(), None, 0, scr.ptr + 4 * ab_off,
                                        B, H, W, Cc, Co, 0, 512, 1, 0, 0, None, 0, None, _s()))

    route = ("groupnorm, then hconv2", lambda c: c[2] >= 1 and c[1] >= 1 and c[0] == 0)
    return protocol(row, [scr], [(X, x)], [Out("conv of SiLU(GroupNorm(x))", Y, ref)], profiled(ctx, seq), route, [size_flag])


def run_gn_gnb(ctx, row, ck):
    """strided_checks.check_wino_records_strided with the scratch exact: forward statistics -> the dgrad conv's epilogue reads the forward's
    coefficients from the scratch (gnb_scratch) and leaves backward sums -> cgd_op_gn_bwd merges them"""
    from cgd_amd import ops
    s = row.spec
    B, H, W, Cn = s["B"], s["H"], s["W"], s["C"]
    HW, lib = H * W, ctx.lib
    xn = 3.0 + _r((B, HW, Cn), 130)
    gam, bet = 1 + 0.1 * _r((Cn,), 93), 0.1 * _r((Cn,), 94)
    dy = _r((B, H, W, Cn), 140)
    wd = _r((Cn, Cn, 3, 3), 141) / math.sqrt(9 * Cn)
    dzref = _conv_ref(dy, wd.flip(2, 3).transpose(0, 1), None, 0).reshape(B, HW, Cn)
    _, dxref = _gn_ref(xn, gam, bet, 1, dzref.float())
    sd = unit_seed(dxref)
    wwd = ops.pack_conv3x3_wino(ctx, wd.to(DEV), dgrad=True)
    gd, bd = _dev(gam, bet)
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr = Scratch(sizes["scratch"], "gn scratch")
    ldxn, lddy, lddz, lddx = Cn + 32, Cn + 32, Cn + 16, Cn + 8
    XN, DY = Guarded((B, HW, Cn), ldxn, 16), Guarded((B, H, W, Cn), lddy, 32)
    DZ, DX = Guarded((B, HW, Cn), lddz, 8), Guarded((B, HW, Cn), lddx, 4)
    merged = []

    def seq():
        m0 = int(lib.cgd_op_gn_record_merges(ctx.h))
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        ctx.check(lib.cgd_op_gn_fwd(ctx.h, XN.ptr, ldxn, None, 4, B, HW, Cn, gd.data_ptr(), bd.data_ptr(), None, 1, 1e-5, scr.ptr, _s()))
        ctx.check(lib.cgd_op_conv3x3_wino_ex(ctx.h, DY.ptr, lddy, wwd.data_ptr(), DZ.ptr, lddz, None, None, 0, None, B, H, W, Cn, Cn, 0, 0,
                                             XN.ptr, ldxn, scr.ptr, _s()))
        ctx.check(lib.cgd_op_gn_bwd(ctx.h, XN.ptr, ldxn, DZ.ptr, lddz, DX.ptr, lddx, None, 0, B, HW, Cn, 1, scr.ptr, _s()))
        merged.append(int(lib.cgd_op_gn_record_merges(ctx.h)) - m0)

    def launch():
        return _routes(ctx, seq)

    route = ("wconv with the backward-sum epilogue (kind 5), groupnorm", lambda c: c[5] == 1 and c[2] >= 1)
    recs = protocol(row, [scr], [(XN, xn), (DY, dy * sd)], [Out("dz", DZ, dzref * sd), Out("dx", DX, dxref * sd)], launch, route, [size_flag])
    return recs + _tag([_flag(f"{row.name}: cgd_op_gn_bwd merged the dgrad conv's records in both runs (merges per run {merged})", merged == [1, 1])],
                       row, "route")


def run_ln(ctx, row, ck):
    s = row.spec
    rows, Cc = s["rows"], s["C"]
    x, gamma, beta, yref, dy, dxref = se.ln_data(rows, Cc)
    lib = ctx.lib
    gd, bd = _dev(gamma, beta)
    sizes, size_flag = sizes_for(ctx, row, ck)
    stats = Scratch(sizes["stats"], "ln stats")
    X, Y, DY, DX = (Guarded((rows, Cc), None, 0, 4) for _ in range(4))

    def seq():
        ctx.check(lib.cgd_op_ln_fwd(ctx.h, X.ptr, Y.ptr, rows, Cc, gd.data_ptr(), bd.data_ptr(), 1e-5, stats.ptr, _s()))
        ctx.check(lib.cgd_op_ln_bwd(ctx.h, X.ptr, DY.ptr, DX.ptr, rows, Cc, gd.data_ptr(), stats.ptr, _s()))

    vec = Cc % 256 == 0 and Cc <= 1024
    extra = [size_flag, (f"norm.hip runs C = {Cc} on the {'vector' if vec else 'generic'} kernel (restated: the profile has no kind for it)", True)]
    return protocol(row, [stats], [(X, x), (DY, dy)], [Out("y", Y, yref), Out("dx", DX, dxref)], profiled(ctx, seq), NO_KIND, extra)


def run_attnpool(ctx, row, ck):
    case = head_case(row.spec["head"])
    B, Cc, S, d, out = case["B"], case["C"], case["S"], case["d"], case["out"]
    pool, lib = case["pool"], ctx.lib
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr = Scratch(sizes["scratch"], "attnpool scratch")
    w = [t.detach().reshape(-1).contiguous().to(DEV) for t in (pool.positional_embedding, pool.qkv_proj.weight, pool.qkv_proj.bias,
                                                               pool.c_proj.weight, pool.c_proj.bias)]
    yd = case["yt"].to(DEV)
    seed = unit_seed(case["dh"])
    Hh = Guarded((B * S * S, Cc), None, 0, 4)
    outs = [_plain((B, Cc), "pooled", case["pooled"]), _plain((B, out), "logits", case["logits"]), _plain((B,), "logp", case["logp"]),
            _plain((B * S * S, Cc), "dh", case["dh"] * seed)]
    P_, L_, LP, DH = (o.G for o in outs)

    def seq():
        ctx.check(lib.cgd_op_attnpool_fwd(ctx.h, Hh.ptr, w[0].data_ptr(), w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(), w[4].data_ptr(),
                                          yd.data_ptr(), P_.ptr, L_.ptr, LP.ptr, scr.ptr, B, S, Cc, d, out, _s()))
        ctx.check(lib.cgd_op_attnpool_bwd(ctx.h, w[1].data_ptr(), w[2].data_ptr(), w[3].data_ptr(), w[4].data_ptr(), seed, DH.ptr, scr.ptr,
                                          B, S, Cc, d, out, _s()))

    return protocol(row, [scr], [(Hh, case["h"])], outs, profiled(ctx, seq), NO_CONV, [size_flag])


def run_cut(ctx, row, ck):
    s = row.spec
    kind, acc = s["kind"], s["acc"]
    c = cut_case(kind, s["big"])
    B, H, W, cutn, cs, layout, patch = (c[k] for k in ("B", "H", "W", "cutn", "cs", "layout", "patch"))
    lib = ctx.lib
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr = Scratch(sizes["scratch"], f"cutouts_{kind} adjoint scratch")
    geo, par = _dev(c["geo"], c["par"])
    flags_p = geo.data_ptr() + 16 * cutn
    X, DY = Guarded((B, 3, H, W), None, 0, 4), Guarded(tuple(c["dy"].shape), None, 0, 4)
    OUT, G_ = Guarded(tuple(c["fwd"].shape), None, 0, 4), Guarded((B, 3, H, W), None, 0, 4)

    def seq():
        if kind == "aug":
            ctx.check(lib.cgd_cutouts_aug_fwd(ctx.h, X.ptr, geo.data_ptr(), par.data_ptr(), None, None, OUT.ptr, B, H, W, cutn, cs, layout, patch, _s()))
            ctx.check(lib.cgd_cutouts_aug_bwd(ctx.h, DY.ptr, geo.data_ptr(), par.data_ptr(), G_.ptr, scr.ptr, B, H, W, cutn, cs, layout, patch, acc, _s()))
        else:
            ctx.check(lib.cgd_cutouts_resize_fwd(ctx.h, X.ptr, geo.data_ptr(), flags_p, OUT.ptr, B, H, W, cutn, cs, layout, patch, _s()))
            ctx.check(lib.cgd_cutouts_resize_bwd(ctx.h, DY.ptr, geo.data_ptr(), flags_p, G_.ptr, scr.ptr, B, H, W, cutn, cs, layout, patch, acc, _s()))

    ins = [(X, c["x"]), (DY, c["dy"])]
    if acc:
        ins.append((G_, c["pre"]))
    outs = [Out("cutouts", OUT, c["fwd"]), Out("adjoint", G_, c["grad"] + (c["pre"].double() if acc else 0.0), poison=not acc)]
    runs = ceil_div(cutn, rows_per_launch(B, cutn))
    extra = [size_flag, (f"{runs} run(s) of at most {rows_per_launch(B, cutn)} cutouts per launch; both check_shape bounds hold",
                         runs == (2 if s["big"] else 1) and cutout_bounds_ok(kind, B, H, W, cutn, cs))]
    return protocol(row, [scr], ins, outs, profiled(ctx, seq), NO_KIND, extra)


def run_ilvr(ctx, row, ck):
    from cgd_amd import diffusion as dd
    from tests import ilvr_ref
    s = row.spec
    B, H, W, N, with_x0, ref_b = (s[k] for k in ("B", "H", "W", "N", "x0", "ref_b"))
    lib = ctx.lib
    gen = g(9000 + 10 * N + 2 * ref_b + with_x0 + H)
    mk = lambda *sh: th.randn(*sh, generator=gen)  # noqa: E731
    sample, x0, noise = mk(B, 3, H, W), (th.tanh(mk(B, 3, H, W)) if with_x0 else None), mk(B, 3, H, W)
    refimg = th.tanh(mk(ref_b, 3, H, W))
    k = dd.create_gaussian_diffusion(1000, "linear", "50", False).mask_coef(20)
    sa, sb = k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev
    want_s, want_x0 = ilvr_ref.refine_fp64(sa, sb, sample, x0, refimg, noise, N)
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr = Scratch(sizes["scratch"], "ilvr scratch")
    Sg, Rg, Ng = Guarded((B, 3, H, W), None, 0, 4), Guarded((ref_b, 3, H, W), None, 0, 4), Guarded((B, 3, H, W), None, 0, 4)
    ins, outs = [(Sg, sample), (Rg, refimg), (Ng, noise)], [Out("sample", Sg, want_s, poison=False)]
    X0 = None
    if with_x0:
        X0 = Guarded((B, 3, H, W), None, 0, 4)
        ins.append((X0, x0))
        outs.append(Out("pred_xstart", X0, want_x0, poison=False))

    def seq():
        ctx.check(lib.cgd_ilvr_refine(ctx.h, Sg.ptr, None if X0 is None else X0.ptr, Rg.ptr, Ng.ptr, scr.ptr, B, H, W, ref_b, N, sa, sb, _s()))

    return protocol(row, [scr], ins, outs, profiled(ctx, seq), NO_KIND, [size_flag])


def run_quantile(ctx, row, ck):
    from cgd_amd import diffusion as dd
    s = row.spec
    B, n, mis = s["B"], s["n"], s["mis"]
    lib = ctx.lib
    tab = dd.create_gaussian_diffusion(1000, "linear", "dpm50", False)
    k, frac = tab.threshold_rank(0.995, n)
    v = _r((B, n), 17 * n + B)
    a = th.sort(v.abs(), dim=1).values
    vk, vk1 = a[:, k], a[:, min(k + 1, n - 1)]
    f32 = float(th.tensor(frac, dtype=th.float32))
    want = th.stack([vk.double(), vk1.double(), vk.double() + (vk1.double() - vk.double()) * f32], dim=1)
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr = Scratch(sizes["scratch"], "quantile scratch")
    # gap rows hold +-1e6 / 7.5e5: a slice that read past its row would select them
    V = Guarded((B, n), None, 0, (-(ceil_div(MIN_GUARD, n) * n) % 4) + (1 if mis else 0), guard_rows=ceil_div(MIN_GUARD, n))
    assert V.ptr % 16 == (4 if mis else 0)
    O3 = Scratch(sizes["out3"], "out3")
    exact = []

    def seq():
        ctx.check(lib.cgd_op_abs_quantile(ctx.h, V.ptr, B, n, k, frac, 0.0, math.inf, O3.ptr, scr.ptr, _s()))

    def launch():
        c = _routes(ctx, seq)
        got = O3.view.view(B, 3).cpu()
        exact.append(bits_equal(got[:, :2].contiguous(), th.stack([vk, vk1], dim=1).contiguous()))
        return c

    vec = n % 4 == 0 and not mis
    extra = [size_flag, (f"{'vector' if vec else 'scalar'} path by the launcher's rule (n % 4 == 0 and 16-byte aligned values), "
                         f"{ceil_div(n, QUANTILE_SLICE)} slice(s)", True)]
    recs = protocol(row, [scr, O3], [(V, v)], [Out("(v_k, v_k+1, s)", _View(lambda: O3.view.view(B, 3)), want)], launch, NO_KIND, extra)
    return recs + _tag([_flag(f"{row.name}: v_k and v_k+1 bit-equal to torch.sort in both runs", exact == [True, True])], row, "parity")


def run_threshold(ctx, row, ck):
    from cgd_amd import diffusion as dd
    from tests import threshold_ref
    s = row.spec
    B, H, W, mis = s["B"], s["H"], s["W"], s["mis"]
    n, lib = 3 * H * W, ctx.lib
    tab = dd.create_gaussian_diffusion(1000, "linear", "dpm50", False)
    kc = tab.step_coef(20, 3)
    rank, frac = tab.threshold_rank(0.9, n)
    x, x0, gg = (_r((B, 3, H, W), 640 + i + W) for i in range(3))
    a_, b_, s1 = float(kc.sqrt_recip), float(kc.sqrt_recipm1), float(kc.sqrt_one_minus_ab)
    e = (a_ * x.double() - x0.double()) / b_ - s1 * gg.double()
    x0c = a_ * x.double() - b_ * e
    sref = threshold_ref.scales(x0c, 0.9, 1.5)
    sizes, size_flag = sizes_for(ctx, row, ck)
    scr, T3 = Scratch(sizes["scratch"], "quantile scratch"), Scratch(sizes["thr3"], "thr3")
    off = 1 if mis else 0
    X, X0, Gg = (Guarded((B, 3, H, W), None, 0, 4) for _ in range(3))
    RAW = Guarded((B, 3, H, W), None, 0, 4 + off)

    def seq():
        ctx.check(lib.cgd_dpmpp_threshold(ctx.h, X.ptr, X0.ptr, Gg.ptr, None, RAW.ptr, B, H, W, kc, rank, frac, 1.0, 1.5, T3.ptr, scr.ptr, _s()))

    vec = n % 4 == 0 and not mis
    extra = [size_flag, (f"{'vector' if vec else 'scalar'} path by the launcher's rule, {ceil_div(n, QUANTILE_SLICE)} slice(s)", True)]
    return protocol(row, [scr, T3], [(X, x), (X0, x0), (Gg, gg)], [Out("x0c", RAW, x0c), Out("s", _View(lambda: T3.view.view(B, 3)[:, 2]), sref)],
                    profiled(ctx, seq), NO_KIND, extra)


class _View:
    """an output that is a function of device buffers (a column group times a unit-peak factor, the column sums of a partial array): graded
    and compared between the runs like a view, and not guarded itself (the buffers behind it are)"""

    def __init__(self, fn):
        self.fn = fn

    @property
    def view(self):
        return self.fn()


def run_tail(ctx, row, ck):
    """cgd_guidance_combine -> cgd_grad_finish -> cgd_scalars on partial buffers of exactly cgd_guidance_part_blocks entries, graded as
    tests/test_gpu_tail.py grades them: gradients at unit peak, the partials by their column sums, the scalars (but the cancelling gradient
    mean) as ratios to the float64 evaluation of the device's own partials"""
    from cgd_amd import diffusion as dd
    from tests import tail_ref as tr
    s = row.spec
    shape = B, H, W = s["B"], s["H"], s["W"]
    lib = ctx.lib
    k = dd.create_gaussian_diffusion(*tr.SCHEDULE).step_coef(125, 125)
    x_in, x0, g_clip = tr.combine_inputs(shape, 125)
    g_direct, seed_eps, losses = tr.guidance_combine(g_clip, x_in, x0, k, *tr.SCALES)
    gu = tr.finish_inputs(shape)[1]
    g_ref, _, s2_ref, _ = tr.grad_finish(g_direct, gu)
    sizes, size_flag = sizes_for(ctx, row, ck)
    LP, GP, SC = Scratch(sizes["loss_part"], "loss_part"), Scratch(sizes["g_part"], "g_part"), Scratch(sizes["scalars"], "scalars")
    n_clip, total = 7, B * 3 * H * W
    clip_part = tr.scalars_inputs(n_clip, 1, 1, 0.4)[0]
    cp = clip_part.to(DEV)
    GC, XI, XZ, GU = (Guarded((B, 3, H, W), None, 0, 4) for _ in range(4))
    GD, S6, Gg = Guarded((B, 3, H, W), None, 0, 4), Guarded((B, 6, H, W), None, 0, 4), Guarded((B, 3, H, W), None, 0, 4)
    sdd, sde, sdg = unit_seed(g_direct), unit_seed(seed_eps), unit_seed(g_ref)
    keep = [0, 1, 2, 3, 4, 5, 7]

    def seq():
        ctx.check(lib.cgd_guidance_combine(ctx.h, GC.ptr, XI.ptr, XZ.ptr, GD.ptr, S6.ptr, LP.ptr, B, H, W, k, *tr.SCALES, _s()))
        ctx.check(lib.cgd_grad_finish(ctx.h, GD.ptr, GU.ptr, Gg.ptr, GP.ptr, B, H, W, _s()))
        ctx.check(lib.cgd_scalars(ctx.h, cp.data_ptr(), n_clip, LP.ptr, GP.ptr, B, H, W, 1, SC.ptr, _s()))

    def scalars_ratio():
        want = tr.scalars(clip_part, LP.view.cpu(), GP.view.cpu(), total, 1)
        return SC.view.double().cpu()[keep] / want[keep]

    outs = [Out("g_direct", GD, None, grade=False), Out("seed6", S6, None, grade=False), Out("g", Gg, None, grade=False),
            Out("g_direct (unit peak)", _View(lambda: GD.view * sdd), g_direct * sdd),
            Out("seed_eps (unit peak)", _View(lambda: S6.view[:, :3] * sde), seed_eps * sde),
            Out("variance half of the seed", _View(lambda: S6.view[:, 3:]), th.zeros(B, 3, H, W, dtype=th.float64), allow_small=True),
            Out("g (unit peak)", _View(lambda: Gg.view * sdg), g_ref * sdg),
            Out("loss_part column sums (tv, range, sat)", _View(lambda: LP.view.double().reshape(-1, 3).sum(0)), losses),
            Out("g_part sum g^2 / float64", _View(lambda: GP.view.double().reshape(-1, 2)[:, 1].sum().reshape(1) / s2_ref), th.ones(1, dtype=th.float64)),
            Out("scalars / float64 of the device's partials", _View(scalars_ratio), th.ones(len(keep), dtype=th.float64))]
    return protocol(row, [LP, GP, SC], [(GC, g_clip), (XI, x_in), (XZ, x0), (GU, gu)], outs, profiled(ctx, seq), NO_KIND, [size_flag])


def run_secondary(ctx, row, ck):
    """cgd_secondary_combine against autograd, as tests/test_gpu_secondary.py::test_combine_against_autograd states it"""
    from oracle import guidance as og
    s = row.spec
    B, H, W = s["B"], s["H"], s["W"]
    lib = ctx.lib
    fac, alpha, sigma, tvs, rs, sat = 0.6, 0.8, 0.6, 40.0, 30.0, 3.0
    x = th.randn(B, 3, H, W, generator=g(340)).requires_grad_()
    v = th.randn(B, 3, H, W, generator=g(341)).requires_grad_()
    gin = th.randn(B, 3, H, W, generator=g(342)) * 1e-2
    pred = x * alpha - v * sigma
    x_in = pred * fac + x * (1 - fac)
    tv_l, rng_l = og.tv_loss(x_in).sum() * tvs, og.range_loss(pred).sum() * rs
    sat_l = th.abs(x_in - x_in.clamp(min=-1, max=1)).mean().sum() * sat
    dx_ref, dv_ref = th.autograd.grad((x_in * gin).sum() + tv_l + rng_l + sat_l, [x, v])
    sizes, size_flag = sizes_for(ctx, row, ck)
    LP = Scratch(sizes["loss_part"], "loss_part")
    GI, XI, PR = (Guarded((B, 3, H, W), None, 0, 4) for _ in range(3))
    GD, SD = Guarded((B, 3, H, W), None, 0, 4), Guarded((B, 3, H, W), None, 0, 4)

    def seq():
        ctx.check(lib.cgd_secondary_combine(ctx.h, GI.ptr, XI.ptr, PR.ptr, GD.ptr, SD.ptr, LP.ptr, B, H, W, fac, alpha, sigma, tvs, rs, sat, _s()))

    outs = [Out("direct part", GD, dx_ref.double()), Out("seed", SD, dv_ref.double()),
            Out("loss_part column sums (tv, range, sat)", _View(lambda: LP.view.double().reshape(-1, 3).sum(0)),
                th.stack([tv_l, rng_l, sat_l]).detach().double())]
    return protocol(row, [LP], [(GI, gin), (XI, x_in.detach()), (PR, pred.detach())], outs, profiled(ctx, seq), NO_KIND, [size_flag])


def run_records(ctx, row, ck):
    """cgd_op_gn_records at cap = exactly the count it reports: the forward records the unsplit hconv2 tile leaves (tests/test_gpu_hconv_unsplit.py),
    one (mean, M2) pair per (4 x 16-pixel tile, channel), against float64 statistics of y as stored"""
    from cgd_amd import ops
    s = row.spec
    B, H, W, Ci, Co = s["B"], s["H"], s["W"], s["Ci"], s["Co"]
    lib = ctx.lib
    x, w, b = _r((B, H, W, Ci), 7801), _r((Co, Ci, 3, 3), 7802) / math.sqrt(9 * Ci), _r((Co,), 7803, 0.3)
    ref = _conv_ref(x, w, b, 0)
    wt, bd = _dev(ops.pack_conv3x3(w)[0], b)
    wfrag = ops.pack_conv3x3_frag(ctx, w.to(DEV))
    sizes, size_flag = sizes_for(ctx, row, ck)
    n = sizes["records"]
    REC = Scratch(n, "record buffer")
    X, Y = Guarded((B, H, W, Ci), None, 0, 4), Guarded((B, H, W, Co), None, 0, 4)
    pix = C.c_int()
    seen = []

    def seq():
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        ctx.check(lib.cgd_op_conv3x3_ex(ctx.h, X.ptr, Ci, wt.data_ptr(), wfrag.data_ptr(), Y.ptr, Co, bd.data_ptr(), None, 0, None, B, H, W, Ci, Co, 0, 512,
                                        1, 0, 1, None, 0, None, _s()))
        ctx.check(lib.cgd_op_gn_records(ctx.h, Y.ptr, Co, B * H * W, Co, 0, REC.ptr, n, C.byref(pix), _s()))
        seen.append((pix.value, B * H * W // max(pix.value, 1) * Co * 2))

    t = ref.reshape(B, H // 4, 4, W // 16, 16, Co).permute(0, 1, 3, 2, 4, 5).reshape(-1, 64, Co)  # (sample, tile row, tile column) order
    mean_ref, var_ref = t.mean(1), ((t - t.mean(1, keepdim=True)) ** 2).sum(1) / 64

    def launch():
        ctx.check(lib.cgd_set_hconv(ctx.h, 1 + 16 * 8, 256))
        try:
            return _routes(ctx, seq)
        finally:
            ctx.check(lib.cgd_set_hconv(ctx.h, 1, 256))

    got = lambda j: REC.view.double().cpu().reshape(-1, Co, 2)[..., j]  # noqa: E731
    outs = [Out("y", Y, ref), Out("record means", _View(lambda: got(0)), mean_ref), Out("record M2 / 64", _View(lambda: got(1) / 64), var_ref)]
    route = ("hconv2 (the unsplit tile), records taken", lambda c: c[1] >= 1 and c[0] == 0)
    recs = protocol(row, [REC], [(X, x)], outs, launch, route, [size_flag])
    return recs + _tag([_flag(f"{row.name}: the entry reports 64-pixel records and the count the buffer was sized for, in both runs "
                              f"(pixels, floats) = {seen}", seen == [(64, n)] * 2)], row, "route")


def run_spherical(ctx, row, ck):
    s = row.spec
    cutn, B, P, D = s["cutn"], s["B"], s["P"], s["D"]
    emb, tn, wm, part_ref, grad = spherical_case(cutn, B, P, D)
    lib = ctx.lib
    sizes, size_flag = sizes_for(ctx, row, ck)
    LP = Scratch(sizes["loss_part"], "loss_part")
    E, DE = Guarded((cutn * B, D), None, 0, 4), Guarded((cutn * B, D), None, 0, 4)
    td, wd = _dev(tn, wm)

    def seq():
        ctx.check(lib.cgd_spherical_loss(ctx.h, E.ptr, td.data_ptr(), wd.data_ptr(), DE.ptr, LP.ptr, cutn, B, P, D, 1000.0, _s()))

    # D = 1: a normalised 1-vector is +-1, the distance is 0 or 2 and the gradient 0 x infinity: only the loss is graded there
    outs = [Out("loss_part", _View(lambda: LP.view), part_ref), Out("d_emb", DE, grad, grade=D > 1)]
    return protocol(row, [LP], [(E, emb)], outs, profiled(ctx, seq), NO_KIND, [size_flag])


def run_directional(ctx, row, ck):
    from tests import direction_ref as dr
    s = row.spec
    cutn, B, Bs, P, D = s["cutn"], s["B"], s["Bs"], s["P"], s["D"]
    lib = ctx.lib
    if D > 1:
        e, src, dn, w = dr.make_case((cutn, B, Bs, P, D))
    else:  # make_case needs a direction orthogonal to the source row: in one dimension every row is +-1, delta is 0 or +-2
        e, src = th.tensor([[1.5], [-0.5], [2.0], [0.3], [-1.0], [0.7]]), th.tensor([[1.0], [1.0], [-1.0]])
        dn, w = th.tensor([[1.0], [-1.0]]), th.tensor([[0.5, 0.25], [0.75, -0.5]])
    loss, grad, _ = dr.loss_and_grad(e, src, dn, w, cutn, B)
    sizes, size_flag = sizes_for(ctx, row, ck)
    LP = Scratch(sizes["loss_part"], "loss_part")
    E, DE = Guarded((cutn * B, D), None, 0, 4), Guarded((cutn * B, D), None, 0, 4)
    sd_, dd_, wd = _dev(src, dn, w)

    def seq():
        ctx.check(lib.cgd_directional_loss(ctx.h, E.ptr, sd_.data_ptr(), dd_.data_ptr(), wd.data_ptr(), DE.ptr, LP.ptr, cutn, B, Bs, P, D, dr.SCALE, 0, _s()))

    sdg = unit_seed(grad) if D > 1 else 1.0

    # (the gradient is homogeneous of degree -1 in |e|: graded at unit peak, as test_gpu_direction.py does; D = 1: identically zero)
    outs = [Out("loss_part", _View(lambda: LP.view), loss), Out("d_emb", DE, grad, grade=False),
            Out("d_emb (unit peak)", _View(lambda: DE.view * sdg), grad * sdg, allow_small=D == 1)]
    return protocol(row, [LP], [(E, e)], outs, profiled(ctx, seq), NO_KIND, [size_flag])


RUNNERS = {"attn": run_attn, "gn": run_gn, "gn_ab": run_gn_ab, "gn_gnb": run_gn_gnb, "ln": run_ln, "attnpool": run_attnpool, "cut": run_cut,
           "ilvr": run_ilvr, "quantile": run_quantile, "threshold": run_threshold, "tail": run_tail, "secondary": run_secondary,
           "spherical": run_spherical, "directional": run_directional, "records": run_records}


def check_group(fam, ck, ctx=None):
    ctx = ctx or make_ctx(ck)
    out = []
    for row in rows_of(fam, ck):
        out += RUNNERS[row.op](ctx, row, ck)
    th.cuda.synchronize()
    return out


def verdicts_complete(recs, rows):
    """the rows that lack one of the four verdicts"""
    have = {}
    for r in recs:
        have.setdefault(r["row"], set()).add(r["verdict"])
    return [row.name for row in rows if not have.get(row.name, set()) >= VERDICTS]


# ---- the detector: torch ops only, nothing outside any allocation ---------------------------------------------------------------------------
def detector(device=DEV):
    """Three fake kernels through `protocol`: {fake: the verdicts that failed}.  `overrun` writes one float into the guard behind its scratch,
    `stale` reads scratch[0] before writing it (through a maximum that swallows NaN), `idle` writes nothing."""
    row = Row("detector", "fake", "fake", ("p1",), {})
    x = th.arange(1.0, 9.0)
    want = (2 * x).double()
    caught = {}
    for fake in ("honest", "overrun", "stale", "idle"):
        scr = Scratch(16, "fake scratch", device)
        X, Y = Guarded((8,), None, 0, 4, device=device), Guarded((8,), None, 0, 4, device=device)

        def launch(fake=fake, scr=scr, X=X, Y=Y):
            if fake == "idle":
                return [0] * 6
            first = scr.view[0].clone()
            scr.view[:8] = 2 * X.view
            if fake == "overrun":
                base = scr.G.view.storage_offset()
                scr.G.buf[base + scr.n] = 3.0  # one float past the last element of the scratch, inside the allocation
            Y.view.copy_(scr.view[:8])
            if fake == "stale":  # fmax swallows the NaN of the first run; the 1e6 of the second moves the value within the tolerance
                Y.view[0] = th.fmax(Y.view[0], Y.view[0] + first * 1e-12)
            return [0] * 6

        recs = protocol(row._replace(name=fake), [scr], [(X, x)], [Out("y", Y, want)], launch, ("none", lambda c: True))
        caught[fake] = sorted({r["verdict"] for r in recs if not r["ok"]})
    return caught


def detector_problems(caught):
    """what a vacuous tier would look like: the list is empty when every fake is caught by the verdict that is meant to catch it"""
    bad = []
    if caught["honest"]:
        bad.append(f"the honest fake fails {caught['honest']}")
    if "guards" not in caught["overrun"]:
        bad.append("a write of one float into the guard of a Guarded scratch was NOT flagged: the tier is vacuous")
    if "rerun" not in caught["stale"]:
        bad.append("a read of scratch[0] before it is written gave EQUAL outputs under the two poisons: the tier is vacuous")
    if "parity" not in caught["idle"]:
        bad.append("a kernel that writes nothing PASSED parity: the tier is vacuous")
    return bad


if __name__ == "__main__":  # one report: the failed records, the sizes per row and the wall time per group, as JSON on stdout
    import json
    import sys
    import time
    recs, times = [], {}
    for fam_, ck_ in GROUPS:
        t0 = time.time()
        try:
            recs += [dict(r, group=f"{fam_}[{ck_}]") for r in check_group(fam_, ck_)]
        except Exception as exc:  # noqa: BLE001  (a report tool: the group's error is part of the report)
            recs.append(dict(name=f"{fam_}[{ck_}] raised {type(exc).__name__}: {exc}", ok=False, row="", verdict="error"))
            if "illegal memory access" in str(exc):
                break
        times[f"{fam_}[{ck_}]"] = round(time.time() - t0, 2)
    bad = [r for r in recs if not r["ok"]]
    sizes = {r["name"]: 1 for r in recs if r.get("verdict") == "route" and "sizes {" in r["name"]}
    json.dump({"failed": len(bad), "bad": bad[:200], "seconds": times, "records": len(recs), "sizes": sorted(sizes), "detector": detector()},
              sys.stdout, indent=1, default=str)
    print()
    sys.exit(1 if bad else 0)
