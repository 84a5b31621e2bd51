"""Shape-edge parity of the op kernels (tests/test_gpu_shape_edges.py, tests/test_shape_edges_host.py).

Every other tier takes its shapes from the workloads.  This one takes them from the launchers: for each kernel family, the smallest value a
dimension may have and t - g, t, t + g around every tile size t at the dimension's granularity g, on both sides of each clause that accepts,
routes or refuses a problem (CLAUSES names the clause of every row as file:line; the host test checks that the cited line still holds it).
Dimensions are combined pairwise: one dimension sweeps while the others sit at an edge value of their own.

Graded as the strided tier, with its machinery (tests/strided_checks.py): every operand lives in a `Guarded` allocation, outputs start as a
NaN sentinel, parity is `rec` against float64 at the literal 1e-4 + 1e-3 |ref| (inputs O(1), alpha = 1 / sqrt(K), backward seeds at unit
peak), nothing may be written outside the view, a rerun must be bit-identical, the launch profile must show the claimed route, and a refused
call must raise with its text and write nothing.  Every shape a forced route refuses is run again with force_tile = 0 (family "fallthrough").

One TABLE drives the GPU file and the host file.  The references are built here, once per shape (`*_data`), for both."""
import contextlib
import ctypes as C
import functools
import math
import os
from collections import namedtuple

import torch as th
import torch.nn.functional as F

from tests.parity_checks import ATOL, DEV, RTOL, _ctx, _flag, g, rec, unit_seed
from tests.strided_checks import GAP, HALO, OUT_BITS, ROUTE_LOG, Guarded, _conv_ref, _refusal, _routes, _s

NUM_CU = 256  # what cgd_op_plan is asked with; no row's claim depends on the CU count of the device (GEMV_BIG_N holds for up to 304)
GEMV_BIG_N = 16 * 4 * 304 + 17  # more columns than 4 workgroups per CU cover in one pass on any CDNA part

# context key -> (precision, environment of cgd_ctx_create)
CONTEXTS = {
    "p0": (0, {}), "p1": (1, {}), "p2": (2, {}),
    "p1_epi0": (1, {"CGD_HGEMM_EPI": "0"}), "p1_kg2": (1, {"CGD_HGEMM_KG": "2"}), "p1_tm128": (1, {"CGD_HGEMM_VAR": "2"}),
    "p1_kgemm64": (1, {"CGD_KGEMM": "2,256,1"}), "p1_kconv16": (1, {"CGD_KCONV": "1,1024,4,1,0,2,256"}),
    "p1_flash0": (1, {"CGD_ATTN_FLASH": "0"}), "p1_flash1": (1, {"CGD_ATTN_FLASH": "1"}), "p1_flash2": (1, {"CGD_ATTN_FLASH": "2"}),
    "p1_x3off": (1, {"CGD_ATTN_X3": "0"}),
}
ATTN_CTXS = ("p0", "p1", "p1_flash0", "p1_flash1", "p1_flash2", "p1_x3off")

# clause key -> (file under csrc/, line, a token that line must contain, what "lo" / "hi" mean)
CLAUSES = {
    "igemm.rows": ("gemm.hip", 464, "cdiv(p.M, BM)", "M <= BM: one row tile / M > BM: a second, ragged one (a_ok, gemm.hip:96)"),
    "igemm.cols": ("gemm.hip", 464, "cdiv(p.N, BN)", "N <= BN / N > BN (b_ok, gemm.hip:113)"),
    "igemm.ktail": ("gemm.hip", 73, "(p.K + BK - 1) / BK", "K a multiple of BK = 32 / a ragged last k-tile"),
    "igemm.empty_slice": ("gemm.hip", 233, "if (kt0 < kt1)", "every slice has k-tiles / a slice is empty and writes a zero slab"),
    "reduce.vec": ("gemm.hip", 415, "!(N & 3)", "split-K reduce on float4 / on scalars"),
    "gemv.rows": ("gemm.hip", 505, "p.M <= 4", "M <= 4 / M = 5 refused when forced"),
    "gemv.lds": ("gemm.hip", 506, "48 * 1024", "A rows within 48 KiB of LDS / above: refused when forced"),
    "gemv.kpass": ("gemm.hip", 360, "k0 += 256", "K <= 256: one pass over K / a second pass"),
    "gemv.cols": ("gemm.hip", 745, "cdiv(p.N, 16)", "N <= 16: one workgroup / N > 16"),
    "gemv.grid": ("gemm.hip", 745, "4L * ctx->num_cu", "every workgroup owns one 16-column block / a second pass of the grid (gemm.hip:354)"),
    "hgemm.rows64": ("hgemm.hip", 1051, "cdiv(g.M, tm)", "64-row tiles (hgemm.hip:951): M <= 64 / 64 < M <= 128 / beyond"),
    "hgemm.rows128": ("hgemm.hip", 945, "hgemm_var == 3", "128-row tiles (CGD_HGEMM_VAR=2, hgemm.hip:953): M <= 128 / M > 128"),
    "hgemm.cols": ("hgemm.hip", 1051, "cdiv(g.N, GN)", "N <= 128 / N > 128: a partial column tile"),
    "hgemm.k64": ("hgemm.hip", 915, "p.K % GK", "K a multiple of 64 / refused when forced"),
    "hgemm.n32": ("hgemm.hip", 915, "p.N & 31", "N a multiple of 32 / refused when forced"),
    "hgemm.empty_slice": ("hgemm.hip", 410, "if (c0 < c1)", "every slice has chunks / a slice is empty"),
    "hgemm.kg2": ("hgemm.hip", 1074, "g.K % (2 * GK) == 0", "CGD_HGEMM_KG=2 takes the row (two K-groups) / K = 64, 192 stay on four wavefronts"),
    "kgemm.min_rows": ("hgemm.hip", 966, "p.M > 4", "M >= 5 / M = 4 refused when forced"),
    "kgemm.rows": ("hgemm.hip", 999, "cdiv(g.M, 32 * ni)", "M within one 32- (64-) row tile / a second tile"),
    "hconv.h8": ("hconv.hip", 502, "(p.H & 7)", "H a multiple of 8 / H = 12 refused when forced"),
    "hconv.w16": ("hconv.hip", 502, "(p.W & 15) && p.W != 8", "W a multiple of 16, or 8 / W = 24, 4 refused when forced"),
    "hconv.n32": ("hconv.hip", 500, "(p.N & 31)", "N a multiple of 32 / N = 48 refused when forced"),
    "hconv.h16": ("hconv.hip", 503, "(p.H & 15)", "the 16-row variants: H a multiple of 16 / H = 8, 24 refused when forced"),
    "hconv.cols": ("hconv.hip", 562, "cdiv(g.N, HB_N)", "N <= 128 / N > 128"),
    "hconv.wtiles": ("hconv.hip", 545, "cdiv(p.W, 16)", "one tile column (W = 8 half-filled) / several"),
    "hconv.empty_slice": ("hconv.hip", 263, "if (c0 < c1)", "every slice has chunks / a slice is empty"),
    "hconv.unsplit": ("hconv.hip", 529, "hconv_var & 8", "the 4x16-pixel x 128-channel tile: one 128-channel panel / two"),
    "kconv.supported": ("kconv.hip", 377, "cgd_hconv_supported", "hconv2's shapes at 8-row tiles / H = 12, W = 24, W = 4, N = 48 refused when forced"),
    "kconv.empty_slice": ("kconv.hip", 160, "if (c0 < c1)", "every slice has chunks / a slice is empty"),
    "kconv.th16": ("kconv.hip", 364, "kconv_th16", "CGD_KCONV=..,256: H, W multiples of 16 take the 16x16 tile / the others keep 8 rows"),
    "kconv.blocks": ("kconv.hip", 387, "(g.N >> 5)", "one 32-channel block / several"),
    "wconv.h8": ("wconv.hip", 667, "(p.H & 7)", "H a multiple of 8 / H = 12 refused"),
    "wconv.w16": ("wconv.hip", 667, "(p.W & 15)", "W a multiple of 16 / W = 8 refused"),
    "wconv.h16": ("wconv.hip", 668, "(p.H & 15) && (ctx->wino_mode & 3) == 2", "mode 2: H a multiple of 16 / H = 8, 24 refused"),
    "wconv.nc256": ("wconv.hip", 652, "p.N % 256 == 0", "mode 5: whole 256-channel panels take two channel blocks per wavefront / other N keep one"),
    "wconv.cols": ("wconv.hip", 702, "cdiv(g.N, 128 * nc)", "one channel panel / several, the last partial"),
    "attn.s64": ("attn.hip", 685, "sh.T <= AS_T", "T <= 64 on attn_s64_* (where no flash kernel takes it) / T > 64"),
    "attn.flash": ("attn.hip", 678, "sh.T > 32 && ctx->attn_flash >= 2", "T <= 32 stays on attn_s64_* / 33 is the first T on the flash kernels (modes 2, 3), 65 in mode 1"),
    "attn.block32": ("attn.hip", 769, "cdiv(T, 32)", "T a multiple of the 32-row block / one key or query either side"),
    "attn.generic": ("attn.hip", 687, "ATTN_GENERIC", "d = 64 on a fused family / any other head dim on batched GEMMs"),
    "attn.d80": ("attn.hip", 677, "sh.d != 80", "d = 80: T <= 32 on batched GEMMs / T > 32 on the flash kernels (bf16x3)"),
    "sconv.tile": ("sconv.hip", 292, "big < num_cu", "fewer 128 x 64 tiles than CUs: the 64 x 32 tile / big >= num_cu (256 = num_cu exactly included): 128 x 64"),
    "sconv.rows": ("sconv.hip", 295, "cdiv(M, pl.bm)", "M <= bm: one row tile / a second, ragged one (a_ok, sconv.hip:99)"),
    "sconv.cols": ("sconv.hip", 296, "cdiv(N, pl.bn)", "N <= bn / N > bn (b_off, sconv.hip:110; the last column tile half filled where N % bn)"),
    "sconv.grid8": ("sconv.hip", 298, "cdiv(tiles, 8) * 32", "backward: a tile count that is a multiple of 8 / surplus workgroups return (sconv.hip:82)"),
    "sconv.work": ("sconv.hip", 306, "work < num_cu", "fewer workgroups than CUs: split-K is considered / work >= num_cu: one slice"),
    "sconv.short": ("sconv.hip", 307, "short_nkt / 2", "the slice count comes from the work or the cap of 16 / from two K tiles per slice of the shortest class"),
    "sconv.cap16": ("sconv.hip", 307, ", 16)", "fewer than 16 slices / the cap of 16"),
    "sconv.want2": ("sconv.hip", 309, "want >= 2", "at least two slices: split / the shortest class has fewer than 4 K tiles: one slice"),
    "sconv.empty_slice": ("sconv.hip", 221, "if (kt0 < kt1)", "every slice of every parity class has K tiles / a slice is empty and writes a zero slab"),
    "sconv.size": ("sconv.hip", 364, "H < 2 || W < 2", "a map of at least 2 x 2 / refused"),
    "sconv.even": ("sconv.hip", 365, "(H | W) & 1", "even H and W / refused"),
    "sconv.c32": ("sconv.hip", 366, "(Cin & 31) || (Cout & 31)", "Cin and Cout multiples of 32 / refused"),
    "sconv.ld": ("sconv.hip", 368, "ld_in < c_in || ld_out < c_out", "row strides of at least the channel count / refused"),
    "sconv.ld4": ("sconv.hip", 369, "(ld_in | ld_out | ldadd) & 3", "row strides multiples of 4 / refused"),
    "sconv.lim": ("sconv.hip", 372, ">= lim", "every operand below 2^31 bytes / refused (the far-extent tier sits on the line itself)"),
    "gn.small_hw": ("norm.hip", 1257, "HW <= GN_SMALL_HW", "HW <= 1024: single launch / the chunked kernels"),
    "gn.c32": ("norm.hip", 1213, "C % 32 || C > 4096", "C a multiple of 32 up to 4096 / C = 48, 4128 refused"),
    "gn.v4": ("norm.hip", 1120, "!(cpg & 3)", "4 | C / 32: float4 kernel / scalar kernel"),
    "gn.cache": ("norm.hip", 1124, "8L * (GS_NT >> lg)", "the register-cached single-launch kernel / the streaming one"),
    "gn.chunks": ("norm.hip", 1170, "> 2048", "at most 2048 chunks of 256 pixels / the chunk grows"),
    "ln.vec": ("norm.hip", 1371, "C % 256 == 0 && C <= 1024", "C = 256 ... 1024 in steps of 256: vector kernels / the generic kernel"),
    "ln.rows": ("norm.hip", 1372, "cdiv(rows, 4)", "rows <= 4: one workgroup / two"),
    "act.blocks": ("elem.hip", 294, "elem_grid(n)", "n <= 256: one workgroup / several"),
    "pool.c4": ("elem.hip", 222, "(C & 3)", "C a multiple of 4 / refused"),
    "pool.size": ("elem.hip", 221, "Ho <= 0", "a positive output map / refused"),
    "ups.c4": ("elem.hip", 236, "(C & 3)", "C a multiple of 4 / refused"),
    "ups.even": ("elem.hip", 235, "((Ho | Wo) & 1)", "an even output map (2 x 2 is the smallest) / an odd one has no input map: refused"),
    "bil.c4": ("secondary.hip", 246, "(C & 3)", "C a multiple of 4 / refused"),
    "bil.size": ("secondary.hip", 246, "Hi <= 0", "a positive input map / refused"),
}

# fam: the kernel family the row is about; op: which runner; ctxs: the contexts it runs in; verdict "run" / "refuse"; route: the claimed route
# (ROUTES); text: what a refusal must say; marks: ((clause, "lo" | "hi"), ...); spec: the shape
Row = namedtuple("Row", "fam op name ctxs verdict spec route text marks")
REFUSED = {
    "gemv": "the GEMV kernel takes M <= 4", "hgemm2": "weight GEMM kernel does not support this problem",
    "kgemm": "few-row weight GEMM kernel does not support this problem", "hconv2": "halo conv kernel does not support this problem",
    "kconv": "weight-streaming conv kernel does not support this problem", "wconv": "Winograd conv kernel does not support this problem",
    "gn": "C must be a multiple of 32 and <= 4096", "c4": "C and strides must be multiples of 4", "pool.size": "must be positive",
    "ups.even": "positive and even", "bil": "C and the row strides must be multiples of 4",
    "sconv.size": "B, H and W must be positive", "sconv.even": "H and W must be even", "sconv.c32": "Cin and Cout must be positive multiples of 32",
    "sconv.ld": "a row stride is smaller than its channel count", "sconv.ld4": "row strides must be multiples of 4",
    "sconv.lim": "an operand of 2^31 bytes or more",
}
ROUTES = {
    "gemm": ("igemm/hgemm/kgemm/gemv (kind 0, no halo kernel)", lambda c: c[0] >= 1 and all(c[j] == 0 for j in HALO)),
    "igemm": ("igemm (no halo kernel)", lambda c: c[0] >= 1 and all(c[j] == 0 for j in HALO)),
    "hconv2": ("hconv2", lambda c: c[1] >= 1 and c[3] == 0 and c[4] == 0 and c[0] == 0),
    "kconv": ("kconv", lambda c: c[4] >= 1 and c[3] == 0 and c[1] == 0 and c[0] == 0),
    "wconv": ("wconv", lambda c: c[3] >= 1 and c[1] == 0 and c[4] == 0 and c[0] == 0),
    "gn": ("groupnorm", lambda c: c[2] >= 1 and c[0] == 0),
    "none": ("no profiled kind", lambda c: sum(c) == 0),
    "attn_fused": ("a fused attention family (no GEMM launch)", lambda c: sum(c) == 0),
    "attn_generic": ("batched GEMMs + row softmax", lambda c: c[0] >= 2 and all(c[j] == 0 for j in HALO)),
}


def ceil_div(a, b):
    return -(-a // b)


def empty_slices(units, sk):
    """slices of a split over `units` K units that get none: per = ceil(units / sk), slice z covers [z per, min(units, (z + 1) per))"""
    if sk <= 1:
        return 0
    per = ceil_div(units, sk)
    return sk - ceil_div(units, per)


def _side(cond):
    return "lo" if cond else "hi"


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
IGEMM_TILES = {64: (64, 64), 128: (128, 128), 256: (256, 128)}


def _gemm_rows():
    rows = {}

    def add(fam, ctxs, M, N, K, tile, sk, marks, verdict="run", text=None, op="gemm", tag=""):
        name = f"{fam}{tag} tile{tile} {M}x{N}x{K} sk{sk}"
        if name in rows:
            marks = tuple(rows[name].marks) + tuple(marks)
        rows[name] = Row(fam, op, name, ctxs, verdict, dict(M=M, N=N, K=K, tile=tile, sk=sk), "gemm", text, tuple(marks))

    ctx3 = ("p0", "p1", "p2")
    for tile, (bm, bn) in IGEMM_TILES.items():
        for M in (1, bm - 1, bm, bm + 1):
            add("igemm", ctx3, M, bn + 4, 68, tile, 1, [("igemm.rows", _side(M <= bm))])
        for N in (4, bn - 4, bn, bn + 4, bn + 1):
            add("igemm", ctx3, bm + 1, N, 36, tile, 1, [("igemm.cols", _side(N <= bn))])
        for K in (4, 28, 32, 36, 68):
            add("igemm", ctx3, bm - 1, bn - 4, K, tile, 1, [("igemm.ktail", _side(K % 32 == 0))])
        for N in (bn + 4, bn + 1):  # nkt = 3: sk = 4 leaves one slice empty; N = bn + 1 puts the reduce on its scalar path
            for sk in (1, 2, 3, 4):
                add("igemm", ctx3, bm + 1, N, 68, tile, sk, [("igemm.empty_slice", _side(empty_slices(3, sk) == 0)), ("reduce.vec", _side(N % 4 == 0))])
        add("igemm", ctx3, bm - 1, bn - 4, 32, tile, 2, [("igemm.empty_slice", "hi")])  # nkt = 1, nkt + 1 slices
    # GEMV (517): exact fp32 FMAs in every precision mode
    gv = ("p0", "p1")
    for M in (1, 2, 3, 4):
        for K in (4, 252, 256, 260):
            add("gemv", gv, M, 17, K, 517, 1, [("gemv.kpass", _side(K <= 256)), ("gemv.rows", "lo")])
        for N in (1, 15, 16, 17):
            add("gemv", gv, M, N, 260, 517, 1, [("gemv.cols", _side(N <= 16)), ("gemv.grid", "lo")])
    add("gemv", gv, 2, GEMV_BIG_N, 4, 517, 1, [("gemv.grid", "hi")])
    add("gemv", gv, 4, 40, 3072, 517, 1, [("gemv.lds", "lo")])
    add("gemv", gv, 4, 40, 3076, 517, 1, [("gemv.lds", "hi")], "refuse", REFUSED["gemv"])
    add("fallthrough", gv, 4, 40, 3076, 0, 1, [], tag=" of gemv")
    add("gemv", gv, 5, 40, 260, 517, 1, [("gemv.rows", "hi")], "refuse", REFUSED["gemv"])
    add("fallthrough", gv, 5, 40, 260, 0, 1, [], tag=" of gemv")
    # hgemm2 (513): bf16x3.  64-row tiles at these sizes (hgemm.hip:946-951), 128-row tiles with CGD_HGEMM_VAR=2
    hg = ("p1", "p1_epi0", "p1_kg2", "p1_tm128")

    def hmarks(M, N, K, sk):
        return [("hgemm.rows64", _side(M <= 64)), ("hgemm.rows128", _side(M <= 128)), ("hgemm.cols", _side(N <= 128)), ("hgemm.k64", "lo"),
                ("hgemm.n32", "lo"), ("hgemm.kg2", _side(K % 128 == 0)), ("hgemm.empty_slice", _side(empty_slices(K // 64, sk) == 0))]

    for M in (1, 63, 64, 65, 127, 128, 129):
        add("hgemm2", hg, M, 160, 128, 513, 1, hmarks(M, 160, 128, 1))
    for N in (32, 96, 128, 160):
        add("hgemm2", hg, 65, N, 192, 513, 1, hmarks(65, N, 192, 1))
    for K in (64, 128, 192):
        add("hgemm2", hg, 129, 96, K, 513, 1, hmarks(129, 96, K, 1))
    for (M, N, K) in ((65, 160, 192), (129, 96, 128), (64, 32, 64)):
        for sk in sorted({1, 2, K // 64, K // 64 + 1}):
            add("hgemm2", hg, M, N, K, 513, sk, hmarks(M, N, K, sk))
    for (M, N, K, clause) in ((65, 96, 96, "hgemm.k64"), (65, 48, 128, "hgemm.n32")):
        add("hgemm2", ("p1",), M, N, K, 513, 1, [(clause, "hi")], "refuse", REFUSED["hgemm2"])
        add("fallthrough", ("p1",), M, N, K, 0, 1, [], tag=" of hgemm2")
    # kgemm (518): 32-row tiles, 64-row tiles with CGD_KGEMM=2,256,1
    kg = ("p1", "p1_kgemm64")
    for M in (5, 31, 32, 33, 63, 64, 65):
        add("kgemm", kg, M, 96, 320, 518, 1, [("kgemm.rows", _side(M <= 32)), ("kgemm.min_rows", "lo")])
    for N in (32, 64, 96):
        add("kgemm", kg, 33, N, 128, 518, 1, [("kgemm.rows", "hi")])
    for K in (64, 128, 256, 320):
        add("kgemm", kg, 65, 64, K, 518, 1, [("kgemm.rows", "hi")])
    add("kgemm", ("p1",), 4, 96, 128, 518, 1, [("kgemm.min_rows", "hi")], "refuse", REFUSED["kgemm"])
    add("fallthrough", ("p1",), 4, 96, 128, 0, 1, [], tag=" of kgemm")
    return list(rows.values())


def _conv_spec(B, H, W, Ci, Co, tile, var=0, ups=0, sk=1, dgrad=0):
    return dict(B=B, H=H, W=W, Ci=Ci, Co=Co, tile=tile, var=var, ups=ups, sk=sk, dgrad=dgrad)


def _conv_name(fam, s, tag=""):
    return (f"{fam}{tag} tile{s['tile']} var{s['var']} B{s['B']} {s['H']}x{s['W']} {s['Ci']}->{s['Co']} ups{s['ups']} sk{s['sk']}"
            + (" dgrad" if s["dgrad"] else ""))


def _halo_rows():
    rows = {}

    def add(fam, ctxs, spec, marks, verdict="run", text=None, route=None, tag=""):
        name = _conv_name(fam, spec, tag)
        if name in rows:
            marks = tuple(rows[name].marks) + tuple(marks)
        rows[name] = Row(fam, "conv", name, ctxs, verdict, spec, route or fam, text, tuple(marks))

    for fam, tile, variants, ctxs in (("hconv2", 512, (0, 1, 4, 5, 8), ("p1",)), ("kconv", 516, (0,), ("p1", "p1_kconv16"))):
        es = fam.rstrip("2") + ".empty_slice"
        for var in variants:
            h16, unsplit = bool(var & 1), var == 8
            H0 = 16 if h16 else 8
            wide, n0 = (256 if unsplit else 160), (128 if unsplit else 32)

            def marks(s, fam=fam, unsplit=unsplit, es=es):
                m = [(es, _side(empty_slices(s["Ci"] // 32, s["sk"]) == 0))]
                if fam == "hconv2":
                    m += [("hconv.h8", "lo"), ("hconv.w16", "lo"), ("hconv.n32", "lo"), ("hconv.cols", _side(s["Co"] <= 128)),
                          ("hconv.wtiles", _side(s["W"] <= 16))]
                    if unsplit:
                        m.append(("hconv.unsplit", _side(s["Co"] <= 128)))
                    if s["var"] & 1:
                        m.append(("hconv.h16", "lo"))
                else:
                    m += [("kconv.supported", "lo"), ("kconv.blocks", _side(s["Co"] == 32)),
                          ("kconv.th16", _side(s["H"] % 16 == 0 and s["W"] % 16 == 0))]
                return m

            shapes = [_conv_spec(2, H, 16, 32, n0, tile, var) for H in ((16,) if h16 else (8, 16, 24))]
            shapes += [_conv_spec(1, H0, W, 64, 128 if unsplit else 96, tile, var) for W in (8, 16, 32, 48)]
            shapes += [_conv_spec(1, H0, 8, Ci, wide, tile, var) for Ci in (32, 64, 96)]
            shapes += [_conv_spec(2, 16, 16, 32, N, tile, var) for N in ((128, 256) if unsplit else (32, 96, 128, 160))]
            shapes += [_conv_spec(1, H0, W, 32, n0, tile, var) for W in (8, 16)]  # the smallest maps with the smallest Cin and N together
            shapes.append(_conv_spec(1, 16, 32, 64, 128 if unsplit else 96, tile, var, ups=1))
            shapes.append(_conv_spec(1, 16, 16, 128 if unsplit else 96, 64, tile, var, dgrad=1))
            if not unsplit:  # (the unsplit tile holds all of K in one workgroup: a split launch keeps the variant's ordinary tile)
                shapes += [_conv_spec(1, H0, 16, 96, 96, tile, var, sk=sk) for sk in (1, 2, 3, 4)]
                shapes.append(_conv_spec(1, H0, 16, 576, 32, tile, var, sk=7))  # 18 chunks in 7 slices of 3: the seventh is empty
            for s in shapes:
                add(fam, ctxs, s, marks(s))
        # refused when forced, then again with force_tile = 0
        bad = [(_conv_spec(1, 12, 16, 32, 32, tile), "hconv.h8"), (_conv_spec(1, 8, 24, 32, 32, tile), "hconv.w16"),
               (_conv_spec(1, 8, 4, 32, 32, tile), "hconv.w16"), (_conv_spec(1, 8, 16, 32, 48, tile), "hconv.n32")]
        if fam == "hconv2":
            bad += [(_conv_spec(1, 8, 16, 32, 32, tile, 1), "hconv.h16"), (_conv_spec(1, 24, 16, 32, 32, tile, 1), "hconv.h16")]
        for s, clause in bad:
            add(fam, ("p1",), s, [(clause if fam == "hconv2" else "kconv.supported", "hi")], "refuse", REFUSED[fam])
            # (with the default variant the two maps the 16-row variant refuses are small maps of the weight-streaming kernel)
            add("fallthrough", ("p1",), dict(s, tile=0, var=0), [], route="kconv" if clause == "hconv.h16" else "igemm", tag=f" of {fam}")
    return list(rows.values())


def _wino_rows():
    rows = {}

    def add(fam, op, ctxs, spec, marks, verdict="run", text=None, route="wconv", name=None):
        rows[name] = Row(fam, op, name, ctxs, verdict, spec, route, text, tuple(marks))

    for mode in (2, 3, 5):
        ctxs = ("p1",) if mode == 2 else ("p1", "p0")
        Hs = (16,) if mode == 2 else (8, 16, 24)
        H0 = Hs[0]
        shapes = [(2, H, 16, 32, 32, 0, i & 1) for i, H in enumerate(Hs)]
        shapes += [(1, H0, W, 64, 96, 0, i & 1) for i, W in enumerate((16, 32, 48))]
        shapes += [(1, 16, 32, 32, N, 0, (i + 1) & 1) for i, N in enumerate((32, 96, 128, 160) + ((256, 512) if mode == 5 else ()))]
        shapes += [(1, H0, 16, 32, 32, 0, 0), (1, H0, 16, 32, 32, 0, 1), (1, 16, 32, 32, 64, 1, 1)]
        for (B, H, W, Ci, Co, ups, gn) in shapes:
            s = dict(B=B, H=H, W=W, Ci=Ci, Co=Co, ups=ups, gn=gn, mode=mode)
            m = [("wconv.h8", "lo"), ("wconv.w16", "lo"), ("wconv.cols", _side(Co <= 128))]
            if mode == 2:
                m.append(("wconv.h16", "lo"))
            if mode == 5:
                m.append(("wconv.nc256", _side(Co % 256 == 0)))
            add("wconv", "wino", ctxs, s, m, name=f"wconv m{mode} B{B} {H}x{W} {Ci}->{Co} ups{ups} gn{gn}")
        bad = [((1, 8, 8, 32, 32), "wconv.w16"), ((1, 12, 16, 32, 32), "wconv.h8")]
        if mode == 2:
            bad += [((1, 8, 16, 32, 32), "wconv.h16"), ((1, 24, 16, 32, 32), "wconv.h16")]
        for (B, H, W, Ci, Co), clause in bad:
            s = dict(B=B, H=H, W=W, Ci=Ci, Co=Co, ups=0, gn=0, mode=mode)
            add("wconv", "wino", ctxs, s, [(clause, "hi")], "refuse", REFUSED["wconv"], name=f"wconv m{mode} B{B} {H}x{W} {Ci}->{Co} ups0 gn0")
            # cgd_op_conv3x3 with force_tile = 0: exact-fp32 contexts have the implicit GEMM only below wino_min_m; bf16x3 contexts put the small
            # maps that kconv accepts on it (8 x 8, 8 x 16, 24 x 16) and 12 x 16 on the implicit GEMM
            cs = _conv_spec(B, H, W, Ci, Co, 0)
            for ck in ctxs:
                route = "igemm" if ck == "p0" or H == 12 else "kconv"
                add("fallthrough", "conv", (ck,), cs, [], route=route, name=_conv_name("fallthrough", cs, f" of wconv[{ck}]"))  # (one per shape)
    return list(rows.values())


def attn_family(T, d, ck):
    """restatement of attn.hip attn_select for a dense op-level call (row strides multiples of 4): 0 generic, 1 s64, 2 mid, 3 flash"""
    prec, env = CONTEXTS[ck]
    x3 = prec == 1 and env.get("CGD_ATTN_X3", "1") != "0"
    flash = int(env.get("CGD_ATTN_FLASH", "3"))
    if x3 and d in (64, 80) and ((T > 64 and flash >= 1) or (32 < T <= 64 and flash >= 2)):
        return 3
    if d == 64:
        return 1 if T <= 64 else 2
    return 0


def _attn_rows():
    rows = []
    T64 = (1, 2, 7, 16, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129)

    def add(nb, heads, T, d, legacy, causal=0):
        m = [("attn.block32", _side(T % 32 == 0)), ("attn.generic", _side(d == 64))]
        if d == 64:
            m += [("attn.s64", _side(T <= 64)), ("attn.flash", _side(T <= 32))]
        if d == 80:
            m.append(("attn.d80", _side(T <= 32)))
        name = f"attn{' causal' if causal else ''} nb{nb} h{heads} T{T} d{d} legacy{legacy}"
        rows.append(Row("attn", "attn", name, ATTN_CTXS, "run", dict(nb=nb, heads=heads, T=T, d=d, legacy=legacy, causal=causal), "attn", None, tuple(m)))

    # layouts x (nb, heads) pairwise: the whole T sweep on (legacy, (2, 3)) and ([Q | K | V], (1, 1)), the other two pairs at the family changes
    for T in T64:
        add(2, 3, T, 64, 1)
        add(1, 1, T, 64, 0)
    for T in (1, 33, 65, 129):
        add(1, 1, T, 64, 1)
        add(2, 3, T, 64, 0)
    for T in (31, 32, 33, 65):
        add(2, 3, T, 80, 0)
    for i, d in enumerate((4, 32, 96, 192, 256)):
        for T in (1, 5, 64, 65):
            add(2, 2, T, d, i & 1)
    for T in (1, 2, 31, 32, 33, 65):
        add(2, 3, T, 64, 0, causal=1)
    # one head of 512 channels over a 16 x 16 map (the community checkpoints of the classic architecture at a 256 x 256 frame) and one
    # position either side: batched GEMMs with K = 512 (QK^T) and K = T (PV), both head orders
    for T in (255, 256, 257):
        for nb in (1, 2):
            for legacy in (0, 1):
                add(nb, 1, T, 512, legacy)
    return rows


def gn_kernel(HW, C):
    """restatement of norm.hip launch_gn_small_fwd for aligned operands: (float4?, register-cached?) or 'chunked'"""
    if HW > 1024:
        return "chunked"
    cpg = C // 32
    v4 = cpg % 4 == 0
    cq = cpg // 4 if v4 else cpg
    lg = max(0, (cq - 1).bit_length())
    return ("v4" if v4 else "scalar", "cached" if HW <= 8 * (1024 >> lg) else "streaming")


def gn_chunk(HW, B):
    """restatement of norm.hip pick_chunk"""
    chunk = min(max(HW * B // 512, 8), 256)
    if ceil_div(HW, chunk) > 2048:
        chunk = (HW + 2047) // 2048
    return min(chunk, HW)


def _norm_rows():
    rows = []

    def gn(B, HW, C, bwd=1, verdict="run", marks=()):
        m = list(marks)
        if verdict == "run":
            k = gn_kernel(HW, C)
            m += [("gn.small_hw", _side(HW <= 1024)), ("gn.c32", "lo")]
            if k != "chunked":
                m += [("gn.v4", _side(k[0] == "v4")), ("gn.cache", _side(k[1] == "cached"))]
            else:
                m.append(("gn.chunks", _side(ceil_div(HW, min(max(HW * B // 512, 8), 256)) <= 2048)))
        rows.append(Row("gn", "gn", f"gn B{B} HW{HW} C{C}" + ("" if bwd else " fwd only"), ("p1",), verdict, dict(B=B, HW=HW, C=C, bwd=bwd),
                        "gn", REFUSED["gn"] if verdict == "refuse" else None, tuple(m)))

    for C_ in (32, 64):
        for HW in (1, 2, 3, 1023, 1024, 1025, 1152):
            for B in (1, 3):
                gn(B, HW, C_)
    # C = 4096 (the cap; 128 channels per group on the float4 kernels): HW pairwise with B, the streaming kernel from 257 pixels on
    for (B, HW) in ((1, 1), (3, 2), (1, 3), (3, 256), (1, 257), (1, 1024), (1, 1025)):
        gn(B, HW, 4096)
    gn(1, 524288, 32, bwd=0)  # exactly 2048 chunks of 256 pixels
    gn(1, 524296, 32, bwd=0)  # 2049 chunks of 256: the chunk grows to 257 pixels (2041 chunks, the last one holds 16)
    gn(1, 16, 48, verdict="refuse", marks=[("gn.c32", "hi")])
    gn(1, 16, 4128, verdict="refuse", marks=[("gn.c32", "hi")])
    for r in (1, 2, 3, 4, 5):
        for C_ in (4, 252, 256, 260, 1024, 1280):
            rows.append(Row("ln", "ln", f"ln {r}x{C_}", ("p1",), "run", dict(rows=r, C=C_), "none", None,
                            (("ln.vec", _side(C_ % 256 == 0 and C_ <= 1024)), ("ln.rows", _side(r <= 4)))))
    return rows


def _elem_rows():
    rows = []
    for kind in (1, 2):
        for n in (1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025):
            for bwd in (0, 1):
                rows.append(Row("act", "act", f"act{kind} {'bwd' if bwd else 'fwd'} n{n}", ("p1",), "run", dict(kind=kind, n=n, bwd=bwd), "none", None,
                                (("act.blocks", _side(n <= 256)),)))

    def rs(fam, B, H, W, C_, adj=0, verdict="run", text=None, marks=()):
        nm = f"{fam} B{B} {H}x{W} C{C_}" + (" adjoint" if adj else "")
        rows.append(Row(fam, fam, nm, ("p1",), verdict, dict(B=B, H=H, W=W, C=C_, adj=adj), "none", text, tuple(marks)))

    # (H, W) = the OUTPUT map of pool2x2 / upsample2x and the INPUT map of bilinear_up2x, as their entries take it.  Channel counts: 4 is the
    # smallest the launchers accept (float4 accesses), 12 is not a power of two
    for (B, H, W, C_) in ((1, 1, 1, 4), (2, 1, 5, 4), (2, 5, 1, 12), (1, 1, 1, 12), (2, 3, 3, 4)):
        rs("pool2x2", B, H, W, C_, marks=[("pool.c4", "lo"), ("pool.size", "lo")])
    rs("pool2x2", 1, 2, 2, 6, verdict="refuse", text=REFUSED["c4"], marks=[("pool.c4", "hi")])
    rs("pool2x2", 1, 0, 2, 4, verdict="refuse", text=REFUSED["pool.size"], marks=[("pool.size", "hi")])
    for (B, H, W, C_) in ((1, 2, 2, 4), (2, 2, 10, 4), (2, 10, 2, 12), (1, 2, 2, 12), (2, 6, 6, 4)):
        rs("upsample2x", B, H, W, C_, marks=[("ups.c4", "lo"), ("ups.even", "lo")])
    rs("upsample2x", 1, 2, 2, 6, verdict="refuse", text=REFUSED["c4"], marks=[("ups.c4", "hi")])
    for (H, W) in ((1, 1), (1, 4), (4, 1), (3, 2)):  # an output of 1 x 1, 1 x W or H x 1 has no input map
        rs("upsample2x", 2, H, W, 4, verdict="refuse", text=REFUSED["ups.even"], marks=[("ups.even", "hi")])
    for adj in (0, 1):
        for (B, H, W, C_) in ((1, 1, 1, 4), (2, 1, 5, 4), (2, 5, 1, 12), (1, 1, 1, 12), (2, 3, 3, 4)):
            rs("bilinear_up2x", B, H, W, C_, adj, marks=[("bil.c4", "lo"), ("bil.size", "lo")])
        rs("bilinear_up2x", 1, 2, 2, 6, adj, verdict="refuse", text=REFUSED["bil"], marks=[("bil.c4", "hi")])
        rs("bilinear_up2x", 1, 0, 2, 4, adj, verdict="refuse", text=REFUSED["bil"], marks=[("bil.size", "hi")])
    return rows


def sconv_plan(dgrad, B, H, W, Ci, Co, num_cu=NUM_CU):
    """restatement of sconv.hip sconv_select for a dense problem: dict(M, N, Kc, bm, bn, ntm, ntn, tiles, work, short, want, sk, wg).  M: rows
    (per parity class in the backward), want: the slice count before `want >= 2` (the 256 MiB workspace never binds: the host file enumerates)"""
    M, N, Kc = B * (H // 2) * (W // 2), (Ci if dgrad else Co), (Co if dgrad else Ci)
    cls = 4 if dgrad else 1
    small = ceil_div(M, 128) * ceil_div(N, 64) * cls < num_cu
    bm, bn = (64, 32) if small else (128, 64)
    ntm, ntn = ceil_div(M, bm), ceil_div(N, bn)
    tiles = ntm * ntn
    work, short = tiles * cls, (1 if dgrad else 9) * (Kc // 32)
    want = min(ceil_div(2 * num_cu, work), short // 2, 16) if work < num_cu else 1
    sk = want if want >= 2 else 1
    return dict(M=M, N=N, Kc=Kc, bm=bm, bn=bn, ntm=ntm, ntn=ntn, tiles=tiles, work=work, short=short, want=want, sk=sk,
                wg=(ceil_div(tiles, 8) * 32 if dgrad else tiles) * sk)


def sconv_empty(dgrad, Kc, sk):
    """empty slices per parity class (taps 1, 2, 2, 4; the forward is one class of 9 taps)"""
    return [empty_slices(t * (Kc // 32), sk) for t in ((1, 2, 2, 4) if dgrad else (9,))]


def _sconv_rows():
    rows = {}
    ctx3 = ("p0", "p1", "p2")

    def add(dgrad, B, H, W, Kc, N, verdict="run", text=None, marks=(), ctxs=ctx3, ld=(0, 0, 0), tag=""):
        Ci, Co = (N, Kc) if dgrad else (Kc, N)
        name = f"sconv{tag} {'bwd' if dgrad else 'fwd'} B{B} {H}x{W} {Ci}->{Co}"
        m = list(marks)
        if verdict == "run":
            p = sconv_plan(dgrad, B, H, W, Ci, Co)
            m += [("sconv.tile", _side(p["bm"] == 64)), ("sconv.rows", _side(p["M"] <= p["bm"])), ("sconv.cols", _side(N <= p["bn"])),
                  ("sconv.work", _side(p["work"] < NUM_CU)), ("sconv.empty_slice", _side(not any(sconv_empty(dgrad, Kc, p["sk"])))),
                  ("sconv.size", "lo"), ("sconv.even", "lo"), ("sconv.c32", "lo"), ("sconv.ld", "lo"), ("sconv.ld4", "lo"), ("sconv.lim", "lo")]
            if dgrad:
                m.append(("sconv.grid8", _side(p["tiles"] % 8 == 0)))
            if p["work"] < NUM_CU:
                m += [("sconv.want2", _side(p["want"] >= 2)), ("sconv.short", _side(p["want"] < p["short"] // 2)),
                      ("sconv.cap16", _side(p["want"] < 16))]
        if name in rows:
            m = list(rows[name].marks) + m
        rows[name] = Row("sconv", "sconv", name, ctxs, verdict, dict(dgrad=dgrad, B=B, H=H, W=W, Ci=Ci, Co=Co, ld=ld), "igemm", text, tuple(m))

    # rows per parity class M = B (H / 2) (W / 2): 63 / 64 / 65 around the 64-row tile, 127 / 128 / 129 around two of them, from non-square maps and
    # B = 3 so that a tile crosses a sample boundary (63 = 3 x (3 x 7), 129 = 3 x (1 x 43)) and a map-row boundary (65 = 5 x 13, 129 = 3 x 43);
    # 127 = 1 x 127 is one output row of a map with H = 2
    MS = ((3, 6, 14), (1, 8, 32), (1, 10, 26), (1, 2, 254), (1, 16, 32), (1, 6, 86), (3, 2, 86))
    for dgrad in (0, 1):
        for (B, H, W) in MS:
            add(dgrad, B, H, W, 32, 96)  # (backward: 3 column tiles x 1 / 2 / 3 row tiles = 3 / 6 / 9 tiles of the 8-tile groups)
        for N in (32, 64, 96, 160):
            add(dgrad, 1, 10, 26, 64, N)
        for Kc in (32, 64, 96, 128, 288):  # one tile: forward 4 / 9 / 13 / 16 / 16 slices; backward 1 / 1 / 1 / 2 / 4, the last with an empty one
            add(dgrad, 3, 6, 14, Kc, 32)
        add(dgrad, 1, 26, 2, 64, 64)  # one output column
        add(dgrad, 1, 2, 2, 32, 32)  # one output pixel: five of the nine taps are padding
        add(dgrad, 2, 4, 4, 1024, 32)  # backward: 32 K tiles in the one-tap class, the cap of 16 slices
    add(1, 1, 32, 56, 32, 32)  # backward: 7 tiles
    add(1, 1, 16, 32, 32, 128)  # backward: 8 tiles
    # either side of `big < num_cu` at 256 CUs: the forward of 256 x 256 x 128 -> 128 is 128 x 2 = 256 tiles of 128 x 64, the backward of
    # 128 x 128 x 128 <- 128 is 32 x 2 x 4; one row of tiles fewer takes the 64 x 32 tile.  The ragged 128-row tile: 16383 = 129 x 127 rows in the
    # forward and 4095 = 63 x 65 per class in the backward hold 127 rows in their last tile (32 channels per tap keep the reference cheap)
    add(0, 1, 256, 256, 128, 128)
    add(0, 1, 254, 256, 128, 128)
    add(0, 1, 258, 254, 32, 128)
    add(1, 1, 128, 128, 128, 128)
    add(1, 1, 124, 128, 128, 128)
    add(1, 1, 126, 130, 32, 128)
    # either side of `work < num_cu`: 64 x 4 = 256 tiles of 64 x 32 forward (63 x 4 = 252: 3 slices), 16 x 4 x 4 = 256 backward (15 x 4 x 4 = 240:
    # two slices, two K tiles each in the one-tap class)
    add(0, 1, 128, 128, 32, 128)
    add(0, 1, 126, 128, 32, 128)
    add(1, 1, 64, 64, 128, 128)
    add(1, 1, 60, 64, 128, 128)
    # every clause of cgd_sconv_refusal, forward and backward (ld: what is added to the row stride of the gathered / written / add operand)
    for dgrad in (0, 1):
        r = dict(verdict="refuse", ctxs=("p1",))
        add(dgrad, 1, 0, 4, 32, 32, text=REFUSED["sconv.size"], marks=[("sconv.size", "hi")], **r)
        add(dgrad, 1, 6, 5, 32, 32, text=REFUSED["sconv.even"], marks=[("sconv.even", "hi")], **r)
        add(dgrad, 1, 3, 4, 32, 32, text=REFUSED["sconv.even"], marks=[("sconv.even", "hi")], **r)
        add(dgrad, 1, 4, 4, 48, 32, text=REFUSED["sconv.c32"], marks=[("sconv.c32", "hi")], **r)
        add(dgrad, 1, 4, 4, 32, 80, text=REFUSED["sconv.c32"], marks=[("sconv.c32", "hi")], **r)
        add(dgrad, 1, 4, 4, 64, 32, text=REFUSED["sconv.ld"], marks=[("sconv.ld", "hi")], ld=(-12, 0, 0), tag=" ld_in = channels - 4", **r)
        add(dgrad, 1, 4, 4, 32, 64, text=REFUSED["sconv.ld"], marks=[("sconv.ld", "hi")], ld=(0, -12, 0), tag=" ld_out = channels - 4", **r)
        add(dgrad, 1, 4, 4, 32, 32, text=REFUSED["sconv.ld4"], marks=[("sconv.ld4", "hi")], ld=(2, 0, 0), tag=" ld_in+2", **r)
        add(dgrad, 1, 4, 4, 32, 32, text=REFUSED["sconv.ld4"], marks=[("sconv.ld4", "hi")], ld=(0, 6, 0), tag=" ld_out+6", **r)
        # 16 (4 in the half-size map) rows at a row stride of 2^28 floats more than the channels: the fourth row ends beyond 2^31 bytes.  Refused before anything is read
        add(dgrad, 1, 4, 4, 32, 32, text=REFUSED["sconv.lim"], marks=[("sconv.lim", "hi")], ld=(2 ** 28, 0, 0), tag=" ld_in far", **r)
        add(dgrad, 1, 4, 4, 32, 32, text=REFUSED["sconv.lim"], marks=[("sconv.lim", "hi")], ld=(0, 2 ** 28, 0), tag=" ld_out far", **r)
    add(1, 1, 4, 4, 32, 64, text=REFUSED["sconv.ld"], marks=[("sconv.ld", "hi")], ld=(0, 0, -8), tag=" ldadd = channels - 4", verdict="refuse", ctxs=("p1",))
    add(1, 1, 4, 4, 32, 32, text=REFUSED["sconv.ld4"], marks=[("sconv.ld4", "hi")], ld=(0, 0, 2), tag=" ldadd+2", verdict="refuse", ctxs=("p1",))
    add(1, 1, 4, 4, 32, 32, text=REFUSED["sconv.lim"], marks=[("sconv.lim", "hi")], ld=(0, 0, 2 ** 28), tag=" ldadd far", verdict="refuse", ctxs=("p1",))
    return list(rows.values())


TABLE = _gemm_rows() + _halo_rows() + _wino_rows() + _attn_rows() + _norm_rows() + _elem_rows() + _sconv_rows()
GROUPS = sorted({(r.fam, ck) for r in TABLE for ck in r.ctxs})


def rows_of(fam, ck):
    return [r for r in TABLE if r.fam == fam and ck in r.ctxs]


# ---- inputs and float64 references, shared by the GPU runners and the host file -------------------------------------------------------
def _r(shape, seed, scale=1.0):
    return scale * th.randn(*shape, generator=g(seed))


@functools.lru_cache(maxsize=None)
def gemm_data(M, N, K, dtype=th.float64):
    a, b, bias, r = _r((M, K), 1), _r((N, K), 2), _r((N,), 3, 0.3), _r((M, N), 4, 0.3)
    alpha = 1.0 / math.sqrt(K)
    ref = alpha * (a.to(dtype) @ b.to(dtype).T) + bias.to(dtype) + r.to(dtype)
    return a, b, bias, r, alpha, ref


@functools.lru_cache(maxsize=None)
def conv_data(B, H, W, Ci, Co, ups, dgrad, gn=0):
    """inputs of one conv row in the torch layout and its float64 reference: x (B,Hs,Ws,cin) NHWC, w (Co,Ci,3,3), bias (forward only),
    residual, optional GroupNorm pairs {a, b}; a dgrad row convolves Co -> Ci channels with the rotated, transposed weights"""
    cin, cout = (Co, Ci) if dgrad else (Ci, Co)
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    w = _r((Co, Ci, 3, 3), 6) / math.sqrt(9 * cin)
    x = _r((B, Hs, Ws, cin), 5)
    b = None if dgrad else _r((cout,), 7, 0.3)
    r = _r((B, H, W, cout), 17, 0.3)
    ab = th.stack([0.5 + th.rand(B, cin, generator=g(18)), 0.5 * th.randn(B, cin, generator=g(19))], dim=2).contiguous() if gn else None
    wref = w.flip(2, 3).transpose(0, 1) if dgrad else w
    return x, w, b, r, ab, _conv_ref(x, wref, b, ups, r, ab)


@functools.lru_cache(maxsize=None)
def sconv_data(dgrad, B, H, W, Ci, Co, dtype=th.float64):
    """one stride-2 conv row, NHWC: forward (x, w, bias, y = conv2d(stride=2, padding=1)); backward (dy at unit-peak gradient, w, add, dx = the
    autograd gradient of that conv2d + add)"""
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    w = _r((Co, Ci, 3, 3), 52) / math.sqrt(9 * Ci)
    x = _r((B, H, W, Ci), 51)
    if not dgrad:
        b = _r((Co,), 53, 0.3)
        y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype), b.to(dtype), stride=2, padding=1)
        return x, w, b, nhwc(y)
    dy, add = _r((B, H // 2, W // 2, Co), 54), _r((B, H, W, Ci), 55, 0.3)
    xr = x.to(dtype).permute(0, 3, 1, 2).requires_grad_()
    (gx,) = th.autograd.grad(F.conv2d(xr, w.to(dtype), None, stride=2, padding=1), xr, dy.to(dtype).permute(0, 3, 1, 2))
    sd = unit_seed(gx)
    return dy * sd, w, add, nhwc(gx) * sd + add.to(dtype)


def attn_cols(heads, d, legacy):
    """column indices of q, k and v inside a qkv row of 3 heads d floats"""
    Cc = heads * d
    if not legacy:
        return [th.arange(i * Cc, (i + 1) * Cc) for i in range(3)]
    base = th.arange(heads)[:, None] * 3 * d + th.arange(d)[None, :]
    return [(base + i * d).reshape(-1) for i in range(3)]


def _attn_ref(qkv, nb, heads, T, d, legacy, causal):
    Cc = heads * d
    x = qkv.reshape(nb, T, 3 * Cc).permute(0, 2, 1)
    if legacy:
        q, k, v = x.reshape(nb * heads, 3 * d, T).split(d, dim=1)
    else:
        q, k, v = (z.reshape(nb * heads, d, T) for z in x.chunk(3, dim=1))
    s = 1 / math.sqrt(math.sqrt(d))
    logits = th.einsum("bct,bcs->bts", q * s, k * s)
    if causal:
        logits = logits.masked_fill(th.ones(T, T, dtype=th.bool).triu(1), float("-inf"))
    a = th.einsum("bts,bcs->bct", th.softmax(logits, dim=-1), v).reshape(nb, Cc, T)
    return a.permute(0, 2, 1).reshape(nb * T, Cc)


@functools.lru_cache(maxsize=None)
def attn_data(nb, heads, T, d, legacy, causal, dtype=th.float64):
    Cc = heads * d
    qkv, dout = _r((nb * T, 3 * Cc), 40), _r((nb * T, Cc), 41)
    qr = qkv.to(dtype).requires_grad_()
    ref = _attn_ref(qr, nb, heads, T, d, legacy, causal)
    if causal:
        return qkv, None, ref.detach(), None
    (ref * dout.to(dtype)).sum().backward()
    sd = unit_seed(qr.grad)
    return qkv, dout * sd, ref.detach(), qr.grad * sd


@functools.lru_cache(maxsize=2)
def gn_data(B, HW, C_, bwd, dtype=th.float64):
    """GroupNorm(32) + FiLM + SiLU of x (B,HW,C) and, with bwd, dx for the seed dz (unit peak) plus the `add` operand"""
    x = _r((B, HW, C_), 20) * 2 + 0.7
    gamma, beta, film = 1 + 0.1 * _r((C_,), 21), 0.1 * _r((C_,), 22), 0.3 * _r((B, 2 * C_), 23)
    xr = x.to(dtype).requires_grad_(bool(bwd))
    # (written out: F.group_norm refuses one value per channel, which B = 1, HW = 1 is)
    xg = xr.reshape(B, HW, 32, C_ // 32)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((xg - mean) / (var + 1e-5).sqrt()).reshape(B, HW, C_) * gamma.to(dtype) + beta.to(dtype)
    y = F.silu(y * (1 + film.to(dtype)[:, None, :C_]) + film.to(dtype)[:, None, C_:])
    if not bwd:
        return x, gamma, beta, film, y.detach(), None, None, None
    dz, add = _r((B, HW, C_), 24), _r((B, HW, C_), 25, 0.3)
    (y * dz.to(dtype)).sum().backward()
    # A group of n values leaves the gradient n - 2 degrees of freedom: with one or two values per group (HW = 1, 2 at one channel per group,
    # HW = 1 at two) the gradient through the norm is zero up to terms in eps / var, a difference of nearly equal numbers that a unit-peak seed
    # would blow up to O(1) in fp32 PyTorch as well.  Those rows keep the seed as drawn; their dx is the `add` operand plus that remainder.
    sd = unit_seed(xr.grad) if HW * (C_ // 32) > 2 else 1.0
    return x, gamma, beta, film, y.detach(), dz * sd, add, xr.grad * sd + add.to(dtype)


@functools.lru_cache(maxsize=None)
def ln_data(rows, C_, dtype=th.float64):
    x = _r((rows, C_), 25) * 1.5 + 0.3
    gamma, beta, dy = 1 + 0.1 * _r((C_,), 26), 0.1 * _r((C_,), 27), _r((rows, C_), 28)
    xr = x.to(dtype).requires_grad_()
    y = F.layer_norm(xr, (C_,), gamma.to(dtype), beta.to(dtype), 1e-5)
    (y * dy.to(dtype)).sum().backward()
    sd = unit_seed(xr.grad)
    return x, gamma, beta, y.detach(), dy * sd, xr.grad * sd


@functools.lru_cache(maxsize=None)
def act_data(kind, n, dtype=th.float64):
    v, dy = _r((n,), 31, 3.0), _r((n,), 32)
    vr = v.to(dtype).requires_grad_()
    yy = F.silu(vr) if kind == 1 else vr * th.sigmoid(1.702 * vr)
    (yy * dy.to(dtype)).sum().backward()
    return v, dy, yy.detach(), vr.grad


@functools.lru_cache(maxsize=None)
def resample_data(fam, B, H, W, C_, adj, dtype=th.float64):
    """(input NHWC, float64 output NHWC); H x W is the output map of pool2x2 / upsample2x and the input map of bilinear_up2x"""
    nchw = lambda t: t.permute(0, 3, 1, 2)  # noqa: E731
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()  # noqa: E731
    if fam == "pool2x2":
        x = _r((B, 2 * H, 2 * W, C_), 30)
        return x, nhwc(F.avg_pool2d(nchw(x.to(dtype)), 2))
    if fam == "upsample2x":
        x = _r((B, H // 2, W // 2, C_), 30)
        return x, nhwc(F.interpolate(nchw(x.to(dtype)), scale_factor=2, mode="nearest"))
    if not adj:
        x = _r((B, H, W, C_), 30)
        return x, nhwc(F.interpolate(nchw(x.to(dtype)), scale_factor=2, mode="bilinear", align_corners=False))
    gup = _r((B, 2 * H, 2 * W, C_), 33)  # the gradient of the upsampled map; the adjoint of a linear map is its autograd gradient
    lo = th.zeros(B, C_, H, W, dtype=dtype, requires_grad=True)
    (F.interpolate(lo, scale_factor=2, mode="bilinear", align_corners=False) * nchw(gup.to(dtype))).sum().backward()
    return gup, nhwc(lo.grad)


def bound_fraction(got, ref):
    """largest |got - ref| in units of the bound 1e-4 + 1e-3 |ref|"""
    ref = ref.double()
    return ((got.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max().item() if ref.numel() else 0.0


def references(row, dtype=th.float64):
    """[(label, reference tensor)] of a row that runs, computed in `dtype` (the host file compares fp32 with float64 and checks the peaks)"""
    s = row.spec
    if row.op == "gemm":
        return [("C", gemm_data(s["M"], s["N"], s["K"], dtype)[5])]
    if row.op == "conv":
        return [("y", conv_data(s["B"], s["H"], s["W"], s["Ci"], s["Co"], s["ups"], s["dgrad"])[5])]
    if row.op == "wino":
        return [("y", conv_data(s["B"], s["H"], s["W"], s["Ci"], s["Co"], s["ups"], 0, s["gn"])[5])]
    if row.op == "sconv":
        return [("dx" if s["dgrad"] else "y", sconv_data(s["dgrad"], s["B"], s["H"], s["W"], s["Ci"], s["Co"], dtype)[3])]
    if row.op == "attn":
        _, _, out, dq = attn_data(s["nb"], s["heads"], s["T"], s["d"], s["legacy"], s["causal"], dtype)
        res = [("out", out)]
        if dq is not None:
            res += [(nm, dq[:, idx]) for nm, idx in zip(("dq", "dk", "dv"), attn_cols(s["heads"], s["d"], s["legacy"]))]
        return res
    if row.op == "gn":
        d = gn_data(s["B"], s["HW"], s["C"], s["bwd"], dtype)
        return [("y", d[4])] + ([("dx", d[7])] if s["bwd"] else [])
    if row.op == "ln":
        d = ln_data(s["rows"], s["C"], dtype)
        return [("y", d[3]), ("dx", d[5])]
    if row.op == "act":
        d = act_data(s["kind"], s["n"], dtype)
        return [("dx", d[3])] if s["bwd"] else [("y", d[2])]
    return [("out", resample_data(row.fam, s["B"], s["H"], s["W"], s["C"], s["adj"], dtype)[1])]


def vacuous_ok(row, label):
    """the only records a reference of (nearly) zero peak may grade: dq and dk at T = 1 (one key: the softmax is constant)"""
    return row.op == "attn" and row.spec["T"] == 1 and label in ("dq", "dk")


# ---- GPU runners ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_ctx(ck):
    prec, env = CONTEXTS[ck]
    with _environ(env):
        return _ctx(prec)


def _tag(recs, row, verdict):
    return [dict(r, row=row.name, verdict=verdict) for r in recs]


def _sanity(name, got, ref):
    """precision 2 (one bf16 product) is a speed mode: bounded as test_gemm_bf16_single_product_is_bf16_accurate bounds it"""
    r = rec(name + " [bf16 sanity: error below 1e-2 of the peak]", got, ref)
    return dict(r, criterion="sanity", ok=bool(th.isfinite(got).all().item()) and r["err_rel"] < 1e-2)


def _case(ctx, row, inputs, outputs, refs, launch, route, labels=None, parts=None, sanity=False, tag=""):
    """strided_checks._case with the verdict of every record named: inputs [(Guarded, values)], outputs [Guarded], refs their float64
    references; parts {output index: [(label, column indices)]} grades column groups of an output separately"""
    out, first = [], None
    name = row.name + tag
    labels = labels or [f"out{i}" for i in range(len(outputs))]
    for k in range(2):
        for G, t in inputs:
            G.load(t, GAP[k])
        for G in outputs:
            G.poison(OUT_BITS[k])
        counts = _routes(ctx, launch)
        got = [G.view.clone() for G in outputs]
        if k == 0:
            first = got
            par = []
            for i, (G, ref) in enumerate(zip(outputs, refs)):
                for label, idx in ((parts or {}).get(i) or [(labels[i], None)]):
                    a, b = (got[i], ref) if idx is None else (got[i][:, idx.to(got[i].device)], ref[:, idx])
                    par.append(_sanity(f"{name} {label}", a, b) if sanity else rec(f"{name} {label}", a, b, allow_small=vacuous_ok(row, label)))
            out += _tag(par, row, "parity")
            desc, pred = ROUTES[route]
            ROUTE_LOG.append((name, desc, counts))
            out += _tag([_flag(f"{name}: route {desc} (launches per kind {counts})", pred(counts))], row, "route")
        out += _tag([_flag(f"{name} {labels[i]}: nothing written outside the view (sentinel {k})", G.intact(OUT_BITS[k]))
                     for i, G in enumerate(outputs)], row, "sentinel")
    out += _tag([_flag(f"{name}: a rerun into a fresh sentinel is bit-identical",
                       all(th.equal(a.view(th.int32), b.view(th.int32)) for a, b in zip(first, got)))], row, "rerun")
    return out, first


def _refuse(ctx, row, outputs, launch, tag=""):
    recs = _refusal(ctx, row.name + tag, outputs, launch, row.text)
    return _tag(recs[:1], row, "refused") + _tag(recs[1:], row, "untouched")


def _up4(n):
    return ceil_div(n, 4) * 4


def run_gemm(ctx, row, ck, keep):
    s = row.spec
    M, N, K, tile, sk = s["M"], s["N"], s["K"], s["tile"], s["sk"]
    a, b, bias, r, alpha, ref = gemm_data(M, N, K)
    lda, ldb, ldc, ldr = K + 8, K + 4, _up4(N) + 8, _up4(N) + 4
    A, B, Cg, R, bg = Guarded((M, K), lda, 4), Guarded((N, K), ldb, 0), Guarded((M, N), ldc, 4), Guarded((M, N), ldr, 0), Guarded((N,), None, 0, 4)
    lib = ctx.lib

    def launch():
        ctx.check(lib.cgd_op_gemm(ctx.h, A.ptr, lda, B.ptr, ldb, Cg.ptr, ldc, bg.ptr, R.ptr, ldr, M, N, K, alpha, tile, sk, _s()))

    ins = [(A, a), (B, b), (R, r), (bg, bias)]
    if row.verdict == "refuse":
        for G, t in ins:
            G.load(t, GAP[0])
        return _refuse(ctx, row, [Cg], launch)
    recs, first = _case(ctx, row, ins, [Cg], [ref], launch, row.route, labels=["C"], sanity=CONTEXTS[ck][0] == 2)
    if keep is not None:
        keep[row.name] = first[0]
    return recs


def run_conv(ctx, row, ck, keep):
    from cgd_amd import ops
    s = row.spec
    Bn, H, W, ups, dgrad, tile, sk = s["B"], s["H"], s["W"], s["ups"], s["dgrad"], s["tile"], s["sk"]
    x, w, b, r, _, ref = conv_data(Bn, H, W, s["Ci"], s["Co"], ups, dgrad)
    cin, cout = x.shape[-1], r.shape[-1]
    lib = ctx.lib
    ctx.check(lib.cgd_set_hconv(ctx.h, 1 + 16 * s["var"], 256))
    wf, wd = ops.pack_conv3x3(w)
    wt = (wd if dgrad else wf).to(DEV)
    # (the fragment packing exists for whole 32-channel blocks only: a caller with other channel counts has no packed copy to hand over)
    wfrag = ops.pack_conv3x3_frag(ctx, w.to(DEV), dgrad=bool(dgrad)) if cin % 32 == 0 and cout % 32 == 0 else None
    bd = None if b is None else b.to(DEV)
    ldx, ldy, ldr = cin + 8, cout + 8, cout + 4
    X, Y, R = Guarded(tuple(x.shape), ldx, 4), Guarded((Bn, H, W, cout), ldy, 4), Guarded((Bn, H, W, cout), ldr, 0)

    def launch():
        ctx.check(lib.cgd_op_conv3x3(ctx.h, X.ptr, ldx, wt.data_ptr(), None if wfrag is None else wfrag.data_ptr(), Y.ptr, ldy, None if bd is None else bd.data_ptr(),
                                     R.ptr, ldr, Bn, H, W, cin, cout, ups, tile, sk, _s()))

    try:
        if row.verdict == "refuse":
            X.load(x, GAP[0])
            R.load(r, GAP[0])
            return _refuse(ctx, row, [Y], launch)
        return _case(ctx, row, [(X, x), (R, r)], [Y], [ref], launch, row.route, labels=["y"])[0]
    finally:
        ctx.check(lib.cgd_set_hconv(ctx.h, 1, 256))


def run_wino(ctx, row, ck, keep):
    from cgd_amd import ops
    s = row.spec
    Bn, H, W, Ci, Co, ups = s["B"], s["H"], s["W"], s["Ci"], s["Co"], s["ups"]
    x, w, b, r, ab, ref = conv_data(Bn, H, W, Ci, Co, ups, 0, s["gn"])
    lib = ctx.lib
    ctx.check(lib.cgd_set_wino(ctx.h, s["mode"], 0))
    ww = ops.pack_conv3x3_wino(ctx, w.to(DEV))
    bd, abd = b.to(DEV), None if ab is None else ab.to(DEV)
    ldx, ldy, ldr = Ci + 8, Co + 8, Co + 4
    X, Y, R = Guarded(tuple(x.shape), ldx, 4), Guarded((Bn, H, W, Co), ldy, 4), Guarded((Bn, H, W, Co), ldr, 0)

    def launch():
        ctx.check(lib.cgd_op_conv3x3_wino(ctx.h, X.ptr, ldx, ww.data_ptr(), Y.ptr, ldy, bd.data_ptr(), R.ptr, ldr,
                                          None if abd is None else abd.data_ptr(), Bn, H, W, Ci, Co, ups, _s()))

    try:
        if row.verdict == "refuse":
            X.load(x, GAP[0])
            R.load(r, GAP[0])
            return _refuse(ctx, row, [Y], launch)
        return _case(ctx, row, [(X, x), (R, r)], [Y], [ref], launch, row.route, labels=["y"])[0]
    finally:
        ctx.check(lib.cgd_set_wino(ctx.h, 1, 0))


def run_attn(ctx, row, ck, keep):
    s = row.spec
    nb, heads, T, d, legacy, causal = s["nb"], s["heads"], s["T"], s["d"], s["legacy"], s["causal"]
    qkv, dout, ref, dref = attn_data(nb, heads, T, d, legacy, causal)
    Cc = heads * d
    lib = ctx.lib
    bufs = [th.zeros(lib.cgd_op_attn_buf_floats(nb, heads, T, d, i), device=DEV) for i in range(5)]
    arr = (C.c_void_p * 5)(*[t.data_ptr() for t in bufs])
    Q, O = Guarded((nb * T, 3 * Cc), None, 0, 4), Guarded((nb * T, Cc), None, 0, 4)
    route = "attn_generic" if attn_family(T, d, ck) == 0 else "attn_fused"

    def fwd():
        if causal:
            ctx.check(lib.cgd_op_attn_fwd_causal(ctx.h, Q.ptr, O.ptr, nb, heads, T, d, arr, _s()))
        else:
            ctx.check(lib.cgd_op_attn_fwd(ctx.h, Q.ptr, O.ptr, nb, heads, T, d, legacy, arr, _s()))

    out = _case(ctx, row, [(Q, qkv)], [O], [ref], fwd, route, labels=["out"], tag=" fwd")[0]
    if causal:
        return out
    DO, DQ = Guarded((nb * T, Cc), None, 0, 4), Guarded((nb * T, 3 * Cc), None, 0, 4)

    def bwd():
        ctx.check(lib.cgd_op_attn_bwd(ctx.h, Q.ptr, DO.ptr, DQ.ptr, nb, heads, T, d, legacy, arr, _s()))

    parts = {0: list(zip(("dq", "dk", "dv"), attn_cols(heads, d, legacy)))}
    return out + _case(ctx, row, [(Q, qkv), (DO, dout)], [DQ], [dref], bwd, route, labels=["dqkv"], parts=parts, tag=" bwd")[0]


def run_gn(ctx, row, ck, keep):
    s = row.spec
    B, HW, C_, bwd = s["B"], s["HW"], s["C"], s["bwd"]
    lib = ctx.lib
    big = HW > 4096  # the two 2048-chunk rows: dense operands, one guard row either side
    ldx, ldy, lddz, lddx, ldadd = (C_,) * 5 if big else (C_ + 8, C_ + 4, C_ + 12, C_ + 4, C_ + 8)
    col = 0 if big else 4
    X, Y = Guarded((B, HW, C_), ldx, col), Guarded((B, HW, C_), ldy, 0)
    scr = th.zeros(int(lib.cgd_op_gn_scratch_floats(B, HW, C_)), device=DEV)
    if row.verdict == "refuse":
        gd = th.ones(C_, device=DEV)
        DX = Guarded((B, HW, C_), lddx, 0)

        def fwd0():
            ctx.check(lib.cgd_op_gn_fwd(ctx.h, X.ptr, ldx, Y.ptr, ldy, B, HW, C_, gd.data_ptr(), gd.data_ptr(), None, 1, 1e-5, scr.data_ptr(), _s()))

        def bwd0():
            ctx.check(lib.cgd_op_gn_bwd(ctx.h, X.ptr, ldx, X.ptr, ldx, DX.ptr, lddx, None, 0, B, HW, C_, 1, scr.data_ptr(), _s()))

        return _refuse(ctx, row, [Y], fwd0, " fwd") + _refuse(ctx, row, [DX], bwd0, " bwd")
    x, gamma, beta, film, yref, dz, add, dxref = gn_data(B, HW, C_, bwd)
    gd, bd, fd = gamma.to(DEV), beta.to(DEV), film.to(DEV)

    def fwd():
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        ctx.check(lib.cgd_op_gn_fwd(ctx.h, X.ptr, ldx, Y.ptr, ldy, B, HW, C_, gd.data_ptr(), bd.data_ptr(), fd.data_ptr(), 1, 1e-5, scr.data_ptr(), _s()))

    out = _case(ctx, row, [(X, x)], [Y], [yref], fwd, "gn", labels=["y"], tag=" fwd")[0]
    if not bwd:
        return out
    DZ, DX, AD = Guarded((B, HW, C_), lddz, 4), Guarded((B, HW, C_), lddx, 0), Guarded((B, HW, C_), ldadd, 4)

    def bwd_():
        ctx.check(lib.cgd_op_gn_bwd(ctx.h, X.ptr, ldx, DZ.ptr, lddz, DX.ptr, lddx, AD.ptr, ldadd, B, HW, C_, 1, scr.data_ptr(), _s()))

    return out + _case(ctx, row, [(X, x), (DZ, dz), (AD, add)], [DX], [dxref], bwd_, "gn", labels=["dx"], tag=" bwd")[0]


def run_ln(ctx, row, ck, keep):
    s = row.spec
    rows, C_ = s["rows"], s["C"]
    x, gamma, beta, yref, dy, dxref = ln_data(rows, C_)
    lib = ctx.lib
    gd, bd = gamma.to(DEV), beta.to(DEV)
    stats = th.zeros(rows, 2, device=DEV)
    X, Y, DY, DX = (Guarded((rows, C_), None, 0, 4) for _ in range(4))

    def fwd():
        ctx.check(lib.cgd_op_ln_fwd(ctx.h, X.ptr, Y.ptr, rows, C_, gd.data_ptr(), bd.data_ptr(), 1e-5, stats.data_ptr(), _s()))

    def bwd():
        ctx.check(lib.cgd_op_ln_bwd(ctx.h, X.ptr, DY.ptr, DX.ptr, rows, C_, gd.data_ptr(), stats.data_ptr(), _s()))

    return _case(ctx, row, [(X, x)], [Y], [yref], fwd, "none", labels=["y"], tag=" fwd")[0] + \
        _case(ctx, row, [(X, x), (DY, dy)], [DX], [dxref], bwd, "none", labels=["dx"], tag=" bwd")[0]


def run_act(ctx, row, ck, keep):
    s = row.spec
    kind, n, bwd = s["kind"], s["n"], s["bwd"]
    v, dy, yref, dxref = act_data(kind, n)
    lib = ctx.lib
    X, DYg, Y = Guarded((n,), None, 0, 4), Guarded((n,), None, 0, 4), Guarded((n,), None, 0, 4)

    def launch():
        ctx.check(lib.cgd_op_act(ctx.h, X.ptr, DYg.ptr if bwd else None, Y.ptr, n, kind, _s()))

    return _case(ctx, row, [(X, v), (DYg, dy)], [Y], [dxref if bwd else yref], launch, "none", labels=["dx" if bwd else "y"])[0]


def run_resample(ctx, row, ck, keep):
    s = row.spec
    B, H, W, C_, adj = s["B"], s["H"], s["W"], s["C"], s["adj"]
    lib = ctx.lib
    fam = row.fam
    p = lambda v: max(v, 1)  # noqa: E731  (a refused row of zero height still needs an allocation to watch)
    if fam == "pool2x2":
        ishape, oshape = (B, 2 * p(H), 2 * p(W), C_), (B, p(H), p(W), C_)
    elif fam == "upsample2x":
        ishape, oshape = (B, p(H // 2), p(W // 2), C_), (B, p(H), p(W), C_)
    else:
        lo_, hi_ = (B, p(H), p(W), C_), (B, 2 * p(H), 2 * p(W), C_)
        ishape, oshape = (hi_, lo_) if adj else (lo_, hi_)
    X, Y = Guarded(ishape, None, 0, 4), Guarded(oshape, None, 0, 4)

    def launch():
        if fam == "pool2x2":
            ctx.check(lib.cgd_op_pool2x2(ctx.h, X.ptr, Y.ptr, B, H, W, C_, 0.25, _s()))
        elif fam == "upsample2x":
            ctx.check(lib.cgd_op_upsample2x(ctx.h, X.ptr, Y.ptr, B, H, W, C_, 1.0, _s()))
        else:
            ctx.check(lib.cgd_op_bilinear_up2x(ctx.h, X.ptr, C_, Y.ptr, C_, B, H, W, C_, adj, _s()))

    if row.verdict == "refuse":
        X.load(_r(ishape, 30), GAP[0])
        return _refuse(ctx, row, [Y], launch)
    x, ref = resample_data(fam, B, H, W, C_, adj)
    return _case(ctx, row, [(X, x)], [Y], [ref], launch, "none", labels=["out"])[0]


def reduce_launches(lib):
    """split-K reduce launches of the library since it was loaded (cgd_launch_counts)"""
    o = (C.c_uint64 * 2)()
    assert lib.cgd_launch_counts(o) == 0
    return int(o[1])


def run_sconv(ctx, row, ck, keep):
    s = row.spec
    dgrad, B, H, W, Ci, Co = s["dgrad"], s["B"], s["H"], s["W"], s["Ci"], s["Co"]
    lib = ctx.lib
    p1 = lambda v: max(v, 1)  # noqa: E731  (a refused row of zero height still needs an allocation to watch)
    big, small = (B, p1(H), p1(W), Ci), (B, p1(H // 2), p1(W // 2), Co)
    ishape, oshape = (small, big) if dgrad else (big, small)
    # the allocations keep their own strides; a refused row passes the stride it names (nothing is read or written before the refusal)
    a_in, a_out, a_add = ishape[-1] + 8, oshape[-1] + 8, Ci + 4
    ld_in, ld_out, ldadd = (a + d for a, d in zip((a_in, a_out, a_add), s["ld"]))
    X, Y = Guarded(ishape, a_in, 4), Guarded(oshape, a_out, 4)
    AD = Guarded(big, a_add, 0) if dgrad else None
    wshape = (Co, Ci, 3, 3)

    def call(wptr, bptr):
        if dgrad:
            return lib.cgd_op_conv3x3_s2_dgrad(ctx.h, X.ptr, ld_in, wptr, Y.ptr, ld_out, AD.ptr, ldadd, B, H, W, Ci, Co, _s())
        return lib.cgd_op_conv3x3_s2(ctx.h, X.ptr, ld_in, wptr, bptr, Y.ptr, ld_out, B, H, W, Ci, Co, _s())

    if row.verdict == "refuse":
        # the host predicate first: a row it accepts at these strides is not launched (its strides do not describe the allocations)
        if lib.cgd_op_conv3x3_s2_accepts(dgrad, ld_in, ld_out, ldadd if dgrad else 0, B, H, W, Ci, Co) != 0:
            return _tag([_flag(f"{row.name}: cgd_op_conv3x3_s2_accepts refuses the row", False)], row, "refused")
        wd = th.zeros(wshape, device=DEV)
        X.load(_r(ishape, 51), GAP[0])
        return _refuse(ctx, row, [Y], lambda: ctx.check(call(wd.data_ptr(), None)))
    xin, w, third, ref = sconv_data(dgrad, B, H, W, Ci, Co)
    wd = w.to(DEV)
    bd = None if dgrad else third.to(DEV)
    plan = (C.c_int * 4)()
    ncu = th.cuda.get_device_properties(0).multi_processor_count  # what cgd_ctx_create reads
    assert lib.cgd_op_plan_conv_s2(dgrad, B, H, W, Ci, Co, ncu, plan) == 0, row.name
    deltas = []

    def launch():
        before = reduce_launches(lib)
        ctx.check(call(wd.data_ptr(), None if bd is None else bd.data_ptr()))
        deltas.append(reduce_launches(lib) - before)

    ins = [(X, xin)] + ([(AD, third)] if dgrad else [])
    recs = _case(ctx, row, ins, [Y], [ref], launch, row.route, labels=["dx" if dgrad else "y"], sanity=CONTEXTS[ck][0] == 2)[0]
    want = int(plan[2] > 1)
    recs += _tag([_flag(f"{row.name}: plan {list(plan)} on {ncu} CUs, reduce launches per call {deltas} (one exactly when the plan splits)",
                        len(deltas) == 2 and all(d == want for d in deltas))], row, "plan")
    if dgrad:
        recs += _tag([_flag(f"{row.name}: the add operand and its gaps are unchanged",
                            th.equal(AD.view, third.to(DEV)) and bool((AD.buf[~AD.inside] == GAP[1]).all().item()))], row, "sentinel")
    return recs


RUNNERS = {"sconv": run_sconv, "gemm": run_gemm, "conv": run_conv, "wino": run_wino, "attn": run_attn, "gn": run_gn, "ln": run_ln, "act": run_act,
           "pool2x2": run_resample, "upsample2x": run_resample, "bilinear_up2x": run_resample}
VERDICTS_RUN = {"parity", "sentinel", "rerun", "route"}
VERDICTS_REFUSE = {"refused", "untouched"}
VERDICTS_EXTRA = {"sconv": {"plan"}}  # the plan entry's slice count against the reduce counter


def check_group(fam, ck, keep=None, ctx=None):
    """every row of one family in one context: the records, each tagged with its row and the verdict it carries"""
    ctx = ctx or make_ctx(ck)
    out = []
    for row in rows_of(fam, ck):
        out += RUNNERS[row.op](ctx, row, ck, keep)
    th.cuda.synchronize()
    return out


def verdicts_complete(recs, fam, ck):
    """every accepted row carries all four verdicts, every refused row both of its own: the rows that lack one"""
    have = {}
    for r in recs:
        have.setdefault(r["row"], set()).add(r["verdict"])
    need = lambda row: (VERDICTS_RUN | VERDICTS_EXTRA.get(row.fam, set())) if row.verdict == "run" else VERDICTS_REFUSE  # noqa: E731
    return [row.name for row in rows_of(fam, ck) if not have.get(row.name, set()) >= need(row)]


if __name__ == "__main__":  # one report: every record with its figures, the route table and the wall time per group, as JSON on stdout
    import json
    import sys
    import time
    recs, times = [], {}
    for fam_, ck_ in GROUPS:
        t0 = time.time()
        recs += [dict(r, group=f"{fam_}[{ck_}]") for r in check_group(fam_, ck_)]
        times[f"{fam_}[{ck_}]"] = round(time.time() - t0, 2)
    bad = [r for r in recs if not r["ok"]]
    json.dump({"failed": len(bad), "bad": bad, "seconds": times, "records": len(recs), "routes": len(ROUTE_LOG)}, sys.stdout, indent=1, default=str)
    print()
    sys.exit(1 if bad else 0)
