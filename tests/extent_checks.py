"""Op kernels on operands whose extent crosses 2 GiB (tests/test_gpu_extents.py), through the C ABI.

The MFMA kernels read their activations through raw buffer resources with 32-bit BYTE offsets (csrc/mfma_stage.h: offset 0x80000000 = "zeros"),
which is right only while every wanted offset stays below 2^31; the launchers guard that line (`M * lda < 2^29`, `H * W * lda * 4 < 2^31`,
Gram's `lda <= 2^20`) and route or refuse above it, and every epilogue claims 64-bit row arithmetic.  Each case here puts exactly ONE operand
across the line (`Far`), the others are compact (`strided_checks.Guarded`), and is named `below` (largest stride, a multiple of 4, that keeps the
guarded product under its limit) or `at` (smallest that reaches it); operands without a guard are simply `far` (their last row starts beyond
2^31 bytes).  Criterion, sentinels, two bit-identical runs and the route assertions are those of strided_checks (`_case`, `_refusal`).

`Far`: a logical view (rows, width) with row stride `ld` at column `col` of its rows, inside ONE torch.empty allocation of which only BANDS
are ever touched: `guard` floats left and right of the view in every row, and the same width in one whole row before and after the view.
Input bands hold the large finite sentinels (GAP), output bands the NaN sentinels (OUT_BITS); after a call the view must match float64 (an
unwritten element stays NaN) and every band must still hold the sentinel's bits.

Alias bands make a wrong kernel FAIL A COMPARISON instead of faulting.  Let e = r * ld be the float offset of row r (0 .. rows, i.e. the row
after the view included) from the operand pointer and o = 4 e its byte offset.  A kernel that narrows one of them lands at
    s32(o), u32(o) bytes   (a signed / unsigned 32-bit byte offset:  o - 2^32 for 2^31 <= o < 2^32,  o mod 2^32 beyond)
    s32(e), u32(e) floats  (a 32-bit element index: differs from e only beyond 2^31 floats, tier B)
from the pointer, with s32(v) = ((v + 2^31) mod 2^32) - 2^31 and u32(v) = v mod 2^32.  Every such address that differs from the true one gets
a band of its own, and the allocation carries a lead-in in front of the view that is long enough for the most negative of them:
    lead-in floats = max(0, -(min alias float offset - guard) - ld - col)   (rounded up to 4 floats; the view starts at lead-in + ld + col)
In tier A (extent just over 2^31 BYTES) the most negative alias is s32(o) >= -2^31 bytes: a lead-in of at most 2 GiB, about 4.3 GiB per
allocation.  In tier B (extent just over 2^31 ELEMENTS, 8 GiB) it is s32(e) >= -2^31 floats: at most 8 GiB of lead-in, about 17 GiB.
One far allocation is alive at a time (`_arena`: dropped, with torch.cuda.empty_cache(), before a larger one is made and at the end of every
check), and it is made only when torch.cuda.mem_get_info() shows at least twice the need free: tier A fails otherwise, tier B skips.  Two
shapes are larger than tier A's 4.5 GiB by their definition: the 4-row GEMV (three rows must span 2^31 bytes, and the rows before and after the
view are as long: 5.3 GiB) and the Gram case (C 64, B 2, N 512, lda 2^20: 4 GiB of operand, 6 GiB with its lead-in).

`at` is where a guard sits, not where its kernel breaks: the guards count M * lda (one more row than is addressed), so at the `at` stride every
wanted byte still lies below 2^31.  `beyond` (far A, far x) is the smallest stride that puts the START of the last row at 2^31 bytes: there a
32-bit byte offset is wrong for certain, and that is the case a widened guard fails (tests/test_extents_host.py has the arithmetic).

Out of scope: LayerNorm, activations, attention, pooling and resampling take no stride at the op ABI; their dense sizes at this extent would
need real data of that size and a reference nobody can compute in seconds."""
import math

import pytest
import torch as th
import torch.nn.functional as F

from tests.parity_checks import DEV, _ctx, _flag, g, rec, unit_seed  # noqa: F401
from tests.strided_checks import GAP, OUT_BITS, Guarded, _case, _conv_ref, _gn_ref, _r, _refusal, _s, any_halo, off_halo, on  # noqa: F401

P31, P32 = 1 << 31, 1 << 32
_ARENA = None
_LIVE = []  # the Far objects that hold views of the arena


def s32(v):
    return ((v + P31) % P32) - P31


def u32(v):
    return v % P32


def below_at(limit, rows):
    """(largest multiple of 4 with rows * ld < limit, smallest multiple of 4 with rows * ld >= limit)"""
    b = ((limit - 1) // rows) // 4 * 4
    a = b + 4
    assert rows * b < limit <= rows * a
    return b, a


def far_ld(rows, elements=False):
    """smallest multiple of 4 that puts the start of the LAST row at or beyond 2^31 bytes (elements=True: 2^31 floats) from the pointer"""
    lim = P31 if elements else P31 // 4
    return -(-lim // (rows - 1) // 4) * 4 + 4


def alias_offsets(e):
    """float offsets from the operand pointer at which a narrowed offset of the row at float offset e >= 0 lands (without e itself)"""
    o = 4 * e
    return sorted({s32(o) // 4, u32(o) // 4, s32(e), u32(e)} - {e})


def release():
    """drops the far allocation: the `Far` objects that were carved from it lose their tensors, so nothing keeps it alive"""
    global _ARENA
    for f in _LIVE:
        f.buf = f.ibuf = f.view = f.view2 = None
    _LIVE.clear()
    _ARENA = None
    th.cuda.empty_cache()


def _arena(n, tier_b=False):
    """the one far allocation: at least n floats of torch.empty; made anew (after dropping the old one) only to grow"""
    global _ARENA
    if _ARENA is None or _ARENA.numel() < n:
        release()
        free, _ = th.cuda.mem_get_info()
        if free < 2 * 4 * n:
            msg = f"a far operand of {4 * n / 2 ** 30:.1f} GiB needs twice that free, {free / 2 ** 30:.1f} GiB are"
            if tier_b:
                pytest.skip(msg)
            raise RuntimeError(msg)
        _ARENA = th.empty(n, device=DEV, dtype=th.float32)
    return _ARENA[:n]


def far_layout(shape, ld, col=0, guard=8):
    """host arithmetic of `Far` (no device): lead-in, float index of the view's first element, floats of the allocation, and the band starts
    as float offsets from the operand pointer"""
    shape = tuple(shape)
    width, rows = shape[-1], math.prod(shape[:-1])
    assert ld % 4 == 0 and col % 4 == 0 and 0 <= col and col + width <= ld and guard >= 1
    band = width + 2 * guard
    real = {r * ld - guard for r in range(-1, rows + 1)}
    end = rows * ld + width + guard  # one past the last float of the band in the row after the view
    alias = set()
    for r in range(0, rows + 1):
        for a in alias_offsets(r * ld):
            if a - guard + band <= end:  # (always: an alias lies below the true offset)
                alias.add(a - guard)
    starts = real | alias
    lead = max(0, -min(starts) - ld - col)
    lead = -(-lead // 4) * 4
    base = lead + ld + col
    n = lead + (rows + 2) * ld + guard
    assert base + min(starts) >= 0 and base + end <= n
    return dict(rows=rows, width=width, band=band, lead=lead, base=base, n=n, starts=sorted(starts), alias=sorted(alias - real))


class Far:
    """see the module docstring; duck-types strided_checks.Guarded (view, ptr, ld, load, poison, intact)"""

    def __init__(self, shape, ld, col=0, guard=8, tier_b=False):
        shape = tuple(shape)
        lay = far_layout(shape, ld, col, guard)
        rows, width, base, n = lay["rows"], lay["width"], lay["base"], lay["n"]
        self.bytes = 4 * n
        self.buf = _arena(n, tier_b)
        _LIVE.append(self)
        self.ibuf = self.buf.view(th.int32)
        strides, s = [], ld
        for d in reversed(shape[:-1]):
            strides.insert(0, s)
            s *= d
        self.view = self.buf.as_strided(shape, tuple(strides) + (1,), base)
        self.view2 = self.buf.as_strided((rows, width), (ld, 1), base)
        rel = th.tensor(lay["starts"], dtype=th.int64)[:, None] + th.arange(lay["band"], dtype=th.int64)[None, :]  # float offsets from the pointer
        row, c = th.div(rel, ld, rounding_mode="floor"), rel % ld
        self.inside = ((row >= 0) & (row < rows) & (c < width)).reshape(-1).to(DEV)
        self.idx = (rel + base).reshape(-1).to(DEV)
        self.ld, self.rows, self.lead_bytes = ld, rows, 4 * lay["lead"]

    @property
    def ptr(self):
        return self.view.data_ptr()

    def poison(self, bits):
        self.ibuf[self.idx] = bits

    def load(self, t, gap):
        self.buf[self.idx] = gap
        self.view2.copy_(t.reshape(self.view2.shape))

    def intact(self, bits, whole=False):
        ok = self.ibuf[self.idx] == bits
        if not whole:
            ok = ok | self.inside
        return bool(ok.all().item())


def _op(shape, ld, col, far, tier_b=False):
    return Far(shape, ld, col, tier_b=tier_b) if far else Guarded(shape, ld, col)


NO_HALO = ("no halo conv kernel", lambda c: all(c[j] == 0 for j in (1, 3, 4)))
GEMM_ROUTE = on(0)  # the profile has one kind for every GEMM kernel (igemm, hgemm, hgemm2, kgemm, GEMV)


# ---------------------------------------------------------------------------------------------------------
def _gemm_run(ctx, p, tag, M, N, K, tile, sk, far, ld, col, refuse=None, tier_b=False):
    """cgd_op_gemm with bias and residual; `far` in "ACR" names the operand that takes (ld, col), the others are compact"""
    lib = ctx.lib
    lda, ldc, ldr = K + 32, N + 32, N + 12
    cols = {"A": 16, "C": 16, "R": 8}
    if far == "A":
        lda = ld
    elif far == "C":
        ldc = ld
    else:
        ldr = ld
    cols[far] = col
    A = _op((M, K), lda, cols["A"], far == "A", tier_b)
    Cg = _op((M, N), ldc, cols["C"], far == "C", tier_b)
    R = _op((M, N), ldr, cols["R"], far == "R", tier_b)
    B, bias = Guarded((N, K), K + 8, 4), Guarded((N,), None, 0)
    a, b, r, bb = _r((M, K), 1), _r((N, K), 2), _r((M, N), 4, 0.3), _r((N,), 3, 0.3)
    alpha = 1.0 / math.sqrt(K)
    name = f"gemm[p{p}] far {far} {tag} {M}x{N}x{K} tile{tile} sk{sk} ld{ld}+{col}"

    def launch():
        ctx.check(lib.cgd_op_gemm(ctx.h, A.ptr, lda, B.ptr, K + 8, Cg.ptr, ldc, bias.ptr, R.ptr, ldr, M, N, K, alpha, tile, sk, _s()))

    if refuse:
        for G, t in ((A, a), (B, b), (R, r), (bias, bb)):
            G.load(t, GAP[0])
        return _refusal(ctx, name, [Cg], launch, refuse)
    ref = alpha * (a.double() @ b.double().T) + bb.double() + r.double()
    return _case(ctx, name, [(A, a), (B, b), (R, r), (bias, bb)], [Cg], [ref], launch, GEMM_ROUTE)


def check_gemm_far_a(precision=1):
    """far A: igemm tile codes and split-K; the weight GEMM (513: hgemm2 below the line, hgemm_kernel at it, split-K 1 / 2 / auto), kgemm (518:
    runs below, refused at), the GEMV (517: no guard, both sides must be right).  The columns sit at the right edge of the stride (col = lda - K)
    in the first case of every kernel."""
    ctx = _ctx(precision)
    out = []
    M, N, K = 130, 96, 256
    lim = 1 << 29
    try:
        # `at` is where the guard sits (M * lda); the last ROW starts beyond 2^31 bytes one row's worth of stride later: `beyond`
        for side, lda in zip(("below", "at", "beyond"), below_at(lim, M) + (far_ld(M),)):
            for i, (tile, sk) in enumerate(((0, 1), (64, 1), (128, 1), (256, 1), (64, 3))):
                out += _gemm_run(ctx, precision, side, M, N, K, tile, sk, "A", lda, lda - K if i < 2 else 16)
            if precision != 0:
                for i, sk in enumerate((1, 2, 0)):
                    out += _gemm_run(ctx, precision, side, M, N, K, 513, sk, "A", lda, lda - K if i == 0 else 16)
        if precision != 0:
            lb, la = below_at(lim, 70)
            out += _gemm_run(ctx, precision, "below", 70, N, K, 518, 1, "A", lb, lb - K)
            out += _gemm_run(ctx, precision, "below", 70, N, K, 518, 1, "A", lb, 16)
            for side, ld in (("at", la), ("beyond", far_ld(70))):
                out += _gemm_run(ctx, precision, side, 70, N, K, 518, 1, "A", ld, ld - K, refuse="few-row weight GEMM kernel does not support this problem")
            # few rows: kgemm does not clamp the rows beyond M of its 64-row tile, so 64 * lda < 2^30 is its line (row 63's byte offset stays
            # below 2^32); the M * lda line alone would accept 8 rows at a stride eight times that
            lb8, la8 = below_at(1 << 30, 64)
            out += _gemm_run(ctx, precision, "below (64-row tile)", 8, N, K, 518, 1, "A", lb8, lb8 - K)
            for ld in (la8, below_at(lim, 8)[0]):
                out += _gemm_run(ctx, precision, "at (64-row tile)", 8, N, K, 518, 1, "A", ld, ld - K,
                                 refuse="few-row weight GEMM kernel does not support this problem")
        assert below_at(lim, 4) == ((1 << 27) - 4, 1 << 27)
        for side, lda in zip(("below", "at", "beyond"), below_at(lim, 4) + (far_ld(4),)):
            out += _gemm_run(ctx, precision, side, 4, N, K, 517, 1, "A", lda, lda - K)
        th.cuda.synchronize()
    finally:
        release()
    return out


def check_gemm_far_cr(precision=1, tier_b=False):
    """far C, then far R, with A compact: the 64-bit row arithmetic of every epilogue (igemm, the split-K reduce, hgemm2, kgemm, the GEMV).
    tier_b: the last row starts beyond 2^31 FLOATS (tile codes 64 and 513 only)."""
    ctx = _ctx(precision)
    out = []
    N, K = 96, 256
    cases = [(130, 64, 1), (130, 513, 1)] if tier_b else [(130, 0, 1), (130, 64, 3), (130, 513, 1), (70, 518, 1), (4, 517, 1)]
    try:
        for far in "CR":
            for M, tile, sk in cases:
                if precision == 0 and tile in (513, 518):
                    continue
                ld = far_ld(M, elements=tier_b)
                out += _gemm_run(ctx, precision, "far B" if tier_b else "far", M, N, K, tile, sk, far, ld, ld - N if tile in (64, 513) else 16, tier_b=tier_b)
        th.cuda.synchronize()
    finally:
        release()
    return out


# ---------------------------------------------------------------------------------------------------------
def check_gemm_gn_bwd_far():
    """cgd_op_gemm_gn_bwd at (B 2, HW 256, C 96, K 64, add): lda / lddx / ldx / lddz / ldadd far in turn.  lda has the weight GEMM's line
    (M * lda < 2^29: `below` runs, `at` is refused by the device call and by cgd_op_gemm_gn_bwd_accepts alike, nothing written); the epilogue
    indexes dx / x / dz / add with 64-bit rows (hgemm.hip: `long row[]`), so a far stride there is accepted and must be right."""
    from tests.test_gpu_gemm_gn_bwd import case
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    B, HW, Cc, K = 2, 256, 96, 64
    M = B * HW
    c = case(B, HW, Cc, K, True)
    coef, bcoef, w = c["coef"].to(DEV), c["bcoef"].to(DEV), c["w"].to(DEV)
    lb, la = below_at(1 << 29, M)
    fl = far_ld(M)
    cases = [("lda", "below", lb, lb - K), ("lda", "at", la, la - K)]
    for nm in ("lddx", "ldx", "lddz", "ldadd"):
        cases += [(nm, "far", fl, fl - Cc), (nm, "far", fl, 16)]
    refusal = "cgd_op_gemm_gn_bwd: needs a bf16x3 context"
    try:
        for nm, side, ld, col in cases:
            lds = {"lda": K + 12, "lddx": Cc + 24, "ldx": Cc + 40, "lddz": Cc + 16, "ldadd": Cc + 20}
            cols = {"lda": 8, "lddx": 8, "ldx": 32, "lddz": 4, "ldadd": 16}
            lds[nm], cols[nm] = ld, col
            A = _op((B, HW, K), lds["lda"], cols["lda"], nm == "lda")
            DX = _op((B, HW, Cc), lds["lddx"], cols["lddx"], nm == "lddx")
            X = _op((B, HW, Cc), lds["ldx"], cols["ldx"], nm == "ldx")
            DZ = _op((B, HW, Cc), lds["lddz"], cols["lddz"], nm == "lddz")
            AD = _op((B, HW, Cc), lds["ldadd"], cols["ldadd"], nm == "ldadd")
            name = f"gemm_gn_bwd {nm} {side} {ld}+{col}"
            acc = int(lib.cgd_op_gemm_gn_bwd_accepts(1, lds["lda"], K, lds["lddx"], lds["ldx"], lds["lddz"], lds["ldadd"], 0, B, HW, Cc, K))

            def launch():
                ctx.check(lib.cgd_op_gemm_gn_bwd(ctx.h, A.ptr, lds["lda"], w.data_ptr(), K, DX.ptr, lds["lddx"], X.ptr, lds["ldx"], DZ.ptr, lds["lddz"],
                                                 AD.ptr, lds["ldadd"], coef.data_ptr(), bcoef.data_ptr(), B, HW, Cc, K, _s()))

            ins = [(A, c["dout"]), (X, c["x"]), (DZ, c["dz"]), (AD, c["skip"])]
            want = side != "at"
            out.append(_flag(f"{name}: cgd_op_gemm_gn_bwd_accepts says {acc}, the device call must {'run' if want else 'refuse'}", acc == int(want)))
            if want:
                out += _case(ctx, name, ins, [DX], [c["ref"]], launch, GEMM_ROUTE)
            else:
                for G, t in ins:
                    G.load(t, GAP[0])
                out += _refusal(ctx, name, [DX], launch, refusal)
        th.cuda.synchronize()
    finally:
        release()
    return out


# ---------------------------------------------------------------------------------------------------------
CONV_REFUSE = {512: "halo conv kernel does not support this problem", 516: "weight-streaming conv kernel does not support this problem"}


def _conv_run(ctx, p, tag, tile, far, ld, col, var=0, ups=0, dgrad=False, gn=False, Bn=1, route=None, refuse=None):
    """cgd_op_conv3x3_ex (cgd_op_conv3x3 without gn_ab) at B x 16 x 16, 64 -> 64; `far` in "xyR" names the operand that takes (ld, col)"""
    from cgd_amd import ops
    lib = ctx.lib
    H = W = 16
    Ci = Co = 64
    if tile in (0, 512, 516):
        ctx.check(lib.cgd_set_hconv(ctx.h, 1 + 16 * var, 256))
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    w = _r((Co, Ci, 3, 3), 6) / math.sqrt(9 * Ci)
    wf, wd = ops.pack_conv3x3(w)
    wt = (wd if dgrad else wf).to(DEV)
    wfrag = ops.pack_conv3x3_frag(ctx, w.to(DEV), dgrad=dgrad)
    x = _r((Bn, Hs, Ws, Ci), 5)
    b = None if dgrad else _r((Co,), 7, 0.3)
    r = _r((Bn, H, W, Co), 17, 0.3)
    ab = th.stack([0.5 + th.rand(Bn, Ci, generator=g(18)), 0.5 * th.randn(Bn, Ci, generator=g(19))], dim=2).contiguous() if gn else None
    lds, cols = {"x": Ci + 32, "y": Co + 32, "R": Co + 48}, {"x": 32, "y": 16, "R": 4}
    lds[far], cols[far] = ld, col
    X = _op((Bn, Hs, Ws, Ci), lds["x"], cols["x"], far == "x")
    Y = _op((Bn, H, W, Co), lds["y"], cols["y"], far == "y")
    R = _op((Bn, H, W, Co), lds["R"], cols["R"], far == "R")
    bd, abd = None if b is None else b.to(DEV), None if ab is None else ab.to(DEV)
    name = f"conv3x3[p{p}] far {far} {tag} tile{tile} var{var} B{Bn} ups{ups} gn{int(gn)}{' dgrad' if dgrad else ''} ld{ld}+{col}"

    def launch():
        if gn:
            ctx.check(lib.cgd_op_conv3x3_ex(ctx.h, X.ptr, lds["x"], wt.data_ptr(), wfrag.data_ptr(), Y.ptr, lds["y"], None if bd is None else bd.data_ptr(),
                                            R.ptr, lds["R"], abd.data_ptr(), Bn, H, W, Ci, Co, ups, tile, 1, 0, 0, None, 0, None, _s()))
        else:
            ctx.check(lib.cgd_op_conv3x3(ctx.h, X.ptr, lds["x"], wt.data_ptr(), wfrag.data_ptr(), Y.ptr, lds["y"], None if bd is None else bd.data_ptr(),
                                         R.ptr, lds["R"], Bn, H, W, Ci, Co, ups, tile, 1, _s()))

    if refuse:
        X.load(x, GAP[0])
        R.load(r, GAP[0])
        res = _refusal(ctx, name, [Y], launch, refuse)
    else:
        wref = w.flip(2, 3).transpose(0, 1) if dgrad else w
        res = _case(ctx, name, [(X, x), (R, r)], [Y], [_conv_ref(x, wref, b, ups, r, ab)], launch, route)
    ctx.check(lib.cgd_set_hconv(ctx.h, 1, 256))
    return res


def check_conv_far(precision=1):
    """cgd_op_conv3x3[_ex], 16 x 16, 64 -> 64.  Far x (line H * W * ldx * 4 < 2^31: ldx = 2^21 - 4 / 2^21): below it the forced halo routes run
    (hconv2 variants 0 and 8, kconv, with gn_ab, upsampled input, dgrad packing), at it they refuse and the automatic selection computes the conv
    on the implicit GEMM; B = 2 with each image below the line and the second image's rows beyond 2^31 bytes stays on the halo kernels (the image
    base is 64-bit).  Then far y and far R with x compact.  Exact-fp32 contexts have no halo kernel for this op: implicit GEMM throughout."""
    ctx = _ctx(precision)
    out = []
    p = precision
    lb, la = below_at(P31 // 4, 256)
    assert (lb, la) == ((1 << 21) - 4, 1 << 21)
    fl = far_ld(256)
    try:
        for tile in (64, 128):
            out += _conv_run(ctx, p, "below", tile, "x", lb, lb - 64, route=off_halo())
            out += _conv_run(ctx, p, "at", tile, "x", la, la - 64, route=off_halo())
        out += _conv_run(ctx, p, "at auto", 0, "x", la, la - 64, route=off_halo())
        out += _conv_run(ctx, p, "at auto", 0, "x", la, 32, route=off_halo())
        out += _conv_run(ctx, p, "beyond auto", 0, "x", fl, fl - 64, route=off_halo())  # the last pixel's row starts beyond 2^31 bytes
        if p != 0:
            out += _conv_run(ctx, p, "below auto", 0, "x", lb, lb - 64, route=any_halo())
            for var in (0, 8):
                out += _conv_run(ctx, p, "below", 512, "x", lb, lb - 64, var=var, route=on(1))
                out += _conv_run(ctx, p, "below", 512, "x", lb, 32, var=var, gn=True, route=on(1))
            out += _conv_run(ctx, p, "below", 512, "x", lb, lb - 64, ups=1, route=on(1))  # (the guard counts the OUTPUT's 256 pixels)
            out += _conv_run(ctx, p, "below", 512, "x", lb, lb - 64, dgrad=True, route=on(1))
            out += _conv_run(ctx, p, "below", 516, "x", lb, lb - 64, route=on(4))
            out += _conv_run(ctx, p, "below", 516, "x", lb, 32, gn=True, route=on(4))
            out += _conv_run(ctx, p, "below", 516, "x", lb, lb - 64, dgrad=True, route=on(4))
            for tile in (512, 516):
                out += _conv_run(ctx, p, "at", tile, "x", la, la - 64, refuse=CONV_REFUSE[tile])
                out += _conv_run(ctx, p, "beyond", tile, "x", fl, fl - 64, refuse=CONV_REFUSE[tile])
            out += _conv_run(ctx, p, "at", 512, "x", la, la - 64, var=8, refuse=CONV_REFUSE[512])
            # two images of 2^30 + 2^27 bytes: every row of the second half of image 1 starts beyond 2^31 bytes
            l2 = (1 << 20) + (1 << 17)
            for tile, kind in ((512, 1), (516, 4)):
                out += _conv_run(ctx, p, "B2 images below, tensor above", tile, "x", l2, l2 - 64, Bn=2, route=on(kind))
        for far in "yR":
            out += _conv_run(ctx, p, "far", 64, far, fl, fl - 64, route=off_halo())
            out += _conv_run(ctx, p, "far", 0, far, fl, 16, route=any_halo() if p != 0 else off_halo())
            if p != 0:
                out += _conv_run(ctx, p, "far", 512, far, fl, fl - 64, route=on(1))
                out += _conv_run(ctx, p, "far", 512, far, fl, 16, var=8, route=on(1))
                out += _conv_run(ctx, p, "far", 516, far, fl, fl - 64, route=on(4))
        th.cuda.synchronize()
    finally:
        release()
    return out


# ---------------------------------------------------------------------------------------------------------
SCONV_REFUSE = "an operand of 2^31 bytes or more"


def sconv_below_at(rows, width):
    """(largest accepted, smallest refused) row stride of a stride-2 conv operand of `rows` rows of `width` floats: cgd_sconv_refusal counts
    the operand's extent ((rows - 1) * ld + width) * 4 < 2^31 bytes, not rows * ld"""
    b = ((P31 // 4 - 1 - width) // (rows - 1)) // 4 * 4
    assert ((rows - 1) * b + width) * 4 < P31 <= ((rows - 1) * (b + 4) + width) * 4
    return b, b + 4


# (far operand, B, Cin, Cout): 8 x 8 input maps.  The forward splits K (4 slices at 32 channels per tap, 9 at 64: the reduce launch writes y), the
# backward at 32 / 64 channels per tap does not (the kernel's own epilogue writes dx and reads add) and at 128 takes two slices (the reduce does)
SCONV_FAR = (("x", 1, 32, 64), ("x", 2, 64, 32), ("y", 2, 32, 64), ("y", 1, 64, 32), ("dy", 2, 32, 32), ("dy", 1, 64, 64), ("dx", 1, 32, 64),
             ("dx", 2, 64, 128), ("add", 2, 32, 64), ("add", 1, 64, 128))


def sconv_far_shape(far, Bn, Ci, Co, H=8, W=8):
    """(shape of the far operand, backward?)"""
    return {"x": ((Bn, H, W, Ci), 0), "y": ((Bn, H // 2, W // 2, Co), 0), "dy": ((Bn, H // 2, W // 2, Co), 1), "dx": ((Bn, H, W, Ci), 1),
            "add": ((Bn, H, W, Ci), 1)}[far]


def _sconv_run(ctx, p, tag, far, Bn, Ci, Co, ld, col, refuse=None):
    """cgd_op_conv3x3_s2 (far x / y) or cgd_op_conv3x3_s2_dgrad with add (far dy / dx / add) at Bn x 8 x 8"""
    lib = ctx.lib
    H = W = 8
    shape, dgrad = sconv_far_shape(far, Bn, Ci, Co)
    w = _r((Co, Ci, 3, 3), 6) / math.sqrt(9 * Ci)
    wd = w.to(DEV)
    name = f"conv3x3_s2[p{p}] far {far} {tag} B{Bn} {Ci}->{Co} ld{ld}+{col}"
    big, small = (Bn, H, W, Ci), (Bn, H // 2, W // 2, Co)
    if not dgrad:
        x, b = _r(big, 5), _r((Co,), 7, 0.3)
        bd = b.to(DEV)
        X = _op(big, ld if far == "x" else Ci + 32, col if far == "x" else 32, far == "x")
        Y = _op(small, ld if far == "y" else Co + 32, col if far == "y" else 16, far == "y")

        def launch():
            ctx.check(lib.cgd_op_conv3x3_s2(ctx.h, X.ptr, X.ld, wd.data_ptr(), bd.data_ptr(), Y.ptr, Y.ld, Bn, H, W, Ci, Co, _s()))

        if refuse:
            X.load(x, GAP[0])
            return _refusal(ctx, name, [Y], launch, refuse)
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=2, padding=1).permute(0, 2, 3, 1)
        return _case(ctx, name, [(X, x)], [Y], [ref], launch, GEMM_ROUTE)
    dy, add = _r(small, 8), _r(big, 9, 0.3)
    xr = th.zeros(Bn, Ci, H, W, dtype=th.float64, requires_grad=True)
    (gx,) = th.autograd.grad(F.conv2d(xr, w.double(), None, stride=2, padding=1), xr, dy.double().permute(0, 3, 1, 2))
    sd = unit_seed(gx)
    dy = dy * sd
    ref = gx.permute(0, 2, 3, 1) * sd + add.double()
    DY = _op(small, ld if far == "dy" else Co + 32, col if far == "dy" else 32, far == "dy")
    DX = _op(big, ld if far == "dx" else Ci + 32, col if far == "dx" else 16, far == "dx")
    AD = _op(big, ld if far == "add" else Ci + 48, col if far == "add" else 4, far == "add")

    def launch():
        ctx.check(lib.cgd_op_conv3x3_s2_dgrad(ctx.h, DY.ptr, DY.ld, wd.data_ptr(), DX.ptr, DX.ld, AD.ptr, AD.ld, Bn, H, W, Ci, Co, _s()))

    if refuse:
        DY.load(dy, GAP[0])
        AD.load(add, GAP[0])
        return _refusal(ctx, name, [DX], launch, refuse)
    return _case(ctx, name, [(DY, dy), (AD, add)], [DX], [ref], launch, GEMM_ROUTE)


def check_sconv_far(precision=1):
    """cgd_op_conv3x3_s2 / _dgrad at B x 8 x 8 with ONE far operand (SCONV_FAR): x, y of the forward, dy, dx, add of the backward, each at the
    last row stride cgd_sconv_refusal accepts (the operand ends within one stride step below 2^31 bytes; the columns once at the right edge of the
    stride, once at 16) and at the next one up, which must be refused with nothing written.  Both the call and cgd_op_conv3x3_s2_accepts are
    asked.  sconv_kernel forms 32-bit byte offsets for x / dy and the weights; y, dx and add are indexed with 64-bit rows."""
    ctx = _ctx(precision)
    lib, out = ctx.lib, []
    try:
        for far, Bn, Ci, Co in SCONV_FAR:
            shape, dgrad = sconv_far_shape(far, Bn, Ci, Co)
            lb, la = sconv_below_at(math.prod(shape[:-1]), shape[-1])
            for side, ld, cols in (("below", lb, (lb - shape[-1], 16)), ("at", la, (la - shape[-1],))):
                cin, cout = (Co, Ci) if dgrad else (Ci, Co)
                lds = {"in": cin + 32, "out": cout + 32, "add": Ci + 48 if dgrad else 0}
                lds[{"x": "in", "dy": "in", "y": "out", "dx": "out", "add": "add"}[far]] = ld
                acc = int(lib.cgd_op_conv3x3_s2_accepts(dgrad, lds["in"], lds["out"], lds["add"], Bn, 8, 8, Ci, Co))
                out.append(_flag(f"conv3x3_s2 far {far} {side} ld{ld}: cgd_op_conv3x3_s2_accepts says {acc}", acc == int(side == "below")))
                if acc != int(side == "below"):
                    continue  # (a stride the predicate would let through is not launched)
                for col in cols:
                    out += _sconv_run(ctx, precision, side, far, Bn, Ci, Co, ld, col, refuse=None if side == "below" else SCONV_REFUSE)
        th.cuda.synchronize()
    finally:
        release()
    return out


# ---------------------------------------------------------------------------------------------------------
WINO_REFUSE = "Winograd conv kernel does not support this problem"


def check_wino_far(precision=1):
    """cgd_op_conv3x3_wino at 16 x 16, 64 -> 64 (256 outputs in tile mode 5), every tile mode of the precision: far x below the line (with and
    without gn_ab, upsampled input, dgrad packing) and refused at it; far y and far R."""
    from cgd_amd import ops
    ctx = _ctx(precision)
    lib, out = ctx.lib, []
    Bn, H, W, Ci = 1, 16, 16, 64
    lb, la = below_at(P31 // 4, H * W)
    fl = far_ld(H * W)

    def run(mode, tag, far, ld, col, gn=False, ups=0, dgrad=False, refuse=None):
        Co = 256 if mode == 5 else 64
        Hs, Ws = (H // 2, W // 2) if ups else (H, W)
        cin, cout = (Co, Ci) if dgrad else (Ci, Co)
        x = _r((Bn, Hs, Ws, cin), 5)
        w = _r((Co, Ci, 3, 3), 6) / math.sqrt(9 * cin)
        b = None if dgrad else _r((cout,), 7, 0.3)
        r = _r((Bn, H, W, cout), 17, 0.3)
        ab = th.stack([0.5 + th.rand(Bn, cin, generator=g(18)), 0.5 * th.randn(Bn, cin, generator=g(19))], dim=2).contiguous() if gn else None
        ww = ops.pack_conv3x3_wino(ctx, w.to(DEV), dgrad=dgrad)
        bd, abd = None if b is None else b.to(DEV), None if ab is None else ab.to(DEV)
        lds, cols = {"x": cin + 32, "y": cout + 64, "R": cout + 4}, {"x": 32, "y": 32, "R": 4}
        lds[far], cols[far] = ld, col
        X = _op((Bn, Hs, Ws, cin), lds["x"], cols["x"], far == "x")
        Y = _op((Bn, H, W, cout), lds["y"], cols["y"], far == "y")
        R = _op((Bn, H, W, cout), lds["R"], cols["R"], far == "R")
        name = f"wconv[p{precision}] m{mode} far {far} {tag} {cin}->{cout} ups{ups} gn{int(gn)}{' dgrad' if dgrad else ''} ld{ld}+{col}"

        def launch():
            ctx.check(lib.cgd_op_conv3x3_wino(ctx.h, X.ptr, lds["x"], ww.data_ptr(), Y.ptr, lds["y"], None if bd is None else bd.data_ptr(), R.ptr, lds["R"],
                                              None if abd is None else abd.data_ptr(), Bn, H, W, cin, cout, ups, _s()))

        if refuse:
            X.load(x, GAP[0])
            R.load(r, GAP[0])
            return _refusal(ctx, name, [Y], launch, refuse)
        wref = w.flip(2, 3).transpose(0, 1) if dgrad else w
        return _case(ctx, name, [(X, x), (R, r)], [Y], [_conv_ref(x, wref, b, ups, r, ab)], launch, on(3))

    try:
        for mode in ((2, 3, 5) if precision == 1 else (3, 5)):
            ctx.check(lib.cgd_set_wino(ctx.h, mode, 0))
            out += run(mode, "below", "x", lb, lb - Ci)
            out += run(mode, "below", "x", lb, 32, gn=True)
            out += run(mode, "at", "x", la, la - Ci, refuse=WINO_REFUSE)
            out += run(mode, "beyond", "x", fl, fl - Ci, refuse=WINO_REFUSE)
            if mode != 5:
                out += run(mode, "below", "x", lb, lb - Ci, ups=1)
                out += run(mode, "below", "x", lb, lb - 64, dgrad=True)
            for far in "yR":
                co = 256 if mode == 5 else 64
                out += run(mode, "far", far, fl, fl - co)
        th.cuda.synchronize()
    finally:
        ctx.check(lib.cgd_set_wino(ctx.h, 1, 0))
        release()
    return out


def check_wino_records_far():
    """cgd_op_conv3x3_wino_ex with stats = 1 writing a far y (1 x 64 x 64, 32 -> 64; the last row starts beyond 2^31 bytes): the conv's output, no
    write outside it, and the GroupNorm over that far y, which must merge the epilogue's records (cgd_op_gn_record_merges) and match float64."""
    from cgd_amd import ops
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    B, H, W, Ci, Co = 1, 64, 64, 32, 64
    HW = H * W
    fl = far_ld(HW)
    try:
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        x = _r((B, H, W, Ci), 100)
        w = _r((Co, Ci, 3, 3), 101) / math.sqrt(9 * Ci)
        b = 50.0 + 3.0 * _r((Co,), 102)
        X = Guarded((B, H, W, Ci), Ci + 32, 32)
        X.load(x, GAP[0])
        Y = Far((B, HW, Co), fl, fl - Co)
        Y.poison(OUT_BITS[0])
        ww, bd = ops.pack_conv3x3_wino(ctx, w.to(DEV)), b.to(DEV)
        ctx.check(lib.cgd_op_conv3x3_wino_ex(ctx.h, X.ptr, Ci + 32, ww.data_ptr(), Y.ptr, fl, bd.data_ptr(), None, 0, None, B, H, W, Ci, Co, 0, 1,
                                             None, 0, None, _s()))
        th.cuda.synchronize()
        yref = _conv_ref(x, w, b, 0).reshape(B, HW, Co)
        out.append(rec(f"wconv_ex stats=1 far y ld{fl}: content", Y.view, yref))
        out.append(_flag(f"wconv_ex stats=1 far y ld{fl}: nothing written outside the view", Y.intact(OUT_BITS[0])))
        gamma, beta = 1 + 0.1 * _r((Co,), 91), 0.1 * _r((Co,), 92)
        gd, btd = gamma.to(DEV), beta.to(DEV)
        scr = ops.gn_scratch(ctx, B, HW, Co, DEV)
        Yn = Guarded((B, HW, Co), Co + 4, 0, 4)
        Yn.poison(OUT_BITS[0])
        m0 = int(lib.cgd_op_gn_record_merges(ctx.h))
        ctx.check(lib.cgd_op_gn_fwd(ctx.h, Y.ptr, fl, Yn.ptr, Co + 4, B, HW, Co, gd.data_ptr(), btd.data_ptr(), None, 1, 1e-5, scr.data_ptr(), _s()))
        th.cuda.synchronize()
        out.append(_flag("gn over the far y merged the conv's records", int(lib.cgd_op_gn_record_merges(ctx.h)) == m0 + 1))
        out.append(rec("gn fwd over the far y (records)", Yn.view, _gn_ref(Y.view.cpu(), gamma, beta, 1)[0]))
        out.append(_flag("gn fwd over the far y: nothing written outside the view", Yn.intact(OUT_BITS[0])))
    finally:
        release()
    return out


# ---------------------------------------------------------------------------------------------------------
# (B, HW, C): the register-cached float4 single-launch kernels; their streaming form (C / 32 = 64 channels per group: 16 float4 per pixel, more
# than 8 vectors per thread from 513 pixels on, forward and backward); the scalar single-launch kernels (3 channels per group); the chunked kernels
GN_SHAPES = (("register-cached", 2, 256, 128), ("streaming", 1, 520, 2048), ("scalar", 2, 300, 96), ("chunked", 2, 2048, 64))


def check_gn_far(tier_b=False):
    """cgd_op_gn_fwd / _bwd with ldx, ldy, lddz, lddx, ldadd far in turn (no guard: all must be right).  tier_b: ldy of the forward beyond 2^31
    floats on the register-cached and the chunked shapes."""
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    gn = ("groupnorm", lambda c: c[2] >= 1)
    names = ("ldx", "ldy", "lddz", "lddx", "ldadd")
    try:
        for tag, B, HW, Cc in (GN_SHAPES[0], GN_SHAPES[3]) if tier_b else GN_SHAPES:
            x = _r((B, HW, Cc), 20) * 2 + 0.7
            gamma, beta = 1 + 0.1 * _r((Cc,), 21), 0.1 * _r((Cc,), 22)
            dz, add = _r((B, HW, Cc), 24), _r((B, HW, Cc), 25, 0.3)
            yref, dxref = _gn_ref(x, gamma, beta, 1, dz, add)
            sd = unit_seed(dxref)
            gd, bd = gamma.to(DEV), beta.to(DEV)
            scr = th.zeros(int(lib.cgd_op_gn_scratch_floats(B, HW, Cc)), device=DEV)
            fl = far_ld(B * HW, elements=tier_b)
            for which in ((1,) if tier_b else range(5)):
                for col in (fl - Cc, 16):
                    lds = [Cc + d for d in (32, 8, 64, 16, 4)]
                    cols = [16, 4, 32, 8, 0]
                    lds[which], cols[which] = fl, col
                    X, Y, DZ, DX, AD = (_op((B, HW, Cc), lds[i], cols[i], i == which, tier_b) for i in range(5))
                    name = f"gn {tag} B{B} HW{HW} C{Cc} far {names[which]} {fl}+{col}{' (tier B)' if tier_b else ''}"

                    def fwd():
                        ctx.check(lib.cgd_op_new_pass(ctx.h))
                        ctx.check(lib.cgd_op_gn_fwd(ctx.h, X.ptr, lds[0], Y.ptr, lds[1], B, HW, Cc, gd.data_ptr(), bd.data_ptr(), None, 1, 1e-5,
                                                    scr.data_ptr(), _s()))

                    def bwd():
                        ctx.check(lib.cgd_op_gn_bwd(ctx.h, X.ptr, lds[0], DZ.ptr, lds[2], DX.ptr, lds[3], AD.ptr, lds[4], B, HW, Cc, 1, scr.data_ptr(), _s()))

                    if which in (0, 1):
                        out += _case(ctx, name + " fwd", [(X, x)], [Y], [yref], fwd, gn)
                    else:
                        X.load(x, GAP[0])
                        Y.poison(OUT_BITS[0])
                        fwd()  # the statistics the backward reads
                    if which != 1:
                        out += _case(ctx, name + " bwd (unit peak)", [(X, x), (DZ, dz * sd), (AD, add * sd)], [DX], [dxref * sd], bwd, gn)
        th.cuda.synchronize()
    finally:
        release()
    return out


# ---------------------------------------------------------------------------------------------------------
def check_thin_out_far():
    """cgd_op_conv_thin_out (64 -> 3, 16 x 24) on a far x: the im2col GEMM route, the last pixel's row beyond 2^31 bytes"""
    from cgd_amd import ops
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    Bn, H, W, Ci, Co = 1, 16, 24, 64, 3
    fl = far_ld(Bn * H * W)
    try:
        for col in (fl - Ci, 32):
            x = _r((Bn, H, W, Ci), 15)
            w = _r((Co, Ci, 3, 3), 13) / math.sqrt(9 * Ci)
            b = _r((Co,), 14, 0.3)
            wf, _ = ops.pack_conv3x3(w)
            wfd, bd = wf.to(DEV), b.to(DEV)
            X, Y = Far((Bn, H, W, Ci), fl, col), Guarded((Bn, Co, H, W), None, 0, 4)
            ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)

            def launch():
                ctx.check(lib.cgd_op_conv_thin_out(ctx.h, X.ptr, fl, wfd.data_ptr(), bd.data_ptr(), Y.ptr, Bn, H, W, Ci, Co, _s()))

            out += _case(ctx, f"conv_thin_out {Ci}->{Co} far x {fl}+{col}", [(X, x)], [Y], [ref], launch, on(0))
        th.cuda.synchronize()
    finally:
        release()
    return out


def check_sr_stem_far():
    """cgd_op_sr_stem (B 2, 32 x 32 frame, 8 x 8 low-resolution image per sample, 32 channels) writing a far y: the only operand with a row stride"""
    from cgd_amd import ops
    from tests import superres_ref as sr
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    B, H, W, h, w_, Co = 2, 32, 32, 8, 8, 32
    x = th.randn(B, 3, H, W, generator=g(70))
    low = th.rand(B, 3, h, w_, generator=g(71)) * 2 - 1
    w = (th.rand(Co, 6, 3, 3, generator=g(72)) * 2 - 1) * (3.0 / 54) ** 0.5
    bias = th.randn(Co, generator=g(73)) * 0.02
    ref = sr.sr_stem(x, low, w, bias)
    xd, lowd, wf, bd = x.to(DEV), low.to(DEV), ops.pack_conv3x3(w.to(DEV))[0], bias.to(DEV)
    fl = far_ld(B * H * W)
    try:
        for col in (fl - Co, 16):
            Y = Far((B, H, W, Co), fl, col)

            def launch():
                ctx.check(lib.cgd_op_sr_stem(ctx.h, xd.data_ptr(), lowd.data_ptr(), B, h, w_, wf.data_ptr(), bd.data_ptr(), Y.ptr, fl, B, H, W, Co, _s()))

            out += _case(ctx, f"sr_stem B{B} {H}x{W} low {h}x{w_} C{Co} far y {fl}+{col}", [], [Y], [ref], launch,
                         NO_HALO)
        th.cuda.synchronize()
    finally:
        release()
    return out


def check_gram_far():
    """cgd_op_gram at C 64, B 2, N 512 (two slabs of 256 rows per sample) and lda = 2^20, the cap: all of sample 1 lies beyond 2^31 bytes (and
    beyond every 32-bit byte offset's reach but the slab base, which is 64-bit); lda = 2^20 + 4 is refused and writes nothing."""
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    B, N, Cc = 2, 512, 64
    scale = 1.0 / N
    a = _r((B, N, Cc), 40)
    ref = scale * th.einsum("bnc,bnd->bcd", a.double(), a.double())
    try:
        for col in ((1 << 20) - Cc, 16):
            lda = 1 << 20
            A, G = Far((B, N, Cc), lda, col), Guarded((B, Cc, Cc), None, 0, 4)

            def launch():
                ctx.check(lib.cgd_op_gram(ctx.h, A.ptr, lda, B, N, Cc, scale, G.ptr, _s()))

            out += _case(ctx, f"gram C{Cc} B{B} N{N} at the cap lda {lda}+{col}", [(A, a)], [G], [ref], launch,
                         NO_HALO)
        lda = (1 << 20) + 4
        A, G = Far((B, N, Cc), lda, lda - Cc), Guarded((B, Cc, Cc), None, 0, 4)
        A.load(a, GAP[0])
        out += _refusal(ctx, f"gram lda {lda} beyond the cap", [G], lambda: ctx.check(lib.cgd_op_gram(ctx.h, A.ptr, lda, B, N, Cc, scale, G.ptr, _s())),
                        "gram: lda must be a multiple of 4 in [C, 2^20]")
        th.cuda.synchronize()
    finally:
        release()
    return out


ALL = {"gemm_far_a_p1": lambda: check_gemm_far_a(1), "gemm_far_a_p0": lambda: check_gemm_far_a(0), "gemm_far_cr_p1": lambda: check_gemm_far_cr(1),
       "gemm_far_cr_p0": lambda: check_gemm_far_cr(0), "gemm_gn_bwd": check_gemm_gn_bwd_far, "conv_p1": lambda: check_conv_far(1),
       "conv_p0": lambda: check_conv_far(0), "wino_p1": lambda: check_wino_far(1), "wino_p0": lambda: check_wino_far(0),
       "wino_records": check_wino_records_far, "gn": check_gn_far, "thin_out": check_thin_out_far, "sr_stem": check_sr_stem_far, "gram": check_gram_far,
       "gemm_far_cr_tier_b": lambda: check_gemm_far_cr(1, tier_b=True), "gn_tier_b": lambda: check_gn_far(tier_b=True)}
