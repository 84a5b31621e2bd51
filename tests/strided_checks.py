"""Strided-operand parity of the op kernels (tests/test_gpu_strided.py), through the C ABI so that any row stride and offset can be passed.

In the nets most convs, GEMMs and GroupNorms read or write row-strided views at a channel offset (the skip-concat producers write into
their slice of the concat buffer), and every launcher picks a kernel from stride and alignment checks.  Each operand here is therefore a
view inside a larger allocation (`Guarded`): guard columns beside the slice where the stride leaves room, guard rows before and after, and
a float offset of the view into the allocation.  All guard space lies inside the allocation, so an overrun fails a comparison instead of
faulting.
- outputs: the whole allocation is poisoned with a NaN sentinel; the view must match float64 (`rec`, strict: an element left unwritten
  stays NaN and fails) and every element outside it must still hold the sentinel's bits;
- inputs: the gaps hold a large finite sentinel (1e6), so a kernel that USES out-of-view data fails grossly;
- determinism: every case runs twice, the second time into a freshly poisoned buffer (another sentinel) with other input gaps, and the
  views must be bit-identical (csrc/ has no atomics);
- route: each case runs under the launch profile (cgd_profile kinds 0 igemm / hgemm, 1 hconv2, 3 wconv, 4 kconv, 5 wconv with the
  GroupNorm-backward-sum epilogue) and asserts the kernel family it claims to cover; the GEMV (517) and kgemm (518) tile codes are
  forced, which either runs that kernel or refuses.
Misaligned pointers go only to launchers that check alignment and refuse or fall back."""
import ctypes as C
import math

import torch as th
import torch.nn.functional as F

from tests.parity_checks import DEV, _ctx, _flag, g, rec, unit_seed

OUT_BITS = (0x7FC0BEEF, 0x7FE1CAFE)  # two quiet-NaN output sentinels, one per run
GAP = (1.0e6, -7.5e5)  # input gap sentinels, one per run
KIND = {0: "igemm/hgemm", 1: "hconv2", 2: "groupnorm", 3: "wconv", 4: "kconv", 5: "wconv+gnb"}
HALO = (1, 3, 4)
ROUTE_LOG = []  # (case, claimed route, launches per profiled kind): the route table of the report


class Guarded:
    """A view of `shape` (rows of its last dimension, row stride `ld`, at column `col`) inside an allocation with `guard_rows` whole rows
    before and after it and `off` extra floats in front, so the view starts at float off + guard_rows * ld + col of the allocation."""

    def __init__(self, shape, ld=None, col=0, off=0, guard_rows=1, device=DEV):
        shape = tuple(shape)
        width = shape[-1]
        ld = width if ld is None else ld
        assert col >= 0 and col + width <= ld and guard_rows >= 1 and off >= 0
        rows = math.prod(shape[:-1])
        n = off + (rows + 2 * guard_rows) * ld
        strides, s = [], ld
        for d in reversed(shape[:-1]):
            strides.insert(0, s)
            s *= d
        strides = tuple(strides) + (1,)
        base = off + guard_rows * ld + col
        self.buf = th.zeros(n, device=device, dtype=th.float32)
        self.view = self.buf.as_strided(shape, strides, base)
        idx = th.arange(n, device=device).as_strided(shape, strides, base)
        self.inside = th.zeros(n, dtype=th.bool, device=device)
        self.inside[idx.reshape(-1)] = True
        self.ld = ld

    @property
    def ptr(self):
        return self.view.data_ptr()

    def poison(self, bits):
        self.buf.view(th.int32).fill_(bits)

    def load(self, t, gap):
        self.buf.fill_(gap)
        self.view.copy_(t)

    def intact(self, bits, whole=False):
        """every element outside the view (or, with whole=True, of the allocation) still holds the sentinel's bits"""
        w = self.buf.view(th.int32)
        if not whole:
            w = w[~self.inside]
        return bool((w == bits).all().item())


def check_out(name, G, ref, bits):
    """parity of an output view against float64 plus the check that nothing outside it was written"""
    return [rec(name, G.view, ref), _flag(f"{name}: nothing written outside the view", G.intact(bits))]


def _routes(ctx, launch):
    """launch() under the context's launch profile; returns the launches per profiled kind"""
    lib = ctx.lib
    n = lib.cgd_profile_kinds()
    buf = (C.c_double * (3 * n))()
    ctx.check(lib.cgd_profile_read(ctx.h, buf))  # drop earlier records
    ctx.check(lib.cgd_profile(ctx.h, 1))
    try:
        launch()
    finally:
        ctx.check(lib.cgd_profile(ctx.h, 0))
    ctx.check(lib.cgd_profile_read(ctx.h, buf))
    return [int(buf[3 * k + 2]) for k in range(n)]


def on(kind):
    """route predicate: `kind` ran, and no halo conv family other than it"""
    return (KIND[kind], lambda c: c[kind] >= 1 and all(c[j] == 0 for j in HALO if j != kind))


def off_halo():
    return ("igemm (no halo kernel)", lambda c: c[0] >= 1 and all(c[j] == 0 for j in HALO))


def any_halo():
    return ("a halo kernel (auto)", lambda c: sum(c[j] for j in HALO) >= 1)


def _case(ctx, name, inputs, outputs, refs, launch, route):
    """inputs: [(Guarded, values)], outputs: [Guarded], refs: float64 references of the output views, launch(): the C call(s)"""
    out, first = [], None
    for k in range(2):
        for G, t in inputs:
            G.load(t, GAP[k])
        for G in outputs:
            G.poison(OUT_BITS[k])
        counts = _routes(ctx, launch)
        got = [G.view.clone() for G in outputs]
        if k == 0:
            first = got
            for i, (G, ref) in enumerate(zip(outputs, refs)):
                out.append(rec(f"{name} out{i}", G.view, ref))
            desc, pred = route
            ROUTE_LOG.append((name, desc, counts))
            out.append(_flag(f"{name}: route {desc} (launches per kind {counts})", pred(counts)))
        for i, G in enumerate(outputs):
            out.append(_flag(f"{name} out{i}: nothing written outside the view (sentinel {k})", G.intact(OUT_BITS[k])))
    out.append(_flag(f"{name}: a rerun into a fresh sentinel is bit-identical",
                     all(th.equal(a.view(th.int32), b.view(th.int32)) for a, b in zip(first, got))))
    return out


def _refusal(ctx, name, outputs, launch, msg):
    """launch() must raise CgdError carrying `msg` before anything is written"""
    from cgd_amd.lib import CgdError
    for G in outputs:
        G.poison(OUT_BITS[0])
    try:
        launch()
        err = "(no error)"
    except CgdError as e:
        err = str(e)
    th.cuda.synchronize()
    return [_flag(f"{name}: refused with '{msg}' (got: {err})", msg in err)] + \
           [_flag(f"{name}: allocation {i} untouched after the refusal", G.intact(OUT_BITS[0], whole=True)) for i, G in enumerate(outputs)]


def _s():
    from cgd_amd import lib as L
    return L.stream_ptr()


def _r(shape, seed, scale=1.0):
    return scale * th.randn(*shape, generator=g(seed))


# ---------------------------------------------------------------------------------------------------------
def check_gemm_strided(precision=1):
    """cgd_op_gemm on strided A / B, C written into a slice of a wider buffer, R at another stride, a bias: tile codes 0 / 64 / 128 / 256 / 257 / 513 /
    517 / 518, auto and explicit split-K; the scalar epilogues (misaligned C / R / bias, ldc = 1 mod 4, N % 4 != 0); refusals of unaligned A / B / lda."""
    ctx = _ctx(precision)
    lib, out = ctx.lib, []

    def run(tag, M, N, K, tile, sk, lda=None, ldb=None, ldc=None, ldr=None, a_col=16, c_col=16, r_col=8, c_off=0, r_off=0, bias_off=0,
            a_off=0, b_off=0, route=None, refuse=None):
        lda = lda or K + 32
        ldb = ldb or K + 8
        ldc = ldc or N + 32
        ldr = ldr or N + 12
        A = Guarded((M, K), lda, a_col, a_off)
        B = Guarded((N, K), ldb, 4 if ldb >= K + 4 else 0, b_off)
        Cg = Guarded((M, N), ldc, c_col, c_off)
        R = Guarded((M, N), ldr, r_col, r_off)
        bias = Guarded((N,), None, 0, bias_off)
        a, b, r, bb = _r((M, K), 1), _r((N, K), 2), _r((M, N), 4, 0.3), _r((N,), 3, 0.3)
        alpha = 1.0 / math.sqrt(K)
        name = f"gemm[p{precision}] {tag} {M}x{N}x{K} tile{tile} sk{sk} lda{lda} ldb{ldb} ldc{ldc}+{c_col}(+{c_off}) ldr{ldr}(+{r_off}) bias+{bias_off}"

        def launch():
            ctx.check(lib.cgd_op_gemm(ctx.h, A.ptr, lda, B.ptr, ldb, Cg.ptr, ldc, bias.ptr, R.ptr, ldr, M, N, K, alpha, tile, sk, _s()))

        if refuse:
            for G, t in ((A, a), (B, b), (R, r), (bias, bb)):
                G.load(t, GAP[0])
            return _refusal(ctx, name, [Cg], launch, refuse)
        ref = alpha * (a.double() @ b.double().T) + bb.double() + r.double()
        return _case(ctx, name, [(A, a), (B, b), (R, r), (bias, bb)], [Cg], [ref], launch, route or on(0))

    for tile, sk in ((0, 1), (0, 3), (64, 1), (128, 2), (256, 1), (257, 4), (64, 2)):
        out += run("strided", 130, 100, 256, tile, sk)
    out += run("strided", 3, 100, 256, 517, 1)  # GEMV
    out += run("scalar epilogue", 3, 97, 256, 517, 1, ldc=101, c_off=1, r_off=1, bias_off=1, c_col=3)
    if precision != 0:
        for tile, sk in ((513, 1), (513, 2), (513, 0), (518, 1)):
            out += run("strided", 70, 96, 256, tile, sk)
    # the scalar epilogues: misaligned C / R / bias, ldc = 1 mod 4, N % 4 != 0 (igemm's epilogue and the split-K reduce both)
    for tile, sk in ((64, 1), (64, 3), (0, 1)):
        out += run("scalar epilogue", 130, 97, 256, tile, sk, ldc=113, ldr=101, c_off=1, r_off=1, bias_off=1, c_col=3, r_col=4)
    out += run("N%4 aligned", 130, 98, 256, 64, 3)
    out += run("bias misaligned", 130, 96, 256, 128, 2, bias_off=1)
    # refusals: nothing may be written
    out += run("lda%4", 130, 100, 256, 0, 1, lda=257, a_col=0, refuse="K, lda, ldb must be multiples of 4")
    out += run("A+1", 130, 100, 256, 0, 1, a_off=1, refuse="A/B must be 16-byte aligned")
    out += run("B+1", 130, 100, 256, 64, 1, b_off=1, refuse="A/B must be 16-byte aligned")
    if precision != 0:
        out += run("C+1 forced 513", 70, 96, 256, 513, 1, c_off=1, refuse="weight GEMM kernel does not support this problem")
        out += run("bias+1 forced 518", 70, 96, 256, 518, 1, bias_off=1, refuse="few-row weight GEMM kernel does not support this problem")
    th.cuda.synchronize()
    return out


def _conv_ref(x, w, b, ups, r=None, ab=None):
    """NHWC float64 reference of conv3x3(pad 1) on x (B,Hs,Ws,Ci) [optionally SiLU(x*a+b) first, nearest-2x upsampled] + bias + R"""
    xa = x.double().permute(0, 3, 1, 2)
    if ab is not None:
        xa = F.silu(xa * ab[:, :, 0, None, None].double() + ab[:, :, 1, None, None].double())
    if ups:
        xa = F.interpolate(xa, scale_factor=2, mode="nearest")
    y = F.conv2d(xa, w.double(), None if b is None else b.double(), padding=1).permute(0, 2, 3, 1)
    return y if r is None else y + r.double()


def check_conv_strided(precision=1):
    """cgd_op_conv3x3: x a channel slice of a concat (at offset 0 and at the sibling's width), y into a slice, R at another stride; igemm
    64 / 128, hconv2 (512, variants 0 / 1 / 4 / 5), kconv (516) and auto; upsampled input, split-K, batch 2, dgrad packing; misaligned y / R
    (auto: no halo kernel may run), forced halo routes that cannot run, an x stride that is not a multiple of 4."""
    from cgd_amd import ops
    ctx = _ctx(precision)
    lib, out = ctx.lib, []
    Bn, H, W, Ci, Cother, Co = 2, 16, 16, 64, 32, 64

    def run(tag, tile, var=0, x_col=Cother, ups=0, sk=1, dgrad=False, y_off=0, ldr=Co + 48, r_col=4, r_off=0, ldx=Ci + Cother, route=None,
            refuse=None):
        if var is not None and tile in (0, 512, 516):
            ctx.check(lib.cgd_set_hconv(ctx.h, 1 + 16 * var, 256))
        cin, cout = (Co, Ci) if dgrad else (Ci, Co)
        ldx = ldx if not dgrad else cin + Cother
        Hs, Ws = (H // 2, W // 2) if ups else (H, W)
        w = _r((Co, Ci, 3, 3), 6) / math.sqrt(9 * (Co if dgrad else Ci))
        wf, wd = ops.pack_conv3x3(w)
        wt = (wd if dgrad else wf).to(DEV)
        wfrag = ops.pack_conv3x3_frag(ctx, w.to(DEV), dgrad=dgrad)
        x = _r((Bn, Hs, Ws, cin), 5)
        b = None if dgrad else _r((cout,), 7, 0.3)
        r = _r((Bn, H, W, cout), 17, 0.3)
        X = Guarded((Bn, Hs, Ws, cin), ldx, x_col)
        Y = Guarded((Bn, H, W, cout), cout + 32, 16, y_off)
        R = Guarded((Bn, H, W, cout), ldr, r_col, r_off)
        # the residual is read at its own stride and column: a kernel that read it through y's stride / offset would fail
        assert (ldr, r_col) != (cout + 32, 16)
        bd = None if b is None else b.to(DEV)
        name = f"conv3x3[p{precision}] {tag} tile{tile} var{var} B{Bn} {H}x{W} {cin}->{cout} ldx{ldx}+{x_col} ups{ups} sk{sk}" + \
               f"{' dgrad' if dgrad else ''} ldy{cout + 32}+16(+{y_off}) ldr{ldr}+{r_col}(+{r_off})"

        def launch():
            ctx.check(lib.cgd_op_conv3x3(ctx.h, X.ptr, ldx, wt.data_ptr(), wfrag.data_ptr(), Y.ptr, cout + 32, None if bd is None else bd.data_ptr(),
                                         R.ptr, ldr, Bn, H, W, cin, cout, ups, tile, sk, _s()))

        if refuse:
            X.load(x, GAP[0])
            R.load(r, GAP[0])
            res = _refusal(ctx, name, [Y], launch, refuse)
        else:
            wref = w.flip(2, 3).transpose(0, 1) if dgrad else w
            res = _case(ctx, name, [(X, x), (R, r)], [Y], [_conv_ref(x, wref, b, ups, r)], launch, route)
        ctx.check(lib.cgd_set_hconv(ctx.h, 1, 256))  # the default variant
        return res

    for tile in (64, 128):
        out += run("concat slice", tile, route=off_halo())
    out += run("concat slice at 0", 64, x_col=0, route=off_halo())
    out += run("dgrad", 64, dgrad=True, route=off_halo())
    auto = any_halo() if precision != 0 else off_halo()  # exact-fp32 contexts have no halo kernel for this op (no Winograd weights)
    out += run("auto", 0, route=auto)
    out += run("auto ups", 0, ups=1, route=auto)
    if precision != 0:
        for var in (0, 1, 4, 5):
            out += run("concat slice", 512, var=var, route=on(1))
        out += run("concat slice at 0", 512, x_col=0, route=on(1))
        out += run("ups sk2", 512, ups=1, sk=2, route=on(1))
        out += run("dgrad", 512, dgrad=True, route=on(1))
        out += run("concat slice", 516, route=on(4))
        out += run("ups", 516, ups=1, route=on(4))
        out += run("sk2", 516, sk=2, route=on(4))
        out += run("dgrad", 516, dgrad=True, route=on(4))
        # misaligned y / R: the halo kernels' 16-byte epilogues must step aside, igemm (scalar epilogue) computes it
        out += run("y+1 R ldr%4=2 auto", 0, y_off=1, ldr=Co + 2, r_col=0, route=off_halo())
        out += run("R+1 auto", 0, r_off=1, route=off_halo())
        out += run("y+1 forced 512", 512, y_off=1, refuse="halo conv kernel does not support this problem")
        out += run("y+1 forced 516", 516, y_off=1, refuse="weight-streaming conv kernel does not support this problem")
    out += run("ldx%4=2", 0, ldx=Ci + Cother + 2, x_col=2, refuse="K, lda, ldb must be multiples of 4")
    th.cuda.synchronize()
    return out


def check_wino_strided(precision=1):
    """cgd_op_conv3x3_wino on a strided x slice, y into a slice, R at another stride, with and without gn_ab, every tile mode of the
    precision; a misaligned y refused."""
    from cgd_amd import ops
    ctx = _ctx(precision)
    lib, out = ctx.lib, []
    for mode in ((2, 3, 5) if precision == 1 else (3, 5)):
        ctx.check(lib.cgd_set_wino(ctx.h, mode, 0))
        for (Bn, H, W, Ci, Co, ups, gn) in [(1, 32, 32, 32, 64, 0, 1), (2, 16, 32, 64, 256 if mode == 5 else 96, 1, 0)]:
            Hs, Ws = (H // 2, W // 2) if ups else (H, W)
            x = _r((Bn, Hs, Ws, Ci), 5)
            w = _r((Co, Ci, 3, 3), 6) / math.sqrt(9 * Ci)
            b = _r((Co,), 7, 0.3)
            r = _r((Bn, H, W, Co), 17, 0.3)
            ab = th.stack([0.5 + th.rand(Bn, Ci, generator=g(18)), 0.5 * th.randn(Bn, Ci, generator=g(19))], dim=2).contiguous() if gn else None
            ww = ops.pack_conv3x3_wino(ctx, w.to(DEV))
            bd, abd = b.to(DEV), None if ab is None else ab.to(DEV)
            ldx, ldy, ldr = Ci + 32, Co + 64, Co + 4
            X, Y, R = Guarded((Bn, Hs, Ws, Ci), ldx, 32), Guarded((Bn, H, W, Co), ldy, 32), Guarded((Bn, H, W, Co), ldr, 4)
            name = f"wconv[p{precision}] m{mode} B{Bn} {H}x{W} {Ci}->{Co} ups{ups} gn{gn} ldx{ldx}+32 ldy{ldy}+32 ldr{ldr}+4"

            def launch(X=X, Y=Y, R=R, ldx=ldx, ldy=ldy, ldr=ldr, ww=ww, bd=bd, abd=abd, Bn=Bn, H=H, W=W, Ci=Ci, Co=Co, ups=ups):
                ctx.check(lib.cgd_op_conv3x3_wino(ctx.h, X.ptr, ldx, ww.data_ptr(), Y.ptr, ldy, bd.data_ptr(), R.ptr, ldr,
                                                  None if abd is None else abd.data_ptr(), Bn, H, W, Ci, Co, ups, _s()))

            out += _case(ctx, name, [(X, x), (R, r)], [Y], [_conv_ref(x, w, b, ups, r, ab)], launch, on(3))
    Y1 = Guarded((1, 32, 32, 64), 96, 16, 1)
    X1 = Guarded((1, 32, 32, 32), 64, 32)
    X1.load(_r((1, 32, 32, 32), 5), GAP[0])
    ww = ops.pack_conv3x3_wino(ctx, (_r((64, 32, 3, 3), 6) / math.sqrt(288)).to(DEV))
    out += _refusal(ctx, f"wconv[p{precision}] y+1", [Y1], lambda: ctx.check(lib.cgd_op_conv3x3_wino(
        ctx.h, X1.ptr, 64, ww.data_ptr(), Y1.ptr, 96, None, None, 0, None, 1, 32, 32, 32, 64, 0, _s())),
                    "Winograd conv kernel does not support this problem")
    ctx.check(lib.cgd_set_wino(ctx.h, 1, 0))
    th.cuda.synchronize()
    return out


def _gn_ref(x, gamma, beta, act, dz=None, add=None):
    """float64 GroupNorm(32) (+ SiLU) of x (B,HW,C) and, with dz, its input gradient (+ add)"""
    xr = x.double().requires_grad_()
    y = F.group_norm(xr.permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-5)
    if act:
        y = F.silu(y)
    y = y.permute(0, 2, 1)
    if dz is None:
        return y.detach(), None
    (y * dz.double()).sum().backward()
    dx = xr.grad
    return y.detach(), dx if add is None else dx + add.double()


def check_wino_records_strided():
    """cgd_op_conv3x3_wino_ex: the two halves of a concat that itself sits at an offset inside a wider buffer take GroupNorm statistics
    records (stats=1), which the GroupNorm over the concat merges; a dgrad conv takes the backward sums from a strided GroupNorm input
    (gnb_ldx > Cin: the epilogue runs, kind 5, and gn_bwd merges) or not (gnb_ldx = 2 mod 4: no kind-5 launch, gn_bwd sweeps)."""
    from cgd_amd import ops
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    merges = lambda: int(lib.cgd_op_gn_record_merges(ctx.h))  # noqa: E731
    B, H, W, Ci, C0, C1 = 1, 64, 64, 32, 64, 32
    HW, Ct, ldcat = H * W, C0 + C1, 128
    ctx.check(lib.cgd_op_new_pass(ctx.h))
    cat = Guarded((B, HW, Ct), ldcat, 16)
    cat.poison(OUT_BITS[0])
    xs, ws, bs = [], [], []
    for i, Cn in enumerate((C0, C1)):
        xs.append(_r((B, H, W, Ci), 100 + 10 * i))
        ws.append(_r((Cn, Ci, 3, 3), 101 + 10 * i) / math.sqrt(9 * Ci))
        bs.append(50.0 + 3.0 * _r((Cn,), 102 + 10 * i))
    X = Guarded((B, H, W, Ci), Ci + 32, 32)
    counts = [0] * 6
    for i, (Cn, c_off) in enumerate(((C0, 0), (C1, C0))):
        X.load(xs[i], GAP[0])
        ww = ops.pack_conv3x3_wino(ctx, ws[i].to(DEV))
        bd = bs[i].to(DEV)
        c = _routes(ctx, lambda: ctx.check(lib.cgd_op_conv3x3_wino_ex(ctx.h, X.ptr, Ci + 32, ww.data_ptr(), cat.ptr + 4 * c_off, ldcat, bd.data_ptr(),
                                                                     None, 0, None, B, H, W, Ci, Cn, 0, 1, None, 0, None, _s())))
        counts = [a + b for a, b in zip(counts, c)]
    ROUTE_LOG.append(("wconv_ex stats=1 into a concat slice (2 launches)", KIND[3], counts))
    out.append(_flag(f"wconv_ex stats: both halves ran on wconv (launches per kind {counts})", counts[3] == 2))
    out.append(_flag("wconv_ex stats: nothing written outside the concat slice", cat.intact(OUT_BITS[0])))
    yref = th.cat([_conv_ref(xs[i], ws[i], bs[i], 0) for i in range(2)], dim=3).reshape(B, HW, Ct)
    out.append(rec("wconv_ex stats: concat content", cat.view, yref))
    gamma, beta = 1 + 0.1 * _r((Ct,), 91), 0.1 * _r((Ct,), 92)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    scr = ops.gn_scratch(ctx, B, HW, Ct, DEV)
    Yn = Guarded((B, HW, Ct), Ct + 4, 0, 4)
    Yn.poison(OUT_BITS[0])
    m0 = merges()
    ctx.check(lib.cgd_op_gn_fwd(ctx.h, cat.ptr, ldcat, Yn.ptr, Ct + 4, B, HW, Ct, gd.data_ptr(), bd.data_ptr(), None, 1, 1e-5, scr.data_ptr(), _s()))
    th.cuda.synchronize()
    out.append(_flag("gn over the strided concat merged the records of both halves", merges() == m0 + 1))
    out += check_out("gn fwd over the strided concat (records)", Yn, _gn_ref(cat.view.cpu(), gamma, beta, 1)[0], OUT_BITS[0])

    # backward sums: dz = dgrad conv output, its epilogue reads the norm's input xn through gnb_x / gnb_ldx
    Cn = 64
    xn = 3.0 + _r((B, HW, Cn), 130)
    gam_b, bet_b = 1 + 0.1 * _r((Cn,), 93), 0.1 * _r((Cn,), 94)
    gbd, bbd = gam_b.to(DEV), bet_b.to(DEV)
    dy = _r((B, H, W, Cn), 140)
    wd = _r((Cn, Cn, 3, 3), 141) / math.sqrt(9 * Cn)
    wwd = ops.pack_conv3x3_wino(ctx, wd.to(DEV), dgrad=True)
    dzref = _conv_ref(dy, wd.flip(2, 3).transpose(0, 1), None, 0).reshape(B, HW, Cn)
    _, dxref = _gn_ref(xn, gam_b, bet_b, 1, dzref.float())
    sd = unit_seed(dxref)
    for gld, col, want in ((Cn + 32, 16, True), (Cn + 2, 2, False)):
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        xn_d = xn.to(DEV)  # the GroupNorm itself runs on an aligned copy (its wide-map kernels need 4-float strides)
        scrb = ops.gn_scratch(ctx, B, HW, Cn, DEV)
        ctx.check(lib.cgd_op_gn_fwd(ctx.h, xn_d.data_ptr(), Cn, None, 4, B, HW, Cn, gbd.data_ptr(), bbd.data_ptr(), None, 1, 1e-5,
                                    scrb.data_ptr(), _s()))
        XN = Guarded((B, HW, Cn), gld, col)
        XN.load(xn, GAP[0])
        DY = Guarded((B, H, W, Cn), Cn + 32, 32)
        DY.load(dy * sd, GAP[0])
        DZ = Guarded((B, HW, Cn), Cn + 16, 8)
        DZ.poison(OUT_BITS[0])
        c = _routes(ctx, lambda: ctx.check(lib.cgd_op_conv3x3_wino_ex(ctx.h, DY.ptr, Cn + 32, wwd.data_ptr(), DZ.ptr, Cn + 16, None, None, 0, None,
                                                                     B, H, W, Cn, Cn, 0, 0, XN.ptr, gld, scrb.data_ptr(), _s())))
        tag = f"wconv_ex gnb_ldx {gld} (= {gld % 4} mod 4)"
        ROUTE_LOG.append((tag, KIND[5] if want else f"{KIND[3]}, no backward sums", c))
        out.append(_flag(f"{tag}: backward-sum epilogue {'ran' if want else 'did not run'} (launches per kind {c})",
                         (c[5] == 1) if want else (c[5] == 0 and c[3] == 1)))
        out += check_out(f"{tag}: dz", DZ, dzref * sd, OUT_BITS[0])
        m0 = merges()
        DX = Guarded((B, HW, Cn), Cn + 8, 4)
        DX.poison(OUT_BITS[0])
        ctx.check(lib.cgd_op_gn_bwd(ctx.h, xn_d.data_ptr(), Cn, DZ.ptr, Cn + 16, DX.ptr, Cn + 8, None, 0, B, HW, Cn, 1, scrb.data_ptr(), _s()))
        th.cuda.synchronize()
        out.append(_flag(f"{tag}: gn_bwd {'merged the records' if want else 'swept'}", merges() == m0 + (1 if want else 0)))
        out += check_out(f"{tag}: gn_bwd dx (unit peak)", DX, dxref * sd, OUT_BITS[0])
    return out


def check_thin_out_strided():
    """cgd_op_conv_thin_out on a channel slice: the im2col GEMM route (aligned slice) and the direct kernel (ldx = 2 mod 4)"""
    from cgd_amd import ops
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    Bn, H, W, Ci = 2, 16, 24, 64
    for Co in (3, 6):
        for ldx, col, route in ((96, 32, on(0)), (98, 2, ("direct kernel (no GEMM)", lambda c: c[0] == 0))):
            x = _r((Bn, H, W, Ci), 15)
            w = _r((Co, Ci, 3, 3), 13) / math.sqrt(9 * Ci)
            b = _r((Co,), 14, 0.3)
            wf, _ = ops.pack_conv3x3(w)
            wfd, bd = wf.to(DEV), b.to(DEV)
            X, Y = Guarded((Bn, H, W, Ci), ldx, col), Guarded((Bn, Co, H, W), None, 0, 4)
            ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1)

            def launch(X=X, Y=Y, ldx=ldx, wfd=wfd, bd=bd, Co=Co):
                ctx.check(lib.cgd_op_conv_thin_out(ctx.h, X.ptr, ldx, wfd.data_ptr(), bd.data_ptr(), Y.ptr, Bn, H, W, Ci, Co, _s()))

            out += _case(ctx, f"conv_thin_out {Ci}->{Co} ldx{ldx}+{col}", [(X, x)], [Y], [ref], launch, route)
    return out


def check_gn_strided():
    """cgd_op_gn_fwd / _bwd with ldx, ldy, lddz, lddx and ldadd all different: the single-launch kernels (v4 and scalar: 3 channels per
    group, odd backward strides, views 1 float into their allocation) and the chunked kernels; the refusals of odd forward strides and of
    odd strides / misaligned views above the single-launch size."""
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    # the profile has one kind for every GroupNorm kernel: this shows that a GroupNorm ran, not which of the v4 / scalar single-launch or
    # chunked kernels it was (the HW and the strides / offsets of each case decide that, norm.hip launch_gn_small_*)
    gn = ("groupnorm", lambda c: c[2] >= 1)

    def run(tag, B, HW, Cc, act=1, lds=(None,) * 5, offs=(0,) * 5, refuse_fwd=None, refuse_bwd=None):
        ldx, ldy, lddz, lddx, ldadd = (l or Cc + d for l, d in zip(lds, (32, 8, 64, 16, 4)))
        X = Guarded((B, HW, Cc), ldx, 16 if ldx >= Cc + 16 else 0, offs[0])
        Y = Guarded((B, HW, Cc), ldy, 4 if ldy >= Cc + 4 else 0, offs[1])
        DZ = Guarded((B, HW, Cc), lddz, 32 if lddz >= Cc + 32 else 0, offs[2])
        DX = Guarded((B, HW, Cc), lddx, 8 if lddx >= Cc + 8 else 0, offs[3])
        AD = Guarded((B, HW, Cc), ldadd, 0, offs[4])
        x = _r((B, HW, Cc), 20) * 2 + 0.7
        gamma, beta = 1 + 0.1 * _r((Cc,), 21), 0.1 * _r((Cc,), 22)
        dz, add = _r((B, HW, Cc), 24), _r((B, HW, Cc), 25, 0.3)
        yref, dxref = _gn_ref(x, gamma, beta, act, dz, add)
        gd, bd = gamma.to(DEV), beta.to(DEV)
        scr = th.zeros(int(lib.cgd_op_gn_scratch_floats(B, HW, Cc)), device=DEV)
        name = f"gn {tag} B{B} HW{HW} C{Cc} act{act} ld x{ldx} y{ldy} dz{lddz} dx{lddx} add{ldadd} offs{offs}"

        def fwd():
            ctx.check(lib.cgd_op_new_pass(ctx.h))
            ctx.check(lib.cgd_op_gn_fwd(ctx.h, X.ptr, ldx, Y.ptr, ldy, B, HW, Cc, gd.data_ptr(), bd.data_ptr(), None, act, 1e-5, scr.data_ptr(), _s()))

        def bwd():
            ctx.check(lib.cgd_op_gn_bwd(ctx.h, X.ptr, ldx, DZ.ptr, lddz, DX.ptr, lddx, AD.ptr, ldadd, B, HW, Cc, act, scr.data_ptr(), _s()))

        if refuse_fwd:
            X.load(x, GAP[0])
            return _refusal(ctx, name + " fwd", [Y], fwd, refuse_fwd)
        res = _case(ctx, name + " fwd", [(X, x)], [Y], [yref], fwd, gn)
        if refuse_bwd:
            for G, t in ((DZ, dz), (AD, add)):
                G.load(t, GAP[0])
            return res + _refusal(ctx, name + " bwd", [DX], bwd, refuse_bwd)
        return res + _case(ctx, name + " bwd", [(X, x), (DZ, dz), (AD, add)], [DX], [dxref], bwd, gn)

    out += run("single-launch v4", 2, 256, 128)
    out += run("single-launch cpg3", 2, 300, 96)
    out += run("single-launch act0", 1, 1024, 64, act=0)
    out += run("single-launch odd bwd strides", 2, 256, 128, lds=(None, None, 129, 133, 131))
    out += run("single-launch views at +1 float", 2, 256, 128, offs=(1, 1, 1, 1, 1))
    out += run("single-launch views at +2 floats", 1, 200, 64, offs=(2, 0, 0, 2, 0))
    out += run("chunked", 2, 2048, 64)
    out += run("chunked cpg3", 1, 5000, 96, act=0)
    out += run("odd fwd stride", 2, 256, 128, lds=(130, None, None, None, None), refuse_fwd="row strides must be multiples of 4")
    out += run("chunked x+1", 1, 2048, 64, offs=(1, 0, 0, 0, 0), refuse_fwd="16-byte aligned above the single-launch size")
    out += run("chunked odd bwd stride", 1, 2048, 64, lds=(None, None, 97, None, None), refuse_bwd="row strides must be multiples of 4")
    out += run("chunked dx+1", 1, 2048, 64, offs=(0, 0, 0, 1, 0), refuse_bwd="row strides must be multiples of 4")
    th.cuda.synchronize()
    return out


def check_ln_act_strided():
    """cgd_op_ln_fwd / _bwd at C = 96 / 640 / 1280 (the generic kernels) and 768 / 1024 (the vector kernels) and on views 1 float into
    their allocation (generic); cgd_op_act with n % 4 != 0, a view 1 float in, and inputs in the exp overflow tails (|x| up to 100)."""
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    any_route = ("elementwise (no profiled kind)", lambda c: sum(c[j] for j in (0, 1, 3, 4)) == 0)
    for rows, Cc, off in ((50, 96, 0), (33, 640, 0), (20, 1280, 0), (50, 768, 0), (7, 1024, 0), (50, 768, 1), (9, 1024, 3)):
        x = _r((rows, Cc), 25) * 1.5 + 0.3
        gamma, beta = 1 + 0.1 * _r((Cc,), 26), 0.1 * _r((Cc,), 27)
        dy = _r((rows, Cc), 28)
        xr = x.double().requires_grad_()
        y = F.layer_norm(xr, (Cc,), gamma.double(), beta.double(), 1e-5)
        (y * dy.double()).sum().backward()
        sd = unit_seed(xr.grad)
        gd, bd = gamma.to(DEV), beta.to(DEV)
        stats = th.zeros(rows, 2, device=DEV)
        X, Y, DY, DX = (Guarded((rows, Cc), None, 0, off) for _ in range(4))
        name = f"layernorm {rows}x{Cc} views +{off}"

        def fwd(X=X, Y=Y, rows=rows, Cc=Cc, gd=gd, bd=bd, stats=stats):
            ctx.check(lib.cgd_op_ln_fwd(ctx.h, X.ptr, Y.ptr, rows, Cc, gd.data_ptr(), bd.data_ptr(), 1e-5, stats.data_ptr(), _s()))

        def bwd(X=X, DY=DY, DX=DX, rows=rows, Cc=Cc, gd=gd, stats=stats):
            ctx.check(lib.cgd_op_ln_bwd(ctx.h, X.ptr, DY.ptr, DX.ptr, rows, Cc, gd.data_ptr(), stats.data_ptr(), _s()))

        out += _case(ctx, name + " fwd", [(X, x)], [Y], [y.detach()], fwd, any_route)
        out += _case(ctx, name + " bwd", [(X, x), (DY, dy * sd)], [DX], [xr.grad * sd], bwd, any_route)
    n = 1001
    v = th.cat([3 * _r((n - 200,), 31), th.linspace(-100, 100, 200)])
    dyv = _r((n,), 32)
    for kind, fn in ((1, F.silu), (2, lambda t: t * th.sigmoid(1.702 * t))):
        for off in (0, 1):
            vr = v.double().requires_grad_()
            yy = fn(vr)
            (yy * dyv.double()).sum().backward()
            X, DYg, Y = Guarded((n,), None, 0, off), Guarded((n,), None, 0, off), Guarded((n,), None, 0, off)

            def f(X=X, Y=Y, kind=kind):
                ctx.check(lib.cgd_op_act(ctx.h, X.ptr, None, Y.ptr, n, kind, _s()))

            def b(X=X, DYg=DYg, Y=Y, kind=kind):
                ctx.check(lib.cgd_op_act(ctx.h, X.ptr, DYg.ptr, Y.ptr, n, kind, _s()))

            out += _case(ctx, f"act{kind} fwd n{n} +{off} |x| <= 100", [(X, v)], [Y], [yy.detach()], f, any_route)
            out += _case(ctx, f"act{kind} bwd n{n} +{off} |x| <= 100", [(X, v), (DYg, dyv)], [Y], [vr.grad], b, any_route)
    return out


def check_resample_refusals():
    """cgd_op_pool2x2 / _upsample2x: C % 4 != 0 and views that are not 16-byte aligned are refused, and nothing is written"""
    ctx = _ctx(1)
    lib, out = ctx.lib, []
    for nm, fn, (Hi, Ho) in (("pool2x2", lib.cgd_op_pool2x2, (8, 4)), ("upsample2x", lib.cgd_op_upsample2x, (4, 8))):
        for Cc, off, msg in ((6, 0, "C and strides must be multiples of 4"), (8, 1, "16-byte aligned")):
            X, Y = Guarded((2, Hi, Hi, Cc), None, 0, 4), Guarded((2, Ho, Ho, Cc), None, 0, off)
            X.load(_r((2, Hi, Hi, Cc), 30), GAP[0])
            scale = 0.25 if nm == "pool2x2" else 1.0
            out += _refusal(ctx, f"{nm} C{Cc} out+{off}", [Y], lambda fn=fn, X=X, Y=Y, Cc=Cc, scale=scale: ctx.check(
                fn(ctx.h, X.ptr, Y.ptr, 2, Ho, Ho, Cc, scale, _s())), msg)
    return out


ALL = {"gemm_p1": lambda: check_gemm_strided(1), "gemm_p0": lambda: check_gemm_strided(0), "conv_p1": lambda: check_conv_strided(1),
       "conv_p0": lambda: check_conv_strided(0), "wino_p1": lambda: check_wino_strided(1), "wino_p0": lambda: check_wino_strided(0),
       "wino_records": check_wino_records_strided, "thin_out": check_thin_out_strided, "gn": check_gn_strided, "ln_act": check_ln_act_strided,
       "resample": check_resample_refusals}


if __name__ == "__main__":  # one report: every record and the route table, as JSON on stdout
    import json
    import sys
    recs = []
    for key, fn in ALL.items():
        recs += [dict(r, group=key) for r in fn()]
    bad = [r for r in recs if not r["ok"]]
    json.dump({"records": recs, "failed": len(bad), "routes": ROUTE_LOG}, sys.stdout, indent=1, default=str)
    print()
    sys.exit(1 if bad else 0)
