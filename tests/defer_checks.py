"""Deferred split-K slices through the kernels that sum them (tests/test_gpu_defer.py; host half: tests/test_defer_host.py).

A conv or GEMM launched with `defer` leaves its K slices in the context workspace; the GroupNorm / LayerNorm that reads the tensor next sums
them at load time (csrc/norm.hip split_load4 / split_load1) and writes the finished tensor back; anything else runs the reduce launch first.
Every case here says WHICH of the two happened, through the host-side view of the pending entry (`cgd_op_pending`) and the reduce counter of
`cgd_launch_counts`:
- the output C is NaN before the producer (with an in-place residual: the residual's values): a split producer writes only the workspace, so a
  reader of the unreduced tensor cannot pass;
- after the producer the entry is pending with exactly the requested slice count, rows, columns and row stride, and no reduce launch ran;
- after a consumer that takes the slices the counter has not moved and nothing is pending; after one that must flush it has moved by one;
- the tensor written back is `th.equal` to the same producer's output with defer = 0 (the control; graded once against the float64 conv / GEMM);
- y, the statistics and dx are graded with `rec` at the literal 1e-4 + 1e-3 |ref| against the float64 norm of the control tensor as stored on the
  device; backward seeds (the producer's linear terms) are scaled so that the reference gradient has unit peak;
- every case runs twice, bit for bit.
All slice counts are explicit, so no case depends on the CU count."""
import contextlib
import ctypes as C
import math
import os

import torch as th
import torch.nn.functional as F

from tests.parity_checks import DEV, _ctx, _flag, g, rec, unit_seed

NAN = float("nan")
EPS = 1e-5
SMALL_HW = 1024  # norm.hip gn_small_hw(): maps of up to this many pixels take the single-launch GroupNorm kernels

# ---- producers --------------------------------------------------------------------------------------------------------------------------
# ("conv", tile, Bn, H, W, Cin, Cout) | ("gemm", tile, M, N, K); the slice count belongs to the case.  Tile 64 is the implicit GEMM (the 8 x 12,
# 30 x 35 maps have no halo route: W is neither 8 nor a multiple of 16), 512 hconv2, 516 kconv, 513 the weight GEMM kernel.
IGEMM_CONV = ("conv", 64, 2, 8, 12, 32, 128)
IGEMM_CONV96 = ("conv", 64, 2, 8, 12, 32, 96)      # three channels per group: the scalar single-launch kernels
IGEMM_CONV_BIG = ("conv", 64, 2, 30, 35, 32, 64)   # 1050 pixels: just above the single-launch size, not a multiple of the chunk (8), B = 2
HCONV16 = ("conv", 512, 2, 16, 16, 96, 128)
HCONV32 = ("conv", 512, 1, 32, 32, 96, 128)
KCONV8 = ("conv", 516, 2, 8, 8, 128, 128)
KCONV16 = ("conv", 516, 1, 16, 16, 128, 128)
GEMM_STREAM = ("gemm", 64, 1024, 2048, 128)        # one 1024-pixel map x 2048 channels: the streaming single-launch kernels
GEMM_BIG = ("gemm", 513, 2100, 64, 320)            # B = 2 maps of 1050 pixels x 64 channels: the chunked kernels
GEMM_BIG64 = ("gemm", 64, 2100, 64, 320)           # the same on the implicit GEMM, which takes a residual at any stride and alignment
GEMM_LN9 = ("gemm", 64, 200, 512, 288)             # nine K tiles: nine slices of one tile each


def gemm_ln(tile, rows, Cc):
    return ("gemm", tile, rows, Cc, 320)


def prod_shape(p):
    """(rows, columns) of a producer's output"""
    return (p[2] * p[3] * p[4], p[6]) if p[0] == "conv" else (p[2], p[3])


def prod_cpu(p, seed=0):
    """CPU operands of a producer and the float64 value of its product term + bias (no residual), (rows, cols)"""
    if p[0] == "conv":
        _, _, Bn, H, W, Ci, Co = p
        x = th.randn(Bn, H, W, Ci, generator=g(5 + seed))
        w = th.randn(Co, Ci, 3, 3, generator=g(6 + seed)) / math.sqrt(9 * Ci)
        b = 0.3 * th.randn(Co, generator=g(7 + seed))
        ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(Bn * H * W, Co)
        return {"x": x, "w": w, "b": b, "alpha": 1.0}, ref
    _, _, M, N, K = p
    A = th.randn(M, K, generator=g(1 + seed))
    B = th.randn(N, K, generator=g(2 + seed))
    b = 0.3 * th.randn(N, generator=g(3 + seed))
    alpha = 1.0 / math.sqrt(K)  # != 1: the slices are scaled after they are summed
    return {"x": A, "w": B, "b": b, "alpha": alpha}, alpha * (A.double() @ B.double().T) + b.double()


def residual_cpu(p, seed=0, mean=0.0):
    M, N = prod_shape(p)
    return mean + 0.3 * th.randn(M, N, generator=g(17 + seed))


def _s():
    from cgd_amd import lib as L
    return L.stream_ptr()


def reduces(ctx):
    out = (C.c_uint64 * 2)()
    assert ctx.lib.cgd_launch_counts(out) == 0
    return int(out[1])


def pending(ctx):
    from cgd_amd import ops
    return ops.pending(ctx)


class Producer:
    """Device operands of one producer, its linear terms scaled by `scale` (a backward seed: dz = scale * (conv + bias + R))."""

    def __init__(self, ctx, p, cpu, scale=1.0):
        from cgd_amd import ops
        self.ctx, self.p = ctx, p
        self.M, self.N = prod_shape(p)
        self.x = cpu["x"].to(DEV)
        self.b = (cpu["b"] * scale).to(DEV)
        self.alpha = cpu["alpha"]
        if p[0] == "conv":
            w = cpu["w"] * scale
            self.w = ops.pack_conv3x3(w)[0].to(DEV)
            self.wfrag = ops.pack_conv3x3_frag(ctx, w.to(DEV)) if p[1] != 64 else None
        else:
            self.w = cpu["w"].to(DEV)
            self.alpha = cpu["alpha"] * scale

    def launch(self, c_ptr, ldc, sk, defer, r_ptr=None, ldr=0, bias_ptr=-1):
        ctx, lib, p = self.ctx, self.ctx.lib, self.p
        bias_ptr = self.b.data_ptr() if bias_ptr == -1 else bias_ptr
        if p[0] == "conv":
            _, tile, Bn, H, W, Ci, Co = p
            ctx.check(lib.cgd_op_conv3x3_ex(ctx.h, self.x.data_ptr(), Ci, self.w.data_ptr(), None if self.wfrag is None else self.wfrag.data_ptr(),
                                            c_ptr, ldc, bias_ptr, r_ptr, ldr, None, Bn, H, W, Ci, Co, 0, tile, sk, int(defer), 0, None, 0, None, _s()))
        else:
            _, tile, M, N, K = p
            ctx.check(lib.cgd_op_gemm_ex(ctx.h, self.x.data_ptr(), K, self.w.data_ptr(), K, c_ptr, ldc, bias_ptr, r_ptr, ldr, M, N, K, self.alpha,
                                         tile, sk, 0, int(defer), _s()))


class Out:
    """The producer's output: `rows` rows of `cols` floats at column `col` of a (rows, ld) buffer.  Pre-filled with NaN, or with the residual
    when the residual is accumulated in place; the columns beside the view hold finite filler a whole-buffer consumer can read."""

    def __init__(self, rows, cols, ld=None, col=0, fill=None):
        ld = ld or cols
        self.buf = th.full((rows, ld), 0.25, device=DEV)
        self.view = self.buf[:, col:col + cols]
        self.ld = ld
        if fill is None:
            self.view.fill_(NAN)
        else:
            self.view.copy_(fill)

    @property
    def ptr(self):
        return self.view.data_ptr()


def split_producer(P, out, sk, mode, r_dev, defer=1, ldr=None, r_ptr=None):
    """launch producer P into `out` and return the records that say whether it split and deferred.  mode: "bias" | "R" (separate residual
    r_dev) | "alias" (the residual is what `out` holds)."""
    ctx = P.ctx
    n0 = reduces(ctx)
    if mode == "alias":
        P.launch(out.ptr, out.ld, sk, defer, out.ptr, out.ld)
    elif mode == "R":
        P.launch(out.ptr, out.ld, sk, defer, r_dev.data_ptr() if r_ptr is None else r_ptr, ldr or r_dev.stride(0))
    else:
        P.launch(out.ptr, out.ld, sk, defer)
    q = pending(ctx)
    if defer:
        want = {"valid": 1, "slices": sk, "rows": P.M, "cols": P.N, "ldc": out.ld}
        return [_flag(f"producer split and deferred: pending {q}, wanted {want}; reduce launches {reduces(ctx) - n0}", q == want and reduces(ctx) == n0)]
    return [_flag(f"producer with defer = 0 reduced at once: pending {q}, reduce launches {reduces(ctx) - n0}", q["valid"] == 0 and reduces(ctx) == n0 + 1)]


def path_flag(ctx, name, n0, expect):
    """after a consumer: `take` = no reduce launch and nothing pending, `flush` = exactly one reduce launch and nothing pending"""
    q, dn = pending(ctx), reduces(ctx) - n0
    return _flag(f"{name}: {expect} (reduce launches {dn}, pending {q})", q["valid"] == 0 and dn == (0 if expect == "take" else 1))


# ---- float64 references of the consumers (the norm of the tensor as stored on the device) --------------------------------------------------
def gn_ref(x, gamma, beta, film, act, dz=None, add=None, dtype=th.float64):
    """GroupNorm(32) (+ FiLM) (+ SiLU) of x (B,HW,C): y, statistics [B][32][2] = (mean, rstd) and, with dz, the input gradient (+ add)"""
    B, HW, Cc = x.shape
    xr = x.to(dtype).requires_grad_()
    y = F.group_norm(xr.permute(0, 2, 1), 32, gamma.to(dtype), beta.to(dtype), EPS)
    if film is not None:
        y = y * (1 + film.to(dtype)[:, :Cc, None]) + film.to(dtype)[:, Cc:, None]
    if act:
        y = F.silu(y)
    y = y.permute(0, 2, 1)
    xg = x.to(dtype).reshape(B, HW, 32, Cc // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
    stats = th.stack([xg.mean(2), 1.0 / th.sqrt(xg.var(2, unbiased=False) + EPS)], dim=2)
    dx = None
    if dz is not None:
        (y * dz.to(dtype)).sum().backward()
        dx = xr.grad if add is None else xr.grad + add.to(dtype)
    return y.detach(), stats, dx


def ln_ref(x, gamma, beta, dy=None, dtype=th.float64):
    xr = x.to(dtype).requires_grad_()
    y = F.layer_norm(xr, (x.shape[1],), gamma.to(dtype), beta.to(dtype), EPS)
    stats = th.stack([xr.detach().mean(1), 1.0 / th.sqrt(xr.detach().var(1, unbiased=False) + EPS)], dim=1)
    dx = None
    if dy is not None:
        (y * dy.to(dtype)).sum().backward()
        dx = xr.grad
    return y.detach(), stats, dx


def norm_params(Cc, B, film, seed=0):
    gamma = 1 + 0.1 * th.randn(Cc, generator=g(21 + seed))
    beta = 0.1 * th.randn(Cc, generator=g(22 + seed))
    fl = 0.3 * th.randn(B, 2 * Cc, generator=g(23 + seed)) if film else None
    return gamma, beta, fl


def plain_x(rows, Cc, seed=0):
    """the forward input of a backward consumer (a finished tensor)"""
    return th.randn(rows, Cc, generator=g(20 + seed)) * 1.5 + 0.4


# ---- consumers ----------------------------------------------------------------------------------------------------------------------------
# ("gn_fwd", B, film, act, stats_only) | ("gn_bwd", B, act, add) | ("ln_fwd",) | ("ln_bwd",): rows and channels are the producer's
def gn_fwd_call(ctx, x_ptr, ldx, B, HW, Cc, gd, bd, fd, act, scr, y):
    ctx.check(ctx.lib.cgd_op_gn_fwd(ctx.h, x_ptr, ldx, None if y is None else y.data_ptr(), Cc, B, HW, Cc, gd.data_ptr(), bd.data_ptr(),
                                    None if fd is None else fd.data_ptr(), act, EPS, scr.data_ptr(), _s()))


def gn_stats(ctx, scr, B, HW, Cc):
    off = int(ctx.lib.cgd_op_gn_stats_offset(B, HW, Cc))
    return scr[off:off + B * 64].reshape(B, 32, 2).clone()


def gn_scratch(ctx, B, HW, Cc):
    return th.zeros(int(ctx.lib.cgd_op_gn_scratch_floats(B, HW, Cc)), device=DEV)


def gn_family(kind, HW, Cc, odd_stride=False):
    """the kernel family a GroupNorm forward / backward of HW pixels x Cc channels selects (norm.hip launch_gn_small_fwd / _bwd): float4 accesses
    need 4 | Cc / 32 and 4-float strides; the register-cached forms hold at most 8 (forward) / 4 (backward) vectors per thread of 1024"""
    if HW > SMALL_HW:
        return "chunked"
    cpg = Cc // 32
    if cpg % 4 or odd_stride:
        return "scalar"
    lg = max(0, (cpg // 4 - 1).bit_length())
    return "cached" if HW <= (8 if kind == "gn_fwd" else 4) * (1024 >> lg) else "streaming"


def gn_bwd_keeps_dz_in_registers(HW, Cc, odd_stride=False):
    """gn_small_bwd_kernel<.., CACHE = true> (float4 or scalar) sums the slices into registers and never writes dz ("register-resident: never
    written"), like ln_bwd_kernel with dy: nothing can be asserted about the buffer there"""
    if HW > SMALL_HW:
        return False
    cpg = Cc // 32
    cq = cpg if (cpg % 4 or odd_stride) else cpg // 4
    return HW <= 4 * (1024 >> max(0, (cq - 1).bit_length()))


class Case:
    def __init__(self, prod, sk, mode, cons, expect="take", ld=None, col=0, precision=1, r_ld_extra=0, r_off=0):
        self.prod, self.sk, self.mode, self.cons, self.expect = prod, sk, mode, cons, expect
        self.ld, self.col, self.precision, self.r_ld_extra, self.r_off = ld, col, precision, r_ld_extra, r_off

    @property
    def name(self):
        p = "x".join(str(v) for v in self.prod[1:])
        extra = (f" ld{self.ld}+{self.col}" if self.ld else "") + (f" ldr+{self.r_ld_extra}" if self.r_ld_extra else "") + (f" R+{self.r_off}" if self.r_off else "")
        return f"{self.prod[0]}{p} sk{self.sk} {self.mode}{extra} p{self.precision} -> {' '.join(str(v) for v in self.cons)} [{self.expect}]"


_GRADED = set()  # (producer, slices, mode, precision, scaled?) whose merged output was graded against float64 already


def case_refs(case):
    """CPU side of a case: the producer's operands, the backward seed scale and the float64 product term"""
    cpu, ref = prod_cpu(case.prod)
    M, N = prod_shape(case.prod)
    r = residual_cpu(case.prod) if case.mode != "bias" else None
    full = ref if r is None else ref + r.double()
    kind = case.cons[0]
    scale, xin, par = 1.0, None, None
    if kind in ("gn_fwd", "gn_bwd"):
        B = case.cons[1]
        par = norm_params(N, B, kind == "gn_fwd" and case.cons[2])
    else:
        par = norm_params(N, 1, False, seed=5)
    if kind == "gn_bwd":
        xin = plain_x(M, N)
        B = case.cons[1]
        _, _, dx = gn_ref(xin.reshape(B, M // B, N), par[0], par[1], None, case.cons[2], full.reshape(B, M // B, N))
        scale = unit_seed(dx)
    elif kind == "ln_bwd":
        xin = plain_x(M, N)
        _, _, dx = ln_ref(xin, par[0], par[1], full)
        scale = unit_seed(dx)
    return cpu, ref, r, full, scale, xin, par


def run_case(ctx, case):
    """one producer -> consumer case, twice (module docstring)"""
    out = []
    name = case.name
    cpu, ref, r, full, scale, xin, par = case_refs(case)
    P = Producer(ctx, case.prod, cpu, scale)
    M, N = P.M, P.N
    kind = case.cons[0]
    gd, bd = par[0].to(DEV), par[1].to(DEV)
    fd = None if par[2] is None else par[2].to(DEV)
    r_s = None if r is None else r * scale
    # the separate residual: dense, or at an odd row stride / one float into its allocation (the misaligned fallbacks)
    r_dev = r_ptr = None
    ldr = N + case.r_ld_extra
    if case.mode == "R":
        r_buf = th.zeros(M * ldr + case.r_off + 4, device=DEV)
        r_dev = r_buf[case.r_off:case.r_off + M * ldr].reshape(M, ldr)[:, :N]
        r_dev.copy_(r_s)
        r_ptr = r_dev.data_ptr()
    fill = r_s if case.mode == "alias" else None

    # control: the same producer with defer = 0 (the reduce launch runs inside the call)
    ctl = Out(M, N, case.ld, case.col, fill)
    out += split_producer(P, ctl, case.sk, case.mode, r_dev, defer=0, ldr=ldr, r_ptr=r_ptr)
    th.cuda.synchronize()
    x0 = ctl.view.clone()
    key = (case.prod, case.sk, case.mode, case.precision, scale != 1.0, case.r_ld_extra, case.r_off)
    if key not in _GRADED:
        _GRADED.add(key)
        out.append(rec(f"{name}: merged producer output vs float64", x0, full * scale))
    x0c = x0.cpu()
    add = None
    # float64 references on the tensor as stored
    if kind == "gn_fwd":
        _, B, film, act, stats_only = case.cons
        yref, sref, _ = gn_ref(x0c.reshape(B, M // B, N), gd.cpu(), bd.cpu(), None if fd is None else fd.cpu(), act)
    elif kind == "gn_bwd":
        _, B, act, with_add = case.cons
        add = 0.3 * th.randn(B, M // B, N, generator=g(25)) if with_add else None
        _, _, dxref = gn_ref(xin.reshape(B, M // B, N), gd.cpu(), bd.cpu(), None, act, x0c.reshape(B, M // B, N), add)
    elif kind == "ln_fwd":
        yref, sref, _ = ln_ref(x0c, gd.cpu(), bd.cpu())
    else:
        _, _, dxref = ln_ref(xin, gd.cpu(), bd.cpu(), x0c)
    first = None
    for k in range(2):
        o = Out(M, N, case.ld, case.col, fill)
        if case.mode == "R":
            r_dev.copy_(r_s)
        got = {}
        if kind == "gn_bwd":  # the norm's forward on the finished input first: its statistics and coefficients live in the scratch
            B = case.cons[1]
            xd, scr = xin.to(DEV), gn_scratch(ctx, B, M // B, N)
            gn_fwd_call(ctx, xd.data_ptr(), N, B, M // B, N, gd, bd, None, case.cons[2], scr, None)
        elif kind == "ln_bwd":
            xd, st, ytmp = xin.to(DEV), th.zeros(M, 2, device=DEV), th.empty(M, N, device=DEV)
            ctx.check(ctx.lib.cgd_op_ln_fwd(ctx.h, xd.data_ptr(), ytmp.data_ptr(), M, N, gd.data_ptr(), bd.data_ptr(), EPS, st.data_ptr(), _s()))
        out_k = split_producer(P, o, case.sk, case.mode, r_dev, defer=1, ldr=ldr, r_ptr=r_ptr)
        n0 = reduces(ctx)
        if kind == "gn_fwd":
            _, B, film, act, stats_only = case.cons
            HW = M // B
            scr = gn_scratch(ctx, B, HW, N)
            y = None if stats_only else th.full((B, HW, N), NAN, device=DEV)
            gn_fwd_call(ctx, o.ptr, o.ld, B, HW, N, gd, bd, fd, act, scr, y)
            got["stats"] = gn_stats(ctx, scr, B, HW, N)
            if y is not None:
                got["y"] = y
        elif kind == "gn_bwd":
            _, B, act, with_add = case.cons
            HW = M // B
            dx = th.full((B, HW, N), NAN, device=DEV)
            ad = None if add is None else add.to(DEV)
            ctx.check(ctx.lib.cgd_op_gn_bwd(ctx.h, xd.data_ptr(), N, o.ptr, o.ld, dx.data_ptr(), N, None if ad is None else ad.data_ptr(), N,
                                            B, HW, N, act, scr.data_ptr(), _s()))
            got["dx"] = dx
        elif kind == "ln_fwd":
            assert o.ld == N
            y, st = th.full((M, N), NAN, device=DEV), th.full((M, 2), NAN, device=DEV)
            ctx.check(ctx.lib.cgd_op_ln_fwd(ctx.h, o.ptr, y.data_ptr(), M, N, gd.data_ptr(), bd.data_ptr(), EPS, st.data_ptr(), _s()))
            got["y"], got["stats"] = y, st
        else:
            assert o.ld == N
            dx = th.full((M, N), NAN, device=DEV)
            ctx.check(ctx.lib.cgd_op_ln_bwd(ctx.h, xd.data_ptr(), o.ptr, dx.data_ptr(), M, N, gd.data_ptr(), st.data_ptr(), _s()))
            got["dx"] = dx
        out_k.append(path_flag(ctx, name, n0, case.expect))
        th.cuda.synchronize()
        # ln_bwd sums dy for itself and never writes it back, and so does the register-cached single-launch GroupNorm backward with dz: nothing
        # is asserted about the buffer there (a reduce launch always writes it)
        silent = kind == "ln_bwd" or (kind == "gn_bwd" and gn_bwd_keeps_dz_in_registers(M // case.cons[1], N, bool(case.r_ld_extra)))
        if case.expect == "flush" or not silent:
            got["x"] = o.view.clone()
        if k == 0:
            out += out_k
            if "x" in got:
                nd = int((got["x"].view(th.int32) != x0.view(th.int32)).sum())
                worst = float((got["x"].double() - x0.double()).abs().max()) if not bool(th.isnan(got["x"]).any()) else NAN
                out.append(_flag(f"{name}: the tensor written back equals the defer = 0 output bit for bit ({nd} of {x0.numel()} words differ, "
                                 f"largest difference {worst:.3e})", th.equal(got["x"], x0)))
            if "y" in got:
                out.append(rec(f"{name}: y", got["y"], yref.reshape(got["y"].shape)))
            if "stats" in got:
                out.append(rec(f"{name}: statistics (mean, rstd)", got["stats"], sref.reshape(got["stats"].shape)))
            if "dx" in got:
                out.append(rec(f"{name}: dx (unit peak)", got["dx"], dxref.reshape(got["dx"].shape)))
            first = got
        else:
            out.append(_flag(f"{name}: the rerun took the same path", all(r_["ok"] for r_ in out_k)))
            out.append(_flag(f"{name}: the rerun is bit-identical",
                             all(th.equal(first[n_].view(th.int32), got[n_].view(th.int32)) for n_ in first)))
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
GN_F = ("gn_fwd", 2, False, 1, False)


def producer_cases():
    """every producer x slice count x residual mode into the GroupNorm forward its map selects (precision 1; the implicit GEMM at precision 0 too)"""
    cs = []
    for mode in ("bias", "R", "alias"):
        for prec in (1, 0):
            for sk in (2, 3, 9):
                cs.append(Case(IGEMM_CONV, sk, mode, GN_F, precision=prec))
        for p, B in ((HCONV16, 2), (HCONV32, 1)):
            for sk in (2, 3):
                cs.append(Case(p, sk, mode, ("gn_fwd", B, False, 1, False)))
        for p, B in ((KCONV8, 2), (KCONV16, 1)):
            for sk in (2, 4):
                cs.append(Case(p, sk, mode, ("gn_fwd", B, False, 1, False)))
        for tile, rows, sk in ((513, 120, 2), (513, 120, 5), (64, 36, 4)):
            cs.append(Case(gemm_ln(tile, rows, 512), sk, mode, ("ln_fwd",)))
    return cs


def gn_cases():
    """GroupNorm forward and backward: the register-cached, streaming, scalar and chunked kernels, FiLM, both activations, statistics only"""
    cs = []
    for mode in ("bias", "alias"):
        cs += [Case(IGEMM_CONV, 3, mode, ("gn_fwd", 2, True, 1, False)),        # cached, FiLM
               Case(IGEMM_CONV, 9, mode, ("gn_fwd", 2, False, 0, False)),       # cached, act 0, the second batch of eight slice loads
               Case(IGEMM_CONV, 2, mode, ("gn_fwd", 2, False, 1, True)),        # statistics only
               Case(IGEMM_CONV96, 3, mode, ("gn_fwd", 2, True, 1, False)),      # scalar
               Case(IGEMM_CONV96, 9, mode, ("gn_fwd", 2, False, 0, True)),
               Case(GEMM_STREAM, 4, mode, ("gn_fwd", 1, True, 1, False)),       # streaming
               Case(GEMM_STREAM, 4, mode, ("gn_fwd", 1, False, 0, True)),
               Case(IGEMM_CONV_BIG, 3, mode, ("gn_fwd", 2, True, 1, False)),    # chunked
               Case(IGEMM_CONV_BIG, 9, mode, ("gn_fwd", 2, False, 0, False)),
               Case(GEMM_BIG, 5, mode, ("gn_fwd", 2, False, 1, True)),
               # backward: dz in slices
               Case(IGEMM_CONV, 9, mode, ("gn_bwd", 2, 1, True)),
               Case(IGEMM_CONV, 2, mode, ("gn_bwd", 2, 0, False)),
               Case(IGEMM_CONV96, 3, mode, ("gn_bwd", 2, 1, False)),
               Case(IGEMM_CONV96, 9, mode, ("gn_bwd", 2, 0, True)),
               Case(GEMM_STREAM, 4, mode, ("gn_bwd", 1, 1, True)),
               Case(IGEMM_CONV_BIG, 3, mode, ("gn_bwd", 2, 1, True)),
               Case(GEMM_BIG, 5, mode, ("gn_bwd", 2, 0, False))]
    cs.append(Case(KCONV16, 4, "R", ("gn_bwd", 1, 1, True)))
    cs.append(Case(HCONV32, 3, "R", ("gn_bwd", 1, 1, False)))
    return cs


def ln_cases():
    """LayerNorm forward and backward at the four vector widths x rows 7 / 50 / 200 (row blocks of 4, ragged last one); C = 520 runs the generic
    kernel, which takes no slices"""
    cs = []
    for Cc in (256, 512, 768, 1024):
        for rows, tile, sk, mode in ((7, 64, 4, "alias"), (50, 64, 4, "R"), (200, 513, 5, "bias"), (200, 513, 2, "alias")):
            for kind in ("ln_fwd", "ln_bwd"):
                cs.append(Case(gemm_ln(tile, rows, Cc), sk, mode, (kind,)))
    cs.append(Case(GEMM_LN9, 9, "R", ("ln_fwd",)))
    cs.append(Case(GEMM_LN9, 9, "R", ("ln_bwd",)))
    for kind in ("ln_fwd", "ln_bwd"):
        cs.append(Case(gemm_ln(64, 50, 520), 4, "R", (kind,), expect="flush"))
    return cs


def fallback_cases():
    """a residual at a row stride that is no multiple of 4, or one float into its allocation: the chunked GroupNorms and the LayerNorms read
    float4 only, re-arm the entry and finish the reduction the plain way; the single-launch GroupNorm takes the slices on its scalar kernel"""
    cs = []
    for extra, off in ((1, 0), (0, 1)):
        cs += [Case(GEMM_BIG64, 5, "R", ("gn_fwd", 2, False, 1, False), expect="flush", r_ld_extra=extra, r_off=off),
               Case(GEMM_BIG64, 5, "R", ("gn_bwd", 2, 1, False), expect="flush", r_ld_extra=extra, r_off=off),
               Case(gemm_ln(64, 50, 512), 4, "R", ("ln_fwd",), expect="flush", r_ld_extra=extra, r_off=off),
               Case(gemm_ln(64, 50, 512), 4, "R", ("ln_bwd",), expect="flush", r_ld_extra=extra, r_off=off)]
    cs.append(Case(IGEMM_CONV, 3, "R", GN_F, expect="take", r_ld_extra=1))
    cs.append(Case(IGEMM_CONV, 3, "R", ("gn_bwd", 2, 1, False), expect="take", r_ld_extra=1))
    return cs


def concat_cases():
    """the producer writes a channel slice of a wider buffer (ldc > N); the GroupNorm over that slice takes the slices"""
    return [Case(IGEMM_CONV, 3, "bias", GN_F, ld=320, col=64),
            Case(KCONV16, 2, "alias", ("gn_fwd", 1, True, 1, False), ld=192, col=64),
            Case(IGEMM_CONV_BIG, 3, "R", ("gn_fwd", 2, False, 1, False), ld=96, col=32),
            Case(IGEMM_CONV_BIG, 3, "bias", ("gn_bwd", 2, 1, True), ld=96, col=32)]


GROUPS = {"producers": producer_cases, "groupnorm": gn_cases, "layernorm": ln_cases, "fallbacks": fallback_cases, "concat": concat_cases}


def all_cases():
    return [c for fn in GROUPS.values() for c in fn()]


_CTX = {}


def shared_ctx(precision):
    if precision not in _CTX:
        _CTX[precision] = _ctx(precision)
    return _CTX[precision]


def check_group(group):
    out = []
    for case in GROUPS[group]():
        out += run_case(shared_ctx(case.precision), case)
    return out


# ---- stale state ---------------------------------------------------------------------------------------------------------------------------
class Setup:
    """a deferred igemm conv (B2 8x12, 32 -> 128, 3 slices, bias + separate R) and the GroupNorm forward over its output: the fixture of the
    stale-state cases.  `produce(out, defer)`, `consume(x_ptr, ldx, B, HW, C)` -> (y, stats), and the control tensor / outputs."""

    def __init__(self, ctx, prod=IGEMM_CONV, sk=3, B=2, seed=0):
        self.ctx, self.prod, self.sk, self.B = ctx, prod, sk, B
        cpu, ref = prod_cpu(prod, seed)
        self.P = Producer(ctx, prod, cpu)
        self.M, self.N = self.P.M, self.P.N
        r = residual_cpu(prod, seed)
        self.full = ref + r.double()
        self.r = r.to(DEV)
        gm, bt, _ = norm_params(self.N, B, False)
        self.gamma, self.beta = gm, bt
        self.gd, self.bd = gm.to(DEV), bt.to(DEV)
        ctl = Out(self.M, self.N)
        self.produce(ctl, 0)
        th.cuda.synchronize()
        self.x0 = ctl.view.clone()
        self.y0, self.s0 = self.consume(ctl.ptr, self.N, B, self.M // B, self.N)
        th.cuda.synchronize()

    def produce(self, out, defer=1):
        return split_producer(self.P, out, self.sk, "R", self.r, defer=defer)

    def consume(self, x_ptr, ldx, B, HW, Cc, gd=None, bd=None):
        scr = gn_scratch(self.ctx, B, HW, Cc)
        y = th.full((B, HW, Cc), NAN, device=DEV)
        gn_fwd_call(self.ctx, x_ptr, ldx, B, HW, Cc, gd if gd is not None else self.gd, bd if bd is not None else self.bd, None, 1, scr, y)
        return y, gn_stats(self.ctx, scr, B, HW, Cc)

    def grade(self, name, y, x_stored, B=None, gamma=None, beta=None):
        B = B or self.B
        xs = x_stored.cpu()
        yref, _, _ = gn_ref(xs.reshape(B, -1, xs.shape[-1]), self.gamma if gamma is None else gamma, self.beta if beta is None else beta, None, 1)
        return rec(name, y, yref)


def check_mismatch():
    """a consumer that differs from the pending entry in exactly one of pointer, rows, columns or row stride must flush (the stream: check_second_stream)"""
    ctx = shared_ctx(1)
    S = Setup(ctx)
    M, N, B = S.M, S.N, S.B
    HW = M // B
    out = [S.grade("mismatch: control y", S.y0, S.x0)]
    # pointer: the norm of ANOTHER finished tensor of the same shape
    o = Out(M, N)
    other = (0.7 + 1.3 * th.randn(M, N, generator=g(90))).to(DEV)
    out += S.produce(o)
    n0 = reduces(ctx)
    y, _ = S.consume(other.data_ptr(), N, B, HW, N)
    out.append(path_flag(ctx, "mismatch in the pointer", n0, "flush"))
    th.cuda.synchronize()
    out += [_flag("mismatch in the pointer: the pending tensor was reduced", th.equal(o.view, S.x0)), S.grade("mismatch in the pointer: y of the other tensor", y, other)]
    # rows: the first sample only
    o = Out(M, N)
    out += S.produce(o)
    n0 = reduces(ctx)
    y, _ = S.consume(o.ptr, N, 1, HW, N)
    out.append(path_flag(ctx, "mismatch in the rows", n0, "flush"))
    th.cuda.synchronize()
    out += [_flag("mismatch in the rows: tensor reduced", th.equal(o.view, S.x0)), S.grade("mismatch in the rows: y", y, S.x0[:HW], B=1),
            _flag("mismatch in the rows: equal to the control's first sample", th.equal(y[0], S.y0[0]))]
    # columns: the first 64 channels at the same row stride
    o = Out(M, N)
    out += S.produce(o)
    n0 = reduces(ctx)
    y, _ = S.consume(o.ptr, N, B, HW, 64, S.gd[:64].contiguous(), S.bd[:64].contiguous())
    out.append(path_flag(ctx, "mismatch in the columns", n0, "flush"))
    th.cuda.synchronize()
    out += [_flag("mismatch in the columns: tensor reduced", th.equal(o.view, S.x0)),
            S.grade("mismatch in the columns: y", y, S.x0[:, :64], gamma=S.gamma[:64], beta=S.beta[:64])]
    # row stride: the producer writes the left half of a (M, 2N) buffer; the consumer reads M rows of N floats densely from the same pointer
    o = Out(M, N, 2 * N, 0)
    o.buf[:, N:] = (0.5 * th.randn(M, N, generator=g(91)) - 0.2).to(DEV)
    ctl = Out(M, N, 2 * N, 0)
    ctl.buf[:, N:] = o.buf[:, N:]
    out += S.produce(ctl, 0)
    out += S.produce(o)
    n0 = reduces(ctx)
    y, _ = S.consume(o.ptr, N, B, HW, N)
    out.append(path_flag(ctx, "mismatch in the row stride", n0, "flush"))
    th.cuda.synchronize()
    out += [_flag("mismatch in the row stride: tensor reduced", th.equal(o.buf, ctl.buf)),
            S.grade("mismatch in the row stride: y of the dense reading", y, ctl.buf.reshape(2 * M, N)[:M])]
    return out


def check_concat_whole():
    """the producer writes channels [64, 192) of a 320-wide concat buffer; the GroupNorm over the WHOLE buffer does not match the entry (pointer,
    columns) and must flush; its result is the norm of the finished buffer"""
    ctx = shared_ctx(1)
    S = Setup(ctx)
    M, N, B, ld = S.M, S.N, S.B, 320
    side = (0.6 * th.randn(M, ld, generator=g(92)) + 0.1).to(DEV)
    gm, bt, _ = norm_params(ld, B, False, seed=3)
    out = []
    bufs = []
    for defer in (0, 1):
        o = Out(M, N, ld, 64)
        o.buf[:, :64], o.buf[:, 192:] = side[:, :64], side[:, 192:]
        out += S.produce(o, defer)
        n0 = reduces(ctx)
        y, st = S.consume(o.buf.data_ptr(), ld, B, M // B, ld, gm.to(DEV), bt.to(DEV))
        out.append(path_flag(ctx, f"GroupNorm over the whole concat buffer (defer = {defer})", n0, "flush" if defer else "take"))  # defer = 0: plain, no launch
        th.cuda.synchronize()
        bufs.append((o.buf.clone(), y, st))
    out += [_flag("whole concat: the slice was reduced into the buffer", th.equal(bufs[0][0], bufs[1][0]) and th.equal(bufs[1][0][:, 64:192], S.x0)),
            _flag("whole concat: outputs equal the defer = 0 control", th.equal(bufs[0][1], bufs[1][1]) and th.equal(bufs[0][2], bufs[1][2])),
            S.grade("whole concat: y", bufs[1][1], bufs[1][0], gamma=gm, beta=bt)]
    return out


def check_gemm_between():
    """another GEMM between producer and consumer: the first tensor comes out finished and the consumer runs on a plain tensor; two deferred
    producers back to back: the first is reduced by the second's launch, the second is taken"""
    from cgd_amd import ops
    ctx = shared_ctx(1)
    S = Setup(ctx)
    S2 = Setup(ctx, prod=KCONV8, sk=2, seed=40)
    out = []
    o = Out(S.M, S.N)
    out += S.produce(o)
    n0 = reduces(ctx)
    A, Bm = th.randn(70, 64, generator=g(1)), th.randn(96, 64, generator=g(2))
    cg = ops.gemm(ctx, A.to(DEV), Bm.to(DEV), force_tile=64, splitk=-1)  # one slice: no reduce launch of its own
    out.append(path_flag(ctx, "a plain GEMM behind a deferred producer", n0, "flush"))
    y, st = S.consume(o.ptr, S.N, S.B, S.M // S.B, S.N)
    out.append(_flag("the consumer behind it ran on a plain tensor (no further reduce launch)", reduces(ctx) == n0 + 1))
    th.cuda.synchronize()
    out += [rec("the GEMM in between", cg, A.double() @ Bm.double().T), _flag("first tensor finished", th.equal(o.view, S.x0)),
            _flag("consumer output equals the control", th.equal(y, S.y0) and th.equal(st, S.s0))]
    o1, o2 = Out(S.M, S.N), Out(S2.M, S2.N)
    out += S.produce(o1)
    n0 = reduces(ctx)
    S2.P.launch(o2.ptr, o2.ld, S2.sk, 1, S2.r.data_ptr(), S2.N)
    q = pending(ctx)
    out.append(_flag(f"a second deferred producer reduced the first and is pending itself ({q}, reduce launches {reduces(ctx) - n0})",
                     reduces(ctx) == n0 + 1 and q == {"valid": 1, "slices": S2.sk, "rows": S2.M, "cols": S2.N, "ldc": S2.N}))
    n0 = reduces(ctx)
    y2, _ = S2.consume(o2.ptr, S2.N, S2.B, S2.M // S2.B, S2.N)
    out.append(path_flag(ctx, "the second producer's consumer", n0, "take"))
    y1, _ = S.consume(o1.ptr, S.N, S.B, S.M // S.B, S.N)
    th.cuda.synchronize()
    out += [_flag("back to back: first tensor finished", th.equal(o1.view, S.x0)), _flag("back to back: second tensor written back", th.equal(o2.view, S2.x0)),
            _flag("back to back: the first consumer (plain tensor) equals its control", th.equal(y1, S.y0)),
            S2.grade("back to back: y of the second", y2, S2.x0)]
    return out


def check_refused_consumer():
    """a GroupNorm over 48 channels is refused before it looks at the pending entry: status -2, nothing written, the entry still pending, and the
    matching consumer afterwards takes the slices"""
    from cgd_amd.lib import CgdError
    ctx = shared_ctx(1)
    S = Setup(ctx)
    o = Out(S.M, S.N)
    out = S.produce(o)
    n0 = reduces(ctx)
    before = pending(ctx)
    y = th.full((S.B, S.M // S.B, 48), NAN, device=DEV)
    scr = th.full((4096,), NAN, device=DEV)
    rc = ctx.lib.cgd_op_gn_fwd(ctx.h, o.ptr, S.N, y.data_ptr(), 48, S.B, S.M // S.B, 48, S.gd.data_ptr(), S.bd.data_ptr(), None, 1, EPS, scr.data_ptr(), _s())
    th.cuda.synchronize()
    try:
        ctx.check(rc)
        msg = "(no error)"
    except CgdError as e:
        msg = str(e)
    out += [_flag(f"C = 48 refused with status -2 (got {rc}: {msg})", rc == -2 and "multiple of 32" in msg),
            _flag("the refusal wrote nothing (y, scratch and the producer's output still NaN)",
                  bool(th.isnan(y).all()) and bool(th.isnan(scr).all()) and bool(th.isnan(o.view).all())),
            _flag(f"the entry is still pending ({pending(ctx)}) and no reduce launch ran", pending(ctx) == before and before["valid"] == 1 and reduces(ctx) == n0)]
    y, st = S.consume(o.ptr, S.N, S.B, S.M // S.B, S.N)
    out.append(path_flag(ctx, "the matching consumer after the refusal", n0, "take"))
    th.cuda.synchronize()
    out += [_flag("after the refusal: tensor written back", th.equal(o.view, S.x0)), S.grade("after the refusal: y", y, S.x0)]
    return out


def check_state_changes():
    """a pending entry across cgd_op_new_pass and across cgd_set_precision.  Reading the code: cgd_op_new_pass only advances the serial of the
    conv-epilogue records and cgd_set_precision only stores the mode, so the entry MUST survive both and the matching consumer must still take
    it; either way the tensor is never left unreduced and the reader gets the finished values."""
    ctx = shared_ctx(1)
    S = Setup(ctx)
    out = []
    for what, change, undo in (("cgd_op_new_pass", lambda: ctx.check(ctx.lib.cgd_op_new_pass(ctx.h)), None),
                               ("cgd_set_precision(0)", lambda: ctx.set_precision(0), lambda: ctx.set_precision(1))):
        o = Out(S.M, S.N)
        out += S.produce(o)
        before = pending(ctx)
        n0 = reduces(ctx)
        change()
        out.append(_flag(f"{what}: the entry survives ({pending(ctx)}), no reduce launch", pending(ctx) == before and reduces(ctx) == n0))
        y, st = S.consume(o.ptr, S.N, S.B, S.M // S.B, S.N)
        out.append(path_flag(ctx, f"the matching consumer after {what}", n0, "take"))
        th.cuda.synchronize()
        if undo:
            undo()
        out += [_flag(f"{what}: tensor written back, not left unreduced", th.equal(o.view, S.x0)), S.grade(f"{what}: y", y, S.x0)]
        # ... and a reader that takes no slices after the same change gets the finished tensor
        o = Out(S.M, S.N)
        out += S.produce(o)
        n0 = reduces(ctx)
        change()
        a = th.full((S.M, S.N), NAN, device=DEV)
        ctx.check(ctx.lib.cgd_op_act(ctx.h, o.ptr, None, a.data_ptr(), S.M * S.N, 1, _s()))
        out.append(path_flag(ctx, f"an activation after {what}", n0, "flush"))
        th.cuda.synchronize()
        if undo:
            undo()
        out.append(rec(f"{what}: SiLU of the finished tensor", a, F.silu(S.x0.double().cpu())))
    return out


def check_second_stream():
    """the producer runs on its own stream behind a delay; the consumer on a second stream does not match (stream), so the reduction runs on
    the PRODUCER's stream and the consumer is ordered behind it with an event (gemm.hip cgd_flush_pending): equal to the one-stream control"""
    from tests.stream_checks import enqueue_delay
    ctx = shared_ctx(1)
    S = Setup(ctx)
    th.cuda.synchronize()
    s1, s2 = th.cuda.Stream(), th.cuda.Stream()
    o = Out(S.M, S.N)
    x_true = S.P.x.clone()
    th.cuda.synchronize()
    out = []
    with th.cuda.stream(s1):
        S.P.x.fill_(NAN)  # the producer's input arrives only behind the delay
        enqueue_delay()
        S.P.x.copy_(x_true)
        armed = th.cuda.Event()
        armed.record(s1)
        out += S.produce(o)
    with th.cuda.stream(s2):
        n0 = reduces(ctx)
        y, st = S.consume(o.ptr, S.N, S.B, S.M // S.B, S.N)
        early = not armed.query()
        out.append(path_flag(ctx, "consumer on a second stream", n0, "flush"))
        s2.synchronize()  # the only synchronisation: s2 must have waited for the producer's stream
    out += [_flag("second stream: the consumer's result equals the one-stream control", th.equal(y, S.y0) and th.equal(st, S.s0)),
            _flag("second stream: the tensor was reduced", th.equal(o.view, S.x0))]
    out.append(dict(_flag(f"second stream: the call returned while the delay was still running (reported, not asserted: {early})", True)))
    th.cuda.synchronize()
    return out


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def check_defer_modes():
    """CGD_DEFER = 0 and 1 in fresh contexts.  At 0 every producer reduces at once although it asked to defer; at 1 the single-launch GroupNorm
    flushes and the chunked one takes.  Both show that the counter and cgd_op_pending tell the paths apart."""
    out = []
    for mode in ("0", "1"):
        with _env("CGD_DEFER", mode):
            ctx = _ctx(1)
        for prod, B in ((IGEMM_CONV, 2), (IGEMM_CONV_BIG, 2)):
            S = Setup(ctx, prod=prod, B=B)
            o = Out(S.M, S.N)
            n0 = reduces(ctx)
            S.P.launch(o.ptr, o.ld, S.sk, 1, S.r.data_ptr(), S.N)
            q, dn = pending(ctx), reduces(ctx) - n0
            tag = f"CGD_DEFER={mode} {'chunked' if S.M // B > SMALL_HW else 'single-launch'} map"
            if mode == "0":
                out.append(_flag(f"{tag}: the producer reduced at once (pending {q}, reduce launches {dn})", q["valid"] == 0 and dn == 1))
            else:
                out.append(_flag(f"{tag}: the producer deferred (pending {q}, reduce launches {dn})", q["valid"] == 1 and q["slices"] == S.sk and dn == 0))
            n0 = reduces(ctx)
            y, st = S.consume(o.ptr, S.N, B, S.M // B, S.N)
            if mode == "0":
                out.append(_flag(f"{tag}: the consumer found a plain tensor", reduces(ctx) == n0 and pending(ctx)["valid"] == 0))
            else:
                out.append(path_flag(ctx, f"{tag}: consumer", n0, "take" if S.M // B > SMALL_HW else "flush"))
            th.cuda.synchronize()
            out += [_flag(f"{tag}: tensor finished", th.equal(o.view, S.x0)), S.grade(f"{tag}: y", y, S.x0)]
            if not (mode == "1" and S.M // B > SMALL_HW):  # a consumer of a plain tensor runs the control's kernels on the control's bits
                out.append(_flag(f"{tag}: outputs equal the control", th.equal(y, S.y0) and th.equal(st, S.s0)))
        ctx.close()
    return out


def check_other_readers():
    """every other cgd_op_* entry that reads a device operand, on a tensor whose reduction is pending: each must return the result for the
    finished tensor (th.equal to the same call on the control) after exactly one reduce launch"""
    from cgd_amd import ops
    ctx = shared_ctx(1)
    lib = ctx.lib
    out = []
    S = Setup(ctx, prod=KCONV16, sk=2, B=1)  # (1, 16, 16, 128) NHWC = 256 rows x 128; attention reads its first 64 x 384 floats as qkv of 2 heads x 64
    Bn, H, W, Cc = 1, 16, 16, 128
    w3 = th.randn(64, Cc, 3, 3, generator=g(60)) / math.sqrt(9 * Cc)
    w3p = ops.pack_conv3x3(w3)[0].to(DEV)
    wt = th.randn(3, Cc, 3, 3, generator=g(61)) / math.sqrt(9 * Cc)
    wtp, bt = ops.pack_conv3x3(wt)[0].to(DEV), (0.1 * th.randn(3, generator=g(62))).to(DEV)
    att = ops.Attention(ctx, 1, 2, 64, 64, 0, DEV)
    gm, bb = (1 + 0.1 * th.randn(512, generator=g(63))).to(DEV), (0.1 * th.randn(512, generator=g(64))).to(DEV)

    def readers(x):  # x: the (256, 128) tensor, pending or finished
        px = x.data_ptr()

        def pool():
            y = th.full((Bn, H // 2, W // 2, Cc), NAN, device=DEV)
            ctx.check(lib.cgd_op_pool2x2(ctx.h, px, y.data_ptr(), Bn, H // 2, W // 2, Cc, 0.25, _s()))
            return y

        def ups():
            y = th.full((Bn, 2 * H, 2 * W, Cc), NAN, device=DEV)
            ctx.check(lib.cgd_op_upsample2x(ctx.h, px, y.data_ptr(), Bn, 2 * H, 2 * W, Cc, 1.0, _s()))
            return y

        def act():
            y = th.full((H * W, Cc), NAN, device=DEV)
            ctx.check(lib.cgd_op_act(ctx.h, px, None, y.data_ptr(), H * W * Cc, 1, _s()))
            return y

        def attn():
            y = th.full((64, 128), NAN, device=DEV)
            ctx.check(lib.cgd_op_attn_fwd(ctx.h, px, y.data_ptr(), 1, 2, 64, 64, 0, att._arr, _s()))
            return y

        def conv():
            y = th.full((Bn, H, W, 64), NAN, device=DEV)
            ctx.check(lib.cgd_op_conv3x3(ctx.h, px, Cc, w3p.data_ptr(), None, y.data_ptr(), 64, None, None, 0, Bn, H, W, Cc, 64, 0, 64, 1, _s()))
            return y

        def thin():
            y = th.full((Bn, 3, H, W), NAN, device=DEV)
            ctx.check(lib.cgd_op_conv_thin_out(ctx.h, px, Cc, wtp.data_ptr(), bt.data_ptr(), y.data_ptr(), Bn, H, W, Cc, 3, _s()))
            return y

        def gram():
            y = th.full((1, Cc, Cc), NAN, device=DEV)
            ctx.check(lib.cgd_op_gram(ctx.h, px, Cc, 1, H * W, Cc, 1.0 / (H * W), y.data_ptr(), _s()))
            return y

        def ln_generic():  # 64 rows x 512 with a gamma one float into its allocation: cgd_launch_ln_fwd takes the generic kernel
            y, st = th.full((64, 512), NAN, device=DEV), th.full((64, 2), NAN, device=DEV)
            ctx.check(lib.cgd_op_ln_fwd(ctx.h, px, y.data_ptr(), 64, 512, gm1.data_ptr(), bb.data_ptr(), EPS, st.data_ptr(), _s()))
            return y

        return {"pool2x2": pool, "upsample2x": ups, "act": act, "attention forward": attn, "conv3x3 (input)": conv, "conv_thin_out": thin, "gram": gram,
                "ln on the generic kernel": ln_generic}

    gm_buf = th.zeros(516, device=DEV)
    gm1 = gm_buf[1:513]  # one float into its allocation: cgd_launch_ln_fwd takes the generic kernel (no float4 loads of gamma)
    gm1.copy_(gm)
    ctl = Out(S.M, S.N)
    S.produce(ctl, 0)
    th.cuda.synchronize()
    want, own = {}, {}  # the result on the finished tensor and the reduce launches the entry runs for itself (an auto-split GEMM inside it)
    for k, f in readers(ctl.view).items():
        n0 = reduces(ctx)
        want[k] = f()
        own[k] = reduces(ctx) - n0
    th.cuda.synchronize()
    xs = S.x0.double().cpu()
    x4 = xs.reshape(Bn, H, W, Cc).permute(0, 3, 1, 2)
    refs = {"pool2x2": F.avg_pool2d(x4, 2).permute(0, 2, 3, 1), "upsample2x": F.interpolate(x4, scale_factor=2, mode="nearest").permute(0, 2, 3, 1),
            "act": F.silu(xs), "conv3x3 (input)": F.conv2d(x4, w3.double(), None, padding=1).permute(0, 2, 3, 1),
            "conv_thin_out": F.conv2d(x4, wt.double(), bt.double().cpu(), padding=1), "gram": (xs.T @ xs / (H * W))[None],
            "ln on the generic kernel": F.layer_norm(xs.reshape(64, 512), (512,), gm.double().cpu(), bb.double().cpu(), EPS)}
    q3 = xs.reshape(-1)[:64 * 384].reshape(64, 3, 2, 64)  # the first 64 x 384 floats of the tensor, read as token-major [Q | K | V] rows
    qq, kk, vv = (q3[:, i].permute(1, 0, 2) for i in range(3))
    refs["attention forward"] = (th.softmax(qq @ kk.transpose(1, 2) / 8.0, dim=-1) @ vv).permute(1, 0, 2).reshape(64, 128)
    for k in want:
        out.append(rec(f"other readers: {k} on the finished tensor vs float64", want[k], refs[k].reshape(want[k].shape)))
        o = Out(S.M, S.N)
        out += S.produce(o)
        n0 = reduces(ctx)
        got = readers(o.view)[k]()
        dn, q = reduces(ctx) - n0, pending(ctx)
        out.append(_flag(f"other readers: {k} flushed first (reduce launches {dn}, {own[k]} of them its own; pending {q})", dn == own[k] + 1 and q["valid"] == 0))
        th.cuda.synchronize()
        out += [_flag(f"other readers: {k} returns the finished tensor's result", th.equal(got, want[k])),
                _flag(f"other readers: {k} left the tensor reduced", th.equal(o.view, S.x0))]
    return out


# ---- value regime: the residual carries the mean -------------------------------------------------------------------------------------------
LADDER = (3, 10, 30, 100)  # |mean| / sigma arriving through R
REGIME_PRODS = {"cached": (IGEMM_CONV, 3, 2), "chunked": (IGEMM_CONV_BIG, 3, 2)}
ADMISSIBLE_FRACTION = 0.25


def regime_tensor(prod, m):
    """the merged float64 tensor of the regime case: a unit-variance conv term (bias folded in) + R = m + noise"""
    cpu, ref = prod_cpu(prod)
    r = residual_cpu(prod, mean=float(m))
    return cpu, ref, r, ref + r.double()


def bound_fraction(got, ref):
    """largest |got - ref| / (1e-4 + 1e-3 |ref|) over the elements: 1 is the bound of `rec`"""
    got, ref = got.double(), ref.double()
    return float(((got - ref).abs() / (1e-4 + 1e-3 * ref.abs())).max())


def admissible(prod, B, m):
    """the project's rule: a magnitude is admissible where fp32 F.group_norm on the merged tensor stays within 0.25 of the bound against float64.
    Returns (fraction of y, fraction of the statistics)."""
    _, _, _, full = regime_tensor(prod, m)
    M, N = prod_shape(prod)
    gm, bt, _ = norm_params(N, B, False)
    x = full.float().reshape(B, M // B, N)  # the tensor as a device would store it
    y64, s64, _ = gn_ref(x, gm, bt, None, 1)
    y32, s32, _ = gn_ref(x, gm, bt, None, 1, dtype=th.float32)
    return bound_fraction(y32, y64), bound_fraction(s32, s64)


def check_mean_through_R(path):
    """GroupNorm forward (cached / chunked) on slices whose mean arrives through R, separate and in place, at every magnitude of the ladder
    that is admissible; the largest admissible one is the case that grades the kernel"""
    ctx = shared_ctx(1)
    prod, sk, B = REGIME_PRODS[path]
    out = []
    for m in LADDER:
        fy, fs = admissible(prod, B, m)
        ok = max(fy, fs) <= ADMISSIBLE_FRACTION
        out.append(_flag(f"mean through R, {path}, |m|/sigma = {m}: fp32 reference at {fy:.3f} (y) / {fs:.3f} (statistics) of the bound: "
                         f"{'admissible' if ok else 'NOT admissible, not run'}", True))
        if not ok:
            continue
        cpu, ref, r, full = regime_tensor(prod, m)
        P = Producer(ctx, prod, cpu)
        M, N = P.M, P.N
        HW = M // B
        gm, bt, _ = norm_params(N, B, False)
        gd, bd = gm.to(DEV), bt.to(DEV)
        r_dev = r.to(DEV)
        for mode in ("R", "alias"):
            name = f"mean through R, {path}, |m|/sigma = {m}, {mode}"
            ctl = Out(M, N, fill=r if mode == "alias" else None)
            split_producer(P, ctl, sk, mode, r_dev, defer=0)
            th.cuda.synchronize()
            x0 = ctl.view.clone()
            yref, sref, _ = gn_ref(x0.cpu().reshape(B, HW, N), gm, bt, None, 1)
            o = Out(M, N, fill=r if mode == "alias" else None)
            out += split_producer(P, o, sk, mode, r_dev, defer=1)
            n0 = reduces(ctx)
            scr = gn_scratch(ctx, B, HW, N)
            y = th.full((B, HW, N), NAN, device=DEV)
            gn_fwd_call(ctx, o.ptr, N, B, HW, N, gd, bd, None, 1, scr, y)
            out.append(path_flag(ctx, name, n0, "take"))
            th.cuda.synchronize()
            st = gn_stats(ctx, scr, B, HW, N)
            print(f"{name}: y at {bound_fraction(y.cpu(), yref):.3f}, statistics at {bound_fraction(st.cpu(), sref):.3f} of the bound")
            out += [_flag(f"{name}: tensor written back bit for bit", th.equal(o.view, x0)), rec(f"{name}: y", y, yref),
                    rec(f"{name}: statistics", st, sref)]
    return out


STALE = {"mismatch": check_mismatch, "concat_whole": check_concat_whole, "gemm_between": check_gemm_between, "refused": check_refused_consumer, "state_changes": check_state_changes,
         "second_stream": check_second_stream, "defer_modes": check_defer_modes, "other_readers": check_other_readers}


if __name__ == "__main__":  # one report: every record as JSON on stdout (keeps going after failures)
    import json
    import sys
    import time
    recs, times = [], {}
    for key in GROUPS:
        t0 = time.time()
        recs += [dict(r_, group=key) for r_ in check_group(key)]
        times[key] = time.time() - t0
    for key, fn in STALE.items():
        t0 = time.time()
        recs += [dict(r_, group=key) for r_ in fn()]
        times[key] = time.time() - t0
    for path in REGIME_PRODS:
        t0 = time.time()
        recs += [dict(r_, group="regime_" + path) for r_ in check_mean_through_R(path)]
        times["regime_" + path] = time.time() - t0
    bad = [r_ for r_ in recs if not r_["ok"]]
    json.dump({"records": recs, "failed": len(bad), "seconds": times}, sys.stdout, indent=1, default=str)
    print()
    sys.exit(1 if bad else 0)
