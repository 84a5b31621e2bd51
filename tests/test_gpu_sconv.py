"""The stride-2 3x3 conv (csrc/sconv.hip) through the C ABI: cgd_op_conv3x3_s2 and cgd_op_conv3x3_s2_dgrad against torch's float64
conv2d(stride=2, padding=1) and its autograd input gradient on the CPU, in the three precision modes.

Bound: that of the existing 3x3 conv op tests (tests/shape_edge_checks.py, tests/strided_checks.py): |a - b| <= 1e-4 + 1e-3 |ref| for every
element in modes 0 (f32) and 1 (bf16x3); mode 2 (one bf16 product) is the speed mode and is bounded as those tests bound it (error below
1e-2 of the reference's peak, and the strict bound must NOT hold, or it would not be biting).  Inputs are O(1): x, dy ~ N(0, 1), w ~ N(0, 1 / (9 Cin)).

Shapes (B, H, W, Cin, Cout): one output pixel with five of nine taps in the padding; a non-square map far below any tile with channel counts
that are multiples of 32 but not of 64; two samples with sample 0 set to NaN (nothing is read across the sample boundary); many K chunks; and
strided operands whose gaps and guard regions are pre-filled with NaN and must stay untouched."""
import functools
import math

import pytest
import torch as th
import torch.nn.functional as F

from tests import parity_checks as pc

pytestmark = pytest.mark.gpu

# (B, H, W, Cin, Cout, ldx - Cin, ldy - Cout)
SHAPES = [(1, 2, 2, 128, 128, 0, 0), (1, 4, 6, 96, 160, 0, 0), (2, 8, 8, 256, 128, 0, 0), (1, 16, 16, 512, 512, 0, 0), (3, 6, 10, 128, 128, 64, 32)]
IDS = ["one_pixel", "nonsquare_96_160", "two_samples", "many_chunks", "strided"]
GUARD = 4096  # floats behind every buffer


@functools.lru_cache(maxsize=None)
def context(precision):
    return pc._ctx(precision)


@functools.lru_cache(maxsize=None)
def case(B, H, W, Ci, Co):
    gen = pc.g(9100 + 7 * H + W + Ci + 3 * Co + B)
    x = th.randn(B, Ci, H, W, generator=gen)
    w = th.randn(Co, Ci, 3, 3, generator=gen) / math.sqrt(9 * Ci)
    b = 0.3 * th.randn(Co, generator=gen)
    dy = th.randn(B, Co, H // 2, W // 2, generator=gen)
    add = 0.5 * th.randn(B, Ci, H, W, generator=gen)
    xr = x.double().requires_grad_(True)
    y = F.conv2d(xr, w.double(), b.double(), stride=2, padding=1)
    (dx,) = th.autograd.grad(y, xr, dy.double())
    return dict(x=x, w=w, b=b, dy=dy, add=add, y=y.detach(), dx=dx.detach())


class Guarded:
    """(B, H, W, C) NHWC device view of row stride ld inside a NaN-filled buffer with a NaN guard behind it"""

    def __init__(self, B, H, W, C, ld, values_nchw=None):
        rows = B * H * W
        self.buf = th.full((rows * ld + GUARD,), float("nan"), device=pc.DEV)
        self.view = self.buf[: rows * ld].view(B, H, W, ld)[..., :C]
        self.C, self.ld, self.rows = C, ld, rows
        if values_nchw is not None:
            self.view.copy_(values_nchw.permute(0, 2, 3, 1).to(pc.DEV))

    def nchw(self):
        return self.view.permute(0, 3, 1, 2)

    def untouched(self):
        """the gaps between the rows and the guard still hold NaN"""
        gaps = self.buf[: self.rows * self.ld].view(self.rows, self.ld)[:, self.C:]
        return bool(th.isnan(gaps).all().item()) and bool(th.isnan(self.buf[self.rows * self.ld:]).all().item())


def grade(name, got, ref, precision):
    r = pc.rec(name, got, ref)
    print(f"{name}: abs {r['err_abs']:.3e} rel-to-peak {r['err_rel']:.3e} peak {r['ref_max']:.2f} strict {r['ok_strict']}")
    if precision == 2:
        assert bool(th.isfinite(got).all().item()) and r["err_rel"] < 1e-2, r
    else:
        assert r["ok"], r
    return r


def run_pair(ctx, c, B, H, W, Ci, Co, gx, gy, with_add, ldadd_gap=32):
    """forward into a guarded y, dgrad of c['dy'] into a guarded dx (+ add at its own stride) -> (X, Y, DY, DX, ADD)"""
    from cgd_amd import ops
    dev = pc.DEV
    X = Guarded(B, H, W, Ci, Ci + gx, c["x"])
    Y = Guarded(B, H // 2, W // 2, Co, Co + gy)
    w, b = c["w"].to(dev), c["b"].to(dev)
    ops.conv3x3_s2(ctx, X.view, w, b, out=Y.view)
    DY = Guarded(B, H // 2, W // 2, Co, Co + gy, c["dy"])
    DX = Guarded(B, H, W, Ci, Ci + gx)
    ADD = Guarded(B, H, W, Ci, Ci + ldadd_gap, c["add"]) if with_add else None
    ops.conv3x3_s2_dgrad(ctx, DY.view, w, add=ADD.view if with_add else None, out=DX.view)
    th.cuda.synchronize()
    return X, Y, DY, DX, ADD


@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_dgrad_match_float64(shape, precision):
    B, H, W, Ci, Co, gx, gy = shape
    ctx, c = context(precision), case(B, H, W, Ci, Co)
    tag = f"sconv[p{precision}] B{B} {H}x{W} {Ci}->{Co} ldx+{gx} ldy+{gy}"
    strict = []
    for with_add in (False, True):
        X, Y, DY, DX, ADD = run_pair(ctx, c, B, H, W, Ci, Co, gx, gy, with_add)
        strict.append(grade(f"{tag} y", Y.nchw(), c["y"], precision)["ok_strict"])
        ref_dx = c["dx"] + (c["add"].double() if with_add else 0.0)
        strict.append(grade(f"{tag} dx add={int(with_add)}", DX.nchw(), ref_dx, precision)["ok_strict"])
        for name, G in (("x", X), ("y", Y), ("dy", DY), ("dx", DX)) + ((("add", ADD),) if with_add else ()):
            assert G.untouched(), f"{tag}: the gaps or the guard of {name} were written"
        if not with_add:
            # the adjoint identity <conv(x) - bias, g> = <x, dgrad(g)> on the DEVICE outputs in float64.  It is exact for the references, and every
            # device element is within the parity bound e of its reference, so the two sides differ by sum g e(y) - sum x e(dx).  The element
            # errors are rounding errors of separate sums: taken as independent and each as large as its bound, that difference has the standard
            # deviation sqrt(sum g^2 e(y)^2 + sum x^2 e(dx)^2); the slack is six of them (the worst case, sum |g| e + sum |x| e, is ~100 times
            # wider and would let a dropped tap through)
            yd, dxd = Y.nchw().double().cpu(), DX.nchw().double().cpu()
            g, x = c["dy"].double(), c["x"].double()
            lhs = ((yd - c["b"].double()[None, :, None, None]) * g).sum().item()
            rhs = (x * dxd).sum().item()
            if precision == 2:
                ey, edx = 1e-2 * c["y"].abs().max(), 1e-2 * c["dx"].abs().max()
            else:
                ey, edx = 1e-4 + 1e-3 * c["y"].abs(), 1e-4 + 1e-3 * c["dx"].abs()
            slack = 6.0 * math.sqrt(((g * ey) ** 2).sum().item() + ((x * edx) ** 2).sum().item())
            print(f"{tag} adjoint: {lhs:.9e} vs {rhs:.9e}, |difference| {abs(lhs - rhs):.3e}, slack {slack:.3e}")
            assert abs(lhs - rhs) <= slack
    if precision == 2 and Ci * 9 >= 1024:
        assert not all(strict), "a single bf16 product cannot meet the fp32 tolerance: the strict criterion is not biting"


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_large_tile_with_a_half_filled_channel_block_and_a_row_tail(precision):
    """the 128 x 64 tile is chosen only where it gives every CU a workgroup, so none of the shapes above reaches it with a ragged edge:
    258 x 258 x 96 -> 96 is 131 row tiles (the last one holds 1 of 128 rows) by 2 channel tiles (the second one holds 32 of 64 columns) in
    the forward, and the same tiles per parity class in the backward"""
    B, H, W, Ci, Co = 1, 258, 258, 96, 96
    ctx, c = context(precision), case(B, H, W, Ci, Co)
    tag = f"sconv[p{precision}] B{B} {H}x{W} {Ci}->{Co} (128 x 64 tile, ragged)"
    X, Y, DY, DX, ADD = run_pair(ctx, c, B, H, W, Ci, Co, 0, 32, True)
    grade(f"{tag} y", Y.nchw(), c["y"], precision)
    grade(f"{tag} dx", DX.nchw(), c["dx"] + c["add"].double(), precision)
    for name, G in (("x", X), ("y", Y), ("dy", DY), ("dx", DX), ("add", ADD)):
        assert G.untouched(), f"{tag}: the gaps or the guard of {name} were written"


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_nothing_is_read_across_the_sample_boundary(precision):
    B, H, W, Ci, Co = 2, 8, 8, 256, 128
    ctx, c = context(precision), case(B, H, W, Ci, Co)
    from cgd_amd import ops
    dev = pc.DEV
    w, b = c["w"].to(dev), c["b"].to(dev)
    x = c["x"].permute(0, 2, 3, 1).contiguous().to(dev)
    x[0] = float("nan")
    y = ops.conv3x3_s2(ctx, x, w, b)
    dy = c["dy"].permute(0, 2, 3, 1).contiguous().to(dev)
    dy[0] = float("nan")
    dx = ops.conv3x3_s2_dgrad(ctx, dy, w)
    th.cuda.synchronize()
    assert bool(th.isnan(y[0]).all().item()) and bool(th.isnan(dx[0]).all().item())
    grade(f"sconv[p{precision}] sample 1 behind a NaN sample 0: y", y[1:].permute(0, 3, 1, 2), c["y"][1:], precision)
    grade(f"sconv[p{precision}] sample 1 behind a NaN sample 0: dx", dx[1:].permute(0, 3, 1, 2), c["dx"][1:], precision)


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_two_runs_are_bit_identical(precision):
    ctx = context(precision)
    for (B, H, W, Ci, Co, gx, gy) in (SHAPES[1], SHAPES[3], SHAPES[4]):
        c = case(B, H, W, Ci, Co)
        runs = [run_pair(ctx, c, B, H, W, Ci, Co, gx, gy, True) for _ in range(2)]
        for k, name in ((1, "y"), (3, "dx")):
            a, b = runs[0][k].view.contiguous(), runs[1][k].view.contiguous()
            assert th.equal(a.view(th.int32), b.view(th.int32)), f"p{precision} {name} of {B}x{H}x{W} {Ci}->{Co} differs between two runs"


def test_on_a_created_stream_behind_pending_work():
    """the launches follow the caller's stream: x and dy are produced on a created stream behind a queue of matmuls; a launch on another stream
    would read the NaN the buffers hold until then"""
    from cgd_amd import ops
    B, H, W, Ci, Co = 3, 6, 10, 128, 128
    ctx, c, dev = context(1), case(3, 6, 10, 128, 128), pc.DEV
    w, b = c["w"].to(dev), c["b"].to(dev)
    src_x = c["x"].permute(0, 2, 3, 1).contiguous().to(dev)
    src_dy = c["dy"].permute(0, 2, 3, 1).contiguous().to(dev)
    x, dy = th.full_like(src_x, float("nan")), th.full_like(src_dy, float("nan"))
    heavy = th.randn(2048, 2048, device=dev)
    th.cuda.synchronize()
    s = th.cuda.Stream(priority=-1)
    with th.cuda.stream(s):
        z = heavy
        for _ in range(20):
            z = (z @ heavy) * (1.0 / 64.0)
        zero = (z.sum() * 0.0).nan_to_num(0.0)
        x.copy_(src_x + zero)
        dy.copy_(src_dy + zero)
        y = ops.conv3x3_s2(ctx, x, w, b)
        dx = ops.conv3x3_s2_dgrad(ctx, dy, w)
    s.synchronize()
    grade("sconv on a created stream: y", y.permute(0, 3, 1, 2), c["y"], 1)
    grade("sconv on a created stream: dx", dx.permute(0, 3, 1, 2), c["dx"], 1)


def test_refusals_raise_and_write_nothing():
    from cgd_amd import ops
    ctx, dev = context(1), pc.DEV
    w = th.zeros(32, 32, 3, 3, device=dev)
    y = th.full((1, 2, 2, 32), float("nan"), device=dev)
    for x in (th.zeros(1, 3, 4, 32, device=dev), th.zeros(1, 4, 5, 32, device=dev)):
        with pytest.raises(RuntimeError, match="even"):
            ops.conv3x3_s2(ctx, x, w, out=y)
    with pytest.raises(RuntimeError, match="multiples of 32"):
        ops.conv3x3_s2(ctx, th.zeros(1, 4, 4, 48, device=dev), th.zeros(32, 48, 3, 3, device=dev), out=y)
    wide = th.zeros(1, 4, 4, 34, device=dev)[..., :32]
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.conv3x3_s2(ctx, wide, w, out=y)
    th.cuda.synchronize()
    assert bool(th.isnan(y).all().item())
