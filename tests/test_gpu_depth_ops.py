"""The depth network's own kernels (csrc/depth.hip) through their cgd_op_* entries against torch on the CPU, at the project's literal
|a - b| <= 1e-4 + 1e-3 |ref|; every refusal is checked to come before any launch (cgd_launch_counts)."""
import ctypes as C
import functools

import pytest
import torch as th
import torch.nn.functional as F

from tests import depth_ref as R
from tests import parity_checks as pc
from tests.parity_checks import DEV, g, rec

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ctx():
    return pc._ctx(1)


def _s():
    return _ctx().stream()


def _ok(records):
    bad = [r for r in records if not r["ok"]]
    assert not bad, bad[0]


def _launches():
    counts = (C.c_uint64 * 2)()
    _ctx().lib.cgd_launch_counts(counts)
    return counts[0]


def _refused(call, text):
    from cgd_amd.lib import CgdError
    th.cuda.synchronize()
    before = _launches()
    with pytest.raises(CgdError, match=text):
        _ctx().check(call())
    assert _launches() == before


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("Hi,Wi", [(1, 1), (1, 3), (2, 5), (12, 12)])
@pytest.mark.parametrize("Cn", [4, 32, 256])
def test_bilinear_up2x_align_corners(Hi, Wi, Cn):
    ctx, B = _ctx(), 2
    x = th.randn(B, Cn, Hi, Wi, generator=g(Hi * 100 + Wi + Cn))
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)
    xd = _nhwc(x).to(DEV)
    out = th.empty(B, 2 * Hi, 2 * Wi, Cn, device=DEV)
    ctx.check(ctx.lib.cgd_op_bilinear_up2x_ac(ctx.h, xd.data_ptr(), Cn, out.data_ptr(), Cn, None, 0, B, Hi, Wi, Cn, _s()))
    _ok([rec(f"up2x_ac {Hi}x{Wi} C{Cn}", out.permute(0, 3, 1, 2), ref)])
    if (Hi, Wi) == (1, 1):  # the degenerate case is a copy
        assert th.equal(out.cpu(), _nhwc(x)[:, :, :, None, :].expand(B, 1, 1, 4, Cn).reshape(B, 2, 2, Cn))


def test_bilinear_up2x_align_corners_strided_and_fused_add():
    ctx, B, Hi, Wi, Cn = _ctx(), 2, 2, 5, 32
    x = th.randn(B, Cn, Hi, Wi, generator=g(1))
    add = th.randn(B, Cn, 2 * Hi, 2 * Wi, generator=g(2))
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)
    # row strides larger than C: channel slices of wider buffers, whose other columns must stay untouched
    xin = th.full((B, Hi, Wi, Cn + 8), 7.0, device=DEV)
    xin[..., 4:4 + Cn] = _nhwc(x).to(DEV)
    out = th.full((B, 2 * Hi, 2 * Wi, Cn + 16), -3.0, device=DEV)
    ctx.check(ctx.lib.cgd_op_bilinear_up2x_ac(ctx.h, xin.data_ptr() + 16, Cn + 8, out.data_ptr() + 32, Cn + 16, None, 0, B, Hi, Wi, Cn, _s()))
    _ok([rec("up2x_ac strided", out[..., 8:8 + Cn].permute(0, 3, 1, 2), ref)])
    assert bool((out[..., :8] == -3.0).all()) and bool((out[..., 8 + Cn:] == -3.0).all())
    ad = _nhwc(add).to(DEV)
    xd = _nhwc(x).to(DEV)
    out2 = th.empty(B, 2 * Hi, 2 * Wi, Cn, device=DEV)
    ctx.check(ctx.lib.cgd_op_bilinear_up2x_ac(ctx.h, xd.data_ptr(), Cn, out2.data_ptr(), Cn, ad.data_ptr(), Cn, B, Hi, Wi, Cn, _s()))
    _ok([rec("up2x_ac + add", out2.permute(0, 3, 1, 2), ref + add.double())])
    lib = ctx.lib
    _refused(lambda: lib.cgd_op_bilinear_up2x_ac(ctx.h, xd.data_ptr(), 6, out2.data_ptr(), 6, None, 0, B, Hi, Wi, 6, _s()), "multiples of 4")
    _refused(lambda: lib.cgd_op_bilinear_up2x_ac(ctx.h, xd.data_ptr() + 4, Cn, out2.data_ptr(), Cn, None, 0, B, Hi, Wi, Cn, _s()), "16-byte aligned")
    _refused(lambda: lib.cgd_op_bilinear_up2x_ac(ctx.h, xd.data_ptr(), Cn, out2.data_ptr(), Cn - 4, None, 0, B, Hi, Wi, Cn, _s()), "strides >= C")
    _refused(lambda: lib.cgd_op_bilinear_up2x_ac(ctx.h, xd.data_ptr(), Cn, out2.data_ptr(), Cn, ad.data_ptr(), Cn - 4, B, Hi, Wi, Cn, _s()), "add operand")
    _refused(lambda: lib.cgd_op_bilinear_up2x_ac(ctx.h, xd.data_ptr(), Cn, out2.data_ptr(), Cn, None, 0, B, 0, Wi, Cn, _s()), "out of range")


def test_relu_rows():
    ctx, rows, Cn = _ctx(), 37, 32
    x = th.randn(rows, Cn + 4, generator=g(3)).to(DEV)
    out = th.zeros(rows, Cn, device=DEV)
    ctx.check(ctx.lib.cgd_op_relu_rows(ctx.h, x.data_ptr(), Cn + 4, out.data_ptr(), Cn, rows, Cn, _s()))
    assert th.equal(out, x[:, :Cn].clamp(min=0))
    ctx.check(ctx.lib.cgd_op_relu_rows(ctx.h, out.data_ptr(), Cn, out.data_ptr(), Cn, rows, Cn, _s()))  # in place
    assert th.equal(out, x[:, :Cn].clamp(min=0))
    _refused(lambda: ctx.lib.cgd_op_relu_rows(ctx.h, x.data_ptr(), Cn + 4, out.data_ptr(), Cn, rows, 6, _s()), "multiples of 4")
    _refused(lambda: ctx.lib.cgd_op_relu_rows(ctx.h, x.data_ptr(), Cn + 4, out.data_ptr(), Cn, 0, Cn, _s()), "rows must be positive")


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("Cin,Cout", [(32, 32), (64, 32)])
def test_conv_transpose_against_torch(k, Cin, Cout):
    ctx = _ctx()
    recs = []
    for B in (1, 2):
        for H, W in ((1, 1), (2, 3)):
            x = th.randn(B, Cin, H, W, generator=g(k + Cin + B + H))
            w = th.randn(Cin, Cout, k, k, generator=g(5)) / Cin ** 0.5
            bias = 0.3 * th.randn(Cout, generator=g(6))
            ref = F.conv_transpose2d(x.double(), w.double(), bias.double(), stride=k)
            xd, wd, bd = _nhwc(x).to(DEV), w.to(DEV), bias.to(DEV)
            out = th.empty(B, H * k, W * k, Cout, device=DEV)
            wpack = th.empty(Cin * Cout * k * k, device=DEV)
            gbuf = th.empty(B * H * W * Cout * k * k, device=DEV)
            ctx.check(ctx.lib.cgd_op_conv_transpose(ctx.h, xd.data_ptr(), Cin, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), Cout, wpack.data_ptr(),
                                                    gbuf.data_ptr(), B, H, W, Cin, Cout, k, _s()))
            recs.append(rec(f"conv_transpose k{k} {Cin}->{Cout} B{B} {H}x{W}", out.permute(0, 3, 1, 2), ref))
    _ok(recs)
    args = (xd.data_ptr(), Cin, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), Cout, wpack.data_ptr(), gbuf.data_ptr())
    _refused(lambda: ctx.lib.cgd_op_conv_transpose(ctx.h, *args, B, H, W, Cin, Cout, 3, _s()), "must be 2 or 4")
    _refused(lambda: ctx.lib.cgd_op_conv_transpose(ctx.h, *args, B, H, W, Cin, 48, k, _s()), "multiples of 32")
    _refused(lambda: ctx.lib.cgd_op_conv_transpose(ctx.h, xd.data_ptr() + 4, *args[1:], B, H, W, Cin, Cout, k, _s()), "misaligned")


@pytest.mark.parametrize("gh,gw", [(1, 1), (2, 3)])
def test_readout_against_torch(gh, gw):
    ctx, B, W, L = _ctx(), 2, 128, gh * gw
    tok = th.randn(B, L + 1, W, generator=g(7))
    tok[1, 0] = tok[0, 0] * -0.5 + 1.0  # the class rows differ per image
    w = th.randn(W, 2 * W, generator=g(8)) / (2 * W) ** 0.5
    bias = 0.3 * th.randn(W, generator=g(9))
    cat = th.cat([tok[:, 1:], tok[:, :1].expand(-1, L, -1)], -1)
    ref = F.gelu(F.linear(cat.double(), w.double(), bias.double()))
    td, wd, bd = tok.to(DEV), w.to(DEV), bias.to(DEV)
    out, tmp, clsv = th.empty(B, L, W, device=DEV), th.empty(B * (L + 1) * W, device=DEV), th.empty(B * W, device=DEV)
    ctx.check(ctx.lib.cgd_op_depth_readout(ctx.h, td.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), tmp.data_ptr(), clsv.data_ptr(), B, L, W,
                                           _s()))
    _ok([rec(f"readout {gh}x{gw}", out, ref)])
    _refused(lambda: ctx.lib.cgd_op_depth_readout(ctx.h, td.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), tmp.data_ptr(), clsv.data_ptr(), B, L,
                                                  100, _s()), "multiple of 32")
    _refused(lambda: ctx.lib.cgd_op_depth_readout(ctx.h, td.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), None, clsv.data_ptr(), B, L, W, _s()),
             "missing buffer")


@pytest.mark.parametrize("H,W", [(2, 2), (32, 48)])
def test_head_tail_against_torch(H, W):
    ctx, rows = _ctx(), H * W
    offset, scale, floor = 1.0, 2.0, 0.3
    w = th.randn(32, generator=g(10)) / 32 ** 0.5
    bias = th.tensor([0.1])
    x = th.randn(rows, 40, generator=g(11))  # row stride 40 > 32
    x[0, :32], x[1, :32], x[2, :32], x[3, :32] = 4 * w, -4 * w, 0.4 * w, th.relu(-w) * 9  # far above / below zero, small and positive, negative lobes only
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    recs = []
    for relu_in in (0, 1):
        xin = (x[:, :32].clamp(min=0) if relu_in else x[:, :32]).double()
        inv_ref = (xin @ w.double() + bias.double()).clamp(min=0)
        dep_ref = ((offset - inv_ref) / scale).clamp(min=floor)
        assert bool((inv_ref == 0).any()) and bool((inv_ref > 0).any())                    # both sides of the ReLU
        assert bool((dep_ref == floor).any()) and bool((dep_ref > floor).any())            # the floor clamp and the plain mapping
        inv, dep = th.empty(rows, device=DEV), th.empty(rows, device=DEV)
        ctx.check(ctx.lib.cgd_op_depth_head_tail(ctx.h, xd.data_ptr(), 40, wd.data_ptr(), bd.data_ptr(), inv.data_ptr(), dep.data_ptr(), rows, relu_in,
                                                 offset, scale, floor, _s()))
        recs += [rec(f"head tail inv {H}x{W} relu_in{relu_in}", inv, inv_ref, allow_small=True), rec(f"head tail depth {H}x{W} relu_in{relu_in}", dep, dep_ref)]
        only = th.empty(rows, device=DEV)
        ctx.check(ctx.lib.cgd_op_depth_head_tail(ctx.h, xd.data_ptr(), 40, wd.data_ptr(), bd.data_ptr(), None, only.data_ptr(), rows, relu_in, offset,
                                                 scale, floor, _s()))
        assert th.equal(only, dep)
    _ok(recs)
    a = (wd.data_ptr(), bd.data_ptr(), inv.data_ptr(), dep.data_ptr(), rows, 1)
    _refused(lambda: ctx.lib.cgd_op_depth_head_tail(ctx.h, xd.data_ptr(), 30, *a, offset, scale, floor, _s()), "stride >= 32")
    _refused(lambda: ctx.lib.cgd_op_depth_head_tail(ctx.h, xd.data_ptr(), 40, *a, offset, 0.0, floor, _s()), "scale must not be zero")
    _refused(lambda: ctx.lib.cgd_op_depth_head_tail(ctx.h, xd.data_ptr(), 40, wd.data_ptr(), bd.data_ptr(), None, None, rows, 1, offset, scale, floor, _s()),
             "missing or misaligned")


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(256, 256, 384, 384), (96, 64, 160, 96), (384, 384, 256, 256), (64, 64, 32, 32), (48, 80, 64, 96), (40, 24, 40, 24)])
@pytest.mark.parametrize("Cn", [1, 3])
def test_resize_cubic_against_the_edge_replicating_reference(Hi, Wi, Ho, Wo, Cn):
    ctx, B = _ctx(), 2
    x = th.rand(B, Cn, Hi, Wi, generator=g(Hi + Wo + Cn))
    xd = x.to(DEV)
    out = th.empty(B, Cn, Ho, Wo, device=DEV)
    ctx.check(ctx.lib.cgd_op_resize_cubic(ctx.h, xd.data_ptr(), out.data_ptr(), B * Cn, Hi, Wi, Ho, Wo, 1.0, 0.0, 0.0, 0, _s()))
    ref = R.resize_edge(x.double(), Ho, Wo)
    if (Hi, Wi) == (Ho, Wo):
        assert th.equal(out.cpu(), x)  # an identical size copies bits
    _ok([rec(f"resize_cubic {Hi}x{Wi}->{Ho}x{Wo} C{Cn}", out, ref)])
    # normalised in the same launch, and the lower clamp
    ctx.check(ctx.lib.cgd_op_resize_cubic(ctx.h, xd.data_ptr(), out.data_ptr(), B * Cn, Hi, Wi, Ho, Wo, 2.0, -1.0, -0.5, 1, _s()))
    _ok([rec("resize_cubic affine + clamp", out, (2 * ref - 1).clamp(min=-0.5))])


def test_resize_cubic_refusals():
    ctx = _ctx()
    x, out = th.zeros(1, 1, 512, 16, device=DEV), th.zeros(1, 1, 32, 16, device=DEV)
    lib = ctx.lib
    _refused(lambda: lib.cgd_op_resize_cubic(ctx.h, x.data_ptr(), out.data_ptr(), 1, 512, 16, 32, 16, 1.0, 0.0, 0.0, 0, _s()), "8-fold")
    _refused(lambda: lib.cgd_op_resize_cubic(ctx.h, x.data_ptr(), out.data_ptr(), 0, 64, 16, 32, 16, 1.0, 0.0, 0.0, 0, _s()), "out of range")
    _refused(lambda: lib.cgd_op_resize_cubic(ctx.h, x.data_ptr(), x.data_ptr(), 1, 64, 16, 32, 16, 1.0, 0.0, 0.0, 0, _s()), "must differ")
    _refused(lambda: lib.cgd_op_resize_cubic(ctx.h, None, out.data_ptr(), 1, 64, 16, 32, 16, 1.0, 0.0, 0.0, 0, _s()), "required")
