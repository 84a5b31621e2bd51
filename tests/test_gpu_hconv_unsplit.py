"""hconv2_kernel on the unsplit 4x16-pixel x 128-channel tile (cgd_set_hconv variant bit 3: all of K in one workgroup, bf16x3), through the C ABI
(cgd_op_conv3x3_ex) against a float64 conv at the bound of the existing hconv2 op-level checks (parity_checks.check_conv: |a - b| <= 1e-4 +
1e-3 |ref| per element, O(1) outputs, unit-peak gradients).

Shapes: maps 8x16, 16x16 and 8x32 (2-4 pixel tiles, tile borders in both directions, the padding ring), batch 1 and 2; Cin 32, 96, 160 (one chunk,
an odd chunk count, a chunk tail of the 9-slot fragment ring) and 160 as a 96 + 64 concat buffer read at row stride 192; Cout 128 and 256.  Each
case runs the plain conv, bias + residual, fused GroupNorm + SiLU staging, the nearest-2x upsampled input view and the dgrad packing.

The records its epilogue leaves (second half of the file): forward (mean, M2) and backward sums per (64-pixel tile, channel) against float64, their
merge by the GroupNorm launchers (beside 128-pixel records of wconv_kernel in the other half of a concat) against float64 and against the sweep path
on the same tensor, and the fused skip dgrad (cgd_op_gemm_gn_bwd) on tables folded from 64-pixel records against the two launches."""
import functools
import math

import pytest
import torch as th
import torch.nn.functional as F

from tests import parity_checks as pc

pytestmark = pytest.mark.gpu

MAPS = [(8, 16), (16, 16), (8, 32)]
CINS = [(32, 32), (96, 96), (160, 160), (160, 192)]  # (Cin, row stride of x)
CASES = [(B, H, W, ci, ld, co) for (H, W) in MAPS for B in (1, 2) for (ci, ld) in CINS for co in (128, 256)]
UNSPLIT = 1 + 16 * 8  # cgd_set_hconv mode: automatic halo kernel, tile variant bit 3


@functools.lru_cache(maxsize=None)
def context():
    ctx = pc._ctx(1)
    ctx.check(ctx.lib.cgd_set_hconv(ctx.h, UNSPLIT, 256))
    return ctx


@functools.lru_cache(maxsize=None)
def case(B, H, W, Ci, Co):
    gen = pc.g(7700 + H * W + Ci + Co + B)
    x = th.randn(B, Ci, H, W, generator=gen)
    xs = th.randn(B, Ci, H // 2, W // 2, generator=gen)
    w = th.randn(Co, Ci, 3, 3, generator=gen) / math.sqrt(9 * Ci)
    b = 0.3 * th.randn(Co, generator=gen)
    r = 0.3 * th.randn(B, H, W, Co, generator=gen)
    ab = th.stack([1 + 0.2 * th.randn(B, Ci, generator=gen), 0.3 * th.randn(B, Ci, generator=gen)], -1)
    wd_, xd = w.double(), x.double()
    ref = {"plain": F.conv2d(xd, wd_, None, padding=1), "bias_res": F.conv2d(xd, wd_, b.double(), padding=1) + r.double().permute(0, 3, 1, 2),
           "gn": F.conv2d(F.silu(xd * ab[..., 0].double()[:, :, None, None] + ab[..., 1].double()[:, :, None, None]), wd_, b.double(), padding=1),
           "ups": F.conv2d(F.interpolate(xs.double(), scale_factor=2, mode="nearest"), wd_, b.double(), padding=1)}
    # dgrad packing: dy has Ci channels here (the launch's K), the gradient Co (its N): torch weight [Ci][Co]
    wt = th.randn(Ci, Co, 3, 3, generator=gen) / math.sqrt(9 * Ci)
    dy = th.randn(B, Ci, H, W, generator=gen)
    xr = th.zeros(B, Co, H, W, dtype=th.float64, requires_grad=True)
    (F.conv2d(xr, wt.double(), None, padding=1) * dy.double()).sum().backward()
    sd = pc.unit_seed(xr.grad)
    ref["dgrad"] = xr.grad * sd
    return dict(x=x, xs=xs, w=w, b=b, r=r, ab=ab.contiguous(), wt=wt, dy=dy * sd, ref={k: v.float() for k, v in ref.items()})


def wide(t_nchw, ld):
    """NCHW host tensor -> NHWC device view of row stride ld (NaN beyond the channels: a concat buffer's sibling must never be read)"""
    B, C, H, W = t_nchw.shape
    buf = th.full((B, H, W, ld), float("nan"), device=pc.DEV)
    buf[..., :C] = t_nchw.permute(0, 2, 3, 1).to(pc.DEV)
    return buf[..., :C]


def conv_ex(ctx, x, w_packed, w_frag, B, H, W, Ci, Co, bias=None, R=None, gn_ab=None, ups=0, splitk=1, stats=0, gnb=None, y=None):
    from cgd_amd import lib as L
    y = th.full((B, H, W, Co), float("nan"), device=pc.DEV) if y is None else y
    gx, gld, gscr = (gnb[0].data_ptr(), gnb[1], gnb[2].data_ptr()) if gnb else (None, 0, None)
    ctx.check(ctx.lib.cgd_op_conv3x3_ex(ctx.h, x.data_ptr(), x.stride(2), w_packed.data_ptr(), w_frag.data_ptr(), y.data_ptr(), y.stride(2),
                                        None if bias is None else bias.data_ptr(), None if R is None else R.data_ptr(), 0 if R is None else R.stride(2),
                                        None if gn_ab is None else gn_ab.data_ptr(), B, H, W, Ci, Co, ups, 512, splitk, 0, stats, gx, gld, gscr,
                                        L.stream_ptr()))
    return y


@pytest.mark.parametrize("B,H,W,Ci,ld,Co", CASES)
def test_unsplit_tile_matches_float64(B, H, W, Ci, ld, Co):
    from cgd_amd import ops
    ctx, c = context(), case(B, H, W, Ci, Co)
    dev = pc.DEV
    wf = ops.pack_conv3x3(c["w"])[0].to(dev)
    wfrag = ops.pack_conv3x3_frag(ctx, c["w"].to(dev), dgrad=False)
    x, xs = wide(c["x"], ld), wide(c["xs"], ld)
    b, r, ab = c["b"].to(dev), c["r"].to(dev), c["ab"].to(dev)
    got = {"plain": conv_ex(ctx, x, wf, wfrag, B, H, W, Ci, Co),
           "bias_res": conv_ex(ctx, x, wf, wfrag, B, H, W, Ci, Co, bias=b, R=r),
           "gn": conv_ex(ctx, x, wf, wfrag, B, H, W, Ci, Co, bias=b, gn_ab=ab),
           "ups": conv_ex(ctx, xs, wf, wfrag, B, H, W, Ci, Co, bias=b, ups=1)}
    wd = ops.pack_conv3x3(c["wt"])[1].to(dev)
    wdfrag = ops.pack_conv3x3_frag(ctx, c["wt"].to(dev), dgrad=True)
    got["dgrad"] = conv_ex(ctx, wide(c["dy"], ld), wd, wdfrag, B, H, W, Ci, Co)
    th.cuda.synchronize()
    recs = [pc.rec(f"hconv unsplit {k} B{B} {H}x{W} {Ci}(ld {ld})->{Co}", v.permute(0, 3, 1, 2), c["ref"][k]) for k, v in got.items()]
    for q in recs:
        print(f"{q['name']}: abs {q['err_abs']:.3e} of peak {q['ref_max']:.2f}")
    for q in recs:
        assert q["ok"], q


# ---- GroupNorm records from the unsplit tile's epilogue --------------------------------------------------------------------------------------------
# One map of 32 x 64 pixels (above the single-launch GroupNorm size, 32 tiles of 64 pixels per sample), B = 2, Cin = 32.  Bounds: those of
# parity_checks.check_gn_records (the existing op-level record test): means within 2e-4 sigma of float64 at |mean| / sigma = 1e3, everything else
# at the literal 1e-4 + 1e-3 |ref|.
RB, RH, RW, RCI = 2, 32, 64, 32
RHW = RH * RW


def peek(ctx, y, C, kind):
    """(records [B * HW / pixels][C][2] as a host tensor, pixels per record) of the live records of tensor y"""
    import ctypes
    from cgd_amd import lib as L
    pix = ctypes.c_int()
    buf = th.zeros(RB * RHW // 64 * C * 2, device=pc.DEV)
    ctx.check(ctx.lib.cgd_op_gn_records(ctx.h, y.data_ptr(), y.stride(1), RB * RHW, C, kind, buf.data_ptr(), buf.numel(), ctypes.byref(pix), L.stream_ptr()))
    assert pix.value, "the launch left no records"
    n = RB * RHW // pix.value
    return buf[:n * C * 2].reshape(n, C, 2).double().cpu(), pix.value


def tiles64(t):
    """[B, HW, C] -> [B * tiles, 64, C] in the launch's tile order (sample, tile row of 4 image rows, tile column of 16)"""
    B, _, C = t.shape
    return t.reshape(B, RH // 4, 4, RW // 16, 16, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (RH // 4) * (RW // 16), 64, C)


def gn_fwd(ctx, x3, C, act=1):
    from cgd_amd import lib as L
    from cgd_amd import ops
    gen = pc.g(91)
    gamma, beta = (1 + 0.1 * th.randn(C, generator=gen)).to(pc.DEV), (0.1 * th.randn(C, generator=gen)).to(pc.DEV)
    scr = ops.gn_scratch(ctx, RB, RHW, C, pc.DEV)
    y = th.empty(RB, RHW, C, device=pc.DEV)
    ctx.check(ctx.lib.cgd_op_gn_fwd(ctx.h, x3.data_ptr(), x3.stride(1), y.data_ptr(), C, RB, RHW, C, gamma.data_ptr(), beta.data_ptr(), None, act, 1e-5,
                                    scr.data_ptr(), L.stream_ptr()))
    return y, scr, gamma, beta


def ref_fwd(x3, gamma, beta):
    xr = x3.detach().double().cpu().requires_grad_()
    y = F.silu(F.group_norm(xr.permute(0, 2, 1), 32, gamma.double().cpu(), beta.double().cpu(), 1e-5))
    return xr, y.permute(0, 2, 1)


def group_stats_recs(ctx, tag, scr, x3, C):
    off = int(ctx.lib.cgd_op_gn_stats_offset(RB, RHW, C))
    st = scr[off:off + RB * 64].reshape(RB, 32, 2).double().cpu()
    xg = x3.detach().double().cpu().reshape(RB, RHW, 32, C // 32).permute(0, 2, 1, 3).reshape(RB, 32, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    return [pc.rec(f"{tag} (group mean - float64 mean) / sigma", (st[..., 0] - mean) / var.sqrt(), th.zeros_like(mean), rtol=0.0, atol=2e-4, allow_small=True),
            pc.rec(f"{tag} group rstd", st[..., 1], 1.0 / (var + 1e-5).sqrt())]


def coef_table(ctx, scr, C):
    off = int(ctx.lib.cgd_op_gn_stats_offset(RB, RHW, C)) + RB * 64
    return scr[off:off + RB * C * 4].reshape(RB, C, 4).clone()


def report(recs):
    for q in recs:
        print(f"{q['name']}: abs {q['err_abs']:.3e} (ref peak {q['ref_max']:.3g})")
    for q in recs:
        assert q["ok"], q


def test_forward_records_of_64_pixel_tiles_and_their_merge_with_128_pixel_records():
    from cgd_amd import lib as L
    from cgd_amd import ops
    ctx = context()
    lib = ctx.lib
    C0, C1 = 128, 64  # 192 channels, 6 per group: group 21 straddles the halves; the first comes from the unsplit tile, the second from wconv_kernel
    Ct = C0 + C1
    cat = th.zeros(RB, RHW, Ct, device=pc.DEV)
    gen = pc.g(7801)
    x = th.randn(RB, RH, RW, RCI, generator=gen).to(pc.DEV)
    w0 = (th.randn(C0, RCI, 3, 3, generator=gen) / math.sqrt(9 * RCI)).to(pc.DEV)
    w1 = (th.randn(C1, RCI, 3, 3, generator=gen) / math.sqrt(9 * RCI)).to(pc.DEV)
    b0, b1 = (1000.0 + 3.0 * th.randn(C0, generator=gen)).to(pc.DEV), (1000.0 + 3.0 * th.randn(C1, generator=gen)).to(pc.DEV)
    ctx.check(lib.cgd_op_new_pass(ctx.h))

    def producers():
        y0 = cat[:, :, :C0]
        conv_ex(ctx, x, ops.pack_conv3x3(w0)[0].to(pc.DEV), ops.pack_conv3x3_frag(ctx, w0), RB, RH, RW, RCI, C0, bias=b0, stats=1,
                y=cat.reshape(RB, RH, RW, Ct)[..., :C0])
        ctx.check(lib.cgd_op_conv3x3_wino_ex(ctx.h, x.data_ptr(), RCI, ops.pack_conv3x3_wino(ctx, w1).data_ptr(), cat[:, :, C0:].data_ptr(), Ct,
                                             b1.data_ptr(), None, 0, None, RB, RH, RW, RCI, C1, 0, 1, None, 0, None, L.stream_ptr()))
        return y0

    y0 = producers()
    recs, pix = peek(ctx, y0, C0, 0)
    assert pix == 64
    t = tiles64(y0.detach().double().cpu())
    mean, m2 = t.mean(1), ((t - t.mean(1, keepdim=True)) ** 2).sum(1)
    out = [pc.rec("records fwd: (tile mean - float64) / tile sigma", (recs[..., 0] - mean) / (m2 / 64).sqrt(), th.zeros_like(mean), rtol=0.0, atol=2e-4,
                  allow_small=True),
           pc.rec("records fwd: M2 / 64", recs[..., 1] / 64, m2 / 64)]
    m0 = int(lib.cgd_op_gn_record_merges(ctx.h))
    y, scr, gamma, beta = gn_fwd(ctx, cat, Ct)
    assert int(lib.cgd_op_gn_record_merges(ctx.h)) == m0 + 1, "the GroupNorm of the concat did not merge the 64- and 128-pixel records"
    _, yref = ref_fwd(cat, gamma, beta)
    out += group_stats_recs(ctx, "merge of 64- + 128-pixel records", scr, cat, Ct)
    out.append(pc.rec("merge: y", y, yref.float()))
    cm = coef_table(ctx, scr, Ct)
    ctx.check(lib.cgd_op_new_pass(ctx.h))  # the records are dead: the sweep path on the same tensor
    y2, scr2, _, _ = gn_fwd(ctx, cat, Ct)
    assert int(lib.cgd_op_gn_record_merges(ctx.h)) == m0 + 1
    out += group_stats_recs(ctx, "sweep of the same tensor", scr2, cat, Ct)
    cs = coef_table(ctx, scr2, Ct)
    out += [pc.rec("folded a: merge against sweep", cm[..., 0], cs[..., 0]), pc.rec("folded b: merge against sweep", cm[..., 1], cs[..., 1])]
    report(out)


def test_backward_records_of_64_pixel_tiles_and_the_fused_skip_dgrad_behind_them():
    from cgd_amd import lib as L
    from cgd_amd import ops
    ctx = context()
    lib = ctx.lib
    Cn, K = 128, 64
    gen = pc.g(7802)
    ctx.check(lib.cgd_op_new_pass(ctx.h))
    xn = (1000.0 + th.randn(RB, RHW, Cn, generator=gen)).to(pc.DEV)  # the norm's input, |mean| / sigma = 1e3
    _, scr, gamma, beta = gn_fwd(ctx, xn, Cn)
    # dz = a dgrad conv's output: dy has RCI channels, torch weight [RCI][Cn]
    wt = (th.randn(RCI, Cn, 3, 3, generator=gen) / math.sqrt(9 * RCI)).to(pc.DEV)
    dy = th.randn(RB, RH, RW, RCI, generator=gen).to(pc.DEV)
    dz = conv_ex(ctx, dy, ops.pack_conv3x3(wt)[1].to(pc.DEV), ops.pack_conv3x3_frag(ctx, wt, dgrad=True), RB, RH, RW, RCI, Cn,
                 gnb=(xn, Cn, scr)).reshape(RB, RHW, Cn)
    recs, pix = peek(ctx, dz, Cn, 1)
    assert pix == 64
    # float64 sums from the tensors as stored and the float32 table the kernel read
    coef = coef_table(ctx, scr, Cn).double().cpu()  # {a, b, gcoef, mean}
    xd, dzd = xn.double().cpu(), dz.double().cpu()
    u = xd * coef[:, None, :, 0] + coef[:, None, :, 1]
    sg = th.sigmoid(u)
    du = dzd * sg * (1 + u * (1 - sg))
    q1 = tiles64(du * coef[:, None, :, 2]).sum(1)
    q2 = tiles64(du * (xd - coef[:, None, :, 3]) * coef[:, None, :, 2]).sum(1)
    s1, s2 = 1.0 / q1.abs().max().item(), 1.0 / q2.abs().max().item()  # unit peak: the sums are linear in dz
    out = [pc.rec("records bwd: gcoef sum du (unit peak)", recs[..., 0] * s1, q1 * s1), pc.rec("records bwd: gcoef sum du (x - mean) (unit peak)", recs[..., 1] * s2, q2 * s2)]
    # the norm's backward merges them; the sweep path on the same tensors agrees
    xr, yref = ref_fwd(xn, gamma, beta)
    (gref,) = th.autograd.grad((yref * dzd).sum(), xr)
    sd = pc.unit_seed(gref)
    m0 = int(lib.cgd_op_gn_record_merges(ctx.h))
    dx = th.empty(RB, RHW, Cn, device=pc.DEV)
    ctx.check(lib.cgd_op_gn_bwd(ctx.h, xn.data_ptr(), Cn, dz.data_ptr(), Cn, dx.data_ptr(), Cn, None, 0, RB, RHW, Cn, 1, scr.data_ptr(), L.stream_ptr()))
    assert int(lib.cgd_op_gn_record_merges(ctx.h)) == m0 + 1, "the GroupNorm backward did not merge the 64-pixel records"
    out.append(pc.rec("merge: dx (unit peak)", dx * sd, (gref * sd).float()))
    # the fused skip dgrad (weight GEMM + this norm's backward in its epilogue) on the tables the merge just folded, against the two launches
    off = int(lib.cgd_op_gn_stats_offset(RB, RHW, Cn)) + RB * 64
    bcoef = scr[off + RB * Cn * 4:off + 2 * RB * Cn * 4].reshape(RB, Cn, 4).clone()
    a = (th.randn(RB, RHW, K, generator=gen) / sd).to(pc.DEV)  # gradient-sized, like dz
    w = (th.randn(Cn, K, generator=gen) / K ** 0.5).to(pc.DEV)
    fused = ops.gemm_gn_bwd(ctx, a, w, xn, dz, coef_table(ctx, scr, Cn), bcoef)
    ctx.check(lib.cgd_op_new_pass(ctx.h))
    t = ops.gemm(ctx, a.reshape(RB * RHW, K), w, force_tile=513).reshape(RB, RHW, Cn)
    two = ops.groupnorm_bwd(ctx, xn, dz, scr, act=1, add=t)
    assert int(lib.cgd_op_gn_record_merges(ctx.h)) == m0 + 1  # (a later pass: the sweep path)
    ref2 = gref + a.double().cpu() @ w.double().cpu().t()
    sd2 = pc.unit_seed(ref2)
    out += [pc.rec("fused skip dgrad behind 64-pixel records (unit peak)", fused * sd2, (ref2 * sd2).float()),
            pc.rec("the two launches, sweep path (unit peak)", two * sd2, (ref2 * sd2).float())]
    report(out)
