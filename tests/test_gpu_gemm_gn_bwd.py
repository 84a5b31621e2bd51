"""The weight GEMM whose epilogue applies a GroupNorm + SiLU backward (ops.gemm_gn_bwd / cgd_op_gemm_gn_bwd: a ResBlock's 1x1 skip dgrad and
GN1's backward in one launch) against a float64 reference, at the suite's literal bound |a - b| <= 1e-4 + 1e-3 |ref| per element, and against
the two launches it replaces (ops.gemm + ops.groupnorm_bwd(add=...)), which must meet the same bound.  The test builds the per-(sample, channel)
tables itself in float64.  Inputs are in trained-network ranges: every other group sits at |mean| = 100 sigma (value_regime_checks.GN_MEAN).

Shapes: M = 680 rows in one sample (five full 128-row tiles and a ragged sixth) and two samples of 256 rows (the table of the second sample);
K in {64, 320} (one 64-deep chunk, an odd number of chunks); C in {64, 96, 512} (2, 3 and 16 channels per group; 96 = a ragged 128-column
panel, 512 = four panels); `add` present and absent; x, dz, add, the GEMM's A and the output as channel slices of wider buffers."""
import functools

import pytest
import torch as th
import torch.nn.functional as F

from tests import parity_checks as pc
from tests.value_regime_checks import GN_MEAN, frac

pytestmark = pytest.mark.gpu

CASES = [(1, 680, C, K, add) for C in (64, 96, 512) for K in (64, 320) for add in (False, True)] + [(2, 256, 96, 64, True)]


@functools.lru_cache(maxsize=None)
def case(B, HW, C, K, add):
    gen = pc.g(9100 + C + K)
    cpg = C // 32
    x = th.randn(B, HW, C, generator=gen) + 0.5
    grp_mean = th.zeros(32)
    grp_mean[0::2] = GN_MEAN * th.tensor([1.0, -1.0] * 8)  # every other group far from zero, ordinary groups beside them
    x = x + grp_mean.repeat_interleave(cpg)
    gamma = 1 + 0.1 * th.randn(C, generator=gen)
    beta = 0.1 * th.randn(C, generator=gen)
    dz = th.randn(B, HW, C, generator=gen)
    dout = th.randn(B, HW, K, generator=gen)
    w = th.randn(C, K, generator=gen) / K ** 0.5
    skip = th.randn(B, HW, C, generator=gen) if add else None
    # float64 reference: autograd through GroupNorm + SiLU, plus the GEMM and the addend
    xr = x.double().requires_grad_()
    y = F.silu(F.group_norm(xr.permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-5)).permute(0, 2, 1)
    (gn,) = th.autograd.grad((y * dz.double()).sum(), xr)
    ref = gn + dout.double() @ w.double().t() + (skip.double() if add else 0.0)
    sd = pc.unit_seed(ref)  # the backward is linear in (dz, dout, skip): unit peak, so that atol counts in units of the gradient's peak
    # the tables, float64: coef {a, b, gcoef, mean}, bcoef {rstd gcoef, rstd^3 p2 / N, rstd p1 / N, 0} with the sums over the SCALED upstream gradient
    xd = x.double()
    xg = xd.reshape(B, HW, 32, cpg)
    mean = xg.mean((1, 3))
    rstd = 1.0 / (xg.var((1, 3), unbiased=False) + 1e-5).sqrt()
    mean_c, rstd_c = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)  # [B, C]
    a = rstd_c * gamma.double()
    b = beta.double() - mean_c * a
    u = xd * a[:, None] + b[:, None]
    sg = th.sigmoid(u)
    du = dz.double() * sd * (sg * (1 + u * (1 - sg))) * gamma.double()
    n = HW * cpg
    p1 = du.reshape(B, HW, 32, cpg).sum((1, 3))
    p2 = (du * (xd - mean_c[:, None])).reshape(B, HW, 32, cpg).sum((1, 3))
    coef = th.stack([a, b, gamma.double().expand(B, C), mean_c], -1)
    bcoef = th.stack([rstd_c * gamma.double(), (rstd ** 3 * p2 / n).repeat_interleave(cpg, 1), (rstd * p1 / n).repeat_interleave(cpg, 1),
                      th.zeros(B, C, dtype=th.float64)], -1)
    return dict(x=x, gamma=gamma, beta=beta, dz=dz * sd, dout=dout * sd, w=w, skip=None if skip is None else skip * sd, ref=(ref * sd).float(),
                coef=coef.float().contiguous(), bcoef=bcoef.float().contiguous())


def sliced(t, pad_l, pad_r):
    """t as a channel slice of a wider (NaN-filled) device buffer"""
    B, HW, C = t.shape
    buf = th.full((B, HW, pad_l + C + pad_r), float("nan"), device=pc.DEV)
    buf[..., pad_l:pad_l + C] = t.to(pc.DEV)
    return buf[..., pad_l:pad_l + C]


@pytest.mark.parametrize("B,HW,C,K,add", CASES)
def test_fused_epilogue_matches_float64_and_the_two_launches(B, HW, C, K, add):
    from cgd_amd import ops
    c = case(B, HW, C, K, add)
    ctx = pc._ctx(1)
    x, dz, dout = sliced(c["x"], 32, 8), sliced(c["dz"], 4, 12), sliced(c["dout"], 8, 4)
    skip = sliced(c["skip"], 16, 4) if add else None
    w = c["w"].to(pc.DEV)
    outbuf = th.full((B, HW, C + 24), float("nan"), device=pc.DEV)
    out = outbuf[..., 8:8 + C]
    ops.gemm_gn_bwd(ctx, dout, w, x, dz, c["coef"].to(pc.DEV), c["bcoef"].to(pc.DEV), add=skip, out=out)
    # the two launches: the GEMM (weight GEMM kernel, + skip as its residual), then the norm's backward with that as `add`
    _, scr = ops.groupnorm_fwd(ctx, x, c["gamma"].to(pc.DEV), c["beta"].to(pc.DEV), act=1)
    t = ops.gemm(ctx, dout.reshape(B * HW, K), w, R=None if skip is None else skip.reshape(B * HW, C), force_tile=513).reshape(B, HW, C)
    two = ops.groupnorm_bwd(ctx, x, dz, scr, act=1, add=t)
    th.cuda.synchronize()
    r1 = pc.rec(f"gemm_gn_bwd B{B} HW{HW} C{C} K{K} add{int(add)} fused", out, c["ref"])
    r2 = pc.rec(f"gemm_gn_bwd B{B} HW{HW} C{C} K{K} add{int(add)} two launches", two, c["ref"])
    print(f"fused {frac(out.cpu(), c['ref']):.3f} of the bound (abs {r1['err_abs']:.3e}); two launches {frac(two.cpu(), c['ref']):.3f} (abs {r2['err_abs']:.3e}); "
          f"fused vs two launches max |diff| {(out - two).abs().max().item():.3e}")
    assert th.isnan(outbuf[..., :8]).all() and th.isnan(outbuf[..., 8 + C:]).all(), "the fused launch wrote outside its channel slice"
    assert r1["ok"], r1
    assert r2["ok"], r2


def test_op_entry_refuses_what_the_kernel_cannot_run():
    from cgd_amd import ops
    c = case(1, 680, 64, 64, False)
    dev = {k: v.to(pc.DEV) for k, v in c.items() if isinstance(v, th.Tensor)}
    with pytest.raises(RuntimeError):  # exact-fp32 context
        ops.gemm_gn_bwd(pc._ctx(0), dev["dout"], dev["w"], dev["x"], dev["dz"], dev["coef"], dev["bcoef"])
    ctx = pc._ctx(1)
    odd = th.zeros(1, 680, 66, device=pc.DEV)[..., 1:65]  # row stride 66, pointer 4 bytes off a 16-byte boundary
    odd.copy_(dev["x"])
    with pytest.raises(RuntimeError):
        ops.gemm_gn_bwd(ctx, dev["dout"], dev["w"], odd, dev["dz"], dev["coef"], dev["bcoef"])
    with pytest.raises(RuntimeError):  # two samples of 340 rows: a 128-row tile would straddle them
        ops.gemm_gn_bwd(ctx, dev["dout"].reshape(2, 340, 64), dev["w"], dev["x"].reshape(2, 340, 64), dev["dz"].reshape(2, 340, 64),
                        dev["coef"].expand(2, 64, 4).contiguous(), dev["bcoef"].expand(2, 64, 4).contiguous())
