"""Float64 restatement of the conditioned stem of the super-resolution UNets (csrc/superres.hip):
    y = conv2d(cat([x, bilinear(low -> H x W)], 1), weight, bias, padding=1)
The bilinear operator is F.interpolate(mode="bilinear", align_corners=False), stated per axis as a matrix built from exact integer
geometry (python ints and Fractions): for an extent n_in resized to n_out,
    src_d = max(((2d+1) n_in - n_out) / (2 n_out), 0),  i0 = floor(src_d),  i1 = i0 + (i0 < n_in - 1),  weights 1 - (src_d - i0), src_d - i0.
Zero padding belongs to the concatenated tensor (conv2d's padding): the interpolation itself clamps at the low-res border."""
from fractions import Fraction

import torch as th
import torch.nn.functional as F


def axis_matrix(n_in, n_out):
    """(n_out, n_in) float64 matrix of the per-axis operator"""
    m = th.zeros(n_out, n_in, dtype=th.float64)
    for d in range(n_out):
        src = max(Fraction((2 * d + 1) * n_in - n_out, 2 * n_out), Fraction(0))
        i0 = src.numerator // src.denominator
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        f = float(src - i0)
        m[d, i0] += 1.0 - f
        m[d, i1] += f
    return m


def bilinear(low, H, W):
    """low (N,3,h,w) -> (N,3,H,W) in float64"""
    low = low.double()
    return th.einsum("yh,nchw,xw->ncyx", axis_matrix(low.shape[2], H), low, axis_matrix(low.shape[3], W))


def sr_input(x, low):
    """cat([x, bilinear(low)], 1) in float64; a low of batch 1 is shared by the batch of x"""
    B, _, H, W = x.shape
    up = bilinear(low, H, W)
    if up.shape[0] == 1 and B > 1:
        up = up.expand(B, -1, -1, -1)
    return th.cat([x.double(), up], 1)


def sr_stem(x, low, weight, bias=None):
    """x (B,3,H,W), low (1 or B,3,h,w), weight (Cout,6,3,3), bias (Cout) -> (B,H,W,Cout) NHWC float64"""
    y = F.conv2d(sr_input(x, low), weight.double(), None if bias is None else bias.double(), padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def sr_stem_torch32(x, low, weight, bias=None):
    """the float32 composition upstream runs: F.interpolate + cat + conv2d -> NHWC"""
    B, _, H, W = x.shape
    up = F.interpolate(low.float(), (H, W), mode="bilinear")
    if up.shape[0] == 1 and B > 1:
        up = up.expand(B, -1, -1, -1)
    y = F.conv2d(th.cat([x.float(), up], 1), weight.float(), None if bias is None else bias.float(), padding=1)
    return y.permute(0, 2, 3, 1).contiguous()
