"""Dense-matrix restatement of the antialiased cubic resize of the resized cutouts (csrc/cutresize.hip), in float64.

Per axis, a crop extent n resized to m (s = m / n):
    c_o    = ((2o+1) n - m) / (2m)                         centre of output o in input coordinates
    k(d)   = cubic(d), S = 4             for s >= 1
    k(d)   = s cubic(s d), S = 4n / m    for s <  1         (antialiasing)
    T      = ceil(S) taps j = left_o .. left_o + T - 1,  left_o = ceil(c_o - S / 2)
    w_oj   = k(c_o - j) / sum_j k(c_o - j)                  the sum over all T taps (a zero sum divides by 1)
Taps outside [0, n) read zero and the weights are not renormalised over the taps inside; m == n is the identity.
The default mode takes c_o, left_o and T from exact rational arithmetic.  `reference_grid=True` forms the grid and the weights in float32 the way
torch evaluates `arange(m) / s + (n - 1) / 2 - (m - 1) / (2 s)` and what follows from it (ResizeRight's own arithmetic), which is what the fixture
tests/golden/reference_resize.npz was produced with.
"""
import math
from fractions import Fraction

import numpy as np
import torch as th

LUMA = (0.2989, 0.587, 0.114)


def cubic(d):
    a = np.abs(np.asarray(d, dtype=np.float64))
    inner = 1.5 * a ** 3 - 2.5 * a ** 2 + 1.0
    outer = -0.5 * a ** 3 + 2.5 * a ** 2 - 4.0 * a + 2.0
    return np.where(a <= 1.0, inner, np.where(a <= 2.0, outer, 0.0))


def taps_exact(n, m):
    """(left [m] int64, T, weights [m, T] float64) from exact geometry."""
    s = Fraction(m, n)
    S = Fraction(4) if s >= 1 else Fraction(4 * n, m)
    T = math.ceil(S)
    left = np.empty(m, np.int64)
    w = np.empty((m, T), np.float64)
    for o in range(m):
        c = Fraction((2 * o + 1) * n - m, 2 * m)
        left[o] = math.ceil(c - S / 2)
        d = np.array([float(c - (int(left[o]) + t)) for t in range(T)])
        k = cubic(d) if s >= 1 else float(s) * cubic(float(s) * d)
        tot = k.sum()
        w[o] = k / (tot if tot != 0 else 1.0)
    return left, T, w


def taps_reference_grid(n, m):
    """The same three, with the grid, the field of view and the weights in float32 as torch forms them."""
    s = float(m / n)
    eps = th.finfo(th.float32).eps
    grid = th.arange(m) / s + (n - 1) / 2 - (m - 1) / (2 * s)
    S = 4 if s >= 1.0 else 4 / s
    left = (grid - S / 2 - eps).ceil().long()
    T = math.ceil(S - eps)
    fov = left[:, None] + th.arange(T)
    pad = -int(fov[0, 0])  # the padded input's coordinates: both shift by the left padding
    fov = fov + pad
    grid = grid + pad
    d = grid[:, None] - fov

    def cub(x):
        a = th.abs(x)
        a2, a3 = a ** 2, a ** 3
        return ((1.5 * a3 - 2.5 * a2 + 1.) * (a <= 1.).to(x.dtype) + (-0.5 * a3 + 2.5 * a2 - 4. * a + 2.) * ((1. < a) & (a <= 2.)).to(x.dtype))

    k = cub(d) if s >= 1.0 else s * cub(s * d)
    tot = k.sum(1, keepdim=True)
    tot[tot == 0] = 1
    w = k / tot
    return left.numpy(), T, w.double().numpy()


def matrix(n, m, reference_grid=False):
    """Dense (m, n) float64 resize matrix (the taps outside [0, n) dropped: they read zero)."""
    if m == n:
        return np.eye(n)
    left, T, w = (taps_reference_grid if reference_grid else taps_exact)(n, m)
    M = np.zeros((m, n), np.float64)
    for o in range(m):
        for t in range(T):
            j = int(left[o]) + t
            if 0 <= j < n:
                M[o, j] += w[o, t]
    return M


def resize(x, mh, mw, reference_grid=False):
    """x (..., h, w) torch tensor -> (..., mh, mw): Wy x Wx^T in x's dtype (differentiable)."""
    Wy = th.as_tensor(matrix(x.shape[-2], mh, reference_grid), dtype=x.dtype, device=x.device)
    Wx = th.as_tensor(matrix(x.shape[-1], mw, reference_grid), dtype=x.dtype, device=x.device)
    return Wy @ x @ Wx.t()


def grayscale(z):
    g = LUMA[0] * z[:, 0:1] + LUMA[1] * z[:, 1:2] + LUMA[2] * z[:, 2:3]
    return g.expand(-1, 3, -1, -1)


def cutouts(x01, records, cs):
    """The resized cutouts of x01 (B,3,H,W in [0,1]) for (ox, oy, w, h, flags) records: (len(records) * B, 3, cs, cs), row k * B + b, not
    normalised.  flags bit 0: grayscale before the resize; bit 1: flip along W after it."""
    outs = []
    for ox, oy, w, h, fl in records:
        z = x01[:, :, oy:oy + h, ox:ox + w]
        if fl & 1:
            z = grayscale(z)
        r = resize(z, cs, cs)
        if fl & 2:
            r = r.flip(-1)
        outs.append(r)
    return th.cat(outs)
