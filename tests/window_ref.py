"""Reference of windowed sampling (cgd_window_gather / cgd_window_merge, nets.WindowedUNet), written from the formulas of
include/cgd_mi355x.h in plain torch indexing, independently of cgd_amd/windows.py:

  gather  win[b,k,c,u,v]   = ay[ky][u] ax[kx][v] full[b,c,(oy[ky]+u) mod H,(ox[kx]+v) mod W]          k = ky nx + kx
  merge   full[b,c,y,x] (+)= sum over the windows that cover (y,x) of ay[ky][u] ax[kx][v] win[b,k,c,u,v]

`gather` / `merge` keep the dtype of their input (the fp64 restatement when handed fp64, an autograd-capable fp32 graph inside
`WindowedRef`); `origins` and `tables` restate the planner's two rules with explicit loops; `WindowedRef` is the torch module around any
UNet module that the oracle loops take in the model's place."""
import math

import torch as th


def origins(L, S, stride, wrap=False):
    """without wrap 0, stride, ... while o + S < L, then L - S; with wrap 0, stride, ... < L (L % stride == 0)"""
    if wrap:
        assert L % stride == 0
        return list(range(0, L, stride))
    out, o = [], 0
    while o + S < L:
        out.append(o)
        o += stride
    return out + [L - S]


def profile(S, name):
    assert name in ("uniform", "feather")
    return [1.0 if name == "uniform" else math.sin(math.pi * (u + 0.5) / S) ** 2 for u in range(S)]


def tables(orig, L, S, name="uniform"):
    """(n, S) fp64: a[k][u] = w(u) / sum_j w((o_k + u - o_j) mod L) over the windows j whose offset (o_k + u - o_j) mod L is below S"""
    w = profile(S, name)
    a = th.zeros(len(orig), S, dtype=th.float64)
    for k, ok in enumerate(orig):
        for u in range(S):
            total = sum(w[(ok + u - oj) % L] for oj in orig if (ok + u - oj) % L < S)
            a[k, u] = w[u] / total
    return a


def _index(o, S, L):
    return (o + th.arange(S)) % L


def gather(full, oy, ox, S, ay=None, ax=None):
    """(B,C,H,W) -> (B * ny * nx, C, S, S); ay (ny,S), ax (nx,S) or None (ones)"""
    B, C, H, W = full.shape
    wins = []
    for ky, o_y in enumerate(oy):
        rows = _index(o_y, S, H)
        for kx, o_x in enumerate(ox):
            cols = _index(o_x, S, W)
            w = full[:, :, rows[:, None], cols[None, :]]
            if ay is not None:
                w = w * (ay[ky].to(full.dtype)[:, None] * ax[kx].to(full.dtype)[None, :])
            wins.append(w)
    return th.stack(wins, 1).reshape(B * len(oy) * len(ox), C, S, S)


def merge(win, oy, ox, H, W, ay=None, ax=None, base=None):
    """(B * ny * nx, C, S, S) -> (B,C,H,W), added to `base` when given.  Inside one window every (row, column) pair occurs once (S <= H, W),
    so the indexed add below has no duplicate targets."""
    n = len(oy) * len(ox)
    S, C = win.shape[-1], win.shape[1]
    B = win.shape[0] // n
    win = win.reshape(B, n, C, S, S)
    out = th.zeros(B, C, H, W, dtype=win.dtype)
    for ky, o_y in enumerate(oy):
        rows = _index(o_y, S, H)
        for kx, o_x in enumerate(ox):
            cols = _index(o_x, S, W)
            w = win[:, ky * len(ox) + kx]
            if ay is not None:
                w = w * (ay[ky].to(win.dtype)[:, None] * ax[kx].to(win.dtype)[None, :])
            canvas = th.zeros_like(out)
            canvas[:, :, rows[:, None], cols[None, :]] = w
            out = out + canvas
    return out if base is None else base + out


class WindowedRef(th.nn.Module):
    """model(x, ts, y) on overlapping S x S windows of x, the window outputs averaged with the normalised weights: what nets.WindowedUNet
    computes, as a differentiable torch module around `unet` (any module called as unet(x, ts, y))."""

    def __init__(self, unet, S, stride, wrap="", feather=False):
        super().__init__()
        assert wrap in ("", "x", "y", "xy")
        self.unet, self.S, self.stride, self.wrap, self.name = unet, S, stride, wrap, ("feather" if feather else "uniform")
        self.num_classes = getattr(unet, "num_classes", None)

    def plan(self, H, W):
        oy, ox = origins(H, self.S, self.stride, "y" in self.wrap), origins(W, self.S, self.stride, "x" in self.wrap)
        return oy, ox, tables(oy, H, self.S, self.name), tables(ox, W, self.S, self.name)

    def forward(self, x, ts, y=None):
        H, W = x.shape[2:]
        oy, ox, ay, ax = self.plan(H, W)
        n = len(oy) * len(ox)
        xw = gather(x, oy, ox, self.S)
        out = self.unet(xw, ts.repeat_interleave(n), None if y is None else y.repeat_interleave(n))
        return merge(out, oy, ox, H, W, ay, ax)
