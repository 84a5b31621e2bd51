"""Host planner of windowed sampling (MultiDiffusion, Bar-Tal et al., 2023): where the windows of a frame sit and with which weights their
outputs are averaged.  No GPU needed; the kernels that use a plan are cgd_window_gather / cgd_window_merge (csrc/window.hip), the model
wrapper is nets.WindowedUNet.

A plan is per axis: `window_origins` places windows of side S along an axis of length L, `window_tables` gives every window its normalised
weights along that axis.  The 2-D window grid is the outer product of the two axes and the 2-D weight of a pixel in a window the product
of its two axis weights; because the normaliser factorises per axis, those products sum to 1 at every pixel of the frame.
"""
import math

import torch as th

MAX_WINDOWS = 16  # per axis: the origins travel in the kernel arguments
PROFILES = ("uniform", "feather")
WRAPS = {"": 0, "x": 1, "y": 2, "xy": 3}  # the kernels' wrap bits: bit 0 the right edge, bit 1 the bottom edge


def window_origins(L, S, stride, wrap=False):
    """Origins of the windows of side S along an axis of length L.  Without wrap: 0, stride, ... while o + S < L, then L - S: the last window
    sits flush with the edge.  With wrap: 0, stride, ... < L, which needs L % stride == 0; windows run over the edge and continue at 0, and
    L == S is allowed (the windows are then rolled copies of the whole axis, which is what makes the axis tile)."""
    for name, v in (("L", L), ("S", S), ("stride", stride)):
        if isinstance(v, bool) or not isinstance(v, int) or v <= 0 or v % 8:
            raise ValueError(f"windows: {name} must be a positive multiple of 8, got {v!r}")
    if S > L:
        raise ValueError(f"windows: the window side {S} exceeds the axis length {L}")
    if stride > S:
        raise ValueError(f"windows: a stride of {stride} leaves gaps between windows of side {S}")
    if wrap:
        if L % stride:
            raise ValueError(f"windows: a wrapping axis of length {L} needs a stride that divides it, got {stride}")
        origins = list(range(0, L, stride))
    else:
        origins, o = [], 0
        while o + S < L:
            origins.append(o)
            o += stride
        origins.append(L - S)
    if len(origins) > MAX_WINDOWS:
        raise ValueError(f"windows: {len(origins)} windows along an axis of length {L} (at most {MAX_WINDOWS}): use a larger stride")
    return origins


def profile_weights(S, profile="uniform"):
    """w(u), u = 0 .. S-1, in fp64: 'uniform' is 1 (MultiDiffusion's plain average), 'feather' is sin^2(pi (u + 0.5) / S), strictly positive."""
    if profile not in PROFILES:
        raise ValueError(f"windows: the profile must be one of {PROFILES}, got {profile!r}")
    if profile == "uniform":
        return th.ones(S, dtype=th.float64)
    return th.sin(math.pi * (th.arange(S, dtype=th.float64) + 0.5) / S) ** 2


def window_tables(origins, L, S, profile="uniform"):
    """(n, S) fp32 table a[k][u] = w(u) / sum_j w((o_k + u - o_j) mod L), the sum over the windows j that include pixel (o_k + u) mod L, i.e.
    whose offset (o_k + u - o_j) mod L is below S.  Computed in fp64, stored as fp32.  Summed over the windows that cover a pixel the entries
    give 1."""
    w = profile_weights(S, profile)
    o = th.tensor(list(origins), dtype=th.int64)
    pix = (o[:, None] + th.arange(S)[None, :]) % L               # (n, S): the pixel under entry u of window k
    off = (pix[:, :, None] - o[None, None, :]) % L               # (n, S, n): that pixel's offset in window j
    inside = off < S
    total = (w[off.clamp(max=S - 1)] * inside).sum(-1)           # (n, S)
    return (w[None, :] / total).to(th.float32)


class WindowPlan:
    """The windows of one (H, W) frame: origins per axis, wrap bits, and the per-axis weight tables (host fp32; `to(device)` uploads them)."""

    def __init__(self, H, W, S, stride, wrap="", feather=False):
        if wrap not in WRAPS:
            raise ValueError(f"windows: wrap must be one of {sorted(WRAPS)}, got {wrap!r}")
        self.H, self.W, self.S, self.stride = H, W, S, stride
        self.wrap = WRAPS[wrap]
        self.profile = "feather" if feather else "uniform"
        self.oy = window_origins(H, S, stride, bool(self.wrap & 2))
        self.ox = window_origins(W, S, stride, bool(self.wrap & 1))
        self.ny, self.nx = len(self.oy), len(self.ox)
        self.n = self.ny * self.nx
        self.ay = window_tables(self.oy, H, S, self.profile)
        self.ax = window_tables(self.ox, W, S, self.profile)

    def to(self, device):
        self.ay, self.ax = self.ay.to(device).contiguous(), self.ax.to(device).contiguous()
        return self
