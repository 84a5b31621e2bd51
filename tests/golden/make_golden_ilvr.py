"""Generates tests/golden/reference_ilvr.npz: ILVR's low-pass phi_N, the reference's vendored ResizeRight (cubic, antialiasing,
pad_mode='constant') called down by 1/N and back up by N, as the authors of ILVR call it.  ResizeRight is loaded as
tests/golden/make_golden_resize.py loads it.

    python tests/golden/make_golden_ilvr.py REFERENCE_ROOT      (or $CGD_REFERENCE: the checkout of the reference project)

Fixture: float64 inputs x_<H>x<W>_<N> (2,3,H,W) on a 1/128 grid in [-1,1] and y_<H>x<W>_<N> = resize(resize(x, 1/N), N) for the cases
(H, W, N) = (32,32,2), (32,32,8), (24,40,4), (64,64,32) (low resolution 2x2) and (16,16,16) (low resolution 1x1).
"""
import os
import sys

import numpy as np
import torch as th

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_resize import load_resize_right  # noqa: E402

CASES = [(32, 32, 2), (32, 32, 8), (24, 40, 4), (64, 64, 32), (16, 16, 16)]


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ["CGD_REFERENCE"]
    rr, im = load_resize_right(root)
    gen = th.Generator().manual_seed(20211208)
    kw = dict(interp_method=im.cubic, antialiasing=True, pad_mode="constant")
    fx = {}
    for H, W, N in CASES:
        x = th.randint(-128, 129, (2, 3, H, W), generator=gen).double() / 128
        low = rr.resize(x, scale_factors=1.0 / N, **kw)
        assert tuple(low.shape) == (2, 3, H // N, W // N)
        y = rr.resize(low, scale_factors=float(N), **kw)
        assert tuple(y.shape) == (2, 3, H, W) and y.dtype == th.float64
        fx[f"x_{H}x{W}_{N}"], fx[f"y_{H}x{W}_{N}"] = x.numpy(), y.numpy()
    path = os.path.join(OUT, "reference_ilvr.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
