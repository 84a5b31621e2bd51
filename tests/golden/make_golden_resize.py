"""Generates tests/golden/reference_resize.npz by running the reference's vendored ResizeRight (cubic, antialiasing, pad_mode='constant') on
the CPU.  The two ResizeRight modules are loaded by file path under the names they import each other by; the reference package itself is not
imported.

    python tests/golden/make_golden_resize.py REFERENCE_ROOT      (or $CGD_REFERENCE: the checkout of the reference project)

Fixture: float64 inputs x_<case> (2,3,h,w) in [-1,1] and ResizeRight's outputs y_<case> for the (n -> m) cases 40->16, 23->16, 9->16,
16->16, 17->32, 37->32 and the non-square 24x40 -> 16x16, plus for 23->16 the cotangent d_23_16 and the autograd gradient g_23_16 of
(y * d).sum() with respect to x.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch as th

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = [("40_16", 40, 40, 16), ("23_16", 23, 23, 16), ("9_16", 9, 9, 16), ("16_16", 16, 16, 16), ("17_32", 17, 17, 32), ("37_32", 37, 37, 32),
         ("24x40_16", 24, 40, 16)]


def load_resize_right(root):
    d = os.path.join(root, "cgd", "ResizeRight")
    saved = {k: sys.modules.get(k) for k in ("cgd", "cgd.ResizeRight", "cgd.ResizeRight.interp_methods")}
    try:
        pkg, sub = types.ModuleType("cgd"), types.ModuleType("cgd.ResizeRight")
        pkg.__path__, sub.__path__ = [], []
        sys.modules["cgd"], sys.modules["cgd.ResizeRight"] = pkg, sub
        mods = {}
        for name in ("interp_methods", "resize_right"):
            spec = importlib.util.spec_from_file_location(f"cgd.ResizeRight.{name}", os.path.join(d, f"{name}.py"))
            mods[name] = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mods[name]
            spec.loader.exec_module(mods[name])
            setattr(sub, name, mods[name])
        return mods["resize_right"], mods["interp_methods"]
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        sys.modules.pop("cgd.ResizeRight.resize_right", None)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ["CGD_REFERENCE"]
    rr, im = load_resize_right(root)
    gen = th.Generator().manual_seed(20240611)
    fx = {}
    for name, h, w, m in CASES:
        x = th.randint(-128, 129, (2, 3, h, w), generator=gen).double() / 128  # on a 1/128 grid: the archive stays small
        x.requires_grad_(name == "23_16")
        y = rr.resize(x, out_shape=(m, m), interp_method=im.cubic, antialiasing=True, pad_mode="constant")
        assert tuple(y.shape) == (2, 3, m, m) and y.dtype == th.float64
        fx[f"x_{name}"], fx[f"y_{name}"] = x.detach().numpy(), y.detach().numpy()
        if name == "23_16":
            d = th.randint(-256, 257, tuple(y.shape), generator=gen).double() / 64
            g, = th.autograd.grad((y * d).sum(), x)
            fx["d_23_16"], fx["g_23_16"] = d.numpy(), g.numpy()
    path = os.path.join(OUT, "reference_resize.npz")
    np.savez_compressed(path, **fx)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
