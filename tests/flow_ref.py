"""float64 restatement of csrc/flow.hip for the tests: dense pyramidal Lucas-Kanade flow in the PATCH form (each pixel moves its whole
window by its own flow) and the warp that follows a flow (include/cgd_mi355x.h: cgd_flow_estimate, cgd_op_flow_level, cgd_frame_warp_flow).
Plain torch on the CPU.  The pyramid is the edge-replicating antialiased cubic resize of tests/resize_ref.py (through depth_ref.resize_edge,
the reference of cgd_op_resize_cubic); the sampling uses the border rule and the cubic weights of tests/warp_ref.py.

    flow        (B, 2, H, W), channel 0 the x displacement in pixels, channel 1 the y displacement; estimate(tmpl, img) returns F with
                img(p + F(p)) ~ tmpl(p); pixel centres sit on integers
    luminance   C == 3: 0.2989 R + 0.587 G + 0.114 B; C == 1: the plane
    pyramid     level l + 1 = resize of level l to (ceil(H_l / 2), ceil(W_l / 2)); levels(): the largest L <= levels whose coarsest level has
                a shorter side of at least 2 radius + 1, at least 1
    a level     the coarsest starts from zero; a finer one reads the coarser flow bilinearly (replicate border) at
                ((x + 0.5) Wc / Wf - 0.5, (y + 0.5) Hc / Hf - 0.5) and scales it by Wf / Wc (x) and Hf / Hc (y)
    iteration   over the window q = p + (dx, dy), |dx|, |dy| <= radius, q inside the frame, ascending dy then dx: bx, by the central differences
                of the template divided by 2 (replicate border); s = q + u counts when 0 <= sx <= W - 1 and 0 <= sy <= H - 1 and contributes
                to nothing otherwise; a(s) bilinear; e = b(q) - a(s); Gxx = lambda + sum bx^2, Gyy = lambda + sum by^2, Gxy = sum bx by,
                rx = sum bx e, ry = sum by e; det = Gxx Gyy - Gxy^2; du = (Gyy rx - Gxy ry) / det, dv = (Gxx ry - Gxy rx) / det; a non-finite
                step is zero, a step longer than max_step is scaled to that length; u += (du, dv)
The flow is rounded to fp32 wherever the kernel stores it: at the start of a level (the value read from the coarser level) and at its end.
`dtype=torch.float32` is the float32 restatement the GPU tests use to choose their inputs: the planes, the weights, the sums and the step
arithmetic are fp32, the coordinates and the validity test stay fp64, as in the kernel.  lambda, max_step, blend, alpha and beta are taken
as the fp32 numbers the C structures hold."""
import math

import numpy as np
import torch as th

from tests import depth_ref
from tests import warp_ref as R

DEFAULTS = dict(levels=4, iters=4, radius=4, lam=1e-3, max_step=1.0)


def f32(v):
    return float(np.float32(v))


def luminance(x):
    """(B, C, H, W) -> (B, H, W) float64"""
    x = x.detach().double().cpu()
    if x.shape[1] == 1:
        return x[:, 0].clone()
    if x.shape[1] != 3:
        raise ValueError(f"C must be 1 or 3, got {x.shape[1]}")
    return (f32(0.2989) * x[:, 0] + f32(0.587) * x[:, 1]) + f32(0.114) * x[:, 2]


def levels(H, W, levels, radius):
    L = 1
    for l in range(1, levels):
        H, W = (H + 1) // 2, (W + 1) // 2
        if min(H, W) < 2 * radius + 1:
            break
        L = l + 1
    return L


def scratch_floats(B, H, W, levels_, radius):
    n = 0
    for l in range(levels(H, W, levels_, radius)):
        n += 2 * B * H * W * (1 if l == 0 else 2)
        H, W = (H + 1) // 2, (W + 1) // 2
    return n


def pyramid(y, L):
    """y (B, H, W) float64 -> [level 0 .. level L - 1]"""
    out = [y]
    for _ in range(1, L):
        h, w = out[-1].shape[-2:]
        out.append(depth_ref.resize_edge(out[-1], (h + 1) // 2, (w + 1) // 2))
    return out


def _gather(planes, iy, ix):
    """planes (B, H, W), iy / ix (B, H', W') long -> planes[b, iy, ix]"""
    B, _, W = planes.shape
    return planes.reshape(B, -1).gather(1, (iy * W + ix).reshape(B, -1)).reshape(iy.shape)


def bilinear_replicate(D, sx, sy):
    """D (B, H, W) float64 at the float64 positions (sx, sy) (B, H', W'), clamped into the frame"""
    _, H, W = D.shape
    px, py = sx.clamp(0, W - 1), sy.clamp(0, H - 1)
    fx, fy = px.floor(), py.floor()
    tx, ty = px - fx, py - fy
    x0, y0 = fx.long(), fy.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    a0 = (1 - tx) * _gather(D, y0, x0) + tx * _gather(D, y0, x1)
    a1 = (1 - tx) * _gather(D, y1, x0) + tx * _gather(D, y1, x1)
    return (1 - ty) * a0 + ty * a1


def _grid(B, H, W):
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float64), th.arange(W, dtype=th.float64), indexing="ij")
    return xs.expand(B, H, W), ys.expand(B, H, W)


def start_flow(coarse, H, W):
    """The coarser level's flow (B, 2, Hc, Wc) read at a (H, W) level: (B, 2, H, W) float32"""
    coarse = coarse.detach().double().cpu()
    B, _, Hc, Wc = coarse.shape
    xs, ys = _grid(B, H, W)
    cx, cy = (xs + 0.5) * Wc / W - 0.5, (ys + 0.5) * Hc / H - 0.5
    u = bilinear_replicate(coarse[:, 0], cx, cy) * (W / Wc)
    v = bilinear_replicate(coarse[:, 1], cx, cy) * (H / Hc)
    return th.stack([u, v], dim=1).float()


def level(b, a, coarse=None, iters=4, radius=4, lam=1e-3, max_step=1.0, dtype=th.float64):
    """One pyramid level: b, a (B, H, W) template and image planes, coarse None or (B, 2, Hc, Wc) -> the flow (B, 2, H, W) float32"""
    b, a = b.detach().cpu().to(dtype), a.detach().cpu().to(dtype)
    B, H, W = b.shape
    lam, max_step = f32(lam), f32(max_step)
    xs, ys = _grid(B, H, W)
    xi, yi = xs.long(), ys.long()
    flow = th.zeros(B, 2, H, W) if coarse is None else start_flow(coarse, H, W)
    u, v = flow[:, 0].to(dtype), flow[:, 1].to(dtype)
    bx = (_gather(b, yi, (xi + 1).clamp(max=W - 1)) - _gather(b, yi, (xi - 1).clamp(min=0))) / 2
    by = (_gather(b, (yi + 1).clamp(max=H - 1), xi) - _gather(b, (yi - 1).clamp(min=0), xi)) / 2
    zero = th.zeros((), dtype=dtype)
    for _ in range(iters):
        sxx, syy, sxy, rx, ry = (th.zeros(B, H, W, dtype=dtype) for _ in range(5))
        for dy in range(-radius, radius + 1):
            for dx in range(-radius, radius + 1):
                qx, qy = xi + dx, yi + dy
                sx, sy = qx.double() + u.double(), qy.double() + v.double()
                valid = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H) & (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
                qx, qy = qx.clamp(0, W - 1), qy.clamp(0, H - 1)
                sx, sy = th.where(valid, sx, zero.double()), th.where(valid, sy, zero.double())
                fx0, fy0 = sx.floor(), sy.floor()
                tx, ty = (sx - fx0).to(dtype), (sy - fy0).to(dtype)
                ix, iy = fx0.long(), fy0.long()
                ix1, iy1 = (ix + 1).clamp(max=W - 1), (iy + 1).clamp(max=H - 1)
                a0 = (1 - tx) * _gather(a, iy, ix) + tx * _gather(a, iy, ix1)
                a1 = (1 - tx) * _gather(a, iy1, ix) + tx * _gather(a, iy1, ix1)
                e = _gather(b, qy, qx) - ((1 - ty) * a0 + ty * a1)
                gx, gy = _gather(bx, qy, qx), _gather(by, qy, qx)
                sxx = sxx + th.where(valid, gx * gx, zero)
                syy = syy + th.where(valid, gy * gy, zero)
                sxy = sxy + th.where(valid, gx * gy, zero)
                rx = rx + th.where(valid, gx * e, zero)
                ry = ry + th.where(valid, gy * e, zero)
        gxx, gyy = lam + sxx, lam + syy
        det = gxx * gyy - sxy * sxy
        du, dv = (gyy * rx - sxy * ry) / det, (gxx * ry - sxy * rx) / det
        finite = th.isfinite(du) & th.isfinite(dv)
        du, dv = th.where(finite, du, zero), th.where(finite, dv, zero)
        length = (du * du + dv * dv).sqrt()
        scale = th.where(length > max_step, max_step / th.where(length > 0, length, th.ones_like(length)), th.ones_like(length))
        u, v = u + du * scale, v + dv * scale
    return th.stack([u, v], dim=1).float()


def estimate(tmpl, img, levels_=4, iters=4, radius=4, lam=1e-3, max_step=1.0, dtype=th.float64):
    """tmpl, img (B, C, H, W) -> F (B, 2, H, W) float32 with img(p + F(p)) ~ tmpl(p)"""
    yt, yi = luminance(tmpl), luminance(img)
    B, H, W = yt.shape
    L = levels(H, W, levels_, radius)
    pyr = pyramid(th.cat([yt, yi]).to(dtype).double(), L)  # one resize for both frames, as the kernel's one launch; fp32 planes in the fp32 restatement
    flow = None
    for l in range(L - 1, -1, -1):
        flow = level(pyr[l][:B], pyr[l][B:], flow, iters, radius, lam, max_step, dtype)
    return flow


def warp_flow(src, flow, flow_back=None, fallback=None, blend=1.0, alpha=0.01, beta=0.5, interp="bicubic", border="replicate", clamp=False):
    """-> (dst (B, C, H, W) float64, m (B, 1, H, W) float64, margin): dst = w S(p + F(p)) + (1 - w) fallback, w = blend m; `margin` is the
    smallest |lhs - rhs| of the forward-backward check over the pixels that reach it (inf without flow_back)"""
    src = src.detach().double().cpu()
    B, _, H, W = src.shape
    flow = flow.detach().double().cpu().expand(B, -1, -1, -1)
    blend, alpha, beta = f32(blend), f32(alpha), f32(beta)
    xs, ys = _grid(B, H, W)
    finite = th.isfinite(flow[:, 0]) & th.isfinite(flow[:, 1])
    Fx, Fy = th.where(finite, flow[:, 0], th.zeros(())), th.where(finite, flow[:, 1], th.zeros(()))
    Fx, Fy = Fx.double(), Fy.double()
    m = finite.double()
    sx, sy = xs + Fx, ys + Fy
    margin = math.inf
    if flow_back is not None:
        back = flow_back.detach().double().cpu().expand(B, -1, -1, -1)
        inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        bx, by = bilinear_replicate(back[:, 0], sx, sy), bilinear_replicate(back[:, 1], sx, sy)
        lhs = (Fx + bx) ** 2 + (Fy + by) ** 2
        rhs = alpha * ((Fx * Fx + Fy * Fy) + (bx * bx + by * by)) + beta
        ok = inside & th.isfinite(bx) & th.isfinite(by) & (lhs <= rhs)
        m = m * ok.double()
        reach = inside & finite & th.isfinite(bx) & th.isfinite(by)
        if bool(reach.any()):
            margin = float((lhs - rhs).abs()[reach].min())
    sx, sy = sx.clamp(-2.0 ** 30, 2.0 ** 30), sy.clamp(-2.0 ** 30, 2.0 ** 30)
    fx, fy = sx.floor(), sy.floor()
    tx, ty = sx - fx, sy - fy
    ix, iy = fx.long(), fy.long()
    if interp == "bilinear":
        offs, wx, wy = (0, 1), (1 - tx, tx), (1 - ty, ty)
    elif interp == "bicubic":
        offs, wx, wy = (-1, 0, 1, 2), R.cubic_weights(tx), R.cubic_weights(ty)
    else:
        raise ValueError(interp)
    out = th.zeros_like(src)
    for c in range(src.shape[1]):
        plane = src[:, c]
        acc = th.zeros(B, H, W, dtype=th.float64)
        for oy, w_y in zip(offs, wy):
            yy = R.border_index(iy + oy, H, border)
            row = th.zeros(B, H, W, dtype=th.float64)
            for ox, w_x in zip(offs, wx):
                row = row + w_x * _gather(plane, yy, R.border_index(ix + ox, W, border))
            acc = acc + w_y * row
        out[:, c] = acc
    if clamp:
        out = out.clamp(-1, 1)
    if fallback is not None:
        w = (blend * m)[:, None]
        out = w * out + (1 - w) * fallback.detach().double().cpu()
    return out, m[:, None], margin


# ---- analytic test scenes ---------------------------------------------------------------------------------------------------------------
def texture(xs, ys, seed=0, terms=24, max_freq=0.8):
    """A sum of `terms` sinusoids with frequencies up to `max_freq` rad / px, evaluated exactly at any float64 positions; values in about
    [-1, 1]"""
    g = th.Generator().manual_seed(1000 + seed)
    freq = th.rand(terms, generator=g, dtype=th.float64) * (max_freq - 0.1) + 0.1
    angle = th.rand(terms, generator=g, dtype=th.float64) * (2 * math.pi)
    phase = th.rand(terms, generator=g, dtype=th.float64) * (2 * math.pi)
    amp = (th.rand(terms, generator=g, dtype=th.float64) + 0.5) / freq.sqrt()
    out = th.zeros_like(xs)
    for k in range(terms):
        out = out + amp[k] * th.sin(freq[k] * (math.cos(angle[k]) * xs + math.sin(angle[k]) * ys) + phase[k])
    return out / float(amp.pow(2).sum().sqrt() * 1.5)


def scene(H, W, motion, seed=0, channels=1):
    """(tmpl, img, F): two fp32 frames (1, channels, H, W) of the analytic texture and the analytic flow (1, 2, H, W) float64 with
    img(p + F(p)) = tmpl(p) exactly.  motion = (shift_x, shift_y) or (shift_x, shift_y, degrees, zoom): p -> c + zoom R (p - c) + shift."""
    sx, sy, deg, zoom = (tuple(motion) + (0.0, 1.0))[:4] if len(motion) == 2 else motion
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float64), th.arange(W, dtype=th.float64), indexing="ij")
    cx, cy = (W - 1) / 2, (H - 1) / 2
    cos, sin = zoom * math.cos(math.radians(deg)), zoom * math.sin(math.radians(deg))
    # forward map p' = c + A (p - c) + shift, A = [[cos, -sin], [sin, cos]]; img(x) = T(c + A^-1 (x - shift - c))
    px, py = cx + cos * (xs - cx) - sin * (ys - cy) + sx, cy + sin * (xs - cx) + cos * (ys - cy) + sy
    det = cos * cos + sin * sin
    qx, qy = xs - sx - cx, ys - sy - cy
    bx, by = cx + (cos * qx + sin * qy) / det, cy + (-sin * qx + cos * qy) / det
    tmpl = th.stack([texture(xs, ys, seed + 7 * c) for c in range(channels)])[None]
    img = th.stack([texture(bx, by, seed + 7 * c) for c in range(channels)])[None]
    return tmpl.float(), img.float(), th.stack([px - xs, py - ys])[None]


def share_within(flow, want, tol=0.25):
    """share of all pixels whose flow lies within `tol` px (Euclidean) of `want`, and the largest error"""
    err = (flow.double() - want.double()).pow(2).sum(dim=1).sqrt()
    return float((err <= tol).double().mean()), float(err.max())
