"""float64 restatement of csrc/warp3d.hip for the tests: the source position of every destination pixel by the rules of
include/cgd_mi355x.h (cgd_frame_warp3d: pinhole camera, backward map G, fixed-point depth lookup), then the sampling of tests/warp_ref.py
(the same border rule and cubic weights as the 2D warp).  Plain torch on the CPU.  A camera is anything with the fields R (9, row-major), T,
f, cx, cy, z0, near (cgd_amd.animate.camera's result)."""
import torch as th

from tests import warp_ref as R2

MAX_COORD = 2.0 ** 30


def depth_at(D, sx, sy):
    """D (H,W) float64 at the positions (sx, sy): bilinear, replicate border, the stored value at an integer position (a tap of weight 0
    is not read into the sum)."""
    H, W = D.shape
    px = th.nan_to_num(sx, nan=0.0).clamp(0, W - 1)
    py = th.nan_to_num(sy, nan=0.0).clamp(0, H - 1)
    fx, fy = px.floor(), py.floor()
    tx, ty = px - fx, py - fy
    x0, y0 = fx.long(), fy.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    a0 = th.where(tx == 0, D[y0, x0], (1 - tx) * D[y0, x0] + tx * D[y0, x1])
    a1 = th.where(tx == 0, D[y1, x0], (1 - tx) * D[y1, x0] + tx * D[y1, x1])
    return th.where(ty == 0, a0, (1 - ty) * a0 + ty * a1)


def _fmax(v, floor):
    """C's fmax(v, floor): a NaN reads as the floor"""
    return th.where(v >= floor, v, th.full_like(v, floor))


def positions(cam, H, W, depth=None, iters=1):
    """-> (sx, sy, clamped): float64 (N,H,W) source positions, N = 1 without a depth map and the map's batch with one (depth (N,1,H,W)),
    and how many pixels met the a_z or the near clamp (of lambda; over all sets and steps, a pixel counted once)."""
    Rm = [float(v) for v in cam.R]
    T = [float(v) for v in cam.T]
    f, cx, cy, z0, near = float(cam.f), float(cam.cx), float(cam.cy), float(cam.z0), float(cam.near)
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float64), th.arange(W, dtype=th.float64), indexing="ij")
    rx, ry = (xs - cx) / f, (ys - cy) / f
    ax = (Rm[0] * rx + Rm[3] * ry) + Rm[6]
    ay = (Rm[1] * rx + Rm[4] * ry) + Rm[7]
    az_raw = (Rm[2] * rx + Rm[5] * ry) + Rm[8]
    az = _fmax(az_raw, 1e-6)
    b = [Rm[i] * T[0] + Rm[3 + i] * T[1] + Rm[6 + i] * T[2] for i in range(3)]
    hit = ~(az_raw >= 1e-6)
    maps = [None] if depth is None else [d[0].detach().double().cpu() for d in depth]
    out_x, out_y = [], []
    for D in maps:
        sx, sy = xs.clone(), ys.clone()
        for _ in range(1 if D is None else iters):
            z = _fmax(th.full_like(xs, z0) if D is None else depth_at(D, sx, sy), near)
            lam_raw = (z + b[2]) / az
            lam = _fmax(lam_raw, near)
            hit = hit | ~(lam_raw >= near)
            sx = cx + f * (lam * ax - b[0]) / z
            sy = cy + f * (lam * ay - b[1]) / z
        out_x.append(th.nan_to_num(sx, nan=-MAX_COORD, posinf=MAX_COORD, neginf=-MAX_COORD).clamp(-MAX_COORD, MAX_COORD))
        out_y.append(th.nan_to_num(sy, nan=-MAX_COORD, posinf=MAX_COORD, neginf=-MAX_COORD).clamp(-MAX_COORD, MAX_COORD))
    return th.stack(out_x), th.stack(out_y), int(hit.sum())


def sample_fp64(src, sx, sy, interp="bicubic", border="wrap", clamp=False):
    """src (B,C,H,W) read at the positions sx, sy (1 or B, H, W) -> float64 (B,C,H,W); tests/warp_ref.warp_fp64's sampling."""
    src = src.detach().double().cpu()
    B, _, H, W = src.shape
    sx, sy = sx.expand(B, H, W), sy.expand(B, H, W)
    fx, fy = sx.floor(), sy.floor()
    tx, ty = (sx - fx)[:, None], (sy - fy)[:, None]
    ix, iy = fx.long(), fy.long()
    if interp == "bilinear":
        offs, wx, wy = (0, 1), (1 - tx, tx), (1 - ty, ty)
    elif interp == "bicubic":
        offs, wx, wy = (-1, 0, 1, 2), R2.cubic_weights(tx), R2.cubic_weights(ty)
    else:
        raise ValueError(interp)
    bi = th.arange(B)[:, None, None]
    out = th.zeros_like(src)
    for oy, w_y in zip(offs, wy):
        yy = R2.border_index(iy + oy, H, border)
        row = th.zeros_like(src)
        for ox, w_x in zip(offs, wx):
            xx = R2.border_index(ix + ox, W, border)
            row = row + w_x * src[bi, :, yy, xx].permute(0, 3, 1, 2)
        out = out + w_y * row
    return out.clamp(-1, 1) if clamp else out


def warp3d_fp64(src, cam, depth=None, iters=1, interp="bicubic", border="wrap", clamp=False):
    """-> (float64 (B,C,H,W), clamped pixel count): what cgd_frame_warp3d computes, in float64 throughout."""
    _, _, H, W = src.shape
    sx, sy, clamped = positions(cam, H, W, depth, iters)
    return sample_fp64(src, sx, sy, interp, border, clamp), clamped


def grid_sample_grid(sx, sy, H, W):
    """The (N,H,W,2) float64 grid that makes torch.nn.functional.grid_sample(..., align_corners=True) read at (sx, sy)."""
    gx = sx * 2 / (W - 1) - 1 if W > 1 else th.zeros_like(sx)
    gy = sy * 2 / (H - 1) - 1 if H > 1 else th.zeros_like(sy)
    return th.stack([gx, gy], dim=-1)
