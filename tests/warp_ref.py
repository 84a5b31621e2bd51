"""float64 restatements of csrc/warp.hip for the tests: the affine frame warp (bilinear / Keys bicubic with a = -0.75; wrap / reflect-101 /
replicate borders applied per tap) and the per-plane colour statistics and their transfer.  Plain torch on the CPU; the formulas are those of
include/cgd_mi355x.h (cgd_frame_warp, cgd_channel_stats, cgd_color_match)."""
import torch as th

INTERPS = ("bilinear", "bicubic")
BORDERS = ("wrap", "reflect", "replicate")


def border_index(i, n, border):
    """The tap indices i (int64 tensor, any sign) brought into [0, n)."""
    if border == "replicate":
        return i.clamp(0, n - 1)
    if border == "wrap":
        return i % n  # torch's remainder takes the divisor's sign: correct for negative i
    if border != "reflect":
        raise ValueError(border)
    if n == 1:
        return th.zeros_like(i)
    p = 2 * (n - 1)
    r = i % p
    return th.where(r >= n, p - r, r)


def cubic_weights(t):
    """Keys kernel, a = -0.75, at the distances t + 1, t, 1 - t, 2 - t (t float64 tensor) -> four tensors."""
    a = -0.75

    def near(x):
        return ((a + 2) * x - (a + 3)) * x * x + 1

    def far(x):
        return ((a * x - 5 * a) * x + 8 * a) * x - 4 * a

    return far(t + 1), near(t), near(1 - t), far(2 - t)


def warp_fp64(src, matrix, interp="bicubic", border="wrap", clamp=False):
    """src (B,C,H,W) -> float64 (B,C,H,W): destination pixel (x, y) reads the source at (m0 x + m1 y + m2, m3 x + m4 y + m5)."""
    src = src.detach().double().cpu()
    _, _, H, W = src.shape
    m = [float(v) for v in matrix]
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float64), th.arange(W, dtype=th.float64), indexing="ij")
    sx = m[0] * xs + m[1] * ys + m[2]
    sy = m[3] * xs + m[4] * ys + m[5]
    fx, fy = sx.floor(), sy.floor()
    tx, ty = sx - fx, sy - fy
    ix, iy = fx.long(), fy.long()
    if interp == "bilinear":
        offs, wx, wy = (0, 1), (1 - tx, tx), (1 - ty, ty)
    elif interp == "bicubic":
        offs, wx, wy = (-1, 0, 1, 2), cubic_weights(tx), cubic_weights(ty)
    else:
        raise ValueError(interp)
    out = th.zeros_like(src)
    for oy, w_y in zip(offs, wy):
        yy = border_index(iy + oy, H, border)
        row = th.zeros_like(src)
        for ox, w_x in zip(offs, wx):
            xx = border_index(ix + ox, W, border)
            row = row + w_x * src[:, :, yy, xx]
        out = out + w_y * row
    return out.clamp(-1, 1) if clamp else out


def stats_fp64(x):
    """(B,C,2) float64: mean and population standard deviation of every plane."""
    x = x.detach().double().cpu()
    return th.stack([x.mean(dim=(2, 3)), x.var(dim=(2, 3), unbiased=False).sqrt()], dim=-1)


def color_match_fp64(x, stats_x, stats_ref, amount, clamp=False):
    """x + amount ((mu_ref + (x - mu_x) r) - x) per plane, r = sigma_ref / sigma_x and 1 where sigma_x < 1e-6; stats_ref (1 or B, C, 2)."""
    x = x.detach().double().cpu()
    sx, sr = stats_x.detach().double().cpu(), stats_ref.detach().double().cpu().expand(x.shape[0], -1, -1)
    mx, sdx, mr, sdr = (t[:, :, None, None] for t in (sx[..., 0], sx[..., 1], sr[..., 0], sr[..., 1]))
    r = th.where(sdx < 1e-6, th.ones_like(sdx), sdr / th.where(sdx < 1e-6, th.ones_like(sdx), sdx))
    out = x + amount * ((mr + (x - mx) * r) - x)
    return out.clamp(-1, 1) if clamp else out


def grid_sample_matrix(matrix, H, W):
    """The (1,H,W,2) float64 grid that makes torch.nn.functional.grid_sample(..., align_corners=True) read where `matrix` reads."""
    m = [float(v) for v in matrix]
    ys, xs = th.meshgrid(th.arange(H, dtype=th.float64), th.arange(W, dtype=th.float64), indexing="ij")
    sx = m[0] * xs + m[1] * ys + m[2]
    sy = m[3] * xs + m[4] * ys + m[5]
    gx = sx * 2 / (W - 1) - 1 if W > 1 else th.zeros_like(sx)
    gy = sy * 2 / (H - 1) - 1 if H > 1 else th.zeros_like(sy)
    return th.stack([gx, gy], dim=-1).unsqueeze(0)
