"""Host side of the native `use_augs` cutouts (csrc/cutaug.hip): the parameter draws that feed the kernels follow reference_augs'
stream on the global CPU generator, the shared source-coordinate function reproduces grid_sample's picks and weights exactly as the
torch restatement applies them, and the new entry points reject NULL handles.  No GPU needed."""
import ctypes as C
import random

import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

import cgd_amd  # noqa: F401
from cgd_amd import guidance as dg
from cgd_amd import lib


@pytest.fixture
def no_noise(monkeypatch):
    monkeypatch.setattr(dg, "AUG_NOISE_STD", 0.0)


def sample_map(rec, h, w):
    """cgd_op_aug_sample_map of a 16-float record: (affine source index [h*w], perspective taps [h*w,4], weights [h*w,4])."""
    handle = lib.load()
    p = np.ascontiguousarray(rec, dtype=np.float32)
    aff = np.empty(h * w, np.int32)
    idx = np.empty((h * w, 4), np.int32)
    wt = np.empty((h * w, 4), np.float32)
    rc = handle.cgd_op_aug_sample_map(p.ctypes.data, h, w, aff.ctypes.data, idx.ctypes.data, wt.ctypes.data)
    assert rc == 0
    return aff, idx, wt


def param_sets(n, seed):
    """(h, w, AugParams) triples: drawn the way the product draws them on square / rectangular, odd / even crops, with every
    flip / perspective / grayscale combination forced on and off."""
    rnd = random.Random(seed)
    th.manual_seed(seed)
    out = []
    for k in range(n):
        h = rnd.randint(3, 24)
        w = h if k % 3 == 0 else rnd.randint(3, 24)
        p = dg.draw_aug_params(h, w)
        p.flip = bool(k & 1) if k % 5 else p.flip
        p.gray = bool(k & 2) if k % 7 else p.gray
        if k % 4 == 0 and p.persp:  # also perspective off
            p.persp = False
        out.append((h, w, p))
    return out


def test_draw_aug_params_follows_the_reference_augs_stream(no_noise):
    """draw_aug_params and reference_augs share _aug_draws, so this checks their agreement (generator state, outputs, record), not the
    draw order itself: the independent pin of that order is tests/test_host_logic.py::test_use_augs_pipeline_ops_match_their_torchvision_definitions."""
    sizes = [(17, 17), (9, 14), (24, 11), (16, 16), (5, 8), (13, 13)]
    x = th.rand(2, 3, 30, 30, generator=th.Generator().manual_seed(3))
    th.manual_seed(11)
    ref = [dg.reference_augs(x[:, :, :h, :w]) for h, w in sizes]
    state = th.get_rng_state()
    th.manual_seed(11)
    params = [dg.draw_aug_params(h, w) for h, w in sizes]
    assert th.equal(th.get_rng_state(), state)
    flags = set()
    for (h, w), p, r in zip(sizes, params, ref):
        y = x[:, :, :h, :w]
        y = y.flip(-1) if p.flip else y
        y = dg.aug_affine(y, p.angle, p.tx, p.ty)
        if p.persp:
            y = dg.aug_perspective(y, p.startpoints, p.endpoints, p.coeffs)
            assert np.allclose(p.coeffs, dg.perspective_coeffs(p.startpoints, p.endpoints), rtol=1e-6, atol=1e-9)
        y = dg.aug_grayscale(y) if p.gray else y
        assert th.equal(y, r)
        rec = p.record()
        assert len(rec) == 16 and rec[0] == float(p.flip) and rec[5] == float(p.persp) and rec[14] == float(p.gray) and rec[15] == 0.0
        flags.add((p.flip, p.persp))
    assert len(flags) >= 2


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sample_map_matches_grid_sample_exactly(seed):
    for h, w, p in param_sets(100, seed):
        rec = p.record()
        aff, idx, wt = sample_map(rec, h, w)
        # nearest: an index image (1 + pixel index, 0 = fill) through the torch restatement
        ids = (th.arange(h * w, dtype=th.float32) + 1).view(1, 1, h, w)
        want = dg.aug_affine(ids, p.angle, p.tx, p.ty).view(-1).to(th.int64) - 1
        assert np.array_equal(aff, want.numpy()), (h, w, p.angle, p.tx, p.ty)
        # bilinear: one-hot channels give the dense resampling matrix [source pixel, output pixel]
        if p.persp:
            start, end = p.startpoints, p.endpoints
        else:  # the map reports the perspective of the record's coefficients whatever its flag: pin a fresh homography too
            end = [[1, 0], [w - 1, 1], [w - 2, h - 1], [0, h - 2]] if h > 4 and w > 4 else [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]
            start = [[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]]
            rec = rec[:6] + dg.perspective_coeffs(start, end) + rec[14:]
            aff, idx, wt = sample_map(rec, h, w)
        eye = th.eye(h * w, dtype=th.float32).view(1, h * w, h, w)
        dense = dg.aug_perspective(eye, start, end, rec[6:14]).view(h * w, h * w).numpy()  # [source, output]
        mine = np.zeros((h * w, h * w), np.float32)
        for q in range(h * w):
            for k in range(4):
                if idx[q, k] >= 0:
                    mine[idx[q, k], q] += wt[q, k]
        assert (idx >= -1).all() and (idx < h * w).all() and ((idx >= 0) | (wt == 0)).all()
        assert np.abs(mine - dense).max() <= 1e-6, (h, w, np.abs(mine - dense).max())


def emulate(x_pm1, geo, recs, cs):
    """The kernel's forward, restated on the host from the sample maps and the record's flags (noise off): CLIP-normalised cutouts."""
    mean = th.tensor(dg.CLIP_MEAN).view(1, 3, 1, 1)
    std = th.tensor(dg.CLIP_STD).view(1, 3, 1, 1)
    outs = []
    for (oy, ox, h, w), rec in zip(geo, recs):
        z = (x_pm1[:, :, oy:oy + h, ox:ox + w] + 1) / 2
        z = z.flip(-1) if rec[0] else z
        aff, idx, wt = sample_map(rec, h, w)
        flat = th.cat([z.reshape(z.shape[0], 3, -1), th.zeros(z.shape[0], 3, 1)], -1)  # index -1 -> the zero column
        z = flat[:, :, th.as_tensor(aff, dtype=th.int64)]
        if rec[5]:
            flat = th.cat([z, th.zeros(z.shape[0], 3, 1)], -1)
            ii, ww = th.as_tensor(idx, dtype=th.int64), th.as_tensor(wt)
            z = sum(flat[:, :, ii[:, k]] * ww[:, k] for k in range(4))
        z = z.view(-1, 3, h, w)
        z = dg.aug_grayscale(z) if rec[14] else z
        outs.append((F.adaptive_avg_pool2d(z, cs) - mean) / std)
    return th.cat(outs)


def test_record_semantics_match_reference_augs(no_noise):
    """Flip / affine / perspective / grayscale flags of the record, consumed as the kernel consumes them, give reference_augs'
    output for the same draws (crop -> augment -> pool -> normalise), truncated rectangular crops included."""
    x = th.rand(2, 3, 40, 36, generator=th.Generator().manual_seed(7)) * 2 - 1
    th.manual_seed(21)
    coords = dg.generate_coords(40, 36, 12, 16, 1.0)
    coords += [(30, 25, 14), (0, 33, 9)]  # boxes truncated at the border: rectangular crops
    geo = dg.crop_geometry(coords, 40, 36)
    assert any(h != w for _, _, h, w in geo)
    th.manual_seed(5)
    recs = [dg.draw_aug_params(h, w).record() for _, _, h, w in geo]
    th.manual_seed(5)
    mk = dg.MakeCutouts(16, len(coords), use_augs=True)
    ref = mk.augmented((x + 1) / 2, coords)
    mean = th.tensor(dg.CLIP_MEAN).view(1, 3, 1, 1)
    std = th.tensor(dg.CLIP_STD).view(1, 3, 1, 1)
    got = emulate(x, geo, recs, 16)
    assert {(r[0], r[5], r[14]) for r in recs} and len({r[5] for r in recs}) == 2
    assert th.allclose(got, (ref - mean) / std, atol=1e-5, rtol=1e-5)


def test_new_entry_points_reject_null_handles():
    handle = lib.load()
    assert handle.cgd_cutouts_aug_fwd(None, None, None, None, None, None, None, 1, 8, 8, 1, 4, 0, 0, None) == -3
    assert handle.cgd_cutouts_aug_bwd(None, None, None, None, None, None, 1, 8, 8, 1, 4, 0, 0, 0, None) == -3
    buf = (C.c_int32 * 4)()
    assert handle.cgd_op_aug_sample_map(None, 2, 2, buf, buf, buf) == -3
    rec = (C.c_float * 16)()
    assert handle.cgd_op_aug_sample_map(rec, 2, 2, None, buf, buf) == -3
    # scratch: two (B,3,H,W) planes per cutout of a launch
    assert handle.cgd_cutouts_aug_scratch_floats(2, 64, 48, 5) == 2 * 5 * 2 * 3 * 64 * 48
    assert handle.cgd_cutouts_aug_scratch_floats(0, 64, 48, 5) == 0


def test_perspective_draws_keep_the_vanishing_line_off_the_crop():
    """cutaug_bwd_persp_kernel bounds its candidates by mapping the corners of a pixel's tap box through the inverse homography, which
    is exact when the homogeneous coordinate has one sign over the box; otherwise it scans the whole crop.  For RandomPerspective(0.4)
    draws the sign is constant over the crop widened by 1.5 px on every side (the largest tap box reach), so the scan is never taken."""
    rnd = random.Random(4)
    th.manual_seed(4)
    n = 0
    while n < 3000:
        h, w = rnd.randint(2, 256), rnd.randint(2, 256)
        p = dg.draw_aug_params(h, w)
        if not p.persp:
            continue
        n += 1
        a, b, c, d, e, f, g, hh = (float(v) for v in p.coeffs)
        m20, m21, m22 = d * hh - e * g, b * g - a * hh, a * e - b * d
        wz = [m20 * X + m21 * Y + m22 for X in (-1.5, w + 1.5) for Y in (-1.5, h + 1.5)]
        assert all(v > 0 for v in wz) or all(v < 0 for v in wz), (h, w, p.endpoints, wz)


# ---- ClipGuidance with a recording library --------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_std", [0.01, 0.0])
def test_guidance_launch_order_with_use_augs_and_a_recording_library(monkeypatch, noise_std):
    """The C-ABI calls of one guided step with use_augs cutouts on two towers: every tower draws its own parameters (six cutouts, in
    tower order, right before its forward launch), the adjoint's scratch size is asked inside each tower's backward, the second tower
    accumulates, and the noise and offset pointers are NULL exactly when the noise is off."""
    import types
    monkeypatch.setattr(dg, "AUG_NOISE_STD", noise_std)
    calls = []
    draw = dg.draw_aug_params

    def recorded_draw(h, w):
        p = draw(h, w)
        calls.append(("draw", p.record()))
        return p

    monkeypatch.setattr(dg, "draw_aug_params", recorded_draw)

    class FakeLib:
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, args))
                return {"cgd_guidance_part_blocks": 32, "cgd_cutouts_aug_scratch_floats": 7}.get(name, 0)
            return fn

    ctx = types.SimpleNamespace(lib=FakeLib(), h=1, check=lambda rc: None, stream=lambda: 0)

    class Tower:
        def __init__(self, name, res, patch, dim):
            self.name, self.input_resolution, self.patch, self.out_dim = name, res, patch, dim

        def encode_image(self, img, layout=0, n=None, out=None):
            calls.append((f"{self.name}.encode_image", (layout, n, tuple(img.shape))))
            return out

        def dgrad(self, d_emb, d_img=None):
            calls.append((f"{self.name}.dgrad", (tuple(d_emb.shape),)))
            return d_img

    unet = types.SimpleNamespace(dgrad=lambda seed, out: out)
    diffusion = types.SimpleNamespace(num_timesteps=50)
    vit, rn = Tower("vit", 32, 8, 16), Tower("rn", 64, 0, 24)
    B, H, W = 2, 32, 48
    guid = dg.ClipGuidance(ctx, unet, [vit, rn], diffusion, [th.randn(2, 16), th.randn(2, 24)], [1.0, -0.25], 6,
                           make_cutouts=dg.MakeCutouts(32, 6, use_augs=True))
    guid.current_timestep = 49
    guid.coords_tape = [[(0, 0, 32), (4, 0, 20)] * 3]
    x = th.zeros(B, 3, H, W)
    th.manual_seed(3)
    guid.native(x, x.clone(), x.clone(), coef=None)
    names = [c[0] for c in calls]
    leg = ["draw"] * 6 + ["cgd_cutouts_aug_fwd", "{}.encode_image", "cgd_spherical_loss", "{}.dgrad", "cgd_cutouts_aug_scratch_floats",
                          "cgd_cutouts_aug_bwd"]
    assert names == [n.format("vit") for n in leg] + [n.format("rn") for n in leg] + [
        "cgd_guidance_part_blocks", "cgd_guidance_combine", "cgd_grad_finish", "cgd_scalars"]
    by = {n: [c[1] for c in calls if c[0] == n] for n in set(names)}
    fwd, bwd = by["cgd_cutouts_aug_fwd"], by["cgd_cutouts_aug_bwd"]  # (h, x, boxes, params, noise, offsets, out, B, H, W, n, cs, layout, patch, s)
    assert fwd[0][7:] == (B, H, W, 6, 32, 1, 8, 0) and fwd[1][7:] == (B, H, W, 6, 64, 0, 0, 0)
    for f in fwd:
        assert (f[4] is None) == (f[5] is None) == (noise_std == 0.0)
    assert [c[-2] for c in bwd] == [0, 1]
    assert by["draw"][:6] != by["draw"][6:]  # a parameter table of its own per tower
    assert by["vit.encode_image"] == [(1, 6 * B, (6 * B * 16, 3 * 64))] and by["rn.encode_image"] == [(0, 6 * B, (6 * B, 3, 64, 64))]
    assert guid.make_cutouts.last_coords == guid.coords_tape[0] and guid.calls == 1 and guid.clip_part.numel() == 2 * 6 * B
