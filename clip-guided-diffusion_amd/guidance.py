"""CLIP guidance (`cond_fn`) without autograd: the MI355X replacement of the closure defined at
/root/reference/cgd/cgd.py:151-239.

`ClipGuidance` keeps the reference's plugin signature `cond_fn(x, t, out, y=None) -> Tensor[B,3,H,W]` and its
closure-variable semantics (`current_timestep`, set by the generator at cgd.py:265-267), but evaluates the
gradient in closed form through the C ABI:
    cutouts -> CLIP ViT forward -> spherical loss (+grad) -> ViT dgrad -> cutout scatter -> tv/range/sat grads
    -> chain through the blend and x0 = a*x - b*eps -> UNet dgrad -> negative gradient (-> magnitude clamp).
Cutout coordinates are drawn exactly like the reference does (three CPU-generator draws per cutout,
/root/reference/cgd/modules.py:44-46).  With `use_augs=True` the cutouts are augmented (flip / nearest affine / bilinear
perspective / grayscale / additive noise) inside the cutaug HIP kernels, whose adjoint is a deterministic gather; the parameters
are drawn like reference_augs draws them (draw_aug_params), the noise on the device generator in its randn_like order.
`MakeCutoutsResized` is a second cutter: overview + inner cuts through an antialiased cubic resize (the cutresize HIP kernels).
With `direction_embeds` the CLIP leg also scores the directional loss of prompt-pair edits against a source image (the direction HIP kernel).
With `aesthetic_heads` it also scores the LAION aesthetic predictors on the cutouts' embeddings (the aesthetic HIP kernel).
With `regions` (a regions.RegionPlan) every prompt weighs on a cutout by the share of its mask the cutout sees, inside the `_regions` loss entries.
Every cutter reaches the kernels through one per-step launch object (_CutLaunch, _AugLaunch: forward, backward, and torch_cuts, the same
cutouts in torch ops), so there is one CLIP leg (ClipGuidance._clip_leg) and one torch restatement of it (_clip_leg_torch) for all of them.
"""
import math

import torch as th
import torch.nn.functional as F

from . import lib as L


def generate_coords(side_x, side_y, cutn, cut_size, cut_pow, generator=None):
    """(offsetx, offsety, size) per cutout; same draw order as MakeCutouts._generate_coords."""
    max_size = min(side_y, side_x)
    min_size = min(side_y, side_x, cut_size)
    coords = []
    for _ in range(cutn):
        size = int(th.rand([], generator=generator) ** cut_pow * (max_size - min_size) + min_size)
        ox = th.randint(0, side_x - size + 1, (), generator=generator).item()
        oy = th.randint(0, side_y - size + 1, (), generator=generator).item()
        coords.append((ox, oy, size))
    return coords


def crop_geometry(coords, H, W):
    """(ox, oy, size) -> (oy, ox, h, w) of the slice input[:, :, oy:oy+size, ox:ox+size] (truncated at the border)."""
    return [(oy, ox, max(0, min(size, H - oy)), max(0, min(size, W - ox))) for (ox, oy, size) in coords]


def _sample_grid(x, xi, yi, mode):
    """x (N,C,H,W) sampled at input pixel-centre coordinates (xi, yi) of shape (H,W) each; zeros outside (torchvision fill=0)."""
    _, _, H, W = x.shape
    grid = th.stack([xi / (W / 2), yi / (H / 2)], dim=-1).unsqueeze(0).expand(x.shape[0], -1, -1, -1)
    return F.grid_sample(x, grid.to(x.dtype), mode=mode, padding_mode="zeros", align_corners=False)


def aug_affine(x, angle_deg, tx, ty):
    """torchvision.transforms.functional.affine(x, angle, (tx, ty), scale=1, shear=0), NEAREST, fill 0: rotation about the image
    centre (positive angle = clockwise, like torchvision), then translation; expressed as the inverse map output pixel -> input
    pixel, i.e. torchvision's _get_inverse_affine_matrix with shear 0: [[cos a, sin a], [-sin a, cos a]] applied to (xo - tx, yo - ty)."""
    _, _, H, W = x.shape
    ys, xs = th.meshgrid(th.arange(H, device=x.device, dtype=th.float32) + 0.5 - H / 2,
                         th.arange(W, device=x.device, dtype=th.float32) + 0.5 - W / 2, indexing="ij")
    a = math.radians(angle_deg)
    xo, yo = xs - tx, ys - ty
    xi = math.cos(a) * xo + math.sin(a) * yo
    yi = -math.sin(a) * xo + math.cos(a) * yo
    return _sample_grid(x, xi, yi, "nearest")


def perspective_coeffs(startpoints, endpoints):
    """The 8 coefficients of the homography that takes the `endpoints` (output corners) to the `startpoints` (input corners), solved
    like torchvision's _get_perspective_coeffs (float64 least squares), as the float32 values aug_perspective and the kernels use."""
    A = th.zeros(8, 8, dtype=th.float64)
    for i, ((x1, y1), (x2, y2)) in enumerate(zip(endpoints, startpoints)):
        A[2 * i] = th.tensor([x1, y1, 1, 0, 0, 0, -x2 * x1, -x2 * y1], dtype=th.float64)
        A[2 * i + 1] = th.tensor([0, 0, 0, x1, y1, 1, -y2 * x1, -y2 * y1], dtype=th.float64)
    b = th.tensor([c for p in startpoints for c in p], dtype=th.float64)
    return th.linalg.lstsq(A, b).solution.float().tolist()


def aug_perspective(x, startpoints, endpoints, coeffs=None):
    """torchvision.transforms.functional.perspective(x, startpoints, endpoints), BILINEAR, fill 0: the homography that takes the
    `endpoints` (output corners) to the `startpoints` (input corners), solved like torchvision's _get_perspective_coeffs (or the
    already solved `coeffs`: the least-squares solve is not bit-reproducible from call to call in its near-zero coefficients)."""
    _, _, H, W = x.shape
    co = perspective_coeffs(startpoints, endpoints) if coeffs is None else coeffs
    ys, xs = th.meshgrid(th.arange(H, device=x.device, dtype=th.float32) + 0.5, th.arange(W, device=x.device, dtype=th.float32) + 0.5,
                         indexing="ij")
    den = co[6] * xs + co[7] * ys + 1.0
    xi = (co[0] * xs + co[1] * ys + co[2]) / den - W / 2
    yi = (co[3] * xs + co[4] * ys + co[5]) / den - H / 2
    return _sample_grid(x, xi, yi, "bilinear")


def aug_grayscale(x):
    """torchvision rgb_to_grayscale with 3 output channels (ITU-R 601-2 luma)."""
    gray = 0.2989 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3]
    return gray.expand(-1, 3, -1, -1)


AUG_NOISE_STD = 0.01  # the reference's `x + randn_like(x) * 0.01` between the transforms (tests set it to 0 for CPU/GPU comparisons)


class AugParams:
    """One cutout's draw of the `use_augs` parameters (see draw_aug_params) and its record for the cutaug kernels."""
    __slots__ = ("flip", "angle", "tx", "ty", "persp", "startpoints", "endpoints", "coeffs", "gray")

    def __init__(self):
        self.flip = self.persp = self.gray = False
        self.angle, self.tx, self.ty = 0.0, 0, 0
        self.startpoints = self.endpoints = self.coeffs = None

    def record(self):
        """The 16-float parameter record of include/cgd_mi355x.h (cgd_cutouts_aug_fwd): flip, cos, sin, tx, ty, perspective flag,
        8 homography coefficients, grayscale flag, 0.  cos / sin / coefficients become float32 exactly as aug_affine / aug_perspective
        apply them to a float32 tensor."""
        a = math.radians(self.angle)
        co = self.coeffs if self.persp else [0.0] * 8
        return [float(self.flip), math.cos(a), math.sin(a), float(self.tx), float(self.ty), float(self.persp), *co, float(self.gray), 0.0]


def _aug_draws(H, W):
    """The parameter draws of reference_augs on an (N,3,H,W) cutout, in torchvision's order on the global CPU generator, one
    transform at a time: yields the same AugParams after the flip, the affine, the perspective and the grayscale draws (the torch
    path adds its noise in between; on CPU tensors that noise comes from the same generator)."""
    p = AugParams()
    p.flip = th.rand(1).item() < 0.5
    yield p
    p.angle = float(th.empty(1).uniform_(-15.0, 15.0).item())
    p.tx = int(round(th.empty(1).uniform_(-0.1 * W, 0.1 * W).item()))
    p.ty = int(round(th.empty(1).uniform_(-0.1 * H, 0.1 * H).item()))
    yield p
    if th.rand(1).item() < 0.7:
        hw, hh = W // 2, H // 2
        d = 0.4
        tl = [int(th.randint(0, int(d * hw) + 1, (1,)).item()), int(th.randint(0, int(d * hh) + 1, (1,)).item())]
        tr = [int(th.randint(W - int(d * hw) - 1, W, (1,)).item()), int(th.randint(0, int(d * hh) + 1, (1,)).item())]
        br = [int(th.randint(W - int(d * hw) - 1, W, (1,)).item()), int(th.randint(H - int(d * hh) - 1, H, (1,)).item())]
        bl = [int(th.randint(0, int(d * hw) + 1, (1,)).item()), int(th.randint(H - int(d * hh) - 1, H, (1,)).item())]
        p.persp = True
        p.startpoints, p.endpoints = [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], [tl, tr, br, bl]
        p.coeffs = perspective_coeffs(p.startpoints, p.endpoints)
    yield p
    p.gray = th.rand(1).item() < 0.15
    yield p


def draw_aug_params(h, w):
    """All parameter draws of reference_augs on one h x w cutout, in its order on the global CPU generator (flip; angle, tx, ty;
    perspective and its 8 corner offsets if taken; grayscale): what the native `use_augs` path draws per cutout."""
    for p in _aug_draws(h, w):
        pass
    return p


def reference_augs(x):
    """The reference's `use_augs` pipeline (/root/reference/cgd/modules.py:13-24) on one batched cutout (N,3,h,w):
    RandomHorizontalFlip(0.5), RandomAffine(degrees=15, translate=(0.1, 0.1)), RandomPerspective(0.4, p=0.7),
    RandomGrayscale(0.15), each followed by additive N(0, 0.01^2) noise.  Restated with plain torch ops (differentiable through
    grid_sample); the parameter draws follow torchvision's order on the global CPU generator (one draw set per call, shared by
    the batch, like a torchvision transform on a batched tensor).  torchvision is not installed in the build environment, so the
    stream equivalence with its own `get_params` is by construction, not pinned by a fixture."""
    _, _, H, W = x.shape
    # no draw at all when the noise is switched off: on CPU tensors randn_like advances the same generator the parameters come from
    noise = lambda t: t + th.randn_like(t) * AUG_NOISE_STD if AUG_NOISE_STD else t  # noqa: E731
    draws = _aug_draws(H, W)
    p = next(draws)
    if p.flip:
        x = x.flip(-1)
    x = noise(x)
    next(draws)
    x = noise(aug_affine(x, p.angle, p.tx, p.ty))
    next(draws)
    if p.persp:
        x = aug_perspective(x, p.startpoints, p.endpoints, p.coeffs)
    x = noise(x)
    next(draws)
    if p.gray:
        x = aug_grayscale(x)
    return noise(x)


CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _clip_mean_std(dev):
    return [th.tensor(c, device=dev).view(1, 3, 1, 1) for c in (CLIP_MEAN, CLIP_STD)]


AUG_GROUP_FLOATS = 1 << 25  # cutouts per launch group of the native `use_augs` path: noise + adjoint scratch of a group <= 128 MiB


def _upload(t, dev):
    """Small host table -> device without stalling the enqueueing thread: staged in pinned memory and copied asynchronously (torch's
    pinned allocator does not hand the staging block out again before the copy that reads it has completed)."""
    if th.device(dev).type != "cuda":
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


class _AugLaunch:
    """One draw of the native `use_augs` inputs for a list of cutout boxes: the parameters of every cutout (global CPU generator,
    draw_aug_params order), then, per launch group of cutouts, the additive noise (4 x randn((B,3,h,w)) per cutout on the device
    generator, the torch path's randn_like order; none while AUG_NOISE_STD is 0) right before the group's forward launch.  The
    two generators are independent, so the same seed gives the same augmentations and noise as reference_augs on the device."""

    def __init__(self, lib, coords, B, H, W, dev):
        self.lib, self.B, self.H, self.W = lib, B, H, W
        self.geo_list = crop_geometry(coords, H, W)
        self.n = len(self.geo_list)
        recs = [draw_aug_params(h, w).record() for (_, _, h, w) in self.geo_list]
        self.geo = _upload(th.tensor(self.geo_list, dtype=th.int32).view(-1, 4), dev)
        self.params = _upload(th.tensor(recs, dtype=th.float32).view(-1, 16), dev)
        self.std = float(AUG_NOISE_STD)
        self.groups, k0, used = [], 0, 0
        for k, (_, _, h, w) in enumerate(self.geo_list):
            n = (12 * B * h * w if self.std else 0) + 6 * B * H * W
            if k > k0 and used + n > AUG_GROUP_FLOATS:
                self.groups.append((k0, k))
                k0, used = k, 0
            used += n
        if self.geo_list:
            self.groups.append((k0, len(self.geo_list)))

    def forward(self, ctx, x_pm1, out, cs, layout, patch):
        """out rows (cut*B + b) of the cutouts of x_pm1 (B,3,H,W in [-1,1]), layout 0 or 1, CLIP-normalised."""
        B, H, W, dev = self.B, self.H, self.W, x_pm1.device
        row = out.element_size() * 3 * cs * cs * B
        for k0, k1 in self.groups:
            noise = off = None
            if self.std:
                sizes = [3 * B * h * w for (_, _, h, w) in self.geo_list[k0:k1]]
                noise = th.empty(4 * sum(sizes), device=dev)
                o, offs = 0, []
                for (_, _, h, w), n in zip(self.geo_list[k0:k1], sizes):
                    offs.append(o)
                    for _ in range(4):
                        noise[o:o + n].view(B, 3, h, w).normal_()
                        o += n
                noise.mul_(self.std)
                off = _upload(th.tensor(offs, dtype=th.int64), dev)
            ctx.check(self.lib.cgd_cutouts_aug_fwd(ctx.h, x_pm1.data_ptr(), self.geo[k0].data_ptr(), self.params[k0].data_ptr(),
                                                   None if noise is None else noise.data_ptr(), None if off is None else off.data_ptr(),
                                                   out.data_ptr() + k0 * row, B, H, W, k1 - k0, cs, layout, patch, ctx.stream()))

    def backward(self, ctx, d_out, g, cs, layout, patch, accumulate):
        """g (+)= d/dx_pm1 of <forward(x_pm1), d_out> (deterministic: the groups accumulate in order)."""
        B, H, W = self.B, self.H, self.W
        if not self.groups:  # no cutout: a zero adjoint
            if not accumulate:
                g.zero_()
            return
        row = d_out.element_size() * 3 * cs * cs * B
        most = max(k1 - k0 for k0, k1 in self.groups)
        scratch = th.empty(max(1, self.lib.cgd_cutouts_aug_scratch_floats(B, H, W, most)), device=d_out.device)
        for k0, k1 in self.groups:
            ctx.check(self.lib.cgd_cutouts_aug_bwd(ctx.h, d_out.data_ptr() + k0 * row, self.geo[k0].data_ptr(), self.params[k0].data_ptr(),
                                                   g.data_ptr(), scratch.data_ptr(), B, H, W, k1 - k0, cs, layout, patch,
                                                   int(bool(accumulate) or k0 > 0), ctx.stream()))


class _AugCuts:
    """The `use_augs` cutter of one step as the CLIP leg takes it: every tower gets an _AugLaunch of its own, and so parameter draws of
    its own, made right before its forward launch."""

    def __init__(self, lib, coords, B, H, W, dev):
        self.coords, self.args = coords, (lib, coords, B, H, W, dev)

    def per_tower(self):
        return _AugLaunch(*self.args)

    def torch_cuts(self, img01, cs):
        """The cutouts of img01 (B,3,H,W in [0,1]) at cut size cs in torch ops (fresh draws, in _AugLaunch's order), not normalised."""
        return MakeCutouts(cs, len(self.coords), use_augs=True).augmented(img01, self.coords)


class _CutLaunch:
    """The plain cutter (crop + adaptive average pool, cgd_cutouts_*) or the resized one (cgd_cutouts_resize_*) on one step's uploaded
    table `geo`, with _AugLaunch's two methods: crop_geometry rows of the (ox, oy, size) `coords`, or the resize_table of the
    (ox, oy, w, h, flags) records (boxes, then flags).  `scratch`: the resized adjoint's buffer (allocated at the first backward if None)."""

    def __init__(self, lib, coords, geo, resized=False, scratch=None):
        self.lib, self.coords, self.geo, self.n, self.resized, self.scratch = lib, coords, geo, len(coords), resized, scratch
        self.flags_p = geo.data_ptr() + 16 * self.n if resized else None

    def per_tower(self):
        return self

    def forward(self, ctx, x_pm1, out, cs, layout, patch):
        """out rows (cut*B + b) of the cutouts of x_pm1 (any B,3,H,W in [-1,1]), layout 0 or 1, CLIP-normalised."""
        B, _, H, W = x_pm1.shape
        if self.resized:
            ctx.check(self.lib.cgd_cutouts_resize_fwd(ctx.h, x_pm1.data_ptr(), self.geo.data_ptr(), self.flags_p, out.data_ptr(), B, H, W,
                                                      self.n, cs, layout, patch, ctx.stream()))
        else:
            ctx.check(self.lib.cgd_cutouts_fwd(ctx.h, x_pm1.data_ptr(), self.geo.data_ptr(), out.data_ptr(), B, H, W, self.n, cs, layout, patch,
                                               ctx.stream()))

    def backward(self, ctx, d_out, g, cs, layout, patch, accumulate):
        """g (B,3,H,W) (+)= d/dx_pm1 of <forward(x_pm1), d_out>."""
        B, _, H, W = g.shape
        if not self.resized:
            ctx.check(self.lib.cgd_cutouts_bwd(ctx.h, d_out.data_ptr(), self.geo.data_ptr(), g.data_ptr(), B, H, W, self.n, cs, layout, patch,
                                               int(accumulate), ctx.stream()))
            return
        if self.scratch is None:
            self.scratch = th.empty(max(1, self.lib.cgd_cutouts_resize_scratch_floats(B, H, W, self.n)), device=g.device)
        ctx.check(self.lib.cgd_cutouts_resize_bwd(ctx.h, d_out.data_ptr(), self.geo.data_ptr(), self.flags_p, g.data_ptr(), self.scratch.data_ptr(),
                                                  B, H, W, self.n, cs, layout, patch, int(accumulate), ctx.stream()))

    def torch_cuts(self, img01, cs):
        """The cutouts of img01 (any B,3,H,W in [0,1]) at cut size cs in torch ops with autograd, not normalised."""
        if self.resized:
            return MakeCutoutsResized(cs).resized(img01, self.coords)
        return th.cat([F.adaptive_avg_pool2d(img01[:, :, oy:oy + size, ox:ox + size], cs) for ox, oy, size in self.coords])


def _cutouts(mk, input, launch):
    """The cutouts of `input` (B,3,H,W in [0,1]) of the cutter module `mk` through `launch` (_CutLaunch or _AugLaunch), NCHW and not
    normalised; an autograd node over launch.backward when `input` requires grad."""
    if input.requires_grad and th.is_grad_enabled():
        return _CutoutsFunction.apply(input, mk.ctx, launch, mk.cut_size)
    return _cut_pool(input, mk.ctx, launch, mk.cut_size)


def _cut_pool(input, ctx, launch, cs):
    # the kernels cut (x+1)/2 and apply the CLIP normalisation; undo both to return the raw cutouts
    x_pm1 = (input.detach().float() * 2 - 1).contiguous()
    out = th.empty((launch.n * input.shape[0], 3, cs, cs), device=input.device, dtype=th.float32)
    launch.forward(ctx, x_pm1, out, cs, 0, 0)
    mean, std = _clip_mean_std(input.device)
    return out * std + mean


class _CutoutsFunction(th.autograd.Function):
    """_cut_pool as an autograd node (user-supplied cond_fns that follow the reference recipe, cgd.py:190-194); its backward is the
    launch's adjoint kernel."""

    @staticmethod
    def forward(ctx, input, lctx, launch, cs):
        ctx.args, ctx.in_shape = (lctx, launch, cs), tuple(input.shape)
        return _cut_pool(input, lctx, launch, cs)

    @staticmethod
    def backward(ctx, d_out):
        lctx, launch, cs = ctx.args
        # the adjoint kernels return d/dx of their own convention, out = (cut((x+1)/2) - mean) / std: feed them d_out * std and double the
        # result to get the adjoint of the plain cutouts
        d = (d_out.float() * th.tensor(CLIP_STD, device=d_out.device).view(1, 3, 1, 1)).contiguous()
        g = th.empty(ctx.in_shape, device=d_out.device, dtype=th.float32)
        launch.backward(lctx, d, g, cs, 0, 0, accumulate=False)
        return g * 2, None, None, None


class MakeCutouts(th.nn.Module):
    """Drop-in for cgd.modules.MakeCutouts (modules.py:5-66): same constructor, forward(input, use_cache,
    num_cutouts_override) and cache_coordinates(side_x, side_y); the crop+pool runs in one HIP kernel.
    `use_augs=True` (Python API only: the reference CLI hard-codes False, cgd.py:402) applies the reference's augmentation
    pipeline to every crop before pooling: on a GPU input in the cutaug HIP kernels (crop + augment + pool in one launch, a
    deterministic gather-form adjoint as the autograd backward), on a CPU input as plain differentiable torch ops
    (`augmented`, the `reference_augs` restatement)."""

    def __init__(self, cut_size, num_cutouts, cutout_size_power=1.0, use_augs=False, ctx=None):
        super().__init__()
        self.augs = reference_augs if use_augs else None
        self.cut_size, self.cutn, self.cut_pow = cut_size, num_cutouts, cutout_size_power
        self.cached_coords = None
        self.ctx = ctx
        self.last_coords = None

    def cache_coordinates(self, side_x, side_y):
        self.cached_coords = generate_coords(side_x, side_y, self.cutn, self.cut_size, self.cut_pow)

    def draw(self, side_x, side_y, use_cache=False, num_cutouts_override=None):
        cutn = num_cutouts_override if num_cutouts_override is not None else self.cutn
        if use_cache and self.cached_coords is not None:
            return self.cached_coords[:cutn]
        return generate_coords(side_x, side_y, cutn, self.cut_size, self.cut_pow)

    def forward(self, input, use_cache=False, num_cutouts_override=None):
        """input (B,3,H,W) in [0,1] -> (cutn*B,3,cut,cut) NCHW, *not* normalised (as in the reference).  Differentiable: when
        `input` requires grad the result is an autograd node whose backward is the cutout scatter kernel (cgd_cutouts_bwd)."""
        _, _, H, W = input.shape
        coords = self.draw(H, W, use_cache, num_cutouts_override)  # (side_x, side_y) = (H, W): reference naming
        self.last_coords = coords
        if self.augs is not None and input.device.type != "cuda":
            return self.augmented(input, coords)
        if self.ctx is None:
            self.ctx = L.Context(input.device.index or 0)
        if self.augs is not None:
            return _cutouts(self, input, _AugLaunch(self.ctx.lib, coords, input.shape[0], H, W, input.device))
        geo = th.tensor(crop_geometry(coords, H, W), dtype=th.int32, device=input.device)
        return _cutouts(self, input, _CutLaunch(self.ctx.lib, coords, geo))

    def augmented(self, input, coords):
        """crop -> augment -> adaptive average pool -> cat, as modules.py:58-66 does with `self.augs` set: torch ops with autograd."""
        outs = []
        for ox, oy, size in coords:
            cut = self.augs(input[:, :, oy:oy + size, ox:ox + size])
            outs.append(F.adaptive_avg_pool2d(cut, self.cut_size))
        return th.cat(outs)


RESIZE_GRAY, RESIZE_FLIP = 1, 2  # flag bits of a resized cutout: grayscale before the resize, horizontal flip after it


def _resize_cubic(d):
    a = d.abs()
    return th.where(a <= 1, (1.5 * a - 2.5) * a * a + 1, th.where(a <= 2, ((-0.5 * a + 2.5) * a - 4) * a + 2, th.zeros_like(a)))


def resize_matrix(n, m, dtype=th.float32, device=None):
    """Dense (m, n) matrix of the antialiased cubic resize of an extent n to m (include/cgd_mi355x.h, cgd_cutouts_resize_fwd): centres
    c_o = ((2o+1) n - m) / (2m), T = ceil(S) taps from ceil(c_o - S / 2) with S = 4 (m >= n) or 4n / m, weights cubic(c_o - j) (or
    s cubic(s (c_o - j)), s = m / n < 1) over their sum over all T taps; taps outside [0, n) are dropped, not renormalised.  Integer
    geometry, float64 polynomial: the CPU restatement of the kernels' weight rows."""
    if m == n:
        return th.eye(n, dtype=dtype, device=device)
    big = max(m, n)
    T = 4 if m >= n else -(-4 * n // m)
    o = th.arange(m, dtype=th.int64)
    num = (2 * o + 1) * n - m
    left = -((4 * big - num) // (2 * m))  # ceil((num - 4 big) / (2m))
    j = left[:, None] + th.arange(T, dtype=th.int64)
    k = _resize_cubic((num[:, None] - 2 * m * j).double() / (2 * big))  # c_o - j for m >= n, s (c_o - j) for m < n (s cancels below)
    tot = k.sum(1, keepdim=True)
    w = k / th.where(tot == 0, th.ones_like(tot), tot)
    inside = (j >= 0) & (j < n)
    M = th.zeros(m, n, dtype=th.float64)
    M.scatter_add_(1, j.clamp(0, n - 1), th.where(inside, w, th.zeros_like(w)))
    return M.to(dtype=dtype, device=device)


def resize_table(records, H, W):
    """(ox, oy, w, h, flags) records -> the int32 rows a step uploads: len(records) rows (oy, ox, h, w), then the flags packed four to a
    row.  A box with an extent below 1 or outside the H x W image is refused here: the kernels only see the table on the device."""
    rows, flags = [], []
    for ox, oy, w, h, fl in records:
        if h < 1 or w < 1 or ox < 0 or oy < 0 or oy + h > H or ox + w > W:
            raise ValueError(f"cutout box (ox {ox}, oy {oy}, w {w}, h {h}) is empty or outside the {H} x {W} image")
        rows.append((oy, ox, h, w))
        flags.append(int(fl))
    flags += [0] * (-len(flags) % 4)
    return rows + [tuple(flags[i:i + 4]) for i in range(0, len(flags), 4)]


class MakeCutoutsResized(th.nn.Module):
    """The cutout scheme of the CLIP-guided-diffusion notebooks: `overview` cuts of the whole frame (for overview <= 4: plain, grayscale,
    mirrored, grayscale + mirrored, in that order; all plain beyond 4) followed by `inner` random square crops, every cut brought to
    cut_size x cut_size by the antialiased cubic resize (resize_matrix) instead of adaptive average pooling.  Inner cut i has
    size = int(rand() ** ic_size_pow * (max_size - min_size) + min_size) with max_size = min(H, W), min_size = min(H, W, cut_size), then
    ox = randint(0, W - size + 1), oy = randint(0, H - size + 1) (three CPU-generator draws per cut, in generate_coords' order), and is
    grayscale when i <= int(ic_gray_p * inner).  `schedule`: optional rows (until_fraction_done, overview, inner); the first row whose
    bound exceeds the fraction of the run that is done gives the step's counts (the constructor's counts when none does).
    A cut is the record (ox, oy, w, h, flags)."""
    augs = None  # no `use_augs` pipeline on this cutter

    def __init__(self, cut_size, overview=4, inner=12, ic_size_pow=0.5, ic_gray_p=0.2, schedule=None, ctx=None):
        super().__init__()
        self.cut_size, self.overview, self.inner = cut_size, int(overview), int(inner)
        self.ic_size_pow, self.ic_gray_p = ic_size_pow, ic_gray_p
        self.schedule = [(float(u), int(ov), int(inn)) for (u, ov, inn) in schedule] if schedule else None
        for ov, inn in [(self.overview, self.inner)] + [r[1:] for r in self.schedule or []]:
            if ov < 0 or inn < 0 or ov + inn < 1:
                raise ValueError(f"overview / inner cut counts must be >= 0 with at least one cut, got {ov}:{inn}")
        self.cached_coords = None
        self.ctx = ctx
        self.last_coords = None

    @property
    def cutn(self):
        return self.overview + self.inner

    def counts(self, fraction_done=0.0):
        """(overview, inner) at this point of the run."""
        for until, ov, inn in self.schedule or []:
            if fraction_done < until:
                return ov, inn
        return self.overview, self.inner

    def _counts(self, override):
        if override is None:
            return self.overview, self.inner
        if isinstance(override, (tuple, list)):
            return int(override[0]), int(override[1])
        ov = min(self.overview, int(override))  # a plain count keeps the overview cuts and trims the inner ones
        return ov, int(override) - ov

    def _inner_boxes(self, side_x, side_y, count):
        max_size = min(side_x, side_y)
        min_size = min(side_x, side_y, self.cut_size)
        boxes = []
        for _ in range(count):
            size = int(th.rand([]) ** self.ic_size_pow * (max_size - min_size) + min_size)
            ox = th.randint(0, side_x - size + 1, ()).item()
            oy = th.randint(0, side_y - size + 1, ()).item()
            boxes.append((ox, oy, size, size))
        return boxes

    def cache_coordinates(self, side_x, side_y):
        """Draw the inner boxes once (as many as the largest count of the schedule) for draw(..., use_cache=True)."""
        most = max([self.inner] + [r[2] for r in self.schedule or []])
        self.cached_coords = self._inner_boxes(side_x, side_y, most)

    def draw(self, side_x, side_y, use_cache=False, num_cutouts_override=None):
        """The records of one step on a side_x (width) x side_y (height) image.  num_cutouts_override: (overview, inner), or one count."""
        ov, inn = self._counts(num_cutouts_override)
        flags = [0, RESIZE_GRAY, RESIZE_FLIP, RESIZE_GRAY | RESIZE_FLIP][:ov] if ov <= 4 else [0] * ov
        recs = [(0, 0, side_x, side_y, fl) for fl in flags]
        if use_cache and self.cached_coords is not None:
            boxes = self.cached_coords[:inn]
        else:
            boxes = self._inner_boxes(side_x, side_y, inn)
        gray_upto = int(self.ic_gray_p * inn)
        return recs + [(ox, oy, w, h, RESIZE_GRAY if i <= gray_upto else 0) for i, (ox, oy, w, h) in enumerate(boxes)]

    def forward(self, input, use_cache=False, num_cutouts_override=None):
        """input (B,3,H,W) in [0,1] -> (n*B,3,cut,cut) NCHW, not normalised.  On a GPU input the resize runs in the cutresize HIP kernels
        (an autograd node over cgd_cutouts_resize_fwd / _bwd when `input` requires grad), on a CPU input as torch ops (`resized`)."""
        _, _, H, W = input.shape
        recs = self.draw(W, H, use_cache, num_cutouts_override)
        self.last_coords = recs
        if input.device.type != "cuda":
            return self.resized(input, recs)
        if self.ctx is None:
            self.ctx = L.Context(input.device.index or 0)
        table = th.tensor(resize_table(recs, H, W), dtype=th.int32, device=input.device)
        return _cutouts(self, input, _CutLaunch(self.ctx.lib, recs, table, resized=True))

    def resized(self, input, records, cut_size=None):
        """crop -> (grayscale) -> Wy crop Wx^T -> (flip) -> cat: the torch restatement, with autograd."""
        cs = cut_size or self.cut_size
        outs = []
        for ox, oy, w, h, fl in records:
            z = input[:, :, oy:oy + h, ox:ox + w]
            if fl & RESIZE_GRAY:
                z = aug_grayscale(z)
            r = resize_matrix(h, cs, input.dtype, input.device) @ z @ resize_matrix(w, cs, input.dtype, input.device).t()
            outs.append(r.flip(-1) if fl & RESIZE_FLIP else r)
        return th.cat(outs)


def prompt_weight_matrix(weights, batch, device):
    """The reference broadcasts (1,cutn,B,D) against (1,P,D) (cgd.py:196-200): valid for B==1, P==1 or B==P.
    Returns the dense (B,P) weights the loss kernel consumes; B==P>1 scores sample b against prompt b only and
    scales by sum(w)."""
    w = th.as_tensor(weights, dtype=th.float32).flatten()
    P = w.numel()
    if batch == 1 or P == 1:
        m = w.view(1, P).expand(batch, P)
    elif batch == P:
        m = th.eye(batch) * w.sum()
    else:
        raise RuntimeError(f"The size of tensor a ({batch}) must match the size of tensor b ({P}) at non-singleton dimension 2")
    return m.contiguous().to(device)


def guidance_schedule(total, current_timestep, num_cutouts, reduce_clip=False, progressive_cutout=False):
    """(skip_guidance, cutouts_this_step) of /root/reference/cgd/cgd.py:155-175: with reduce_clip, guidance runs on every 4th
    step while less than 70 % of the schedule is done (the first 20 % are skipped through skip_timesteps, cgd.py:140-144); with
    progressive_cutout the cutout count is max(4, n//4) below 30 %, max(8, n//2) below 70 %, n afterwards.  `current_timestep`
    is the reference's closure counter, not the sampler's t."""
    pct = (total - current_timestep) / total
    if reduce_clip and pct < 0.7:
        if int((pct - 0.2) * total) % 4 != 0:
            return True, 0
    if progressive_cutout:
        n = num_cutouts
        return False, (max(4, n // 4) if pct < 0.3 else (max(8, n // 2) if pct < 0.7 else n))
    return False, num_cutouts


class ClipGuidance:
    def __init__(self, ctx, unet, clip_tower, diffusion, target_embeds, weights, num_cutouts, cutout_power=1.0,
                 clip_guidance_scale=1000.0, tv_scale=150.0, range_scale=50.0, sat_scale=0.0, use_magnitude=False,
                 reduce_clip=False, progressive_cutout=False, cached_cutouts=False, make_cutouts=None, lpips=None, init_tensor=None,
                 init_scale=0.0, secondary=None, classifier=None, classifier_scale=1.0, classifier_class=None, direction_embeds=None,
                 direction_weights=None, direction_source=None, direction_columns=None, style_tensor=None, style_scale=0.0,
                 style_weights=(1, 1, 1, 1, 0), regions=None, aesthetic_heads=None, aesthetic_scale=0.0):
        # Multi-CLIP (BASELINE config 5, a build extension: the reference takes one clip_model_name): `clip_tower` / `target_embeds`
        # may be lists; the CLIP losses of the towers are summed (same cutout boxes, prompt weights and guidance scale).
        self.towers = list(clip_tower) if isinstance(clip_tower, (list, tuple)) else [clip_tower]
        # directional loss of prompt-pair edits (csrc/direction.hip), off without `direction_embeds`: one (P_d, D) tensor of raw text
        # differences E(target caption) - E(source caption) per tower, `direction_weights` (P_d,) and `direction_source`, the source image
        # (1 or B, 3, H, W) in [-1, 1].  The B x P weight matrix is built over the P_t + P_d prompts together, the directions in the columns
        # `direction_columns` of that list (default: behind the targets) and `weights` in the others in order, and then split into the
        # two groups.  `target_embeds` may be None (or empty tensors) when there are only directions: the spherical launch is then not made
        # aesthetic-predictor guidance (csrc/aesthetic.hip), off without `aesthetic_heads`: one nets.AestheticHead
        # or None per tower, or a single head for a single tower, and `aesthetic_scale`, a float or one per tower; the loss gains
        # -aesthetic_scale_k * sum_b mean_cut (a_k . normalize(e) + beta_k) for every tower k with a head.  A scale of 0 means no head.  The head
        # is no prompt: it has no column in the weight matrix and takes no region weight.  `target_embeds` may be None with a head present
        self.aes_list = self._aesthetic_heads(aesthetic_heads, aesthetic_scale)
        self.aes_score = None
        has_dir = direction_embeds is not None
        if has_dir:
            dirs = list(direction_embeds) if isinstance(direction_embeds, (list, tuple)) else [direction_embeds]
            assert len(dirs) == len(self.towers), "one direction-embedding tensor per CLIP tower"
            if target_embeds is None:
                target_embeds = [d.new_zeros((0, d.shape[-1])) for d in dirs]
                weights = []
        # VGG Gram-matrix style term (csrc/gram.hip, nets.LpipsVGG.set_style): `style_tensor` (1,3,Hs,Ws) in [-1,1] on the `lpips` handle's trunk,
        # the loss gains style_scale * sum_b L_style(x_in_b).  With a style and no prompt of either kind the CLIP leg is not run at all
        # (`target_embeds` None): the extension of the direction-only path
        has_style = style_tensor is not None and style_scale != 0
        if has_style and lpips is None:
            raise ValueError("style_tensor needs the LPIPS-VGG16 handle (lpips=): the style term runs on its trunk")
        if has_style and not (float(style_scale) > 0):
            raise ValueError(f"style_scale must be positive, got {style_scale}")
        if target_embeds is None and not has_dir:
            if not has_style and self.aes_list is None:
                raise ValueError("no target embeddings: only a run with direction prompts, a style image or an aesthetic head goes without")
            like = style_tensor if self.aes_list is None else next(a[0] for a in self.aes_list if a is not None)
            target_embeds = [like.new_zeros((0, t.out_dim)) for t in self.towers]
            weights = []
        embeds = list(target_embeds) if isinstance(target_embeds, (list, tuple)) else [target_embeds]
        assert len(embeds) == len(self.towers), "one target-embedding tensor per CLIP tower"
        self.ctx, self.unet, self.clip, self.diffusion = ctx, unet, self.towers[0], diffusion
        clip_tower = self.towers[0]
        dev = embeds[0].device
        self.targets_list = [F.normalize(e.float(), dim=-1).contiguous() for e in embeds]
        self.targets_n = self.targets_list[0]
        self.weights = th.as_tensor(weights, dtype=th.float32, device=dev).flatten()
        self.dirs_list = self.direction_weights = self.direction_source = self.direction_columns = None
        self._src_emb = {}       # (cutn, B) -> (boxes, per-tower source embeddings): reused while cached_cutouts keeps the boxes
        self.clip_part = None
        if has_dir:
            if direction_source is None:
                raise ValueError("direction_embeds needs direction_source: the image whose embedding the edit starts from")
            if direction_source.dim() != 4 or direction_source.shape[1] != 3:
                raise ValueError(f"direction_source must be (1 or B, 3, H, W), got {tuple(direction_source.shape)}")
            self.dirs_list = [F.normalize(d.float(), dim=-1).contiguous() for d in dirs]
            pd, pt = self.dirs_list[0].shape[0], self.weights.numel()
            self.direction_weights = th.as_tensor(th.ones(pd) if direction_weights is None else direction_weights, dtype=th.float32).flatten()
            cols = list(range(pt, pt + pd)) if direction_columns is None else [int(c) for c in direction_columns]
            if self.direction_weights.numel() != pd or len(cols) != pd or len(set(cols)) != pd or not all(0 <= c < pt + pd for c in cols):
                raise ValueError(f"{pd} direction prompts need {pd} direction_weights and {pd} distinct direction_columns below {pt + pd}")
            if any(t.shape[0] != pt for t in self.targets_list) or any(d.shape[0] != pd for d in self.dirs_list):
                raise ValueError("every tower needs the same number of target and of direction embeddings as there are weights")
            self.direction_columns = cols
            self.direction_source = direction_source.detach().float().contiguous()
        # region prompts (regions.RegionPlan over the P_t + P_d prompts in the order of the weight list, or None): every prompt's weight on a
        # cutout is scaled by the share of its mask the cutout sees, inside the `_regions` loss entries; split by column like the weights
        self.regions = self._reg_t = self._reg_d = self._reg_cols = None
        if regions is not None:
            pt = self.weights.numel()
            dcols = self.direction_columns or []
            if regions.P != pt + len(dcols):
                raise ValueError(f"the region plan covers {regions.P} prompts, the weights {pt + len(dcols)}")
            self.regions = regions
            self._reg_cols = ([c for c in range(regions.P) if c not in dcols], list(dcols))
        self.num_cutouts = num_cutouts
        self.cgs, self.tvs, self.rs, self.sats = float(clip_guidance_scale), float(tv_scale), float(range_scale), float(sat_scale)
        self.use_magnitude = bool(use_magnitude)
        self.reduce_clip, self.progressive_cutout, self.cached_cutouts = reduce_clip, progressive_cutout, cached_cutouts
        self.make_cutouts = make_cutouts or MakeCutouts(clip_tower.input_resolution, num_cutouts, cutout_power, ctx=ctx)
        if isinstance(self.make_cutouts, MakeCutoutsResized) and progressive_cutout:
            raise ValueError("progressive_cutout does not apply to MakeCutoutsResized: its cut counts come from its own schedule")
        if has_dir and self.make_cutouts.augs is not None:
            raise ValueError("direction prompts do not work with use_augs cutouts: the random warp of every cut would have to be replayed on "
                             "the source image")
        if regions is not None and self.make_cutouts.augs is not None:
            raise ValueError("region prompts do not work with use_augs cutouts: the box is warped after the crop, so its share of a mask is "
                             "not the share the cutout shows")
        # init-image perceptual term (cgd.py:147-148,220-224): `lpips` is a nets.LpipsVGG, its reference = the init image
        self.lpips, self.init_scale, self.init_tensor = None, float(init_scale), None
        if lpips is not None and init_tensor is not None and init_scale != 0:
            self.lpips, self.init_tensor = lpips, init_tensor.float()
        self._lpips_ref_batch = 0
        self.style, self.style_scale, self.style_tensor, self.style_weights = None, float(style_scale), None, tuple(style_weights)
        if has_style:
            self.style, self.style_tensor = lpips, style_tensor.float()
        self._style_set = False
        self.style_loss = None
        # style (and init) terms only: no cutouts, no CLIP pass
        self.no_clip = self.dirs_list is None and self.aes_list is None and self.targets_list[0].shape[0] == 0
        # secondary model (nets.SecondaryModel) or None: with one, pred / x_in of the guidance losses come from it and the gradient returns to x
        # through it; the UNet's backward pass is not run (its forward still gives the update's mean, variance and the yielded pred_xstart)
        self.secondary = secondary
        # noisy classifier (nets.NoisyClassifier) or None: with one, the loss gains -classifier_scale * sum_b log p(classifier_class | x_t, t),
        # evaluated on the step's x at the model timesteps the UNet's forward received; its gradient joins the direct part of g
        self.classifier, self.classifier_scale, self.classifier_class = classifier, float(classifier_scale), classifier_class
        if classifier is not None:
            if classifier_class is None or not (0 <= int(classifier_class) < classifier.out_channels):
                raise ValueError(f"classifier_class must be a class id in [0, {classifier.out_channels}), got {classifier_class}")
            if not (self.classifier_scale > 0):
                raise ValueError(f"classifier_scale must be positive, got {classifier_scale}")
            self.classifier_class = int(classifier_class)
        self.classifier_logp = None
        self.step_ts = None      # set by the sampler before native(): the model timesteps of the step's UNet forward
        self.lpips_loss = None
        self.current_timestep = None  # closure counter of cgd.py:149,265-267
        self.scalars = None
        self.coords_tape = None  # optional replay of cutout coordinates (tests)
        self.calls = 0
        self.last_ran = False    # did the last call evaluate the guidance (False on a --reduce-clip gated step)?
        self.shard = None        # (indices of the global batch on this rank, global batch size): rows of the B x P weight matrix
        self._wm = {}
        self._wmd = {}           # the direction columns of the weight matrix, per batch size
        self._buf = {}
        self._lpips_net = lpips  # the handle as given: set_init can switch the init-image term on later

    # -- between runs on the same guidance (cgd_amd.animate; nothing on the existing paths calls these) --------------------------
    def set_init(self, init_tensor, init_scale, lpips=None):
        """Replace the image the LPIPS term holds the sample to, (1 or B, 3, H, W) in [-1, 1], and its weight; the next call hands the new
        image to the LPIPS handle (set_reference).  None or a zero scale switches the term off.  `lpips`: a nets.LpipsVGG for a guidance
        that was built without one."""
        self.init_scale = float(init_scale)
        if lpips is not None:
            self._lpips_net = lpips
        if init_tensor is None or init_scale == 0:
            self.lpips = self.init_tensor = None
        else:
            if self._lpips_net is None:
                raise ValueError("set_init needs the LPIPS-VGG16 handle the guidance was built with (lpips=)")
            if init_tensor.dim() != 4 or init_tensor.shape[1] != 3:
                raise ValueError(f"init_tensor must be (1 or B, 3, H, W), got {tuple(init_tensor.shape)}")
            self.lpips, self.init_tensor = self._lpips_net, init_tensor.detach().float()
        self._lpips_ref_batch = 0

    def set_targets(self, embeds, weights):
        """Replace the target embeddings (one (P, D) tensor per tower, or one tensor) and their P weights (as the constructor takes them);
        the B x P weight matrices are rebuilt at the next call.  Not with direction prompts or regions: their columns index the old list."""
        if self.dirs_list is not None or self.regions is not None:
            raise ValueError("set_targets does not work with direction prompts or region prompts: their columns index the first prompt list")
        embeds = list(embeds) if isinstance(embeds, (list, tuple)) else [embeds]
        if len(embeds) != len(self.towers):
            raise ValueError("one target-embedding tensor per CLIP tower")
        w = th.as_tensor(weights, dtype=th.float32).flatten()
        if any(e.dim() != 2 or e.shape[0] != w.numel() for e in embeds) or w.numel() == 0:
            raise ValueError(f"every tower needs as many target embeddings as there are weights ({w.numel()}), and at least one")
        self.targets_list = [F.normalize(e.float(), dim=-1).contiguous() for e in embeds]
        self.targets_n = self.targets_list[0]
        self.weights = w.to(self.targets_n.device)
        self.no_clip = False
        self._wm, self._wmd = {}, {}

    # -- helpers ------------------------------------------------------------------------------------
    def _aesthetic_heads(self, heads, scales):
        """The constructor's `aesthetic_heads` / `aesthetic_scale` -> None (no head anywhere: every path is then as without the keywords), or
        per tower None or (the (D + 1,) fp32 vector, the scale).  Refuses a list of another length than the towers and a head of another
        width than its tower's embeddings, naming both."""
        if heads is None:
            return None
        heads = list(heads) if isinstance(heads, (list, tuple)) else [heads]
        if len(heads) != len(self.towers):
            raise ValueError(f"{len(heads)} aesthetic heads for {len(self.towers)} CLIP towers: give one head or None per tower")
        scales = [float(v) for v in scales] if isinstance(scales, (list, tuple)) else [float(scales)] * len(heads)
        if len(scales) != len(heads):
            raise ValueError(f"{len(scales)} aesthetic scales for {len(heads)} heads: give one float, or one per tower")
        out = []
        for k, (head, scale, tower) in enumerate(zip(heads, scales, self.towers)):
            if head is None or scale == 0:
                out.append(None)
                continue
            if not math.isfinite(scale):
                raise ValueError(f"aesthetic_scale of tower {k} must be finite, got {scale}")
            vec, dim = head.vec, int(head.dim)
            if vec is None or vec.numel() != dim + 1:
                raise ValueError(f"aesthetic head of tower {k}: expected a loaded (dim + 1,) vector")
            if dim != tower.out_dim:
                raise ValueError(f"the aesthetic head of tower {k} is for {dim}-wide embeddings, the tower gives {tower.out_dim}")
            out.append((vec.detach().float().flatten().contiguous(), scale))
        return out if any(a is not None for a in out) else None

    def _b(self, name, shape, device, dtype=th.float32):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.device != device:
            t = self._buf[name] = th.empty(shape, device=device, dtype=dtype)
        return t

    def _upload_geometry(self, geo, dev):
        """Crop table of this step -> device: written into one of four pinned staging rows and copied asynchronously (a
        pageable-memory `th.tensor(...).to(dev)` stalls the enqueueing thread on every step).  A slot is reused only after the
        copy that last read it has completed (event; already signalled in steady state)."""
        n = len(geo)
        if th.device(dev).type != "cuda":  # host-logic tests drive this class with a recording library and CPU tensors
            return th.as_tensor(geo, dtype=th.int32).view(n, 4).to(dev)
        ring = self._buf.get("_geo_ring")
        if ring is None or ring["host"].shape[1] < n or ring["dev"].device != dev:
            cap = max(n, 64)
            ring = self._buf["_geo_ring"] = {"host": th.empty((4, cap, 4), dtype=th.int32).pin_memory(),
                                             "dev": th.empty((4, cap, 4), dtype=th.int32, device=dev),
                                             "done": [None] * 4, "next": 0}
        k = ring["next"]
        ring["next"] = (k + 1) % 4
        if ring["done"][k] is not None:
            ring["done"][k].synchronize()
        host = ring["host"][k, :n]
        host.copy_(th.as_tensor(geo, dtype=th.int32).view(n, 4))
        out = ring["dev"][k, :n]
        out.copy_(host, non_blocking=True)
        # blocking=True: a host that has run four steps ahead SLEEPS until the slot is free instead of spinning on the event — with one
        # driver process per GPU the spin would keep 8 cores busy doing nothing (36 ms of CPU per 20 ms step per rank measured,
        # profiles/r3_host_contention.txt; the enqueue itself needs 4 ms)
        ev = th.cuda.Event(blocking=True)
        ev.record(th.cuda.current_stream(dev))
        ring["done"][k] = ev
        return out

    def schedule(self):
        """Returns (skip_guidance, current_cutn) per cgd.py:155-175."""
        return guidance_schedule(self.diffusion.num_timesteps, self.current_timestep, self.num_cutouts, self.reduce_clip,
                                 self.progressive_cutout)

    def fac_index(self):
        return self.current_timestep

    def secondary_level(self):
        """(alpha, sigma, t) of the secondary model at this step: sqrt(abar) and sqrt(1 - abar) at the table row `fac_index()` that `fac` comes
        from, and the model's own time t = atan2(sigma, alpha) 2 / pi (alpha = cos(t pi / 2), sigma = sin(t pi / 2))."""
        tables = getattr(self.diffusion, "tables", self.diffusion)
        i = self.fac_index()
        alpha, sigma = float(tables.sqrt_alphas_cumprod[i]), float(tables.sqrt_one_minus_alphas_cumprod[i])
        return alpha, sigma, math.atan2(sigma, alpha) * 2.0 / math.pi

    # -- the native gradient ---------------------------------------------------------------------------
    def native(self, x, x0, x_in, coef, ts=None):
        """x, x0 = pred_xstart, x_in = blend: (B,3,H,W) on the GPU.  Returns g (B,3,H,W) or None when the
        reduce_clip gate skips this step (the reference returns zeros_like(x)).  With a secondary model, x0 and x_in are replaced by
        its prediction from x and the blend of that, and g = -dL/dx runs back through it instead of through the UNet.  `ts` (B,): the model
        timesteps the UNet's forward received at this step (default: `step_ts`, which the sampler sets); only a classifier reads them."""
        skip, cutn = self.schedule()
        self.last_ran = not skip
        if skip:
            return None
        ctx, lib = self.ctx, self.ctx.lib
        B, _, H, W = x.shape
        dev = x.device
        s = ctx.stream()
        resized = isinstance(self.make_cutouts, MakeCutoutsResized)
        if self.dirs_list is not None:
            self._direction_source_on(dev, B, H, W)  # refuses a source of another size before anything is drawn or launched
        if self.regions is not None:
            if (self.regions.H, self.regions.W) != (H, W):
                raise ValueError(f"the region masks are {self.regions.H} x {self.regions.W}, the sample is {H} x {W}")
            if self._reg_t is None or self._reg_t.sat is None or self._reg_t.sat.device != dev:  # one upload; both parts share the tables
                self.regions.to(dev)
                self._reg_t, self._reg_d = (self.regions.columns(c) for c in self._reg_cols)
        if self.coords_tape is not None:
            coords = self.coords_tape[self.calls]
        elif resized:  # (ox, oy, w, h, flags) records; this step's counts from the cutter's own schedule
            coords = self.make_cutouts.draw(W, H, self.cached_cutouts, self.make_cutouts.counts(self.fraction_done()))
        else:
            coords = self.make_cutouts.draw(H, W, self.cached_cutouts, cutn)
        self.calls += 1
        self.make_cutouts.last_coords = coords
        cutn = len(coords)
        geo = self._upload_geometry(resize_table(coords, H, W) if resized else crop_geometry(coords, H, W), dev)
        N = cutn * B
        wm = self._wm.get(B)
        if wm is None and self.dirs_list is not None:
            wm = self._split_weight_matrix(B, dev)
        if wm is None and not self.no_clip and self.weights.numel() > 0:  # (no prompt at all: the CLIP leg runs for the aesthetic heads alone)
            if self.shard is None:
                wm = prompt_weight_matrix(self.weights.cpu(), B, dev)
            else:  # the B <-> P broadcast rule is decided on the GLOBAL batch (sample b <-> prompt b when B == P)
                wm = prompt_weight_matrix(self.weights.cpu(), self.shard[1], dev)[self.shard[0]].contiguous()
            self._wm[B] = wm
        sec = self.secondary
        if sec is not None:
            alpha, sigma, t_sec = self.secondary_level()
            x0, x_in = sec.forward(x, self._b("sec_t", (B,), dev).fill_(t_sec), fac=coef.fac, pred=self._b("sec_pred", (B, 3, H, W), dev),
                                   x_in=self._b("sec_xin", (B, 3, H, W), dev))
        gclip = self._b("gclip", (B, 3, H, W), dev)
        acc = 0
        if self.lpips is not None:
            if self._lpips_ref_batch != B:  # the reference broadcasts a (1,3,H,W) init image over the batch (cgd.py:221)
                self.lpips.set_reference(self.init_tensor.to(dev).expand(B, -1, -1, -1).contiguous())
                self._lpips_ref_batch = B
        if self.style is not None:
            if not self._style_set:  # once: the Gram matrices of the style image (every rank of a sharded run computes its own)
                self.style.set_style(self.style_tensor.to(dev), self.style_weights)
                self._style_set = True
            # one trunk pass for the style term and, when there is an init image, the LPIPS term
            with_lp = self.lpips is not None
            self.style_loss, lp, _ = self.style.style_loss_grad(
                x_in, style_scale=self.style_scale, lpips_scale=self.init_scale if with_lp else None, g=gclip, accumulate=False,
                style_loss=self._b("style_loss", (B,), dev), lpips_loss=self._b("lpips_loss", (B,), dev) if with_lp else None)
            if with_lp:
                self.lpips_loss = lp
            acc = 1
        elif self.lpips is not None:
            # d(init_scale * sum_b lpips(x_in_b, init_b)) / dx_in goes into the same buffer as the CLIP gradient w.r.t. x_in
            self.lpips_loss, _ = self.lpips.loss_grad(x_in, grad_scale=self.init_scale, g=gclip, accumulate=False,
                                                      loss=self._b("lpips_loss", (B,), dev))
            acc = 1
        clip_part = self._b("clip_part", (len(self.towers) * N * self._clip_kinds(),), dev)
        self.clip_part = clip_part
        if self.no_clip:
            clip_part.zero_()
            cuts = None
        elif resized:
            scratch = self._b("resize_scratch", (max(1, lib.cgd_cutouts_resize_scratch_floats(B, H, W, cutn)),), dev)  # one query per step
            cuts = _CutLaunch(lib, coords, geo, True, scratch)
        elif self.make_cutouts.augs is not None:
            cuts = _AugCuts(lib, coords, B, H, W, dev)
        else:
            cuts = _CutLaunch(lib, coords, geo)
        if cuts is not None:
            self._clip_leg(x_in, cuts, wm, self._wmd.get(B), gclip, clip_part, acc)
        nblk = lib.cgd_guidance_part_blocks(B, H, W)
        # the saturation term is a mean over the WHOLE batch (cgd.py:214-218): a rank that holds B of the run's shard[1] samples scales
        # it so that its per-sample gradient equals the batched run's (the logged value is then this rank's share of the loss)
        sats = self.sats if self.shard is None else self.sats * (B / float(self.shard[1]))
        gdir = self._b("gdir", (B, 3, H, W), dev)
        lpart = self._b("lpart", (nblk, 3), dev)
        if sec is not None:
            # pred = alpha x - sigma v: the direct part and the seed dL/dv, which the secondary net's dgrad turns into the rest
            seed3 = self._b("seed3", (B, 3, H, W), dev)
            ctx.check(lib.cgd_secondary_combine(ctx.h, gclip.data_ptr(), x_in.data_ptr(), x0.data_ptr(), gdir.data_ptr(), seed3.data_ptr(),
                                                lpart.data_ptr(), B, H, W, coef.fac, alpha, sigma, self.tvs, self.rs, sats, s))
            gunet = sec.dgrad(seed3, self._b("gsec", (B, 3, H, W), dev))
        else:
            seed6 = self._b("seed6", (B, 6, H, W), dev)
            ctx.check(lib.cgd_guidance_combine(ctx.h, gclip.data_ptr(), x_in.data_ptr(), x0.data_ptr(), gdir.data_ptr(), seed6.data_ptr(),
                                               lpart.data_ptr(), B, H, W, coef, self.tvs, self.rs, sats, s))
            gunet = self.unet.dgrad(seed6, self._b("gunet", (B, 3, H, W), dev))
        if self.classifier is not None:
            # L += -scale * sum_b log p(class | x_b, t_b): dL/dx joins the direct part, so the logged Grad, the magnitude clamp and scalars[7]
            # below see the sum and the sampler's update needs no change
            ts = self.step_ts if ts is None else ts
            if ts is None:
                raise ValueError("classifier guidance needs the step's model timesteps: native(..., ts=...) or step_ts")
            ycls = self._buf.get("cls_y")
            if ycls is None or ycls.shape[0] != B or ycls.device != dev:
                ycls = self._buf["cls_y"] = th.full((B,), self.classifier_class, dtype=th.int64, device=dev)
            _, self.classifier_logp = self.classifier.forward(x, ts, ycls, logits=self._b("cls_logits", (B, self.classifier.out_channels), dev),
                                                              logp=self._b("cls_logp", (B,), dev))
            self.classifier.dgrad(-self.classifier_scale, gdir, accumulate=True)
        g = self._b("g", (B, 3, H, W), dev)
        gpart = self._b("gpart", (nblk, 2), dev)
        ctx.check(lib.cgd_grad_finish(ctx.h, gdir.data_ptr(), gunet.data_ptr(), g.data_ptr(), gpart.data_ptr(), B, H, W, s))
        self.scalars = self._b("scalars", (8,), dev)
        ctx.check(lib.cgd_scalars(ctx.h, clip_part.data_ptr(), clip_part.numel(), lpart.data_ptr(), gpart.data_ptr(), B, H, W,
                                  int(self.use_magnitude), self.scalars.data_ptr(), s))
        self._keep = geo
        return g

    def fraction_done(self):
        """Fraction of the run that is done, from the closure counter (as guidance_schedule measures it)."""
        total = self.diffusion.num_timesteps
        return (total - self.current_timestep) / total

    # -- directional loss ------------------------------------------------------------------------------
    def _clip_kinds(self):
        """Partial-loss rows per (tower, cut, sample): one for each kind of CLIP term that is present, in the order spherical (target prompts),
        directional (direction prompts), aesthetic (a head on any tower); 1 without directions and heads, as ever."""
        return self._has_targets() + int(self.dirs_list is not None) + int(self.aes_list is not None)

    def _has_targets(self):
        """1 when the spherical launch is made: with target prompts, and (as ever) in a leg that has neither directions nor heads."""
        return int(self.targets_list[0].shape[0] > 0 or (self.dirs_list is None and self.aes_list is None))

    def _split_weight_matrix(self, B, dev):
        """The B x P matrix of prompt_weight_matrix over targets and directions together (the B <-> P pairing rule sees the whole list,
        rows as `shard` takes them), split by column into the target part (returned, kept in _wm) and the direction part (_wmd)."""
        cols = self.direction_columns
        P = self.weights.numel() + len(cols)
        tcols = [c for c in range(P) if c not in cols]
        full = th.zeros(P)
        full[tcols] = self.weights.cpu()
        full[cols] = self.direction_weights.cpu()
        if self.shard is None:
            m = prompt_weight_matrix(full, B, dev)
        else:
            m = prompt_weight_matrix(full, self.shard[1], dev)[self.shard[0]]
        self._wm[B], self._wmd[B] = m[:, tcols].contiguous(), m[:, cols].contiguous()
        return self._wm[B]

    def _aes_head_on(self, k, dev):
        """Tower k's (D + 1,) head vector on the device (moved there once)."""
        vec, scale = self.aes_list[k]
        if vec.device != dev:
            vec = vec.to(dev)
            self.aes_list[k] = (vec, scale)
        return vec

    def _direction_source_on(self, dev, B, H, W):
        """The source image on the device, (1 or B, 3, H, W): a (1, ...) source is shared by all samples, one with the run's global batch
        gives this rank its rows."""
        hit = self._buf.get("_direction_src")
        if hit is not None and hit[0] == (dev, B, H, W):
            return hit[1]
        src = self.direction_source
        if tuple(src.shape[-2:]) != (H, W):
            raise ValueError(f"direction_source is {src.shape[-2]} x {src.shape[-1]}, the sample is {H} x {W}")
        if self.shard is not None and src.shape[0] == self.shard[1] and src.shape[0] > 1:
            src = src[self.shard[0]]
        if src.shape[0] not in (1, B):
            raise ValueError(f"direction_source holds {src.shape[0]} images, the batch has {B}: give one image or one per sample")
        src = src.to(dev).contiguous()
        self._buf["_direction_src"] = ((dev, B, H, W), src)
        return src

    # -- the CLIP leg ------------------------------------------------------------------------------------
    def _clip_in(self, name, k, tower, n, dev):
        """(buffer, layout) of n cutouts for tower k: the cutout kernels write the patch rows of a ViT tower's patch-embedding GEMM directly
        (layout 1), plain (n,3,cs,cs) images for a ModifiedResNet tower (layout 0)."""
        cs, patch = tower.input_resolution, tower.patch
        if patch:
            gsz = cs // patch
            return self._b(f"{name}patches{k}", (n * gsz * gsz, 3 * patch * patch), dev), 1
        return self._b(f"{name}cut_images{k}", (n, 3, cs, cs), dev), 0

    def _clip_leg(self, x_in, cuts, wm, wmd, gclip, clip_part, accumulate):
        """d(CLIP loss)/dx_in into gclip for every cutter.  `cuts`: this step's _CutLaunch (plain or resized) or _AugCuts.  Per tower, in tower
        order, on the same boxes at the tower's own cut size: cutouts of x_in -> tower forward -> spherical loss (mean over this step's
        cuts, per-row partials into clip_part) -> tower dgrad -> the cutouts' adjoint into gclip (the first tower overwrites unless
        `accumulate`).  With direction prompts the cutouts and the forward of the source image go first, into buffers of their own (the
        tower keeps its last input for dgrad, and dgrad differentiates the LAST forward), the spherical launch is made only with target
        prompts, and the directional loss follows it, accumulating onto the spherical gradient when that ran; partials: per tower the
        spherical rows (if any), then the directional rows.  With cached_cutouts the boxes do not change, and the source embeddings of
        a cut count are computed once.  With a region plan both losses go through their `_regions` entries, which read this step's boxes from
        the cutter's uploaded table; without one the plain entries are called as ever.  With aesthetic heads the aesthetic launch of a tower
        that has one comes last, accumulating iff one of the other two ran; its partials are the last rows of every tower (zeros for a tower
        without a head), and a head sees no region weight.  _clip_leg_torch is the same leg with autograd."""
        ctx, lib = self.ctx, self.ctx.lib
        B, _, H, W = x_in.shape
        dev = x_in.device
        s = ctx.stream()
        cutn = len(cuts.coords)
        N = cutn * B
        dirs_list = self.dirs_list
        if dirs_list is not None:
            src = self._direction_source_on(dev, B, H, W)
            Bs = src.shape[0]
            boxes = [tuple(c) for c in cuts.coords]
            hit = self._src_emb.get((cutn, B)) if self.cached_cutouts else None
            src_embs = hit[1] if hit is not None and hit[0] == boxes else None
            fresh = []
        kinds, has_t = self._clip_kinds(), self._has_targets()
        aes_list = self.aes_list
        if aes_list is not None:  # one row of predicted scores per head, for the log
            self.aes_score = self._b("aes_score", (sum(a is not None for a in aes_list), N), dev)
            heads_done = 0
        acc = accumulate
        for k, (tower, targets) in enumerate(zip(self.towers, self.targets_list)):
            if aes_list is not None and aes_list[k] is None and not has_t and dirs_list is None:
                clip_part[k * N * kinds:(k + 1) * N * kinds].zero_()  # heads only, and none on this tower: it has no term and is not run
                continue
            cut = cuts.per_tower()
            cs, patch = tower.input_resolution, tower.patch
            if dirs_list is not None and src_embs is None:
                src_in, layout = self._clip_in("src_", k, tower, cutn * Bs, dev)
                cut.forward(ctx, src, src_in, cs, layout, patch)
                name = f"src_emb{k}_{cutn}" if self.cached_cutouts else f"src_emb{k}"
                fresh.append(tower.encode_image(src_in, layout=layout, n=cutn * Bs, out=self._b(name, (cutn * Bs, tower.out_dim), dev)))
            clip_in, layout = self._clip_in("", k, tower, N, dev)
            cut.forward(ctx, x_in, clip_in, cs, layout, patch)
            emb = tower.encode_image(clip_in, layout=layout, n=N, out=self._b(f"emb{k}", (N, tower.out_dim), dev))
            demb = self._b(f"demb{k}", (N, tower.out_dim), dev)
            part = clip_part[k * N * kinds:]
            if has_t and self.regions is not None:
                ctx.check(lib.cgd_spherical_loss_regions(ctx.h, emb.data_ptr(), targets.data_ptr(), wm.data_ptr(), demb.data_ptr(), part.data_ptr(),
                                                         cutn, B, targets.shape[0], tower.out_dim, self.cgs, *self._reg_t.args(cuts.geo), s))
            elif has_t:
                ctx.check(lib.cgd_spherical_loss(ctx.h, emb.data_ptr(), targets.data_ptr(), wm.data_ptr(), demb.data_ptr(), part.data_ptr(),
                                                 cutn, B, targets.shape[0], tower.out_dim, self.cgs, s))
            if dirs_list is not None:
                semb, dirs = (fresh if src_embs is None else src_embs)[k], dirs_list[k]
                dir_args = (ctx.h, emb.data_ptr(), semb.data_ptr(), dirs.data_ptr(), wmd.data_ptr(), demb.data_ptr(), part[N * has_t:].data_ptr(),
                            cutn, B, Bs, dirs.shape[0], tower.out_dim, self.cgs, has_t)
                if self.regions is not None:
                    ctx.check(lib.cgd_directional_loss_regions(*dir_args, *self._reg_d.args(cuts.geo), s))
                else:
                    ctx.check(lib.cgd_directional_loss(*dir_args, s))
            if aes_list is not None:
                rows = part[N * (kinds - 1):N * kinds]
                if aes_list[k] is None:  # a tower without a head: zeros in its aesthetic rows
                    rows.zero_()
                else:
                    head = self._aes_head_on(k, dev)
                    ctx.check(lib.cgd_aesthetic_loss(ctx.h, emb.data_ptr(), head.data_ptr(), demb.data_ptr(), rows.data_ptr(),
                                                     self.aes_score[heads_done].data_ptr(), cutn, B, tower.out_dim, aes_list[k][1],
                                                     int(bool(has_t or dirs_list is not None)), s))
                    heads_done += 1
            dclip_in = tower.dgrad(demb, self._b(f"dclip_in{k}", tuple(clip_in.shape), dev))
            cut.backward(ctx, dclip_in, gclip, cs, layout, patch, acc)
            acc = 1
            if k == 0:
                self.emb = emb
        if dirs_list is not None and self.cached_cutouts and src_embs is None:
            self._src_emb[(cutn, B)] = (boxes, fresh)

    def _clip_leg_torch(self, x_in, cuts, wm, wmd, gclip, clip_part, accumulate):
        """The torch restatement of _clip_leg (the equivalence reference of the tests; swap it in with `guid._clip_leg = guid._clip_leg_torch`):
        it follows the reference recipe (cgd.py:190-204) with torch autograd — the cutouts (cuts.torch_cuts) and the normalisation in torch
        ops, the CLIP tower as the autograd node over cgd_*_forward / _dgrad, both losses in torch ops — and hands d(CLIP loss)/dx_in to
        the native chain.  Same draws, in the same order, as the native leg; the source forward runs first here too.  clip_part gets
        each tower's spherical total in the first of its spherical rows, its directional total in the first of its directional rows and its
        aesthetic total in the first of its aesthetic rows; the heads' scores go to aes_score as in the native leg."""
        from .nets import EncodeImageFunction
        B, _, H, W = x_in.shape
        dev = x_in.device
        mean, std = _clip_mean_std(dev)
        n = len(cuts.coords)
        N = n * B
        kinds, has_t = self._clip_kinds(), self._has_targets()
        aes_list = self.aes_list
        if aes_list is not None:
            self.aes_score = self._b("aes_score", (sum(a is not None for a in aes_list), N), dev)
            heads_done = 0
        if self.dirs_list is not None:
            src = self._direction_source_on(dev, B, H, W)
        wm3 = wm.view(1, B, -1) if wm is not None else None
        wmd3 = wmd.view(1, B, -1) if wmd is not None else None
        if self.regions is not None:  # w_eff[cut, b, p] = w[b, p] cov[cut, p] ** power[p], the coverage from the host restatement
            from .regions import boxes_of
            boxes = boxes_of(cuts.coords, H, W, cuts.resized)
            if wm3 is not None and self._reg_t.P:
                wm3 = wm3 * self._reg_t.coverage(boxes).to(dev, th.float32).view(n, 1, -1)
            if wmd3 is not None and self._reg_d.P:
                wmd3 = wmd3 * self._reg_d.coverage(boxes).to(dev, th.float32).view(n, 1, -1)

        def clip_cuts(img, cs):
            return ((cuts.torch_cuts(img.add(1).div(2), cs) - mean) / std).contiguous()

        clip_part.zero_()
        with th.enable_grad():
            xr = x_in.detach().requires_grad_()
            total = 0
            for k, (tower, targets) in enumerate(zip(self.towers, self.targets_list)):
                if aes_list is not None and aes_list[k] is None and not has_t and self.dirs_list is None:
                    continue  # heads only, and none on this tower
                if self.dirs_list is not None:
                    with th.no_grad():
                        sn = F.normalize(tower.encode_image(clip_cuts(src, tower.input_resolution)).clone().view(n, src.shape[0], -1), dim=-1)
                emb = EncodeImageFunction.apply(clip_cuts(xr, tower.input_resolution), tower).view(n, B, -1)
                en = F.normalize(emb, dim=-1)
                if self.dirs_list is not None:
                    delta = en - sn
                    live = delta.norm(dim=-1, keepdim=True) > 1e-6
                    safe = th.where(live, delta, th.ones_like(delta))
                    cos = th.where(live, (safe / safe.norm(dim=-1, keepdim=True)) @ self.dirs_list[k].t(), th.zeros((), device=dev))  # (n, B, P_d)
                    l_dir = ((1 - cos) * wmd3).sum(2).mean(0).sum() * self.cgs
                    total = total + l_dir
                    clip_part[k * N * kinds + N * has_t] = l_dir.detach()
                if has_t:
                    d = (en.unsqueeze(2) - targets.view(1, 1, -1, targets.shape[-1])).norm(dim=-1).div(2).arcsin().pow(2).mul(2)  # (n, B, P)
                    l_sph = (d * wm3).sum(2).mean(0).sum() * self.cgs
                    total = total + l_sph
                    clip_part[k * N * kinds] = l_sph.detach()
                if aes_list is not None and aes_list[k] is not None:
                    head = self._aes_head_on(k, dev)
                    score = en @ head[:-1] + head[-1]  # (n, B)
                    l_aes = score.mean(0).sum() * -aes_list[k][1]
                    total = total + l_aes
                    clip_part[k * N * kinds + N * (kinds - 1)] = l_aes.detach()
                    self.aes_score[heads_done] = score.detach().reshape(N)
                    heads_done += 1
                if k == 0:
                    self.emb = emb.detach().view(N, -1)
            g_in, = th.autograd.grad(total, xr)
        if accumulate:
            gclip.add_(g_in)
        else:
            gclip.copy_(g_in)

    def snapshot(self):
        """Asynchronous host copies of the last call's scalars: `log(snapshot)` later costs no wait on newer GPU work."""
        from .hostcopy import HostCopy
        snap = {"scalars": HostCopy(self.scalars.clone()), "lpips": HostCopy(self.lpips_loss.clone()) if self.lpips is not None else None}
        if self.style is not None:
            snap["style"] = HostCopy(self.style_loss.clone())
        if self.classifier is not None:
            snap["classifier"] = HostCopy(self.classifier_logp.clone())
        if self.dirs_list is not None:
            snap["direction"] = HostCopy(self.clip_part.clone())
        if self.aes_list is not None:
            snap["aesthetic"] = snap["direction"] if "direction" in snap else HostCopy(self.clip_part.clone())  # one copy of the partials
            snap["aesthetic_score"] = HostCopy(self.aes_score.clone())
        return snap

    def _direction_share(self, clip_part):
        """The directional rows of the per-tower partials (towers, kinds, N): their sum is the directional share of 'CLIP Loss'."""
        return float(clip_part.double().view(len(self.towers), self._clip_kinds(), -1)[:, self._has_targets()].sum().item())

    def _aesthetic_share(self, clip_part):
        """The aesthetic rows of the per-tower partials, the last kind: their sum is the aesthetic share of 'CLIP Loss'."""
        return float(clip_part.double().view(len(self.towers), self._clip_kinds(), -1)[:, -1].sum().item())

    def log(self, snapshot=None):
        """Scalar log of the last call (or of a `snapshot()`) with the reference's keys (one host sync; call lazily)."""
        v = (snapshot["scalars"].get() if snapshot is not None else self.scalars).tolist()
        lpips_loss = snapshot["lpips"].get() if (snapshot is not None and snapshot["lpips"] is not None) else self.lpips_loss
        out = {"CLIP Loss": v[0], "Range Loss": v[2], "TV Loss": v[1]}
        if self.dirs_list is not None:  # already part of 'CLIP Loss' and 'Total Loss' (cgd_scalars sums every partial row)
            out["Direction Loss"] = self._direction_share(snapshot["direction"].get() if snapshot is not None else self.clip_part)
        if self.aes_list is not None:  # likewise part of 'CLIP Loss'; the score is the mean over cuts, samples and heads
            out["Aesthetic Loss"] = self._aesthetic_share(snapshot["aesthetic"].get() if snapshot is not None else self.clip_part)
            out["Aesthetic Score"] = float((snapshot["aesthetic_score"].get() if snapshot is not None else self.aes_score).double().mean().item())
        if self.sats != 0:
            out["Saturation Loss"] = v[3]
        out["Total Loss"] = v[4]
        if self.lpips is not None:
            out["Init VGG Loss"] = float(lpips_loss.sum().item()) * self.init_scale
            out["Total Loss"] += out["Init VGG Loss"]
        if self.style is not None:
            style_loss = snapshot["style"].get() if snapshot is not None else self.style_loss
            out["Style Loss"] = float(style_loss.sum().item()) * self.style_scale
            out["Total Loss"] += out["Style Loss"]
        if self.classifier is not None:
            logp = snapshot["classifier"].get() if snapshot is not None else self.classifier_logp
            out["Classifier Loss"] = -self.classifier_scale * float(logp.sum().item())
            out["Total Loss"] += out["Classifier Loss"]
        if self.use_magnitude:
            out["Magnitude"] = v[5]
        out["Grad"] = v[6]
        return out

    # -- reference plugin signature ----------------------------------------------------------------------
    def __call__(self, x, t, out, y=None, low_res=None):
        """cond_fn(x, t, out, y=None): `out['pred_xstart']` must come from the last `unet.forward(x, ...)`.  `low_res` (super-resolution
        sampling hands the whole model_kwargs to cond_fn, as upstream does) is accepted and ignored."""
        coef = self.diffusion.step_coef(int(t.flatten()[0].item()), self.fac_index())
        x = x.detach().contiguous().float()
        x0 = out["pred_xstart"].detach().contiguous().float()
        x_in = (x0 * coef.fac + x * (1 - coef.fac)).contiguous()
        ts = None
        if self.classifier is not None:  # the model timestep of index t, as the sampler hands it to the UNet
            tables = getattr(self.diffusion, "tables", self.diffusion)
            ts = th.tensor([float(tables.model_timestep(int(k))) for k in t.flatten().tolist()], dtype=th.float32, device=x.device)
        g = self.native(x, x0, x_in, coef, ts=ts)
        if g is None:
            return th.zeros_like(x)
        if self.use_magnitude:
            g = g * self.scalars[7]
        return g.clone()
