"""Keyframed 2D animation in the manner of Disco Diffusion's 2D mode and Deforum: frame k is sampled from frame k - 1 after zooming,
rotating and shifting it and noising it part of the way up the schedule; an LPIPS term holds it to the warped frame, and the text prompts may
change at keyframes.

    python -m cgd_amd.animate --frames 120 --zoom "0:(1.02)" --angle "0:(0),60:(2)" --translation_x 0 --translation_y "0:(0),120:(-40)" \\
        --border wrap --interp bicubic --frames_skip 0.6 --frames_scale 1500 --color_match 1 [--fixed_seed] \\
        [--prompts_at "40=a city at night|a skyline:0.5"]... -- <cgd command-line flags>
    python -m cgd_amd.animate --frames 120 --mode 3d --translation_z "0:(4)" --rotation_3d_y "0:(0),60:(0.5)" --translation_x 2 --fov 40 \\
        [--depth_model dpt_large-midas-2f21e586.pt[:size=384][:offset=50][:scale=19] | --depth_fn MODULE:FUNCTION] [--depth_iters 2] ... \\
        -- <cgd command-line flags>

    python -m cgd_amd.animate --frames 120 --mode video --video_frames DIR_OR_GLOB [--flow_blend 0.999] [--check_consistency] \\
        [--flow_levels 4] [--flow_iters 4] [--flow_radius 4] ... -- <cgd command-line flags>

or, from Python, `animate(frames, zoom=..., **clip_guided_diffusion_kwargs)`, a generator of `(frame_idx, batch_idx, png_path)`.

Networks, cutout maker, tables and guidance are built once (cgd.cgd.prepare_run) and every frame runs the sampler loop on them.  Between two
frames the state stays fp32 on the GPU: the final `sample` of frame k - 1 goes through cgd_frame_warp (one launch, csrc/warp.hip) and, with
`color_match`, through cgd_color_match against frame 0's channel statistics; nothing passes through a file or through 8 bits.

Conventions (motion_matrix).  The forward map of a frame is p' = t + c + z R(theta) (p - c) with
  c = ((W - 1) / 2, (H - 1) / 2), the geometric centre of the pixel grid (pixel centres sit on integers).  Disco Diffusion and OpenCV recipes
      use (W // 2, H // 2), which on even sizes lies half a pixel to the lower right: a pure zoom or rotation there drifts by up to half a
      pixel per frame toward the upper left, and a 180 degree turn is no permutation of the pixels.  Here it is;
  R(theta) = [[cos, sin], [-sin, cos]], OpenCV's getRotationMatrix2D convention: a positive angle (degrees) turns the picture
      counter-clockwise on the screen (y points down);
  t = (translation_x, translation_y): positive values move the content right and down;
  z = zoom: above 1 magnifies.
The kernel takes the inverse map, which is what motion_matrix returns.

3D mode (`--mode 3d`, Disco's and Deforum's 3D animation): the previous frame is seen by a pinhole camera that has moved, with a depth for
every pixel, so that near things move faster than far ones (cgd_frame_warp3d, csrc/warp3d.hip).  Conventions (camera, project, unproject):
  axes x right, y down, z into the screen; c as above; focal length f = (H / 2) / tan(fov / 2) pixels, fov the vertical field of view in
      degrees (default 40); a source position q of depth z is the point X = z ((qx - cx) / f, (qy - cy) / f, 1);
  between two frames X' = R X + T, seen at c + f (X'x, X'y) / X'z, with T = (translation_x, translation_y, -translation_z) / 200 (the 1 / 200
      is Deforum's translation scale as remembered, not checked against its source) and R = Rx(rotation_3d_x) Ry(rotation_3d_y)
      Rz(rotation_3d_z), degrees, Rx(a) = [[1,0,0],[0,cos,sin],[0,-sin,cos]], Ry(b) = [[cos,0,-sin],[0,1,0],[sin,0,cos]],
      Rz(c) = [[cos,sin,0],[-sin,cos,0],[0,0,1]];
  on the screen: translation_x > 0 moves the content right by f tx / 200 / z pixels (parallax), translation_y > 0 down, translation_z > 0
      flies forward (at flat depth z0 a magnification of z0 / (z0 - tz / 200)), rotation_3d_z > 0 turns the picture counter-clockwise like
      `angle`, rotation_3d_y > 0 turns the camera right (content moves left), rotation_3d_x > 0 tilts it up (content moves down).  These
      signs are this project's own; they have not been compared with Deforum's.
Depth is flat (Deforum's use_depth_warping=False), the caller's (a tensor, or a callable of the previous frame), or DPT-Large's
(`--depth_model FILE`, nets.DepthNet: the MiDaS network Disco Diffusion and Deforum use, run natively once per frame).

Video mode (`--mode video`, Disco Diffusion's video input and Warp notebooks, Deforum's hybrid video): an existing clip is stylised.  The motion
is not typed in but estimated from the clip, natively (csrc/flow.hip): dense pyramidal Lucas-Kanade optical flow, then a warp that follows it.
  A flow is (B, 2, H, W) fp32, channel 0 the x displacement in pixels (positive: right), channel 1 the y displacement (positive: down), pixel
      centres on integers; ops.flow_estimate(tmpl, img) returns F with img(p + F(p)) ~ tmpl(p).
  Frame 0 starts from video frame 0 (the init image, skip_timesteps = round(frames_skip T), LPIPS weight frames_scale).  Frame k > 0 takes
      F = flow_estimate(video_k, video_{k-1}), so that the previous stylised frame read at p + F(p) lies where the clip's frame k has it, and
      starts from  w S(p + F(p)) + (1 - w) video_k(p),  w = flow_blend m(p): `flow_blend` is the share of the warped previous stylised frame
      where the flow is trusted (m = 1); the rest, and everything where it is not (m = 0), is the clip's own frame k.  With
      `check_consistency` the flow of the opposite direction is estimated too and m = 0 where the two disagree (occlusions) or where the
      flow leaves the frame; without it m = 1 everywhere.
  `border` and `interp` are the warp's, as in the other modes.  The driver's default border, wrap, suits a tiling 2D zoom and is a poor choice
      for a clip: a flow that points out of the frame then reads the opposite edge.  Give `--border replicate` (or reflect), or
      `--check_consistency`, which falls back to the clip's frame wherever the flow leaves the frame.
  Only the clip's frames k - 1 and k are on the GPU at a time.  Image quality on trained weights and on real footage has not been judged here:
      only seeded random weights and synthetic clips were available.
"""
import argparse
import collections
import glob
import importlib
import math
import re
import sys

BORDERS = ("wrap", "reflect", "replicate")
INTERPS = ("bilinear", "bicubic")
MODES = ("2d", "3d", "video")
VIDEO_EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".webp", ".tif", ".tiff")
VIDEO_DEFAULTS = dict(video_frames=None, flow_blend=0.999, check_consistency=False, flow_levels=4, flow_iters=4, flow_radius=4)
TRANSLATION_SCALE = 200.0

Camera = collections.namedtuple("Camera", "R T f cx cy z0 near")

_KEY = re.compile(r"^\s*([^:\s]+)\s*:\s*\(\s*([^()\s]+)\s*\)\s*$")


def _number(text, what):
    try:
        value = float(text)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {text!r} is not a number") from None
    if not math.isfinite(value):
        raise ValueError(f"{what}: {text!r} is not finite")
    return value


def keyframes(spec, frames):
    """Disco's keyframe syntax '0:(1.0), 30:(1.04), 90:(1.0)' (or a bare number) -> one float per frame: linear between keys, the first
    value before the first key, the last value after the last key.  ValueError on malformed text, a repeated key, or a key frame that is
    negative or no integer."""
    frames = int(frames)
    if frames < 1:
        raise ValueError(f"frames must be at least 1, got {frames}")
    if isinstance(spec, bool):
        raise ValueError(f"keyframes: {spec!r} is not a number")
    if isinstance(spec, (int, float)):
        return [_number(spec, "keyframes")] * frames
    text = str(spec).strip()
    if not text:
        raise ValueError("keyframes: empty")
    if ":" not in text and "(" not in text and "," not in text:
        return [_number(text, "keyframes")] * frames
    keys = {}
    for item in text.split(","):
        m = _KEY.match(item)
        if m is None:
            raise ValueError(f"keyframes {spec!r}: {item.strip()!r} is not 'FRAME:(VALUE)'")
        if not re.fullmatch(r"\+?\d+", m.group(1)):
            raise ValueError(f"keyframes {spec!r}: the frame {m.group(1)!r} must be a non-negative integer")
        frame = int(m.group(1))
        if frame in keys:
            raise ValueError(f"keyframes {spec!r}: frame {frame} is given twice")
        keys[frame] = _number(m.group(2), f"keyframes {spec!r}")
    at = sorted(keys)
    out = []
    for k in range(frames):
        if k <= at[0]:
            out.append(keys[at[0]])
        elif k >= at[-1]:
            out.append(keys[at[-1]])
        else:
            hi = next(i for i, f in enumerate(at) if f >= k)
            f0, f1 = at[hi - 1], at[hi]
            u = (k - f0) / (f1 - f0)
            out.append(keys[f1] if k == f1 else keys[f0] + (keys[f1] - keys[f0]) * u)
    return out


def motion_matrix(zoom, angle_deg, tx, ty, H, W):
    """The six float64 entries (m0 .. m5) of the INVERSE map of p' = t + c + zoom R(angle) (p - c) (module docstring): destination pixel
    (x, y) reads the source at (m0 x + m1 y + m2, m3 x + m4 y + m5)."""
    zoom, angle_deg, tx, ty = (_number(v, n) for v, n in ((zoom, "zoom"), (angle_deg, "angle"), (tx, "translation_x"), (ty, "translation_y")))
    if not zoom > 0:
        raise ValueError(f"zoom must be positive, got {zoom}")
    if H < 1 or W < 1:
        raise ValueError(f"the frame must be at least 1 x 1, got {H} x {W}")
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    a = math.radians(angle_deg)
    cos, sin = math.cos(a), math.sin(a)
    # p = c + R^T (p' - t - c) / zoom,  R^T = [[cos, -sin], [sin, cos]]
    ux, uy = tx + cx, ty + cy
    return (cos / zoom, -sin / zoom, cx - (cos * ux - sin * uy) / zoom,
            sin / zoom, cos / zoom, cy - (sin * ux + cos * uy) / zoom)


def forward_matrix(zoom, angle_deg, tx, ty, H, W):
    """The forward map itself, in the same row layout (for tests and for drawing motion paths)."""
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    a = math.radians(angle_deg)
    cos, sin = math.cos(a) * zoom, math.sin(a) * zoom
    return (cos, sin, tx + cx - (cos * cx + sin * cy), -sin, cos, ty + cy - (-sin * cx + cos * cy))


def camera(tx, ty, tz, rx, ry, rz, fov, H, W, z0=1.0, near=0.05):
    """The Camera (R as 9 row-major float64 entries, T, f, cx, cy, z0, near) of one frame's 3D motion (module docstring): translations in
    Deforum units (1 / 200 of a depth unit), rotations and the vertical field of view `fov` in degrees.  ValueError on a non-finite value, a
    fov outside (0, 180), or a z0 or near that is not positive."""
    tx, ty, tz, rx, ry, rz, fov, z0, near = (_number(v, n) for v, n in (
        (tx, "translation_x"), (ty, "translation_y"), (tz, "translation_z"), (rx, "rotation_3d_x"), (ry, "rotation_3d_y"),
        (rz, "rotation_3d_z"), (fov, "fov"), (z0, "z0"), (near, "near")))
    if not 0 < fov < 180:
        raise ValueError(f"fov must lie in (0, 180) degrees, got {fov}")
    if not z0 > 0 or not near > 0:
        raise ValueError(f"z0 and near must be positive, got {z0} and {near}")
    if H < 1 or W < 1:
        raise ValueError(f"the frame must be at least 1 x 1, got {H} x {W}")
    (ca, sa), (cb, sb), (cc, sc) = ((math.cos(math.radians(v)), math.sin(math.radians(v))) for v in (rx, ry, rz))
    # Rx(a) Ry(b) Rz(c), written out
    R = (cb * cc, cb * sc, -sb,
         sa * sb * cc - ca * sc, sa * sb * sc + ca * cc, sa * cb,
         ca * sb * cc + sa * sc, ca * sb * sc - sa * cc, ca * cb)
    R = tuple(v + 0.0 for v in R)  # no negative zeros: an identity camera is the identity matrix to the bit
    T = (tx / TRANSLATION_SCALE, ty / TRANSLATION_SCALE, -tz / TRANSLATION_SCALE + 0.0)
    return Camera(R, T, (H / 2.0) / math.tan(math.radians(fov) / 2.0), (W - 1) / 2.0, (H - 1) / 2.0, z0, near)


def project(cam, q, z):
    """Forward map: where the source position q = (x, y) of depth z is seen after the camera's motion."""
    X = (z * (q[0] - cam.cx) / cam.f, z * (q[1] - cam.cy) / cam.f, z)
    R, T = cam.R, cam.T
    Y = [R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + T[i] for i in range(3)]
    return cam.cx + cam.f * Y[0] / Y[2], cam.cy + cam.f * Y[1] / Y[2]


def unproject(cam, p, z):
    """Backward map G(p, z): the source position that a source point of depth z must have to be seen at p = (x, y); what the kernel
    evaluates (a_z is kept at or above 1e-6 and lambda at or above near, which the exact inverse never needs inside the view)."""
    r = ((p[0] - cam.cx) / cam.f, (p[1] - cam.cy) / cam.f, 1.0)
    R, T = cam.R, cam.T
    a = [R[i] * r[0] + R[3 + i] * r[1] + R[6 + i] * r[2] for i in range(3)]
    b = [R[i] * T[0] + R[3 + i] * T[1] + R[6 + i] * T[2] for i in range(3)]
    a[2] = max(a[2], 1e-6)
    lam = max((z + b[2]) / a[2], cam.near)
    return cam.cx + cam.f * (lam * a[0] - b[0]) / z, cam.cy + cam.f * (lam * a[1] - b[1]) / z


def parse_prompts_at(values):
    """CLI '--prompts_at "40=a city at night|a skyline:0.5"' entries -> {40: ['a city at night', 'a skyline:0.5']}."""
    out = {}
    for value in values or []:
        frame, sep, text = str(value).partition("=")
        if not sep or not re.fullmatch(r"\s*\d+\s*", frame) or not text.strip():
            raise ValueError(f"prompts_at {value!r}: expected 'FRAME=prompt|prompt...'")
        if int(frame) in out:
            raise ValueError(f"prompts_at: frame {int(frame)} is given twice")
        out[int(frame)] = text.split("|")
    return out


def _check(frames, border, interp, frames_skip, frames_scale, color_match, prompts_at, kw):
    """Every refusal of animate that needs nothing loaded -> (frames, prompts_at as {int: [str]})."""
    from cgd import script_util
    from cgd_amd import diffusion as dd
    from cgd_amd import shard
    if isinstance(frames, bool) or int(frames) != frames or frames < 1:
        raise ValueError(f"frames must be an integer of at least 1, got {frames!r}")
    frames = int(frames)
    if border not in BORDERS or interp not in INTERPS:
        raise ValueError(f"border must be one of {BORDERS} and interp one of {INTERPS}, got {border!r} and {interp!r}")
    if not (0 <= frames_skip < 1):
        raise ValueError(f"frames_skip must lie in [0, 1), got {frames_skip!r}")
    if not (frames_scale >= 0):
        raise ValueError(f"frames_scale must not be negative, got {frames_scale!r}")
    if not (0 <= color_match <= 1):
        raise ValueError(f"color_match must lie in [0, 1], got {color_match!r}")
    if kw.get("use_augs"):
        raise ValueError("animate does not work with use_augs")
    if shard.world()[1] > 1:
        raise ValueError("animate runs in one process: frames are sequential, a sharded run would leave the other GPUs idle")
    init = kw.get("init_image")
    if init:
        image, mask = script_util.split_init_mask(init)
        if mask is not None:
            raise ValueError(f"init image {init!r}: animate takes a plain init image for frame 0, not '::MASK'")
        for what, split in (("invert=", script_util.split_init_invert), ("upsample=", script_util.split_init_upsample),
                            ("ilvrN=", script_util.split_init_ilvr)):
            if split(image)[1]:
                raise ValueError(f"init image {init!r}: animate takes a plain init image for frame 0, not '{what}'")
    plan = {}
    for frame, texts in (prompts_at or {}).items():
        if isinstance(frame, bool) or int(frame) != frame or frame < 0:
            raise ValueError(f"prompts_at: the frame {frame!r} must be a non-negative integer")
        texts = [texts] if isinstance(texts, str) else list(texts)
        if not texts:
            raise ValueError(f"prompts_at[{frame}]: at least one prompt")
        plan[int(frame)] = texts
    every = list(kw.get("prompts") or []) + [t for texts in plan.values() for t in texts]
    if any(script_util.split_direction(script_util.parse_prompt(p)[0]) is not None for p in every):
        raise ValueError("animate does not take 'SOURCE=>TARGET' prompts: the source image would change every frame")
    if plan:
        if any(script_util.REGION_SEP in str(p) for p in every + list(kw.get("image_prompts") or [])):
            raise ValueError("prompts_at does not work with 'TEXT@@REGION' prompts: the region plan is built once, over the first prompt list")
        for frame, texts in plan.items():
            if abs(sum(script_util.parse_prompt(t)[1] for t in texts) + 0.0) < 1e-3 and not kw.get("image_prompts"):
                raise ValueError(f"prompts_at[{frame}]: the weights must not sum to 0")
    # how many steps the run has, from the tables alone (the suffixes of the spacing are the generator's to judge)
    spacing = script_util.split_model(kw.get("timestep_respacing", "1000"))[0]  # '+model=' is the last suffix and comes off first
    spacing = script_util.split_threshold(script_util.split_windows(spacing)[0])[0]
    steps = dd.create_gaussian_diffusion(kw.get("diffusion_steps", 1000), kw.get("noise_schedule", "linear"), spacing).num_timesteps
    if frames > 1 and round(frames_skip * steps) >= steps:
        raise ValueError(f"frames_skip {frames_skip} leaves no step of the {steps} for the frames after the first")
    return frames, plan


def parse_depth_model(spec):
    """'FILE[:size=N][:offset=A][:scale=B]' -> (FILE, {'size': int, 'offset': float, 'scale': float} of the options given); None -> None.
    ValueError for an empty file name, an unknown or repeated option, or a value that is no number."""
    if spec is None:
        return None
    file, *opts = str(spec).split(":")
    if not file.strip():
        raise ValueError(f"depth_model {spec!r}: expected 'FILE[:size=N][:offset=A][:scale=B]'")
    out = {}
    for opt in opts:
        key, sep, val = opt.partition("=")
        key = key.strip()
        if not sep or key not in ("size", "offset", "scale") or key in out:
            raise ValueError(f"depth_model {spec!r}: {opt!r} is not one of size=N, offset=A, scale=B (each at most once)")
        try:
            out[key] = int(val) if key == "size" else float(val)
        except ValueError:
            raise ValueError(f"depth_model {spec!r}: {val!r} is no number") from None
        if not math.isfinite(out[key]) or (key == "size" and out[key] < 32) or (key == "scale" and out[key] == 0):
            raise ValueError(f"depth_model {spec!r}: size must be at least 32, offset finite, scale finite and not 0")
    return file.strip(), out


def load_depth_model(ctx, spec):
    """The DepthNet of a parsed `depth_model` on the run's context: the checkpoint FILE (a torch file holding the published state dict, or
    {'state_dict': ...}); with CGD_SYNTHETIC_WEIGHTS=1 a known file name gets seeded random weights and FILE is not read."""
    import os

    import torch as th

    from cgd import script_util
    from cgd_amd import nets, synthetic
    file, opts = spec
    config = nets.DEPTH_CHECKPOINTS.get(os.path.basename(file), "dpt_large")
    if script_util.synthetic_weights_enabled():
        if os.path.basename(file) not in nets.DEPTH_CHECKPOINTS:
            raise ValueError(f"depth_model {file!r}: with CGD_SYNTHETIC_WEIGHTS=1 the file is not read, so only {sorted(nets.DEPTH_CHECKPOINTS)} work")
        sd = synthetic.depth_state_dict(config)
    elif not os.path.isfile(file):
        raise FileNotFoundError(f"{file} not found (set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")
    else:
        sd = th.load(file, map_location="cpu")
        if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
            sd = sd["state_dict"]
    return nets.DepthNet(ctx, config, **opts).load_state_dict(sd)


def list_video_frames(spec):
    """The clip of video mode: a tensor (N, 3, H, W) in [-1, 1] passes through; a directory gives its image files (VIDEO_EXTENSIONS) and a
    glob pattern its matches, both in name order; a list or tuple of paths is taken as it stands.  ValueError for anything else."""
    import os
    if spec is None:
        raise ValueError("mode='video' needs video_frames: a directory, a glob, a list of paths or a tensor (N, 3, H, W)")
    if hasattr(spec, "dim"):
        if spec.dim() != 4 or spec.shape[1] != 3:
            raise ValueError(f"video_frames: a tensor must be (N, 3, H, W), got {tuple(spec.shape)}")
        return spec
    if isinstance(spec, (list, tuple)):
        return [os.fspath(p) for p in spec]
    spec = os.fspath(spec)
    if os.path.isdir(spec):
        return [os.path.join(spec, n) for n in sorted(os.listdir(spec)) if n.lower().endswith(VIDEO_EXTENSIONS)]
    return sorted(glob.glob(spec))


def _check_video(mode, frames, video, motion, motion3d, fov, depth, depth_iters, near, depth_model, kw):
    """The refusals of video mode and of its arguments in the other modes, before anything is loaded -> the clip (list_video_frames) or
    None.  `video`: the six video arguments by name; `motion`: zoom, angle, translation_x, translation_y."""
    if mode != "video":
        given = [n for n, v in video.items() if v is not VIDEO_DEFAULTS[n] and v != VIDEO_DEFAULTS[n]]
        if given:
            raise ValueError(f"{', '.join(given)}: only with mode='video'")
        return None
    names = ("zoom", "angle", "translation_x", "translation_y", "translation_z", "rotation_3d_x", "rotation_3d_y", "rotation_3d_z", "fov")
    neutral = (1, 0, 0, 0, 0, 0, 0, 0, 40)
    given = [n for n, spec, v0 in zip(names, tuple(motion) + tuple(motion3d) + (fov,), neutral) if any(v != v0 for v in keyframes(spec, frames))]
    given += ["depth"] * (depth is not None) + ["depth_iters"] * (depth_iters != 1) + ["near"] * (near != 0.05)
    given += ["depth_model"] * (depth_model is not None)
    if given:
        raise ValueError(f"{', '.join(given)}: not with mode='video', where the motion comes from the clip")
    if kw.get("init_image"):
        raise ValueError("mode='video' takes no init_image: frame 0 starts from the clip's first frame")
    if not (0 <= video["flow_blend"] <= 1):
        raise ValueError(f"flow_blend must lie in [0, 1], got {video['flow_blend']!r}")
    for name, lo, hi in (("flow_levels", 1, 8), ("flow_iters", 1, 16), ("flow_radius", 1, 7)):
        v = video[name]
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    clip = list_video_frames(video["video_frames"])
    if len(clip) < 1:
        raise ValueError(f"video_frames {video['video_frames']!r}: fewer than one frame")
    if frames > len(clip):
        raise ValueError(f"frames = {frames}, but the clip has {len(clip)} frames")
    return clip


def _video_frame(clip, k, B, H, W, device):
    """Frame k of the clip as (B, 3, H, W) fp32 in [-1, 1] on `device`: a file is opened with PIL and resized to the run's frame as the
    init image is; a tensor must have the run's frame size."""
    import numpy as np
    import torch as th
    if hasattr(clip, "dim"):
        if tuple(clip.shape[2:]) != (H, W):
            raise ValueError(f"video_frames: the tensor's frames are {tuple(clip.shape[2:])}, the run's {(H, W)}")
        frame = clip[k:k + 1].detach().to(device=device, dtype=th.float32)
    else:
        from PIL import Image
        pil = Image.open(clip[k]).convert("RGB").resize((W, H))
        frame = th.from_numpy(np.array(pil)).float().div(255).permute(2, 0, 1).to(device).unsqueeze(0).mul(2).sub(1)
    return frame.expand(B, -1, -1, -1).contiguous()


def _check_mode(mode, frames, zoom, angle, motion3d, fov, depth, depth_iters, near, depth_model=None):
    """The refusals of the mode arguments, before anything is loaded -> the five 3D tracks (translation_z, rotation_3d_x / y / z, fov)."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    names = ("translation_z", "rotation_3d_x", "rotation_3d_y", "rotation_3d_z")
    tracks = [keyframes(spec, frames) for spec in motion3d] + [keyframes(fov, frames)]
    if isinstance(depth_iters, bool) or not isinstance(depth_iters, int) or not 1 <= depth_iters <= 4:
        raise ValueError(f"depth_iters must be an integer in 1..4, got {depth_iters!r}")
    near = _number(near, "near")
    if not near > 0:
        raise ValueError(f"near must be positive, got {near}")
    if any(not 0 < v < 180 for v in tracks[4]):
        raise ValueError("fov must stay inside (0, 180) degrees on every frame")
    if mode == "2d":
        given = [n for n, t in zip(names, tracks) if any(v != 0 for v in t)]
        given += ["fov"] * any(v != 40 for v in tracks[4]) + ["depth"] * (depth is not None) + ["depth_iters"] * (depth_iters != 1)
        given += ["near"] * (near != 0.05) + ["depth_model"] * (depth_model is not None)
        if given:
            raise ValueError(f"{', '.join(given)}: only with mode='3d'")
        return tracks
    if any(v != 1 for v in keyframes(zoom, frames)) or any(v != 0 for v in keyframes(angle, frames)):
        raise ValueError("mode='3d' takes no zoom or angle: fly with translation_z and turn with rotation_3d_z")
    if depth is not None and depth_model is not None:
        raise ValueError("depth_model and depth (--depth_fn) exclude each other: one source of depth")
    if depth is not None and not callable(depth):
        import torch as th
        if not isinstance(depth, th.Tensor) or depth.dim() not in (2, 4):
            raise ValueError("depth must be None, a callable, or a tensor (1 or B, 1, H, W) or (H, W)")
    return tracks


def _depth_map(depth, k, B, H, W, device=None):
    """A depth tensor as cgd_frame_warp3d takes it: (1 or B, 1, H, W) fp32, on `device` if given; ValueError naming frame k otherwise."""
    import torch as th
    if not isinstance(depth, th.Tensor):
        raise ValueError(f"frame {k}: the depth must be a tensor, got {type(depth).__name__}")
    if depth.dim() == 2:
        depth = depth[None, None]
    if depth.dim() != 4 or tuple(depth.shape[1:]) != (1, H, W) or depth.shape[0] not in (1, B):
        raise ValueError(f"frame {k}: the depth must have shape (1 or {B}, 1, {H}, {W}) or ({H}, {W}), got {tuple(depth.shape)}")
    depth = depth.detach().to(device=depth.device if device is None else device, dtype=th.float32).contiguous()
    if not bool((th.isfinite(depth) & (depth > 0)).all()):
        raise ValueError(f"frame {k}: the depth must be finite and positive everywhere")
    return depth


def animate(frames, zoom=1.0, angle=0.0, translation_x=0.0, translation_y=0.0, border="wrap", interp="bicubic", frames_skip=0.6,
            frames_scale=1500, color_match=0.0, fixed_seed=False, prompts_at=None, mode="2d", translation_z=0.0, rotation_3d_x=0.0,
            rotation_3d_y=0.0, rotation_3d_z=0.0, fov=40.0, depth=None, depth_iters=1, near=0.05, depth_model=None, video_frames=None, flow_blend=0.999,
            check_consistency=False, flow_levels=4, flow_iters=4, flow_radius=4, **cgd_kwargs):
    """Generator of `(frame_idx, batch_idx, png_path)`: `frames` frames, each the last image of one sampling run, written to
    prefix_path/<prompts>/<batch_idx:02>/<frame_idx:04>.png.

    Frame 0 is an ordinary run of `cgd_kwargs` (cgd.cgd.clip_guided_diffusion's keywords; its own init_image / skip_timesteps / init_scale
    apply).  Frame k > 0 starts from the final `sample` of frame k - 1 of each of the batch's samples (B independent chains, one motion):
    warped by frame k's motion (`zoom`, `angle` in degrees, `translation_x`, `translation_y`: numbers or keyframe strings, see keyframes and
    motion_matrix; `border` wrap / reflect / replicate, `interp` bilinear / bicubic) and clamped to [-1, 1], moved toward frame 0's channel
    statistics by `color_match` in [0, 1], then used as the init image with skip_timesteps = round(frames_skip * num_timesteps) and the LPIPS
    weight `frames_scale` (0: no LPIPS term, and the LPIPS network is not loaded).  th.manual_seed(seed + k) precedes frame k (`fixed_seed`:
    seed itself).  `prompts_at` = {frame: [prompt strings]} replaces the text prompts from that frame on (image prompts stay; the weights are
    normalised together as at the start); a text is encoded when first needed and kept.

    `mode="3d"` replaces the affine warp by the camera's (module docstring; ops.frame_warp3d): `translation_x`, `translation_y`,
    `translation_z`, `rotation_3d_x`, `rotation_3d_y`, `rotation_3d_z` and `fov` are numbers or keyframe strings, `near` the near plane;
    everything else of the frame step is the same.  `depth`: None (flat, depth 1.0 everywhere: no parallax), a tensor (1 or B, 1, H, W) or
    (H, W) used for every frame, or a callable that is called once per frame k > 0 with the previous frame's pred_xstart as (B, 3, H, W) in
    [0, 1] on the GPU and returns such a tensor; the units are those in which the flat depth is 1.0.  `depth_iters` in 1..4: fixed-point steps
    that look the depth up at the source pixel (1: the destination pixel's own depth).  A depth of the wrong shape, or one that is not finite
    and positive everywhere, raises ValueError naming the frame.  A nets.DepthNet is such a callable; `depth_model` =
    'FILE[:size=N][:offset=A][:scale=B]' (parse_depth_model) builds one from a DPT-Large checkpoint, once, on the run's context, and excludes
    `depth`.

    `mode="video"` stylises a clip (module docstring): `video_frames` is a directory or a glob of image files (taken in name order), a list of
    paths, or a tensor (N, 3, H, W) in [-1, 1]; files are opened with PIL and resized to the run's frame as an init image is.  Frame 0 starts
    from the clip's frame 0 (skip_timesteps = round(frames_skip * num_timesteps), LPIPS weight `frames_scale`); frame k > 0 from
    ops.frame_warp_flow(previous, ops.flow_estimate(clip_k, clip_{k-1}, flow_levels, flow_iters, flow_radius), flow_back, fallback=clip_k,
    blend=flow_blend, interp, border, clamp=True), with flow_back = ops.flow_estimate(clip_{k-1}, clip_k, ...) under `check_consistency` and
    None otherwise; colour matching, seeds, `prompts_at` and the PNG paths are those of the other modes.  Video mode takes no `zoom`, `angle`,
    `translation_*`, `rotation_3d_*`, `fov`, depth argument or `init_image`, the other modes take no video argument, and `frames` may not
    exceed the clip's length.

    Refused before anything is loaded (ValueError): an unknown `mode`, `zoom` / `angle` in 3D mode, a 3D-only argument in 2D mode,
    `depth_iters` outside 1..4, a `fov` that leaves (0, 180), an init_image with '::MASK', 'invert=', 'upsample=' or 'ilvrN=', 'SOURCE=>TARGET'
    prompts, use_augs, a world size above 1, frames < 1, frames_skip outside [0, 1) or so high that no step is left, and prompts_at together
    with region prompts.  Everything else in `cgd_kwargs` passes through: samplers, '+thr=', '+windows=', '+model=', 'cuts=', regions, style,
    secondary, classifier."""
    import torch as th

    from cgd import cgd as entry
    from cgd import clip_util, script_util
    from cgd_amd import ops
    frames, plan = _check(frames, border, interp, frames_skip, frames_scale, color_match, prompts_at, cgd_kwargs)
    tracks = [keyframes(spec, frames) for spec in (zoom, angle, translation_x, translation_y)]
    if any(not z > 0 for z in tracks[0]):
        raise ValueError("zoom must stay positive on every frame")
    depth_model = parse_depth_model(depth_model)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    motion3d = (translation_z, rotation_3d_x, rotation_3d_y, rotation_3d_z)
    clip = _check_video(mode, frames, dict(video_frames=video_frames, flow_blend=flow_blend, check_consistency=check_consistency,
                                           flow_levels=flow_levels, flow_iters=flow_iters, flow_radius=flow_radius),
                        (zoom, angle, translation_x, translation_y), motion3d, fov, depth, depth_iters, near, depth_model, cgd_kwargs)
    tracks3d = _check_mode("2d" if mode == "video" else mode, frames, zoom, angle, motion3d, fov, depth, depth_iters, near, depth_model)
    seed = cgd_kwargs.get("seed", 0)
    run = entry.prepare_run(**cgd_kwargs, lpips_for_later=(frames > 1 or mode == "video") and frames_scale != 0)
    if run is None:
        return
    cond_fn, ctx = run.cond_fn, run.model.ctx
    _, _, H, W = run.shape
    skip = int(round(frames_skip * run.diffusion.num_timesteps))
    if (frames > 1 or mode == "video") and skip >= run.diffusion.num_timesteps:
        raise ValueError(f"frames_skip {frames_skip} leaves no step of the {run.diffusion.num_timesteps} for the frames after the first")

    def retarget(texts):
        embeds, weights = [[] for _ in run.clip_names], []
        for prompt in texts:
            text, weight = script_util.parse_prompt(prompt)
            for k, name in enumerate(run.clip_names):
                if (text, name) not in run.text_cache:
                    run.text_cache[(text, name)] = clip_util.encode_text_prompt(text, weight, name, run.device)[0]
                embeds[k].append(run.text_cache[(text, name)])
            weights.append(float(weight))
        weights += [float(w) for w in run.image_weights]
        w = th.tensor(weights)
        if w.sum().abs() < 1e-3:
            raise RuntimeError("The weights must not sum to 0.")
        cond_fn.set_targets([th.cat(e + list(img)) for e, img in zip(embeds, run.image_embeds)], w / w.sum().abs())

    B = run.shape[0]
    if depth_model is not None and frames > 1:
        depth = load_depth_model(ctx, depth_model)
    if mode == "3d" and depth is not None and not callable(depth):
        depth = _depth_map(depth, 0, B, H, W)  # judged now that the frame size is known; it joins the state's device at its first use
    previous = previous_x0 = stats0 = video_now = video_before = None
    flow_kw = dict(levels=flow_levels, iters=flow_iters, radius=flow_radius)
    for k in range(frames):
        if k in plan:
            retarget(plan[k])
        init = None
        if mode == "video":  # only the clip's frames k - 1 and k are on the GPU
            video_before, video_now = video_now, _video_frame(clip, k, B, H, W, run.device)
            if k == 0:
                init = video_now
                cond_fn.set_init(init if frames_scale != 0 else None, frames_scale)
        if k > 0:
            th.manual_seed(seed if fixed_seed else seed + k)
            if mode == "video":
                flow = ops.flow_estimate(ctx, video_now[:1], video_before[:1], **flow_kw)
                back = ops.flow_estimate(ctx, video_before[:1], video_now[:1], **flow_kw) if check_consistency else None
                init = ops.frame_warp_flow(ctx, previous, flow, flow_back=back, fallback=video_now, blend=flow_blend, interp=interp,
                                           border=border, clamp=True)
            elif mode == "3d":
                cam = camera(tracks[2][k], tracks[3][k], *(t[k] for t in tracks3d), H, W, near=near)
                if callable(depth):
                    dmap = _depth_map(depth((previous_x0.clamp(-1, 1) + 1) / 2), k, B, H, W, previous.device)
                else:
                    dmap = depth = None if depth is None else depth.to(previous.device)
                init = ops.frame_warp3d(ctx, previous, cam, depth=dmap, interp=interp, border=border, clamp=True, iters=depth_iters)
            else:
                matrix = motion_matrix(tracks[0][k], tracks[1][k], tracks[2][k], tracks[3][k], H, W)
                init = ops.frame_warp(ctx, previous, matrix, interp=interp, border=border, clamp=True)
            if color_match > 0:
                ops.color_match(ctx, init, stats0, amount=color_match, clamp=True)
            cond_fn.set_init(init if frames_scale != 0 else None, frames_scale)
        last = None
        for last in (run.samples() if init is None else run.samples(init_image=init, skip_timesteps=skip)):
            cond_fn.current_timestep -= 1
        if last is None:
            raise RuntimeError(f"frame {k}: the sampler loop made no step")
        staged = script_util.stage_images(last["pred_xstart"])
        previous = last["sample"].detach().clone()  # the loop's buffers are reused by the next frame
        if callable(depth) and k + 1 < frames:
            previous_x0 = last["pred_xstart"].detach().clone()
        if k == 0 and color_match > 0 and frames > 1:
            stats0 = ops.channel_stats(ctx, previous)
        for batch_idx, path in run.write(staged.get().numpy(), k):
            yield k, batch_idx, path


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--frames", type=int, required=True, help="number of frames")
    for name, default, what in (("zoom", "1.0", "magnification per frame (above 1 zooms in)"),
                                ("angle", "0", "degrees per frame, positive turns the picture counter-clockwise"),
                                ("translation_x", "0", "pixels per frame, positive moves the content right"),
                                ("translation_y", "0", "pixels per frame, positive moves the content down")):
        p.add_argument(f"--{name}", default=default, help=f"{what}: a number or keyframes 'FRAME:(VALUE), ...'")
    p.add_argument("--mode", default="2d", choices=MODES, help="2d: affine warp (zoom, angle, translation_x / y); 3d: a moving pinhole camera; "
                                                               "video: the motion of a clip (--video_frames), estimated as optical flow")
    p.add_argument("--video_frames", default=None, help="video: a directory or a glob of image files, taken in name order")
    p.add_argument("--flow_blend", type=float, default=0.999, help="video: share of the warped previous frame where the flow is trusted, in [0, 1]; "
                                                                   "the rest is the clip's own frame")
    p.add_argument("--check_consistency", action="store_true", help="video: also estimate the opposite flow and fall back to the clip's frame "
                                                                    "where the two disagree (occlusions)")
    p.add_argument("--flow_levels", type=int, default=4, help="video: pyramid levels of the flow, 1..8")
    p.add_argument("--flow_iters", type=int, default=4, help="video: iterations per level, 1..16")
    p.add_argument("--flow_radius", type=int, default=4, help="video: window radius in pixels, 1..7")
    for name, default, what in (("translation_z", "0", "3d: 1 / 200 depth units per frame, positive flies forward"),
                                ("rotation_3d_x", "0", "3d: degrees per frame, positive tilts the camera up (the content moves down)"),
                                ("rotation_3d_y", "0", "3d: degrees per frame, positive turns the camera right (the content moves left)"),
                                ("rotation_3d_z", "0", "3d: degrees per frame, positive turns the picture counter-clockwise"),
                                ("fov", "40", "3d: vertical field of view in degrees, inside (0, 180)")):
        p.add_argument(f"--{name}", default=default, help=f"{what}: a number or keyframes 'FRAME:(VALUE), ...'")
    p.add_argument("--depth_fn", default=None, help="3d: MODULE:FUNCTION, called with the previous frame (B,3,H,W) in [0,1], returns its depth "
                                                    "(1 or B,1,H,W), 1.0 = the flat default; without it the depth is flat")
    p.add_argument("--depth_model", default=None, help="3d: FILE[:size=N][:offset=A][:scale=B], a DPT-Large (MiDaS v3) checkpoint such as "
                                                       "dpt_large-midas-2f21e586.pt: the depth of the previous frame from the native depth network "
                                                       "(net size N, depth = (A - inverse depth) / B); not together with --depth_fn")
    p.add_argument("--depth_iters", type=int, default=1, help="3d: fixed-point steps of the depth lookup, 1..4")
    p.add_argument("--near", type=float, default=0.05, help="3d: the near plane, in depth units")
    p.add_argument("--border", default="wrap", choices=BORDERS, help="what the warp reads outside the frame (video: prefer replicate; wrap reads the opposite edge)")
    p.add_argument("--interp", default="bicubic", choices=INTERPS, help="interpolation of the warp")
    p.add_argument("--frames_skip", type=float, default=0.6, help="fraction of the schedule the frames after the first skip")
    p.add_argument("--frames_scale", type=float, default=1500, help="LPIPS weight toward the warped previous frame (0: no LPIPS)")
    p.add_argument("--color_match", type=float, default=0.0, help="how far every frame's channel mean / std are moved to frame 0's, in [0, 1]")
    p.add_argument("--fixed_seed", action="store_true", help="the same seed for every frame instead of seed + frame")
    p.add_argument("--prompts_at", action="append", default=[], help="'FRAME=prompt|prompt...': the text prompts from FRAME on (repeatable)")
    return p


def load_depth_fn(spec):
    """'MODULE:FUNCTION' -> the callable (importlib); ValueError when the text has another form or the attribute is not callable."""
    if spec is None:
        return None
    module, sep, name = str(spec).partition(":")
    if not sep or not module.strip() or not name.strip():
        raise ValueError(f"depth_fn {spec!r}: expected 'MODULE:FUNCTION'")
    fn = getattr(importlib.import_module(module.strip()), name.strip(), None)
    if not callable(fn):
        raise ValueError(f"depth_fn {spec!r}: {name.strip()!r} of {module.strip()!r} is not callable")
    return fn


def main(argv=None):
    from cgd import cgd as entry
    argv = list(sys.argv[1:] if argv is None else argv)
    own, rest = (argv[:argv.index("--")], argv[argv.index("--") + 1:]) if "--" in argv else (argv, [])
    a = build_parser().parse_args(own)
    kwargs = entry.kwargs_from_args(entry.build_parser().parse_args(rest))
    kwargs.pop("save_frequency", None)  # one PNG per frame
    for item in animate(a.frames, zoom=a.zoom, angle=a.angle, translation_x=a.translation_x, translation_y=a.translation_y, border=a.border,
                        interp=a.interp, frames_skip=a.frames_skip, frames_scale=a.frames_scale, color_match=a.color_match,
                        fixed_seed=a.fixed_seed, prompts_at=parse_prompts_at(a.prompts_at), mode=a.mode, translation_z=a.translation_z,
                        rotation_3d_x=a.rotation_3d_x, rotation_3d_y=a.rotation_3d_y, rotation_3d_z=a.rotation_3d_z, fov=a.fov,
                        depth=load_depth_fn(a.depth_fn), depth_iters=a.depth_iters, near=a.near, depth_model=a.depth_model,
                        video_frames=a.video_frames, flow_blend=a.flow_blend, check_consistency=a.check_consistency, flow_levels=a.flow_levels,
                        flow_iters=a.flow_iters, flow_radius=a.flow_radius, **kwargs):
        print("\t".join(str(v) for v in item))


if __name__ == "__main__":
    main()
