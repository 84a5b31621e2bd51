"""Plugin surface `cgd.script_util` (reference: /root/reference/cgd/script_util.py).

The hot-path boundary here is `load_guided_diffusion` (reference :281-324): it returns the MI355X UNet handle and
the guided sampler instead of guided_diffusion's (UNetModel, SpacedDiffusion).  The I/O helpers the generator needs
(prompt parsing, image logging, cached download) keep the reference's behaviour; ffmpeg post-processing and the
network retry machinery are outside the hot-path scope (control plane) and kept minimal.
"""
import io
import math
import os
import time
import re
from functools import lru_cache
from pathlib import Path

import torch as th

from cgd_amd import diffusion as _diffusion
from cgd_amd import lib as _lib
from cgd_amd import nets as _nets
from cgd_amd import shard as _shard
from cgd_amd import sampler as _sampler
from cgd_amd import synthetic as _synthetic

from .model_flags import DIFFUSION_LOOKUP, MODEL_AND_DIFFUSION_DEFAULTS, UPSAMPLER_LOOKUP

CACHE_PATH = os.path.expanduser("~/.cache/clip-guided-diffusion")
TIMESTEP_RESPACINGS = tuple(p + n for p in ("", "ddim") for n in ("25", "50", "100", "250", "500", "1000"))
DIFFUSION_SCHEDULES = (25, 50, 100, 250, 500, 1000)
IMAGE_SIZES = (64, 128, 256, 512)


def synthetic_weights_enabled():
    """CGD_SYNTHETIC_WEIGHTS=1: seeded random weights instead of checkpoints (bench / CI boxes have no network)."""
    return os.environ.get("CGD_SYNTHETIC_WEIGHTS", "0") not in ("", "0")


def parse_prompt(prompt):
    """'<text or url>[:<weight>]' -> (text, weight); URLs keep their scheme colon."""
    is_url = prompt.startswith(("http://", "https://"))
    parts = prompt.rsplit(":", 2 if is_url else 1)
    if is_url:
        parts = [parts[0] + ":" + parts[1]] + parts[2:]
    text = parts[0]
    weight = float(parts[1]) if len(parts) > 1 else 1.0
    return text, weight


def split_init_mask(value):
    """'IMAGE::MASK' -> (IMAGE, MASK), split at the last '::'; a value without '::' -> (value, None).  The mask of masked sampling rides
    on --init_image / init_image= (white regenerates, black keeps).  The '://' of a URL is no separator."""
    value = str(value)
    image, sep, mask = value.rpartition("::")
    if not sep:
        return value, None
    if not image or not mask:
        raise ValueError(f"init image {value!r}: 'IMAGE::MASK' needs both an image and a mask")
    return image, mask


THRESHOLD_SEP = "+thr="


def split_threshold(respacing):
    """'dpmN+thr=P' or 'dpmsdeN+thr=P:CAP' -> (the spacing without the suffix, (P, CAP)); CAP is None when not given; a value without
    '+thr=' -> (value, None).  Dynamic thresholding of the guided pred_xstart (GuidedSampler.dpmpp_sample_loop_progressive, threshold=)
    rides on --timestep_respacing / timestep_respacing=, and only the DPM-Solver++ spacings 'dpmN' / 'dpmsdeN' take it."""
    respacing = str(respacing)
    spec, sep, value = respacing.partition(THRESHOLD_SEP)
    if not sep:
        return respacing, None
    if not spec.startswith("dpm"):
        raise ValueError(f"timestep_respacing {respacing!r}: '+thr=' needs a DPM-Solver++ spacing, 'dpmN' or 'dpmsdeN'")
    parts = value.split(":")
    try:
        if len(parts) not in (1, 2):
            raise ValueError(value)
        p, cap = float(parts[0]), (float(parts[1]) if len(parts) == 2 else None)
    except ValueError:
        raise ValueError(f"timestep_respacing {respacing!r}: '+thr=' takes P or P:CAP (e.g. dpmN+thr=0.995 or dpmN+thr=0.995:1.5)") from None
    if not 0.0 < p <= 1.0:
        raise ValueError(f"timestep_respacing {respacing!r}: the quantile P of '+thr=' must lie in (0, 1]")
    if cap is not None and not cap >= 1.0:
        raise ValueError(f"timestep_respacing {respacing!r}: the CAP of '+thr=' must be >= 1")
    return spec, (p, cap)


WINDOWS_SEP = "+windows="


def split_windows(respacing, image_size=None, height_offset=0, width_offset=0, init_image=None, clip_model_name=""):
    """'250+windows=STRIDE[:wrapx|:wrapy|:wrap][:feather]' -> (the spacing without the suffix, (STRIDE, wrap, feather)) with wrap in '', 'x',
    'y', 'xy'; a value without '+windows=' -> (value, None).  Windowed sampling (nets.WindowedUNet: the model runs on overlapping windows of
    image_size, STRIDE apart, whose predictions are averaged over the image_size + offsets frame; a wrapping axis tiles seamlessly) rides on
    --timestep_respacing / timestep_respacing= as its last suffix: what is returned still carries a '+thr=' for split_threshold.  Refuses a
    malformed suffix and, when `image_size` is given, before anything is loaded: a STRIDE that is no positive multiple of 8 or exceeds
    image_size, frame sides that are no multiples of 8, wrap on an axis whose length STRIDE does not divide, and any combination with
    'upsample=', 'invert=' (`init_image`) or '+classifier=' (`clip_model_name`)."""
    respacing = str(respacing)
    spec, sep, value = respacing.partition(WINDOWS_SEP)
    if not sep:
        return respacing, None
    usage = f"timestep_respacing {respacing!r}: '+windows=' takes STRIDE[:wrapx|:wrapy|:wrap][:feather] (e.g. 250+windows=128:wrapx)"
    parts = value.split(":")
    if not spec or not parts[0].isdigit():
        raise ValueError(usage)
    stride, rest = int(parts[0]), parts[1:]
    feather = bool(rest) and rest[-1] == "feather"
    if feather:
        rest = rest[:-1]
    if len(rest) > 1 or (rest and rest[0] not in ("wrapx", "wrapy", "wrap")):
        raise ValueError(usage)
    wrap = {"wrapx": "x", "wrapy": "y", "wrap": "xy"}[rest[0]] if rest else ""
    if stride <= 0 or stride % 8:
        raise ValueError(f"timestep_respacing {respacing!r}: the STRIDE of '+windows=' must be a positive multiple of 8")
    if image_size is not None:
        if stride > image_size:
            raise ValueError(f"timestep_respacing {respacing!r}: the STRIDE of '+windows=' exceeds the window, image_size {image_size}")
        height, width = image_size + height_offset, image_size + width_offset
        if height % 8 or width % 8 or height < image_size or width < image_size:
            raise ValueError(f"timestep_respacing {respacing!r}: '+windows=' needs frame sides that are multiples of 8 and at least image_size "
                             f"{image_size}, got {height} x {width}")
        for axis, length in (("x", width), ("y", height)):
            if axis in wrap and length % stride:
                raise ValueError(f"timestep_respacing {respacing!r}: STRIDE {stride} does not divide the wrapping {axis} axis of length {length}")
        part = split_init_mask(init_image)[0] if init_image else ""
        for prefix in (UPSAMPLE_PREFIX, INVERT_PREFIX):
            if part.startswith(prefix):
                raise ValueError(f"timestep_respacing {respacing!r}: '+windows=' cannot be combined with init image '{prefix}...'")
        if "+classifier=" in str(clip_model_name):
            raise ValueError(f"timestep_respacing {respacing!r}: '+windows=' cannot be combined with '+classifier=' (the classifier is not windowed)")
    return spec, (stride, wrap, feather)


INVERT_PREFIX = "invert="


def split_init_invert(image_part):
    """'invert=IMAGE' -> (IMAGE, True); anything else -> (value, False).  Takes the image part split_init_mask returns: the request to
    start from the image's own DDIM-inverted latent rides on --init_image / init_image=, like the mask ('invert=IMAGE::MASK')."""
    image_part = str(image_part)
    if not image_part.startswith(INVERT_PREFIX):
        return image_part, False
    image = image_part[len(INVERT_PREFIX):]
    if not image:
        raise ValueError(f"init image {image_part!r}: 'invert=IMAGE' needs an image")
    return image, True


UPSAMPLE_PREFIX = "upsample="


def split_init_upsample(image_part):
    """'upsample=IMAGE' -> (IMAGE, True); anything else -> (value, False).  Takes the image part split_init_mask returns, next to
    split_init_invert: the request to run a super-resolution checkpoint on IMAGE rides on --init_image / init_image=, like the mask
    ('upsample=IMAGE::MASK').  IMAGE at a quarter of the frame conditions the model; at the full frame it stays the ordinary init image."""
    image_part = str(image_part)
    if not image_part.startswith(UPSAMPLE_PREFIX):
        return image_part, False
    image = image_part[len(UPSAMPLE_PREFIX):]
    if not image:
        raise ValueError(f"init image {image_part!r}: 'upsample=IMAGE' needs an image")
    return image, True


def check_init_upsample(init_image, image_size, class_cond):
    """Whether `init_image` asks for super-resolution ('upsample=IMAGE[::MASK]'), after refusing, before anything is loaded, what is not
    built: other sizes than the two published upsamplers', the unconditional flag (both upsamplers are class-conditional), and
    'invert=' together with 'upsample=' in either order (the inversion loop of the drop-in generator runs unconditioned)."""
    if not init_image:
        return False
    part = split_init_mask(init_image)[0]
    image, upsample = split_init_upsample(part)
    inverted, invert = split_init_invert(part)
    if (upsample and image.startswith(INVERT_PREFIX)) or (invert and inverted.startswith(UPSAMPLE_PREFIX)):
        raise ValueError(f"init image {init_image!r}: 'invert=' and 'upsample=' cannot be combined (inversion under a low-resolution "
                         "condition is not built)")
    if not upsample:
        return False
    if image_size not in UPSAMPLER_LOOKUP:
        raise ValueError(f"init image 'upsample=...' needs image_size {' or '.join(str(s) for s in sorted(UPSAMPLER_LOOKUP))} (the published "
                         f"64->256 and 128->512 upsamplers), got {image_size}")
    if not class_cond:
        raise ValueError("init image 'upsample=...' does not work with --uncond: both upsamplers are class-conditional")
    return True


ILVR_PREFIX = "ilvr"


def split_init_ilvr(image_part):
    """'ilvrN=IMAGE' -> (IMAGE, (N, 1.0)); 'ilvrN@U=IMAGE' -> (IMAGE, (N, U)); anything else -> (value, None).  Takes the image part
    split_init_mask returns, next to split_init_invert: the request to condition sampling on IMAGE's low frequencies (ILVR,
    GuidedSampler's ilvr=) rides on --init_image / init_image=.  N, the down-sampling factor, is a power of two in [2, 64]; U in (0, 1] is
    the fraction of the run after which the refinement ends (ilvr_stop)."""
    image_part = str(image_part)
    m = re.match(r"ilvr([^=/]*)=(.*)$", image_part, flags=re.S)
    if not m:
        return image_part, None
    spec, image = m.groups()
    factor, sep, until = spec.partition("@")
    try:
        if not factor.isdigit() or (sep and not until):
            raise ValueError(spec)
        factor, until = int(factor), (float(until) if sep else 1.0)
    except ValueError:
        raise ValueError(f"init image {image_part!r}: 'ilvrN=IMAGE' or 'ilvrN@U=IMAGE' takes an integer N and a number U "
                         "(e.g. ilvr8=a.png or ilvr8@0.8=a.png)") from None
    if not 2 <= factor <= 64 or factor & (factor - 1):
        raise ValueError(f"init image {image_part!r}: the factor N of 'ilvrN=IMAGE' must be a power of two in [2, 64]")
    if not 0.0 < until <= 1.0:
        raise ValueError(f"init image {image_part!r}: the U of 'ilvrN@U=IMAGE' must lie in (0, 1]")
    if not image:
        raise ValueError(f"init image {image_part!r}: 'ilvrN=IMAGE' needs an image")
    return image, (factor, until)


def ilvr_stop(until, num_timesteps):
    """The step index below which ILVR no longer refines: ceil((1 - U) num_timesteps), the product rounded to nine places first so that
    a U such as 0.7 does not land one index high"""
    return int(math.ceil(round((1.0 - until) * num_timesteps, 9)))


def check_init_ilvr(init_image, image_size, height_offset=0, width_offset=0):
    """(N, U) when `init_image` asks for ILVR ('ilvrN[@U]=IMAGE'), else None, after refusing, before anything is loaded, what is not
    built: a mask ('::MASK'), 'invert=' or 'upsample=' next to it in either order, and a factor that does not divide both frame sides."""
    if not init_image:
        return None
    part, mask = split_init_mask(init_image)
    image, spec = split_init_ilvr(part)
    if spec is None:
        for prefix in (INVERT_PREFIX, UPSAMPLE_PREFIX):
            if part.startswith(prefix) and split_init_ilvr(part[len(prefix):])[1] is not None:
                raise ValueError(f"init image {init_image!r}: 'ilvrN=' cannot be combined with '{prefix}'")
        return None
    if mask is not None:
        raise ValueError(f"init image {init_image!r}: 'ilvrN=' cannot be combined with a mask ('::MASK'): both rewrite the state after every step")
    for prefix in (INVERT_PREFIX, UPSAMPLE_PREFIX):
        if image.startswith(prefix):
            raise ValueError(f"init image {init_image!r}: 'ilvrN=' cannot be combined with '{prefix}'")
    height, width = image_size + height_offset, image_size + width_offset
    if height % spec[0] or width % spec[0]:
        raise ValueError(f"init image {init_image!r}: the factor {spec[0]} does not divide the {height} x {width} frame")
    return spec


DIRECTION_SEP = "=>"


def split_direction(text):
    """'SOURCE CAPTION=>TARGET CAPTION' -> (source, target), split at the first '=>' and stripped; a text without '=>' -> None.  Takes the
    text parse_prompt returns (the weight is already off).  A direction prompt rides on --prompts / prompts=: the change of the image
    embedding relative to the init image is steered along E(target) - E(source) instead of the image toward one caption."""
    source, sep, target = str(text).partition(DIRECTION_SEP)
    if not sep:
        return None
    source, target = source.strip(), target.strip()
    if not source or not target:
        raise ValueError(f"prompt {text!r}: 'SOURCE=>TARGET' needs a caption on both sides")
    return source, target


STYLE_PREFIX = "style="
REGION_SEP = "@@"


def split_region(prompt):
    """'TEXT@@REGION[^POWER][:weight]' -> ('TEXT[:weight]', REGION, POWER), split at the last '@@'; a prompt without '@@' -> (prompt, None, 1.0).
    A region rides on an entry of --prompts (direction prompts included: 'SRC=>TGT@@REGION:1.5') or of --image_prompts: the prompt then acts
    on a cutout in proportion to the share of REGION the cutout sees, raised to POWER (default 1).  REGION is a mask file (white inside) or
    a box 'x0,y0,x1,y1' in fractions of the frame (cgd_amd.regions.parse_region).  Refuses, before anything is loaded: a missing TEXT or
    REGION, a malformed box, a POWER or weight that is no number, a POWER that is not positive, and '@@' on a 'style=' entry."""
    from cgd_amd.regions import parse_box
    prompt = str(prompt)
    text, sep, tail = prompt.rpartition(REGION_SEP)
    if not sep:
        return prompt, None, 1.0
    if prompt.startswith(STYLE_PREFIX):
        raise ValueError(f"image prompt {prompt!r}: a 'style=' entry is no CLIP prompt and takes no '@@REGION'")
    is_url = tail.startswith(("http://", "https://"))
    head, colon, weight = tail.rpartition(":")
    if not colon or (is_url and head in ("http", "https")):
        head, weight = tail, None
    if weight is not None:
        try:
            float(weight)
        except ValueError:
            raise ValueError(f"prompt {prompt!r}: the weight behind 'TEXT@@REGION[^POWER]:' must be a number, got {weight!r}") from None
    region, hat, power = head.partition("^")
    if hat:
        try:
            power = float(power)
        except ValueError:
            raise ValueError(f"prompt {prompt!r}: the POWER of '@@REGION^POWER' must be a number, got {power!r}") from None
        if not power > 0 or power == float("inf"):
            raise ValueError(f"prompt {prompt!r}: the POWER of '@@REGION^POWER' must be positive and finite")
    else:
        power = 1.0
    if not text.strip() or not region.strip():
        raise ValueError(f"prompt {prompt!r}: 'TEXT@@REGION[^POWER][:weight]' needs a prompt and a region")
    parse_box(region.strip())  # a list of numbers that is no box is refused here; a file is opened once the frame is known
    return text + (":" + weight if weight is not None else ""), region.strip(), power


def split_region_prompts(prompts):
    """split_region over a list -> (the prompts without their '@@...' parts, [(REGION or None, POWER)] per prompt)."""
    parts = [split_region(p) for p in prompts]
    return [p[0] for p in parts], [(p[1], p[2]) for p in parts]


def split_style_prompts(image_prompts, height=None, width=None):
    """The entries of `image_prompts` without the 'style=FILE[:SCALE]' one, and (FILE, SCALE) of that one or None.  A style entry rides on
    --image_prompts / image_prompts= but is no CLIP image prompt: FILE is the style image of the VGG Gram-matrix style loss and SCALE the
    weight of that loss itself (default 1), so the entry stays out of the CLIP embeddings, the prompt weights, their normalisation and the
    zero-sum check.  Refuses, before anything is loaded: an entry without a file, a SCALE that is no positive number, a second style entry,
    and (when given) frame sides that are no multiples of 16 (the VGG trunk pools four times)."""
    rest, style = [], None
    for p in image_prompts:
        if not str(p).startswith(STYLE_PREFIX):
            rest.append(p)
            continue
        if style is not None:
            raise ValueError(f"image prompt {p!r}: at most one 'style=FILE[:SCALE]' entry (one style image)")
        try:
            file, scale = parse_prompt(str(p)[len(STYLE_PREFIX):])
        except ValueError:
            raise ValueError(f"image prompt {p!r}: 'style=FILE[:SCALE]' takes a number as SCALE") from None
        if not file:
            raise ValueError(f"image prompt {p!r}: 'style=FILE[:SCALE]' needs a file")
        if not scale > 0:
            raise ValueError(f"image prompt {p!r}: the SCALE of 'style=FILE:SCALE' is the weight of the style loss and must be positive")
        style = (file, scale)
    if style is not None and height is not None and (height % 16 or width % 16):
        raise ValueError(f"image prompt 'style=...' needs frame sides that are multiples of 16, got {height} x {width}")
    return rest, style


def direction_prompts(prompts, image_prompts=(), init_image=None, height_offset=0, width_offset=0):
    """Per entry of `prompts`: None, or the (source, target) captions of a direction prompt.  Refuses, before anything is loaded: a malformed
    entry, an image prompt with '=>', direction prompts without an init image (it is their source image) or with height / width offsets
    (the init image has the checkpoint's size), and weights that sum to zero over all prompts (the reference's rule, cgd.py:103-105)."""
    pairs = [split_direction(parse_prompt(p)[0]) for p in prompts]
    image_prompts = [p for p in image_prompts if not str(p).startswith(STYLE_PREFIX)]  # (split_style_prompts: no CLIP prompt, no prompt weight)
    for p in image_prompts:
        if DIRECTION_SEP in parse_prompt(p)[0]:
            raise ValueError(f"image prompt {p!r}: only text prompts can be 'SOURCE=>TARGET' directions")
    if any(pair is not None for pair in pairs):
        if not init_image:
            raise ValueError("a 'SOURCE=>TARGET' prompt needs an init image (--init_image IMAGE, IMAGE::MASK or invert=IMAGE): it is the source "
                             "image the edit is measured from")
        if height_offset or width_offset:
            raise ValueError(f"a 'SOURCE=>TARGET' prompt needs height_offset = width_offset = 0, got {height_offset} and {width_offset}: the "
                             "source image has the init image's size")
        if abs(sum(parse_prompt(p)[1] for p in list(prompts) + list(image_prompts))) < 1e-3:
            raise RuntimeError("The weights must not sum to 0.")
    return pairs


def fetch(url_or_path):
    if str(url_or_path).startswith(("http://", "https://")):
        import requests
        r = requests.get(url_or_path)
        r.raise_for_status()
        return io.BytesIO(r.content)
    return open(url_or_path, "rb")


def alphanumeric_filter(s: str) -> str:
    return re.sub(r"[^\w\s]", "", s).replace(" ", "_")


def clean_and_combine_prompts(base_path, txts, batch_idx, max_length=255) -> str:
    stem = "_".join(alphanumeric_filter(t) for t in txts)[:max_length]
    return os.path.join(base_path, stem, f"{batch_idx:02}")


def to_uint8_hwc(image: th.Tensor) -> th.Tensor:
    """(...,3,H,W) in [-1,1] -> (...,H,W,3) uint8, on the tensor's device (reference: TF.to_pil_image(image.add(1).div(2).clamp(0, 1)))."""
    return image.detach().float().add(1).div(2).clamp(0, 1).mul(255).byte().movedim(-3, -1).contiguous()


def stage_images(pred_xstart: th.Tensor):
    """Starts the uint8 conversion and an asynchronous device->host copy of a (B,3,H,W) batch; `.get()` of the returned
    handle yields the (B,H,W,3) uint8 host tensor without waiting for GPU work enqueued after this call."""
    from cgd_amd.hostcopy import HostCopy
    return HostCopy(to_uint8_hwc(pred_xstart))


def write_image(arr, base_path: str, txts: list, current_step: int, batch_idx: int) -> str:
    """(H,W,3) uint8 array -> '<base>/<prompts>/<batch:02>/<step:04>.png' (+ ./current.png), returns the path."""
    from PIL import Image
    dirname = clean_and_combine_prompts(base_path, txts, batch_idx)
    os.makedirs(dirname, exist_ok=True)
    filename = os.path.join(dirname, f"{current_step:04}.png")
    pil_image = Image.fromarray(arr)
    pil_image.save(os.path.join(os.getcwd(), "current.png"))
    pil_image.save(filename)
    return str(filename)


def log_image(image: th.Tensor, base_path: str, txts: list, current_step: int, batch_idx: int) -> str:
    """(3,H,W) in [-1,1] -> PNG as above (reference signature, /root/reference/cgd/script_util.py:93-101)."""
    return write_image(to_uint8_hwc(image).cpu().numpy(), base_path, txts, current_step, batch_idx)


def download(url: str, filename: str, root: str = CACHE_PATH, max_retries: int = 3) -> str:
    """Cached download: returns the target immediately when it exists; otherwise streams to a per-process temporary file and moves it
    into place atomically.  In a multi-GPU run (cgd_amd.launch: one process per GPU) only rank 0 downloads; the other ranks wait for it
    and then find the finished file in the cache."""
    return _shard.on_rank0(lambda: _download(url, filename, root, max_retries))


def _download(url: str, filename: str, root: str, max_retries: int) -> str:
    os.makedirs(root, exist_ok=True)
    target = Path(root) / filename
    if target.exists() and not target.is_file():
        raise RuntimeError(f"{target} exists and is not a regular file")
    if target.is_file():
        return str(target)
    import requests
    tmp = target.with_name(f"{target.name}.tmp.{os.getpid()}")  # never shared between processes (two launches on one cache directory)
    last = None
    for attempt in range(max_retries):
        try:
            with requests.get(url, stream=True, timeout=(30, 120)) as resp:
                resp.raise_for_status()
                expected = int(resp.headers.get("Content-Length", 0) or 0)
                with open(tmp, "wb") as out:
                    for chunk in resp.iter_content(chunk_size=1 << 16):
                        out.write(chunk)
                    out.flush()
                    os.fsync(out.fileno())
            got = tmp.stat().st_size
            if expected and got != expected:  # a connection that closed early without raising must not reach the cache
                raise OSError(f"download incomplete: expected {expected} bytes, got {got}")
            os.replace(tmp, target)  # atomic: a reader sees the old state or the complete file
            return str(target)
        except (requests.exceptions.RequestException, OSError) as e:
            last = e
            if tmp.exists():
                tmp.unlink()
            if attempt < max_retries - 1:
                time.sleep(float(os.environ.get("CGD_DOWNLOAD_BACKOFF", "1")) * 2 ** attempt)
    raise RuntimeError(f"Download failed after {max_retries} attempts: {last}") from last


def download_guided_diffusion(image_size: int, class_cond: bool, checkpoints_dir: str = CACHE_PATH, overwrite: bool = False) -> str:
    info = DIFFUSION_LOOKUP["cond" if class_cond else "uncond"][image_size]
    target = Path(checkpoints_dir) / info["filename"]
    if synthetic_weights_enabled():
        return str(target)
    # the cache check is part of what rank 0 decides for everybody: a rank that arrived late and found the freshly downloaded file must
    # not skip the collective the others are waiting in
    return _shard.on_rank0(lambda: str(target) if (not overwrite and target.exists()) else
                           _download(info["url"], info["filename"], checkpoints_dir, 3))


_CTX = {}


def get_context(device):
    """One library context per GPU ('cuda', 'cuda:N')."""
    dev = th.device(device)
    if dev.type != "cuda":
        raise ValueError(f"the MI355X path needs a GPU device string ('cuda[:N]'), got {device!r}; there is no CPU fallback")
    idx = dev.index if dev.index is not None else th.cuda.current_device()
    if idx not in _CTX:
        _CTX[idx] = _lib.Context(idx, os.environ.get("CGD_PRECISION", "bf16x3"))
    return _CTX[idx]


def model_config(image_size, class_cond, diffusion_steps=None, timestep_respacing=None, use_fp16=True, noise_schedule="linear",
                 dropout=0.0):
    """Per-checkpoint flags over upstream defaults, then the user-level overrides (reference :305-315)."""
    cfg = dict(MODEL_AND_DIFFUSION_DEFAULTS)
    cfg.update(DIFFUSION_LOOKUP["cond" if class_cond else "uncond"][image_size]["model_flags"])
    cfg.update(diffusion_steps=diffusion_steps, timestep_respacing=timestep_respacing, use_fp16=use_fp16, noise_schedule=noise_schedule,
               dropout=dropout)
    return cfg


def unet_kwargs(cfg):
    """guided_diffusion's create_model flags -> the device UNet's constructor arguments (NUM_CLASSES = 1000 upstream; the channel
    multipliers default per image size like upstream's create_model)."""
    return dict(image_size=cfg["image_size"], model_channels=cfg["num_channels"], num_res_blocks=cfg["num_res_blocks"],
                attention_resolutions=cfg["attention_resolutions"].replace(" ", ""), channel_mult=None,
                num_classes=1000 if cfg["class_cond"] else None, num_heads=cfg["num_heads"], num_head_channels=cfg["num_head_channels"],
                use_new_attention_order=cfg["use_new_attention_order"], out_channels=6 if cfg["learn_sigma"] else 3)


def upsampler_config(large_size, diffusion_steps=None, timestep_respacing=None, use_fp16=True, noise_schedule="linear", dropout=0.0):
    """model_config for the super-resolution checkpoint of `large_size` (UPSAMPLER_LOOKUP): upstream's defaults, the checkpoint's flags,
    then the user-level overrides."""
    cfg = dict(MODEL_AND_DIFFUSION_DEFAULTS)
    cfg.update(UPSAMPLER_LOOKUP[large_size]["model_flags"])
    cfg.update(diffusion_steps=diffusion_steps or cfg["diffusion_steps"], timestep_respacing=timestep_respacing, use_fp16=use_fp16,
               noise_schedule=noise_schedule, dropout=dropout)
    return cfg


def upsampler_unet_kwargs(cfg):
    """upstream's sr_create_model flags -> the device UNet's constructor arguments: the UNet of large_size with its own channel_mult and
    a 6-channel stem (x_t and the upsampled low-resolution image)."""
    return dict(image_size=cfg["large_size"], model_channels=cfg["num_channels"], num_res_blocks=cfg["num_res_blocks"],
                attention_resolutions=cfg["attention_resolutions"].replace(" ", ""), channel_mult=tuple(cfg["channel_mult"]),
                num_classes=1000 if cfg["class_cond"] else None, num_heads=cfg["num_heads"], num_head_channels=cfg["num_head_channels"],
                use_new_attention_order=cfg["use_new_attention_order"], in_channels=6, out_channels=6 if cfg["learn_sigma"] else 3)


def check_upsampler_state_dict(sd, specs, what="upsampler"):
    """Every tensor of a loaded state dict against the manifest `specs` ([(name, numel)]: nets.manifest / UNet.param_specs) of the flag
    table, which was written without a checkpoint at hand: a missing or unknown key, a wrong element count or a stem that is not
    [ch0, 6, 3, 3] is a ValueError that names the tensor, before anything is uploaded."""
    specs = dict(specs)
    missing = [k for k in specs if k not in sd]
    if missing:
        raise ValueError(f"{what}: the checkpoint lacks {len(missing)} tensors the flag table expects, first {missing[0]!r}")
    extra = [k for k in sd if k not in specs]
    if extra:
        raise ValueError(f"{what}: the checkpoint has {len(extra)} tensors the flag table does not expect, first {extra[0]!r}")
    for name, numel in specs.items():
        if sd[name].numel() != numel:
            raise ValueError(f"{what}: {name} has shape {tuple(sd[name].shape)} ({sd[name].numel()} elements), the flag table expects {numel}")
    stem = sd["input_blocks.0.0.weight"]
    if stem.dim() != 4 or tuple(stem.shape[1:]) != (6, 3, 3):
        raise ValueError(f"{what}: input_blocks.0.0.weight has shape {tuple(stem.shape)}, a super-resolution stem is [ch0, 6, 3, 3]")


def download_upsampler(large_size: int, checkpoints_dir: str = CACHE_PATH) -> str:
    """Path of the super-resolution checkpoint, found by name in `checkpoints_dir` (downloaded there when absent, as the base models are)."""
    info = UPSAMPLER_LOOKUP[large_size]
    target = Path(checkpoints_dir) / info["filename"]
    if synthetic_weights_enabled():
        return str(target)
    return _shard.on_rank0(lambda: str(target) if target.exists() else _download(info["url"], info["filename"], checkpoints_dir, 3))


@lru_cache(maxsize=1)
def load_upsampler(checkpoint_path: str, large_size: int, diffusion_steps: int = None, timestep_respacing: str = None, device: str = "",
                   noise_schedule: str = "linear", dropout: float = 0.0):
    """-> (model, diffusion) like load_guided_diffusion, for the super-resolution checkpoint of `large_size`: the model is a 6-channel
    nets.UNet, conditioned by model.set_low_res (the sampler does that from model_kwargs["low_res"])."""
    if not (len(device) > 0):
        raise ValueError("device must be set")
    cfg = upsampler_config(large_size, diffusion_steps, timestep_respacing, True, noise_schedule, dropout)
    ctx = get_context(device)
    model = _nets.UNet(ctx, **upsampler_unet_kwargs(cfg))
    dev = f"cuda:{ctx.device}"

    def read():
        sd = th.load(checkpoint_path, map_location="cpu")
        check_upsampler_state_dict(sd, model.param_specs(), os.path.basename(checkpoint_path))
        return sd

    if os.path.isfile(checkpoint_path):
        _shard.load_broadcast(model, read, dev)
    elif synthetic_weights_enabled():
        _shard.load_broadcast(model, lambda: _synthetic.synthetic_state_dict(model, seed=1234, device=dev), dev)
    else:
        raise FileNotFoundError(f"{checkpoint_path} not found (set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")
    tables = _diffusion.create_gaussian_diffusion(steps=cfg["diffusion_steps"], noise_schedule=cfg["noise_schedule"],
                                                  timestep_respacing=cfg["timestep_respacing"] or "",
                                                  rescale_timesteps=cfg["rescale_timesteps"])
    return model, _sampler.GuidedSampler(ctx, tables)


@lru_cache(maxsize=1)
def load_guided_diffusion(checkpoint_path: str, image_size: int, class_cond: bool, diffusion_steps: int = None,
                          timestep_respacing: str = None, use_fp16: bool = True, device: str = "", noise_schedule: str = "linear",
                          dropout: float = 0.0):
    """-> (model, diffusion): the device UNet handle (`model(x, ts, y)`, `.dgrad`, `.num_classes`) and the guided sampler
    (`.num_timesteps`, `.sqrt_one_minus_alphas_cumprod`, `.p_sample_loop_progressive`, `.ddim_sample_loop_progressive`)."""
    if not (len(device) > 0):
        raise ValueError("device must be set")
    if noise_schedule not in ("linear", "cosine"):
        raise ValueError("linear_or_cosine must be set")
    cfg = model_config(image_size, class_cond, diffusion_steps, timestep_respacing, use_fp16, noise_schedule, dropout)
    ctx = get_context(device)
    model = _nets.UNet(ctx, **unet_kwargs(cfg))
    # multi-GPU runs (cgd_amd.launch): rank 0 reads / draws the weights, one RCCL broadcast hands them to the other ranks
    dev = f"cuda:{ctx.device}"
    if os.path.isfile(checkpoint_path):
        _shard.load_broadcast(model, lambda: th.load(checkpoint_path, map_location="cpu"), dev)
    elif synthetic_weights_enabled():
        _shard.load_broadcast(model, lambda: _synthetic.synthetic_state_dict(model, seed=1234, device=dev), dev)
    else:
        raise FileNotFoundError(f"{checkpoint_path} not found (set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")
    steps = cfg["diffusion_steps"]
    tables = _diffusion.create_gaussian_diffusion(steps=steps, noise_schedule=cfg["noise_schedule"],
                                                  timestep_respacing=cfg["timestep_respacing"] or "",
                                                  rescale_timesteps=cfg["rescale_timesteps"])
    return model, _sampler.GuidedSampler(ctx, tables)


MODEL_SEP = "+model="


def split_model(respacing):
    """'ddim100+model=FILE[:heads=N | :head_channels=N][:new_order]' -> (the spacing without the suffix, (FILE, heads, head_channels,
    new_order)) with None for an option not given; a value without '+model=' -> (value, None).  A community checkpoint of the classic UNet
    architecture (COMMUNITY_LOOKUP, unet_flags_from_state_dict) rides on --timestep_respacing / timestep_respacing= as its LAST suffix, split
    off before split_windows; what is returned still carries '+windows=' / '+thr='.  The head count and the attention order change the output
    and show in no tensor shape: they come from the table (by FILE's basename) or from these options.  Malformed text is refused here, before
    anything is loaded."""
    respacing = str(respacing)
    spec, sep, value = respacing.partition(MODEL_SEP)
    if not sep:
        return respacing, None
    usage = (f"timestep_respacing {respacing!r}: '+model=' takes FILE[:heads=N | :head_channels=N][:new_order] "
             "(e.g. ddim100+model=pixel_art_diffusion_hard_256.pt or 250+model=mine.pt:heads=4)")
    if not spec:
        raise ValueError(usage)
    if "+" in value and any(s in value for s in (MODEL_SEP, WINDOWS_SEP, THRESHOLD_SEP)):
        raise ValueError(f"timestep_respacing {respacing!r}: '+model=' is the last suffix ('+thr=' and '+windows=' come before it)")
    parts = value.split(":")
    file, heads, head_channels, new_order = parts[0], None, None, False
    if not file:
        raise ValueError(usage)
    for opt in parts[1:]:
        key, eq, num = opt.partition("=")
        if opt == "new_order" and not new_order:
            new_order = True
        elif key in ("heads", "head_channels") and eq and num.isdigit() and int(num) > 0 and heads is None and head_channels is None:
            heads, head_channels = (int(num), None) if key == "heads" else (None, int(num))
        else:
            raise ValueError(usage)
    return spec, (file, heads, head_channels, new_order)


def unwrap_state_dict(sd, what="checkpoint"):
    """What th.load gave -> the flat {name: tensor} state dict: a {'state_dict': {...}} or {'model': {...}} wrapper (training scripts save
    those) is opened; anything that is then no mapping of names to tensors is refused by the name of the first offending entry."""
    for key in ("state_dict", "model"):
        if isinstance(sd, dict) and key in sd and isinstance(sd[key], dict) and not th.is_tensor(sd[key]):
            sd = sd[key]
    if not isinstance(sd, dict) or not sd:
        raise ValueError(f"{what}: th.load gave a {type(sd).__name__}, not a state dict")
    for name, v in sd.items():
        if not th.is_tensor(v):
            raise ValueError(f"{what}: entry {name!r} is a {type(v).__name__}, not a tensor: no plain state dict")
    return sd


def _shape(sd, name, dims=None):
    if name not in sd:
        raise ValueError(f"{name}: the checkpoint has no such tensor; it is no guided-diffusion / improved-diffusion UNet this build supports")
    shape = tuple(sd[name].shape)
    if dims is not None and len(shape) != dims:
        raise ValueError(f"{name}: expected {dims} dimensions, got shape {shape}")
    return shape


def unet_flags_from_state_dict(sd, image_size):
    """The create_model flags a UNet state dict reveals, from its tensor SHAPES alone: num_channels (from time_embed.0.weight: the 512 model's
    stem is half as wide), channel_mult and num_res_blocks (from the widths and the grouping of the output blocks), attention_resolutions
    (which input blocks hold a '.norm.weight'), resblock_updown (no '.op.weight'), use_scale_shift_norm (rows of emb_layers.1.weight against
    the block's width), class_cond (label_emb.weight), learn_sigma (rows of out.2.weight) and in_channels.  The head count, the attention
    order and the noise schedule show in no shape.  Raises ValueError naming the tensor for anything that fits no supported architecture:
    learn_sigma=False (a 3-row out.2) among them, which the sampler's variance blend does not cover."""
    ted, mc = _shape(sd, "time_embed.0.weight", 2)
    if mc <= 0 or ted != 4 * mc or mc % 32:
        raise ValueError(f"time_embed.0.weight: shape {(ted, mc)} is no [4 * num_channels, num_channels] with num_channels a multiple of 32")
    stem = _shape(sd, "input_blocks.0.0.weight", 4)
    if stem[1] not in (3, 6) or stem[2:] != (3, 3):
        raise ValueError(f"input_blocks.0.0.weight: shape {stem} is no 3x3 stem over 3 (or, super-resolution, 6) channels")
    head = _shape(sd, "out.2.weight", 4)
    if head[0] == 3:
        raise ValueError("out.2.weight: 3 output channels, a learn_sigma=False model; only learn_sigma=True checkpoints (6 channels) are supported")
    if head[0] != 6 or head[1] != stem[0]:
        raise ValueError(f"out.2.weight: shape {head} is no [6, {stem[0]}, 3, 3] head")
    # levels from the output blocks: the last block of every level but the final one ends in the upsampler, a second ResBlock
    # (resblock_updown) or a '.conv' (the classic Upsample)
    widths, per_level, count, k = [], [], 0, 0
    while f"output_blocks.{k}.0.in_layers.2.weight" in sd:
        pre = f"output_blocks.{k}"
        width = _shape(sd, f"{pre}.0.in_layers.2.weight", 4)[0]
        count += 1
        ends = any(f"{pre}.{j}.conv.weight" in sd or f"{pre}.{j}.in_layers.2.weight" in sd for j in (1, 2))
        if ends:
            widths.append(width)
            per_level.append(count)
            count = 0
        k += 1
    if k == 0:
        raise ValueError("output_blocks.0.0.in_layers.2.weight: the checkpoint has no such tensor; it is no UNet this build supports")
    widths.append(_shape(sd, f"output_blocks.{k - 1}.0.in_layers.2.weight", 4)[0])
    per_level.append(count)
    if len(set(per_level)) != 1 or per_level[0] < 2:
        raise ValueError(f"output_blocks.{k - 1}.0.in_layers.2.weight: the output blocks group into levels of {per_level} blocks, not into equal "
                         "levels of num_res_blocks + 1")
    num_res_blocks, widths = per_level[0] - 1, widths[::-1]
    mult = []
    for level, w in enumerate(widths):
        m = w / mc
        if w % 32 or m <= 0:
            raise ValueError(f"output_blocks: level {level} is {w} channels wide, no multiple of 32")
        mult.append(int(m) if m == int(m) else m)
    if widths[0] != stem[0]:
        raise ValueError(f"input_blocks.0.0.weight: the stem is {stem[0]} channels wide, the last output level {widths[0]}")
    # the input side must be the mirror of that plan
    classic = any(name.endswith(".0.op.weight") for name in sd)
    att_ds, idx = [], 1
    for level, w in enumerate(widths):
        flags_here = set()
        for _ in range(num_res_blocks):
            got = _shape(sd, f"input_blocks.{idx}.0.in_layers.2.weight", 4)[0]
            if got != w:
                raise ValueError(f"input_blocks.{idx}.0.in_layers.2.weight: {got} output channels, the mirrored output level has {w}")
            flags_here.add(f"input_blocks.{idx}.1.norm.weight" in sd)
            idx += 1
        if len(flags_here) != 1:
            raise ValueError(f"input_blocks.{idx - 1}.1.norm.weight: only some of the blocks of level {level} carry attention")
        if flags_here.pop():
            att_ds.append(1 << level)
        if level != len(widths) - 1:
            name = f"input_blocks.{idx}.0.op.weight" if classic else f"input_blocks.{idx}.0.in_layers.2.weight"
            if _shape(sd, name, 4) != (w, w, 3, 3):
                raise ValueError(f"{name}: shape {tuple(sd[name].shape)} is no [{w}, {w}, 3, 3] downsampler")
            idx += 1
    if f"input_blocks.{idx}.0.in_layers.2.weight" in sd or f"input_blocks.{idx}.0.op.weight" in sd:
        raise ValueError(f"input_blocks.{idx}: more input blocks than the output blocks mirror")
    if image_size % (1 << (len(widths) - 1)):
        raise ValueError(f"output_blocks: {len(widths)} levels do not divide image_size {image_size}")
    rows = _shape(sd, "input_blocks.1.0.emb_layers.1.weight", 2)[0]
    if rows not in (widths[0], 2 * widths[0]):
        raise ValueError(f"input_blocks.1.0.emb_layers.1.weight: {rows} rows for a block of {widths[0]} channels: neither an additive embedding "
                         "nor scale and shift")
    num_classes = 0
    if "label_emb.weight" in sd:
        num_classes, width = _shape(sd, "label_emb.weight", 2)
        if width != ted or num_classes < 1:
            raise ValueError(f"label_emb.weight: shape {(num_classes, width)} is no [num_classes, {ted}] class embedding")
    # attention_resolutions "" = no attention level on the way down (the middle block always attends): nets.UNet.make_config takes it
    return dict(image_size=image_size, num_channels=mc, num_res_blocks=num_res_blocks, channel_mult=tuple(mult),
                attention_resolutions=",".join(str(image_size // ds) for ds in att_ds), resblock_updown=not classic,
                use_scale_shift_norm=rows == 2 * widths[0], class_cond=num_classes > 0, num_classes=num_classes, learn_sigma=True,
                in_channels=stem[1])


SNIFFED_FLAGS = ("num_channels", "num_res_blocks", "attention_resolutions", "resblock_updown", "use_scale_shift_norm", "class_cond", "learn_sigma")


def community_flags(model_spec, image_size, class_cond, noise_schedule="linear", sd=None):
    """The flags of a '+model=' run: the table entry of FILE's basename (COMMUNITY_LOOKUP) or, with `sd`, what the state dict's shapes show,
    plus the head count and attention order of the options.  Refuses: neither a table hit nor 'heads=' / 'head_channels=' (the head count
    changes the output and no shape shows it); a table entry of another image_size; a class conditioning that disagrees with the checkpoint;
    a state dict that contradicts its table entry (by flag); a super-resolution checkpoint."""
    from .model_flags import COMMUNITY_LOOKUP
    file, heads, head_channels, new_order = model_spec
    hit = COMMUNITY_LOOKUP.get(os.path.basename(file))
    if hit is None and heads is None and head_channels is None:
        raise ValueError(f"'+model={file}': not among the known checkpoints ({', '.join(sorted(COMMUNITY_LOOKUP))}); give the head count with "
                         "':heads=N' or ':head_channels=N' (it changes the output and no tensor shape shows it)")
    if hit is None and sd is None:
        raise ValueError(f"'+model={file}': with CGD_SYNTHETIC_WEIGHTS=1 the file is not read, so only the known checkpoints work "
                         f"({', '.join(sorted(COMMUNITY_LOOKUP))})")
    flags = dict(MODEL_AND_DIFFUSION_DEFAULTS)
    if hit is not None:
        flags.update(hit["model_flags"])
        if flags["image_size"] != image_size:
            raise ValueError(f"'+model={file}' is a {flags['image_size']} x {flags['image_size']} checkpoint, image_size is {image_size}")
    if sd is not None:
        seen = unet_flags_from_state_dict(sd, image_size)
        if seen["in_channels"] != 3:
            raise ValueError(f"'+model={file}': input_blocks.0.0.weight takes 6 channels, a super-resolution checkpoint; use init image 'upsample=...'")
        if hit is not None:
            for key in SNIFFED_FLAGS:
                if str(flags[key]).replace(" ", "") != str(seen[key]):
                    raise ValueError(f"'+model={file}': the checkpoint's shapes give {key}={seen[key]!r}, the table says {flags[key]!r}")
            default = _nets.DEFAULT_CHANNEL_MULT.get(image_size)
            if tuple(flags.get("channel_mult") or default or ()) != tuple(seen["channel_mult"]):
                raise ValueError(f"'+model={file}': the checkpoint's shapes give channel_mult={seen['channel_mult']!r}, the table says "
                                 f"{tuple(flags.get('channel_mult') or default or ())!r}")
        flags.update(seen)
    elif not flags.get("channel_mult"):
        flags["channel_mult"] = _nets.DEFAULT_CHANNEL_MULT[image_size]
    if bool(flags["class_cond"]) != bool(class_cond):
        raise ValueError(f"'+model={file}' is {'class-conditional' if flags['class_cond'] else 'unconditional'}: run it "
                         f"{'without' if flags['class_cond'] else 'with'} --uncond")
    if heads is not None:
        flags.update(num_heads=heads, num_head_channels=-1)
    if head_channels is not None:
        flags.update(num_head_channels=head_channels)
    if new_order:
        flags["use_new_attention_order"] = True
    flags["noise_schedule"] = noise_schedule
    return flags


def community_unet_kwargs(flags):
    """community_flags -> the device UNet's constructor arguments"""
    return dict(image_size=flags["image_size"], model_channels=flags["num_channels"], num_res_blocks=flags["num_res_blocks"],
                attention_resolutions=str(flags["attention_resolutions"]).replace(" ", ""), channel_mult=tuple(flags["channel_mult"]),
                num_classes=(flags.get("num_classes") or 1000) if flags["class_cond"] else None, num_heads=flags["num_heads"],
                num_head_channels=flags["num_head_channels"],
                use_new_attention_order=flags["use_new_attention_order"], out_channels=6, resblock_updown=flags["resblock_updown"],
                use_scale_shift_norm=flags["use_scale_shift_norm"])


def check_model(model_spec, image_size, class_cond, init_image=None):
    """What a '+model=' run refuses before anything is loaded: a file that is neither known nor given a head count (community_flags, for a
    known file also its size and class conditioning), and init image 'upsample=' (that run loads the super-resolution checkpoint instead)."""
    from .model_flags import COMMUNITY_LOOKUP
    file = model_spec[0]
    if init_image and split_init_mask(init_image)[0].startswith(UPSAMPLE_PREFIX):
        raise ValueError(f"'+model={file}' cannot be combined with init image 'upsample=...': that run samples with the super-resolution checkpoint")
    if os.path.basename(file) in COMMUNITY_LOOKUP:
        community_flags(model_spec, image_size, class_cond)
    elif model_spec[1] is None and model_spec[2] is None or synthetic_weights_enabled():
        community_flags(model_spec, image_size, class_cond)  # raises


def check_state_dict(sd, specs, what):
    """Every tensor of a loaded state dict against the manifest `specs` ([(name, numel)]) of the flags it is loaded under: a missing or
    unknown key or a wrong element count is a ValueError that names the tensor, before anything is uploaded."""
    specs = dict(specs)
    missing = [k for k in specs if k not in sd]
    if missing:
        raise ValueError(f"{what}: the checkpoint lacks {len(missing)} tensors its flags expect, first {missing[0]!r}")
    extra = [k for k in sd if k not in specs]
    if extra:
        raise ValueError(f"{what}: the checkpoint has {len(extra)} tensors its flags do not expect, first {extra[0]!r}")
    for name, numel in specs.items():
        if sd[name].numel() != numel:
            raise ValueError(f"{what}: {name} has shape {tuple(sd[name].shape)} ({sd[name].numel()} elements), its flags expect {numel}")


@lru_cache(maxsize=1)
def load_community_model(model_spec, image_size: int, class_cond: bool, diffusion_steps: int = None, timestep_respacing: str = None,
                         device: str = "", noise_schedule: str = "linear", checkpoints_dir: str = CACHE_PATH):
    """-> (model, diffusion) like load_guided_diffusion, for the checkpoint a '+model=FILE...' suffix names (split_model's tuple): FILE as
    given or, when that is no file, under `checkpoints_dir`.  With CGD_SYNTHETIC_WEIGHTS=1 the file is not read: table names only, seeded
    weights drawn from param_specs."""
    if not (len(device) > 0):
        raise ValueError("device must be set")
    if noise_schedule not in ("linear", "cosine"):
        raise ValueError("linear_or_cosine must be set")
    file = model_spec[0]
    path = file if os.path.isfile(file) else os.path.join(checkpoints_dir, file)
    ctx = get_context(device)
    dev = f"cuda:{ctx.device}"
    if synthetic_weights_enabled():
        flags = community_flags(model_spec, image_size, class_cond, noise_schedule)
        model = _nets.UNet(ctx, **community_unet_kwargs(flags))
        _shard.load_broadcast(model, lambda: _synthetic.synthetic_state_dict(model, seed=1234, device=dev), dev)
    elif os.path.isfile(path):
        # every rank reads it: the flags come from its shapes.  (fp16 tensors are fine: the upload converts every tensor to fp32)
        sd = unwrap_state_dict(th.load(path, map_location="cpu"), os.path.basename(path))
        flags = community_flags(model_spec, image_size, class_cond, noise_schedule, sd=sd)
        model = _nets.UNet(ctx, **community_unet_kwargs(flags))
        check_state_dict(sd, model.param_specs(), os.path.basename(path))
        _shard.load_broadcast(model, lambda: sd, dev)
    else:
        raise FileNotFoundError(f"{path} not found (for a known checkpoint, CGD_SYNTHETIC_WEIGHTS=1 gives seeded random weights)")
    tables = _diffusion.create_gaussian_diffusion(steps=diffusion_steps or flags["diffusion_steps"], noise_schedule=flags["noise_schedule"],
                                                  timestep_respacing=timestep_respacing or "", rescale_timesteps=flags["rescale_timesteps"])
    return model, _sampler.GuidedSampler(ctx, tables)


def load_lpips(ctx, checkpoints_dir: str = CACHE_PATH, device="cuda"):
    """Device LPIPS-VGG16 (reference: `lpips.LPIPS(net='vgg')`, cgd.py:147-148).  Weights: `<checkpoints_dir>/lpips_vgg16.pt`, a
    state dict with the package's keys (torchvision VGG16 trunk as `net.slice{k}.{idx}.weight|bias`, heads `lin{k}.model.1.weight`);
    with CGD_SYNTHETIC_WEIGHTS=1 seeded synthetic weights are used (no network on the build / bench boxes)."""
    from cgd_amd import nets, synthetic
    net = nets.LpipsVGG(ctx)
    path = os.path.join(checkpoints_dir, "lpips_vgg16.pt")
    if os.path.isfile(path):
        sd = th.load(path, map_location="cpu")
        sd = {k: (v.reshape(-1) if k.startswith("lin") else v) for k, v in sd.items()}
        return net.load_state_dict({k: v.to(device) for k, v in sd.items() if k.startswith(("net.slice", "lin"))})
    if synthetic_weights_enabled():
        return net.load_state_dict(synthetic.lpips_state_dict(device=device))
    raise FileNotFoundError(f"{path} not found: export lpips.LPIPS(net='vgg').state_dict() there (or set CGD_SYNTHETIC_WEIGHTS=1)")
