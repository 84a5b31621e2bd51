"""Plugin surface `cgd.clip_util` (reference: /root/reference/cgd/clip_util.py).

Hot path: `CLIP_NORMALIZE` (:45, fused into the cutout kernel on the native path) and `load_clip(...)` whose
`.encode_image` / `.visual.input_resolution` (:59-66) are served by the MI355X image tower.  Prompt encoding
(`encode_text_prompt`, :104-108) is one-off setup: with the optional `clip` package installed it runs there, unchanged; without it a
checkpoint's text weights go to the native text tower (`cgd_amd.nets.ClipTextTower`) and prompts are tokenised by `cgd_amd.tokenizer`
(merges file: $CGD_CLIP_BPE or <cache>/clip/bpe_simple_vocab_16e6.txt.gz).  Synthetic-weight runs without text weights keep the
hash-seeded prompt embeddings.
"""
import hashlib
import os
from functools import lru_cache

import torch as th

from cgd_amd import nets as _nets
from cgd_amd import shard as _shard
from cgd_amd import synthetic as _synthetic
from cgd_amd import tokenizer as _tokenizer
from cgd_amd.guidance import CLIP_MEAN, CLIP_STD, MakeCutouts, MakeCutoutsResized  # noqa: F401

from . import script_util

CLIP_MODEL_NAMES = ("ViT-B/16", "ViT-B/32", "RN50", "RN101", "RN50x4", "RN50x16", "ViT-L/14")
_AZURE = "https://openaipublic.azureedge.net/clip/models/"
CLIP_MODEL_URLS = {
    "RN50": _AZURE + "afeb0e10f9e5a86da6080e35cf09123aca3b358a0c3e3b6c78a7b63bc04b6762/RN50.pt",
    "RN101": _AZURE + "8fa8567bab74a42d41c5915025a8e4538c3bdbe8804a470a72f30b0d94fab599/RN101.pt",
    "RN50x4": _AZURE + "7e526bd135e493cef0776de27d5f42653e6b4c8bf9e0f653bb11773263205fdd/RN50x4.pt",
    "RN50x16": _AZURE + "52378b407f34354e150460fe41077663dd5b39c54cd0bfd2b27167a4a06ec9aa/RN50x16.pt",
    "ViT-B/32": _AZURE + "40d365715913c9da98579312b702a82c18be219cc2a73407c4526f58eba950af/ViT-B-32.pt",
    "ViT-B/16": _AZURE + "5806e77cd80f8b59890b7e101eabd078d9fb84e6937f9e85e4ecb61988df416f/ViT-B-16.pt",
    "ViT-L/14": _AZURE + "b8cca3fd41ae0c99ba7e8951adf17d267cdb84cd88be6f7c2e0eca1737a03836/ViT-L-14.pt",
    "ViT-L/14@336px": _AZURE + "3035c92b350959924f9f00213499208652fc7ea050643e8b385c2dac08641f02/ViT-L-14-336px.pt",
}


class _Normalize:
    """torchvision.transforms.Normalize(mean, std) for (...,3,H,W) tensors."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, x):
        m = th.tensor(self.mean, dtype=x.dtype, device=x.device).view(3, 1, 1)
        s = th.tensor(self.std, dtype=x.dtype, device=x.device).view(3, 1, 1)
        return (x - m) / s


CLIP_NORMALIZE = _Normalize(CLIP_MEAN, CLIP_STD)


def download_clip_model(model_name: str) -> str:
    if model_name not in CLIP_MODEL_URLS:
        raise ValueError(f"Unknown CLIP model: {model_name}. Available: {list(CLIP_MODEL_URLS.keys())}")
    filename = model_name.replace("/", "-") + ".pt"
    cache_dir = os.path.join(script_util.CACHE_PATH, "clip")
    if script_util.synthetic_weights_enabled():
        return os.path.join(cache_dir, filename)
    return script_util.download(CLIP_MODEL_URLS[model_name], filename, root=cache_dir)


class _Visual:
    def __init__(self, tower):
        self.input_resolution = tower.input_resolution
        self.output_dim = tower.out_dim
        self.tower = tower


_EncodeImageFunction = _nets.EncodeImageFunction  # autograd node over cgd_*_forward / cgd_*_dgrad


class ClipModel:
    """The slice of clip.model.CLIP the generator touches: `.visual.input_resolution`, `.encode_image`, and (when a checkpoint with text
    weights is loaded) `.encode_text` — the `clip` package's text model when it is installed, else the native text tower."""

    def __init__(self, tower, text_model=None, name="ViT-B/32"):
        self.visual = _Visual(tower)
        self.tower = tower
        self.text_model = text_model
        self.name = name

    def encode_image(self, image):
        """(N,3,res,res) CLIP-normalised -> (N,D).  Differentiable w.r.t. `image` (autograd node over cgd_*_forward / _dgrad) so
        that a user-supplied cond_fn written like the reference's (cgd.py:190-228) works unchanged."""
        if image.requires_grad and th.is_grad_enabled():
            return _EncodeImageFunction.apply(image, self.tower)
        return self.tower.encode_image(image)

    def encode_text(self, tokens):
        if self.text_model is None:
            raise RuntimeError("text encoding needs a CLIP checkpoint with text weights (the native text tower, or the `clip` package)")
        return self.text_model.encode_text(tokens)

    @property
    def native_text(self):
        return isinstance(self.text_model, _nets.ClipTextTower)

    def eval(self):
        return self


def _vit_config_from_state_dict(sd):
    """clip.model.build_model's shape inference for the visual tower."""
    width = sd["visual.conv1.weight"].shape[0]
    layers = len([k for k in sd if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    patch = sd["visual.conv1.weight"].shape[-1]
    grid = round((sd["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    return (patch * grid, patch, width, layers, width // 64, sd["visual.proj"].shape[1])


def _text_config_from_state_dict(sd):
    """clip.model.build_model's shape inference for the text tower: (context_length, vocab_size, width, layers, heads, out_dim)."""
    width = sd["ln_final.weight"].shape[0]
    layers = len({k.split(".")[2] for k in sd if k.startswith("transformer.resblocks.")})
    return (sd["positional_embedding"].shape[0], sd["token_embedding.weight"].shape[0], width, layers, width // 64,
            sd["text_projection"].shape[1])


def parse_clip_model_name(model_name):
    """One `--clip_model` entry (after the 'A+B' split) -> (arch, activation, path).  open_clip architecture names are dash-spelled
    (`cgd_amd.nets.OPENCLIP_CONFIGS`, optional `-quickgelu` suffix): 'ARCH=PATH' loads the checkpoint PATH as that architecture, 'ARCH' alone is
    for CGD_SYNTHETIC_WEIGHTS=1.  Everything else — OpenAI's slash-spelled names, plain checkpoint paths — is (None, 'quick_gelu', model_name):
    today's behaviour."""
    head, sep, path = model_name.partition("=")
    arch = _nets.openclip_arch(head.strip())
    if arch is None:
        return None, "quick_gelu", model_name
    if sep and not path.strip():
        raise ValueError(f"{model_name}: 'ARCH=PATH' needs a checkpoint path after '='")
    return arch[0], arch[1], (path.strip() if sep else None)


def split_secondary(clip_model_name, image_size=None, height_offset=0, width_offset=0):
    """The '+'-separated `--clip_model` list -> (CLIP tower entries, secondary-model checkpoint path or None).  A `secondary=FILE` entry switches
    the secondary model on (`cgd_amd.nets.SecondaryModel`: the guidance gradient returns to x through it instead of through the UNet); it is a
    value like 'plmsN' and 'ARCH=FILE', counts as no tower, and FILE is not read under CGD_SYNTHETIC_WEIGHTS=1.  Refused here, before
    anything is loaded: a list with a secondary model but no CLIP tower, more than one secondary model, an empty FILE, and — when
    `image_size` is given — an image whose height or width (image_size + offset) is not a multiple of 32."""
    names, secondary = [], None
    for entry in (n.strip() for n in clip_model_name.split("+")):
        head, sep, path = entry.partition("=")
        if sep and head.strip() == "secondary":
            if secondary is not None:
                raise ValueError(f"{clip_model_name}: more than one 'secondary=FILE' entry")
            if not path.strip():
                raise ValueError(f"{entry}: 'secondary=FILE' needs a checkpoint path after '='")
            secondary = path.strip()
        else:
            names.append(entry)
    if secondary is not None:
        if not any(names):
            raise ValueError(f"{clip_model_name}: 'secondary=FILE' needs a CLIP tower beside it, e.g. 'ViT-B/32+secondary=FILE'")
        if image_size is not None:
            for what, size in (("height", image_size + height_offset), ("width", image_size + width_offset)):
                if size % 32:
                    raise ValueError(f"the secondary model needs an image {what} that is a multiple of 32, got {size} "
                                     f"(image_size {image_size} + offset {size - image_size})")
    return names, secondary


CUTS_SWITCH_FRACTION = 0.4  # 'cuts=A:B/C:D': the first pair while less than this fraction of the run is done, the second afterwards


def split_cuts(clip_model_name, progressive_cutout=False, use_augs=False):
    """The '+'-separated `--clip_model` list -> (the list without its `cuts=` entry, None or (overview, inner, schedule)).  A `cuts=OV:IN`
    entry switches the resized overview + inner cutouts on (`cgd_amd.guidance.MakeCutoutsResized(cut_size, overview, inner, schedule=schedule)`);
    `cuts=OV:IN/OV2:IN2` uses the first pair while less than 40 % of the run is done and the second afterwards.  It is a value like 'plmsN' and
    'secondary=FILE' and counts as no tower.  Refused here, before anything is loaded: a malformed value (counts that are not non-negative
    integers, a pair without a cut, more than two pairs, more than one entry), a list with no tower beside it, and the entry together with
    progressive cutouts or cutout augmentations (the cut counts follow the entry's own schedule, and the resized cutter has no augmentations)."""
    names, cuts = [], None
    for entry in (n.strip() for n in clip_model_name.split("+")):
        head, sep, value = entry.partition("=")
        if not (sep and head.strip() == "cuts"):
            names.append(entry)
            continue
        if cuts is not None:
            raise ValueError(f"{clip_model_name}: more than one 'cuts=' entry")
        pairs = []
        for part in value.split("/"):
            fields = part.strip().split(":")
            if len(fields) != 2 or not all(f.strip().isdigit() for f in fields):
                raise ValueError(f"{entry}: expected 'cuts=OV:IN' or 'cuts=OV:IN/OV2:IN2' with non-negative integer counts")
            ov, inn = int(fields[0]), int(fields[1])
            if ov + inn < 1:
                raise ValueError(f"{entry}: a pair needs at least one cut")
            pairs.append((ov, inn))
        if len(pairs) > 2:
            raise ValueError(f"{entry}: at most two OV:IN pairs")
        cuts = (*pairs[-1], [(CUTS_SWITCH_FRACTION, *pairs[0])] if len(pairs) == 2 else None)
    if cuts is not None:
        if not any(n and not n.startswith("secondary=") for n in names):
            raise ValueError(f"{clip_model_name}: 'cuts=' needs a CLIP tower beside it, e.g. 'ViT-B/32+cuts=4:12'")
        if progressive_cutout:
            raise ValueError("'cuts=' sets the cut counts of every step itself: it cannot be combined with --progressive-cutout")
        if use_augs:
            raise ValueError("'cuts=' selects the resized cutouts, which have no use_augs augmentations")
    return "+".join(names), cuts


def load_secondary(ctx, path, device):
    """The device secondary model (`secondary=FILE`): FILE is the published secondary_model_imagenet_2.pth state dict (or a checkpoint that
    wraps it as {'state_dict': ...}), read on rank 0 and broadcast; with CGD_SYNTHETIC_WEIGHTS=1 seeded random weights, FILE is not read."""
    dev = f"cuda:{ctx.device}"
    net = _nets.SecondaryModel(ctx)
    if script_util.synthetic_weights_enabled():
        _shard.load_broadcast(net, lambda: _synthetic.secondary_state_dict(device=dev), dev)
        return net
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found (set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")
    _shard.load_broadcast(net, lambda: _openclip_clean_state_dict(th.load(path, map_location="cpu")), dev)
    return net


_NO_TOWER_ENTRIES = ("secondary=", "cuts=", "classifier=", "aesthetic=")
AESTHETIC_PLUS_HINT = ("the list is split on '+', so a checkpoint whose own name contains '+' (sac+logos+ava1-l14-linearMSE.pth) has to be "
                       "renamed or symlinked first")


def _known_tower_entry(entry):
    """Can load_clip make something of this piece of the list: a tower name, an open_clip 'ARCH' or 'ARCH=FILE', or a checkpoint file?"""
    return (entry in CLIP_MODEL_URLS or entry in _nets.VIT_CONFIGS or entry in _nets.RN_CONFIGS
            or _nets.openclip_arch(entry.partition("=")[0].strip()) is not None or os.path.isfile(entry))


def split_aesthetic(clip_model_name):
    """The '+'-separated `--clip_model` list -> (the list without its `aesthetic=` entries, one (FILE, SCALE) or None per tower entry of that
    list, in order).  An `aesthetic=FILE:SCALE` entry puts an aesthetic predictor (`cgd_amd.nets.AestheticHead`: the guidance loss gains
    -SCALE * sum_b mean_cut score) on the tower entry BEFORE it, `secondary=` / `cuts=` / `classifier=` entries in between not counting:
    'ViT-L/14+aesthetic=sa_0_4_vit_l_14_linear.pth:500+ViT-B/32' scores ViT-L/14's embeddings only.  It is a value like 'secondary=FILE' and
    counts as no tower.  FILE may contain colons of its own: it is split from SCALE at the last ':'; a negative SCALE steers away.  FILE is not
    read under CGD_SYNTHETIC_WEIGHTS=1.  Refused here, before anything is loaded (FILE is never opened): no tower before the entry, an empty
    FILE, a SCALE that is missing, not a finite float or zero, and two heads on one tower.  A list without the entry passes through unchanged
    (the very string).  The list is split on '+': a checkpoint whose own name contains '+' has to be renamed or symlinked, and the errors
    about a missing SCALE and about an unknown piece behind an `aesthetic=` entry say so."""
    entries = [n.strip() for n in clip_model_name.split("+")]
    if not any(e.partition("=")[1] and e.partition("=")[0].strip() == "aesthetic" for e in entries):
        return clip_model_name, [None] * sum(1 for e in entries if e and not e.startswith(_NO_TOWER_ENTRIES))
    names, heads, seen = [], [], False
    for entry in entries:
        head, sep, value = entry.partition("=")
        if not (sep and head.strip() == "aesthetic"):
            names.append(entry)
            if entry and not entry.startswith(_NO_TOWER_ENTRIES):
                if seen and not _known_tower_entry(entry):
                    raise ValueError(f"{clip_model_name}: '{entry}' behind an 'aesthetic=' entry is no CLIP tower, checkpoint file or known entry; "
                                     f"{AESTHETIC_PLUS_HINT}")
                heads.append(None)
            continue
        seen = True
        usage = f"{entry}: expected 'aesthetic=FILE:SCALE' (SCALE a finite non-zero number); {AESTHETIC_PLUS_HINT}"
        if not heads:
            raise ValueError(f"{clip_model_name}: 'aesthetic=' needs a CLIP tower before it, e.g. 'ViT-L/14+aesthetic=FILE:500'")
        path, colon, scale_text = value.strip().rpartition(":")
        path, scale_text = path.strip(), scale_text.strip()
        if not colon:
            raise ValueError(usage if value.strip() else f"{entry}: 'aesthetic=FILE:SCALE' needs a checkpoint path after '='")
        if not path:
            raise ValueError(f"{entry}: 'aesthetic=FILE:SCALE' needs a checkpoint path after '='")
        try:
            scale = float(scale_text)
        except ValueError:
            raise ValueError(usage) from None
        if scale != scale or scale in (float("inf"), float("-inf")) or scale == 0:
            raise ValueError(f"{entry}: SCALE must be a finite non-zero number, got {scale_text}")
        if heads[-1] is not None:
            raise ValueError(f"{clip_model_name}: two 'aesthetic=' entries on one tower ('{heads[-1][0]}' and '{path}'); each binds to the tower "
                             "entry before it")
        heads[-1] = (path, scale)
    return "+".join(names), heads


def load_aesthetic(ctx, path, device, dim, what="the tower"):
    """The device aesthetic head (`aesthetic=FILE:SCALE`) for a tower of embedding width `dim`: FILE is a published linear or five-layer
    predictor (nets.collapse_aesthetic_state_dict), read and collapsed on rank 0 and broadcast as one (dim + 1,) vector; a head of another
    width is refused naming both.  With CGD_SYNTHETIC_WEIGHTS=1 a seeded head, FILE is not read."""
    dev = f"cuda:{ctx.device}"
    head = _nets.AestheticHead(dim, dev)
    if script_util.synthetic_weights_enabled():
        _shard.load_broadcast(head, lambda: _synthetic.aesthetic_head(dim), dev)
        return head
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found (set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")
    held = {}

    def probe():  # rank 0 only: the other ranks receive the width, never the file
        held["vec"] = _nets.collapse_aesthetic_state_dict(th.load(path, map_location="cpu"))
        return held["vec"].numel() - 1

    got = _shard.on_rank0(probe)
    if got != dim:
        raise ValueError(f"{path} is an aesthetic head for {got}-wide embeddings, {what} gives {dim}")
    _shard.load_broadcast(head, lambda: {"head": held["vec"]}, dev)
    held.clear()
    return head


def split_classifier(clip_model_name, height_offset=0, width_offset=0):
    """The '+'-separated `--clip_model` list -> (the list without its `classifier=` entry, None or (FILE, CLASS, SCALE)).  A
    `classifier=FILE:CLASS[:SCALE]` entry switches classifier guidance on (`cgd_amd.nets.NoisyClassifier`: the guidance loss gains
    -SCALE * sum_b log p(CLASS | x_t, t), SCALE defaults to 1); it is a value like 'secondary=FILE' and 'cuts=OV:IN' and counts as no tower.
    FILE may contain colons of its own: CLASS and SCALE are taken from the right.  Refused here, before anything is loaded (FILE is never
    opened): more than one entry, an empty FILE, a missing or non-integer CLASS, a negative CLASS, SCALE <= 0 or not a number, a list with no
    tower beside it, and a non-zero height or width offset (the classifier's positional embedding fixes the map size)."""
    names, found = [], None
    for entry in (n.strip() for n in clip_model_name.split("+")):
        head, sep, value = entry.partition("=")
        if not (sep and head.strip() == "classifier"):
            names.append(entry)
            continue
        if found is not None:
            raise ValueError(f"{clip_model_name}: more than one 'classifier=' entry")
        usage = f"{entry}: expected 'classifier=FILE:CLASS' or 'classifier=FILE:CLASS:SCALE' (CLASS an integer class id, SCALE > 0)"
        fields = [f.strip() for f in value.strip().split(":")]

        def is_int(f):
            return f.isdigit() or (f[:1] in "+-" and f[1:].isdigit())

        def is_number(f):
            try:
                float(f)
            except ValueError:
                return False
            return True

        # taken from the right: two trailing numeric fields with an integer first are CLASS:SCALE, one trailing integer is CLASS
        if len(fields) >= 3 and is_int(fields[-2]) and is_number(fields[-1]):
            path, cls, scale = ":".join(fields[:-2]), int(fields[-2]), float(fields[-1])
        elif len(fields) >= 2 and is_int(fields[-1]):
            path, cls, scale = ":".join(fields[:-1]), int(fields[-1]), 1.0
        else:
            raise ValueError(usage)
        if not path:
            raise ValueError(usage)
        if cls < 0:
            raise ValueError(f"{entry}: CLASS must be a non-negative class id")
        if not (0.0 < scale < float("inf")):
            raise ValueError(f"{entry}: SCALE must be a positive number, got {fields[-1]}")
        found = (path, cls, scale)
    if found is not None:
        if not any(n and not n.startswith(("secondary=", "cuts=")) for n in names):
            raise ValueError(f"{clip_model_name}: 'classifier=' needs a CLIP tower beside it, e.g. 'ViT-B/32+classifier=FILE:207'")
        if height_offset or width_offset:
            raise ValueError("'classifier=' needs height_offset = width_offset = 0: the classifier's positional embedding fixes the map size "
                             f"(got {height_offset}, {width_offset})")
    return "+".join(names), found


def classifier_config_from_state_dict(sd, num_head_channels=None):
    """The configuration of a noisy-classifier checkpoint (guided-diffusion's `EncoderUNetModel`, pool="attention"), as the keyword arguments
    of `cgd_amd.nets.NoisyClassifier`, and the cleaned state dict: -> (state dict, kwargs).  Every dimension is inferred from shapes and the
    key set: the width from `time_embed.0.weight` / `input_blocks.0.0.weight`, the final map S from the positional embedding (S*S + 1
    positions), the classes from `out.2.c_proj`, levels and depth from the numbered input blocks (the one split of them into `levels` runs of
    `depth` blocks with a `down` block between runs in which every run has one width and one attention flag and no `down` block attends or
    changes the width), image_size = S * 2^(levels-1), channel_mult and the attention resolutions from the runs.  The head width is in no
    shape: it comes from `nets.CLASSIFIER_CONFIGS[image_size]`, else from `num_head_channels`, else 64.  For a published size everything
    inferred must equal the table's entry.  A `{'state_dict': ...}` wrapper and `module.` prefixes are removed.  ValueError names what does
    not fit."""
    sd = _openclip_clean_state_dict(sd)
    for key in ("input_blocks.0.0.weight", "out.2.positional_embedding", "out.2.qkv_proj.weight", "out.2.c_proj.weight", "time_embed.0.weight"):
        if key not in sd:
            raise ValueError(f"classifier checkpoint: no '{key}' (not an EncoderUNetModel with pool='attention')")
    if any(k.startswith(("output_blocks.", "label_emb.")) for k in sd):
        raise ValueError("classifier checkpoint: it has output_blocks / label_emb — a diffusion UNet, not a classifier")
    ch0 = int(sd["input_blocks.0.0.weight"].shape[0])
    width = int(sd["time_embed.0.weight"].shape[1])
    idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("input_blocks.")})
    if idx != list(range(len(idx))):
        raise ValueError(f"classifier checkpoint: input_blocks are not numbered 0..{len(idx) - 1} (a level is missing)")
    widths, att = [], []
    for i in idx[1:]:
        k = f"input_blocks.{i}.0.in_layers.2.weight"
        if k not in sd:
            raise ValueError(f"classifier checkpoint: no '{k}'")
        widths.append(int(sd[k].shape[0]))
        att.append(f"input_blocks.{i}.1.qkv.weight" in sd)
    C, T = (int(v) for v in sd["out.2.positional_embedding"].shape)
    S = round((T - 1) ** 0.5)
    if S < 1 or S * S + 1 != T:
        raise ValueError(f"classifier checkpoint: positional_embedding has {T} positions, not S*S + 1")
    if tuple(sd["out.2.qkv_proj.weight"].shape[:2]) != (3 * C, C):
        raise ValueError(f"classifier checkpoint: qkv_proj.weight is {tuple(sd['out.2.qkv_proj.weight'].shape)}, not (3C, C) with C = {C}")
    out_channels = int(sd["out.2.c_proj.weight"].shape[0])
    n = len(widths)
    fits = []
    for depth in range(1, n + 1):
        if (n + 1) % (depth + 1):
            continue
        levels = (n + 1) // (depth + 1)
        runs, ok, prev = [], levels <= 8, ch0
        for level in range(levels):
            lo = level * (depth + 1)
            run_w, run_a = widths[lo:lo + depth], att[lo:lo + depth]
            ok = ok and len(set(run_w)) == 1 and len(set(run_a)) == 1
            if level != levels - 1:  # the `down` block behind the run: same width, no attention
                ok = ok and widths[lo + depth] == run_w[0] and not att[lo + depth]
            runs.append((run_w[0], run_a[0]))
        if ok:
            fits.append((levels, depth, runs))
    if len(fits) != 1:
        raise ValueError(f"classifier checkpoint: the {n} input blocks after the stem split into levels of equal depth in {len(fits)} ways "
                         "(a level is missing, or the block widths / attention blocks are not an EncoderUNetModel's)")
    levels, depth, runs = fits[0]
    if runs[0][0] != ch0 or runs[-1][0] != C:
        raise ValueError(f"classifier checkpoint: first / last level widths {runs[0][0]} / {runs[-1][0]} against the stem's {ch0} and the pool's {C}")
    if width <= 0 or any(w * 2 % width for w, _ in runs):
        raise ValueError(f"classifier checkpoint: level widths {[w for w, _ in runs]} are not multiples of half the width {width}")
    size = S * 2 ** (levels - 1)
    mult = tuple((w // width) if w % width == 0 else w / width for w, _ in runs)
    res = [size >> level for level, (_, a) in enumerate(runs) if a]
    if not res:
        raise ValueError("classifier checkpoint: no level carries attention")
    table = _nets.CLASSIFIER_CONFIGS.get(size)
    kw = dict(image_size=size, model_channels=width, num_res_blocks=depth, attention_resolutions=",".join(str(r) for r in res),
              channel_mult=mult, num_head_channels=int(table["num_head_channels"] if table else (num_head_channels or 64)), out_channels=out_channels)
    if table:
        for name in ("model_channels", "num_res_blocks", "attention_resolutions", "channel_mult", "out_channels"):
            got, want = kw[name], table[name]
            if (tuple(float(v) for v in got) != tuple(float(v) for v in want)) if name == "channel_mult" else got != want:
                raise ValueError(f"classifier checkpoint ({size}x{size}): {name} {got}, the published architecture has {want}")
    if C % kw["num_head_channels"]:
        raise ValueError(f"classifier checkpoint: final width {C} is not a whole number of {kw['num_head_channels']}-wide heads")
    return sd, kw


def load_classifier(ctx, path, device, image_size=None):
    """The device classifier (`classifier=FILE:CLASS[:SCALE]`): FILE is a published NxN_classifier.pt state dict, read on rank 0 and
    broadcast; with CGD_SYNTHETIC_WEIGHTS=1 seeded random weights of the `image_size` classifier, FILE is not read."""
    dev = f"cuda:{ctx.device}"
    if script_util.synthetic_weights_enabled():
        if image_size not in _nets.CLASSIFIER_CONFIGS:
            raise ValueError(f"no published classifier for image size {image_size}: {sorted(_nets.CLASSIFIER_CONFIGS)}")
        net = _nets.NoisyClassifier(ctx, **_nets.CLASSIFIER_CONFIGS[image_size])
        _shard.load_broadcast(net, lambda: _synthetic.classifier_state_dict(net.cfg, device=dev), dev)
        return net
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found (set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")
    held = {}

    def probe():  # rank 0 only: the other ranks receive the configuration, never the file
        held["sd"], kw = classifier_config_from_state_dict(th.load(path, map_location="cpu"))
        return kw

    kw = _shard.on_rank0(probe)
    net = _nets.NoisyClassifier(ctx, **kw)
    _shard.load_broadcast(net, lambda: {k: v.float() for k, v in held["sd"].items()}, dev)
    held.clear()
    return net


def _openclip_clean_state_dict(sd):
    """open_clip training checkpoints wrap the weights ({'state_dict': ...}) and DataParallel prefixes every key with 'module.'; entries that are
    not tensors go (epoch counters and the like).  `logit_scale`, `attn_mask` and other tensors no tower asks for are simply never read."""
    if isinstance(sd, dict) and isinstance(sd.get("state_dict"), dict):
        sd = sd["state_dict"]
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items() if isinstance(v, th.Tensor)}


def openclip_configs_from_state_dict(arch, sd):
    """The tower configurations of an open_clip checkpoint loaded as architecture `arch`: every dimension is inferred from tensor shapes as for
    OpenAI's checkpoints, except the head counts, which no shape reveals (ViT-H-14: width 1280, 16 heads of 80) and which come from the table.
    The inferred dimensions must equal the table's (ValueError names the first that does not); a tower whose MLP is not 4 x width (g-14,
    bigG-14) is refused.  -> (cleaned state dict, image tower config, text tower config or None)."""
    sd = _openclip_clean_state_dict(sd)
    if "visual.proj" not in sd or "visual.conv1.weight" not in sd:
        raise NotImplementedError(f"{arch}: the checkpoint has no ViT image tower in open_clip's native key scheme (visual.conv1 / visual.proj)")
    vit_table, text_table = _nets.OPENCLIP_CONFIGS[arch]
    towers = [("image", "visual.transformer.resblocks.0.mlp.c_fc.weight", sd["visual.conv1.weight"].shape[0])]
    have_text = "text_projection" in sd
    if have_text:
        towers.append(("text", "transformer.resblocks.0.mlp.c_fc.weight", sd["ln_final.weight"].shape[0]))
    for tower, key, width in towers:
        if key in sd and tuple(sd[key].shape) != (4 * width, width):
            raise NotImplementedError(f"{arch}: the {tower} tower's mlp.c_fc.weight is {tuple(sd[key].shape)}, not 4 x width = {(4 * width, width)}: "
                                      "towers with another MLP ratio (ViT-g-14, ViT-bigG-14) are not supported")
    vit = _vit_config_from_state_dict(sd)
    vit = vit[:4] + (vit_table[4],) + vit[5:]
    text = None
    if have_text:
        text = _text_config_from_state_dict(sd)
        text = text[:4] + (text_table[4],) + text[5:]
    fields = {"image": ("resolution", "patch", "width", "layers", "heads", "out_dim"),
              "text": ("context_length", "vocab_size", "width", "layers", "heads", "out_dim")}
    for tower, got, want in (("image", vit, vit_table), ("text", text, text_table)):
        for name, g, w in zip(fields[tower], got or (), want):
            if int(g) != int(w):
                raise ValueError(f"{arch}: the checkpoint's {tower} tower has {name} {int(g)}, the architecture has {int(w)}")
    return sd, tuple(int(v) for v in vit), (tuple(int(v) for v in text) if text else None)


def _is_text_key(k):
    return k.startswith(("token_embedding.", "transformer.", "ln_final.")) or k in ("positional_embedding", "text_projection")


def _clip_importable():
    try:
        import clip  # noqa: F401  (optional, setup-time only)
    except ImportError:
        return False
    return True


def _rn_config_from_state_dict(sd):
    """clip.model.build_model's shape inference for a ModifiedResNet tower."""
    counts = [len({k.split(".")[2] for k in sd if k.startswith(f"visual.layer{b}")}) for b in (1, 2, 3, 4)]
    width = sd["visual.layer1.0.conv1.weight"].shape[0]
    grid = round((sd["visual.attnpool.positional_embedding"].shape[0] - 1) ** 0.5)
    out_dim = sd["visual.attnpool.c_proj.weight"].shape[0]
    return (grid * 32, width, tuple(counts), out_dim, width * 32 // 64)


@lru_cache(maxsize=4)  # the reference caches one model; "A+B" multi-CLIP runs keep several
def load_clip(model_name="ViT-B/32", device="cpu"):
    print(f"Loading clip model\t{model_name}\ton device\t{device}.")
    if device == "cpu" or "cuda" not in device:
        raise ValueError("Invalid or unspecified device: {} (the MI355X path needs 'cuda[:N]'; no CPU fallback)".format(device))
    ctx = script_util.get_context(device)
    arch, activation, arch_path = parse_clip_model_name(model_name)
    if arch is not None:
        return _load_openclip(ctx, model_name, arch, activation, arch_path, device)
    model_path = download_clip_model(model_name) if model_name in CLIP_MODEL_URLS else model_name
    if os.path.isfile(model_path):
        held = {}
        have_clip = _clip_importable()

        def probe():  # rank 0 only (multi-GPU runs): un-pickle the archive once, infer the tower(s) like clip.model.build_model
            try:
                sd = th.jit.load(model_path, map_location="cpu").state_dict()
            except RuntimeError:
                sd = th.load(model_path, map_location="cpu")
            held["sd"] = sd
            text_cfg = _text_config_from_state_dict(sd) if (not have_clip and "text_projection" in sd) else None
            if "visual.proj" in sd:
                return "vit", _vit_config_from_state_dict(sd), text_cfg
            return "rn", _rn_config_from_state_dict(sd), text_cfg

        kind, cfg, text_cfg = _shard.on_rank0(probe)  # the other ranks receive the configurations, never the file
        tower = _nets.ClipImageTower(ctx, config=cfg) if kind == "vit" else _nets.ClipResNetTower(ctx, config=cfg)
        _shard.load_broadcast(tower, lambda: {k: v.float() for k, v in held["sd"].items() if k.startswith("visual.")},
                              f"cuda:{ctx.device}", prefix="visual.")
        text_model = None
        if have_clip:
            import clip
            text_model = clip.load(model_path, jit=False, device=device)[0].eval().requires_grad_(False)
        elif text_cfg is not None:  # no `clip` package: the archive's text weights go to the native text tower
            text_model = _nets.ClipTextTower(ctx, config=text_cfg)
            _shard.load_broadcast(text_model, lambda: {k: v.float() for k, v in held["sd"].items() if _is_text_key(k)}, f"cuda:{ctx.device}")
        held.clear()
        return ClipModel(tower, text_model, model_name), tower.input_resolution
    if script_util.synthetic_weights_enabled():
        if model_name in _nets.VIT_CONFIGS:
            tower = _nets.ClipImageTower(ctx, model_name)
            _shard.load_broadcast(tower, lambda: _synthetic.synthetic_state_dict(tower, seed=4321, device=f"cuda:{ctx.device}"),
                                  f"cuda:{ctx.device}")
        elif model_name in _nets.RN_CONFIGS:
            tower = _nets.ClipResNetTower(ctx, model_name)
            _shard.load_broadcast(tower, lambda: _synthetic.resnet_state_dict(tower, seed=2468, device=f"cuda:{ctx.device}"),
                                  f"cuda:{ctx.device}")
        else:
            raise NotImplementedError(f"{model_name}: supported towers are {sorted(_nets.VIT_CONFIGS) + sorted(_nets.RN_CONFIGS)}")
        return ClipModel(tower, None, model_name), tower.input_resolution
    raise FileNotFoundError(f"{model_path} not found (set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")


def _load_openclip(ctx, model_name, arch, activation, path, device):
    """An open_clip (LAION) ViT: 'ARCH=PATH' reads the checkpoint into the native image and text towers (the `clip` package cannot build these
    models, so prompts always go through the native text tower), 'ARCH' alone draws seeded random weights under CGD_SYNTHETIC_WEIGHTS=1."""
    dev = f"cuda:{ctx.device}"
    if path is None:
        if not script_util.synthetic_weights_enabled():
            raise FileNotFoundError(f"{model_name}: give the checkpoint as '{model_name}=PATH' (or set CGD_SYNTHETIC_WEIGHTS=1 for seeded random weights)")
        tower = _nets.ClipImageTower(ctx, config=_nets.OPENCLIP_CONFIGS[arch][0], activation=activation)
        _shard.load_broadcast(tower, lambda: _synthetic.synthetic_state_dict(tower, seed=4321, device=dev), dev)
        return ClipModel(tower, None, model_name), tower.input_resolution
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not found")
    held = {}

    def probe():  # rank 0 only: the other ranks receive the configurations, never the file
        try:
            sd = th.jit.load(path, map_location="cpu").state_dict()
        except RuntimeError:
            sd = th.load(path, map_location="cpu")
        held["sd"], cfg, text_cfg = openclip_configs_from_state_dict(arch, sd)
        return cfg, text_cfg

    cfg, text_cfg = _shard.on_rank0(probe)
    tower = _nets.ClipImageTower(ctx, config=cfg, activation=activation)
    _shard.load_broadcast(tower, lambda: {k: v.float() for k, v in held["sd"].items() if k.startswith("visual.")}, dev, prefix="visual.")
    text_model = None
    if text_cfg is not None:
        text_model = _nets.ClipTextTower(ctx, config=text_cfg, activation=activation)  # the same activation as its image tower
        _shard.load_broadcast(text_model, lambda: {k: v.float() for k, v in held["sd"].items() if _is_text_key(k)}, dev)
    held.clear()
    return ClipModel(tower, text_model, model_name), tower.input_resolution


def _synthetic_text_embedding(txt, dim, device):
    seed = int.from_bytes(hashlib.sha256(txt.encode()).digest()[:8], "little") % (2 ** 31)
    return th.randn(1, dim, generator=th.Generator().manual_seed(seed)).to(device)


def encode_text_prompt(txt, weight, clip_model_name="ViT-B/32", device="cpu"):
    clip_model, _ = load_clip(clip_model_name, device)
    if clip_model.text_model is None:
        if script_util.synthetic_weights_enabled():
            return _synthetic_text_embedding(txt, clip_model.visual.output_dim, device), weight
        raise RuntimeError("encode_text_prompt needs a CLIP checkpoint with text weights (native text tower) or the `clip` package")
    if clip_model.native_text:
        tokens = _tokenizer.tokenize(txt, clip_model.text_model.context_length, checkpoints_dir=script_util.CACHE_PATH)
        return clip_model.encode_text(tokens.to(device)).float(), weight
    import clip
    tokens = clip.tokenize(txt).to(device)
    return clip_model.encode_text(tokens).float(), weight


def encode_image_prompt(image: str, weight: float, diffusion_size: int, num_cutouts, clip_model_name: str = "ViT-B/32",
                        device: str = "cpu"):
    """Image prompt -> (cutn, D) embeddings with weight/cutn each (reference :90-101).  The reference resizes with the
    vendored ResizeRight lanczos3; here PIL's LANCZOS does the one-off resize (setup-time, outside the hot path)."""
    import numpy as np
    from PIL import Image
    clip_model, clip_size = load_clip(clip_model_name, device)
    make_cutouts = MakeCutouts(cut_size=clip_size, num_cutouts=num_cutouts, ctx=clip_model.tower.ctx)
    pil_img = Image.open(script_util.fetch(image)).convert("RGB")
    smallest = min(diffusion_size, *pil_img.size)
    scale = smallest / min(pil_img.size)
    pil_img = pil_img.resize((max(1, round(pil_img.size[0] * scale)), max(1, round(pil_img.size[1] * scale))), Image.LANCZOS)
    img = th.from_numpy(np.asarray(pil_img)).float().div(255).permute(2, 0, 1).unsqueeze(0).to(device)
    batch = make_cutouts(img)
    # quirk kept: the reference's `tf` is torch.nn.functional, so `tf.normalize(batch)` (clip_util.py:99) L2-normalises along the
    # channel axis instead of applying CLIP_NORMALIZE
    batch_embed = clip_model.encode_image(th.nn.functional.normalize(batch)).float()
    return batch_embed, [weight / make_cutouts.cutn] * make_cutouts.cutn
