"""Region prompts: a prompt acts on a cutout in proportion to the share of the prompt's mask that the cutout sees (include/cgd_mi355x.h,
cgd_spherical_loss_regions).  Host side: masks from a file or a box, their summed-area tables, and the plan ClipGuidance hands to the
`_regions` loss entries.  Everything here runs once per run; the coverage itself is computed inside the loss kernels from the table.

A region is a uint8 (H, W) mask of the frame, 255 inside and 0 outside.  Its table S is int32 (H+1, W+1), S[y][x] = sum of the mask over rows
< y and columns < x.  For a cutout box (oy, ox, h, w): cov = (S[oy+h][ox+w] - S[oy][ox+w] - S[oy+h][ox] + S[oy][ox]) / (255 h w), 0 for an
empty box, and prompt p weighs cov[region_of[p]] ** power[p] times its weight on that cutout (region_of -1: everywhere, factor 1)."""
import torch as th

INT32_LIMIT = 1 << 31


def parse_box(spec):
    """'x0,y0,x1,y1' in fractions of the frame -> the four floats, None for anything that is no list of numbers (a file name).  A list of
    numbers that is no box (another count, outside [0, 1], x0 >= x1 or y0 >= y1) is refused."""
    try:
        vals = [float(v) for v in str(spec).split(",")]
    except ValueError:
        return None
    if len(vals) != 4 or not all(0.0 <= v <= 1.0 for v in vals) or not (vals[0] < vals[2] and vals[1] < vals[3]):
        raise ValueError(f"region {spec!r}: a box is 'x0,y0,x1,y1' with 0 <= x0 < x1 <= 1 and 0 <= y0 < y1 <= 1 (fractions of the frame)")
    return vals


def parse_region(spec, H, W):
    """A mask file (opened as 'L', resized to W x H as the init mask is) or a box 'x0,y0,x1,y1' in fractions of the frame -> uint8 (H, W).
    Pixel (i, j) is inside a box when x0 W <= j + 0.5 < x1 W and y0 H <= i + 0.5 < y1 H; a box that contains no pixel centre is refused."""
    box = parse_box(spec)
    if box is None:
        import numpy as np
        from PIL import Image
        from .cgd import script_util
        pil = Image.open(script_util.fetch(spec)).convert("L").resize((W, H))
        return th.from_numpy(np.array(pil)).to(th.uint8).contiguous()
    x0, y0, x1, y1 = box
    cx, cy = th.arange(W, dtype=th.float64) + 0.5, th.arange(H, dtype=th.float64) + 0.5
    inx, iny = (cx >= x0 * W) & (cx < x1 * W), (cy >= y0 * H) & (cy < y1 * H)
    if not bool(inx.any()) or not bool(iny.any()):
        raise ValueError(f"region {spec!r} contains no pixel centre of the {H} x {W} frame")
    return ((iny[:, None] & inx[None, :]).to(th.uint8) * 255).contiguous()


def build_sat(masks):
    """uint8 (R, H, W) masks (or a list of (H, W) ones) -> their summed-area tables, int32 (R, H+1, W+1).  A frame whose full sum
    255 H W does not fit int32 is refused."""
    if isinstance(masks, (list, tuple)):
        masks = th.stack(list(masks))
    if masks.dim() != 3 or masks.dtype != th.uint8 or masks.shape[0] < 1:
        raise ValueError(f"region masks must be uint8 (R, H, W) with R >= 1, got {masks.dtype} {tuple(masks.shape)}")
    R, H, W = masks.shape
    if 255 * H * W >= INT32_LIMIT:
        raise ValueError(f"region masks of {H} x {W}: 255 H W must stay below 2^31 (the summed-area table is int32)")
    sat = th.zeros((R, H + 1, W + 1), dtype=th.int64)
    sat[:, 1:, 1:] = masks.cpu().to(th.int64).cumsum(1).cumsum(2)
    assert int(sat.max()) < INT32_LIMIT
    return sat.to(th.int32)


class RegionPlan:
    """What the `_regions` loss entries take on top of the plain ones, for the P prompts of a run in the order of its weight list:
    `sat` int32 (R, H+1, W+1), `region_of` (P,) table index or -1, `power` (P,) > 0.  Holds the device tensors, the host copy of region_of
    (checked here and handed to every launch, which checks it again), and `coverage`, the float64 host restatement."""

    def __init__(self, sat, region_of, power=None, device=None):
        sat = th.as_tensor(sat)
        if sat.dim() != 3 or sat.dtype != th.int32 or sat.shape[0] < 1 or sat.shape[1] < 2 or sat.shape[2] < 2:
            raise ValueError(f"sat must be int32 (R, H+1, W+1) with R >= 1, got {sat.dtype} {tuple(sat.shape)}")
        self.R, self.H, self.W = sat.shape[0], sat.shape[1] - 1, sat.shape[2] - 1
        if 255 * self.H * self.W >= INT32_LIMIT:
            raise ValueError(f"regions of {self.H} x {self.W}: 255 H W must stay below 2^31 (the summed-area table is int32)")
        self.region_of_host = th.as_tensor(region_of, dtype=th.int32).flatten().cpu().contiguous()
        self.P = self.region_of_host.numel()
        self.power_host = (th.ones(self.P) if power is None else th.as_tensor(power, dtype=th.float32).flatten().cpu()).contiguous()
        if self.power_host.numel() != self.P:
            raise ValueError(f"{self.P} region_of entries need {self.P} powers, got {self.power_host.numel()}")
        if not bool((self.power_host > 0).all()):
            raise ValueError(f"region powers must be positive, got {self.power_host.tolist()}")
        self.validate()
        self.sat_host = sat.cpu().contiguous()
        self.sat = self.region_of = self.power = None
        if device is not None:
            self.to(device)

    def validate(self):
        """region_of entries are table indices in [-1, R): checked on the host copy before every launch."""
        r = self.region_of_host
        if r.numel() and (int(r.min()) < -1 or int(r.max()) >= self.R):
            raise ValueError(f"region_of entries must be in [-1, {self.R}), got {r.tolist()}")

    def to(self, device):
        if self.sat is None or self.sat.device != th.device(device):
            self.sat, self.region_of, self.power = (t.to(device) for t in (self.sat_host, self.region_of_host, self.power_host))
        return self

    def columns(self, cols):
        """The plan of the prompts `cols` (same tables): how ClipGuidance splits it into the target and the direction part."""
        cols = list(cols)
        sub = RegionPlan.__new__(RegionPlan)
        sub.__dict__.update(self.__dict__)
        sub.region_of_host, sub.power_host, sub.P = self.region_of_host[cols].contiguous(), self.power_host[cols].contiguous(), len(cols)
        if self.sat is not None:
            idx = th.as_tensor(cols, dtype=th.long, device=self.sat.device)
            sub.region_of, sub.power = self.region_of[idx].contiguous(), self.power[idx].contiguous()
        return sub

    def args(self, geo):
        """The trailing arguments of a `_regions` entry in front of the stream: sat, region_of, region_of_host, power, geo, R, H, W."""
        self.validate()
        return (self.sat.data_ptr(), self.region_of.data_ptr(), self.region_of_host.data_ptr(), self.power.data_ptr(), geo.data_ptr(),
                self.R, self.H, self.W)

    def coverage(self, boxes):
        """float64 (len(boxes), P): cov ** power of every prompt on the boxes (oy, ox, h, w), from the table; 1 where region_of is -1."""
        S = self.sat_host.to(th.int64)
        out = th.ones((len(boxes), self.P), dtype=th.float64)
        for k, (oy, ox, h, w) in enumerate(boxes):
            for p in range(self.P):
                r = int(self.region_of_host[p])
                if r < 0:
                    continue
                if h <= 0 or w <= 0:
                    out[k, p] = 0.0
                    continue
                num = int(S[r, oy + h, ox + w] - S[r, oy, ox + w] - S[r, oy + h, ox] + S[r, oy, ox])
                cov = num / (255.0 * h * w)
                pw = float(self.power_host[p])
                out[k, p] = cov if pw == 1.0 else cov ** pw
        return out


def plan_from_specs(specs, H, W, device=None):
    """[(region spec or None, power)] per prompt, in the order of the weight list -> RegionPlan, or None when no prompt has a region.
    Identical specs share one table."""
    if all(spec is None for spec, _ in specs):
        return None
    tables, masks, region_of = {}, [], []
    for spec, _ in specs:
        if spec is None:
            region_of.append(-1)
            continue
        if spec not in tables:
            tables[spec] = len(masks)
            masks.append(parse_region(spec, H, W))
        region_of.append(tables[spec])
    return RegionPlan(build_sat(masks), region_of, [pw for _, pw in specs], device=device)


def boxes_of(coords, H, W, resized=False):
    """The (oy, ox, h, w) rows of a step's cutouts as the kernels read them from the uploaded table (crop_geometry / resize_table)."""
    if resized:
        return [(oy, ox, h, w) for (ox, oy, w, h, _) in coords]
    return [(oy, ox, max(0, min(size, H - oy)), max(0, min(size, W - ox))) for (ox, oy, size) in coords]
