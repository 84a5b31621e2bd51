"""Float64 reference of region prompts (include/cgd_mi355x.h, cgd_spherical_loss_regions / cgd_directional_loss_regions) and the cases their
tests share.

A region is a uint8 mask of the frame; the coverage of a cutout box (oy, ox, h, w) is the mask's sum over the box divided by 255 h w (0 for an
empty box), summed here pixel by pixel, not through a table.  Prompt p weighs w_eff[cut, b, p] = w[b, p] cov[cut, region_of[p]] ** power[p]
on row cut * B + b (region_of -1: cov = 1); both losses are the plain ones with w_eff for the weight:
    spherical:    loss[r] = c sum_p w_eff 2 asin(min(|e^ - t_p| / 2, 1)) ** 2
    directional:  loss[r] = c sum_p w_eff (1 - cos_p), cos_p as in tests/direction_ref.py (0 when n <= 1e-6)
with c = clip_guidance_scale / cutn.  The gradients are autograd's on these restatements."""
import torch as th

from tests import direction_ref as D

SCALE = D.SCALE
H, W = 24, 40  # the frame of the op-level cases: not square

# (oy, ox, h, w): the whole frame, a single pixel, flush with the right and bottom edges (table row H and column W), wholly outside region 0
# (whose mask is zero over the top-left 8 x 8 pixels), a truncated row with h = 0
BOXES = [(0, 0, H, W), (9, 13, 1, 1), (10, 20, 14, 20), (1, 2, 6, 5), (H, 3, 0, 5)]
OUTSIDE, EMPTY = 3, 4  # indices of the last two


def make_masks(R, kind, seed=0):
    """uint8 (R, H, W): 'gray' uniform random values, 'binary' 0 / 255; region 0 is zero over the top-left 8 x 8 pixels, the pixel of the
    single-pixel box is set."""
    gen = th.Generator().manual_seed(31 * seed + R + (0 if kind == "gray" else 100))
    m = th.randint(0, 256, (R, H, W), generator=gen, dtype=th.int64)
    if kind == "binary":
        m = (m >= 96).long() * 255
    m[0, :8, :8] = 0
    m[:, 9, 13] = 255 if kind == "binary" else 131  # the single-pixel box sees something
    return m.to(th.uint8)


def coverage(masks, region_of, power, boxes):
    """float64 (len(boxes), P): (direct sum of the mask over the box / (255 h w)) ** power, 1 where region_of is -1."""
    out = th.ones((len(boxes), len(region_of)), dtype=th.float64)
    for k, (oy, ox, h, w) in enumerate(boxes):
        for p, r in enumerate(region_of):
            if r < 0:
                continue
            cov = float(masks[r, oy:oy + h, ox:ox + w].double().sum()) / (255.0 * h * w) if h * w > 0 else 0.0
            out[k, p] = cov if float(power[p]) == 1.0 else cov ** float(power[p])
    return out


def effective_weights(w, cov, B):
    """(B, P) weights and (cutn, P) coverage -> float64 (cutn * B, P), row = cut * B + b."""
    cutn = cov.shape[0]
    return (w.double().view(1, B, -1) * cov.view(cutn, 1, -1)).reshape(cutn * B, -1)


def spherical_rows(e, t, weff, cutn, scale=SCALE):
    e, t = e.double(), t.double()
    eh = e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)
    dist = (eh[:, None, :] - t[None, :, :]).norm(dim=-1)
    return (scale / cutn) * (weff * 2 * th.asin((dist / 2).clamp(max=1.0)) ** 2).sum(1)


def directional_rows(e, s, d, weff, cutn, B, scale=SCALE):
    _, cos, n = D.rows(e, s, d, th.ones(B, d.shape[0]), cutn, B, scale)
    return (scale / cutn) * (weff * (1 - cos)).sum(1), n


def spherical(e, t, weff, cutn, scale=SCALE):
    """float64 (loss per row, d sum(loss) / d e)"""
    er = e.detach().double().requires_grad_()
    loss = spherical_rows(er, t, weff, cutn, scale)
    g, = th.autograd.grad(loss.sum(), er)
    return loss.detach(), g


def directional(e, s, d, weff, cutn, B, scale=SCALE):
    """float64 (loss per row, d sum(loss) / d e, n per row)"""
    er = e.detach().double().requires_grad_()
    loss, n = directional_rows(er, s, d, weff, cutn, B, scale)
    g, = th.autograd.grad(loss.sum(), er)
    return loss.detach(), g, n.detach()


# (cutn, B, P, D, R, mask kind, region_of, power): D one element per lane / a power of two / a partly filled last stride / the limit; P 1 and 3;
# B 1 and 2; cutn 1 and 5; R 1 and 2; gray and binary masks; powers 1 and 2.5.  cutn 5 takes BOXES, cutn 1 the box flush with the edges
CASES = [
    (5, 2, 3, 512, 2, "gray", (0, -1, 1), (1.0, 2.5, 2.5)),
    (5, 1, 1, 64, 1, "binary", (0,), (1.0,)),
    (1, 2, 3, 640, 2, "gray", (1, 0, 0), (2.5, 1.0, 2.5)),
    (5, 1, 3, 2048, 2, "binary", (1, 1, 0), (2.5, 1.0, 1.0)),
    (1, 1, 1, 2048, 1, "gray", (0,), (2.5,)),
]


def case_id(c):
    return f"cutn{c[0]}-B{c[1]}-P{c[2]}-D{c[3]}-R{c[4]}-{c[5]}"


def boxes_of(cutn):
    return BOXES[:cutn] if cutn == len(BOXES) else [BOXES[2]] * cutn


def make_case(case, kind="ordinary", seed=0):
    """dict of a case's inputs (float32 e, s, t = d, w from direction_ref.make_case at Bs = 1; masks; boxes) and its float64 coverage and
    effective weights.  The unit rows d serve as spherical targets and as directions."""
    cutn, B, P, Dm, R, mkind, region_of, power = case
    e, s, d, w = D.make_case((cutn, B, 1, P, Dm), kind, seed)
    masks, boxes = make_masks(R, mkind, seed), boxes_of(cutn)
    cov = coverage(masks, region_of, power, boxes)
    return dict(e=e, s=s, d=d, w=w, masks=masks, boxes=boxes, region_of=list(region_of), power=list(power), cov=cov,
                weff=effective_weights(w, cov, B), cutn=cutn, B=B, P=P, D=Dm, R=R)
