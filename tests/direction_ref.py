"""Float64 reference of the directional CLIP loss (include/cgd_mi355x.h, cgd_directional_loss) and the cases its tests share.

Per row r = cut * B + b, with e the generated image's embedding, s the source image's embedding of the same cutout (row cut * Bs + (0 if Bs == 1
else b)), unit text directions d_p and weights w_bp:
    e^ = e / max(|e|, 1e-12)    s^ = s / max(|s|, 1e-12)    delta = e^ - s^    n = |delta|
    cos_p = delta . d_p / n  if n > 1e-6 else 0            loss[r] = c sum_p w_bp (1 - cos_p),  c = clip_guidance_scale / cutn
The gradient is autograd's on this restatement; a row with n <= 1e-6 has none."""
import torch as th

# (cutn, B, Bs, P, D): shared source; per-sample source; five cuts of one sample; the open_clip head width (a partly dead second register
# slot of the kernel's 64-lane rows); the full register budget
SHAPES = [(3, 2, 1, 2, 512), (2, 3, 3, 1, 1024), (5, 1, 1, 3, 640), (2, 2, 2, 2, 80), (1, 1, 1, 1, 2048)]
SCALE = 1000.0


def source_rows(s, cutn, B):
    """(cutn * Bs, D) -> the (cutn * B, D) source rows the loss pairs with the embedding rows."""
    Bs = s.shape[0] // cutn
    r = th.arange(cutn * B)
    return s[(r // B) * Bs + (0 if Bs == 1 else r % B)]


def rows(e, s, d, w, cutn, B, scale=SCALE):
    """(loss per row, cos (N, P), n (N,)) of float64 copies of the inputs; differentiable in e when e requires grad."""
    e, s, d, w = (t.double() for t in (e, s, d, w))
    eh = e / e.norm(dim=1, keepdim=True).clamp_min(1e-12)
    sr = source_rows(s, cutn, B)
    sh = sr / sr.norm(dim=1, keepdim=True).clamp_min(1e-12)
    delta = eh - sh
    n = delta.norm(dim=1, keepdim=True)
    live = n > 1e-6
    safe = th.where(live, delta, th.ones_like(delta))  # keeps 0 / 0 out of the graph of a row without a direction
    cos = th.where(live, (safe / safe.norm(dim=1, keepdim=True)) @ d.t(), th.zeros((), dtype=th.float64))
    wb = w[th.arange(cutn * B) % B]
    return (scale / cutn) * (wb * (1 - cos)).sum(1), cos, n.squeeze(1)


def loss_and_grad(e, s, d, w, cutn, B, scale=SCALE):
    """float64 (loss per row (N,), d sum(loss) / d e (N, D), n (N,))"""
    er = e.detach().double().requires_grad_()
    loss, _, n = rows(er, s, d, w, cutn, B, scale)
    g, = th.autograd.grad(loss.sum(), er)
    return loss.detach(), g, n.detach()


STRESS_N = (0.05, 1.0, 1.95)
STRESS_E = (1e-3, 1.0, 1e3)


def make_case(shape, kind="ordinary", seed=0):
    """float32 (e, s, d, w) of a shape.  The source rows are unit-normal vectors; e^ is placed at a chosen chord length n from its source row
    (e^ = cos(t) s^ + sin(t) u, u a unit vector orthogonal to s^, n = 2 sin(t / 2)) and scaled to a chosen length:
      ordinary: n uniform in [0.75, 1.35], |e| that of a unit-normal vector;
      stressed: n = 0.05 / 1.0 / 1.95 and |e| = 1e-3 / 1 / 1e3, cycled over the rows (seeds 0, 1, 2 together reach all nine pairs from three rows on).
    Each unit direction d_p leans toward the delta of row p, so that cosines of both signs and sizes occur."""
    cutn, B, Bs, P, D = shape
    N = cutn * B
    gen = th.Generator().manual_seed(1000 * seed + D + 7 * N + (1 if kind == "ordinary" else 2))
    s = th.randn(cutn * Bs, D, generator=gen, dtype=th.float64)
    sh = source_rows(s, cutn, B)
    sh = sh / sh.norm(dim=1, keepdim=True)
    u = th.randn(N, D, generator=gen, dtype=th.float64)
    u = u - (u * sh).sum(1, keepdim=True) * sh
    u = u / u.norm(dim=1, keepdim=True)
    r = th.arange(N)
    if kind == "ordinary":
        n = 0.75 + 0.6 * th.rand(N, generator=gen, dtype=th.float64)
        length = th.randn(N, D, generator=gen, dtype=th.float64).norm(dim=1)
    else:
        n = th.tensor(STRESS_N, dtype=th.float64)[(r + seed) % 3]
        length = th.tensor(STRESS_E, dtype=th.float64)[(r // 3 + r + 2 * seed) % 3]
    t = 2 * th.asin(n / 2)
    eh = th.cos(t)[:, None] * sh + th.sin(t)[:, None] * u
    e = eh * length[:, None]
    delta = eh - sh
    d = th.randn(P, D, generator=gen, dtype=th.float64)
    lean = delta[th.arange(P) % N]
    d = d / d.norm(dim=1, keepdim=True) + th.linspace(0.9, -0.6, P, dtype=th.float64)[:, None] * lean / lean.norm(dim=1, keepdim=True)
    d = d / d.norm(dim=1, keepdim=True)
    w = (0.25 + th.rand(B, P, generator=gen, dtype=th.float64)) * th.where(th.rand(B, P, generator=gen) < 0.3, -1.0, 1.0)
    e, s, d, w = (x.float() for x in (e, s, d, w))
    got = rows(e, s, d, w, cutn, B)[2]
    lo, hi = (0.7, 1.4) if kind == "ordinary" else (0.049, 1.951)
    assert bool(((got >= lo) & (got <= hi)).all()), got
    return e, s, d, w


def degree_scale(e, n):
    """Per-row factor |e_r| n_r: the gradient is homogeneous of degree -1 in both, so a row's gradient times it is O(1) whatever the regime."""
    return (e.double().norm(dim=1) * n.double())[:, None]


def within(got, ref, atol=1e-4, rtol=1e-3):
    """(all inside the literal bound |a - b| <= atol + rtol |ref|, the largest used fraction of it)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    use = (got - ref).abs() / (atol + rtol * ref.abs())
    return bool(th.isfinite(got).all()) and bool((use <= 1).all()), float(use.max()) if use.numel() else 0.0


def unit_peak(*tensors_ref_last):
    """The tensors divided by the peak of the last one (the reference)."""
    p = max(float(tensors_ref_last[-1].abs().max()), 1e-300)
    return [t.detach().double().cpu() / p for t in tensors_ref_last]
