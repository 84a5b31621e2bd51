"""Float64 reference of the aesthetic-predictor loss (include/cgd_mi355x.h, cgd_aesthetic_loss) and the cases its tests share.

Per row r = cut * B + b, with e the row of the embeddings and the head (a, beta) stored as D + 1 values:
    e^ = e / max(|e|, 1e-12)      s_r = a . e^ + beta      loss[r] = -c s_r,  c = scale / cutn
    grad[r] = -c (a - (a . e^) e^) / max(|e|, 1e-12)       (a row of exact zeros: s_r = beta and no gradient)
The gradient is written in closed form; tests/test_aesthetic_host.py holds it against torch's float64 autograd of the F.normalize formulation."""
import torch as th

from tests.direction_ref import unit_peak, within  # noqa: F401  (the direction tests' conventions: the literal bound, unit peak)

# (cutn, B, D): the smallest shapes that reach each edge of the kernel's lane + 64 k register layout: ViT-B widths; ViT-L's width, one sample;
# a half-filled last register slot; the largest accepted width; one element in the second slot; one element in all; the headline cut count
SHAPES = [(4, 2, 512), (3, 1, 768), (2, 3, 640), (1, 1, 2048), (5, 2, 65), (2, 2, 1), (16, 1, 1024)]
SCALE = 500.0
KINDS = ("ordinary", "stressed")
SEEDS = {"ordinary": (0,), "stressed": (0, 1, 2)}  # the seeds the GPU tests use


def loss_grad_score(e, head, cutn, B, scale=SCALE):
    """float64 (loss per row (N,), d sum(loss) / d e (N, D), score per row (N,)) of float64 copies of the inputs"""
    e, head = e.detach().double(), head.detach().double().flatten()
    N, D = e.shape
    assert N == cutn * B and head.numel() == D + 1
    a, beta = head[:D], head[D]
    norm = e.norm(dim=1, keepdim=True)
    inv = 1.0 / norm.clamp_min(1e-12)
    eh = e * inv
    dot = eh @ a
    score = dot + beta
    c = scale / cutn
    grad = -c * (a[None, :] - dot[:, None] * eh) * inv
    grad = th.where(norm > 0, grad, th.zeros_like(grad))
    return -c * score, grad, score


STRESS_NORM = (1e-3, 1.0, 1e3)


def make_case(shape, kind="ordinary", seed=0):
    """float32 (e (N, D), head (D + 1,)) of a shape.
      ordinary: embeddings of a trained tower's magnitude (|e| about 10, as CLIP's image embeddings before normalisation), a ~ N(0, 1);
      stressed: row norms 1e-3 / 1 / 1e3 cycled over the rows (seeds 0, 1, 2 together give every row every norm), entries of a of random
                sign with magnitudes 10^u, u uniform in [-2, 2]: four decades.
    beta is chosen from the case's own a . e^: |beta| = 1 + 2 max_r |a . e^_r|, negative on odd seeds.  Every score then has beta's sign and
    |s_r| >= 1 + max |a . e^|: the loss cannot cancel between a . e^ and beta, so the bound of the GPU tests measures the kernel
    (test_aesthetic_host.py checks that a float32 evaluation in another summation order stays within a quarter of it)."""
    cutn, B, D = shape
    N = cutn * B
    gen = th.Generator().manual_seed(1000 * seed + D + 7 * N + (1 if kind == "ordinary" else 2))
    e = th.randn(N, D, generator=gen, dtype=th.float64)
    e = e / e.norm(dim=1, keepdim=True)
    r = th.arange(N)
    if kind == "ordinary":
        length = 10.0 * (0.8 + 0.4 * th.rand(N, generator=gen, dtype=th.float64))
        a = th.randn(D, generator=gen, dtype=th.float64)
    else:
        length = th.tensor(STRESS_NORM, dtype=th.float64)[(r + seed) % 3]
        u = 4.0 * th.rand(D, generator=gen, dtype=th.float64) - 2.0
        a = th.where(th.rand(D, generator=gen) < 0.5, -1.0, 1.0).double() * 10.0 ** u
    e = (e * length[:, None]).float()
    a = a.float()
    dot = (e.double() / e.double().norm(dim=1, keepdim=True)) @ a.double()
    beta = (1.0 + 2.0 * float(dot.abs().max())) * (-1.0 if seed % 2 else 1.0)
    head = th.cat([a, th.tensor([beta], dtype=th.float32)])
    s = loss_grad_score(e, head, cutn, B)[2]
    assert bool((s.abs() >= 1.0 + dot.abs().max() - 1e-3 * abs(beta)).all()), s
    return e, head


def graded_gradient(got, ref, e, head, cutn, scale=SCALE):
    """The gradient as the stressed tests grade it: each row multiplied by |e_r| (it is homogeneous of degree -1 in e) and the tensor brought
    to the unit peak of the reference -> (got, ref, peak of the scaled reference).  At D = 1 the unit sphere is two points and the reference
    gradient is identically zero; there is then no peak to divide by, and both are divided by c max|a| instead, the size of the two terms
    a and (a . e^) e^ that cancel."""
    f = e.double().norm(dim=1)[:, None]
    g, r = got.detach().double().cpu() * f, ref.detach().double().cpu() * f
    peak = float(r.abs().max())
    unit = peak if peak > 0 else abs(scale) / cutn * float(head[:-1].double().abs().max())
    return g / unit, r / unit, peak
