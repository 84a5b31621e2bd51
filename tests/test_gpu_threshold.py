"""GPU tests of dynamic thresholding under DPM-Solver++ sampling (csrc/threshold.hip): the selection against torch.sort (bit for bit: radix
selection on bit patterns is exact), the thresholded update against fp64 torch and against cgd_dpmpp_update where nothing is thresholded,
and whole trajectories of the native sampler against the restatement (tests/threshold_ref.py) on the mini scene of tests/step_checks.py,
spaced 'dpm8', with a replayed tape.

Tolerance on s = min(max(v_k + (v_{k+1} - v_k) frac, floor), cap), given the exact v_k <= v_{k+1}: the device rounds the difference, then
either the product and the sum or, contracted, one fused multiply-add; every intermediate lies in [0, v_{k+1}], so each rounding is at most
2^-24 v_{k+1} and the float64 evaluation from the same two values is met within 2 * 2^-24 v_{k+1} < 2^-22 v_{k+1}."""
import itertools
import math
import os

import pytest
import torch as th

from tests import parity_checks as pc
from tests import step_checks, threshold_ref
from tests.test_gpu_dpm import SHAPES, _assert_all, _compare, _inputs, _mkw, _tensor

pytestmark = pytest.mark.gpu

DEV = pc.DEV
INF = math.inf


@pytest.fixture(scope="module")
def op_rig():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    return L.Context(0, 1), dd.create_gaussian_diffusion(1000, "linear", "dpm50", False), L


# ---- selection, op level -----------------------------------------------------------------------------------------------------------------
def _slice(L):
    return int(L.load().cgd_abs_quantile_slice())


def _rows_on_device(rows, misalign):
    """(B, n) CPU tensor -> a contiguous device tensor with the same bits, starting 4 bytes past a 16-byte boundary when `misalign`"""
    B, n = rows.shape
    flat = th.empty(B * n + 8, device=DEV)
    off = 1 if misalign else 0
    view = flat[off:off + B * n].view(B, n)
    view.view(th.int32).copy_(rows.contiguous().view(th.int32))  # as integers: no float path may touch NaN payloads or denormals
    assert view.data_ptr() % 16 == 4 * off
    return view


def _select(rig, rows, k, frac, floor=0.0, cap=INF, misalign=False):
    ctx, _, L = rig
    B, n = rows.shape
    v = _rows_on_device(rows, misalign)
    out = th.full((B, 3), float("nan"), device=DEV)
    scratch = th.empty(int(ctx.lib.cgd_abs_quantile_scratch_bytes(B, n)), dtype=th.uint8, device=DEV)
    ctx.check(ctx.lib.cgd_op_abs_quantile(ctx.h, v.data_ptr(), B, n, k, frac, floor, cap, out.data_ptr(), scratch.data_ptr(), ctx.stream()))
    th.cuda.synchronize()
    return out.cpu()


def _check_rows(tag, out, rows, k, frac, floor=0.0, cap=INF, skip=()):
    a = th.sort(rows.abs(), dim=1).values
    n = rows.shape[1]
    f32 = float(th.tensor(frac, dtype=th.float32))
    for b in range(rows.shape[0]):
        if b in skip:
            continue
        vk, vk1 = a[b, k], a[b, min(k + 1, n - 1)]
        got = out[b]
        assert got[0].view(th.int32) == vk.view(th.int32), f"{tag} row {b}: v_k {got[0].item()!r} vs {vk.item()!r}"
        assert got[1].view(th.int32) == vk1.view(th.int32), f"{tag} row {b}: v_k+1 {got[1].item()!r} vs {vk1.item()!r}"
        want = min(max(float(vk) + (float(vk1) - float(vk)) * f32, floor), cap)
        err = abs(float(got[2]) - want)
        print(f"{tag} row {b}: v_k {vk.item():.9g} v_k+1 {vk1.item():.9g} s {float(got[2]):.9g} |s - f64| {err:.3g}")
        assert err <= 2.0 ** -22 * float(vk1), f"{tag} row {b}: s {float(got[2])!r} vs {want!r}"


def _data(kind, B, n, seed=0):
    gen = th.Generator().manual_seed(seed + 17 * n + B)
    if kind == "normal":
        return th.randn(B, n, generator=gen)
    if kind == "negative":
        return -th.randn(B, n, generator=gen).abs() - 0.001
    if kind == "equal":
        return th.full((B, n), -0.7321)
    if kind == "two":  # two values from different top-digit bins, split at n // 2
        rows = th.where(th.arange(n) < n // 2, th.tensor(0.004), th.tensor(-300.0)).repeat(B, 1)
        return th.stack([r[th.randperm(n, generator=gen)] for r in rows])
    if kind == "lastdigit":  # 1 + j 2^-23: equal down to the last digit pass (for n <= 256 only that pass separates them)
        base = 1.0 + th.arange(n, dtype=th.float64) * 2.0 ** -23
        return th.stack([base[th.randperm(n, generator=gen)].float() for _ in range(B)])
    if kind == "extremes":  # +-0, denormals, +-3e38
        pool = th.tensor([0.0, -0.0, 1e-45, -1e-45, 3e-39, -7e-40, 3e38, -3e38, 1.1754944e-38, -2.5, 1.0])
        return pool[th.randint(0, len(pool), (B, n), generator=gen)]
    raise KeyError(kind)


def _ranks(tab, n):
    out = {"p0.5": tab.threshold_rank(0.5, n), "p0.995": tab.threshold_rank(0.995, n), "p1": tab.threshold_rank(1.0, n), "k0": (0, 0.25),
           "frac0": (min(n - 1, (n - 1) // 3), 0.0)}
    assert out["p1"] == (n - 1, 0.0)
    return out


def _shapes(L):
    S = _slice(L)
    # (B, n, misaligned): less than one wavefront on the scalar path; two rows; one and several units per thread; a row of three workgroup
    # slices with a ragged last one, on both paths
    return [(1, 105, True), (2, 2880, False), (1, 18432, False), (3, 18435, False), (1, 2 * S + 4, False), (2, 2 * S + 1, False)]


def test_slice_constant_and_scratch_size(op_rig):
    ctx, _, L = op_rig
    S = _slice(L)
    assert S > 0 and S % 4 == 0
    size = ctx.lib.cgd_abs_quantile_scratch_bytes
    assert size(1, S) < size(1, S + 1) and size(1, 2 * S) < size(1, 2 * S + 1) == size(1, 3 * S)  # one more workgroup per started slice
    assert size(3, 2 * S + 1) == 3 * size(1, 2 * S + 1)
    assert size(0, 5) < 0 and size(1, 0) < 0 and size(1, 2 ** 31) < 0


@pytest.mark.parametrize("kind", ["normal", "negative", "equal", "two", "lastdigit", "extremes"])
def test_selection_is_exact(op_rig, kind):
    _, tab, L = op_rig
    for B, n, mis in _shapes(L):
        rows = _data(kind, B, n)
        ranks = _ranks(tab, n)
        if kind == "two":
            ranks["boundary"] = (n // 2 - 1, 0.5)  # v_k is the last small value, v_k+1 the first large one
        for name, (k, frac) in ranks.items():
            out = _select(op_rig, rows, k, frac, misalign=mis)
            _check_rows(f"{kind} ({B},{n}) {name}", out, rows, k, frac)
        if kind == "two":
            k = n // 2 - 1
            out = _select(op_rig, rows, k, 0.5)
            assert out[0, 0].item() == pytest.approx(0.004) and out[0, 1].item() == 300.0


def test_last_digit_only_rows(op_rig):
    """n <= 256 values 1 + j 2^-23: every digit pass but the last sees a single bin"""
    _, tab, _ = op_rig
    rows = _data("lastdigit", 2, 256)
    for name, (k, frac) in _ranks(tab, 256).items():
        _check_rows(f"lastdigit (2,256) {name}", _select(op_rig, rows, k, frac), rows, k, frac)


def test_floor_and_cap_bound_the_scale(op_rig):
    rows = _data("normal", 2, 2880) * 3.0
    k, frac = op_rig[1].threshold_rank(0.995, 2880)
    for floor, cap in ((1.0, INF), (1.0, 1.5), (20.0, 30.0), (1.0, 1.0)):
        out = _select(op_rig, rows, k, frac, floor, cap)
        _check_rows(f"floor {floor} cap {cap}", out, rows, k, frac, floor, cap)
        assert floor <= out[:, 2].min() and out[:, 2].max() <= cap


def test_two_runs_give_identical_bits(op_rig):
    rows = _data("normal", 3, 18435)
    k, frac = op_rig[1].threshold_rank(0.995, 18435)
    a, b = _select(op_rig, rows, k, frac), _select(op_rig, rows, k, frac)
    assert th.equal(a.view(th.int32), b.view(th.int32))


def test_a_row_with_a_nan_leaves_the_other_rows_exact(op_rig):
    _, tab, L = op_rig
    for B, n, mis in ((3, 2880, False), (3, 2 * _slice(L) + 1, False)):
        rows = _data("normal", B, n)
        rows[1, n // 3] = float("nan")
        rows[1, n - 1] = float("inf")
        for k, frac in (tab.threshold_rank(0.995, n), tab.threshold_rank(1.0, n)):
            out = _select(op_rig, rows, k, frac, misalign=mis)  # returns 0 (ctx.check)
            _check_rows(f"nan row ({B},{n}) k{k}", out, rows, k, frac, skip=(1,))


def test_selection_bad_arguments_are_refused(op_rig):
    ctx, _, L = op_rig
    B, n = 2, 640
    v = th.randn(B, n, device=DEV)
    scratch = th.empty(int(ctx.lib.cgd_abs_quantile_scratch_bytes(B, n)), dtype=th.uint8, device=DEV)
    out = th.full((B, 3), float("nan"), device=DEV)

    def call(v=v.data_ptr(), B=B, n=n, k=5, frac=0.5, floor=1.0, cap=INF, out=out.data_ptr(), scratch=scratch.data_ptr()):
        return ctx.lib.cgd_op_abs_quantile(ctx.h, v, B, n, k, frac, floor, cap, out, scratch, ctx.stream())

    bad = [dict(v=None), dict(out=None), dict(scratch=None), dict(B=0), dict(n=0), dict(n=-4), dict(k=-1), dict(k=n), dict(frac=-0.1),
           dict(frac=1.5), dict(frac=float("nan")), dict(floor=2.0, cap=1.0), dict(cap=float("nan"))]
    for kw in bad:
        assert call(**kw) == -2 and ctx.lib.cgd_last_error(ctx.h), kw
    th.cuda.synchronize()
    assert th.isnan(out).all()  # nothing was launched
    assert call() == 0 and call(k=n - 1, frac=1.0) == 0 and call(k=0, frac=0.0, floor=1.0, cap=1.0) == 0
    th.cuda.synchronize()
    assert th.isfinite(out).all()


# ---- thresholded update, op level --------------------------------------------------------------------------------------------------------
P = 0.9


def _ref_thr_update(x, x0, g, fct, noise, hist, k, d, p, cap):
    """fp64 restatement of cgd_dpmpp_threshold + cgd_dpmpp_update_thr with the float32 coefficients the kernels see"""
    dbl = lambda t: None if t is None else t.double().cpu()  # noqa: E731
    x, x0, g, noise, hist = dbl(x), dbl(x0), dbl(g), dbl(noise), dbl(hist)
    a, b, s1 = float(k.sqrt_recip), float(k.sqrt_recipm1), float(k.sqrt_one_minus_ab)
    e = (a * x - x0) / b - s1 * (g * fct if g is not None else 0.0)
    x0c = a * x - b * e
    s = threshold_ref.scales(x0c, p, cap).view(-1, 1, 1, 1)
    x0t = th.maximum(th.minimum(x0c, s), -s) / s
    dd_ = x0t + float(d.c_r) * (x0t - hist) if d.c_r != 0 else x0t
    if not k.nonzero:
        return (x0t, x0t, x0), x0c, s.flatten()
    smp = float(d.c_x) * x + float(d.c_d) * dd_
    if d.c_n != 0:
        smp = smp + float(d.c_n) * noise
    return (smp, x0t, x0), x0c, s.flatten()


def _launch_thr(rig, shape, inputs, t, order, eta, p, cap, outputs=(True, True), arena=None):
    ctx, tab, L = rig
    x, x0, g, scal, noise, hist = inputs
    B, _, H, W = shape
    k, d = tab.step_coef(t, 3), tab.dpmpp_coef(t, order, eta)
    n = 3 * H * W
    rank, frac = tab.threshold_rank(p, n)
    raw = _tensor(shape, fill=float("nan"))
    thr3 = th.full((B, 3), float("nan"), device=DEV)
    scratch = th.empty(int(ctx.lib.cgd_abs_quantile_scratch_bytes(B, n)), dtype=th.uint8, device=DEV) if cap > 1.0 else None
    if arena is None:
        sample = _tensor(shape, fill=float("nan"))
        x0c_out = _tensor(shape, fill=float("nan")) if outputs[0] else None
        x0_out = _tensor(shape, fill=float("nan")) if outputs[1] else None
    else:
        sample, x0c_out, x0_out = arena
    ctx.check(ctx.lib.cgd_dpmpp_threshold(ctx.h, x.data_ptr(), x0.data_ptr(), L.ptr(g), L.ptr(scal), raw.data_ptr(), B, H, W, k, rank, frac,
                                          1.0, cap, thr3.data_ptr(), L.ptr(scratch), ctx.stream()))
    # unused inputs are not passed at all: a launch that read them would fault on NULL, not pass by luck
    ctx.check(ctx.lib.cgd_dpmpp_update_thr(ctx.h, x.data_ptr(), x0.data_ptr(), raw.data_ptr(), thr3.data_ptr(),
                                           noise.data_ptr() if d.c_n and t else None, hist.data_ptr() if d.c_r else None, L.ptr(x0c_out),
                                           sample.data_ptr(), L.ptr(x0_out), B, H, W, k, d, ctx.stream()))
    th.cuda.synchronize()
    return (sample, x0c_out, x0_out), raw, thr3, (k, d)


@pytest.mark.parametrize("name", list(SHAPES))
def test_thresholded_update_matches_fp64(op_rig, name):
    shape = SHAPES[name]
    recs = []
    for t, order, eta, (with_g, with_scal) in itertools.product((20, 0), (1, 2), (0.0, 1.0), ((False, False), (True, False), (True, True))):
        inputs = _inputs(shape, 1000 * t + 100 * order + int(10 * eta) + with_g + 2 * with_scal, with_g, with_scal)
        for cap in (INF, 1.5, 1.0):
            outs, raw, thr3, (k, d) = _launch_thr(op_rig, shape, inputs, t, order, eta, P, cap)
            ref, x0c_ref, s_ref = _ref_thr_update(*inputs[:2], inputs[2], 0.37 if with_scal else 1.0, inputs[4], inputs[5], k, d, P, cap)
            # the inputs are standard normal: the guided prediction leaves [-s, s] in every sample, and s > 1 unless capped
            assert (x0c_ref.abs().flatten(1).max(dim=1).values > s_ref).all() and (s_ref > 1.0).all() == (cap > 1.0)
            tag = f"thr {name} t{t} order{order} eta{eta:g} g{int(with_g)} clamp{int(with_scal)} cap{cap:g}"
            assert th.isfinite(raw).all() and th.isfinite(thr3).all()
            recs.append(pc.rec(f"{tag} x0c buffer", raw, x0c_ref))
            recs.append(pc.rec(f"{tag} s", thr3[:, 2], s_ref))
            for what, got, want in zip(("sample", "x0c_out", "pred_xstart"), outs, ref):
                assert th.isfinite(got).all(), f"{tag} {what}: an element was not written"
                recs.append(pc.rec(f"{tag} {what}", got, want))
            assert th.equal(outs[2].cpu(), ref[2].float())  # a copy, bit for bit
            # the scale on the device is the selection's on the buffer's own bits, and x0c_out is the clamp and the division in float32
            a = th.sort(raw.cpu().abs().flatten(1), dim=1).values
            rank, frac = op_rig[1].threshold_rank(P, a.shape[1])
            if cap > 1.0:
                assert th.equal(thr3[:, 0].cpu(), a[:, rank]) and th.equal(thr3[:, 1].cpu(), a[:, min(rank + 1, a.shape[1] - 1)])
            s = thr3[:, 2].cpu().view(-1, 1, 1, 1)
            assert th.equal(outs[1].cpu(), th.maximum(th.minimum(raw.cpu(), s), -s) / s)
            assert float(outs[1].abs().max()) <= 1.0
    _assert_all(recs)


@pytest.mark.parametrize("name", list(SHAPES))
def test_outputs_that_are_not_asked_for_are_not_written(op_rig, name):
    """one NaN arena holds the three outputs with guard floats between them: every element of a passed output is written, the arena around
    them and the slot of an omitted output stay NaN"""
    shape = SHAPES[name]
    n = math.prod(shape)
    step = n + 8  # 32 guard bytes: keeps the 16-byte alignment class of the first slot
    off = 1 if name == "odd" else 0
    inputs = _inputs(shape, 7, True, False)
    for passed in ((True, True), (True, False), (False, True), (False, False)):
        arena = th.full((3 * step + 8,), float("nan"), device=DEV)
        slots = [arena[4 + off + j * step:4 + off + j * step + n].view(shape) for j in range(3)]
        _launch_thr(op_rig, shape, inputs, 20, 2, 1.0, P, INF, arena=(slots[0], slots[1] if passed[0] else None, slots[2] if passed[1] else None))
        written = th.isfinite(arena)
        expect = th.zeros_like(written)
        for j, on in enumerate((True,) + passed):
            if on:
                expect[4 + off + j * step:4 + off + j * step + n] = True
        assert th.equal(written, expect), passed


@pytest.mark.parametrize("name", list(SHAPES))
def test_inside_the_range_it_is_the_plain_update(op_rig, name):
    """inputs for which every |x0c| <= 1: s = 1, the clamp and the division change nothing"""
    ctx, tab, L = op_rig
    shape = SHAPES[name]
    recs = []
    for t, order, eta, (with_g, with_scal) in itertools.product((20, 0), (1, 2), (0.0, 1.0), ((False, False), (True, True))):
        x, x0, g, scal, noise, hist = _inputs(shape, 31 + t + order, with_g, with_scal)
        k, d = tab.step_coef(t, 3), tab.dpmpp_coef(t, order, eta)
        # x0c = pred_xstart + sqrt_recipm1 sqrt(1 - abar) fct g: small inputs keep it inside
        for buf in (x, x0, g, hist):
            if buf is not None:
                buf.mul_(0.2)
        outs, raw, thr3, _ = _launch_thr(op_rig, shape, (x, x0, g, scal, noise, hist), t, order, eta, 0.995, INF)
        assert float(raw.abs().max()) <= 1.0 and th.equal(thr3[:, 2].cpu(), th.ones(shape[0]))
        plain = [_tensor(shape, fill=float("nan")) for _ in range(3)]
        ctx.check(ctx.lib.cgd_dpmpp_update(ctx.h, x.data_ptr(), x0.data_ptr(), L.ptr(g), L.ptr(scal), noise.data_ptr() if d.c_n and t else None,
                                           hist.data_ptr() if d.c_r else None, plain[1].data_ptr(), plain[0].data_ptr(), plain[2].data_ptr(),
                                           shape[0], shape[2], shape[3], k, d, ctx.stream()))
        th.cuda.synchronize()
        tag = f"inside {name} t{t} order{order} eta{eta:g} g{int(with_g)}"
        assert th.equal(outs[1], plain[1]) and th.equal(raw, plain[1]), f"{tag}: x0c_out"
        assert th.equal(outs[2], plain[2])
        if t == 0:
            assert th.equal(outs[0], plain[0]), f"{tag}: sample"
        else:  # two kernels may contract the affine update differently
            recs.append(pc.rec(f"{tag} sample", outs[0], plain[0]))
    _assert_all(recs)


def test_update_bad_arguments_are_refused(op_rig):
    ctx, tab, L = op_rig
    B, H, W = 1, 8, 8
    n = 3 * H * W
    bufs = [th.zeros(B, 3, H, W, device=DEV) for _ in range(8)]
    x, x0, g, noise, hist, x0c_out, sample, x0o = (b.data_ptr() for b in bufs)
    raw_t, thr_t = th.full((B, 3, H, W), float("nan"), device=DEV), th.full((B, 3), float("nan"), device=DEV)
    raw, thr3 = raw_t.data_ptr(), thr_t.data_ptr()
    scratch = th.empty(int(ctx.lib.cgd_abs_quantile_scratch_bytes(B, n)), dtype=th.uint8, device=DEV).data_ptr()
    k1, k0 = tab.step_coef(5), tab.step_coef(0)
    ode, sde = tab.dpmpp_coef(5, 2, 0.0), tab.dpmpp_coef(5, 1, 1.0)

    def select(x=x, x0=x0, g=g, raw=raw, B=B, H=H, W=W, k=7, frac=0.5, floor=1.0, cap=INF, thr3=thr3, scratch=scratch):
        return ctx.lib.cgd_dpmpp_threshold(ctx.h, x, x0, g, None, raw, B, H, W, k1, k, frac, floor, cap, thr3, scratch, ctx.stream())

    bad = [dict(x=None), dict(x0=None), dict(raw=None), dict(thr3=None), dict(scratch=None), dict(B=0), dict(H=0), dict(W=-1), dict(k=-1),
           dict(k=n), dict(frac=-0.5), dict(frac=1.01), dict(floor=1.0, cap=0.5), dict(raw=x), dict(raw=x0), dict(raw=g)]
    for kw in bad:
        assert select(**kw) == -2 and ctx.lib.cgd_last_error(ctx.h), kw
    th.cuda.synchronize()
    assert th.isnan(raw_t).all() and th.isnan(thr_t).all()  # nothing was launched
    assert select() == 0 and select(g=None) == 0 and select(cap=1.0, scratch=None) == 0  # the static clip needs no scratch
    th.cuda.synchronize()
    assert th.equal(thr_t[:, 2].cpu(), th.ones(B)) and th.isfinite(raw_t).all()

    out_t = [th.full((B, 3, H, W), float("nan"), device=DEV) for _ in range(3)]
    sample, x0c_out, x0o = (o.data_ptr() for o in out_t)

    def update(x=x, x0=x0, raw=raw, thr3=thr3, noise=noise, hist=hist, x0c_out=x0c_out, sample=sample, x0o=x0o, B=B, H=H, W=W, k=k1, d=ode):
        return ctx.lib.cgd_dpmpp_update_thr(ctx.h, x, x0, raw, thr3, noise, hist, x0c_out, sample, x0o, B, H, W, k, d, ctx.stream())

    bad = [dict(x=None), dict(x0=None), dict(sample=None), dict(raw=None), dict(thr3=None),  # a missing required buffer
           dict(hist=None), dict(d=sde, noise=None),  # c_r != 0 without the history, c_n != 0 at t != 0 without the noise
           dict(B=0), dict(H=0), dict(W=-1),  # non-positive sizes
           dict(sample=x), dict(x0c_out=x), dict(x0o=x), dict(x0c_out=sample), dict(x0o=sample), dict(x0o=x0c_out),  # aliasing outputs
           dict(sample=raw), dict(x0c_out=raw), dict(x0o=raw)]  # an output on the x0c buffer
    for kw in bad:
        assert update(**kw) == -2 and ctx.lib.cgd_last_error(ctx.h), kw
    th.cuda.synchronize()
    assert all(th.isnan(o).all() for o in out_t)  # nothing was launched
    assert update() == 0 and update(d=sde) == 0 and update(x0c_out=None, x0o=None) == 0
    assert update(d=sde, noise=None, k=k0) == 0  # at t == 0 nothing reads the noise
    th.cuda.synchronize()
    assert all(th.isfinite(o).all() for o in out_t)


# ---- trajectories ------------------------------------------------------------------------------------------------------------------------
SPEC, STEPS = "dpm8", 5
# The scene, chosen on the CPU restatement alone (asserted on the reference in _assert_the_scene_thresholds).  On the mini scene as
# tests/test_gpu_dpm.py runs it, s > 1 on every step whatever the guidance scale: the state carries the first step's excursion down the
# schedule (x0c' ~ 1/4 x0c + 3/4 D per step), so s - 1 shrinks by about 4 per step and never reaches 0.  Here the start noise and the
# step noise are a tenth of a standard normal and the UNet's eps head is a fifth of the scene's: the first step's guidance shift (the
# scene's own clip_guidance_scale, times (1 - abar) / abar = 6.3 at that level) takes the 0.995-quantile of |x0c| to 7.4, and from the
# second step on fewer than 0.5 % of the values leave [-1, 1] (max |x0c| 1.2 .. 1.007: they are still clamped) and s = 1.
NOISE_SCALE, HEAD_SCALE = 0.1, 0.02


@pytest.fixture(scope="module")
def scene():
    """the mini scene of tests/step_checks.py re-spaced to 'dpm8' as in tests/test_gpu_dpm.py, with a smaller noise and eps head (above)"""
    from cgd_amd import diffusion as dd
    from oracle import guidance as og
    sc = step_checks.Scenario("mini", ddim=True, steps=STEPS, head_scale=HEAD_SCALE)
    N = dd.create_gaussian_diffusion(1000, sc.schedule, SPEC).num_timesteps
    assert N == 8
    sc.spec, sc.N, sc.t_first = SPEC, N, STEPS - 1
    sc.skip, sc.counter0 = N - STEPS, STEPS - 1
    sc.tape["x_T"] = NOISE_SCALE * sc.tape["x_T"]
    sc.tape["noise"] = [NOISE_SCALE * v for v in sc.tape["noise"]]
    gen = th.Generator().manual_seed(4321)
    sc.tape["coords"] = [og.generate_coords(sc.H, sc.W, sc.cutn, sc.res, 1.0, generator=gen) for _ in range(STEPS)]
    sc.tape["known_noise"] = [th.randn(sc.B, 3, sc.H, sc.W, generator=gen) for _ in range(STEPS)]
    sc.mask = th.zeros(1, 1, sc.H, sc.W)
    sc.mask[..., : sc.W // 2] = 1.0
    sc.cache = {}
    return sc


def _oracle(sc, order, eta, threshold, mask=None):
    """-> (records, the reference's scales per step); computed once per case and shared"""
    key = (order, eta, threshold, mask is not None)
    if key in sc.cache:
        return sc.cache[key]
    og = sc.og
    diff = threshold_ref.create_threshold_diffusion(1000, sc.schedule, sc.spec, sc.rescale, threshold=threshold)
    cgs, tvs, rs = sc.scales
    cond, st = og.make_cond_fn(diffusion=diff, clip_model=sc.ref_clip, make_cutouts=og.MakeCutouts(sc.res, sc.cutn),
                               target_embeds=sc.targets, weights=sc.w, num_cutouts=sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                               range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude, coords_tape=sc.tape["coords"])
    mkw = _mkw(sc, "cpu")
    gen = diff.dpmpp_sample_loop_progressive(sc.ref_unet, (sc.B, 3, sc.H, sc.W), clip_denoised=False, cond_fn=cond, model_kwargs=dict(mkw),
                                             skip_timesteps=sc.skip, init_image=sc.x0_star.expand(sc.B, -1, -1, -1),
                                             randomize_class=bool(mkw), order=order, eta=eta, tape=sc.tape, mask=mask)
    st["current_timestep"] = sc.counter0
    out = []
    for o in gen:
        st["current_timestep"] -= 1
        out.append((o["sample"].clone(), o["pred_xstart"].clone(), dict(st.get("log", {}))))
    sc.cache[key] = (out, diff.seen_scales, diff.seen_excess)
    return sc.cache[key]


def _device(sc, order, eta, threshold, mask=None):
    from cgd_amd import diffusion as dd
    from cgd_amd import guidance as dg
    from cgd_amd import lib, nets, sampler
    ctx = lib.Context(0, 1)
    unet = nets.UNet(ctx, **sc.kw)
    unet.load_state_dict({k: v.to(DEV) for k, v in sc.ref_unet.state_dict().items()})
    clip = nets.ClipImageTower(ctx, config=sc.vit_cfg)
    clip.load_clip_state_dict({k: v.to(DEV) for k, v in sc.ref_clip.state_dict().items()})
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, sc.schedule, sc.spec, sc.rescale))
    smp.tape = sc.tape
    cgs, tvs, rs = sc.scales
    cond = dg.ClipGuidance(ctx, unet, clip, smp, sc.targets.to(DEV), sc.w, sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                           range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude)
    cond.coords_tape = sc.tape["coords"]
    cond.current_timestep = sc.counter0
    mkw = _mkw(sc, DEV)
    gen = smp.dpmpp_sample_loop_progressive(unet, (sc.B, 3, sc.H, sc.W), clip_denoised=False, cond_fn=cond, model_kwargs=mkw, device=DEV,
                                            skip_timesteps=sc.skip, init_image=sc.x0_star.expand(sc.B, -1, -1, -1).to(DEV),
                                            randomize_class=bool(mkw), cond_fn_with_grad=True, order=order, eta=eta,
                                            **({} if threshold is None else {"threshold": threshold}),
                                            **({} if mask is None else {"mask": mask.to(DEV)}))
    out = []
    for o in gen:
        th.cuda.synchronize()
        out.append((o["sample"].cpu(), o["pred_xstart"].cpu(), cond.log()))
        cond.current_timestep -= 1
    assert cond.calls == STEPS, "one cond_fn call per step"
    return out


def _assert_the_scene_thresholds(scales, excess, capped=False):
    """on the reference: every sample has s > 1 on at least one step and s = 1 on at least one (capped at 1: the prediction leaves
    [-1, 1] on at least one step)"""
    s = th.stack(scales)  # (steps, B)
    print("reference scales per step:", [[round(float(v), 4) for v in row] for row in s],
          "max |x0c|:", [[round(float(v), 3) for v in row] for row in th.stack(excess)])
    if capped:
        assert (s == 1.0).all() and (th.stack(excess) > 1.0).any(dim=0).all()
    else:
        assert (s > 1.0).any(dim=0).all() and (s == 1.0).any(dim=0).all()


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_trajectory_order2_native_guidance_thresholded(scene, eta):
    o_out, scales, excess = _oracle(scene, 2, eta, 0.995)
    _assert_the_scene_thresholds(scales, excess)
    _assert_all(_compare(f"dpmpp 2M thr eta {eta:g} mini", _device(scene, 2, eta, 0.995), o_out))


def test_trajectory_thresholded_differs_from_the_unthresholded_one(scene):
    """the test that fails without the feature: thresholding moves the trajectory by far more than the tolerance, on the reference and
    on the device alike"""
    o_thr, scales, excess = _oracle(scene, 2, 0.0, 0.995)
    o_plain, _, _ = _oracle(scene, 2, 0.0, None)
    _assert_the_scene_thresholds(scales, excess)
    d_thr, d_plain = _device(scene, 2, 0.0, 0.995), _device(scene, 2, 0.0, None)
    _assert_all(_compare("dpmpp 2M plain mini (large scale)", d_plain, o_plain))
    for a, b in ((o_thr, o_plain), (d_thr, d_plain)):
        diff = (a[-1][0] - b[-1][0]).abs()
        print(f"last sample, thresholded vs not: max |diff| {float(diff.max()):.4f}")
        assert float(diff.max()) > 100 * (pc.ATOL + pc.RTOL * float(b[-1][0].abs().max()))
        assert not pc.rec("thr vs plain", a[-1][0], b[-1][0])["ok"]


def test_trajectory_thresholded_under_a_half_image_mask(scene):
    o_out, scales, excess = _oracle(scene, 2, 0.0, 0.995, mask=scene.mask)
    _assert_the_scene_thresholds(scales, excess)
    d_out = _device(scene, 2, 0.0, 0.995, mask=scene.mask)
    _assert_all(_compare("dpmpp 2M thr masked mini", d_out, o_out))
    keep = scene.W // 2
    init = scene.x0_star.expand(scene.B, -1, -1, -1)
    assert th.equal(d_out[-1][0][..., keep:], init[..., keep:]) and th.equal(d_out[-1][1][..., keep:], init[..., keep:])


def test_trajectory_static_clip(scene):
    o_out, scales, excess = _oracle(scene, 2, 0.0, (0.995, 1.0))
    _assert_the_scene_thresholds(scales, excess, capped=True)
    d_out = _device(scene, 2, 0.0, (0.995, 1.0))
    _assert_all(_compare("dpmpp 2M static clip mini", d_out, o_out))
    assert float(d_out[-1][0].abs().max()) <= 1.0  # the last sample is a clipped prediction


def test_dropin_generator_thresholded_synthetic_weights(tmp_path, monkeypatch):
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion
    from cgd_amd import diffusion as dd
    from cgd_amd import sampler
    levels = dd.create_gaussian_diffusion(1000, "linear", "dpm8").num_timesteps
    seen = []
    plain = sampler.GuidedSampler.dpmpp_sample_loop_progressive

    def recording(self, *a, **kw):
        seen.append((kw.get("order"), kw.get("eta"), kw.get("threshold"), self.num_timesteps, []))
        for out in plain(self, *a, **kw):
            seen[-1][4].append(out["sample"].detach().clone())
            yield out

    monkeypatch.setattr(sampler.GuidedSampler, "dpmpp_sample_loop_progressive", recording)
    kw = dict(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=2, seed=7, prefix_path=str(tmp_path / "out"),
              checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=False, device="cuda")
    items = list(clip_guided_diffusion(timestep_respacing="dpm8+thr=0.995", **kw))
    assert len(items) == levels and all(os.path.isfile(p) for _, p in items)
    assert [s[:4] for s in seen] == [(2, 0.0, 0.995, levels)] and len(seen[0][4]) == levels
    assert all(th.isfinite(s).all() for s in seen[0][4])
    with pytest.raises(ValueError, match="dpmN"):
        list(clip_guided_diffusion(timestep_respacing="ddim8+thr=0.995", **kw))
