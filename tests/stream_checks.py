"""Every entry on a CREATED stream, behind pending work (tests/test_gpu_streams.py).

Every other GPU test runs on torch's default stream, which on ROCm is the legacy null stream: it orders with itself, and the tests
synchronise the device before they compare.  A launch, memset or copy that passes 0 instead of the caller's stream, a wrapper that takes the
stream of the wrong device, a warm-path synchronisation or pageable copy are all invisible there.  PyTorch creates its streams non-blocking,
so on a `th.cuda.Stream()` each of them is a race or a stall.

`behind_delay(fn, inputs, warm=...)` makes the race deterministic:
  control  on the default stream, device-synchronised before and after: ref = fn(*inputs), outputs cloned;
  trial    on a fresh th.cuda.Stream() s, inside th.cuda.stream(s): staging copies of every input filled with POISON (NaN; integer operands
           another valid value), a DELAY (torch.cuda._sleep) on s, staging.copy_(input) for every input (device to device: the true values
           arrive only after the delay), an event `armed`, fn(*staging), `early = not armed.query()` on the host, and then s.synchronize(),
           the only synchronisation of the trial.
Verdicts: every output th.equal to the control (same kernels in the same order; the suite already asserts bit-identical reruns of them),
every input unchanged (unless the case names it as an in / out operand), and with warm=True `early`: the call returned to the host while the
delay was still running.  A launch on the null stream reads poison, or is overwritten by the NaN pre-fill queued behind the delay.

Outputs start as NaN: while a control or a trial runs, `th.empty` / `th.empty_like` (what the wrappers in cgd_amd.ops / cgd_amd.nets
allocate outputs with) hand out NaN-filled floating-point tensors, filled on the current stream — in the trial, behind the delay.

The delay is 5 x the largest host time of any case's control call (perf_counter around fn, no synchronisation), at least 20 ms: `prepare()`
builds every case, runs its warm-up and control once and only then fixes the delay, so the test module calls it from one fixture and every
test runs a trial only.  The `_sleep` count is calibrated once per session with events.
"""
import contextlib
import ctypes as C
import math
import time
import traceback

import torch as th

from tests import lifecycle_checks as lc
from tests import parity_checks as pc
from tests.parity_checks import DEV, _flag, g, rec, rec_flips

NAN = float("nan")
MIN_DELAY_MS = 20.0  # below this a scheduling hiccup of the host could pass for a synchronisation
DELAY_FACTOR = 5.0

# Python wrappers that block the host on every call because they read or upload host data; their raw C entry with device operands is
# what the cases call, and that call is asserted `early`.  No warm C entry is on this table.
SYNCS_BY_DESIGN = {
    "nets.ClipTextTower.encode_text": ("clip-guided-diffusion_amd/nets.py:424", "int(tokens.min()), int(tokens.max()): the token ids are "
                                       "range-checked on the host before the launch; raw entry: cgd_text_forward"),
    "lifecycle_checks.*Call.forward / dgrad": ("tests/lifecycle_checks.py:129", "the calls keep their inputs on the CPU and upload them per call "
                                               "(pageable copy); the cases hand device copies to the nets.* wrappers instead"),
    "test_gpu_resize_cutouts.table_of": ("tests/test_gpu_resize_cutouts.py:73", "th.tensor(..., device=) uploads the tap table per call; the "
                                         "cases stage the table on the device; raw entries: cgd_cutouts_resize_fwd / _bwd"),
}

_STATE = {}


# ---- the delay ---------------------------------------------------------------------------------------------------------------------------
def cycles_per_ms():
    """torch.cuda._sleep counts per millisecond, measured once with events (the count is doubled until one sleep lasts at least 5 ms)."""
    if "cpm" not in _STATE:
        th.cuda._sleep(1000)
        th.cuda.synchronize()
        n, ms = 1_000_000, 0.0
        for _ in range(12):
            a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
            a.record()
            th.cuda._sleep(n)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0:
                break
            n *= 2
        assert ms >= 5.0, f"torch.cuda._sleep({n}) lasted {ms:.3f} ms: no usable delay on this machine"
        _STATE["cpm"], _STATE["calibration"] = n / ms, (n, ms)
    return _STATE["cpm"]


def delay_ms():
    return _STATE.get("delay_ms", MIN_DELAY_MS)


def enqueue_delay(ms=None):
    """a delay of `ms` (default: the session's) on the current stream"""
    th.cuda._sleep(int((delay_ms() if ms is None else ms) * cycles_per_ms()))


@contextlib.contextmanager
def nan_outputs():
    """th.empty / th.empty_like give NaN-filled floating-point GPU tensors (filled on the current stream): an output no launch wrote, or one
    written before its turn, does not compare equal"""
    empty, empty_like = th.empty, th.empty_like

    def _fill(t):
        if t.is_cuda and t.is_floating_point():
            t.fill_(NAN)
        return t

    th.empty, th.empty_like = (lambda *a, **k: _fill(empty(*a, **k))), (lambda *a, **k: _fill(empty_like(*a, **k)))
    try:
        yield
    finally:
        th.empty, th.empty_like = empty, empty_like


def poison_like(t):
    """NaN for floating-point operands; for integer operands another VALID value in every element (0, or 1 where the value is 0): a
    premature read gives a different result, never an out-of-range access"""
    if t.is_floating_point():
        return th.full_like(t, NAN)
    p = th.zeros_like(t)
    p[t == 0] = 1
    return p


def _tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def control(fn, inputs):
    """ref = fn(*inputs) on the default stream, device-synchronised before and after -> (outputs cloned, host milliseconds of the call)"""
    th.cuda.synchronize()
    with nan_outputs():
        t0 = time.perf_counter()
        out = fn(*inputs)
        host = (time.perf_counter() - t0) * 1e3
    th.cuda.synchronize()
    return tuple(o.clone() for o in _tuple(out)), host


class Verdict:
    """what one trial showed: `equal` per output, `inputs_unchanged` per input, `early`, the host time of fn and the delay as it ran"""

    def __init__(self, name, warm):
        self.name, self.warm = name, warm
        self.equal, self.inputs_unchanged, self.early, self.host_ms, self.delay_ran_ms, self.outs = [], [], None, 0.0, 0.0, ()

    def problems(self):
        bad = [f"output {k} differs from the control (NaN in it: {nan})" for k, (eq, nan) in enumerate(self.equal) if not eq]
        bad += [f"input {k} was modified" for k, same in enumerate(self.inputs_unchanged) if not same]
        if not self.equal:
            bad.append("no output")
        if self.warm and not self.early:
            bad.append(f"the call did not return while the delay was running (fn blocked the host for {self.host_ms:.2f} ms of a "
                       f"{self.delay_ran_ms:.1f} ms delay)")
        return bad

    def records(self):
        tag = f"streams: {self.name}"
        recs = [_flag(f"{tag} output {k} bit-equal to the control", eq) for k, (eq, _) in enumerate(self.equal)]
        recs += [_flag(f"{tag} input {k} unchanged", same) for k, same in enumerate(self.inputs_unchanged)]
        if self.warm:
            recs.append(_flag(f"{tag} returned early (host {self.host_ms:.2f} ms, delay {self.delay_ran_ms:.1f} ms)", bool(self.early)))
        return recs or [_flag(f"{tag} produced an output", False)]


def behind_delay(fn, inputs, *, warm, ref=None, poison=None, inout=(), name="", control_fn=None):
    """The harness (module docstring).  ref: the control's outputs when the caller already has them; poison: {input index: tensor} for
    operands whose poison the case chooses (box tables); inout: indices of inputs the entry documents as in / out operands."""
    inputs = list(inputs)
    if ref is None:
        ref, _ = control(control_fn or fn, inputs)
    v = Verdict(name, warm)
    s = th.cuda.Stream()
    t0e, t1e = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    with th.cuda.stream(s), nan_outputs():
        staging = [(poison[k].clone() if poison and k in poison else poison_like(t)) for k, t in enumerate(inputs)]
        t0e.record(s)
        enqueue_delay()
        t1e.record(s)
        for st, t in zip(staging, inputs):
            st.copy_(t)
        armed = th.cuda.Event()
        armed.record(s)
        t0 = time.perf_counter()
        out = fn(*staging)
        v.host_ms = (time.perf_counter() - t0) * 1e3
        v.early = not armed.query()
        s.synchronize()  # the only synchronisation of the trial
    v.outs = _tuple(out)
    v.delay_ran_ms = t0e.elapsed_time(t1e)
    assert len(v.outs) == len(ref), f"{name}: {len(v.outs)} outputs, the control has {len(ref)}"
    v.equal = [(bool(th.equal(o, r)), bool(th.isnan(o).any()) if o.is_floating_point() else False) for o, r in zip(v.outs, ref)]
    v.inputs_unchanged = [k in inout or bool(th.equal(st, t)) for k, (st, t) in enumerate(zip(staging, inputs))]
    return v


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, build, warm):
        self.name, self.build, self.warm = name, build, warm
        self.error = self.ref = self.spec = None
        self.host_ms = 0.0


CASES = {}


def case(name, warm=True):
    """registers `build() -> dict(fn=, inputs=[device tensors], poison=, inout=, grade=, control_fn=, keep=)` under `name`"""
    def deco(build):
        assert name not in CASES, name
        CASES[name] = Case(name, build, warm)
        return build
    return deco


def prepare():
    """Once per session: calibrates the delay counter, builds every case, runs its untimed warm-up call and its control (host time taken),
    fixes the delay at 5 x the largest host time (at least 20 ms) and runs the premise trial (a pure-torch call must return early: the fixture asserts it)."""
    if _STATE.get("prepared"):
        return _STATE
    cycles_per_ms()
    for c in CASES.values():
        try:
            c.spec = c.build()
            c.spec.setdefault("control_fn", None)
            fn = c.spec["control_fn"] or c.spec["fn"]
            if c.warm:
                with nan_outputs():
                    fn(*c.spec["inputs"])  # the untimed first call: allocations, packing
            c.ref, c.host_ms = control(fn, c.spec["inputs"])
        except Exception:  # shown by the case's own test
            c.error = traceback.format_exc()
    host = max([c.host_ms for c in CASES.values() if c.error is None] or [0.0])
    _STATE["largest_host_ms"] = host
    _STATE["delay_ms"] = max(MIN_DELAY_MS, DELAY_FACTOR * host)
    a = th.randn(1000, generator=g(1)).to(DEV)
    th.cuda.synchronize()
    v = behind_delay(lambda t: t * 2, [a], warm=True, name="premise")
    _STATE["premise"] = v
    _STATE["prepared"] = True
    return _STATE


def report():
    """the measured host times and the chosen delay, for the log"""
    n, ms = _STATE["calibration"]
    lines = [f"_sleep({n}) = {ms:.2f} ms; largest control host time {_STATE['largest_host_ms']:.3f} ms; delay {_STATE['delay_ms']:.1f} ms"]
    lines += [f"  {c.name}: control host {c.host_ms:.3f} ms" + ("" if c.warm else " (warm=False)") + (" BUILD FAILED" if c.error else "")
              for c in CASES.values()]
    return "\n".join(lines)


def run_case(name):
    """one trial of a prepared case -> records"""
    prepare()
    c = CASES[name]
    if c.error:
        raise AssertionError(f"{name}: building the case or its control failed\n{c.error}")
    sp = c.spec
    if sp.get("before_trial"):
        sp["before_trial"]()
        th.cuda.synchronize()
    v = behind_delay(sp["fn"], sp["inputs"], warm=c.warm, ref=c.ref, poison=sp.get("poison"), inout=sp.get("inout", ()), name=name)
    recs = v.records()
    if sp.get("grade"):
        recs += sp["grade"](v.outs)
    return recs


def _dev(*ts):
    out = [None if t is None else t.to(DEV) for t in ts]
    th.cuda.synchronize()
    return out


_CTX = {}


def ctx_of(precision=1, **envd):
    """one context per (precision, environment) for the op-level cases"""
    key = (precision, tuple(sorted(envd.items())))
    if key not in _CTX:
        from tests.value_regime_checks import env
        with env(**envd):
            _CTX[key] = pc._ctx(precision)
    return _CTX[key]


# ---- op level: cgd_op_gemm ------------------------------------------------------------------------------------------------------------------
def _gemm_operands(M, N, K, seed=0):
    return _dev(th.randn(M, K, generator=g(1 + seed)), th.randn(N, K, generator=g(2 + seed)), 0.3 * th.randn(N, generator=g(3 + seed)),
                0.3 * th.randn(M, N, generator=g(4 + seed)))


def _gemm_case(M, N, K, tile, sk, precision=1):
    def build():
        from cgd_amd import ops
        ctx = ctx_of(precision)
        return dict(fn=lambda A, B, bias, R: ops.gemm(ctx, A, B, bias, R, alpha=1.0 / math.sqrt(K), force_tile=tile, splitk=sk),
                    inputs=_gemm_operands(M, N, K))
    return build


# 513 with split-K: workspace, reduce and frag_tmp; 518: the fragment cache (the staging B is a new pointer: the call packs, on the stream);
# 517: the weight-streaming GEMV; 64 with split-K 4: the implicit GEMM's workspace and reduce, in both precisions
case("gemm 200x96x256 tile513 sk2")(_gemm_case(200, 96, 256, 513, 2))
case("gemm 70x96x256 tile518")(_gemm_case(70, 96, 256, 518, 1))
case("gemm 3x1000x260 tile517")(_gemm_case(3, 1000, 260, 517, 1))
case("gemm 256x192x1024 tile64 sk4")(_gemm_case(256, 192, 1024, 64, 4))
case("gemm 256x192x1024 tile64 sk4 p0")(_gemm_case(256, 192, 1024, 64, 4, precision=0))


@case("gemm tile513: a larger B grows frag_tmp", warm=False)
def _gemm_grow():
    """hgemm.hip cgd_launch_hgemm synchronises the stream before it frees the smaller frag_tmp, by design: only values are judged.  The
    control runs on a context of its own, so that the TRIAL is the call that grows the buffer of a context which has just used the small
    one on another stream."""
    from cgd_amd import ops
    M, N, K = 200, 192, 512
    ctx_c, ctx_t = pc._ctx(1), pc._ctx(1)
    small = _gemm_operands(200, 96, 256)
    alpha = 1.0 / math.sqrt(K)

    def before():
        ops.gemm(ctx_t, *small, alpha=1.0, force_tile=513, splitk=2)

    return dict(fn=lambda A, B, bias, R: ops.gemm(ctx_t, A, B, bias, R, alpha=alpha, force_tile=513, splitk=2),
                control_fn=lambda A, B, bias, R: ops.gemm(ctx_c, A, B, bias, R, alpha=alpha, force_tile=513, splitk=2),
                inputs=_gemm_operands(M, N, K, seed=10), before_trial=before, keep=(ctx_c, ctx_t, small))


# ---- op level: conv ------------------------------------------------------------------------------------------------------------------------
def _conv_operands(Bn, H, W, Ci, Co):
    x = th.randn(Bn, H, W, Ci, generator=g(5))
    w = th.randn(Co, Ci, 3, 3, generator=g(6)) / math.sqrt(9 * Ci)
    b = 0.3 * th.randn(Co, generator=g(7))
    r = 0.3 * th.randn(Bn, H, W, Co, generator=g(17))
    return x, w, b, r


def _conv_case(Bn, H, W, Ci, Co, tile, sk):
    def build():
        from cgd_amd import ops
        ctx = ctx_of(1)
        x, w, b, r = _conv_operands(Bn, H, W, Ci, Co)
        wf = ops.pack_conv3x3(w)[0]
        xd, wd, wfd, bd, rd = _dev(x, w, wf, b, r)
        if tile in (512, 516):
            frag = ops.pack_conv3x3_frag(ctx, wd, dgrad=False)
            th.cuda.synchronize()
            return dict(fn=lambda x_, wf_, b_, r_, fr_: ops.conv3x3(ctx, x_, wf_, b_, R=r_, force_tile=tile, splitk=sk, w_frag=fr_),
                        inputs=[xd, wfd, bd, rd, frag])
        return dict(fn=lambda x_, wf_, b_, r_: ops.conv3x3(ctx, x_, wf_, b_, R=r_, force_tile=tile, splitk=sk), inputs=[xd, wfd, bd, rd])
    return build


case("conv3x3 igemm 2x12x20 64->96")(_conv_case(2, 12, 20, 64, 96, 0, 1))
case("conv3x3 hconv2 1x32x32 128->128 sk2")(_conv_case(1, 32, 32, 128, 128, 512, 2))
case("conv3x3 kconv 1x16x16 160->32")(_conv_case(1, 16, 16, 160, 32, 516, 1))


def _sconv_case(Bn, H, W, Ci, Co):
    """cgd_op_conv3x3_s2 and its dgrad with `add` (csrc/sconv.hip; the weight is packed per call into the context's scratch copy, on the stream)"""
    def build():
        from cgd_amd import ops
        ctx = ctx_of(1)
        x, w, b, _ = _conv_operands(Bn, H, W, Ci, Co)
        dy = th.randn(Bn, H // 2, W // 2, Co, generator=g(8))
        add = 0.3 * th.randn(Bn, H, W, Ci, generator=g(9))
        return dict(fn=lambda x_, w_, b_, dy_, add_: (ops.conv3x3_s2(ctx, x_, w_, b_), ops.conv3x3_s2_dgrad(ctx, dy_, w_, add=add_)),
                    inputs=_dev(x, w, b, dy, add))
    return build


# (the launcher's plan at 256 CUs, cgd_op_plan_conv_s2: 16 slices forward and 2 backward; one slice both ways)
case("conv3x3_s2 + dgrad 2x8x8 128->128 split-K")(_sconv_case(2, 8, 8, 128, 128))
case("conv3x3_s2 + dgrad 1x128x128 32->128 one slice")(_sconv_case(1, 128, 128, 32, 128))


@case("conv3x3_wino 1x16x16 32->32 gn_ab")
def _wconv():
    from cgd_amd import ops
    ctx = ctx_of(1)
    x, w, b, r = _conv_operands(1, 16, 16, 32, 32)
    ab = th.stack([0.5 + th.rand(1, 32, generator=g(18)), 0.5 * th.randn(1, 32, generator=g(19))], dim=2).contiguous()
    xd, wd, bd, rd, abd = _dev(x, w, b, r, ab)
    ww = ops.pack_conv3x3_wino(ctx, wd, dgrad=False)
    th.cuda.synchronize()
    return dict(fn=lambda x_, ww_, b_, r_, ab_: ops.conv3x3_wino(ctx, x_, ww_, 32, b_, R=r_, gn_ab=ab_), inputs=[xd, ww, bd, rd, abd])


@case("conv_in 2x16x24 3->64")
def _conv_in():
    from cgd_amd import ops
    ctx = ctx_of(1)
    x = th.randn(2, 3, 16, 24, generator=g(9))
    w = th.randn(64, 3, 3, 3, generator=g(10)) / math.sqrt(27)
    b = 0.3 * th.randn(64, generator=g(11))
    return dict(fn=lambda x_, wf_, b_: ops.conv_in(ctx, x_, wf_, b_, 64), inputs=_dev(x, ops.pack_conv3x3(w)[0], b))


@case("conv_thin_out 2x16x24 64->6")
def _conv_thin_out():
    from cgd_amd import ops
    ctx = ctx_of(1)
    w6 = th.randn(6, 64, 3, 3, generator=g(13)) / math.sqrt(9 * 64)
    b6 = 0.3 * th.randn(6, generator=g(14))
    h = th.randn(2, 16, 24, 64, generator=g(15))
    return dict(fn=lambda h_, wf_, b_: ops.conv_thin_out(ctx, h_, wf_, b_, 6), inputs=_dev(h, ops.pack_conv3x3(w6)[0], b6))


@case("sr_stem 2x32x32 low 8x8 ->32")
def _sr_stem():
    from cgd_amd import ops
    ctx = ctx_of(1)
    x = th.randn(2, 3, 32, 32, generator=g(70))
    low = th.rand(2, 3, 8, 8, generator=g(71)) * 2 - 1
    w = (th.rand(32, 6, 3, 3, generator=g(72)) * 2 - 1) * (3.0 / 54) ** 0.5
    bias = th.randn(32, generator=g(73)) * 0.02
    return dict(fn=lambda x_, low_, wf_, b_: ops.sr_stem(ctx, x_, low_, wf_, b_), inputs=_dev(x, low, ops.pack_conv3x3(w)[0], bias))


# ---- op level: norms and elementwise -----------------------------------------------------------------------------------------------------
# (B, HW, C, film, act, kernel family): one shape per family of value_regime_checks.GN_SHAPES
GN_SHAPES = [(2, 64, 128, True, 1, "register-cached"), (1, 1024, 2048, False, 1, "streaming"), (2, 64, 1344, True, 0, "scalar"),
             (1, 8192, 64, False, 1, "chunked")]


def _gn_case(B, HW, Cc, film, act):
    def build():
        from cgd_amd import ops
        ctx = ctx_of(1)
        x = th.randn(B, HW, Cc, generator=g(20)) * 2 + 0.7
        gamma = 1 + 0.1 * th.randn(Cc, generator=g(21))
        beta = 0.1 * th.randn(Cc, generator=g(22))
        fl = 0.3 * th.randn(B, 2 * Cc, generator=g(23)) if film else None
        dz = th.randn(B, HW, Cc, generator=g(24))

        def fn(x_, gamma_, beta_, dz_, fl_=None):
            y, scr = ops.groupnorm_fwd(ctx, x_, gamma_, beta_, fl_, act=act)
            return y, ops.groupnorm_bwd(ctx, x_, dz_, scr, act=act)

        return dict(fn=fn, inputs=[t for t in _dev(x, gamma, beta, dz, fl) if t is not None])
    return build


for _B, _HW, _C, _film, _act, _fam in GN_SHAPES:
    case(f"gn fwd+bwd {_fam} B{_B} HW{_HW} C{_C}")(_gn_case(_B, _HW, _C, _film, _act))


@case("ln fwd+bwd 50x768")
def _ln():
    from cgd_amd import ops
    ctx = ctx_of(1)
    x = th.randn(50, 768, generator=g(25)) * 1.5 + 0.3
    gamma = 1 + 0.1 * th.randn(768, generator=g(26))
    beta = 0.1 * th.randn(768, generator=g(27))
    dy = th.randn(50, 768, generator=g(28))

    def fn(x_, gamma_, beta_, dy_):
        y, st = ops.layernorm_fwd(ctx, x_, gamma_, beta_)
        return y, st, ops.layernorm_bwd(ctx, x_, dy_, gamma_, st)

    return dict(fn=fn, inputs=_dev(x, gamma, beta, dy))


@case("act fwd+bwd SiLU, QuickGELU; pool2x2; upsample2x")
def _elem():
    from cgd_amd import ops
    ctx = ctx_of(1)
    x = th.randn(2, 8, 12, 64, generator=g(30))
    v = th.randn(1000, generator=g(31)) * 3
    dy = th.randn(1000, generator=g(32))

    def fn(x_, v_, dy_):
        return (ops.act(ctx, v_, 1), ops.act(ctx, v_, 1, dy_), ops.act(ctx, v_, 2), ops.act(ctx, v_, 2, dy_), ops.pool2x2(ctx, x_),
                ops.upsample2x(ctx, x_))

    return dict(fn=fn, inputs=_dev(x, v, dy))


@case("bilinear_up2x fwd + adjoint 2x6x10 C32")
def _bilinear():
    ctx = ctx_of(1)
    B, Hi, Wi, Cc = 2, 6, 10, 32
    a = th.randn(B * Hi * Wi, Cc, generator=g(33))
    d = th.randn(B * 4 * Hi * Wi, Cc, generator=g(34))

    def fn(a_, d_):
        big, small = th.empty(B * 4 * Hi * Wi, Cc, device=DEV), th.empty(B * Hi * Wi, Cc, device=DEV)
        ctx.check(ctx.lib.cgd_op_bilinear_up2x(ctx.h, a_.data_ptr(), Cc, big.data_ptr(), Cc, B, Hi, Wi, Cc, 0, ctx.stream()))
        ctx.check(ctx.lib.cgd_op_bilinear_up2x(ctx.h, d_.data_ptr(), Cc, small.data_ptr(), Cc, B, Hi, Wi, Cc, 1, ctx.stream()))
        return big, small

    return dict(fn=fn, inputs=_dev(a, d))


# ---- op level: attention -----------------------------------------------------------------------------------------------------------------
def _attn_case(nb, heads, T, d, legacy, precision, envd, causal=False):
    def build():
        from cgd_amd import ops
        ctx = ctx_of(precision, **envd)
        Cc = heads * d
        qkv = th.randn(nb * T, 3 * Cc, generator=g(40))
        dout = th.randn(nb * T, Cc, generator=g(41))
        at = ops.Attention(ctx, nb, heads, T, d, legacy, DEV)
        if causal:
            return dict(fn=lambda q_: at.forward_causal(q_), inputs=_dev(qkv), keep=at)
        return dict(fn=lambda q_, do_: (at.forward(q_), at.backward(q_, do_)), inputs=_dev(qkv, dout), keep=at)
    return build


ATTN_CONTEXTS = [("p1", 1, {}), ("p1 flash0", 1, {"CGD_ATTN_FLASH": "0"}), ("p0", 0, {})]
ATTN_SHAPES = [(2, 2, 64, 64, 1), (3, 12, 50, 64, 0), (1, 2, 50, 80, 0)]
for _tag, _p, _env in ATTN_CONTEXTS:
    for _shape in ATTN_SHAPES:
        case(f"attn fwd+bwd [{_tag}] nb{_shape[0]} h{_shape[1]} T{_shape[2]} d{_shape[3]} legacy{_shape[4]}")(_attn_case(*_shape, _p, _env))
    case(f"attn causal fwd [{_tag}] T77")(_attn_case(1, 2, 77, 64, 0, _p, _env, causal=True))


# ---- op level: cutouts and the spherical loss -----------------------------------------------------------------------------------------------
def _cutouts_case(accumulate):
    """cgd_cutouts_fwd + cgd_cutouts_bwd, NCHW and patch-row layouts, at the smallest shape of parity_checks.check_cutouts_loss"""
    def build():
        ctx = ctx_of(1)
        B, H, W, cutn, cs, P = 1, 96, 96, 2, 64, 16
        coords = [(5, 9, 80), (0, 0, 96)]
        geo = th.tensor([(oy, ox, min(s, H - oy), min(s, W - ox)) for (ox, oy, s) in coords], dtype=th.int32)
        x = th.rand(B, 3, H, W, generator=g(50)) * 2.4 - 1.2
        dy = th.randn(cutn * B, 3, cs, cs, generator=g(51))
        rows = dy.reshape(cutn * B, 3, cs // P, P, cs // P, P).permute(0, 2, 4, 1, 3, 5).reshape(cutn * B * (cs // P) ** 2, -1).contiguous()
        pre = th.randn(B, 3, H, W, generator=g(54))
        lib = ctx.lib

        def fn(x_, cd_, dy_, rows_, g0_, g1_):
            s = ctx.stream()
            o0, o1 = th.empty(cutn * B, 3, cs, cs, device=DEV), th.empty(tuple(rows.shape), device=DEV)
            ctx.check(lib.cgd_cutouts_fwd(ctx.h, x_.data_ptr(), cd_.data_ptr(), o0.data_ptr(), B, H, W, cutn, cs, 0, 0, s))
            ctx.check(lib.cgd_cutouts_fwd(ctx.h, x_.data_ptr(), cd_.data_ptr(), o1.data_ptr(), B, H, W, cutn, cs, 1, P, s))
            ctx.check(lib.cgd_cutouts_bwd(ctx.h, dy_.data_ptr(), cd_.data_ptr(), g0_.data_ptr(), B, H, W, cutn, cs, 0, 0, int(accumulate), s))
            ctx.check(lib.cgd_cutouts_bwd(ctx.h, rows_.data_ptr(), cd_.data_ptr(), g1_.data_ptr(), B, H, W, cutn, cs, 1, P, int(accumulate), s))
            return o0, o1, g0_, g1_

        # g0 / g1 are in / out: the pre-fill when accumulating; NaN (which the launch must overwrite) when not
        g0 = pre if accumulate else th.full_like(pre, NAN)
        ins = _dev(x, geo, dy, rows, g0, g0.clone())
        return dict(fn=_fresh_inout(fn, ins, (4, 5)), inputs=ins, inout=(4, 5), poison={1: th.roll(ins[1], 1, 0)})
    return build


def _fresh_inout(fn, inputs, idx):
    """fn runs on clones of the in / out operands when it is handed the case's own inputs (warm-up, control), so that these keep their
    initial value for the trial's staging copies"""
    own = {inputs[k].data_ptr() for k in idx}

    def wrapped(*a):
        a = list(a)
        for k in idx:
            if a[k].data_ptr() in own:
                a[k] = a[k].clone()
        return fn(*a)
    return wrapped


case("cutouts fwd+bwd non-accumulating")(_cutouts_case(False))
case("cutouts fwd+bwd accumulating")(_cutouts_case(True))


def _resize_case(accumulate):
    """cgd_cutouts_resize_fwd / _bwd at the smallest case of test_gpu_resize_cutouts.py ('48-16': four flipped overviews, two inner cuts) and,
    for the adjoint, with NO cutout as well: that call is a hipMemsetAsync alone when it does not accumulate"""
    def build():
        from cgd_amd import guidance as dg
        ctx = ctx_of(1)
        B, H, W, cs = 1, 48, 48, 16
        recs = [(0, 0, 48, 48, f) for f in range(4)] + [(7, 11, 9, 9, 1), (32, 32, 16, 16, 0)]
        n = len(recs)
        tab = th.tensor(dg.resize_table(recs, H, W), dtype=th.int32)
        tab_p = th.tensor(dg.resize_table(recs[1:] + recs[:1], H, W), dtype=th.int32)  # the poison: the same boxes in another order
        gen = g(53)
        x = th.rand(B, 3, H, W, generator=gen) * 2 - 1
        d = th.randn(n * B, 3, cs, cs, generator=gen)
        pre = th.randn(B, 3, H, W, generator=g(54))
        lib = ctx.lib
        nscr = int(lib.cgd_cutouts_resize_scratch_floats(B, H, W, n))

        def fn(x_, tab_, d_, g_, gz_):
            s = ctx.stream()
            out, scratch = th.empty(n * B, 3, cs, cs, device=DEV), th.empty(nscr, device=DEV)
            ctx.check(lib.cgd_cutouts_resize_fwd(ctx.h, x_.data_ptr(), tab_.data_ptr(), tab_.data_ptr() + 16 * n, out.data_ptr(), B, H, W, n, cs,
                                                 0, 0, s))
            ctx.check(lib.cgd_cutouts_resize_bwd(ctx.h, d_.data_ptr(), tab_.data_ptr(), tab_.data_ptr() + 16 * n, g_.data_ptr(), scratch.data_ptr(),
                                                 B, H, W, n, cs, 0, 0, int(accumulate), s))
            ctx.check(lib.cgd_cutouts_resize_bwd(ctx.h, None, None, None, gz_.data_ptr(), None, B, H, W, 0, cs, 0, 0, int(accumulate), s))
            return out, g_, gz_

        g0 = pre if accumulate else th.full_like(pre, NAN)
        ins = _dev(x, tab, d, g0, g0.clone())
        return dict(fn=_fresh_inout(fn, ins, (3, 4)), inputs=ins, inout=(3, 4), poison={1: tab_p.to(DEV)})
    return build


case("resize cutouts fwd+bwd non-accumulating")(_resize_case(False))
case("resize cutouts fwd+bwd accumulating")(_resize_case(True))


@case("spherical loss cutn3 B2 P2 D768")
def _spherical():
    import torch.nn.functional as F
    ctx = ctx_of(1)
    cutn, B, P, D = 3, 2, 2, 768
    emb = th.randn(cutn * B, D, generator=g(52))
    tg = F.normalize(th.randn(P, D, generator=g(53)), dim=-1)
    wm = (th.eye(B) * 0.7).contiguous()

    def fn(e_, t_, w_):
        demb, part = th.empty(cutn * B, D, device=DEV), th.empty(cutn * B, device=DEV)
        ctx.check(ctx.lib.cgd_spherical_loss(ctx.h, e_.data_ptr(), t_.data_ptr(), w_.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B, P, D,
                                             1000.0, ctx.stream()))
        return demb, part

    return dict(fn=fn, inputs=_dev(emb, tg, wm))


# ---- op level: the guided step's tail and the samplers' update kernels ------------------------------------------------------------------------
def _randn_dev(n, shape, seed):
    gen = g(seed)
    return _dev(*[th.randn(*shape, generator=gen) for _ in range(n)])


def _scal():
    return th.tensor([0, 0, 0, 0, 0, 0, 0, 0.37]).float()  # cgd_scalars' record: slot 7 is the clamp factor


@case("step tail: pmv_blend, guidance_combine, grad_finish, scalars, sample_update (p_sample, ddim) 2x24x40")
def _tail():
    """the five entries of test_gpu_tail.py chained as a guided step chains them, at tail_ref.SHAPES[3] and the middle step"""
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    from tests import tail_ref as tr
    ctx = ctx_of(1)
    lib = ctx.lib
    shape = B, H, W = tr.SHAPES[3]
    k = dd.create_gaussian_diffusion(*tr.SCHEDULE).step_coef(tr.STEPS["mid"], tr.STEPS["mid"])
    nblk = int(lib.cgd_guidance_part_blocks(B, H, W))
    x, out6 = tr.pmv_inputs(shape, tr.STEPS["mid"], k)
    g_clip = tr.combine_inputs(shape, tr.STEPS["mid"])[2]
    gu = tr.finish_inputs(shape)[1]
    clip_part = th.rand(7, generator=g(61))
    noise = th.randn(B, 3, H, W, generator=g(62))

    def fn(x_, out6_, gclip_, gu_, cp_, noise_):
        s = ctx.stream()
        img = lambda c=3: th.empty(B, c, H, W, device=DEV)  # noqa: E731
        px0, mean, logvar, x_in = img(), img(), img(), img()
        ctx.check(lib.cgd_pmv_blend(ctx.h, x_.data_ptr(), out6_.data_ptr(), px0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), x_in.data_ptr(),
                                    B, H, W, k, s))
        gdir, seed6, lpart = img(), img(6), th.empty(nblk * 3, device=DEV)
        ctx.check(lib.cgd_guidance_combine(ctx.h, gclip_.data_ptr(), x_in.data_ptr(), px0.data_ptr(), gdir.data_ptr(), seed6.data_ptr(),
                                           lpart.data_ptr(), B, H, W, k, *tr.SCALES, s))
        gg, gpart = img(), th.empty(nblk * 2, device=DEV)
        ctx.check(lib.cgd_grad_finish(ctx.h, gdir.data_ptr(), gu_.data_ptr(), gg.data_ptr(), gpart.data_ptr(), B, H, W, s))
        scal = th.empty(8, device=DEV)
        ctx.check(lib.cgd_scalars(ctx.h, cp_.data_ptr(), cp_.numel(), lpart.data_ptr(), gpart.data_ptr(), B, H, W, 1, scal.data_ptr(), s))
        outs = [px0, mean, logvar, x_in, gdir, seed6, lpart, gg, gpart, scal]
        for mode in (0, 1):
            sample, x0_out = img(), img()
            ctx.check(lib.cgd_sample_update(ctx.h, x_.data_ptr(), px0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), gg.data_ptr(),
                                            noise_.data_ptr(), scal.data_ptr(), sample.data_ptr(), x0_out.data_ptr(), B, H, W, k, mode, s))
            outs += [sample, x0_out]
        return outs

    return dict(fn=fn, inputs=_dev(x, out6, g_clip, gu, clip_part, noise))


def _dpm_rig():
    from cgd_amd import diffusion as dd
    return ctx_of(1), dd.create_gaussian_diffusion(1000, "linear", "dpm50", False)


@case("dpmpp_update 2x24x40 order 2 eta 1")
def _dpmpp_update():
    ctx, tab = _dpm_rig()
    shape = B, _, H, W = (2, 3, 24, 40)
    k, d = tab.step_coef(20, 3), tab.dpmpp_coef(20, 2, 1.0)
    assert d.c_n != 0 and d.c_r != 0  # the noise and the history are read

    def fn(x_, x0_, g_, scal_, noise_, hist_):
        sample, x0c, x0o = (th.empty(shape, device=DEV) for _ in range(3))
        ctx.check(ctx.lib.cgd_dpmpp_update(ctx.h, x_.data_ptr(), x0_.data_ptr(), g_.data_ptr(), scal_.data_ptr(), noise_.data_ptr(), hist_.data_ptr(),
                                           x0c.data_ptr(), sample.data_ptr(), x0o.data_ptr(), B, H, W, k, d, ctx.stream()))
        return sample, x0c, x0o

    x, x0, gg, noise, hist = _randn_dev(5, shape, 63)
    return dict(fn=fn, inputs=[x, x0, gg, _dev(_scal())[0], noise, hist])


@case("dpmpp_threshold (five launches) + dpmpp_update_thr 2x24x40 cap 1.5")
def _dpmpp_thr():
    ctx, tab = _dpm_rig()
    shape = B, _, H, W = (2, 3, 24, 40)
    k, d = tab.step_coef(20, 3), tab.dpmpp_coef(20, 2, 1.0)
    n = 3 * H * W
    rank, frac = tab.threshold_rank(0.9, n)
    nbytes = int(ctx.lib.cgd_abs_quantile_scratch_bytes(B, n))

    def fn(x_, x0_, g_, scal_, noise_, hist_):
        s = ctx.stream()
        raw, thr3 = th.empty(shape, device=DEV), th.empty(B, 3, device=DEV)
        scratch = th.zeros(nbytes, dtype=th.uint8, device=DEV)
        ctx.check(ctx.lib.cgd_dpmpp_threshold(ctx.h, x_.data_ptr(), x0_.data_ptr(), g_.data_ptr(), scal_.data_ptr(), raw.data_ptr(), B, H, W, k, rank,
                                              frac, 1.0, 1.5, thr3.data_ptr(), scratch.data_ptr(), s))
        sample, x0c, x0o = (th.empty(shape, device=DEV) for _ in range(3))
        ctx.check(ctx.lib.cgd_dpmpp_update_thr(ctx.h, x_.data_ptr(), x0_.data_ptr(), raw.data_ptr(), thr3.data_ptr(), noise_.data_ptr(),
                                               hist_.data_ptr(), x0c.data_ptr(), sample.data_ptr(), x0o.data_ptr(), B, H, W, k, d, s))
        return raw, thr3, sample, x0c, x0o

    x, x0, gg, noise, hist = _randn_dev(5, shape, 64)
    return dict(fn=fn, inputs=[x, x0, gg, _dev(_scal())[0], noise, hist])


@case("abs_quantile 3 rows of 2880")
def _abs_quantile():
    ctx, tab = _dpm_rig()
    B, n = 3, 2880
    rank, frac = tab.threshold_rank(0.9, n)
    nbytes = int(ctx.lib.cgd_abs_quantile_scratch_bytes(B, n))

    def fn(v_):
        out, scratch = th.empty(B, 3, device=DEV), th.zeros(nbytes, dtype=th.uint8, device=DEV)
        ctx.check(ctx.lib.cgd_op_abs_quantile(ctx.h, v_.data_ptr(), B, n, rank, frac, 0.0, math.inf, out.data_ptr(), scratch.data_ptr(), ctx.stream()))
        return out

    return dict(fn=fn, inputs=_randn_dev(1, (B, n), 65))


@case("multistep_update 2x24x40: Adams-Bashforth order 4, corrector, ddim eta")
def _multistep():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    ctx = ctx_of(1)
    tab = dd.create_gaussian_diffusion(1000, "linear", "plms50", False)
    shape = B, _, H, W = (2, 3, 24, 40)
    t = 20
    ab, abp = tab.alphas_cumprod[t], tab.alphas_cumprod_prev[t]
    sigma = 0.5 * math.sqrt((1 - abp) / (1 - ab)) * math.sqrt(1 - ab / abp)
    # (phase, order, k, ks, sigma, dirc): the cases of test_gpu_plms.py
    phases = [(0, 4, tab.step_coef(t, 3), None, 0.0, 0.0), (2, 0, tab.step_coef(t - 1, 3), tab.step_coef(t, 3), 0.0, 0.0),
              (3, 0, tab.step_coef(t, 3), None, sigma, math.sqrt(1 - abp - sigma ** 2))]

    def fn(x_, xe_, x0_, g_, scal_, noise_, h0_, h1_, h2_):
        hp = (C.c_void_p * 3)(h0_.data_ptr(), h1_.data_ptr(), h2_.data_ptr())
        outs = []
        for phase, order, k, ks, sg, dc in phases:
            sample, x0_out, eps_out = (th.empty(shape, device=DEV) for _ in range(3))
            ctx.check(ctx.lib.cgd_multistep_update(ctx.h, x_.data_ptr(), xe_.data_ptr() if phase == 2 else None, x0_.data_ptr(), g_.data_ptr(),
                                                   scal_.data_ptr(), noise_.data_ptr() if phase == 3 else None, hp, eps_out.data_ptr(),
                                                   sample.data_ptr(), x0_out.data_ptr(), B, H, W, k, ks, L.Multistep(phase, order, sg, dc),
                                                   ctx.stream()))
            outs += [sample] if phase == 2 else [sample, x0_out] + ([eps_out] if phase == 0 else [])  # the corrector writes the sample alone
        return outs

    x, xe, x0, gg, noise, h0, h1, h2 = _randn_dev(8, shape, 66)
    return dict(fn=fn, inputs=[x, xe, x0, gg, _dev(_scal())[0], noise, h0, h1, h2])


@case("ddim_reverse_update 2x24x40 with pred_xstart and noise")
def _reverse():
    from cgd_amd import diffusion as dd
    ctx = ctx_of(1)
    k = dd.create_gaussian_diffusion(1000, "linear", "50", False).reverse_coef(5)
    shape = B, _, H, W = (2, 3, 24, 40)

    def fn(x_, out6_, init_):
        xn, x0, nz = (th.empty(shape, device=DEV) for _ in range(3))
        ctx.check(ctx.lib.cgd_ddim_reverse_update(ctx.h, x_.data_ptr(), out6_.data_ptr(), init_.data_ptr(), xn.data_ptr(), x0.data_ptr(), nz.data_ptr(),
                                                  B, H, W, 1, k, ctx.stream()))
        return xn, x0, nz

    gen = g(67)
    return dict(fn=fn, inputs=_dev(th.randn(shape, generator=gen), th.randn(B, 6, H, W, generator=gen), th.tanh(th.randn(1, 3, H, W, generator=gen))))


@case("masked_merge 2x24x40 with pred_xstart and re-noise")
def _masked():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    from tests import masked_ref
    ctx = ctx_of(1)
    shape = B, _, H, W = (2, 3, 24, 40)
    k = dd.create_gaussian_diffusion(1000, "linear", "50", False).mask_coef(20)
    assert k.sqrt_one_minus_ab_prev != 0.0
    k.flags = L.MASK_PRED_XSTART | L.MASK_N_KNOWN | L.MASK_RENOISE
    gen = g(68)
    sample, x0, n_known, n_re = (th.randn(shape, generator=gen) for _ in range(4))
    init = th.tanh(th.randn(1, 3, H, W, generator=gen))
    mask = masked_ref.make_mask((B, 1, H, W), seed=5).float()

    def fn(sample_, x0_, init_, mask_, nk_, nre_):
        xre = th.empty(shape, device=DEV)
        ctx.check(ctx.lib.cgd_masked_merge(ctx.h, sample_.data_ptr(), x0_.data_ptr(), init_.data_ptr(), mask_.data_ptr(), nk_.data_ptr(),
                                           nre_.data_ptr(), xre.data_ptr(), B, H, W, 1, B, 1, k, ctx.stream()))
        return sample_, x0_, xre

    ins = _dev(sample, x0, init, mask, n_known, n_re)
    return dict(fn=_fresh_inout(fn, ins, (0, 1)), inputs=ins, inout=(0, 1))


@case("ilvr_refine (two launches) 2x32x48 N 4 with pred_xstart and noise")
def _ilvr():
    ctx = ctx_of(1)
    B, H, W, N = 2, 32, 48, 4
    nscr = int(ctx.lib.cgd_ilvr_scratch_floats(B, H, W, N, 1))
    gen = g(69)
    sample, x0, noise = (th.randn(B, 3, H, W, generator=gen) for _ in range(3))
    ref = th.tanh(th.randn(1, 3, H, W, generator=gen))

    def fn(sample_, x0_, ref_, noise_):
        scratch = th.empty(nscr, device=DEV)
        ctx.check(ctx.lib.cgd_ilvr_refine(ctx.h, sample_.data_ptr(), x0_.data_ptr(), ref_.data_ptr(), noise_.data_ptr(), scratch.data_ptr(), B, H, W, 1,
                                          N, 0.8, 0.6, ctx.stream()))
        return sample_, x0_

    ins = _dev(sample, x0, ref, noise)
    return dict(fn=_fresh_inout(fn, ins, (0, 1)), inputs=ins, inout=(0, 1))


@case("window_gather + window_merge 1x3 40x48, window 32 stride 8, wrap x, feathered")
def _window():
    from cgd_amd import windows
    ctx = ctx_of(1)
    B, Cn, H, W, S = 1, 3, 40, 48, 32
    p = windows.WindowPlan(H, W, S, 8, "x", True).to(DEV)
    th.cuda.synchronize()
    oy, ox = (C.c_int * p.ny)(*p.oy), (C.c_int * p.nx)(*p.ox)

    def fn(full_, ay_, ax_):
        s = ctx.stream()
        win, back = th.empty(B * p.n, Cn, S, S, device=DEV), th.empty(B, Cn, H, W, device=DEV)
        ctx.check(ctx.lib.cgd_window_gather(ctx.h, full_.data_ptr(), win.data_ptr(), oy, p.ny, ox, p.nx, None, None, B, Cn, H, W, S, p.wrap, s))
        ctx.check(ctx.lib.cgd_window_merge(ctx.h, win.data_ptr(), back.data_ptr(), oy, p.ny, ox, p.nx, ay_.data_ptr(), ax_.data_ptr(), B, Cn, H, W, S,
                                           p.wrap, 0, s))
        return win, back

    return dict(fn=fn, inputs=_randn_dev(1, (B, Cn, H, W), 70) + [p.ay, p.ax], keep=p)


# ---- op level: Gram, the fused GEMM + GroupNorm backward, the attention-pool head ---------------------------------------------------------
@case("gram (two kernels) B2 N192 C256")
def _gram():
    ctx = ctx_of(1)
    B, N, Cc = 2, 192, 256
    rows = th.relu(th.randn(B * N, Cc, generator=g(60)))

    def fn(a_):
        out = th.empty(B, Cc, Cc, device=DEV)
        ctx.check(ctx.lib.cgd_op_gram(ctx.h, a_.data_ptr(), Cc, B, N, Cc, 1.0 / N, out.data_ptr(), ctx.stream()))
        return out

    return dict(fn=fn, inputs=_dev(rows))


@case("gemm_gn_bwd B2 HW256 C96 K64 with addend")
def _gemm_gn_bwd():
    from cgd_amd import ops
    from tests import test_gpu_gemm_gn_bwd as tg
    ctx = ctx_of(1)
    c = tg.case(2, 256, 96, 64, True)
    ins = _dev(c["dout"], c["w"], c["x"], c["dz"], c["coef"], c["bcoef"], c["skip"])
    return dict(fn=lambda a_, w_, x_, dz_, cf_, bc_, add_: ops.gemm_gn_bwd(ctx, a_, w_, x_, dz_, cf_, bc_, add=add_), inputs=ins)


@case("attnpool fwd+bwd B3 C128 S4 d32 out7")
def _attnpool():
    ctx = ctx_of(1)
    B, Cc, S, d, out = 3, 128, 4, 32, 7
    gen = g(71)
    h = th.randn(B * S * S, Cc, generator=gen)
    w = [th.randn(Cc * (S * S + 1), generator=gen) / Cc ** 0.5, th.randn(3 * Cc * Cc, generator=gen) / Cc ** 0.5, th.randn(3 * Cc, generator=gen) * 0.1,
         th.randn(out * Cc, generator=gen) * 4.0 / Cc ** 0.5, th.randn(out, generator=gen) * 0.1]
    y = th.tensor([0, 6, 2])
    n = int(ctx.lib.cgd_op_attnpool_scratch_floats(B, S, Cc, d, out))

    def fn(h_, w0, w1, w2, w3, w4, y_):
        s = ctx.stream()
        scratch = th.empty(n, device=DEV)
        pooled, logits, logp = th.empty(B, Cc, device=DEV), th.empty(B, out, device=DEV), th.empty(B, device=DEV)
        ctx.check(ctx.lib.cgd_op_attnpool_fwd(ctx.h, h_.data_ptr(), w0.data_ptr(), w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), w4.data_ptr(),
                                              y_.data_ptr(), pooled.data_ptr(), logits.data_ptr(), logp.data_ptr(), scratch.data_ptr(), B, S, Cc, d, out, s))
        dh = th.empty(B * S * S, Cc, device=DEV)
        ctx.check(ctx.lib.cgd_op_attnpool_bwd(ctx.h, w1.data_ptr(), w2.data_ptr(), w3.data_ptr(), w4.data_ptr(), 0.5, dh.data_ptr(), scratch.data_ptr(),
                                              B, S, Cc, d, out, s))
        return pooled, logits, logp, dh

    return dict(fn=fn, inputs=_dev(h, *w, y))


# ---- op level: augmented cutouts, the directional loss, region prompts, the secondary model's kernels -------------------------------------
def _aug_case(accumulate):
    """cgd_cutouts_aug_fwd / _bwd with the noise on, patch-row layout; every box has the same extent, so that the poison of the box and
    parameter tables — the same records in another order — stays consistent with the noise offsets"""
    def build():
        from cgd_amd import guidance as dg
        ctx = ctx_of(1)
        B, H, W, cs, P = 1, 48, 64, 32, 16
        coords = [(3, 5, 24), (20, 9, 24), (40, 24, 24), (11, 17, 24)]  # (ox, oy, size), all inside the frame
        n = len(coords)
        th.manual_seed(5)
        aug = dg._AugLaunch(ctx.lib, coords, B, H, W, th.device(DEV))
        th.cuda.synchronize()
        assert all((h, w) == (24, 24) for _, _, h, w in aug.geo_list)
        per = 4 * 3 * B * 24 * 24
        noise = th.randn(n * per, generator=g(72)) * 0.01
        off = th.arange(n, dtype=th.int64) * per
        x = th.tanh(th.randn(B, 3, H, W, generator=g(73)))
        d = th.randn(n * B * (cs // P) ** 2, 3 * P * P, generator=g(74))
        pre = th.randn(B, 3, H, W, generator=g(75))
        nscr = int(ctx.lib.cgd_cutouts_aug_scratch_floats(B, H, W, n))
        lib = ctx.lib

        def fn(x_, geo_, par_, noise_, off_, d_, g_):
            s = ctx.stream()
            out, scratch = th.empty(tuple(d.shape), device=DEV), th.empty(nscr, device=DEV)
            ctx.check(lib.cgd_cutouts_aug_fwd(ctx.h, x_.data_ptr(), geo_.data_ptr(), par_.data_ptr(), noise_.data_ptr(), off_.data_ptr(), out.data_ptr(),
                                              B, H, W, n, cs, 1, P, s))
            ctx.check(lib.cgd_cutouts_aug_bwd(ctx.h, d_.data_ptr(), geo_.data_ptr(), par_.data_ptr(), g_.data_ptr(), scratch.data_ptr(), B, H, W, n, cs,
                                              1, P, int(accumulate), s))
            return out, g_

        ins = [x.to(DEV), aug.geo.clone(), aug.params.clone(), noise.to(DEV), off.to(DEV), d.to(DEV), (pre if accumulate else th.full_like(pre, NAN)).to(DEV)]
        th.cuda.synchronize()
        return dict(fn=_fresh_inout(fn, ins, (6,)), inputs=ins, inout=(6,),
                    poison={1: th.roll(ins[1], 1, 0), 2: th.roll(ins[2], 1, 0), 4: ins[4].clone()})
    return build


case("aug cutouts fwd+bwd non-accumulating")(_aug_case(False))
case("aug cutouts fwd+bwd accumulating")(_aug_case(True))


def _region_case():
    from tests import region_ref as R
    return R.make_case(R.CASES[0])  # cutn 5, B 2, P 3, D 512, two gray masks, one prompt without a region


def _region_tensors(c):
    from cgd_amd import regions
    sat = regions.build_sat(c["masks"])
    ro = th.tensor(list(c["region_of"]), dtype=th.int32)
    return sat, ro, th.tensor(c["power"], dtype=th.float32), th.tensor(c["boxes"], dtype=th.int32).view(-1, 4)


@case("directional_loss + spherical / directional _regions + region_coverage (cutn5 B2 P3 D512)")
def _losses():
    from tests import region_ref as R
    ctx = ctx_of(1)
    lib = ctx.lib
    c = _region_case()
    cutn, B, P, Dm = c["cutn"], c["B"], c["P"], c["D"]
    N = cutn * B
    sat, ro, power, geo = _region_tensors(c)
    nreg = sat.shape[0]
    ins = _dev(c["e"].float().contiguous(), c["s"].float().contiguous(), c["d"].float().contiguous(), c["w"].float().contiguous(), sat, ro, power, geo)
    Bs = c["s"].shape[0] // cutn
    nbox = geo.shape[0]

    def fn(e_, s_, d_, w_, sat_, ro_, pw_, geo_):
        st = ctx.stream()
        tail = (sat_.data_ptr(), ro_.data_ptr(), ro.data_ptr(), pw_.data_ptr(), geo_.data_ptr(), nreg, R.H, R.W)
        outs = []
        for regions_on in (False, True):
            demb, part = th.empty(N, Dm, device=DEV), th.empty(N, device=DEV)
            ctx.check(getattr(lib, "cgd_directional_loss" + ("_regions" if regions_on else ""))(
                ctx.h, e_.data_ptr(), s_.data_ptr(), d_.data_ptr(), w_.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B, Bs, P, Dm, R.SCALE, 0,
                *(tail if regions_on else ()), st))
            outs += [demb, part]
        demb, part = th.empty(N, Dm, device=DEV), th.empty(N, device=DEV)
        ctx.check(lib.cgd_spherical_loss_regions(ctx.h, e_.data_ptr(), d_.data_ptr(), w_.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B, P, Dm,
                                                 R.SCALE, *tail, st))
        cov = th.empty(nbox, P, device=DEV)
        ctx.check(lib.cgd_op_region_coverage(ctx.h, *tail[:5], cov.data_ptr(), nbox, P, *tail[5:], st))
        return outs + [demb, part, cov]

    # the boxes' poison is the same boxes in another order (valid, different coverage)
    return dict(fn=fn, inputs=ins, poison={7: th.roll(ins[7], 1, 0)}, keep=ro)


@case("secondary_pack + secondary_head + secondary_combine 1x32x32")
def _secondary_ops():
    ctx = ctx_of(1)
    lib = ctx.lib
    B, H, W = 1, 32, 32
    gen = g(76)
    x, v, gin = th.randn(B, 3, H, W, generator=gen), th.randn(B, 3, H, W, generator=gen), th.randn(B, 3, H, W, generator=gen) * 1e-2
    t = th.tensor([0.37])
    wemb = th.randn(8, generator=gen)  # timestep_embed.weight: 8 frequencies, 16 Fourier features
    nblk = int(lib.cgd_guidance_part_blocks(B, H, W))

    def fn(x_, t_, w_, v_, gin_):
        s = ctx.stream()
        packed = th.empty(B * H * W, 32, device=DEV)
        ctx.check(lib.cgd_op_secondary_pack(ctx.h, x_.data_ptr(), t_.data_ptr(), w_.data_ptr(), packed.data_ptr(), B, H, W, s))
        pred, xin = th.empty(B, 3, H, W, device=DEV), th.empty(B, 3, H, W, device=DEV)
        ctx.check(lib.cgd_secondary_head(ctx.h, v_.data_ptr(), x_.data_ptr(), t_.data_ptr(), 0.3, pred.data_ptr(), xin.data_ptr(), B, H, W, s))
        gdir, seed, part = th.empty(B, 3, H, W, device=DEV), th.empty(B, 3, H, W, device=DEV), th.empty(nblk, 3, device=DEV)
        ctx.check(lib.cgd_secondary_combine(ctx.h, gin_.data_ptr(), xin.data_ptr(), pred.data_ptr(), gdir.data_ptr(), seed.data_ptr(), part.data_ptr(),
                                            B, H, W, 0.3, 0.8, 0.6, 40.0, 30.0, 3.0, s))
        return packed, pred, xin, gdir, seed, part

    return dict(fn=fn, inputs=_dev(x, t, wemb, v, gin))


# ---- network passes: warm, bit-equal to the control on the same handle, and once against the oracle ----------------------------------------
def _grade(call, seed, flips_bwd=False):
    def grade(outs):
        ora = lc.oracle(call, seed)
        recs = [rec(f"streams: {call.tag} trial forward vs the oracle", outs[0], ora["fwd"])]
        if len(outs) > 1 and ora["bwd"] is not None:
            recs.append((rec_flips if flips_bwd else rec)(f"streams: {call.tag} trial dgrad vs the oracle", outs[1], ora["bwd"]))
        return recs
    return grade


def _unet_case(precision, slots=False):
    def build():
        seed = lc.SEEDS["unet"][0]
        ctx = pc._ctx(precision)
        dev = lc._handle(ctx, "unet", seed, lc.UNET_CASE)
        call = lc.UNetCall(1, 64, 64, 0)
        sd = lc.oracle(call, seed)["sd"]

        def fn(x_, t_, y_, go_):
            if slots:
                dev.embed(t_, y_, 1)
                o = dev.forward_slot(x_, 1)
            else:
                o = dev.forward(x_, t_, y_)
            return o, dev.dgrad(go_)

        return dict(fn=fn, inputs=_dev(call.x, call.t, call.y, call.gout * sd), grade=_grade(call, seed), keep=(ctx, dev))
    return build


case("unet mini 1x64x64 forward + dgrad p1")(_unet_case(1))
case("unet mini 1x64x64 forward + dgrad p0")(_unet_case(0))
case("unet mini 1x64x64 embed + forward_slot + dgrad")(_unet_case(1, slots=True))


@case("unet classic narrow 1x64x64 forward + dgrad p1")
def _classic_unet_case():
    """the narrow community structure (conv resampling, additive embedding): five Downsamples and Upsamples"""
    seed = lc.SEEDS["unet"][0]
    ctx = pc._ctx(1)
    dev = lc._handle(ctx, "unet", seed, lc.CLASSIC_CASE)
    call = lc.UNetCall(1, 64, 64, 0, lc.CLASSIC_CASE)
    sd = lc.oracle(call, seed)["sd"]
    return dict(fn=lambda x_, t_, go_: (dev.forward(x_, t_), dev.dgrad(go_)), inputs=_dev(call.x, call.t, call.gout * sd), grade=_grade(call, seed),
                keep=(ctx, dev))


def _tower_case(kind):
    def build():
        seed = lc.SEEDS[kind][0]
        ctx = pc._ctx(1)
        dev = lc._handle(ctx, kind, seed)
        call = lc.VitCall(3) if kind == "vit" else lc.RnCall(2)
        sd = lc.oracle(call, seed)["sd"]
        return dict(fn=lambda img_, de_: (dev.encode_image(img_), dev.dgrad(de_)), inputs=_dev(call.img, call.de * sd),
                    grade=_grade(call, seed, flips_bwd=call.flips), keep=(ctx, dev))
    return build


case("vit ViT-B/32 N3 forward + dgrad")(_tower_case("vit"))
case("resnet tiny N2 forward + dgrad")(_tower_case("rn"))


@case("text tower N2 forward (cgd_text_forward)")
def _text():
    seed = lc.SEEDS["text"][0]
    ctx = pc._ctx(1)
    dev = lc._handle(ctx, "text", seed)
    call = lc.TextCall(2)

    def fn(tok_):  # the raw entry: the wrapper range-checks the ids on the host (SYNCS_BY_DESIGN)
        out = th.empty(tok_.shape[0], dev.out_dim, device=DEV)
        ctx.check(ctx.lib.cgd_text_forward(dev.h, tok_.data_ptr(), tok_.shape[0], out.data_ptr(), ctx.stream()))
        return out

    return dict(fn=fn, inputs=_dev(call.tok.to(th.int64)), grade=_grade(call, seed), keep=(ctx, dev))


@case("lpips set_reference + loss_grad 2x64x64")
def _lpips():
    seed = lc.SEEDS["lpips"][0]
    ctx = pc._ctx(1)
    dev = lc._handle(ctx, "lpips", seed)
    call = lc.LpipsCall(2, 64, 64)
    sd = lc.oracle(call, seed)["sd"]

    def fn(ref_, x_):
        dev.set_reference(ref_)
        return dev.loss_grad(x_, grad_scale=sd)

    return dict(fn=fn, inputs=_dev(call.ref, call.x), grade=_grade(call, seed), keep=(ctx, dev))


@case("lpips set_style + style_loss_grad 2x64x64")
def _style():
    from tests import test_gpu_style as ts
    case_ = ts._head_case(2, 64, 64, 48, 80)
    ctx = pc._ctx(1)
    dev = ts._device_net(ctx, case_["orc"])
    gs = pc.unit_seed(case_["grad"])

    def fn(style_, x_):
        dev.set_style(style_)
        loss, _, gx = dev.style_loss_grad(x_, style_scale=gs)
        return loss, gx

    def grade(outs):
        return [rec("streams: lpips style trial loss vs the oracle", outs[0], case_["loss"].float()),
                rec("streams: lpips style trial gradient vs the oracle", outs[1], (case_["grad"] * gs).float())]

    return dict(fn=fn, inputs=_dev(case_["style"], case_["x"]), grade=grade, keep=(ctx, dev))


@case("secondary model 1x32x32 forward + dgrad")
def _secondary_net():
    from tests import test_gpu_secondary as tsec
    ctx, _, dev = tsec._pair()
    r = tsec._reference(1, 32, 32)

    def grade(outs):
        return [rec("streams: secondary trial pred vs the reference", outs[0], r["pred"]),
                rec_flips("streams: secondary trial dx vs the reference", outs[1], r["dx"])]

    return dict(fn=lambda x_, t_, dv_: (dev.forward(x_, t_), dev.dgrad(dv_)), inputs=_dev(r["x"], r["t"], r["dv"]), grade=grade, keep=(ctx, dev))


@case("classifier clsA forward + dgrad")
def _classifier():
    from tests import test_gpu_classifier as tcl
    _, dev = tcl._net_pair("clsA")
    r = tcl._net_reference("clsA")

    def fn(x_, t_, y_):
        logits, logp = dev.forward(x_, t_, y_)
        return logits, logp, dev.dgrad(r["seed"])

    def grade(outs):
        return [rec("streams: classifier trial logits vs the reference", outs[0], r["logits"]),
                rec("streams: classifier trial logp vs the reference", outs[1], r["logp"]),
                rec("streams: classifier trial dx vs the reference", outs[2], r["dx"] * r["seed"])]

    return dict(fn=fn, inputs=_dev(r["x"], r["t"], r["y"]), grade=grade, keep=dev)


@case("super-resolution mini set_low_res + forward + dgrad 2x32x40")
def _superres():
    from oracle.unet import UNetModel, synthetic_init_
    from tests import test_gpu_superres as tsr
    unet = synthetic_init_(UNetModel(**tsr.SR_CASE), seed=1234).eval()
    for p in unet.parameters():
        p.requires_grad_(False)
    B, (H, W) = 2, tsr.FRAME
    x, t, y = th.randn(B, 3, H, W, generator=g(60)), th.tensor([417.0] * B), th.randint(0, 10, (B,), generator=g(61))
    low = th.rand(B, 3, *tsr.LOW, generator=g(63)) * 2 - 1
    gout = th.randn(B, 6, H, W, generator=g(62))
    gout[:, 3:] = 0
    xr = x.clone().requires_grad_()
    o = tsr.SuperResModel(unet)(xr, t, y, low_res=low)
    (o * gout).sum().backward()
    sd = pc.unit_seed(xr.grad)
    ctx = pc._ctx(1)
    dev = tsr._device_net(ctx, unet)

    def fn(low_, x_, t_, y_, go_):
        dev.set_low_res(low_)
        return dev.forward(x_, t_, y_), dev.dgrad(go_)

    def grade(outs):
        return [rec("streams: super-resolution trial forward vs the oracle", outs[0], o.detach()),
                rec("streams: super-resolution trial dgrad vs the oracle", outs[1], xr.grad * sd)]

    return dict(fn=fn, inputs=_dev(low, x, t, y, gout * sd), grade=grade, keep=(ctx, dev))


# ---- hand-over between streams on one context ------------------------------------------------------------------------------------------------
def _two_streams():
    return th.cuda.Stream(), th.cuda.Stream()


def _staged(s, tensors):
    """on stream s: poison staging copies, the delay, the true values behind it"""
    with th.cuda.stream(s):
        st = [poison_like(t) for t in tensors]
        enqueue_delay()
        for a, b in zip(st, tensors):
            a.copy_(b)
    return st


def check_handover(kind):
    """Forward on s1, dgrad on s2 after s2.wait_stream(s1) — the caller orders the streams, as the header asks —, each stream behind its own
    delay: bit-equal to the one-stream result of the same handle."""
    prepare()
    seed = lc.SEEDS[kind][0]
    ctx = pc._ctx(1)
    dev = lc._handle(ctx, kind, seed, lc.UNET_CASE if kind == "unet" else None)
    if kind == "unet":
        call = lc.UNetCall(1, 64, 64, 0)
        fwd_in, bwd_in = _dev(call.x, call.t, call.y), _dev(call.gout * lc.oracle(call, seed)["sd"])
        fwd, bwd = (lambda x, t, y: dev.forward(x, t, y)), (lambda go: dev.dgrad(go))
    else:
        call = lc.VitCall(3)
        fwd_in, bwd_in = _dev(call.img), _dev(call.de * lc.oracle(call, seed)["sd"])
        fwd, bwd = (lambda img: dev.encode_image(img)), (lambda de: dev.dgrad(de))
    with nan_outputs():
        fwd(*fwd_in), bwd(*bwd_in)  # warm
        th.cuda.synchronize()
        o_ref, g_ref = fwd(*fwd_in).clone(), bwd(*bwd_in).clone()
        th.cuda.synchronize()
        s1, s2 = _two_streams()
        a, b = _staged(s1, fwd_in), _staged(s2, bwd_in)
        with th.cuda.stream(s1):
            o = fwd(*a)
        s2.wait_stream(s1)
        with th.cuda.stream(s2):
            gx = bwd(*b)
        s2.synchronize()  # s2 waited for s1
    tag = f"streams hand-over [{call.tag}]: forward on s1, dgrad on s2"
    ora = lc.oracle(call, seed)
    return [_flag(f"{tag}: forward bit-equal to the one-stream result", th.equal(o, o_ref)),
            _flag(f"{tag}: dgrad bit-equal to the one-stream result", th.equal(gx, g_ref)),
            rec(f"{tag}: forward vs the oracle", o, ora["fwd"]), rec(f"{tag}: dgrad vs the oracle", gx, ora["bwd"])]


def check_alternating():
    """The UNet on s1 and ViT-B/32 on s2, alternating over two rounds through ONE context (shared split-K workspace and fragment cache); the
    caller orders every pass behind the one before it with wait_stream.  Bit-equal to the same passes on the default stream."""
    prepare()
    ctx = pc._ctx(1)
    su, sv = lc.SEEDS["unet"][0], lc.SEEDS["vit"][0]
    unet, vit = lc._handle(ctx, "unet", su, lc.UNET_CASE), lc._handle(ctx, "vit", sv)
    cu, cv = lc.UNetCall(1, 64, 64, 0), lc.VitCall(3)
    uin = _dev(cu.x, cu.t, cu.y, cu.gout * lc.oracle(cu, su)["sd"])
    vin = _dev(cv.img, cv.de * lc.oracle(cv, sv)["sd"])

    def upass(x, t, y, go):
        return unet.forward(x, t, y), unet.dgrad(go)

    def vpass(img, de):
        return vit.encode_image(img), vit.dgrad(de)

    with nan_outputs():
        upass(*uin), vpass(*vin)
        th.cuda.synchronize()
        ref = [t.clone() for t in upass(*uin) + vpass(*vin)]
        th.cuda.synchronize()
        s1, s2 = _two_streams()
        a, b = _staged(s1, uin), _staged(s2, vin)
        got = []
        for _ in range(2):
            s1.wait_stream(s2)
            with th.cuda.stream(s1):
                ou = upass(*a)
            s2.wait_stream(s1)
            with th.cuda.stream(s2):
                ov = vpass(*b)
            got.append(ou + ov)
        s2.synchronize()
    names = ("unet forward", "unet dgrad", "vit forward", "vit dgrad")
    return [_flag(f"streams alternating, round {r}: {n} bit-equal to the default-stream pass", th.equal(t, ref[k]))
            for r, outs in enumerate(got) for k, (n, t) in enumerate(zip(names, outs))]


def check_records_across_streams():
    """parity_checks.check_gn_records' scheme, across streams: a cgd_op_conv3x3_wino_ex that leaves GroupNorm records (stats = 1) on s1,
    followed by cgd_op_gn_fwd of its output.  On s1 the norm merges the records; on s2, ordered behind s1 by an event, it must NOT (the
    records are served to the producing stream only: cgd_op_gn_record_merges stays put) and must still match float64."""
    import torch.nn.functional as F
    from cgd_amd import ops
    prepare()
    ctx = pc._ctx(1)
    lib = ctx.lib
    B, H, W, Ci, Cn = 2, 64, 64, 32, 128
    HW = H * W
    x, w, b = _dev(th.randn(B, H, W, Ci, generator=g(100)), th.randn(Cn, Ci, 3, 3, generator=g(101)) / math.sqrt(9 * Ci),
                   3.0 * th.randn(Cn, generator=g(102)))
    gamma, beta = _dev(1 + 0.1 * th.randn(Cn, generator=g(91)), 0.1 * th.randn(Cn, generator=g(92)))
    ww = ops.pack_conv3x3_wino(ctx, w)
    th.cuda.synchronize()
    merges = lambda: int(lib.cgd_op_gn_record_merges(ctx.h))  # noqa: E731
    out = []
    for same in (True, False):
        ctx.check(lib.cgd_op_new_pass(ctx.h))
        s1, s2 = _two_streams()
        with th.cuda.stream(s1):
            conv_y = th.full((B, HW, Cn), NAN, device=DEV)
            enqueue_delay()
            ctx.check(lib.cgd_op_conv3x3_wino_ex(ctx.h, x.data_ptr(), Ci, ww.data_ptr(), conv_y.data_ptr(), Cn, b.data_ptr(), None, 0, None, B, H, W,
                                                 Ci, Cn, 0, 1, None, 0, None, s1.cuda_stream))
            done = th.cuda.Event()
            done.record(s1)
        sn = s1 if same else s2
        if not same:
            s2.wait_event(done)
        m0 = merges()
        with th.cuda.stream(sn):
            scr = ops.gn_scratch(ctx, B, HW, Cn, DEV)
            y = th.full((B, HW, Cn), NAN, device=DEV)
            ctx.check(lib.cgd_op_gn_fwd(ctx.h, conv_y.data_ptr(), Cn, y.data_ptr(), Cn, B, HW, Cn, gamma.data_ptr(), beta.data_ptr(), None, 1, 1e-5,
                                        scr.data_ptr(), sn.cuda_stream))
        m1 = merges()
        sn.synchronize()
        where = "on the producing stream" if same else "on another stream, ordered by an event"
        out.append(_flag(f"streams gn records: GroupNorm {where} " + ("merges the conv's records" if same else "does not merge them"),
                         m1 == m0 + (1 if same else 0)))
        yref = F.silu(F.group_norm(conv_y.double().cpu().permute(0, 2, 1), 32, gamma.double().cpu(), beta.double().cpu(), 1e-5)).permute(0, 2, 1)
        out.append(rec(f"streams gn records: y {where} vs float64", y, yref.float()))
    return out


# ---- weight upload ------------------------------------------------------------------------------------------------------------------------
UPLOAD_KINDS = ("unet", "rn", "text")


def _upload_call(kind):
    return {"unet": lambda: lc.UNetCall(1, 64, 64, 0), "rn": lambda: lc.RnCall(2), "text": lambda: lc.TextCall(2)}[kind]()


def _forward_only(kind, ctx, dev, ins):
    if kind == "unet":
        return dev.forward(*ins)
    if kind == "rn":
        return dev.encode_image(*ins)
    out = th.empty(ins[0].shape[0], dev.out_dim, device=DEV)
    ctx.check(ctx.lib.cgd_text_forward(dev.h, ins[0].data_ptr(), ins[0].shape[0], out.data_ptr(), ctx.stream()))
    return out


def _forward_inputs(kind, call):
    if kind == "unet":
        return _dev(call.x, call.t, call.y)
    return _dev(call.img) if kind == "rn" else _dev(call.tok.to(th.int64))


def _cpu_sd(kind, seed):
    net = lc._oracle_net(kind, seed, lc.UNET_CASE if kind == "unet" else None)
    return {k: v.float() for k, v in net.state_dict().items() if "num_batches_tracked" not in k}


def _load(dev, kind, sd):
    return dev.load_state_dict(sd) if kind == "unet" else dev.load_clip_state_dict(sd)


def _fp16_exact(sd):
    """the weights rounded to fp16 (so that an fp16 state dict and its fp32 twin hold the same values)"""
    return {k: v.half().float() for k, v in sd.items()}


def check_upload(kind, dtype):
    """Inside th.cuda.stream(s), behind the delay: the state dict is built ON THE DEVICE ON THAT STREAM — as fp16, so that load_state_dict
    converts on the stream, or as fp32 written by a copy_ queued behind the delay —, then load_state_dict and a forward.  Bit-equal to a
    handle loaded from CPU tensors (warm=False: the upload may synchronise; only values are judged)."""
    prepare()
    seed = lc.SEEDS[kind][0]
    case_ = lc.UNET_CASE if kind == "unet" else None
    sd_cpu = _fp16_exact(_cpu_sd(kind, seed))
    call = _upload_call(kind)
    ins = _forward_inputs(kind, call)
    # the reference handle lives in a context of its own: in a shared one its packed weights would sit in the fragment cache, and the
    # hipFree that clears the cache at the first set_param would drain the device by accident
    ctx_ref, ctx = pc._ctx(1), pc._ctx(1)
    ref_dev = lc._new_handle(ctx_ref, kind, case_)
    _load(ref_dev, kind, sd_cpu)
    with nan_outputs():
        ref = _forward_only(kind, ctx_ref, ref_dev, ins).clone()
    th.cuda.synchronize()
    src = {k: v.to(DEV) for k, v in sd_cpu.items()}  # complete device sources for the copies below
    th.cuda.synchronize()
    dev = lc._new_handle(ctx, kind, case_)
    s = th.cuda.Stream()
    with th.cuda.stream(s), nan_outputs():
        sd = {k: th.full(v.shape, NAN, device=DEV, dtype=dtype) for k, v in src.items()}
        enqueue_delay()
        for k in sd:
            sd[k].copy_(src[k])  # fp32 -> fp16 converts exactly: the values are fp16 numbers
        _load(dev, kind, sd)
        out = _forward_only(kind, ctx, dev, ins)
        s.synchronize()
    name = str(dtype).replace("torch.", "")
    return [_flag(f"streams upload [{kind}, {name} state dict built on the stream behind the delay]: forward bit-equal to the handle loaded "
                  f"from CPU tensors (NaN in it: {bool(th.isnan(out).any())})", th.equal(out, ref))]


def check_reupload_in_flight(kind="unet", source="device"):
    """The delay, a forward with the seed-1 weights into a NaN-filled output, and IMMEDIATELY load_state_dict with seed 2 (a state dict on
    the device, or on the CPU): the forward's output equals the seed-1 control bit for bit (the upload must not overtake the pass in
    flight), a forward after the upload the seed-2 control."""
    prepare()
    s1, s2 = lc.SEEDS[kind]
    case_ = lc.UNET_CASE if kind == "unet" else None
    call = _upload_call(kind)
    ins = _forward_inputs(kind, call)
    ctx = pc._ctx(1)
    sd1, sd2 = _cpu_sd(kind, s1), {k: (v.to(DEV) if source == "device" else v) for k, v in _cpu_sd(kind, s2).items()}
    refs = []
    dev = lc._new_handle(ctx, kind, case_)
    with nan_outputs():
        for sd in (sd1, sd2):
            _load(dev, kind, sd)
            refs.append(_forward_only(kind, ctx, dev, ins).clone())
        th.cuda.synchronize()
        _load(dev, kind, sd1)
        _forward_only(kind, ctx, dev, ins)  # warm with seed 1
        th.cuda.synchronize()
        s = th.cuda.Stream()
        with th.cuda.stream(s):
            st = _staged(s, ins)
            o1 = _forward_only(kind, ctx, dev, st)
            _load(dev, kind, sd2)
            o2 = _forward_only(kind, ctx, dev, st)
            s.synchronize()
    tag = f"streams re-upload in flight [{kind}, {source} state dict]"
    return [_flag(f"{tag}: the forward in flight kept the seed-1 weights", th.equal(o1, refs[0])),
            _flag(f"{tag}: the forward after the upload runs the seed-2 weights", th.equal(o2, refs[1]))]


# ---- a whole run ----------------------------------------------------------------------------------------------------------------------------
def check_guided_run():
    """The `mini` scene of step_checks.Scenario, three guided DDIM steps with the native ClipGuidance, entirely under a created stream with one
    delay in front of the first step: x_(t-1), pred_xstart, g and the loss scalars are bit-equal to the default-stream run on fresh objects.
    While the streamed run goes, the scenario's per-step th.cuda.synchronize() is the STREAM's synchronize: nothing synchronises the device.
    `early` (the stream still had work pending when the step's host code was through) is recorded per step and reported, not asserted: the
    sampler uploads its taped draws and the plugin surface reads t on the host."""
    from tests import step_checks as stc
    prepare()

    def snap(it):
        out = []
        for o, guid, legs in it:
            out.append(({k: v.clone() for k, v in o.items() if th.is_tensor(v)}, stc._FrozenLog(guid.log()), legs))
        return out

    scn = stc.Scenario("mini", ddim=True, steps=3)
    plain = snap(scn.run_device(1))
    th.cuda.synchronize()
    s = th.cuda.Stream()
    early = []
    device_sync = th.cuda.synchronize

    def stream_sync(*a, **k):
        early.append(not s.query())
        s.synchronize()

    th.cuda.synchronize = stream_sync
    try:
        with th.cuda.stream(s):
            enqueue_delay()
            streamed = snap(scn.run_device(1))
            s.synchronize()
    finally:
        th.cuda.synchronize = device_sync
    _STATE["guided_run_early"] = early
    recs = [_flag(f"streams guided run: {len(streamed)} steps ran, early per step {early}", len(streamed) == len(plain) == 3)]
    for k, ((o_s, log_s, legs_s), (o_p, log_p, legs_p)) in enumerate(zip(streamed, plain)):
        for name in ("sample", "pred_xstart"):
            recs.append(_flag(f"streams guided run: step {k} {name} bit-equal to the default-stream run", th.equal(o_s[name], o_p[name])))
        recs.append(_flag(f"streams guided run: step {k} g bit-equal to the default-stream run",
                          legs_s is not None and legs_p is not None and th.equal(legs_s["g"], legs_p["g"])))
        a, b = log_s.log(), log_p.log()
        same = len(b) > 0 and a.keys() == b.keys() and all(a[key] == b[key] or (math.isnan(a[key]) and math.isnan(b[key])) for key in b)
        recs.append(_flag(f"streams guided run: step {k} loss scalars equal to the default-stream run", same))
    return recs
