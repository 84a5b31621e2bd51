"""CPU test of the complete host sequence of the `GuidedSampler` loops when features combine: every C-ABI call with its arguments, every
model and cond_fn call, every random draw and every yield, in order, against `tests/golden/sampler_trace.json`.  The fixture is a recorded
result of this project's own code (`python -m tests.test_sampler_trace_host --write`, written before the sampler's host code was
restructured); the other `test_*_host.py` files pin selected arguments of their own feature, this one the whole sequence.

A call is stored as its name and its arguments after the context handle, typed by `lib._SIGS`: ints and floats as they are, coefficient
structs as field dicts, pointer arrays as null / non-null per entry, a pointer as None or as its alias class inside that call ("p0", "p1",
... by first appearance), tagged "=sample" / "=pred_xstart" when it is the tensor of that name of the previous yield.  No address is stored.
Everything compares exactly except floats (rel 1e-6, as tests/test_dpm_host.py compares the same coefficient structs: they pass through
math.exp / log on the host and may differ in the last place between machines).  All twelve cases are kept: no existing test pins a complete
sequence."""
import ctypes as C
import json
import os
import sys
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from cgd_amd import guidance as dg
from cgd_amd import lib as L
from cgd_amd import sampler
from tests.test_ops_wrappers import _RecordingLib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_trace.json")
SHAPE = (2, 3, 4, 8)
SIZE_QUERIES = ("cgd_ilvr_scratch_floats", "cgd_abs_quantile_scratch_bytes")


class _Trace:
    """the events of one loop in canonical form; `last` holds the previous yield (alive, so that its addresses stay its own)"""

    def __init__(self):
        self.events, self.last = [], {}

    def pointer(self, v, classes):
        v = getattr(v, "value", v)  # a c_void_p entry of a pointer array
        if v is None:
            return None
        name = classes.setdefault(v, f"p{len(classes)}")
        tags = [k for k in ("sample", "pred_xstart") if k in self.last and self.last[k].data_ptr() == v]
        return name + "".join("=" + t for t in tags)

    def call(self, name, args):
        argtypes = L._SIGS[name][1][1:]
        assert len(args) == len(argtypes) + 1, name  # the context handle comes first
        classes, out = {}, []
        for v, t in zip(args[1:], argtypes):
            if t is L.vp:
                out.append(self.pointer(v, classes))
            elif t in (L.i32, L.i64, C.c_long):
                assert isinstance(v, int) and not isinstance(v, bool), (name, v)
                out.append(v)
            elif t is L.f32:
                out.append(float(v))
            elif v is None:
                out.append(None)
            elif t._type_ is L.vp:  # C.POINTER(c_void_p): an array of pointers
                out.append({"ptrs": [p is not None for p in v]})
            else:  # a pointer to a coefficient struct: the struct itself is passed
                assert isinstance(v, t._type_), (name, v)
                out.append({"struct": {f: getattr(v, f) for f, _ in v._fields_}})
        self.events.append(["call", name, out])


class _TraceLib(_RecordingLib):
    """`_RecordingLib` whose calls also go to the trace as they happen (the tables hand out coefficient structs the host may write to
    afterwards), and whose two scratch-size queries return a size"""

    def __init__(self, trace):
        super().__init__()
        self.trace = trace

    def __getattr__(self, name):
        record = super().__getattr__(name)

        def fn(*args):
            record(*args)
            if name in SIZE_QUERIES:
                return 16
            self.trace.call(name, args)
            return 0
        return fn


def _rig(spec):
    trace = _Trace()
    ctx = types.SimpleNamespace(lib=_TraceLib(trace), h=1, check=lambda rc: None, device=0, stream=lambda: 0)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", spec, False))
    guid = object.__new__(dg.ClipGuidance)
    guid.use_magnitude, guid.scalars, guid.current_timestep = True, th.zeros(8), smp.num_timesteps - 1

    def native(x, x0, x_in, coef):
        trace.events.append(["cond_fn", guid.current_timestep, coef.fac])
        return th.ones_like(x)

    guid.native = native

    def forward(x, ts, y, out=None):
        trace.events.append(["forward", float(ts[0]), None if y is None else y.tolist()])
        return out

    model = types.SimpleNamespace(forward=forward, num_classes=5)
    plain = smp._draw_like

    def draw(x):
        trace.events.append(["draw", list(x.shape)])
        return plain(x)

    smp._draw_like = draw
    return smp, guid, model, trace


def _drain(gen, trace, guid=None):
    for out in gen:
        trace.events.append(["yield", sorted(out)])
        trace.last = out
        if guid is not None:
            guid.current_timestep -= 1
    return {"events": trace.events, "end": float(th.rand(1))}


def _mask():
    mask = th.zeros(1, 1, 4, 8)
    mask[..., :3] = 1.0
    return mask


def _run(loop, spec, plugin=False, tape=False, **kw):
    smp, guid, model, trace = _rig(spec)
    th.manual_seed(7)
    gen = th.Generator().manual_seed(17)  # the inputs, apart from the global generator the loop draws from
    if "mask" in kw or tape:
        kw.update(mask=_mask(), init_image=th.rand(SHAPE, generator=gen))
    if "ilvr" in kw:
        kw["ilvr"] = (th.rand(SHAPE, generator=gen),) + kw["ilvr"]
    if tape:
        evals = 2 * (smp.num_timesteps - 1) + 1  # resamples = 2: every step index > 0 runs twice
        smp.tape = {"x_T": th.randn(SHAPE, generator=gen), "noise": [th.randn(SHAPE, generator=gen) for _ in range(evals)],
                    "y": [th.randint(0, 5, (2,), generator=gen) for _ in range(smp.num_timesteps)],
                    "known_noise": [th.randn(SHAPE, generator=gen) for _ in range(evals)],
                    "renoise": [th.randn(SHAPE, generator=gen) for _ in range(smp.num_timesteps - 1)]}
        kw["resamples"] = 2
    cond_fn = guid
    if plugin:
        # the generic plug-in branch: a plain Python cond_fn, a model called as model(x, ts, y) whose output is differentiable in x
        def model(x, ts, y):  # noqa: F811
            trace.events.append(["forward", float(ts[0]), None if y is None else y.tolist()])
            return th.cat([0.5 * x, th.zeros_like(x)], dim=1)

        model.num_classes = 5

        def cond_fn(x, t, out, y=None):
            trace.events.append(["cond_fn", t.tolist(), sorted(out)])
            return -th.autograd.grad(out["pred_xstart"].sum(), x)[0]

        guid = None
    loop = getattr(smp, loop + "_sample_loop_progressive")
    return _drain(loop(model, SHAPE, clip_denoised=False, cond_fn=cond_fn, model_kwargs={"y": th.zeros(2, dtype=th.long)}, device="cpu",
                       randomize_class=True, cond_fn_with_grad=True, **kw), trace, guid)


def _run_reverse():
    smp, _, model, trace = _rig("ddim6")
    th.manual_seed(7)
    image = th.rand(SHAPE, generator=th.Generator().manual_seed(17))
    return _drain(smp.ddim_reverse_sample_loop_progressive(model, image, model_kwargs={"y": th.ones(2, dtype=th.long)}, device="cpu"), trace)


CASES = {
    "p": lambda: _run("p", "6"),
    "p_mask_resamples2_skip1": lambda: _run("p", "6", mask=True, resamples=2, skip_timesteps=1),
    "ddim_eta0": lambda: _run("ddim", "ddim6"),
    "ddim_eta0.5_ilvr2_stop2": lambda: _run("ddim", "ddim6", eta=0.5, ilvr=(2, 2)),
    "plms4_mask": lambda: _run("plms", "ddim6", order=4, mask=True),
    "plms1": lambda: _run("plms", "ddim6", order=1),
    "dpm2_threshold": lambda: _run("dpmpp", "dpm6", order=2, threshold=(0.99, 2.0)),
    "dpm2_eta1_ilvr4": lambda: _run("dpmpp", "dpm6", order=2, eta=1, ilvr=(4,)),
    "dpm1_mask": lambda: _run("dpmpp", "dpm6", order=1, mask=True),
    "p_plugin": lambda: _run("p", "6", plugin=True),
    "p_tape_mask_resamples2": lambda: _run("p", "6", tape=True),
    "ddim_reverse": _run_reverse,
}


def _same(got, want, where):
    """exact, except floats: rel 1e-6"""
    assert type(got) is type(want), where
    if isinstance(want, dict):
        assert list(got) == list(want), where
        for k in want:
            _same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, list):
        assert len(got) == len(want), where
        for n, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{n}]")
    elif isinstance(want, float):
        assert got == pytest.approx(want, rel=1e-6, abs=0.0), where
    else:
        assert got == want, where


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_exactly_the_cases(recorded):
    assert list(recorded) == list(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_loop_issues_the_recorded_sequence(case, recorded):
    got = json.loads(json.dumps(CASES[case]()))  # through JSON, as the fixture went
    want = recorded[case]
    assert got["end"] == want["end"], "the generator's state after the loop: something else was drawn"
    assert [e[:2] for e in got["events"]] == [e[:2] for e in want["events"]]  # names and order first: the readable failure
    _same(got["events"], want["events"], case)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python -m tests.test_sampler_trace_host --write")
    with open(FIXTURE, "w") as f:
        json.dump({name: run() for name, run in CASES.items()}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes")
