"""GPU tests of windowed sampling.  Op level: cgd_window_gather / cgd_window_merge against the restatement of tests/window_ref.py (fp64 for
the weighted cases, at the criterion tests/test_gpu_tail.py applies to its elementwise kernels: parity_checks.rec's literal
|a - b| <= 1e-4 + 1e-3 |ref|; bit for bit for the unweighted gather), their fixed summation order, the scalar path and the refusals.  Model
level: nets.WindowedUNet against window_ref.WindowedRef around the oracle UNet, forward and dgrad.  Trajectory level: the native guided
sampler with the wrapper against the oracle loops with WindowedRef on the `mini` scene of tests/step_checks.py (same tape, same records and
criterion as step_checks.compare), every loop, a masked and an ILVR step on a windowed frame, and the drop-in generator with '+windows='."""
import ctypes as C
import itertools
import os

import pytest
import torch as th

from tests import parity_checks as pc
from tests import step_checks
from tests import window_ref as wr

pytestmark = pytest.mark.gpu

DEV = pc.DEV
S_OP = 16
# (H, W, stride, wrap) at window side 16: the flush-last rule on both axes; wrap on both axes (16 windows); a wrapping axis of the window's length
OP_PLANS = [(40, 24, 16, ""), (32, 32, 8, "xy"), (16, 32, 8, "y")]
WRAP_BITS = {"": 0, "x": 1, "y": 2, "xy": 3}


def _assert_all(recs):
    for r in recs:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3e}")
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


def _same_bits(a, b):
    return a.shape == b.shape and th.equal(a.contiguous().view(th.int32), b.contiguous().view(th.int32))


# ---- op level --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def op_rig():
    from cgd_amd import lib as L
    return L.Context(0, 1), L


def _dev(t, offset=False):
    """the tensor on the device; `offset`: as a contiguous view that starts one float into its allocation (4-byte aligned only)"""
    if t is None:
        return None
    if not offset:
        return t.to(DEV).contiguous()
    flat = th.empty(t.numel() + 1, device=DEV)
    flat[1:].copy_(t.reshape(-1))
    view = flat[1:].view(t.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


class _Plan:
    def __init__(self, H, W, stride, wrap, S=S_OP):
        self.H, self.W, self.S, self.wrap = H, W, S, WRAP_BITS[wrap]
        self.oy, self.ox = wr.origins(H, S, stride, "y" in wrap), wr.origins(W, S, stride, "x" in wrap)
        self.n = len(self.oy) * len(self.ox)

    def tables(self, profile):
        """the fp32 tables the kernel reads (the restatement's, rounded); None for the unweighted pair"""
        if profile is None:
            return None, None
        return wr.tables(self.oy, self.H, self.S, profile).float(), wr.tables(self.ox, self.W, self.S, profile).float()


def _ints(v):
    return (C.c_int * len(v))(*v)


def _gather(rig, p, full, win, ay, ax, B, Cn):
    ctx, L = rig
    return ctx.lib.cgd_window_gather(ctx.h, full.data_ptr(), win.data_ptr(), _ints(p.oy), len(p.oy), _ints(p.ox), len(p.ox), L.ptr(ay), L.ptr(ax),
                                     B, Cn, p.H, p.W, p.S, p.wrap, ctx.stream())


def _merge(rig, p, win, full, ay, ax, B, Cn, accumulate):
    ctx, L = rig
    return ctx.lib.cgd_window_merge(ctx.h, win.data_ptr(), full.data_ptr(), _ints(p.oy), len(p.oy), _ints(p.ox), len(p.ox), L.ptr(ay), L.ptr(ax),
                                    B, Cn, p.H, p.W, p.S, p.wrap, int(accumulate), ctx.stream())


def _op_case(rig, p, B, Cn, profile, gen, offset=False):
    """gather, merge with accumulate 0 and 1 (each launched twice: same bits), and merge(gather(x)) under the normalised weights"""
    ctx, _ = rig
    tag = f"{p.H}x{p.W} wrap{p.wrap} B{B} C{Cn} {profile or 'ones'}{' offset' if offset else ''}"
    ay, ax = p.tables(profile)
    d_ay, d_ax = _dev(ay, offset), _dev(ax, offset)
    ay64, ax64 = (None, None) if ay is None else (ay.double(), ax.double())
    full = th.randn(B, Cn, p.H, p.W, generator=gen)
    win = th.randn(B * p.n, Cn, p.S, p.S, generator=gen)
    recs = []
    # gather
    d_win = _dev(th.full(win.shape, float("nan")), offset)
    ctx.check(_gather(rig, p, _dev(full, offset), d_win, d_ay, d_ax, B, Cn))
    got = d_win.cpu()
    if profile is None:
        assert _same_bits(got, wr.gather(full, p.oy, p.ox, p.S)), f"gather {tag}: a copy keeps every bit"
    else:
        recs.append(pc.rec(f"gather {tag}", got, wr.gather(full.double(), p.oy, p.ox, p.S, ay64, ax64)))
    # merge
    base = th.randn(B, Cn, p.H, p.W, generator=gen)
    for acc in (0, 1):
        runs = []
        for _ in range(2):
            d_full = _dev(base if acc else th.full(base.shape, float("nan")), offset)
            ctx.check(_merge(rig, p, _dev(win, offset), d_full, d_ay, d_ax, B, Cn, acc))
            runs.append(d_full.cpu())
        assert _same_bits(*runs), f"merge {tag} acc{acc}: two launches, the same bits"
        recs.append(pc.rec(f"merge {tag} acc{acc}", runs[0], wr.merge(win.double(), p.oy, p.ox, p.H, p.W, ay64, ax64, base.double() if acc else None)))
    # merge(gather(x)) = x when the merge carries normalised weights
    if profile == "uniform":
        d_back = _dev(th.full(full.shape, float("nan")), offset)
        ctx.check(_gather(rig, p, _dev(full, offset), d_win, None, None, B, Cn))
        ctx.check(_merge(rig, p, d_win, d_back, d_ay, d_ax, B, Cn, 0))
        recs.append(pc.rec(f"merge(gather(x)) {tag}", d_back.cpu(), full.double()))
    return recs


@pytest.mark.parametrize("H,W,stride,wrap", OP_PLANS)
def test_window_pair_matches_the_restatement(op_rig, H, W, stride, wrap):
    p = _Plan(H, W, stride, wrap)
    assert (p.oy, p.ox) == {(40, 24): ([0, 16, 24], [0, 8]), (32, 32): ([0, 8, 16, 24],) * 2, (16, 32): ([0, 8], [0, 8, 16])}[(H, W)]
    gen = th.Generator().manual_seed(H * 100 + W)
    recs = []
    for B, Cn, profile in itertools.product((1, 2), (3, 6), (None, "uniform", "feather")):
        recs += _op_case(op_rig, p, B, Cn, profile, gen)
    _assert_all(recs)


def test_window_pair_on_pointers_offset_by_one_float(op_rig):
    """every pointer, the tables included, only 4-byte aligned: the scalar path"""
    gen = th.Generator().manual_seed(77)
    recs = []
    for (H, W, stride, wrap), profile in zip(OP_PLANS, ("feather", "uniform", None)):
        recs += _op_case(op_rig, _Plan(H, W, stride, wrap), 2, 3, profile, gen, offset=True)
    _assert_all(recs)


def test_window_merge_sums_in_window_order_and_gather_is_its_adjoint_on_the_device(op_rig):
    """the fixed order, ky ascending outside and kx ascending inside: under wrap on both axes a pixel is covered by four windows, and the
    fp32 sum ((w00 + w01) + w10) + w11 is reproduced bit for bit; <merge(w), f> = <w, gather(f)> with the device's own results"""
    ctx, _ = op_rig
    p = _Plan(32, 32, 8, "xy")
    gen = th.Generator().manual_seed(9)
    B, Cn = 1, 3
    win = th.randn(B * p.n, Cn, p.S, p.S, generator=gen)
    d_full = _dev(th.full((B, Cn, 32, 32), float("nan")))
    ctx.check(_merge(op_rig, p, _dev(win), d_full, None, None, B, Cn, 0))
    expect = th.zeros(B, Cn, 32, 32)
    first = th.ones(32, 32, dtype=th.bool)
    for ky, o_y in enumerate(p.oy):
        rows = (o_y + th.arange(p.S)) % 32
        for kx, o_x in enumerate(p.ox):
            cols = (o_x + th.arange(p.S)) % 32
            canvas = th.zeros_like(expect)
            canvas[:, :, rows[:, None], cols[None, :]] = win[ky * len(p.ox) + kx][None]
            expect = expect + canvas  # fp32, one rounded add per covering window, in window order (adding an exact 0 elsewhere changes nothing)
            first[rows[:, None], cols[None, :]] = False
    assert not first.any() and _same_bits(d_full.cpu() + 0.0, expect + 0.0)  # (+ 0.0: a sum that is exactly zero may carry either sign)
    ay, ax = p.tables("feather")
    f = th.randn(B, Cn, 32, 32, generator=gen)
    d_m, d_g = _dev(th.empty_like(f)), _dev(th.empty_like(win))
    ctx.check(_merge(op_rig, p, _dev(win), d_m, _dev(ay), _dev(ax), B, Cn, 0))
    ctx.check(_gather(op_rig, p, _dev(f), d_g, _dev(ay), _dev(ax), B, Cn))
    lhs, rhs = (d_m.cpu().double() * f.double()).sum(), (win.double() * d_g.cpu().double()).sum()
    # each side is a sum of products rounded to fp32: relative 2^-23 per weighted term (two products), against the sum of magnitudes
    bound = 4 * 2.0 ** -23 * float((wr.merge(win.double().abs(), p.oy, p.ox, 32, 32, ay.double(), ax.double()) * f.double().abs()).sum())
    assert abs(float(lhs - rhs)) <= bound and abs(float(lhs)) > 1e-3


def test_window_pair_refuses_bad_arguments_and_launches_nothing(op_rig):
    ctx, L = op_rig
    buf = th.zeros(1 << 16, device=DEV)
    ptr = buf.data_ptr()
    good = dict(full=ptr, win=ptr, oy=[0, 16, 24], ox=[0, 8], ay=None, ax=None, B=2, Cn=3, H=40, W=24, S=16, wrap=0)

    def call(which, **kw):
        a = {**good, **kw}
        oy = None if a["oy"] is None else _ints(a["oy"])
        ox = None if a["ox"] is None else _ints(a["ox"])
        ny = a.get("ny", 0 if a["oy"] is None else len(a["oy"]))
        nx = a.get("nx", 0 if a["ox"] is None else len(a["ox"]))
        if which == "gather":
            return ctx.lib.cgd_window_gather(ctx.h, a["full"], a["win"], oy, ny, ox, nx, a["ay"], a["ax"], a["B"], a["Cn"], a["H"], a["W"], a["S"],
                                             a["wrap"], ctx.stream())
        return ctx.lib.cgd_window_merge(ctx.h, a["win"], a["full"], oy, ny, ox, nx, a["ay"], a["ax"], a["B"], a["Cn"], a["H"], a["W"], a["S"],
                                        a["wrap"], 1, ctx.stream())

    bad = [dict(S=12, oy=[0, 12, 24, 28], ox=[0, 12]), dict(H=44, oy=[0, 16, 28]), dict(W=20, ox=[0, 4]),  # S, H, W: multiples of 8
           dict(oy=[0, 12, 24]), dict(ox=[0, 4, 8]),                                                     # ... and every origin
           dict(S=48, oy=[0], ox=[0]), dict(S=32, oy=[0, 8], ox=[0]),                                    # S <= H, S <= W
           dict(oy=[0, 16, 40]), dict(oy=[-8, 0, 16, 24]), dict(ox=[0, 8, 24]),                          # origins in range
           dict(oy=[0, 16, 32]), dict(ox=[0, 16]), dict(ox=[0, 16], wrap=2),                             # no wrap: o + S <= L (wrap on the other axis does not help)
           dict(oy=[0, 24]), dict(ox=[8]), dict(H=48, oy=[0, 32], wrap=2),                               # an uncovered pixel, with and without wrap
           dict(oy=[], ny=0), dict(ox=list(range(0, 136, 8)), W=136 + 8),                                # 1 <= ny, nx <= 16
           dict(oy=[0] * 17),
           dict(H=65536, W=65536), dict(S=65536, H=65536, W=65536, oy=[0], ox=[0]),                      # planes below 2^31
           dict(full=None), dict(win=None), dict(oy=None, ny=3), dict(ox=None, nx=2),                    # required pointers
           dict(ay=ptr), dict(ax=ptr),                                                                   # the tables come as a pair
           dict(B=0), dict(Cn=0), dict(H=0), dict(W=-8), dict(S=0), dict(wrap=4)]
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    for kw in bad:
        for which in ("gather", "merge"):
            assert call(which, **kw) == -2 and ctx.lib.cgd_last_error(ctx.h), (which, kw)
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before, "a refused call launched a kernel"
    # the same arguments with nothing wrong are accepted (one launch each); so are 16 windows along an axis and a wrapping window
    big = th.zeros(2 * 3 * 16 * 16 * 16 * 2, device=DEV)
    for which in ("gather", "merge"):
        assert call(which, win=big.data_ptr()) == 0
        assert call(which, win=big.data_ptr(), ay=ptr, ax=ptr) == 0
        assert call(which, win=big.data_ptr(), W=128, ox=list(range(0, 128, 8)), wrap=1, B=1, H=16, oy=[0]) == 0
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before + 6
    th.cuda.synchronize()


# ---- model level -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unet_pair():
    ctx = pc._ctx(1)
    ref, dev = pc.build_unet_pair(ctx, "mini")
    return ctx, ref, dev


@pytest.mark.parametrize("H,W,wrap,feather,B", [(48, 64, "", False, 1), (32, 64, "x", True, 2)])
def test_windowed_unet_forward_and_dgrad_match_the_windowed_oracle(unet_pair, H, W, wrap, feather, B):
    """frame 48 x 64 at stride 16: six windows (origins 0, 16 by 0, 16, 32); frame 32 x 64 with wrapx: four, the last one over the edge"""
    from cgd_amd import nets
    ctx, ref, dev = unet_pair
    wdev = nets.WindowedUNet(dev, 16, wrap, feather)
    wref = wr.WindowedRef(ref, 32, 16, wrap, feather)
    plan = wdev.plan(H, W)
    assert (plan.oy, plan.ox) == wref.plan(H, W)[:2] and plan.n == (6 if H == 48 else 4)
    x = th.randn(B, 3, H, W, generator=pc.g(60))
    t = th.tensor([417.0, 36.0][:B])
    y = th.randint(0, 10, (B,), generator=pc.g(61))
    gout = th.randn(B, 6, H, W, generator=pc.g(62))
    gout[:, 3:] = 0  # the guidance only seeds the epsilon channels
    xr = x.clone().requires_grad_()
    o = wref(xr, t, y)
    (o * gout).sum().backward()
    sd = pc.unit_seed(xr.grad)
    od = wdev.forward(x.to(DEV), t.to(DEV), y.to(DEV))
    gx = wdev.dgrad((gout * sd).to(DEV))
    # the autograd node over the wrapper gives the same gradient
    xa = x.to(DEV).requires_grad_()
    (wdev(xa, t.to(DEV), y.to(DEV)) * (gout * sd).to(DEV)).sum().backward()
    th.cuda.synchronize()
    tag = f"windowed unet[mini B{B} {H}x{W} wrap'{wrap}'{' feather' if feather else ''}]"
    _assert_all([pc.rec(f"{tag} forward", od, o.detach()), pc.rec(f"{tag} dgrad", gx, xr.grad * sd),
                 pc.rec(f"{tag} autograd", xa.grad, xr.grad * sd)])


def test_a_single_window_equal_to_the_frame_is_the_bare_forward_bit_for_bit(unet_pair):
    from cgd_amd import nets
    ctx, ref, dev = unet_pair
    x = th.randn(2, 3, 32, 32, generator=pc.g(63)).to(DEV)
    t, y = th.tensor([417.0, 3.0], device=DEV), th.tensor([1, 8], device=DEV)
    bare = dev.forward(x, t, y).clone()
    for feather in (False, True):
        wdev = nets.WindowedUNet(dev, 16, "", feather)
        assert wdev.plan(32, 32).n == 1
        got = wdev.forward(x, t, y)
        th.cuda.synchronize()
        assert _same_bits(got.cpu(), bare.cpu())
    assert th.isfinite(bare).all() and float(bare.abs().max()) > 1e-2


def test_the_wrapper_keeps_the_surface_the_sampler_uses_and_refuses_the_rest(unet_pair):
    from cgd_amd import nets
    ctx, ref, dev = unet_pair
    w = nets.WindowedUNet(dev, 16, "x")
    assert w.ctx is ctx and (w.num_classes, w.in_channels, w.out_channels) == (10, 3, 6) and w.cfg is dev.cfg
    assert not hasattr(w, "embed") and not hasattr(w, "forward_slot")  # EmbedAhead stays off
    with pytest.raises(ValueError):
        w.set_low_res(th.zeros(1, 3, 8, 8))
    for kw in (dict(stride=12), dict(stride=40), dict(stride=0), dict(stride=16, wrap="z"), dict(stride=16, window=16)):
        with pytest.raises(ValueError):
            nets.WindowedUNet(dev, **kw)
    assert nets.WindowedUNet(dev, 16, window=32).window == 32
    for shape in ((1, 3, 32, 72), (1, 3, 36, 64), (1, 3, 16, 64)):  # wrap: 72 % 16; a side that is no multiple of 8; a frame below the window
        with pytest.raises(ValueError):
            w.forward(th.zeros(shape, device=DEV), th.zeros(1, device=DEV), th.zeros(1, dtype=th.long, device=DEV))
    with pytest.raises(RuntimeError):
        nets.WindowedUNet(dev, 16).dgrad(th.zeros(1, 6, 32, 64, device=DEV))


# ---- trajectory level ------------------------------------------------------------------------------------------------------------------
STRIDE, WRAP = 16, "x"


class WindowedScenario(step_checks.Scenario):
    """step_checks' scene with the model wrapped on both sides: WindowedRef around the oracle UNet, nets.WindowedUNet around the device's"""

    def __init__(self, feather=False, **kw):
        super().__init__("mini", hw=(32, 64), **kw)
        self.feather = feather
        self.bare_unet = self.ref_unet
        self.ref_unet = wr.WindowedRef(self.bare_unet, 32, STRIDE, WRAP, feather)

    def _make_device(self, precision):
        from cgd_amd import nets
        wrapped, self.ref_unet = self.ref_unet, self.bare_unet  # the handle loads the bare module's state dict
        try:
            ctx, unet, *rest = super()._make_device(precision)
        finally:
            self.ref_unet = wrapped
        return (ctx, nets.WindowedUNet(unet, STRIDE, WRAP, self.feather), *rest)


@pytest.mark.parametrize("ddim", [False, True])
def test_windowed_guided_trajectory_matches_the_oracle(ddim):
    """two guided steps (p_sample) / one (DDIM) at 32 x 64, four windows of which one runs over the right edge: sample, pred_xstart, g and
    its legs (g_unet is the wrapper's dgrad) and the loss scalars, as step_checks.compare grades every scene"""
    sc = WindowedScenario(ddim=ddim, steps=1 if ddim else 2)
    recs = step_checks.compare(sc, 1, sc.run_oracle(), sc.run_device(1))
    assert any("g_unet" in r["name"] for r in recs)
    _assert_all(recs)


@pytest.fixture(scope="module")
def loop_rig():
    sc = WindowedScenario(feather=True, steps=1)
    ctx, wunet, clip, _, _, smp = sc._make_device(1)
    return sc, ctx, wunet, clip


def _run_loop(rig, kind, steps=1, **extra):
    """`steps` yields of one of the four loops with the wrapper and native guidance, untaped; [(sample, pred_xstart)] on the host"""
    from cgd_amd import diffusion as dd
    from cgd_amd import guidance as dg
    from cgd_amd import sampler
    sc, ctx, wunet, clip = rig
    spec = {"p": "50", "ddim": "ddim50", "plms": "ddim50", "dpm": "dpm8"}[kind]
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", spec))
    cgs, tvs, rs = sc.scales
    cond = dg.ClipGuidance(ctx, wunet, clip, smp, sc.targets.to(DEV), sc.w, sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs, range_scale=rs)
    cond.current_timestep = smp.num_timesteps // 4
    th.manual_seed(11)
    shape = (sc.B, 3, sc.H, sc.W)
    kw = dict(clip_denoised=False, cond_fn=cond, model_kwargs={"y": th.zeros(sc.B, dtype=th.long, device=DEV)}, device=DEV,
              skip_timesteps=smp.num_timesteps - 1 - smp.num_timesteps // 4, init_image=sc.x0_star.expand(sc.B, -1, -1, -1).to(DEV),
              randomize_class=True, cond_fn_with_grad=True, **extra)
    loop = {"p": smp.p_sample_loop_progressive, "ddim": smp.ddim_sample_loop_progressive, "plms": smp.plms_sample_loop_progressive,
            "dpm": smp.dpmpp_sample_loop_progressive}[kind]
    out = []
    for o in itertools.islice(loop(wunet, shape, **kw), steps):
        th.cuda.synchronize()
        out.append((o["sample"].cpu(), o["pred_xstart"].cpu()))
        cond.current_timestep -= 1
    assert cond.calls >= steps
    return out


@pytest.mark.parametrize("kind", ["ddim", "plms", "dpm"])
def test_each_loop_steps_with_the_wrapper(loop_rig, kind):
    """(PLMS: the start step, two windowed evaluations; DPM-Solver++: with dynamic thresholding, which sees the whole frame)"""
    extra = {"threshold": 0.995} if kind == "dpm" else {}
    (sample, x0), = _run_loop(loop_rig, kind, **extra)
    assert tuple(sample.shape) == (1, 3, 32, 64) and th.isfinite(sample).all() and th.isfinite(x0).all()
    assert float(sample.abs().max()) > 1e-2 and not th.equal(sample, x0)


def test_a_masked_and_an_ilvr_step_run_on_a_windowed_frame(loop_rig):
    sc = loop_rig[0]
    mask = th.zeros(1, 1, 32, 64)
    mask[..., 24:56] = 1.0  # regenerated: a band that the wrapping window covers too
    (sample, x0), = _run_loop(loop_rig, "ddim", mask=mask.to(DEV))
    assert th.isfinite(sample).all() and th.isfinite(x0).all()
    assert th.equal(x0[..., :24], sc.x0_star[..., :24]) and not th.equal(x0[..., 24:56], sc.x0_star[..., 24:56])  # kept / regenerated
    ref = th.tanh(th.randn(1, 3, 32, 64, generator=pc.g(5)))
    (plain, _), = _run_loop(loop_rig, "p")
    (sample, x0), = _run_loop(loop_rig, "p", ilvr=(ref.to(DEV), 4, 0))
    assert th.isfinite(sample).all() and th.isfinite(x0).all() and not th.equal(sample, plain)


# ---- drop-in ---------------------------------------------------------------------------------------------------------------------------
def test_dropin_generator_samples_a_windowed_wrapping_frame(tmp_path, monkeypatch):
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion
    from cgd_amd import nets, sampler
    seen = []
    plain = sampler.GuidedSampler.ddim_sample_loop_progressive

    def recording(self, model, shape, *a, **kw):
        seen.append((model, tuple(shape), kw["cond_fn"].unet, []))
        for out in plain(self, model, shape, *a, **kw):
            seen[-1][3].append(out["pred_xstart"].detach().clone())
            yield out

    monkeypatch.setattr(sampler.GuidedSampler, "ddim_sample_loop_progressive", recording)
    items = list(clip_guided_diffusion(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=2, width_offset=32,
                                       timestep_respacing="ddim4+windows=16:wrapx", seed=7, prefix_path=str(tmp_path / "out"),
                                       checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=False, device="cuda"))
    assert len(items) == 4 and all(os.path.isfile(p) for _, p in items)
    (model, shape, guided, frames), = seen
    assert isinstance(model, nets.WindowedUNet) and guided is model and shape == (1, 3, 64, 96)
    assert (model.window, model.stride, model.wrap, model.feather) == (64, 16, "x", False) and model.plan(64, 96).n == 6
    assert len(frames) == 4 and all(tuple(f.shape) == (1, 3, 64, 96) and th.isfinite(f).all() for f in frames)
    from PIL import Image
    assert Image.open(items[-1][1]).size == (96, 64)
    with pytest.raises(ValueError):  # refused before any load
        next(clip_guided_diffusion(prompts=["x"], image_size=64, width_offset=40, timestep_respacing="ddim4+windows=16:wrapx", device="cuda",
                                   checkpoints_dir=str(tmp_path / "none"), prefix_path=str(tmp_path / "none_out")))
    assert not (tmp_path / "none").exists()
