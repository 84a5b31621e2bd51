"""GPU tests of ILVR: cgd_ilvr_refine's operator against the vendored ResizeRight's fixture, the refinement against its fp64 restatement
(tests/ilvr_ref.py) and its exactness rules, whole trajectories of the native sampler with `ilvr=` against the restatement's loops on the
`mini` scene of tests/step_checks.py (replayed tape: x_T, class ids, step noise per evaluation, the reference's noise per refinement, cutout
coordinates per cond_fn call), properties that need no reference, and the drop-in generator with `init_image="ilvr8=IMAGE"`."""
import itertools
import os

import numpy as np
import pytest
import torch as th

from tests import ilvr_ref
from tests import parity_checks as pc
from tests import step_checks
from tests.test_gpu_masked import _dev

pytestmark = pytest.mark.gpu

DEV = pc.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_CASES = [(32, 32, 2), (32, 32, 8), (24, 40, 4), (64, 64, 32), (16, 16, 16)]


def _assert_all(recs):
    for r in recs:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3e}")
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


@pytest.fixture(scope="module")
def op_rig():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    return L.Context(0, 1), dd.create_gaussian_diffusion(1000, "linear", "50", False), L


def _refine(rig, sample, x0, ref, noise, N, sa, sb, offset=False):
    """one cgd_ilvr_refine call on copies of the arguments -> (sample, pred_xstart or None) on the host"""
    ctx, _, L = rig
    B, _, H, W = sample.shape
    d_s, d_x0, d_ref, d_n = (_dev(t, offset) for t in (sample, x0, ref, noise))
    scratch = _dev(th.full((int(ctx.lib.cgd_ilvr_scratch_floats(B, H, W, N, int(x0 is not None))),), float("nan")), offset)
    ctx.check(ctx.lib.cgd_ilvr_refine(ctx.h, d_s.data_ptr(), L.ptr(d_x0), d_ref.data_ptr(), L.ptr(d_n), scratch.data_ptr(), B, H, W,
                                      ref.shape[0], N, sa, sb, ctx.stream()))
    th.cuda.synchronize()
    return d_s.cpu(), None if x0 is None else d_x0.cpu()


# ---- the operator alone, against the real ResizeRight --------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,N", FIXTURE_CASES)
def test_operator_matches_resize_right(op_rig, H, W, N):
    fx = np.load(os.path.join(ROOT, "tests", "golden", "reference_ilvr.npz"))
    x, y = th.from_numpy(fx[f"x_{H}x{W}_{N}"]), th.from_numpy(fx[f"y_{H}x{W}_{N}"])
    ref = x.float()  # on a 1/128 grid: exact in float32
    assert th.equal(ref.double(), x)
    zeros = th.zeros_like(ref)
    got_s, none = _refine(op_rig, zeros, None, ref, None, N, 1.0, 0.0)
    assert none is None
    got_s2, got_x0 = _refine(op_rig, zeros, zeros, ref, None, N, 1.0, 0.0)
    assert th.equal(got_s, got_s2)  # the pred_xstart pair changes nothing of the sample's
    _assert_all([pc.rec(f"phi_{N} {H}x{W} sample", got_s, y), pc.rec(f"phi_{N} {H}x{W} pred_xstart", got_x0, y)])


# ---- the refinement against refine_fp64 ----------------------------------------------------------------------------------------------
REFINE_SHAPES = [((2, 3, 24, 40), 4), ((1, 3, 16, 16), 16), ((1, 3, 64, 64), 32), ((1, 3, 128, 64), 64), ((1, 3, 72, 264), 8)]


def _refine_case(rig, shape, N, i, ref_b1, with_x0, offset=False, seed=0):
    _, tab, _ = rig
    B, _, H, W = shape
    gen = th.Generator().manual_seed(1000 * seed + 10 * i + 2 * ref_b1 + with_x0 + N)
    mk = lambda *s: th.randn(*s, generator=gen)  # noqa: E731
    sample, x0, noise = mk(*shape), (th.tanh(mk(*shape)) if with_x0 else None), mk(*shape)
    ref = th.tanh(mk(1 if ref_b1 else B, 3, H, W))
    k = tab.mask_coef(i)
    sa, sb = k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev
    if sb == 0.0:
        noise = None
    got_s, got_x0 = _refine(rig, sample, x0, ref, noise, N, sa, sb, offset)
    want_s, want_x0 = ilvr_ref.refine_fp64(sa, sb, sample, x0, ref, noise, N)
    tag = f"refine {tuple(shape)} N{N} i{i} ref{'1' if ref_b1 else 'B'} x0{int(with_x0)}{' offset' if offset else ''}"
    recs = [pc.rec(f"{tag} sample", got_s, want_s)]
    if with_x0:
        recs.append(pc.rec(f"{tag} pred_xstart", got_x0, want_x0))
    return recs


@pytest.mark.parametrize("shape,N", REFINE_SHAPES)
def test_refinement_matches_fp64(op_rig, shape, N):
    """(1,3,16,16) N 16: one low-resolution pixel, every up row has taps outside; (1,3,128,64) N 64: 256-tap rows; (1,3,72,264) N 8: a
    row wider than one pass of a 256-thread workgroup, at a frame with offsets"""
    recs = []
    for i, ref_b1, with_x0 in itertools.product((20, 0), (True, False), (True, False)):
        recs += _refine_case(op_rig, shape, N, i, ref_b1, with_x0)
    _assert_all(recs)


def test_refinement_on_pointers_offset_by_one_float(op_rig):
    recs = []
    for i in (20, 0):
        recs += _refine_case(op_rig, (2, 3, 24, 40), 4, i, True, True, offset=True, seed=3)
    _assert_all(recs)


# ---- exactness -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,N", [((2, 3, 24, 40), 4), ((1, 3, 64, 64), 32)])
def test_a_state_equal_to_the_reference_keeps_its_bits(op_rig, shape, N):
    gen = th.Generator().manual_seed(11)
    ref = th.randn(shape, generator=gen)
    got_s, got_x0 = _refine(op_rig, ref.clone(), ref.clone(), ref, None, N, 1.0, 0.0)
    assert th.equal(got_s, ref) and th.equal(got_x0, ref)  # d is exactly 0


def test_two_calls_on_the_same_inputs_give_the_same_bits(op_rig):
    _, tab, _ = op_rig
    k = tab.mask_coef(20)
    gen = th.Generator().manual_seed(12)
    shape = (2, 3, 72, 264)
    sample, x0, ref, noise = (th.randn(shape, generator=gen) for _ in range(4))
    a = _refine(op_rig, sample, x0, ref, noise, 8, k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev)
    b = _refine(op_rig, sample, x0, ref, noise, 8, k.sqrt_ab_prev, k.sqrt_one_minus_ab_prev)
    assert th.isfinite(a[0]).all() and th.equal(a[0], b[0]) and th.equal(a[1], b[1]) and not th.equal(a[0], sample)


def test_refinement_refuses_bad_arguments(op_rig):
    ctx, _, _ = op_rig
    B, H, W = 2, 16, 32
    x = th.zeros(B, 3, H, W, device=DEV)
    p = x.data_ptr()

    def call(sample=p, x0=p, ref=p, noise=p, scratch=p, B=B, H=H, W=W, rb=B, N=4, sa=0.8, sb=0.6):
        return ctx.lib.cgd_ilvr_refine(ctx.h, sample, x0, ref, noise, scratch, B, H, W, rb, N, sa, sb, ctx.stream())

    bad = [dict(sample=None), dict(ref=None), dict(scratch=None),       # a required buffer is missing
           dict(N=3), dict(N=1), dict(N=0), dict(N=128), dict(N=-4),     # no power of two in [2, 64]
           dict(N=32), dict(N=64), dict(N=8, H=20),                      # does not divide H and W
           dict(rb=3), dict(rb=0),                                       # the reference's batch
           dict(noise=None),                                             # no noise although its coefficient is not 0
           dict(B=0), dict(H=0), dict(W=-4)]                             # sizes
    for kw in bad:
        assert call(**kw) == -2 and ctx.lib.cgd_last_error(ctx.h), kw
    # the same arguments with nothing wrong are accepted; without pred_xstart, with a broadcast reference, and without noise at sb == 0 too
    scratch = th.empty(int(ctx.lib.cgd_ilvr_scratch_floats(B, H, W, 4, 1)), device=DEV)
    sample, x0 = th.zeros_like(x), th.zeros_like(x)
    ok = dict(sample=sample.data_ptr(), x0=x0.data_ptr(), scratch=scratch.data_ptr())
    assert call(**ok) == 0
    assert call(**{**ok, "x0": None}) == 0 and call(**ok, rb=1) == 0 and call(**ok, noise=None, sa=1.0, sb=0.0) == 0
    th.cuda.synchronize()


# ---- trajectories ----------------------------------------------------------------------------------------------------------------------
FACTOR = 4


def _scene(kind, steps, calls=None):
    """the `mini` scene (32 x 32) with one step noise and one reference noise per evaluation, one coordinate entry per cond_fn call and a
    reference image of its own; 'dpm': re-spaced to 'dpm8' as in tests/test_gpu_dpm.py (the last `steps` levels)"""
    from cgd_amd import diffusion as dd
    from oracle import guidance as og
    sc = step_checks.Scenario("mini", ddim=True, steps=steps)
    if kind == "dpm":
        sc.spec = "dpm8"
        sc.N = dd.create_gaussian_diffusion(1000, sc.schedule, sc.spec).num_timesteps
        assert sc.N == 8
        sc.t_first, sc.skip, sc.counter0 = steps - 1, sc.N - steps, steps - 1
    gen = th.Generator().manual_seed(1357)
    shape = (sc.B, 3, sc.H, sc.W)
    assert (sc.H, sc.W) == (32, 32)
    for key in ("noise", "ilvr_noise"):
        sc.tape[key] = [th.randn(shape, generator=gen) for _ in range(calls or steps)]
    sc.tape["coords"] = [og.generate_coords(sc.H, sc.W, sc.cutn, sc.res, 1.0, generator=gen) for _ in range(calls or steps)]
    sc.ilvr_ref = th.tanh(th.randn(1, 3, sc.H, sc.W, generator=gen))
    return sc


def _mkw(sc, dev):
    return {"y": th.zeros(sc.B, dtype=th.long, device=dev)} if sc.kw.get("num_classes") else {}


def _oracle(sc, kind, stop=0, eta=0.0, order=2):
    og = sc.og
    diff = ilvr_ref.create_ilvr_diffusion(1000, sc.schedule, sc.spec, sc.rescale)
    cgs, tvs, rs = sc.scales
    cond, st = og.make_cond_fn(diffusion=diff, clip_model=sc.ref_clip, make_cutouts=og.MakeCutouts(sc.res, sc.cutn),
                               target_embeds=sc.targets, weights=sc.w, num_cutouts=sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                               range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude, coords_tape=sc.tape["coords"])
    mkw = _mkw(sc, "cpu")
    gen = diff.ilvr_loop(kind, sc.ref_unet, (sc.B, 3, sc.H, sc.W), sc.ilvr_ref, FACTOR, sc.tape, stop=stop, cond_fn=cond, model_kwargs=mkw,
                         skip_timesteps=sc.skip, init_image=sc.x0_star.expand(sc.B, -1, -1, -1), randomize_class=bool(mkw), eta=eta,
                         order=order)
    st["current_timestep"] = sc.counter0
    out = []
    for o in itertools.islice(gen, sc.steps):
        st["current_timestep"] -= 1
        out.append((o["sample"].clone(), o["pred_xstart"].clone()))
    return out


def _device(sc, kind, stop=0, eta=0.0, order=2, ilvr=True, tape=True):
    """[(sample, pred_xstart)] per yielded step of the device loop; ilvr False = the loop without `ilvr=`"""
    from cgd_amd import diffusion as dd
    from cgd_amd import guidance as dg
    from cgd_amd import lib, nets, sampler
    ctx = lib.Context(0, 1)
    unet = nets.UNet(ctx, **sc.kw)
    unet.load_state_dict({k: v.to(DEV) for k, v in sc.ref_unet.state_dict().items()})
    clip = nets.ClipImageTower(ctx, config=sc.vit_cfg)
    clip.load_clip_state_dict({k: v.to(DEV) for k, v in sc.ref_clip.state_dict().items()})
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, sc.schedule, sc.spec, sc.rescale))
    smp.tape = sc.tape if tape else None
    cgs, tvs, rs = sc.scales
    cond = dg.ClipGuidance(ctx, unet, clip, smp, sc.targets.to(DEV), sc.w, sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                           range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude)
    if tape:
        cond.coords_tape = sc.tape["coords"]
    cond.current_timestep = sc.counter0
    shape, mkw = (sc.B, 3, sc.H, sc.W), _mkw(sc, DEV)
    kw = dict(clip_denoised=False, cond_fn=cond, model_kwargs=mkw, device=DEV, skip_timesteps=sc.skip,
              init_image=sc.x0_star.expand(sc.B, -1, -1, -1).to(DEV), randomize_class=bool(mkw), cond_fn_with_grad=True)
    if ilvr:
        kw["ilvr"] = (sc.ilvr_ref.to(DEV), FACTOR, stop)
    if kind == "plms":
        gen = smp.plms_sample_loop_progressive(unet, shape, order=order, **kw)
    elif kind == "dpm":
        gen = smp.dpmpp_sample_loop_progressive(unet, shape, order=order, eta=eta, **kw)
    elif kind == "ddim":
        gen = smp.ddim_sample_loop_progressive(unet, shape, eta=eta, **kw)
    else:
        gen = smp.p_sample_loop_progressive(unet, shape, **kw)
    out = []
    for o in itertools.islice(gen, sc.steps):
        th.cuda.synchronize()
        out.append((o["sample"].cpu(), o["pred_xstart"].cpu()))
        cond.current_timestep -= 1
    if tape:
        assert cond.calls == len(sc.tape["coords"]), "one tape entry of coordinates per cond_fn call"
    return out


def _compare(sc, tag, d_out, o_out):
    recs = []
    assert len(d_out) == len(o_out) == sc.steps
    for k, ((ds, dx), (os_, ox)) in enumerate(zip(d_out, o_out)):
        recs.append(pc.rec(f"{tag} step{k} sample", ds, os_))
        recs.append(pc.rec(f"{tag} step{k} pred_xstart", dx, ox))
    return recs


@pytest.mark.parametrize("kind,eta,steps,calls", [("p", 0.0, 4, 4), ("ddim", 0.0, 4, 4), ("ddim", 0.5, 4, 4), ("plms", 0.0, 5, 6),
                                                  ("dpm", 0.0, 5, 5)])
def test_ilvr_trajectory_native_guidance_mini(kind, eta, steps, calls):
    sc = _scene(kind, steps, calls)
    _assert_all(_compare(sc, f"ilvr {kind} eta {eta}", _device(sc, kind, eta=eta), _oracle(sc, kind, eta=eta)))


def test_ilvr_trajectory_stops_refining_below_the_stop_index():
    sc = _scene("p", 4)
    stop = sc.t_first - 1  # the first two of the four steps are refined
    d_out = _device(sc, "p", stop=stop)
    _assert_all(_compare(sc, f"ilvr p stop {stop}", d_out, _oracle(sc, "p", stop=stop)))


@pytest.mark.parametrize("kind,steps,calls", [("p", 4, 4), ("plms", 5, 6), ("dpm", 5, 5)])
def test_a_stop_index_at_the_number_of_timesteps_is_the_loop_without_ilvr_bit_for_bit(kind, steps, calls):
    sc = _scene(kind, steps, calls)
    with_ilvr, plain = _device(sc, kind, stop=sc.N), _device(sc, kind, ilvr=False)
    assert len(with_ilvr) == len(plain) == steps
    for (a_s, a_x), (b_s, b_x) in zip(with_ilvr, plain):
        assert th.isfinite(b_s).all() and th.equal(a_s, b_s) and th.equal(a_x, b_x)
    # ... and with stop = 0 it is another trajectory
    assert not th.equal(_device(sc, kind)[0][0], plain[0][0])


def test_untaped_deterministic_ilvr_runs_repeat():
    sc = _scene("ddim", 4)
    runs = []
    for _ in range(2):
        th.manual_seed(31)
        runs.append(_device(sc, "ddim", eta=0.0, tape=False))
    for (a_s, a_x), (b_s, b_x) in zip(*runs):
        assert th.isfinite(a_s).all() and th.equal(a_s, b_s) and th.equal(a_x, b_x)


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------
def test_dropin_generator_samples_with_an_ilvr_value(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion
    from cgd_amd import sampler
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    Image.fromarray(img).save(tmp_path / "a.png")
    seen = []
    plain = sampler.GuidedSampler.ddim_sample_loop_progressive

    def recording(self, *a, **kw):
        seen.append((kw.get("ilvr"), kw.get("init_image"), kw.get("mask"), []))
        for out in plain(self, *a, **kw):
            seen[-1][3].append(out["pred_xstart"].detach().clone())
            yield out

    monkeypatch.setattr(sampler.GuidedSampler, "ddim_sample_loop_progressive", recording)
    items = list(clip_guided_diffusion(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=2, timestep_respacing="ddim8",
                                       init_image=f"ilvr8@0.75={tmp_path / 'a.png'}", seed=7, prefix_path=str(tmp_path / "out"),
                                       checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=False, device="cuda"))
    assert len(items) == 8 and all(os.path.isfile(p) for _, p in items)
    (ilvr, init, mask, frames), = seen
    assert mask is None and len(frames) == 8 and all(th.isfinite(f).all() for f in frames)
    ref, factor, stop = ilvr
    want = th.from_numpy(img).float().div(255).permute(2, 0, 1).unsqueeze(0).mul(2).sub(1)
    assert factor == 8 and stop == 2 and th.equal(ref.cpu(), want) and th.equal(init.cpu(), want)  # the image is also the init image
