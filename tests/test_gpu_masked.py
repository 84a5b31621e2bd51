"""GPU tests of masked sampling: cgd_masked_merge against its fp64 restatement and its exactness rules, whole masked trajectories of
the native sampler against tests/masked_ref.py on the `mini` scene of tests/step_checks.py (replayed tape: x_T, class ids, step noise per
evaluation, the known region's noise per merge, the re-noise per repeat, cutout coordinates per cond_fn call), properties that need no
reference, and the drop-in generator with `init_image="IMAGE::MASK"`."""
import itertools
import os

import pytest
import torch as th

from tests import masked_ref
from tests import parity_checks as pc
from tests import step_checks

pytestmark = pytest.mark.gpu

DEV = pc.DEV


def _assert_all(recs):
    for r in recs:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3e}")
    bad = [r for r in recs if not r["ok"]]
    assert not bad, bad[:3]


# ---- op level ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def op_rig():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    return L.Context(0, 1), dd.create_gaussian_diffusion(1000, "linear", "50", False), L


def _dev(t, offset):
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


def _check_mask(mask):
    n = mask.numel()
    ones, zeros = int((mask == 1).sum()), int((mask == 0).sum())
    assert 0.25 * n <= ones <= 0.75 * n and n - ones - zeros >= 0.1 * n and zeros > 0


def _merge_case(rig, shape, i, mask_b1, mask_c, init_b1, with_x0, with_re, offset=False, poison=False, seed=0):
    """One launch; returns the parity records (fp64 restatement) after asserting the exactness rules."""
    ctx, tab, L = rig
    B, _, H, W = shape
    gen = th.Generator().manual_seed(1000 * seed + 10 * i + mask_c + 2 * mask_b1 + 4 * init_b1)
    mk = lambda *s: th.randn(*s, generator=gen)  # noqa: E731
    sample, x0, n_known, n_re = mk(*shape), mk(*shape), mk(*shape), mk(*shape)
    init = th.tanh(mk(1 if init_b1 else B, 3, H, W))
    mask = masked_ref.make_mask((1 if mask_b1 else B, mask_c, H, W), seed=seed + i)
    _check_mask(mask)
    m_full, init_full = mask.expand(shape), init.expand(shape)
    keep, regen = m_full == 0, m_full == 1
    if poison:  # non-finite state where the init image is kept: nothing of it may reach the output
        bad = th.where(th.rand(shape, generator=gen) < 0.5, th.tensor(float("inf")), th.tensor(float("nan")))
        sample, x0 = th.where(keep, bad, sample), th.where(keep, -bad, x0)
    k = tab.mask_coef(i)
    if k.sqrt_one_minus_ab_prev == 0.0:
        n_known = None
    if not with_x0:
        x0 = None
    if not with_re:
        n_re = None
    k.flags = (L.MASK_PRED_XSTART if with_x0 else 0) | (L.MASK_N_KNOWN if n_known is not None else 0) | (L.MASK_RENOISE if with_re else 0)
    d_sample, d_x0, d_init, d_mask, d_nk, d_nre = (_dev(t, offset) for t in (sample, x0, init, mask, n_known, n_re))
    d_xre = _dev(th.full(shape, float("nan")), offset) if with_re else None
    ctx.check(ctx.lib.cgd_masked_merge(ctx.h, d_sample.data_ptr(), L.ptr(d_x0), d_init.data_ptr(), d_mask.data_ptr(), L.ptr(d_nk),
                                       L.ptr(d_nre), L.ptr(d_xre), B, H, W, init.shape[0], mask.shape[0], mask_c, k, ctx.stream()))
    th.cuda.synchronize()
    got_s = d_sample.cpu()
    got_x0 = d_x0.cpu() if with_x0 else None
    # exactness: the fp32 value of the formula as written where the mask is 0, untouched bits where it is 1
    known32 = k.sqrt_ab_prev * init_full if n_known is None else k.sqrt_ab_prev * init_full + k.sqrt_one_minus_ab_prev * n_known
    assert th.equal(got_s[keep], known32[keep]) and th.isfinite(got_s[keep]).all()
    assert th.equal(got_s[regen], sample[regen])
    if i == 0:
        assert th.equal(got_s[keep], init_full[keep])
    if with_x0:
        assert th.equal(got_x0[keep], init_full[keep]) and th.equal(got_x0[regen], x0[regen])
    tag = f"merge {tuple(shape)} i{i} mask{'1' if mask_b1 else 'B'}x{mask_c} init{'1' if init_b1 else 'B'} x0{int(with_x0)} re{int(with_re)}" \
          f"{' offset' if offset else ''}{' poisoned' if poison else ''}"
    if poison:  # the parity records are taken over the state with the poison removed (it never reaches the output)
        sample = th.where(keep, th.zeros(()), sample)
        x0 = None if x0 is None else th.where(keep, th.zeros(()), x0)
    ref_s, ref_x0, ref_re = masked_ref.merge_fp64(k, sample, x0, init, mask, n_known, n_re)
    recs = [pc.rec(f"{tag} sample", got_s, ref_s)]
    if with_x0:
        recs.append(pc.rec(f"{tag} pred_xstart", got_x0, ref_x0))
    if with_re:
        got_re = d_xre.cpu()
        assert th.isfinite(got_re[keep]).all()
        recs.append(pc.rec(f"{tag} x_re", got_re, ref_re))
    return recs


@pytest.mark.parametrize("shape", [(2, 3, 24, 40), (3, 3, 7, 9)])
def test_masked_merge_matches_fp64_and_selects_at_the_endpoints(op_rig, shape):
    """(3, 3, 7, 9): a plane of 63 floats, no multiple of 4 — the scalar path; (2, 3, 24, 40): the 16-byte path"""
    recs = []
    for i, (mask_b1, mask_c), init_b1, with_x0, with_re in itertools.product((20, 0), ((True, 1), (False, 1), (False, 3)), (True, False),
                                                                             (True, False), (True, False)):
        recs += _merge_case(op_rig, shape, i, mask_b1, mask_c, init_b1, with_x0, with_re)
    _assert_all(recs)


def test_masked_merge_on_pointers_offset_by_one_float(op_rig):
    recs = []
    for i, with_re in itertools.product((20, 0), (True, False)):
        recs += _merge_case(op_rig, (2, 3, 24, 40), i, False, 1, True, True, with_re, offset=True)
    _assert_all(recs)


@pytest.mark.parametrize("shape", [(2, 3, 24, 40), (3, 3, 7, 9)])
def test_masked_merge_keeps_non_finite_state_out_of_the_kept_region(op_rig, shape):
    recs = []
    for i in (20, 0):
        recs += _merge_case(op_rig, shape, i, False, 3, False, True, True, poison=True, seed=1)
        recs += _merge_case(op_rig, shape, i, True, 1, True, True, False, poison=True, seed=2)
    _assert_all(recs)


def test_masked_merge_refuses_bad_arguments(op_rig):
    ctx, tab, L = op_rig
    B, H, W = 2, 8, 8
    x = th.zeros(B, 3, H, W, device=DEV)
    p = x.data_ptr()
    full = L.MASK_PRED_XSTART | L.MASK_N_KNOWN | L.MASK_RENOISE

    def call(sample=p, x0=p, init=p, mask=p, nk=p, nre=p, xre=p, B=B, H=H, W=W, ib=B, mb=B, mc=3, i=5, flags=full):
        k = tab.mask_coef(i)
        k.flags = flags
        return ctx.lib.cgd_masked_merge(ctx.h, sample, x0, init, mask, nk, nre, xre, B, H, W, ib, mb, mc, k, ctx.stream())

    bad = [dict(sample=None), dict(init=None), dict(mask=None),                      # a required buffer is missing
           dict(nk=None, flags=full & ~L.MASK_N_KNOWN),                              # no known noise although its coefficient is not 0
           dict(nre=None), dict(xre=None),                                           # re-noise draw and output come together
           dict(x0=None), dict(flags=0), dict(nre=None, xre=None),                   # flags that disagree with the pointers
           dict(ib=3), dict(ib=0), dict(mb=3), dict(mc=2), dict(mc=0),               # broadcast extents
           dict(B=0), dict(H=0), dict(W=-1)]                                         # sizes
    for kw in bad:
        assert call(**kw) == -2 and ctx.lib.cgd_last_error(ctx.h), kw
    # the same arguments with nothing wrong are accepted, and at i == 0 the known noise may be absent
    assert call() == 0
    assert call(i=0, nk=None, flags=full & ~L.MASK_N_KNOWN) == 0
    th.cuda.synchronize()


# ---- trajectories --------------------------------------------------------------------------------------------------------------------
def _scene(steps, evals, calls=None, t_first=None):
    """the `mini` scene with one step noise / known noise / re-noise entry per evaluation and one coordinate entry per cond_fn call"""
    from oracle import guidance as og
    sc = step_checks.Scenario("mini", ddim=True, steps=steps, t_first=t_first)
    gen = th.Generator().manual_seed(2468)
    shape = (sc.B, 3, sc.H, sc.W)
    for key in ("noise", "known_noise", "renoise"):
        sc.tape[key] = [th.randn(shape, generator=gen) for _ in range(evals)]
    sc.tape["coords"] = [og.generate_coords(sc.H, sc.W, sc.cutn, sc.res, 1.0, generator=gen) for _ in range(calls or evals)]
    sc.mask = masked_ref.make_mask((1, 1, sc.H, sc.W), seed=7)
    _check_mask(sc.mask)
    return sc


def _user_cond(target):
    def make(dev):
        tgt = target.to(dev)

        def cond_fn(x, t, out, y=None):
            loss = 0.1 * ((out["pred_xstart"] - tgt) ** 2).sum()
            return -th.autograd.grad(loss, x)[0]
        return cond_fn
    return make


def _mkw(sc, dev):
    return {"y": th.zeros(sc.B, dtype=th.long, device=dev)} if sc.kw.get("num_classes") else {}


def _oracle(sc, kind, mask, eta=0.0, order=2, resamples=1, user_cond=None):
    og = sc.og
    diff = masked_ref.create_masked_diffusion(1000, sc.schedule, sc.spec, sc.rescale)
    cgs, tvs, rs = sc.scales
    if user_cond is None:
        cond, st = og.make_cond_fn(diffusion=diff, clip_model=sc.ref_clip, make_cutouts=og.MakeCutouts(sc.res, sc.cutn),
                                   target_embeds=sc.targets, weights=sc.w, num_cutouts=sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                                   range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude, coords_tape=sc.tape["coords"])
    else:
        cond, st = user_cond("cpu"), {}
    mkw = _mkw(sc, "cpu")
    gen = diff.masked_loop(kind, sc.ref_unet, (sc.B, 3, sc.H, sc.W), sc.x0_star.expand(sc.B, -1, -1, -1), mask, sc.tape, cond_fn=cond,
                           model_kwargs=mkw, skip_timesteps=sc.skip, randomize_class=bool(mkw), eta=eta, order=order, resamples=resamples)
    st["current_timestep"] = sc.counter0
    out = []
    for o in itertools.islice(gen, sc.steps):
        st["current_timestep"] -= 1
        out.append((o["sample"].clone(), o["pred_xstart"].clone()))
    return out


def _device(sc, kind, mask, eta=0.0, order=2, resamples=1, user_cond=None, tape=True, init=None):
    """[(sample, pred_xstart)] per yielded step of the device loop; mask None = the unmasked loop"""
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
    if user_cond is None:
        cond = dg.ClipGuidance(ctx, unet, clip, smp, sc.targets.to(DEV), sc.w, sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                               range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude)
        if tape:
            cond.coords_tape = sc.tape["coords"]
        cond.current_timestep = sc.counter0
    else:
        cond = user_cond(DEV)
    shape, mkw = (sc.B, 3, sc.H, sc.W), _mkw(sc, DEV)
    init = sc.x0_star.expand(sc.B, -1, -1, -1) if init is None else init
    kw = dict(clip_denoised=False, cond_fn=cond, model_kwargs=mkw, device=DEV, skip_timesteps=sc.skip, init_image=init.to(DEV),
              randomize_class=bool(mkw), cond_fn_with_grad=True)
    if mask is not None:
        kw["mask"] = mask.to(DEV)
    if resamples != 1:
        kw["resamples"] = resamples
    if kind == "plms":
        gen = smp.plms_sample_loop_progressive(unet, shape, order=order, **kw)
    elif kind == "ddim":
        gen = smp.ddim_sample_loop_progressive(unet, shape, eta=eta, **kw)
    else:
        gen = smp.p_sample_loop_progressive(unet, shape, **kw)
    out = []
    for o in itertools.islice(gen, sc.steps):
        th.cuda.synchronize()
        out.append((o["sample"].cpu(), o["pred_xstart"].cpu()))
        if user_cond is None:
            cond.current_timestep -= 1
    if user_cond is None and tape:
        assert cond.calls == len(sc.tape["coords"]), "one tape entry of coordinates per cond_fn call"
    return out


def _compare(sc, tag, d_out, o_out):
    recs = []
    assert len(d_out) == len(o_out) == sc.steps
    for k, ((ds, dx), (os_, ox)) in enumerate(zip(d_out, o_out)):
        recs.append(pc.rec(f"{tag} step{k} sample", ds, os_))
        recs.append(pc.rec(f"{tag} step{k} pred_xstart", dx, ox))
        keep = (sc.mask == 0).expand_as(dx)
        assert th.equal(dx[keep], sc.x0_star.expand_as(dx)[keep]), "pred_xstart is the init image where the mask is 0"
    return recs


@pytest.mark.parametrize("kind,eta", [("p", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_masked_trajectory_native_guidance_mini(kind, eta):
    sc = _scene(steps=4, evals=4)
    _assert_all(_compare(sc, f"masked {kind} eta {eta}", _device(sc, kind, sc.mask, eta=eta), _oracle(sc, kind, sc.mask, eta=eta)))


def test_masked_plms_trajectory_merges_the_predictor():
    sc = _scene(steps=5, evals=5, calls=6)
    _assert_all(_compare(sc, "masked plms order 2", _device(sc, "plms", sc.mask, order=2), _oracle(sc, "plms", sc.mask, order=2)))


def test_masked_trajectory_with_two_resamples():
    sc = _scene(steps=4, evals=8)
    _assert_all(_compare(sc, "masked p resamples 2", _device(sc, "p", sc.mask, resamples=2), _oracle(sc, "p", sc.mask, resamples=2)))


def test_masked_trajectory_generic_cond_fn_through_autograd():
    sc = _scene(steps=4, evals=4)
    uc = _user_cond(sc.x0_star)
    _assert_all(_compare(sc, "masked p generic", _device(sc, "p", sc.mask, user_cond=uc), _oracle(sc, "p", sc.mask, user_cond=uc)))


# ---- properties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,calls", [("p", 4), ("plms", 5)])
def test_an_all_ones_mask_is_the_unmasked_loop_bit_for_bit(kind, calls):
    sc = _scene(steps=4, evals=4, calls=calls)
    ones = th.ones(1, 1, sc.H, sc.W)
    masked, plain = _device(sc, kind, ones), _device(sc, kind, None)
    assert len(masked) == len(plain) == 4
    for (ms, mx), (ps, px) in zip(masked, plain):
        assert th.isfinite(ps).all() and th.equal(ms, ps) and th.equal(mx, px)


def test_an_all_zeros_mask_returns_the_init_image():
    from cgd_amd import diffusion as dd
    sc = _scene(steps=4, evals=4, t_first=3)  # runs to step index 0
    zeros = th.zeros(sc.B, 3, sc.H, sc.W)
    out = _device(sc, "p", zeros)
    init = sc.x0_star.expand(sc.B, -1, -1, -1)
    tab = dd.create_gaussian_diffusion(1000, sc.schedule, sc.spec, sc.rescale)
    for n, (s, x0) in enumerate(out):
        k = tab.mask_coef(3 - n)
        # the kept state is q_sample(init, level i - 1) with the taped noise, in fp32 as written (two products, one sum)
        want = k.sqrt_ab_prev * init + k.sqrt_one_minus_ab_prev * sc.tape["known_noise"][n] if n < 3 else init
        assert th.equal(s, want) and th.equal(x0, init)
    assert th.equal(out[-1][0], init) and th.equal(out[-1][1], init)


def test_untaped_deterministic_masked_runs_repeat():
    sc = _scene(steps=4, evals=4)
    runs = []
    for _ in range(2):
        th.manual_seed(31)
        runs.append(_device(sc, "ddim", sc.mask, eta=0.0, tape=False))
    for (a_s, a_x), (b_s, b_x) in zip(*runs):
        assert th.isfinite(a_s).all() and th.equal(a_s, b_s) and th.equal(a_x, b_x)


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------
def test_dropin_generator_inpaints_with_an_image_and_mask_value(tmp_path, monkeypatch):
    import numpy as np
    from PIL import Image
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion
    from cgd_amd import sampler
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    m = np.zeros((64, 64), dtype=np.uint8)
    m[:, 32:] = 255  # the right half is regenerated
    Image.fromarray(img).save(tmp_path / "a.png")
    Image.fromarray(m).save(tmp_path / "m.png")
    seen = []
    plain = sampler.GuidedSampler.ddim_sample_loop_progressive

    def recording(self, *a, **kw):
        seen.append((kw.get("mask"), kw.get("init_image"), []))
        for out in plain(self, *a, **kw):
            seen[-1][2].append(out["pred_xstart"].detach().clone())
            yield out

    monkeypatch.setattr(sampler.GuidedSampler, "ddim_sample_loop_progressive", recording)
    items = list(clip_guided_diffusion(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=2, timestep_respacing="ddim8",
                                       init_image=f"{tmp_path / 'a.png'}::{tmp_path / 'm.png'}", seed=7, prefix_path=str(tmp_path / "out"),
                                       checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=1, progress=False, device="cuda"))
    assert len(items) == 8 and all(os.path.isfile(p) for _, p in items)
    (mask, init, frames), = seen
    assert tuple(mask.shape) == (1, 1, 64, 64) and len(frames) == 8
    want_init = th.from_numpy(img).float().div(255).permute(2, 0, 1).unsqueeze(0).mul(2).sub(1)
    assert th.equal(init.cpu(), want_init)
    assert th.equal(mask.cpu()[0, 0], th.from_numpy(m).float().div(255)) and set(mask.unique().tolist()) == {0.0, 1.0}
    last = frames[-1].cpu()
    assert th.equal(last[..., :32], want_init[..., :32])            # black half: the init image, exactly
    assert not th.equal(last[..., 32:], want_init[..., 32:])        # white half: regenerated
    assert (last[..., 32:] != want_init[..., 32:]).float().mean() > 0.9
