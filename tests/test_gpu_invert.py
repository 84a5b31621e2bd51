"""GPU tests of DDIM inversion: cgd_ddim_reverse_update against its fp64 restatement, what it refuses, whole inversion trajectories of the
native sampler against tests/invert_ref.py on the `mini` scene of tests/step_checks.py, the start state a sampling loop forms from the
returned noise, inversion composed with guided (and masked) DDIM sampling, and the drop-in generator with `init_image="invert=IMAGE"`."""
import itertools
import os

import pytest
import torch as th

from tests import invert_ref
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


# ---- op level ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def op_rig():
    from cgd_amd import diffusion as dd
    from cgd_amd import lib as L
    return L.Context(0, 1), dd.create_gaussian_diffusion(1000, "linear", "50", False), L


def _reverse_case(rig, shape, i, with_x0, with_noise, init_b1, offset=False):
    """One launch; the parity records against the fp64 restatement.  Outputs start as NaN, the variance planes of the model output hold
    NaN / Inf: every output must come out finite, so those planes were never read and every element was written."""
    ctx, tab, L = rig
    B, _, H, W = shape
    gen = th.Generator().manual_seed(100 * i + 8 * B + 4 * with_x0 + 2 * with_noise + init_b1)
    x = th.randn(shape, generator=gen)
    out6 = th.randn(B, 6, H, W, generator=gen)
    out6[:, 3:] = th.where(th.rand(B, 3, H, W, generator=gen) < 0.5, th.tensor(float("inf")), th.tensor(float("nan")))
    out6[:, 4] = -out6[:, 4]
    init = th.tanh(th.randn(1 if init_b1 else B, 3, H, W, generator=gen))
    k = tab.reverse_coef(i)
    nan = th.full(shape, float("nan"))
    d_x, d_o6, d_init = (_dev(t, offset) for t in (x, out6, init))
    d_xn = _dev(nan, offset)
    d_x0 = _dev(nan, offset) if with_x0 else None
    d_nz = _dev(nan, offset) if with_noise else None
    ctx.check(ctx.lib.cgd_ddim_reverse_update(ctx.h, d_x.data_ptr(), d_o6.data_ptr(), d_init.data_ptr() if with_noise else None,
                                              d_xn.data_ptr(), L.ptr(d_x0), L.ptr(d_nz), B, H, W, init.shape[0], k, ctx.stream()))
    th.cuda.synchronize()
    ref_xn, ref_x0, ref_nz = invert_ref.reverse_update_fp64(k, x, out6, init if with_noise else None)
    tag = f"reverse {tuple(shape)} i{i} x0{int(with_x0)} noise{int(with_noise)} init{'1' if init_b1 else 'B'}{' offset' if offset else ''}"
    assert th.equal(d_x.cpu(), x) and th.equal(d_o6.cpu()[:, :3], out6[:, :3])  # inputs untouched
    recs = [pc.rec(f"{tag} x_next", d_xn.cpu(), ref_xn)]
    if with_x0:
        recs.append(pc.rec(f"{tag} pred_xstart", d_x0.cpu(), ref_x0))
    if with_noise:
        recs.append(pc.rec(f"{tag} noise_out", d_nz.cpu(), ref_nz))
    return recs


@pytest.mark.parametrize("shape", [(2, 3, 24, 40), (3, 3, 7, 9)])
def test_reverse_update_matches_fp64(op_rig, shape):
    """(2, 3, 24, 40): the 16-byte path, and a batch of 2 tells a plane stride of 3 from the model output's 6; (3, 3, 7, 9): a plane of 63
    floats, no multiple of 4 — the scalar path"""
    recs = []
    for i, with_x0, with_noise, init_b1 in itertools.product((0, 20), (True, False), (True, False), (True, False)):
        recs += _reverse_case(op_rig, shape, i, with_x0, with_noise, init_b1)
    _assert_all(recs)


def test_reverse_update_on_pointers_offset_by_one_float(op_rig):
    recs = []
    for i, with_noise in itertools.product((0, 20), (True, False)):
        recs += _reverse_case(op_rig, (2, 3, 24, 40), i, True, with_noise, False, offset=True)
    _assert_all(recs)


def test_reverse_update_refuses_bad_arguments(op_rig):
    ctx, tab, L = op_rig
    B, H, W = 2, 8, 8
    bufs = [th.zeros(B, 3, H, W, device=DEV) for _ in range(5)]
    o6 = th.zeros(B, 6, H, W, device=DEV)
    px, pi, pn, p0, pz = (t.data_ptr() for t in bufs)

    def call(x=px, out6=o6.data_ptr(), init=pi, xn=pn, x0=p0, nz=pz, B=B, H=H, W=W, ib=B, k=None):
        return ctx.lib.cgd_ddim_reverse_update(ctx.h, x, out6, init, xn, x0, nz, B, H, W, ib, k or tab.reverse_coef(5), ctx.stream())

    flat = tab.reverse_coef(5)
    flat.sqrt_ab_next, flat.sqrt_one_minus_ab_next, flat.inv_sqrt_one_minus_ab_next = 1.0, 0.0, 0.0
    bad = [dict(B=0), dict(H=0), dict(W=-1),                              # an empty shape
           dict(x=None), dict(out6=None), dict(xn=None),                  # a required buffer is missing
           dict(xn=px), dict(x0=px), dict(nz=px),                         # no output may alias x
           dict(x0=pn), dict(nz=pn), dict(nz=p0),                         # the outputs are distinct buffers
           dict(init=None),                                               # noise_out without init
           dict(ib=3), dict(ib=0),                                        # an init batch that is neither 1 nor B
           dict(k=flat)]                                                  # sqrt(1 - abar_next) == 0 with noise_out requested
    for kw in bad:
        assert call(**kw) == -2 and ctx.lib.cgd_last_error(ctx.h), kw
    th.cuda.synchronize()
    assert all(float(t.abs().max()) == 0.0 for t in bufs)  # refused before any launch
    # the same call with nothing wrong is accepted; so is one without the optional outputs, and init batch 1
    assert call() == 0 and call(x0=None) == 0 and call(nz=None, init=None) == 0 and call(ib=1) == 0
    assert call(k=flat, nz=None) == 0  # the undefined inverse matters only to noise_out
    assert call(k=tab.reverse_coef(tab.num_timesteps - 1)) == 0  # the last index: abar_next = 0, the root is 1
    assert ctx.lib.cgd_ddim_reverse_update(None, px, o6.data_ptr(), pi, pn, p0, pz, B, H, W, B, tab.reverse_coef(5), ctx.stream()) == -3
    th.cuda.synchronize()


# ---- trajectories --------------------------------------------------------------------------------------------------------------------
def _image(sc):
    return sc.x0_star.expand(sc.B, -1, -1, -1).contiguous()


def _ykw(sc, dev):
    return {"y": th.zeros(sc.B, dtype=th.long, device=dev)} if sc.kw.get("num_classes") else {}


def _make_device(sc, precision=1):
    from cgd_amd import diffusion as dd
    from cgd_amd import lib, nets, sampler
    ctx = lib.Context(0, precision)
    unet = nets.UNet(ctx, **sc.kw)
    unet.load_state_dict({k: v.to(DEV) for k, v in sc.ref_unet.state_dict().items()})
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, sc.schedule, sc.spec, sc.rescale))
    return ctx, unet, smp


def _device_inversion(sc, skip, precision=1, dev_objs=None):
    ctx, unet, smp = dev_objs or _make_device(sc, precision)
    out = []
    for o in smp.ddim_reverse_sample_loop_progressive(unet, _image(sc).to(DEV), model_kwargs=_ykw(sc, DEV), device=DEV, skip_timesteps=skip):
        th.cuda.synchronize()
        out.append({k: v.cpu() for k, v in o.items()})
    return out


def _oracle_inversion(sc, skip):
    ref = invert_ref.create_invert_diffusion(1000, sc.schedule, sc.spec, sc.rescale)
    return list(ref.reverse_loop(sc.ref_unet, _image(sc), model_kwargs=_ykw(sc, "cpu"), skip_timesteps=skip))


_ORACLE = {}


def _inversion_pair(respacing, precision):
    """(records, device outputs) of a five-step inversion on the `mini` scene, class-conditional with y = 0.  "6": the whole schedule in five
    steps (indices 0..4 up to level 5), so the largest coefficients of a schedule are covered; "50": the first five levels."""
    sc = step_checks.Scenario("mini", ddim=True, respacing=respacing, steps=5)
    skip = sc.N - 1 - 5
    assert (respacing, sc.N, skip) in (("6", 6, 0), ("50", 50, 44))
    if respacing not in _ORACLE:  # computed once, shared, left unchanged
        _ORACLE[respacing] = _oracle_inversion(sc, skip)
    o_out, d_out = _ORACLE[respacing], _device_inversion(sc, skip, precision)
    assert len(o_out) == len(d_out) == 5
    recs = []
    for k, (d, o) in enumerate(zip(d_out, o_out)):
        assert sorted(d) == sorted(o) == (["noise", "pred_xstart", "sample"] if k == 4 else ["pred_xstart", "sample"])
        for key in sorted(o):
            recs.append(pc.rec(f"invert[mini ddim{respacing} p{precision}] step{k} {key}", d[key], o[key]))
    return recs


@pytest.mark.parametrize("respacing", ["6", "50"])
def test_inversion_trajectory_mini(respacing):
    _assert_all(_inversion_pair(respacing, 1))


def test_inversion_trajectory_mini_exact_fp32():
    _assert_all(_inversion_pair("6", 0))


# ---- start state -----------------------------------------------------------------------------------------------------------------------
def test_a_sampling_loop_given_the_noise_starts_from_the_latent():
    """q_sample(image, t0, noise) as the sampling loop forms it against the latent, within the bound derived in tests/test_invert_host.py
    (test_implied_noise_reproduces_the_latent_in_float32): 8 2^-24 (|latent| + |image|) elementwise"""
    sc = step_checks.Scenario("mini", ddim=True, steps=4)
    ctx, unet, smp = _make_device(sc)
    image = _image(sc).to(DEV)
    latent, noise = smp.ddim_invert(unet, image, model_kwargs=_ykw(sc, DEV), device=DEV, skip_timesteps=sc.skip)
    seen = []
    plain = unet.forward

    def recording(x, ts, y=None, out=None):
        seen.append((x.detach().clone(), ts.detach().clone()))
        return plain(x, ts, y, out=out)

    unet.forward = recording
    try:
        gen = smp.ddim_sample_loop_progressive(unet, tuple(image.shape), noise=noise, clip_denoised=False, model_kwargs=_ykw(sc, DEV),
                                               device=DEV, skip_timesteps=sc.skip, init_image=image)
        next(gen)
    finally:
        unet.forward = plain
    th.cuda.synchronize()
    first, ts = seen[0]
    assert float(ts[0]) == float(smp.tables.model_timestep(sc.t_first))  # the level the inversion stopped at
    bound = 8 * 2.0 ** -24 * (latent.abs() + image.abs())
    ratio = ((first - latent).abs() / bound).max().item()
    print(f"start state: worst |first state - latent| / bound = {ratio:.3f}")
    assert th.isfinite(first).all() and ratio <= 1.0


# ---- composition ---------------------------------------------------------------------------------------------------------------------
def _guided_device(sc, mask, dev_objs, noise):
    """4 guided DDIM steps of the device loop from `noise=noise, init_image=image, skip_timesteps=sc.skip` with the replayed tape"""
    from cgd_amd import guidance as dg
    from cgd_amd import nets
    ctx, unet, smp = dev_objs
    clip = nets.ClipImageTower(ctx, config=sc.vit_cfg)
    clip.load_clip_state_dict({k: v.to(DEV) for k, v in sc.ref_clip.state_dict().items()})
    smp.tape = sc.tape
    cgs, tvs, rs = sc.scales
    cond = dg.ClipGuidance(ctx, unet, clip, smp, sc.targets.to(DEV), sc.w, sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs, range_scale=rs,
                           sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude)
    cond.coords_tape = sc.tape["coords"]
    cond.current_timestep = sc.counter0
    mkw = _ykw(sc, DEV)
    gen = smp.ddim_sample_loop_progressive(unet, (sc.B, 3, sc.H, sc.W), noise=noise, clip_denoised=False, cond_fn=cond, model_kwargs=mkw,
                                           device=DEV, skip_timesteps=sc.skip, init_image=_image(sc).to(DEV), randomize_class=bool(mkw),
                                           cond_fn_with_grad=True, **({} if mask is None else {"mask": mask.to(DEV)}))
    out = []
    for o in itertools.islice(gen, sc.steps):
        th.cuda.synchronize()
        out.append((o["sample"].cpu(), o["pred_xstart"].cpu()))
        cond.current_timestep -= 1
    smp.tape = None
    return out


def _guided_oracle(sc, mask, noise):
    og = sc.og
    diff = sc.o_diff if mask is None else masked_ref.create_masked_diffusion(1000, sc.schedule, sc.spec, sc.rescale)
    cgs, tvs, rs = sc.scales
    cond, st = og.make_cond_fn(diffusion=diff, clip_model=sc.ref_clip, make_cutouts=og.MakeCutouts(sc.res, sc.cutn),
                               target_embeds=sc.targets, weights=sc.w, num_cutouts=sc.cutn, clip_guidance_scale=cgs, tv_scale=tvs,
                               range_scale=rs, sat_scale=sc.sat_scale, use_magnitude=sc.use_magnitude, coords_tape=sc.tape["coords"])
    mkw = _ykw(sc, "cpu")
    if mask is not None:  # masked_ref's loop takes its initial noise from the tape
        gen = diff.masked_loop("ddim", sc.ref_unet, (sc.B, 3, sc.H, sc.W), _image(sc), mask, dict(sc.tape, x_T=noise), cond_fn=cond,
                               model_kwargs=mkw, skip_timesteps=sc.skip, randomize_class=bool(mkw))
    else:
        gen = sc.o_diff.ddim_sample_loop_progressive(sc.ref_unet, (sc.B, 3, sc.H, sc.W), noise=noise, clip_denoised=False, cond_fn=cond,
                                                     model_kwargs=mkw, device="cpu", skip_timesteps=sc.skip, init_image=_image(sc),
                                                     randomize_class=bool(mkw), cond_fn_with_grad=True, tape=sc.tape)
    st["current_timestep"] = sc.counter0
    out = []
    for o in itertools.islice(gen, sc.steps):
        st["current_timestep"] -= 1
        out.append((o["sample"].clone(), o["pred_xstart"].clone()))
    return out


@pytest.fixture(scope="module")
def composed():
    """a guided DDIM scene with a scattered mask, its inversion on both sides (once), and the device objects"""
    from oracle import guidance as og
    sc = step_checks.Scenario("mini", ddim=True, steps=4)
    gen = th.Generator().manual_seed(2468)
    sc.tape["coords"] = [og.generate_coords(sc.H, sc.W, sc.cutn, sc.res, 1.0, generator=gen) for _ in range(4)]
    sc.mask = masked_ref.make_mask((1, 1, sc.H, sc.W), seed=7)
    assert 0 < int((sc.mask == 0).sum()) and 0 < int((sc.mask == 1).sum())
    dev_objs = _make_device(sc)
    d_inv = _device_inversion(sc, sc.skip, dev_objs=dev_objs)[-1]
    o_inv = _oracle_inversion(sc, sc.skip)[-1]
    return sc, dev_objs, d_inv, o_inv


@pytest.mark.parametrize("masked", [False, True])
def test_inversion_then_guided_ddim_steps(composed, masked):
    """device: ddim_invert's noise into the device loop; reference: the restatement's noise into the oracle loop (tests/masked_ref.py under
    the mask).  Both loops get `noise=`, the init image and the same skip, and replay the same tape."""
    sc, dev_objs, d_inv, o_inv = composed
    mask = sc.mask if masked else None
    recs = [pc.rec("compose latent", d_inv["sample"], o_inv["sample"]), pc.rec("compose noise", d_inv["noise"], o_inv["noise"])]
    d_out = _guided_device(sc, mask, dev_objs, d_inv["noise"].to(DEV))
    o_out = _guided_oracle(sc, mask, o_inv["noise"])
    assert len(d_out) == len(o_out) == sc.steps
    for k, ((ds, dx), (os_, ox)) in enumerate(zip(d_out, o_out)):
        recs.append(pc.rec(f"compose{' masked' if masked else ''} step{k} sample", ds, os_))
        recs.append(pc.rec(f"compose{' masked' if masked else ''} step{k} pred_xstart", dx, ox))
        if masked:
            keep = (sc.mask == 0).expand_as(dx)
            assert th.equal(dx[keep], _image(sc)[keep]), "pred_xstart is the init image where the mask is 0"
    _assert_all(recs)


def test_untaped_inversions_repeat_bit_for_bit_and_draw_nothing(composed):
    sc, dev_objs, d_inv, _ = composed
    th.manual_seed(31)
    before = (th.cuda.get_rng_state(0).clone(), th.get_rng_state().clone())
    runs = [_device_inversion(sc, sc.skip, dev_objs=dev_objs) for _ in range(2)]
    assert th.equal(th.cuda.get_rng_state(0), before[0]) and th.equal(th.get_rng_state(), before[1])
    assert len(runs[0]) == len(runs[1]) == sc.t_first
    for a, b in zip(*runs):
        for key in a:
            assert th.isfinite(a[key]).all() and th.equal(a[key], b[key])
    assert th.equal(runs[0][-1]["noise"], d_inv["noise"])


# ---- drop-in -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mask", [False, True])
def test_dropin_generator_starts_from_the_inverted_latent(tmp_path, monkeypatch, with_mask):
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
    loops, inversions = [], []
    plain_loop, plain_invert = sampler.GuidedSampler.ddim_sample_loop_progressive, sampler.GuidedSampler.ddim_invert

    def recording_loop(self, *a, **kw):
        loops.append((kw, []))
        for out in plain_loop(self, *a, **kw):
            loops[-1][1].append(out["pred_xstart"].detach().clone())
            yield out

    def recording_invert(self, model, image, **kw):
        got = plain_invert(self, model, image, **kw)
        again = plain_invert(self, model, image, **dict(kw, progress=False))  # deterministic: the same bits
        inversions.append((image.detach().clone(), kw, [t.detach().clone() for t in got], [t.detach().clone() for t in again]))
        return got

    monkeypatch.setattr(sampler.GuidedSampler, "ddim_sample_loop_progressive", recording_loop)
    monkeypatch.setattr(sampler.GuidedSampler, "ddim_invert", recording_invert)
    value = f"invert={tmp_path / 'a.png'}" + (f"::{tmp_path / 'm.png'}" if with_mask else "")
    items = list(clip_guided_diffusion(prompts=["Loose seal."], image_size=64, batch_size=1, num_cutouts=2, timestep_respacing="ddim8",
                                       init_image=value, seed=7, prefix_path=str(tmp_path / "out"), checkpoints_dir=str(tmp_path / "ckpt"),
                                       save_frequency=1, progress=False, device="cuda"))
    assert len(items) == 8 and all(os.path.isfile(p) for _, p in items)
    (kw, frames), = loops
    (image, inv_kw, (latent, noise), (latent2, noise2)), = inversions
    want_init = th.from_numpy(img).float().div(255).permute(2, 0, 1).unsqueeze(0).mul(2).sub(1)
    assert th.equal(image.cpu(), want_init) and th.equal(kw["init_image"].cpu(), want_init)
    assert inv_kw["skip_timesteps"] == kw["skip_timesteps"] == 0 and not inv_kw.get("clip_denoised")
    assert inv_kw["model_kwargs"]["y"].tolist() == [0]
    assert th.isfinite(noise).all() and th.equal(latent, latent2) and th.equal(noise, noise2)
    assert tuple(kw["noise"].shape) == (1, 3, 64, 64) and th.equal(kw["noise"], noise)  # the loop is handed ddim_invert's noise
    assert len(frames) == 8
    assert (kw.get("mask") is not None) == with_mask
    if with_mask:
        last = frames[-1].cpu()
        assert th.equal(last[..., :32], want_init[..., :32])      # black half: the init image, exactly
        assert not th.equal(last[..., 32:], want_init[..., 32:])  # white half: regenerated
