"""Host side of the directional CLIP loss (csrc/direction.hip): the float64 reference (tests/direction_ref.py) against finite differences and
its invariances, the 'SOURCE=>TARGET' prompt parser and its refusals, and ClipGuidance's call sequence with a recording library.  No GPU."""
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import guidance as dg
from tests import direction_ref as R


# ---- the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2, 1, 2, 24), (2, 3, 3, 3, 17)])
def test_reference_gradient_matches_central_differences(shape):
    cutn, B, _, _, D = shape
    e, s, d, w = (t.double() for t in R.make_case(shape))
    _, g, _ = R.loss_and_grad(e, s, d, w, cutn, B)
    h = 1e-6
    fd = th.zeros_like(g)
    for r in range(e.shape[0]):
        for c in range(D):
            ep, em = e.clone(), e.clone()
            ep[r, c] += h
            em[r, c] -= h
            fd[r, c] = (R.rows(ep, s, d, w, cutn, B)[0].sum() - R.rows(em, s, d, w, cutn, B)[0].sum()) / (2 * h)
    err = float((fd - g).abs().max())
    print(f"{shape}: |autograd - central differences| {err:.3e}, peak |g| {float(g.abs().max()):.3e}")
    assert err <= 1e-6 * max(1.0, float(g.abs().max()))


def test_reference_invariances():
    shape = (3, 2, 1, 2, 48)
    cutn, B = shape[:2]
    e, s, d, w = (t.double() for t in R.make_case(shape))
    loss, g, _ = R.loss_and_grad(e, s, d, w, cutn, B)
    # the source's length does not matter
    loss_s, g_s, _ = R.loss_and_grad(e, 37.5 * s, d, w, cutn, B)
    assert float((loss_s - loss).abs().max()) <= 1e-12 * float(loss.abs().max()) and float((g_s - g).abs().max()) <= 1e-12 * float(g.abs().max())
    # scaling e by k keeps the loss and scales the gradient by 1 / k
    loss_k, g_k, _ = R.loss_and_grad(8.0 * e, s, d, w, cutn, B)
    assert float((loss_k - loss).abs().max()) <= 1e-12 * float(loss.abs().max())
    assert float((8.0 * g_k - g).abs().max()) <= 1e-12 * float(g.abs().max())
    # the gradient is orthogonal to e
    assert float((g * e).sum(1).abs().max()) <= 1e-12 * float(g.norm(dim=1).max() * e.norm(dim=1).max())
    assert float(g.abs().max()) > 0


def test_reference_row_without_a_direction():
    shape = (2, 2, 2, 3, 32)
    cutn, B = shape[:2]
    e, s, d, w = R.make_case(shape)
    e[1] = 2 * R.source_rows(s, cutn, B)[1]
    loss, g, n = R.loss_and_grad(e, s, d, w, cutn, B)
    assert float(n[1]) <= 1e-6
    assert float(loss[1]) == pytest.approx(R.SCALE / cutn * float(w[1 % B].double().sum()), rel=1e-12)
    assert not g[1].any() and all(bool(g[r].any()) for r in (0, 2, 3))


def test_reference_shared_source_equals_the_repeated_source():
    shape = (3, 2, 1, 2, 40)
    cutn, B = shape[:2]
    e, s, d, w = R.make_case(shape)
    rep = s.repeat_interleave(B, dim=0)  # row cut * B + b = the shared row of the cut
    a, b = R.loss_and_grad(e, s, d, w, cutn, B), R.loss_and_grad(e, rep, d, w, cutn, B)
    assert th.equal(a[0], b[0]) and th.equal(a[1], b[1])


def test_case_builder_reaches_the_stated_regimes():
    for shape in R.SHAPES:
        cutn, B = shape[:2]
        e, s, d, w = R.make_case(shape)
        n = R.rows(e, s, d, w, cutn, B)[2]
        assert 0.7 <= float(n.min()) and float(n.max()) <= 1.4
        assert float((d.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    seen = set()
    for seed in range(3):
        e, s, d, w = R.make_case(R.SHAPES[0], "stressed", seed)
        n = R.rows(e, s, d, w, 3, 2)[2]
        seen |= {(round(float(a), 2), float(f"{float(b):.0e}")) for a, b in zip(n, e.double().norm(dim=1))}
    assert seen == {(a, b) for a in R.STRESS_N for b in R.STRESS_E}


# ---- the prompt parser --------------------------------------------------------------------------------------------------------------
def test_direction_prompt_parsing_and_refusals():
    from cgd import script_util as su
    assert su.split_direction("a cat") is None
    assert su.split_direction(su.parse_prompt("a photo of a cat=>a photo of a dog:1.5")[0]) == ("a photo of a cat", "a photo of a dog")
    assert su.parse_prompt("a photo of a cat=>a photo of a dog:1.5")[1] == 1.5
    assert su.split_direction(" x => y=>z ") == ("x", "y=>z")  # the first '=>' separates
    for bad in ("=>a dog", "a cat=>", " => ", "a cat=>  :2"):
        with pytest.raises(ValueError, match="both sides"):
            su.direction_prompts([bad], [], "init.png")
    assert su.direction_prompts(["a cat", "a cat=>a dog:2"], [], "init.png") == [None, ("a cat", "a dog")]
    assert su.direction_prompts(["a cat", "a dog:-1"], ["img.png"], None) == [None, None]  # no direction: nothing else is checked
    for init in (None, ""):
        with pytest.raises(ValueError, match="init image"):
            su.direction_prompts(["a cat=>a dog"], [], init)
    with pytest.raises(ValueError, match="image prompt"):
        su.direction_prompts(["a cat"], ["a.png=>b.png"], "init.png")
    with pytest.raises(ValueError, match="offset"):
        su.direction_prompts(["a cat=>a dog"], [], "init.png", 0, 64)
    with pytest.raises(RuntimeError, match="sum to 0"):
        su.direction_prompts(["a tree:1", "a cat=>a dog:-1"], [], "init.png")  # across both kinds
    su.direction_prompts(["a tree:1", "a cat=>a dog:-1", "a house:0.5"], [], "invert=init.png::mask.png")


def test_generator_refuses_before_anything_is_loaded(monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    monkeypatch.setattr(clip_util, "load_clip", no_load)
    monkeypatch.setattr(script_util, "download_guided_diffusion", no_load)
    for kw in (dict(prompts=["a cat=>a dog"]), dict(prompts=["=>a dog"], init_image="i.png"), dict(prompts=["a cat=>"], init_image="i.png"),
               dict(prompts=["a cat"], image_prompts=["a.png=>b.png"], init_image="i.png"),
               dict(prompts=["a cat=>a dog"], init_image="i.png", use_augs=True),
               dict(prompts=["a cat=>a dog"], init_image="i.png", width_offset=64)):
        with pytest.raises(ValueError):
            next(mine.clip_guided_diffusion(device="cuda", **kw))
    with pytest.raises(RuntimeError, match="sum to 0"):
        next(mine.clip_guided_diffusion(device="cuda", prompts=["a tree:1", "a cat=>a dog:-1"], init_image="i.png"))
    text = " ".join(mine.build_parser().format_help().split())
    assert "SOURCE CAPTION=>TARGET CAPTION" in text and "source image of 'SOURCE=>TARGET'" in text


# ---- ClipGuidance with a recording library --------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = calls = []

        class FakeLib:
            def __getattr__(self, name):
                def fn(*args):
                    calls.append((name, args))
                    return {"cgd_guidance_part_blocks": 32, "cgd_cutouts_resize_scratch_floats": 7}.get(name, 0)
                return fn

        self.ctx = types.SimpleNamespace(lib=FakeLib(), h=1, check=lambda rc: None, stream=lambda: 0)
        self.unet = types.SimpleNamespace(dgrad=lambda seed, out: calls.append(("unet.dgrad", ())) or out)
        self.diffusion = types.SimpleNamespace(num_timesteps=50)

    def tower(self, name, res, patch, dim):
        calls = self.calls

        class Tower:
            input_resolution, out_dim = res, dim

            def encode_image(self, img, layout=0, n=None, out=None):
                calls.append((f"{name}.encode_image", (layout, n, tuple(img.shape), img.data_ptr(), out.data_ptr())))
                return out

            def dgrad(self, d_emb, d_img=None):
                calls.append((f"{name}.dgrad", (tuple(d_emb.shape),)))
                return d_img

        t = Tower()
        t.patch = patch
        return t

    def names(self):
        return [c[0] for c in self.calls]

    def args(self, name):
        return [c[1] for c in self.calls if c[0] == name]


B, H, W = 2, 32, 48
TAIL = ["cgd_guidance_part_blocks", "cgd_guidance_combine", "unet.dgrad", "cgd_grad_finish", "cgd_scalars"]


def leg(tower, cut="cgd_cutouts", targets=True, source=True):
    src = [f"{cut}_fwd", f"{tower}.encode_image"] if source else []
    return src + [f"{cut}_fwd", f"{tower}.encode_image"] + (["cgd_spherical_loss"] if targets else []) + [
        "cgd_directional_loss", f"{tower}.dgrad", f"{cut}_bwd"]


def test_call_sequence_with_targets_and_directions_on_two_towers():
    r = _Recorder()
    vit, rn = r.tower("vit", 32, 8, 16), r.tower("rn", 64, 0, 24)
    guid = dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, [th.randn(1, 16), th.randn(1, 24)], [0.5], 6,
                           direction_embeds=[th.randn(1, 16), th.randn(1, 24)], direction_weights=[0.75], direction_source=th.zeros(1, 3, H, W))
    guid.current_timestep, guid.coords_tape = 49, [[(0, 0, 32)] * 6]
    x = th.zeros(B, 3, H, W)
    g = guid.native(x, x.clone(), x.clone(), coef=None)
    assert r.names() == leg("vit") + leg("rn") + TAIL and tuple(g.shape) == (B, 3, H, W)
    fwd = r.args("cgd_cutouts_fwd")  # (h, image, boxes, out, B, H, W, cutn, cut_size, layout, patch, stream)
    assert [f[4] for f in fwd] == [1, B, 1, B]  # the shared source goes first, at its own batch size, on the same boxes
    assert len({f[2] for f in fwd}) == 1 and fwd[0][1] != fwd[1][1] and fwd[0][3] != fwd[1][3]  # buffers of its own
    assert fwd[0][5:11] == fwd[1][5:11] == (H, W, 6, 32, 1, 8) and fwd[2][5:11] == fwd[3][5:11] == (H, W, 6, 64, 0, 0)
    enc = r.args("vit.encode_image")
    assert [e[:3] for e in enc] == [(1, 6, (6 * 16, 3 * 64)), (1, 12, (12 * 16, 3 * 64))] and enc[0][4] != enc[1][4]
    assert [e[:3] for e in r.args("rn.encode_image")] == [(0, 6, (6, 3, 64, 64)), (0, 12, (12, 3, 64, 64))]
    sph, drc = r.args("cgd_spherical_loss"), r.args("cgd_directional_loss")
    # (h, emb, src_emb, dirs, weights, d_emb, loss_part, cutn, B, Bs, P, D, scale, accumulate, stream)
    assert drc[0][7:14] == (6, B, 1, 1, 16, 1000.0, 1) and drc[1][7:14] == (6, B, 1, 1, 24, 1000.0, 1)
    assert drc[0][2] == enc[0][4] and drc[0][1] == enc[1][4] == sph[0][1] and drc[0][5] == sph[0][4]  # onto the spherical gradient
    # partial rows: per tower the N spherical rows, then the N directional rows
    N = 6 * B
    assert [s[5] - sph[0][5] for s in sph] == [0, 4 * 2 * N] and [d[6] - sph[0][5] for d in drc] == [4 * N, 4 * 3 * N]
    assert r.args("cgd_scalars")[0][2] == 2 * N * 2 and guid.clip_part.numel() == 2 * N * 2
    assert [c[-2] for c in r.args("cgd_cutouts_bwd")] == [0, 1]
    # the weight matrix is built over the whole list (B == P == 2 pairs sample b with prompt b, scaled by sum(w)) and split by column
    assert th.equal(guid._wm[B], th.tensor([[1.25], [0.0]])) and th.equal(guid._wmd[B], th.tensor([[0.0], [1.25]]))
    assert sph[0][8] == 1 and sph[0][3] == guid._wm[B].data_ptr() and drc[0][4] == guid._wmd[B].data_ptr()
    assert list(guid.log()) == ["CLIP Loss", "Range Loss", "TV Loss", "Direction Loss", "Total Loss", "Grad"]


def test_call_sequence_with_directions_only_and_a_per_sample_source():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, None, None, 6, direction_embeds=th.randn(2, 16), direction_weights=[1.0, 2.0],
                           direction_source=th.zeros(B, 3, H, W))
    guid.current_timestep, guid.coords_tape = 49, [[(0, 0, 32)] * 6]
    x = th.zeros(B, 3, H, W)
    guid.native(x, x.clone(), x.clone(), coef=None)
    assert r.names() == leg("vit", targets=False) + TAIL and "cgd_spherical_loss" not in r.names()
    drc = r.args("cgd_directional_loss")[0]
    assert drc[7:14] == (6, B, B, 2, 16, 1000.0, 0)  # nothing wrote d_emb before: accumulate 0
    assert r.args("cgd_scalars")[0][2] == 6 * B and [f[4] for f in r.args("cgd_cutouts_fwd")] == [B, B]
    # B == P pairs sample b with prompt b over the WHOLE list (here the two directions): eye * sum(w)
    assert th.equal(guid._wmd[B], th.eye(2) * 3.0) and guid._wm[B].shape == (B, 0)


def test_weight_columns_follow_the_order_the_prompts_were_given():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [0.25], 6, direction_embeds=th.randn(1, 16),
                           direction_weights=[0.75], direction_columns=[0], direction_source=th.zeros(1, 3, H, W))
    guid.current_timestep, guid.coords_tape = 49, [[(0, 0, 32)] * 6]
    x = th.zeros(B, 3, H, W)
    guid.native(x, x.clone(), x.clone(), coef=None)
    # B == P == 2: sample 0 is paired with the first prompt of the list, the direction; sample 1 with the target
    assert th.equal(guid._wmd[B], th.tensor([[1.0], [0.0]])) and th.equal(guid._wm[B], th.tensor([[0.0], [1.0]]))
    # sharded: rows of the global matrix, as the target prompts take them
    guid2 = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [0.25], 6, direction_embeds=th.randn(1, 16),
                            direction_weights=[0.75], direction_columns=[0], direction_source=th.zeros(1, 3, H, W))
    guid2.current_timestep, guid2.coords_tape, guid2.shard = 49, [[(0, 0, 32)] * 6], ([1], 2)
    guid2.native(x[:1], x[:1].clone(), x[:1].clone(), coef=None)
    assert th.equal(guid2._wmd[1], th.tensor([[0.0]])) and th.equal(guid2._wm[1], th.tensor([[1.0]]))


def test_call_sequence_with_the_resized_cutter():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    mk = dg.MakeCutoutsResized(32, overview=2, inner=3)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 16, make_cutouts=mk, direction_embeds=th.randn(1, 16),
                           direction_weights=[1.0], direction_source=th.zeros(1, 3, H, W))
    guid.current_timestep = 49
    x = th.zeros(B, 3, H, W)
    th.manual_seed(3)
    guid.native(x, x.clone(), x.clone(), coef=None)
    assert r.names() == ["cgd_cutouts_resize_scratch_floats"] + leg("vit", "cgd_cutouts_resize") + TAIL
    fwd, bwd = r.args("cgd_cutouts_resize_fwd"), r.args("cgd_cutouts_resize_bwd")  # (h, image, boxes, flags, out, B, H, W, cutn, cs, layout, patch, s)
    assert [f[5] for f in fwd] == [1, B] and fwd[0][2:4] == fwd[1][2:4] == bwd[0][2:4] and fwd[0][3] == fwd[0][2] + 16 * 5  # one table: boxes and flags
    assert fwd[0][6:12] == fwd[1][6:12] == (H, W, 5, 32, 1, 8) and [e[:2] for e in r.args("vit.encode_image")] == [(1, 5), (1, 5 * B)]


def test_cached_cutouts_run_the_source_forward_once_per_cut_count():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 16, cached_cutouts=True, progressive_cutout=True,
                           direction_embeds=th.randn(1, 16), direction_weights=[1.0], direction_source=th.zeros(1, 3, H, W))
    th.manual_seed(4)
    guid.make_cutouts.cache_coordinates(H, W)
    x = th.zeros(B, 3, H, W)
    seen = []
    for timestep in (49, 48, 30, 29):  # 2 % and 4 % done: 4 cuts; 40 % and 42 %: 8 cuts
        del r.calls[:]
        guid.current_timestep = timestep
        guid.native(x, x.clone(), x.clone(), coef=None)
        seen.append((r.args("cgd_cutouts_fwd")[0][7], len(r.args("vit.encode_image")), r.args("cgd_directional_loss")[0][2]))
        assert r.names() == leg("vit", source=len(r.args("vit.encode_image")) == 2) + TAIL
    assert [s[:2] for s in seen] == [(4, 2), (4, 1), (8, 2), (8, 1)]
    assert seen[0][2] == seen[1][2] and seen[2][2] == seen[3][2] and seen[0][2] != seen[2][2]  # the kept embeddings reach the loss
    # without cached_cutouts every step embeds the source
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 4, direction_embeds=th.randn(1, 16),
                           direction_weights=[1.0], direction_source=th.zeros(1, 3, H, W))
    for timestep in (49, 48):
        del r.calls[:]
        guid.current_timestep = timestep
        guid.native(x, x.clone(), x.clone(), coef=None)
        assert r.names() == leg("vit") + TAIL


def test_refusals_of_the_class():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    kw = dict(direction_embeds=th.randn(1, 16), direction_weights=[1.0])
    with pytest.raises(ValueError, match="use_augs"):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 4, direction_source=th.zeros(1, 3, H, W),
                        make_cutouts=dg.MakeCutouts(32, 4, use_augs=True), **kw)
    with pytest.raises(ValueError, match="direction_source"):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 4, **kw)
    x = th.zeros(B, 3, H, W)
    for bad in (th.zeros(1, 3, H, W + 8), th.zeros(3, 3, H, W)):
        guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 4, direction_source=bad, **kw)
        guid.current_timestep, guid.coords_tape = 49, [[(0, 0, 32)] * 4]
        del r.calls[:]
        with pytest.raises(ValueError, match="direction_source"):
            guid.native(x, x.clone(), x.clone(), coef=None)
        assert not r.calls


def test_without_direction_prompts_nothing_changes():
    r = _Recorder()
    vit = r.tower("vit", 32, 8, 16)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(2, 16), [1.0, 0.5], 6)
    guid.current_timestep, guid.coords_tape = 49, [[(0, 0, 32)] * 6]
    x = th.zeros(B, 3, H, W)
    guid.native(x, x.clone(), x.clone(), coef=None)
    assert r.names() == ["cgd_cutouts_fwd", "vit.encode_image", "cgd_spherical_loss", "vit.dgrad", "cgd_cutouts_bwd"] + TAIL
    assert r.args("cgd_scalars")[0][2] == 6 * B
    assert list(guid.log()) == ["CLIP Loss", "Range Loss", "TV Loss", "Total Loss", "Grad"]
    assert not any(k.startswith("src_") for k in guid._buf)
