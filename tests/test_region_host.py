"""Host side of region prompts (cgd_amd/regions.py): the 'TEXT@@REGION[^POWER][:weight]' grammar and its refusals, box rasterisation at the
half-pixel rule, summed-area tables against direct sums, the int32 limit, RegionPlan.coverage against the float64 reference
(tests/region_ref.py), and ClipGuidance's call sequence with a recording library.  No GPU."""
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import guidance as dg
from cgd_amd import regions as rg
from tests import region_ref as R
from tests import test_direction_host as dh


# ---- the prompt grammar -------------------------------------------------------------------------------------------------------------
def test_split_region_grammar():
    from cgd import script_util as su
    assert su.split_region("a cat:0.5") == ("a cat:0.5", None, 1.0)
    assert su.split_region("a castle@@0,0,0.5,1") == ("a castle", "0,0,0.5,1", 1.0)
    assert su.split_region("a castle@@0,0,0.5,1:2") == ("a castle:2", "0,0,0.5,1", 1.0)
    assert su.split_region("a castle@@0,0,0.5,1^2.5:-0.5") == ("a castle:-0.5", "0,0,0.5,1", 2.5)
    assert su.split_region("a castle@@mask.png^3") == ("a castle", "mask.png", 3.0)
    assert su.split_region("a cat=>a dog@@masks/animal.png:1.5") == ("a cat=>a dog:1.5", "masks/animal.png", 1.0)
    assert su.split_region("img.png@@https://host/m.png") == ("img.png", "https://host/m.png", 1.0)
    assert su.split_region("img.png@@https://host/m.png^2:0.25") == ("img.png:0.25", "https://host/m.png", 2.0)
    assert su.split_region("a@@b@@0,0,1,1") == ("a@@b", "0,0,1,1", 1.0)  # the last '@@' separates
    # what reaches the tokenizer and the file name has no '@@' part
    assert su.parse_prompt(su.split_region("a castle@@0,0,0.5,1^2:2")[0]) == ("a castle", 2.0)
    assert su.split_direction(su.parse_prompt(su.split_region("a cat=>a dog@@m.png:1.5")[0])[0]) == ("a cat", "a dog")
    texts, specs = su.split_region_prompts(["a@@0,0,0.5,1", "b", "c@@m.png^2:3"])
    assert texts == ["a", "b", "c:3"] and specs == [("0,0,0.5,1", 1.0), (None, 1.0), ("m.png", 2.0)]
    assert "@@" not in su.clean_and_combine_prompts("out", texts, 0)


@pytest.mark.parametrize("bad,match", [
    ("@@0,0,1,1", "needs a prompt and a region"), ("a cat@@", "needs a prompt and a region"), ("a cat@@:2", "needs a prompt and a region"),
    ("a cat@@0,0,1", "a box is"), ("a cat@@0,0,1,1,1", "a box is"), ("a cat@@0.5,0,0.5,1", "a box is"), ("a cat@@0,0,1.5,1", "a box is"),
    ("a cat@@-0.1,0,1,1", "a box is"), ("a cat@@m.png^0", "positive"), ("a cat@@m.png^-1", "positive"), ("a cat@@m.png^x", "POWER"),
    ("a cat@@m.png^", "POWER"), ("a cat@@m.png^inf", "positive"), ("a cat@@m.png^nan", "positive"), ("a cat@@m.png:heavy", "weight"),
    ("style=s.png@@0,0,1,1", "style="),
])
def test_split_region_refusals(bad, match):
    from cgd import script_util as su
    with pytest.raises(ValueError, match=match):
        su.split_region(bad)


def test_generator_refuses_before_anything_is_loaded(monkeypatch):
    from cgd import cgd as mine
    from cgd import clip_util, script_util

    def no_load(*a, **k):
        raise AssertionError("a refusal must come before any load")

    monkeypatch.setattr(clip_util, "load_clip", no_load)
    monkeypatch.setattr(script_util, "download_guided_diffusion", no_load)
    for kw in (dict(prompts=["a cat@@0,0,1"]), dict(prompts=["a cat@@m.png^0"]), dict(prompts=["a"], image_prompts=["style=s.png@@0,0,1,1"]),
               dict(prompts=["a cat@@0,0,0.5,1"], use_augs=True), dict(prompts=["a"], image_prompts=["i.png@@0,0,0.5,1"], use_augs=True)):
        with pytest.raises(ValueError):
            next(mine.clip_guided_diffusion(device="cuda", **kw))
    text = " ".join(mine.build_parser().format_help().split())
    assert "TEXT@@REGION[^POWER][:weight]" in text


# ---- masks and tables ---------------------------------------------------------------------------------------------------------------
def test_box_rasterisation_at_the_half_pixel_rule():
    m = rg.parse_region("0,0,0.5,1", 4, 6)  # x0 W = 0 <= j + 0.5 < 3: columns 0, 1, 2
    assert m.dtype == th.uint8 and tuple(m.shape) == (4, 6)
    assert th.equal(m, th.tensor([[255, 255, 255, 0, 0, 0]] * 4, dtype=th.uint8))
    # an edge exactly on a pixel centre: x0 W = 1.5 takes column 1 in (>=), x1 W = 3.5 leaves column 3 out (<)
    m = rg.parse_region("0.25,0.125,0.5833333333333334,0.625", 4, 6)
    assert 0.5833333333333334 * 6 == 3.5 and 0.125 * 4 == 0.5 and 0.625 * 4 == 2.5
    want = th.zeros(4, 6, dtype=th.uint8)
    want[0:2, 1:3] = 255
    assert th.equal(m, want)
    # the two halves of a frame of odd width share no pixel and miss none
    a, b = rg.parse_region("0,0,0.5,1", 3, 7), rg.parse_region("0.5,0,1,1", 3, 7)
    assert th.equal(a.int() + b.int(), th.full((3, 7), 255, dtype=th.int32)) and int(a[0].ne(0).sum()) == 3
    with pytest.raises(ValueError, match="no pixel centre"):
        rg.parse_region("0.4,0,0.6,1", 4, 4)  # 1.6 <= j + 0.5 < 2.4: no centre
    with pytest.raises(ValueError, match="a box is"):
        rg.parse_region("0,0,1", 4, 4)


def test_mask_file_is_opened_as_L_and_resized_to_the_frame(tmp_path):
    import numpy as np
    from PIL import Image
    arr = np.zeros((8, 12, 3), dtype=np.uint8)
    arr[:, 6:] = 255
    Image.fromarray(arr).save(tmp_path / "m.png")
    m = rg.parse_region(str(tmp_path / "m.png"), 16, 24)
    assert m.dtype == th.uint8 and tuple(m.shape) == (16, 24) and int(m[:, :10].max()) == 0 and int(m[:, 14:].min()) == 255


def test_build_sat_against_direct_sums_for_every_box_of_a_small_frame():
    Hs, Ws = 7, 5
    masks = th.randint(0, 256, (3, Hs, Ws), generator=th.Generator().manual_seed(3), dtype=th.int64).to(th.uint8)
    sat = rg.build_sat(masks)
    assert sat.dtype == th.int32 and tuple(sat.shape) == (3, Hs + 1, Ws + 1)
    assert not sat[:, 0, :].any() and not sat[:, :, 0].any()
    n = 0
    for r in range(3):
        for oy in range(Hs + 1):
            for ox in range(Ws + 1):
                for h in range(Hs - oy + 1):
                    for w in range(Ws - ox + 1):
                        got = int(sat[r, oy + h, ox + w]) - int(sat[r, oy, ox + w]) - int(sat[r, oy + h, ox]) + int(sat[r, oy, ox])
                        assert got == int(masks[r, oy:oy + h, ox:ox + w].long().sum())
                        n += 1
    assert n == 3 * 36 * 21
    assert th.equal(rg.build_sat([masks[0], masks[1]]), sat[:2])


def test_int32_limit_is_refused():
    # 255 * 2902 * 2902 = 2147509020 >= 2^31 > 255 * 2901 * 2901; the refusal comes before any table is built
    class Huge:
        dtype, shape = th.uint8, (1, 2902, 2902)

        def dim(self):
            return 3

    with pytest.raises(ValueError, match="2\\^31"):
        rg.build_sat(Huge())
    assert 255 * 2901 * 2901 < rg.INT32_LIMIT <= 255 * 2902 * 2902
    with pytest.raises(ValueError, match="uint8"):
        rg.build_sat(th.zeros(1, 4, 4))


def test_plan_refusals_and_shared_tables():
    sat = rg.build_sat(R.make_masks(2, "gray"))
    for bad in ([2], [-2], [0, 5]):
        with pytest.raises(ValueError, match="region_of"):
            rg.RegionPlan(sat, bad)
    with pytest.raises(ValueError, match="positive"):
        rg.RegionPlan(sat, [0], [0.0])
    with pytest.raises(ValueError, match="powers"):
        rg.RegionPlan(sat, [0, 1], [1.0])
    plan = rg.RegionPlan(sat, [0, -1])
    plan.region_of_host[0] = 7  # the host copy is checked again before every launch
    with pytest.raises(ValueError, match="region_of"):
        plan.args(th.zeros(1, 4, dtype=th.int32))
    assert rg.plan_from_specs([(None, 1.0), (None, 1.0)], 8, 8) is None
    plan = rg.plan_from_specs([("0,0,0.5,1", 1.0), (None, 1.0), ("0.5,0,1,1", 2.0), ("0,0,0.5,1", 3.0)], 8, 12)
    assert plan.R == 2 and plan.region_of_host.tolist() == [0, -1, 1, 0] and plan.power_host.tolist() == [1.0, 1.0, 2.0, 3.0]
    assert (plan.H, plan.W) == (8, 12)
    sub = plan.columns([2, 3])
    assert sub.P == 2 and sub.region_of_host.tolist() == [1, 0] and sub.power_host.tolist() == [2.0, 3.0] and sub.sat_host is plan.sat_host


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_plan_coverage_matches_the_reference(case):
    c = R.make_case(case)
    plan = rg.RegionPlan(rg.build_sat(c["masks"]), c["region_of"], c["power"])
    got = plan.coverage(R.BOXES)
    want = R.coverage(c["masks"], c["region_of"], c["power"], R.BOXES)
    assert got.dtype == th.float64 and float((got - want).abs().max()) <= 1e-15
    regioned = [p for p, r in enumerate(c["region_of"]) if r >= 0]
    assert not got[R.EMPTY, regioned].any() and float(got[:, [p for p, r in enumerate(c["region_of"]) if r < 0]].sub(1).abs().sum()) == 0
    if 0 in c["region_of"]:
        assert float(got[R.OUTSIDE, c["region_of"].index(0)]) == 0.0
    assert 0 < float(got[0, regioned[0]]) < 1


def test_boxes_of_restates_the_uploaded_tables():
    coords = [(0, 0, 32), (20, 10, 30), (40, 30, 8)]
    assert rg.boxes_of(coords, 32, 48) == dg.crop_geometry(coords, 32, 48)
    recs = [(0, 0, 48, 32, 0), (3, 5, 20, 16, dg.RESIZE_FLIP)]
    assert rg.boxes_of(recs, 32, 48, resized=True) == dg.resize_table(recs, 32, 48)[:2]


# ---- ClipGuidance with a recording library --------------------------------------------------------------------------------------------
B, H, W = dh.B, dh.H, dh.W


def _plan(specs):
    return rg.plan_from_specs(specs, H, W)


def _run(guid, tape=None):
    guid.current_timestep, guid.coords_tape = 49, [tape or [(0, 0, 32)] * 6]
    x = th.zeros(B, 3, H, W)
    return guid.native(x, x.clone(), x.clone(), coef=None)


def test_without_regions_the_entries_called_are_todays():
    r = dh._Recorder()
    vit, rn = r.tower("vit", 32, 8, 16), r.tower("rn", 64, 0, 24)
    guid = dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, [th.randn(1, 16), th.randn(1, 24)], [0.5], 6,
                           direction_embeds=[th.randn(1, 16), th.randn(1, 24)], direction_weights=[0.75], direction_source=th.zeros(1, 3, H, W),
                           regions=None)
    _run(guid)
    assert r.names() == dh.leg("vit") + dh.leg("rn") + dh.TAIL
    assert len(r.args("cgd_spherical_loss")[0]) == 12 and len(r.args("cgd_directional_loss")[0]) == 15
    r2 = dh._Recorder()
    guid = dg.ClipGuidance(r2.ctx, r2.unet, r2.tower("vit", 32, 8, 16), r2.diffusion, th.randn(2, 16), [0.5, 0.5], 6)
    _run(guid)
    assert r2.names() == ["cgd_cutouts_fwd", "vit.encode_image", "cgd_spherical_loss", "vit.dgrad", "cgd_cutouts_bwd"] + dh.TAIL


def test_with_regions_the_regions_entries_get_the_plans_pointers():
    r = dh._Recorder()
    vit, rn = r.tower("vit", 32, 8, 16), r.tower("rn", 64, 0, 24)
    # the weight list: target, direction (column 1), target
    plan = _plan([("0,0,0.5,1", 1.0), ("0.5,0,1,1", 2.0), (None, 1.0)])
    guid = dg.ClipGuidance(r.ctx, r.unet, [vit, rn], r.diffusion, [th.randn(2, 16), th.randn(2, 24)], [0.5, 0.25], 6,
                           direction_embeds=[th.randn(1, 16), th.randn(1, 24)], direction_weights=[0.75], direction_columns=[1],
                           direction_source=th.zeros(1, 3, H, W), regions=plan)
    x = th.zeros(1, 3, H, W)
    guid.current_timestep, guid.coords_tape = 49, [[(0, 0, 32)] * 6]
    guid.native(x, x.clone(), x.clone(), coef=None)
    swap = {"cgd_spherical_loss": "cgd_spherical_loss_regions", "cgd_directional_loss": "cgd_directional_loss_regions"}
    assert r.names() == [swap.get(n, n) for n in dh.leg("vit") + dh.leg("rn") + dh.TAIL]  # the same launches, through the other entries
    sph, drc = r.args("cgd_spherical_loss_regions"), r.args("cgd_directional_loss_regions")
    geo = r.args("cgd_cutouts_fwd")[0][2]
    t, d = guid._reg_t, guid._reg_d
    assert t.region_of_host.tolist() == [0, -1] and t.power_host.tolist() == [1.0, 1.0] and d.region_of_host.tolist() == [1]
    assert d.power_host.tolist() == [2.0] and t.sat is d.sat is plan.sat
    for call in sph:  # (..., scale, sat, region_of, region_of_host, power, geo, R, H, W, stream)
        assert call[6:11] == (6, 1, 2, call[9], 1000.0) and len(call) == 20
        assert call[11:19] == (plan.sat.data_ptr(), t.region_of.data_ptr(), t.region_of_host.data_ptr(), t.power.data_ptr(), geo, 2, H, W)
    for call in drc:
        assert call[7:11] == (6, 1, 1, 1) and call[12:14] == (1000.0, 1) and len(call) == 23
        assert call[14:22] == (plan.sat.data_ptr(), d.region_of.data_ptr(), d.region_of_host.data_ptr(), d.power.data_ptr(), geo, 2, H, W)
    assert [c[9] for c in sph] == [16, 24] and [c[11] for c in drc] == [16, 24]


def test_regions_on_the_resized_cutter_read_the_resize_table():
    r = dh._Recorder()
    mk = dg.MakeCutoutsResized(32, overview=2, inner=1)
    guid = dg.ClipGuidance(r.ctx, r.unet, r.tower("vit", 32, 8, 16), r.diffusion, th.randn(1, 16), [1.0], 3, make_cutouts=mk,
                           regions=_plan([("0,0,0.5,1", 1.0)]))
    _run(guid, [(0, 0, W, H, 0), (0, 0, W, H, dg.RESIZE_FLIP), (3, 5, 20, 16, 0)])
    assert "cgd_spherical_loss_regions" in r.names() and "cgd_spherical_loss" not in r.names()
    assert r.args("cgd_spherical_loss_regions")[0][15] == r.args("cgd_cutouts_resize_fwd")[0][2]  # its first cutn rows are the boxes


def test_refusals_of_the_guidance_object():
    r = dh._Recorder()
    vit = r.tower("vit", 32, 8, 16)
    plan = _plan([("0,0,0.5,1", 1.0)])
    with pytest.raises(ValueError, match="use_augs"):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 6, make_cutouts=dg.MakeCutouts(32, 6, use_augs=True),
                        regions=plan)
    with pytest.raises(ValueError, match="covers 1 prompts, the weights 2"):
        dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(2, 16), [0.5, 0.5], 6, regions=plan)
    guid = dg.ClipGuidance(r.ctx, r.unet, vit, r.diffusion, th.randn(1, 16), [1.0], 6, regions=rg.plan_from_specs([("0,0,0.5,1", 1.0)], H, W + 8))
    with pytest.raises(ValueError, match="the region masks are"):
        _run(guid)
    assert not r.calls
