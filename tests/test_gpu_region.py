"""Region prompts on the GPU.  Op level: cgd_op_region_coverage, cgd_spherical_loss_regions and cgd_directional_loss_regions through the C ABI
against the float64 reference (tests/region_ref.py: coverage by direct sums of the mask) at the literal |a - b| <= 1e-4 + 1e-3 |ref|; on the
stressed value set each row's gradient is first multiplied by |e_r| (and n_r for the directional loss: it is homogeneous of degree -1 in both)
and the tensor brought to unit peak.  Bit-for-bit anchors against the plain entries, the skipping rules, determinism and the -2 returns.
Step level: ClipGuidance.native with a region plan against the same step with the CLIP leg restated in torch ops (_clip_leg_torch), and one
short run of the drop-in generator."""
import ctypes as C
import functools
import math
import os

import pytest
import torch as th

from tests import direction_ref as D
from tests import parity_checks as pc
from tests import region_ref as R
from tests.parity_checks import DEV, g, rec

pytestmark = pytest.mark.gpu

PAD = 5  # the outputs are allocated this many floats too long
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _ctx():
    return pc._ctx(1)


@functools.lru_cache(maxsize=None)
def _case(case, kind="ordinary", seed=0):
    """inputs and the float64 references of a case, computed once and never modified"""
    c = R.make_case(case, kind, seed)
    c["sph_loss"], c["sph_grad"] = R.spherical(c["e"], c["d"], c["weff"], c["cutn"])
    c["dir_loss"], c["dir_grad"], c["n"] = R.directional(c["e"], c["s"], c["d"], c["weff"], c["cutn"], c["B"])
    return c


def _sat(masks):
    from cgd_amd import regions
    return regions.build_sat(masks)


class Regions:
    """device copies of a case's region arguments and the trailing arguments of a `_regions` entry"""

    def __init__(self, c, region_of=None, power=None, masks=None, boxes=None, host_region_of=None, R_=None, H=R.H, W=R.W):
        self.sat = _sat(c["masks"] if masks is None else masks).to(DEV)
        ro = list(c["region_of"] if region_of is None else region_of)
        self.region_of = th.tensor(ro, dtype=th.int32, device=DEV)
        self.region_of_host = th.tensor(ro if host_region_of is None else host_region_of, dtype=th.int32)
        self.power = th.tensor(c["power"] if power is None else power, dtype=th.float32, device=DEV)
        self.geo = th.tensor(c["boxes"] if boxes is None else boxes, dtype=th.int32, device=DEV).view(-1, 4)
        self.R, self.H, self.W = self.sat.shape[0] if R_ is None else R_, H, W
        self.null = ()

    def args(self):
        ptrs = {"sat": self.sat, "region_of": self.region_of, "region_of_host": self.region_of_host, "power": self.power, "geo": self.geo}
        return tuple(None if k in self.null else t.data_ptr() for k, t in ptrs.items()) + (self.R, self.H, self.W)


def run(kind, c, rg=None, e=None, t=None, w=None, shape=None, s=None, accumulate=0, prefill=NAN, scale=R.SCALE, check=True):
    """One launch of cgd_<kind>_loss[_regions] (rg None: the plain entry) -> (d_emb (N, D), loss_part (N,), the two padding tails, return code)"""
    ctx = _ctx()
    cutn, B, P, Dm = shape or (c["cutn"], c["B"], c["P"], c["D"])
    N = cutn * B
    ed, sd, td, wd = (x.float().contiguous().to(DEV) for x in (c["e"] if e is None else e, c["s"] if s is None else s,
                                                                c["d"] if t is None else t, c["w"] if w is None else w))
    demb = th.full((N * Dm + PAD,), NAN, device=DEV)
    if isinstance(prefill, th.Tensor):
        demb[:N * Dm] = prefill.to(DEV).reshape(-1)
    else:
        demb[:N * Dm] = prefill
    part = th.full((N + PAD,), NAN, device=DEV)
    tail = () if rg is None else rg.args()
    name = f"cgd_{kind}_loss" + ("" if rg is None else "_regions")
    if kind == "spherical":
        rc = getattr(ctx.lib, name)(ctx.h, ed.data_ptr(), td.data_ptr(), wd.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B, P, Dm, scale,
                                    *tail, ctx.stream())
    else:
        Bs = sd.shape[0] // cutn
        rc = getattr(ctx.lib, name)(ctx.h, ed.data_ptr(), sd.data_ptr(), td.data_ptr(), wd.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B,
                                    Bs, P, Dm, scale, accumulate, *tail, ctx.stream())
    if check:
        ctx.check(rc)
    th.cuda.synchronize()
    return demb[:N * Dm].view(N, Dm).cpu(), part[:N].cpu(), (demb[N * Dm:].cpu(), part[N:].cpu()), rc


def tails_untouched(tails):
    return all(bool(th.isnan(t).all()) and t.numel() == PAD for t in tails)


def grade(tag, got_g, got_l, ref_l, ref_g, scale_rows=None):
    ok_l, use_l = D.within(got_l.double().sum().view(1), ref_l.sum().view(1))
    if scale_rows is not None:
        a, b = D.unit_peak(got_g.double() * scale_rows, ref_g * scale_rows)
    else:
        a, b = got_g.double(), ref_g
    ok_g, use_g = D.within(a, b)
    print(f"{tag}: loss sum {float(got_l.double().sum()):.6f} (ref {float(ref_l.sum()):.6f}), use of the bound: loss {use_l:.4f}, gradient "
          f"{use_g:.4f} ({'rows scaled, unit peak' if scale_rows is not None else 'as it stands'}; peak |ref| {float(b.abs().max()):.3e}, "
          f"peak |ref loss| {float(ref_l.abs().max()):.3e})")
    assert float(b.abs().max()) >= 100 * 1e-4 and float(ref_l.abs().max()) >= 100 * 1e-4, "a reference this small would pass on atol alone"
    assert ok_l and ok_g, tag
    assert D.within(got_l, ref_l)[0], tag  # every row's own partial loss too


# ---- the coverage op --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_coverage_op_against_direct_sums_for_every_box(case):
    c = _case(case)
    ctx, rg = _ctx(), Regions(c, boxes=R.BOXES)
    n, P = len(R.BOXES), c["P"]
    out = th.full((n * P + PAD,), NAN, device=DEV)
    ctx.check(ctx.lib.cgd_op_region_coverage(ctx.h, *rg.args()[:5], out.data_ptr(), n, P, *rg.args()[5:], ctx.stream()))
    th.cuda.synchronize()
    got, want = out[:n * P].view(n, P).cpu(), R.coverage(c["masks"], c["region_of"], c["power"], R.BOXES)
    ok, use = D.within(got, want)
    print(f"coverage {R.case_id(case)}: use of the bound {use:.4f}, peak |ref| {float(want.abs().max()):.3e}\n{got}")
    assert float(want.abs().max()) >= 100 * 1e-4 and ok
    assert bool(th.isnan(out[n * P:]).all())
    regioned = [p for p, r in enumerate(c["region_of"]) if r >= 0]
    assert not got[R.EMPTY, regioned].view(th.int32).any(), "an empty box has coverage 0"
    assert all(float(got[k, p]) == 1.0 for k in range(n) for p, r in enumerate(c["region_of"]) if r < 0)
    if 0 in c["region_of"]:
        assert float(got[R.OUTSIDE, c["region_of"].index(0)]) == 0.0


def test_coverage_of_a_full_mask_is_exactly_one():
    c = _case(R.CASES[0])
    ctx, rg = _ctx(), Regions(c, masks=th.full((2, R.H, R.W), 255, dtype=th.uint8), boxes=R.BOXES, power=[1.0] * 3)
    out = th.empty((len(R.BOXES), 3), device=DEV)
    ctx.check(ctx.lib.cgd_op_region_coverage(ctx.h, *rg.args()[:5], out.data_ptr(), len(R.BOXES), 3, *rg.args()[5:], ctx.stream()))
    want = th.ones(len(R.BOXES), 3)
    want[R.EMPTY, [p for p, r in enumerate(c["region_of"]) if r >= 0]] = 0
    assert th.equal(out.cpu(), want)


# ---- both losses against the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spherical", "directional"])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_ordinary_values_against_the_reference(case, kind):
    c = _case(case)
    got_g, got_l, tails, _ = run(kind, c, Regions(c))
    key = kind[:3]
    grade(f"{kind} regions {R.case_id(case)} ordinary", got_g, got_l, c[f"{key}_loss"], c[f"{key}_grad"])
    assert tails_untouched(tails), "the padding behind the outputs was written"


@pytest.mark.parametrize("kind", ["spherical", "directional"])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[3]], ids=R.case_id)
def test_stressed_values_against_the_reference(case, seed, kind):
    c = _case(case, "stressed", seed)
    got_g, got_l, tails, _ = run(kind, c, Regions(c))
    f = c["e"].double().norm(dim=1)[:, None] if kind == "spherical" else D.degree_scale(c["e"], c["n"])
    key = kind[:3]
    grade(f"{kind} regions {R.case_id(case)} stressed/{seed}", got_g, got_l, c[f"{key}_loss"], c[f"{key}_grad"], scale_rows=f)
    assert tails_untouched(tails)


# ---- bit-for-bit anchors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spherical", "directional"])
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[2], R.CASES[3]], ids=R.case_id)
def test_without_a_region_the_outputs_are_those_of_the_plain_entry(case, kind):
    c = _case(case)
    plain = run(kind, c)
    everywhere = run(kind, c, Regions(c, region_of=[-1] * c["P"]))
    assert th.equal(plain[0], everywhere[0]) and th.equal(plain[1], everywhere[1]) and tails_untouched(everywhere[2])
    # a mask of all 255 at power 1 has coverage exactly 1 on every box that is not empty
    cutn = c["cutn"]
    boxes = [b for b in c["boxes"]]
    if cutn == len(R.BOXES):
        boxes[R.EMPTY] = (3, 3, 4, 9)
    full = run(kind, c, Regions(c, masks=th.full((c["R"], R.H, R.W), 255, dtype=th.uint8), power=[1.0] * c["P"], boxes=boxes))
    assert th.equal(plain[0], full[0]) and th.equal(plain[1], full[1])


@pytest.mark.parametrize("kind", ["spherical", "directional"])
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[1]], ids=R.case_id)
def test_power_one_equals_the_plain_entry_on_precomputed_weights(case, kind):
    """w * cov as float weights of cutn * B 'samples' of one cut each, at clip_guidance_scale / cutn: the same c for every row"""
    c = _case(case)
    cutn, B, P, Dm = c["cutn"], c["B"], c["P"], c["D"]
    one = [1.0] * P
    cov = R.coverage(c["masks"], c["region_of"], one, c["boxes"])
    weff = R.effective_weights(c["w"], cov, B)
    got_g, got_l, _, _ = run(kind, c, Regions(c, power=one))
    ref_g, ref_l, _, _ = run(kind, c, None, w=weff.float(), shape=(1, cutn * B, P, Dm), s=D.source_rows(c["s"], cutn, B), scale=R.SCALE / cutn)
    ok_g, use_g = D.within(got_g, ref_g)
    ok_l, use_l = D.within(got_l, ref_l)
    print(f"{kind} {R.case_id(case)}: use of the bound against the plain entry: gradient {use_g:.4f}, loss {use_l:.4f}; peak "
          f"{float(ref_g.abs().max()):.3e} / {float(ref_l.abs().max()):.3e}")
    assert float(ref_g.abs().max()) >= 100 * 1e-4 and float(ref_l.abs().max()) >= 100 * 1e-4
    assert ok_g and ok_l


# ---- skipping -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spherical", "directional"])
def test_row_without_coverage_has_no_loss_and_zero_gradient_bits(kind):
    c = _case(R.CASES[0])
    cutn, B, P = c["cutn"], c["B"], c["P"]
    ro = [0] * P  # every prompt in region 0: the cuts OUTSIDE and EMPTY see none of it
    weff = R.effective_weights(c["w"], R.coverage(c["masks"], ro, c["power"], c["boxes"]), B)
    dead = [k * B + b for k in (R.OUTSIDE, R.EMPTY) for b in range(B)]
    assert not weff[dead].any() and all(bool(weff[r].any()) for r in range(cutn * B) if r not in dead)
    e = c["e"].clone()
    e[dead[0]] = NAN  # nothing of a skipped row reaches its result, whatever the embedding holds
    if kind == "spherical":
        ref_l, ref_g = R.spherical(c["e"], c["d"], weff, cutn)
    else:
        ref_l, ref_g, _ = R.directional(c["e"], c["s"], c["d"], weff, cutn, B)
    got_g, got_l, tails, _ = run(kind, c, Regions(c, region_of=ro), e=e)
    assert not got_g[dead].view(th.int32).any() and not got_l[dead].view(th.int32).any(), "loss and gradient bits of a skipped row must be zero"
    assert D.within(got_g, ref_g)[0] and D.within(got_l, ref_l)[0] and tails_untouched(tails)
    if kind == "directional":  # accumulate leaves such a row as it is
        pre = th.randn(got_g.shape, generator=g(5))
        acc_g, acc_l, _, _ = run(kind, c, Regions(c, region_of=ro), e=e, accumulate=1, prefill=pre)
        live = [r for r in range(cutn * B) if r not in dead]
        assert th.equal(acc_g[dead], pre[dead]) and th.equal(acc_g[live], pre[live] + got_g[live]) and th.equal(acc_l, got_l)


@pytest.mark.parametrize("kind", ["spherical", "directional"])
def test_skipped_column_is_not_read(kind):
    c = _case(R.CASES[0])  # region_of (0, -1, 1)
    masks = c["masks"].clone()
    masks[1] = 0  # prompt 2 sees nothing on any cut
    rg = Regions(c, masks=masks)
    got_g, got_l, _, _ = run(kind, c, rg)
    t = c["d"].clone()
    t[2] = NAN
    nan_g, nan_l, _, _ = run(kind, c, rg, t=t)
    assert bool(th.isfinite(got_g).all()) and th.equal(nan_g, got_g) and th.equal(nan_l, got_l)
    # ... and equals the launch with that prompt's weight set to zero
    w = c["w"].clone()
    w[:, 2] = 0
    zero_g, zero_l, _, _ = run(kind, c, Regions(c), w=w)
    assert th.equal(zero_g, got_g) and th.equal(zero_l, got_l)


@pytest.mark.parametrize("kind", ["spherical", "directional"])
def test_runs_are_bit_identical(kind):
    c = _case(R.CASES[0])
    a, b = run(kind, c, Regions(c)), run(kind, c, Regions(c), prefill=7.0)
    assert th.equal(a[0], b[0]) and th.equal(a[1], b[1])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_minus_two_and_write_nothing():
    ctx = _ctx()
    c = _case(R.CASES[0])
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    variants = []
    for name in ("sat", "region_of", "region_of_host", "power", "geo"):
        rg = Regions(c)
        rg.null = (name,)
        variants.append((f"null {name}", rg, None, b"null pointer"))
    variants.append(("R = 0", Regions(c, R_=0), None, b"R must be"))
    variants.append(("region_of = R", Regions(c, host_region_of=[0, -1, 2]), None, b"region_of"))
    variants.append(("region_of = -2", Regions(c, host_region_of=[-2, -1, 1]), None, b"region_of"))
    variants.append(("frame over the int32 limit", Regions(c, H=2902, W=2902), None, b"2^31"))  # refused before any read: the small table is enough
    variants.append(("D = 2049", Regions(c), (c["cutn"], c["B"], c["P"], 2049), b"embedding dim"))
    for tag, rg, shape, msg in variants:
        for kind in ("spherical", "directional"):
            e = th.randn(c["cutn"] * c["B"], 2049) if shape else None
            s = th.randn(c["cutn"], 2049) if shape else None
            t = th.randn(c["P"], 2049) if shape else None
            got_g, got_l, tails, rc = run(kind, c, rg, e=e, s=s, t=t, shape=shape, check=False)
            assert rc == -2 and msg in ctx.lib.cgd_last_error(ctx.h), (tag, kind, rc, ctx.lib.cgd_last_error(ctx.h))
            assert bool(th.isnan(got_g).all()) and bool(th.isnan(got_l).all()) and tails_untouched(tails), (tag, kind)
        if shape is None:
            out = th.full((len(c["boxes"]) * c["P"],), NAN, device=DEV)
            rc = ctx.lib.cgd_op_region_coverage(ctx.h, *rg.args()[:5], out.data_ptr(), len(c["boxes"]), c["P"], *rg.args()[5:], ctx.stream())
            th.cuda.synchronize()
            assert rc == -2 and msg in ctx.lib.cgd_last_error(ctx.h) and bool(th.isnan(out).all()), tag
    for kind in ("spherical", "directional"):  # a null pointer among the plain arguments
        assert run(kind, c, Regions(c), check=False)[3] == 0
    rg = Regions(c)
    p = rg.sat.data_ptr()  # never read: the refusal comes first
    rc = ctx.lib.cgd_spherical_loss_regions(ctx.h, None, p, p, p, p, c["cutn"], c["B"], c["P"], c["D"], 1000.0, *rg.args(), ctx.stream())
    assert rc == -2 and b"null pointer" in ctx.lib.cgd_last_error(ctx.h)
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before + 2  # only the two accepted launches above


# ---- one guided step ------------------------------------------------------------------------------------------------------------------------
STEP_I, HW = 12, 64
TAPE = [(0, 0, 64), (5, 9, 40), (20, 3, 44), (29, 30, 34)]  # (ox, oy, size): the whole frame and three inner crops


def _step_plan():
    """two regions and one prompt without: the left half at power 1, a gray mask at power 2, everywhere"""
    from cgd_amd import regions
    gray = th.randint(0, 256, (HW, HW), generator=g(77), dtype=th.int64).to(th.uint8)
    gray[:, 40:] = 0
    sat = regions.build_sat([regions.parse_region("0,0,0.5,1", HW, HW), gray])
    return regions.RegionPlan(sat, [0, 1, -1], [1.0, 2.0, 1.0])


def _guided(leg, cutter=None, tape=None, direction=False):
    """ClipGuidance.native at step STEP_I, batch 1, three prompts (the third a direction prompt if `direction`) -> (g, d loss / d x_in, log, launches)"""
    from cgd_amd import guidance
    from tests import step_checks
    from tests.test_gpu_direction import _step_setup
    st = _step_setup()
    ctx, tables, unet, vit = st["ctx"], st["tables"], st["unet"], st["towers"][0]
    gen = g(741)
    embeds = th.randn(3, vit.out_dim, generator=gen).to(DEV)
    cgs, tvs, rs = step_checks.default_scales(HW, HW)
    sampler = type("D", (), {"tables": tables, "num_timesteps": tables.num_timesteps, "step_coef": lambda self, a, b=None: tables.step_coef(a, b)})()
    kw = {}
    if direction:  # the gray region's prompt is the direction: column 1 of the weight list
        kw = dict(direction_embeds=[embeds[1:2]], direction_weights=th.tensor([0.3]), direction_columns=[1], direction_source=st["source"])
        targets, weights = embeds[[0, 2]], th.tensor([0.5, 0.2])
    else:
        targets, weights = embeds, th.tensor([0.5, 0.3, 0.2])
    cond = guidance.ClipGuidance(ctx, unet, [vit], sampler, [targets], weights, len(TAPE), clip_guidance_scale=cgs, tv_scale=tvs, range_scale=rs,
                                 make_cutouts=cutter, regions=_step_plan(), **kw)
    if leg == "torch":
        cond._clip_leg = cond._clip_leg_torch
    cond.current_timestep = STEP_I
    cond.coords_tape = [tape or TAPE]
    coef = tables.step_coef(STEP_I, STEP_I)
    xd = st["x"][:1].to(DEV)
    ts = th.full((1,), float(tables.model_timestep(STEP_I)), device=DEV)
    out6 = unet.forward(xd, ts, th.full((1,), 7, device=DEV))
    x0, mean, logvar, xin = (th.empty_like(xd) for _ in range(4))
    ctx.check(ctx.lib.cgd_pmv_blend(ctx.h, xd.data_ptr(), out6.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), xin.data_ptr(),
                                    1, HW, HW, coef, ctx.stream()))
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    g_dev = cond.native(xd, x0, xin, coef)
    ctx.lib.cgd_launch_counts(counts)
    th.cuda.synchronize()
    return g_dev.clone(), cond._buf["gclip"].clone(), cond.log(), counts[0] - before


def _compare(tag, native, torch_):
    (g_n, c_n, log_n, _), (g_t, c_t, log_t, _) = native, torch_
    out = []
    for name, a, b in (("g", g_n, g_t), ("g_clip_in", c_n, c_t)):
        sd = pc.unit_seed(b)
        out.append(rec(f"{tag} {name} (unit peak)", a * sd, b * sd))
        out.append(rec(f"{tag} {name}", a, b, allow_small=True))
    for key in [k for k in log_t if "Loss" in k]:
        out.append(rec(f"{tag} {key}", th.tensor([log_n[key]]), th.tensor([log_t[key]]), allow_small=True))
    for r in out:
        print(("OK   " if r["ok"] else "FAIL ") + f"{r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e} "
              f"[{r['criterion']}] strict={r['ok_strict']}")
    assert math.isfinite(log_n["CLIP Loss"]) and log_n["CLIP Loss"] != 0
    bad = [r for r in out if not r["ok"]]
    assert not bad, bad


@pytest.mark.parametrize("case", ["pooled", "resized", "direction in a region"])
def test_guided_step_matches_the_torch_leg(case):
    from cgd_amd import guidance
    kw = {}
    if case == "resized":
        st_ctx = _ctx()
        # (ox, oy, w, h, flags): the overview, its mirror image (same coverage), a gray and a non-square inner cut
        kw = dict(cutter=guidance.MakeCutoutsResized(224, overview=2, inner=2, ctx=st_ctx),
                  tape=[(0, 0, HW, HW, 0), (0, 0, HW, HW, guidance.RESIZE_FLIP), (3, 5, 40, 40, guidance.RESIZE_GRAY), (10, 20, 44, 30, 0)])
    if case == "direction in a region":
        kw = dict(direction=True)
    native, torch_ = _guided("native", **kw), _guided("torch", **kw)
    _compare(f"region step[{case}]", native, torch_)
    if case == "direction in a region":
        assert native[2]["Direction Loss"] != 0


def test_step_with_regions_makes_as_many_launches_as_without():
    """the plan only swaps the loss entries: same launch count, another gradient"""
    from cgd_amd import guidance
    from tests import step_checks
    from tests.test_gpu_direction import _step_setup
    st = _step_setup()
    with_plan = _guided("native")
    ctx, tables, unet, vit = st["ctx"], st["tables"], st["unet"], st["towers"][0]
    embeds = th.randn(3, vit.out_dim, generator=g(741)).to(DEV)
    cgs, tvs, rs = step_checks.default_scales(HW, HW)
    sampler = type("D", (), {"tables": tables, "num_timesteps": tables.num_timesteps})()
    cond = guidance.ClipGuidance(ctx, unet, [vit], sampler, [embeds], th.tensor([0.5, 0.3, 0.2]), len(TAPE), clip_guidance_scale=cgs, tv_scale=tvs,
                                 range_scale=rs)
    cond.current_timestep, cond.coords_tape = STEP_I, [TAPE]
    coef = tables.step_coef(STEP_I, STEP_I)
    xd = st["x"][:1].to(DEV)
    out6 = unet.forward(xd, th.full((1,), float(tables.model_timestep(STEP_I)), device=DEV), th.full((1,), 7, device=DEV))
    x0, mean, logvar, xin = (th.empty_like(xd) for _ in range(4))
    ctx.check(ctx.lib.cgd_pmv_blend(ctx.h, xd.data_ptr(), out6.data_ptr(), x0.data_ptr(), mean.data_ptr(), logvar.data_ptr(), xin.data_ptr(),
                                    1, HW, HW, coef, ctx.stream()))
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    g_plain = cond.native(xd, x0, xin, coef)
    ctx.lib.cgd_launch_counts(counts)
    th.cuda.synchronize()
    assert counts[0] - before == with_plan[3] > 0
    assert not th.equal(g_plain, with_plan[0])


# ---- the drop-in generator ------------------------------------------------------------------------------------------------------------------
def test_dropin_generator_with_region_prompts(tmp_path, monkeypatch):
    import numpy as np
    from PIL import Image
    monkeypatch.setenv("CGD_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.chdir(tmp_path)
    from cgd.cgd import clip_guided_diffusion

    def final_frame(tag, prompts):
        items = list(clip_guided_diffusion(prompts=prompts, image_size=64, batch_size=1, num_cutouts=2, timestep_respacing="ddim4",
                                           prefix_path=str(tmp_path / tag), checkpoints_dir=str(tmp_path / "ckpt"), save_frequency=4,
                                           progress=False, device="cuda", width_offset=64))
        assert items and all(os.path.isfile(p) and "@@" not in p for _, p in items)
        return np.array(Image.open(items[-1][1]))

    regions_a = final_frame("a", ["a@@0,0,0.5,1", "b@@0.5,0,1,1"])
    regions_b = final_frame("b", ["a@@0,0,0.5,1", "b@@0.5,0,1,1"])
    plain = final_frame("c", ["a", "b"])
    assert regions_a.shape == (64, 128, 3) and np.array_equal(regions_a, regions_b), "the run with regions must repeat itself"
    assert not np.array_equal(regions_a, plain), "the regions must change the result"
