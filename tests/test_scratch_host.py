"""Host side of the scratch tier (tests/scratch_checks.py): every size query against its closed form at every row of the table, the
attention per-family sizes against cgd_op_attn_plan and the upper bound, the bounds of the multi-run cutout row, the detector, and the
Python callers (guidance.py's cutters, sampler.py's ILVR and thresholding set-ups) on a recording fake with the REAL size queries: every
scratch tensor handed to a call holds at least what the query returns for that call's own arguments.  No GPU."""
import ctypes as C
import os
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import diffusion as dd
from cgd_amd import guidance as dg
from cgd_amd import lib as L
from tests import scratch_checks as sc
from tests import shape_edge_checks as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "clip-guided-diffusion_amd", "csrc")
BUFS = ("qkvT", "P", "Pt", "dP", "dAt")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_every_size_query_matches_its_closed_form_at_every_row(lib):
    seen = {}
    for row in sc.TABLE:
        if row.op == "attn":
            continue
        got, want = sc.queried(lib, row), sc.closed_form(row)
        assert got and set(got) <= set(want) or row.op in ("ln", "spherical", "directional", "records"), row.name  # (sizes the header states: no query)
        for k, v in got.items():
            assert v == want[k] and v > 0, (row.name, k, v, want[k])
        seen.setdefault(row.fam, []).append((row.name, want))
    for fam, rows in sorted(seen.items()):
        print(fam, "; ".join(f"{n}: {w}" for n, w in rows))
    assert set(seen) == {"gn", "ln", "attnpool", "cutaug", "cutresize", "ilvr", "quantile", "partials"}
    assert lib.cgd_abs_quantile_slice() == sc.QUANTILE_SLICE
    # the restated offsets inside the GroupNorm scratch are the library's
    for (B, HW, Cc) in ((1, 64, 64), (2, 1050, 64), (1, 256, 64), (1, 524288, 32)):
        assert lib.cgd_op_gn_stats_offset(B, HW, Cc) == sc.gn_sizes(B, HW, Cc)["stats"]
        assert sc.gn_sizes(B, HW, Cc)["ab"] + 2 * B * Cc == sc.gn_sizes(B, HW, Cc)["total"]
    # the with_pred_xstart switch, and a refused factor
    assert lib.cgd_ilvr_scratch_floats(2, 24, 40, 4, 1) == 2 * lib.cgd_ilvr_scratch_floats(2, 24, 40, 4, 0) == 2 * 2 * 3 * 6 * 10
    assert lib.cgd_ilvr_scratch_floats(2, 24, 40, 16, 1) == 0 == sc.ilvr_size(2, 24, 40, 16, 1)


def test_attention_per_family_sizes_follow_the_plan_and_stay_below_the_upper_bound(lib):
    fams = {}
    for row in sc.TABLE:
        if row.op != "attn":
            continue
        s = row.spec
        nb, heads, T, d = s["nb"], s["heads"], s["T"], s["d"]
        upper = [int(lib.cgd_op_attn_buf_floats(nb, heads, T, d, i)) for i in range(5)]
        assert upper == sc.attn_upper(nb, heads, T, d)
        for ck in row.ctxs:
            prec, env = sc.CONTEXTS[ck]
            fam = sc.attn_family_of(T, d, prec, env)
            plan = (C.c_int * 2)()
            # (the plan does not read CGD_ATTN_X3: with the bf16x3 products off the choice is that of an exact-fp32 context)
            assert lib.cgd_op_attn_plan(T, d, 3 * heads * d, heads * d, prec if env.get("CGD_ATTN_X3", "1") != "0" else 0,
                                        int(env.get("CGD_ATTN_FLASH", "-1")), plan) == 0
            assert plan[0] == fam, (row.name, ck, plan[0], fam)
            if ck in se.CONTEXTS:
                assert fam == se.attn_family(T, d, ck)
            sizes = sc.closed_form(row, ck)
            assert all(0 <= sizes[n] <= u for n, u in zip(BUFS, upper)), (row.name, ck, sizes, upper)
            assert sizes["P"] > 0 and (fam == 1) == (sizes["qkvT"] == 0)
            fams.setdefault(ck, set()).add(fam)
            if fam == 3:  # the statistics rows are padded to whole 32-query blocks: Tq >= T
                assert sizes["P"] == 2 * nb * heads * 32 * -(-T // 32) >= 2 * nb * heads * T and sizes["qkvT"] == nb * T * heads * d
                if ck == "p1_flash3":
                    assert T <= 64 and plan[1] == 1 and sizes["P"] == 2 * nb * heads * 64  # the one-workgroup backward, Tq = 64
    print({ck: sorted(v) for ck, v in fams.items()})
    assert fams["p1"] == {0, 1, 3} and fams["p0"] == fams["p1_x3off"] == fams["p1_flash0"] == {0, 1, 2}
    assert fams["p1_flash1"] == {0, 1, 3} and fams["p1_flash2"] == {0, 1, 3} and fams["p1_flash3"] == {3}
    # the entry that reports the per-context sizes needs its context
    assert lib.cgd_op_attn_buf_floats_ctx(None, 1, 1, 33, 64, 0, 0, 1) == -1


def test_the_table_reaches_every_rounding_point():
    attn = [r.spec for r in sc.TABLE if r.op == "attn"]
    assert any(s["T"] % 4 for s in attn) and any(s["T"] % 4 == 0 for s in attn)  # Tp = (T + 3) & ~3
    assert {s["T"] % 32 for s in attn if s["d"] == 64} >= {0, 1, 31}  # Tq = 32 ceil(T / 32)
    assert {(s["nb"], s["heads"]) for s in attn if s["d"] == 64} >= {(1, 1), (2, 3)} and {s["legacy"] for s in attn} == {0, 1}
    gn = {(r.spec["B"], r.spec["HW"], r.spec["C"]) for r in sc.TABLE if r.op == "gn"}
    kinds = {se.gn_kernel(HW, Cc) if se.gn_kernel(HW, Cc) == "chunked" else "-".join(se.gn_kernel(HW, Cc)) for _, HW, Cc in gn}
    assert kinds == {"scalar-cached", "v4-cached", "v4-streaming", "chunked"}, kinds
    assert (2, 1050, 64) in gn and se.gn_chunk(1050, 2) == 8 and 1050 % 8 == 2  # a ragged last chunk
    assert (1, 524288, 32) in gn and sc.gn_nchunk(1, 524288) == 2048 and se.gn_chunk(524288, 1) == 256  # the ceiling
    assert {sc.ceil_div(r.spec["n"], sc.QUANTILE_SLICE) for r in sc.TABLE if r.op == "quantile"} == {1, 2, 3}
    assert {sc.ceil_div(3 * r.spec["W"], sc.QUANTILE_SLICE) for r in sc.TABLE if r.op == "threshold"} == {1, 2, 3}
    assert {(r.spec["N"], r.spec["x0"]) for r in sc.TABLE if r.op == "ilvr"} == {(N, x) for N in (2, 4, 64) for x in (0, 1)}
    assert {sc.part_blocks(r.spec["B"], r.spec["H"], r.spec["W"]) for r in sc.TABLE if r.op == "tail"} == {1, 23, 1024}
    assert {sc.HEADS[r.spec["head"]]["out"] % 4 for r in sc.TABLE if r.op == "attnpool"} >= {0, 1, 3}
    names = [r.name for r in sc.TABLE]
    assert len(names) == len(set(names))


def test_the_multi_run_cutout_row_passes_both_bounds_checks_and_takes_two_runs(lib):
    k = sc.BIG_CUT
    B, H, W, cutn, cs = k["B"], k["H"], k["W"], k["cutn"], k["cs"]
    per = sc.rows_per_launch(B, cutn)
    assert cutn * B > 65535 and per == 21845 and sc.ceil_div(cutn, per) == 2 and cutn - per == 1
    assert sc.cutout_bounds_ok("aug", B, H, W, cutn, cs) and sc.cutout_bounds_ok("resize", B, H, W, cutn, cs)
    assert not sc.cutout_bounds_ok("aug", B, 128, 128, cutn, cs) and not sc.cutout_bounds_ok("resize", 65536, H, W, cutn, cs)
    assert lib.cgd_cutouts_aug_scratch_floats(B, H, W, cutn) == 2 * 21845 * 3 * 3 * 16 == 2 * lib.cgd_cutouts_resize_scratch_floats(B, H, W, cutn)
    # the restated bounds are the launchers' (file, a token of the clause)
    for name, tokens in (("cutaug.hip", ("(long)cutn * B * 3 * H * W > lim", "(long)cs * cs * 3 * B * std::max(cutn, 1) > lim", "65535 / B")),
                         ("cutresize.hip", ("8L * cs * std::max(std::max(H, W), cs) > lim", "(long)cs * cs * 3 * B * std::max(cutn, 1) > lim", "65535 / B"))):
        src = open(os.path.join(CSRC, name)).read()
        assert all(t in src for t in tokens), name
    boxes = sc.big_cut_boxes(cutn, H, W, cs)
    assert all(0 <= ox and ox + sz <= W and 0 <= oy and oy + sz <= H and cs <= sz for ox, oy, sz in boxes)
    assert {sz for _, _, sz in boxes} == {2, 3, 4} and boxes[per] != boxes[per - 1]  # the second run's only cutout differs from its neighbour


def test_the_tier_detects_what_it_is_for_on_the_cpu():
    caught = sc.detector("cpu")
    assert not sc.detector_problems(caught), caught
    assert caught["overrun"] == ["guards"], "one float in a guard damages nothing else"


def test_scratch_views_are_exact_aligned_and_guarded_on_both_sides():
    for n in (1, 2, 10, 4095, 4096, 4097, 12345):
        s = sc.Scratch(n, device="cpu")
        assert s.view.numel() == n and s.ptr % 16 == 0
        lo = s.view.storage_offset()
        assert lo >= sc.MIN_GUARD and s.G.buf.numel() - lo - n >= max(n, sc.MIN_GUARD) and lo >= n
    z = sc.Scratch(0, device="cpu")
    assert z.G.buf.numel() == 2 * sc.MIN_GUARD + 1 and z.view.storage_offset() == sc.MIN_GUARD
    z.poison(1)
    assert z.intact(1)
    z.G.buf[sc.MIN_GUARD] = 0.0  # a write THROUGH the pointer of a zero-size buffer
    assert not z.intact(1)


# ---- the Python callers on a recording fake with the real size queries ------------------------------------------------------------------------
QUERIES = ("cgd_cutouts_aug_scratch_floats", "cgd_cutouts_resize_scratch_floats", "cgd_ilvr_scratch_floats", "cgd_abs_quantile_scratch_bytes",
           "cgd_guidance_part_blocks")


class Recorder:
    """every entry is recorded and returns 0, except the host-only size queries, which are the library's own"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name in QUERIES:
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def allocations(monkeypatch):
    """bytes of every tensor torch.empty / empty_like hands out while the test runs, by data pointer (the tensors are kept alive: no pointer is reused)"""
    sizes, live = {}, []

    def tracked(real):
        def alloc(*a, **k):
            t = real(*a, **k)
            live.append(t)
            if t.numel():
                sizes[t.data_ptr()] = t.numel() * t.element_size()
            return t
        return alloc

    for name in ("empty", "empty_like"):
        monkeypatch.setattr(th, name, tracked(getattr(th, name)))
    return sizes


def _fake_ctx(lib):
    rec = Recorder(lib)
    return types.SimpleNamespace(lib=rec, h=1, check=lambda rc: None, device=0, stream=lambda: 0), rec


def test_augmented_cutter_sizes_its_scratch_for_the_largest_group(lib, allocations, monkeypatch):
    """guidance.py _AugLaunch.backward: ONE scratch for every launch group, sized for the group with the most cutouts"""
    B, H, W, cs = 2, 16, 24, 8
    monkeypatch.setattr(dg, "AUG_NOISE_STD", 0.01)
    monkeypatch.setattr(dg, "AUG_GROUP_FLOATS", 22000)  # two 16 x 16 cutouts or three 8 x 8 ones per group (their noise counts)
    th.manual_seed(3)
    coords = [(0, 0, 16), (0, 0, 16), (1, 2, 8), (3, 1, 8), (5, 3, 8), (0, 0, 16)]
    ctx, rec = _fake_ctx(lib)
    aug = dg._AugLaunch(rec, coords, B, H, W, th.device("cpu"))
    counts = [k1 - k0 for k0, k1 in aug.groups]
    assert counts == [2, 3, 1], counts  # uneven groups, the first not the largest
    g_ = th.zeros(B, 3, H, W)
    aug.backward(ctx, th.zeros(len(coords) * B, 3, cs, cs), g_, cs, 0, 0, accumulate=False)
    calls = [a for n, a in rec.calls if n == "cgd_cutouts_aug_bwd"]
    assert [a[9] for a in calls] == counts
    assert len({a[5] for a in calls}) == 1  # one scratch
    for a in calls:  # (ctx, dout, geo, params, g, scratch, B, H, W, n, cs, layout, patch, accumulate, stream)
        need = 4 * lib.cgd_cutouts_aug_scratch_floats(a[6], a[7], a[8], a[9])
        assert allocations[a[5]] >= need > 0, (a[9], allocations[a[5]], need)
    assert allocations[calls[0][5]] == 4 * lib.cgd_cutouts_aug_scratch_floats(B, H, W, max(counts))
    assert [a[13] for a in calls] == [0] + [1] * (len(calls) - 1)  # the groups after the first accumulate


def test_resized_cutter_sizes_its_scratch_for_the_call(lib, allocations):
    """guidance.py _CutLaunch (resized): its own allocation at the first backward, and ClipGuidance.native's per-step buffer (one query per
    step with that step's cut count)"""
    B, H, W, cs = 2, 40, 56, 16
    for recs in (sc.RESIZE_RECS, sc.RESIZE_RECS[:2]):
        n = len(recs)
        geo = th.tensor(dg.resize_table(recs, H, W), dtype=th.int32)
        need = 4 * lib.cgd_cutouts_resize_scratch_floats(B, H, W, n)
        for scratch in (None, th.empty(max(1, lib.cgd_cutouts_resize_scratch_floats(B, H, W, n)))):  # guidance.py:304 and :855
            ctx, rec = _fake_ctx(lib)
            cut = dg._CutLaunch(rec, recs, geo, True, scratch)
            g_ = th.zeros(B, 3, H, W)
            cut.backward(ctx, th.zeros(n * B, 3, cs, cs), g_, cs, 0, 0, False)
            cut.backward(ctx, th.zeros(n * B, 3, cs, cs), g_, cs, 0, 0, True)
            calls = [a for nm, a in rec.calls if nm == "cgd_cutouts_resize_bwd"]
            assert len(calls) == 2 and calls[0][5] == calls[1][5] and calls[0][6:10] == (B, H, W, n)
            assert allocations[calls[0][5]] >= need > 0
    # the plain cutter has no scratch argument at all
    ctx, rec = _fake_ctx(lib)
    plain = dg._CutLaunch(rec, [(0, 0, 16)], th.tensor(dg.crop_geometry([(0, 0, 16)], H, W), dtype=th.int32))
    plain.backward(ctx, th.zeros(B, 3, cs, cs), th.zeros(B, 3, H, W), cs, 0, 0, False)
    # (ctx, dout, geo, g, B, H, W, n, cs, layout, patch, accumulate, stream)
    assert [nm for nm, _ in rec.calls] == ["cgd_cutouts_bwd"] and len(rec.calls[0][1]) == 13


def _sampler(lib, spec):
    from cgd_amd import sampler
    ctx, rec = _fake_ctx(lib)
    smp = sampler.GuidedSampler(ctx, dd.create_gaussian_diffusion(1000, "linear", spec, False))
    model = types.SimpleNamespace(forward=lambda x, ts, y, out=None: out)
    return smp, rec, model


@pytest.mark.parametrize("factor", [2, 4])
def test_sampler_sizes_the_ilvr_scratch_for_every_refinement(lib, allocations, factor):
    """sampler.py _Ilvr: one scratch per loop, sized with pred_xstart; the PLMS predictor's refinement (no pred_xstart) needs half"""
    shape = (2, 3, 8, 12)
    for loop in ("ddim_sample_loop_progressive", "plms_sample_loop_progressive", "dpmpp_sample_loop_progressive"):
        smp, rec, model = _sampler(lib, "ddim10")
        assert len(list(getattr(smp, loop)(model, shape, ilvr=(th.zeros(1, 3, 8, 12), factor, 0), clip_denoised=False, device="cpu"))) == 10
        calls = [a for n, a in rec.calls if n == "cgd_ilvr_refine"]
        assert len(calls) >= 10
        for a in calls:  # (ctx, sample, pred_xstart, ref, noise, scratch, B, H, W, ref_batch, factor, sa, sb, stream)
            need = 4 * lib.cgd_ilvr_scratch_floats(a[6], a[7], a[8], a[10], int(a[2] is not None))
            assert allocations[a[5]] >= need > 0, (loop, allocations[a[5]], need)
        assert {int(a[2] is not None) for a in calls} == ({0, 1} if loop.startswith("plms") else {1})


@pytest.mark.parametrize("threshold", [0.995, (0.9, 2.0)])
def test_sampler_sizes_the_selection_scratch_and_result_for_every_step(lib, allocations, threshold):
    """sampler.py _Dpmpp: the selection's scratch, the (B, 3) result and the x0c buffer are allocated once and hold what each call needs"""
    shape = B, _, H, W = (2, 3, 8, 12)
    smp, rec, model = _sampler(lib, "dpm10")
    assert len(list(smp.dpmpp_sample_loop_progressive(model, shape, clip_denoised=False, device="cpu", order=2, threshold=threshold))) == 10
    calls = [a for n, a in rec.calls if n == "cgd_dpmpp_threshold"]
    assert len(calls) == 10
    for a in calls:  # (ctx, x, x0, g, scalars, x0c, B, H, W, coef, k, frac, floor, cap, thr3, scratch, stream)
        assert a[6:9] == (B, H, W) and a[13] > a[12]
        assert allocations[a[15]] >= lib.cgd_abs_quantile_scratch_bytes(a[6], 3 * a[7] * a[8]) > 0
        assert allocations[a[14]] >= 4 * 3 * a[6] and allocations[a[5]] >= 4 * 3 * a[6] * a[7] * a[8]
    assert len({a[15] for a in calls}) == 1 and len({a[14] for a in calls}) == 1
