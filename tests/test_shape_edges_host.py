"""CPU half of the shape-edge tier (tests/shape_edge_checks.py, tests/test_gpu_shape_edges.py): the table against the launchers' host-side
plans (cgd_op_plan, cgd_op_plan_conv, cgd_op_attn_plan), against the source lines it cites, against its own empty-slice claims, and the
admissibility of every reference by the value-regime tier's rule (fp32 PyTorch within 0.25 of the bound against float64, no reference
peak below MIN_PEAK except the named T = 1 records)."""
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib as L
from tests import shape_edge_checks as se
from tests.parity_checks import MIN_PEAK, ROOT

ADMISSIBLE_FRACTION = 0.25
RUN = [r for r in se.TABLE if r.verdict == "run"]
FORCED = ("gemv", "hgemm2", "kgemm", "hconv2", "kconv", "wconv")


def _plan(M, N, K, weight, precision):
    o = (C.c_int * 4)()
    rc = L.load().cgd_op_plan(0, M, N, K, 0, 0, 0, weight, precision, se.NUM_CU, o)
    return rc, list(o)


def _plan_conv(s, precision):
    cin, cout = (s["Co"], s["Ci"]) if s["dgrad"] else (s["Ci"], s["Co"])
    o = (C.c_int * 5)()
    rc = L.load().cgd_op_plan_conv(s["B"], s["H"], s["W"], cin, cout, precision, se.NUM_CU, s["var"], 0, 0, o)
    return rc, list(o)


def test_table_is_well_formed():
    names = [r.name for r in se.TABLE]
    assert len(set(names)) == len(names), [n for n, c in Counter(names).items() if c > 1]
    for r in se.TABLE:
        assert r.verdict in ("run", "refuse") and (r.route in se.ROUTES or r.route == "attn"), r.name
        assert (r.text is not None) == (r.verdict == "refuse"), r.name
        assert all(c in se.CLAUSES and side in ("lo", "hi") for c, side in r.marks), r.name
        assert all(ck in se.CONTEXTS for ck in r.ctxs), r.name
    per = Counter(r.fam for r in se.TABLE)
    runs = Counter(r.fam for r in se.TABLE for _ in r.ctxs)
    print("rows per family: " + ", ".join(f"{f} {n}" for f, n in sorted(per.items())))
    print("row x context runs per family: " + ", ".join(f"{f} {n}" for f, n in sorted(runs.items())) + f"; {len(se.GROUPS)} groups")


def test_every_cited_line_still_holds_its_clause():
    src = {}
    for key, (fname, line, token, _) in se.CLAUSES.items():
        if fname not in src:
            with open(os.path.join(ROOT, "clip-guided-diffusion_amd", "csrc", fname)) as f:
                src[fname] = f.read().split("\n")
        assert token in src[fname][line - 1], f"{key}: {fname}:{line} reads {src[fname][line - 1].strip()!r}, expected {token!r}"


def test_every_clause_has_a_row_on_each_side():
    sides = {}
    for r in se.TABLE:
        for c, side in r.marks:
            sides.setdefault(c, set()).add(side)
    lacking = {c: sorted(sides.get(c, ())) for c in se.CLAUSES if sides.get(c) != {"lo", "hi"}}
    assert not lacking, lacking


def test_every_forced_refusal_has_its_automatic_counterpart():
    fall = [r for r in se.TABLE if r.fam == "fallthrough"]
    shape = lambda s: tuple(s[k] for k in (("M", "N", "K") if "M" in s else ("B", "H", "W", "Ci", "Co")))  # noqa: E731
    for r in se.TABLE:
        if r.verdict != "refuse" or r.fam not in FORCED:
            continue
        for ck in r.ctxs:
            twins = [f for f in fall if ck in f.ctxs and shape(f.spec) == shape(r.spec) and f.spec["tile"] == 0 and f" of {r.fam}" in f.name]
            assert twins, f"{r.name} [{ck}] has no force_tile = 0 row"
    assert all(f.verdict == "run" for f in fall)  # at these shapes the fallback always computes; none is refused


@pytest.mark.parametrize("row", [r for r in se.TABLE if r.op == "gemm"], ids=lambda r: r.name)
def test_gemm_rows_against_the_planner(row):
    s, fam = row.spec, row.fam
    M, N, K = s["M"], s["N"], s["K"]
    for ck in row.ctxs:
        prec = se.CONTEXTS[ck][0]
        if fam == "igemm":  # (a tile code is taken as given; the planner can only say that the automatic choice for the shape exists)
            assert _plan(M, N, K, 0, prec)[0] == 0
        elif fam == "gemv":
            rc, o = _plan(M, N, K, 0, prec)
            assert rc == 0 and ((o[0], o[1]) == (3, 517)) == (row.verdict == "run"), o
            if row.verdict == "run":  # one 16-column block per workgroup, at most 4 workgroups per CU
                assert o[2] == 1 and o[3] == min(se.ceil_div(N, 16), 4 * se.NUM_CU)
        elif fam == "hgemm2":
            # whether the weight GEMM kernel takes a problem does not depend on its row count (hgemm.hip cgd_hgemm_supported); the policy hands
            # few-row problems to kgemm, so the route is asked at 1024 rows, where the policy picks it by itself (as test_defer_host.py does)
            rc, o = _plan(1024, N, K, 1, prec)
            assert rc == 0 and ((o[0], o[1]) == (2, 513)) == (row.verdict == "run"), o
            if row.verdict == "run":
                # tile height: 64 rows while 128-row tiles leave CUs without a workgroup (hgemm.hip:946-951).  The workgroup count at 1024
                # rows shows it for this N; fewer rows only make the 128-row grid smaller.  The profile cannot (hgemm2 and hgemm_kernel are kind 0)
                assert se.ceil_div(1024, 128) * se.ceil_div(N, 128) < se.NUM_CU and o[3] == o[2] * 16 * se.ceil_div(N, 128), o
                assert M * (K + 8) < 2 ** 29  # hgemm2, not hgemm_kernel (hgemm.hip:1049)
        elif fam == "kgemm":
            rc, o = _plan(M, N, K, 1, prec)
            assert rc == 0 and ((o[0], o[1]) == (4, 518)) == (row.verdict == "run"), o
            if row.verdict == "run":
                assert o[3] == se.ceil_div(M, 32) * (N // 32), o  # 32-row tiles by default
        else:  # the automatic route of a shape its forced route refuses
            rc, o = _plan(M, N, K, 0, prec)
            want = (3, 517) if " of kgemm" in row.name else (0, 64)  # 4 rows: the GEMV; everything else here: the 64 x 64 implicit-GEMM tile
            assert rc == 0 and (o[0], o[1]) == want, (row.name, o)


@pytest.mark.parametrize("row", [r for r in se.TABLE if r.op == "conv"], ids=lambda r: r.name)
def test_conv_rows_against_the_planner(row):
    s = row.spec
    for ck in row.ctxs:
        prec, env = se.CONTEXTS[ck]
        rc, o = _plan_conv(s, prec)
        assert rc == 0, row.name
        if row.fam == "hconv2":  # a halo kernel takes the shape (kconv's test includes hconv2's: kconv.hip cgd_kconv_supported)
            assert (o[0] == 1) == (row.verdict == "run"), o
        elif row.fam == "kconv":
            assert ((o[0], o[1]) == (1, 516)) == (row.verdict == "run"), o
        else:
            assert (o[0], o[1]) == {"igemm": (0, 64), "kconv": (1, 516)}[row.route], (row.name, o)


def test_halo_rows_restate_the_support_predicates():
    """cgd_hconv_supported / cgd_wconv_supported on dense, aligned operands, restated: H % 8, W % 16 (or 8 for hconv2 / kconv), Cin % 32, N % 32,
    H % 16 for the 16-row variants and Winograd mode 2"""
    for r in se.TABLE:
        s = r.spec
        if r.fam in ("hconv2", "kconv"):
            cin, cout = (s["Co"], s["Ci"]) if s["dgrad"] else (s["Ci"], s["Co"])
            ok = s["H"] % 8 == 0 and (s["W"] % 16 == 0 or s["W"] == 8) and cin % 32 == 0 and cout % 32 == 0 and not (s["var"] & 1 and s["H"] % 16)
            ok = ok and not (s["ups"] and (s["H"] | s["W"]) & 1)
        elif r.fam == "wconv":
            ok = s["H"] % 8 == 0 and s["W"] % 16 == 0 and s["Ci"] % 32 == 0 and s["Co"] % 32 == 0 and not (s["mode"] == 2 and s["H"] % 16)
            assert s["mode"] != 2 or "p0" not in r.ctxs  # forced 16-row tiles: bf16x3 only (wconv.hip:669)
        else:
            continue
        assert ok == (r.verdict == "run"), r.name
        if r.fam == "hconv2" and s["var"] == 8 and r.verdict == "run":  # the unsplit tile: whole 128-channel panels, one slice (hconv.hip:528)
            assert (s["Ci"] if s["dgrad"] else s["Co"]) % 128 == 0 and s["sk"] == 1, r.name


@pytest.mark.parametrize("ck", se.ATTN_CTXS)
def test_attention_rows_against_the_planner(ck):
    prec, env = se.CONTEXTS[ck]
    flash = int(env.get("CGD_ATTN_FLASH", "-1"))
    plan_prec = 0 if env.get("CGD_ATTN_X3") == "0" else prec  # the plan reads no environment: exact products select as an exact-fp32 context does
    fams = Counter()
    for r in se.rows_of("attn", ck):
        s = r.spec
        o = (C.c_int * 2)()
        assert L.load().cgd_op_attn_plan(s["T"], s["d"], 3 * s["heads"] * s["d"], s["heads"] * s["d"], plan_prec, flash, o) == 0
        assert o[0] == se.attn_family(s["T"], s["d"], ck), (r.name, ck, list(o))
        fams[o[0]] += 1
    print(f"{ck}: rows per family (0 GEMMs, 1 s64, 2 mid, 3 flash) {dict(fams)}")
    assert fams[0] and fams[1]
    assert (fams[3] > 0) == (prec == 1 and env.get("CGD_ATTN_X3") != "0" and flash != 0)
    assert (fams[2] > 0) == (fams[3] == 0)  # at d = 64, T > 64 is flash wherever a flash kernel is selected at all


def test_split_rows_name_their_empty_slices():
    seen = Counter()
    for r in se.TABLE:
        s = r.spec
        sk = s.get("sk", 1)
        marks = dict((c, side) for c, side in r.marks if c.endswith(".empty_slice"))
        if not marks:
            continue
        if r.fam == "sconv":  # slices per parity class: test_sconv_rows_name_their_empty_slices_per_parity_class
            continue
        (clause, side), = marks.items()
        units = {"igemm": -(-s.get("K", 0) // 32), "hgemm": s.get("K", 0) // 64}.get(clause.split(".")[0], s.get("Ci", 0) // 32)
        per = int(np.ceil(units / max(sk, 1)))
        lo = np.arange(max(sk, 1)) * per
        hi = np.minimum(units, lo + per)
        empty = int((lo >= hi).sum()) if sk > 1 else 0
        assert empty == se.empty_slices(units, sk) and (side == "hi") == (empty > 0), (r.name, units, sk, empty)
        if sk == units + 1:
            assert empty == 1, r.name
            seen[clause] += 1
        if units == 18 and sk == 7:  # what the automatic policy can ask for: ceil(18 / 7) * 6 >= 18
            assert empty == 1 and per * (sk - 1) >= units
            seen[clause + " 18 in 7"] += 1
    assert all(seen[c + ".empty_slice"] for c in ("igemm", "hgemm", "hconv", "kconv")) and seen["hconv.empty_slice 18 in 7"] and seen["kconv.empty_slice 18 in 7"], seen


def test_groupnorm_rows_reach_every_kernel_and_both_chunk_regimes():
    kinds = {se.gn_kernel(r.spec["HW"], r.spec["C"]) for r in se.TABLE if r.fam == "gn" and r.verdict == "run"}
    assert kinds == {"chunked", ("scalar", "cached"), ("v4", "cached"), ("v4", "streaming")}, kinds
    # (the scalar kernel streams above 8 x 1024 / cpg pixels only: beyond the single-launch size for C = 32, 64, 96)
    assert se.gn_chunk(1025, 1) == 8 and 1025 % 8 == 1  # the last chunk is one pixel
    assert se.gn_chunk(524288, 1) == 256 and 524288 // 256 == 2048 and se.gn_chunk(524296, 1) == 257 and 524296 % 257 == 16
    h = L.load()
    for HW in (1025, 524288, 524296):  # the scratch size is the launcher's own view of the chunk count
        nchunk = se.ceil_div(HW, se.gn_chunk(HW, 1))
        assert h.cgd_op_gn_scratch_floats(1, HW, 32) == nchunk * 64 + 64 + 32 * 8 + 32 * 2


def test_no_reference_is_vacuous_and_backward_seeds_have_unit_peak():
    low = []
    for r in RUN:
        for label, ref in se.references(r):
            peak = ref.abs().max().item()
            if se.vacuous_ok(r, label):
                assert peak < MIN_PEAK, (r.name, label, peak)  # identically zero in exact arithmetic
            elif peak < MIN_PEAK:
                low.append((r.name, label, peak))
            if label in ("dq", "dx") and r.op in ("attn", "ln"):
                whole = max(t.abs().max().item() for lb, t in se.references(r) if lb in ("dq", "dk", "dv", "dx"))
                assert abs(whole - 1.0) < 1e-9, (r.name, whole)
    assert not low, low


NON_MFMA = [r for r in RUN if r.op in ("gn", "ln", "act", "pool2x2", "upsample2x", "bilinear_up2x") or r.fam == "gemv"]


def test_fp32_references_of_the_non_mfma_rows_stay_within_a_quarter_of_the_bound():
    """the float64 references evaluated in fp32 PyTorch on the same inputs: a reference that fp32 itself cannot reproduce within 0.25 of
    1e-4 + 1e-3 |ref| would make the bound a statement about the reference, not about the kernel"""
    worst = {}
    for r in NON_MFMA:
        for (label, r64), (_, r32) in zip(se.references(r), se.references(r, th.float32)):
            f = se.bound_fraction(r32, r64)
            if f >= worst.get(r.fam, (0.0, ""))[0]:
                worst[r.fam] = (f, f"{r.name} {label}")
            assert f <= ADMISSIBLE_FRACTION, f"{r.name} {label}: fp32 PyTorch at {f:.3f} of the bound"
    print("worst fp32 fraction of the bound per family: " + ", ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in sorted(worst.items())))


# ---- the stride-2 conv (csrc/sconv.hip): the plan entry against the clauses restated in numpy ----------------------------------------------------
SCONV = [r for r in se.TABLE if r.fam == "sconv"]
WS_BYTES = 256 << 20


def _sconv_plan_np(dgrad, B, H, W, Ci, Co, ncu):
    """sconv.hip sconv_select in numpy integers, clause by clause (lines 291-310): (bm, bn, slices, workgroups of the main launch)"""
    M = np.int64(B) * (H // 2) * (W // 2)
    N, Kc = np.int64(Ci if dgrad else Co), np.int64(Co if dgrad else Ci)
    cls = np.int64(4 if dgrad else 1)
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    big = cdiv(M, 128) * cdiv(N, 64) * cls
    bm, bn = (64, 32) if big < ncu else (128, 64)
    tiles = cdiv(M, bm) * cdiv(N, bn)
    grid = cdiv(tiles, 8) * 32 if dgrad else tiles
    out_rows, work, short = cls * M if dgrad else M, tiles * cls, (1 if dgrad else 9) * (Kc // 32)
    sk = 1
    if work < ncu:
        want = min(cdiv(2 * ncu, work), short // 2, 16)
        while want > 1 and want * out_rows * N * 4 > WS_BYTES:
            want -= 1
        if want >= 2:
            sk = want
    return int(bm), int(bn), int(sk), int(grid * sk)


def _plan_s2(s, ncu):
    o = (C.c_int * 4)()
    rc = L.load().cgd_op_plan_conv_s2(s["dgrad"], s["B"], s["H"], s["W"], s["Ci"], s["Co"], ncu, o)
    return rc, tuple(o)


@pytest.mark.parametrize("ncu", [256, 304, 64])
def test_sconv_rows_against_the_plan_entry(ncu):
    """every row's plan {bm, bn, slices, workgroups} = the numpy restatement, at the table's 256 CUs = what the table claims (tile, slices, the
    closed form of the grid), and refused where the table says so (dense strides: the stride rows are asked through _accepts)"""
    h = L.load()
    seen, bwd_tiles = Counter(), Counter()
    for r in SCONV:
        s = r.spec
        dense = s["ld"] == (0, 0, 0)
        rc, o = _plan_s2(s, ncu)
        if r.verdict == "refuse":
            cin, cout = (s["Co"], s["Ci"]) if s["dgrad"] else (s["Ci"], s["Co"])
            ld = [c + 8 + d for c, d in zip((cin, cout), s["ld"][:2])] + [s["Ci"] + 4 + s["ld"][2] if s["dgrad"] else 0]
            assert h.cgd_op_conv3x3_s2_accepts(s["dgrad"], ld[0], ld[1], ld[2], s["B"], s["H"], s["W"], s["Ci"], s["Co"]) == 0, r.name
            assert rc == (-2 if dense else 0), (r.name, rc)  # (the plan entry asks for the dense problem)
            continue
        assert h.cgd_op_conv3x3_s2_accepts(s["dgrad"], (s["Co"] if s["dgrad"] else s["Ci"]) + 8, (s["Ci"] if s["dgrad"] else s["Co"]) + 8,
                                           s["Ci"] + 4 if s["dgrad"] else 0, s["B"], s["H"], s["W"], s["Ci"], s["Co"]) == 1, r.name
        assert rc == 0 and o == _sconv_plan_np(s["dgrad"], s["B"], s["H"], s["W"], s["Ci"], s["Co"], ncu), (r.name, o)
        if ncu == se.NUM_CU:
            p = se.sconv_plan(s["dgrad"], s["B"], s["H"], s["W"], s["Ci"], s["Co"])
            assert o == (p["bm"], p["bn"], p["sk"], p["wg"]), (r.name, o, p)
            tiles = se.ceil_div(p["M"], o[0]) * se.ceil_div(p["N"], o[1])
            assert o[3] == (se.ceil_div(tiles, 8) * 32 if s["dgrad"] else tiles) * o[2]  # the closed form of the grid
            seen[(s["dgrad"], o[0], o[2])] += 1
            if s["dgrad"]:
                bwd_tiles[tiles] += 1
    if ncu == se.NUM_CU:
        print("rows per (backward, tile rows, slices): " + ", ".join(f"{k} {v}" for k, v in sorted(seen.items(), key=str)))
        for dgrad in (0, 1):
            assert seen[(dgrad, 128, 1)] >= 2 and {sk for (d, bm, sk) in seen if d == dgrad and bm == 64} >= {1, 2 + (1 - dgrad), 4, 16}, seen
        assert all(bwd_tiles[t] for t in (1, 7, 8, 9)), bwd_tiles
        assert h.cgd_op_plan_conv_s2(0, 1, 4, 4, 32, 32, 256, None) == -3


def test_sconv_boundary_shapes_sit_on_their_clauses():
    """big = num_cu exactly takes the 128 x 64 tile (`<`, not `<=`), one row of tiles fewer the 64 x 32 one; work = num_cu exactly is unsplit"""
    plan = lambda *a: _plan_s2(dict(zip(("dgrad", "B", "H", "W", "Ci", "Co"), a)), 256)[1]  # noqa: E731
    assert plan(0, 1, 256, 256, 128, 128) == (128, 64, 1, 256) and plan(0, 1, 254, 256, 128, 128) == (64, 32, 1, 1016)
    assert plan(1, 1, 128, 128, 128, 128) == (128, 64, 1, 256) and plan(1, 1, 124, 128, 128, 128) == (64, 32, 1, 992)
    assert plan(0, 1, 128, 128, 32, 128) == (64, 32, 1, 256) and plan(0, 1, 126, 128, 32, 128) == (64, 32, 3, 756)
    assert plan(1, 1, 64, 64, 128, 128) == (64, 32, 1, 256) and plan(1, 1, 60, 64, 128, 128) == (64, 32, 2, 512)
    # the five Downsamples of the community checkpoints at a 256 x 256 frame, forward / backward
    want = {(256, 128): ((128, 64, 1), (128, 64, 1)), (128, 128): ((64, 32, 1), (128, 64, 1)), (64, 256): ((64, 32, 4), (64, 32, 1)),
            (32, 256): ((64, 32, 16), (64, 32, 4)), (16, 512): ((64, 32, 16), (64, 32, 8))}
    for (hw, c), (f, b) in want.items():
        assert plan(0, 1, hw, hw, c, c)[:3] == f and plan(1, 1, hw, hw, c, c)[:3] == b, (hw, c, plan(0, 1, hw, hw, c, c), plan(1, 1, hw, hw, c, c))


def test_sconv_rows_name_their_empty_slices_per_parity_class():
    seen = Counter()
    for r in SCONV:
        if r.verdict != "run":
            continue
        s = r.spec
        p = se.sconv_plan(s["dgrad"], s["B"], s["H"], s["W"], s["Ci"], s["Co"])
        empties = []
        for taps in ((1, 2, 2, 4) if s["dgrad"] else (9,)):
            nkt = taps * (p["Kc"] // 32)
            per = int(np.ceil(nkt / p["sk"]))
            lo = np.arange(p["sk"]) * per
            empties.append(int((lo >= np.minimum(nkt, lo + per)).sum()))
        assert empties == se.sconv_empty(s["dgrad"], p["Kc"], p["sk"]), r.name
        assert (dict(r.marks)["sconv.empty_slice"] == "hi") == (sum(empties) > 0), (r.name, empties)
        if sum(empties):
            seen[(s["dgrad"], p["sk"], tuple(empties))] += 1
    print("rows with empty slices (backward, slices, empty per class): " + ", ".join(f"{k} x{v}" for k, v in sorted(seen.items())))
    assert seen[(1, 4, (1, 0, 0, 0))], seen  # Kc = 288 backward: 9 K tiles of the one-tap class in 4 slices of 3
    assert any(k[0] == 0 for k in seen)


def test_sconv_workspace_cap_is_unreachable():
    """the `ws_bytes` clause of the want loop (sconv.hip:308): split-K is considered below num_cu workgroups only, so the slices hold at most
    16 x (tiles x 64 x 32) floats; enumerated for every tile grid below 304 CUs"""
    worst = 0
    for ncu in (256, 304):
        for dgrad in (0, 1):
            cls = 4 if dgrad else 1
            for ntm in range(1, ncu):
                for ntn in range(1, ncu // ntm + 1):
                    if ntm * ntn * cls < ncu:
                        worst = max(worst, 16 * cls * (ntm * 64) * (ntn * 32) * 4)
    print(f"largest split-K workspace the stride-2 conv can ask for: {worst} bytes of {WS_BYTES}: the cap is " + ("REACHABLE" if worst > WS_BYTES else "unreachable"))
    assert worst <= WS_BYTES


def test_sconv_references_are_admissible():
    worst = (0.0, "")
    for r in SCONV:
        if r.verdict != "run":
            continue
        s = r.spec
        (label, r64), = se.references(r)
        (_, r32), = se.references(r, th.float32)
        assert r64.abs().max().item() >= MIN_PEAK, r.name
        if s["dgrad"]:
            add = se.sconv_data(1, s["B"], s["H"], s["W"], s["Ci"], s["Co"])[2]
            assert abs((r64 - add.double()).abs().max().item() - 1.0) < 1e-9, r.name
        f = se.bound_fraction(r32, r64)
        worst = max(worst, (f, f"{r.name} {label}"))
        assert f <= ADMISSIBLE_FRACTION, f"{r.name} {label}: fp32 PyTorch at {f:.3f} of the bound"
    print(f"worst fp32 fraction of the bound over the stride-2 conv rows: {worst[0]:.3f} ({worst[1]})")
