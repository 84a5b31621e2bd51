"""CPU half of the deferred split-K tests (tests/defer_checks.py, tests/test_gpu_defer.py): the case table against the launcher's host-side
plan, the float64 reference compositions against themselves in fp32, the admissibility ladder of the mean-through-R regime, and the two
test-support bindings against a recording fake."""
import ctypes as C
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib as L
from cgd_amd import ops
from tests import defer_checks as dc
from tests.test_ops_wrappers import _RecordingLib

CASES = dc.all_cases()
PRODUCERS = sorted({(c.prod, c.precision) for c in CASES} | {(p, 1) for p, _, _ in dc.REGIME_PRODS.values()} | {(dc.KCONV8, 1), (dc.KCONV16, 1)})


def _plan(handle, p, precision):
    if p[0] == "conv":
        _, _, Bn, H, W, Ci, Co = p
        out = (C.c_int * 5)()
        rc = handle.cgd_op_plan_conv(Bn, H, W, Ci, Co, precision, 256, 0, 0, 0, out)
    else:
        _, tile, M, N, K = p
        out = (C.c_int * 4)()
        # whether the weight GEMM kernel takes a problem does not depend on its row count (hgemm.hip cgd_hgemm_supported); the POLICY hands few-row
        # problems to other kernels, so the forced route is asked at 1024 rows, where the policy picks it by itself
        rc = handle.cgd_op_plan(0, 1024 if tile == 513 else M, N, K, 0, 0, 0, 1 if tile == 513 else 0, precision, 256, out)
    return rc, tuple(out)


@pytest.mark.parametrize("p,precision", PRODUCERS, ids=[f"{'x'.join(map(str, p))} p{pr}" for p, pr in PRODUCERS])
def test_every_forced_route_accepts_its_shape(p, precision):
    handle = L.load()
    rc, out = _plan(handle, p, precision)
    assert rc == 0, (p, rc)
    kernel, tile = out[0], out[1]
    if p[1] == 64 and p[0] == "conv":
        assert kernel != 1, f"{p}: the map has a halo route ({out}); the case is meant for the implicit GEMM"
    elif p[1] == 516:
        assert (kernel, tile) == (1, 516), out
    elif p[1] == 512:
        assert kernel == 1 and precision == 1, out  # a halo kernel takes the shape (kconv's test includes hconv2's: kconv.hip cgd_kconv_supported)
    elif p[1] == 513:
        assert (kernel, tile) == (2, 513) and precision == 1, out
    if precision == 0:
        assert p[1] == 64, "exact-fp32 contexts run the implicit GEMM producers only"


def test_no_case_has_an_empty_slice_or_an_implicit_slice_count():
    for c in CASES:
        p = c.prod
        k_units = (9 * p[5] // 32 if p[1] == 64 else p[5] // 32) if p[0] == "conv" else (p[4] // 32 if p[1] == 64 else p[4] // 64)
        per = -(-k_units // c.sk)
        assert c.sk >= 2 and per * (c.sk - 1) < k_units, f"{c.name}: {k_units} K units in {c.sk} slices leaves one empty"
    assert {c.sk for c in CASES if c.prod == dc.IGEMM_CONV} >= {2, 3, 9}
    assert {c.sk for c in CASES if c.prod in (dc.HCONV16, dc.HCONV32)} == {2, 3}
    assert {c.sk for c in CASES if c.prod in (dc.KCONV8, dc.KCONV16)} == {2, 4}
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


def test_case_table_selects_each_groupnorm_family():
    """norm.hip launch_gn_small_fwd / _bwd: float4 needs 4 | C / 32; cached needs HW <= 8 (forward) / 4 (backward) x 1024 >> lg rows"""
    fam = set()
    for c in CASES:
        if c.cons[0] not in ("gn_fwd", "gn_bwd") or c.expect != "take":
            continue
        M, N = dc.prod_shape(c.prod)
        HW, cpg = M // c.cons[1], N // 32
        f = dc.gn_family(c.cons[0], HW, N, bool(c.r_ld_extra))
        fam.add((c.cons[0], f))
        if f == "chunked":
            assert HW % 8, "the chunk (8 pixels at this size) must not divide the map"
        if c.cons[0] == "gn_bwd":
            assert dc.gn_bwd_keeps_dz_in_registers(HW, N, bool(c.r_ld_extra)) == (f == "cached" or (f == "scalar" and HW <= 4 * (1024 >> 2)))
    assert fam == {(k, f) for k in ("gn_fwd", "gn_bwd") for f in ("cached", "streaming", "scalar", "chunked")}, fam


def _unique_refs():
    seen, outc = set(), []
    for c in CASES:
        key = (c.prod, c.mode, c.cons)
        if key not in seen:
            seen.add(key)
            outc.append(c)
    return outc


def test_fp32_references_stay_within_a_quarter_of_the_bound():
    """the float64 compositions the GPU cases are graded against, evaluated in fp32 on the same stored tensor: a reference that fp32 itself
    cannot reproduce within 0.25 of 1e-4 + 1e-3 |ref| would make the bound a statement about the reference, not about the kernel"""
    worst = 0.0
    for c in _unique_refs():
        cpu, ref, r, full, scale, xin, par = dc.case_refs(c)
        M, N = dc.prod_shape(c.prod)
        x = (full * scale).float()  # the tensor as stored
        kind = c.cons[0]
        pairs = []
        for dt in (th.float64, th.float32):
            if kind == "gn_fwd":
                _, B, film, act, _ = c.cons
                y, s, _ = dc.gn_ref(x.reshape(B, M // B, N), par[0], par[1], par[2], act, dtype=dt)
                pairs.append((y, s))
            elif kind == "gn_bwd":
                _, B, act, _ = c.cons
                _, _, dx = dc.gn_ref(xin.reshape(B, M // B, N), par[0], par[1], None, act, x.reshape(B, M // B, N), dtype=dt)
                pairs.append((dx,))
            elif kind == "ln_fwd":
                y, s, _ = dc.ln_ref(x, par[0], par[1], dtype=dt)
                pairs.append((y, s))
            else:
                _, _, dx = dc.ln_ref(xin, par[0], par[1], x, dtype=dt)
                pairs.append((dx,))
        for a64, a32 in zip(*pairs):
            f = dc.bound_fraction(a32, a64)
            worst = max(worst, f)
            assert f <= dc.ADMISSIBLE_FRACTION, f"{c.name}: fp32 reference at {f:.3f} of the bound"
        if kind in ("gn_bwd", "ln_bwd"):
            assert 0.5 <= pairs[0][0].abs().max() <= 2.5, f"{c.name}: the backward seed does not bring dx to unit peak"
    print(f"worst fp32 reference: {worst:.3f} of the bound")


@pytest.mark.parametrize("path", list(dc.REGIME_PRODS))
def test_admissibility_ladder_of_the_mean_through_R_regime(path):
    """fp32 F.group_norm on the merged tensor against float64, as a fraction of the bound, for |m| / sigma = 3, 10, 30, 100; the GPU test grades
    the kernels at every admissible magnitude and so at the largest"""
    prod, _, B = dc.REGIME_PRODS[path]
    fr = {m: dc.admissible(prod, B, m) for m in dc.LADDER}
    print(f"{path}: fraction of the bound (y, statistics) per |m|/sigma: " + ", ".join(f"{m}: {a:.3f} / {b:.3f}" for m, (a, b) in fr.items()))
    ok = [m for m in dc.LADDER if max(fr[m]) <= dc.ADMISSIBLE_FRACTION]
    assert ok == list(dc.LADDER), f"{path}: admissible magnitudes {ok}: the GPU test's docstring and the README row name all four"
    _, ref, r, full = dc.regime_tensor(prod, 100)
    conv_sd = float(ref.std())
    assert 0.8 <= conv_sd <= 1.3 and abs(float(r.mean()) - 100.0) < 0.05, (conv_sd, float(r.mean()))


# ---- the bindings of the two test-support entries ------------------------------------------------------------------------------------------
def test_lib_declares_the_two_entries():
    i32, i64, vp, f32 = C.c_int, C.c_int64, C.c_void_p, C.c_float
    assert L._SIGS["cgd_op_gemm_ex"] == (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, f32, i32, i32, i32, i32, vp])
    assert L._SIGS["cgd_op_gemm_ex"][1][:16] == L._SIGS["cgd_op_gemm"][1][:16] and L._SIGS["cgd_op_gemm"][1][16] is vp
    assert L._SIGS["cgd_op_pending"] == (i32, [vp, C.POINTER(i64)])
    handle = L.load()
    out = (i64 * 5)(7, 7, 7, 7, 7)
    assert handle.cgd_op_pending(None, out) == -3 and list(out) == [7] * 5  # NULL handle: status -3, nothing written
    assert handle.cgd_op_gemm_ex(None, None, 0, None, 0, None, 0, None, None, 0, 1, 1, 4, 1.0, 0, 1, 0, 0, None) == -3


def test_ops_gemm_ex_passes_strides_and_the_two_switches(monkeypatch):
    lib = _RecordingLib()
    monkeypatch.setattr(ops, "_DEVICE_TYPE", "cpu")
    monkeypatch.setattr(ops, "_s", lambda: 0)
    fake = types.SimpleNamespace(lib=lib, h=None, check=lambda rc: None)
    M, N, K = 6, 8, 12
    A, B = th.zeros(M, K + 4)[:, 4:], th.zeros(N, K)
    Cbuf, Rbuf, bias = th.zeros(M, 3 * N), th.zeros(M, N + 4), th.zeros(N)
    Cv, R = Cbuf[:, N:2 * N], Rbuf[:, :N]
    assert ops.gemm_ex(fake, A, B, bias, R, alpha=0.5, force_tile=513, splitk=5, weight=True, defer=True, out=Cv) is Cv
    ((name, a),) = lib.calls
    assert name == "cgd_op_gemm_ex"
    assert a[1:7] == (A.data_ptr(), K + 4, B.data_ptr(), K, Cv.data_ptr(), 3 * N) and a[7:10] == (bias.data_ptr(), R.data_ptr(), N + 4)
    assert a[10:18] == (M, N, K, 0.5, 513, 5, 1, 1)
    ops.gemm_ex(fake, A, B)
    assert lib.calls[-1][1][13:18] == (1.0, 0, 1, 0, 0)
    ops.gemm_ex(fake, A, B, R=Cv, out=Cv, defer=True)  # an in-place residual: the same pointer and stride twice
    a = lib.calls[-1][1]
    assert a[5:7] == a[8:10] == (Cv.data_ptr(), 3 * N)
    with pytest.raises(ValueError):
        ops.gemm_ex(fake, A.double(), B)


def test_ops_pending_reads_five_fields():
    class Lib:
        def cgd_op_pending(self, h, out):
            for i, v in enumerate((1, 9, 192, 128, 320)):
                out[i] = v
            return 0
    ctx = types.SimpleNamespace(lib=Lib(), h=None, check=lambda rc: None)
    assert ops.pending(ctx) == {"valid": 1, "slices": 9, "rows": 192, "cols": 128, "ldc": 320}
