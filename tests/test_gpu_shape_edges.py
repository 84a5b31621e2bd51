"""Op kernels at the edges of the shapes their launchers accept (pytest -m gpu): per kernel family, the smallest accepted value of every
dimension and one granule either side of every tile size, on both sides of each accept / route / refuse clause (tests/shape_edge_checks.py
holds the table and names the clauses).  Every accepted row: strict parity against float64, intact NaN sentinels around every output view,
a bit-identical rerun, the claimed route.  Every refused row: the call raised with its text and wrote nothing; a shape that a forced route
refuses runs again with force_tile = 0 (family "fallthrough")."""
import pytest
import torch as th

from tests import shape_edge_checks as se
from tests.parity_checks import MIN_PEAK
from tests.test_gpu_parity import _assert_all

pytestmark = pytest.mark.gpu

PAIRED = {("hgemm2", "p1"), ("hgemm2", "p1_epi0")}  # run together by test_hgemm2_epilogues_agree_bit_for_bit_at_the_tile_edges


def _judge(recs, fam, ck):
    assert recs, (fam, ck)
    missing = se.verdicts_complete(recs, fam, ck)
    assert not missing, f"rows without all of their verdicts: {missing}"
    sanity = se.CONTEXTS[ck][0] == 2
    _assert_all(recs, allowed=("strict", "sanity") if sanity else ("strict",))
    if sanity:
        par = [r for r in recs if r["verdict"] == "parity"]
        assert not all(r["ok_strict"] for r in par), "a single bf16 product cannot meet the fp32 tolerance: the strict criterion is not biting"
    # the only records graded on a reference of (nearly) zero peak: dq and dk at T = 1
    small = [r["name"] for r in recs if r["verdict"] == "parity" and r["ref_max"] < MIN_PEAK]
    assert all(" T1 " in n and (n.endswith(" dq") or n.endswith(" dk")) for n in small), small


@pytest.mark.parametrize("fam,ck", [gk for gk in se.GROUPS if gk not in PAIRED], ids=[f"{f}-{c}" for f, c in se.GROUPS if (f, c) not in PAIRED])
def test_shape_edges(fam, ck):
    _judge(se.check_group(fam, ck), fam, ck)


def test_hgemm2_epilogues_agree_bit_for_bit_at_the_tile_edges():
    """CGD_HGEMM_EPI = 1 (the block through LDS, whole-line stores) and 0 (per-lane 16-byte accesses): the same operations per element in
    the same order, so every row of the hgemm2 table, split or not, ragged or not, must come out bit-identical on the two"""
    keep = {"p1": {}, "p1_epi0": {}}
    for ck in keep:
        _judge(se.check_group("hgemm2", ck, keep=keep[ck]), "hgemm2", ck)
    assert keep["p1"] and set(keep["p1"]) == set(keep["p1_epi0"])
    differ = [n for n, a in keep["p1"].items() if not th.equal(a.view(th.int32), keep["p1_epi0"][n].view(th.int32))]
    assert not differ, differ
