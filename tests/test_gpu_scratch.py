"""Scratch buffers and saved state at their exact size, guarded and poisoned (pytest -m gpu; tests/scratch_checks.py holds the table, the
runners and the detector).  Every buffer a size query sizes is a guarded view of exactly that many floats, filled with quiet NaNs in one run
and with 1.0e6 in the next; every row must carry four verdicts per run: guards bit-intact, outputs strict against the reference of the
entry's own test, outputs bit-equal between the two poisons, and the kernel family or route it claims."""
import pytest

from tests import scratch_checks as sc
from tests.parity_checks import MIN_PEAK
from tests.test_gpu_parity import _assert_all

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fam,ck", sc.GROUPS, ids=[f"{f}-{c}" for f, c in sc.GROUPS])
def test_scratch_and_saved_state(fam, ck):
    recs = sc.check_group(fam, ck)
    rows = sc.rows_of(fam, ck)
    assert recs and rows, (fam, ck)
    missing = sc.verdicts_complete(recs, rows)
    assert not missing, f"rows without all four verdicts: {missing}"
    _assert_all(recs)
    # references of (nearly) zero peak are graded only where the table says the quantity is identically zero
    small = [r["name"] for r in recs if r["verdict"] == "parity" and r["ref_max"] < MIN_PEAK]
    assert all((" T1 " in n and (" dq " in n or " dk " in n)) or "variance half of the seed" in n or (" D1" in n and "d_emb" in n) for n in small), small


def test_the_tier_detects_what_it_is_for():
    """three fake kernels made of torch ops, inside their allocations: one float written into a guard, scratch[0] read before it is
    written, nothing written at all"""
    caught = sc.detector()
    print(caught)
    problems = sc.detector_problems(caught)
    assert not problems, problems
