"""Deferred split-K slices through the norms that sum them (pytest -m gpu; tests/defer_checks.py explains the verdicts): every producer is
asserted split, every consumer's path (slices taken / reduce launch) is asserted through `cgd_op_pending` and the reduce counter, the tensor
written back is bit-equal to the reduce kernel's, outputs are strict against float64, every case runs twice bit for bit."""
import pytest

from tests import defer_checks as dc
from tests.test_gpu_parity import _assert_all

pytestmark = pytest.mark.gpu

_CASES = [(grp, c) for grp, fn in dc.GROUPS.items() for c in fn()]


@pytest.mark.parametrize("case", [c for _, c in _CASES], ids=[f"{grp}: {c.name}" for grp, c in _CASES])
def test_deferred_slices_producer_to_consumer(case):
    _assert_all(dc.run_case(dc.shared_ctx(case.precision), case))


def test_every_case_names_a_different_combination():
    names = [c.name for _, c in _CASES]
    assert len(set(names)) == len(names)


def test_consumer_that_differs_in_one_key_flushes():
    _assert_all(dc.check_mismatch())


def test_groupnorm_over_the_whole_concat_buffer_flushes():
    _assert_all(dc.check_concat_whole())


def test_gemm_between_and_two_deferred_producers_back_to_back():
    _assert_all(dc.check_gemm_between())


def test_refused_consumer_leaves_the_entry_pending():
    _assert_all(dc.check_refused_consumer())


def test_pending_entry_across_new_pass_and_set_precision():
    _assert_all(dc.check_state_changes())


def test_consumer_on_a_second_stream_is_ordered_behind_the_producer():
    _assert_all(dc.check_second_stream())


def test_cgd_defer_0_and_1_in_fresh_contexts():
    _assert_all(dc.check_defer_modes())


def test_other_readers_get_the_finished_tensor():
    _assert_all(dc.check_other_readers())


@pytest.mark.parametrize("path", list(dc.REGIME_PRODS))
def test_groupnorm_when_the_residual_carries_the_mean(path):
    """Value regime: the shift of the GroupNorm sums is taken from the slices without R, so a mean that arrives through R is not shifted away.
    Graded at every admissible magnitude of the ladder |m| / sigma = 3, 10, 30, 100 (all four are admissible: tests/test_defer_host.py), R
    separate and in place."""
    recs = dc.check_mean_through_R(path)
    assert sum("admissible" in r["name"] and "NOT" not in r["name"] for r in recs) >= 1
    _assert_all(recs)
