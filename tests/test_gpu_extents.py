"""Op kernels on operands whose extent crosses 2 GiB (pytest -m gpu): one operand per case with a row stride that puts its rows just below,
at and beyond the 2^31-byte line the buffer-load kernels are guarded at (tier A, about 4.3 GiB reserved per case, a few hundred kilobytes
touched) or beyond 2^31 elements (tier B, about 17 GiB; skipped only when the device has less than twice that free).  Strict parity against
float64, no write outside the view or at any address a 32-bit wrap of the offset would reach, bit-identical reruns, the route each case
claims, refusals that write nothing (tests/extent_checks.py explains the far operands)."""
import pytest

from tests import extent_checks as ec
from tests.test_gpu_parity import _assert_all

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", [0, 1])
def test_gemm_far_a(precision):
    _assert_all(ec.check_gemm_far_a(precision))


@pytest.mark.parametrize("precision", [0, 1])
def test_gemm_far_c_and_r(precision):
    _assert_all(ec.check_gemm_far_cr(precision))


def test_gemm_gn_bwd_far_operands_and_its_predicate():
    _assert_all(ec.check_gemm_gn_bwd_far())


@pytest.mark.parametrize("precision", [0, 1])
def test_conv3x3_far_operands(precision):
    _assert_all(ec.check_conv_far(precision))


@pytest.mark.parametrize("precision", [0, 1])
def test_conv3x3_winograd_far_operands(precision):
    _assert_all(ec.check_wino_far(precision))


def test_conv3x3_winograd_groupnorm_records_of_a_far_output():
    _assert_all(ec.check_wino_records_far())


@pytest.mark.parametrize("precision", [0, 1])
def test_conv3x3_stride2_far_operands(precision):
    _assert_all(ec.check_sconv_far(precision))


def test_groupnorm_far_operands():
    _assert_all(ec.check_gn_far())


def test_conv_thin_out_far_input():
    _assert_all(ec.check_thin_out_far())


def test_sr_stem_far_output():
    _assert_all(ec.check_sr_stem_far())


def test_gram_at_and_beyond_its_stride_cap():
    _assert_all(ec.check_gram_far())


def test_tier_b_gemm_far_c_and_r_beyond_2_31_elements():
    _assert_all(ec.check_gemm_far_cr(1, tier_b=True))


def test_tier_b_groupnorm_far_output_beyond_2_31_elements():
    _assert_all(ec.check_gn_far(tier_b=True))
