"""Op kernels on strided, sliced and misaligned operands (pytest -m gpu): parity against float64 at the strict criterion of
test_gpu_parity.py, no write outside the output view, bit-identical reruns, and the kernel family each case claims to cover
(tests/strided_checks.py explains the guarded buffers)."""
import pytest

from tests import strided_checks as sc
from tests.test_gpu_parity import _assert_all

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", [0, 1])
def test_gemm_strided_operands(precision):
    _assert_all(sc.check_gemm_strided(precision))


@pytest.mark.parametrize("precision", [0, 1])
def test_conv3x3_strided_operands(precision):
    _assert_all(sc.check_conv_strided(precision))


@pytest.mark.parametrize("precision", [0, 1])
def test_conv3x3_winograd_strided_operands(precision):
    _assert_all(sc.check_wino_strided(precision))


def test_conv3x3_winograd_groupnorm_records_on_strided_operands():
    _assert_all(sc.check_wino_records_strided())


def test_conv_thin_out_on_a_channel_slice():
    _assert_all(sc.check_thin_out_strided())


def test_groupnorm_strided_operands():
    _assert_all(sc.check_gn_strided())


def test_layernorm_and_activation_strided_operands():
    _assert_all(sc.check_ln_act_strided())


def test_resample_refusals_leave_the_output_untouched():
    _assert_all(sc.check_resample_refusals())
