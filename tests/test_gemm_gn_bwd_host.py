"""cgd_op_gemm_gn_bwd (the weight GEMM with a GroupNorm backward in its epilogue) has no other kernel behind it: what the kernel cannot run is an
error.  cgd_op_gemm_gn_bwd_accepts evaluates the op entry's own predicate on the host, without a GPU or a context."""
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib, ops


def accepts(precision=1, lda=64, ldw=64, lddx=64, ldx=64, lddz=64, ldadd=0, x_misalign=0, B=1, HW=680, N=64, K=64):
    return lib.load().cgd_op_gemm_gn_bwd_accepts(precision, lda, ldw, lddx, ldx, lddz, ldadd, x_misalign, B, HW, N, K)


def test_accepts_the_supported_problems():
    assert accepts() == 1
    assert accepts(N=512, K=320, lda=328, ldx=544, lddz=516, lddx=536, ldadd=520, ldw=320) == 1  # channel slices of wider buffers
    assert accepts(B=2, HW=256) == 1 and accepts(B=1, HW=65536, N=512, K=256, lda=256, ldw=256, ldx=512, lddz=512, lddx=512, ldadd=512) == 1


def test_refuses_other_precision_modes():
    assert accepts(precision=0) == 0  # exact fp32: the GEMM stays on the fp32 kernel, which has no such epilogue
    assert accepts(precision=2) == 0  # bf16: the kernel's LDS epilogue exists in the bf16x3 mode only


@pytest.mark.parametrize("bad", [dict(ldx=66), dict(lddz=65), dict(ldadd=67), dict(lddx=70), dict(lda=66), dict(x_misalign=4), dict(x_misalign=8),
                                 dict(K=96, lda=96, ldw=96), dict(N=48), dict(B=2, HW=340), dict(B=0), dict(HW=0)])
def test_refuses_strides_alignment_and_shapes_the_kernel_cannot_run(bad):
    assert accepts(**bad) == 0


def test_null_context_and_cpu_tensors():
    assert lib.load().cgd_op_gemm_gn_bwd(None, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, None, 1, 128, 32, 64, None) == -3
    t = th.zeros(1, 128, 64)
    with pytest.raises(ValueError):
        ops.gemm_gn_bwd(object(), t, th.zeros(64, 64), t, t, th.zeros(1, 64, 4), th.zeros(1, 64, 4))
