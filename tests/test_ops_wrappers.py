"""CPU tests of the single-op wrappers (cgd_amd/ops.py) against a recording fake of the C library: the row stride and pointer of a
sliced view are what reach the C call, and tensors the ABI cannot express (CPU, non-fp32, non-collapsible layouts) are refused before any
call.  Also the self-test of the guarded-buffer checker of tests/strided_checks.py."""
import types

import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import ops
from tests import strided_checks as sc


class _RecordingLib:
    """every cgd_* attribute is a function that records (name, args) and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("cgd_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def fake(monkeypatch):
    """a context on the recording library; CPU tensors stand in for device tensors"""
    lib = _RecordingLib()
    monkeypatch.setattr(ops, "_DEVICE_TYPE", "cpu")
    monkeypatch.setattr(ops, "_s", lambda: 0)
    return types.SimpleNamespace(lib=lib, h=None, check=lambda rc: None)


def _ptr(t):
    return t.data_ptr()


def test_gemm_passes_the_real_row_strides_of_sliced_views(fake):
    M, N, K = 6, 5, 8
    Abuf, Bbuf = th.zeros(M, K + 12), th.zeros(N, K + 4)
    A, B = Abuf[:, 4:4 + K], Bbuf[:, :K]
    Rbuf, Cbuf = th.zeros(M, N + 3), th.zeros(M, 2 * N + 7)
    R, Cv = Rbuf[:, 2:2 + N], Cbuf[:, N:2 * N]
    bias = th.zeros(N)
    ops.gemm(fake, A, B, bias, R, out=Cv, force_tile=64, splitk=2)
    ((name, a),) = fake.lib.calls
    assert name == "cgd_op_gemm"
    assert a[1:7] == (_ptr(A), K + 12, _ptr(B), K + 4, _ptr(Cv), 2 * N + 7)
    assert a[7:10] == (_ptr(bias), _ptr(R), N + 3)
    assert a[10:13] == (M, N, K) and a[14:16] == (64, 2)


def test_conv_and_groupnorm_take_a_channel_slice_of_a_concat(fake):
    Bn, H, W, C0, C1 = 2, 4, 6, 32, 64
    cat = th.zeros(Bn, H, W, C0 + C1)
    x = cat[..., C0:]  # the second half of the concat: row stride C0 + C1, pointer at channel C0
    wf = th.zeros(16, 9 * C1)
    ops.conv3x3(fake, x, wf)
    (name, a), = fake.lib.calls
    assert name == "cgd_op_conv3x3" and a[1:3] == (_ptr(x), C0 + C1) and a[1] == _ptr(cat) + 4 * C0
    Rbuf = th.zeros(Bn, H, W, 24)
    ops.conv3x3(fake, x, wf, R=Rbuf[..., 4:20])
    a = fake.lib.calls[-1][1]
    assert a[8:10] == (Rbuf[..., 4:20].data_ptr(), 24)
    ops.conv_thin_out(fake, x, th.zeros(3, 9 * C1), None, 3)
    a = fake.lib.calls[-1][1]
    assert fake.lib.calls[-1][0] == "cgd_op_conv_thin_out" and a[1:3] == (_ptr(x), C0 + C1)
    x3 = cat.reshape(Bn, H * W, C0 + C1)[..., C0:]
    gamma, beta, scr = th.zeros(C1), th.zeros(C1), th.zeros(16)
    ops.groupnorm_fwd(fake, x3, gamma, beta, scratch=scr)
    name, a = fake.lib.calls[-1]
    assert name == "cgd_op_gn_fwd" and a[1:3] == (_ptr(x3), C0 + C1) and a[4] == C1  # y is a fresh dense tensor
    dzbuf, addbuf = th.zeros(Bn, H * W, C1 + 8), th.zeros(Bn, H * W, C1 + 16)
    dz, add = dzbuf[..., 8:], addbuf[..., :C1]
    ops.groupnorm_bwd(fake, x3, dz, scr, add=add)
    name, a = fake.lib.calls[-1]
    assert name == "cgd_op_gn_bwd"
    assert a[1:5] == (_ptr(x3), C0 + C1, _ptr(dz), C1 + 8) and a[6] == C1 and a[7:9] == (_ptr(add), C1 + 16)


def test_size_one_dimensions_and_dense_tensors(fake):
    A = th.zeros(1, 8)[:, :]  # one row: the stride of the size-1 dimension carries no layout
    ops.gemm(fake, A, th.zeros(4, 8))
    assert fake.lib.calls[-1][1][2] == 8
    x = th.zeros(1, 1, 3, 64)
    ops.conv3x3(fake, x, th.zeros(32, 9 * 64))
    assert fake.lib.calls[-1][1][2] == 64


@pytest.mark.parametrize("bad", ["cpu", "fp16", "fp64", "permuted", "strided_last", "uncollapsible", "overlapping"])
def test_inputs_the_abi_cannot_express_are_refused_before_any_call(bad, monkeypatch):
    lib = _RecordingLib()
    ctx = types.SimpleNamespace(lib=lib, h=None, check=lambda rc: None)
    monkeypatch.setattr(ops, "_s", lambda: 0)
    if bad != "cpu":
        monkeypatch.setattr(ops, "_DEVICE_TYPE", "cpu")
    M, K = 6, 8
    A = {"cpu": th.zeros(M, K), "fp16": th.zeros(M, K, dtype=th.float16), "fp64": th.zeros(M, K, dtype=th.float64),
         "permuted": th.zeros(K, M).t(), "strided_last": th.zeros(M, 2 * K)[:, ::2],
         "uncollapsible": None, "overlapping": th.zeros(M * K).as_strided((M, K), (4, 1))}[bad]
    with pytest.raises(ValueError):
        if bad == "uncollapsible":
            x = th.zeros(2, 4, 6, 32)[:, :, :3, :]  # rows of 3 pixels out of 6: H and W do not collapse to one row stride
            ops.conv3x3(ctx, x, th.zeros(16, 9 * 32))
        else:
            ops.gemm(ctx, A, th.zeros(4, K))
    assert lib.calls == []


@pytest.mark.parametrize("op", ["groupnorm_fwd", "groupnorm_bwd", "layernorm_fwd", "act", "pool2x2", "upsample2x", "conv_in", "conv3x3_wino"])
def test_every_wrapper_refuses_cpu_and_half_tensors(op, monkeypatch):
    for dtype, dev in ((th.float32, "cuda"), (th.float16, "cpu")):
        lib = _RecordingLib()
        ctx = types.SimpleNamespace(lib=lib, h=None, check=lambda rc: None)
        monkeypatch.setattr(ops, "_s", lambda: 0)
        monkeypatch.setattr(ops, "_DEVICE_TYPE", dev)  # float32 CPU tensors against a GPU requirement, fp16 against the fp32 one
        t3, t4, v = th.zeros(1, 16, 32, dtype=dtype), th.zeros(1, 4, 4, 32, dtype=dtype), th.zeros(32, dtype=dtype)
        call = {"groupnorm_fwd": lambda: ops.groupnorm_fwd(ctx, t3, v, v, scratch=th.zeros(8)),
                "groupnorm_bwd": lambda: ops.groupnorm_bwd(ctx, t3, t3, th.zeros(8)),
                "layernorm_fwd": lambda: ops.layernorm_fwd(ctx, t3[0], v, v),
                "act": lambda: ops.act(ctx, v, 1),
                "pool2x2": lambda: ops.pool2x2(ctx, t4),
                "upsample2x": lambda: ops.upsample2x(ctx, t4),
                "conv_in": lambda: ops.conv_in(ctx, th.zeros(1, 3, 4, 4, dtype=dtype), th.zeros(32, 27, dtype=dtype), None, 32),
                "conv3x3_wino": lambda: ops.conv3x3_wino(ctx, t4, th.zeros(12 * 32 * 32, dtype=dtype), 32)}[op]
        with pytest.raises(ValueError):
            call()
        assert lib.calls == []


def test_dense_only_operands_refuse_views(fake):
    x = th.zeros(4, 64)[:, :32]
    with pytest.raises(ValueError):
        ops.layernorm_fwd(fake, x, th.zeros(32), th.zeros(32))
    with pytest.raises(ValueError):
        ops.act(fake, x, 1)
    assert fake.lib.calls == []


# ---- the guarded-buffer checker of the strided GPU tests ---------------------------------------------------------------------------
def test_guard_checker_flags_a_flipped_guard_word_and_an_unwritten_element():
    ref = th.randn(2, 3, 5, 8, generator=th.Generator().manual_seed(0))
    for ld, col, off in ((12, 2, 1), (8, 0, 4), (20, 12, 0)):
        G = sc.Guarded(ref.shape, ld, col, off, device="cpu")
        assert G.view.stride() == (15 * ld, 5 * ld, ld, 1) and G.ptr == G.buf.data_ptr() + 4 * (off + ld + col)
        G.poison(sc.OUT_BITS[0])
        G.view.copy_(ref)
        recs = sc.check_out("clean", G, ref.double(), sc.OUT_BITS[0])
        assert all(r["ok"] for r in recs), recs
        # one flipped guard word: before the view, between two rows, after the view
        for pos in (0, off + ld + col + 8 if ld > col + 8 else off + 1, G.buf.numel() - 1):
            if G.inside[pos]:
                continue
            w = G.buf.view(th.int32)
            keep = int(w[pos])
            w[pos] = keep ^ 1
            recs = sc.check_out("flipped guard", G, ref.double(), sc.OUT_BITS[0])
            assert [r["ok"] for r in recs] == [True, False], (pos, recs)
            w[pos] = keep
        # one unwritten output element keeps the NaN sentinel: the parity record fails, the guard record does not
        G.view[1, 2, 4, 7] = float("nan")
        G.view.view(th.int32)[1, 2, 4, 7] = sc.OUT_BITS[0]
        recs = sc.check_out("unwritten", G, ref.double(), sc.OUT_BITS[0])
        assert [r["ok"] for r in recs] == [False, True], recs
        # the second sentinel is a different NaN: a stale buffer is not mistaken for a fresh one
        assert not G.intact(sc.OUT_BITS[1])


def test_guarded_inputs_fill_the_gaps_with_the_sentinel():
    G = sc.Guarded((3, 4), 10, 3, 2, device="cpu")
    t = th.arange(12.0).reshape(3, 4)
    G.load(t, sc.GAP[0])
    assert th.equal(G.view, t)
    assert bool((G.buf[~G.inside] == sc.GAP[0]).all()) and int(G.inside.sum()) == 12
