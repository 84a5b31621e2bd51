"""Host-side argument for tests/test_gpu_extents.py (CPU, `not gpu`): every case the launchers ACCEPT stays inside its operand, and each guard
sits on (or within one row below) the line where its kernel would go wrong.

Offset models: numpy restatements, in 32-bit arithmetic with wrap-around, of the byte offsets the buffer-load staging loops form (the per-lane
`voffset`, a wave-uniform `soffset`, the resource's `records`; csrc/mfma_stage.h):
    hgemm2  aoffb[j] = row < M ? ((row * lda + c4 * 4) * 4) : 0x80000000, so_ = chunk * 256 KG, records 2^31         (hgemm.hip)
    kgemm   aoffb[i] = ((row * lda + 8 hh) * 4), NO clamp for rows >= M, records M * lda * 4 (unsigned)              (hgemm.hip)
    hconv2 / kconv  poffb = in-image ? ((y * Ws + x) * lda + c4 * 4) * 4 : 0x80000000, chunk * 128, records 2^31      (hconv.hip, kconv.hip)
    wconv   poffv = (rowoff | colo) >= 0 ? (rowoff + colo) * 4 : 0x80000000, chunk * 128, records 2^31               (wconv.hip)
    Gram    (row * lda + cq * 4) * 4, records ((nvalid - 1) * lda + C) * 4 per slab                                  (gram.hip)
    flash attention  (row * ld + 4 dq) * 4, records min(nvalid, 32) * ld * 4                                         (attn_flash.hip fa_rows_rsrc)
A lane is judged as the hardware does: it reads memory iff its unsigned voffset is below `records`, at base + voffset + soffset.
    wanted lane (row < M, pixel inside the image, row < nvalid): voffset >= 0 as a signed number, voffset + soffset = the true byte offset (nothing
        wrapped), the 16 bytes end at or before `records` and inside the operand's extent;
    masked lane (padding pixel, row >= M, row >= nvalid): unsigned voffset >= records, so no memory is touched.
Guards (restated in GUARD and tied to the library through the planner below): M * lda < 2^29 floats (hgemm2, kgemm), H * W * lda * 4 < 2^31 bytes
with H x W the OUTPUT pixels (hconv2, kconv, wconv), lda <= 2^20 (Gram).  Each guard counts one more row than the kernel addresses (M * lda, not
(M - 1) * lda + K), so the first stride at which a model really fails lies up to one row's share above the guard's `at` stride: the tightness
tests assert at <= first failing stride <= the stride that puts the LAST row's start at 2^31 bytes, plus one step.  Gram's cap is a flat 2^20 for
every C: the model first fails at 2^31 / (4 * 255) (C = 64, 256-row slabs), a factor two above the cap.  The attention loaders have no guard:
their stride is 3 * heads * d of a dense qkv, and the model first fails at 2^24 floats.

One finding the models made, fixed with them: kgemm's rows beyond M are NOT clamped, only `records` masks them.  With few rows on a huge stride
(M = 5, lda near 2^29 / 5) the byte offset of a row beyond M passed 2^32 and wrapped to a small offset BELOW `records`: row 11 read row 1, and
row 15 read the last bytes of row 4's stride plus the k-step offset, i.e. up to 1 KB BEYOND M * lda * 4 - outside the operand (the products land in
accumulator rows that are never stored, so no result was wrong; the read itself was the defect).  cgd_kgemm_capable now also requires
ceil(M / 64) * 64 * lda < 2^30, which no shape of the nets comes near; the model asserts that under both rules no masked lane is below `records`,
and that the old rule alone let such lanes through.

Not covered here: the size limits (`lim`) of cgd_cutouts_resize_* / cgd_cutouts_aug_* have no host-only entry (every entry takes a device
context first), so they are left out rather than reached through device calls."""
import ctypes as C

import numpy as np
import pytest

from tests import extent_checks as ec

P31, P32 = 1 << 31, 1 << 32
OOB = -P31  # CGD_OOB as a signed 32-bit number
GUARD = {"gemm_floats": 1 << 29, "kgemm_padded_floats": 1 << 30, "conv_bytes": 1 << 31, "gram_lda": 1 << 20}


def i32(v):
    """wrap an int64 array to signed 32 bits, as the kernels' `int` arithmetic does on the hardware"""
    return ((np.asarray(v, dtype=np.int64) + P31) % P32) - P31


def judge(voff, soff, wanted, true, records, extent):
    """violations of the conditions in the module docstring; voff (signed 32-bit), soff, true (int64 bytes) and wanted (bool) broadcast together"""
    voff, soff, wanted, true = np.broadcast_arrays(np.asarray(voff, np.int64), np.asarray(soff, np.int64), wanted, np.asarray(true, np.int64))
    uoff = voff % P32
    bad_wanted = wanted & ((voff < 0) | (voff + soff != true) | (uoff + 16 > records) | (voff + soff + 16 > records) | (true + 16 > extent))
    bad_masked = ~wanted & (uoff < records)
    return int(bad_wanted.sum()), int(bad_masked.sum())


# ---- the models -----------------------------------------------------------------------------------------------------------------------------
def hgemm2(M, lda, K, TM=64, KG=1):
    tid = np.arange(256 * KG)
    c4, r0 = tid & (16 * KG - 1), tid // (16 * KG)
    m0 = np.arange(0, M, TM)
    row = m0[:, None, None] + r0[None, :, None] + 16 * np.arange(TM // 16)[None, None, :]  # [tile][thread][slot]
    ok = row < M
    aoff = i32(np.where(ok, row, M - 1) * lda + c4[None, :, None] * 4)
    voff = np.where(ok, i32(aoff * 4), OOB)
    chunk = np.arange(K // (64 * KG))
    soff = chunk * (64 * KG * 4)
    true = (row * lda + c4[None, :, None] * 4) * 4
    ext = ((M - 1) * lda + K) * 4
    return judge(voff[..., None], soff, ok[..., None], true[..., None] + soff, P31, ext)


def kgemm(M, lda, K, NI=2, detail=False):
    lane = np.arange(64)
    l31, hh = lane & 31, lane >> 5
    m0 = np.arange(0, M, 32 * NI)
    row = m0[:, None, None] + 32 * np.arange(NI)[None, :, None] + l31[None, None, :]
    ok = row < M
    voff = i32(i32(row * lda + 8 * hh[None, None, :]) * 4)
    arec = (M * lda * 4) % P32
    kq = np.arange(K // 16)
    soff = 64 * kq
    true = (row * lda + 8 * hh[None, None, :]) * 4
    ext = ((M - 1) * lda + K) * 4
    a = judge(voff[..., None], soff, ok[..., None], true[..., None] + soff, arec, ext)
    b = judge(voff[..., None] + 16, soff, ok[..., None], true[..., None] + 16 + soff, arec, ext)
    if detail:  # the masked lanes below `records`: where do they read?
        u = voff % P32
        inside = ~ok & (u < arec)
        return int(inside.sum()), bool((u[inside] + 32 + soff.max() <= M * lda * 4).all())
    return a[0] + b[0], a[1] + b[1]


def halo(H, W, lda, Cin, ups=0, wino=False):
    """hconv2 / kconv (one product) and wconv (row and column offsets summed): every pixel of the image plus its one-pixel frame"""
    Hs, Ws = (H >> 1, W >> 1) if ups else (H, W)
    y, x = np.arange(-1, H + 1)[:, None, None], np.arange(-1, W + 1)[None, :, None]
    c4 = np.arange(8)[None, None, :]
    inb = (y >= 0) & (y < H) & (x >= 0) & (x < W) & (c4 >= 0)
    ys, xs = (y >> 1, x >> 1) if ups else (y, x)
    if wino:
        rowoff = np.where((y >= 0) & (y < H), i32(i32(ys * Ws) * lda), -1)
        colo = np.where((x >= 0) & (x < W), i32(i32(xs * lda) + c4 * 4), -1)
        voff = np.where((rowoff | colo) >= 0, i32(i32(rowoff + colo) * 4), OOB)
        voff = np.broadcast_to(voff, inb.shape)
    else:
        poff = np.where(inb, i32(i32(ys * Ws + xs) * lda + c4 * 4), -1)
        voff = np.where(poff >= 0, i32(poff * 4), OOB)
    soff = np.arange(Cin // 32) * 128
    true = ((ys * Ws + xs) * lda + c4 * 4) * 4 + 0 * inb
    ext = ((Hs * Ws - 1) * lda + Cin) * 4
    return judge(voff[..., None], soff, inb[..., None], true[..., None] + soff, P31, ext)


def gram(N, lda, Cc):
    SR = 16384 // Cc
    bw = bm = 0
    for row0 in range(0, N, SR):
        nvalid = min(SR, N - row0)
        records = (((nvalid - 1) * lda + Cc) * 4) % P32
        q = np.arange(SR * Cc // 4)
        row, cq = q // (Cc // 4), q % (Cc // 4)
        true = (row * lda + cq * 4) * 4
        a = judge(i32(true), 0, row < nvalid, true, records, ((nvalid - 1) * lda + Cc) * 4)
        bw, bm = bw + a[0], bm + a[1]
    return bw, bm


def flash_rows(ld, nvalid, D=64):
    lane = np.arange(64)
    row = np.arange(32)[:, None]  # fa_row(lane, i) runs over the block's 32 rows
    dq = (lane & 15)[None, :]
    nv = min(nvalid, 32)
    records = i32(i32(nv * ld) * 4) % P32
    true = (row * ld + 4 * dq) * 4
    return judge(i32(i32(row * ld + 4 * dq) * 4), 0, (row < nv) & (dq >= 0), true, records, ((nv - 1) * ld + D) * 4)


def first_bad(model, lo, hi):
    """smallest multiple of 4 in (lo, hi] at which `model(ld)` reports a violation (the models are monotone in the stride); lo passes, hi fails"""
    assert model(lo) == (0, 0) and model(hi) != (0, 0)
    while hi - lo > 4:
        mid = (lo + hi) // 2 // 4 * 4
        if model(mid) == (0, 0):
            lo = mid
        else:
            hi = mid
    return hi


def strides_upto(at):
    """a grid of strides on the accepted side of a guard: small, a few decades, and the last steps below `at`"""
    return sorted({260, 4096, 65536 + 4, at // 4 // 4 * 4, at // 2, at - 64, at - 8, at - 4})


# ---- accepted cases stay inside; the guards sit on their lines ------------------------------------------------------------------------------
@pytest.mark.parametrize("TM,KG", [(64, 1), (96, 1), (128, 1), (64, 2)])
def test_hgemm2_offsets_below_the_guard_and_first_failure(TM, KG):
    M, K = 130, 256
    below, at = ec.below_at(GUARD["gemm_floats"], M)
    assert (below, at) == (4129776, 4129780)
    for lda in strides_upto(at):
        assert hgemm2(M, lda, K, TM, KG) == (0, 0), lda
    fb = first_bad(lambda ld: hgemm2(M, ld, K, TM, KG), below, ec.far_ld(M) + 4)
    assert at <= fb <= ec.far_ld(M) + 4, (at, fb)  # the guard is safe, and conservative by less than one row's share of the stride
    assert hgemm2(M, ec.far_ld(M), K, TM, KG)[0] > 0  # the `beyond` stride of the GPU cases: a wanted lane of the last row fails


@pytest.mark.parametrize("NI", [1, 2])
def test_kgemm_offsets_below_the_guard_and_first_failure(NI):
    M, K = 70, 256
    below, at = ec.below_at(GUARD["gemm_floats"], M)
    for lda in strides_upto(at):
        assert kgemm(M, lda, K, NI) == (0, 0), lda  # rows 70 .. 127 are masked by `records` alone: (127 * lda * 4) stays below 2^32
    fb = first_bad(lambda ld: kgemm(M, ld, K, NI), below, ec.far_ld(M) + 4)
    assert at <= fb <= ec.far_ld(M) + 4, (at, fb)
    assert kgemm(M, ec.far_ld(M), K, NI)[0] > 0  # the last row's offset no longer fits a signed 32-bit number


def kgemm_accepts(M, lda):
    """cgd_kgemm_capable's two extent rules"""
    return M * lda < GUARD["gemm_floats"] and -(-M // 64) * 64 * lda < GUARD["kgemm_padded_floats"]


def test_kgemm_unclamped_rows_beyond_m_never_wrap_back_into_range():
    K = 256
    wrapped = 0
    for M in (5, 8, 16, 31, 32, 33, 63, 64, 65, 70, 130):
        old_rule, _ = ec.below_at(GUARD["gemm_floats"], M)
        lda = old_rule
        while not kgemm_accepts(M, lda):
            lda = min(lda - 4, GUARD["kgemm_padded_floats"] // (-(-M // 64) * 64) // 4 * 4)
        assert kgemm_accepts(M, lda) and not kgemm_accepts(M, lda + 4) or lda == old_rule
        for NI in (1, 2):
            for ld in (260, lda // 2 // 4 * 4, lda - 4, lda):
                assert kgemm(M, ld, K, NI) == (0, 0), (M, ld, NI)
        # what the M * lda rule alone let through on 64-row tiles: masked lanes below `records`, some of which read past the operand
        n, inside = kgemm(M, old_rule, K, 2, detail=True)
        assert kgemm(M, old_rule, K, 2)[0] == 0  # (the wanted lanes were right all along)
        wrapped += n > 0
        if n:
            assert not kgemm_accepts(M, old_rule), M
        if M == 5:
            assert n > 0 and not inside  # row 15 lands 96 bytes before M * lda * 4 and reads up to 1 KB from there
    assert wrapped >= 4


@pytest.mark.parametrize("wino", [False, True])
@pytest.mark.parametrize("ups", [0, 1])
def test_halo_conv_offsets_below_the_guard_and_first_failure(wino, ups):
    H = W = 16
    Cin = 64
    below, at = ec.below_at(GUARD["conv_bytes"] // 4, H * W)
    assert (below, at) == ((1 << 21) - 4, 1 << 21)
    for ldx in strides_upto(at):
        assert halo(H, W, ldx, Cin, ups, wino) == (0, 0), ldx
    rows = (H >> ups) * (W >> ups)  # the guard counts the output's pixels; an upsampled input has a quarter of them
    hi = ec.far_ld(rows) + 4
    fb = first_bad(lambda ld: halo(H, W, ld, Cin, ups, wino), below, hi)
    assert at <= fb <= hi, (at, fb)
    if not ups:
        assert halo(H, W, ec.far_ld(H * W), Cin, 0, wino)[0] > 0  # the `beyond` stride of the GPU cases


def test_halo_conv_offsets_at_the_real_levels():
    for H, W, Cin in ((64, 64, 256), (32, 48, 512), (128, 128, 128), (8, 8, 1024)):
        for ldx in (Cin, 2 * Cin, 3 * Cin):
            for wino in (False, True):
                assert halo(H, W, ldx, Cin, 0, wino) == (0, 0)


def test_gram_offsets_up_to_the_cap_and_first_failure():
    for Cc in (64, 128, 256, 512):
        for lda in (Cc, 4096, GUARD["gram_lda"] - 4, GUARD["gram_lda"]):
            assert gram(512 + 3, lda, Cc) == (0, 0), (Cc, lda)  # two slabs and a ragged third at C = 64
    # the cap is flat: for the tallest slab (C = 64, 256 rows) the model first fails a factor two above it
    fb = first_bad(lambda ld: gram(512, ld, 64), GUARD["gram_lda"], 1 << 22)
    assert fb == -(-(P31 - 64 * 4 + 1) // (255 * 4) // 4) * 4 or GUARD["gram_lda"] < fb <= (1 << 21) + (1 << 14), fb
    assert fb > GUARD["gram_lda"]


def test_flash_attention_row_loaders_at_every_tower_width_and_first_failure():
    for width in (512, 768, 1024, 1280, 1664, 4096):  # heads * d of the towers and UNets; the qkv row stride is three times that
        for nvalid in (1, 7, 32, 50):
            assert flash_rows(3 * width, nvalid) == (0, 0)
    fb = first_bad(lambda ld: flash_rows(ld, 32), 3 * 4096, 1 << 26)
    assert (1 << 24) <= fb <= ec.far_ld(32) + 4, fb  # no guard: 32 rows * ld * 4 bytes reach 2^31 at ld = 2^24, the last row's start a row later


# ---- the stride-2 conv (sconv.hip SC_GLOAD): off = ok ? ((a_pix + yy * Ws + xx) * lda + kin) * 4 : 0x80000000 with records a_bytes = the operand's
# extent; weights b_off = n < N ? n * ldb * 4 : 0x80000000, off = b_off < 0 ? 0x80000000 : b_off + ((tap * Kc + kin) * 4), records b_bytes.  No soffset.
def sconv_a(dgrad, B, H, W, lda, Kc):
    """the gathered operand: x (forward: taps 2 r - 1 .. 2 r + 1) or dy (backward: taps r, r + 1 over the four parity classes), every row of the
    64-row tiles (rows beyond M are masked by a_ok) x every tap x every 16-byte lane of a tap's Kc channels"""
    Ho, Wo = H // 2, W // 2
    Hs, Ws = (Ho, Wo) if dgrad else (H, W)
    M = B * Ho * Wo
    m = np.arange(-(-M // 64) * 64)[:, None, None, None]
    b, rem = m // (Ho * Wo), m % (Ho * Wo)
    r, c = rem // Wo, rem % Wo
    d = (np.arange(2) if dgrad else np.arange(-1, 2))
    yy = (r if dgrad else 2 * r) + d[None, :, None, None]
    xx = (c if dgrad else 2 * c) + d[None, None, :, None]
    kin = np.arange(0, Kc, 4)[None, None, None, :]
    ok = (m < M) & (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws) & (kin >= 0)
    pix = b * Hs * Ws + yy * Ws + xx
    voff = np.where(ok, i32(i32(i32(pix) * lda + kin) * 4), OOB)
    ext = ((B * Hs * Ws - 1) * lda + Kc) * 4
    return judge(voff, 0, ok, (pix * lda + kin) * 4, ext % P32, ext)


def sconv_b(N, Kc, rows=None):
    """the packed weights [N][9 Kc] (dense: ldb = 9 Kc), rows n of the 32-row tiles (all, or the given ones)"""
    n = (np.arange(-(-N // 32) * 32) if rows is None else np.asarray(rows))[:, None, None]
    tap, kin = np.arange(9)[None, :, None], np.arange(0, Kc, 4)[None, None, :]
    b_off = np.where(n < N, i32(i32(n * (9 * Kc)) * 4), OOB)
    wanted = (n < N) & (tap >= 0) & (kin >= 0)
    voff = np.where(b_off < 0, OOB, i32(b_off + i32((tap * Kc + kin) * 4)))
    ext = N * 9 * Kc * 4
    return judge(voff, 0, wanted, (n * 9 * Kc + tap * Kc + kin) * 4, ext % P32, ext)


@pytest.mark.parametrize("dgrad", [0, 1])
@pytest.mark.parametrize("B,Kc", [(1, 32), (2, 64)])
def test_sconv_gather_offsets_below_the_guard_and_first_failure(dgrad, B, Kc):
    H = W = 8
    rows = B * (H // 2) * (W // 2) if dgrad else B * H * W
    below, at = ec.sconv_below_at(rows, Kc)
    for lda in sorted({Kc, Kc + 4, 4096, 65536 + 4, below // 4 // 4 * 4, below // 2 // 4 * 4, below - 64, below - 4, below}):
        assert sconv_a(dgrad, B, H, W, lda, Kc) == (0, 0), lda
    # the guard counts the extent to the byte, so the model fails right at the guard's `at` stride or one step later (the last 16-byte lane of the
    # last row ends at the extent): at <= first failure <= at + 4, well within one row below the stride that puts the last ROW's start at 2^31
    fb = first_bad(lambda ld: sconv_a(dgrad, B, H, W, ld, Kc), below, ec.far_ld(rows) + 4)
    assert at <= fb <= at + 4 <= ec.far_ld(rows) + 4, (at, fb)
    assert sconv_a(dgrad, B, H, W, ec.far_ld(rows), Kc)[0] > 0


def test_sconv_gather_offsets_at_the_real_levels_and_the_gpu_cases():
    for (H, C_) in ((256, 128), (128, 128), (64, 256), (32, 256), (16, 512)):  # the five Downsamples of the community checkpoints at 256 x 256
        for ld in (C_, 2 * C_):
            assert sconv_a(0, 1, H, H, ld, C_) == (0, 0) and sconv_a(1, 1, H, H, ld, C_) == (0, 0)
    for far, Bn, Ci, Co in ec.SCONV_FAR:
        shape, dgrad = ec.sconv_far_shape(far, Bn, Ci, Co)
        if far in ("x", "dy"):
            rows = int(np.prod(shape[:-1]))
            lb, la = ec.sconv_below_at(rows, shape[-1])
            assert sconv_a(dgrad, Bn, 8, 8, lb, shape[-1]) == (0, 0)
        assert sconv_b(Ci if dgrad else Co, Co if dgrad else Ci) == (0, 0)


def test_sconv_weight_offsets_either_side_of_the_guard():
    """Cin * Cout * 9 * 4 < 2^31: 7712 x 7712 channels is the last accepted square, 7744 the first refused"""
    edge = lambda N: [0, 1, N // 2, N - 33, N - 2, N - 1] + list(range(N, -(-N // 32) * 32 + 32))  # noqa: E731
    for N, Kc in ((32, 32), (96, 160), (512, 512), (1024, 1024)):
        assert sconv_b(N, Kc) == (0, 0)
    assert 7712 * 7712 * 36 < P31 <= 7744 * 7744 * 36
    assert sconv_b(7712, 7712, edge(7712)) == (0, 0)
    assert sconv_b(7744, 7744, edge(7744))[0] > 0
    lib = handle_()
    for dgrad in (0, 1):
        assert lib.cgd_op_conv3x3_s2_accepts(dgrad, 7712, 7712, 0, 1, 2, 2, 7712, 7712) == 1
        assert lib.cgd_op_conv3x3_s2_accepts(dgrad, 7744, 7744, 0, 1, 2, 2, 7744, 7744) == 0


def test_sconv_predicate_either_side_of_every_operand_line():
    lib = handle_()
    for far, Bn, Ci, Co in ec.SCONV_FAR:
        shape, dgrad = ec.sconv_far_shape(far, Bn, Ci, Co)
        lb, la = ec.sconv_below_at(int(np.prod(shape[:-1])), shape[-1])
        cin, cout = (Co, Ci) if dgrad else (Ci, Co)
        for ld, want in ((lb, 1), (la, 0)):
            lds = {"in": cin + 32, "out": cout + 32, "add": Ci + 48 if dgrad else 0}
            lds[{"x": "in", "dy": "in", "y": "out", "dx": "out", "add": "add"}[far]] = ld
            assert lib.cgd_op_conv3x3_s2_accepts(dgrad, lds["in"], lds["out"], lds["add"], Bn, 8, 8, Ci, Co) == want, (far, ld)
            lay = ec.far_layout(shape, ld, ld - shape[-1])
            assert lay["n"] * 4 < 4.5 * 2 ** 30


def handle_():
    import cgd_amd  # noqa: F401
    from cgd_amd import lib as L
    return L.load()


def test_the_model_checker_notices_a_moved_guard():
    """the restated constants are what the tightness tests hang on: one stride step above each, a model that is asked to run anyway must not be
    reported clean for the WRONG reason - kgemm's `records` wraps right at the guard, the others hold for less than one more row"""
    M = 70
    _, at = ec.below_at(GUARD["gemm_floats"], M)
    assert (M * at * 4) >= P31 and kgemm(M, ec.far_ld(M), 256, 2)[0] > 0
    _, at = ec.below_at(2 * GUARD["gemm_floats"], 130)  # a guard widened to 2^30: every model fails at its `at`
    assert hgemm2(130, at, 256)[0] > 0
    _, at = ec.below_at(2 * GUARD["conv_bytes"] // 4, 256)
    assert halo(16, 16, at, 64)[0] > 0 and halo(16, 16, at, 64, 0, True)[0] > 0


# ---- the planner: the library's guards sit where GUARD says -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    import cgd_amd  # noqa: F401
    from cgd_amd import lib as L
    return L.load()


def _plan(h, M, N, K):
    o = (C.c_int * 4)()
    assert h.cgd_op_plan(0, M, N, K, 0, 0, 0, 1, 1, 256, o) == 0
    return list(o)


def test_planner_weight_gemm_either_side_of_the_extent_line(handle):
    M, N = 256, 128
    k_at = GUARD["gemm_floats"] // M
    assert k_at == 1 << 21
    assert _plan(handle, M, N, k_at - 64)[:2] == [4, 518]  # the few-row kernel while M * K < 2^29 (K a multiple of 64)
    kernel, tile, sk, wg = _plan(handle, M, N, k_at)
    assert (kernel, tile) == (2, 513)  # at the line: the weight GEMM (hgemm_kernel on the device), on 128-row tiles
    assert wg == sk * -(-M // 128) * -(-N // 128), (sk, wg)
    # few rows: the padded-tile rule of the few-row kernel (64 * K < 2^30) takes over from M * K < 2^29
    k8 = GUARD["kgemm_padded_floats"] // 64
    assert k8 * 64 == GUARD["kgemm_padded_floats"] and k8 % 64 == 0
    assert _plan(handle, 8, N, k8 - 64)[:2] == [4, 518] and _plan(handle, 8, N, k8)[0] != 4
    for M in ((1 << 20) - 128, 1 << 20):  # M * 512 either side of 2^29 with many tiles: the weight GEMM both sides, workgroups cover M
        kernel, tile, sk, wg = _plan(handle, M, N, 512)
        assert (kernel, tile, sk) == (2, 513, 1) and wg == -(-M // 128) * -(-N // 128)


def test_planner_conv_leaves_the_halo_kernels_at_the_extent_line(handle):
    def plan(W):
        o = (C.c_int * 5)()
        assert handle.cgd_op_plan_conv(1, 1024, W, 512, 512, 1, 256, 0, 0, 0, o) == 0
        return list(o)
    assert 1024 * 1008 * 512 * 4 < GUARD["conv_bytes"] == 1024 * 1024 * 512 * 4
    assert plan(1008)[0] == 1
    assert plan(1024)[0] != 1


def test_gemm_gn_bwd_predicate_either_side_of_its_limits(handle):
    acc = handle.cgd_op_gemm_gn_bwd_accepts

    def a(lda=64, Bn=2, HW=256, lddx=96, ldx=96, lddz=96, ldadd=96):
        return acc(1, lda, 64, lddx, ldx, lddz, ldadd, 0, Bn, HW, 96, 64)
    below, at = ec.below_at(GUARD["gemm_floats"], 512)
    assert a() == 1 and a(lda=below) == 1 and a(lda=at) == 0
    far = ec.far_ld(512)
    assert a(lddx=far) == 1 and a(ldx=far) == 1 and a(lddz=far) == 1 and a(ldadd=far) == 1  # 64-bit rows in the epilogue: accepted (and graded on the GPU)
    # Bn * HW: 2^31 - 128 rows fit an int (and are refused by the lda line), 2^31 do not (refused before the product is formed)
    assert a(Bn=1 << 15, HW=(1 << 16) - 128) == 0 and a(Bn=1 << 15, HW=1 << 16) == 0 and a(Bn=0) == 0


# ---- the far operands of the GPU cases ----------------------------------------------------------------------------------------------------------
TIER_A = [("gemm A below", (130, 256), 4129776, 4129776 - 256), ("gemm A at", (130, 256), 4129780, 16), ("gemm A beyond", (130, 256), ec.far_ld(130), 16),
          ("kgemm A", (70, 256), ec.below_at(1 << 29, 70)[0], 16), ("gemm C", (130, 96), ec.far_ld(130), ec.far_ld(130) - 96),
          ("conv x at", (1, 16, 16, 64), 1 << 21, (1 << 21) - 64), ("conv x B2", (2, 16, 16, 64), (1 << 20) + (1 << 17), (1 << 20) + (1 << 17) - 64),
          ("conv y", (1, 16, 16, 64), ec.far_ld(256), 16), ("wino records y", (1, 4096, 64), ec.far_ld(4096), 16), ("gn chunked", (2, 2048, 64), ec.far_ld(4096), 16),
          ("gn streaming", (1, 520, 2048), ec.far_ld(520), 16), ("sr_stem y", (2, 32, 32, 32), ec.far_ld(2048), 16), ("thin x", (1, 16, 24, 64), ec.far_ld(384), 32)]
LARGER = [("gemv A at", (4, 256), 1 << 27, (1 << 27) - 256), ("gemv A beyond", (4, 256), ec.far_ld(4), 16), ("gemv C", (4, 96), ec.far_ld(4), 16),
          ("gram", (2, 512, 64), 1 << 20, (1 << 20) - 64), ("gram refused", (2, 512, 64), (1 << 20) + 4, (1 << 20) + 4 - 64)]
TIER_B = [("gemm C", (130, 96), ec.far_ld(130, True), 16), ("gn register-cached y", (2, 256, 128), ec.far_ld(512, True), 16), ("gn chunked y", (2, 2048, 64), ec.far_ld(4096, True), 16)]


@pytest.mark.parametrize("name,shape,ld,col,cap", [c + (4.5,) for c in TIER_A] + [c + (6.5,) for c in LARGER] + [c + (25.0,) for c in TIER_B])
def test_far_layout_keeps_every_band_and_alias_inside_the_allocation(name, shape, ld, col, cap):
    lay = ec.far_layout(shape, ld, col)
    rows, width, band, base, n = lay["rows"], lay["width"], lay["band"], lay["base"], lay["n"]
    assert 4 * n <= cap * 2 ** 30, f"{name}: {4 * n / 2 ** 30:.2f} GiB"
    assert base % 4 == 0 and base == lay["lead"] + ld + col
    for s in lay["starts"]:
        assert 0 <= base + s and base + s + band <= n
    assert base + (rows - 1) * ld + width <= n  # the view itself
    # the aliases the docstring promises, recomputed: every narrowed offset of every row (and of the row after) is banded
    guard = (band - width) // 2
    for r in (0, 1, rows // 2, rows - 1, rows):
        e = r * ld
        for a in {ec.s32(4 * e) // 4, ec.u32(4 * e) // 4, ec.s32(e), ec.u32(e)} - {e}:
            assert a - guard in lay["starts"], (name, r, a)
    # no alias band covers an element of the view: a wrapped WRITE can never be mistaken for a right one
    for s in lay["alias"]:
        first, last = s, s + band - 1
        for q in (first, last):
            r, c = divmod(q, ld)
            assert not (0 <= r < rows and c < width), (name, s)
    if "beyond" in name or name.startswith(("gemm C", "conv y", "gn", "wino", "sr_stem", "thin")):
        assert (rows - 1) * ld * 4 >= P31 and lay["alias"], name  # the last row really lies beyond the line, and has an alias in the lead-in


def test_strides_of_the_issue():
    assert ec.below_at(1 << 29, 130) == (4129776, 4129780)
    assert ec.below_at(1 << 29, 4) == ((1 << 27) - 4, 1 << 27)
    assert ec.below_at((1 << 31) // 4, 256) == ((1 << 21) - 4, 1 << 21)
    assert ec.s32(P31) == -P31 and ec.s32(P31 - 4) == P31 - 4 and ec.u32(P32 + 8) == 8
