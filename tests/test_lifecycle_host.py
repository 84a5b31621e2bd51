"""CPU tier of the lifecycle tests (tests/lifecycle_checks.py): no device work.  The scenario tables must do what they say — a walk that no
longer crosses the boundary it names would be a vacuous GPU test — and the `nets.py` wrappers must hand the CURRENT batch and shape to the
library on every call (recording fake of the C library, as in tests/test_ops_wrappers.py)."""
import types

import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import lib, nets
from tests import lifecycle_checks as lc
from tests import parity_checks as pc
from tests.test_cabi import _plan
from tests.test_ops_wrappers import _RecordingLib

HCONV, WCONV, KCONV = 512, 515, 516  # tile codes of the halo, Winograd and weight-streaming conv kernels (cgd_op_plan)


def _conv_plan(B, H, W, cin, cout, precision=1):
    rc, (kernel, tile, splitk, _) = _plan(lib.load(), conv=1, M=B * H * W, N=cout, H=H, W=W, Cin=cin, precision=precision)
    assert rc == 0
    return kernel, tile, splitk


def _levels(case, B, H, W):
    """(B, h, w, channels) of every resolution level of the UNet configuration"""
    kw = pc.UNET_CASES[case]
    mult = kw.get("channel_mult") or nets.DEFAULT_CHANNEL_MULT[kw["image_size"]]
    return [(B, H >> lvl, W >> lvl, int(m * kw["model_channels"])) for lvl, m in enumerate(mult)]


def test_the_walk_crosses_the_winograd_threshold_and_changes_the_kernel_family_of_the_first_level():
    first = lambda k: _levels(lc.UNET_CASE, *lc.UNET_WALK[k])[0]  # noqa: E731
    small, large = _conv_plan(*first(0), first(0)[3]), _conv_plan(*first(1), first(1)[3])
    assert small[1] == HCONV and large[1] == WCONV, (small, large)
    # the threshold as the plan sees it: every 128 x 128 step is on the Winograd kernel (at batch 1 too), no other step is
    for k, (B, H, W) in enumerate(lc.UNET_WALK):
        assert (_conv_plan(*first(k), first(k)[3])[1] == WCONV) == ((H, W) == (128, 128)), k
    # ... and the lower levels of those steps stay below it: their Winograd copies are never packed, only the first level's are, mid-life
    assert all(_conv_plan(*lv, lv[3])[1] != WCONV for k in (1, 4) for lv in _levels(lc.UNET_CASE, *lc.UNET_WALK[k])[1:])
    assert lc.UNET_WALK_F32 == lc.UNET_WALK[:3] and lc.CFG64_WALK[1][0] > lc.CFG64_WALK[0][0] == lc.CFG64_WALK[2][0]


def test_the_non_square_steps_reach_the_kernels_they_name():
    # 32 x 48: its first level runs non-square on the halo
    # kernel, its 16 x 24 and 8 x 12 levels on the implicit GEMM with deferred split-K slices — the halo kernels need W to be a multiple of 16
    lv = _levels(lc.UNET_CASE, *lc.UNET_WALK[3])
    assert lc.UNET_WALK[3] == (2, 32, 48)
    assert _conv_plan(*lv[0], lv[0][3])[1] == HCONV
    for l in lv[1:]:
        kernel, tile, splitk = _conv_plan(*l, l[3])
        assert kernel == 0 and splitk > 1, (l, kernel, tile, splitk)
    # 32 x 64: the 16 x 32 and 8 x 16 levels select the weight-streaming kernel on non-square maps
    lv = _levels(lc.UNET_CASE, *lc.UNET_WALK[6])
    assert all(l[1] != l[2] for l in lv)
    assert [_conv_plan(*l, l[3])[1] for l in lv] == [HCONV, KCONV, KCONV]


def test_grow_steps_grow_every_buffer_and_shrink_steps_shrink():
    counts = [lc.unet_buffer_counts(lc.UNET_CASE, *s) for s in lc.UNET_WALK]
    for k, c in enumerate(counts):
        if k == 0:
            continue
        peak = {name: max(p[name] for p in counts[:k]) for name in c}
        if k in lc.UNET_WALK_GROWS:
            assert all(c[n] > peak[n] for n in c), (k, c, peak)
        elif k in lc.UNET_WALK_SHRINKS:
            assert all(c[n] <= peak[n] for n in c) and all(c[n] < peak[n] for n in c if n != "embedding head"), (k, c, peak)
        else:
            assert c == peak, (k, c, peak)  # an "equal" step: exactly the largest shape seen
    assert 1 in lc.UNET_WALK_GROWS and {2, 3, 4} <= set(lc.UNET_WALK_SHRINKS)
    # the warm passes never exceed the walk's largest shape, alternate smaller / equal, and the "larger" call exceeds it
    peak = {n: max(c[n] for c in counts) for n in counts[0]}
    warm = [lc.unet_buffer_counts(lc.UNET_CASE, *s) for s in lc.UNET_WARM]
    assert len(warm) == 8 and all(all(w[n] <= peak[n] for n in w) for w in warm)
    assert [w == peak for w in warm] == [False, True] * 4
    assert all(s in lc.UNET_WALK for s in lc.UNET_WARM)
    big = lc.unet_buffer_counts(lc.UNET_CASE, *lc.UNET_LARGER)
    assert all(big[n] >= peak[n] for n in big) and big["level 0 activations"] > peak["level 0 activations"]
    # towers: the second step is the largest of each walk, the last one smaller; the ViT walk uses both layouts
    ns = [n for n, _ in lc.VIT_WALK]
    assert ns[1] == max(ns) > ns[0] > ns[2] and {lay for _, lay in lc.VIT_WALK} == {0, 1} and lc.VIT_LARGER[0] > max(ns)
    assert len(lc.VIT_WARM) == 8 and all(n <= max(ns) for n, _ in lc.VIT_WARM) and [n == max(ns) for n, _ in lc.VIT_WARM] == [False, True] * 4
    for w in (lc.TEXT_WALK, lc.RN_WALK):
        assert w[1] == max(w) and w[2] < w[1] and w[0] < w[1]
    vol = [b * h * w for b, h, w in lc.LPIPS_WALK]
    assert lc.LPIPS_WALK[0] == lc.LPIPS_WALK[2] and vol[1] > vol[0] and lc.LPIPS_WALK[1][0] < lc.LPIPS_WALK[0][0]
    assert all(s1 != s2 for s1, s2 in lc.SEEDS.values())


def _fake_ctx():
    rec = _RecordingLib()
    return types.SimpleNamespace(lib=rec, h=None, check=lambda rc: None, stream=lambda: 0, _nets=set(), device=0), rec


def _last(rec, name):
    return [a for n, a in rec.calls if n == name][-1]


def test_the_wrappers_pass_the_current_batch_and_shape_on_every_call():
    """Fails if a wrapper caches B, H, W, N or an output tensor from an earlier call."""
    ctx, rec = _fake_ctx()
    unet = nets.UNet(ctx, **pc.UNET_CASES[lc.UNET_CASE])
    outs = []
    for (B, H, W) in lc.UNET_WALK:
        x, t, y = th.zeros(B, 3, H, W), th.zeros(B), th.zeros(B, dtype=th.int64)
        out = unet.forward(x, t, y)
        a = _last(rec, "cgd_unet_forward")
        assert a[5:8] == (B, H, W) and tuple(out.shape) == (B, 6, H, W) and a[4] == out.data_ptr() and a[1] == x.data_ptr()
        assert all(out is not o for o in outs)
        outs.append(out)
        gout = th.zeros(B, 6, H, W)
        gx = unet.dgrad(gout)
        a = _last(rec, "cgd_unet_dgrad")
        assert tuple(gx.shape) == (B, 3, H, W) and a[1:3] == (gout.data_ptr(), gx.data_ptr())
        unet.embed(t, y, B & 1)
        assert _last(rec, "cgd_unet_embed")[3:5] == (B, B & 1)
        out = unet.forward_slot(x, B & 1)
        a = _last(rec, "cgd_unet_forward_slot")
        assert a[2] == (B & 1) and a[4:7] == (B, H, W) and tuple(out.shape) == (B, 6, H, W)
    vit = nets.ClipImageTower(ctx, lc.VIT_NAME)
    for (N, lay) in lc.VIT_WALK:
        img = th.zeros(N, 3, 224, 224) if lay == 0 else th.zeros(N * 49, 3072)
        emb = vit.encode_image(img, layout=lay, n=N if lay else None)
        a = _last(rec, "cgd_vit_forward")
        assert a[1:4] == (img.data_ptr(), lay, N) and tuple(emb.shape) == (N, 512) and a[4] == emb.data_ptr()
        d = vit.dgrad(th.zeros(N, 512))
        assert tuple(d.shape) == tuple(img.shape) and _last(rec, "cgd_vit_dgrad")[2] == d.data_ptr()
    # (ClipTextTower.encode_text places the ids on the context's GPU itself: its N is covered by the GPU tier only)
    rn = nets.ClipResNetTower(ctx, "tiny", lc.RN_CFG)
    for N in lc.RN_WALK:
        img = th.zeros(N, 3, 64, 64)
        emb = rn.encode_image(img)
        assert _last(rec, "cgd_rn_forward")[2] == N and tuple(emb.shape) == (N, 128)
        assert tuple(rn.dgrad(th.zeros(N, 128)).shape) == (N, 3, 64, 64)
    lp = nets.LpipsVGG(ctx)
    for (B, H, W) in lc.LPIPS_WALK:
        lp.set_reference(th.zeros(B, 3, H, W))
        assert _last(rec, "cgd_lpips_set_reference")[2:5] == (B, H, W)
        loss, gx = lp.loss_grad(th.zeros(B, 3, H, W))
        assert tuple(loss.shape) == (B,) and tuple(gx.shape) == (B, 3, H, W)
    # an x of another shape than the current reference never reaches the library
    n = len(rec.calls)
    try:
        lp.loss_grad(th.zeros(1, 3, 96, 128))
        raised = False
    except AssertionError:
        raised = True
    assert raised and len(rec.calls) == n


def test_classic_walk_grows_shrinks_and_repeats_every_resampling_buffer():
    """CLASSIC_WALK B1 64^2 -> B2 128^2 -> B1 64^2 -> B2 32x64 -> B1 128^2 -> B2 128^2 over Downsample::out / dx and Upsample::out / d1 / dx: step 1
    grows every buffer, steps 2 - 4 run on buffers that are too large, step 5 is exactly the largest shape seen; frames are multiples of 32 (five
    Downsamples), 32 x 64 ends on a 1 x 2 map; the warm passes stay within the peak and end on it"""
    assert lc.CLASSIC_WALK == [(1, 64, 64), (2, 128, 128), (1, 64, 64), (2, 32, 64), (1, 128, 128), (2, 128, 128)]
    counts = [lc.classic_resample_counts(lc.CLASSIC_CASE, *s) for s in lc.CLASSIC_WALK]
    assert len(counts[0]) == 25 and all(v > 0 for c in counts for v in c.values())
    for k in range(1, len(counts)):
        c = counts[k]
        peak = {n: max(p[n] for p in counts[:k]) for n in c}
        if k == 1:
            assert all(c[n] > peak[n] for n in c)
        elif k == 5:
            assert c == peak
        else:
            assert all(c[n] < peak[n] for n in c)
    assert all(H % 32 == 0 and W % 32 == 0 for _, H, W in lc.CLASSIC_WALK) and (32 >> 5, 64 >> 5) == (1, 2)
    peak = {n: max(c[n] for c in counts) for n in counts[0]}
    warm = [lc.classic_resample_counts(lc.CLASSIC_CASE, *s) for s in lc.CLASSIC_WARM]
    assert all(s in lc.CLASSIC_WALK for s in lc.CLASSIC_WARM) and all(w[n] <= peak[n] for w in warm for n in w) and warm[2] == peak
    kw = lc.pc.UNET_CASES[lc.CLASSIC_CASE]
    from tests import classic_unet_ref as R
    assert {k: kw[k] for k in R.NARROW} == R.NARROW and (kw["resblock_updown"], kw["use_scale_shift_norm"]) == (False, False)
