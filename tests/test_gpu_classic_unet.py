"""The classic UNet architecture on the device (cgd_unet_config::classic_resample / additive_emb; nets.UNet(resblock_updown=False,
use_scale_shift_norm=False)) against tests/classic_unet_ref.py on the CPU: fp32 forward, autograd for the input gradient.

Net: image 32 x 32, model_channels 64, one res block, channel_mult (1, 2), attention at the 16 x 16 level with num_heads = 1 (head dim 128),
seeded weights, all four combinations of the two switches at batch 1 and 2.  Bound: that of the existing whole-network tests
(parity_checks.check_unet, test_gpu_superres.py, test_gpu_classifier.py): |a - b| <= 1e-4 + 1e-3 |ref| for every element of the output and of
the input gradient, the gradient's seed scaled so that the reference gradient has unit peak."""
import copy
import ctypes as C
import functools

import pytest
import torch as th

from tests import classic_unet_ref as R
from tests import parity_checks as pc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def context(precision):
    return pc._ctx(precision)


@functools.lru_cache(maxsize=None)
def reference(updown, film, seed=1234):
    ref = R.synthetic_init_(R.ClassicUNetModel(**R.TINY, resblock_updown=updown, use_scale_shift_norm=film), seed=seed).eval()
    for p in ref.parameters():
        p.requires_grad_(False)
    return ref


@functools.lru_cache(maxsize=None)
def device_net(updown, film, precision=1):
    from cgd_amd import nets
    dev = nets.UNet(context(precision), **R.TINY, resblock_updown=updown, use_scale_shift_norm=film)
    return dev.load_state_dict(pc.device_sd(reference(updown, film)))


@functools.lru_cache(maxsize=None)
def scenario(updown, film, B, H, W, timestep=417.0):
    """inputs and the CPU reference's output and unit-peak input gradient, computed once and shared"""
    x = th.randn(B, 3, H, W, generator=pc.g(60))
    t = th.tensor([float(timestep) + 100.0 * b for b in range(B)])
    gout = th.randn(B, 6, H, W, generator=pc.g(62))
    gout[:, 3:] = 0  # the guidance only seeds the epsilon channels
    xr = x.clone().requires_grad_()
    o = reference(updown, film)(xr, t)
    (o * gout).sum().backward()
    sd = pc.unit_seed(xr.grad)
    return dict(x=x, t=t, gout=gout * sd, out=o.detach(), grad=xr.grad * sd)


def run(dev, s):
    od = dev.forward(s["x"].to(pc.DEV), s["t"].to(pc.DEV)).clone()
    gx = dev.dgrad(s["gout"].to(pc.DEV)).clone()
    th.cuda.synchronize()
    return od, gx


def grade(tag, od, gx, s):
    recs = [pc.rec(f"{tag} forward", od, s["out"]), pc.rec(f"{tag} dgrad", gx, s["grad"])]
    for r in recs:
        print(f"{r['name']}: abs {r['err_abs']:.3e} rel-to-peak {r['err_rel']:.3e} peak {r['ref_max']:.3f} [{r['criterion']}]")
    for r in recs:
        assert r["ok"], r


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("updown,film", R.FLAG_COMBOS)
def test_forward_and_dgrad_match_the_reference(updown, film, B):
    s = scenario(updown, film, B, 32, 32)
    od, gx = run(device_net(updown, film), s)
    grade(f"classic unet[updown={updown} film={film} B{B} 32x32]", od, gx, s)


def _plan(B, S, ci, co, precision=1):
    o = (C.c_int * 5)()
    assert context(1).lib.cgd_op_plan_conv(B, S, S, ci, co, precision, 256, 0, 1, 0, o) == 0  # (256 CUs: the MI355X)
    return list(o)


def _conv1_shapes(frame):
    """(side, Cin, Cout) of every ResBlock conv1 of the tiny classic net at a square frame"""
    h = frame // 2
    return [(frame, 64, 64), (h, 64, 128), (h, 128, 128), (h, 256, 128), (h, 192, 128), (frame, 192, 64), (frame, 128, 64)]


def _smallest_frame(pred):
    for frame in (4, 8, 16, 32, 64, 128):
        hits = [(S, ci, co, _plan(1, S, ci, co)) for (S, ci, co) in _conv1_shapes(frame) if pred(_plan(1, S, ci, co))]
        if hits:
            return frame, hits
    return None, []


def test_additive_embedding_where_conv1_would_split_k():
    """GN2 of an additive block normalises conv1's output PLUS the embedding.  A conv1 that splits K would hand its slices to the norm, which
    would sum them into statistics of the tensor BEFORE the addition; additive blocks therefore switch the deferral off and add with one small
    kernel.  The smallest frame at which a conv1 of the net plans a split (cgd_op_plan_conv), whole-network output and gradient: wrong group
    statistics in any block are O(1) errors in both."""
    frame, hits = _smallest_frame(lambda o: o[2] > 1)
    assert frame is not None, "no conv1 of the tiny net plans a split-K launch at any frame up to 128: the case is not reached"
    print(f"frame {frame}: split-K conv1 launches {hits}")
    s = scenario(False, False, 2, frame, frame)
    od, gx = run(device_net(False, False), s)
    grade(f"classic unet[additive, conv resampling, B2 {frame}x{frame}: split-K conv1]", od, gx, s)


def test_additive_embedding_where_conv1_would_leave_groupnorm_records():
    """the same for the conv kernels whose epilogue leaves GroupNorm statistics of their output (wconv_kernel, tile code 515; the unsplit
    hconv2 tile of 64 pixels): taken before the addition they would be those of the wrong tensor.  The smallest frame at which a conv1 of the
    net is planned onto such a kernel; the FiLM flavour of the same net at that frame does merge records (the counter moves), the additive one
    matches the reference"""
    frame, hits = _smallest_frame(lambda o: o[0] == 1 and (o[1] == 515 or (o[1] == 512 and o[4] == 64)))
    assert frame is not None, "no conv1 of the tiny net is planned onto a record-taking kernel at any frame up to 128: the case is not reached"
    print(f"frame {frame}: record-taking conv1 launches {hits}")
    film = device_net(False, True)
    ctx = film.ctx
    merges = lambda: int(ctx.lib.cgd_op_gn_record_merges(ctx.h))  # noqa: E731
    m0 = merges()
    film.forward(scenario(False, True, 1, frame, frame)["x"].to(pc.DEV), scenario(False, True, 1, frame, frame)["t"].to(pc.DEV))
    th.cuda.synchronize()
    assert merges() > m0, "the FiLM flavour merged no epilogue records at this frame: the shape does not exercise them"
    s = scenario(False, False, 1, frame, frame)
    od, gx = run(device_net(False, False), s)
    grade(f"classic unet[additive, conv resampling, B1 {frame}x{frame}: record-taking conv1]", od, gx, s)
    od_f, gx_f = run(film, scenario(False, True, 1, frame, frame))
    grade(f"classic unet[FiLM, conv resampling, B1 {frame}x{frame}]", od_f, gx_f, scenario(False, True, 1, frame, frame))


def test_exact_fp32_mode():
    """precision mode 0: every conv of this net splits K on the implicit GEMM there (cgd_op_plan_conv), the stride-2 conv runs its fp32 MFMA path"""
    s = scenario(False, False, 2, 32, 32)
    od, gx = run(device_net(False, False, 0), s)
    grade("classic unet[additive, conv resampling, p0 B2 32x32]", od, gx, s)


def test_gradient_belongs_to_the_last_forward():
    dev = device_net(False, False)
    a, b = scenario(False, False, 1, 32, 32, 417.0), scenario(False, False, 1, 32, 32, 33.0)
    dev.forward(a["x"].to(pc.DEV), a["t"].to(pc.DEV))
    od, gx = run(dev, b)
    grade("classic unet[forward(t=417), forward(t=33), dgrad]", od, gx, b)
    assert not pc.rec("the other forward's gradient", gx, a["grad"] * (b["gout"].abs().max() / a["gout"].abs().max()))["ok"]


def test_default_flags_are_the_published_architecture():
    """a net built without the two new arguments is the one built with them spelled out, bit for bit, and matches oracle/unet.py under the
    existing bound"""
    from cgd_amd import nets
    from oracle.unet import UNetModel
    ref = reference(True, True)
    plain = nets.UNet(context(1), **R.TINY).load_state_dict(pc.device_sd(ref))
    assert (plain.cfg.classic_resample, plain.cfg.additive_emb) == (0, 0)
    s = scenario(True, True, 2, 32, 32)
    od, gx = run(plain, s)
    od2, gx2 = run(device_net(True, True), s)
    assert th.equal(od.view(th.int32), od2.view(th.int32)) and th.equal(gx.view(th.int32), gx2.view(th.int32))
    orc = UNetModel(**R.TINY).eval()
    orc.load_state_dict(ref.state_dict())
    xr = s["x"].clone().requires_grad_()
    o = orc(xr, s["t"])
    (o * s["gout"]).sum().backward()
    for r in (pc.rec("default flags vs oracle/unet.py forward", od, o.detach()), pc.rec("default flags vs oracle/unet.py dgrad", gx, xr.grad)):
        assert r["ok"], r


@pytest.mark.parametrize("legacy", [1, 0])
def test_attention_at_head_dim_512(legacy):
    """num_heads = 1 at a 512-channel attention level: T = 16, d = 512, one head, both attention orders, on the generic path"""
    from tests import shape_edge_checks as se
    from cgd_amd import lib as L
    ctx = context(1)
    nb, heads, T, d = 1, 1, 16, 512
    qkv, dout, ref, dref = se.attn_data(nb, heads, T, d, legacy, 0)
    lib = ctx.lib
    bufs = [th.zeros(lib.cgd_op_attn_buf_floats(nb, heads, T, d, i), device=pc.DEV) for i in range(5)]
    arr = (C.c_void_p * 5)(*[t.data_ptr() for t in bufs])
    q, do = qkv.float().to(pc.DEV).contiguous(), dout.float().to(pc.DEV).contiguous()
    out, dq = th.full((nb * T, d), float("nan"), device=pc.DEV), th.full((nb * T, 3 * d), float("nan"), device=pc.DEV)
    ctx.check(lib.cgd_op_attn_fwd(ctx.h, q.data_ptr(), out.data_ptr(), nb, heads, T, d, legacy, arr, L.stream_ptr()))
    ctx.check(lib.cgd_op_attn_bwd(ctx.h, q.data_ptr(), do.data_ptr(), dq.data_ptr(), nb, heads, T, d, legacy, arr, L.stream_ptr()))
    th.cuda.synchronize()
    for r in (pc.rec(f"attention T16 d512 legacy{legacy} out", out, ref), pc.rec(f"attention T16 d512 legacy{legacy} dqkv", dq, dref)):
        print(f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3f}")
        assert r["ok"], r


# ---- the community structure as a network: six levels, five Downsamples / Upsamples (classic_unet_ref.NARROW, .COMICS), against FLOAT64 ----------
@functools.lru_cache(maxsize=None)
def wide_reference(case, film):
    ref = R.synthetic_init_(R.ClassicUNetModel(**R.CASES[case], resblock_updown=False, use_scale_shift_norm=film), seed=1234).eval()
    for p in ref.parameters():
        p.requires_grad_(False)
    return ref


@functools.lru_cache(maxsize=None)
def wide_net(case, film, precision):
    from cgd_amd import nets
    dev = nets.UNet(context(precision), **R.CASES[case], resblock_updown=False, use_scale_shift_norm=film)
    return dev.load_state_dict(pc.device_sd(wide_reference(case, film)))


@functools.lru_cache(maxsize=None)
def wide_scenario(case, film, B, H, W):
    """the float64 copy of the fp32 weights the device holds: output and unit-peak input gradient, once per scenario"""
    ref = copy.deepcopy(wide_reference(case, film)).double()
    x = th.randn(B, 3, H, W, generator=pc.g(60))
    t = th.tensor([417.0 + 100.0 * b for b in range(B)])
    gout = th.randn(B, 6, H, W, generator=pc.g(62))
    gout[:, 3:] = 0
    xr = x.double().requires_grad_()
    o = ref(xr, t.double())
    (o * gout.double()).sum().backward()
    sd = pc.unit_seed(xr.grad)
    return dict(x=x, t=t, gout=gout * sd, out=o.detach(), grad=xr.grad * sd)


# 32 x 32: the last Downsample makes a 1 x 1 map; 64 x 96: non-square, bottom map 2 x 3; 128 x 128: the Downsamples' forward runs 1 / 4 / 9 / 16 / 16
# slices at this width
NARROW_RUNS = [(False, 2, 32, 32, 1), (False, 2, 64, 96, 1), (False, 1, 128, 128, 1), (False, 2, 32, 32, 0), (False, 2, 64, 96, 0), (True, 2, 64, 96, 1)]


@pytest.mark.parametrize("film,B,H,W,precision", NARROW_RUNS, ids=[f"{'film' if f else 'additive'}-B{b}-{h}x{w}-p{p}" for f, b, h, w, p in NARROW_RUNS])
def test_community_structure_at_a_narrow_width_matches_float64(film, B, H, W, precision):
    s = wide_scenario("narrow", film, B, H, W)
    od, gx = run(wide_net("narrow", film, precision), s)
    grade(f"classic unet[narrow community structure, film={film} p{precision} B{B} {H}x{W}]", od, gx, s)


def test_community_flags_at_128x128_match_float64():
    """model_channels 128 as the checkpoints have it: d = 512 attention at T = 64 and two of the five Downsamples on split-K"""
    s = wide_scenario("comics", False, 1, 128, 128)
    od, gx = run(wide_net("comics", False, 1), s)
    grade("classic unet[community flags, p1 B1 128x128]", od, gx, s)
