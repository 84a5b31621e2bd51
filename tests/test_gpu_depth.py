"""The whole depth network (nets.DepthNet, csrc/depth.hip) against tests/depth_ref.py on the same synthetic weights, at the project's literal
|a - b| <= 1e-4 + 1e-3 |ref| on inv_depth, on the four reassembled maps and on the final depth."""
import functools

import pytest
import torch as th

from tests import depth_ref as R
from tests import parity_checks as pc
from tests.parity_checks import DEV, g, rec

pytestmark = pytest.mark.gpu

CONFIGS = {
    # tap 4 of a 2 x 2 grid is a 1 x 1 map: the first upsample is the degenerate case
    "tiny": dict(patch=16, width=128, layers=4, heads=2, hooks=(0, 1, 2, 3), native_grid=2, features=32, reassemble_channels=(32, 64, 128, 128)),
    # the channel counts of the published file on a map small enough for a CPU reference in seconds
    "wide": dict(patch=16, width=1024, layers=4, heads=16, hooks=(0, 1, 2, 3), native_grid=24, features=256, reassemble_channels=(256, 512, 1024, 1024)),
}
OFFSET, SCALE, FLOOR = 3.0, 2.0, 0.05  # with synthetic weights inv_depth is O(1): constants that put the mapping and its floor inside its range


@functools.lru_cache(maxsize=None)
def _ctx():
    return pc._ctx(1)


@functools.lru_cache(maxsize=None)
def _weights(name):
    from cgd_amd import synthetic
    return synthetic.depth_state_dict(CONFIGS[name], seed=11)


@functools.lru_cache(maxsize=None)
def _net(name, size=384):
    from cgd_amd import nets
    return nets.DepthNet(_ctx(), CONFIGS[name], size=size, offset=OFFSET, scale=SCALE, floor=FLOOR).load_state_dict(_weights(name))


@functools.lru_cache(maxsize=None)
def _case(name, B, h, w):
    """(img, reference inv_depth, reference taps), computed once"""
    img = th.randn(B, 3, h, w, generator=g(h + w)).clamp(-1, 1)
    with th.no_grad():
        inv, taps = R.forward(CONFIGS[name], _weights(name), img)
    return img, inv, taps


def _ok(records):
    for r in records:
        print(f"{r['name']}: abs {r['err_abs']:.3e} peak {r['ref_max']:.3e} ok {r['ok']}")
    bad = [r for r in records if not r["ok"]]
    assert not bad, bad[0]


@pytest.mark.parametrize("name,B,h,w", [("tiny", 1, 32, 32), ("tiny", 2, 64, 96), ("wide", 1, 64, 64)])
def test_forward_matches_the_reference(name, B, h, w):
    img, inv_ref, taps_ref = _case(name, B, h, w)
    net = _net(name)
    inv, dep = net.forward(img.to(DEV), want="both")
    recs = [rec(f"{name} {h}x{w} inv_depth", inv, inv_ref), rec(f"{name} {h}x{w} depth", dep, R.depth_map(inv_ref, OFFSET, SCALE, FLOOR))]
    for k in range(4):
        recs.append(rec(f"{name} {h}x{w} reassembled map {k + 1}", net.debug_map(k), taps_ref[k]))
    assert inv.shape == (B, 1, h, w) and bool((inv_ref > 0).any())
    worst = ((inv.cpu().double() - inv_ref.double()).abs() / (1e-4 + 1e-3 * inv_ref.double().abs())).max()
    print(f"{name} {h}x{w} inv_depth: largest |a - b| / (1e-4 + 1e-3 |ref|) = {float(worst):.3f}")
    _ok(recs)


def test_sizes_alternate_on_one_handle_bit_identically():
    net = _net("tiny")
    a = _case("tiny", 1, 32, 32)[0].to(DEV)
    b = _case("tiny", 2, 64, 96)[0].to(DEV)
    first = net.forward(a).clone()
    other = net.forward(b).clone()
    again = net.forward(a).clone()
    assert th.equal(first, again) and th.equal(other, net.forward(b))


def test_refusals_come_before_any_launch():
    import ctypes as C

    from cgd_amd.lib import CgdError
    net, ctx = _net("tiny"), _ctx()
    th.cuda.synchronize()
    counts = (C.c_uint64 * 2)()
    ctx.lib.cgd_launch_counts(counts)
    before = counts[0]
    inv = th.empty(1, 1, 48, 64, device=DEV)
    with pytest.raises(CgdError, match="multiples of 32"):
        ctx.check(ctx.lib.cgd_depth_forward(net.h, th.zeros(1, 3, 48, 64, device=DEV).data_ptr(), 1, 48, 64, 1.0, 1.0, 0.1, inv.data_ptr(), None, ctx.stream()))
    with pytest.raises(CgdError, match="no position embedding"):  # a grid nobody uploaded
        ctx.check(ctx.lib.cgd_depth_forward(net.h, th.zeros(1, 3, 32, 160, device=DEV).data_ptr(), 1, 32, 160, 1.0, 1.0, 0.1, inv.data_ptr(), None, ctx.stream()))
    with pytest.raises(CgdError, match="inv_depth or depth"):
        ctx.check(ctx.lib.cgd_depth_forward(net.h, th.zeros(1, 3, 32, 32, device=DEV).data_ptr(), 1, 32, 32, 1.0, 1.0, 0.1, None, None, ctx.stream()))
    ctx.lib.cgd_launch_counts(counts)
    assert counts[0] == before


def test_call_resizes_maps_and_resizes_back():
    net = _net("tiny", 64)
    B, H, W = 2, 48, 80
    frame = th.rand(B, 3, H, W, generator=g(5))
    with th.no_grad():
        ref = R.frame_to_depth(CONFIGS["tiny"], _weights("tiny"), frame, size=64, offset=OFFSET, scale=SCALE, floor=FLOOR)
    got = net(frame.to(DEV))
    assert got.shape == (B, 1, H, W) and got.dtype == th.float32
    assert bool(th.isfinite(got).all()) and float(got.min()) >= FLOOR
    _ok([rec("DepthNet.__call__ 48x80 at size 64", got, ref)])
