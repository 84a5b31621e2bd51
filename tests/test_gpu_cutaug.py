"""Native `use_augs` cutouts (csrc/cutaug.hip) on the GPU: forward and adjoint against the torch restatement (same parameter and
noise draws by seed), the adjoint identity, bit-reproducible backward, the single-tower ClipGuidance CLIP leg against _clip_leg_torch,
and MakeCutouts(use_augs=True) as an autograd node.

Criterion `nearest-ties`: |a - b| <= 1e-4 + 1e-3 |ref| except for at most 1e-4 of the elements.  GPU torch divides the grid by a
scalar through its reciprocal while the kernels divide (as the CPU oracle does), so a nearest pick that sits on an exact half-pixel
tie can land on the neighbouring pixel; the count of such elements is reported."""
import pytest
import torch as th

import cgd_amd  # noqa: F401
from cgd_amd import guidance as dg

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ctx():
    from cgd_amd import lib
    return lib.Context(0, 1)


@pytest.fixture
def noise_std(monkeypatch):
    def set_std(v):
        monkeypatch.setattr(dg, "AUG_NOISE_STD", v)
    return set_std


def close_with_ties(name, got, ref):
    bad = ((got - ref).abs() > 1e-4 + 1e-3 * ref.abs())
    n = int(bad.sum())
    print(f"{name}: nearest-ties {n} of {ref.numel()} elements, max |diff| {float((got - ref).abs().max()):.3e}")
    assert th.isfinite(got).all()
    assert n <= 1e-4 * ref.numel(), (name, n, ref.numel())


def to_patch_rows(img, P):
    N, C, cs, _ = img.shape
    g = cs // P
    return img.view(N, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N * g * g, C * P * P)


def setup(B, H, W, cutn, cs, seed):
    gen = th.Generator().manual_seed(seed)
    x = (th.rand(B, 3, H, W, generator=gen) * 2 - 1).to(DEV)
    th.manual_seed(seed)
    coords = dg.generate_coords(H, W, cutn, cs, 1.0)
    return x, coords


def native_fwd(ctx, x, coords, cs, layout, patch, seed):
    B, _, H, W = x.shape
    th.manual_seed(seed)
    th.cuda.manual_seed(seed)
    aug = dg._AugLaunch(ctx.lib, coords, B, H, W, x.device)
    N = len(coords) * B
    out = th.empty((N * (cs // patch) ** 2, 3 * patch * patch) if layout else (N, 3, cs, cs), device=DEV)
    aug.forward(ctx, x, out, cs, layout, patch)
    return aug, out


def torch_fwd(x, coords, cs, seed, requires_grad=False):
    th.manual_seed(seed)
    th.cuda.manual_seed(seed)
    xr = x.detach().clone().requires_grad_(requires_grad)
    mk = dg.MakeCutouts(cs, len(coords), use_augs=True)
    mean = th.tensor(dg.CLIP_MEAN, device=DEV).view(1, 3, 1, 1)
    std = th.tensor(dg.CLIP_STD, device=DEV).view(1, 3, 1, 1)
    return xr, (mk.augmented(xr.add(1).div(2), coords) - mean) / std


@pytest.mark.parametrize("std", [0.0, 0.01])
@pytest.mark.parametrize("B,H,W,cutn,cs,layout,patch", [(1, 96, 96, 12, 64, 0, 0), (2, 80, 112, 9, 64, 1, 16),
                                                         (2, 128, 96, 16, 32, 1, 8), (1, 64, 64, 7, 96, 0, 0)])
def test_forward_matches_torch(ctx, noise_std, std, B, H, W, cutn, cs, layout, patch):
    noise_std(std)
    x, coords = setup(B, H, W, cutn, cs, 100 + cutn)
    _, got = native_fwd(ctx, x, coords, cs, layout, patch, 7)
    _, ref = torch_fwd(x, coords, cs, 7)
    ref = to_patch_rows(ref, patch) if layout else ref
    close_with_ties(f"fwd B{B} {H}x{W} cutn{cutn} cs{cs} layout{layout} std{std}", got, ref)


def test_forward_with_num_cutouts_override_and_truncated_crops(ctx, noise_std):
    noise_std(0.01)
    B, H, W, cs = 2, 72, 100, 48
    x, _ = setup(B, H, W, 1, cs, 5)
    mk = dg.MakeCutouts(cs, 20, ctx=ctx)
    th.manual_seed(9)
    coords = mk.draw(H, W, num_cutouts_override=6) + [(60, 50, 40), (0, 50, 30)]  # two boxes cut by the border
    assert any(h != w for _, _, h, w in dg.crop_geometry(coords, H, W))
    _, got = native_fwd(ctx, x, coords, cs, 0, 0, 3)
    _, ref = torch_fwd(x, coords, cs, 3)
    close_with_ties("fwd override + truncated", got, ref)


def test_adjoint_identity(ctx, noise_std):
    noise_std(0.0)
    B, H, W, cutn, cs = 2, 96, 80, 10, 64
    x, coords = setup(B, H, W, cutn, cs, 31)
    aug, fx = native_fwd(ctx, x, coords, cs, 1, 16, 4)
    f0 = th.empty_like(fx)
    aug.forward(ctx, th.zeros_like(x), f0, cs, 1, 16)
    y = th.randn(fx.shape, generator=th.Generator(device=DEV).manual_seed(2), device=DEV)
    g = th.empty_like(x)
    aug.backward(ctx, y, g, cs, 1, 16, accumulate=False)
    lhs = float(((fx - f0).double() * y.double()).sum())
    rhs = float((x.double() * g.double()).sum())
    print(f"adjoint identity: {lhs:.9e} vs {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


@pytest.mark.parametrize("layout,patch", [(0, 0), (1, 16)])
def test_backward_matches_autograd_and_is_deterministic(ctx, noise_std, layout, patch):
    noise_std(0.01)
    B, H, W, cutn, cs = 2, 96, 112, 12, 64
    x, coords = setup(B, H, W, cutn, cs, 57)
    aug, out = native_fwd(ctx, x, coords, cs, layout, patch, 8)
    xr, ref = torch_fwd(x, coords, cs, 8, requires_grad=True)
    y = th.randn(ref.shape, generator=th.Generator(device=DEV).manual_seed(5), device=DEV)
    want, = th.autograd.grad((ref * y).sum(), xr)
    dy = to_patch_rows(y, patch).contiguous() if layout else y
    g1 = th.full_like(x, 0.25)
    aug.backward(ctx, dy, g1, cs, layout, patch, accumulate=True)
    g2 = th.empty_like(x)
    aug.backward(ctx, dy, g2, cs, layout, patch, accumulate=False)
    g3 = th.empty_like(x)
    aug.backward(ctx, dy, g3, cs, layout, patch, accumulate=False)
    assert th.equal(g2, g3)
    assert th.equal(g1, g2 + 0.25) or (g1 - g2 - 0.25).abs().max() < 1e-6
    close_with_ties(f"bwd layout{layout}", g2, want)


def _guidance(ctx, names, cutn):
    from cgd_amd import nets, synthetic
    towers, targets = [], []
    for k, name in enumerate(names):
        if name in nets.VIT_CONFIGS:
            t = nets.ClipImageTower(ctx, name)
            t.load_state_dict(synthetic.synthetic_state_dict(t, seed=4321))
        else:
            t = nets.ClipResNetTower(ctx, name)
            t.load_state_dict(synthetic.resnet_state_dict(t, seed=2468))
        towers.append(t)
        targets.append(th.randn(2, t.out_dim, generator=th.Generator(device=DEV).manual_seed(11 + k), device=DEV))
    return dg.ClipGuidance(ctx, None, towers, None, targets, [1.0, 0.5], cutn)


@pytest.mark.parametrize("names", [("ViT-B/32",), ("RN50",)])
def test_clip_leg_matches_the_torch_leg(ctx, noise_std, names):
    """ClipGuidance's use_augs CLIP leg, native against _clip_leg_torch with the same seed and the noise on: d(CLIP loss)/dx_in
    (accumulated onto a non-zero gclip), the CLIP loss and the tower's embeddings."""
    noise_std(0.01)
    cutn, B, H, W = 16, 1, 256, 256
    guid = _guidance(ctx, names, cutn)
    x_in = th.tanh(th.randn(B, 3, H, W, generator=th.Generator(device=DEV).manual_seed(3), device=DEV))
    th.manual_seed(1)
    coords = dg.generate_coords(H, W, cutn, 224, 1.0)
    wm = dg.prompt_weight_matrix(th.tensor([1.0, 0.5]), B, DEV)
    res = {}
    for leg in ("native", "torch"):
        gclip = th.full((B, 3, H, W), 0.5, device=DEV)  # accumulate=1: added to what is there (the LPIPS leg's gradient)
        part = th.empty(len(names) * cutn * B, device=DEV)
        th.manual_seed(77)
        th.cuda.manual_seed(77)
        fn = guid._clip_leg if leg == "native" else guid._clip_leg_torch
        fn(x_in, dg._AugCuts(ctx.lib, coords, B, H, W, x_in.device), wm, None, gclip, part, 1)
        th.cuda.synchronize()
        res[leg] = (gclip - 0.5, float(part.double().sum()), guid.emb.clone())
    (g_n, l_n, e_n), (g_t, l_t, e_t) = res["native"], res["torch"]
    print(f"{names}: CLIP loss native {l_n:.6f} torch {l_t:.6f}; |g| peak {float(g_t.abs().max()):.3e}")
    assert abs(l_n - l_t) <= 1e-4 + 1e-3 * abs(l_t)
    close_with_ties("emb", e_n, e_t)
    err = (g_n - g_t).abs()
    print(f"g_clip_in: max err {float(err.max()):.3e}, rel-to-peak {float(err.max() / g_t.abs().max()):.3e}")
    close_with_ties("g_clip_in", g_n, g_t)


def test_make_cutouts_use_augs_on_the_gpu(ctx, noise_std):
    noise_std(0.01)
    B, H, W, cs, cutn = 2, 64, 80, 32, 5
    x = th.rand(B, 3, H, W, generator=th.Generator().manual_seed(4)).to(DEV)
    outs = []
    for native in (True, False):
        th.manual_seed(6)
        th.cuda.manual_seed(6)
        mk = dg.MakeCutouts(cs, cutn, use_augs=True, ctx=ctx)
        xr = x.clone().requires_grad_()
        out = mk(xr) if native else mk.augmented(xr, mk.draw(H, W))
        assert out.shape == (cutn * B, 3, cs, cs) and out.requires_grad
        w = th.linspace(-1, 1, out.numel(), device=DEV).view_as(out)
        g, = th.autograd.grad((out * w).sum(), xr)
        outs.append((out.detach(), g))
    close_with_ties("MakeCutouts fwd", outs[0][0], outs[1][0])
    close_with_ties("MakeCutouts bwd", outs[0][1], outs[1][1])
    with th.no_grad():
        th.manual_seed(6)
        th.cuda.manual_seed(6)
        plain = dg.MakeCutouts(cs, cutn, use_augs=True, ctx=ctx)(x)
    assert th.equal(plain, outs[0][0])


def test_dual_tower_clip_leg_against_the_cpu_oracle(noise_std):
    """RN50 + ViT-B/32 (BASELINE config 5's dual-tower mode) with use_augs: the native leg's d(CLIP loss)/dx_in, CLIP loss and first-tower
    embeddings against the CPU oracle towers running the torch restatement (noise off, one seed, draws in tower order).  The CPU is the
    judge here rather than _clip_leg_torch on the GPU: GPU torch scales the sampling grid by a reciprocal, so a few nearest
    picks per hundred thousand land on the neighbouring pixel, and through two random-weight towers that moves g well beyond rounding
    (reported below, not graded).  The kernels reproduce the CPU's picks exactly (tests/test_cutaug_host.py)."""
    import torch.nn.functional as F
    from cgd_amd import lib, nets
    from oracle import clip_resnet as ocr
    from oracle import clip_vit as ocv
    noise_std(0.0)
    ctx32 = lib.Context(0, 0)  # fp32 products: the comparison is against fp32 CPU towers
    o_rn = ocr.synthetic_init_(ocr.ClipResNetImageModel(config=ocr.RN_CONFIGS["RN50"])).eval().float()
    o_vit = ocv.synthetic_init_(ocv.ClipImageModel("ViT-B/32")).eval().float()
    towers = []
    for o, t in ((o_rn, nets.ClipResNetTower(ctx32, "RN50")), (o_vit, nets.ClipImageTower(ctx32, "ViT-B/32"))):
        for p in o.parameters():
            p.requires_grad_(False)
        t.load_clip_state_dict({k: v.to(DEV) for k, v in o.state_dict().items() if "num_batches_tracked" not in k})
        towers.append(t)
    cutn, B, H, W = 6, 1, 256, 256
    gen = th.Generator().manual_seed(12)
    targets = [th.randn(2, t.out_dim, generator=gen) for t in towers]
    guid = dg.ClipGuidance(ctx32, None, towers, None, [t.to(DEV) for t in targets], [1.0, 0.5], cutn)
    x_cpu = th.tanh(th.randn(B, 3, H, W, generator=gen))
    x_in = x_cpu.to(DEV)
    th.manual_seed(1)
    coords = dg.generate_coords(H, W, cutn, 224, 1.0)
    wm = dg.prompt_weight_matrix(th.tensor([1.0, 0.5]), B, DEV)

    def device_leg(fn):
        gclip = th.zeros((B, 3, H, W), device=DEV)
        part = th.zeros(2 * cutn * B, device=DEV)
        th.manual_seed(77)
        fn(x_in, dg._AugCuts(ctx32.lib, coords, B, H, W, x_in.device), wm, None, gclip, part, 0)
        th.cuda.synchronize()
        return gclip.cpu(), float(part.double().sum()), guid.emb.cpu().clone()

    g_n, l_n, e_n = device_leg(guid._clip_leg)
    g_t, l_t, _ = device_leg(guid._clip_leg_torch)
    # the oracle: the reference recipe (cgd.py:190-204) on the CPU, towers in order, parameters from the same CPU seed
    mean = th.tensor(dg.CLIP_MEAN).view(1, 3, 1, 1)
    std = th.tensor(dg.CLIP_STD).view(1, 3, 1, 1)
    th.manual_seed(77)
    xr = x_cpu.clone().requires_grad_()
    total, e_o = 0, None
    for model, tgt in zip((o_rn, o_vit), targets):
        cut = dg.MakeCutouts(224, cutn, use_augs=True).augmented(xr.add(1).div(2), coords)
        emb = model.encode_image((cut - mean) / std).float().view(cutn, B, 1, -1)
        e_o = emb.detach().view(cutn * B, -1) if e_o is None else e_o
        tn = F.normalize(tgt, dim=-1)
        d = (F.normalize(emb, dim=-1) - tn.view(1, 1, -1, tn.shape[-1])).norm(dim=-1).div(2).arcsin().pow(2).mul(2)
        total = total + (d * wm.cpu().view(1, B, -1)).sum(2).mean(0).sum() * guid.cgs
    g_o, = th.autograd.grad(total, xr)
    l_o = float(total)
    peak = float(g_o.abs().max())
    print(f"CLIP loss native {l_n:.6f} torch-on-GPU {l_t:.6f} oracle {l_o:.6f}; g peak {peak:.3e}")
    print(f"g_clip_in max |native - oracle| {float((g_n - g_o).abs().max()):.3e}, "
          f"max |torch-on-GPU - oracle| {float((g_t - g_o).abs().max()):.3e}")
    assert abs(l_n - l_o) <= 1e-4 + 1e-3 * abs(l_o)
    close_with_ties("emb vs oracle", e_n, e_o)
    close_with_ties("g_clip_in vs oracle", g_n, g_o)
