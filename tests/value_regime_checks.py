"""Op kernels on the VALUE ranges of trained networks (tests/test_gpu_value_regimes.py, pytest -m gpu; tests/test_value_regimes_host.py, CPU).

The parity and strided-operand families draw every operand from the regime of a freshly initialised network: attention logits N(0, 1), GroupNorm /
LayerNorm inputs without outliers, |u| < 10 in front of the activations, random embeddings in the spherical loss.  This family keeps the shapes small
and moves the values: peaked and shifted softmaxes, outliers where a kernel takes its variance shift from, |mean| >> sigma, constant groups, the
range where __expf overflows, near-parallel / near-antipodal embeddings.  Every case goes through the C ABI, is compared with a float64 PyTorch
reference of the same operation and judged by `parity_checks.rec` at the literal |a-b| <= 1e-4 + 1e-3 |ref| (backward seeds scaled by `unit_seed`).

Admissibility (how extreme a case may be): a regime magnitude is the largest value of a short ladder for which, on the CPU, plain fp32 PyTorch of
the same op stays within 0.25 of that bound against float64 on every element and — for attention in a bf16x3 context — an emulation of the bf16x3
MFMA products (hi = bf16(v), lo = bf16(v - hi), lo*hi + hi*lo + hi*hi accumulated in float64, splitting exactly what attn_flash.hip splits:
alpha Q, K, the unnormalised P, V; dO, dS in the backward) stays within 1.0 of it.  The chosen magnitudes are the constants below;
test_value_regimes_host.py re-derives each of them from the ladder, asserts the fractions and asserts that each case IS in the regime it names.
"""
import contextlib
import functools
import math
import os

import torch as th
import torch.nn.functional as F

from tests import parity_checks as pc
from tests.parity_checks import ATOL, RTOL, g, rec, unit_seed

DEV = pc.DEV
GAIN_LADDER = (2, 4, 6, 8, 12, 16)
OUTLIER_LADDER = (30, 100, 300, 1000)
FP32_SHARE, EMU_SHARE = 0.25, 1.0

# chosen by the ladder rule (test_value_regimes_host.py asserts that the rule still gives these)
ATTN_GAIN = {"f32": 16, "x3": 6}
GN_OUTLIER = 1000
LN_OUTLIER = 1000
GN_MEAN_LADDER = (1e2, 1e3)
GN_MEAN = 1e2  # at 1e3 fp32 PyTorch itself (y = x * a + b with b = -mean * a) uses 0.5 - 1.7 of the bound: there only rstd is judged


def frac(got, ref):
    """largest |got - ref| in units of the suite's literal bound 1e-4 + 1e-3 |ref|"""
    got, ref = got.detach().double(), ref.detach().double()
    if not bool(th.isfinite(got).all()):
        return float("inf")
    return ((got - ref).abs() / (ATOL + RTOL * ref.abs())).max().item()


def choose(ladder, admissible):
    """the largest ladder value below which every value (itself included) is admissible; None if the first one is not"""
    best = None
    for v in ladder:
        if not admissible(v):
            break
        best = v
    return best


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- attention -------------------------------------------------------------------------------------------------------------------------------
# (nb, heads, T, d, legacy): T <= 64 (attn_s64_* / the one-workgroup flash backward), T > 64 at d = 64 (flash / attn_mid_*; ragged last 32-key blocks:
# 100 = 3 x 32 + 4, 197 = 6 x 32 + 5, 257 = 8 x 32 + 1, 1152 = 36 whole blocks), d = 128 (batched GEMMs + row softmax); both head layouts
ATTN_SHAPES = [(2, 2, 64, 64, 1), (1, 3, 50, 64, 0), (1, 2, 100, 64, 0), (1, 2, 197, 64, 0), (1, 2, 257, 64, 1), (1, 2, 1152, 64, 1),
               (1, 2, 64, 128, 1), (1, 2, 100, 128, 0)]
ATTN_CAUSAL_SHAPES = [(1, 2, 77, 64, 0), (1, 2, 100, 64, 0), (1, 2, 50, 64, 0)]
# one head of 512 channels over a 16 x 16 map (the classic architecture's community checkpoints at 256 x 256): the logit-gain case only
ATTN_GAIN_ONLY = [(1, 1, 256, 512, 0)]
ATTN_REGIMES = ("gain", "planted", "ascending", "descending", "offset", "identical")
# peaked (half the rows one-hot to 0.9): "planted" in every context, "gain" at the gain exact-fp32 products admit; at the gain the bf16x3
# emulation admits, "gain" is a logit-gain case only
ATTN_PEAKED = {"f32": ("gain", "planted"), "x3": ("planted",)}
NRES = 8  # coordinates the random part of q and k leaves at zero: the planted terms live there, in values bf16 holds exactly
# (name, precision, environment of the context): every kernel selection the parity tests grade
ATTN_CONTEXTS = [("p0", 0, {}), ("p1", 1, {}), ("p1 flash0", 1, {"CGD_ATTN_FLASH": "0"}), ("p1 flash1", 1, {"CGD_ATTN_FLASH": "1"}),
                 ("p1 flash2", 1, {"CGD_ATTN_FLASH": "2"}), ("p1 x3off", 1, {"CGD_ATTN_X3": "0"})]


# (shape, regime, dout kind) the bf16x3 emulation itself fails (1.03 of the bound: dP of the dominant key is a bf16x3 product, D = rowsum(dO O) is
# exact, and the seed scale of a near one-hot row is large): left out of the bf16x3 contexts, run in the exact-fp32 ones
ATTN_X3_LEFT_OUT = {((2, 2, 64, 64, 1), "planted", "aligned")}


def attn_class(precision, envd, d):
    """which arithmetic a context runs a head dim on: exact fp32 products, or bf16x3 (the fused kernels with X3, and the batched-GEMM path of a
    bf16x3 context whatever CGD_ATTN_X3 says)"""
    return "x3" if precision == 1 and (envd.get("CGD_ATTN_X3") != "0" or d != 64) else "f32"


def planted_positions(T):
    """dominant keys, one per group of query rows (row i belongs to group i % len): key 0, the last valid key, and a key in each of the four
    per-wavefront key partitions of the flash forward (32-key blocks 0, 1, 2, 3)"""
    pos = []
    for p in (0, T - 1, 5, 32 + 3, 64 + 7, 96 + 1):
        if p < T and p not in pos:
            pos.append(p)
    return pos


def attn_qkv(shape, regime, gain=None, causal=False):
    """fp32 q, k, v (nb, heads, T, d) of one case, and dom (T,) = the planted dominant key of every query row (or None).
    logit[i][j] = q_i . k_j / sqrt(d)"""
    nb, heads, T, d, _ = shape
    q, k, v = (th.randn(nb, heads, T, d, generator=g(400 + i)) for i in range(3))
    dom = None
    if regime == "gain":  # logits N(0, gain^2)
        q, k = q * math.sqrt(gain), k * math.sqrt(gain)
        return q, k, v, dom
    if regime == "planted" and causal:
        # the diagonal: q_i = 5 k_i gives logit_ii = 5 |k_i|^2 / 8 = 40 +- 7 over off-diagonal logits N(0, 25)
        return 5.0 * k, k, v, th.arange(T)
    q[..., :NRES] = 0
    k[..., :NRES] = 0
    big = 24.0 if d == 64 else 32.0  # 8 * 24 / sqrt(64) = 24, 8 * 32 / sqrt(128) = 22.6: margin >= 15 over the N(0, 1) rest
    if regime == "planted":
        pos = planted_positions(T)
        dom = th.tensor([pos[i % len(pos)] for i in range(T)])
        for gi, p in enumerate(pos):
            q[:, :, gi::len(pos), gi] = 8.0
            k[:, :, p, gi] = big
    elif regime in ("ascending", "descending"):  # the running maximum changes in every 32-key block, or never: + 2 per block (1.41 at d = 128)
        blk = th.arange(T) // 32
        q[..., 0] = 8.0
        k[..., 0] = (2.0 * (blk if regime == "ascending" else blk.max() - blk)).float()
    elif regime == "offset":  # every logit of every row carries + 104 (d = 64) / + 101.8 (d = 128): beyond exp's range, softmax unchanged
        q[..., 0] = 32.0
        k[..., 0] = 26.0 if d == 64 else 36.0
    elif regime == "identical":  # every probability is 1 / T (1 / (i + 1) under the causal mask)
        k = k[:, :, :1].expand(nb, heads, T, d).contiguous()
    else:
        raise ValueError(regime)
    return q, k, v, dom


def attn_pack(q, k, v, legacy):
    """(nb, heads, T, d) x 3 -> token-major qkv (nb * T, 3 C) in the layout `legacy` names (parity_checks._attn_ref reads it back)"""
    nb, heads, T, d = q.shape
    z = th.stack([q, k, v], dim=0)  # (3, nb, heads, T, d)
    z = z.permute(1, 3, 2, 0, 4) if legacy else z.permute(1, 3, 0, 2, 4)  # (nb, T, heads, 3, d) / (nb, T, 3, heads, d)
    return z.reshape(nb * T, 3 * heads * d).contiguous()


def attn_unpack_grad(dqkv, shape):
    nb, heads, T, d, legacy = shape
    z = dqkv.reshape(nb, T, heads, 3, d).permute(3, 0, 2, 1, 4) if legacy else dqkv.reshape(nb, T, 3, heads, d).permute(2, 0, 3, 1, 4)
    return z[0], z[1], z[2]


def attn_dout(shape, v, dom, kind):
    """upstream gradient (nb * T, C): random, or aligned with the dominant key's value row (dP - D cancels in dS = P (dP - D))"""
    nb, heads, T, d, _ = shape
    if kind == "random":
        return th.randn(nb * T, heads * d, generator=g(410))
    return v[:, :, dom].permute(0, 2, 1, 3).reshape(nb * T, heads * d).contiguous()  # out rows are [head][d] in both layouts


def attn_ref(qkv, shape, causal=False):
    """float64 / float32 PyTorch reference of the op on the packed rows (parity_checks._attn_ref + the text tower's causal mask)"""
    nb, heads, T, d, legacy = shape
    if not causal:
        return pc._attn_ref(qkv, nb, heads, T, d, legacy)
    Cc = heads * d
    q, k, v = (z.reshape(nb, T, heads, d).permute(0, 2, 1, 3) for z in qkv.reshape(nb, T, 3 * Cc).chunk(3, dim=2))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(d)
    s = s.masked_fill(th.ones(T, T, dtype=th.bool).triu(1), float("-inf"))
    return (th.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(nb * T, Cc)


def attn_probs(q, k, causal=False):
    """float64 logits and probabilities (nb, heads, T, T)"""
    T, d = q.shape[-2:]
    s = (q.double() @ k.double().transpose(-1, -2)) / math.sqrt(d)
    sm = s.masked_fill(th.ones(T, T, dtype=th.bool).triu(1), float("-inf")) if causal else s
    return sm, th.softmax(sm, dim=-1)


def _split(x):
    x32 = x.float()
    hi = x32.bfloat16().float()
    return hi.double(), (x32 - hi).bfloat16().double()


def mm3(X, Y):
    """sum_k X[.., i, k] Y[.., j, k] as the kernels' bf16x3 MFMA triple of fp32 operands, accumulated in float64"""
    xh, xl = _split(X)
    yh, yl = _split(Y)
    yh, yl = yh.transpose(-1, -2), yl.transpose(-1, -2)
    return xl @ yh + xh @ yl + xh @ yh


def attn_emulate_x3(q, k, v, dout, causal=False):
    """bf16x3 emulation of attn_flash.hip on (nb, heads, T, d) float32 inputs; dout (nb, heads, T, d) or None.  Splits what the kernels split: alpha Q,
    K, the unnormalised probabilities exp(s - max) and V in the forward; P = exp(s - lse), dS, dO, K, alpha Q in the backward.  Everything else in
    float64 (the kernels' fp32 accumulation and __expf are part of the 0.75 of the bound fp32 PyTorch leaves them)."""
    T, d = q.shape[-2:]
    alpha = 1.0 / math.sqrt(d)
    qa = (q * alpha).float()
    s = mm3(qa, k)
    if causal:
        s = s.masked_fill(th.ones(T, T, dtype=th.bool).triu(1), float("-inf"))
    m = s.max(-1, keepdim=True).values
    pu = th.exp(s - m)
    L = pu.sum(-1, keepdim=True)
    out = mm3(pu, v.transpose(-1, -2)) / L
    if dout is None:
        return out, None
    P = th.exp(s - (m + th.log(L)))
    dP = mm3(dout, v)
    D = (dout.double() * out).sum(-1, keepdim=True)
    dS = P * (dP - D)
    dq = mm3(dS, k.transpose(-1, -2)) * alpha
    dk = mm3(dS.transpose(-1, -2), qa.transpose(-1, -2))
    dv = mm3(P.transpose(-1, -2), dout.transpose(-1, -2))
    return out, (dq, dk, dv)


def _heads(out, shape):
    nb, heads, T, d, _ = shape
    return out.reshape(nb, T, heads, d).permute(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def attn_case(shape, regime, gain=None, causal=False):
    """one case: packed fp32 qkv, float64 forward reference, and per dout kind (dout, float64 gradient, seed scale)"""
    q, k, v, dom = attn_qkv(shape, regime, gain, causal)
    qkv = attn_pack(q, k, v, shape[4])
    qr = qkv.double().requires_grad_(not causal)
    ref = attn_ref(qr, shape, causal)
    bwd = {}
    if not causal:
        for kind in ("random", "aligned") if regime == "planted" else ("random",):
            dout = attn_dout(shape, v, dom, kind)
            (gr,) = th.autograd.grad((ref * dout.double()).sum(), qr, retain_graph=True)
            bwd[kind] = (dout, gr, unit_seed(gr))
    return {"q": q, "k": k, "v": v, "dom": dom, "qkv": qkv, "ref": ref.detach(), "bwd": bwd}


def attn_fractions(shape, regime, gain=None, causal=False, emulate=True):
    """(fp32 PyTorch fraction, bf16x3 emulation fraction or None) of the bound, the worst over forward and backward records"""
    c = attn_case(shape, regime, gain, causal)
    q32 = c["qkv"].clone().requires_grad_(not causal)
    o32 = attn_ref(q32, shape, causal)
    f32 = frac(o32, c["ref"])
    emu = None
    for kind, (dout, gr, sd) in c["bwd"].items():
        (g32,) = th.autograd.grad((o32 * dout).sum(), q32, retain_graph=True)
        f32 = max(f32, frac(g32 * sd, gr * sd))
    if emulate:
        kinds = [kd for kd in c["bwd"] if (shape, regime, kd) not in ATTN_X3_LEFT_OUT] or [None]
        emu = 0.0
        for kind in kinds:
            dh = None if kind is None else _heads(c["bwd"][kind][0], shape)
            oe, ge = attn_emulate_x3(c["q"], c["k"], c["v"], dh, causal)
            emu = max(emu, frac(oe, _heads(c["ref"], shape)))
            if ge is not None:
                _, gr, sd = c["bwd"][kind]
                for a, b in zip(ge, attn_unpack_grad(gr, shape)):
                    emu = max(emu, frac(a * sd, b * sd))
    return f32, emu


def attn_cases_for(cls, causal=False):
    """(shape, regime, gain) of every attention case a context of arithmetic class `cls` runs"""
    shapes = ATTN_CAUSAL_SHAPES if causal else ATTN_SHAPES
    return [(sh, rg, ATTN_GAIN[cls] if rg == "gain" else None) for sh in shapes for rg in ATTN_REGIMES]


def check_attn_regimes(name, precision, envd):
    from cgd_amd import ops
    out = []
    with env(**envd):
        ctx = pc._ctx(precision)
    for causal in (False, True):
        for shape in (ATTN_CAUSAL_SHAPES if causal else ATTN_SHAPES + ATTN_GAIN_ONLY):
            nb, heads, T, d, legacy = shape
            cls = attn_class(precision, envd, d)
            at = ops.Attention(ctx, nb, heads, T, d, legacy, DEV)
            for regime in (("gain",) if shape in ATTN_GAIN_ONLY else ATTN_REGIMES):
                gain = ATTN_GAIN[cls] if regime == "gain" else None
                c = attn_case(shape, regime, gain, causal)
                tag = f"attn[{name}] {'causal ' if causal else ''}nb{nb} h{heads} T{T} d{d} legacy{legacy} {regime}{'' if gain is None else gain}"
                qd = c["qkv"].to(DEV)
                got = at.forward_causal(qd) if causal else at.forward(qd)
                out.append(rec(f"{tag} fwd", got, c["ref"].float()))
                for kind, (dout, gr, sd) in c["bwd"].items():
                    if cls == "x3" and (shape, regime, kind) in ATTN_X3_LEFT_OUT:
                        continue
                    at.forward(qd)
                    dq = at.backward(qd, (dout * sd).to(DEV))
                    out.append(rec(f"{tag} bwd dout {kind}", dq, (gr * sd).float()))
    th.cuda.synchronize()
    return out


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------
# (B, HW, C, film, act, path): the kernel each size selects (norm.hip launch_gn_small_fwd / cgd_launch_gn_fwd)
GN_SHAPES = [(2, 64, 128, True, 1, "cached"),         # float4, <= 8 vectors per thread: x read once
             (1, 1024, 2048, False, 1, "streaming"),  # float4, 64 channels per group: 16 vectors per thread, two sweeps
             (2, 64, 1344, True, 0, "scalar"),        # 42 channels per group: scalar accesses
             (1, 300, 1344, False, 1, "scalar-streaming"),
             (1, 8192, 64, False, 1, "chunked"),      # > 1024 pixels: gn_stats_partial / final / apply
             (2, 5000, 96, True, 0, "chunked")]
GN_REGIMES = ("outlier-at-shift", "outlier-elsewhere", "outlier-first-pixel", "outlier-first-channel", "mean", "mean1e3-stats", "constant",
              "sigma1e-3")
GN_OUTLIER_REGIMES = GN_REGIMES[:4]


def gn_pick_chunk(HW, B):
    """norm.hip pick_chunk: pixels per workgroup of the chunked path"""
    chunk = min(max(HW * B // 512, 8), 256)
    if (HW + chunk - 1) // chunk > 2048:
        chunk = (HW + 2047) // 2048
    return min(chunk, HW)


def gn_shift_index(shape, group):
    """(pixel, channel) of the element the case plants.  Single-launch kernel (HW <= 1024): the first pixel of the group's first channel, the first of
    the three elements ((pixel i, channel i), i = 0, 1, 2) whose median shifts the sums; `outlier-first-pixel` makes the group's whole first pixel
    large, `outlier-first-channel` its first channel in the first eight pixels.  Chunked path: every (chunk, channel) is shifted by the chunk's first
    pixel; the case plants one channel of chunk 3."""
    B, HW, C, _, _, path = shape
    cpg = C // 32
    return (3 * gn_pick_chunk(HW, B) if path == "chunked" else 0, group * cpg)


def gn_input(shape, regime, mag=None):
    B, HW, C, film, act, path = shape
    cpg = C // 32
    x = th.randn(B, HW, C, generator=g(420)) + 0.5
    if regime in ("outlier-at-shift", "outlier-elsewhere"):
        for grp in range(0, 32, 2):  # every other group: ordinary groups stay beside them
            p, c = gn_shift_index(shape, grp)
            if regime == "outlier-elsewhere":
                p, c = p + HW // 2 + 1, c + 1
            x[:, p, c] = float(mag) * (1 if grp % 4 == 0 else -1)
    elif regime in ("outlier-first-pixel", "outlier-first-channel"):  # a whole token / a whole channel (of a few pixels) that is large
        for grp in range(0, 32, 2):
            p, c = gn_shift_index(shape, grp)
            if regime == "outlier-first-pixel":
                x[:, p, c:c + cpg] = float(mag) * (1 if grp % 4 == 0 else -1)
            else:
                x[:, p:p + 8, c] = float(mag) * (1 if grp % 4 == 0 else -1)
    elif regime in ("mean", "mean1e3-stats"):
        x = x + float(mag)
    elif regime == "constant":
        x[:, :, 0:cpg] = 0.0
        x[:, :, cpg:2 * cpg] = 1.5
        x[:, :, 5 * cpg:6 * cpg] = -0.3
    elif regime == "sigma1e-3":
        x = (x - 0.5) * 1e-3 + 0.2
    else:
        raise ValueError(regime)
    return x


def _gn_forward(x, gamma, beta, fl, act):
    Cc = x.shape[2]
    y = F.group_norm(x.permute(0, 2, 1), 32, gamma, beta, 1e-5)
    if fl is not None:
        y = y * (1 + fl[:, :Cc, None]) + fl[:, Cc:, None]
    if act:
        y = F.silu(y)
    return y.permute(0, 2, 1)


@functools.lru_cache(maxsize=None)
def gn_case(shape, regime, mag=None):
    B, HW, C, film, act, _ = shape
    x = gn_input(shape, regime, mag)
    gamma = 1 + 0.1 * th.randn(C, generator=g(421))
    beta = 0.1 * th.randn(C, generator=g(422))
    fl = 0.3 * th.randn(B, 2 * C, generator=g(423)) if film else None
    dz = th.randn(B, HW, C, generator=g(424))
    xr = x.double().requires_grad_()
    y = _gn_forward(xr, gamma.double(), beta.double(), None if fl is None else fl.double(), act)
    (gr,) = th.autograd.grad((y * dz.double()).sum(), xr)
    xg = x.double().reshape(B, HW, 32, C // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
    rstd = 1.0 / (xg.var(-1, unbiased=False) + 1e-5).sqrt()
    return {"mean": xg.mean(-1), "x": x, "gamma": gamma, "beta": beta, "film": fl, "dz": dz, "y": y.detach(), "dx": gr, "sd": unit_seed(gr), "rstd": rstd}


def gn_fraction(shape, regime, mag=None):
    c = gn_case(shape, regime, mag)
    if regime == "mean1e3-stats":  # the statistics only: fp32 PyTorch's own rstd
        B, HW, C = shape[:3]
        _, m32, r32 = th.native_group_norm(c["x"].permute(0, 2, 1).contiguous(), c["gamma"], c["beta"], B, C, HW, 32, 1e-5)
        return max(frac(r32.reshape(B, 32), c["rstd"]), frac(m32.reshape(B, 32), c["mean"]))
    xr = c["x"].clone().requires_grad_()
    y = _gn_forward(xr, c["gamma"], c["beta"], c["film"], shape[4])
    (gr,) = th.autograd.grad((y * c["dz"]).sum(), xr)
    return max(frac(y, c["y"]), frac(gr * c["sd"], c["dx"] * c["sd"]))


def gn_cases():
    mag = {"mean": GN_MEAN, "mean1e3-stats": 1e3, **{rg: GN_OUTLIER for rg in GN_OUTLIER_REGIMES}}
    return [(sh, rg, mag.get(rg)) for sh in GN_SHAPES for rg in GN_REGIMES]


def check_gn_regimes():
    from cgd_amd import ops
    ctx = pc._ctx(1)
    out = []
    for shape, regime, mag in gn_cases():
        B, HW, C, film, act, path = shape
        c = gn_case(shape, regime, mag)
        tag = f"groupnorm[{path}] B{B} HW{HW} C{C} film{int(film)} act{act} {regime}{'' if mag is None else ' %g' % mag}"
        xd = c["x"].to(DEV)
        yd, scr = ops.groupnorm_fwd(ctx, xd, c["gamma"].to(DEV), c["beta"].to(DEV), None if c["film"] is None else c["film"].to(DEV), act=act)
        if regime == "mean1e3-stats":
            off = int(ctx.lib.cgd_op_gn_stats_offset(B, HW, C))
            st = scr[off:off + B * 64].reshape(B, 32, 2)
            out.append(rec(f"{tag} group mean", st[..., 0], c["mean"].float()))
            out.append(rec(f"{tag} group rstd", st[..., 1], c["rstd"].float()))
            continue
        out.append(rec(f"{tag} fwd", yd, c["y"].float()))
        dx = ops.groupnorm_bwd(ctx, xd, (c["dz"] * c["sd"]).to(DEV), scr, act=act)
        out.append(rec(f"{tag} bwd", dx, (c["dx"] * c["sd"]).float()))
    th.cuda.synchronize()
    return out


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------------
LN_SHAPES = [(50, 768), (7, 1024), (33, 520)]  # the register-resident kernels of the ViT widths and the generic three-pass kernel
LN_REGIMES = ("outlier-channels", "row-offset", "constant-row")


def ln_input(shape, regime, mag=None):
    rows, C = shape
    x = th.randn(rows, C, generator=g(430)) * 1.5 + 0.3
    if regime == "outlier-channels":  # the residual stream of a trained CLIP tower: the same few channels are huge in every token
        x[:, 7] = 1.5 * mag
        x[:, C // 2 + 1] = -1.5 * mag
        x[:, C - 3] = 0.5 * 1.5 * mag
    elif regime == "row-offset":  # tens of sigma, another offset per row
        x = x + th.linspace(-60.0, 90.0, rows)[:, None]
    elif regime == "constant-row":  # variance 0 (rstd = eps^-1/2) beside ordinary rows
        x[0] = 2.0
        x[rows // 2] = 0.0
    else:
        raise ValueError(regime)
    return x


@functools.lru_cache(maxsize=None)
def ln_case(shape, regime, mag=None):
    rows, C = shape
    x = ln_input(shape, regime, mag)
    gamma = 1 + 0.1 * th.randn(C, generator=g(431))
    beta = 0.1 * th.randn(C, generator=g(432))
    dy = th.randn(rows, C, generator=g(433))
    xr = x.double().requires_grad_()
    y = F.layer_norm(xr, (C,), gamma.double(), beta.double(), 1e-5)
    (gr,) = th.autograd.grad((y * dy.double()).sum(), xr)
    return {"x": x, "gamma": gamma, "beta": beta, "dy": dy, "y": y.detach(), "dx": gr, "sd": unit_seed(gr)}


def ln_fraction(shape, regime, mag=None):
    c = ln_case(shape, regime, mag)
    xr = c["x"].clone().requires_grad_()
    y = F.layer_norm(xr, (shape[1],), c["gamma"], c["beta"], 1e-5)
    (gr,) = th.autograd.grad((y * c["dy"]).sum(), xr)
    return max(frac(y, c["y"]), frac(gr * c["sd"], c["dx"] * c["sd"]))


def ln_cases():
    return [(sh, rg, LN_OUTLIER if rg == "outlier-channels" else None) for sh in LN_SHAPES for rg in LN_REGIMES]


def check_ln_regimes():
    from cgd_amd import ops
    ctx = pc._ctx(1)
    out = []
    for shape, regime, mag in ln_cases():
        c = ln_case(shape, regime, mag)
        tag = f"layernorm {shape[0]}x{shape[1]} {regime}{'' if mag is None else mag}"
        xd, gd = c["x"].to(DEV), c["gamma"].to(DEV)
        yd, st = ops.layernorm_fwd(ctx, xd, gd, c["beta"].to(DEV))
        out.append(rec(f"{tag} fwd", yd, c["y"].float()))
        out.append(rec(f"{tag} bwd", ops.layernorm_bwd(ctx, xd, (c["dy"] * c["sd"]).to(DEV), gd, st), (c["dx"] * c["sd"]).float()))
    th.cuda.synchronize()
    return out


# ---- activations -----------------------------------------------------------------------------------------------------------------------------
ACT_KU = (20.0, 60.0, 87.0, 89.0, 104.0, 150.0)  # |k u|: both sides of 88.7 (__expf overflows) and of the denormal quotient (> 87.3 + log|u|)
ACT_KINDS = {1: 1.0, 2: 1.702}  # SiLU, QuickGELU: u sigmoid(k u)


def act_grid(kind):
    k = ACT_KINDS[kind]
    pts = [0.0, 1e-30, -1e-30, 1e-6, -1e-6] + [s * v / k for v in ACT_KU for s in (1.0, -1.0)]
    fill = th.randn(256 - len(pts), generator=g(440)) * 3  # today's range around the grid: the records keep an O(1)-and-up peak either way
    return th.cat([th.tensor(pts, dtype=th.float32), fill])


def _act_fn(kind):
    k = ACT_KINDS[kind]
    return lambda t: t * th.sigmoid(k * t)


@functools.lru_cache(maxsize=None)
def act_case(kind):
    u = act_grid(kind)
    dy = th.randn(u.numel(), generator=g(441)).abs() + 0.5  # no accidental zero seed on a grid point
    ur = u.double().requires_grad_()
    y = _act_fn(kind)(ur)
    (gr,) = th.autograd.grad((y * dy.double()).sum(), ur)
    return {"u": u, "dy": dy, "y": y.detach(), "du": gr}


def act_fraction(kind):
    c = act_case(kind)
    ur = c["u"].clone().requires_grad_()
    y = _act_fn(kind)(ur)
    (gr,) = th.autograd.grad((y * c["dy"]).sum(), ur)
    return max(frac(y, c["y"]), frac(gr, c["du"]))


def check_act_regimes():
    from cgd_amd import ops
    ctx = pc._ctx(1)
    out = []
    for kind in ACT_KINDS:
        c = act_case(kind)
        ud = c["u"].to(DEV)
        out.append(rec(f"act{kind} fwd on |k u| up to 150", ops.act(ctx, ud, kind), c["y"].float()))
        out.append(rec(f"act{kind} bwd on |k u| up to 150", ops.act(ctx, ud, kind, c["dy"].to(DEV)), c["du"].float()))
    th.cuda.synchronize()
    return out


# ---- spherical loss --------------------------------------------------------------------------------------------------------------------------
SPH_SHAPES = [(6, 1, 2, 512), (6, 2, 1, 768)]  # (cutn, B, P, D)
SPH_ROWS = ("near 0.05", "far 1.95", "norm 1e-3", "norm 1e3", "ordinary", "ordinary")  # what row `cut` of every sample is


def sph_input(shape):
    """embeddings (cutn * B, D), targets (P, D): row kinds per cut as SPH_ROWS, measured against target 0"""
    cutn, B, P, D = shape
    tg = th.randn(P, D, generator=g(450))
    emb = th.randn(cutn, B, D, generator=g(451))
    t0 = F.normalize(tg[0].double(), dim=-1)
    for b in range(B):
        for cut, dist in ((0, 0.05), (1, 1.95)):
            o = emb[cut, b].double()
            o = F.normalize(o - (o @ t0) * t0, dim=-1)  # unit vector orthogonal to the target
            ang = 2 * math.asin(dist / 2)  # chord length `dist` on the unit sphere
            emb[cut, b] = (3.0 * (math.cos(ang) * t0 + math.sin(ang) * o)).float()
        emb[2, b] *= 1e-3 / emb[2, b].norm()
        emb[3, b] *= 1e3 / emb[3, b].norm()
    return emb.reshape(cutn * B, D), tg


def _sph_loss(er, tg, wts, shape):
    from oracle import guidance as og
    cutn, B, P, D = shape
    d = og.spherical_dist_loss(er.view(cutn, B, D).unsqueeze(0), tg.unsqueeze(0)).view(cutn, B, -1)
    return d.mul(wts).sum(2).mean(0).sum() * 1000.0


@functools.lru_cache(maxsize=None)
def sph_case(shape):
    """the gradient is homogeneous of degree -1 in the embedding: it is judged per row in units of 1 / |e| (times one unit_seed for the tensor),
    which is the same statement for every row and keeps the 1e-3 / 1e3-norm rows from hiding behind (or drowning) the others"""
    cutn, B, P, D = shape
    emb, tg = sph_input(shape)
    wts = th.tensor([1.0, 0.5][:P])
    wts = wts / wts.sum().abs()
    er = emb.double().requires_grad_()
    loss = _sph_loss(er, tg.double(), wts.double(), shape)
    (gr,) = th.autograd.grad(loss, er)
    nrm = emb.double().norm(dim=-1, keepdim=True)
    return {"emb": emb, "tg": tg, "wts": wts, "loss": loss.detach(), "grad": gr, "nrm": nrm, "sd": unit_seed(gr * nrm)}


def sph_fraction(shape):
    c = sph_case(shape)
    er = c["emb"].clone().requires_grad_()
    loss = _sph_loss(er, c["tg"], c["wts"], shape)
    (gr,) = th.autograd.grad(loss, er)
    sc = c["nrm"] * c["sd"]
    return max(frac(loss.reshape(1), c["loss"].reshape(1)), frac(gr * sc, c["grad"] * sc))


def check_sph_regimes():
    from cgd_amd import lib as L
    ctx = pc._ctx(1)
    out = []
    for shape in SPH_SHAPES:
        cutn, B, P, D = shape
        c = sph_case(shape)
        wm = c["wts"].view(1, P).expand(B, P).contiguous()  # B == 1 or P == 1: the broadcast rule of the prompt weights
        ed, tn, wd = c["emb"].to(DEV), F.normalize(c["tg"], dim=-1).to(DEV), wm.float().to(DEV)
        demb, part = th.empty_like(ed), th.empty(cutn * B, device=DEV)
        ctx.check(ctx.lib.cgd_spherical_loss(ctx.h, ed.data_ptr(), tn.data_ptr(), wd.data_ptr(), demb.data_ptr(), part.data_ptr(), cutn, B, P, D,
                                             1000.0, L.stream_ptr()))
        sc = c["nrm"] * c["sd"]
        out.append(rec(f"spherical loss value cutn{cutn} B{B} P{P} (distances 0.05 / 1.95, norms 1e-3 / 1e3)", part.sum().reshape(1),
                       c["loss"].float().reshape(1)))
        out.append(rec(f"spherical loss grad x |e| cutn{cutn} B{B} P{P}", demb.double().cpu() * sc, c["grad"] * sc))
        o = slice(4 * B, cutn * B)  # the ordinary rows as they are, one seed scale
        so = unit_seed(c["grad"][o])
        out.append(rec(f"spherical loss grad, ordinary rows unscaled cutn{cutn} B{B} P{P}", demb.double().cpu()[o] * so, c["grad"][o] * so))
    th.cuda.synchronize()
    return out


# ---- the fused GroupNorm + SiLU staging of the Winograd conv kernel ----------------------------------------------------------------------------
# The only fused activation form the op-level ABI reaches (cgd_op_conv3x3_wino's gn_ab): the conv stages SiLU(x * a + b) with the reciprocal form
# x * rcp(1 + __expf(-u)).  cgd_op_gemm has no activation argument and cgd_op_conv3x3 no gn_ab, so the QuickGELU GEMM epilogue, its derivative
# operand, the SiLU A-row mode of the embedding GEMVs and the staging of hconv2 / kconv are reached through the networks below, at shapes that
# select them (VIT_N, UNET_HW, UNET_FUSE_ALL; net_plans and the launch profile say which kernels ran).  Not reached: the SiLU variant of the GEMM
# epilogue (no network of the library fuses SiLU into hgemm2: the UNet's SiLU sits in GroupNorm, conv staging and GEMV A rows).
# (mode, B, H, W, Ci, Co): both tile heights and the 256-channel panel tile
WSTAGE_SHAPES = [(2, 1, 16, 32, 64, 64), (3, 2, 24, 32, 64, 96), (5, 1, 16, 16, 32, 256)]
WSTAGE_SPAN = 60.0  # u = x * a + b spans +- 60 and more: both tails of the sigmoid, 1 + __expf(-u) up to 1e26


def wstage_case_inputs(shape):
    mode, B, H, W, Ci, Co = shape
    x = th.randn(B, Ci, H, W, generator=g(460))
    w = th.randn(Co, Ci, 3, 3, generator=g(461)) / math.sqrt(9 * Ci)
    bias = 0.3 * th.randn(Co, generator=g(462))
    a = WSTAGE_SPAN / 3 * (0.5 + th.rand(B, Ci, generator=g(463)))  # |x| reaches 3 and more: |x a| >= 60 in every channel with a >= 20, most others
    b = WSTAGE_SPAN / 3 * th.randn(B, Ci, generator=g(464))
    ab = th.stack([a, b], dim=2).contiguous()
    # O(1) outputs, as everywhere in the suite: the staged activations have an rms of about 17 (SiLU(u) = u on the positive tail), the weights take it
    # out (with unit-variance weights the bf16x3 emulation itself uses 1.9 - 2.8 of the bound on the outputs that cancel to near 0)
    rms = F.silu(x.double() * a[:, :, None, None].double() + b[:, :, None, None].double()).pow(2).mean().sqrt().item()
    return x, w / rms, bias, ab


def _wstage_fwd(x, w, bias, ab):
    u = x * ab[:, :, 0, None, None] + ab[:, :, 1, None, None]
    return F.conv2d(F.silu(u), w, bias, padding=1), u


@functools.lru_cache(maxsize=None)
def wstage_case(shape):
    x, w, bias, ab = wstage_case_inputs(shape)
    y, u = _wstage_fwd(x.double(), w.double(), bias.double(), ab.double())
    return {"x": x, "w": w, "bias": bias, "ab": ab, "y": y, "u": u}


def wstage_fractions(shape):
    """fp32 PyTorch, and a bf16x3 emulation of the contraction: float64 SiLU, activations and weights split into bf16 hi / lo, three products"""
    c = wstage_case(shape)
    y32, _ = _wstage_fwd(c["x"], c["w"], c["bias"], c["ab"])
    act = F.silu(c["u"])
    cols = F.unfold(act, 3, padding=1).transpose(1, 2)  # (B, HW, 9 Ci)
    ye = mm3(cols, c["w"].reshape(c["w"].shape[0], -1).expand(cols.shape[0], -1, -1)).transpose(1, 2).reshape(c["y"].shape) + c["bias"].double()[:, None, None]
    return frac(y32, c["y"]), frac(ye, c["y"])


def check_wstage_regimes():
    from cgd_amd import ops
    out = []
    for precision in (1, 0):
        ctx = pc._ctx(precision)
        for shape in WSTAGE_SHAPES:
            mode, B, H, W, Ci, Co = shape
            if precision == 0 and mode == 2:
                continue  # the 16 x 16-pixel tile exists on bf16x3 products only
            ctx.check(ctx.lib.cgd_set_wino(ctx.h, mode, 0))
            c = wstage_case(shape)
            ww = ops.pack_conv3x3_wino(ctx, c["w"].to(DEV), dgrad=False)
            got = ops.conv3x3_wino(ctx, c["x"].permute(0, 2, 3, 1).contiguous().to(DEV), ww, Co, c["bias"].to(DEV), gn_ab=c["ab"].to(DEV))
            out.append(rec(f"wconv[p{precision}] m{mode} B{B} {H}x{W} {Ci}->{Co} fused GroupNorm + SiLU input, u spans +-{WSTAGE_SPAN:g}",
                           got.permute(0, 3, 1, 2), c["y"].float()))
        ctx.check(ctx.lib.cgd_set_wino(ctx.h, 1, 0))
    th.cuda.synchronize()
    return out


# ---- networks with trained-like synthetic weights ------------------------------------------------------------------------------------------------
# q and k rows of every attention projection scaled by sqrt(s) (logits N(0, s^2)), outlier channels in the positional embedding (ViT) / the stem conv
# bias (UNet), and pre-activations of +-60 ... +-102 in front of the fused activation forms: the QuickGELU epilogue of hgemm2 and its derivative
# operand (ViT c_fc bias), the SiLU A-row mode of the embedding GEMVs (UNet time_embed bias), the GroupNorm + SiLU staging of hconv2 and, under
# UNET_FUSE_ALL, kconv (gamma / beta of the first ResBlock's norm).  Both oracles run in float64; a whole-network bf16x3 emulation does not exist,
# so the gain is the ladder's choice under the fp32-oracle rule, capped in bf16x3 contexts by the op-level emulation's choice (ATTN_GAIN["x3"]).
# Exact-fp32 contexts have no hgemm2 / halo kernels: there the planted values run through elem.hip's and norm.hip's activations.
VIT_N = 8      # 400 token rows: c_fc and the c_proj backward GEMM run on hgemm2 in one slice, which is what fuses QuickGELU (50 rows: kgemm, unfused)
UNET_HW = 64   # first level 4096 pixels: hconv2 with GroupNorm + SiLU staging (fuse_gn_min_m); UNET_FUSE_ALL also stages the smaller maps on kconv
UNET_FUSE_ALL = {"CGD_FUSE_GN": "1,1073741824,0"}
NET_GAIN = {"vit": {"f32": 8, "x3": 6}, "unet": {"f32": 16, "x3": 6}}


def trained_like_(ref, net, s):
    r = math.sqrt(s)
    with th.no_grad():
        sd = dict(ref.named_parameters())
        if net == "vit":
            for n, p in sd.items():
                if n.endswith("attn.in_proj_weight") or n.endswith("attn.in_proj_bias"):
                    p[:2 * p.shape[0] // 3] *= r
            pe = sd["visual.positional_embedding"]
            pe[:, 5] += 8.0
            pe[:, 300] -= 8.0
            pe[:, 611] += 4.0
            for blk in (0, 5, 11):
                sd[f"visual.transformer.resblocks.{blk}.mlp.c_fc.bias"][:4] = th.tensor([60.0, -60.0, 35.0, -35.0])  # 1.702 u = +-102, +-60
        else:
            for n, p in sd.items():
                if n.endswith(".qkv.weight") or n.endswith(".qkv.bias"):  # legacy order: [q | k | v] of 64 channels per head
                    v = p.view(-1, 3, 64, *p.shape[1:])
                    v[:, :2] *= r
            sd["input_blocks.0.0.bias"][[3, 40]] = th.tensor([30.0, -30.0])
            gn = "input_blocks.1.0.in_layers.0."
            sd[gn + "weight"][[1, 9]] = 40.0
            sd[gn + "bias"][[1, 9]] = th.tensor([20.0, -20.0])
            sd["time_embed.0.bias"][[2, 7, 11]] = th.tensor([95.0, -95.0, 60.0])
    return ref


def build_net_oracle(net, s, dtype):
    if net == "vit":
        from oracle.clip_vit import ClipImageModel, synthetic_init_
        ref = synthetic_init_(ClipImageModel("ViT-B/32"), seed=4321)
    else:
        from oracle.unet import UNetModel, synthetic_init_
        ref = synthetic_init_(UNetModel(**pc.UNET_CASES["mini"]), seed=1234)
    ref = trained_like_(ref.eval().float(), net, s).to(dtype)
    for p in ref.parameters():
        p.requires_grad_(False)
    return ref


def net_inputs(net):
    if net == "vit":
        return {"x": th.randn(VIT_N, 3, 224, 224, generator=g(470)), "seed": th.randn(VIT_N, 512, generator=g(471))}
    seed = th.randn(1, 6, UNET_HW, UNET_HW, generator=g(472))
    seed[:, 3:] = 0
    return {"x": th.randn(1, 3, UNET_HW, UNET_HW, generator=g(470)), "seed": seed, "t": th.tensor([417.0]), "y": th.tensor([3])}


def net_plans(lib):
    """The launcher's own choice (cgd_op_plan: host logic of cgd_launch_gemm, no GPU) for the launches the planted pre-activations sit in front of, in a
    bf16x3 context: {name: [kernel, tile, slices, workgroups]}.  The ViT's c_fc GEMM and the c_proj backward GEMM fuse QuickGELU / its derivative
    operand when they run on hgemm2 (kernel 2) in one slice (cgd_gemm_fuses_act); the UNet's first ResBlock convs stage GroupNorm + SiLU when they
    run on a halo kernel (kernel 1: tile 512 hconv2, 516 kconv) and have at least fuse_gn_min_m pixels (cgd_conv_uses_hconv)."""
    import ctypes as C
    out = {}
    rows = 50 * VIT_N
    for name, args in (("vit c_fc", (0, rows, 3072, 768, 0, 0, 0, 1, 1, 256)), ("vit c_proj backward", (0, rows, 3072, 768, 0, 0, 0, 1, 1, 256)),
                       ("unet 64-channel conv, first level", (1, UNET_HW * UNET_HW, 64, 9 * 64, UNET_HW, UNET_HW, 64, 1, 1, 256)),
                       ("unet 128-channel conv, second level", (1, UNET_HW * UNET_HW // 4, 128, 9 * 128, UNET_HW // 2, UNET_HW // 2, 128, 1, 1, 256))):
        o = (C.c_int * 4)()
        assert lib.cgd_op_plan(*args, o) == 0
        out[name] = list(o)
    return out


def net_preacts(net, s=2):
    """float64 pre-activations in front of the fused forms of the trained-like network: {name: tensor}"""
    ref, io, got = build_net_oracle(net, s, th.float64), net_inputs(net), {}
    if net == "vit":
        mods = {f"c_fc {b}": ref.visual.transformer.resblocks[b].mlp.c_fc for b in (0, 5, 11)}
    else:
        mods = {"time_embed.0": ref.time_embed[0], "first ResBlock norm": ref.input_blocks[1][0].in_layers[0]}
    hooks = [m.register_forward_hook(lambda _m, _i, o, n=n: got.__setitem__(n, o.detach())) for n, m in mods.items()]
    with th.no_grad():
        ref.encode_image(io["x"].double()) if net == "vit" else ref(io["x"].double(), io["t"].double(), io["y"])
    for h in hooks:
        h.remove()
    return got


def net_oracle_run(net, s, dtype):
    """forward and input gradient of the oracle in `dtype` (a UNet oracle moved to double is float64 throughout: oracle/unet.py _f32)"""
    ref, io = build_net_oracle(net, s, dtype), net_inputs(net)
    xr = io["x"].to(dtype).requires_grad_()
    out = ref.encode_image(xr) if net == "vit" else ref(xr, io["t"].to(dtype), io["y"])
    (gr,) = th.autograd.grad((out * io["seed"].to(dtype)).sum(), xr)
    return out.detach(), gr


@functools.lru_cache(maxsize=None)
def net_case(net, s):
    out, gr = net_oracle_run(net, s, th.float64)
    return {"out": out, "grad": gr, "sd": unit_seed(gr)}


def net_fraction(net, s):
    c = net_case(net, s)
    o32, g32 = net_oracle_run(net, s, th.float32)
    return max(frac(o32, c["out"]), frac(g32 * c["sd"], c["grad"] * c["sd"]))


def _profile(ctx, run):
    """run() under the context's launch profile: per kind (ms, work, launches); work is bytes for kind 2 (GroupNorm: 8 per element, 4 when it
    takes statistics only because the consuming conv applies it while staging)"""
    import ctypes as C
    lib = ctx.lib
    n = lib.cgd_profile_kinds()
    buf = (C.c_double * (3 * n))()
    ctx.check(lib.cgd_profile_read(ctx.h, buf))
    ctx.check(lib.cgd_profile(ctx.h, 1))
    try:
        res = run()
    finally:
        ctx.check(lib.cgd_profile(ctx.h, 0))
    ctx.check(lib.cgd_profile_read(ctx.h, buf))
    return res, [(buf[3 * k], buf[3 * k + 1], int(buf[3 * k + 2])) for k in range(n)]


def check_net_regimes(net, precision, envd=None):
    """envd: environment of the context.  Besides the parity records: the launch profile of the device forward, read back — halo-conv launches per
    family and the GroupNorm bytes, from which the caller tells staged from materialised GroupNorm + SiLU."""
    from cgd_amd import nets
    cls = "x3" if precision == 1 else "f32"
    s = NET_GAIN[net][cls]
    with env(**(envd or {})):
        ctx = pc._ctx(precision)
    ref, io, c = build_net_oracle(net, s, th.float32), net_inputs(net), net_case(net, s)
    state = {k: v.to(DEV) for k, v in ref.state_dict().items()}
    if net == "vit":
        dev = nets.ClipImageTower(ctx, "ViT-B/32")
        dev.load_clip_state_dict(state)
        od, prof = _profile(ctx, lambda: dev.encode_image(io["x"].to(DEV)))
    else:
        dev = nets.UNet(ctx, **pc.UNET_CASES["mini"])
        dev.load_state_dict(state)
        od, prof = _profile(ctx, lambda: dev.forward(io["x"].to(DEV), io["t"].to(DEV), io["y"].to(DEV)))
    gd = dev.dgrad((io["seed"] * c["sd"]).to(DEV))
    th.cuda.synchronize()
    tag = f"{net}[p{precision}{' ' + ','.join(envd.values()) if envd else ''}] trained-like weights, logit gain {s}"
    return [rec(f"{tag} forward", od, c["out"].float()), rec(f"{tag} dgrad", gd, (c["grad"] * c["sd"]).float())], prof
