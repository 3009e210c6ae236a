"""Where the per-element bounds of tests/test_gpu_bwd_walk_ops.py come from: float64 references of GroupNorm(+SiLU) backward and
LayerNorm backward (the formulas of the csrc/bwd.hip comments, cross-checked against torch.autograd in float64), and fp32 emulations on
the CPU of what the kernels compute, in the kernels' own order.

GroupNorm, three-phase kernel (gn_bwd_phase_kernel): a thread owns 8 channels and adds its chunk's pixels p0 + tp + k TP one after the
other (gnb_nchunk's chunking, lanes past the chunk end add zero); thread g of the block adds the TP x cpg partials of its group one after
the other; every block then adds the per-chunk partials of a group in 256 / G interleaved running sums and those one after the other.
mean = s / n, var = max(q / n - mean^2, 0), rstd = rsqrt(var + eps), all fp32; the same chain for sum(h), sum(h xhat).  The
one-block-per-group kernel (groupnorm_bwd_kernel): 1024 running sums, a butterfly over 64 lanes, 16 wavefront sums one after the other.

With r = rstd (h - ma - xhat mb) in float64 (ma = mean(h), mb = mean(h xhat) over the group) the bound on the fp16 result is

    |dx - r| <= 2^-11 |r| + 2^-24 + kappa 2^-24 rstd (|h| + |ma| + |xhat| |mb|)

the first two terms the final fp16 rounding, the third fp32 arithmetic (and the device's rsqrtf / __expf) on the terms of the final
subtraction.  With acc = 1 the stored value is fp16(old + fp16(r)): the bound above plus 2^-11 |old + r| + 2^-24.  kappa is measured, not
chosen: the smallest power of two that keeps the emulation's worst |err| / bound at or below 0.5 over every case of the GPU test (the
factor 2 left is for the device's intrinsics and FMA contraction).  LayerNorm (layernorm_bwd_kernel: a wavefront per row, lane sums over
its vectors, butterfly; two-pass variance) has the same construction with g = dy gamma, a = mean(g), b = mean(g xhat) and its own kappa.

Measured with this file's seeds (test_kappa_* assert these: the value below holds the ratio at or under 0.5, half of it does not):

    GroupNorm   kappa    = 32768   worst emulation |err| / bound = 0.317  (0.564 at 16384; three-phase and one-block kernels, plain store)
    LayerNorm   kappa_ln =  8192   worst emulation |err| / bound = 0.497  (0.663 at 4096)

What sets these values is mostly the fp16 rounding, not fp32 arithmetic: a half-ulp error is up to 2^-11 |r|, all of the first term, so
the 0.5 criterion asks kappa 2^-24 slack >= 2^-11 |r| of elements without cancellation (slack = |r|): kappa = 2^13 before any fp32 error.
The cases with 15360 and 122880 elements per group (HW = 256 at 60 and HW = 4096 at 30 channels per group) need 16142 and 19084, the
others 7538 .. 8162; LayerNorm's rows 3520 .. 8094.  In effect the bound is 2^-11 |r| + 2^-9 slack (2^-11 slack for LayerNorm): 0.2 % of
the largest term of the final subtraction, per element.
The accumulating store is held to its bound, not to half of it (worst emulation ratio 0.977): its second rounding alone spends up to all
of 2^-11 |old + r|, which no kappa changes where |r| is small against |old|.

Inputs: x with per-(sample, group) mean in +-4 and std in 0.25 .. 2, dy ~ N(0, 1) 2^k with k per sample, gamma ~ 1 +- 0.2, beta ~ +-0.2,
and one all-constant group (sample B - 1, group 1, x = -2) where var clamps to 0 and rstd = rsqrt(eps).  The constant is a power of two on
purpose: its sums and squares are exact in fp32, so q / n - mean^2 is exactly 0.  For any other constant c the fp32 roundings of q / n
leave +-c^2 2^-24 k in var, against eps = 1e-5 a relative change of rstd of the order of 1e-3: the sign of rounding noise decides the
result, and no bound around the float64 value can hold there (a property of the E[x^2] - mean^2 form, the forward's as well).

The mutants at the end show that the bound has teeth: each is the emulation with one of the mistakes such a kernel can make, and each
exceeds the bound on at least one element of at least one case."""
import functools

import pytest
import torch
import torch.nn.functional as F

KAPPA_GN = 32768.0
KAPPA_LN = 8192.0
GNB_MAX_CHUNKS = 256

# (B, C1, C2, HW, G, silu): the cases of tests/test_gpu_bwd_walk_ops.py
GN_CASES = [
    (3, 64, 0, 200, 32, 1),        # TP = 32, two chunks, clamped lanes within a trip
    (2, 8, 24, 50, 32, 1),         # cpg = 1: an 8-vector spans 8 groups, the concat boundary inside the first vector row
    (2, 64, 32, 64, 32, 1),        # cpg = 3: vectors straddle groups and the C1 boundary
    (1, 1280, 640, 256, 32, 1),    # C8 = 240: 16 idle threads
    (1, 1280, 1280, 64, 32, 1),    # C8 = 320: second cv trip
    (1, 1280, 0, 1100, 32, 0),     # chunk cap with TP = 1: ppc = 5, 36 empty trailing chunks
    (1, 640, 320, 4096, 32, 1),    # cap with TP = 2: two trips per thread
    (2, 128, 0, 96, 64, 1),        # nsub = 4
    (2, 64, 64, 96, 16, 0),        # nsub = 16
]
# the one-block-per-group kernel: C1 & 7 (the only way the walk reaches it), and a shape the three-phase kernel also takes
FALLBACK_CASES = [(2, 12, 20, 40, 4, 1), (2, 64, 32, 64, 32, 1)]
LN_CASES = [(M, C) for C in (32, 520, 1032, 2048) for M in (1, 7)]
GN_MUTANTS = ("n8", "group8", "noacc", "dup", "nomb", "sample0", "cv2")
LN_MUTANTS = ("nomb", "nfull")


def eps_of(silu):
    """the two GroupNorm flavours of the UNet: resnet norms (SiLU, eps 1e-5) and the transformer's entry norm (none, 1e-6)"""
    return 1e-5 if silu else 1e-6


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def gn_inputs(case):
    """x [B, HW, C] fp16, dy fp16, gamma / beta fp32 [C], old [B, HW, C] fp16 (what an accumulating destination holds), on the CPU"""
    B, C1, C2, HW, G, silu = case
    C, cpg = C1 + C2, (C1 + C2) // G
    g = torch.Generator().manual_seed(1000 + 7 * _case_seed(case))
    mean = (torch.rand(B, 1, G, 1, generator=g) * 8 - 4)
    std = 0.25 + torch.rand(B, 1, G, 1, generator=g) * 1.75
    x = mean + std * torch.randn(B, HW, G, cpg, generator=g)
    x[B - 1, :, 1, :] = -2.0
    k = torch.tensor([2.0, -3.0, 0.0])[torch.arange(B) % 3].reshape(B, 1, 1)
    dy = torch.randn(B, HW, C, generator=g) * torch.exp2(k)
    gamma = 1 + (torch.rand(C, generator=g) * 0.4 - 0.2)
    beta = torch.rand(C, generator=g) * 0.4 - 0.2
    old = torch.randn(B, HW, C, generator=g)
    return x.reshape(B, HW, C).half(), dy.half(), gamma.float(), beta.float(), old.half()


def _case_seed(case):
    return (GN_CASES + FALLBACK_CASES).index(case)


@functools.lru_cache(maxsize=None)
def ln_inputs(case):
    """x [M, C] fp16 (row 3 of a 7-row case constant), dy fp16, gamma fp32, on the CPU"""
    M, C = case
    g = torch.Generator().manual_seed(2000 + LN_CASES.index(case))
    mean = torch.rand(M, 1, generator=g) * 8 - 4
    std = 0.25 + torch.rand(M, 1, generator=g) * 1.75
    x = mean + std * torch.randn(M, C, generator=g)
    if M > 3:
        x[3] = -2.0
    k = torch.tensor([2.0, -3.0, 0.0])[torch.arange(M) % 3].reshape(M, 1)
    dy = torch.randn(M, C, generator=g) * torch.exp2(k)
    gamma = 1 + (torch.rand(C, generator=g) * 0.4 - 0.2)
    return x.half(), dy.half(), gamma.float()


# ------------------------------------------------------------------------------------------------ float64 references and bounds
def gn_bwd_ref64(x, dy, gamma, beta, G, eps, silu):
    """-> r [B, HW, C] float64 and slack = rstd (|h| + |ma| + |xhat| |mb|), the magnitude of the final subtraction's terms"""
    B, HW, C = x.shape
    cpg = C // G
    xd = x.double().reshape(B, HW, G, cpg)
    mean = xd.mean((1, 3), keepdim=True)
    var = ((xd - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + eps) ** -0.5
    xh = (xd - mean) * rstd
    ga, be = gamma.double().reshape(1, 1, G, cpg), beta.double().reshape(1, 1, G, cpg)
    d = dy.double().reshape(B, HW, G, cpg)
    if silu:
        z = xh * ga + be
        sg = torch.sigmoid(z)
        d = d * (sg * (1 + z * (1 - sg)))
    h = d * ga
    ma = h.mean((1, 3), keepdim=True)
    mb = (h * xh).mean((1, 3), keepdim=True)
    r = rstd * (h - ma - xh * mb)
    slack = rstd * (h.abs() + ma.abs() + xh.abs() * mb.abs())
    return r.reshape(B, HW, C), slack.reshape(B, HW, C)


def ln_bwd_ref64(x, dy, gamma, eps):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    xh = (xd - mean) * rstd
    g = dy.double() * gamma.double()
    a = g.mean(1, keepdim=True)
    b = (g * xh).mean(1, keepdim=True)
    r = rstd * (g - a - xh * b)
    return r, rstd * (g.abs() + a.abs() + xh.abs() * b.abs())


def norm_bwd_bound(r, slack, kappa):
    return r.abs() * 2.0 ** -11 + 2.0 ** -24 + kappa * 2.0 ** -24 * slack


def acc_bound(r, slack, old, kappa):
    """the accumulated value fp16(old + fp16(r)) against old + r"""
    return norm_bwd_bound(r, slack, kappa) + (old.double() + r).abs() * 2.0 ** -11 + 2.0 ** -24


@functools.lru_cache(maxsize=None)
def gn_reference(case):
    """(r, slack) of a case's inputs: computed once, shared by the host and the GPU tests, never modified"""
    B, C1, C2, HW, G, silu = case
    x, dy, gamma, beta, _ = gn_inputs(case)
    return gn_bwd_ref64(x, dy, gamma, beta, G, eps_of(silu), silu)


@functools.lru_cache(maxsize=None)
def ln_reference(case):
    x, dy, gamma = ln_inputs(case)
    return ln_bwd_ref64(x, dy, gamma, 1e-5)


def worst_ratio(got, want, bound):
    return ((got.double() - want).abs() / bound).max().item()


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels' order
def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _seq_sum(v, dim):
    """fp32 running sum along dim, one addition after the other"""
    assert v.dtype == torch.float32
    v = v.movedim(dim, 0)
    acc = v[0].clone()
    for k in range(1, v.shape[0]):
        acc = acc + v[k]
    return acc


def _tree_sum(v):
    """butterfly over the last dim (a power of two): offsets n / 2, n / 4, ..., 1, as wave_sum"""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def gnb_nchunk(HW, C):
    C8 = C >> 3
    TC = min(C8, 256)
    TP = 256 // TC
    return max(1, min(GNB_MAX_CHUNKS, (HW + 4 * TP - 1) // (4 * TP)))


def _phase_group_sums(a, b, G, mutant):
    """a, b [B, HW, C] fp32 per-element terms -> their (sample, group) sums [B, G] in the three-phase kernel's order.  Built from index
    tables: chunk, trip slot k and pixel lane tp name the pixel p0 + tp + k TP; a slot past the chunk's end adds zero (mutant "dup": adds
    the clamped load of the chunk's last pixel, wherever the thread makes that trip)."""
    B, HW, C = a.shape
    C8, cpg = C >> 3, C // G
    TC = min(C8, 256)
    TP = 256 // TC
    nchunk = gnb_nchunk(HW, C)
    ppc = (HW + nchunk - 1) // nchunk
    K = ((ppc + TP - 1) // TP + 3) // 4 * 4
    ch = torch.arange(nchunk).reshape(-1, 1, 1)
    k = torch.arange(K).reshape(1, -1, 1)
    tp = torch.arange(TP).reshape(1, 1, -1)
    p0 = ch * ppc
    p1 = torch.clamp(p0 + ppc, max=HW)
    pix = p0 + tp + k * TP
    ok = pix < p1
    if mutant == "dup":
        ok = (p0 + tp + (k // 4) * 4 * TP) < p1
    idx = torch.minimum(pix, p1 - 1).clamp(min=0).reshape(-1)
    okf = ok.reshape(1, nchunk, K, TP, 1).float()
    if mutant == "cv2":                                   # the second cv trip skipped: channels 2048 .. C never reach the sums
        a, b = a.clone(), b.clone()
        a[..., 2048:] = 0
        b[..., 2048:] = 0
    out = []
    for v in (a, b):
        t = v[:, idx].reshape(B, nchunk, K, TP, C) * okf
        t = _seq_sum(t, 2)                                                                    # a thread's pixels     [B, nchunk, TP, C]
        t = t.reshape(B, nchunk, TP, G, cpg).permute(0, 1, 3, 2, 4).reshape(B, nchunk, G, TP * cpg)
        t = _seq_sum(t, 3)                                                                    # the chunk's partial   [B, nchunk, G]
        nsub = 256 // G
        t = torch.cat([t, t.new_zeros(B, (-nchunk) % nsub, G)], 1).reshape(B, -1, nsub, G)
        out.append(_seq_sum(_seq_sum(t, 1), 1))                                               # chunks ch = sub, sub + nsub, ...; then sub
    return out


def _block_group_sums(a, b, G, mutant):
    """the one-block-per-group kernel: element i = pix * cpg + channel goes to thread i % 1024"""
    B, HW, C = a.shape
    cpg = C // G
    out = []
    for v in (a, b):
        t = v.reshape(B, HW, G, cpg).permute(0, 2, 1, 3).reshape(B, G, HW * cpg)
        t = torch.cat([t, t.new_zeros(B, G, (-HW * cpg) % 1024)], 2).reshape(B, G, -1, 1024)
        t = _tree_sum(_seq_sum(t, 2).reshape(B, G, 16, 64))
        out.append(_seq_sum(t, 2))
    return out


def emulate_gn_bwd(x, dy, gamma, beta, G, eps, silu, kernel="phase", mutant=None):
    """fp16 [B, HW, C]: what the kernel stores without accumulation (every step fp32, one rounding at the end)"""
    B, HW, C = x.shape
    cpg = C // G
    sums = _phase_group_sums if kernel == "phase" else _block_group_sums
    n = _f32(HW * (8 if mutant == "n8" else cpg))
    gidx = torch.arange(C) // cpg
    if mutant == "group8":
        gidx = (torch.arange(C) // 8).clamp(max=G - 1)

    def per_channel(t):                                   # [B, G] -> [B, 1, C]
        if mutant == "sample0":
            t = t[:1].expand(B, G)
        return t[:, gidx].reshape(B, 1, C)

    xf = x.float()
    s, q = sums(xf, xf * xf, G, mutant)
    mean = s / n
    var = torch.clamp(q / n - mean * mean, min=0.0)
    rstd = torch.rsqrt(var + _f32(eps))
    mean_c, rstd_c = per_channel(mean), per_channel(rstd)
    ga, be = gamma.float().reshape(1, 1, C), beta.float().reshape(1, 1, C)
    xh = (xf - mean_c) * rstd_c
    d = dy.float()
    if silu:
        z = xh * ga + be
        sg = 1.0 / (1.0 + torch.exp(-z))
        d = d * (sg * (1.0 + z * (1.0 - sg)))
    hh = d * ga
    sa, sb = sums(hh, hh * xh, G, mutant)
    ma_c, mb_c = per_channel(sa / n), per_channel(sb / n)
    r = rstd_c * ((hh - ma_c) if mutant == "nomb" else (hh - ma_c - xh * mb_c))
    assert r.dtype == torch.float32
    out = r.half()
    if mutant == "cv2":
        out[..., 2048:] = 0
    return out


def emulate_acc(old, r16, mutant=None):
    """the accumulating store: fp16(old + fp16(r)) ("noacc": acc ignored, the destination overwritten)"""
    return r16 if mutant == "noacc" else (old.float() + r16.float()).half()


def emulate_ln_bwd(x, dy, gamma, eps, mutant=None):
    M, C = x.shape
    C8 = C >> 3
    VPL = 1 if C8 <= 64 else 2 if C8 <= 128 else 4
    W = VPL * 512
    cn = _f32(W if mutant == "nfull" else C)

    def lanes(v):                                         # [M, C] -> the row's sum: lane = vector % 64 adds its vectors' elements in order
        v = torch.cat([v, v.new_zeros(M, W - C)], 1).reshape(M, VPL, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, VPL * 8)
        return _tree_sum(_seq_sum(v, 2)).reshape(M, 1)

    xf = x.float()
    mean = lanes(xf) / cn
    dd = xf - mean
    rstd = torch.rsqrt(lanes(dd * dd) / cn + _f32(eps))
    g = dy.float() * gamma.float().reshape(1, C)
    xh = (xf - mean) * rstd
    a = lanes(g) / cn
    b = lanes(g * xh) / cn
    r = rstd * ((g - a) if mutant == "nomb" else (g - a - xh * b))
    assert r.dtype == torch.float32
    return r.half()


# ------------------------------------------------------------------------------------------------ the emulation against the bound
def gn_case_ratios(case, kappa, kernel="phase", mutant=None):
    """worst |err| / bound of the emulation on one case: (plain store, accumulating store)"""
    B, C1, C2, HW, G, silu = case
    x, dy, gamma, beta, old = gn_inputs(case)
    r, slack = gn_reference(case)
    out = emulate_gn_bwd(x, dy, gamma, beta, G, eps_of(silu), silu, kernel, mutant)
    plain = worst_ratio(out, r, norm_bwd_bound(r, slack, kappa))
    acc = worst_ratio(emulate_acc(old, out, mutant), old.double() + r, acc_bound(r, slack, old, kappa))
    return plain, acc


def gn_emulation_worst(kappa, store=0):
    """over every case and both kernels; store 0: the plain store (what kappa is measured on), 1: the accumulating store"""
    w = [gn_case_ratios(c, kappa)[store] for c in GN_CASES]
    w += [gn_case_ratios(c, kappa, "block")[store] for c in FALLBACK_CASES]
    return max(w)


def ln_case_ratio(case, kappa, mutant=None):
    x, dy, gamma = ln_inputs(case)
    r, slack = ln_reference(case)
    return worst_ratio(emulate_ln_bwd(x, dy, gamma, 1e-5, mutant), r, norm_bwd_bound(r, slack, kappa))


def ln_emulation_worst(kappa):
    return max(ln_case_ratio(c, kappa) for c in LN_CASES)


def test_formulas_against_autograd():
    """the bwd.hip formulas are the derivative: float64 autograd of F.group_norm (+ SiLU) and F.layer_norm on the same inputs"""
    for case in (GN_CASES[2], GN_CASES[8]):
        B, C1, C2, HW, G, silu = case
        x, dy, gamma, beta, _ = gn_inputs(case)
        xin = x.double().requires_grad_(True)
        y = F.group_norm(xin.permute(0, 2, 1), G, gamma.double(), beta.double(), eps_of(silu))
        (F.silu(y) if silu else y).backward(dy.double().permute(0, 2, 1))
        r, _ = gn_reference(case)
        assert (xin.grad - r).abs().max().item() <= 1e-9 * r.abs().max().item()
    x, dy, gamma = ln_inputs((7, 520))
    xin = x.double().requires_grad_(True)
    F.layer_norm(xin, (520,), gamma.double(), None, 1e-5).backward(dy.double())
    r, _ = ln_reference((7, 520))
    assert (xin.grad - r).abs().max().item() <= 1e-9 * r.abs().max().item()


def test_constant_group_clamps():
    """the all-constant group: var = 0 exactly, rstd = rsqrt(eps), in the reference and in the emulation"""
    case = GN_CASES[0]
    B, C1, C2, HW, G, silu = case
    x, dy, gamma, beta, _ = gn_inputs(case)
    xf = x.float()
    s, q = _phase_group_sums(xf, xf * xf, G, None)
    n = _f32(HW * (C1 + C2) // G)
    assert (s / n)[B - 1, 1].item() == -2.0 and (q / n)[B - 1, 1].item() == 4.0
    r, _ = gn_reference(case)
    assert r[B - 1, :, 2:4].abs().max().item() > 100.0       # rstd = 316: the group's gradient is large, not zero


def test_kappa_gn_is_the_smallest_power_of_two():
    w = gn_emulation_worst(KAPPA_GN)
    print("GroupNorm backward: kappa = %g, worst emulation |err| / bound = %.3f (at kappa / 2: %.3f)"
          % (KAPPA_GN, w, gn_emulation_worst(KAPPA_GN / 2)))
    assert w <= 0.5
    assert gn_emulation_worst(KAPPA_GN / 2) > 0.5


def test_accumulating_store_is_within_its_bound():
    """fp16(old + fp16(r)): the second rounding alone spends up to all of its own term 2^-11 |old + r|, whatever kappa is (where |r| is
    small against |old| no kappa short of 2^23 would bring the ratio to 0.5), so here the emulation is held to the bound itself"""
    w = gn_emulation_worst(KAPPA_GN, store=1)
    print("GroupNorm backward, acc = 1: worst emulation |err| / bound = %.3f" % w)
    assert w < 1.0


def test_kappa_ln_is_the_smallest_power_of_two():
    w = ln_emulation_worst(KAPPA_LN)
    print("LayerNorm backward: kappa_ln = %g, worst emulation |err| / bound = %.3f (at kappa_ln / 2: %.3f)"
          % (KAPPA_LN, w, ln_emulation_worst(KAPPA_LN / 2)))
    assert w <= 0.5
    assert ln_emulation_worst(KAPPA_LN / 2) > 0.5


@pytest.mark.parametrize("mutant", GN_MUTANTS)
def test_gn_mutant_exceeds_the_bound(mutant):
    """each mistake breaks the bound on some element of some case (the cases in order, until the first that catches it)"""
    caught = None
    for case in GN_CASES:
        if max(gn_case_ratios(case, KAPPA_GN, "phase", mutant)) > 1.0:
            caught = case
            break
    assert caught is not None, "mutant %s stays within the bound on every case" % mutant


@pytest.mark.parametrize("mutant", LN_MUTANTS)
def test_ln_mutant_exceeds_the_bound(mutant):
    assert any(ln_case_ratio(c, KAPPA_LN, mutant) > 1.0 for c in LN_CASES)
