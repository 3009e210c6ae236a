"""Where the per-element bounds of tests/test_gpu_norm_fwd_instances.py come from: float64 references of the forward bandwidth kernels of
csrc/norm.hip -- GroupNorm (+SiLU), LayerNorm, GEGLU, the two row softmaxes, the GEMV -- and fp32 emulations on the CPU of what each
kernel computes, in the kernel's own summation order.

GroupNorm, one-launch kernel (gn_small_kernel<NT>, NT = 1024 or 256): thread tid adds the 4-channel vectors tid + u NT of its (item,
group) slice one after the other, a butterfly over 64 lanes, the NT / 64 wavefront sums one after the other; y = (x - mean) (rstd gamma)
+ beta.  Three-pass kernels: gn_stats_kernel's chunking (nchunk = HW / 64 in 1 .. 128, ppc = ceil(HW / nchunk)), a thread owns 8
channels and adds its pixels p0 + tp + k TP four at a time as (f0 + f1) + (f2 + f3), then one at a time; thread g adds the TP x cpg
partials of its group; gn_finalize_kernel adds the chunks in 8 interleaved running sums and those by a 3-step butterfly, and writes
scale = rstd gamma and the mean; gn_apply_kernel computes (x - mean) scale + beta.  mean = s / n, var = max(q / n - mean^2, 0),
rstd = rsqrt(var + eps) in both.  LayerNorm (layernorm_kernel<VPL, RPW>): lane l adds the elements of its vectors l, l + 64, ... in
order, butterfly; two passes.  SiLU and the softmaxes use __expf as HIP defines it, exp2(log2(e) x) with the product rounded to fp32.

Bounds (ref the float64 value of the stored inputs, kappa per operation):

    GroupNorm, LayerNorm   |y - ref| <= 2^-11 |ref| + 2^-24 + kappa 2^-24 slack,   slack = |x - mean| rstd |gamma| + |beta|
                           (with SiLU: ref = silu(z), slack times max(1, |silu'(z)|))
    GEGLU                  |y - ref| <= 2^-11 |ref| + 2^-24 + kappa 2^-24 |ref| + |a| |g| E,   E = 0.75e-7
    softmax, fp16 rows     |p - ref| <= 2^-11 ref + 2^-25 + kappa 2^-24 ref (1 + |x - max|)
    softmax, fp32 rows     |p - ref| <= kappa 2^-24 ref (1 + |x - max|)
    GEMV                   |o - ref| <= kappa 2^-24 (sum_k |act(x_k) W_nk| + |bias| + |bias2|)

E is the absolute error of the Abramowitz-Stegun 7.1.26 form of Phi(-|x|), half of the published 1.5e-7 on erfc: a property of the
approximation, not of the code.  kappa is measured, not chosen: the smallest power of two that keeps the emulation's worst |err| / bound
at or below 0.5 over exactly the cases of the GPU file (the factor 2 left is for the device's rsqrtf, v_rcp, v_exp and FMA contraction).

Measured with this file's seeds (test_kappa_is_the_smallest_power_of_two asserts these):

    operation      kappa      worst emulation |err| / bound    at kappa / 2    the real kappa that 0.5 needs
    GroupNorm      16384      0.482                            0.703           15429
    LayerNorm      262144     0.432                            0.835           225378
    GEGLU          16384      0.495                            0.532           9497
    softmax fp16   1048576    0.498                            0.663           1038295
    softmax fp32   8          0.283                            0.566           4.5
    GEMV           8          0.494                            0.988           7.9

What sets them.  A half-ulp error of the one fp16 rounding is up to 2^-11 |ref|, all of the first term, so the 0.5 criterion alone asks
kappa 2^-24 slack >= 2^-11 |ref|: 2^13 where slack = |ref|, before any fp32 error.  GroupNorm: most runs need 6500 .. 8150; nine runs without SiLU need 8790
.. 15429, on elements where x - mean and beta are both small, so that slack = |ref| is small too: the rounding of the mean, |mean| 2^-24
times rstd, is an absolute error that slack does not scale with, and at |mean| / std = 16 it is as large as the fp16 rounding there.  LayerNorm: every row but one needs
5100 .. 8140; the row with mean 100 and std 0.1 needs up to 225378 at the widths that are no power of two (320, 520, 1032), where mean =
s / C is rounded: an error of up to 100 x 2^-25 in the mean, times rstd = 10, on elements whose slack is small because x - mean and beta
cancel.  The two-pass kernel is within half the bound there all the same, and a one-pass variance 4.8 times outside it
(test_ln_one_pass_variance_leaves_the_bound_on_the_high_mean_row).  softmax fp16: probabilities below 2^-14 are stored as fp16
subnormals, whose half-ulp is the bound's own absolute term 2^-25, so only the kappa term can bring the ratio to 0.5 there, and
ref (1 + |x - max|) is as small as 1e-6 on such elements; on results in the normal range 8192 would do.  In effect that bound is 2^-11
ref + 2^-25 + ref (1 + |x - max|) / 16: it holds the sum, the maximum and the column walk (both mutants leave it), not the last bits of
__expf.  softmax fp32 and GEMV: a few roundings of fp32 arithmetic.

gelu_f on the gates in [-6, -3] (every fp16 value there, the emulation against float64 erf): worst relative error 3.6e-3, which is 0.97
fp16 ulps of the result, at g = -4.012 (gelu = -1.2e-4); at -6 the result is 5.9e-9, below the smallest fp16 subnormal.  The E term
|a| |g| E is 4 % of the bound at g = -3, 55 % at -4, 80 % at -4.5 and 88 % at -6: it dominates the bound beyond g = -4, where the result
is below 1.3e-4 and an fp16 ulp of the product a gelu(g) is no longer resolved by the approximation.  So the tail of gelu_f costs at most
one fp16 ulp where the result is representable as a normal number; gelu_f was left as it is.

One kernel changed with these tests.  The three-pass GroupNorm (and the statistics-fed one, which shares gn_apply_kernel) applied y = x
scale + shift with shift = beta - mean scale.  That shift is rounded at the magnitude of mean scale, which the all-constant group makes
|mean| / sqrt(eps): 632 at eps 1e-5, 2000 at 1e-6, an absolute error of up to 3e-5 and 6e-5 on outputs that are beta, about 0.1.  With
that form the emulation needed kappa = 2^25 on the constant group (8150 on everything else), a bound of 2 slack that no mutant leaves.
gn_apply_kernel and gn_fin_apply_kernel now compute (x - mean) scale + beta, as gn_small_kernel always did; the constant group gives
beta exactly, and kappa is the 16384 above.

Inputs.  GroupNorm: per (item, group) mean in +-4 plus an offset of -2, 0, 2 per item, std in 0.25 .. 2 and at least |mean| / 16 (what
the E[x^2] - mean^2 form affords, tests/test_gn_stats_host.py), each slice brought to exactly that mean and std before the fp16
rounding; gamma ~ 1 +- 0.2, beta ~ +-0.2; item B - 1, group 1 is all -2, a power of two, so that its sums are exact and the variance
clamps to exactly 0.  LayerNorm: the same per row, row 2 of the 5- and 17-row cases with mean 100 and std 0.1, row 3 all -2.  GEGLU: a
uniform in +-8, a quarter of the gates uniform in [-6, -3], the others N(0, 2^2).  Softmax rows by row index % 4: N(0, 3^2); one
dominant entry (65504 against -65504, 3e38 against -3e38 in fp32); all equal to the most negative finite value; constant.

The mutants at the end show that each bound has teeth: each is the emulation with one of the mistakes such a kernel can make, and each
exceeds the bound on at least one element of at least one case."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

KAPPA_GN = 16384.0
KAPPA_LN = 262144.0
KAPPA_GEGLU = 16384.0
KAPPA_SM16 = 1048576.0
KAPPA_SM32 = 8.0
KAPPA_GEMV = 8.0
E_AS = 0.75e-7
GN_SMALL_ELEMS = 24576
LOG2E = 1.4426950408889634       # rounds to 0x1.715476p+0 in fp32, the constant of __expf

# (B, C1, C2, HW, G): the one-launch kernel, each under gn_wide_below = 1 << 30 (1024 threads) and 0 (256 threads)
GN_SMALL_CASES = [
    (2, 128, 0, 1, 32),            # one 4-vector per block, every other load clamped
    (2, 64, 64, 4, 32),            # groups 16 .. come wholly from x2
    (2, 40, 88, 50, 8),            # cpg 16; group 2 straddles the concat boundary at channel 40
    (1, 2048, 0, 24, 2),           # cpg = 1024, slice exactly 24576: the LDS limit and the GPT limit together
    (48, 256, 0, 1024, 32),        # slice 8192 at 1536 blocks; still the one-launch kernel
]
GN_PASS_CASES = [
    (1, 2048, 0, 25, 2),           # one element over the slice limit
    (48, 256, 0, 1028, 32),        # just over the 8192 limit at 1536 blocks
    (2, 8, 0, 70, 8),              # C8 = 1, TP = 256, cpg 1
    (2, 8, 24, 50, 32),            # cpg 1; the concat boundary inside the first vector row; HW < 64
    (2, 96, 0, 50, 32),            # cpg 3; TC = 12, TP = 21; four idle threads
    (2, 320, 0, 200, 32),          # TP = 6, 16 idle threads; three chunks of 67, 67, 66
    (1, 1040, 1040, 70, 32),       # C8 = 260: the second cv trip has four vectors
    (1, 96, 0, 8200, 32),          # 128-chunk cap; ppc = 65; chunk 126 holds 10 pixels and chunk 127 is empty
    (2, 192, 0, 40, 64),           # G = 64
    (1, 32, 0, 3100, 4),           # G < 32; slice 24800
]
GN_FLAVOURS = [(1, 1e-5), (1, 1e-6), (0, 1e-5), (0, 1e-6)]     # (silu, eps)
# (case, kernel) of every GPU run; kernel: "small1024", "small256" or "pass"
GN_RUNS = [(c, k) for c in GN_SMALL_CASES for k in ("small1024", "small256")] + [(c, "pass") for c in GN_PASS_CASES]
LN_CASES = [(M, C, eps) for C in (8, 32, 320, 512, 520, 768, 1024, 1032, 2048) for M in (1, 5, 17) for eps in (1e-5, 1e-6)]
GEGLU_CASES = [(3, 32), (333, 96), (7, 1280), (4100, 2048)]      # the last: M I / 8 > 4096 x 256, a second stride trip of the grid
SM16_CASES = [(5, 8, 8), (5, 520, 528), (6, 4096, 4096), (3, 1024, 1040)]      # (M, N, ld)
SM32_CASES = [(5, N) for N in (1, 64, 65, 77, 4096)]
GEMV_CASES = [(K, N, s, b1, b2) for K in (8, 320, 1280) for N in (5, 1280) for s in (0, 1) for b1 in (0, 1) for b2 in (0, 1)]
# mutant -> the kernels whose cases it is walked over
GN_MUTANTS = {"n8": ("small1024", "pass"), "group8": ("pass",), "dup": ("small1024",), "x2stride": ("small1024", "pass"),
              "sample0": ("small1024", "pass"), "cv2": ("pass",), "g0": ("pass",), "lastchunk": ("pass",)}
LN_MUTANTS = ("onepass", "nfull")
GEGLU_MUTANTS = ("gate0", "tanh")
SM_MUTANTS = ("trip2", "lanemax")
GEMV_MUTANTS = ("nomask", "nobias2")


def gn_small_ok(B, C1, C2, HW, G):
    """gn_small_ok of csrc/norm.hip at the default "gn_small_max": the one-launch kernel takes the tensor"""
    cpg = (C1 + C2) // G
    lim = 8192 if B * G >= 1536 else GN_SMALL_ELEMS
    return cpg % 4 == 0 and C1 % 4 == 0 and cpg <= 1024 and HW * cpg <= lim


def gn_nchunk(HW):
    return max(1, min(128, HW // 64))


# ------------------------------------------------------------------------------------------------ fp32 helpers
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


def _fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in float64, one rounding of the sum there and one to fp32"""
    return (a.double() * b.double() + c.double()).float()


def _expf(x):
    """__expf: exp2(log2(e) x), the product rounded to fp32"""
    assert x.dtype == torch.float32
    return torch.exp2(x * _f32(LOG2E))


def _silu_f(x):
    return x / (1.0 + _expf(-x))


def worst_ratios(got, want, base, slack, kappas):
    """max |got - want| / (base + kappa 2^-24 slack) for every kappa, and the smallest kappa that holds the ratio at 0.5"""
    err = (got.double() - want).abs()
    need = ((2.0 * err - base) / (slack * 2.0 ** -24).clamp(min=1e-300)).max().item()
    return [torch.where(err > 0, err / (base + k * 2.0 ** -24 * slack), err).max().item() for k in kappas], need


# ------------------------------------------------------------------------------------------------ GroupNorm
@functools.lru_cache(maxsize=None)
def gn_inputs(case):
    """x [B, HW, C] fp16, gamma / beta fp32 [C], on the CPU"""
    B, C1, C2, HW, G = case
    C, cpg = C1 + C2, (C1 + C2) // G
    g = torch.Generator().manual_seed(3000 + 7 * (GN_SMALL_CASES + GN_PASS_CASES).index(case))
    mean = torch.rand(B, 1, G, 1, generator=g) * 8 - 4 + ((torch.arange(B) % 3).float() - 1).reshape(B, 1, 1, 1) * 2
    std = torch.maximum(0.25 + torch.rand(B, 1, G, 1, generator=g) * 1.75, mean.abs() / 16)
    z = torch.randn(B, HW, G, cpg, generator=g)
    z = z - z.mean((1, 3), keepdim=True)
    z = z / (z * z).mean((1, 3), keepdim=True).sqrt()
    x = mean + std * z
    x[B - 1, :, 1, :] = -2.0
    gamma = 1 + (torch.rand(C, generator=g) * 0.4 - 0.2)
    beta = torch.rand(C, generator=g) * 0.4 - 0.2
    return x.reshape(B, HW, C).half(), gamma.float(), beta.float()


def gn_stats64(x, G):
    """float64 (mean, biased variance) [B, G]"""
    B, HW, C = x.shape
    xd = x.double().reshape(B, HW, G, C // G)
    mean = xd.mean((1, 3))
    return mean, ((xd - mean[:, None, :, None]) ** 2).mean((1, 3))


def gn_formula64(x, mean, var, gamma, beta, eps, silu):
    """-> (ref, slack) [B, HW, C] float64 of x under the statistics given (the input's own: F.group_norm + F.silu)"""
    B, HW, C = x.shape
    G = mean.shape[1]
    rstd = (var + eps) ** -0.5
    d = (x.double().reshape(B, HW, G, C // G) - mean[:, None, :, None]) * rstd[:, None, :, None]
    t = d.reshape(B, HW, C) * gamma.double()
    ref = t + beta.double()
    slack = t.abs() + beta.double().abs()
    if silu:
        sg = torch.sigmoid(ref)
        slack = slack * (sg * (1 + ref * (1 - sg))).abs().clamp(min=1.0)
        ref = ref * sg
    return ref, slack


@functools.lru_cache(maxsize=4)
def gn_reference(case, silu, eps):
    """(ref, slack) of a case: ref is F.group_norm, then F.silu, in float64; computed once, shared by the host and the GPU tests"""
    x, gamma, beta = gn_inputs(case)
    G = case[4]
    ref = F.group_norm(x.double().permute(0, 2, 1), G, gamma.double(), beta.double(), eps).permute(0, 2, 1)
    ref = F.silu(ref) if silu else ref
    _, slack = gn_formula64(x, *gn_stats64(x, G), gamma, beta, eps, silu)
    return ref.contiguous(), slack


def gn_bound(ref, slack, kappa=None):
    kappa = KAPPA_GN if kappa is None else kappa
    return ref.abs() * 2.0 ** -11 + 2.0 ** -24 + kappa * 2.0 ** -24 * slack


def _small_sums(xf, G, NT, mutant=None):
    """[B, HW, C] fp32 -> (s, q) [B, G] in gn_small_kernel<NT>'s order (mutant "dup": the clamped duplicate loads are added too)"""
    B, HW, C = xf.shape
    cpg = C // G
    nvec = HW * cpg // 4
    trips = GN_SMALL_ELEMS // 4 // NT if mutant == "dup" else (nvec + NT - 1) // NT
    v = xf.reshape(B, HW, G, cpg).permute(0, 2, 1, 3).reshape(B, G, nvec, 4)
    pad = trips * NT - nvec
    if pad:
        v = torch.cat([v, v[:, :, -1:].expand(B, G, pad, 4) if mutant == "dup" else v.new_zeros(B, G, pad, 4)], 2)
    v = v.reshape(B, G, trips, NT, 4).permute(0, 1, 3, 2, 4).reshape(B, G, NT, trips * 4)
    return tuple(_seq_sum(_tree_sum(_seq_sum(t, 3).reshape(B, G, NT // 64, 64)), 2) for t in (v, v * v))


def _pass_sums(xf, G, mutant=None):
    """[B, HW, C] fp32 -> (s, q) [B, G] in the order of gn_stats_kernel + gn_finalize_kernel"""
    B, HW, C = xf.shape
    C8, cpg = C >> 3, C // G
    TP = 256 // min(C8, 256)
    nchunk = gn_nchunk(HW)
    ppc = (HW + nchunk - 1) // nchunk
    p0 = (torch.arange(nchunk) * ppc).reshape(-1, 1)
    p1 = torch.clamp(p0 + ppc, max=HW)
    tp = torch.arange(TP).reshape(1, -1)
    cnt = torch.clamp((p1 - p0 - tp + TP - 1) // TP, min=0)      # pixels p0 + tp + k TP < p1 of thread row tp in the chunk
    nq, rem = cnt // 4, cnt % 4

    def take(k, on):                                             # pixel k of every (chunk, tp), zero where `on` is false
        pix = (p0 + tp + k * TP).clamp(max=HW - 1)
        return xf[:, pix.reshape(-1)].reshape(B, nchunk, TP, C) * on.reshape(1, nchunk, TP, 1).float()

    s = xf.new_zeros(B, nchunk, TP, C)
    q = xf.new_zeros(B, nchunk, TP, C)
    for m in range(int(nq.max())):
        f0, f1, f2, f3 = (take(4 * m + i, m < nq) for i in range(4))
        s = s + ((f0 + f1) + (f2 + f3))
        q = q + ((f0 * f0 + f1 * f1) + (f2 * f2 + f3 * f3))
    for i in range(3):
        f = take(4 * nq + i, i < rem)
        s = s + f
        q = q + f * f
    out = []
    for t in (s, q):
        if mutant == "cv2":                                      # the second cv trip skipped: channels 2048 .. C never reach the sums
            t = t.clone()
            t[..., 2048:] = 0
        t = _seq_sum(t.reshape(B, nchunk, TP, G, cpg).permute(0, 1, 3, 2, 4).reshape(B, nchunk, G, TP * cpg), 3)      # [B, nchunk, G]
        if mutant == "lastchunk":                                # the last, partial chunk dropped
            t = t.clone()
            t[:, (HW - 1) // ppc] = 0
        t = torch.cat([t, t.new_zeros(B, (-nchunk) % 8, G)], 1).reshape(B, -1, 8, G)
        out.append(_tree_sum(_seq_sum(t, 1).permute(0, 2, 1)))   # lane sub: chunks sub, sub + 8, ...; then offsets 4, 2, 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _gn_sums_of(case, kernel):
    x = gn_inputs(case)[0].float()
    return _pass_sums(x, case[4]) if kernel == "pass" else _small_sums(x, case[4], int(kernel[5:]))


def emulate_gn(x, gamma, beta, G, eps, silu, kernel, mutant=None, sums=None, C1=None):
    """fp16 [B, HW, C]: what the kernel stores (every step fp32, one rounding at the end)"""
    B, HW, C = x.shape
    cpg = C // G
    xf = x.float()
    if mutant == "x2stride" and C1 < C:                          # x2 [B HW][C2] addressed with C1 as its row stride
        x2 = xf[:, :, C1:].reshape(-1)
        at = (torch.arange(B * HW).reshape(-1, 1) * C1 + torch.arange(C - C1).reshape(1, -1)) % x2.numel()
        xf = torch.cat([xf[:, :, :C1], x2[at].reshape(B, HW, C - C1)], 2)
    if sums is None or mutant is not None:
        sums = _pass_sums(xf, G, mutant) if kernel == "pass" else _small_sums(xf, G, int(kernel[5:]), mutant)
    s, q = sums
    n = _f32(HW * (8 if mutant == "n8" else cpg))
    mean = s / n
    var = torch.clamp(q / n - mean * mean, min=0.0)
    rstd = torch.rsqrt(var + _f32(eps))
    gidx = torch.arange(C) // cpg
    if mutant == "group8":                                       # the group of an 8-vector's first channel for all eight
        gidx = (torch.arange(C) // 8 * 8) // cpg
    if mutant == "g0":                                           # the second g0 pass skipped: groups 32 .. keep what 0 .. 31 left
        gidx = gidx % 32

    def per_channel(t):                                          # [B, G] -> [B, 1, C]
        if mutant == "sample0":
            t = t[:1].expand(B, G)
        return t[:, gidx].reshape(B, 1, C)

    mean_c, rstd_c = per_channel(mean), per_channel(rstd)
    ga, be = gamma.float().reshape(1, 1, C), beta.float().reshape(1, 1, C)
    sc = rstd_c * ga
    y = (xf - mean_c) * sc + be
    if silu:
        y = _silu_f(y)
    assert y.dtype == torch.float32
    y = y.half()
    if mutant == "cv2":
        y[..., 2048:] = 0
    return y


def gn_run_ratios(case, kernel, silu, eps, kappas, mutant=None):
    x, gamma, beta = gn_inputs(case)
    ref, slack = gn_reference(case, silu, eps)
    y = emulate_gn(x, gamma, beta, case[4], eps, silu, kernel, mutant, None if mutant else _gn_sums_of(case, kernel), case[1])
    return worst_ratios(y, ref, gn_bound(ref, 0.0, 0.0), slack, kappas)


# ------------------------------------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=None)
def ln_inputs(M, C):
    """x [M, C] fp16 (row 2 of a case of more than 2 rows: mean 100, std 0.1; row 3: all -2), gamma / beta fp32"""
    g = torch.Generator().manual_seed(4000 + 31 * C + M)
    mean = torch.rand(M, 1, generator=g) * 8 - 4
    std = 0.25 + torch.rand(M, 1, generator=g) * 1.75
    z = torch.randn(M, C, generator=g)
    x = mean + std * z
    if M > 3:
        x[2] = 100.0 + 0.1 * z[2]
        x[3] = -2.0
    gamma = 1 + (torch.rand(C, generator=g) * 0.4 - 0.2)
    beta = torch.rand(C, generator=g) * 0.4 - 0.2
    return x.half(), gamma.float(), beta.float()


@functools.lru_cache(maxsize=None)
def ln_reference(case):
    M, C, eps = case
    x, gamma, beta = ln_inputs(M, C)
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = (((xd - mean) ** 2).mean(1, keepdim=True) + eps) ** -0.5
    ref = F.layer_norm(xd, (C,), gamma.double(), beta.double(), eps)
    return ref, ((xd - mean) * rstd * gamma.double()).abs() + beta.double().abs()


def ln_bound(ref, slack, kappa=None):
    kappa = KAPPA_LN if kappa is None else kappa
    return ref.abs() * 2.0 ** -11 + 2.0 ** -24 + kappa * 2.0 ** -24 * slack


def emulate_ln(x, gamma, beta, eps, mutant=None):
    M, C = x.shape
    C8 = C >> 3
    VPL = 1 if C8 <= 64 else 2 if C8 <= 128 else 4
    W = VPL * 512
    cn = _f32(W if mutant == "nfull" else C)

    def lanes(v):                                                # [M, C] -> the row's sum: lane = vector % 64 adds its vectors' elements in order
        v = torch.cat([v, v.new_zeros(M, W - C)], 1).reshape(M, VPL, 64, 8).permute(0, 2, 1, 3).reshape(M, 64, VPL * 8)
        return _tree_sum(_seq_sum(v, 2)).reshape(M, 1)

    xf = x.float()
    mean = lanes(xf) / cn
    if mutant == "onepass":
        var = torch.clamp(lanes(xf * xf) / cn - mean * mean, min=0.0)
    else:
        d = xf - mean
        var = lanes(d * d) / cn
    rstd = torch.rsqrt(var + _f32(eps))
    y = (xf - mean) * rstd * gamma.float().reshape(1, C) + beta.float().reshape(1, C)
    assert y.dtype == torch.float32
    return y.half()


def ln_case_ratios(case, kappas, mutant=None):
    M, C, eps = case
    ref, slack = ln_reference(case)
    return worst_ratios(emulate_ln(*ln_inputs(M, C), eps, mutant), ref, ln_bound(ref, 0.0, 0.0), slack, kappas)


# ------------------------------------------------------------------------------------------------ GEGLU
@functools.lru_cache(maxsize=None)
def geglu_inputs(case):
    """a, g [M, I] fp16: a uniform in +-8, a quarter of the gates uniform in [-6, -3], the others N(0, 2^2)"""
    M, I = case
    gen = torch.Generator().manual_seed(5000 + GEGLU_CASES.index(case))
    a = torch.rand(M, I, generator=gen) * 16 - 8
    tail = torch.rand(M, I, generator=gen) < 0.25
    g = torch.where(tail, -3 - 3 * torch.rand(M, I, generator=gen), 2 * torch.randn(M, I, generator=gen))
    return a.half(), g.half()


def ilv32(a, g):
    """[.., I] x and gate -> [.., 2 I] packed as [x(32) | gate(32)] groups (the layout geglu_kernel reads)"""
    I = a.shape[-1]
    return torch.stack([a.reshape(*a.shape[:-1], I // 32, 32), g.reshape(*g.shape[:-1], I // 32, 32)], dim=-2).reshape(*a.shape[:-1], 2 * I)


@functools.lru_cache(maxsize=None)
def geglu_reference(case):
    """(ref, |a| |g|): ref = a gelu(g) in float64, with erf"""
    a, g = geglu_inputs(case)
    return a.double() * F.gelu(g.double()), a.double().abs() * g.double().abs()


def geglu_bound(ref, ag, kappa=None):
    kappa = KAPPA_GEGLU if kappa is None else kappa
    return ref.abs() * 2.0 ** -11 + 2.0 ** -24 + kappa * 2.0 ** -24 * ref.abs() + ag * E_AS


def gelu_f(x):
    """gelu_f of csrc/common.h term for term in fp32 (the device's v_rcp and v_exp are a division and an exp2 here)"""
    assert x.dtype == torch.float32
    z = x.abs() * _f32(0.70710678118654752440)
    t = 1.0 / _fma(_f32(0.3275911), z, _f32(1.0))
    p = _fma(_f32(1.061405429), t, _f32(-1.453152027))
    p = _fma(p, t, _f32(1.421413741))
    p = _fma(p, t, _f32(-0.284496736))
    p = _fma(p, t, _f32(0.254829592))
    half_erfc = 0.5 * p * t * torch.exp2(-z * z * _f32(1.44269504088896340736))
    return x * torch.where(x >= 0, 1.0 - half_erfc, half_erfc)


def emulate_geglu(a, g, mutant=None):
    af, gf = a.float(), g.float()
    if mutant == "gate0":                                        # the gate read at + 0 instead of + 32: the x column again
        gf = af
    if mutant == "tanh":
        y = af * (0.5 * gf * (1.0 + torch.tanh(_f32(0.7978845608028654) * (gf + _f32(0.044715) * gf * gf * gf))))
    else:
        y = af * gelu_f(gf)
    assert y.dtype == torch.float32
    return y.half()


def geglu_case_ratios(case, kappas, mutant=None):
    ref, ag = geglu_reference(case)
    return worst_ratios(emulate_geglu(*geglu_inputs(case), mutant), ref, geglu_bound(ref, ag, 0.0), ref.abs(), kappas)


def gelu_tail():
    """over every fp16 gate in [-6, -3]: (worst |gelu_f - gelu| / |gelu|, the same in fp16 ulps of the result, the gate it is at, the
    largest share of the E term |g| E in the bound of a = 1 there)"""
    g = torch.arange(-6.0, -3.0 + 2.0 ** -9, 2.0 ** -9).half().unique()
    ref = F.gelu(g.double())
    err = (gelu_f(g.float()).double() - ref).abs()
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs())).clamp(min=-14.0) - 10)
    rel, ulps = err / ref.abs(), err / ulp
    e_share = (g.double().abs() * E_AS / geglu_bound(ref, g.double().abs(), KAPPA_GEGLU))
    k = int(ulps.argmax())
    return rel.max().item(), ulps[k].item(), g[k].item(), e_share.min().item(), e_share.max().item()


# ------------------------------------------------------------------------------------------------ row softmax
@functools.lru_cache(maxsize=None)
def softmax_inputs(M, N, fp32):
    """[M, N]: row r is N(0, 3^2), one dominant entry, all the most negative finite value, or constant, by r % 4"""
    dt = torch.float32 if fp32 else torch.float16
    big = 3e38 if fp32 else 65504.0
    gen = torch.Generator().manual_seed(6000 + 13 * N + M + fp32)
    x = (torch.randn(M, N, generator=gen) * 3).to(dt)
    for r in range(M):
        if r % 4 == 1:
            x[r] = -big
            x[r, (7 * r + 3) % N] = big
        elif r % 4 == 2:
            x[r] = torch.finfo(dt).min
        elif r % 4 == 3:
            x[r] = 1.5
    return x


@functools.lru_cache(maxsize=None)
def softmax_reference(M, N, fp32):
    """(ref, 1 + |x - max|) float64 of the stored inputs"""
    xd = softmax_inputs(M, N, fp32).double()
    return torch.softmax(xd, 1), 1 + (xd - xd.max(1, keepdim=True).values).abs()


def softmax_base(ref, fp32):
    return torch.zeros_like(ref) if fp32 else ref * 2.0 ** -11 + 2.0 ** -25


def softmax_bound(ref, dist, fp32, kappa=None):
    kappa = (KAPPA_SM32 if fp32 else KAPPA_SM16) if kappa is None else kappa
    return softmax_base(ref, fp32) + kappa * 2.0 ** -24 * ref * dist


def emulate_softmax(x, mutant=None):
    """softmax_rows_kernel (fp16: a lane walks columns lane 8 + 512 k) or softmax_rows_f32_kernel (fp32: lane + 64 k)"""
    M, N = x.shape
    V = 8 if x.dtype == torch.float16 else 1
    W = 64 * V
    trips = (N + W - 1) // W
    xf = x.float()

    def lanes(v, fill):                                          # [M, N] -> [M, 64, trips V]: each lane's columns in order
        v = torch.cat([v, v.new_full((M, trips * W - N), fill)], 1)
        return v.reshape(M, trips, 64, V).permute(0, 2, 1, 3).reshape(M, 64, trips * V)

    live = torch.arange(N) < (W if mutant == "trip2" else N)     # "trip2": the second column trip dropped
    mx = torch.where(live, xf, _f32(-math.inf)).max(1, keepdim=True).values
    if mutant == "lanemax":                                      # the maximum of the lane's own columns, no butterfly
        lane_of = (torch.arange(N) // V) % 64
        mx = lanes(xf, -math.inf).max(2).values[:, lane_of]
    e = _expf(xf - mx) * live.float()
    s = _tree_sum(_seq_sum(lanes(e, 0.0), 2)).reshape(M, 1)
    p = (e * (1.0 / s)).to(x.dtype)
    return torch.where(live, p, x)


def softmax_case_ratios(M, N, fp32, kappas, mutant=None):
    ref, dist = softmax_reference(M, N, fp32)
    return worst_ratios(emulate_softmax(softmax_inputs(M, N, fp32), mutant), ref, softmax_base(ref, fp32), ref * dist, kappas)


# ------------------------------------------------------------------------------------------------ GEMV
@functools.lru_cache(maxsize=None)
def gemv_inputs(K, N):
    """x [K] fp32, W [N, K] fp16, bias, bias2 [N] fp32"""
    gen = torch.Generator().manual_seed(7000 + 3 * K + N)
    x = torch.randn(K, generator=gen) * 1.5
    W = (torch.randn(N, K, generator=gen) / math.sqrt(K)).half()
    return x, W, torch.randn(N, generator=gen), torch.randn(N, generator=gen)


@functools.lru_cache(maxsize=None)
def gemv_reference(case):
    """(ref, sum |act(x_k) W_nk| + |bias| + |bias2|) float64"""
    K, N, silu, b1, b2 = case
    x, W, bias, bias2 = gemv_inputs(K, N)
    xd = F.silu(x.double()) if silu else x.double()
    b = bias.double() * b1, bias2.double() * b2
    return W.double() @ xd + b[0] + b[1], W.double().abs() @ xd.abs() + b[0].abs() + b[1].abs()


def gemv_bound(mag, kappa=None):
    return (KAPPA_GEMV if kappa is None else kappa) * 2.0 ** -24 * mag


def emulate_gemv(x, W, bias, bias2, silu, mutant=None):
    """gemv_kernel: lane l walks k = 8 l + 512 j with eight FMAs each, butterfly, then the biases ("nomask": a lane past K / 8 adds the
    last vector again)"""
    N, K = W.shape
    trips = (K + 511) // 512
    xv = _silu_f(x) if silu else x
    prod = torch.cat([xv.reshape(1, K).expand(N, K).reshape(N, K // 8, 8), W.float().reshape(N, K // 8, 8)], 2)      # [N, K / 8, 16]
    pad = trips * 64 - K // 8
    if pad:
        prod = torch.cat([prod, prod[:, -1:].expand(N, pad, 16) if mutant == "nomask" else prod.new_zeros(N, pad, 16)], 1)
    prod = prod.reshape(N, trips, 64, 16).permute(1, 3, 0, 2)    # [trips, 16, N, 64]
    acc = torch.zeros(N, 64)
    for j in range(trips):
        for i in range(8):
            acc = _fma(prod[j, i], prod[j, 8 + i], acc)
    out = _tree_sum(acc)
    if bias is not None:
        out = out + bias
    if bias2 is not None and mutant != "nobias2":
        out = out + bias2
    return out


def gemv_case_ratios(case, kappas, mutant=None):
    K, N, silu, b1, b2 = case
    x, W, bias, bias2 = gemv_inputs(K, N)
    ref, mag = gemv_reference(case)
    return worst_ratios(emulate_gemv(x, W, bias if b1 else None, bias2 if b2 else None, silu, mutant), ref, torch.zeros_like(ref), mag, kappas)


# ------------------------------------------------------------------------------------------------ the emulation against the bounds
def _gn_all(kappas):
    return [gn_run_ratios(c, k, silu, eps, kappas) for c, k in GN_RUNS for silu, eps in GN_FLAVOURS]


OPERATIONS = {
    "GroupNorm": (lambda: KAPPA_GN, _gn_all),
    "LayerNorm": (lambda: KAPPA_LN, lambda ks: [ln_case_ratios(c, ks) for c in LN_CASES]),
    "GEGLU": (lambda: KAPPA_GEGLU, lambda ks: [geglu_case_ratios(c, ks) for c in GEGLU_CASES]),
    "softmax fp16": (lambda: KAPPA_SM16, lambda ks: [softmax_case_ratios(M, N, False, ks) for M, N, _ in SM16_CASES]),
    "softmax fp32": (lambda: KAPPA_SM32, lambda ks: [softmax_case_ratios(M, N, True, ks) for M, N in SM32_CASES]),
    "GEMV": (lambda: KAPPA_GEMV, lambda ks: [gemv_case_ratios(c, ks) for c in GEMV_CASES]),
}


def emulation_worst(op):
    """-> (kappa, worst ratio at kappa, worst ratio at kappa / 2, the smallest real kappa that would hold 0.5) over every case of op"""
    kappa, walk = OPERATIONS[op][0](), OPERATIONS[op][1]
    res = walk((kappa, kappa / 2))
    return kappa, max(r[0][0] for r in res), max(r[0][1] for r in res), max(r[1] for r in res)


@pytest.mark.parametrize("op", list(OPERATIONS))
def test_kappa_is_the_smallest_power_of_two(op):
    kappa, at, at_half, need = emulation_worst(op)
    print("%s: kappa = %g, worst emulation |err| / bound = %.3f (at kappa / 2: %.3f; 0.5 needs %.1f)" % (op, kappa, at, at_half, need))
    assert math.log2(kappa) == int(math.log2(kappa))
    assert at <= 0.5
    assert at_half > 0.5


def test_references_agree_with_torch():
    """the formulas behind slack (and behind the swapped-items check of the GPU file) are F.group_norm + F.silu; the references of the
    other operations are torch's float64 ops by construction, held here against the plain formulas"""
    for case in GN_SMALL_CASES[:4] + GN_PASS_CASES[2:6]:
        x, gamma, beta = gn_inputs(case)
        for silu, eps in GN_FLAVOURS:
            ref, _ = gn_reference(case, silu, eps)
            mine, _ = gn_formula64(x, *gn_stats64(x, case[4]), gamma, beta, eps, silu)
            assert (mine - ref).abs().max().item() <= 1e-9 * ref.abs().max().item()
    for case in ((5, 520, 1e-5), (17, 8, 1e-6)):
        x, gamma, beta = ln_inputs(case[0], case[1])
        xd = x.double()
        mean = xd.mean(1, keepdim=True)
        mine = (xd - mean) / (((xd - mean) ** 2).mean(1, keepdim=True) + case[2]).sqrt() * gamma.double() + beta.double()
        assert (mine - ln_reference(case)[0]).abs().max().item() <= 1e-9
    a, g = geglu_inputs((333, 96))
    mine = a.double() * 0.5 * g.double() * torch.special.erfc(-g.double() / math.sqrt(2.0))
    ref = geglu_reference((333, 96))[0]
    assert ((mine - ref).abs() <= 1e-14 * geglu_reference((333, 96))[1]).all()      # 1 + erf loses relative, not absolute, accuracy in the tail
    xd = softmax_inputs(5, 520, False).double()
    e = torch.exp(xd - xd.max(1, keepdim=True).values)
    assert (e / e.sum(1, keepdim=True) - softmax_reference(5, 520, False)[0]).abs().max().item() <= 1e-15


def test_inputs_are_what_the_docstring_says():
    for case in GN_SMALL_CASES[:4] + GN_PASS_CASES[2:]:
        x, _, _ = gn_inputs(case)
        B, G = case[0], case[4]
        mean, var = gn_stats64(x, G)
        live = torch.ones(B, G, dtype=torch.bool)
        live[B - 1, 1] = False
        assert (mean.abs() / var.sqrt())[live].max().item() <= 16.1
        assert mean[B - 1, 1].item() == -2.0 and var[B - 1, 1].item() == 0.0
        for kernel in ("pass", "small256") if gn_small_ok(*case) else ("pass",):      # the emulated variance clamps to exactly 0 there
            xf = x.float()
            s, q = _pass_sums(xf, G) if kernel == "pass" else _small_sums(xf, G, 256)
            n = _f32(case[3] * (case[1] + case[2]) // G)
            assert (s / n)[B - 1, 1].item() == -2.0 and (q / n)[B - 1, 1].item() == 4.0
    x, _, _ = ln_inputs(5, 1024)
    xd = x.double()
    assert 900 < (xd[2].mean() / xd[2].std()).item() < 1100
    _, g = geglu_inputs((333, 96))
    assert 0.25 <= ((g.float() >= -6) & (g.float() <= -3)).float().mean().item() < 0.35      # the quarter drawn there, and N(0, 4)'s own 6 %


def test_gelu_tail_is_reported():
    rel, ulps, at, e_min, e_max = gelu_tail()
    print("gelu_f on [-6, -3]: worst relative error %.3e, worst %.2f fp16 ulps of the result at g = %g; |g| E is %.0f %% .. %.0f %% of the bound"
          % (rel, ulps, at, 100 * e_min, 100 * e_max))
    g = torch.arange(-6.0, -3.0 + 2.0 ** -9, 2.0 ** -9).half().unique()
    ref = F.gelu(g.double())      # the published error of the approximation, and fp32 arithmetic on top of it
    assert ((gelu_f(g.float()).double() - ref).abs() <= g.double().abs() * E_AS + 2.0 ** -20 * ref.abs()).all()


def _first_caught(ratios):
    for where, r in ratios:
        if r > 1.0:
            return where
    return None


@pytest.mark.parametrize("mutant", list(GN_MUTANTS))
def test_gn_mutant_exceeds_the_bound(mutant):
    """each mistake breaks the bound on some element of some case (the cases of the kernels it can be made in, in order)"""
    runs = ((c, k) for c, k in GN_RUNS if k in GN_MUTANTS[mutant])
    caught = _first_caught(((c, k), gn_run_ratios(c, k, 1, 1e-5, (KAPPA_GN,), mutant)[0][0]) for c, k in runs)
    print("GroupNorm mutant %s: caught on %s" % (mutant, caught))
    assert caught is not None, "mutant %s stays within the bound on every case" % mutant


@pytest.mark.parametrize("mutant", LN_MUTANTS)
def test_ln_mutant_exceeds_the_bound(mutant):
    assert _first_caught((c, ln_case_ratios(c, (KAPPA_LN,), mutant)[0][0]) for c in LN_CASES) is not None


def test_ln_one_pass_variance_leaves_the_bound_on_the_high_mean_row():
    """row 2 (mean 100, std 0.1): the two-pass kernel is within half its bound there, E[x^2] - mean^2 far outside"""
    case = (5, 1024, 1e-5)
    ref, slack = ln_reference(case)
    bound = ln_bound(ref, slack)
    x, gamma, beta = ln_inputs(5, 1024)
    two = ((emulate_ln(x, gamma, beta, 1e-5).double() - ref).abs() / bound)[2].max().item()
    one = ((emulate_ln(x, gamma, beta, 1e-5, "onepass").double() - ref).abs() / bound)[2].max().item()
    print("LayerNorm, |mean| / std = 1000 row: two-pass ratio %.3f, one-pass ratio %.1f" % (two, one))
    assert two <= 0.5 and one > 1.0


@pytest.mark.parametrize("mutant", GEGLU_MUTANTS)
def test_geglu_mutant_exceeds_the_bound(mutant):
    assert _first_caught((c, geglu_case_ratios(c, (KAPPA_GEGLU,), mutant)[0][0]) for c in GEGLU_CASES[:3]) is not None


@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("mutant", SM_MUTANTS)
def test_softmax_mutant_exceeds_the_bound(mutant, fp32):
    cases = [(M, N) for M, N in SM32_CASES] if fp32 else [(M, N) for M, N, _ in SM16_CASES]
    kappa = KAPPA_SM32 if fp32 else KAPPA_SM16
    assert _first_caught(((M, N), softmax_case_ratios(M, N, fp32, (kappa,), mutant)[0][0]) for M, N in cases) is not None


@pytest.mark.parametrize("mutant", GEMV_MUTANTS)
def test_gemv_mutant_exceeds_the_bound(mutant):
    assert _first_caught((c, gemv_case_ratios(c, (KAPPA_GEMV,), mutant)[0][0]) for c in GEMV_CASES) is not None


if __name__ == "__main__":      # the table of the docstring
    for op_ in OPERATIONS:
        print("%-14s kappa = %-8g worst emulation |err| / bound = %.3f  (%.3f at kappa / 2; 0.5 needs %.1f)" % ((op_,) + emulation_worst(op_)))
    print("gelu_f tail: rel %.3e, %.2f ulps at g = %g, E share %.3f .. %.3f" % gelu_tail())
