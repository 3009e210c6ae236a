"""Where the tolerances of tests/test_gpu_attn_instances.py come from: a torch emulation, on the CPU, of what each family of attention
forward kernels computes (csrc/attn.hip), held against float64 softmax attention of the same fp16 inputs, and the per-element bound for O
and the per-query bound for the log-sum-exp that the GPU tests apply unchanged.

What is emulated
    plain  (attn_flash_kernel<DP, PF>, attn_flash_dma64_kernel<., ., false>): 64-key tiles; fp32 scores S = q k^T; per tile the maximum, and
           the deferred rescale -- the running reference m only moves to max(m, tile max) when (tile max - m) c > 8 for some query of the
           wavefront (32 consecutive queries decide together, as __any does), c = fp32(scale * log2 e); P = exp2(fma(S, c, -m c)) in fp32;
           l += sum P (the UNROUNDED P); P rounded to fp16; O += P V in fp32; at the end one fp16 rounding of O * (1 / l) and
           lse = m c + log2 l.  causal: key j > query i scores -inf.
    aug    (attn_flash_dma64_kernel<., 3, true>): Q' = fp16(fp32(q) c); the reference point m is an fp16 value, 0 at the start, carried in
           Q's column dh against the 1.0 in K's, so S' = Q' k^T - m comes out of the matrix pipe; the first tile always moves m (to
           fp16(tile max)), later tiles when the tile max is more than 8 above it; P = fp16(exp2(S')); O += P V and l += sum P with the
           ROUNDED P (V^T's row of ones); O / l rounded once; lse = m + log2 l.
    cross  (attn_cross_edit_kernel, the source row): one pass over <= 96 keys, P = exp2((S - max) c) / sum in fp32, rounded to fp16,
           O = P V rounded once.
The emulation uses torch's fp32 matmul on the CPU, not the MFMA's summation order, and torch's exp2 / log2, not v_exp_f32 / v_log_f32.

The bound for O.  u = 2^-11 (half an fp16 ulp, relative).  p_ij is the float64 softmax, ref = sum_j p_ij v_jd,
A = sum_j p_ij |v_jd|,  Ac = sum_j p_ij |v_jd - ref_id|,  L_i = sum_j 2^(c (s_ij - max_j s_ij)) >= 1.
    (1) the one rounding of the output: u |ref| (+ 2^-24, the spacing of fp16 subnormals, as an absolute floor);
    (2) P rounded to fp16, relative error <= u on every term of the numerator.  plain / cross: the denominator is not touched, so the
        error is <= u A.  aug: numerator and denominator carry the same factors (1 + e_j), which changes O by
        sum_j p_j e_j (v_j - O) / (1 + sum_j p_j e_j): <= u Ac to first order (a constant V is reproduced exactly);
    (3) P below fp16's normal range: absolute error <= 2^-25 per key in the kernel's units, in which the row sum is l = L 2^(c (max - m))
        >= L because m <= max and max - m <= 8 / c.  <= Nk 2^-25 max_j |v_jd| / L   (cross: P is normalised before the rounding, L = 1);
    (4) a perturbation of the scores by at most delta_ij in the log2 domain multiplies term j by 2^(+-delta_ij) in numerator and
        denominator alike: |dO| <= sum_j p_j eta_j |v_j - ref| / (1 - sum_j p_j eta_j), eta_j = 2^delta_ij - 1 -- delta weighted by p, and
        by how far v_j is from the output, not its maximum over the keys.  delta has two parts:
          acc: the fp32 accumulation of S (Dp / 16 dependent MFMA steps), the rounding of c and of the exponent's fma:
               (Dp / 16 + 2) 2^-24 c sum_d |q_id k_jd|;
          q2 (aug only): the second rounding of Q, u c sum_d |q_id k_jd|.
    bound_O = MARGIN * [(1) + (2) + (3) + (4)] + 2^-24,   (1) + (2) = u |ref| + u (A or Ac)
(1) - (4) are worst cases (to first order in u), so the emulation cannot exceed 1 / MARGIN of the bound except through what the
derivation leaves out (second-order terms, the fp32 roundings of l, alpha and 1 / l).  MARGIN = 2 is the one constant chosen from the emulation (the operation counts in delta and in the lse bound -- Dp / 16 + 2,
36 + Nk / 64 + 4, 8 + log2 Nk -- are counted by hand from the kernels' code): the emulation has to
stay at or below half the bound, and the other half is left for the device.  On a row that one key dominates the plain bound is
4 u |ref| (the two roundings can add up to 2 u |ref|), the aug bound 2 u |ref| (its P rounding cancels there).

The bound for lse (absolute, log2 domain; ref = log2 sum_j 2^(c s_ij) in float64, M = c max_j s_ij):
    score perturbation: sum_j p_j delta_ij (d lse / d s_j = c p_j), delta as in (4), plus the fma's own rounding 2^-24 (8 + M - c s_ij);
    l: fp32 sum of Nk terms in 32-term lane chains, one add per tile, one across the half-waves, and exp2 to 2 ulp:
       log2 e (36 + Nk / 64 + 4) 2^-24 relative to l;
    m c + log2 l: 2^-23 (|M| + 8) for c and the product, 2^-23 (8 + log2 Nk) for v_log_f32 at 1 ulp and its argument, 2^-24 |ref| for the add;
    aug: l is summed from the rounded P: + u log2 e;  cross: no lse.
    bound_lse = MARGIN * (all of the above)

Worst |got - ref| / bound of the EMULATION over this file's cases (NQ = 130 queries, five seeds, input std 1 and 3, the constructed rows
of hostile_rows included), as the tests below print them:

    family   shapes (Nk; dh / Dp)                                     worst O ratio    worst lse ratio
    plain    65, 129; 8/32 40/64 80/96 128/128 160/160                0.35 - 0.42      0.12 - 0.18
    dma      128, 192; 40/64 64/64                                    0.35 - 0.37      0.15 - 0.26
    aug      128, 192; 40/64                                          0.44 - 0.45      0.16 - 0.17
    causal   Nq = Nk = 77, 130, 200; 64/64 8/32 (and 128; 40/64)      0.32 - 0.43      0.10 - 0.20
    cross    8, 77, 96; 40/64 160/160                                 0.39 - 0.43      -

MEASURED below holds these figures rounded up to the next 0.05, and the tests assert them as ceilings (never above 0.5).  The GPU tests
apply bound_O and bound_lse unchanged: the factor MARGIN over the worst case of the emulation is left for v_exp_f32 / v_log_f32 and the
MFMA's summation order.

What the bound does not see.  At input std 3 the aug form's term (4) (eta about 0.03 per
key) makes bound_O 13 times (median; at most 64 times) the rounding terms (1) + (2), and the emulation still uses 0.45 of it -- the
second rounding of Q really costs that much -- so on those cases an error below about ten u |v - ref| in one element is not seen; at
input std 1 the factor is 5, and for the plain form 1 (median).  The far query of hostile_rows (|q k| summing to 24 in the log2 domain)
has the same wide bound in the aug form: the kernel sits at 0.004 of it on the device, an aug form without the first move down at 3.
ratio() refuses a bound that is not positive (term (4)'s denominator 1 - sum_j p_j eta_j would have to reach 0: eta of order 1, scores
of order 2^11 in the log2 domain)."""
import math

import pytest
import torch

U = 2.0 ** -11
LOG2E = 1.44269504088896340736
MARGIN = 2.0
KV_TILE = 64
NQ = 130                  # one full 128-query workgroup plus two queries
SEEDS = (0, 1, 2, 3, 4)

# worst emulated ratios per family (O, lse), recorded when the bound was written; asserted as ceilings below
MEASURED = {"plain": (0.45, 0.20), "dma": (0.40, 0.30), "aug": (0.50, 0.20), "causal": (0.45, 0.25), "cross": (0.45, None)}


def c32(scale):
    """the kernels' c = scale * log2(e), both fp32, product rounded to fp32"""
    return torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)


def _wave_any(flag):
    """[..., Nq] bool -> the same, true where any of the 32 consecutive queries of the wavefront is (queries past Nq never ask for a move
    after the first tile, where every lane moves anyway)"""
    n = flag.shape[-1]
    pad = (-n) % 32
    f = torch.cat([flag, flag.new_zeros(*flag.shape[:-1], pad)], -1).reshape(*flag.shape[:-1], -1, 32)
    return f.any(-1, keepdim=True).expand_as(f).reshape(*flag.shape[:-1], -1)[..., :n]


def emulate(q, k, v, scale, form="plain", causal=False, aug_first_move_down=True):
    """q [..., Nq, d], k / v [..., Nk, d] fp16 -> (O fp16 [..., Nq, d], lse fp32 [..., Nq] or None): the kernels' arithmetic in torch.
    aug_first_move_down = False is NOT the kernel: the aug form with a first tile that moves the reference point only upwards, for
    test_far_query_needs_the_first_move_down."""
    assert q.dtype == k.dtype == v.dtype == torch.float16 and form in ("plain", "aug", "cross")
    f32 = torch.float32
    c = c32(scale)
    Nq, Nk = q.shape[-2], k.shape[-2]
    lead = q.shape[:-2]
    if form == "cross":
        s = q.float() @ k.float().transpose(-1, -2)
        e = torch.exp2((s - s.amax(-1, keepdim=True)) * c)
        p = e * (1.0 / e.sum(-1, keepdim=True))
        o = p.half().float() @ v.float()
        assert o.dtype == f32
        return o.half(), None
    aug = form == "aug"
    qf = (q.float() * c).half().float() if aug else q.float()
    O = torch.zeros(*lead, Nq, v.shape[-1], dtype=f32)
    l = torch.zeros(*lead, Nq, dtype=f32)
    mrun = torch.zeros(*lead, Nq, dtype=f32) if aug else torch.full((*lead, Nq), -math.inf, dtype=f32)
    qi = torch.arange(Nq)
    for it, kv0 in enumerate(range(0, Nk, KV_TILE)):
        kt, vt = k[..., kv0:kv0 + KV_TILE, :].float(), v[..., kv0:kv0 + KV_TILE, :].float()
        s = qf @ kt.transpose(-1, -2)
        if aug:
            s = s - mrun[..., None]                      # column dh: (-m) * 1.0 in the same fp32 accumulation
        if causal:
            kj = kv0 + torch.arange(kt.shape[-2])
            s = s.masked_fill(kj[None, :] > qi[:, None], -math.inf)
        mloc = s.amax(-1)
        if aug:
            first = it == 0
            anyg = _wave_any((mloc > 8.0) | first)
            target = mrun + torch.where((mloc > 0.0) | (first and aug_first_move_down), mloc, torch.zeros_like(mloc))
            mnew = torch.where(anyg, target.half().float(), mrun)
            delta = mnew - mrun
            alpha = torch.exp2(-delta)
            O, l, mrun = O * alpha[..., None], l * alpha, mnew
            ph = torch.exp2(s - delta[..., None]).half()
            l = l + ph.float().sum(-1)
        else:
            anyg = _wave_any((mloc - mrun) * c > 8.0)
            mnew = torch.where(anyg, torch.maximum(mrun, mloc), mrun)
            alpha = torch.where(anyg, torch.exp2((mrun - mnew) * c), torch.ones_like(mrun))
            O, l, mrun = O * alpha[..., None], l * alpha, mnew
            mc = mrun * c
            p = torch.exp2((s.double() * c.double() - mc.double()[..., None]).float())      # one fma: the exact result rounded once
            l = l + p.sum(-1)
            ph = p.half()
        O = O + ph.float() @ vt
    assert O.dtype == f32 and l.dtype == f32
    o = (O * (1.0 / l)[..., None]).half()
    lse = (mrun if aug else mrun * c) + torch.log2(l)
    return o, lse


def reference(q, k, v, scale, causal=False):
    """float64 softmax attention of the fp16 values -> (ref O, ref lse in the log2 domain, p, c s); scale as the fp32 value the kernel gets"""
    cs = (q.double() @ k.double().transpose(-1, -2)) * (float(torch.tensor(scale, dtype=torch.float32)) * LOG2E)
    if causal:
        Nq, Nk = cs.shape[-2:]
        cs = cs.masked_fill(torch.ones(Nq, Nk, dtype=torch.bool, device=cs.device).triu(1), -math.inf)
    M = cs.amax(-1, keepdim=True)
    e = torch.exp2(cs - M)
    L = e.sum(-1, keepdim=True)
    p = e / L
    return p @ v.double(), (M + torch.log2(L))[..., 0], p, cs


def bounds(q, k, v, scale, form, Dp, causal=False):
    """-> (ref O, bound O, ref lse, bound lse): functions of the inputs and the float64 reference only (the docstring's derivation).
    Runs on the device of its inputs."""
    assert form in ("plain", "aug", "cross")
    ref, lse, p, cs = reference(q, k, v, scale, causal)
    Nk = k.shape[-2]
    c = float(torch.tensor(scale, dtype=torch.float32)) * LOG2E
    vd = v.double()
    M = cs.amax(-1, keepdim=True)
    L = torch.exp2(cs - M).sum(-1, keepdim=True)
    absqk = c * (q.double().abs() @ k.double().abs().transpose(-1, -2))
    delta = (Dp // 16 + 2) * 2.0 ** -24 * absqk
    if form == "aug":
        delta = delta + U * absqk
    dist = (vd[..., None, :, :] - ref[..., :, None, :]).abs()                  # [..., Nq, Nk, d]: |v_jd - ref_id|
    A = p @ vd.abs()
    Ac = (p[..., None] * dist).sum(-2)
    w = p * (torch.exp2(delta) - 1.0)
    t4 = (w[..., None] * dist).sum(-2) / (1.0 - w.sum(-1, keepdim=True))
    t3 = Nk * 2.0 ** -25 * vd.abs().amax(-2, keepdim=True) / (1.0 if form == "cross" else L)
    bo = MARGIN * (U * ref.abs() + U * (Ac if form == "aug" else A) + t3 + t4) + 2.0 ** -24
    if form == "cross":
        return ref, bo, None, None
    arg = torch.where(p > 0, 8.0 + M - cs, torch.zeros_like(cs))                # masked keys carry no weight
    bl = (p * (delta + 2.0 ** -24 * arg)).sum(-1)
    bl = bl + LOG2E * (36 + Nk / 64.0 + 4) * 2.0 ** -24
    bl = bl + 2.0 ** -23 * (M[..., 0].abs() + 8.0) + 2.0 ** -23 * (8.0 + math.log2(Nk)) + 2.0 ** -24 * lse.abs()
    if form == "aug":
        bl = bl + U * LOG2E
    return ref, bo, lse, MARGIN * bl


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound, in float64 (NaN counts as infinite)"""
    assert (bound > 0).all(), "a bound that is not positive checks nothing (the score term's denominator reached 0?)"
    r = (got.double() - ref).abs() / bound
    return float("inf") if torch.isnan(r).any() else r.max().item()


def attn_inputs(Nq, Nk, dh, std, seed):
    """q [Nq, dh], k / v [Nk, dh] fp16, N(0, std^2) (v: N(0, 1)): flat rows at std 1, peaked ones at std 3"""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(Nq, dh, generator=g) * std).half()
    k = (torch.randn(Nk, dh, generator=g) * std).half()
    v = torch.randn(Nk, dh, generator=g).half()
    return q, k, v


# the constructed queries of hostile_rows: their indices
Q_ZERO, Q_RISE, Q_FALL, Q_SPIKE, Q_FAR = 0, 3, 37, 70, 9


def hostile_rows(q, k, v, scale):
    """rows built to move (or not to move) the running reference, in place on fp16 q / k [N, dh]:
      Q_ZERO   a zero query: every score 0, the output is the mean of V;
      Q_RISE   a query whose logits rise by 10 (log2 domain, > 8) from each 64-key tile to the next: a move on every tile;
      Q_FALL   the same falling: the maximum is in tile 0, no move after it;
      Q_SPIKE  three times the LAST key (a ragged last tile's final key when Nk % 64 != 0): that key has a large weight, at dh >= 40 the
               row's largest;
      Q_FAR    far from EVERY key: all its scores are below -8 in the log2 domain (about -24 +- 3), in every tile.  The aug form computes
               the first tile against the reference point 0, where such a row's P (2^-21 ... 2^-27) would be fp16 subnormals of one to four
               bits or flush to zero; it is right only if the first tile moves the reference point DOWN to the tile's (negative) maximum.  The row has to
               be low in every tile: if later tiles scored near 0 they would carry the row, and a lost first move would not show.
    The rise rides on the last head dimension: k's is the tile index times 2.5 / c, every other query's is 0.  The far query rides on the
    one before: k's is 6 / c for every key, the far query's is -4 (its other dimensions are a random query's, halved), every other query's
    is 0."""
    Nk, dh = k.shape
    c = float(c32(scale))
    q[Q_ZERO] = 0
    q[Q_RISE] = 0
    q[Q_FALL] = 0
    q[Q_SPIKE] = (3.0 * k[Nk - 1].float()).half()
    q[Q_FAR] = (0.5 * q[Q_FAR].float()).half()
    k[:, dh - 1] = ((torch.arange(Nk) // KV_TILE).double() * (2.5 / c)).half()
    k[:, dh - 2] = 6.0 / c
    q[:, dh - 2:] = 0
    q[Q_RISE, dh - 1] = 4.0
    q[Q_FALL, dh - 1] = -4.0
    q[Q_FAR, dh - 2] = -4.0
    return q, k, v


# (Nk, dh, Dp) per family: the shapes of tests/test_gpu_attn_instances.py
PLAIN_SHAPES = [(nk, dh, dp) for nk in (65, 129) for dh, dp in ((8, 32), (40, 64), (80, 96), (128, 128), (160, 160))]
DMA_SHAPES = [(nk, dh, 64) for nk in (128, 192) for dh in (40, 64)]
AUG_SHAPES = [(128, 40, 64), (192, 40, 64)]
CAUSAL_SHAPES = [(n, dh, dp) for n in (77, 130, 200) for dh, dp in ((64, 64), (8, 32))] + [(128, 40, 64)]
CROSS_SHAPES = [(nk, dh, dp) for nk in (8, 77, 96) for dh, dp in ((40, 64), (160, 160))]
# (Nk, dh, Dp, aug, perm): the launches of the GPU file's test_rows_that_move_the_running_reference
HOSTILE_SHAPES = [(65, 40, 64, 0, 0), (129, 8, 32, 0, 0), (200, 80, 96, 0, 0), (129, 160, 160, 0, 0), (192, 40, 64, 0, 0), (192, 40, 64, 1, 1),
                  (192, 64, 64, 0, 1)]


def _worst(form, shapes, causal=False, hostile=True):
    wo, wl = 0.0, 0.0
    for Nk, dh, Dp in shapes:
        Nq = Nk if causal else NQ
        scale = dh ** -0.5
        variants = [(std, False) for std in (1.0, 3.0)] + ([(1.0, True)] if hostile and form != "cross" and not causal else [])
        so, sl = 0.0, 0.0
        for std, host in variants:
            for seed in SEEDS:
                q, k, v = attn_inputs(Nq, Nk, dh, std, 100 * seed + Nk + dh)
                if host:
                    hostile_rows(q, k, v, scale)
                o, lse = emulate(q, k, v, scale, form, causal)
                ref, bo, rl, bl = bounds(q, k, v, scale, form, Dp, causal)
                so = max(so, ratio(o, ref, bo))
                if lse is not None:
                    sl = max(sl, ratio(lse, rl, bl))
        print("%s%s Nk %d dh %d Dp %d: worst O ratio %.3f, worst lse ratio %.3f" % (form, " causal" if causal else "", Nk, dh, Dp, so, sl))
        wo, wl = max(wo, so), max(wl, sl)
    return wo, wl


@pytest.mark.parametrize("family,form,shapes,causal", [("plain", "plain", PLAIN_SHAPES, False), ("dma", "plain", DMA_SHAPES, False),
                                                       ("aug", "aug", AUG_SHAPES, False), ("causal", "plain", CAUSAL_SHAPES, True),
                                                       ("cross", "cross", CROSS_SHAPES, False)])
def test_emulation_leaves_half_the_bound(family, form, shapes, causal):
    wo, wl = _worst(form, shapes, causal)
    print("%s: worst O ratio %.3f, worst lse ratio %.3f" % (family, wo, wl))
    co, cl = MEASURED[family]
    assert wo <= co <= 0.5, (family, wo)
    if cl is not None:
        assert wl <= cl <= 0.5, (family, wl)


def test_emulation_moves_the_reference_where_the_rows_are_built_to():
    """the constructed rows do what they are for: the rising query is exact only if every tile rescales, the zero query gives mean(V),
    the spiked query gives the last key's V, and every score of the far query is below -8 in the log2 domain"""
    Nk, dh = 192, 40
    scale = dh ** -0.5
    q, k, v = hostile_rows(*attn_inputs(NQ, Nk, dh, 1.0, 7), scale)
    for form in ("plain", "aug"):
        o, lse = emulate(q, k, v, scale, form)
        ref, bo, rl, bl = bounds(q, k, v, scale, form, 64)
        assert ratio(o, ref, bo) <= 0.5 and ratio(lse, rl, bl) <= 0.5
        assert ratio(o[Q_FAR], ref[Q_FAR], bo[Q_FAR]) <= 0.5 and ratio(lse[Q_FAR], rl[Q_FAR], bl[Q_FAR]) <= 0.5
        assert (o[Q_ZERO].double() - v.double().mean(0)).abs().max() <= 2 * U * v.double().abs().mean(0).max() + 2.0 ** -24
        assert (o[Q_SPIKE].double() - v[Nk - 1].double()).abs().max() <= bo[Q_SPIKE].max()
    cs = reference(q, k, v, scale)[3]
    tile_max = torch.stack([cs[:, t * 64:(t + 1) * 64].amax(-1) for t in range(3)], -1)
    assert ((tile_max[Q_RISE, 1:] - tile_max[Q_RISE, :-1]) > 8).all() and ((tile_max[Q_FALL, 1:] - tile_max[Q_FALL, :-1]) < -8).all()
    assert (cs[Q_FAR] < -8).all()


@pytest.mark.parametrize("Nk,dh,Dp,aug,perm", HOSTILE_SHAPES)
def test_far_query_is_below_minus_eight_at_every_shape_the_gpu_runs(Nk, dh, Dp, aug, perm):
    """at the shapes and seeds of the GPU file's hostile cases (two heads: seeds 17000, 17001): every score of the far query, the whole
    first tile included, is below -8 in the log2 domain, and the far column leaves the zero query's scores at 0"""
    scale = dh ** -0.5
    for seed in (17000, 17001):
        q, k, v = hostile_rows(*attn_inputs(NQ, Nk, dh, 1.0, seed), scale)
        cs = reference(q, k, v, scale)[3]
        print("Nk %d dh %d seed %d: far query's scores (log2 domain) %.2f ... %.2f" % (Nk, dh, seed, cs[Q_FAR].min(), cs[Q_FAR].max()))
        assert cs[Q_FAR].max() < -8 and cs[Q_FAR, :KV_TILE].max() < -8
        assert (cs[Q_ZERO] == 0).all()


def test_far_query_needs_the_first_move_down():
    """what the far query is for: an aug form whose first tile moves the reference point only upwards (emulate's aug_first_move_down =
    False, not the kernel) leaves that row's P in fp16's subnormal range, where most of it is lost; the row then breaks the per-element
    bound (by a factor of 3: the row is off by 13 %, and its bound is wide through the score term of its large |q k|), and no other row
    notices"""
    Nk, dh = 192, 40
    scale = dh ** -0.5
    q, k, v = hostile_rows(*attn_inputs(NQ, Nk, dh, 1.0, 7), scale)
    ref, bo, rl, bl = bounds(q, k, v, scale, "aug", 64)
    o, lse = emulate(q, k, v, scale, "aug", aug_first_move_down=False)
    others = torch.arange(NQ) != Q_FAR
    far = ratio(o[Q_FAR], ref[Q_FAR], bo[Q_FAR])
    l2 = ((o.double() - ref).norm() / ref.norm()).item()
    print("first move only upwards: far query's O ratio %.1f, the other rows' %.3f, rel-L2 %.2e" % (far, ratio(o[others], ref[others], bo[others]), l2))
    assert far > 2 and ratio(o[others], ref[others], bo[others]) <= 0.5


def test_bound_notices_one_query_that_lost_its_last_key():
    """what the per-element bound is for: one query of 2048 computed without the last key of the ragged tile passes a whole-tensor
    relative L2 of 3e-3 and breaks the per-element bound (and the lse bound) by more than an order of magnitude"""
    Nq, Nk, dh, row = 2048, 129, 40, 777
    scale = dh ** -0.5
    q, k, v = attn_inputs(Nq, Nk, dh, 1.0, 11)
    ref, bo, rl, bl = bounds(q, k, v, scale, "plain", 64)
    o, lse = emulate(q, k, v, scale)
    assert ratio(o, ref, bo) <= 0.5 and ratio(lse, rl, bl) <= 0.5
    o1, lse1 = emulate(q[row:row + 1], k[:Nk - 1], v[:Nk - 1], scale)
    o[row], lse[row] = o1[0], lse1[0]
    l2 = ((o.double() - ref).norm() / ref.norm()).item()
    print("one query without its last key: rel-L2 %.2e, O ratio %.1f, lse ratio %.1f" % (l2, ratio(o, ref, bo), ratio(lse, rl, bl)))
    assert l2 < 3e-3 and ratio(o, ref, bo) > 10 and ratio(lse, rl, bl) > 10
