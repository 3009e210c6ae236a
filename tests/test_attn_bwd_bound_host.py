"""Where the tolerances of tests/test_gpu_attn_bwd_instances.py come from: the plan of the attention backward's dispatch
(pnpi_attn_bwd_plan_query, host only), a torch emulation, on the CPU, of what attn_bwd_flash_kernel (csrc/attn.hip) and the materialised
fallback (csrc/api_backward.inc) compute, held against float64 autograd of softmax(scale q k^T) v on the same fp16 inputs, and the
per-element bounds for dq, dk and dv that the GPU tests apply unchanged.

What is emulated
    two_pass  attn_bwd_flash_kernel without the forward's hand-over.  Tiles of LT loop rows (64; 32 at Dp 160); fp32 S = q k^T and
              dP = dO v^T.  dQ pass 1: plain running maximum m (it moves on every tile that raises it: no deferred rescale here),
              alpha = exp2((m - m') c), pv = exp2(fma(S, c, -m' c)), l = fma(l, alpha, sum pv), d = fma(d, alpha, sum pv dP);
              lse2 = m c + log2 l, D = d / l.  Every launch then: P = exp2(fma(S, c, -lse2)) in fp32; dS = P (dP - D) rounded to fp16
              (dV: P rounded to fp16); fp32 accumulation over the loop tiles; ONE fp16 rounding of acc * scale (dV: of acc).
              A split dK / dV walk (cross-attention, Nq >= 256): every share accumulates its own whole tiles, writes acc * scale in fp32,
              and attn_bwd_reduce_kernel adds the shares in order and rounds once.
    one_pass  the same with lse2 taken from the forward kernel (test_attn_bound_host.emulate, plain form) and
              D = sum_d fp32(dO) fp32(O_fp16), O the forward's fp16 output.
    materialised  S = fp32(scale * q k^T) from the GEMM, fp32 softmax (max, exp, sum, times 1 / sum), dP fp32, D = sum P dP from the fp32 P,
              P and scale P (dP - D) rounded to fp16, three GEMMs with fp32 accumulation and one rounding.
The emulation uses torch's fp32 matmul on the CPU, not the MFMA's summation order, and torch's exp2 / log2.  The register-prefetch
instances (PF) differ from their twins in staging only: the same emulation.

The bounds.  u = 2^-11.  In float64: c = scale log2 e, p = softmax, dp = dO v^T, D_i = sum_j p_ij dp_ij, ds = p (dp - D) (without the
scale), dq = scale ds k, dk = scale ds^T q, dv = p^T dO.  The computed ds_ij is P^ (dP^ - D^) with
    P^ = p 2^(+-(delta_ij + eps_i)) (1 + 6 * 2^-24):  delta_ij = (Dp / 16 + 2) 2^-24 c sum_d |q_id k_jd| for the fp32 accumulation of S
         (Dp / 16 dependent MFMA steps), the rounding of c and of the fma's product, plus 2^-24 |c s_ij - lse_i| for the fma's own
         rounding; eps_i the error of lse2; 6 * 2^-24 for exp2 (2 ulp), the subtraction and the product.  lse2 is FIXED when P is
         formed, so nothing self-normalises: the relative error eta_ij = 2^(delta_ij + eps_i) - 1 + 6 * 2^-24 weighs the summand
         |ds_ij| itself, not its distance from the output;
    dP^: e_dp_ij = (Dp / 16) 2^-24 sum_d |dO_id v_jd|;
    D^:  e_D_i (below), which enters every key of the row with weight p_ij: the cancellation term e_D scale sum_j p_ij |k_jd|.
so, before the fp16 rounding, |ds^ - ds| <= W_ij = eta_ij |ds_ij| + p_ij (e_dp_ij + e_D_i), and the rounding adds u |ds_ij|, or 2^-25
where ds is below fp16's normal range.  With the fp32 accumulation over the loop rows (n / 16 MFMA steps, the scale, and for a split walk
one add per share: (n / 16 + nsplit + 2) 2^-24 of sum |ds| |operand|) and the one output rounding:
    bound_dq = MARGIN [u |dq| + scale (u |ds| + W) |k| + scale Nk 2^-25 max_j |k_jd| + (Nk / 16 + 3) 2^-24 scale |ds| |k|] + EXT + 2^-24
    bound_dk = the same with (.)^T |q|, Nq loop rows and nsplit shares
    bound_dv = MARGIN [u |dv| + (u p + eta p)^T |dO| + Nq 2^-25 max_i |dO_id| + (Nq / 16 + nsplit + 2) 2^-24 p^T |dO|] + EXT + 2^-24
(|ds| |k| etc. are matrix products: nothing of shape [Nq, Nk, d] is formed).  eps and e_D depend on the form:
    two_pass  eps_i = sum_j p_ij (delta0_ij) + log2 e (LT / 2 + 4 Nk / LT + 4) 2^-24 + 2^-23 |M_i| + 2^-23 (1 + log2 Nk) + 2^-24 |lse_i|,
              delta0 the score perturbation with the fma's rounding taken against the running maximum (2^-24 (M_i - c s_ij)); l is a
              chain of LT / 2 adds per lane and tile, one fma, alpha (exp2, 2 ulp) and their product per tile, one add across the
              half-waves; then c and the product m c, v_log_f32 at 1 ulp, and the add.
              e_D_i = sum_j p_ij (2^delta0_ij - 1) |dp_ij - D_i| / (1 - sum_j p_ij (2^delta0_ij - 1)) + sum_j p_ij e_dp_ij
                      + (LT / 2 + 4 Nk / LT + 6) 2^-24 sum_j p_ij |dp_ij|
              (d / l IS self-normalising: a common factor of numerator and denominator cancels, so the first term weighs the distance
              |dp - D|).  Everything is the kernel's own and stands inside MARGIN; EXT = 0.
    one_pass  eps_i = bound_lse_i and e_D_i = sum_d |dO_id| bound_O_id + (Dp / 2 + 1) 2^-24 sum_d |dO_id O_id|, bound_lse and bound_O those
              of test_attn_bound_host.bounds() for the forward's plain form, imported and used whole: they are what the forward kernel is
              allowed on the device, so their share of W is the term EXT, outside MARGIN; the fma chain of D (Dp / 2 terms per half-wave and
              one add) is the kernel's own and inside.  Because bound_O is wide against one more rounding of O (MARGIN and the P term make
              it at least 4 u |O|), the gradients' bounds cannot tell whether D was formed from the O that was handed over: D itself,
              which the launch leaves in its workspace, is held by bound_D_one_pass against that very O.
    materialised  the softmax normalises with its own sum: P^ = p (1 + eta), eta_ij = 2^(dm_ij + sum_j p_ij dm_ij) - 1 + (Nk / 64 + 12) 2^-24,
              dm_ij = (Dp / 16 + 3) 2^-24 c sum_d |q k| + 2 * 2^-24 (M_i - c s_ij) (GEMM, alpha, __expf's product; the subtraction and
              the product's rounding);  e_D_i = sum_j p_ij eta_ij |dp_ij| + sum_j p_ij e_dp_ij + (Nk / 64 + 8) 2^-24 sum_j p_ij |dp_ij| (P^ does
              not sum to one exactly, so |dp| and not |dp - D|); the scale is applied BEFORE the fp16 rounding, so the subnormal term
              is n 2^-25 max |operand| without it; (n / 16 + 8) 2^-24 for the GEMM's accumulation.  dv is bounded with the same form
              argument as dq and dk (its P depends on which lse the launch read).
MARGIN = 2 is the one chosen constant (the operation counts are counted by hand from the kernels' code): the emulation has to stay at or
below half of every bound, the other half is left for v_exp_f32 / v_log_f32 and the MFMA's summation order.

Worst |got - ref| / bound of the EMULATION over this file's cases (five seeds, input std 1 and 3, the constructed rows of hostile_rows and
hostile_do_rows), as test_emulation_leaves_half_the_bound prints them (dq, dk, dv):

    family        shapes, Nk | Nq (dh / Dp: 8/32 40/64 80/96 160/160 unless stated)          two_pass          one_pass
    self          192 | 192                                                                  0.40 0.40 0.41    0.16 0.19 0.41
    cross         8, 65, 77, 128 | 128 (one_pass: 77)                                        0.46 0.43 0.41    0.21 0.20 0.41
    split         77 | 320, 576                                                              0.43 0.41 0.37    -
    pf            512 | 512; 40/64 64/64 80/96 (one_pass: 40/64)                             0.42 0.42 0.41    0.14 0.18 0.41
    hostile       65 | 128 40/64, 192 | 192 40/64, 77 | 576 80/96, 128 | 128 160/160         0.38 0.43 0.39    0.16 0.21 0.39
    materialised  72 | 72 (8/32, 40/64), 4 | 4 (40/64), 136 | 128 (40/64): its own form      0.40 0.40 0.42

MEASURED below holds these figures rounded up to the next 0.05, asserted as ceilings (never above 0.5).

What the bound does not see.  On a row that one key dominates (the spiked query of hostile_rows: that key's p is 0.99995) ds = p (dp - D)
cancels -- |dp - D| is 4e-5 |D| at that key -- so the rounding terms u |dq| + scale u |ds| |k| shrink with it, and the cancellation term
e_D scale sum_j p_ij |k_jd| does not.  On that row (Nk 192, dh 40, median over its elements) the cancellation term is 68 times the
rounding terms in the two_pass form (e_D: some fifty fp32 roundings of sum p |dp|), which makes the whole two_pass bound on dq 264
times the rounding terms, and 1.0e5 times in the one_pass form (e_D = sum_d |dO| bound_O, the fp16 rounding of O): there the one_pass check
sees a wrong D only above about 4 u sum_d |dO_d O_d|.  On the other rows the two_pass bound is 2.1 times its rounding terms and the
one_pass bound 12 times (medians).  test_spiked_query_needs_two_bounds prints these factors.  ratio() refuses a bound that is not
positive."""
import ctypes as C
import math

import pytest
import torch

from pnpinversion_amd import _capi
from tests.test_attn_bound_host import (LOG2E, MARGIN, Q_SPIKE, SEEDS, U, attn_inputs, bounds, c32, emulate, hostile_rows, ratio)

FORMS = ("two_pass", "one_pass", "materialised")
# the constructed rows of hostile_do_rows: their indices (none of hostile_rows' queries)
DO_ZERO, DO_BIG, DO_TINY = 5, 21, 50

# worst emulated ratios (dq, dk, dv) per family and form, recorded when the bounds were written; asserted as ceilings below
MEASURED = {
    ("self", "two_pass"): (0.40, 0.40, 0.45), ("self", "one_pass"): (0.20, 0.20, 0.45),
    ("cross", "two_pass"): (0.50, 0.45, 0.45), ("cross", "one_pass"): (0.25, 0.20, 0.45),
    ("split", "two_pass"): (0.45, 0.45, 0.40),
    ("pf", "two_pass"): (0.45, 0.45, 0.45), ("pf", "one_pass"): (0.15, 0.20, 0.45),
    ("hostile", "two_pass"): (0.40, 0.45, 0.40), ("hostile", "one_pass"): (0.20, 0.25, 0.40),
    ("materialised", "materialised"): (0.40, 0.40, 0.45),
}


# ------------------------------------------------------------------------------------------------ the plan
def plan(heads, Nq, Nk, Dp, dh, scratch=-1, have_fwd=0):
    """pnpi_attn_bwd_plan_query under the tuning in force"""
    lib = _capi.load_library()
    pl = _capi.AttnBwdPlan()
    assert lib.pnpi_attn_bwd_plan_query(heads, Nq, Nk, Dp, dh, scratch, have_fwd, C.byref(pl)) == 0
    return pl


def instance(pl, Dp, mode):
    """the kernel a launch of the plan runs, as the GPU file's table names it"""
    if not pl.flash:
        return "materialised"
    return "attn_bwd_flash_kernel<%d,%d,%d,%s>" % (Dp, pl.lt, mode, "true" if (pl.pf_dq, pl.pf_dk, pl.pf_dv)[mode] else "false")


WIDTHS = [(8, 32), (40, 64), (80, 96), (160, 160)]


def test_plan_flash_conditions():
    for dh, Dp in WIDTHS:
        lt = 32 if Dp == 160 else 64
        for N in (64, 128, 192, 4096):
            pl = plan(2, N, N, Dp, dh)
            assert (pl.flash, pl.lt, pl.nsplit, pl.one_pass, pl.share_rows, pl.empty_shares) == (1, lt, 1, 0, N, 0), (N, Dp)
            assert plan(2, N, N, Dp, dh, have_fwd=1).one_pass == 1
        for N in (4, 32, 63, 72, 100, 130):                    # Nq >= 64 and Nq % 64 == 0
            assert plan(2, N, N, Dp, dh).flash == 0, N
        for Nk in (8, 65, 77, 128):                            # cross-attention: 8 <= Nk <= 128
            assert plan(2, 128, Nk, Dp, dh).flash == 1, Nk
        for Nk in (1, 7, 129, 136, 256):
            pl = plan(2, 128, Nk, Dp, dh)
            assert (pl.flash, pl.lt, pl.nsplit, pl.pf_dq, pl.pf_dk, pl.pf_dv, pl.one_pass) == (0, 0, 1, 0, 0, 0, 0), Nk
    for Dp in (16, 48, 128, 192):                              # head widths without an instance
        assert plan(2, 128, 128, Dp, 8).flash == 0, Dp
    for dh in (4, 12, 20, 36):                                 # dh % 8 == 0
        assert plan(2, 128, 128, 64, dh).flash == 0, dh
    assert plan(2, 128, 128, 32, 40).flash == 0                # dh <= Dp
    lib = _capi.load_library()
    assert lib.pnpi_attn_bwd_plan_query(2, 128, 128, 64, 40, -1, 0, None) == _capi.PNPI_EINVAL
    assert lib.pnpi_attn_bwd_plan_query(0, 128, 128, 64, 40, -1, 0, C.byref(_capi.AttnBwdPlan())) == _capi.PNPI_EINVAL


def test_plan_knob_values():
    lib = _capi.load_library()
    with _capi.tuning(lib, attn_bwd_flash=0):                  # materialised everywhere
        assert plan(2, 128, 128, 64, 40).flash == 0 and plan(2, 128, 77, 64, 40).flash == 0
    with _capi.tuning(lib, attn_bwd_flash=3):                  # self-attention only
        assert plan(2, 128, 128, 64, 40, have_fwd=1).flash == 1 and plan(2, 128, 128, 64, 40, have_fwd=1).one_pass == 1
        assert plan(2, 128, 77, 64, 40).flash == 0 and plan(2, 576, 77, 64, 40).flash == 0
    with _capi.tuning(lib, attn_bwd_flash=2):                  # two-pass dQ always
        pl = plan(2, 128, 128, 64, 40, have_fwd=1)
        assert pl.flash == 1 and pl.one_pass == 0
    assert plan(2, 128, 128, 64, 40, have_fwd=1).one_pass == 1 and plan(2, 128, 77, 64, 40).flash == 1      # and the knobs are back


@pytest.mark.parametrize("Nq,nsplit,rows64,empty64,rows32,empty32", [(128, 1, 128, 0, 128, 0), (256, 2, 128, 0, 128, 0), (320, 2, 192, 0, 160, 0),
                                                                    (576, 4, 192, 1, 160, 0), (4096, 32, 128, 0, 128, 0), (8192, 32, 256, 0, 256, 0)])
def test_plan_split(Nq, nsplit, rows64, empty64, rows32, empty32):
    """the dK / dV walk of a cross-attention site: Nq / 128 shares from 256 queries on, at most 32, each of whole loop tiles -- so at
    Nq 576 and LT 64 the four shares are 192, 192, 192 and 0 queries, at LT 32 160, 160, 160 and 96; self-attention is never split"""
    for dh, Dp in WIDTHS:
        pl = plan(2, Nq, 77, Dp, dh)
        want = (nsplit, rows32, empty32) if Dp == 160 else (nsplit, rows64, empty64)
        assert (pl.flash, pl.nsplit, pl.share_rows, pl.empty_shares) == (1,) + want, (Nq, Dp)
        lse_d = 2 * 2 * Nq * 4
        assert pl.scratch_bytes == lse_d + (0 if nsplit == 1 else (nsplit * 2 * 77 * dh * 4 + 255) // 256 * 256)
        assert pl.pf_dq == 0                                   # 77 loop rows
        assert plan(2, Nq, Nq, Dp, dh).nsplit == 1 and plan(2, Nq, 136, Dp, dh).nsplit == 1


def test_plan_prefetch():
    """PF exactly when Dp is 64 or 96, the walk has at least 8 loop tiles, the grid at most 512 workgroups, and the knob is on"""
    lib = _capi.load_library()
    for dh, Dp in WIDTHS:
        wide = Dp in (64, 96)
        for N, heads in ((448, 2), (512, 2), (4096, 8), (4096, 16), (4096, 17), (8192, 8), (8192, 9)):
            T = (N + 127) // 128 * heads
            want = int(wide and N >= 512 and T <= 512)
            pl = plan(heads, N, N, Dp, dh)
            assert (pl.pf_dq, pl.pf_dk, pl.pf_dv) == (want,) * 3, (N, heads, Dp)
            with _capi.tuning(lib, abf_prefetch=0):
                pl = plan(heads, N, N, Dp, dh)
                assert (pl.flash, pl.pf_dq, pl.pf_dk, pl.pf_dv) == (1, 0, 0, 0)
        # cross-attention: dQ walks 77 keys (never PF); dK / dV walk Nq queries in nsplit workgroups per (key tile, head)
        for Nq, heads, want in ((448, 2, 0), (576, 2, 1), (4096, 8, 1), (4096, 16, 1), (4096, 17, 0)):
            pl = plan(heads, Nq, 77, Dp, dh)
            assert (pl.pf_dq, pl.pf_dk, pl.pf_dv) == (0, int(wide and want), int(wide and want)), (Nq, heads, Dp)


def test_plan_scratch_too_small_is_materialised():
    lib = _capi.load_library()
    for Nq, Nk in ((192, 192), (576, 77)):
        need = plan(2, Nq, Nk, 64, 40).scratch_bytes
        assert plan(2, Nq, Nk, 64, 40, scratch=need).flash == 1
        for have in (need - 1, 0):
            pl = plan(2, Nq, Nk, 64, 40, scratch=have, have_fwd=1)
            assert (pl.flash, pl.lt, pl.nsplit, pl.one_pass) == (0, 0, 1, 0)
            assert pl.scratch_bytes == lib.pnpi_op_attention_bwd_scratch_bytes(Nq, Nk, 40)


# ------------------------------------------------------------------------------------------------ inputs
def bwd_inputs(Nq, Nk, dh, std, seed):
    """attn_inputs' q, k, v and dO [Nq, dh] ~ N(0, 1), all fp16"""
    q, k, v = attn_inputs(Nq, Nk, dh, std, seed)
    do = torch.randn(Nq, dh, generator=torch.Generator().manual_seed(seed + 7919)).half()
    return q, k, v, do


def hostile_do_rows(do):
    """in place on fp16 dO [Nq, dh]: DO_ZERO a zero row (ds = 0 exactly: the row must add nothing to dk and dv, and its dq is 0);
    DO_BIG a row times 2^8 (ds of the order of hundreds: it carries dk and dv, an error relative to IT swamps the small rows);
    DO_TINY a row times 2^-10 (its ds = p (dp - D) lies below fp16's normal range 2^-14: the subnormal term of the bounds)"""
    do[DO_ZERO] = 0
    do[DO_BIG] = (do[DO_BIG].float() * 256.0).half()
    do[DO_TINY] = (do[DO_TINY].float() * 2.0 ** -10).half()
    return do


def stacked(heads, Nq, Nk, dh, std, seed, hostile=False):
    """[heads, N, dh] inputs, head i from seed + i"""
    rows = []
    for i in range(heads):
        q, k, v, do = bwd_inputs(Nq, Nk, dh, std, seed + i)
        if hostile:
            hostile_rows(q, k, v, dh ** -0.5)
            hostile_do_rows(do)
        rows.append((q, k, v, do))
    return [torch.stack(t) for t in zip(*rows)]


# ------------------------------------------------------------------------------------------------ the emulation
def _fma_exp2(s, c, sub):
    """exp2(fma(s, c, -sub)): the exact product and difference rounded once to fp32 (s, c fp32: the product is exact in float64)"""
    return torch.exp2((s.double() * c.double() - sub.double()).float())


def emulate_bwd(q, k, v, do, scale, form, LT=64, nsplit=1, lse_fwd=None, o_fwd=None):
    """q, dO [..., Nq, d], k, v [..., Nk, d] fp16 -> (dq, dk, dv) fp16: the kernels' arithmetic in torch (the module docstring)"""
    assert q.dtype == k.dtype == v.dtype == do.dtype == torch.float16 and form in FORMS
    f32 = torch.float32
    c, sc = c32(scale), torch.tensor(scale, dtype=f32)
    qf, kf, vf, dof = q.float(), k.float(), v.float(), do.float()
    Nq, Nk = q.shape[-2], k.shape[-2]
    T = lambda x: x.transpose(-1, -2)      # noqa: E731
    if form == "materialised":
        S = (qf @ T(kf)) * sc
        e = torch.exp(S - S.amax(-1, keepdim=True))
        P = e * (1.0 / e.sum(-1, keepdim=True))
        dP = dof @ T(vf)
        D = (P * dP).sum(-1, keepdim=True)
        ds16 = ((sc * P) * (dP - D)).half().float()
        assert ds16.dtype == f32
        return (ds16 @ kf).half(), (T(ds16) @ qf).half(), (T(P.half().float()) @ dof).half()
    if form == "one_pass":
        lse, D = lse_fwd.float(), (dof * o_fwd.float()).sum(-1)
    else:
        m = torch.full(q.shape[:-1], -math.inf, dtype=f32)
        l, d = torch.zeros_like(m), torch.zeros_like(m)
        for l0 in range(0, Nk, LT):
            s, dp = qf @ T(kf[..., l0:l0 + LT, :]), dof @ T(vf[..., l0:l0 + LT, :])
            mn = torch.maximum(m, s.amax(-1))
            alpha = torch.exp2((m - mn) * c)
            pv = _fma_exp2(s, c, (mn * c)[..., None])
            l, d, m = l * alpha + pv.sum(-1), d * alpha + (pv * dp).sum(-1), mn
        lse, D = m * c + torch.log2(l), d / l
    assert lse.dtype == f32 and D.dtype == f32
    acc = torch.zeros_like(qf)
    for l0 in range(0, Nk, LT):                  # dQ: block = queries, loop = keys
        kt = kf[..., l0:l0 + LT, :]
        s, dp = qf @ T(kt), dof @ T(vf[..., l0:l0 + LT, :])
        ds16 = (_fma_exp2(s, c, lse[..., None]) * (dp - D[..., None])).half().float()
        acc = acc + ds16 @ kt
    dq = (acc * sc).half()
    share = ((Nq + nsplit - 1) // nsplit + LT - 1) // LT * LT
    pk, pv_ = [], []
    for sp in range(nsplit):                     # dK / dV: block = keys, loop = this share's queries
        ak, av = torch.zeros_like(kf), torch.zeros_like(kf)
        for l0 in range(sp * share, min(Nq, (sp + 1) * share), LT):
            qt, dot = qf[..., l0:l0 + LT, :], dof[..., l0:l0 + LT, :]
            s, dp = qt @ T(kf), dot @ T(vf)
            P = _fma_exp2(s, c, lse[..., l0:l0 + LT, None])
            ds16 = (P * (dp - D[..., l0:l0 + LT, None])).half().float()
            ak, av = ak + T(ds16) @ qt, av + T(P.half().float()) @ dot
        pk.append(ak * sc), pv_.append(av)
    dk, dv = pk[0], pv_[0]
    for sp in range(1, nsplit):                  # attn_bwd_reduce_kernel: the shares in order, one rounding
        dk, dv = dk + pk[sp], dv + pv_[sp]
    assert acc.dtype == f32 and dk.dtype == f32 and dv.dtype == f32
    return dq, dk.half(), dv.half()


def forward_of(q, k, v, scale):
    """what the recording forward hands over: (O fp16, lse fp32) of the forward emulation's plain form"""
    return emulate(q, k, v, scale, "plain")


# ------------------------------------------------------------------------------------------------ reference and bounds
def reference_bwd(q, k, v, do, scale):
    """float64 autograd of softmax(scale q k^T) v on the fp16 values (scale as the fp32 value the kernel gets) -> dq, dk, dv"""
    s = float(torch.tensor(scale, dtype=torch.float32))
    qr, kr, vr = [t.double().detach().clone().requires_grad_(True) for t in (q, k, v)]
    (torch.softmax(s * qr @ kr.transpose(-1, -2), -1) @ vr).backward(do.double())
    return qr.grad, kr.grad, vr.grad


def bounds_bwd(q, k, v, do, scale, Dp, form, LT=64, nsplit=1, parts=False):
    """-> ((ref dq, dk, dv), (bound dq, dk, dv)): functions of the fp16 inputs and the float64 reference only (the docstring's
    derivation; matrix products throughout).  Runs on the device of its inputs.  parts = True: also, for dq, the rounding terms and the
    cancellation term on their own (test_spiked_query_needs_two_bounds)."""
    assert form in FORMS
    ref = reference_bwd(q, k, v, do, scale)
    s = float(torch.tensor(scale, dtype=torch.float32))
    c = s * LOG2E
    Nq, Nk = q.shape[-2], k.shape[-2]
    T = lambda x: x.transpose(-1, -2)      # noqa: E731
    qd, kd, vd, dd = q.double(), k.double(), v.double(), do.double()
    cs = (qd @ T(kd)) * c
    M = cs.amax(-1, keepdim=True)
    e = torch.exp2(cs - M)
    L = e.sum(-1, keepdim=True)
    p = e / L
    lse = M + torch.log2(L)
    dp = dd @ T(vd)
    D = (p * dp).sum(-1, keepdim=True)
    ds = (p * (dp - D)).abs()
    absqk = c * (qd.abs() @ T(kd.abs()))
    e_dp = (Dp // 16) * 2.0 ** -24 * (dd.abs() @ T(vd.abs()))
    eD_ext = eta_ext = 0.0
    if form == "materialised":
        dm = (Dp // 16 + 3) * 2.0 ** -24 * absqk + 2.0 * 2.0 ** -24 * (M - cs)
        eta = torch.exp2(dm + (p * dm).sum(-1, keepdim=True)) - 1.0 + (Nk / 64.0 + 12) * 2.0 ** -24
        eD = (p * (eta * dp.abs() + e_dp)).sum(-1, keepdim=True) + (Nk / 64.0 + 8) * 2.0 ** -24 * (p * dp.abs()).sum(-1, keepdim=True)
        eta = eta + 3 * 2.0 ** -24
        sub_scale, acc_q, acc_k = 1.0, Nk / 16.0 + 8, Nq / 16.0 + 8
    else:
        ntile = -(-Nk // LT)
        d0 = (Dp // 16 + 2) * 2.0 ** -24 * absqk
        delta = d0 + 2.0 ** -24 * (cs - lse).abs()
        if form == "two_pass":
            delta0 = d0 + 2.0 ** -24 * (M - cs)
            eps = (p * delta0).sum(-1, keepdim=True) + LOG2E * (LT / 2 + 4 * ntile + 4) * 2.0 ** -24 + 2.0 ** -23 * M.abs() + \
                2.0 ** -23 * (1 + math.log2(Nk)) + 2.0 ** -24 * lse.abs()
            w = p * (torch.exp2(delta0) - 1.0)
            eD = (w * (dp - D).abs()).sum(-1, keepdim=True) / (1.0 - w.sum(-1, keepdim=True)) + (p * e_dp).sum(-1, keepdim=True) + \
                (LT / 2 + 4 * ntile + 6) * 2.0 ** -24 * (p * dp.abs()).sum(-1, keepdim=True)
            eta = torch.exp2(delta + eps) - 1.0 + 6 * 2.0 ** -24
        else:
            o_ref, bo, _, bl = bounds(q, k, v, scale, "plain", Dp)      # the forward's bounds, whole (MARGIN included): what the device may hand over
            eta = torch.exp2(delta) - 1.0 + 6 * 2.0 ** -24
            eta_ext = torch.exp2(delta) * (torch.exp2(bl[..., None]) - 1.0)
            eD = (Dp // 2 + 1) * 2.0 ** -24 * (dd.abs() * o_ref.abs()).sum(-1, keepdim=True)
            eD_ext = (dd.abs() * bo).sum(-1, keepdim=True)
        sub_scale, acc_q, acc_k = s, Nk / 16.0 + 3, Nq / 16.0 + nsplit + 2
    W = eta * ds + p * (e_dp + eD)
    Wext = eta_ext * ds + p * eD_ext
    ka, qa, da = kd.abs(), qd.abs(), dd.abs()
    floor = 2.0 ** -24
    bq = MARGIN * (U * ref[0].abs() + s * ((U * ds + W) @ ka) + sub_scale * Nk * 2.0 ** -25 * ka.amax(-2, keepdim=True) +
                   acc_q * 2.0 ** -24 * s * (ds @ ka)) + s * (Wext @ ka) + floor
    bk = MARGIN * (U * ref[1].abs() + s * (T(U * ds + W) @ qa) + sub_scale * Nq * 2.0 ** -25 * qa.amax(-2, keepdim=True) +
                   acc_k * 2.0 ** -24 * s * (T(ds) @ qa)) + s * (T(Wext) @ qa) + floor
    bv = MARGIN * (U * ref[2].abs() + T(U * p + eta * p) @ da + Nq * 2.0 ** -25 * da.amax(-2, keepdim=True) +
                   acc_k * 2.0 ** -24 * (T(p) @ da)) + T(eta_ext * p) @ da + floor
    if parts:
        return ref, (bq, bk, bv), (U * ref[0].abs() + s * (U * ds @ ka), s * ((p * (eD + eD_ext)) @ ka))
    return ref, (bq, bk, bv)


def bound_D_one_pass(do, o16, Dp):
    """-> (D, bound): the one-pass D[q] against the O it was GIVEN -- sum_d dO O_fp16 in float64 of the fp16 values, and what the kernel's
    fp32 fma chain (Dp / 2 terms per half-wave, one add across them) may differ from it: MARGIN (Dp / 2 + 1) 2^-24 sum_d |dO O|.  No
    rounding of O is in this bound, so an O that was rounded once more on its way into D breaks it (by about u / (Dp 2^-24), two
    orders of magnitude)."""
    prod = do.double() * o16.double()
    return prod.sum(-1), MARGIN * (Dp // 2 + 1) * 2.0 ** -24 * prod.abs().sum(-1) + 2.0 ** -60


def ratios(got, ref, bnd):
    return tuple(ratio(g, r, b) for g, r, b in zip(got, ref, bnd))


# ------------------------------------------------------------------------------------------------ the emulation against the bounds
# (Nq, Nk, dh, Dp, forms) per family: the shapes of tests/test_gpu_attn_bwd_instances.py
BOTH = ("two_pass", "one_pass")
SELF_SHAPES = [(192, 192, dh, dp, BOTH) for dh, dp in WIDTHS]
CROSS_SHAPES = [(128, nk, dh, dp, BOTH if nk == 77 else BOTH[:1]) for nk in (8, 65, 77, 128) for dh, dp in WIDTHS]
SPLIT_SHAPES = [(nq, 77, dh, dp, BOTH[:1]) for nq in (320, 576) for dh, dp in WIDTHS]
PF_SHAPES = [(512, 512, 40, 64, BOTH), (512, 512, 64, 64, BOTH[:1]), (512, 512, 80, 96, BOTH[:1])]
HOSTILE_BWD_SHAPES = [(128, 65, 40, 64, BOTH), (192, 192, 40, 64, BOTH), (576, 77, 80, 96, BOTH), (128, 128, 160, 160, BOTH)]
MAT_SHAPES = [(72, 72, 8, 32, ("materialised",)), (72, 72, 40, 64, ("materialised",)), (4, 4, 40, 64, ("materialised",)),
              (128, 136, 40, 64, ("materialised",))]
FAMILIES = {"self": SELF_SHAPES, "cross": CROSS_SHAPES, "split": SPLIT_SHAPES, "pf": PF_SHAPES, "hostile": HOSTILE_BWD_SHAPES,
            "materialised": MAT_SHAPES}


def run_emulation(q, k, v, do, scale, Dp, form):
    """the emulation as the plan dispatches this shape (LT, nsplit), and the bounds with the same two numbers"""
    Nq, Nk, dh = q.shape[-2], k.shape[-2], q.shape[-1]
    pl = plan(q.shape[0], Nq, Nk, Dp, dh, have_fwd=int(form == "one_pass"))
    assert pl.flash == int(form != "materialised") and pl.one_pass == int(form == "one_pass"), (Nq, Nk, Dp, form)
    o, lse = forward_of(q, k, v, scale) if form == "one_pass" else (None, None)
    got = emulate_bwd(q, k, v, do, scale, form, pl.lt or 64, pl.nsplit, lse, o)
    ref, bnd = bounds_bwd(q, k, v, do, scale, Dp, form, pl.lt or 64, pl.nsplit)
    return got, ref, bnd


@pytest.mark.parametrize("family", list(FAMILIES))
def test_emulation_leaves_half_the_bound(family):
    worst = {}
    for Nq, Nk, dh, Dp, forms in FAMILIES[family]:
        scale = dh ** -0.5
        variants = [(1.0, True)] if family == "hostile" else [(1.0, False), (3.0, False)]
        for form in forms:
            w = (0.0, 0.0, 0.0)
            for std, host in variants:
                for seed in SEEDS:
                    q, k, v, do = stacked(2, Nq, Nk, dh, std, 100 * seed + Nq + Nk + dh, host)
                    got, ref, bnd = run_emulation(q, k, v, do, scale, Dp, form)
                    w = tuple(max(a, b) for a, b in zip(w, ratios(got, ref, bnd)))
            print("%s %s Nq %d Nk %d dh %d Dp %d: worst dq %.3f dk %.3f dv %.3f" % ((family, form, Nq, Nk, dh, Dp) + w))
            worst[form] = tuple(max(a, b) for a, b in zip(worst.get(form, (0.0,) * 3), w))
    for form, w in worst.items():
        print("%s %s: worst dq %.3f dk %.3f dv %.3f" % ((family, form) + w))
    for form, w in worst.items():
        for got, ceil in zip(w, MEASURED[(family, form)]):
            assert got <= ceil <= 0.5, (family, form, w)


@pytest.mark.parametrize("dh,Dp", WIDTHS)
def test_one_pass_D_against_the_O_it_was_given(dh, Dp):
    """the fp32 sum of the emulation stays inside half of bound_D_one_pass; the same sum over an O rounded a second time (fp16 at
    another scale) is outside the whole bound"""
    q, k, v, do = stacked(2, 192, 192, dh, 1.0, 5, hostile=True)
    o16, _ = forward_of(q, k, v, dh ** -0.5)
    D, bD = bound_D_one_pass(do, o16, Dp)
    r = ratio((do.float() * o16.float()).sum(-1), D, bD)
    twice = ((o16.float() * 1.4426950).half().float() / 1.4426950)
    r2 = ratio((do.float() * twice).sum(-1), D, bD)
    print("one-pass D, dh %d: fp32 sum / bound %.3f, with O rounded twice %.1f" % (dh, r, r2))
    assert r <= 0.5 and r2 > 1.0


def test_analytic_gradients_are_autograd():
    """the closed form the bounds are written in (ds = p (dp - D)) is the float64 autograd the reference is"""
    q, k, v, do = stacked(2, 128, 77, 40, 1.0, 3)
    s = float(torch.tensor(40 ** -0.5, dtype=torch.float32))
    qd, kd, vd, dd = q.double(), k.double(), v.double(), do.double()
    p = torch.softmax(s * qd @ kd.transpose(-1, -2), -1)
    dp = dd @ vd.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    ref = reference_bwd(q, k, v, do, 40 ** -0.5)
    for a, b in zip((s * ds @ kd, s * ds.transpose(-1, -2) @ qd, p.transpose(-1, -2) @ dd), ref):
        assert (a - b).abs().max() <= 1e-12 * b.abs().max()


def test_constructed_do_rows_do_what_they_are_built_for():
    Nq, Nk, dh = 192, 192, 40
    scale = dh ** -0.5
    q, k, v, do = stacked(1, Nq, Nk, dh, 1.0, 7, hostile=True)
    (dq, dk, dv), ref, bnd = run_emulation(q, k, v, do, scale, 64, "two_pass")
    assert ratios((dq, dk, dv), ref, bnd) <= (0.5, 0.5, 0.5)
    # the zero row: its dq is exactly 0, and dk / dv are what they are without that query
    assert (dq[0, DO_ZERO] == 0).all() and (ref[0][0, DO_ZERO] == 0).all()
    keep = torch.arange(Nq) != DO_ZERO
    ref_wo = reference_bwd(q[:, keep], k, v, do[:, keep], scale)
    assert (ref_wo[1] - ref[1]).abs().max() <= 1e-12 and (ref_wo[2] - ref[2]).abs().max() <= 1e-12
    # the big row carries dv: without it dv's norm drops by more than half
    big = torch.arange(Nq) != DO_BIG
    assert reference_bwd(q[:, big], k, v, do[:, big], scale)[2].norm() < 0.5 * ref[2].norm()
    # the tiny row: most of its ds lie below fp16's normal range, and most of them above half the smallest subnormal (not flushed)
    qd, kd, vd, dd = q.double(), k.double(), v.double(), do.double()
    p = torch.softmax(float(torch.tensor(scale, dtype=torch.float32)) * qd @ kd.transpose(-1, -2), -1)
    dp = dd @ vd.transpose(-1, -2)
    ds = (p * (dp - (p * dp).sum(-1, keepdim=True)))[0, DO_TINY].abs()
    print("tiny dO row: |ds| %.2e ... %.2e (fp16 normal range begins at %.2e)" % (ds.min(), ds.max(), 2.0 ** -14))
    assert (ds < 2.0 ** -14).float().mean() > 0.5 and (ds > 2.0 ** -25).float().mean() > 0.5
    assert ratio(dq[0, DO_TINY], ref[0][0, DO_TINY], bnd[0][0, DO_TINY]) <= 0.5


def test_spiked_query_needs_two_bounds():
    """the spiked query of hostile_rows: one key carries the row, so dp - D cancels at that key (|dp - D| small against |D|), and the
    error of D is what is left.  The one-pass D (from the fp16 O) is off by more there than the whole two_pass bound allows, and within
    half of the one_pass bound: the two forms need two bounds.  Prints how many times the rounding terms each bound is on that row."""
    Nq, Nk, dh, Dp = 192, 192, 40, 64
    scale = dh ** -0.5
    q, k, v, do = stacked(1, Nq, Nk, dh, 1.0, 7, hostile=True)
    qd, kd, vd, dd = q.double(), k.double(), v.double(), do.double()
    p = torch.softmax(float(torch.tensor(scale, dtype=torch.float32)) * qd @ kd.transpose(-1, -2), -1)
    dp = dd @ vd.transpose(-1, -2)
    D = (p * dp).sum(-1)
    i = Q_SPIKE
    print("spiked query: p of the last key %.6f, |dp - D| / |D| there %.2e" % (p[0, i, Nk - 1], (dp[0, i, Nk - 1] - D[0, i]).abs() / D[0, i].abs()))
    assert p[0, i, Nk - 1] > 0.99 and (dp[0, i, Nk - 1] - D[0, i]).abs() < 0.01 * D[0, i].abs()
    one, ref, b1 = run_emulation(q, k, v, do, scale, Dp, "one_pass")
    two, _, b2 = run_emulation(q, k, v, do, scale, Dp, "two_pass")
    r_one_own, r_one_two = ratio(one[0][0, i], ref[0][0, i], b1[0][0, i]), ratio(one[0][0, i], ref[0][0, i], b2[0][0, i])
    r_two = ratio(two[0][0, i], ref[0][0, i], b2[0][0, i])
    print("spiked query's dq: one-pass emulation / one_pass bound %.3f, / two_pass bound %.1f; two-pass emulation / two_pass bound %.3f"
          % (r_one_own, r_one_two, r_two))
    assert r_one_own <= 0.5 and r_two <= 0.5 and r_one_two > 1.0
    others = torch.arange(Nq) != i
    for form in BOTH:
        _, bnd, (rnd, canc) = bounds_bwd(q, k, v, do, scale, Dp, form, parts=True)
        print("%s: dq bound / rounding terms, median over the spiked row %.1f, over the other rows %.1f; cancellation term / rounding terms on the "
              "spiked row %.1f" % (form, (bnd[0][0, i] / rnd[0, i]).median(), (bnd[0][0, others] / rnd[0, others]).median(),
                                   (canc[0, i] / rnd[0, i]).median()))


def test_bound_notices_one_query_that_lost_its_last_key():
    """what the per-element bound is for: the dq of ONE query of 2 x 2048 computed without the last of its 77 keys passes the old
    whole-tensor relative error of 6e-3 twenty times over (3e-4) and breaks the per-element bound (by a factor of 2.5: the key
    it lost held about 1 / 77 of the row's weight)"""
    Nq, Nk, dh, Dp, row = 2048, 77, 40, 64, 777
    scale = dh ** -0.5
    q, k, v, do = stacked(2, Nq, Nk, dh, 1.0, 11)
    got, ref, bnd = run_emulation(q, k, v, do, scale, Dp, "two_pass")
    assert ratios(got, ref, bnd) <= (0.5, 0.5, 0.5)
    dq = got[0].clone()
    dq[0, row] = reference_bwd(q[:1, row:row + 1], k[:1, :Nk - 1], v[:1, :Nk - 1], do[:1, row:row + 1], scale)[0][0, 0].half()
    l2 = ((dq.double() - ref[0]).norm() / ref[0].norm()).item()
    print("one query without its last key: dq rel-L2 %.2e, per-element ratio %.1f" % (l2, ratio(dq, ref[0], bnd[0])))
    assert l2 < 6e-3 and ratio(dq, ref[0], bnd[0]) > 2
