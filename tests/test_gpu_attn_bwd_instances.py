"""Every instance the attention backward dispatches -- the 18 of attn_bwd_flash_kernel<DP, LT, MODE, PF>, attn_bwd_reduce_kernel behind a
split cross-attention walk, the one-pass dQ behind the forward's hand-over, and the materialised fallback -- through
pnpi_op_attention_bwd_fwd, each against float64 autograd of the fp16 inputs under the per-element bounds for dq, dk and dv that
tests/test_attn_bwd_bound_host.py derives (applied unchanged), the old whole-tensor rel_err < 6e-3 beside them, with guard bands
checked bit for bit.  Before every launch pnpi_attn_bwd_plan_query has to name the instance of the table below, so a case that
silently moved to another path fails; flash launches also assert the executed_attn_flops delta (10 tile products per pair, 8 one-pass).

Layout (B = 1, two heads unless stated): q | k | v are column ranges of ONE buffer (q_off 8, k_off hd + 16, v_off 2 hd + 24,
ld = 3 hd + 40; cross-attention: q alone with q_off 8 and ld hd + 24, k | v together with k_off 8, v_off hd + 24, ld 2 hd + 40), in which
every column outside the heads' dh columns -- the dh .. Dp pad included -- and one extra row are NaN: the flash kernel reads columns < dh
only.  The materialised form is written for zero pad columns (api_backward.inc's header), so its cases zero the dh .. Dp pad and poison
the rest.  d_o and o_fwd have ld = heads dh + 8 with NaN padding.  The gradients go to buffers of the inputs' layout filled with a
canary: everything outside the heads' dh columns, and the extra row, has to survive bit for bit, and so do 4 KB behind the scratch the
plan asks for (the launch gets exactly that many bytes).

Instance -> case:
    <32,64,M,false> <64,64,M,false> <96,64,M,false> <160,32,M,false>, M = 0, 1, 2     test_self_attention_plain_instances: Nq = Nk = 192, dh / Dp
                                                                                       8/32 40/64 80/96 160/160 (the last block tile is half empty)
    the same, cross-attention unsplit                  test_cross_attention_unsplit: Nq 128, Nk 8, 65, 77, 128
    <.,.,1 / 2,false> + attn_bwd_reduce_kernel         test_cross_attention_split: Nk 77, Nq 320 (2 shares: 192 + 128 at LT 64, 160 + 160 at LT 32),
                                                       Nq 576 (4 shares: 192 192 192 0 at LT 64 -- the fourth is empty -- 160 160 160 96 at LT 32)
    <64,64,1 / 2,true> <96,64,1 / 2,true> + reduce     the same test at Nq 576: the split walk under PF
    <64,64,M,true> <96,64,M,true>, M = 0, 1, 2         test_prefetch_instances: Nq = Nk = 512, 40/64 64/64 80/96, bit for bit against abf_prefetch = 0
    one-pass dQ (<.,.,0,.> with the forward's lse, O)  self 192 and cross 77 | 128 at every width, 512 at 40/64, test_two_batch_rows_three_heads
    materialised                                       test_materialised_fallback: Nq = Nk = 72, Nq = Nk = 4, Nk 136 | Nq 128
No case is left out.

Worst |got - ref| / bound on an MI355X (dq, dk, dv; the emulation's figures are in the host file):
    family          two_pass            one_pass
    self 192        0.39 0.39 0.42      0.15 0.20 0.42
    cross           0.44 0.42 0.39      0.16 0.15 0.35
    split           0.39 0.25 0.24      -
    pf 512          0.33 0.31 0.31      0.08 0.08 0.31      (the abf_prefetch = 0 twin: the same bits)
    B 2, 3 heads    0.36 0.32 0.30      0.10 0.11 0.30
    hostile         0.41 0.43 0.35      0.13 0.16 0.35
    materialised    0.35 0.38 0.40
One-pass against two-pass: at most 0.22 of the sum of the two bounds.  The whole file runs in about five seconds.

Mutations tried on a scratch copy of csrc/attn.hip (not committed), each run against this file and against the old whole-tensor cases
(test_attention_bwd_flash, test_forward_lse_feeds_the_one_pass_dq):
  * D taken from O rounded a second time (fp16 at another scale) in the one-pass dQ: the old cases pass; the gradients' bounds pass too
    (bound_O is at least 4 u |O| wide, the host file says why); caught by the check of D itself against the O handed over
    (bound_D_one_pass, every one-pass case: 14 tests fail).
  * the last of four split shares dropped in attn_bwd_reduce_kernel: the old cases pass; caught by test_cross_attention_split at
    Nq 576, Dp 160 alone -- at LT 64 the fourth share is the empty one, which the plan query states.
  * row < p.nl replaced by row <= p.nl in stage_rows: caught by 22 tests, every cross-attention case with a ragged loop tile (Nk 8, 65,
    77; Nq 320 and 576 in the split walk) and the two hostile cases at Nk 65 and 77: the extra row is NaN.  (Not run against the old
    cases: their buffers end with the last row.)
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402
from tests.test_attn_bound_host import Q_SPIKE, bounds, ratio  # noqa: E402
from tests.test_attn_bwd_bound_host import (DO_BIG, DO_TINY, DO_ZERO, HOSTILE_BWD_SHAPES, WIDTHS, bound_D_one_pass, bounds_bwd, instance, plan,
                                            stacked)  # noqa: E402

DEV = "cuda"
G_CANARY = 3.5               # exactly representable in fp16
GUARD = 4096                 # bytes behind the scratch
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def _counters(ctx):
    c = _capi.Counters()
    assert ctx.lib.pnpi_get_counters(ctx.h, C.byref(c)) == 0
    return c.executed_attn_flops


def lay(buf, x, off, Dp):
    """x [B, heads, N, dh] into rows 0 .. B N of buf, head h at columns off + h Dp"""
    B, heads, N, dh = x.shape
    for h in range(heads):
        buf[:B * N, off + h * Dp:off + h * Dp + dh] = x[:, h].reshape(B * N, dh)


def unlay(buf, off, Dp, B, heads, N, dh):
    return torch.stack([buf[:B * N, off + h * Dp:off + h * Dp + dh].reshape(B, N, dh) for h in range(heads)], 1)


class Case:
    """B batch rows of q, dO [heads, Nq, dh], k, v [heads, Nk, dh] (fp16 values, kept for the reference) in the poisoned device layout"""

    def __init__(self, B, heads, Nq, Nk, dh, Dp, std=1.0, seed=0, hostile=False, zero_pad=False):
        self.B, self.heads, self.Nq, self.Nk, self.dh, self.Dp = B, heads, Nq, Nk, dh, Dp
        self.scale = dh ** -0.5
        rows = [stacked(heads, Nq, Nk, dh, std, 1000 * seed + 10 * b, hostile) for b in range(B)]
        self.q, self.k, self.v, self.do = [torch.stack(t).to(DEV) for t in zip(*rows)]
        hd = heads * Dp
        self.hd = hd
        if Nq == Nk:
            self.q_off, self.k_off, self.v_off = 8, hd + 16, 2 * hd + 24
            self.ldq = self.ldk = self.ldv = 3 * hd + 40
            self.qbuf = self.kbuf = self.vbuf = torch.full((B * Nq + 1, self.ldq), NAN, dtype=torch.half, device=DEV)
            self.bufs = [(self.qbuf, (self.q_off, self.k_off, self.v_off))]
        else:
            self.q_off, self.k_off, self.v_off = 8, 8, hd + 24
            self.ldq, self.ldk = hd + 24, 2 * hd + 40
            self.ldv = self.ldk
            self.qbuf = torch.full((B * Nq + 1, self.ldq), NAN, dtype=torch.half, device=DEV)
            self.kbuf = self.vbuf = torch.full((B * Nk + 1, self.ldk), NAN, dtype=torch.half, device=DEV)
            self.bufs = [(self.qbuf, (self.q_off,)), (self.kbuf, (self.k_off, self.v_off))]
        if zero_pad:      # the materialised form: zero pad columns dh .. Dp inside the head ranges
            for buf, offs in self.bufs:
                for off in offs:
                    buf[:-1, off:off + hd] = 0
        lay(self.qbuf, self.q, self.q_off, Dp), lay(self.kbuf, self.k, self.k_off, Dp), lay(self.vbuf, self.v, self.v_off, Dp)
        self.ldo = heads * dh + 8
        self.d_o = torch.full((B * Nq + 1, self.ldo), NAN, dtype=torch.half, device=DEV)
        lay(self.d_o, self.do, 0, dh)
        self._ref = {}

    def plan(self, have_fwd, flash=True):
        pl = plan(self.heads, self.Nq, self.Nk, self.Dp, self.dh, have_fwd=have_fwd)
        assert pl.flash == int(flash), "the plan moved this shape to the other form"
        return pl

    def forward(self, ctx):
        """pnpi_op_attention_ex (plain form) on zero-padded copies of q | k and V^T -> (O [B Nq + 1, ldo] with NaN padding, lse [B, heads, Nq])"""
        B, heads, Nq, Nk, dh, Dp, hd = self.B, self.heads, self.Nq, self.Nk, self.dh, self.Dp, self.hd
        ld, q_off, k_off = 3 * hd + 24, 8, hd + 16
        fused = torch.full((B * max(Nq, Nk), ld), NAN, dtype=torch.half, device=DEV)
        fused[:B * Nq, q_off:q_off + hd] = 0
        fused[:B * Nk, k_off:k_off + hd] = 0
        lay(fused, self.q, q_off, Dp), lay(fused, self.k, k_off, Dp)
        ldvt = (Nk + 7) // 8 * 8
        vt = torch.full((B, heads, Dp, ldvt), NAN, dtype=torch.half, device=DEV)
        vt[..., :Nk] = 0
        vt[:, :, :dh, :Nk] = self.v.transpose(2, 3)
        o = torch.full((B * Nq + 1, self.ldo), NAN, dtype=torch.half, device=DEV)
        lse = torch.full((B, heads, Nq), NAN, dtype=torch.float32, device=DEV)
        rows = torch.arange(B, dtype=torch.int32, device=DEV).repeat_interleave(4).contiguous()
        with ctx.tuning(op_attention_aug=0, op_attention_vt_perm=0):
            ctx.call("pnpi_op_attention_ex", ptr(fused), ld, q_off, ptr(fused), ld, k_off, ptr(vt), ldvt, ptr(o), self.ldo, heads, Nq, Nk, Dp, dh,
                     self.scale, ptr(rows), B, 0, ptr(lse))
            torch.cuda.synchronize()
        for b in range(B):      # what is handed over is inside the forward's own bounds
            ref, bo, rl, bl = bounds(self.q[b], self.k[b], self.v[b], self.scale, "plain", Dp)
            got = o[b * Nq:(b + 1) * Nq, :heads * dh].reshape(Nq, heads, dh).permute(1, 0, 2)
            assert ratio(got, ref, bo) <= 1.0 and ratio(lse[b], rl, bl) <= 1.0
        return o, lse

    def grads(self):
        """canary-filled gradient buffers in the layout of the inputs -> (dq buffer, dk buffer, dv buffer, [(buffer, offsets)])"""
        gq = torch.full_like(self.qbuf, G_CANARY)
        if self.Nq == self.Nk:
            return gq, gq, gq, [(gq, (self.q_off, self.k_off, self.v_off))]
        gk = torch.full_like(self.kbuf, G_CANARY)
        return gq, gk, gk, [(gq, (self.q_off,)), (gk, (self.k_off, self.v_off))]

    def args(self, gq, gk, gv, scratch, nbytes, fwd):
        o, lse = fwd if fwd else (None, None)
        return [ptr(self.qbuf), self.ldq, self.q_off, ptr(self.kbuf), self.ldk, self.k_off, ptr(self.vbuf), self.ldv, self.v_off, ptr(self.d_o), self.ldo,
                self.heads, self.Nq, self.Nk, self.Dp, self.dh, self.scale, self.B, ptr(gq), ptr(gk), ptr(gv), ptr(scratch), nbytes,
                ptr(lse) if fwd else None, ptr(o) if fwd else None, self.ldo if fwd else 0]

    def untouched(self, gbufs):
        for buf, offs in gbufs:
            keep = torch.ones_like(buf, dtype=torch.bool)
            for off in offs:
                for h in range(self.heads):
                    keep[:-1, off + h * self.Dp:off + h * self.Dp + self.dh] = False
            if not torch.equal(buf.view(torch.int16)[keep], torch.full_like(buf, G_CANARY).view(torch.int16)[keep]):
                return False
        return True

    def backward(self, ctx, pl, fwd=None):
        """one launch with exactly the scratch the plan asks for -> (dq, dk, dv) as [B, heads, N, dh]"""
        nbytes = pl.scratch_bytes * (1 if pl.flash else self.heads)
        scratch = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        assert plan(self.heads, self.Nq, self.Nk, self.Dp, self.dh, scratch=nbytes, have_fwd=int(fwd is not None)).flash == pl.flash
        gq, gk, gv, gbufs = self.grads()
        f0 = _counters(ctx)
        ctx.call("pnpi_op_attention_bwd_fwd", *self.args(gq, gk, gv, scratch, nbytes, fwd))
        torch.cuda.synchronize()
        if pl.flash:
            unit = 2.0 * self.heads * self.Nq * self.Nk * self.Dp * self.B
            assert _counters(ctx) - f0 == unit * ((3 if pl.one_pass else 5) + 3 + 2), "executed_attn_flops: not the form the plan names"
        assert self.untouched(gbufs), "a gradient column outside the heads' dh columns, or the extra row, was written"
        assert (scratch[nbytes:] == 0x5A).all(), "a write past the scratch the plan asks for"
        if pl.one_pass:      # the workspace is [heads][Nq] lse, then [heads][Nq] D (of the last batch row): D against the O it was given
            n4, b = self.heads * self.Nq * 4, self.B - 1
            dsum = scratch[n4:2 * n4].view(torch.float32).reshape(self.heads, self.Nq)
            o16 = fwd[0][b * self.Nq:(b + 1) * self.Nq, :self.heads * self.dh].reshape(self.Nq, self.heads, self.dh).permute(1, 0, 2)
            D, bD = bound_D_one_pass(self.do[b], o16, self.Dp)
            rD = ratio(dsum, D, bD)
            print("one-pass D against the O handed over: ratio %.3f" % rD)
            assert rD <= 1.0, ("D", rD)
        B, heads, dh, Dp = self.B, self.heads, self.dh, self.Dp
        return (unlay(gq, self.q_off, Dp, B, heads, self.Nq, dh), unlay(gk, self.k_off, Dp, B, heads, self.Nk, dh),
                unlay(gv, self.v_off, Dp, B, heads, self.Nk, dh))

    def reference(self, form, pl):
        """per batch row ((ref dq, dk, dv), (bounds)), computed once per form"""
        if form not in self._ref:
            self._ref[form] = [bounds_bwd(self.q[b], self.k[b], self.v[b], self.do[b], self.scale, self.Dp, form, pl.lt or 64, pl.nsplit)
                               for b in range(self.B)]
        return self._ref[form]

    def check(self, tag, got, form, pl):
        """the per-element bounds and the old whole-tensor relative error -> worst (dq, dk, dv) ratio"""
        worst = [0.0, 0.0, 0.0]
        for b, (ref, bnd) in enumerate(self.reference(form, pl)):
            for i, name in enumerate(("dq", "dk", "dv")):
                r, l2 = ratio(got[i][b], ref[i], bnd[i]), rel_err(got[i][b], ref[i])
                print("%s %s row %d %s: ratio %.3f, rel-L2 %.2e" % (tag, form, b, name, r, l2))
                worst[i] = max(worst[i], r)
                assert r <= 1.0, (tag, form, b, name, r)
                assert l2 < 6e-3, (tag, form, b, name, l2)
        return worst

    def run(self, ctx, tag, one_pass, want=None):
        """plan, assert the instances, launch, check; want: (dq, dk, dv) instance names -> (gradients, plan)"""
        form = "one_pass" if one_pass else "two_pass"
        pl = self.plan(int(one_pass))
        assert pl.one_pass == int(one_pass)
        if want is not None:
            assert tuple(instance(pl, self.Dp, m) for m in range(3)) == tuple(want), (tag, [instance(pl, self.Dp, m) for m in range(3)])
        got = self.backward(ctx, pl, self.forward(ctx) if one_pass else None)
        self.check(tag, got, form, pl)
        return got, pl

    def two_forms_agree(self, tag, one, two, pl):
        """one-pass against two-pass: within the sum of both bounds"""
        for b in range(self.B):
            b1, b2 = self.reference("one_pass", pl)[b][1], self.reference("two_pass", pl)[b][1]
            for i, name in enumerate(("dq", "dk", "dv")):
                d = ((one[i][b].double() - two[i][b].double()).abs() / (b1[i] + b2[i])).max().item()
                print("%s row %d %s: |one-pass - two-pass| / (sum of the bounds) %.3f" % (tag, b, name, d))
                assert d <= 1.0, (tag, b, name, d)


def names(Dp, pf=(0, 0, 0)):
    lt = 32 if Dp == 160 else 64
    return tuple("attn_bwd_flash_kernel<%d,%d,%d,%s>" % (Dp, lt, m, "true" if pf[m] else "false") for m in range(3))


@pytest.mark.parametrize("dh,Dp", WIDTHS)
def test_self_attention_plain_instances(ctx, dh, Dp):
    """the twelve <DP, LT, MODE, false> instances: Nq = Nk = 192, one and a half block tiles (bok is false in the last one) and three
    (six at LT 32) loop tiles; both dQ forms"""
    for std in (1.0, 3.0):
        case = Case(1, 2, 192, 192, dh, Dp, std=std, seed=3 + int(std))
        two, pl = case.run(ctx, "self 192 Dp %d std %g" % (Dp, std), False, names(Dp))
        assert (pl.nsplit, pl.lt) == (1, 32 if Dp == 160 else 64)
        one, _ = case.run(ctx, "self 192 Dp %d std %g" % (Dp, std), True, names(Dp))
        case.two_forms_agree("self 192 Dp %d" % Dp, one, two, pl)


@pytest.mark.parametrize("Nk", [8, 65, 77, 128])
@pytest.mark.parametrize("dh,Dp", WIDTHS)
def test_cross_attention_unsplit(ctx, dh, Dp, Nk):
    """Nq = 128: Nk 65 leaves ONE key in the last loop tile of the two-pass dQ (LT 64 and 32), 8 is a tile that is almost all masked;
    in dK / dV the Nk keys are the ragged block tile.  The one-pass dQ at Nk 77."""
    for std in (1.0, 3.0):
        case = Case(1, 2, 128, Nk, dh, Dp, std=std, seed=20 + Nk + int(std))
        two, pl = case.run(ctx, "cross Nk %d Dp %d std %g" % (Nk, Dp, std), False, names(Dp))
        assert pl.nsplit == 1
        if Nk == 77:
            one, _ = case.run(ctx, "cross Nk 77 Dp %d std %g" % (Dp, std), True, names(Dp))
            case.two_forms_agree("cross Nk 77 Dp %d" % Dp, one, two, pl)


@pytest.mark.parametrize("Nq,nsplit,rows64,empty64,rows32,empty32", [(320, 2, 192, 0, 160, 0), (576, 4, 192, 1, 160, 0)])
@pytest.mark.parametrize("dh,Dp", WIDTHS)
def test_cross_attention_split(ctx, dh, Dp, Nq, nsplit, rows64, empty64, rows32, empty32):
    """Nk = 77 with the dK / dV walk over the queries split: fp32 partials and attn_bwd_reduce_kernel; uneven shares (192 + 128) at Nq 320,
    an empty fourth share at Nq 576 and LT 64; at Dp 64 / 96 and Nq 576 the split walk runs the PF instances.  Two launches give the same
    bits: every output element has one writer and a fixed summation order."""
    pf = (0, 1, 1) if (Nq == 576 and Dp in (64, 96)) else (0, 0, 0)
    case = Case(1, 2, Nq, 77, dh, Dp, std=1.5, seed=40 + Nq)
    got, pl = case.run(ctx, "split Nq %d Dp %d" % (Nq, Dp), False, names(Dp, pf))
    assert (pl.nsplit, pl.share_rows, pl.empty_shares) == ((nsplit, rows32, empty32) if Dp == 160 else (nsplit, rows64, empty64))
    again = case.backward(ctx, pl)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "the split walk is not deterministic"


@pytest.mark.parametrize("dh,Dp", [(40, 64), (64, 64), (80, 96)])
def test_prefetch_instances(ctx, dh, Dp):
    """the six PF = true instances: Nq = Nk = 512 (eight loop tiles, the least the plan gives them), against the bounds and bit for bit
    against the same launch under abf_prefetch = 0 -- the two differ in staging only; at 40 / 64 also the one-pass dQ"""
    case = Case(1, 2, 512, 512, dh, Dp, std=1.5, seed=60 + dh)
    got, pl = case.run(ctx, "pf Dp %d dh %d" % (Dp, dh), False, names(Dp, (1, 1, 1)))
    with ctx.tuning(abf_prefetch=0):
        twin, _ = case.run(ctx, "pf twin Dp %d dh %d" % (Dp, dh), False, names(Dp))
    for a, b, name in zip(got, twin, ("dq", "dk", "dv")):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), "%s: the prefetch instance and its twin differ" % name
    if dh == 40:
        one, _ = case.run(ctx, "pf Dp 64", True, names(Dp, (1, 1, 1)))
        case.two_forms_agree("pf Dp 64", one, got, pl)


def test_two_batch_rows_three_heads(ctx):
    """B = 2, three heads, one-pass: lse_fwd's batch stride heads * Nq, and a grid of 3 work items padded to 8 (T % 8 != 0)"""
    case = Case(2, 3, 128, 128, 40, 64, std=1.5, seed=70)
    one, pl = case.run(ctx, "B2 H3", True, names(64))
    two, _ = case.run(ctx, "B2 H3", False, names(64))
    case.two_forms_agree("B2 H3", one, two, pl)


@pytest.mark.parametrize("Nq,Nk,dh,Dp,forms", HOSTILE_BWD_SHAPES, ids=["Nk%d-Nq%d-Dp%d" % (s[1], s[0], s[3]) for s in HOSTILE_BWD_SHAPES])
def test_hostile_rows(ctx, Nq, Nk, dh, Dp, forms):
    """hostile_rows' queries (zero, rising, falling, spiked at the last key, far) and hostile_do_rows' dO rows (zero, times 2^8, times
    2^-10), both dQ forms.  The zero dO row's dq is exactly zero; each constructed row is also held on its own."""
    case = Case(1, 2, Nq, Nk, dh, Dp, std=1.0, seed=17, hostile=True)
    for one_pass in (False, True):
        form = "one_pass" if one_pass else "two_pass"
        got, pl = case.run(ctx, "hostile Nk %d Nq %d Dp %d" % (Nk, Nq, Dp), one_pass)
        ref, bnd = case.reference(form, pl)[0]
        assert (got[0][0][:, DO_ZERO] == 0).all(), "a zero dO row has a zero dq"
        for name, i in (("spike", Q_SPIKE), ("dO zero", DO_ZERO), ("dO big", DO_BIG), ("dO tiny", DO_TINY)):
            r = ratio(got[0][0][:, i], ref[0][:, i], bnd[0][:, i])
            print("hostile Nk %d Nq %d Dp %d %s: dq ratio of the %s row %.3f" % (Nk, Nq, Dp, form, name, r))
            assert r <= 1.0, (name, r)


@pytest.mark.parametrize("Nq,Nk,dh,Dp", [(72, 72, 8, 32), (72, 72, 40, 64), (4, 4, 40, 64), (128, 136, 40, 64)])
def test_materialised_fallback(ctx, Nq, Nk, dh, Dp):
    """only the shapes the fallback alone serves: Nq no multiple of 64, Nq below 64, more than 128 cross-attention keys"""
    for std in (1.0, 3.0):
        case = Case(1, 2, Nq, Nk, dh, Dp, std=std, seed=80 + Nq + int(std), zero_pad=True)
        pl = case.plan(0, flash=False)
        assert instance(pl, Dp, 0) == "materialised" and (pl.lt, pl.nsplit, pl.one_pass) == (0, 1, 0)
        assert pl.scratch_bytes == ctx.lib.pnpi_op_attention_bwd_scratch_bytes(Nq, Nk, dh)
        got = case.backward(ctx, pl)
        case.check("materialised Nq %d Nk %d Dp %d std %g" % (Nq, Nk, Dp, std), got, "materialised", pl)


def test_refusals_leave_every_canary(ctx):
    """a misaligned leading dimension or offset (PNPI_ESHAPE) and a null pointer (PNPI_EINVAL) are refused before anything is launched"""
    case = Case(1, 2, 128, 128, 40, 64, seed=90)
    pl = case.plan(0)
    nbytes = pl.scratch_bytes
    scratch = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    gq, gk, gv, gbufs = case.grads()
    good = case.args(gq, gk, gv, scratch, nbytes, None)
    for idx, val, err in ((1, case.ldq + 4, _capi.PNPI_ESHAPE), (2, 4, _capi.PNPI_ESHAPE), (5, case.k_off + 2, _capi.PNPI_ESHAPE),
                          (10, case.ldo + 4, _capi.PNPI_ESHAPE), (0, None, _capi.PNPI_EINVAL), (9, None, _capi.PNPI_EINVAL),
                          (18, None, _capi.PNPI_EINVAL), (20, None, _capi.PNPI_EINVAL)):
        bad = list(good)
        bad[idx] = val
        assert ctx.lib.pnpi_op_attention_bwd_fwd(ctx.h, *bad) == err, (idx, val)
    torch.cuda.synchronize()
    for buf, _ in gbufs:
        assert (buf == G_CANARY).all()
    assert (scratch == 0x5A).all()
    assert ctx.lib.pnpi_op_attention_bwd_fwd(ctx.h, *good) == 0      # and the same arguments, unspoilt, run
    torch.cuda.synchronize()
    assert case.untouched(gbufs)
