"""Every instance launch_attn_flash dispatches, the causal flag, the log-sum-exp hand-over to the flash backward and the cross-edit
kernel's source row, each against float64 softmax attention of the fp16 inputs under the per-element bound for O and the per-query bound
for lse that tests/test_attn_bound_host.py derives (applied unchanged), with guard bands checked bit for bit:

  * Q and K are column ranges of ONE fused buffer (q_off = 8, k_off = heads * Dp + 16, ld = 3 * heads * Dp + 24) in which every column
    outside the two head ranges, and every line the launch does not own, is NaN;
  * V^T's pad columns past Nk are NaN;
  * O has ldo = heads * dh + 8 and one row more than any launch writes, lse one row more, both filled with a canary that has to survive.

Instance -> case (test_every_forward_instance; Nq = 130, two heads, input std 1 and 3):
    attn_flash_kernel<32, false>   Nk  65 dh   8      attn_flash_kernel<32, true>   Nk 129 dh   8
    attn_flash_kernel<64, false>   Nk  65 dh  40      attn_flash_kernel<64, true>   Nk 129 dh  40   (Nk % 64 != 0: not the DMA kernel)
    attn_flash_kernel<96, false>   Nk  65 dh  80      attn_flash_kernel<96, true>   Nk 129 dh  80
    attn_flash_kernel<128, false>  Nk  65 dh 128      attn_flash_kernel<128, true>  Nk 129 dh 128
    attn_flash_kernel<160, false>  Nk  65 dh 160      attn_flash_kernel<160, true>  Nk 129 dh 160
    attn_flash_dma64_kernel<false, 3>        Nk 128 / 192 dh 40            <true, 3>        the same, op_attention_vt_perm
    attn_flash_dma64_kernel<false, 3, true>  Nk 128 / 192 dh 40, aug       <true, 3, true>  the same, op_attention_vt_perm
    attn_flash_dma64_kernel<false, 4>        Nk 128 / 192 dh 64            <true, 4>        the same, op_attention_vt_perm
Neighbouring paths: the DMA kernel against attn_flash_kernel<128, false> on the same values laid out with Dp = 128; the permuted key order
against the plain one (bit-identical); aug against plain.  PF = true against PF = false on the same data has no means without an
environment switch (the choice is Nk > 128 alone), so that comparison is not made.

Worst |got - ref| / bound on an MI355X (O, lse): plain 0.38, 0.12; DMA 0.35, 0.10; aug 0.45, 0.17; causal 0.39, 0.12; the hand-over's
forward 0.41, 0.06; work decode 0.42, 0.06; cross-edit source row 0.38.  The whole file runs in about five seconds."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402
from tests.test_attn_bound_host import (HOSTILE_SHAPES, NQ, Q_FALL, Q_FAR, Q_RISE, Q_SPIKE, Q_ZERO, attn_inputs, bounds, hostile_rows,  # noqa: E402
                                        ratio)

DEV = "cuda"
O_CANARY = -77.25            # exactly representable in fp16
LSE_CANARY = -12345.5


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


class Case:
    """B batch rows of q [heads, Nq, dh], k / v [heads, Nk, dh] (fp16 values, kept for the reference) in the poisoned device layout"""

    def __init__(self, B, heads, Nq, Nk, dh, Dp, std=1.0, seed=0, aug=False, perm=False, hostile=False, out_rows=None):
        self.B, self.heads, self.Nq, self.Nk, self.dh, self.Dp, self.aug, self.perm = B, heads, Nq, Nk, dh, Dp, aug, perm
        self.scale = dh ** -0.5
        qs, ks, vs = [], [], []
        for i in range(B * heads):
            q, k, v = attn_inputs(Nq, Nk, dh, std, 1000 * seed + i)
            if hostile:
                hostile_rows(q, k, v, self.scale)
            qs.append(q), ks.append(k), vs.append(v)
        self.q = torch.stack(qs).reshape(B, heads, Nq, dh).to(DEV)
        self.k = torch.stack(ks).reshape(B, heads, Nk, dh).to(DEV)
        self.v = torch.stack(vs).reshape(B, heads, Nk, dh).to(DEV)
        hd = heads * Dp
        self.ld, self.q_off, self.k_off = 3 * hd + 24, 8, hd + 16
        self.fused = torch.full((B * max(Nq, Nk), self.ld), float("nan"), dtype=torch.half, device=DEV)
        qp = torch.zeros(B, Nq, heads, Dp, dtype=torch.half, device=DEV)
        kp = torch.zeros(B, Nk, heads, Dp, dtype=torch.half, device=DEV)
        qp[..., :dh] = self.q.permute(0, 2, 1, 3)
        kp[..., :dh] = self.k.permute(0, 2, 1, 3)
        if aug:
            kp[..., dh] = 1.0
        self.fused[:B * Nq, self.q_off:self.q_off + hd] = qp.reshape(B * Nq, hd)
        self.fused[:B * Nk, self.k_off:self.k_off + hd] = kp.reshape(B * Nk, hd)
        self.ldv = (Nk + 7) // 8 * 8
        vt = torch.full((B, heads, Dp, self.ldv), float("nan"), dtype=torch.half, device=DEV)
        vt[..., :Nk] = 0
        vt[:, :, :dh, :Nk] = self.v.transpose(2, 3)
        if aug:
            vt[:, :, dh, :Nk] = 1.0
        if perm:      # each aligned 16-token group stored [0-3, 8-11, 4-7, 12-15] (ops.h vt_perm16_pos)
            assert Nk % 16 == 0
            pos = torch.arange(Nk, device=DEV)
            swap = (((pos >> 2) ^ (pos >> 3)) & 1).bool()
            vtp = vt.clone()
            vtp[..., torch.where(swap, pos ^ 12, pos)] = vt[..., pos]
            vt = vtp
        self.vt = vt.contiguous()
        self.out_rows = (B if out_rows is None else out_rows) + 1      # one row no launch writes
        self.ldo = heads * dh + 8
        self.form = "aug" if aug else "plain"

    def launch(self, ctx, rows, causal=0, want_lse=True):
        """-> (O [out_rows, Nq, ldo], lse [out_rows, heads, Nq] or None, rows as a list)"""
        o = torch.full((self.out_rows, self.Nq, self.ldo), O_CANARY, dtype=torch.half, device=DEV)
        lse = torch.full((self.out_rows, self.heads, self.Nq), LSE_CANARY, dtype=torch.float32, device=DEV) if want_lse else None
        rows_dev = torch.tensor(rows, dtype=torch.int32, device=DEV).reshape(-1, 4).contiguous()
        assert max(r[0] for r in rows) < self.out_rows - 1 and max(max(r[1:]) for r in rows) < self.B
        with ctx.tuning(op_attention_aug=int(self.aug), op_attention_vt_perm=int(self.perm)):
            ctx.call("pnpi_op_attention_ex", ptr(self.fused), self.ld, self.q_off, ptr(self.fused), self.ld, self.k_off, ptr(self.vt), self.ldv,
                     ptr(o), self.ldo, self.heads, self.Nq, self.Nk, self.Dp, self.dh, self.scale, ptr(rows_dev), len(rows), causal,
                     ptr(lse) if want_lse else None)
            torch.cuda.synchronize()
        return o, lse

    def check(self, tag, o, lse, rows, causal=0):
        """the per-element O bound, the per-query lse bound, the old relative L2, and the guard bands; -> (worst O ratio, worst lse ratio)"""
        hdh = self.heads * self.dh
        wo, wl = 0.0, 0.0
        for orow, qrow, krow, vrow in rows:
            ref, bo, rl, bl = bounds(self.q[qrow], self.k[krow], self.v[vrow], self.scale, self.form, self.Dp, bool(causal))
            got = o[orow, :, :hdh].reshape(self.Nq, self.heads, self.dh).permute(1, 0, 2)
            ro = ratio(got, ref, bo)
            l2 = rel_err(got, ref)
            wo = max(wo, ro)
            if lse is not None:
                rlse = ratio(lse[orow], rl, bl)
                wl = max(wl, rlse)
            print("%s row %s: O ratio %.3f, lse ratio %.3f, rel-L2 %.2e" % (tag, (orow, qrow, krow, vrow), ro, rlse if lse is not None else -1, l2))
            assert ro <= 1.0, (tag, orow, ro)
            if lse is not None:
                assert rlse <= 1.0, (tag, orow, rlse)
            assert l2 < 3e-3, (tag, orow, l2)
        written = sorted(set(r[0] for r in rows))
        keep = torch.ones_like(o, dtype=torch.bool)
        keep[written, :, :hdh] = False
        canary = torch.full_like(o, O_CANARY)
        assert torch.equal(o.view(torch.int16)[keep], canary.view(torch.int16)[keep]), (tag, "O: a pad column or a row not listed was written")
        if lse is not None:
            keepl = torch.ones_like(lse, dtype=torch.bool)
            keepl[written] = False
            assert torch.equal(lse[keepl], torch.full_like(lse, LSE_CANARY)[keepl]), (tag, "lse: a row not listed was written")
        return wo, wl


IDENT = [(0, 0, 0, 0)]

INSTANCES = [
    # (instance, Nk, dh, Dp, aug, perm)
    ("attn_flash_kernel<32,false>", 65, 8, 32, 0, 0), ("attn_flash_kernel<32,true>", 129, 8, 32, 0, 0),
    ("attn_flash_kernel<64,false>", 65, 40, 64, 0, 0), ("attn_flash_kernel<64,true>", 129, 40, 64, 0, 0),
    ("attn_flash_kernel<96,false>", 65, 80, 96, 0, 0), ("attn_flash_kernel<96,true>", 129, 80, 96, 0, 0),
    ("attn_flash_kernel<128,false>", 65, 128, 128, 0, 0), ("attn_flash_kernel<128,true>", 129, 128, 128, 0, 0),
    ("attn_flash_kernel<160,false>", 65, 160, 160, 0, 0), ("attn_flash_kernel<160,true>", 129, 160, 160, 0, 0),
    ("attn_flash_dma64_kernel<false,3>", 128, 40, 64, 0, 0), ("attn_flash_dma64_kernel<false,3>", 192, 40, 64, 0, 0),
    ("attn_flash_dma64_kernel<true,3>", 128, 40, 64, 0, 1), ("attn_flash_dma64_kernel<true,3>", 192, 40, 64, 0, 1),
    ("attn_flash_dma64_kernel<false,3,true>", 128, 40, 64, 1, 0), ("attn_flash_dma64_kernel<false,3,true>", 192, 40, 64, 1, 0),
    ("attn_flash_dma64_kernel<true,3,true>", 128, 40, 64, 1, 1), ("attn_flash_dma64_kernel<true,3,true>", 192, 40, 64, 1, 1),
    ("attn_flash_dma64_kernel<false,4>", 128, 64, 64, 0, 0), ("attn_flash_dma64_kernel<false,4>", 192, 64, 64, 0, 0),
    ("attn_flash_dma64_kernel<true,4>", 128, 64, 64, 0, 1), ("attn_flash_dma64_kernel<true,4>", 192, 64, 64, 0, 1),
]


@pytest.mark.parametrize("inst,Nk,dh,Dp,aug,perm", INSTANCES, ids=["%s-Nk%d" % (i[0], i[1]) for i in INSTANCES])
def test_every_forward_instance(ctx, inst, Nk, dh, Dp, aug, perm):
    """one launch per instance of launch_attn_flash's dispatch (the module docstring's table), Nq = 130: one full workgroup plus two
    queries; Nk = 65 / 129: the last tile holds one key; Nk = 128 / 192: the DMA ring's minimum and an odd number of tiles"""
    for std in (1.0, 3.0):
        case = Case(1, 2, NQ, Nk, dh, Dp, std=std, seed=3 + int(std), aug=bool(aug), perm=bool(perm))
        o, lse = case.launch(ctx, IDENT)
        case.check("%s Nk %d std %g" % (inst, Nk, std), o, lse, IDENT)


@pytest.mark.parametrize("Nk,dh", [(128, 40), (192, 40), (128, 64), (192, 64)])
def test_neighbouring_paths_differ_by_rounding_only(ctx, Nk, dh):
    """the same values through the DMA kernel, through its permuted-key-order instance (bit-identical: the same numbers in the same
    order), through attn_flash_kernel<128, false / true> (the same heads laid out with Dp = 128: other staging, other LDS layout, the same
    arithmetic) and, at dh = 40, through the aug form"""
    base = Case(1, 2, NQ, Nk, dh, 64, std=2.0, seed=9)
    o, lse = base.launch(ctx, IDENT)
    base.check("dma", o, lse, IDENT)
    ref, bo, rl, bl = bounds(base.q[0], base.k[0], base.v[0], base.scale, "plain", 64)
    hdh = 2 * dh

    def heads_of(x):
        return x[0, :, :hdh].reshape(NQ, 2, dh).permute(1, 0, 2).double()

    others = [("perm", Case(1, 2, NQ, Nk, dh, 64, std=2.0, seed=9, perm=True)), ("Dp128", Case(1, 2, NQ, Nk, dh, 128, std=2.0, seed=9))]
    if dh == 40:
        others.append(("aug", Case(1, 2, NQ, Nk, dh, 64, std=2.0, seed=9, aug=True)))
    for name, other in others:
        assert torch.equal(other.q, base.q) and torch.equal(other.v, base.v)
        o2, lse2 = other.launch(ctx, IDENT)
        other.check(name, o2, lse2, IDENT)
        if name == "perm":
            assert torch.equal(o2, o) and torch.equal(lse2, lse)
        else:      # each within its own bound of the reference, and of the other within the looser of the two bounds
            _, bo2, _, bl2 = bounds(base.q[0], base.k[0], base.v[0], base.scale, other.form, other.Dp)
            d = ((heads_of(o2) - heads_of(o)).abs() / torch.maximum(bo, bo2)).max().item()
            dl = ((lse2[0].double() - lse[0].double()).abs() / torch.maximum(bl, bl2)).max().item()
            print("dma vs %s, Nk %d dh %d: |difference| / bound: O %.3f, lse %.3f" % (name, Nk, dh, d, dl))
            assert d <= 1.0 and dl <= 1.0, (name, d, dl)


DECODE = [
    # (work items, B, heads, Nq, Nk, rows): heads * nrows * ceil(Nq / 128) work items in a grid padded to a multiple of 8
    (1, 2, 1, 100, 77, [(1, 0, 1, 0)]),                                                        # nrows < batch; 7 padding workgroups
    (3, 4, 3, 64, 77, [(2, 3, 0, 1)]),                                                         # four distinct entries
    (9, 4, 3, 100, 128, [(2, 0, 1, 3), (0, 3, 3, 1), (3, 1, 0, 0)]),                           # 9 of 16; output row 1 not listed
    (17, 5, 1, 32, 128, [(i, i % 5, (2 * i + 1) % 5, (3 * i + 2) % 5) for i in range(17)]),    # every batch row a source several times
]


@pytest.mark.parametrize("items,B,heads,Nq,Nk,rows", DECODE, ids=["items%d" % d[0] for d in DECODE])
def test_work_decode_and_row_indirection(ctx, items, B, heads, Nq, Nk, rows):
    """flash_decode: grids whose work-item count is no multiple of 8 (the padding workgroups return, the XCD deal leaves no item out and
    takes none twice), rows[] with four distinct entries, fewer rows than the batch, batch rows read by several outputs"""
    assert heads * len(rows) * ((Nq + 127) // 128) == items
    case = Case(B, heads, Nq, Nk, 40, 64, std=1.5, seed=items, out_rows=max(r[0] for r in rows) + 1)
    o, lse = case.launch(ctx, rows)
    case.check("decode %d" % items, o, lse, rows)


@pytest.mark.parametrize("Nk,dh,Dp,aug,perm", HOSTILE_SHAPES)
def test_rows_that_move_the_running_reference(ctx, Nk, dh, Dp, aug, perm):
    """tests/test_attn_bound_host.py hostile_rows: a zero query (the mean of V), a query whose logits rise by more than 8 from tile to tile
    (a rescale on every tile), one whose maximum is in tile 0 (none), a spike at the last key (of a ragged last tile where Nk % 64 != 0),
    and a query whose every score is below -8 in the log2 domain (the host file asserts that at these shapes and seeds): the aug form is
    right on that row only if its first tile moves the reference point down"""
    case = Case(1, 2, NQ, Nk, dh, Dp, std=1.0, seed=17, aug=bool(aug), perm=bool(perm), hostile=True)
    o, lse = case.launch(ctx, IDENT)
    case.check("hostile Nk %d Dp %d aug %d" % (Nk, Dp, aug), o, lse, IDENT)
    ref, bo, rl, bl = bounds(case.q[0], case.k[0], case.v[0], case.scale, case.form, Dp)
    got = o[0, :, :2 * dh].reshape(NQ, 2, dh).permute(1, 0, 2).double()
    vd = case.v[0].double()
    assert ((got[:, Q_ZERO] - vd.mean(1)).abs() <= bo[:, Q_ZERO]).all()                   # directly: the mean of V
    assert ((got[:, Q_SPIKE] - vd[:, Nk - 1]).abs() <= bo[:, Q_SPIKE] + (ref[:, Q_SPIKE] - vd[:, Nk - 1]).abs()).all()
    for i in (Q_ZERO, Q_RISE, Q_FALL, Q_SPIKE, Q_FAR):
        assert rel_err(got[:, i], ref[:, i]) < 3e-3, i
    far_o, far_lse = ratio(got[:, Q_FAR], ref[:, Q_FAR], bo[:, Q_FAR]), ratio(lse[0, :, Q_FAR], rl[:, Q_FAR], bl[:, Q_FAR])
    print("hostile Nk %d Dp %d aug %d: the far query's O ratio %.3f, lse ratio %.3f" % (Nk, Dp, aug, far_o, far_lse))
    assert far_o <= 1.0 and far_lse <= 1.0, (far_o, far_lse)


@pytest.mark.parametrize("dh,Dp", [(40, 64), (8, 32), (160, 160)])
def test_one_key(ctx, dh, Dp):
    """Nk = 1: P = 1 and l = 1 exactly, the output is v_0 itself"""
    case = Case(1, 2, NQ, 1, dh, Dp, std=3.0, seed=21)
    o, lse = case.launch(ctx, IDENT)
    case.check("one key", o, lse, IDENT)
    got = o[0, :, :2 * dh].reshape(NQ, 2, dh).permute(1, 0, 2)
    assert torch.equal(got, case.v[0].expand(2, NQ, dh))


@pytest.mark.parametrize("N,dh,Dp", [(77, 64, 64), (130, 64, 64), (200, 64, 64), (77, 8, 32), (130, 8, 32), (200, 8, 32), (128, 40, 64), (128, 64, 64)])
def test_causal(ctx, N, dh, Dp):
    """AttnP::causal (the CLIP text encoder's launch; 64 / 64 is its head) against the reference masked with triu(1); N = 128 with Dp = 64
    is a shape the DMA kernel would take without the flag.  Query 0 sees key 0 only."""
    for std in (1.0, 3.0):
        case = Case(2, 2, N, N, dh, Dp, std=std, seed=30 + int(std))
        rows = [(0, 0, 0, 0), (1, 1, 1, 1)]
        o, lse = case.launch(ctx, rows, causal=1)
        case.check("causal N %d Dp %d std %g" % (N, Dp, std), o, lse, rows, causal=1)
        got = o[:2, :, :2 * dh].reshape(2, N, 2, dh)
        assert torch.equal(got[:, 0], case.v[:, :, 0])
        # and it is not the unmasked result
        o2, _ = case.launch(ctx, rows, causal=0, want_lse=False)
        assert not torch.equal(o2, o)


def test_ex_refuses_null_pointers(ctx):
    case = Case(1, 2, 64, 64, 8, 32)
    o = torch.zeros(2, 64, case.ldo, dtype=torch.half, device=DEV)
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    good = [ptr(case.fused), case.ld, case.q_off, ptr(case.fused), case.ld, case.k_off, ptr(case.vt), case.ldv, ptr(o), case.ldo, 2, 64, 64, 32, 8,
            case.scale, ptr(rows), 1, 0, None]
    assert ctx.lib.pnpi_op_attention_ex(ctx.h, *good) == 0
    for i in (0, 3, 6, 8, 16):
        bad = list(good)
        bad[i] = None
        assert ctx.lib.pnpi_op_attention_ex(ctx.h, *bad) == _capi.PNPI_EINVAL, i
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the hand-over to the backward
def _counters(ctx):
    c = _capi.Counters()
    assert ctx.lib.pnpi_get_counters(ctx.h, C.byref(c)) == 0
    return c.executed_attn_flops


@pytest.mark.parametrize("B,Nq,Nk,dh,Dp", [(2, 128, 128, 40, 64), (1, 128, 128, 64, 64), (1, 192, 192, 80, 96), (2, 64, 64, 160, 160), (2, 128, 77, 40, 64)])
def test_forward_lse_feeds_the_one_pass_dq(ctx, B, Nq, Nk, dh, Dp):
    """pnpi_op_attention_ex leaves lse and O; pnpi_op_attention_bwd_fwd hands them to the flash backward, whose dQ then skips its first
    pass over the keys (3 tile products instead of 5, seen in executed_attn_flops).  dq / dk / dv against float64 autograd and against the
    two-pass dQ (lse_fwd = NULL) at test_attention_bwd_flash's tolerances.  The forward reads q and k from the NaN-poisoned buffer of every
    other case here (q_off = 8, k_off = heads * Dp + 16, ld = 3 * heads * Dp + 24); the backward reads the same values as column ranges of
    q | k | v as in the model (cross-attention: q alone, k | v together), because it needs v row-major next to them, which that layout has
    no room for; gradient columns outside the heads' dh stay untouched."""
    heads = 2
    hd = heads * Dp
    scale = dh ** -0.5
    g = torch.Generator().manual_seed(50 + Nk + dh)

    def padded(n, amp):
        t = torch.zeros(B, n, heads, Dp)
        t[..., :dh] = torch.randn(B, n, heads, dh, generator=g) * amp
        return t.reshape(B * n, hd).half().to(DEV)

    q, k, v = padded(Nq, 1.5), padded(Nk, 1.5), padded(Nk, 1.0)
    d_o = torch.randn(B * Nq, heads * dh, generator=g).half().to(DEV)
    if Nq == Nk:
        qkv = torch.cat([q, k, v], 1).contiguous()
        qb, ldq, q_off, kb, ldk, k_off, vb, ldvb, v_off = qkv, 3 * hd, 0, qkv, 3 * hd, hd, qkv, 3 * hd, 2 * hd
    else:
        kv = torch.cat([k, v], 1).contiguous()
        qb, ldq, q_off, kb, ldk, k_off, vb, ldvb, v_off = q, hd, 0, kv, 2 * hd, 0, kv, 2 * hd, hd
    ld, fq_off, fk_off = 3 * hd + 24, 8, hd + 16
    fused = torch.full((B * max(Nq, Nk), ld), float("nan"), dtype=torch.half, device=DEV)
    fused[:B * Nq, fq_off:fq_off + hd] = q
    fused[:B * Nk, fk_off:fk_off + hd] = k
    ldv = (Nk + 7) // 8 * 8
    vt = torch.full((B, heads, Dp, ldv), float("nan"), dtype=torch.half, device=DEV)
    vt[..., :Nk] = v.reshape(B, Nk, heads, Dp).permute(0, 2, 3, 1)
    ldo = heads * dh + 8
    o = torch.full((B + 1, Nq, ldo), O_CANARY, dtype=torch.half, device=DEV)
    lse = torch.full((B + 1, heads, Nq), LSE_CANARY, dtype=torch.float32, device=DEV)
    rows = torch.arange(B, dtype=torch.int32, device=DEV).repeat_interleave(4).contiguous()
    ctx.call("pnpi_op_attention_ex", ptr(fused), ld, fq_off, ptr(fused), ld, fk_off, ptr(vt), ldv, ptr(o), ldo, heads, Nq, Nk, Dp, dh, scale,
             ptr(rows), B, 0, ptr(lse))
    torch.cuda.synchronize()
    qh, kh, vh = [t.reshape(B, -1, heads, Dp)[..., :dh].permute(0, 2, 1, 3) for t in (q, k, v)]
    form = "plain"
    for b in range(B):
        ref, bo, rl, bl = bounds(qh[b], kh[b], vh[b], scale, form, Dp)
        got_o = o[b, :, :heads * dh].reshape(Nq, heads, dh).permute(1, 0, 2)
        ro, rlse, l2 = ratio(got_o, ref, bo), ratio(lse[b], rl, bl), rel_err(got_o, ref)
        print("hand-over forward Nq %d Nk %d Dp %d row %d: O ratio %.3f, lse ratio %.3f, rel-L2 %.2e" % (Nq, Nk, Dp, b, ro, rlse, l2))
        assert ro <= 1.0 and rlse <= 1.0 and l2 < 3e-3, (b, ro, rlse, l2)
    assert (o[B] == O_CANARY).all() and (o[:, :, heads * dh:] == O_CANARY).all() and (lse[B] == LSE_CANARY).all()

    qr, kr, vr = [t.double().contiguous().requires_grad_(True) for t in (qh, kh, vh)]
    (torch.softmax(scale * qr @ kr.transpose(-1, -2), -1) @ vr).backward(d_o.double().reshape(B, Nq, heads, dh).permute(0, 2, 1, 3))
    nbytes = ctx.lib.pnpi_op_attention_bwd_scratch_bytes(Nq, Nk, dh) * heads + (64 << 20)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    G_CANARY = 3.5
    got, flops = {}, {}
    for with_lse in (1, 0):
        if Nq == Nk:      # one gradient buffer in the layout of q | k | v
            gq = gk = gv = torch.full_like(qb, G_CANARY)
            bufs = [(gq, (q_off, k_off, v_off))]
        else:
            gq, gk = torch.full_like(qb, G_CANARY), torch.full_like(kb, G_CANARY)
            gv = gk
            bufs = [(gq, (q_off,)), (gk, (k_off, v_off))]
        f0 = _counters(ctx)
        ctx.call("pnpi_op_attention_bwd_fwd", ptr(qb), ldq, q_off, ptr(kb), ldk, k_off, ptr(vb), ldvb, v_off, ptr(d_o), heads * dh, heads, Nq, Nk, Dp, dh,
                 scale, B, ptr(gq), ptr(gk), ptr(gv), ptr(scratch), nbytes, ptr(lse) if with_lse else None, ptr(o) if with_lse else None,
                 ldo if with_lse else 0)
        torch.cuda.synchronize()
        flops[with_lse] = _counters(ctx) - f0
        got[with_lse] = (gq[:, q_off:q_off + hd], gk[:, k_off:k_off + hd], gv[:, v_off:v_off + hd])
        for buf, offs in bufs:
            keep = torch.ones(buf.shape[1], dtype=torch.bool, device=DEV)
            for off in offs:
                for h in range(heads):
                    keep[off + h * Dp:off + h * Dp + dh] = False
            assert (buf[:, keep] == G_CANARY).all(), "a gradient column outside the heads' dh columns was written"
    unit = 2.0 * heads * Nq * Nk * Dp * B
    assert flops[1] == unit * (3 + 3 + 2) and flops[0] == unit * (5 + 3 + 2), (flops, unit)      # the one-pass dQ was taken / was not
    for name, i, ref, n in (("dq", 0, qr.grad, Nq), ("dk", 1, kr.grad, Nk), ("dv", 2, vr.grad, Nk)):
        for with_lse in (1, 0):
            gh = got[with_lse][i].float().reshape(B, n, heads, Dp)[..., :dh].permute(0, 2, 1, 3)
            e = rel_err(gh, ref)
            print("hand-over backward %s with_lse %d: rel-L2 %.2e" % (name, with_lse, e))
            assert e < 6e-3, (name, with_lse, e)
        a, b2 = got[1][i].float(), got[0][i].float()
        sel = torch.zeros(hd, dtype=torch.bool, device=DEV)
        for h in range(heads):
            sel[h * Dp:h * Dp + dh] = True
        assert rel_err(a[:, sel], b2[:, sel]) < 4e-3, (name, rel_err(a[:, sel], b2[:, sel]))


# ------------------------------------------------------------------------------------------------ cross-edit
@pytest.mark.parametrize("Nk,dh,Dp", [(8, 40, 64), (77, 40, 64), (96, 40, 64), (77, 160, 160)])
def test_cross_edit_two_pairs_in_a_fused_buffer(ctx, Nk, dh, Dp):
    """pnpi_op_cross_edit with two distinct (source, target) pairs, q / k at non-zero offsets of one poisoned buffer, 8 / 77 / 96 keys and a
    canary gap in O.  test_cross_edit's tolerances, plus the per-element bound on the source rows, which are plain softmax attention."""
    B, heads, Nq = 5, 2, NQ
    case = Case(B, heads, Nq, Nk, dh, Dp, std=1.5, seed=60 + Nk)
    pairs = [(2, 3), (4, 0)]
    g = torch.Generator().manual_seed(5)
    mm = torch.eye(Nk).repeat(2, 1, 1)
    mm[0, 3, 3] = 0; mm[0, 3, 4] = 0.5; mm[0, 3, 5] = 0.5; mm[1, 1] = 0; mm[1, 1, Nk - 1] = 1.0
    c1, c2 = torch.rand(2, 96, generator=g), torch.rand(2, 96, generator=g)
    mmT = torch.zeros(2, 96, 96)
    mmT[:, :Nk, :Nk] = mm.transpose(1, 2)
    mmT16, c1d, c2d = mmT.half().to(DEV).contiguous(), c1.to(DEV), c2.to(DEV)
    pairs_dev = torch.tensor(pairs, dtype=torch.int32, device=DEV)
    o = torch.full((B + 1, Nq, case.ldo), O_CANARY, dtype=torch.half, device=DEV)
    ctx.call("pnpi_op_cross_edit", ptr(case.fused), case.ld, case.q_off, ptr(case.fused), case.ld, case.k_off, ptr(case.vt), case.ldv, ptr(o),
             case.ldo, heads, Nq, Nk, Dp, dh, case.scale, ptr(pairs_dev), 2, ptr(mmT16), ptr(c1d), ptr(c2d), None, None, 0, 2 * heads)
    torch.cuda.synchronize()
    hdh = heads * dh
    p = (case.q.double() @ case.k.double().transpose(-1, -2) * float(torch.tensor(case.scale, dtype=torch.float32))).softmax(-1)
    for pi, (src, tgt) in enumerate(pairs):
        ref, bo, _, _ = bounds(case.q[src], case.k[src], case.v[src], case.scale, "cross", Dp)
        got_src = o[src, :, :hdh].reshape(Nq, heads, dh).permute(1, 0, 2)
        r = ratio(got_src, ref, bo)
        print("cross-edit Nk %d Dp %d pair %d: source-row O ratio %.3f, rel-L2 %.2e" % (Nk, Dp, pi, r, rel_err(got_src, ref)))
        assert r <= 1.0, (pi, r)
        assert rel_err(got_src, ref) < 3e-3
        pnew = c1d[pi, :Nk].double() * (p[src] @ mm[pi].double().to(DEV)) + c2d[pi, :Nk].double() * p[tgt]
        ref_tgt = pnew @ case.v[tgt].double()
        got_tgt = o[tgt, :, :hdh].reshape(Nq, heads, dh).permute(1, 0, 2)
        assert rel_err(got_tgt, ref_tgt) < 4e-3, (pi, rel_err(got_tgt, ref_tgt))
    keep = torch.ones_like(o, dtype=torch.bool)
    keep[[2, 3, 4, 0], :, :hdh] = False
    assert torch.equal(o.view(torch.int16)[keep], torch.full_like(o, O_CANARY).view(torch.int16)[keep])      # row 1, the spare row, the gap
