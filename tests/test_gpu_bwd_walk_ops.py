"""The reverse walk's kernels (csrc/bwd.hip) in the forms tape_backward launches them, element by element.

GroupNorm / LayerNorm backward against the float64 references of tests/test_norm_bwd_bound_host.py under that module's per-element
bounds, imported unchanged (kappa = 32768, kappa_ln = 8192: how they are measured is written there).  The three-phase GroupNorm kernel
runs with the walk's destinations -- dense, two separate buffers, either accumulating, either absent, padded row strides -- between
4 KiB guard bands of a canary bit pattern, with a NaN-filled caller's scratch, twice, and one sample at a time; whatever is not a bound
is bit-exact.  The gradient plumbing (strided_add, accumulate, sumpool2x2, zero_stuff2, pad_heads, add_f16_to_f32, transpose,
repack_dgrad) is one fp32 operation and one rounding per element, so it is compared bit for bit with torch.

Worst |err| / bound over all destination forms, as printed by the first run on an MI355X (the bound admits 1):

    (B, C1, C2, HW, G, silu)        dense   split   acc1    acc2        (acc1: dx1 accumulates, dx2 overwrites; acc2 the reverse)
    (3, 64, 0, 200, 32, 1)          0.199   0.199   0.919   -
    (2, 8, 24, 50, 32, 1)           0.196   0.196   0.795   0.863
    (2, 64, 32, 64, 32, 1)          0.198   0.198   0.898   0.905
    (1, 1280, 640, 256, 32, 1)      0.389   0.389   0.965   0.923
    (1, 1280, 1280, 64, 32, 1)      0.203   0.203   0.832   0.850
    (1, 1280, 0, 1100, 32, 0)       0.200   0.200   0.907   -
    (1, 640, 320, 4096, 32, 1)      0.317   0.317   0.965   0.977
    (2, 128, 0, 96, 64, 1)          0.196   0.196   0.943   -
    (2, 64, 64, 96, 16, 0)          0.197   0.197   0.912   0.883
    one block per group: (2, 12, 20, 40, G = 4) 0.193, (2, 64, 32, 64, G = 32) 0.198
    LayerNorm (M, C): (1, 32) 0.349  (7, 32) 0.428  (1, 520) 0.476  (7, 520) 0.488  (1, 1032) 0.482  (7, 1032) 0.491  (1, 2048) 0.480
    (7, 2048) 0.497

The plain stores sit where the host emulation does (0.2 is the fp16 half-ulp against this kappa; 0.317 and 0.497 are the emulation's own
worst cases, to three digits).  The accumulating stores come close to 1 by construction: the second rounding may spend all of its own
term 2^-11 |old + r| (the emulation's worst is 0.977 as well).
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi  # noqa: E402
from tests import test_norm_bwd_bound_host as H  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402
from tests.test_gpu_kernels import h16, nhwc, pack_w  # noqa: E402

DEV = "cuda"
CANARY = 0x6B5A            # an fp16 bit pattern (3764.0) no result of these tests equals by accident in a whole band
GUARD = 2048               # halfs: 4 KiB on either side of every destination
GRID_VECS = 2048 * 256     # threads of the capped grids: more vectors than this and the grid-stride loops make a second trip


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


class Guarded:
    """rows x ld halfs (the first `cols` of a row are the tensor) between two guard bands, everything preset to the canary"""

    def __init__(self, rows, ld, cols, fill=None, guard=GUARD):
        self.rows, self.ld, self.cols, self.guard = rows, ld, cols, guard
        self.raw = torch.full((guard + rows * ld + guard,), CANARY, dtype=torch.int16, device=DEV)
        self.body = self.raw[guard:guard + rows * ld].view(torch.half).reshape(rows, ld)
        if fill is not None:
            self.body[:, :cols] = fill.reshape(rows, cols)

    @property
    def p(self):
        return ptr(self.body)

    def data(self):
        return self.body[:, :self.cols].clone()

    def intact(self):
        """guard bands and gap columns still hold the canary, bit for bit"""
        g = self.guard
        gaps = self.raw[g:g + self.rows * self.ld].reshape(self.rows, self.ld)[:, self.cols:]
        return bool((self.raw[:g] == CANARY).all() and (self.raw[g + self.rows * self.ld:] == CANARY).all() and (gaps == CANARY).all())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ------------------------------------------------------------------------------------------------ GroupNorm backward
class GnCase:
    def __init__(self, case):
        self.case = case
        self.B, self.C1, self.C2, self.HW, self.G, self.silu = case
        self.C, self.R = self.C1 + self.C2, self.B * self.HW
        self.eps = H.eps_of(self.silu)
        x, dy, gamma, beta, old = H.gn_inputs(case)
        self.x1 = x[..., :self.C1].contiguous().to(DEV)
        self.x2 = x[..., self.C1:].contiguous().to(DEV) if self.C2 else None
        self.dy, self.gamma, self.beta, self.old = dy.to(DEV), gamma.to(DEV), beta.to(DEV), old.to(DEV)
        self.r, self.slack = H.gn_reference(case)                       # float64, CPU, shared and never modified
        self.r2 = self.r.reshape(self.R, self.C)
        self.slack2 = self.slack.reshape(self.R, self.C)
        self.old2 = old.reshape(self.R, self.C)

    def args(self, b=None):
        """the leading arguments, of the whole batch or of sample b alone"""
        if b is None:
            return (ptr(self.x1), ptr(self.x2), self.C1, self.C2, self.B, self.HW, self.G, self.eps, ptr(self.gamma), ptr(self.beta), self.silu,
                    ptr(self.dy))
        self.keep = (self.x1[b:b + 1].contiguous(), self.x2[b:b + 1].contiguous() if self.C2 else None, self.dy[b:b + 1].contiguous())
        return (ptr(self.keep[0]), ptr(self.keep[1]), self.C1, self.C2, 1, self.HW, self.G, self.eps, ptr(self.gamma), ptr(self.beta), self.silu,
                ptr(self.keep[2]))

    def dests(self, pad1=0, pad2=0, old1=False, old2=False, rows=None):
        rows = rows or self.R
        d1 = Guarded(rows, self.C1 + pad1, self.C1, self.old[..., :self.C1] if old1 else None)
        d2 = Guarded(rows, self.C2 + pad2, self.C2, self.old[..., self.C1:] if old2 else None) if self.C2 else None
        return d1, d2

    def split(self, ctx, d1, d2, acc1=0, acc2=0, scratch=None, b=None):
        ctx.call("pnpi_op_groupnorm_bwd_split", *self.args(b), d1.p if d1 else None, d1.ld if d1 else 0, acc1,
                 d2.p if d2 else None, d2.ld if d2 else 0, acc2, ptr(scratch), scratch.numel() if scratch is not None else 0)
        torch.cuda.synchronize()

    def ratio(self, got, cols, acc):
        """worst |err| / bound of columns `cols` (a slice of the C channels), got [R, len(cols)] from the device"""
        r, sl = self.r2[:, cols], self.slack2[:, cols]
        if acc:
            old = self.old2[:, cols]
            return H.worst_ratio(got.cpu(), old.double() + r, H.acc_bound(r, sl, old, H.KAPPA_GN))
        return H.worst_ratio(got.cpu(), r, H.norm_bwd_bound(r, sl, H.KAPPA_GN))


@pytest.mark.parametrize("case", H.GN_CASES, ids=lambda c: "B%d_C%d+%d_HW%d_G%d_silu%d" % c)
def test_groupnorm_bwd_three_phase_destinations(ctx, case):
    k = GnCase(case)
    c1, c2 = slice(0, k.C1), slice(k.C1, k.C)
    worst = {}

    # dense, as pnpi_op_groupnorm_bwd launches it: one [R][C] buffer
    dense = Guarded(k.R, k.C, k.C)
    ctx.call("pnpi_op_groupnorm_bwd", *k.args(), dense.p)
    torch.cuda.synchronize()
    assert dense.intact()
    worst["dense"] = k.ratio(dense.data(), slice(0, k.C), False)
    assert rel_err(dense.data().cpu(), k.r2) < 4e-3                     # the whole-tensor check of test_gpu_backward.py still holds

    # two separate destinations (ld1 = C1, ld2 = C2), the context's scratch: the run everything else is compared with
    d1, d2 = k.dests()
    k.split(ctx, d1, d2)
    assert d1.intact() and (d2 is None or d2.intact())
    base1, base2 = d1.data(), d2.data() if d2 else None
    worst["split"] = max(k.ratio(base1, c1, False), k.ratio(base2, c2, False) if d2 else 0.0)
    assert same_bits(dense.data()[:, c1], base1) and (d2 is None or same_bits(dense.data()[:, c2], base2))

    # a second launch: bit-identical (every reduction runs in a fixed order)
    e1, e2 = k.dests()
    k.split(ctx, e1, e2)
    assert same_bits(e1.data(), base1) and (e2 is None or same_bits(e2.data(), base2))

    # either destination accumulating into old ~ N(0, 1), the other overwriting
    for acc1, acc2 in ((1, 0), (0, 1)) if k.C2 else ((1, 0),):
        a1, a2 = k.dests(old1=bool(acc1), old2=bool(acc2))
        k.split(ctx, a1, a2, acc1, acc2)
        assert a1.intact() and (a2 is None or a2.intact())
        worst["acc%d%d" % (acc1, acc2)] = max(k.ratio(a1.data(), c1, acc1), k.ratio(a2.data(), c2, acc2) if a2 else 0.0)
        if not acc1:
            assert same_bits(a1.data(), base1)
        if a2 and not acc2:
            assert same_bits(a2.data(), base2)

    # a source that needs no gradient: its sibling is what it was, the absent one is not touched (nothing to touch)
    if k.C2:
        _, n2 = k.dests()
        k.split(ctx, None, n2)
        assert n2.intact() and same_bits(n2.data(), base2)
        n1, _ = k.dests()
        k.split(ctx, n1, None)
        assert n1.intact() and same_bits(n1.data(), base1)

    # padded row strides, the gap columns preset to the canary
    p1, p2 = k.dests(pad1=16, pad2=8)
    k.split(ctx, p1, p2)
    assert p1.intact() and (p2 is None or p2.intact())
    assert same_bits(p1.data(), base1) and (p2 is None or same_bits(p2.data(), base2))

    # the caller's scratch, all NaN before the launch: every partial that is read was written by this launch, empty chunks included
    nfl = ctx.lib.pnpi_op_groupnorm_bwd_scratch_floats(k.B, k.HW, k.G)
    assert nfl == k.B * 256 * k.G * 4
    scratch = torch.full((nfl,), float("nan"), device=DEV)
    s1, s2 = k.dests()
    k.split(ctx, s1, s2, scratch=scratch)
    assert same_bits(s1.data(), base1) and (s2 is None or same_bits(s2.data(), base2))
    st = ctx.lib.pnpi_op_groupnorm_bwd_split(ctx.h, *k.args(), s1.p, s1.ld, 0, s2.p if s2 else None, s2.ld if s2 else 0, 0, ptr(scratch), nfl - 1)
    assert st == _capi.PNPI_ESHAPE

    # one sample at a time: the chunking does not depend on B
    if k.B > 1:
        for b in range(k.B):
            o1, o2 = k.dests(rows=k.HW)
            k.split(ctx, o1, o2, b=b)
            rows = slice(b * k.HW, (b + 1) * k.HW)
            assert same_bits(o1.data(), base1[rows]) and (o2 is None or same_bits(o2.data(), base2[rows])), b

    print("\ngn_bwd %s: worst |err| / bound %s" % (case, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) < 1.0, worst


@pytest.mark.parametrize("case", H.FALLBACK_CASES, ids=lambda c: "B%d_C%d+%d_HW%d_G%d_silu%d" % c)
def test_groupnorm_bwd_one_block_per_group(ctx, case):
    """launch_groupnorm_bwd, what the walk launches when C1 is no multiple of 8 (or x2 == x1)"""
    k = GnCase(case)
    dense = Guarded(k.R, k.C, k.C)
    ctx.call("pnpi_op_groupnorm_bwd_ref", *k.args(), dense.p)
    torch.cuda.synchronize()
    assert dense.intact()
    got = dense.data()
    w = k.ratio(got, slice(0, k.C), False)
    print("\ngn_bwd one block per group %s: worst |err| / bound %.3f" % (case, w))
    assert w < 1.0
    assert rel_err(got.cpu(), k.r2) < 4e-3
    if not k.C1 & 7:                                                    # both kernels take this shape: they differ by at most both bounds
        three = Guarded(k.R, k.C, k.C)
        ctx.call("pnpi_op_groupnorm_bwd", *k.args(), three.p)
        torch.cuda.synchronize()
        bound = H.norm_bwd_bound(k.r2, k.slack2, H.KAPPA_GN)
        assert ((got.cpu().double() - three.data().cpu().double()).abs() <= 2 * bound).all()


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("case", H.LN_CASES, ids=lambda c: "M%d_C%d" % c)
def test_layernorm_bwd_per_element(ctx, case):
    M, C = case
    x, dy, gamma = H.ln_inputs(case)
    xd, dyd, gd = x.to(DEV), dy.to(DEV), gamma.to(DEV)
    dx = Guarded(M, C, C)
    ctx.call("pnpi_op_layernorm_bwd", ptr(xd), ptr(dyd), M, C, 1e-5, ptr(gd), dx.p)
    torch.cuda.synchronize()
    assert dx.intact()                                                  # rows M .. 4 of the last block write nothing
    r, slack = H.ln_reference(case)
    w = H.worst_ratio(dx.data().cpu(), r, H.norm_bwd_bound(r, slack, H.KAPPA_LN))
    print("\nln_bwd %s: worst |err| / bound %.3f" % (case, w))
    assert w < 1.0
    assert rel_err(dx.data().cpu(), r) < 3e-3


def test_layernorm_bwd_refuses_more_than_2048_channels(ctx):
    M, C = 1, 2056
    x, dy, gamma = h16(M, C, seed=1), h16(M, C, seed=2), torch.ones(C, device=DEV)
    dx = Guarded(M, C, C)
    assert ctx.lib.pnpi_op_layernorm_bwd(ctx.h, ptr(x), ptr(dy), M, C, 1e-5, ptr(gamma), dx.p) == _capi.PNPI_ESHAPE
    torch.cuda.synchronize()
    assert dx.intact() and (dx.body.view(torch.int16) == CANARY).all()


# ------------------------------------------------------------------------------------------------ plumbing, bit for bit
def add16(a, b):
    """fp16(fp32(a) + fp32(b)): the one rounding of every accumulating kernel"""
    return (a.float() + b.float()).half()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("R,ld,off,C", [(5, 96, 64, 32), (5, 40, 0, 40), (5, 2560, 1280, 1280), (4097, 1040, 8, 1032)])
def test_strided_add(ctx, R, ld, off, C, accumulate):
    assert (R * C // 8 > GRID_VECS) == (R == 4097)                      # the last shape alone makes the grid-stride loop's second trip
    src = h16(R, ld, seed=20)
    old = h16(R, C, seed=21)
    dst = Guarded(R, C, C, old)
    ctx.call("pnpi_op_strided_add", dst.p, ptr(src), ld, off, R, C, accumulate)
    torch.cuda.synchronize()
    want = add16(old, src[:, off:off + C]) if accumulate else src[:, off:off + C]
    assert dst.intact() and same_bits(dst.data(), want)


def test_strided_add_refuses_a_misaligned_offset(ctx):
    src, dst = h16(5, 96, seed=20), Guarded(5, 32, 32)
    assert ctx.lib.pnpi_op_strided_add(ctx.h, dst.p, ptr(src), 96, 4, 5, 32, 0) == _capi.PNPI_ESHAPE
    torch.cuda.synchronize()
    assert dst.intact() and (dst.body.view(torch.int16) == CANARY).all()


def test_accumulate_grid_stride(ctx):
    n = 8 * (GRID_VECS + 3)
    a, b = h16(n, seed=22), h16(n, seed=23)
    dst = Guarded(1, n, n, a)
    ctx.call("pnpi_op_accumulate", dst.p, ptr(b), n)
    torch.cuda.synchronize()
    assert dst.intact() and same_bits(dst.data().reshape(-1), add16(a, b))


def test_sumpool2x2_grid_stride_odd_width(ctx):
    B, Hh, W, C = 2, 65, 65, 512
    assert B * Hh * W * (C // 8) > GRID_VECS
    dup = h16(B, 2 * Hh, 2 * W, C, seed=24)
    dx = Guarded(B * Hh * W, C, C)
    ctx.call("pnpi_op_sumpool2x2", ptr(dup), B, Hh, W, C, dx.p)
    torch.cuda.synchronize()
    f = dup.float()
    want = (((f[:, 0::2, 0::2] + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) + f[:, 1::2, 1::2]).half()      # the kernel's order, fp32
    assert dx.intact() and same_bits(dx.data(), want.reshape(-1, C))


def test_zero_stuff2_grid_stride_odd_width(ctx):
    B, Ho, Wo, C = 1, 33, 31, 1032
    assert B * 2 * Ho * 2 * Wo * (C // 8) > GRID_VECS
    dy = h16(B, Ho, Wo, C, seed=25)
    z = Guarded(B * 2 * Ho * 2 * Wo, C, C)
    ctx.call("pnpi_op_zero_stuff2", ptr(dy), B, Ho, Wo, C, z.p)
    torch.cuda.synchronize()
    want = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=torch.half, device=DEV)
    want[:, ::2, ::2] = dy
    assert z.intact() and same_bits(z.data(), want.reshape(-1, C))


@pytest.mark.parametrize("R,heads,dh,Dp", [(7, 3, 5, 32), (64, 8, 8, 32)])
def test_pad_heads(ctx, R, heads, dh, Dp):
    src = h16(R, heads * dh, seed=26)
    dst = Guarded(R, heads * Dp, heads * Dp)
    ctx.call("pnpi_op_pad_heads", ptr(src), R, heads, dh, Dp, dst.p)
    torch.cuda.synchronize()
    got = dst.data().reshape(R, heads, Dp)
    assert dst.intact() and same_bits(got[..., :dh], src.reshape(R, heads, dh))
    assert (got[..., dh:].contiguous().view(torch.int16) == 0).all()     # +0.0 exactly


@pytest.mark.parametrize("n", [77 * 768, GRID_VECS + 5])
def test_add_f16_to_f32(ctx, n):
    g = torch.Generator(device="cpu").manual_seed(27)
    old = torch.randn(n, generator=g).to(DEV)
    src = h16(n, seed=28)
    buf = torch.full((1024 + n + 1024,), float("nan"), device=DEV)          # 4 KiB of NaN on either side
    dst = buf[1024:1024 + n]
    dst.copy_(old)
    ctx.call("pnpi_op_add_f16_to_f32", ptr(dst), ptr(src), n, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(dst, old + src.float())                          # scale 1: one fp32 addition, with or without contraction
    assert torch.isnan(buf[:1024]).all() and torch.isnan(buf[1024 + n:]).all()
    dst.copy_(old)
    ctx.call("pnpi_op_add_f16_to_f32", ptr(dst), ptr(src), n, 0.375)
    torch.cuda.synchronize()
    want = old.double() + 0.375 * src.double()
    w32 = want.float().abs()
    ulp = (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double()
    assert ((dst.double() - want).abs() <= ulp).all()                   # fma or multiply-then-add: within one fp32 ulp of the exact sum


@pytest.mark.parametrize("R,Cc,ld_src,ld_dst", [(77, 40, 64, 80), (33, 33, 40, 40), (256, 8, 32, 256)])
def test_transpose_batched(ctx, R, Cc, ld_src, ld_dst):
    nb = 3
    s_src = R * ld_src + 24                                             # the matrices of a batch are not back to back
    rows_dst = Cc + 2                                                   # two rows and 8 halfs between the transposed matrices
    s_dst = rows_dst * ld_dst + 8
    src = h16(nb * s_src, seed=29)
    dst = Guarded(1, nb * s_dst, nb * s_dst)
    dst.cols = 0                                                        # everything is canary until written: checked by hand below
    ctx.call("pnpi_op_transpose", ptr(src), ld_src, R, Cc, dst.p, ld_dst, nb, s_src, s_dst)
    torch.cuda.synchronize()
    g = dst.guard
    assert (dst.raw[:g] == CANARY).all() and (dst.raw[g + nb * s_dst:] == CANARY).all()
    for b in range(nb):
        m = src[b * s_src:b * s_src + R * ld_src].reshape(R, ld_src)[:, :Cc]
        out = dst.body.reshape(-1)[b * s_dst:(b + 1) * s_dst]
        got = out[:rows_dst * ld_dst].reshape(rows_dst, ld_dst)
        assert same_bits(got[:Cc, :R], m.t()), b
        assert (got[:Cc, R:].contiguous().view(torch.int16) == 0).all(), b              # the k-extent padding is +0.0
        assert (got[Cc:].contiguous().view(torch.int16) == CANARY).all(), b            # rows >= Cc
        assert (out[rows_dst * ld_dst:].view(torch.int16) == CANARY).all(), b           # the gap to the next matrix


def test_transpose_refuses_a_short_destination_row(ctx):
    src, dst = h16(77, 64, seed=29), Guarded(40, 72, 72)
    assert ctx.lib.pnpi_op_transpose(ctx.h, ptr(src), 64, 77, 40, dst.p, 72, 1, 0, 0) == _capi.PNPI_ESHAPE
    torch.cuda.synchronize()
    assert (dst.raw == CANARY).all()


def test_repack_dgrad_pad_and_the_conv_out_dgrad(ctx):
    """conv_out's record has no fp16 output: its gradient arrives with 8 channels, 4 .. 7 zero, and the dgrad weights are repacked with
    Npad = 8 (tape_backward, o.out == nullptr)"""
    N, Npad, ks, Cin, B, Hh = 4, 8, 3, 32, 2, 16
    taps = ks * ks
    w = h16(N, Cin, ks, ks, scale=1.0 / (taps * Cin) ** 0.5, seed=30)
    wp = pack_w(w)                                                      # [N][taps][Cin]
    wd = Guarded(Cin * taps, Npad, Npad)
    ctx.call("pnpi_op_repack_dgrad_pad", ptr(wp), N, Npad, taps, Cin, wd.p)
    torch.cuda.synchronize()
    got = wd.data().reshape(Cin, taps, Npad)
    assert wd.intact() and same_bits(got[..., :N], wp.reshape(N, taps, Cin).flip(1).permute(2, 1, 0))
    assert (got[..., N:].contiguous().view(torch.int16) == 0).all()
    assert ctx.lib.pnpi_op_repack_dgrad_pad(ctx.h, ptr(wp), N, N - 1, taps, Cin, wd.p) == _capi.PNPI_ESHAPE

    dy = h16(B, N, Hh, Hh, seed=31)
    dy8 = torch.zeros(B, Hh, Hh, Npad, dtype=torch.half, device=DEV)
    dy8[..., :N] = nhwc(dy)
    dx = Guarded(B * Hh * Hh, Cin, Cin)
    wdw = wd.data().contiguous()                                        # [Cin][taps * 8]: the forward kernel's weight rows
    ctx.call("pnpi_op_conv", ptr(dy8), None, Npad, 0, B, Hh, Hh, ks, 1, 1, 0, Hh, Hh, ptr(wdw), None, None, Cin, dx.p, -1, 0)
    torch.cuda.synchronize()
    x = torch.zeros(B, Cin, Hh, Hh, dtype=torch.double, requires_grad=True)                 # float64 on the host
    wc, dyc = w.double().cpu(), dy.double().cpu()
    F.conv2d(x, wc, None, stride=1, padding=1).backward(dyc)
    want = nhwc(x.grad).reshape(-1, Cin)
    mag = nhwc(F.conv_transpose2d(dyc.abs(), wc.abs(), padding=1)).reshape(-1, Cin)
    # 36 non-zero products of fp16 pairs (exact in fp32) summed in fp32 in some order, one rounding to fp16: the textbook bound
    # (n - 1) u sum |a b| with n = 72 terms of the padded K, u = 2^-24, doubled for the order; plus the fp16 half-ulp
    bound = want.abs() * 2.0 ** -11 + 2.0 ** -24 + 2 * 72 * 2.0 ** -24 * mag
    assert dx.intact()
    assert ((dx.data().cpu().double() - want).abs() <= bound).all()
    assert rel_err(dx.data().cpu(), want) < 3e-3
