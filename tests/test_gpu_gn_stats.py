"""The statistics-fed GroupNorm (launch_groupnorm_fused, csrc/norm.hip) through pnpi_op_groupnorm_stats: the norm most of the UNet
forward runs, which takes the per-(m-tile, channel) sum / sum-of-squares partials of the producing convolution's epilogue instead of
a statistics pass.  Two kernel sets exist only for it -- gn_finalize_tiles_kernel + gn_apply_kernel, and gn_fin_apply_kernel under
tuning "gn_inline_rows" -- and every case here runs under both (the `inline` fixture).

Every case checks, against float64 F.group_norm (+ SiLU) of the same fp16 input:
  * per element |y - ref| <= 2^-10 |ref| + 1e-3 -- the bound tests/test_gn_stats_host.py derives from a CPU emulation of the fp32
    partial tree (worst emulated ratio 0.40 at mean/std <= 16, which is what the inputs here keep to);
  * the suite's global rel-L2 < 2e-3 as well;
  * `out` is one batch item longer than needed and pre-filled with 777.0: the tail keeps it, the body holds none;
  * a second launch gives the same bits (fixed reduction order, no atomics).
Inputs carry a per-item offset of (b - 1) * 4 and per-channel offsets in [-2, 2], so that another item's or another group's
statistics break the per-element bound by a wide margin (test_swapped_items_are_noticed shows it does).

The statistics kernels run only where the one-launch gn_small_kernel does not take the tensor: channels per group cpg % 4 != 0
(C = 320 or 960 with 32 groups), or a (item, group) slice of HW * cpg > 24576 elements.  Each case names its condition (`why`) and
asserts it, so a shape shrunk into gn_small_kernel -- which ignores the partials -- fails here instead of passing vacuously.  A
power-of-two width of 256 or 512 channels on a 16 x 16 map has cpg % 4 == 0 and slices far below 24576 at 32 groups: those chains
(tiles 16, 20, 5) run with 4 groups of 128 channels (32768 elements per slice)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402
from tests.test_gn_stats_host import gn_bound_ratio, tile_partials  # noqa: E402

DEV = "cuda"
EPS = 1e-5
SENTINEL = 777.0
WS_BYTES = 96 << 20          # the split-K workspace of a context of up to 12 rows (what the plan query is told)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


@pytest.fixture(params=[0, 1 << 20], ids=["finalize_tiles+apply", "fin_apply"])
def inline(request, ctx):
    """tuning "gn_inline_rows": 0 = two launches (the default), 1 << 20 = the one-launch kernel for every case here"""
    with ctx.tuning(gn_inline_rows=request.param):
        yield request.param


def h16(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().to(DEV)


def make_x(B, HW, Cn, seed, scale=1.0, shift=0.0):
    """N(shift, scale^2) + (b - 1) * 4 per batch item + a per-channel offset in [-2, 2]: |mean| / std <= 16 overall"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, HW, Cn, generator=g) * scale + shift
    x = x + (torch.arange(B, dtype=torch.float32)[:, None, None] - 1.0) * 4.0 + (torch.rand(Cn, generator=g) * 4.0 - 2.0)[None, None]
    return x.half().to(DEV)


def affine(Cn, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(Cn, generator=g) * 0.2 + 1).to(DEV), (torch.randn(Cn, generator=g) * 0.2).to(DEV)


def assert_statistics_path(why, Cn, C1, HW, groups, B):
    """the condition that keeps this case out of gn_small_kernel (gn_small_ok, csrc/norm.hip), as the case states it"""
    cpg = Cn // groups
    assert Cn % groups == 0 and B * groups < 1536
    if why == "cpg%4":
        assert cpg % 4 != 0, cpg
    else:
        assert why == "slice>24576" and HW * cpg > 24576, HW * cpg


def reference(x, groups, gamma, beta, silu):
    ref = F.group_norm(x.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), EPS).permute(0, 2, 1)
    return F.silu(ref) if silu else ref


def reference_with_statistics_of(x, z, groups, gamma, beta, silu):
    """x * sc(z) + sh(z): scale and shift from z's float64 sums"""
    B, HW, Cn = x.shape
    cpg = Cn // groups
    zd = z.double().reshape(B, HW, groups, cpg)
    mean = zd.mean((1, 3))
    rstd = 1.0 / torch.sqrt((zd * zd).mean((1, 3)) - mean * mean + EPS)
    sc = rstd.repeat_interleave(cpg, 1) * gamma.double()[None]
    sh = beta.double()[None] - mean.repeat_interleave(cpg, 1) * sc
    y = x.double() * sc[:, None] + sh[:, None]
    return F.silu(y) if silu else y


def launch(ctx, x1, x2, groups, gamma, beta, silu, st1, rows1, st2=None, rows2=0):
    """-> (status, out [B + 1, HW, C] pre-filled with the sentinel)"""
    B, HW, C1 = x1.shape
    C2 = x2.shape[2] if x2 is not None else 0
    out = torch.full((B + 1, HW, C1 + C2), SENTINEL, dtype=torch.half, device=DEV)
    status = ctx.lib.pnpi_op_groupnorm_stats(ctx.h, ptr(x1), ptr(x2), C1, C2, B, HW, groups, EPS, ptr(gamma), ptr(beta), silu, ptr(out),
                                             ptr(st1), rows1, ptr(st2), rows2)
    torch.cuda.synchronize()
    return status, out


def measure(ctx, ref, *args):
    """launch, the sentinel / finiteness / bit-reproducibility checks; -> (worst per-element ratio, rel-L2)"""
    status, out = launch(ctx, *args)
    assert status == 0, (status, ctx.lib.pnpi_last_error(ctx.h))
    B = ref.shape[0]
    assert torch.equal(out[B], torch.full_like(out[B], SENTINEL)), "wrote past the last batch item"
    assert not (out[:B] == SENTINEL).any(), "left part of the output unwritten"
    assert torch.isfinite(out[:B]).all()
    status2, out2 = launch(ctx, *args)
    assert status2 == 0 and torch.equal(out, out2), "a second launch gave other bits"
    return gn_bound_ratio(out[:B], ref), rel_err(out[:B], ref)


def check(ctx, tag, ref, *args):
    ratio, e = measure(ctx, ref, *args)
    print("gn_stats %s: worst per-element ratio %.3f, rel-L2 %.2e" % (tag, ratio, e))
    assert ratio <= 1.0, ratio
    assert e < 2e-3, e


# ------------------------------------------------------------------------------------------------ a. the consumer alone
@pytest.mark.parametrize("B,HW,Cn,rows,silu,why", [
    (2, 256, 320, 64, 1, "cpg%4"),              # tpb = 4: half of the eight lanes idle
    (1, 192, 320, 64, 1, "cpg%4"),              # tpb = 3
    (3, 64, 320, 64, 1, "cpg%4"),               # tpb = 1
    (1, 16384, 320, 64, 1, "cpg%4"),            # tpb = 256, the most op_gn hands over
    (2, 4096, 640, 128, 1, "slice>24576"),      # cpg = 20: 81920 elements per slice
    (2, 1024, 320, 256, 0, "cpg%4"),            # 256-row partials, no SiLU
])
def test_gn_stats_single_source(ctx, inline, B, HW, Cn, rows, silu, why):
    assert_statistics_path(why, Cn, Cn, HW, 32, B)
    x = make_x(B, HW, Cn, seed=HW + Cn)
    gamma, beta = affine(Cn, 3)
    check(ctx, "a single (%d, %d, %d, %d)" % (B, HW, Cn, rows), reference(x, 32, gamma, beta, silu), x, None, 32, gamma, beta, silu,
          tile_partials(x, rows), rows)


@pytest.mark.parametrize("B,C1,C2,rows1,rows2,why", [
    (2, 320, 640, 64, 64, "cpg%4"),             # cpg = 30: group 10 spans channels 300 .. 329, 20 of x1 and 10 of x2
    (2, 320, 640, 64, 128, "cpg%4"),            # the two sources' tiles differ in height, as in the up blocks
    (2, 320, 640, 256, 64, "cpg%4"),
    (2, 320, 640, 128, 256, "cpg%4"),
    (1, 1280, 640, 64, 128, "slice>24576"),     # cpg = 60: group 21 spans channels 1260 .. 1319
])
def test_gn_stats_two_sources(ctx, inline, B, C1, C2, rows1, rows2, why):
    HW, Cn = 1024, C1 + C2
    assert_statistics_path(why, Cn, C1, HW, 32, B)
    assert C1 % (Cn // 32) != 0                 # a group straddles the two sources
    x = make_x(B, HW, Cn, seed=Cn + rows1)
    x1, x2 = x[:, :, :C1].contiguous(), x[:, :, C1:].contiguous()
    gamma, beta = affine(Cn, 4)
    check(ctx, "a concat (%d + %d, rows %d / %d)" % (C1, C2, rows1, rows2), reference(x, 32, gamma, beta, 1), x1, x2, 32, gamma, beta, 1,
          tile_partials(x1, rows1), rows1, tile_partials(x2, rows2), rows2)


def test_gn_stats_swapped_items_are_noticed(ctx, inline):
    """the harness itself: partials of batch items 0 and 2 exchanged (what `t` for `b * tpb + t` does to item 2, say) must break the
    per-element bound by a wide margin -- the inputs' per-item offsets are there for this"""
    B, HW, Cn, rows = 3, 256, 320, 64
    assert_statistics_path("cpg%4", Cn, Cn, HW, 32, B)
    x = make_x(B, HW, Cn, seed=77)
    gamma, beta = affine(Cn, 5)
    st = tile_partials(x, rows)
    tpb = HW // rows
    swapped = torch.cat([st[2 * tpb:], st[tpb:2 * tpb], st[:tpb]]).contiguous()
    ratio, e = measure(ctx, reference(x, 32, gamma, beta, 1), x, None, 32, gamma, beta, 1, swapped, rows)
    print("gn_stats a swapped items: worst per-element ratio %.1f, rel-L2 %.2e" % (ratio, e))
    assert ratio > 10


@pytest.mark.parametrize("C1,C2", [(320, 0), (320, 640)])
def test_gn_stats_partials_are_what_is_used(ctx, inline, C1, C2):
    """partials of another tensor z: the output is x under z's statistics, so the launch neither recomputed them from x nor went to
    gn_small_kernel"""
    B, HW, Cn, rows = 2, 256, C1 + C2, 64
    assert_statistics_path("cpg%4", Cn, C1, HW, 32, B)
    x = make_x(B, HW, Cn, seed=21)
    z = make_x(B, HW, Cn, seed=22, scale=1.5, shift=1.0)
    gamma, beta = affine(Cn, 6)
    ref = reference_with_statistics_of(x, z, 32, gamma, beta, 1)
    assert gn_bound_ratio(reference(x, 32, gamma, beta, 1), ref) > 10          # the two are far apart
    if C2:
        x1, x2, z1, z2 = (t.contiguous() for t in (x[:, :, :C1], x[:, :, C1:], z[:, :, :C1], z[:, :, C1:]))
        args = (x1, x2, 32, gamma, beta, 1, tile_partials(z1, rows), rows, tile_partials(z2, rows), rows)
    else:
        args = (x, None, 32, gamma, beta, 1, tile_partials(z, rows), rows)
    check(ctx, "a foreign partials (%d + %d)" % (C1, C2), ref, *args)


@pytest.mark.parametrize("HW,rows", [(1200, 128), (264, 1), (256, 0)], ids=["HW%rows", "over_256_tiles", "no_rows"])
def test_gn_stats_refuses_what_the_forward_would_recompute(ctx, inline, HW, rows):
    """op_gn's rule (gn_stats_usable, csrc/api_graph.inc): HW % rows != 0, HW / rows > 256 and rows == 0 are PNPI_ESHAPE here, `out`
    untouched.  (The buffers are as large as an accepted launch would need.)"""
    B, Cn = 2, 320
    x = make_x(B, HW, Cn, seed=31)
    gamma, beta = affine(Cn, 7)
    st = torch.zeros(B * (HW // max(rows, 1) + 1), Cn, 2, device=DEV)
    status, out = launch(ctx, x, None, 32, gamma, beta, 1, st, rows)
    assert status == _capi.PNPI_ESHAPE
    assert torch.equal(out, torch.full_like(out, SENTINEL))
    # the second source is held to the same rule (the first one's 8-row partials are acceptable at every HW here)
    x2 = make_x(B, HW, 640, seed=32)
    st1, st2 = torch.zeros(B * HW // 8, Cn, 2, device=DEV), torch.zeros(B * (HW + 1), 640, 2, device=DEV)
    status, out = launch(ctx, x, x2, 32, gamma.repeat(3), beta.repeat(3), 1, st1, 8, st2, rows)
    assert status == _capi.PNPI_ESHAPE
    assert torch.equal(out, torch.full_like(out, SENTINEL))


# ------------------------------------------------------------------------------------------------ b. producer -> consumer
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def pack_w(w):  # [N, C, kh, kw] -> [N, kh*kw*C] tap-major
    return w.permute(0, 2, 3, 1).contiguous().reshape(w.shape[0], -1)


def plan_of(lib, M, N, Cin, ks, residual, cfg, split):
    K = ks * ks * Cin
    d = _capi.IgemmLaunchDesc(M=M, N=N, K=K, ksize=ks, C1=Cin, C2=0, ldx1=Cin, ldx2=0, ldw=K, ldo=N, ldres=N, bias=1, bias_aligned16=1,
                              residual=int(residual), geglu=0, stats=1, vt_col0=1 << 30, vt_ld=0, vt_f32=0, rows_per_batch=1, vt_perm16=0,
                              nbatch=1, ws_bytes=WS_BYTES, force_cfg=cfg, force_split=split, sel_M=0)
    pl = _capi.IgemmPlan()
    assert lib.pnpi_igemm_plan_query(d, pl) == 0
    return pl


def conv_with_statistics(ctx, B, Cin, H, N, ks, cfg, split, residual, seed):
    """pnpi_op_conv_stats of a stride-1 convolution, held against F.conv2d at the kernel suite's 2e-3 and against the table-driven plan
    -> (out [B, HW, N] fp16 as stored, partials, rows per partial (0: none), plan)"""
    x = h16(B, Cin, H, H, seed=seed)
    w = h16(N, Cin, ks, ks, scale=1.0 / math.sqrt(ks * ks * Cin), seed=seed + 1)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    res = h16(B, N, H, H, seed=seed + 3) if residual else None
    assert bias.data_ptr() % 16 == 0
    M = B * H * H
    out = torch.zeros(B, H, H, N, dtype=torch.half, device=DEV)
    stats = torch.full(((M + 63) // 64, N, 2), float("nan"), device=DEV)
    rows = C.c_int(-1)
    xn, wp, resn = nhwc(x), pack_w(w), (nhwc(res) if residual else None)
    ctx.call("pnpi_op_conv_stats", ptr(xn), None, Cin, 0, B, H, H, ks, 1, 1 if ks == 3 else 0, 0, H, H, ptr(wp), ptr(bias), ptr(resn), N, ptr(out),
             cfg, split, ptr(stats), C.byref(rows))
    torch.cuda.synchronize()
    ref = F.conv2d(x.float(), w.float(), bias, padding=1 if ks == 3 else 0)
    if residual:
        ref = ref + res.float()
    assert rel_err(out.permute(0, 3, 1, 2), ref) < 2e-3
    pl = plan_of(ctx.lib, M, N, Cin, ks, residual, cfg, split)
    assert pl.err == 0 and pl.stats_tile_rows == rows.value, (pl.err, pl.stats_tile_rows, rows.value)
    assert (pl.stats != 0) == (rows.value > 0)
    if rows.value > 0:
        assert torch.isfinite(stats[:(M + rows.value - 1) // rows.value]).all()
    return out.reshape(B, H * H, N), stats, rows.value, pl


# tile ids: 17 / 19 = 192 / 128 x 320 ping-pong, 16 / 20 = 256 / 192 x 256 ping-pong, 4 = 128 x 320, 5 = 128 x 256, 6 = 256 x 320, 12 = 64 x 320.
# (B, Cin, H, N, ksize, tile, split, groups, residual, rows per partial the tile hands over, the condition that keeps gn_small_kernel away)
CHAINS = [
    (2, 64, 16, 320, 3, 17, 0, 32, 0, 64, "cpg%4"),
    (2, 64, 16, 320, 3, 19, 0, 32, 0, 64, "cpg%4"),
    (2, 64, 16, 512, 3, 16, 0, 4, 0, 64, "slice>24576"),
    (2, 64, 16, 512, 3, 20, 0, 4, 0, 128, "slice>24576"),      # takes no statistics launch: the 128 x 128 kernel runs, 128-row partials
    (2, 64, 16, 320, 3, 4, 0, 32, 0, 128, "cpg%4"),
    (2, 64, 16, 512, 3, 5, 0, 4, 0, 128, "slice>24576"),
    (2, 64, 16, 320, 3, 6, 0, 32, 0, 256, "cpg%4"),            # one 256-row partial per item
    (2, 64, 16, 320, 3, 12, 0, 32, 0, 64, "cpg%4"),
    (3, 64, 16, 320, 3, 6, 0, 32, 0, 256, "cpg%4"),            # M = 768: the last 256-row m-tile is whole
    (2, 64, 32, 320, 3, 17, 0, 32, 0, 64, "cpg%4"),            # tpb = 16; 192-row tiles against 64-row partials
    (2, 64, 16, 320, 3, 17, 0, 32, 1, 64, "cpg%4"),            # conv2 + shortcut feeding the next block's norm1
    (2, 64, 16, 320, 1, 17, 0, 32, 0, 64, "cpg%4"),            # 1 x 1: proj_out feeding a ResNet norm
    (2, 64, 16, 320, 1, 17, 0, 32, 1, 64, "cpg%4"),            # ... with its residual
    (2, 1280, 8, 320, 3, 17, 0, 32, 0, 64, "cpg%4"),           # deep K (180 K-tiles), HW = 64: tpb = 1
    (2, 1280, 8, 320, 3, 17, 2, 32, 0, 0, "cpg%4"),            # split-K: the combine kernel writes the output, nobody the statistics
    (2, 1280, 8, 320, 3, 17, 3, 32, 0, 0, "cpg%4"),
]


@pytest.mark.parametrize("B,Cin,H,N,ks,cfg,split,groups,residual,want_rows,why", CHAINS)
def test_gn_stats_chain(ctx, inline, B, Cin, H, N, ks, cfg, split, groups, residual, want_rows, why):
    HW = H * H
    assert_statistics_path(why, N, N, HW, groups, B)
    y, stats, rows, pl = conv_with_statistics(ctx, B, Cin, H, N, ks, cfg, split, residual, seed=100 + cfg)
    assert rows == want_rows, (rows, want_rows)
    assert pl.id == (0 if cfg == 20 else cfg) and pl.split == max(split, 1), (pl.id, pl.split)
    if rows == 0:
        print("gn_stats b chain tile %d split %d: tile_rows_out == 0, as planned" % (cfg, split))
        return
    gamma, beta = affine(N, 8)
    check(ctx, "b chain (B %d, Cin %d, %dx%d, N %d, k %d, tile %d, res %d)" % (B, Cin, H, H, N, ks, cfg, residual), reference(y, groups, gamma, beta, 1),
          y, None, groups, gamma, beta, 1, stats, rows)


@pytest.mark.parametrize("cfg2,want_rows2", [(16, 64), (6, 256)])
def test_gn_stats_chain_two_producers(ctx, inline, cfg2, want_rows2):
    """the up-block norm1 end to end: hidden state (320 channels, tile 17) and skip (640 channels, another tile) concatenated, cpg = 30"""
    B, Cin, H = 2, 64, 16
    assert_statistics_path("cpg%4", 960, 320, H * H, 32, B)
    y1, st1, rows1, _ = conv_with_statistics(ctx, B, Cin, H, 320, 3, 17, 0, 0, seed=200)
    y2, st2, rows2, _ = conv_with_statistics(ctx, B, Cin, H, 640, 3, cfg2, 0, 0, seed=210)
    assert (rows1, rows2) == (64, want_rows2)
    gamma, beta = affine(960, 9)
    check(ctx, "b two producers (tiles 17 + %d)" % cfg2, reference(torch.cat([y1, y2], 2), 32, gamma, beta, 1), y1.contiguous(), y2.contiguous(), 32,
          gamma, beta, 1, st1, rows1, st2, rows2)
