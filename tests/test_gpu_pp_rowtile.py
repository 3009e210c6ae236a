"""The shorter ping-pong GEMM tiles (igemm_pp_kernel<128, 320> = cfg 19, <192, 256> = cfg 20, csrc/igemm_pp.inc) and the row-height
rule that launches them (tuning "pp_rowtile", csrc/gemm.hip).

An output element's K walk and split-K ranges do not depend on the tile's row height, and the GroupNorm partial sums keep one
reduction tree per tile width, so the bar between a new tile and its family's existing one (17 = 192 x 320, 16 = 256 x 256) at the same
split is BIT-IDENTITY of the outputs -- and of the statistics where both produce them (the 192 x 256 tile produces none).  One case per
tile is also held against F.conv2d in fp32 at the kernel suite's 2e-3 rel-L2.

Shapes: 64 / 128 / 192 input channels, 1 x 1 and 3 x 3 -> 1, 2, 3 and 9 K-tiles (prologue, both drains, the steady state); M = 128 k, M = 144
(a partial last tile of 128 rows, less than one of 192), M = 64 (less than any tile); two column tiles; stride 2, the asymmetric
(0, 1, 0, 1) pad, a two-source concat, the fused nearest upsample; bias + residual; split-K 2 and 3 on 3 and 9 K-tiles;
statistics whose 64-row sub-blocks straddle two 144-pixel images; V^T columns plain and in the permuted key order (pnpi_op_gemm, tuning
"op_gemm_vt_perm16"); the GEGLU epilogue (pnpi_op_gemm_geglu, the tile forced through tuning "igemm_force_cfg").  Every epilogue arm
of the new tiles is therefore held against its family's tile directly; the SD-1.x-width cases at the end check the rule inside the
forward (which launches moved, and that nothing changed), not the arms."""
import csv
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SD1  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402

DEV = "cuda"
FAMILY = {19: (17, 320), 20: (16, 256)}         # new tile id -> (its family's existing tile, BN)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def h16(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().to(DEV)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def pack_w(w):  # [N, C, kh, kw] -> [N, kh*kw*C] tap-major
    return w.permute(0, 2, 3, 1).contiguous().reshape(w.shape[0], -1)


def _conv_ref(x, w, bias, ks, stride, pad, ups):
    xr = x.float()
    if ups:
        xr = F.interpolate(xr, scale_factor=2.0, mode="nearest")
    if stride == 2 and pad == 0:
        return F.conv2d(F.pad(xr, (0, 1, 0, 1)), w.float(), bias, stride=2, padding=0)
    return F.conv2d(xr, w.float(), bias, stride=stride, padding=pad if ks == 3 else 0)


# (B, C1, C2, H, ksize, stride, pad, ups, ntiles, split, check)   N = ntiles x the family's BN; check: also against F.conv2d
CASES = [
    (2, 64, 0, 8, 1, 1, 0, 0, 1, 0, False),       # 1 x 1, Cin = 64: one K-tile (prologue only), M = 128 exactly
    (1, 64, 0, 12, 3, 1, 1, 0, 1, 0, True),       # 3 x 3, Cin = 64: 9 K-tiles, M = 144 (partial last tile / less than one tile)
    (4, 128, 0, 8, 1, 1, 0, 0, 1, 0, False),      # two K-tiles, M = 256 = 2 x 128
    (6, 128, 64, 8, 1, 1, 0, 0, 2, 0, False),     # concat, three K-tiles, M = 384 = 3 x 128 = 2 x 192, two column tiles
    (3, 128, 64, 12, 3, 1, 1, 0, 1, 0, False),    # concat 3 x 3 (27 K-tiles, the source switch inside a tap), M = 432: several tiles, ragged
    (1, 64, 0, 8, 3, 1, 1, 0, 1, 0, False),       # M = 64: less than any tile
    (2, 64, 0, 16, 3, 2, 1, 0, 1, 0, False),      # stride 2, M = 128
    (2, 64, 0, 16, 3, 2, 0, 0, 1, 0, False),      # stride 2 with the asymmetric pad (0, 1, 0, 1)
    (2, 64, 0, 8, 3, 1, 1, 1, 2, 0, False),       # fused nearest upsample, M = 512, two column tiles
    (1, 64, 0, 12, 3, 1, 1, 0, 1, 2, False),      # split-K 2 on 9 K-tiles (5 + 4)
    (1, 64, 0, 12, 3, 1, 1, 0, 1, 3, True),       # split-K 3 on 9 K-tiles
    (3, 128, 64, 12, 1, 1, 0, 0, 1, 2, False),    # split-K 2 on 3 K-tiles (2 + 1: a one-K-tile slice)
    (3, 128, 64, 12, 1, 1, 0, 0, 1, 3, False),    # split-K 3 on 3 K-tiles (three one-K-tile slices)
]


@pytest.mark.parametrize("new", [19, 20], ids=["pp128x320", "pp192x256"])
@pytest.mark.parametrize("B,C1,C2,H,ks,stride,pad,ups,ntiles,split,check", CASES)
def test_new_tile_equals_its_family_tile(ctx, new, B, C1, C2, H, ks, stride, pad, ups, ntiles, split, check):
    old, bn = FAMILY[new]
    N, Cin = ntiles * bn, C1 + C2
    x1 = h16(B, C1, H, H, seed=6)
    x2 = h16(B, C2, H, H, seed=7) if C2 else None
    w = h16(N, Cin, ks, ks, scale=1.0 / math.sqrt(ks * ks * Cin), seed=8)
    bias = torch.randn(N, device=DEV)
    xin = x1 if x2 is None else torch.cat([x1, x2], 1)
    ref = _conv_ref(xin, w, bias, ks, stride, pad, ups)
    Ho, Wo = ref.shape[2], ref.shape[3]
    res = h16(B, N, Ho, Wo, seed=9)
    x1n, x2n, wp, resn = nhwc(x1), (nhwc(x2) if C2 else None), pack_w(w), nhwc(res)
    outs = {}
    for cfg in (new, old):
        out = torch.zeros(B, Ho, Wo, N, dtype=torch.half, device=DEV)
        ctx.call("pnpi_op_conv", ptr(x1n), ptr(x2n), C1, C2, B, H, H, ks, stride, pad, ups, Ho, Wo, ptr(wp), ptr(bias), ptr(resn), N,
                 ptr(out), cfg, split)
        torch.cuda.synchronize()
        outs[cfg] = out
    assert torch.isfinite(outs[new]).all() and outs[new].abs().max() > 0
    assert torch.equal(outs[new], outs[old]), (outs[new].float() - outs[old].float()).abs().max().item()
    if check:
        e = rel_err(outs[new].permute(0, 3, 1, 2), ref + res.float())
        print("cfg %d: rel-L2 against F.conv2d %.3e" % (new, e))
        assert e < 2e-3, e


@pytest.mark.parametrize("ks,B,H", [(3, 3, 12), (1, 3, 12), (3, 2, 8)])
def test_statistics_equal_the_192_row_tile(ctx, ks, B, H):
    """128 x 320 against 192 x 320: the per-(64-row sub-block, channel) partial sums, bit for bit.  B = 3, H = 12: M = 432, 144 pixels per
    image -- sub-blocks 2 and 4 straddle two images, the last one is ragged (48 rows); the tile boundaries of the two heights fall in
    different sub-blocks.  B = 2, H = 8: whole tiles only."""
    Cin, N = 64, 640
    x = h16(B, Cin, H, H, seed=31)
    w = h16(N, Cin, ks, ks, scale=1.0 / math.sqrt(ks * ks * Cin), seed=32)
    bias = torch.randn(N, device=DEV)
    M = B * H * H
    xn, wp = nhwc(x), pack_w(w)
    got = {}
    for cfg in (19, 17):
        out = torch.zeros(B, H, H, N, dtype=torch.half, device=DEV)
        stats = torch.full(((M + 63) // 64, N, 2), float("nan"), device=DEV)
        rows = C.c_int(0)
        ctx.call("pnpi_op_conv_stats", ptr(xn), None, Cin, 0, B, H, H, ks, 1, 1 if ks == 3 else 0, 0, H, H, ptr(wp), ptr(bias), None, N, ptr(out), cfg, 0,
                 ptr(stats), C.byref(rows))
        torch.cuda.synchronize()
        assert rows.value == 64, (cfg, rows.value)       # the ping-pong kernel ran (the 4-wave fallback reports 128-row tiles)
        got[cfg] = (out, stats)
    assert torch.isfinite(got[19][1]).all()
    assert torch.equal(got[19][0], got[17][0])
    assert torch.equal(got[19][1], got[17][1]), (got[19][1] - got[17][1]).abs().max().item()
    o = got[19][0].reshape(M, N).float()
    for t in range((M + 63) // 64):
        blk = o[t * 64:(t + 1) * 64]
        assert torch.allclose(got[19][1][t, :, 0], blk.sum(0), rtol=1e-5, atol=1e-3), t
        assert torch.allclose(got[19][1][t, :, 1], (blk * blk).sum(0), rtol=1e-5, atol=1e-3), t


def test_192x256_leaves_statistics_launches_to_other_tiles(ctx):
    """16 row groups over three 64-row sub-blocks cannot reproduce the 256 x 256 tile's tree (8 groups per sub-block): a forced cfg 20 that
    is asked for statistics falls back to the 128 x 128 kernel (128-row partials), output unchanged at fp16 level"""
    B, Cin, H, N = 3, 64, 12, 256
    x = h16(B, Cin, H, H, seed=41)
    w = h16(N, Cin, 3, 3, scale=1.0 / math.sqrt(9 * Cin), seed=42)
    bias = torch.randn(N, device=DEV)
    M = B * H * H
    out = torch.zeros(B, H, H, N, dtype=torch.half, device=DEV)
    stats = torch.full(((M + 63) // 64, N, 2), float("nan"), device=DEV)
    rows = C.c_int(0)
    xn, wp = nhwc(x), pack_w(w)
    ctx.call("pnpi_op_conv_stats", ptr(xn), None, Cin, 0, B, H, H, 3, 1, 1, 0, H, H, ptr(wp), ptr(bias), None, N, ptr(out), 20, 0, ptr(stats), C.byref(rows))
    torch.cuda.synchronize()
    assert rows.value == 128
    assert rel_err(out.permute(0, 3, 1, 2), F.conv2d(x.float(), w.float(), bias, padding=1)) < 2e-3


def vt_perm16_pos(t):
    """csrc/ops.h: inside every aligned group of 16 tokens the two middle quads are swapped"""
    return t ^ (12 if ((t >> 2) ^ (t >> 3)) & 1 else 0)


@pytest.mark.parametrize("perm", [0, 1], ids=["plain", "perm16"])
@pytest.mark.parametrize("new", [19, 20], ids=["pp128x320", "pp192x256"])
def test_transposed_columns(ctx, new, perm):
    """QKV-style launch: the first column tile plain, the second written transposed per batch item (V^T), 72 tokens per item -- M = 216,
    ragged for both heights, 8-token runs inside one item.  perm16 (tuning "op_gemm_vt_perm16": the key order the 4096-token
    self-attention sites read): 80 tokens per item, whole 16-token groups -- M = 240, ragged for both heights, the tiles of the two
    heights start at different 16-token groups of an item"""
    old, bn = FAMILY[new]
    Bn, T, K, N, col0 = 3, (80 if perm else 72), 128, 2 * bn, bn
    M = Bn * T
    a = h16(M, K, seed=4)
    w = h16(N, K, scale=0.1, seed=5)
    bias = torch.randn(N, device=DEV)
    got = {}
    with ctx.tuning(op_gemm_vt_perm16=perm):
        for cfg in (new, old):
            out = torch.zeros(M, col0, dtype=torch.half, device=DEV)
            vt = torch.zeros(Bn, N - col0, T, dtype=torch.half, device=DEV)
            ctx.call("pnpi_op_gemm", ptr(a), K, ptr(w), K, M, N, K, 1.0, ptr(bias), None, ptr(out), col0, col0, ptr(vt), T, 0, T, cfg, 0)
            torch.cuda.synchronize()
            got[cfg] = (out, vt)
    assert torch.equal(got[new][0], got[old][0]) and torch.equal(got[new][1], got[old][1])
    ref = a.float() @ w.float().t() + bias
    assert rel_err(got[new][0], ref[:, :col0]) < 2e-3
    ref_t = ref[:, col0:].reshape(Bn, T, N - col0).permute(0, 2, 1)
    if perm:
        pos = torch.tensor([vt_perm16_pos(t) for t in range(T)], device=DEV)
        stored = torch.empty_like(ref_t)
        stored[:, :, pos] = ref_t
        assert not torch.equal(stored, ref_t)
        ref_t = stored
    assert rel_err(got[new][1], ref_t) < 2e-3


def ilv32(a, g):
    """[.., I] x and gate -> [.., 2I] packed as [x(32) | gate(32)] groups (the layout of the fused GEGLU epilogue)"""
    n = a.shape[-1]
    return torch.stack([a.reshape(*a.shape[:-1], n // 32, 32), g.reshape(*g.shape[:-1], n // 32, 32)], dim=-2).reshape(*a.shape[:-1], 2 * n)


@pytest.mark.parametrize("M,K", [(400, 128), (64, 64), (384, 192)])
@pytest.mark.parametrize("new", [19, 20], ids=["pp128x320", "pp192x256"])
def test_fused_geglu(ctx, new, M, K):
    """The GEGLU epilogue (x * gelu(gate) of interleaved 32-column groups, half as many output columns as the tile has) through
    pnpi_op_gemm_geglu with the tile forced by tuning "igemm_force_cfg": two column tiles; M = 400 ragged for both heights, M = 64 less
    than any tile, M = 384 whole tiles of both; 1, 2, 3 K-tiles.  Bit-identical to the family's tile, and within the kernel suite's
    3e-3 of the fp32 reference (the projection is rounded to fp16 once before the product)."""
    old, bn = FAMILY[new]
    n_int = bn                                                # 2 I = 2 BN columns: two column tiles
    a = h16(M, K, seed=51)
    w = h16(2 * n_int, K, scale=1.0 / math.sqrt(K), seed=52)
    bias = torch.randn(2 * n_int, device=DEV)
    wi = ilv32(w[:n_int].t(), w[n_int:].t()).t().contiguous()
    bi = ilv32(bias[:n_int][None], bias[n_int:][None])[0].contiguous()
    got = {}
    for cfg in (new, old):
        with ctx.tuning(igemm_force_cfg=cfg):
            out = torch.zeros(M, n_int, dtype=torch.half, device=DEV)
            ctx.call("pnpi_op_gemm_geglu", ptr(a), K, ptr(wi), K, M, 2 * n_int, K, ptr(bi), ptr(out), n_int)
            torch.cuda.synchronize()
            got[cfg] = out
    assert torch.equal(got[new], got[old]), (got[new].float() - got[old].float()).abs().max().item()
    h = a.float() @ w.float().t() + bias
    e = rel_err(got[new], h[:, :n_int] * F.gelu(h[:, n_int:]))
    assert e < 3e-3, e


# ------------------------------------------------------------------------------------------------ SD-1.x width: the rule in the forward
STEPS = 2


def _kernels(path):
    """kernel template -> launches, from the per-launch records of a profiled region"""
    n = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            n[r["kernel"]] = n.get(r["kernel"], 0) + 1
    return n


def _profiled(eng, path, fn):
    os.environ["PNPI_PROFILE_DUMP"] = str(path)
    try:
        eng.profile_begin()
        out = fn()
        eng.profile_end()
    finally:
        os.environ.pop("PNPI_PROFILE_DUMP", None)
    return out, _kernels(path)


def _count(kernels, bm, bn):
    return sum(v for k, v in kernels.items() if k.startswith("igemm_pp_kernel<%d %d " % (bm, bn)))


@pytest.fixture(scope="module")
def sd1():
    pipe = NativePipeline(SD1, max_unet_rows=12, max_vae_images=1, text_encoder=SyntheticTextEncoder(SD1.cross_dim, seed=7))
    pipe.load_state_dict(weights.unet_state_dict(SD1, 3), weights.vae_state_dict(SD1, 3))
    yield pipe
    pipe.engine.close()


def test_sd1_eight_row_forward(sd1, tmp_path):
    """one 8-row pnpi_unet_forward: eps bit-identical under both knob values; 128 x 320 launches only under 1"""
    eng = sd1.engine
    S = SD1.sample_size
    lat = torch.randn(8, 4, S, S, generator=torch.Generator().manual_seed(51))
    ctx8 = weights.synth_context(SD1, 8, seed=52)
    got = {}
    for v in (0, 1):
        with eng.tuning(pp_rowtile=v):
            got[v] = _profiled(eng, tmp_path / ("fwd%d.csv" % v), lambda: eng.unet(lat, 500, ctx8).clone())
    print("8-row forward, ping-pong launches by tile: " + ", ".join(
        "pp_rowtile %d: %s" % (v, {k: n for k, n in got[v][1].items() if k.startswith("igemm_pp")}) for v in (0, 1)))
    assert torch.isfinite(got[0][0]).all() and got[0][0].abs().max() > 0
    assert torch.equal(got[1][0], got[0][0]), (got[1][0] - got[0][0]).abs().max().item()
    assert _count(got[0][1], 128, 320) == 0 and _count(got[0][1], 192, 256) == 0
    assert _count(got[0][1], 192, 320) > 0
    assert _count(got[1][1], 128, 320) > 0
    assert _count(got[1][1], 128, 320) + _count(got[1][1], 192, 320) == _count(got[0][1], 192, 320)
    assert _count(got[1][1], 192, 256) + _count(got[1][1], 256, 256) == _count(got[0][1], 256, 256)


def test_sd1_two_step_direct_edit(sd1, tmp_path):
    """a 2-step pnpi_direct_edit of one image, two passes: 12 logical rows launched as 8 on 4 latents, every GEMM configured at the
    12-row count and the row height then chosen on the 8 launched rows -- latents_out and noise_loss_out bit-identical under both knob
    values, both new tiles among the launches under 1 and neither under 0"""
    eng = sd1.engine
    sd1.scheduler.set_timesteps(STEPS)
    ts = sd1.scheduler.timesteps.numpy()
    S = SD1.sample_size
    z0 = torch.randn(1, 4, S, S, generator=torch.Generator().manual_seed(61))
    ctx4 = weights.synth_context(SD1, 4, seed=62).unsqueeze(0)
    traj = eng.ddim_invert(z0, ctx4[:, 2], ts).clone()
    got = {}
    for v in (0, 1):
        with eng.tuning(pp_rowtile=v):
            eng.reset_counters()
            (nl, lats), kern = _profiled(eng, tmp_path / ("edit%d.csv" % v), lambda: eng.direct_edit(traj, ctx4, [None, None], ts, 7.5))
            got[v] = (nl.clone(), lats.clone(), kern, eng.counters())
    print("2-step edit, ping-pong launches by tile: " + ", ".join(
        "pp_rowtile %d: %s" % (v, {k: n for k, n in got[v][2].items() if k.startswith("igemm_pp")}) for v in (0, 1)))
    assert got[0][3]["unet_shared_rows"] == got[1][3]["unet_shared_rows"] == 4 * STEPS
    assert torch.isfinite(got[0][0]).all() and torch.isfinite(got[0][1]).all()
    assert torch.equal(got[1][0], got[0][0]), (got[1][0] - got[0][0]).abs().max().item()
    assert torch.equal(got[1][1], got[0][1]), (got[1][1] - got[0][1]).abs().max().item()
    assert _count(got[0][2], 128, 320) == 0 and _count(got[0][2], 192, 256) == 0
    assert _count(got[1][2], 128, 320) > 0 and _count(got[1][2], 192, 256) > 0
    assert _count(got[1][2], 128, 320) + _count(got[1][2], 192, 320) == _count(got[0][2], 192, 320)
    assert _count(got[1][2], 192, 256) + _count(got[1][2], 256, 256) == _count(got[0][2], 256, 256)
