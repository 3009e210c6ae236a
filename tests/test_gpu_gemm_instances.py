"""Every kernel instance launch_igemm can launch in a product build (csrc/gemm.hip, igemm_dma.inc, igemm_pp.inc), each against the
float64 value of alpha a w^T + bias + res under the per-element bound that tests/test_gemm_bound_host.py derives (applied unchanged), with
the old relative L2 below 2e-3 kept beside it and guard bands checked bit for bit:

  * a is a column range of a NaN-filled buffer (lda = K + 24, data from column 8, one NaN row after row M), w likewise (ldw = K + 8);
  * out has ldo = N rounded up to 8, plus 8 (N + 4 where the case asks for the scalar epilogue) and one spare row, filled with a canary
    that is exact in fp16; transposed outputs have vt_ld = rows_per_batch + 8 and one spare batch item; convolutions one NaN image before
    and after x and one spare output image;
  * before every launch the plan query names the instance the library will launch (its row of the instance table): a forced tile the
    launch is not eligible for (which would silently run as tile 0) fails the test.

Instance -> case: tests/test_gemm_bound_host.py CASES, one row per (instance, K chunk count, epilogue); the parametrised ids are
"<instance>-<M>x<N>x<K>-<epilogue A ... G>[-s<split>]".  In short: every instance at M = BM + 2, N = BN + 8 and 1 / NST - 1 / NST / NST + 1
chunks with the epilogues A (bias as initial accumulator, residual), B (alpha 0.5), C (bias 4-byte aligned), D (plain product), E (scalar
epilogue through ldo % 8 != 0), F (N % 8 != 0); split-K 3 with a short last slice per tile; the k-group tiles at chunk counts their
groups do not divide; the ping-pong tiles at M = 2^15 + 2.

Transposed outputs (test_transposed_outputs): tiles 0 (4-wave), 8 (k-groups), 17 (ping-pong), 0 under igemm_dma = 0 (register-staged), columns
split at vt_col0 = BN, 40 ragged transposed columns, three batch items of rows_per_batch = BM and of 40 tokens, in four forms: fp16 V^T
through the LDS epilogue, the same under igemm_vt_lds = 0 (scalar), fp32 NCHW (vt_col0 = 0), and op_gemm_vt_perm16 held bit-identical to
the plain launch.  40 tokens per item is a multiple of 8, so the LDS form keeps the LDS epilogue there (8-token runs stay inside one
item); its scalar path is what igemm_vt_lds = 0 runs.  The ping-pong kernel has no scalar epilogue: under igemm_vt_lds = 0 and for fp32 the
plan query shows tile 0 in its place (test_gemm_bound_host.py::test_ping_pong_without_row_stores_falls_back_to_tile_0), so those two forms
have no ping-pong case here; the register-staged kernels have no transposed LDS epilogue, so all their forms run the scalar one.

Convolutions (test_every_conv_instance): the same four families at B = 3, H = 7 / 9: 3 x 3 stride 1 pad 1, stride 2 pad 1, stride 2 pad 0 (the
VAE's (0, 1, 0, 1)), the folded 2x upsample, C1 + C2 concat, a 1 x 1 concat; Cin = 8 on the generic-K kernels (both tiles); each of the
four ping-pong tiles (16, 17, 19, 20) in both k orders: the default (igemm_tapin = 0, what the product runs) and igemm_tapin = 1.  S is the
convolution of the absolute values in float64.

GEGLU (test_gemm_geglu_per_element): the tiles of test_gemm_fused_geglu at M = BM + 2, N = 2 (BN + 64), K = 192.

Neighbouring paths (test_neighbouring_paths_bit_identical): tile 17 against 19 and 16 against 20; the ring depths of one tile geometry at
one BKT (128 x 128 x 32: 2 / 3 / 4 / 8 stages; 128 x 128 x 64: 2 / 3; 64 x 64 x 64: 2 / 3 / 4 / 8; 128 x 320 x 32: 2 / 3 / 5; 128 x 256 x 32:
2 / 3 / 6; 256 x 128 x 32: 2 / 3) and tile ids 13, 14, 15, 18 against the id 0 / 5 variant of the same instance; the plan query holds each
launch to the instance its row names.  No comparison is made
between BKT 32 and 64, between k-group and plain tiles (another summation tree), between the ping-pong kernel (16 x 16 x 32 MFMAs) and the
4-wave kernels (32 x 32 x 16), or between the register-staged and the LDS-DMA kernels: nothing in their design promises equal bits.

Worst |got - ref| / bound on an MI355X: register-staged 0.46, 4-wave 0.50, k-groups 0.46, 8-wave 0.48, ping-pong 0.49, split-K 0.50,
transposed 0.47 (fp32 NCHW 0.17), conv 0.47, GEGLU 0.44; the old relative L2 stays at 2.7e-4 or below (GEGLU 4.2e-4).  The device sits
where the host emulation does (0.499): the error is the final fp16 rounding, and every canary and bit-identity pair holds.  With kappa
at 8192 the fp16 bound is in effect 2^-11 (|ref| + S): it catches structural mistakes (a lost term, a wrong row, a shifted bias, a slice
added twice) and not a loss of accumulation precision; only the fp32-output bound (kappa_t 16) holds the accumulation tightly.  The 383
cases of the file run in about four seconds."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402
from tests.test_gemm_bound_host import (CASES, GEGLU_TILES, KAPPA_G, NO_VT, bound_f16, bound_f32, bound_geglu, case_operands,  # noqa: E402
                                        check_case_plan, gemm_inputs, geglu_ref64, geglu_shape, instance_name, query_plan, ref64, worst_ratio)

DEV = "cuda"
CANARY = -77.25              # exactly representable in fp16 and fp32


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def poisoned(t, ld, spare_rows=1):
    """t [rows, cols] as columns 8 ... of a NaN-filled [rows + spare_rows, ld] buffer -> (buffer, pointer to the data)"""
    rows, cols = t.shape
    buf = torch.full((rows + spare_rows, ld), float("nan"), dtype=t.dtype, device=DEV)
    buf[:rows, 8:8 + cols] = t.to(DEV)
    return buf, C.c_void_p(buf.data_ptr() + 8 * t.element_size())


def bias_at(bias, how):
    """-> (buffer, pointer): 'a16' a 16-byte aligned bias, 'a4' one float further (4-byte aligned only), None none"""
    if how is None:
        return None, None
    buf = torch.full((bias.numel() + 1,), float("nan"), dtype=torch.float32, device=DEV)
    off = 1 if how == "a4" else 0
    buf[off:off + bias.numel()] = bias.to(DEV)
    assert (buf.data_ptr() + 4 * off) % 16 == (4 if off else 0)
    return buf, C.c_void_p(buf.data_ptr() + 4 * off)


def canary_intact(buf, written):
    """every element of buf outside the boolean mask `written` still holds the canary, bit for bit"""
    want = torch.full_like(buf, CANARY)
    it = torch.int16 if buf.dtype == torch.half else torch.int32
    return bool((buf.view(it) == want.view(it))[~written].all())


def check(tag, fam, got, ref, S, f32=False, l2=2e-3):
    bound = bound_f32(ref, S) if f32 else bound_f16(ref, S)
    r = worst_ratio(got, ref, bound)
    e = rel_err(got, ref.float())
    print("RATIO %s %s %.3f rel-L2 %.2e" % (fam, tag, r, e))
    assert bool(torch.isfinite(got).all()), tag
    assert r <= 1.0, (tag, r)
    assert e < l2, (tag, e)
    return r


def family_of(case):
    if case.split:
        return "split-K"
    if case.instance.startswith("v1"):
        return "register-staged"
    if case.instance.startswith("pp"):
        return "ping-pong"
    if "kg" in case.instance:
        return "k-groups"
    return "8-wave" if "wgm4" in case.instance else "4-wave"


def run_gemm(ctx, M, N, K, a, w, bias, bias_how, res, alpha, ldo, cfg, split, vt=None):
    """pnpi_op_gemm in the poisoned layout -> (out buffer [M + 1, ldo] or None, vt buffer or None).  vt = (col0, Bn, rpb, f32)"""
    abuf, ap = poisoned(a, K + 24)
    wbuf, wp = poisoned(w, K + 8)
    bbuf, bp = bias_at(bias, bias_how)
    rd = res.to(DEV).contiguous() if res is not None else None
    out = torch.full((M + 1, ldo), CANARY, dtype=torch.half, device=DEV) if ldo else None
    if vt is None:
        ctx.call("pnpi_op_gemm", ap, K + 24, wp, K + 8, M, N, K, alpha, bp, ptr(rd), ptr(out), ldo, NO_VT, None, 0, 0, 1, cfg, split)
        vbuf = None
    else:
        col0, Bn, rpb, f32 = vt
        vbuf = torch.full((Bn + 1, N - col0, rpb + 8), CANARY, dtype=torch.float32 if f32 else torch.half, device=DEV)
        ctx.call("pnpi_op_gemm", ap, K + 24, wp, K + 8, M, N, K, alpha, bp, ptr(rd), ptr(out), ldo if ldo else N, col0, ptr(vbuf), rpb + 8, int(f32), rpb,
                 cfg, split)
    torch.cuda.synchronize()
    del abuf, wbuf, bbuf
    return out, vbuf


# ------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_gemm_instance(ctx, case):
    lib = ctx.lib
    a, w, bias, res = case_operands(case)
    with _capi.tuning(lib, **dict(case.tune)):
        pl = query_plan(lib, case.M, case.N, case.K, cfg=case.cfg, split=case.split, lda=case.K + 24, ldw=case.K + 8, ldo=case.ldo, bias=case.bias,
                        res=case.res)
        check_case_plan(lib, case, pl)
        out, _ = run_gemm(ctx, case.M, case.N, case.K, a, w, bias, case.bias, res, case.alpha, case.ldo, case.cfg, case.split)
    M, N = case.M, case.N
    ref, S = ref64(a.to(DEV), w.to(DEV), bias.to(DEV) if bias is not None else None, res.to(DEV) if res is not None else None, case.alpha)
    check(case.name, family_of(case), out[:M, :N], ref, S)
    written = torch.zeros_like(out, dtype=torch.bool)
    written[:M, :N] = True
    assert canary_intact(out, written), case.name


# ------------------------------------------------------------------------------------------------ transposed outputs
# (family, tile id, tuning, BM, BN)
VT_FAMILIES = [("4-wave", 0, {}, 128, 128), ("k-groups", 8, {}, 64, 64), ("ping-pong", 17, {}, 192, 320), ("register-staged", 0, {"igemm_dma": 0}, 128, 128)]
VT_FORMS = ("lds", "scalar", "f32", "perm16")


def unperm16(t):
    """undo the permuted key order of GemmP::vt_perm16 along the last axis: token t was stored at t ^ 12 where bits 2 and 3 of t differ"""
    pos = torch.arange(t.shape[-1], device=t.device)
    src = torch.where((((pos >> 2) ^ (pos >> 3)) & 1).bool(), pos ^ 12, pos)
    return t[..., src]


# the permuted key order moves whole 16-token groups: the launcher rejects it at rows_per_batch = 40 (err -9, tests/test_igemm_plan_host.py).
# The ping-pong kernel has no scalar epilogue: its scalar and fp32 forms would run on tile 0
# (test_gemm_bound_host.py::test_ping_pong_without_row_stores_falls_back_to_tile_0), which has its own cases here
VT_CASES = [(f, tall, form) for f in VT_FAMILIES for tall in (True, False) for form in VT_FORMS
            if (tall or form != "perm16") and not (f[0] == "ping-pong" and form in ("scalar", "f32"))]


@pytest.mark.parametrize("famrow,tall,form", VT_CASES, ids=["%s-%s-%s" % (f[0], "rpbBM" if t else "rpb40", form) for f, t, form in VT_CASES])
def test_transposed_outputs(ctx, famrow, tall, form):
    lib = ctx.lib
    fam, cfg, tune, bm, bn = famrow
    rpb, Bn, K = (bm if tall else 40), 3, 128
    M = Bn * rpb
    col0 = 0 if form == "f32" else bn
    N = bn + 40
    f32 = form == "f32"
    ldo = 0 if f32 else col0 + 8
    a, w, bias, _ = gemm_inputs(M, N, K)
    tune = dict(tune)
    if form == "scalar":
        tune["igemm_vt_lds"] = 0
    with _capi.tuning(lib, **tune):
        pl = query_plan(lib, M, N, K, cfg=cfg, lda=K + 24, ldw=K + 8, ldo=ldo if ldo else N, bias="a16", vt_col0=col0, vt_ld=rpb + 8, vt_f32=int(f32),
                        rpb=rpb, vt_perm16=int(form == "perm16"))
        assert pl.err == 0
        assert pl.id == cfg and pl.epi_lds == int(form in ("lds", "perm16") and fam != "register-staged") and bool(pl.dma) == (fam != "register-staged"), (pl.id, pl.epi_lds, pl.dma)
        with _capi.tuning(lib, op_gemm_vt_perm16=int(form == "perm16")):
            out, vt = run_gemm(ctx, M, N, K, a, w, bias, "a16", None, 1.0, ldo, cfg, 0, vt=(col0, Bn, rpb, f32))
        if form == "perm16":
            out0, vt0 = run_gemm(ctx, M, N, K, a, w, bias, "a16", None, 1.0, ldo, cfg, 0, vt=(col0, Bn, rpb, f32))
    tag = "%s-%s-rpb%d" % (fam, form, rpb)
    ref, S = ref64(a.to(DEV), w.to(DEV), bias.to(DEV), None, 1.0)
    if form == "perm16":           # the same bits as the plain launch, in the permuted order; the pad and the spare item untouched
        assert torch.equal(out.view(torch.int16), out0.view(torch.int16)), tag
        un = vt.clone()
        un[:, :, :rpb] = unperm16(vt[:, :, :rpb])
        assert torch.equal(un.view(torch.int16), vt0.view(torch.int16)), tag
        vt = un
    gotT = vt[:Bn, :, :rpb].permute(0, 2, 1).reshape(M, N - col0)
    check(tag + "-T", "transposed", gotT, ref[:, col0:], S[:, col0:], f32=f32, l2=2e-3 if not f32 else 1e-5)
    wv = torch.zeros_like(vt, dtype=torch.bool)
    wv[:Bn, :, :rpb] = True
    assert canary_intact(vt, wv), tag
    if out is not None:
        check(tag + "-plain", "transposed", out[:M, :col0], ref[:, :col0], S[:, :col0])
        wo = torch.zeros_like(out, dtype=torch.bool)
        wo[:M, :col0] = True
        assert canary_intact(out, wo), tag


# ------------------------------------------------------------------------------------------------ convolutions
# (name, C1, C2, H, ksize, stride, pad, ups, residual)
CONV_SHAPES = [
    ("s1p1", 64, 0, 7, 3, 1, 1, 0, True),
    ("s2p1", 64, 0, 9, 3, 2, 1, 0, False),
    ("s2p0", 64, 0, 9, 3, 2, 0, 0, False),          # the VAE's (0, 1, 0, 1) padding
    ("ups", 64, 0, 7, 3, 1, 1, 1, True),
    ("concat", 64, 64, 9, 3, 1, 1, 0, False),
    ("1x1concat", 128, 64, 7, 1, 1, 0, 0, True),
]
# (family, tile id, tuning, BN, instance prefix)
CONV_FAMILIES = [("4-wave", 0, {}, 128, "dma<128,128,32,8>"), ("k-groups", 8, {}, 64, "dma<64,64,64,2,kg4>"), ("k-groups2", 10, {}, 128, "dma<128,128,64,2,kg2>"),
                 ("ping-pong-192x320", 17, {}, 320, "pp<192,320>"), ("ping-pong-192x320-tapin", 17, {"igemm_tapin": 1}, 320, "pp<192,320>"),
                 ("ping-pong-256x256", 16, {}, 256, "pp<256,256>"), ("ping-pong-256x256-tapin", 16, {"igemm_tapin": 1}, 256, "pp<256,256>"),
                 ("ping-pong-128x320", 19, {}, 320, "pp<128,320>"), ("ping-pong-128x320-tapin", 19, {"igemm_tapin": 1}, 320, "pp<128,320>"),
                 ("ping-pong-192x256", 20, {}, 256, "pp<192,256>"), ("ping-pong-192x256-tapin", 20, {"igemm_tapin": 1}, 256, "pp<192,256>"),
                 ("register-staged", 0, {"igemm_dma": 0}, 128, "v1<128,128,fast>"), ("register-staged-64", 1, {"igemm_dma": 0}, 64, "v1<64,64,fast>")]
CONV_CASES = [(f, s) for f in CONV_FAMILIES for s in CONV_SHAPES] + \
             [(("generic-K", 0, {}, 128, "v1<128,128,generic>"), ("cin8", 8, 0, 9, 3, 1, 1, 0, True)),
              (("generic-K-64", 1, {}, 64, "v1<64,64,generic>"), ("cin8", 8, 0, 9, 3, 1, 1, 0, True)),
              (("generic-K-64", 1, {}, 64, "v1<64,64,generic>"), ("cin8s2", 8, 0, 9, 3, 2, 0, 0, False))]
CONV_B = 3


@functools.lru_cache(maxsize=None)
def conv_reference(C1, C2, H, ks, stride, pad, ups, N, has_res):
    """x [B, Cin, H, H], w [N, Cin, ks, ks] fp16, bias fp32, res fp16 or None, ref and S float64 [B, N, Ho, Wo]: all on the CPU, shared"""
    g = torch.Generator().manual_seed(101 * C1 + 7 * C2 + 13 * H + ks + 3 * stride + pad + 5 * ups + N)
    Cin = C1 + C2
    x = torch.randn(CONV_B, Cin, H, H, generator=g).half()
    w = (torch.randn(N, Cin, ks, ks, generator=g) / (ks * ks * Cin) ** 0.5).half()
    x[1, :, 2, 3] = 0.0                                 # an all-zero pixel
    bias = torch.randn(N, generator=g)

    def conv(xx, ww):
        if ups:
            xx = F.interpolate(xx, scale_factor=2.0, mode="nearest")
        if stride == 2 and pad == 0:
            return F.conv2d(F.pad(xx, (0, 1, 0, 1)), ww, None, stride=2, padding=0)
        return F.conv2d(xx, ww, None, stride=stride, padding=pad)

    ref = conv(x.double(), w.double()) + bias.double()[None, :, None, None]
    S = conv(x.double().abs(), w.double().abs()) + bias.double().abs()[None, :, None, None]
    res = torch.randn(ref.shape, generator=g).half() if has_res else None
    if has_res:
        ref, S = ref + res.double(), S + res.double().abs()
    return x, w, bias, res, ref, S


@pytest.mark.parametrize("famrow,shape", CONV_CASES, ids=["%s-%s" % (f[0], s[0]) for f, s in CONV_CASES])
def test_every_conv_instance(ctx, famrow, shape):
    lib = ctx.lib
    fam, cfg, tune, bn, instance = famrow
    sname, C1, C2, H, ks, stride, pad, ups, has_res = shape
    N = bn + 8
    x, w, bias, res, ref, S = conv_reference(C1, C2, H, ks, stride, pad, ups, N, has_res)
    B, Ho, Wo = CONV_B, ref.shape[2], ref.shape[3]
    M, K = B * Ho * Wo, ks * ks * (C1 + C2)

    def nhwc_poisoned(t):                               # one NaN image before and one after
        buf = torch.full((B + 2,) + tuple(t.shape[2:]) + (t.shape[1],), float("nan"), dtype=torch.half, device=DEV)
        buf[1:B + 1] = t.permute(0, 2, 3, 1).to(DEV)
        return buf

    x1 = nhwc_poisoned(x[:, :C1])
    x2 = nhwc_poisoned(x[:, C1:]) if C2 else None
    wp = w.permute(0, 2, 3, 1).reshape(N, K).contiguous().to(DEV)
    bd = bias.to(DEV)
    rd = res.permute(0, 2, 3, 1).contiguous().to(DEV) if has_res else None
    out = torch.full((B + 1, Ho, Wo, N), CANARY, dtype=torch.half, device=DEV)
    with _capi.tuning(lib, **tune):
        pl = query_plan(lib, M, N, K, cfg=cfg, bias="a16", res=has_res, ksize=ks, C1=C1, C2=C2)
        assert pl.err == 0 and pl.id == cfg and instance_name(lib, pl) == instance, (pl.err, pl.id, instance_name(lib, pl))
        assert pl.k_order == int(tune.get("igemm_tapin", 0) == 1 and ks == 3 and instance.startswith("pp"))
        ctx.call("pnpi_op_conv", ptr(x1[1:]), ptr(x2[1:]) if C2 else None, C1, C2, B, H, H, ks, stride, pad, ups, Ho, Wo, ptr(wp), ptr(bd), ptr(rd), N,
                 ptr(out), cfg, 0)
        torch.cuda.synchronize()
    tag = "%s-%s" % (fam, sname)
    check(tag, "conv", out[:B].permute(0, 3, 1, 2), ref.to(DEV), S.to(DEV))
    written = torch.zeros_like(out, dtype=torch.bool)
    written[:B] = True
    assert canary_intact(out, written), tag


# ------------------------------------------------------------------------------------------------ GEGLU
@pytest.mark.parametrize("cfg", GEGLU_TILES)
def test_gemm_geglu_per_element(ctx, cfg):
    lib = ctx.lib
    M, N, K = geglu_shape(cfg)
    a, w, bias, _ = gemm_inputs(M, N, K)
    I, ldo = N // 2, N // 2 + 8
    abuf, ap = poisoned(a, K + 24)
    wbuf, wp = poisoned(w, K + 8)
    bbuf, bp = bias_at(bias, "a16")
    out = torch.full((M + 1, ldo), CANARY, dtype=torch.half, device=DEV)
    with _capi.tuning(lib, igemm_force_cfg=cfg):
        pl = query_plan(lib, M, N, K, cfg=-1, lda=K + 24, ldw=K + 8, ldo=ldo, bias="a16", geglu=1)
        assert (pl.err, pl.id, pl.epi_lds) == (0, cfg, 1), (pl.err, pl.id)
        ctx.call("pnpi_op_gemm_geglu", ap, K + 24, wp, K + 8, M, N, K, bp, ptr(out), ldo)
        torch.cuda.synchronize()
    ref, slack = geglu_ref64(a.to(DEV), w.to(DEV), bias.to(DEV))
    got = out[:M, :I]
    r = worst_ratio(got, ref, bound_geglu(ref, slack, KAPPA_G))
    e = rel_err(got, ref.float())
    print("RATIO GEGLU tile%d %.3f rel-L2 %.2e" % (cfg, r, e))
    assert bool(torch.isfinite(got).all())
    assert r <= 1.0, (cfg, r)
    assert e < 3e-3, (cfg, e)                          # test_gemm_fused_geglu's figure
    written = torch.zeros_like(out, dtype=torch.bool)
    written[:M, :I] = True
    assert canary_intact(out, written), cfg


# ------------------------------------------------------------------------------------------------ neighbouring paths
# groups of (tile id, tuning, the instance that row is there for) that walk the same chunks in the same order: bit-identical outputs on
# one input.  (M, N, K, groups)
NEIGHBOURS = [
    ("pp-320", 386, 328, 192, [(17, {}, "pp<192,320>"), (19, {}, "pp<128,320>")]),
    ("pp-256", 514, 264, 192, [(16, {}, "pp<256,256>"), (20, {}, "pp<192,256>")]),
    ("128x128x32", 130, 136, 320, [(0, {"igemm_v128": 4}, "dma<128,128,32,2>"), (0, {"igemm_deep_rings": 0}, "dma<128,128,32,3>"),
                                   (0, {"igemm_v128": 3}, "dma<128,128,32,4>"), (0, {}, "dma<128,128,32,8>"), (13, {}, "dma<128,128,32,2>")]),
    ("128x128x64", 130, 136, 320, [(0, {"igemm_v128": 0}, "dma<128,128,64,2>"), (0, {"igemm_v128": 1}, "dma<128,128,64,3>"),
                                   (14, {}, "dma<128,128,64,2>"), (18, {}, "dma<128,128,64,3>")]),
    ("64x64x64", 66, 72, 576, [(1, {"igemm_v64": 1}, "dma<64,64,64,2>"), (1, {"igemm_deep_rings": 0}, "dma<64,64,64,3>"),
                               (1, {"igemm_v64": 2}, "dma<64,64,64,4>"), (1, {}, "dma<64,64,64,8>")]),
    ("128x320x32", 130, 328, 384, [(4, {"igemm_deep_rings": 0}, "dma<128,320,32,2>"), (4, {"igemm_v320": 0}, "dma<128,320,32,3>"),
                                   (4, {}, "dma<128,320,32,5>")]),
    ("128x256x32", 130, 264, 448, [(5, {"igemm_deep_rings": 0}, "dma<128,256,32,2>"), (5, {"igemm_v256n": 0}, "dma<128,256,32,3>"),
                                   (5, {}, "dma<128,256,32,6>")]),
    ("128x256x64", 130, 264, 192, [(5, {"igemm_v256n": 2}, "dma<128,256,64,2>"), (15, {}, "dma<128,256,64,2>")]),
    ("256x128x32", 258, 136, 256, [(3, {"igemm_v256": 1}, "dma<256,128,32,2>"), (3, {}, "dma<256,128,32,3>")]),
]


# the 256 x 128 tile takes no split-K (kTileDesc)
NEIGHBOUR_CASES = [n + (split,) for n in NEIGHBOURS for split in (0, 3) if not (split and n[0] == "256x128x32")]


@pytest.mark.parametrize("name,M,N,K,group,split", NEIGHBOUR_CASES, ids=["%s-s%d" % (n[0], n[5]) for n in NEIGHBOUR_CASES])
def test_neighbouring_paths_bit_identical(ctx, name, M, N, K, group, split):
    lib = ctx.lib
    a, w, bias, res = gemm_inputs(M, N, K)
    ldo = (N + 7) // 8 * 8 + 8
    outs, names = [], []
    for cfg, tune, instance in group:
        with _capi.tuning(lib, **tune):
            pl = query_plan(lib, M, N, K, cfg=cfg, split=split, lda=K + 24, ldw=K + 8, ldo=ldo, bias="a16", res=True)
            assert pl.err == 0 and pl.id == cfg and pl.split == max(split, 1), (cfg, pl.id, pl.split)
            assert instance_name(lib, pl) == instance, (name, cfg, tune, instance_name(lib, pl))      # the ring depth this row was written for
            out, _ = run_gemm(ctx, M, N, K, a, w, bias, "a16", res, 1.0, ldo, cfg, split)
        outs.append(out)
        names.append(instance)
    assert len(set((cfg, instance) for cfg, _, instance in group)) == len(group), names       # no launch is compared with itself
    assert bool(torch.isfinite(outs[0][:M, :N]).all()) and float(outs[0][:M, :N].abs().max()) > 0
    for n, o in zip(names[1:], outs[1:]):
        assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), (name, names[0], n, (o.float() - outs[0].float())[:M, :N].abs().max().item())
