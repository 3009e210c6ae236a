"""The forward bandwidth kernels of csrc/norm.hip instance by instance, per element against float64: GroupNorm (+SiLU) in its three forms
(gn_small_kernel<1024>, gn_small_kernel<256>, the three-pass gn_stats / gn_finalize / gn_apply kernels), layernorm_kernel<VPL, RPW>,
geglu_kernel, softmax_rows_kernel, softmax_rows_f32_kernel, f32_rows_to_f16_padded_kernel and gemv_kernel (the last three through the
kernel-level entry points pnpi_op_softmax_rows_f32, pnpi_op_f32_rows_to_f16_padded and pnpi_op_gemv).

Inputs, references, bounds and every kappa come from tests/test_norm_fwd_bound_host.py, which shows where they come from.  Every case
checks
  * the per-element bound of its operation;
  * the suite's global rel-L2 < 2e-3 as well;
  * an output one item / row longer than needed and pre-filled with 777.0: the tail keeps it, the body holds none;
  * a second launch gives the same bits.
Every GroupNorm case states the kernel it is there for and asserts the conditions of gn_small_ok / launch_gn_small (cpg % 4, the slice
against 24576, or 8192 from 1536 blocks on, B G against "gn_wide_below"), so a shape shrunk into another kernel fails instead of passing
vacuously.  The refusals at the end are widths and counts the host code rejects before any launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi  # noqa: E402
from tests import test_norm_fwd_bound_host as H  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402

DEV = "cuda"
SENTINEL = 777.0
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx48():
    """the statistics scratch of the three-pass kernels is sized by the context's row count"""
    c = Ctx(max_rows=48)
    yield c
    c.close()


def ratio_of(op, tag, got, ref, bound):
    r = ((got.double().cpu() - ref).abs() / bound).max().item()
    WORST[op] = max(WORST.get(op, 0.0), r)
    print("%s %s: worst |err| / bound %.3f (worst of %s so far %.3f)" % (op, tag, r, op, WORST[op]))
    return r


def guarded(rows, *shape, dtype=torch.half):
    """[rows + 1, *shape] pre-filled with the sentinel"""
    return torch.full((rows + 1,) + shape, SENTINEL, dtype=dtype, device=DEV)


def check_guard(out, rows):
    assert torch.equal(out[rows], torch.full_like(out[rows], SENTINEL)), "wrote past the last row"
    assert not (out[:rows] == SENTINEL).any(), "left part of the output unwritten"
    assert torch.isfinite(out[:rows]).all()


def untouched(out):
    return torch.equal(out, torch.full_like(out, SENTINEL))


# ------------------------------------------------------------------------------------------------ GroupNorm
PASS_WHY = {
    (1, 2048, 0, 25, 2): "slice>24576", (48, 256, 0, 1028, 32): "slice>8192@1536", (2, 8, 0, 70, 8): "cpg%4", (2, 8, 24, 50, 32): "cpg%4",
    (2, 96, 0, 50, 32): "cpg%4", (2, 320, 0, 200, 32): "cpg%4", (1, 1040, 1040, 70, 32): "cpg%4", (1, 96, 0, 8200, 32): "cpg%4",
    (2, 192, 0, 40, 64): "cpg%4", (1, 32, 0, 3100, 4): "slice>24576",
}


def assert_kernel_instance(case, kernel, wide_below):
    """gn_small_ok and launch_gn_small (csrc/norm.hip) restated for the instance this case is there for"""
    B, C1, C2, HW, G = case
    cpg = (C1 + C2) // G
    lim = 8192 if B * G >= 1536 else 24576
    if kernel == "pass":
        why = PASS_WHY[case]
        if why == "cpg%4":
            assert cpg % 4 != 0, cpg
        elif why == "slice>24576":
            assert cpg % 4 == 0 and B * G < 1536 and HW * cpg > 24576, HW * cpg
        else:
            assert why == "slice>8192@1536" and cpg % 4 == 0 and B * G >= 1536 and 8192 < HW * cpg <= 24576, (B * G, HW * cpg)
        return
    assert cpg % 4 == 0 and C1 % 4 == 0 and cpg <= 1024 and HW * cpg <= lim, (cpg, HW * cpg, lim)
    if kernel == "small1024":
        assert B * G < wide_below
    else:
        assert kernel == "small256" and B * G >= wide_below


def gn_launch(c, case, silu, eps):
    B, C1, C2, HW, G = case
    x, gamma, beta = (t.to(DEV) for t in H.gn_inputs(case))
    x1 = x[:, :, :C1].contiguous()
    x2 = x[:, :, C1:].contiguous() if C2 else None
    out = guarded(B, HW, C1 + C2)
    status = c.lib.pnpi_op_groupnorm(c.h, ptr(x1), ptr(x2), C1, C2, B, HW, G, eps, ptr(gamma), ptr(beta), silu, ptr(out))
    torch.cuda.synchronize()
    assert status == 0, (status, c.lib.pnpi_last_error(c.h))
    return out


@pytest.mark.parametrize("silu,eps", H.GN_FLAVOURS)
@pytest.mark.parametrize("case,kernel", H.GN_RUNS, ids=["%s-%s" % ("x".join(map(str, c)), k) for c, k in H.GN_RUNS])
def test_groupnorm_instance(ctx, ctx48, case, kernel, silu, eps):
    wide_below = 0 if kernel == "small256" else 1 << 30
    assert_kernel_instance(case, kernel, wide_below)
    B = case[0]
    c = ctx48 if B > 4 else ctx
    with c.tuning(gn_wide_below=wide_below):
        assert _capi.get_tuning(c.lib, "gn_small_max") == 24576
        out = gn_launch(c, case, silu, eps)
        out2 = gn_launch(c, case, silu, eps)
    check_guard(out, B)
    assert torch.equal(out, out2), "a second launch gave other bits"
    ref, slack = H.gn_reference(case, silu, eps)
    r = ratio_of("GroupNorm", "%s %s silu %d eps %g" % (case, kernel, silu, eps), out[:B], ref, H.gn_bound(ref, slack))
    e = rel_err(out[:B].cpu().double(), ref)
    assert r <= 1.0, r
    assert e < 2e-3, e


@pytest.mark.parametrize("case,kernel", [((2, 40, 88, 50, 8), "small1024"), ((2, 320, 0, 200, 32), "pass")])
def test_groupnorm_swapped_items_are_noticed(ctx, case, kernel):
    """the harness itself: the reference of the two items' statistics exchanged (what `0` for `b` in an index does to item 1) is far
    outside the bound of what the kernel gives -- the inputs' per-item offsets are there for this"""
    assert_kernel_instance(case, kernel, 1 << 30)
    x, gamma, beta = H.gn_inputs(case)
    mean, var = H.gn_stats64(x, case[4])
    ref, slack = H.gn_formula64(x, mean.flip(0), var.flip(0), gamma, beta, 1e-5, 1)
    out = gn_launch(ctx, case, 1, 1e-5)
    r = ((out[:2].double().cpu() - ref).abs() / H.gn_bound(ref, slack)).max().item()
    print("GroupNorm %s %s against swapped statistics: ratio %.1f" % (case, kernel, r))
    assert r > 10


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("M,C,eps", H.LN_CASES)
def test_layernorm_instance(ctx, M, C, eps):
    x, gamma, beta = (t.to(DEV) for t in H.ln_inputs(M, C))

    def launch():
        out = guarded(M, C)
        ctx.call("pnpi_op_layernorm", ptr(x), M, C, eps, ptr(gamma), ptr(beta), ptr(out))
        torch.cuda.synchronize()
        return out

    out = launch()
    check_guard(out, M)
    assert torch.equal(out, launch()), "a second launch gave other bits"
    ref, slack = H.ln_reference((M, C, eps))
    r = ratio_of("LayerNorm", "(%d, %d) eps %g" % (M, C, eps), out[:M], ref, H.ln_bound(ref, slack))
    assert r <= 1.0, r
    assert rel_err(out[:M].cpu().double(), ref) < 2e-3


# ------------------------------------------------------------------------------------------------ GEGLU
@pytest.mark.parametrize("M,I", H.GEGLU_CASES)
def test_geglu_instance(ctx, M, I):
    if M * I // 8 > 4096 * 256:
        assert (M * I // 8 + 255) // 256 > 4096          # the grid is capped: a second stride trip
    a, g = H.geglu_inputs((M, I))
    xi = H.ilv32(a, g).contiguous().to(DEV)

    def launch():
        out = guarded(M, I)
        ctx.call("pnpi_op_geglu", ptr(xi), M, I, ptr(out))
        torch.cuda.synchronize()
        return out

    out = launch()
    check_guard(out, M)
    assert torch.equal(out, launch()), "a second launch gave other bits"
    ref, ag = H.geglu_reference((M, I))
    r = ratio_of("GEGLU", "(%d, %d)" % (M, I), out[:M], ref, H.geglu_bound(ref, ag))
    assert r <= 1.0, r
    assert rel_err(out[:M].cpu().double(), ref) < 2e-3


# ------------------------------------------------------------------------------------------------ row softmax
@pytest.mark.parametrize("M,N,ld", H.SM16_CASES)
def test_softmax_rows_instance(ctx, M, N, ld):
    x = H.softmax_inputs(M, N, False)

    def launch():
        buf = guarded(M, ld)
        buf[:M, :N] = x.to(DEV)
        buf[:M, N:] = float("nan")
        before = buf.clone()
        ctx.call("pnpi_op_softmax_rows", ptr(buf), M, N, ld)
        torch.cuda.synchronize()
        return buf, before

    buf, before = launch()
    assert torch.equal(buf[M], torch.full_like(buf[M], SENTINEL)), "wrote past the last row"
    assert torch.equal(buf[:M, N:].view(torch.int16), before[:M, N:].view(torch.int16)), "the pad columns changed"
    assert torch.isfinite(buf[:M, :N]).all()
    assert torch.equal(buf.view(torch.int16), launch()[0].view(torch.int16)), "a second launch gave other bits"
    ref, dist = H.softmax_reference(M, N, False)
    r = ratio_of("softmax fp16", "(%d, %d, %d)" % (M, N, ld), buf[:M, :N], ref, H.softmax_bound(ref, dist, False))
    assert r <= 1.0, r
    assert rel_err(buf[:M, :N].cpu().double(), ref) < 2e-3


@pytest.mark.parametrize("M,N", H.SM32_CASES)
def test_softmax_rows_f32_instance(ctx, M, N):
    x = H.softmax_inputs(M, N, True)

    def launch():
        buf = guarded(M, N, dtype=torch.float32)
        buf[:M] = x.to(DEV)
        ctx.call("pnpi_op_softmax_rows_f32", ptr(buf), M, N)
        torch.cuda.synchronize()
        return buf

    buf = launch()
    check_guard(buf, M)
    assert torch.equal(buf, launch()), "a second launch gave other bits"
    ref, dist = H.softmax_reference(M, N, True)
    got, bound = buf[:M].double().cpu(), H.softmax_bound(ref, dist, True)
    assert ((got - ref).abs() <= bound).all()                  # (also where ref and the bound are both 0)
    live = bound > 0
    r = ratio_of("softmax fp32", "(%d, %d)" % (M, N), got[live], ref[live], bound[live])
    assert r <= 1.0, r
    assert rel_err(got, ref) < 2e-3


@pytest.mark.parametrize("M,N,ld", [(5, 77, 80), (26300, 77, 80)])
def test_f32_rows_to_f16_padded_instance(ctx, M, N, ld):
    if M > 5:
        assert M * ld > 8192 * 256 and M * ld < 2 * 8192 * 256      # the grid is capped at 8192 blocks: a second stride trip, not a third
    gen = torch.Generator().manual_seed(8000 + M)
    src = torch.softmax(torch.randn(M, N, generator=gen) * 3, 1)
    src[0, :8] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11, 3e-8])
    src = src.to(DEV)

    def launch():
        out = guarded(M, ld)
        ctx.call("pnpi_op_f32_rows_to_f16_padded", ptr(src), M, N, ld, ptr(out))
        torch.cuda.synchronize()
        return out

    out = launch()
    assert torch.equal(out[M], torch.full_like(out[M], SENTINEL)), "wrote past the last row"
    assert torch.equal(out[:M, :N].view(torch.int16), src.half().view(torch.int16))
    assert torch.equal(out[:M, N:].view(torch.int16), torch.zeros(M, ld - N, dtype=torch.int16, device=DEV))
    assert torch.equal(out, launch())


# ------------------------------------------------------------------------------------------------ GEMV
@pytest.mark.parametrize("K,N,silu,b1,b2", H.GEMV_CASES)
def test_gemv_instance(ctx, K, N, silu, b1, b2):
    x, W, bias, bias2 = (t.to(DEV) for t in H.gemv_inputs(K, N))

    def launch():
        out = guarded(N, dtype=torch.float32)
        ctx.call("pnpi_op_gemv", ptr(x), K, ptr(W), N, ptr(bias) if b1 else None, ptr(bias2) if b2 else None, silu, ptr(out))
        torch.cuda.synchronize()
        return out

    out = launch()
    check_guard(out, N)
    assert torch.equal(out, launch()), "a second launch gave other bits"
    ref, mag = H.gemv_reference((K, N, silu, b1, b2))
    r = ratio_of("GEMV", "(%d, %d) silu %d bias %d%d" % (K, N, silu, b1, b2), out[:N], ref, H.gemv_bound(mag))
    assert r <= 1.0, r
    assert rel_err(out[:N].cpu().double(), ref) < 2e-3


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_before_any_launch(ctx):
    """widths and counts the host code rejects: an error, and the sentinel-filled output untouched (no null pointers here)"""
    lib, h = ctx.lib, ctx.h
    half = lambda *s: torch.ones(*s, dtype=torch.half, device=DEV)      # noqa: E731
    f32 = lambda *s: torch.ones(*s, dtype=torch.float32, device=DEV)    # noqa: E731
    for C in (12, 2056):
        out = guarded(4, C)
        assert lib.pnpi_op_layernorm(h, ptr(half(4, C)), 4, C, 1e-5, ptr(f32(C)), ptr(f32(C)), ptr(out)) == _capi.PNPI_ESHAPE
        assert untouched(out)
    for M in (0, -3):
        out = guarded(4, 32)
        assert lib.pnpi_op_layernorm(h, ptr(half(4, 32)), M, 32, 1e-5, ptr(f32(32)), ptr(f32(32)), ptr(out)) != 0
        assert untouched(out)
    for M, I, want in ((4, 48, _capi.PNPI_ESHAPE), (0, 32, _capi.PNPI_EINVAL), (-1, 32, _capi.PNPI_EINVAL), (4, 0, _capi.PNPI_EINVAL)):
        out = guarded(4, 64)
        assert lib.pnpi_op_geglu(h, ptr(half(4, 128)), M, I, ptr(out)) == want, (M, I)
        assert untouched(out)
    for M, N, ld, want in ((4, 12, 16, _capi.PNPI_ESHAPE), (4, 8, 12, _capi.PNPI_ESHAPE), (0, 8, 8, _capi.PNPI_EINVAL), (-2, 8, 8, _capi.PNPI_EINVAL),
                           (4, 0, 8, _capi.PNPI_EINVAL), (4, -8, 8, _capi.PNPI_EINVAL)):
        buf = guarded(4, 16)
        assert lib.pnpi_op_softmax_rows(h, ptr(buf), M, N, ld) == want, (M, N, ld)
        assert untouched(buf)
    for M, N in ((0, 8), (-1, 8), (4, 0), (4, -1)):
        buf = guarded(4, 8, dtype=torch.float32)
        assert lib.pnpi_op_softmax_rows_f32(h, ptr(buf), M, N) == _capi.PNPI_EINVAL, (M, N)
        assert untouched(buf)
        out = guarded(4, 8)
        assert lib.pnpi_op_f32_rows_to_f16_padded(h, ptr(f32(4, 8)), M, N, 8, ptr(out)) == _capi.PNPI_EINVAL, (M, N)
        assert untouched(out)
    for K, N, want in ((12, 4, _capi.PNPI_ESHAPE), (0, 4, _capi.PNPI_EINVAL), (-8, 4, _capi.PNPI_EINVAL), (8, 0, _capi.PNPI_EINVAL), (8, -4, _capi.PNPI_EINVAL)):
        out = guarded(4, dtype=torch.float32)
        assert lib.pnpi_op_gemv(h, ptr(f32(16)), K, ptr(half(4, 16)), N, ptr(f32(4)), ptr(f32(4)), 1, ptr(out)) == want, (K, N)
        assert untouched(out)
    torch.cuda.synchronize()
