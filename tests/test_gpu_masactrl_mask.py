"""Mask-guided MasaCtrl on the GPU: the class-restricted self-attention kernel (pnpi_op_attention_masked) against the reference's own
MutualSelfAttentionControlMask outputs (tests/golden/masactrl_mask_attn.npz), the per-level mask resize against F.interpolate, and whole
edits on SMALL64 against the reference's pipeline (tests/golden/e2e_masactrl_mask.npz); both fixtures by tools/make_golden_masactrl_mask.py.
Tolerances are the existing ones: attention kernels rel-L2 <= 3e-3 (tests/test_gpu_kernels.py, every head width; masking adds no rounding
step), MasaCtrl latents on SMALL64 rel-L2 <= 2e-2 (tests/test_gpu_loops.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi, weights  # noqa: E402
from pnpinversion_amd.config import SMALL64  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402
from tests.gpu_util import Ctx, max_err, ptr, rel_err  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
ATTN_BAR = 3e-3
E2E_BAR = 2e-2
DP = {"d40": 64, "d80": 96, "d160": 160, "d16": 32}
CASES = ["rect", "empty_fg", "full_fg", "single_key", "full_t"]


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "masactrl_mask_attn.npz"))


def one_pass(q, k, v, kcls, qcls, scale):
    """fp32 statement of the kernel's rule: query i sees the keys j with kcls[j] == qcls[i]; no such key -> uniform over all keys"""
    sim = q.float() @ k.float().t() * scale
    allowed = kcls.bool()[None, :] == qcls.bool()[:, None]
    logits = torch.where(allowed, sim, torch.full_like(sim, float("-inf")))
    logits = torch.where(allowed.any(-1, keepdim=True), logits, torch.zeros_like(sim))
    return logits.softmax(-1) @ v.float()


def pack(q, k, v, Dp, perm=False):
    """q / k / v [rows, heads, N, dh] fp16 -> head-padded Q / K rows and V^T (NaN pads, as tests/test_gpu_kernels.py make_qkv)"""
    R, heads, N, dh = q.shape
    Nk = k.shape[2]
    hd = heads * Dp
    qb = torch.zeros(R, N, hd, dtype=torch.half, device=DEV)
    kb = torch.zeros(R, Nk, hd, dtype=torch.half, device=DEV)
    ldv = (Nk + 7) // 8 * 8
    vt = torch.full((R, heads, Dp, ldv), float("nan"), dtype=torch.half, device=DEV)
    vt[:, :, :, :Nk] = 0
    for h in range(heads):
        qb[:, :, h * Dp:h * Dp + dh] = q[:, h]
        kb[:, :, h * Dp:h * Dp + dh] = k[:, h]
        vt[:, h, :dh, :Nk] = v[:, h].transpose(1, 2)
    if perm:
        pos = torch.arange(Nk, device=DEV)
        swap = (((pos >> 2) ^ (pos >> 3)) & 1).bool()
        vtp = torch.empty_like(vt)
        vtp[..., torch.where(swap, pos ^ 12, pos)] = vt[..., pos]
        vt = vtp
    return qb, kb, vt, ldv


def run_masked(ctx, qb, kb, vt, ldv, heads, Nq, Nk, Dp, dh, rows, kcls, qcls, mrow, nrows_out, masked=True):
    o = torch.zeros(nrows_out, Nq, heads * dh, dtype=torch.half, device=DEV)
    rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV).contiguous()
    scale = dh ** -0.5
    if masked:
        mrow_t = torch.tensor(mrow, dtype=torch.int32, device=DEV)
        ctx.call("pnpi_op_attention_masked", ptr(qb), heads * Dp, 0, ptr(kb), heads * Dp, 0, ptr(vt), ldv, ptr(o), heads * dh, heads, Nq, Nk,
                 Dp, dh, scale, ptr(rows_t), len(rows), ptr(kcls), ptr(qcls), ptr(mrow_t))
    else:
        ctx.call("pnpi_op_attention", ptr(qb), heads * Dp, 0, ptr(kb), heads * Dp, 0, ptr(vt), ldv, ptr(o), heads * dh, heads, Nq, Nk,
                 Dp, dh, scale, ptr(rows_t), len(rows))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tag,perm", [("d40", 0), ("d40", 1), ("d80", 0), ("d160", 0), ("d16", 0)])
def test_masked_attention_kernel_against_the_reference(ctx, gold, tag, perm, case):
    """rows [src, tgt]: the target row's queries over the source row's K / V, one head; perm = the permuted V^T of the 4096-token sites"""
    g = gold
    q, k, v = (torch.from_numpy(g[tag + "_" + n].astype(np.float32)).half().to(DEV)[:, None] for n in "qkv")      # [2, 1, N, d]
    N, dh, Dp = q.shape[2], q.shape[3], DP[tag]
    sel = torch.from_numpy(g[tag + "_sel"]).to(DEV)
    kcls = torch.from_numpy(g["%s_%s_mask_s" % (tag, case)]).reshape(1, N).contiguous().to(DEV)
    qcls = torch.from_numpy(g["%s_%s_mask_t" % (tag, case)]).reshape(1, N).contiguous().to(DEV)
    qb, kb, vt, ldv = pack(q, k, v, Dp, perm=bool(perm))
    with ctx.tuning(op_attention_vt_perm=perm):
        o = run_masked(ctx, qb, kb, vt, ldv, 1, N, N, Dp, dh, [[1, 1, 0, 0]], kcls, qcls, [0], 2)
        plain = run_masked(ctx, qb, kb, vt, ldv, 1, N, N, Dp, dh, [[1, 1, 0, 0]], None, None, None, 2, masked=False) if case == "rect" else None
    assert torch.isfinite(o.float()).all()
    assert not o[0].any()                                        # only the listed output row is written
    ref_rows = torch.from_numpy(g["%s_%s_out" % (tag, case)]).to(DEV)
    full = one_pass(q[1, 0], k[0, 0], v[0, 0], kcls[0], qcls[0], dh ** -0.5)
    e_fix, e_full = rel_err(o[1][sel], ref_rows), rel_err(o[1], full)
    print(tag, perm, case, "rel vs fixture rows %.2e, vs the one-pass statement %.2e, max %.2e" % (e_fix, e_full, max_err(o[1], full)))
    assert e_fix < ATTN_BAR, e_fix
    assert e_full < ATTN_BAR, e_full
    if case == "empty_fg":                                       # foreground queries: no key of their class -> the mean of V
        fg = qcls[0].bool()
        assert max_err(o[1][fg], v[0, 0].float().mean(0).expand(int(fg.sum()), -1)) < 2e-3
    if plain is not None:                                        # the mask matters: far outside the bar
        assert max_err(o[1], plain[1]) >= 10 * ATTN_BAR, max_err(o[1], plain[1])
        assert rel_err(plain[1][sel], torch.from_numpy(g[tag + "_plain"]).to(DEV)) < ATTN_BAR


@pytest.mark.parametrize("Nq,Nk,dh,Dp", [(200, 200, 40, 64), (130, 77, 80, 96), (300, 1000, 16, 32)])
def test_masked_attention_ragged_sizes_heads_and_class_rows(ctx, Nq, Nk, dh, Dp):
    """two heads, two target rows with their own class rows, token counts that are no multiple of the 128-query / 64-key tiles (partial last
    tile, the byte-wise class load), class rows where whole key tiles hold one class only (tile skipping)"""
    g = torch.Generator().manual_seed(5)
    R, heads = 4, 2
    q, k, v = (torch.randn(R, heads, n, dh, generator=g).half().to(DEV) for n in (Nq, Nk, Nk))
    kcls = (torch.rand(2, Nk, generator=g) < 0.4).to(torch.uint8)
    kcls[0, :min(128, Nk // 2)] = 0                              # leading key tiles of one class
    kcls[1, Nk // 2:] = 1
    qcls = (torch.rand(2, Nq, generator=g) < 0.5).to(torch.uint8)
    qcls[1, :Nq // 2] = 1                                        # a whole query tile / wave of one class
    kcls, qcls = kcls.contiguous().to(DEV), qcls.contiguous().to(DEV)
    qb, kb, vt, ldv = pack(q, k, v, Dp)
    rows, mrow = [[1, 1, 0, 0], [3, 3, 2, 2]], [1, 0]
    o = run_masked(ctx, qb, kb, vt, ldv, heads, Nq, Nk, Dp, dh, rows, kcls, qcls, mrow, R)
    assert torch.isfinite(o.float()).all() and not o[0].any() and not o[2].any()
    for (orow, qrow, krow, vrow), mi in zip(rows, mrow):
        ref = torch.cat([one_pass(q[qrow, h], k[krow, h], v[vrow, h], kcls[mi], qcls[mi], dh ** -0.5) for h in range(heads)], dim=1)
        assert rel_err(o[orow], ref) < ATTN_BAR, (orow, rel_err(o[orow], ref))


@pytest.mark.parametrize("Nq,Nk,dh,Dp", [(200, 200, 40, 64), (130, 192, 80, 96), (64, 77, 160, 160)])
def test_unrestricted_masked_attention_equals_plain_attention_bit_for_bit(ctx, Nq, Nk, dh, Dp):
    """kcls = qcls = 1 restricts nothing: the masked kernel and attn_flash_kernel run the same shared tile body (attn.hip) on the same
    tiles, and the finite -1e30 start of the running maximum gives alpha = exp2(-huge) = 0 on O = 0, l = 0 exactly as -inf does.  Shapes:
    the prefetch instance with a ragged last key tile, three whole key tiles, and (77 keys) the plain side's non-prefetch instance."""
    g = torch.Generator().manual_seed(11)
    heads = 2
    q, k, v = (torch.randn(4, heads, n, dh, generator=g).half().to(DEV) for n in (Nq, Nk, Nk))
    qb, kb, vt, ldv = pack(q, k, v, Dp)
    kcls = torch.ones(1, Nk, dtype=torch.uint8, device=DEV)
    qcls = torch.ones(1, Nq, dtype=torch.uint8, device=DEV)
    rows = [[1, 1, 0, 0]]                                        # [tgt, tgt, src, src]
    masked = run_masked(ctx, qb, kb, vt, ldv, heads, Nq, Nk, Dp, dh, rows, kcls, qcls, [0], 4)
    plain = run_masked(ctx, qb, kb, vt, ldv, heads, Nq, Nk, Dp, dh, rows, None, None, None, 4, masked=False)
    assert plain[1].any() and torch.isfinite(plain.float()).all()
    assert torch.equal(masked, plain)


def test_masked_attention_refuses_what_it_cannot_run(ctx):
    z = torch.zeros(64, dtype=torch.half, device=DEV)
    b = torch.zeros(64, dtype=torch.uint8, device=DEV)
    r = torch.zeros(4, dtype=torch.int32, device=DEV)
    lib = ctx.lib
    args = lambda Nk, kc: (ctx.h, ptr(z), 64, 0, ptr(z), 64, 0, ptr(z), 8, ptr(z), 40, 1, 1, Nk, 64, 40, 0.1, ptr(r), 1, kc, ptr(b), ptr(r))   # noqa: E731
    assert lib.pnpi_op_attention_masked(*args(16384 + 64, ptr(b))) == _capi.PNPI_ESHAPE          # more keys than the class bits in LDS hold
    assert lib.pnpi_op_attention_masked(*args(8, None)) == _capi.PNPI_EINVAL


@pytest.mark.parametrize("src,dst", [(64, 32), (64, 16), (64, 8), (48, 16), (64, 64), (50, 16)])
def test_mask_resize_equals_interpolate_nearest(ctx, src, dst):
    g = torch.Generator().manual_seed(src * 100 + dst)
    m = (torch.rand(3, src, src, generator=g) < 0.5).to(torch.uint8)
    m[0, 1::2, 1::2] = 1
    m[1, ::2, ::2] = 0
    ref = F.interpolate(m[:, None].float(), (dst, dst))[:, 0].to(torch.uint8)
    out = torch.full((3, dst, dst), 7, dtype=torch.uint8, device=DEV)
    md = m.contiguous().to(DEV)
    ctx.call("pnpi_op_masa_mask_level", ptr(md), 3, src, src, dst, dst, ptr(out))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)


# ------------------------------------------------------------------------------------------------ whole edits
@pytest.fixture(scope="module")
def e2e():
    from pnpinversion_amd.masactrl.diffuser_utils import MasaCtrlPipeline
    g = np.load(os.path.join(GOLD, "e2e_masactrl_mask.npz"))
    cfg = SMALL64
    pipe = MasaCtrlPipeline(cfg, max_unet_rows=12, max_vae_images=2, text_encoder=SyntheticTextEncoder(cfg.cross_dim, seed=7))
    pipe.load_state_dict(weights.unet_state_dict(cfg, int(g["weight_seed"])), weights.vae_state_dict(cfg, int(g["weight_seed"])))
    steps = int(g["steps"])
    pipe.scheduler.set_timesteps(steps)
    tgt = str(g["tgt"])
    ctx4 = torch.cat([pipe._embed(["", ""]), pipe._embed(["", tgt])])                 # [unc_src, unc_tgt, cond_src, cond_tgt]
    st = dict(pipe=pipe, g=g, steps=steps, tgt=tgt, ctx4=ctx4, ts=pipe.scheduler.timesteps.numpy(), x_t=torch.from_numpy(g["x_t"]).to(DEV),
              start_step=int(g["start_step"]), start_layer=int(g["start_layer"]))
    yield st
    pipe.engine.close()


def editors(st, im):
    from pnpinversion_amd.masactrl.masactrl import MutualSelfAttentionControl, MutualSelfAttentionControlMask
    g = st["g"]
    kw = dict(start_step=st["start_step"], start_layer=st["start_layer"], total_steps=st["steps"])
    ms, mt = torch.from_numpy(g["mask_s"][im]).float(), torch.from_numpy(g["mask_t"][im]).float()
    return MutualSelfAttentionControl(**kw), MutualSelfAttentionControlMask(mask_s=ms, mask_t=mt, **kw)


def loop(st, tables, nimg=1):
    eng = st["pipe"].engine
    x = st["x_t"].reshape(1, *st["x_t"].shape[-3:]).expand(nimg, -1, -1, -1)
    return eng.edit_loop(x, st["ctx4"][None].expand(nimg, -1, -1, -1), None, tables, st["ts"], 7.5).cpu()        # [nimg, 2, 4, 64, 64]


def test_level_masks_of_the_context_follow_interpolate_nearest(e2e):
    g, eng = e2e["g"], e2e["pipe"].engine
    eng.masa_set_masks(g["mask_s"], g["mask_t"])
    try:
        for level in range(3):
            side = 64 >> level
            s, t = eng.masa_level_masks(level)
            for got, full in ((s, g["mask_s"]), (t, g["mask_t"])):
                ref = F.interpolate(torch.from_numpy(full)[:, None].float(), (side, side))[:, 0].to(torch.uint8)
                assert torch.equal(torch.from_numpy(got), ref), level
        s32, _ = eng.masa_level_masks(1)
        assert g["mask_s"][1].sum() == 1 and s32[1].sum() == 0          # image 1's one-pixel foreground is gone below 64 x 64
    finally:
        eng.masa_set_masks()


@pytest.mark.parametrize("im", [0, 1])
def test_edit_against_the_references_per_step_latents(e2e, im):
    """MasaCtrlPipeline.__call__ (pnpi_edit_loop) for the final latents, and the same steps one UNet call at a time (pnpi_unet_forward +
    the DDIM step of models/masactrl/diffuser_utils.py:39-57 in torch) for the latent after every step"""
    from pnpinversion_amd.masactrl.masactrl_utils import regiter_attention_editor_diffusers
    st, pipe = e2e, e2e["pipe"]
    eng, g, steps = pipe.engine, e2e["g"], e2e["steps"]
    ref = torch.from_numpy(g["latents_steps_%d" % im])                               # [steps, 2, 4, 64, 64]
    plain_ed, mask_ed = editors(st, im)
    got = {}
    orig = pipe.latent2image
    pipe.latent2image = lambda latents, return_type="np": (got.__setitem__("lat", latents.detach().clone()), orig(latents, return_type=return_type))[1]
    try:
        regiter_attention_editor_diffusers(pipe, mask_ed)
        pipe(["", st["tgt"]], latents=st["x_t"].expand(2, -1, -1, -1), num_inference_steps=steps, guidance_scale=7.5)
        masked = got["lat"].cpu()
        # one UNet call per step, masks still registered
        ac, fa = torch.from_numpy(eng.ac), eng.final_alpha
        lat = st["x_t"].expand(2, -1, -1, -1).clone()
        tables = mask_ed.tables()
        for i, t in enumerate(st["ts"]):
            eps = eng.unet(torch.cat([lat, lat]), int(t), st["ctx4"], rows_per_image=4, ctrls=[tables], cur_step=i)
            e = eps[:2] + 7.5 * (eps[2:] - eps[:2])
            prev = int(t) - 1000 // steps
            a_t, a_p = float(ac[int(t)]), float(ac[prev]) if prev > 0 else fa
            lat = a_p ** 0.5 * ((lat - (1 - a_t) ** 0.5 * e) / a_t ** 0.5) + (1 - a_p) ** 0.5 * e
            err = ((lat.cpu() - ref[i]).norm() / ref[i].norm()).item()
            print("image %d step %d rel %.2e" % (im, i, err))
            assert err < E2E_BAR, (i, err)
        regiter_attention_editor_diffusers(pipe, plain_ed)                           # un-registering the mask editor clears the masks
        pipe(["", st["tgt"]], latents=st["x_t"].expand(2, -1, -1, -1), num_inference_steps=steps, guidance_scale=7.5)
        plain = got["lat"].cpu()
    finally:
        pipe.latent2image = orig
        eng.masa_set_masks()
    err = ((masked - ref[-1]).norm() / ref[-1].norm()).item()
    print("image %d final rel %.2e, |masked - plain| on the target row %.3f" % (im, err, (masked[1] - plain[1]).abs().mean().item()))
    assert err < E2E_BAR, err
    assert torch.equal(masked[0], plain[0])                                          # source rows never see the masks
    assert (masked[1] - plain[1]).abs().mean().item() > 1e-3                         # the target row does


def test_cleared_masks_reproduce_plain_masactrl_bit_for_bit(e2e):
    st, eng = e2e, e2e["pipe"].engine
    plain_ed, mask_ed = editors(st, 0)
    plain = loop(st, [plain_ed.tables()])
    eng.masa_set_masks(mask_ed.tables().mask_s, mask_ed.tables().mask_t)
    masked = loop(st, [mask_ed.tables()])
    eng.masa_set_masks()
    cleared = loop(st, [mask_ed.tables()])
    assert torch.equal(cleared, plain)
    assert not torch.equal(masked, plain) and torch.equal(masked[:, 0], plain[:, 0])


def test_two_images_with_their_own_masks_equal_the_single_image_runs(e2e):
    """the launches of a two-image batch have other row counts than a single image's (other GEMM tiles): equal at the end-to-end bar, not
    bit for bit; each image follows ITS masks (the two target rows differ by far more)"""
    st, eng, g = e2e, e2e["pipe"].engine, e2e["g"]
    single = []
    try:
        for im in range(2):
            _, ed = editors(st, im)
            eng.masa_set_masks(ed.tables().mask_s, ed.tables().mask_t)
            single.append(loop(st, [ed.tables()])[0])
        eng.masa_set_masks(g["mask_s"], g["mask_t"])
        both = loop(st, [ed.tables(), ed.tables()], nimg=2)
    finally:
        eng.masa_set_masks()
    for im in range(2):
        err = ((both[im] - single[im]).norm() / single[im].norm()).item()
        ref = torch.from_numpy(g["latents_steps_%d" % im][-1])
        print("image %d: batch vs single rel %.2e, batch vs reference %.2e" % (im, err, ((both[im] - ref).norm() / ref.norm()).item()))
        assert err < E2E_BAR and ((both[im] - ref).norm() / ref.norm()).item() < E2E_BAR
    swapped = ((both[0, 1] - single[1][1]).norm() / single[1][1].norm()).item()
    assert swapped > 5 * max(((both[im] - single[im]).norm() / single[im].norm()).item() for im in range(2))


def test_refusals_launch_nothing(e2e):
    st, eng = e2e, e2e["pipe"].engine
    lib, h = eng.lib, eng.h
    _, ed = editors(st, 0)
    ok = np.ascontiguousarray(ed.tables().mask_s)
    bad = ok.copy()
    bad[0, 3, 3] = 2
    p = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    eng.reset_counters()
    before = eng.counters()
    assert lib.pnpi_masa_set_masks(h, p(bad), p(ok), 1, 64, 64) == _capi.PNPI_EINVAL
    assert b"binary" in lib.pnpi_last_error(h)
    assert lib.pnpi_masa_set_masks(h, p(ok), None, 1, 64, 64) == _capi.PNPI_EINVAL
    assert b"together" in lib.pnpi_last_error(h)
    assert lib.pnpi_masa_set_masks(h, p(ok), p(ok), 0, 64, 64) == _capi.PNPI_EINVAL
    assert lib.pnpi_masa_set_masks(h, p(ok), p(ok), 4, 64, 64) == _capi.PNPI_EINVAL          # 4 images > max_unet_rows / 4
    # masks for two images, a loop over one
    two = np.ascontiguousarray(np.concatenate([ok, ok]))
    eng.masa_set_masks(two, two)
    try:
        with pytest.raises(_capi.PnpiError, match="another number of images") as ei:
            loop(st, [ed.tables()])
        assert ei.value.status == _capi.PNPI_EINVAL
        with pytest.raises(_capi.PnpiError, match="another number of images"):
            eng.direct_edit(st["x_t"].reshape(1, 1, 4, 64, 64).expand(st["steps"] + 1, -1, -1, -1, -1), st["ctx4"][None], [[ed.tables()]],
                            st["ts"], 7.5)
    finally:
        eng.masa_set_masks()
    assert eng.counters() == before                                                          # no UNet forward ran
