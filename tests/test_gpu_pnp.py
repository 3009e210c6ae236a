"""Plug-and-Play editing on the device (run_editing_pnp.py): the step kernel, the self-attention row table {r, src, src, r} at every
site size, one hooked forward and the whole loops against the reference's own hook functions (fixtures of tools/make_golden_pnp.py), the
dead work an injecting forward does not launch, batching and the refusals.

Bars (existing ones): one forward 4e-3 rel-L2 (tests/test_gpu_model.py), loops 1.5e-2 (tests/test_gpu_loops.py), op-level attention 3e-3,
batching 3e-2 (tests/test_gpu_loops.py::test_batched_images_match_single_image_calls).

Measured on an MI355X (rel-L2): see DESIGN.md section 7e."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import Ctx, ptr, rel_err  # noqa: E402
from pnpinversion_amd import _capi, weights  # noqa: E402
from pnpinversion_amd.config import SMALL64, TINY16  # noqa: E402
from pnpinversion_amd.engine import NativeEngine  # noqa: E402
from pnpinversion_amd.p2p.scheduler_dev import DDIMSchedulerDev  # noqa: E402
from pnpinversion_amd.pnp import source_list  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
FWD_BAR, LOOP_BAR, ATTN_BAR, BATCH_BAR = 4e-3, 1.5e-2, 3e-3, 3e-2


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def sd15_scheduler(engine, nsteps):
    s = DDIMSchedulerDev(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False,
                         steps_offset=1)
    s.bind(engine)
    s.set_timesteps(nsteps)
    return s


def make_engine(cfg, seed, max_rows):
    eng = NativeEngine(cfg, max_unet_rows=max_rows, max_vae_images=1)
    eng.load_state_dict(weights.unet_state_dict(cfg, seed), weights.vae_state_dict(cfg, seed))
    n, names = eng.missing_weights()
    assert n == 0, names[:10]
    return eng


@pytest.fixture(scope="module")
def tiny():
    eng = make_engine(TINY16, 1, 6)           # the weight seed of pnp_unet_tiny.npz
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def small():
    eng = make_engine(SMALL64, 2, 6)          # the weight seed of e2e_pnp.npz
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------------------- 1: the step kernel
@pytest.mark.parametrize("t", [501, 1])
def test_pnp_step_is_bit_exact(tiny, t):
    """pnpi_pnp_step against eager fp32 PyTorch in the reference's operation order (denoise_step :364-365, DDIMScheduler.step at eta 0):
    two images, a middle timestep and the last one (prev_t < 0 -> final_alpha_cumprod)"""
    s = sd15_scheduler(tiny, 50)
    g = torch.Generator().manual_seed(3)
    eps = torch.randn(2, 3, 4, 16, 16, generator=g)
    x = torch.randn(2, 4, 16, 16, generator=g)
    gs, ratio = 7.5, s.step_ratio
    got = tiny.pnp_step(eps, x, t, ratio, gs).cpu()
    eu, ec = eps[:, 1], eps[:, 2]
    noise_pred = eu + gs * (ec - eu)
    prev_t = t - ratio
    a_t = s.alphas_cumprod[t]
    a_p = s.alphas_cumprod[prev_t] if prev_t >= 0 else s.final_alpha_cumprod
    assert (prev_t < 0) == (t == 1)
    beta_t = 1 - a_t
    pred_x0 = (x - beta_t ** 0.5 * noise_pred) / a_t ** 0.5
    direction = (1 - a_p - 0.0 ** 2) ** 0.5 * noise_pred
    want = a_p ** 0.5 * pred_x0 + direction
    assert torch.equal(got, want), (got - want).abs().max().item()
    assert not torch.equal(got[0], got[1])


# ---------------------------------------------------------------------------------------------- 2: the row table at every site size
def pack(q, k, v, Dp, perm=False, aug=False):
    """q / k / v [rows, heads, N, dh] fp16 -> head-padded Q / K rows and V^T (NaN pads beyond the keys), optionally in the permuted key order
    and with the augmented column (K column dh and V^T row dh hold 1.0)"""
    R, heads, N, dh = q.shape
    hd = heads * Dp
    qb = torch.zeros(R, N, hd, dtype=torch.half, device=DEV)
    kb = torch.zeros(R, N, hd, dtype=torch.half, device=DEV)
    ldv = (N + 7) // 8 * 8
    vt = torch.full((R, heads, Dp, ldv), float("nan"), dtype=torch.half, device=DEV)
    vt[:, :, :, :N] = 0
    for h in range(heads):
        qb[:, :, h * Dp:h * Dp + dh] = q[:, h]
        kb[:, :, h * Dp:h * Dp + dh] = k[:, h]
        vt[:, h, :dh, :N] = v[:, h].transpose(1, 2)
        if aug:
            kb[:, :, h * Dp + dh] = 1.0
            vt[:, h, dh, :N] = 1.0
    if perm:
        pos = torch.arange(N, device=DEV)
        swap = (((pos >> 2) ^ (pos >> 3)) & 1).bool()
        vtp = vt.clone()
        vtp[..., torch.where(swap, pos ^ 12, pos)] = vt[..., pos]
        vt = vtp
    return qb, kb, vt, ldv


ATTN_CASES = [(4096, 40, 64, 0, 0), (4096, 40, 64, 1, 0), (4096, 40, 64, 1, 1), (4096, 40, 64, 0, 1), (1024, 80, 96, 0, 0), (256, 160, 160, 0, 0)]


@pytest.fixture(scope="module")
def kctx():
    c = Ctx()
    yield c
    c.close()


@pytest.mark.parametrize("N,dh,Dp,perm,aug", ATTN_CASES)
def test_attention_row_table_source_q_k_own_v(kctx, N, dh, Dp, perm, aug):
    """rows {0,0,0,0}, {1,0,0,1}, {2,0,0,2}: out_r = softmax(q_0 k_0^T scale) v_r.  At N = 4096 the 64-wide LDS-DMA kernel runs with
    q_row != out_row, in plain and permuted V^T and with the augmented column."""
    ctx = kctx
    heads = 2
    g = torch.Generator().manual_seed(N + dh + perm + 2 * aug)
    q, k, v = (torch.randn(3, heads, N, dh, generator=g).half().to(DEV) for _ in range(3))
    qb, kb, vt, ldv = pack(q, k, v, Dp, perm=bool(perm), aug=bool(aug))
    scale = dh ** -0.5

    def run(rows):
        o = torch.zeros(3, N, heads * dh, dtype=torch.half, device=DEV)
        rows_t = torch.tensor(rows, dtype=torch.int32, device=DEV).contiguous()
        with ctx.tuning(op_attention_aug=aug, op_attention_vt_perm=perm):
            ctx.call("pnpi_op_attention", ptr(qb), heads * Dp, 0, ptr(kb), heads * Dp, 0, ptr(vt), ldv, ptr(o), heads * dh, heads, N, N, Dp, dh,
                     scale, ptr(rows_t), len(rows))
            torch.cuda.synchronize()
        return o.view(3, N, heads, dh).permute(0, 2, 1, 3).float()

    got = run([[0, 0, 0, 0], [1, 0, 0, 1], [2, 0, 0, 2]])
    plain = run([[r, r, r, r] for r in range(3)])
    probs = torch.softmax(q[0].float() @ k[0].float().transpose(1, 2) * scale, dim=-1)          # [heads, N, N]
    assert torch.isfinite(got).all()
    for r in range(3):
        e = rel_err(got[r], probs @ v[r].float())
        print("N %d d %d perm %d aug %d row %d rel-L2 %.2e" % (N, dh, perm, aug, r, e))
        assert e < ATTN_BAR, (r, e)
    assert rel_err(plain[0], got[0]) < ATTN_BAR
    for r in (1, 2):          # the redirection matters: far outside the bar
        assert rel_err(got[r], plain[r]) > 10 * ATTN_BAR, rel_err(got[r], plain[r])


# ---------------------------------------------------------------------------------------------- 3: one forward against the hooked UNet
@pytest.fixture(scope="module")
def unet_gold():
    return np.load(os.path.join(GOLD, "pnp_unet_tiny.npz"))


STATES = {"none": (0, 0), "conv": (1, 0), "qk": (0, 1), "both": (1, 1)}


@pytest.mark.parametrize("state", list(STATES))
def test_one_forward_against_the_references_hooked_unet(tiny, unet_gold, state):
    g = unet_gold
    sd15_scheduler(tiny, 50)
    desc = tiny.pnp_desc(50)
    lat = torch.from_numpy(g["latents"])[None]
    ctx = torch.from_numpy(g["context"])[None]
    conv_on, qk_on = STATES[state]
    got = tiny.unet_pnp(lat, int(g["t"]), ctx, desc, conv_on, qk_on)[0]
    want = torch.from_numpy(g["eps_" + state])
    base = torch.from_numpy(g["eps_none"])
    e = rel(got, want)
    print("forward %-4s rel-L2 %.2e (injected vs uninjected reference: %.3f)" % (state, e, rel(want[1:], base[1:])))
    assert torch.isfinite(got).all()
    assert e < FWD_BAR, e
    assert rel(got[1:], want[1:]) < FWD_BAR
    if state != "none":       # the fixture tool asserts >= 10 x the bar: a forward that ignores the injection state cannot pass
        assert rel(want[1:], base[1:]) >= 10 * FWD_BAR


# ---------------------------------------------------------------------------------------------- 4: dead work is not launched
@pytest.mark.parametrize("nimg", [1, 2])
def test_injecting_forward_skips_the_main_branch_of_two_rows_per_image(tiny, nimg):
    cfg = TINY16
    sd15_scheduler(tiny, 50)
    desc = tiny.pnp_desc(50)
    g = torch.Generator().manual_seed(17)
    lat = torch.randn(nimg, 3, 4, 16, 16, generator=g)
    ctx = weights.synth_context(cfg, 3 * nimg, seed=4).reshape(nimg, 3, cfg.ctx_len, cfg.cross_dim)

    def flops(conv_on):
        tiny.reset_counters()
        out = tiny.unet_pnp(lat, 301, ctx, desc, conv_on, 0)
        torch.cuda.synchronize()
        return tiny.counters()["executed_gemm_flops"], out

    plain, out_plain = flops(0)
    inj, out_inj = flops(1)
    # the site: decoder ResNet desc.conv_site = up block i, layer j; its maps are sample_size >> (n_blocks - 1 - i) wide, its input is the
    # previous level's channels concatenated with the skip's, 3 x 3 convolutions conv1 (cin -> cout) and conv2 (cout -> cout)
    boc, n, lpb = list(cfg.block_out_channels), len(cfg.block_out_channels), cfg.layers_per_block
    i, j = divmod(desc.conv_site, lpb + 1)
    assert (i, j) == (1, 1)
    level = n - 1 - i
    side = cfg.sample_size >> level
    cout = boc[level]
    skip_ch = [boc[level]] * lpb + [boc[level - 1]]           # the skips an up block pops: its level's lpb outputs, then the level above's downsample input
    cin = cout + skip_ch[j]                                   # j >= 1: the block's own previous output (cout) + skip
    rows_skipped = 2 * nimg
    want = 2.0 * rows_skipped * side * side * cout * 9 * (cin + cout)
    print("executed_gemm_flops plain %.0f injecting %.0f difference %.0f expected %.0f" % (plain, inj, plain - inj, want))
    assert inj < plain and plain - inj == want
    assert torch.equal(out_plain[:, 0], out_inj[:, 0]) or rel(out_inj[:, 0], out_plain[:, 0]) < FWD_BAR      # the source row's result is the same computation


# ---------------------------------------------------------------------------------------------- 5: the loops on SMALL64
@pytest.fixture(scope="module")
def e2e():
    g = dict(np.load(os.path.join(GOLD, "e2e_pnp.npz")))
    g.update(np.load(os.path.join(GOLD, "e2e_pnp_edit.npz")))
    cfg = SMALL64
    gen = torch.Generator().manual_seed(int(g["z0_seed"]))
    g["z0"] = 0.8 * torch.randn(2, cfg.in_channels, cfg.sample_size, cfg.sample_size, generator=gen)
    g["ctx"] = weights.synth_context(cfg, 5, seed=int(g["context_seed"]))       # source prompt, "", negative, target, second target
    assert np.array_equal(g["z0"][0].numpy(), g["inverted_x"][0])
    return g


def loop_desc(eng, g):
    return eng.pnp_desc(int(g["steps"]), int(g["conv_steps"]), int(g["qk_steps"]))


def composed(eng, src, x, ctx3, desc, ts, ratio, gs, plain=False):
    """the loop from its level-1 calls -> the latent after every step"""
    out = []
    for i, t in enumerate(ts):
        rows = torch.stack([src[i].to(x.device), x, x], 1)                   # [nimg, 3, C, h, w]
        if plain:
            eps = eng.unet(rows.flatten(0, 1), t, ctx3.flatten(0, 1)).view_as(rows)
        else:
            eps = eng.unet_pnp(rows, t, ctx3, desc, i < desc.conv_steps, i < desc.qk_steps)
        x = eng.pnp_step(eps, x, t, ratio, gs)
        out.append(x)
    return out


def test_inversion_and_reconstruction_lists(small, e2e):
    """Preprocess.ddim_inversion / ddim_sample on the steps_offset = 1 timesteps: 7 and 6 latents"""
    from pnpinversion_amd.pnp import Preprocess
    g = e2e
    pre = Preprocess.__new__(Preprocess)
    pre.engine, pre.device = small, small.device
    pre.scheduler = sd15_scheduler(small, int(g["steps"]))
    assert [int(t) for t in pre.scheduler.timesteps] == [int(t) for t in g["timesteps"]]
    cond = g["ctx"][0:1].to(DEV)
    inv = pre.ddim_inversion(cond, g["z0"][0:1].to(DEV))
    rec = pre.ddim_sample(inv[-1], cond)
    assert len(inv) == int(g["steps"]) + 1 and len(rec) == int(g["steps"])
    ei = [rel(a, torch.from_numpy(b)) for a, b in zip(inv, g["inverted_x"])]
    er = [rel(a[0], torch.from_numpy(b)) for a, b in zip(rec, g["latent_reconstruction"])]
    print("inversion rel-L2 per level:", ["%.2e" % v for v in ei], "reconstruction:", ["%.2e" % v for v in er])
    assert max(ei) < LOOP_BAR and max(er) < LOOP_BAR


@pytest.mark.parametrize("method", ["directinversion+pnp", "ddim+pnp"])
def test_edit_loops_against_the_reference(small, e2e, method):
    """conv on steps 0 .. 3, q/k on steps 0 .. 2: every block of the default q/k mask injects, the three 4096-token sites included.  The
    source lists are the reference's (7 inversion latents / 6 reversed reconstruction latents) in the reference's indexing; the latent after
    every step against its fp32 run; the device-resident loop equals its level-1 composition bit for bit."""
    g = e2e
    s = sd15_scheduler(small, int(g["steps"]))
    ts, gs = [int(t) for t in g["timesteps"]], float(g["guidance_scale"])
    desc = loop_desc(small, g)
    assert (desc.conv_steps, desc.qk_steps) == (4, 3) and desc.qk_block_mask == 0xFF00
    noisy = [torch.from_numpy(v)[None] for v in g["inverted_x"]] if method == "directinversion+pnp" else \
        [torch.from_numpy(v)[None] for v in g["latent_reconstruction"][::-1].copy()]
    assert len(noisy) == (7 if method == "directinversion+pnp" else 6)
    src, start = source_list(noisy, len(ts))
    ctx3 = g["ctx"][1:4][None]
    want = torch.from_numpy(g[method + "/latents_steps"])
    x0 = start.to(DEV)
    steps = composed(small, src, x0, ctx3, desc, ts, s.step_ratio, gs)
    errs = [rel(a[0], b) for a, b in zip(steps, want)]
    print(method, "rel-L2 after every step:", ["%.2e" % v for v in errs])
    assert max(errs) < LOOP_BAR, errs
    small.reset_counters()
    loop = small.pnp_edit(torch.stack(src), start, ctx3, desc, ts, gs)
    c = small.counters()
    assert c["unet_calls"] == len(ts) and c["unet_sample_forwards"] == 3 * len(ts) and c["text_kv_rows"] == 3      # text K / V projected once
    assert torch.equal(loop, steps[-1]), rel(loop, steps[-1])


def test_loop_without_injection_equals_the_plain_forward_loop(small, e2e):
    g = e2e
    s = sd15_scheduler(small, int(g["steps"]))
    ts, gs = [int(t) for t in g["timesteps"]], float(g["guidance_scale"])
    desc = small.pnp_desc(len(ts), 0, 0)
    noisy = [torch.from_numpy(v)[None] for v in g["inverted_x"]]
    src, start = source_list(noisy, len(ts))
    ctx3 = g["ctx"][1:4][None]
    loop = small.pnp_edit(torch.stack(src), start, ctx3, desc, ts, gs)
    plain = composed(small, src, start.to(DEV), ctx3.to(DEV), desc, ts, s.step_ratio, gs, plain=True)[-1]
    assert torch.equal(loop, plain), rel(loop, plain)
    injected = torch.from_numpy(g["directinversion+pnp/latents_steps"][-1])
    assert rel(loop[0], injected) > 10 * LOOP_BAR          # and the injection is what the fixture's result rests on


# ---------------------------------------------------------------------------------------------- 6: batching
def test_two_images_in_one_call(small, e2e):
    g = e2e
    sd15_scheduler(small, int(g["steps"]))
    ts, gs = [int(t) for t in g["timesteps"]], float(g["guidance_scale"])
    desc = loop_desc(small, g)
    ctx = g["ctx"]
    inv = small.ddim_invert(g["z0"], torch.stack([ctx[0], ctx[0]]), ts)                  # [7, 2, 4, 64, 64]
    src = torch.stack([inv[len(ts) - i] for i in range(len(ts))])                         # step i reads level n - i
    start = inv[-1]
    ctx3 = torch.stack([ctx[1:4], torch.stack([ctx[1], ctx[2], ctx[4]])])                # the second image edits towards another prompt
    both = small.pnp_edit(src, start, ctx3, desc, ts, gs)
    single = [small.pnp_edit(src[:, i:i + 1], start[i:i + 1], ctx3[i:i + 1], desc, ts, gs)[0] for i in range(2)]
    d = [rel(both[i], single[i]) for i in range(2)]
    wrong = [rel(both[i], single[1 - i]) for i in range(2)]
    print("batched vs single:", d, "against the other image's:", wrong)
    assert max(d) < BATCH_BAR and min(wrong) > BATCH_BAR


# ---------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_launch_nothing(tiny):
    sd15_scheduler(tiny, 4)
    cfg = TINY16
    E = (cfg.in_channels, cfg.sample_size, cfg.sample_size)
    ts = [751, 501, 251, 1]
    desc = tiny.pnp_desc(4)

    def args(nimg):
        return (torch.zeros(4, nimg, *E), torch.zeros(nimg, *E), torch.zeros(nimg, 3, cfg.ctx_len, cfg.cross_dim))

    tiny.reset_counters()
    with pytest.raises(_capi.PnpiError, match="max_unet_rows"):               # 9 rows on a 6-row context
        tiny.pnp_edit(*args(3), desc, ts, 7.5)
    with pytest.raises(_capi.PnpiError, match="max_unet_rows"):
        tiny.unet_pnp(torch.zeros(3, 3, *E), 1, torch.zeros(3, 3, cfg.ctx_len, cfg.cross_dim), desc, 1, 1)
    bad = _capi.PnpDesc.make(3, 2, desc.conv_site, desc.qk_block_mask)
    bad.struct_size = 16
    with pytest.raises(_capi.PnpiError, match="struct_size"):
        tiny.pnp_edit(*args(1), bad, ts, 7.5)
    with pytest.raises(_capi.PnpiError, match="struct_size"):
        tiny.unet_pnp(torch.zeros(1, 3, *E), 1, torch.zeros(1, 3, cfg.ctx_len, cfg.cross_dim), bad, 1, 1)
    src, x, ctx = (t.to(DEV) for t in args(1))
    out = torch.empty_like(x)
    tsa = np.asarray(ts, dtype=np.int32)
    with pytest.raises(_capi.PnpiError, match="nsteps"):                      # nsteps 0
        tiny._call("pnpi_pnp_edit", ptr(src), ptr(x), 1, ptr(ctx), C.byref(desc), 0, tsa.ctypes.data_as(C.POINTER(C.c_int)), 7.5, ptr(out))
    site = _capi.PnpDesc.make(3, 2, 99, desc.qk_block_mask)
    with pytest.raises(_capi.PnpiError, match="conv_site"):
        tiny.pnp_edit(*args(1), site, ts, 7.5)
    torch.cuda.synchronize()
    c = tiny.counters()
    assert c["unet_calls"] == 0 and c["unet_sample_forwards"] == 0 and c["text_kv_rows"] == 0 and c["executed_gemm_flops"] == 0
    # and the context still runs a forward afterwards
    assert torch.isfinite(tiny.unet_pnp(torch.zeros(1, 3, *E), 1, torch.zeros(1, 3, cfg.ctx_len, cfg.cross_dim), desc, 1, 1)).all()
