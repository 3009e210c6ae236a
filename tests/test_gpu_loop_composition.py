"""Bit-exact pins of the level-2 loops (whole inversion / editing loops in one C call) against the SAME steps driven one by one through the
level-1 entry points: text_kv_precompute, unet(..., None), cfg_ddim_prev, ddim_next_step, ef_sample_xts, ef_noise_map, ef_reverse_step.
A loop and its composition launch the same kernels with the same row counts on the same values, so every output is compared with
torch.equal -- what a loop gathers, interleaves and indexes is its own, which is what these tests hold still.  TINY16, 3 steps, up to
8 rows per launch, and TWO images with different contexts and latents wherever the loop takes several: a wrong row map, latent
expansion or [uncond, cond] interleave cannot pass.  (tests/test_gpu_loops.py::test_inversion_guidance_loop_step_by_step_exact pins
pnpi_edit_loop with proximal / inversion guidance the same way.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import p2p_oracle as po  # noqa: E402   (scheduler tables only)
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import TINY16  # noqa: E402
from pnpinversion_amd.engine import NativeEngine  # noqa: E402

STEPS, GS = 3, 7.5
RATIO = 1000 // STEPS
TS = po.make_timesteps(STEPS)           # descending: the denoising order; the DDIM inversions walk it backwards


@pytest.fixture(scope="module")
def eng():
    e = NativeEngine(TINY16, max_unet_rows=8, max_vae_images=1)
    e.load_state_dict(weights.unet_state_dict(TINY16, 5), weights.vae_state_dict(TINY16, 5))
    ac = po.alphas_cumprod()
    e.set_scheduler(ac.numpy(), float(ac[0]))
    yield e
    e.close()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def lat(seed, *lead):
    return randn(seed, *lead, 4, TINY16.sample_size, TINY16.sample_size)


def context4(eng, nimg, seed):
    """[nimg, 4, 77, D] rows [unc_src, unc_tgt, cond_src, cond_tgt], different for every image"""
    return weights.synth_context(eng.cfg, 4 * nimg, seed=seed).reshape(nimg, 4, TINY16.ctx_len, TINY16.cross_dim)


def rows4(cur):
    """latents [nimg, 2, ...] -> the rows [src, tgt, src, tgt] per image of a 4-rows-per-image launch"""
    return torch.cat([torch.cat([c, c]) for c in cur])


def cfg_combine(eps_u, eps_c, gs):
    """eps_u + gs * (eps_c - eps_u), every operation rounded on its own as the step kernels do (fp32 on the host)"""
    eps_u, eps_c = eps_u.cpu(), eps_c.cpu()
    return eps_u + gs * (eps_c - eps_u)


def test_ddim_invert_cfg_equals_level1_steps(eng):
    z0, ctx = lat(31, 2), context4(eng, 2, 32)
    cu, cc = ctx[:, 0], ctx[:, 2]
    got = eng.ddim_invert_cfg(z0, cu, cc, TS, GS).cpu()
    eng.text_kv_precompute(torch.stack([cu, cc], 1).flatten(0, 1))           # rows [img][uncond, cond]
    want = [z0]
    for t in (int(v) for v in TS[::-1]):
        cur = want[-1]
        eps = eng.unet(cur.repeat_interleave(2, 0), t, None).unflatten(0, (2, 2))
        # the loop's fused CFG + next_step kernel is the CFG combine and then the DDIM move of pnpi_ddim_next_step
        want.append(eng.ddim_next_step(cfg_combine(eps[:, 0], eps[:, 1], GS), t, RATIO, cur).cpu())
    assert torch.equal(got, torch.stack(want)), (got - torch.stack(want)).abs().amax(dim=(1, 2, 3, 4))


def offset_steps(eng, x_stars, ctx, rows_of, after_offset_step):
    """The offset pass of direct inversion for one step after the other through level 1.  x_stars [STEPS + 1, nimg, ...];
    rows_of(cur) -> the latent rows of the launch, cur [nimg, 2, ...] = the offset pass's latents; after_offset_step(i, t, eps, loss)
    sees every step's whole prediction.  -> noise_loss [STEPS, nimg, 2, ...]"""
    nimg = x_stars.shape[1]
    cur = x_stars[-1][:, None].expand(-1, 2, -1, -1, -1).clone()
    eng.text_kv_precompute(ctx)
    nl = []
    for i, t in enumerate(int(v) for v in TS):
        eps = eng.unet(rows_of(cur), t, None)
        prev = torch.stack([eng.cfg_ddim_prev(eps[4 * im:4 * im + 4], cur[im], t, RATIO, GS).cpu() for im in range(nimg)])
        loss = x_stars[STEPS - i - 1][:, None] - prev          # (x*_{t-1} - prev) * 1.0
        cur = prev + loss
        nl.append(loss)
        after_offset_step(i, t, eps, loss)
    return torch.stack(nl)


def test_offset_calculate_equals_level1_steps(eng):
    x_stars, ctx = lat(41, STEPS + 1, 2), context4(eng, 2, 42)
    got = eng.offset_calculate(x_stars, ctx, TS, GS).cpu()
    want = offset_steps(eng, x_stars, ctx.flatten(0, 1), rows4, lambda *a: None)
    # every step's offset is equal, and with it the latent each later step started from (cur = prev + loss)
    assert torch.equal(got, want), (got - want).abs().amax(dim=(1, 2, 3, 4, 5))


@pytest.mark.parametrize("first_only", [False, True])
def test_edit_loop_uncond_steps_equals_level1_steps(eng, first_only):
    zT, ctx = lat(51, 2), context4(eng, 2, 52)
    us = randn(53, STEPS, 2, TINY16.ctx_len, TINY16.cross_dim)            # distinct embeddings for every step and image
    before = eng.counters()["text_kv_rows"]
    got = eng.edit_loop_uncond_steps(zT, ctx, us, None, TS, GS, first_only=first_only).cpu()
    assert eng.counters()["text_kv_rows"] - before == STEPS * 8             # the text K / V are projected again at every step
    cur = zT[:, None].expand(-1, 2, -1, -1, -1).clone()
    ctx_step = ctx.clone()
    for i, t in enumerate(int(v) for v in TS):
        ctx_step[:, 0] = us[i]
        if not first_only:
            ctx_step[:, 1] = us[i]
        eng.text_kv_precompute(ctx_step.flatten(0, 1))
        eps = eng.unet(rows4(cur), t, None)
        cur = torch.stack([eng.cfg_ddim_prev(eps[4 * im:4 * im + 4], cur[im], t, RATIO, GS).cpu() for im in range(2)])
    assert torch.equal(got, cur), (got - cur).abs().amax(dim=(2, 3, 4))


@pytest.mark.parametrize("has_cond", [True, False])
def test_ef_invert_equals_level1_steps(eng, has_cond):
    x0, noise, ctx = lat(61, 2), lat(62, STEPS, 2), context4(eng, 2, 63)
    cu, cc = ctx[:, 0], (ctx[:, 2] if has_cond else None)
    rpi, eta, scale = (2 if has_cond else 1), 1.0, 3.5
    got_xts, got_zs = (v.cpu() for v in eng.ef_invert(x0, noise, cu, cc, scale, eta, TS))
    xts = eng.ef_sample_xts(x0, noise, TS).cpu()
    zs = torch.zeros_like(noise)
    eng.text_kv_precompute(torch.stack([cu, cc], 1).flatten(0, 1) if has_cond else cu)      # rows [img][uncond, cond]
    for i, t in enumerate(int(v) for v in TS):
        idx = STEPS - 1 - i
        xt = xts[idx + 1]
        eps = eng.unet(xt.repeat_interleave(rpi, 0), t, None).unflatten(0, (2, rpi))
        z, xprev = eng.ef_noise_map(eps, xt, xts[idx], t, RATIO, eta, cfg_scale=scale if has_cond else None)
        zs[idx], xts[idx] = z.cpu(), xprev.cpu()
    zs[0] = 0
    assert torch.equal(got_xts, xts), (got_xts - xts).abs().amax(dim=(1, 2, 3, 4))
    assert torch.equal(got_zs, zs), (got_zs - zs).abs().amax(dim=(1, 2, 3, 4))


@pytest.mark.parametrize("nprompts", [1, 2])
def test_ef_edit_equals_level1_steps(eng, nprompts):
    P, eta = nprompts, 1.0
    xT, zs = lat(71, 1), lat(72, STEPS, 1)
    ctx = weights.synth_context(eng.cfg, 2 * P, seed=73)[None]              # [1, 2P, 77, D]: P uncond rows, then P cond rows
    scales = [3.5, 15.0][:P]
    got = eng.ef_edit(xT, zs, ctx, scales, None, eta, TS).cpu()
    cur = xT[:, None].expand(-1, P, -1, -1, -1).clone()
    eng.text_kv_precompute(ctx[0])
    for k, t in enumerate(int(v) for v in TS):
        eps = eng.unet(torch.cat([cur[0], cur[0]]), t, None)[None]
        cur = eng.ef_reverse_step(eps, cur, zs[STEPS - 1 - k], t, RATIO, eta, scales).cpu()
    assert torch.equal(got, cur), (got - cur).abs().amax(dim=(2, 3, 4))


def test_direct_edit_plain_pass_equals_level1_steps(eng):
    """pnpi_direct_edit with one controller-free pass: the 8 rows of a step are the offset pass's four and the reconstruction pass's four,
    two cfg_ddim_prev per step -- the second one adds the first one's offset to its source row."""
    x_stars, ctx = lat(81, STEPS + 1, 1), context4(eng, 1, 82)
    got_nl, got_lat = (v.cpu() for v in eng.direct_edit(x_stars, ctx, [None], TS, GS))
    rec = [x_stars[-1].expand(2, -1, -1, -1).clone()]

    def rows_of(cur):
        return torch.cat([cur[0], cur[0], rec[0], rec[0]])

    def reconstruction_step(i, t, eps, loss):
        rec[0] = eng.cfg_ddim_prev(eps[4:], rec[0], t, RATIO, GS, noise_loss=loss[0], offset_rows=1).cpu()

    want_nl = offset_steps(eng, x_stars, ctx[0].repeat(2, 1, 1), rows_of, reconstruction_step)
    assert torch.equal(got_nl, want_nl), (got_nl - want_nl).abs().amax(dim=(1, 2, 3, 4, 5))
    assert torch.equal(got_lat[0, 0], rec[0]), (got_lat[0, 0] - rec[0]).abs().amax(dim=(1, 2, 3))
