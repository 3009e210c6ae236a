"""The bench's extras at the BENCHMARKED width (VERDICT r4 "what's weak" 1): full SD-1.x configuration, every path bench.py times next
to the headline -- 8 images per set of launches (96-row launches: the b96 rows of the tile table, conv M = 393 216), two images
(24-row launches), the pruned schedule (3-row launches), three images in flight on three library contexts, the next image's inversion
overlapped on a second context -- each against the reference's own P2PEditor("directinversion+p2p") run on the same image, prompts and
weights (tests/golden/e2e_sd1.npz, 2 + 2 steps, oracle/make_golden.py e2e_sd1) at the bars of tests/test_gpu_headline_parity.py.
A tile-table row that goes wrong at 3 / 24 / 96 rows turns these red; the TINY16 / SMALL64 tests of test_gpu_loops.py never reach
those rows.  Also one ping-pong convolution at B = 96, H = 64 (M = 393 216) against F.conv2d.
Reference: /root/reference/run_editing_p2p.py:102-146 (the sweep visits images one by one; every mode here is that loop's throughput form)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SD1  # noqa: E402
from pnpinversion_amd.p2p_editor import P2PEditor  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402
from tests.gpu_util import Ctx, ptr, rel_err, max_err  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


def masked_rel(a, b, pix_tol=0.25):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    bad = (a - b).abs().amax(dim=-3) > pix_tol
    keep = (~bad).unsqueeze(-3).expand_as(a)
    return ((a - b)[keep].norm() / b[keep].norm()).item(), bad.float().mean().item()


def psnr_u8(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def _cat_image():
    from PIL import Image
    return np.array(Image.open(os.path.join(GOLD, "example_cat_512.png")))[:, :, :3]


@pytest.fixture(scope="module")
def sd1():
    g = np.load(os.path.join(GOLD, "e2e_sd1.npz"))
    pipe = NativePipeline(SD1, max_unet_rows=96, max_vae_images=2, text_encoder=SyntheticTextEncoder(SD1.cross_dim, seed=7))
    seed = int(g["weight_seed"])
    pipe.load_state_dict(weights.unet_state_dict(SD1, seed), weights.vae_state_dict(SD1, seed))
    yield pipe, g
    pipe.engine.close()


def _kw(g):
    w0, w1 = [str(x) for x in g["blend"]]
    return str(g["src"]), str(g["tgt"]), ((w0,), (w1,)), {"words": (w1,), "values": (2,)}


def _check_panel(panel, g, what):
    """reconstruction / edited panels (4x subsampled) against the reference's own: SURVEY 8(d) mean |diff| <= 2 / 255, PSNR >= 35 dB"""
    p = np.array(panel)
    assert p.shape == (512, 2048, 3), p.shape
    rec_small, edit_small = p[::4, 1024:1536:4], p[::4, 1536::4]
    d_rec = np.abs(rec_small.astype(np.int32) - g["recon_image_small"].astype(np.int32)).mean()
    d_edit = np.abs(edit_small.astype(np.int32) - g["edited_image_small"].astype(np.int32)).mean()
    ps_rec, ps_edit = psnr_u8(rec_small, g["recon_image_small"]), psnr_u8(edit_small, g["edited_image_small"])
    print("%s: panels mean|d| %.2f / %.2f, PSNR %.1f / %.1f dB" % (what, d_rec, d_edit, ps_rec, ps_edit))
    assert d_rec <= 2.0 and d_edit <= 2.0, (what, d_rec, d_edit)
    assert ps_rec >= 35.0 and ps_edit >= 35.0, (what, ps_rec, ps_edit)


@pytest.mark.parametrize("n", [2, 8])
def test_sd1_batched_images_against_reference_golden(sd1, n):
    """bench.py `batched`: n copies of the golden's image through ONE set of launches (n-row inversion, 12n-row lock-step loop)."""
    pipe, g = sd1
    steps = int(g["steps"])
    src, tgt, blend, eq = _kw(g)
    ed = P2PEditor(["directinversion+p2p"], "cuda", num_ddim_steps=steps, pipeline=pipe)
    img = _cat_image()
    panels, st = ed.edit_images_directinversion([img] * n, [src] * n, [tgt] * n, guidance_scale=7.5, cross_replace_steps=0.4,
                                                self_replace_steps=0.6, blend_words=[blend] * n, eq_params=[eq] * n, return_stages=True)
    assert len(panels) == n
    gx, go, gr = torch.from_numpy(g["x_stars"]), torch.from_numpy(g["edited_latents"]), torch.from_numpy(g["reconstruct_latent"])
    for i in range(n):
        xs = st["x_stars"][:, i].cpu()
        r_inv = rel(xs, gx[:, 0])
        assert r_inv < 6e-3, (i, r_inv)                                              # incl. the 512 x 512 VAE encode
        r_rec = rel(st["reconstruct_latents"][i][1], gr[1])
        assert r_rec < 2e-2, (i, r_rec)
        r_e, frac = masked_rel(st["latents"][i], go)
        assert frac <= 0.01 and r_e < 2e-2, (i, r_e, frac)
        _check_panel(panels[i], g, "batched n=%d image %d" % (n, i))
    # the rows of one launch are independent: every copy of the image gives the same latents whatever its row
    for i in range(1, n):
        assert rel(st["latents"][i], st["latents"][0]) < 1e-6


def test_sd1_batched_images_full_schedule_against_reference_golden(sd1):
    """BASELINE config 3's launch shape at the benchmarked SCHEDULE (round 6): 8 copies of the golden's image through one set of launches --
    50 eight-row inversion forwards, 50 ninety-six-row lock-step forwards -- against the reference's own 50 + 50-step run (e2e_sd1_50.npz) at
    the bars of tests/test_gpu_headline_parity.py: what `bench.py`'s `batched` extra times."""
    pipe, _ = sd1
    g = np.load(os.path.join(GOLD, "e2e_sd1_50.npz"))
    steps, n = int(g["steps"]), 8
    assert steps == 50
    src, tgt, blend, eq = _kw(g)
    ed = P2PEditor(["directinversion+p2p"], "cuda", num_ddim_steps=steps, pipeline=pipe)
    img = _cat_image()
    panels, st = ed.edit_images_directinversion([img] * n, [src] * n, [tgt] * n, guidance_scale=7.5, cross_replace_steps=0.4,
                                                self_replace_steps=0.6, blend_words=[blend] * n, eq_params=[eq] * n, return_stages=True)
    xi = [int(i) for i in g["x_stars_index"]]
    gx, go, gr = torch.from_numpy(g["x_stars"]), torch.from_numpy(g["edited_latents"]), torch.from_numpy(g["reconstruct_latent"])
    for i in (0, n - 1):
        for j, k in enumerate(xi):
            r = rel(st["x_stars"][k, i].cpu(), gx[j, 0])
            assert r < 4e-3 * max(k, 1) ** 0.5, (i, k, r)
        assert rel(st["latents"][i][0], go[0]) < 2e-2                              # the source branch returns to x*_0
        assert rel(st["reconstruct_latents"][i][1], gr[1]) < 2e-2
        scale = max(1.0, float(go[1].pow(2).mean().sqrt()))
        r_e, frac = masked_rel(st["latents"][i][1], go[1], pix_tol=0.25 * scale)
        assert frac <= 0.005 and r_e < 2e-2, (i, r_e, frac)
        _check_panel(panels[i], g, "batched n=8, 50 + 50 steps, image %d" % i)
    for i in range(1, n):
        assert rel(st["latents"][i], st["latents"][0]) < 1e-6                       # independent rows: every copy lands on the same latents
    pipe.scheduler.set_timesteps(int(np.load(os.path.join(GOLD, "e2e_sd1.npz"))["steps"]))


def test_sd1_batched_stream_overlaps_the_next_batch_inversion_with_identical_panels(sd1):
    """bench.py `batched.pipelined` (round 6): batches of 4 images, the next batch's 4-row inversion on a second context /
    HIP stream under this batch's 48-row lock-step loop -- the same kernels on the same inputs as the serial batch call -> identical
    panels; and those within the bars of the reference's own run."""
    pipe, g = sd1
    src, tgt, blend, eq = _kw(g)
    ed = P2PEditor(["directinversion+p2p"], "cuda", num_ddim_steps=int(g["steps"]), pipeline=pipe)
    img, n = _cat_image(), 4
    kw = dict(guidance_scale=7.5, cross_replace_steps=0.4, self_replace_steps=0.6)
    imgs = [np.roll(img, 17 * j, axis=1) for j in range(n)]                          # different images per row (image 0 is the golden's)
    serial = [np.array(p) for p in ed.edit_images_directinversion(imgs, [src] * n, [tgt] * n, blend_words=[blend] * n, eq_params=[eq] * n, **kw)]
    _check_panel(serial[0], g, "serial batch, image 0")
    batch = (imgs, [src] * n, [tgt] * n, [blend] * n, [eq] * n)
    try:
        got = [[np.array(p) for p in panels] for panels in ed.edit_stream_images_directinversion([batch] * 3, **kw)]
    finally:
        ed.close_peers()
    assert len(got) == 3 and all(len(b) == n for b in got)
    for bi, b in enumerate(got):
        for i in range(n):
            assert np.array_equal(b[i], serial[i]), "overlapped batch %d: image %d differs from the serial batch's panel" % (bi, i)


def test_sd1_pruned_schedule_against_reference_golden(sd1):
    """bench.py `pruned_schedule`: 3-row launches (source latent assigned from the inversion trajectory) at full width."""
    pipe, g = sd1
    src, tgt, blend, eq = _kw(g)
    ed = P2PEditor(["directinversion+p2p"], "cuda", num_ddim_steps=int(g["steps"]), pipeline=pipe)
    ed.schedule = "pruned"
    panel, st = ed.edit_image_directinversion(_cat_image(), src, tgt, guidance_scale=7.5, cross_replace_steps=0.4, self_replace_steps=0.6,
                                              blend_word=blend, eq_params=eq, return_stages=True)
    r_e, frac = masked_rel(st["latents"][1], torch.from_numpy(g["edited_latents"])[1])
    assert frac <= 0.01 and r_e < 2e-2, (r_e, frac)
    _check_panel(panel, g, "pruned schedule")


def test_sd1_in_flight_and_overlapped_streams_against_reference_golden(sd1):
    """bench.py `in_flight` (three library contexts, three worker threads) and `pipelined` (next image's inversion on a second context):
    the same kernels on the same inputs as the one-by-one call -> identical panels, and those within the bars of the reference's run."""
    pipe, g = sd1
    src, tgt, blend, eq = _kw(g)
    ed = P2PEditor(["directinversion+p2p"], "cuda", num_ddim_steps=int(g["steps"]), pipeline=pipe)
    img = _cat_image()
    kw = dict(guidance_scale=7.5, cross_replace_steps=0.4, self_replace_steps=0.6)
    one = np.array(ed("directinversion+p2p", img, src, tgt, blend_word=blend, eq_params=eq, **kw))
    _check_panel(one, g, "one by one")
    items = [(img, src, tgt, blend, eq)] * 4
    try:
        got = [np.array(p) for p in ed.edit_stream_in_flight("directinversion+p2p", items, n_flight=3, **kw)]
    finally:
        ed.close_peers()
    assert len(got) == 4
    for i, p in enumerate(got):
        assert np.array_equal(p, one), "in flight: image %d differs from the one-by-one panel" % i
    got = [np.array(p) for p in ed.edit_stream_directinversion(items[:3], **kw)]
    assert len(got) == 3
    for i, p in enumerate(got):
        assert np.array_equal(p, one), "overlapped inversion: image %d differs from the one-by-one panel" % i
    ed.close_peers()


def test_pingpong_conv_at_96_rows_of_64x64():
    """The 3 x 3 convolution of the 64 x 64 level at the batched launch size: B = 96, H = W = 64, 320 -> 320 channels, M = 393 216 rows
    (row offsets beyond 2^18, activation byte offsets to 252 MB under the 2 GiB buffer descriptor), both ping-pong geometries."""
    c = Ctx()
    try:
        B, C1, H, N = 96, 320, 64, 320
        g = torch.Generator(device="cpu").manual_seed(11)
        x = (torch.randn(B, H, H, C1, generator=g)).half().cuda()                      # NHWC
        w = (torch.randn(N, C1, 3, 3, generator=g) / math.sqrt(9 * C1)).half().cuda()
        bias = torch.randn(N, generator=g).cuda()
        wp = w.permute(0, 2, 3, 1).contiguous().reshape(N, -1)
        ref = None
        for cfg in (17, 16):
            out = torch.full((B, H, H, N), float("nan"), dtype=torch.half, device="cuda")
            c.call("pnpi_op_conv", ptr(x), None, C1, 0, B, H, H, 3, 1, 1, 0, H, H, ptr(wp), ptr(bias), None, N, ptr(out), cfg, 0)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            if ref is None:
                # fp32 reference in chunks of 8 images (the fp32 NCHW copies of 96 images are 1.9 GB)
                ref = torch.empty(B, H, H, N, device="cuda")
                for b0 in range(0, B, 8):
                    xb = x[b0:b0 + 8].permute(0, 3, 1, 2).float()
                    ref[b0:b0 + 8] = F.conv2d(xb, w.float(), bias, padding=1).permute(0, 2, 3, 1)
            assert rel_err(out, ref) < 2e-3, (cfg, rel_err(out, ref), max_err(out, ref))
            # the last image alone (the highest addresses), and the padded border rows of it
            assert rel_err(out[-1], ref[-1]) < 2e-3 and rel_err(out[-1, 0], ref[-1, 0]) < 2e-3 and rel_err(out[-1, :, -1], ref[-1, :, -1]) < 2e-3
    finally:
        c.close()
