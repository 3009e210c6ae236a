"""Edit-friendly DDPM inversion + P2P (models/edit_friendly_ddm, run_editing_edit_friendly_p2p.py) on the MI355X: the three kernels
bit-exact against a torch fp32 restatement of the reference's lines, the loops against the reference's own outputs
(tests/golden/e2e_edit_friendly*.npz, tools/make_golden_edit_friendly.py), and the script's 50-step schedule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SD1, SMALL64  # noqa: E402
from pnpinversion_amd.edit_friendly_ddm import inversion_utils as iu  # noqa: E402
from pnpinversion_amd.edit_friendly_ddm.ptp_classes import AttentionRefine, AttentionReplace, AttentionStore  # noqa: E402
from pnpinversion_amd.edit_friendly_ddm.ptp_utils import register_attention_control  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


def make_pipe(cfg, rows=8):
    p = NativePipeline(cfg, max_unet_rows=rows, max_vae_images=2, text_encoder=SyntheticTextEncoder(cfg.cross_dim, seed=7))
    p.load_state_dict(weights.unet_state_dict(cfg, 2), weights.vae_state_dict(cfg, 2))
    return p


@pytest.fixture(scope="module")
def small64():
    p = make_pipe(SMALL64)
    yield p
    p.engine.close()


@pytest.fixture(scope="module")
def sd1():
    p = make_pipe(SD1)
    yield p
    p.engine.close()


def seeded_noise(seed, n, shape):
    g = torch.Generator().manual_seed(int(seed))      # == torch.manual_seed(seed) + torch.randn_like on the CPU (the fixtures' draws)
    return torch.stack([torch.randn(shape, generator=g) for _ in range(n)])


def load_script():
    """this repository's run_editing_edit_friendly_p2p.py (by path: the reference tree, when on sys.path, has a script of that name)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pnpi_run_editing_edit_friendly_p2p",
                                                  os.path.join(os.path.dirname(GOLD), "..", "run_editing_edit_friendly_p2p.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------- torch restatement of the reference
def sq(x):
    """`x ** 0.5`, correctly rounded as on the GPU the reference runs on (torch's CPU sqrt is a vectorised approximation, 1 ulp off
    for some operands; tests/test_edit_friendly_host.py)"""
    return torch.from_numpy(np.asarray(np.sqrt(np.asarray(x.numpy(), dtype=np.float32))))


def ref_scalars(sched, t, eta):
    ac = sched.alphas_cumprod
    tp = t - sched.config.num_train_timesteps // sched.num_inference_steps
    ab_t = ac[t]
    ab_p = ac[tp] if tp >= 0 else sched.final_alpha_cumprod
    var = ((1 - ab_p) / (1 - ab_t)) * (1 - ab_t / ab_p)                    # get_variance :91-98
    return ab_t, ab_p, var


def ref_noise_map(sched, eps_u, eps_c, g, xt, xtm1, t, eta):
    """inversion_utils.py:151-171"""
    ab_t, ab_p, var = ref_scalars(sched, t, eta)
    noise_pred = eps_u + g * (eps_c - eps_u) if eps_c is not None else eps_u
    pred_original_sample = (xt - sq(1 - ab_t) * noise_pred) / sq(ab_t)
    pred_sample_direction = sq(1 - ab_p - eta * var) * noise_pred
    mu_xt = sq(ab_p) * pred_original_sample + pred_sample_direction
    z = (xtm1 - mu_xt) / (eta * sq(var))
    return z, mu_xt + (eta * sq(var)) * z


def ref_reverse(sched, eps_u, eps_c, scales, x, z, t, eta):
    """inversion_utils.py:254-258 + reverse_step :179-208"""
    noise_pred = eps_u + torch.tensor(scales, dtype=torch.float32).view(-1, 1, 1, 1) * (eps_c - eps_u)
    ab_t, ab_p, var = ref_scalars(sched, t, eta)
    pred_original_sample = (x - sq(1 - ab_t) * noise_pred) / sq(ab_t)
    prev = sq(ab_p) * pred_original_sample + sq(1 - ab_p - eta * var) * noise_pred
    if eta > 0:
        prev = prev + eta * sq(var) * z
    return prev


def test_kernels_bit_exact(small64):
    pipe, eng = small64, small64.engine
    n = 10
    pipe.scheduler.set_timesteps(n)
    sched = pipe.scheduler
    ts = [int(t) for t in sched.timesteps]
    g = torch.Generator().manual_seed(5)
    nimg, shp = 2, (4, 64, 64)
    x0 = torch.randn(nimg, *shp, generator=g)
    noise = torch.randn(n, nimg, *shp, generator=g)
    # sample_xts_from_x0 :50-53, all levels in one launch
    xts = eng.ef_sample_xts(x0, noise, ts).cpu()
    ab = sched.alphas_cumprod
    for k in range(n):
        t = ts[n - 1 - k]
        assert torch.equal(xts[k + 1], x0 * sq(ab[t]) + noise[k] * sq(1 - ab[t])), k
    assert torch.equal(xts[0], x0)
    etas = [0.3 + 0.07 * i for i in range(n)]
    for t, eta in [(ts[0], etas[3]), (ts[4], 1.0), (0, etas[0])]:
        eps = torch.randn(nimg, 2, *shp, generator=g)
        xt, xprev = torch.randn(nimg, *shp, generator=g), torch.randn(nimg, *shp, generator=g)
        z, xc = eng.ef_noise_map(eps, xt, xprev, t, 100, eta, cfg_scale=1.0)
        z, xc = z.cpu(), xc.cpu()
        if t == 0:                    # var == 0 (ab_prev = final_alpha_cumprod = ab[0]): z = 0, xts[idx] kept, nothing non-finite
            assert ref_scalars(sched, 0, eta)[2].item() == 0.0
            assert torch.equal(z, torch.zeros_like(z)) and torch.equal(xc, xprev)
        else:
            rz, rx = ref_noise_map(sched, eps[:, 0], eps[:, 1], 1.0, xt, xprev, t, eta)
            assert torch.equal(z, rz) and torch.equal(xc, rx), t
        z1, xc1 = eng.ef_noise_map(eps[:, :1], xt, xprev, t, 100, eta)         # prompt "": no CFG
        if t != 0:
            rz, rx = ref_noise_map(sched, eps[:, 0], None, None, xt, xprev, t, eta)
            assert torch.equal(z1.cpu(), rz) and torch.equal(xc1.cpu(), rx)
        for P, scales in [(2, [1.0, 7.5]), (1, [7.5])]:
            e2 = torch.randn(nimg, 2 * P, *shp, generator=g)
            x = torch.randn(nimg, P, *shp, generator=g)
            zz = torch.randn(nimg, *shp, generator=g)
            out = eng.ef_reverse_step(e2, x, zz, t, 100, eta, scales).cpu()
            assert torch.isfinite(out).all()
            for i in range(nimg):
                r = ref_reverse(sched, e2[i, :P], e2[i, P:], scales, x[i], zz[i].expand(P, *shp), t, eta)
                assert torch.equal(out[i], r), (t, P, i)
    with pytest.raises(Exception):
        eng.ef_noise_map(eps, xt, xprev, ts[0], 100, 0.0, cfg_scale=1.0)


def run_native(pipe, gold, case, ctrl_cls):
    steps, skip = int(gold["steps"]), int(gold["skip"])
    pipe.scheduler.set_timesteps(steps)
    w0 = torch.from_numpy(gold["w0"])
    noise = seeded_noise(gold["noise_seed"], steps, w0.shape)
    src, tgt = str(gold["src"]), str(gold["%s_tgt" % case])
    register_attention_control(pipe, AttentionStore())
    _, zs, xts = iu.inversion_forward_process(pipe, w0, etas=1, prompt=src, cfg_scale=1, num_inference_steps=steps, noise=noise)
    ctrl = ctrl_cls([src, tgt], steps, cross_replace_steps=0.4, self_replace_steps=0.6, model=pipe)
    register_attention_control(pipe, ctrl)
    lat, _ = iu.inversion_reverse_process(pipe, xT=xts[steps - skip], etas=1, prompts=[src, tgt], cfg_scales=[1, 7.5], zs=zs[:steps - skip],
                                          controller=ctrl)
    register_attention_control(pipe, None)
    return xts, zs, lat


# Edited latents vs the fp32 reference.  The UNet runs in fp16 here; the eta = 1 chain carries each step's eps error forward multiplied by
# sqrt(ab_prev / ab_t) (> 1 at every step, ~3x from t = 740 to 0) instead of damping it as DDIM's deterministic map does, so end latents
# sit above the 1.5e-2 of tests/test_gpu_loops.py although xts (<= 1e-7) and every zs (<= 1e-3) match.  Measured on MI355X:
# SMALL64 4-step edit src 0.0107 / tgt 0.0155 (replace), 0.0107 / 0.0150 (refine); SD-1.x width 8-step edit src 0.0311 / tgt 0.0096.
LAT_BAR = {"e2e_edit_friendly.npz": 2e-2, "e2e_edit_friendly_sd1.npz": 4e-2}


def check_against_golden(pipe, name, case):
    gold = np.load(os.path.join(GOLD, name))
    is_replace = bool(gold["%s_is_replace" % case])
    xts, zs, lat = run_native(pipe, gold, case, AttentionReplace if is_replace else AttentionRefine)
    xi = gold["xts_index"]
    ref_xts = torch.from_numpy(gold["xts"])
    assert rel(xts[1:][xi], ref_xts) <= 1e-6, rel(xts[1:][xi], ref_xts)
    ref_zs = torch.from_numpy(gold["zs"].astype(np.float32))
    assert torch.equal(zs[0].cpu(), torch.zeros_like(zs[0].cpu()))
    for i in range(1, zs.shape[0]):
        assert rel(zs[i], ref_zs[i]) <= 1.5e-2, (i, rel(zs[i], ref_zs[i]))
    ref_lat = torch.from_numpy(gold["%s_edited_latents" % case].astype(np.float32))
    print("%s/%s: xts %.3g, zs max %.3g, latents src %.3g tgt %.3g" % (name, case, rel(xts[1:][xi], ref_xts),
          max(rel(zs[i], ref_zs[i]) for i in range(1, zs.shape[0])), rel(lat[0], ref_lat[0]), rel(lat[1], ref_lat[1])))
    assert rel(lat[0], ref_lat[0]) <= LAT_BAR[name], rel(lat[0], ref_lat[0])
    assert rel(lat[1], ref_lat[1]) <= LAT_BAR[name], rel(lat[1], ref_lat[1])
    from pnpinversion_amd.utils.utils import latent2image
    img = latent2image(pipe.vae, lat)[:, ::4, ::4].astype(np.float32)
    d = np.abs(img - gold["%s_images_small" % case].astype(np.float32)).mean()
    assert d <= 2.0, d


@pytest.mark.parametrize("case", ["replace", "refine"])
def test_small64_against_reference_golden(small64, case):
    check_against_golden(small64, "e2e_edit_friendly.npz", case)


def test_sd1_against_reference_golden(sd1):
    check_against_golden(sd1, "e2e_edit_friendly_sd1.npz", "replace")


def test_sd1_script_schedule_retraces_inversion(sd1):
    """50 steps, skip 12 (the script's schedule), no golden: forward counts, finiteness, and the replay identity -- a reverse pass with the
    source prompt at guidance 1 sees the same input, eps and z as the inversion at every step, so it retraces the corrected xts and ends
    on xts[1] (at t = 0 the step returns its input).  An off-by-one in the zs index, the timestep or ab_prev breaks it.
    One-prompt replay: the same 2-row UNet launches as the inversion, so the chain is reproduced to rounding (bar 1e-6).
    Source row of the 2-prompt edit: its 4-row launches pick other GEMM tiles / split-K than the 2-row inversion (fp16 summation order,
    ~1e-3 in eps), and eta = 1 carries that forward amplified by sqrt(ab_prev / ab_t) per step; measured 0.033 on MI355X, bar 5e-2."""
    pipe, eng = sd1, sd1.engine
    from PIL import Image
    from pnpinversion_amd.utils.utils import image2latent
    img = np.array(Image.open(os.path.join(GOLD, "example_cat_512.png")))[:, :, :3]
    w0 = image2latent(pipe.vae, img)
    pipe.scheduler.set_timesteps(50)
    src, tgt = "a cat sitting on a wooden chair", "a dog sitting on a wooden chair"
    eng.reset_counters()
    torch.manual_seed(1234)
    _, zs, xts = iu.inversion_forward_process(pipe, w0, etas=1, prompt=src, cfg_scale=1, num_inference_steps=50)
    ctrl = AttentionReplace([src, tgt], 50, cross_replace_steps=0.4, self_replace_steps=0.6, model=pipe)
    register_attention_control(pipe, ctrl)
    lat, _ = iu.inversion_reverse_process(pipe, xT=xts[38], etas=1, prompts=[src, tgt], cfg_scales=[1, 7.5], zs=zs[:38], controller=ctrl)
    register_attention_control(pipe, None)
    torch.cuda.synchronize()
    assert eng.counters()["unet_sample_forwards"] == 50 * 2 + 38 * 4
    for t in (xts, zs, lat):
        assert torch.isfinite(t).all()
    r = rel(lat[0], xts[1])
    rep1, _ = iu.inversion_reverse_process(pipe, xT=xts[38], etas=1, prompts=[src], cfg_scales=[1], zs=zs[:38])
    r1 = rel(rep1[0], xts[1])
    print("edit source row vs xts[1]: rel-L2 %.3g; one-prompt replay %.3g" % (r, r1))
    assert r1 <= 1e-6, r1
    assert r <= 5e-2, r


def test_batched_edit_equals_single(small64):
    """Two images and prompt pairs (one Replace, one Refine) in one pnpi_ef_edit call == the two single-image calls.  Rows are independent
    in every kernel; only the per-launch tile / split-K choice differs with the row count (fp32 summation order of fp16 GEMMs), which the
    eta = 1 chain carries forward (see LAT_BAR): measured 0.0087 on MI355X, bar 1.5e-2 (tests/test_gpu_loops.py uses 1e-2 for the same
    effect in the deterministic DDIM chain)."""
    pipe, eng = small64, small64.engine
    steps, skip = 6, 2
    pipe.scheduler.set_timesteps(steps)
    ts = [int(t) for t in pipe.scheduler.timesteps]
    g = torch.Generator().manual_seed(11)
    x0 = torch.randn(2, 4, 64, 64, generator=g)
    noise = torch.randn(steps, 2, 4, 64, 64, generator=g)
    pairs = [("a cat sitting on a wooden chair", "a dog sitting on a wooden chair"),
             ("a photograph of a mountain", "a watercolor photograph of a snowy mountain")]
    enc = lambda p: iu.encode_text(pipe, p)                        # noqa: E731
    unc = enc("")
    xts, zs = eng.ef_invert(x0, noise, unc.expand(2, -1, -1), torch.cat([enc(pairs[0][0]), enc(pairs[1][0])]), 1.0, 1, ts)
    ctx = torch.stack([torch.cat([unc, unc, enc(list(p))]) for p in pairs])          # [2, 4, 77, D]
    ctrls = [AttentionReplace(list(pairs[0]), steps, 0.4, 0.6, model=pipe).tables(), AttentionRefine(list(pairs[1]), steps, 0.4, 0.6, model=pipe).tables()]
    both = eng.ef_edit(xts[steps - skip], zs[:steps - skip], ctx, [1, 7.5], ctrls, 1, ts)
    for i in range(2):
        one = eng.ef_edit(xts[steps - skip, i:i + 1], zs[:steps - skip, i:i + 1], ctx[i:i + 1], [1, 7.5], ctrls[i:i + 1], 1, ts)
        print("batched vs single, image %d: %.3g" % (i, rel(both[i], one[0])))
        assert rel(both[i], one[0]) <= 1.5e-2, (i, rel(both[i], one[0]))
        # and the batched inversion == the single-image one
        xs1, zs1 = eng.ef_invert(x0[i:i + 1], noise[:, i:i + 1], unc, enc(pairs[i][0]), 1.0, 1, ts)
        print("batched vs single inversion, image %d: xts %.3g zs %.3g" % (i, rel(xts[:, i], xs1[:, 0]), rel(zs[1:, i], zs1[1:, 0])))
        assert rel(xts[:, i], xs1[:, 0]) <= 1e-3 and rel(zs[1:, i], zs1[1:, 0]) <= 1e-2


def test_edit_image_ef_panel(small64):
    ef = load_script()
    panels = ef.edit_images_EF(small64, [os.path.join(GOLD, "example_cat_512.png")], ["a cat sitting on a wooden chair"],
                               ["a dog sitting on a wooden chair"], num_ddim_steps=6, skip=2)
    a = np.array(panels[0])
    assert a.shape == (512, 2048, 3) and a.dtype == np.uint8
    from PIL import Image
    gt = np.array(Image.open(os.path.join(GOLD, "example_cat_512.png")))[:, :, :3]
    assert np.abs(a[:, 512:1024].astype(int) - gt.astype(int)).max() <= 1
