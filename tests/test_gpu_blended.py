"""Blended Latent Diffusion (run_editing_blended_latent_diffusion.py) on the MI355X: the step and mask kernels bit-exact against a torch
fp32 restatement / the reference's own masks, the device-resident loop against its level-1 composition and against invariants that need
no fixture, BlendedLatnetDiffusion.edit_image against the reference's own run (tests/golden/e2e_blended_tiny.npz,
tools/make_golden_blended.py), batching, and the refusals.  TINY16 throughout."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi, weights  # noqa: E402
from pnpinversion_amd.blended_latent_diffusion import BlendedLatnetDiffusion, timestep_slice  # noqa: E402
from pnpinversion_amd.config import TINY16  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GS = 7.5
S = TINY16.sample_size
MAX_ROWS = 6                    # three images of two rows


def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def pipe():
    p = NativePipeline(TINY16, max_unet_rows=MAX_ROWS, max_vae_images=2, text_encoder=SyntheticTextEncoder(TINY16.cross_dim, seed=7))
    p.load_state_dict(weights.unet_state_dict(TINY16, 2), weights.vae_state_dict(TINY16, 2))       # the fixture's weight seed
    yield p
    p.engine.close()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rand_mask(seed, *shape):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < 0.4).float()


# ---------------------------------------------------------------------------------------------- torch restatement of the reference
def sq(x):
    """`x ** 0.5` of a 0-dim fp32 tensor, correctly rounded as on the GPU the reference runs on (torch's CPU sqrt is 1 ulp off for some
    operands; tests/test_edit_friendly_host.py)"""
    return torch.from_numpy(np.asarray(np.sqrt(np.asarray(x.numpy(), dtype=np.float32))))


def alphas(eng, t, ratio):
    ac = torch.from_numpy(eng.ac)
    return ac[t], (ac[t - ratio] if t - ratio >= 0 else torch.tensor(np.float32(eng.final_alpha)))     # DDIMScheduler.step: prev_timestep


def noised_source(eng, src, noise, t):
    """scheduler.add_noise(source, noise, t) (run script :136-138): sqrt(ab_t) * src + sqrt(1 - ab_t) * noise"""
    ab_t = torch.from_numpy(eng.ac)[t]
    return sq(ab_t) * src + sq(1 - ab_t) * noise


def ref_step(eng, eps, x, src, noise, mask, t, ratio, g):
    """run script :127-139 with diffusers' DDIMScheduler.step (eta = 0, no clipping), eager fp32 op by op"""
    ab_t, ab_p = alphas(eng, t, ratio)
    noise_pred = eps[:, 0] + g * (eps[:, 1] - eps[:, 0])                                    # :128-130
    pred_original_sample = (x - sq(1 - ab_t) * noise_pred) / sq(ab_t)                       # step: beta_prod_t ** 0.5, alpha_prod_t ** 0.5
    pred_sample_direction = sq(1 - ab_p) * noise_pred                                       # std_dev_t = 0
    latents = sq(ab_p) * pred_original_sample + pred_sample_direction                       # :133
    latent_mask = mask[:, None]
    return latents * latent_mask + noised_source(eng, src, noise, t) * (1 - latent_mask)    # :139


# ---------------------------------------------------------------------------------------------- 1, 2: the kernels
@pytest.mark.parametrize("t,ratio", [(740, 20), (0, 20), (500, 100)])
def test_bld_step_bit_exact(pipe, t, ratio):
    """nimg = 3, h x w = 5 x 7: E = 140 is no multiple of any vector width and spans more than one wavefront; t = 0 takes the
    final_alpha_cumprod branch"""
    eng = pipe.engine
    nimg, h, w = 3, 5, 7
    eps, x, src, noise = randn(1, nimg, 2, 4, h, w), randn(2, nimg, 4, h, w), randn(3, nimg, 4, h, w), randn(4, nimg, 4, h, w)
    masks = {"random": rand_mask(5, nimg, h, w), "ones": torch.ones(nimg, h, w), "zeros": torch.zeros(nimg, h, w)}
    assert not torch.equal(masks["random"][0], masks["random"][1]) and 0 < masks["random"].mean() < 1
    for name, mask in masks.items():
        want = ref_step(eng, eps, x, src, noise, mask, t, ratio, GS)
        got = eng.bld_step(eps, x, src, noise, mask, t, ratio, GS).cpu()
        assert torch.equal(got, want), (name, (got - want).abs().max())
        xd = x.to(eng.device).clone()
        out = eng.bld_step(eps, xd, src, noise, mask, t, ratio, GS, inplace=True)           # x_out aliases x
        assert out.data_ptr() == xd.data_ptr() and torch.equal(xd.cpu(), want), name
    assert torch.equal(eng.bld_step(eps, x, src, noise, masks["zeros"], t, ratio, GS).cpu(), noised_source(eng, src, noise, t))
    with pytest.raises(ValueError, match=r"mask must be \[nimg, h, w\]"):
        eng.bld_step(eps, x, src, noise, masks["ones"][:, :4], t, ratio, GS)


def test_bld_mask_exact_against_reference_masks(pipe):
    """128 -> 16 on this context; 512 -> 64 on a context of that latent size built without weights (the kernel reads none)"""
    eng = pipe.engine
    g = np.load(os.path.join(GOLD, "blended_mask_cases.npz"))
    names = [str(n) for n in g["names"]]
    small = [n for n in names if int(g[n + "_side"]) == 128]
    large = [n for n in names if int(g[n + "_side"]) == 512]
    assert len(small) >= 4 and len(large) >= 4
    got = eng.bld_mask(torch.from_numpy(np.stack([g[n + "_mask_u8"] for n in small]))).cpu()
    for i, n in enumerate(small):
        assert torch.equal(got[i], torch.from_numpy(g[n + "_latent"])), n
    # any non-zero value is >= 0.5
    assert torch.equal(eng.bld_mask(torch.from_numpy(g[small[0] + "_mask_u8"] * 255)).cpu()[0], torch.from_numpy(g[small[0] + "_latent"]))
    from tests.gpu_util import Ctx, ptr, tiny_config
    ctx = Ctx(tiny_config(sample_size=64), max_rows=1)
    try:
        m = torch.from_numpy(np.stack([g[n + "_mask_u8"] for n in large])).cuda()
        out = torch.empty(len(large), 64, 64, device="cuda")
        ctx.call("pnpi_bld_mask", ptr(m), len(large), 512, 512, ptr(out))
        torch.cuda.synchronize()
        for i, n in enumerate(large):
            assert torch.equal(out[i].cpu(), torch.from_numpy(g[n + "_latent"])), n
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- 3, 4, 7: the loop
def loop_inputs(eng, nimg, n_run, seed):
    ctx = weights.synth_context(eng.cfg, 2 * nimg, seed=seed).reshape(nimg, 2, TINY16.ctx_len, TINY16.cross_dim)
    return dict(x=randn(seed + 1, nimg, 4, S, S), src=randn(seed + 2, nimg, 4, S, S), noise=randn(seed + 3, n_run, nimg, 4, S, S),
                mask=rand_mask(seed + 4, nimg, S, S), cu=ctx[:, 0], cc=ctx[:, 1])


def run_loop(eng, a, ts, **over):
    a = dict(a, **over)
    return eng.bld_edit(a["x"], a["src"], a["noise"], a["mask"], a["cu"], a["cc"], GS, ts).cpu()


def test_bld_edit_equals_level1_steps(pipe):
    """two images with different contexts, latents, sources, draws and masks; 3 executed steps of a 4-step schedule"""
    eng = pipe.engine
    ts, n_run = [750, 500, 250, 0], 3
    a = loop_inputs(eng, 2, n_run, 100)
    got = run_loop(eng, a, ts)
    eng.text_kv_precompute(torch.stack([a["cu"], a["cc"]], 1).flatten(0, 1))                # rows [img][uncond, cond]
    cur = a["x"]
    for k, t in enumerate(ts[-n_run:]):
        eps = eng.unet(cur.repeat_interleave(2, 0), t, None).unflatten(0, (2, 2))
        cur = eng.bld_step(eps, cur, a["src"], a["noise"][k], a["mask"], t, 250, GS).cpu()
    assert torch.equal(got, cur), (got - cur).abs().amax(dim=(1, 2, 3))


def test_bld_edit_invariants_and_counters(pipe):
    eng = pipe.engine
    ts, n_run, nimg = [750, 500, 250, 0], 3, 2
    a = loop_inputs(eng, nimg, n_run, 200)
    anchor = noised_source(eng, a["src"], a["noise"][-1], ts[-1])            # sqrt(ab_0) src + sqrt(1 - ab_0) noise_last
    # all-zeros mask: the output is the re-anchored source, whatever the prompt
    zeros = torch.zeros_like(a["mask"])
    assert torch.equal(run_loop(eng, a, ts, mask=zeros), anchor)
    assert torch.equal(run_loop(eng, a, ts, mask=zeros, cc=a["cu"], cu=a["cc"]), anchor)
    # outside any mask the final latent is that expression
    eng.reset_counters()
    out = run_loop(eng, a, ts)
    c = eng.counters()
    assert c["unet_sample_forwards"] == 2 * nimg * n_run and c["unet_sample_forwards_cached_kv"] == 2 * nimg * n_run, c
    assert c["unet_calls"] == n_run and c["text_kv_rows"] == 2 * nimg, c
    outside = (a["mask"] == 0)[:, None].expand_as(out)
    assert outside.any() and (~outside).any()
    assert torch.equal(out[outside], anchor[outside])
    assert not torch.equal(out[~outside], anchor[~outside])
    # inside the mask a one-step run does not see the source
    one = run_loop(eng, a, ts, noise=a["noise"][:1])
    swapped = run_loop(eng, a, ts, noise=a["noise"][:1], src=a["src"].flip(0) + 1.0)
    assert torch.equal(one[~outside], swapped[~outside]) and not torch.equal(one[outside], swapped[outside])


def test_bld_edit_refusals_launch_nothing(pipe):
    eng = pipe.engine
    ts = [750, 500, 250, 0]
    torch.cuda.synchronize()
    before = eng.counters()
    too_many = loop_inputs(eng, MAX_ROWS // 2 + 1, 2, 300)                                   # 2 * nimg > max_unet_rows
    with pytest.raises(_capi.PnpiError, match=r"2 \* nimg exceeds max_unet_rows") as e:
        run_loop(eng, too_many, ts)
    assert e.value.status == _capi.PNPI_EINVAL
    too_long = loop_inputs(eng, 1, len(ts) + 1, 310)                                         # nsteps_run > nsteps_total
    with pytest.raises(_capi.PnpiError, match="nsteps_run") as e:
        run_loop(eng, too_long, ts)
    assert e.value.status == _capi.PNPI_EINVAL
    assert eng.counters() == before
    with pytest.raises(ValueError, match=r"noise must be \[nsteps_run, nimg, 4, h, w\]"):
        run_loop(eng, too_long, ts, noise=too_long["noise"][:, 0])


# ---------------------------------------------------------------------------------------------- 5: parity with the reference's run
# The bars of tests/test_gpu_loops.py for its deterministic end-to-end fixtures: latents rel-L2 < 1.5e-2 against the reference's fp32
# run, decoded images mean |diff| < 2 (in units of 1/255).
LAT_BAR, IMG_BAR = 1.5e-2, 2.0
# Outside the mask every step stores sqrt(ab_t) src + sqrt(1 - ab_t) noise_k of given operands: two products and a sum, each rounded once
# (<= 0.5 ulp), with scalars that may differ from the reference's by 1 ulp (torch's CPU sqrt).  Per element that is <= 2.5 * 2^-24 of
# |a| + |b|; over the region ||diff|| <= 2.5 * 2^-24 * sqrt(2) * sqrt(||a||^2 + ||b||^2) ~ 2.1e-7 ||ref|| for independent a, b.  No UNet
# output enters, so the bound is the same at every step: it cannot grow with the step index.
OUTSIDE_BAR = 4 * 2.0 ** -22     # 9.5e-7: the estimate above with a factor 4 for the cancellation between a and b in ||ref||


def test_edit_image_against_reference_golden(pipe):
    g = np.load(os.path.join(GOLD, "e2e_blended_tiny.npz"))
    assert int(g["weight_seed"]) == 2
    from PIL import Image
    bld = BlendedLatnetDiffusion(pipe=pipe)
    side, steps, pct = int(g["side"]), int(g["steps"]), float(g["blending_percentage"])
    mask = Image.fromarray(g["mask_u8"]).convert("L")
    prompt = str(g["prompt"])
    noise = (torch.from_numpy(g["draw_start"]), torch.from_numpy(g["draws_blend"]))
    # the inputs the loop sees are the reference's
    ids = pipe.tokenizer([prompt, ""], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert np.array_equal(ids.numpy(), g["prompt_ids"])
    assert torch.equal(bld._encode([prompt, ""]).cpu(), torch.from_numpy(g["embeddings"]))
    assert torch.equal(bld._read_mask(mask, (side // 8, side // 8))[0][0, 0].cpu(), torch.from_numpy(g["mask_latent"]))
    pipe.scheduler.set_timesteps(steps)
    ts = [int(t) for t in pipe.scheduler.timesteps]
    run_ts = [int(t) for t in timestep_slice(ts, pct)]
    assert run_ts == g["timesteps"].tolist() and len(run_ts) == 8
    image = np.array(Image.open(os.path.join(GOLD, "example_cat_512.png")).resize((side, side), Image.BILINEAR))[:, :, :3]
    assert np.array_equal(image, g["image"])
    src = bld._image2latent(image)
    r_src = rel(src, g["source_latent"])
    assert r_src < 4e-3, r_src                           # the image2latent bar of tests/test_gpu_model.py
    # every per-step latent: the loop stopped after k steps IS the loop's state after step k (same launches, same rows)
    eng = pipe.engine
    ref_steps, ref_src = torch.from_numpy(g["latents_steps"]), torch.from_numpy(g["source_latent"])
    lat_mask = torch.from_numpy(g["mask_latent"])
    inside = (lat_mask == 1)[None].expand(4, -1, -1)
    uncond, cond = bld._encode([""]), bld._encode([prompt])
    off = len(ts) - len(run_ts)
    ac = torch.from_numpy(eng.ac)
    d_all, d_out, d_in, d_anchor = [], [], [], []
    for k in range(1, len(run_ts) + 1):
        cut = [ts[0]] * (len(run_ts) - k) + ts[:off + k]       # same length (same step ratio); its last k entries are steps 1 .. k
        run = lambda s: eng.bld_edit(noise[0][None], s, noise[1][:k, None], lat_mask[None], uncond, cond, GS, cut)[0].cpu()   # noqa: E731
        lat, ref = run(src), ref_steps[k - 1]
        d_all.append(rel(lat, ref)); d_out.append(rel(lat[~inside], ref[~inside])); d_in.append(rel(lat[inside], ref[inside]))
        # outside the mask the latent is re-anchored to the GIVEN source at every step.  With the reference's own source latent the
        # distance is rounding only, at every step alike ...
        d_anchor.append(rel(run(ref_src)[~inside], ref[~inside]))
        assert d_anchor[-1] <= OUTSIDE_BAR, (k, d_anchor[-1])
        # ... and with the encoded one it is the encoder's error scaled by sqrt(ab_t): nothing a step adds is carried to the next
        enc = (sq(ac[run_ts[k - 1]]) * (src[0].cpu() - ref_src[0]))[~inside].norm() / ref[~inside].norm()
        assert d_out[-1] <= float(enc) + OUTSIDE_BAR, (k, d_out[-1], float(enc))
    print("blended parity per step, whole latent:", " ".join("%.3g" % d for d in d_all))
    print("blended parity per step, inside mask: ", " ".join("%.3g" % d for d in d_in))
    print("blended parity per step, outside mask:", " ".join("%.3g" % d for d in d_out))
    print("outside the mask with the reference's source latent:", " ".join("%.3g" % d for d in d_anchor))
    for k, d in enumerate(d_all):
        assert d < LAT_BAR, (k, d)
    panels, latents = bld.edit_images([os.path.join(GOLD, "example_cat_512.png")], [mask], [prompt], side, side, steps, GS,
                                      blending_percentage=pct, noise=noise, return_latents=True)
    assert torch.equal(latents[0].cpu(), lat)            # edit_images runs that same loop
    d_final = rel(latents, g["latent_final"])
    assert d_final < LAT_BAR, d_final
    single = bld.edit_image(os.path.join(GOLD, "example_cat_512.png"), mask, [prompt], side, side, steps, GS, blending_percentage=pct, noise=noise)
    assert all(np.array_equal(a, b) for a, b in zip(single, panels[0]))
    p = panels[0]
    assert len(p) == 4 and p[0].shape == (512, 512, 3) and np.array_equal(p[1], g["image"]) and not p[2].any() and p[2].shape == p[0].shape
    d_img = np.abs(p[3].astype(np.float32) - g["edited"].astype(np.float32)).mean()
    print("blended parity: source latent %.3g, final latent %.3g, edited panel mean |diff| %.3g / 255" % (r_src, d_final, d_img))
    assert p[3].shape == g["edited"].shape and p[3].dtype == np.uint8 and d_img < IMG_BAR, d_img


# ---------------------------------------------------------------------------------------------- 6: batching
def test_three_images_in_one_call_equal_single_calls(pipe):
    """Rows are independent in every kernel; only the per-launch tile / split-K choice differs with the row count (6 rows against 2),
    which the existing batching test (tests/test_gpu_loops.py::test_batched_images_match_single_image_calls) bounds by rel-L2 < 3e-2."""
    from PIL import Image
    bld = BlendedLatnetDiffusion(pipe=pipe)
    side = S * 8
    cat = Image.open(os.path.join(GOLD, "example_cat_512.png")).convert("RGB")
    images = [cat, cat.transpose(Image.FLIP_LEFT_RIGHT), cat.transpose(Image.FLIP_TOP_BOTTOM)]
    prompts = ["a dog sitting on a wooden chair", "a photograph of a snowy mountain", "a red bird"]
    masks = []
    for top, bottom, left, right in [(37, 90, 21, 77), (10, 60, 70, 120), (60, 125, 5, 50)]:
        m = np.zeros((side, side), np.uint8)
        m[top:bottom + 1, left:right + 1] = 1
        masks.append(Image.fromarray(m).convert("L"))
    noise = [(randn(400 + i, 4, S, S), randn(410 + i, 8, 4, S, S)) for i in range(3)]
    panels, both = bld.edit_images(images, masks, prompts, side, side, 10, GS, blending_percentage=0.25, noise=noise, return_latents=True)
    singles = []
    for i in range(3):
        p1, one = bld.edit_images(images[i:i + 1], masks[i:i + 1], prompts[i:i + 1], side, side, 10, GS, blending_percentage=0.25,
                                  noise=noise[i:i + 1], return_latents=True)
        singles.append(one[0].cpu())
        assert np.array_equal(p1[0][1], panels[i][1])
        assert np.abs(p1[0][3].astype(np.float32) - panels[i][3].astype(np.float32)).mean() < 2.0
    d = [rel(both[i], singles[i]) for i in range(3)]
    wrong = [rel(both[i], singles[(i + 1) % 3]) for i in range(3)]
    print("batched vs single:", d, "against the next image's:", wrong)
    for i in range(3):
        assert d[i] < 3e-2, (i, d[i])
        assert not wrong[i] < 3e-2, (i, wrong[i])          # the same tolerance sees a cross-row mix-up
    with pytest.raises(_capi.PnpiError, match="max_unet_rows"):
        bld.edit_images(images + images[:1], masks + masks[:1], prompts + prompts[:1], side, side, 10, GS, noise=noise + noise[:1])
    with pytest.raises(ValueError, match="context's 128 x 128"):
        bld.edit_image(images[0], masks[0], prompts[:1], noise=noise[0])                     # the reference's default 512 x 512
