"""InstructPix2Pix host side (no GPU): the restated k-diffusion schedule, its inverse and the eager step against the run recorded from
the reference's own ldm modules (tests/golden/e2e_ip2p_tiny.npz, tools/make_golden_ip2p.py), checkpoint.convert_ldm_state_dict against what
ldm's UNetModel / Encoder / Decoder accepted and computed, the driver's CLI and work plan, the 8-channel configurations and the new entry
points of the library."""
import os

import numpy as np
import pytest
import torch

from pnpinversion_amd import _capi
from pnpinversion_amd import instructpix2pix as ip
from pnpinversion_amd.config import SD1, SD1_IP2P, SMALL64, SMALL64_IP2P, TINY16, TINY16_IP2P

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "e2e_ip2p_tiny.npz"))


@pytest.fixture(scope="module")
def sched():
    return ip.SigmaSchedule()


def test_alphas_cumprod_is_ldm_linear_schedule():
    ac = ip.ldm_alphas_cumprod()
    assert ac.dtype == torch.float32 and ac.shape == (1000,)
    betas = np.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=np.float64) ** 2
    assert np.allclose(ac.numpy(), np.cumprod(1 - betas), rtol=1e-6, atol=0)
    assert abs(float(ac[0]) - 0.99915) < 1e-6 and abs(float(ac[-1]) - 0.0046602) < 1e-6


def test_get_sigmas_and_fractional_timesteps(sched):
    sigmas = sched.get_sigmas(50)
    assert sigmas.shape == (51,) and sigmas.dtype == torch.float32 and sigmas[-1] == 0
    assert torch.equal(sigmas[0], sched.log_sigmas[999].exp()) and torch.equal(sigmas[49], sched.log_sigmas[0].exp())    # linspace(999, 0, 50) ends on integers
    assert (sigmas[:-1][1:] < sigmas[:-1][:-1]).all()
    t = sched.sigma_to_t(sigmas[:-1])
    want = torch.linspace(999, 0, 50)
    assert (t - want).abs().max() < 2e-3                                                              # coarse sanity; the bits: the recorded run below
    assert all(float(x) != round(float(x)) for x in t[1:-1])                                           # every interior timestep is fractional
    assert (t >= 0).all() and (t <= 999).all()


def test_sigma_to_t_inverts_t_to_sigma_at_integers(sched, gold):
    k = torch.arange(1000)
    back = sched.sigma_to_t(sched.t_to_sigma(k.float()))
    assert torch.equal(back, k.float())                              # exactly: the interpolation weight left by log(exp(x)) rounds away
    assert np.array_equal(back.numpy(), gold["roundtrip_k"])
    # below the first and above the last sigma the timestep is clamped to the table
    assert float(sched.sigma_to_t(sched.sigmas[:1] * 0.5)) == 0.0 and float(sched.sigma_to_t(sched.sigmas[-1:] * 2)) == 999.0


def test_schedule_bit_equal_to_the_recorded_run(sched, gold):
    for n, sk, tk in ((50, "sigmas50", "timesteps50"), (int(gold["nsteps"]), "sigmas", "timesteps")):
        sigmas = sched.get_sigmas(n)
        assert np.array_equal(sigmas.numpy(), gold[sk]) and gold[sk].dtype == np.float32 and gold[sk].shape == (n + 1,)
        t = sched.sigma_to_t(sigmas[:-1]).numpy()
        assert np.array_equal(t, gold[tk])
        assert all(float(x) != round(float(x)) for x in gold[tk][1:-1])      # every interior timestep is non-integer
        assert gold[tk][0] == 999 and gold[tk][-1] == 0
        assert np.array_equal(ip.step_table(sigmas, sched)[:, 4], gold[tk])


def test_eager_step_reproduces_the_recorded_z_bit_for_bit(sched, gold):
    """the reference's ldm UNetModel produced eps; the step restated in torch must land on the recorded z of every step"""
    sigmas = torch.from_numpy(gold["sigmas"])
    n = int(gold["nsteps"])
    z = torch.from_numpy(gold["draw0"])[None] * sigmas[0]
    for i in range(n):
        noise = torch.from_numpy(gold["draws"][i])[None] if i < n - 1 else torch.full_like(z, float("nan"))
        z = ip.euler_ancestral_step(z, torch.from_numpy(gold["eps"][i])[None], noise, sigmas[i], sigmas[i + 1], float(gold["cfg_text"]),
                                    float(gold["cfg_image"]))
        assert np.array_equal(z[0].numpy(), gold["z"][i]), i


# ---------------------------------------------------------------------------------------------- CompVis checkpoint conversion
def ldm_state_dict(gold):
    """the CompVis-layout state dict the fixture's ldm modules were loaded from: this project's seeded weights under the (ldm key, source
    key) pairs that ldm's strict load accepted, plus what a training checkpoint carries besides"""
    from pnpinversion_amd import weights
    seed = int(gold["weight_seed"])
    usd, vsd, csd = weights.unet_state_dict(TINY16_IP2P, seed), weights.vae_state_dict(TINY16_IP2P, seed), weights.clip_state_dict(TINY16_IP2P, seed)
    sd = {"model.diffusion_model." + str(n): usd[str(k)] for n, k in zip(gold["unet_ldm_keys"], gold["unet_src_keys"])}
    for n, k in zip(gold["vae_ldm_keys"], gold["vae_src_keys"]):
        n, w = str(n), vsd[str(k)]
        sd["first_stage_model." + n] = w[:, :, None, None] if ".mid.attn_1." in n and w.dim() == 2 else w
    for k, v in csd.items():
        sd["cond_stage_model.transformer.text_model." + k] = v
    sd["cond_stage_model.transformer.text_model.embeddings.position_ids"] = torch.arange(77)[None]
    sd["model_ema.decay"], sd["alphas_cumprod"] = torch.tensor(0.9999), torch.zeros(1000)
    return sd, usd, vsd, csd


def test_convert_ldm_state_dict_consumes_every_key_and_matches_the_reference_modules(gold):
    from oracle import sd_oracle
    from pnpinversion_amd.checkpoint import convert_ldm_state_dict
    sd, usd, vsd, csd = ldm_state_dict(gold)
    assert len(gold["unet_ldm_keys"]) == len(set(gold["unet_ldm_keys"].tolist())) == len(usd)
    assert len(gold["vae_ldm_keys"]) == len(vsd)
    u, v, c = convert_ldm_state_dict(sd)
    # every key consumed, none missing, one to one
    assert set(u) == set(usd) and set(v) == set(vsd) and set(c) == set(csd)
    assert len(u) + len(v) + len(c) == len(sd) - 3                              # position_ids and the two non-model entries are left alone
    for got, want in ((u, usd), (v, vsd), (c, csd)):
        for k in want:
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    assert u["conv_in.weight"].shape[1] == 8
    with pytest.raises(KeyError):
        convert_ldm_state_dict({"model.diffusion_model.input_blocks.1.0.in_layers.1.weight": torch.zeros(1)})
    # the converted weights in the oracle's UNet against the reference UNetModel's eps: fractional t, 8 real input channels
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()      # noqa: E731
    t8, ctx = float(gold["t8"]), torch.from_numpy(gold["context"])
    assert t8 != round(t8)
    with torch.no_grad():
        got = sd_oracle.unet_forward({k: w.float() for k, w in u.items()}, TINY16_IP2P, torch.from_numpy(gold["lat8"]), t8, ctx)
    r = rel(got, torch.from_numpy(gold["eps8"]))
    print("converted UNet in the oracle against ldm's UNetModel at t = %.4f: rel-L2 %.3g" % (t8, r))
    assert r < 1e-5, r
    # the same for the VAE Encoder / Decoder
    vf = {k: w.float() for k, w in v.items()}
    x = (2 * torch.tensor(gold["image"]).float() / 255 - 1).permute(2, 0, 1)[None]
    with torch.no_grad():
        mean = sd_oracle.vae_encode_mean(vf, TINY16_IP2P, x)
        dec = sd_oracle.vae_decode(vf, TINY16_IP2P, 1. / 0.18215 * torch.from_numpy(gold["z"][-1])[None])
    r_e, r_d = rel(mean, torch.from_numpy(gold["c_concat"])), rel(dec[0], torch.from_numpy(gold["decoded"]))
    print("converted VAE in the oracle against ldm's Encoder / Decoder: rel-L2 %.3g / %.3g" % (r_e, r_d))
    assert r_e < 1e-5 and r_d < 1e-5, (r_e, r_d)


# ---------------------------------------------------------------------------------------------- the driver
def load_script():
    import importlib.util
    spec = importlib.util.spec_from_file_location("pnpi_run_editing_instructpix2pix", os.path.join(ROOT, "run_editing_instructpix2pix.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_flags_and_defaults(capsys):
    script = load_script()
    d = script.parse_args([])
    # the reference's six arguments and their defaults (run_editing_instructpix2pix.py:153-160)
    assert (d.rerun_exist_images, d.data_path, d.output_path) == (False, "data", "output")
    assert d.edit_category_list == [str(i) for i in range(10)] and d.edit_method_list == ["instruct-pix2pix"]
    assert d.checkpoint == "data/checkpoints/instruct-pix2pix-00-22000.ckpt"
    assert (script.STEPS, script.CFG_TEXT, script.CFG_IMAGE) == (50, 7.5, 1.5)
    assert script.image_save_paths["instruct-pix2pix"] == "instruct-pix2pix"
    a = script.parse_args(["--edit_method_list", "instruct-diffusion", "--synthetic_weights", "--checkpoint", "x.ckpt"])
    assert a.edit_method_list == ["instruct-diffusion"] and a.synthetic_weights and a.checkpoint == "x.ckpt"
    with pytest.raises(SystemExit):
        script.parse_args(["--edit_method_list", "directinversion+p2p"])
    with pytest.raises(SystemExit, match="does not exist"):
        script.load_weights(script.parse_args(["--checkpoint", "/nonexistent.ckpt"]), TINY16_IP2P)
    with pytest.raises(SystemExit):
        script.parse_args(["--help"])
    text = capsys.readouterr().out
    for flag in ("--rerun_exist_images", "--data_path", "--output_path", "--edit_category_list", "--edit_method_list", "--checkpoint",
                 "--checkpoint_dir", "--synthetic_weights", "--model_config", "--tokenizer_dir"):
        assert flag in text, flag
    import inspect
    assert "setup_seed()" in inspect.getsource(script.main)


def test_work_plan_shards_and_skips_existing(tmp_path):
    script = load_script()
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    items = {"%03d" % i: {"editing_type_id": str(i % 3), "editing_instruction": "make it %d" % i, "editing_prompt": "a [red] bird",
                          "original_prompt": "a bird", "image_path": "c%d/%03d.jpg" % (i % 3, i), "mask": [5, 3], "blended_word": ""}
             for i in range(9)}
    args = script.parse_args(["--data_path", data, "--output_path", out, "--edit_category_list", "0", "1"])
    log = []
    whole = script.plan_work(args, items, "instruct-pix2pix", 0, 1, log.append)
    assert [w[0] for w in whole] == ["make it %d" % i for i in (0, 1, 3, 4, 6, 7)] and not log
    assert whole[1][1] == os.path.join(data + "/annotation_images", "c1/001.jpg")
    assert whole[1][2] == os.path.join(out, "instruct-pix2pix", "annotation_images", "c1/001.jpg")
    r0, r1 = script.plan_work(args, items, "instruct-pix2pix", 0, 2, log.append), script.plan_work(args, items, "instruct-pix2pix", 1, 2, log.append)
    assert r0 == whole[0::2] and r1 == whole[1::2]
    os.makedirs(os.path.dirname(whole[2][2]))
    open(whole[2][2], "w").close()
    assert script.plan_work(args, items, "instruct-pix2pix", 0, 1, log.append) == whole[:2] + whole[3:]
    assert log == ["skip image [%s] with [instruct-pix2pix]" % whole[2][1]]
    args.rerun_exist_images = True
    assert script.plan_work(args, items, "instruct-pix2pix", 0, 1, log.append) == whole
    assert script.plan_work(args, items, "instruct-diffusion", 0, 1, log.append)[0][2].startswith(os.path.join(out, "instruct-diffusion"))


def test_step_table_is_the_reference_expressions(sched):
    sigmas = sched.get_sigmas(50)
    tab = ip.step_table(sigmas, sched)
    assert tab.shape == (50, 6) and tab.dtype == np.float32
    t = sched.sigma_to_t(sigmas[:-1]).numpy()
    for i in range(50):
        s, s1 = sigmas[i], sigmas[i + 1]
        up = min(s1, (s1 ** 2 * (s ** 2 - s1 ** 2) / s ** 2) ** 0.5)
        down = (s1 ** 2 - up ** 2) ** 0.5
        assert tab[i][0] == s.item() and tab[i][1] == (down - s).item() and tab[i][2] == up.item()
        assert tab[i][3] == (1 / (s ** 2 + 1) ** 0.5).item() and tab[i][4] == t[i] and tab[i][5] == float(i < 49)
        assert 0 < up <= s1 or i == 49
    assert tab[49][2] == 0 and tab[49][1] == -tab[49][0]                                               # sigma_next = 0: up = down = 0
    assert np.array_equal(ip.step_table(sigmas[:4], sched), tab[:3])


@pytest.mark.parametrize("i", [0, 25, 49])
def test_eager_step_against_numpy_fp32(sched, i):
    """the same expressions, every operation rounded to fp32 by numpy, scalars from the table"""
    sigmas = sched.get_sigmas(50)
    tab = ip.step_table(sigmas, sched)
    g = torch.Generator().manual_seed(i)
    z, eps = torch.randn(2, 4, 5, 7, generator=g) * sigmas[i], torch.randn(2, 3, 4, 5, 7, generator=g)
    noise = torch.randn(2, 4, 5, 7, generator=g)
    got = ip.euler_ancestral_step(z, eps, noise if i < 49 else torch.full_like(noise, float("nan")), sigmas[i], sigmas[i + 1], 7.5, 1.5).numpy()
    zn, en, s = z.numpy(), eps.numpy(), tab[i][0]
    den = [zn + en[:, k] * f32(-s) for k in range(3)]
    comb = (den[2] + f32(7.5) * (den[0] - den[1])) + f32(1.5) * (den[1] - den[2])
    want = zn + ((zn - comb) / s) * tab[i][1]
    if tab[i][5]:
        want = want + noise.numpy() * tab[i][2]
    assert want.dtype == np.float32 and np.array_equal(got, want)
    assert np.isfinite(got).all()


def test_fit_size_is_the_reference_arithmetic():
    assert ip.fit_size(512, 512) == (512, 512) and ip.fit_size(1024, 768) == (512, 384) and ip.fit_size(500, 333) == (576, 384)
    assert ip.fit_size(300, 300, resolution=128) == (128, 128)


def test_eight_channel_configurations():
    for base, cfg in ((SD1, SD1_IP2P), (TINY16, TINY16_IP2P), (SMALL64, SMALL64_IP2P)):
        assert cfg.in_channels == 8 and cfg.out_channels == 4
        assert cfg == type(base)(**dict(base.__dict__, in_channels=8))
        assert cfg.to_c().in_channels == 8
    assert SMALL64_IP2P.sample_size == 64 and SMALL64_IP2P.block_has_attn[0] == 1


def test_library_exports_the_new_entry_points():
    lib = _capi.load_library()
    for name in ("pnpi_ip2p_step", "pnpi_ip2p_edit", "pnpi_unet_forward_t"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
    # NULL context: refused, nothing dereferenced
    assert lib.pnpi_ip2p_edit(None, None, None, None, 1, None, 7.5, 1.5, 8, None, None, None) == _capi.PNPI_EINVAL
    assert lib.pnpi_ip2p_step(None, None, None, None, None, 1, 16, 7.5, 1.5, None, 1.0, None, None) == _capi.PNPI_EINVAL
    assert lib.pnpi_unet_forward_t(None, None, 1, 1.5, None, None) == _capi.PNPI_EINVAL
