"""InstructDiffusion host side (no GPU): the eager step against the run recorded from the reference's own CFGDenoiser and ldm UNetModel
(tests/golden/e2e_instdiff_tiny.npz, tools/make_golden_instructdiffusion.py), the combine told apart from InstructPix2Pix's, the driver's CLI
and skip-if-exists decision, the CompVis checkpoint conversion with and without a `state_dict` wrapper, and the library's new entry points."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from pnpinversion_amd import _capi
from pnpinversion_amd import instructdiffusion as idf
from pnpinversion_amd import instructpix2pix as ip
from pnpinversion_amd.config import TINY16_IP2P

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_instdiff_tiny.npz"))
    assert float(g["cfg_text"]) == 5.0 and float(g["cfg_image"]) == 1.25 and int(g["nsteps"]) == 8
    return g


def replay(step, gold):
    """z after every step from the recorded eps rows and draws"""
    sigmas = torch.from_numpy(gold["sigmas"])
    n = int(gold["nsteps"])
    z, out = torch.from_numpy(gold["draw0"])[None] * sigmas[0], []
    for i in range(n):
        noise = torch.from_numpy(gold["draws"][i])[None] if i < n - 1 else torch.full_like(z, float("nan"))
        z = step(z, torch.from_numpy(gold["eps"][i])[None], noise, sigmas[i], sigmas[i + 1], float(gold["cfg_text"]), float(gold["cfg_image"]))
        out.append(z[0].numpy())
    return out


def test_the_shared_restatements_are_imported_not_copied():
    for name in ("SigmaSchedule", "step_table", "get_ancestral_step", "fit_size"):
        assert getattr(idf, name) is getattr(ip, name), name
    assert issubclass(idf.InstructDiffusion, ip.InstructPix2Pix)


def test_eager_step_reproduces_the_recorded_z_bit_for_bit(gold):
    """the reference's CFGDenoiser.forward combined the rows of ldm's UNetModel inside the restated sampler; the step restated in torch
    must land on the recorded z of every step"""
    assert gold["eps"].shape == (8, 3, 4, 16, 16) and gold["z"].shape == (8, 4, 16, 16) and gold["z"].dtype == np.float32
    assert np.array_equal(gold["sigmas"], ip.SigmaSchedule().get_sigmas(8).numpy())
    for i, z in enumerate(replay(idf.euler_ancestral_step, gold)):
        assert np.array_equal(z, gold["z"][i]), i


def test_the_instructpix2pix_step_gives_another_z(gold):
    """the same rows under InstructPix2Pix's combine: the fixture tells the two apart at every step, far above rounding"""
    for i, z in enumerate(replay(ip.euler_ancestral_step, gold)):
        d = np.linalg.norm(z - gold["z"][i]) / np.linalg.norm(gold["z"][i])
        assert d > 1e-3, (i, d)
    # and the third text row is the instruction, not the null text
    assert np.array_equal(gold["context"][2], gold["context"][0]) and not np.array_equal(gold["context"][1], gold["context"][0])


@pytest.mark.parametrize("i", [0, 25, 49])
def test_eager_step_against_numpy_fp32(i):
    """the reference's expression, every operation rounded to fp32 by numpy in its evaluation order, scalars from the table"""
    sched = ip.SigmaSchedule()
    sigmas = sched.get_sigmas(50)
    tab = ip.step_table(sigmas, sched)
    g = torch.Generator().manual_seed(i)
    z, eps = torch.randn(2, 4, 5, 7, generator=g) * sigmas[i], torch.randn(2, 3, 4, 5, 7, generator=g)
    noise = torch.randn(2, 4, 5, 7, generator=g)
    got = idf.euler_ancestral_step(z, eps, noise if i < 49 else torch.full_like(noise, float("nan")), sigmas[i], sigmas[i + 1], 5.0, 1.25).numpy()
    zn, en, s = z.numpy(), eps.numpy(), tab[i][0]
    den = [zn + en[:, k] * f32(-s) for k in range(3)]
    comb = (f32(0.5) * (den[1] + den[2]) + f32(5.0) * (den[0] - den[1])) + f32(1.25) * (den[0] - den[2])
    want = zn + ((zn - comb) / s) * tab[i][1]
    if tab[i][5]:
        want = want + noise.numpy() * tab[i][2]
    assert want.dtype == np.float32 and np.array_equal(got, want) and np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------- the driver
def load_script():
    spec = importlib.util.spec_from_file_location("pnpi_run_editing_instructdiffusion", os.path.join(ROOT, "run_editing_instructdiffusion.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_cli_method_folder_defaults_and_scales(capsys):
    script = load_script()
    d = script.parse_args([])
    # the reference's six arguments and their defaults (run_editing_instructdiffusion.py:140-146); --checkpoint is optional
    assert (d.rerun_exist_images, d.data_path, d.output_path) == (False, "data", "output")
    assert d.edit_category_list == [str(i) for i in range(10)] and d.edit_method_list == ["instruct-diffusion"]
    assert d.checkpoint == "data/checkpoints/v1-5-pruned-emaonly-adaption.ckpt"
    assert script.image_save_paths == {"instruct-diffusion": "instruct-diffusion"}
    assert (script.STEPS, script.CFG_TEXT, script.CFG_IMAGE) == (50, 5.0, 1.25)
    a = script.parse_args(["--synthetic_weights", "--checkpoint", "x.ckpt", "--model_config", "small64"])
    assert a.synthetic_weights and a.checkpoint == "x.ckpt" and a.model_config == "small64"
    for other in ("instruct-pix2pix", "directinversion+p2p"):
        with pytest.raises(SystemExit):
            script.parse_args(["--edit_method_list", other])
    with pytest.raises(SystemExit, match="does not exist"):
        script.load_weights(script.parse_args(["--checkpoint", "/nonexistent.ckpt"]), TINY16_IP2P)
    with pytest.raises(SystemExit):
        script.parse_args(["--help"])
    text = capsys.readouterr().out
    for flag in ("--rerun_exist_images", "--data_path", "--output_path", "--edit_category_list", "--edit_method_list", "--checkpoint",
                 "--checkpoint_dir", "--synthetic_weights", "--model_config", "--tokenizer_dir"):
        assert flag in text, flag
    # the editor's own defaults are the reference's (:90)
    import inspect
    for fn in (idf.InstructDiffusion.edit, idf.InstructDiffusion.edit_images):
        p = inspect.signature(fn).parameters
        assert (p["steps"].default, p["cfg_text"].default, p["cfg_image"].default) == (50, 5.0, 1.25)


def test_work_plan_skips_existing_and_shards(tmp_path):
    script = load_script()
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    items = {"%03d" % i: {"editing_type_id": str(i % 3), "editing_instruction": "make it %d" % i, "editing_prompt": "a [red] bird",
                          "original_prompt": "a bird", "image_path": "c%d/%03d.jpg" % (i % 3, i), "mask": [5, 3], "blended_word": ""}
             for i in range(9)}
    args = script.parse_args(["--data_path", data, "--output_path", out, "--edit_category_list", "0", "1"])
    log = []
    whole = script.plan_work(args, items, "instruct-diffusion", 0, 1, log.append)
    assert [w[0] for w in whole] == ["make it %d" % i for i in (0, 1, 3, 4, 6, 7)] and not log
    assert whole[1][1] == os.path.join(data + "/annotation_images", "c1/001.jpg")
    assert whole[1][2] == os.path.join(out, "instruct-diffusion", "annotation_images", "c1/001.jpg")
    assert script.plan_work(args, items, "instruct-diffusion", 0, 2, log.append) == whole[0::2]
    assert script.plan_work(args, items, "instruct-diffusion", 1, 2, log.append) == whole[1::2]
    os.makedirs(os.path.dirname(whole[2][2]))
    open(whole[2][2], "w").close()
    assert script.plan_work(args, items, "instruct-diffusion", 0, 1, log.append) == whole[:2] + whole[3:]
    assert log == ["skip image [%s] with [instruct-diffusion]" % whole[2][1]]
    args.rerun_exist_images = True
    assert script.plan_work(args, items, "instruct-diffusion", 0, 1, log.append) == whole


# ---------------------------------------------------------------------------------------------- CompVis checkpoint conversion
def test_convert_ldm_state_dict_returns_the_project_keys_with_and_without_the_wrapper(gold, tmp_path):
    """the ldm-layout state dict rebuilt from the (ldm key, project key) pairs that the reference's InstructDiffusion UNetModel, Encoder
    and Decoder accepted with strict=True, saved as the two forms load_model_from_config (:50-60) accepts"""
    from pnpinversion_amd import weights
    from pnpinversion_amd.checkpoint import convert_ldm_state_dict, load_ldm_checkpoint
    seed = int(gold["weight_seed"])
    usd, vsd, csd = (f(TINY16_IP2P, seed) for f in (weights.unet_state_dict, weights.vae_state_dict, weights.clip_state_dict))
    sd = {"model.diffusion_model." + str(n): usd[str(k)] for n, k in zip(gold["unet_ldm_keys"], gold["unet_src_keys"])}
    for n, k in zip(gold["vae_ldm_keys"], gold["vae_src_keys"]):
        n, w = str(n), vsd[str(k)]
        sd["first_stage_model." + n] = w[:, :, None, None] if ".mid.attn_1." in n and w.dim() == 2 else w
    for k, v in csd.items():
        sd["cond_stage_model.transformer.text_model." + k] = v
    assert len(set(gold["unet_ldm_keys"].tolist())) == len(usd) and len(gold["vae_ldm_keys"]) == len(vsd)
    torch.save(sd, tmp_path / "bare.ckpt")
    torch.save({"state_dict": sd, "global_step": 7}, tmp_path / "wrapped.ckpt")
    for got in (convert_ldm_state_dict(sd), load_ldm_checkpoint(str(tmp_path / "bare.ckpt")), load_ldm_checkpoint(str(tmp_path / "wrapped.ckpt"))):
        for have, want in zip(got, (usd, vsd, csd)):
            assert set(have) == set(want)
            for k in want:
                assert have[k].shape == want[k].shape and torch.equal(have[k], want[k]), k
        assert got[0]["conv_in.weight"].shape[1] == 8


def test_library_exports_the_new_entry_points():
    lib = _capi.load_library()
    for name in ("pnpi_instdiff_step", "pnpi_instdiff_edit"):
        assert name in _capi.SYMBOLS and hasattr(lib, name)
    assert _capi.SYMBOLS["pnpi_instdiff_step"] == _capi.SYMBOLS["pnpi_ip2p_step"] and _capi.SYMBOLS["pnpi_instdiff_edit"] == _capi.SYMBOLS["pnpi_ip2p_edit"]
    # NULL context: refused, nothing dereferenced
    assert lib.pnpi_instdiff_edit(None, None, None, None, 1, None, 5.0, 1.25, 8, None, None, None) == _capi.PNPI_EINVAL
    assert lib.pnpi_instdiff_step(None, None, None, None, None, 1, 16, 5.0, 1.25, None, 1.0, None, None) == _capi.PNPI_EINVAL
