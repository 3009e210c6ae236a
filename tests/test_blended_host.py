"""Host side of the Blended Latent Diffusion editor (no GPU): the mask rule against masks the reference's own mask_decode + _read_mask
produced (tests/golden/blended_mask_cases.npz, tools/make_golden_blended.py), the timestep slice, the script's CLI and work plan, and the
three C symbols."""
import json
import os
import re
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pnpinversion_amd import _capi  # noqa: E402
from pnpinversion_amd import blended_latent_diffusion as bl  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("pnpi_bld_mask", "pnpi_bld_step", "pnpi_bld_edit")


def load_script():
    """this repository's run_editing_blended_latent_diffusion.py (by path: the reference tree, when on sys.path, has a script of that name)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pnpi_run_editing_blended_latent_diffusion",
                                                  os.path.join(ROOT, "run_editing_blended_latent_diffusion.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def mask_cases():
    g = np.load(os.path.join(GOLD, "blended_mask_cases.npz"))
    return g, [str(n) for n in g["names"]]


def test_read_mask_and_host_rule_equal_reference():
    script = load_script()
    g, names = mask_cases()
    assert {int(g[n + "_side"]) for n in names} == {512, 128}
    bld = bl.BlendedLatnetDiffusion.__new__(bl.BlendedLatnetDiffusion)          # _read_mask needs no model
    for n in names:
        side, rle, want = int(g[n + "_side"]), g[n + "_rle"].tolist(), g[n + "_latent"]
        decoded = script.mask_decode(rle, (side, side))
        assert np.array_equal(np.uint8(decoded), g[n + "_mask_u8"]), n          # run script :22-38, :209
        pil = Image.fromarray(np.uint8(decoded[:, :, np.newaxis].repeat(3, 2))).convert("L")
        lat, org = bld._read_mask(pil, (side // 8, side // 8))
        assert org is pil and lat.shape == (1, 1, side // 8, side // 8) and lat.dtype.is_floating_point
        assert np.array_equal(lat[0, 0].numpy(), want), n
        assert np.array_equal(bl.host_mask(g[n + "_mask_u8"], (side // 8, side // 8)), want), n
        assert set(np.unique(want)) <= {0.0, 1.0}
    # the cases the fixture was built for: the border rows / columns are never sampled; pixel 8i+3 is not read, 8i+4 is
    assert g["empty_512_latent"].sum() == 0 and g["full_512_latent"].all() and g["empty_128_latent"].sum() == 0 and g["full_128_latent"].all()
    e = g["edge_512_latent"]
    assert e[20, 10] == 0 and e[19, 10] == 1 and e[12, 10] == 0 and e[13, 10] == 1         # rows 101 .. 163
    assert e[15, 5] == 1 and e[15, 4] == 0 and e[15, 40] == 1 and e[15, 41] == 0           # columns 44 .. 324
    assert np.array_equal(bl.nearest_source_index(64, 512), 8 * np.arange(64) + 4)
    assert bld._read_mask(pil)[0].shape == (1, 1, 64, 64)                                   # the reference's default dest_size


@pytest.mark.parametrize("n,p,first,count", [(50, 0.25, 740, 38), (10, 0.25, 700, 8), (50, 0, 980, 50), (3, 0.9, 0, 1)])
def test_timestep_slice(n, p, first, count):
    from pnpinversion_amd.p2p.scheduler_dev import DDIMSchedulerDev
    s = DDIMSchedulerDev(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    s.set_timesteps(n)
    got = [int(t) for t in bl.timestep_slice(s.timesteps, p)]
    want = [int(t) for t in s.timesteps[int(len(s.timesteps) * p):]]             # run script :110-112
    assert got == want and len(got) == count and got[0] == first and got[-1] == 0
    assert got == list(range(first, -1, -(1000 // n)))


def test_cli_flags_and_defaults(capsys):
    script = load_script()
    a = script.parse_args(["--data_path", "d", "--output_path", "o", "--edit_category_list", "0", "3", "--rerun_exist_images",
                           "--synthetic_weights"])
    assert a.data_path == "d" and a.output_path == "o" and a.edit_category_list == ["0", "3"] and a.rerun_exist_images
    assert a.edit_method_list == ["blended-latent-diffusion"] and a.batch_size == 1 and a.model_config == "sd1"
    d = script.parse_args([])
    assert (d.data_path, d.output_path, d.rerun_exist_images) == ("data", "output", False)
    assert d.edit_category_list == [str(i) for i in range(10)]
    assert script.image_save_paths == {"blended-latent-diffusion": "blended-latent-diffusion"}
    assert (script.NUM_INFERENCE_STEPS, script.BLENDING_PERCENTAGE, script.GUIDANCE_SCALE) == (50, 0.25, 7.5)
    with pytest.raises(SystemExit):
        script.parse_args(["--edit_method_list", "directinversion+p2p"])
    with pytest.raises(SystemExit):
        script.parse_args(["--batch_size", "0"])
    with pytest.raises(SystemExit):
        script.parse_args(["--help"])
    text = capsys.readouterr().out
    for flag in ("--rerun_exist_images", "--data_path", "--output_path", "--edit_category_list", "--edit_method_list",       # the reference's five
                 "--batch_size", "--model_config", "--checkpoint_dir", "--synthetic_weights"):
        assert flag in text, flag


def test_work_plan_shards_and_skips_existing(tmp_path):
    """the sweep's dry run: category filter, round-robin sharding over the ranks, the reference's output path, skip-if-exists"""
    script = load_script()
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    items = {"%03d" % i: {"editing_type_id": str(i % 3), "editing_prompt": "a [red] bird %d" % i, "original_prompt": "a bird",
                          "image_path": "c%d/%03d.jpg" % (i % 3, i), "mask": [5, 3]} for i in range(9)}
    args = script.parse_args(["--data_path", data, "--output_path", out, "--edit_category_list", "0", "1"])
    log = []
    whole = script.plan_work(args, items, "blended-latent-diffusion", 0, 1, log.append)
    assert [w[3] is items[k] for w, k in zip(whole, ["000", "001", "003", "004", "006", "007"])] == [True] * 6 and not log
    assert whole[0][0] == "a red bird 0"
    assert whole[1][1] == os.path.join(data, "annotation_images", "c1/001.jpg")
    assert whole[1][2] == os.path.join(out, "blended-latent-diffusion", "annotation_images", "c1/001.jpg")
    r0 = script.plan_work(args, items, "blended-latent-diffusion", 0, 2, log.append)
    r1 = script.plan_work(args, items, "blended-latent-diffusion", 1, 2, log.append)
    assert r0 == whole[0::2] and r1 == whole[1::2]
    os.makedirs(os.path.dirname(whole[2][2]))
    open(whole[2][2], "w").close()
    again = script.plan_work(args, items, "blended-latent-diffusion", 0, 1, log.append)
    assert again == whole[:2] + whole[3:] and log == ["skip image [%s] with [blended-latent-diffusion]" % whole[2][1]]
    args.rerun_exist_images = True
    assert script.plan_work(args, items, "blended-latent-diffusion", 0, 1, log.append) == whole
    m = script.item_mask({"mask": [512 * 100 + 7, 30]})
    assert m.mode == "L" and m.size == (512, 512) and np.array(m).max() == 1 and np.array(m)[100, 7:37].all() and np.array(m)[100, 37] == 0


def test_symbols_in_header_library_and_binding():
    hdr = open(os.path.join(ROOT, "include", "pnpi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _capi.load_library()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert hasattr(lib, s), s
        assert s in _capi.SYMBOLS and s in doc, s
    # argument counts of the binding = the header's declarations (the context is the first argument)
    for s in SYMBOLS:
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, hdr, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_capi.SYMBOLS[s][1]), s


def test_generator_size_and_prompt_refusals():
    """checked before anything touches the device"""
    import torch
    bld = bl.BlendedLatnetDiffusion.__new__(bl.BlendedLatnetDiffusion)
    with pytest.raises(ValueError, match="global generator"):
        bld.edit_image("x.png", None, ["a"], generator=torch.Generator().manual_seed(42))
    with pytest.raises(ValueError, match="ONE prompt"):
        bld.edit_image("x.png", None, ["a", "b"])
    with pytest.raises(ValueError, match="pipe="):
        bl.BlendedLatnetDiffusion()
    fixture = json.dumps(sorted(np.load(os.path.join(GOLD, "e2e_blended_tiny.npz")).files))
    for key in ("draw_start", "draws_blend", "latents_steps", "latent_final", "edited", "mask_u8", "mask_latent", "source_latent", "prompt_ids"):
        assert key in fixture, key
