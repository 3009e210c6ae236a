"""Host logic of Plug-and-Play editing (no GPU): the injection schedule and sites against the constants tools/make_golden_pnp.py recorded
from the reference's own init_pnp / register functions (tests/golden/pnp_host.json), the two source-list indexings, the CLI surface of
run_editing_pnp.py and the descriptor's ctypes layout."""
import ctypes as C
import json
import os

import pytest
import torch

import run_editing_pnp as cli          # at collection: tests that load the reference tree put its scripts of the same name first on sys.path
from pnpinversion_amd import _capi
from pnpinversion_amd.config import SD1, SMALL64, TINY16
from pnpinversion_amd.engine import pnp_desc_default
from pnpinversion_amd.p2p.scheduler_dev import DDIMSchedulerDev
from pnpinversion_amd.pnp import NEGATIVE_PROMPT, injection_counts, source_list

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(GOLD, "pnp_host.json")) as f:
        return json.load(f)


def test_descriptor_layout_matches_the_library():
    lib = _capi.load_library()
    assert C.sizeof(_capi.PnpDesc) == lib.pnpi_pnp_desc_sizeof() == 20
    d = _capi.PnpDesc.make(3, 2, 4, 0xFF00)
    assert (d.struct_size, d.conv_steps, d.qk_steps, d.conv_site, d.qk_block_mask) == (20, 3, 2, 4, 0xFF00)
    assert [n for n, _ in _capi.PnpDesc._fields_] == ["struct_size", "conv_steps", "qk_steps", "conv_site", "qk_block_mask"]


@pytest.mark.parametrize("cfg", [SD1, SMALL64, TINY16], ids=["sd1", "small64", "tiny16"])
def test_default_sites_and_schedule_are_the_references(ref, cfg):
    """40 conv and 25 q/k steps of 50; transformer blocks 8 .. 15 and decoder ResNet 4 (up_blocks[1].resnets[1]) -- derived from the block
    layout, so the reduced test configurations (same layout) get the same sites"""
    lib = _capi.load_library()
    n = ref["num_ddim_steps"]
    d = pnp_desc_default(lib, cfg, n)
    assert n == 50 and d.struct_size == C.sizeof(_capi.PnpDesc)
    assert d.conv_steps == len(ref["conv_injection_timesteps"]) == 40
    assert d.qk_steps == len(ref["qk_injection_timesteps"]) == 25
    assert (d.conv_steps, d.qk_steps) == injection_counts(n)
    assert [b for b in range(32) if (d.qk_block_mask >> b) & 1] == ref["qk_blocks"] == list(range(8, 16))
    assert [d.conv_site] == ref["conv_site_decoder_resnet"] == [1 * ref["resnets_per_up_block"] + 1]


def test_default_sites_follow_the_structure_not_sd1_indices():
    """a model whose first TWO decoder levels have no attention: the sites move with the first level that has it"""
    import dataclasses
    lib = _capi.load_library()
    cfg = dataclasses.replace(SD1, block_has_attn=(1, 1, 0, 0))
    d = pnp_desc_default(lib, cfg, 10)
    # transformer blocks: down 0 .. 3, mid 4, up 5 .. 10; the first decoder level with attention is up block 2 -> its first block (5) is left out
    assert [b for b in range(32) if (d.qk_block_mask >> b) & 1] == [6, 7, 8, 9, 10]
    assert d.conv_site == 2 * 3 + 1 and (d.conv_steps, d.qk_steps) == (8, 5)
    none = dataclasses.replace(SD1, block_has_attn=(0, 0, 0, 0))
    with pytest.raises(_capi.PnpiError):
        pnp_desc_default(lib, none, 10)
    with pytest.raises(_capi.PnpiError):
        pnp_desc_default(lib, SD1, 0)


def test_injection_timesteps_are_the_leading_ones(ref):
    """scheduler.timesteps[:n] on the steps_offset = 1 schedule 981, 961, .., 1"""
    s = DDIMSchedulerDev(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False,
                         steps_offset=1)
    s.set_timesteps(50)
    ts = [int(t) for t in s.timesteps]
    assert ts == ref["timesteps"] and ts[0] == 981 and ts[-1] == 1
    assert ts[:40] == ref["conv_injection_timesteps"] and ts[:25] == ref["qk_injection_timesteps"]
    assert float(s.final_alpha_cumprod) == float(s.alphas_cumprod[0])


def test_source_list_indexings():
    """directinversion+pnp: 51 inversion latents (level 0 .. 50), step i reads level 50 - i and starts from level 50.
    ddim+pnp: 50 reconstruction latents (after sampling step 0 .. 49), reversed; step i reads the one after sampling step i and the start
    latent is the one after the FIRST sampling step."""
    n = 50
    inv = [torch.full((1,), float(k)) for k in range(n + 1)]
    src, start = source_list(inv, n)
    assert [int(s) for s in src] == list(range(50, 0, -1)) and int(start) == 50
    recon = [torch.full((1,), float(k)) for k in range(n)]          # value k = after sampling step k
    rev = list(reversed(recon))
    src, start = source_list(rev, n)
    assert [int(s) for s in src] == list(range(0, 50)) and int(start) == 0
    with pytest.raises(ValueError):
        source_list(rev[:10], n)


def test_cli_surface_and_skip_if_exists(ref, tmp_path):
    assert cli.image_save_paths == ref["image_save_paths"] == {"ddim+pnp": "ddim+pnp", "directinversion+pnp": "directinversion+pnp"}
    assert cli.NUM_DDIM_STEPS == ref["num_ddim_steps"]
    assert NEGATIVE_PROMPT == "ugly, blurry, black, low res, unrealistic"
    a = cli.parse_args(["--synthetic_weights"])
    assert a.data_path == "data" and a.output_path == "output" and not a.rerun_exist_images
    assert a.edit_category_list == [str(i) for i in range(10)] and a.edit_method_list == ["ddim+pnp", "directinversion+pnp"]
    with pytest.raises(SystemExit):
        cli.parse_args(["--edit_method_list", "ddim+p2p"])
    data, out = tmp_path / "data", tmp_path / "out"
    instr = {"0": dict(editing_type_id="0", original_prompt="a [cat]", editing_prompt="a [dog]", image_path="0_x/a.jpg"),
             "1": dict(editing_type_id="0", original_prompt="a bird", editing_prompt="a plane", image_path="0_x/b.jpg"),
             "2": dict(editing_type_id="7", original_prompt="p", editing_prompt="q", image_path="7_y/c.jpg")}
    a = cli.parse_args(["--data_path", str(data), "--output_path", str(out), "--edit_category_list", "0", "--synthetic_weights"])
    done = out / "ddim+pnp" / "annotation_images" / "0_x"
    done.mkdir(parents=True)
    (done / "a.jpg").write_bytes(b"x")
    log = []
    todo = cli.plan_work(a, instr, "ddim+pnp", log=log.append)
    assert [t[:2] for t in todo] == [("a bird", "a plane")] and len(log) == 1 and "skip image" in log[0]
    assert todo[0][3] == str(out / "ddim+pnp" / "annotation_images" / "0_x" / "b.jpg")
    todo = cli.plan_work(a, instr, "directinversion+pnp", log=log.append)
    assert [t[:2] for t in todo] == [("a cat", "a dog"), ("a bird", "a plane")]
    a.rerun_exist_images = True
    assert len(cli.plan_work(a, instr, "ddim+pnp", log=log.append)) == 2
    assert len(cli.plan_work(a, instr, "ddim+pnp", rank=1, world=2, log=log.append)) == 1
