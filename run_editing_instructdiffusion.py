#!/usr/bin/env python
"""PIE-Bench sweep driver with the CLI of the reference's run_editing_instructdiffusion.py (same six flags, method `instruct-diffusion`,
output folder `instruct-diffusion` and skip-if-exists resume): InstructDiffusion, the benchmark's second instruction-driven editor, on
NativePipeline with the 8-channel UNet (config.SD1_IP2P).  The sweep itself (work plan, rank sharding, weight flags, setup_seed() before
every image) is run_editing_instructpix2pix.py's, called with this editor and its scales.

Per image (run_editing_instructdiffusion.py:167-197): the mapping file's `editing_instruction`, 50 Euler-ancestral steps, text scale 5.0,
image scale 1.25; panel instruction | source | black | edit.  Weights: --checkpoint <CompVis .ckpt>, with or without a top-level
`state_dict` key as the reference's load_model_from_config accepts (checkpoint.convert_ldm_state_dict; the vocabulary then comes from
--tokenizer_dir), or --checkpoint_dir <diffusers directory>, or --synthetic_weights.  The reference declares --checkpoint with
`require=True`, a misspelt keyword that makes its own parser raise; here the flag is optional and has the reference's default."""
import argparse
import importlib.util
import os

from pnpinversion_amd import sweep


def _sibling(name):
    """the script of that name next to this one, whatever else of the same name is on sys.path"""
    spec = importlib.util.spec_from_file_location("pnpi_" + name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


ip2p = _sibling("run_editing_instructpix2pix")

image_save_paths = {
    "instruct-diffusion": "instruct-diffusion",
}
DEFAULT_CHECKPOINT = "data/checkpoints/v1-5-pruned-emaonly-adaption.ckpt"
STEPS, CFG_TEXT, CFG_IMAGE = 50, 5.0, 1.25
assert all(ip2p.image_save_paths[m] == folder for m, folder in image_save_paths.items())       # the shared work plan writes to these folders
plan_work, load_weights = ip2p.plan_work, ip2p.load_weights


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    sweep.add_sweep_args(ap, ["instruct-diffusion"])
    ap.add_argument("--checkpoint", type=str, default=DEFAULT_CHECKPOINT, help="CompVis-layout .ckpt, as the reference loads it")
    ap.add_argument("--tokenizer_dir", type=str, default=None, help="vocab.json / merges.txt for --checkpoint (a .ckpt holds no vocabulary)")
    args = ap.parse_args(argv)
    sweep.check_methods(ap, args, image_save_paths)
    return args


def main(argv=None):
    ip2p.main(argv, parse=parse_args, editor_name="InstructDiffusion", scales=(STEPS, CFG_TEXT, CFG_IMAGE))


if __name__ == "__main__":
    main()
