#!/usr/bin/env python
"""PIE-Bench sweep driver with the CLI of the reference's run_editing_instructpix2pix.py (same six flags, output folder `instruct-pix2pix`
and skip-if-exists resume): InstructPix2Pix, the benchmark's instruction-driven editor, on NativePipeline with the 8-channel UNet
(config.SD1_IP2P).  Weight / model-config flags and rank sharding as run_editing_p2p.py.

Per image (run_editing_instructpix2pix.py:177-205): the mapping file's `editing_instruction`, 50 Euler-ancestral steps, text scale 7.5,
image scale 1.5, setup_seed() before every image; panel instruction | source | black | edit.  Weights: --checkpoint <CompVis .ckpt> as the
reference loads it (checkpoint.convert_ldm_state_dict; the vocabulary then comes from --tokenizer_dir), or --checkpoint_dir <diffusers
directory>, or --synthetic_weights.  `--edit_method_list instruct-diffusion` here still means THIS editor's loop, rows and scales on another
checkpoint, written to the folder `instruct-diffusion`; InstructDiffusion's own rows, combine and scales are run_editing_instructdiffusion.py."""
import argparse
import os

from pnpinversion_amd import sweep
from pnpinversion_amd.checkpoint import resolve_weights
from pnpinversion_amd.sweep import setup_seed

image_save_paths = {
    "instruct-pix2pix": "instruct-pix2pix",
    "instruct-diffusion": "instruct-diffusion",
}
DEFAULT_CHECKPOINT = "data/checkpoints/instruct-pix2pix-00-22000.ckpt"
STEPS, CFG_TEXT, CFG_IMAGE = 50, 7.5, 1.5


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    sweep.add_sweep_args(ap, ["instruct-pix2pix"])
    ap.add_argument("--checkpoint", type=str, default=DEFAULT_CHECKPOINT, help="CompVis-layout .ckpt, as the reference loads it")
    ap.add_argument("--tokenizer_dir", type=str, default=None, help="vocab.json / merges.txt for --checkpoint (a .ckpt holds no vocabulary)")
    args = ap.parse_args(argv)
    sweep.check_methods(ap, args, image_save_paths)
    return args


def plan_work(args, instructions, method, rank=0, world=1, log=print):
    """This rank's share of the mapping file for `method`, without what is already on disk (:177-191 + round-robin sharding)
    -> [(editing_instruction, image_path, out_path)]"""
    return [(item["editing_instruction"], image_path, out_path)
            for item, image_path, out_path in sweep.plan(args, instructions, image_save_paths[method], rank, world, log, method)]


def load_weights(args, cfg, rank=0):
    """-> (unet_sd, vae_sd, clip_sd, tokenizer or None); --checkpoint_dir / --synthetic_weights as everywhere, else the reference's .ckpt"""
    if args.checkpoint_dir or args.synthetic_weights:
        return resolve_weights(args, cfg, rank)
    if not os.path.exists(args.checkpoint):
        raise SystemExit("no weights: %r does not exist; pass --checkpoint <CompVis .ckpt>, --checkpoint_dir <diffusers directory> or "
                         "--synthetic_weights" % args.checkpoint)
    if not args.tokenizer_dir:
        raise SystemExit("--checkpoint needs --tokenizer_dir <folder with vocab.json and merges.txt>")
    from pnpinversion_amd.checkpoint import load_ldm_checkpoint
    from pnpinversion_amd.text import ClipBPETokenizer
    tok = ClipBPETokenizer(os.path.join(args.tokenizer_dir, "vocab.json"), os.path.join(args.tokenizer_dir, "merges.txt"))
    return (*load_ldm_checkpoint(args.checkpoint), tok) if rank == 0 else (None, None, None, tok)


def main(argv=None, parse=parse_args, editor_name="InstructPix2Pix", scales=(STEPS, CFG_TEXT, CFG_IMAGE)):
    """parse / editor_name / scales: what run_editing_instructdiffusion.py, the same sweep around the other instruction editor, passes"""
    args = parse(argv)
    from pnpinversion_amd.config import SD1_IP2P, SMALL64_IP2P
    from pnpinversion_amd.instructdiffusion import InstructDiffusion
    from pnpinversion_amd.instructpix2pix import InstructPix2Pix
    from pnpinversion_amd.pipeline import NativePipeline
    make_pipeline = lambda cfg, device, tokenizer: NativePipeline(cfg, device=device, max_unet_rows=3, max_vae_images=1,       # noqa: E731
                                                                  text_encoder="native", tokenizer=tokenizer)
    with sweep.session(args, {"sd1": SD1_IP2P, "small64": SMALL64_IP2P}, make_pipeline, load_weights) as s:
        editor = {"InstructPix2Pix": InstructPix2Pix, "InstructDiffusion": InstructDiffusion}[editor_name](s.pipe)
        instructions = sweep.read_mapping(args)
        for method in args.edit_method_list:
            for instruction, image_path, out_path in plan_work(args, instructions, method, s.rank, s.world):
                print(f"editing image [{image_path}] with [{method}]")
                setup_seed()
                sweep.save_panel(editor.edit(image_path, instruction, *scales), out_path)


if __name__ == "__main__":
    main()
