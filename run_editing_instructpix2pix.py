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
import json
import os

import torch

from pnpinversion_amd.checkpoint import add_weight_args, resolve_weights
from pnpinversion_amd.distributed import broadcast_weights, prepare_env, shard_items
from run_editing_p2p import setup_seed

image_save_paths = {
    "instruct-pix2pix": "instruct-pix2pix",
    "instruct-diffusion": "instruct-diffusion",
}
DEFAULT_CHECKPOINT = "data/checkpoints/instruct-pix2pix-00-22000.ckpt"
STEPS, CFG_TEXT, CFG_IMAGE = 50, 7.5, 1.5


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rerun_exist_images", action="store_true")
    ap.add_argument("--data_path", type=str, default="data")
    ap.add_argument("--output_path", type=str, default="output")
    ap.add_argument("--edit_category_list", nargs="+", type=str, default=[str(i) for i in range(10)])
    ap.add_argument("--edit_method_list", nargs="+", type=str, default=["instruct-pix2pix"])
    ap.add_argument("--checkpoint", type=str, default=DEFAULT_CHECKPOINT, help="CompVis-layout .ckpt, as the reference loads it")
    ap.add_argument("--tokenizer_dir", type=str, default=None, help="vocab.json / merges.txt for --checkpoint (a .ckpt holds no vocabulary)")
    ap.add_argument("--model_config", choices=("sd1", "small64"), default="sd1", help="small64: reduced-width test configuration")
    add_weight_args(ap)
    args = ap.parse_args(argv)
    unknown = [m for m in args.edit_method_list if m not in image_save_paths]
    if unknown:
        ap.error("unknown edit method(s) %s; this script runs %s" % (unknown, list(image_save_paths)))
    return args


def plan_work(args, instructions, method, rank=0, world=1, log=print):
    """This rank's share of the mapping file for `method`, without what is already on disk (:177-191 + round-robin sharding)
    -> [(editing_instruction, image_path, out_path)]"""
    work = [(k, v) for k, v in instructions.items() if v["editing_type_id"] in args.edit_category_list]
    todo = []
    for key, item in shard_items(work, rank, world):
        image_path = os.path.join(f"{args.data_path}/annotation_images", item["image_path"])
        out_path = image_path.replace(args.data_path, os.path.join(args.output_path, image_save_paths[method]))
        if os.path.exists(out_path) and not args.rerun_exist_images:
            log(f"skip image [{image_path}] with [{method}]")
            continue
        todo.append((item["editing_instruction"], image_path, out_path))
    return todo


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
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    prepare_env()
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    from pnpinversion_amd.config import SD1_IP2P, SMALL64_IP2P
    from pnpinversion_amd.instructdiffusion import InstructDiffusion
    from pnpinversion_amd.instructpix2pix import InstructPix2Pix
    from pnpinversion_amd.pipeline import NativePipeline
    cfg = SD1_IP2P if args.model_config == "sd1" else SMALL64_IP2P
    unet_sd, vae_sd, clip_sd, tokenizer = load_weights(args, cfg, rank)
    pipe = NativePipeline(cfg, device="cuda:%d" % local_rank, max_unet_rows=3, max_vae_images=1, text_encoder="native", tokenizer=tokenizer)
    if rank == 0:
        pipe.load_state_dict(unet_sd, vae_sd, clip_sd=clip_sd)
    if world > 1:
        broadcast_weights(pipe.engine, src=0)
    editor = {"InstructPix2Pix": InstructPix2Pix, "InstructDiffusion": InstructDiffusion}[editor_name](pipe)

    with open(os.path.join(args.data_path, "mapping_file.json")) as f:
        instructions = json.load(f)
    for method in args.edit_method_list:
        for instruction, image_path, out_path in plan_work(args, instructions, method, rank, world):
            print(f"editing image [{image_path}] with [{method}]")
            setup_seed()
            edited_image = editor.edit(image_path, instruction, *scales)
            os.makedirs(os.path.dirname(out_path), exist_ok=True)
            edited_image.save(out_path)
            print("finish")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
