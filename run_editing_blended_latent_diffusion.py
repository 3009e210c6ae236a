#!/usr/bin/env python
"""PIE-Bench sweep driver with the CLI of the reference's run_editing_blended_latent_diffusion.py (same five flags, output folder
`blended-latent-diffusion` and skip-if-exists resume): Blended Latent Diffusion, the benchmark's mask-driven editor, on NativePipeline.
Weight / model-config flags and rank sharding as run_editing_p2p.py.

Per image (run_editing_blended_latent_diffusion.py:199-228): the editing prompt alone, the PIE-Bench `mask` field (RLE, 1 = edit region,
border forced to 1) as the region, 50 steps of which the last 38 run (blending_percentage 0.25), guidance 7.5; panel [instruction, source
image, zeros, edited].  --batch_size N runs N images per set of launches (pnpi_bld_edit with 2 N UNet rows); every image gets the draws
its sequential run would get -- after setup_seed(1234) the same stream for each.  Model: SD-1.x layout weights (--checkpoint_dir); the
reference's default stabilityai/stable-diffusion-2-1-base is another architecture and out of scope."""
import argparse
import json
import os

import numpy as np
import torch
from PIL import Image

from pnpinversion_amd.checkpoint import add_weight_args, resolve_weights
from pnpinversion_amd.distributed import broadcast_weights, prepare_env, shard_items
from run_editing_p2p import mask_decode, setup_seed

image_save_paths = {
    "blended-latent-diffusion": "blended-latent-diffusion",
}
NUM_INFERENCE_STEPS = 50
BLENDING_PERCENTAGE = 0.25
GUIDANCE_SCALE = 7.5


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rerun_exist_images", action="store_true")
    ap.add_argument("--data_path", type=str, default="data")
    ap.add_argument("--output_path", type=str, default="output")
    ap.add_argument("--edit_category_list", nargs="+", type=str, default=[str(i) for i in range(10)])
    ap.add_argument("--edit_method_list", nargs="+", type=str, default=["blended-latent-diffusion"])
    ap.add_argument("--batch_size", type=int, default=1, help="images per set of launches and GPU (not in the reference: it edits one by one)")
    ap.add_argument("--model_config", choices=("sd1", "small64"), default="sd1", help="small64: reduced-width test configuration")
    add_weight_args(ap)
    args = ap.parse_args(argv)
    unknown = [m for m in args.edit_method_list if m not in image_save_paths]
    if unknown:
        ap.error("unknown edit method(s) %s; this script runs %s" % (unknown, list(image_save_paths)))
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    return args


def item_mask(item):
    """:209: the PIE-Bench RLE mask as the PIL "L" image edit_image takes (values 0 / 1)"""
    return Image.fromarray(np.uint8(mask_decode(item["mask"])[:, :, np.newaxis].repeat(3, 2))).convert("L")


def plan_work(args, instructions, method, rank=0, world=1, log=print):
    """This rank's share of the mapping file for `method`, without what is already on disk (:199-213 + round-robin sharding)
    -> [(editing_prompt, image_path, out_path, item)]"""
    work = [(k, v) for k, v in instructions.items() if v["editing_type_id"] in args.edit_category_list]
    todo = []
    for key, item in shard_items(work, rank, world):
        editing_prompt = item["editing_prompt"].replace("[", "").replace("]", "")
        image_path = os.path.join(args.data_path, "annotation_images", item["image_path"])
        out_path = image_path.replace(args.data_path, os.path.join(args.output_path, image_save_paths[method]))
        if os.path.exists(out_path) and not args.rerun_exist_images:
            log(f"skip image [{image_path}] with [{method}]")
            continue
        todo.append((editing_prompt, image_path, out_path, item))
    return todo


def main(argv=None):
    args = parse_args(argv)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    prepare_env()
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    from pnpinversion_amd.blended_latent_diffusion import BlendedLatnetDiffusion
    from pnpinversion_amd.config import SD1, SMALL64
    from pnpinversion_amd.pipeline import NativePipeline
    cfg = SD1 if args.model_config == "sd1" else SMALL64
    unet_sd, vae_sd, clip_sd, tokenizer = resolve_weights(args, cfg, rank)
    pipe = NativePipeline(cfg, device="cuda:%d" % local_rank, max_unet_rows=2 * args.batch_size, text_encoder="native", tokenizer=tokenizer)
    if rank == 0:
        pipe.load_state_dict(unet_sd, vae_sd, clip_sd=clip_sd)
    if world > 1:
        broadcast_weights(pipe.engine, src=0)
    bld = BlendedLatnetDiffusion(pipe=pipe)
    side = cfg.sample_size * cfg.vae_scale

    with open(os.path.join(args.data_path, "mapping_file.json")) as f:
        instructions = json.load(f)
    for method in args.edit_method_list:
        todo = plan_work(args, instructions, method, rank, world)
        for b0 in range(0, len(todo), args.batch_size):
            chunk = todo[b0:b0 + args.batch_size]
            for c in chunk:
                print(f"editing image [{c[1]}] with [{method}]")
            setup_seed()
            n_run = NUM_INFERENCE_STEPS - int(NUM_INFERENCE_STEPS * BLENDING_PERCENTAGE)
            draws = bld._draw(n_run, side, side)                 # one image's stream after setup_seed(), the same for every image
            panels = bld.edit_images([c[1] for c in chunk], [item_mask(c[3]) for c in chunk], [c[0] for c in chunk], side, side,
                                     NUM_INFERENCE_STEPS, GUIDANCE_SCALE, blending_percentage=BLENDING_PERCENTAGE, noise=draws)
            for panel, c in zip(panels, chunk):
                os.makedirs(os.path.dirname(c[2]), exist_ok=True)
                Image.fromarray(np.concatenate(panel, 1)).save(c[2])
                print("finish")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
