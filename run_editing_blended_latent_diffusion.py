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

import numpy as np
from PIL import Image

from pnpinversion_amd import sweep
from pnpinversion_amd.sweep import mask_decode, setup_seed

image_save_paths = {
    "blended-latent-diffusion": "blended-latent-diffusion",
}
NUM_INFERENCE_STEPS = 50
BLENDING_PERCENTAGE = 0.25
GUIDANCE_SCALE = 7.5


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    sweep.add_sweep_args(ap, ["blended-latent-diffusion"])
    ap.add_argument("--batch_size", type=int, default=1, help="images per set of launches and GPU (not in the reference: it edits one by one)")
    args = ap.parse_args(argv)
    sweep.check_methods(ap, args, image_save_paths)
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    return args


def item_mask(item):
    """:209: the PIE-Bench RLE mask as the PIL "L" image edit_image takes (values 0 / 1)"""
    return Image.fromarray(np.uint8(mask_decode(item["mask"])[:, :, np.newaxis].repeat(3, 2))).convert("L")


def plan_work(args, instructions, method, rank=0, world=1, log=print):
    """This rank's share of the mapping file for `method`, without what is already on disk (:199-213 + round-robin sharding)
    -> [(editing_prompt, image_path, out_path, item)]"""
    return [(sweep.clean_prompt(item["editing_prompt"]), image_path, out_path, item)
            for item, image_path, out_path in sweep.plan(args, instructions, image_save_paths[method], rank, world, log, method)]


def main(argv=None):
    args = parse_args(argv)
    from pnpinversion_amd.blended_latent_diffusion import BlendedLatnetDiffusion
    from pnpinversion_amd.config import SD1, SMALL64
    from pnpinversion_amd.pipeline import NativePipeline
    make_pipeline = lambda cfg, device, tokenizer: NativePipeline(cfg, device=device, max_unet_rows=2 * args.batch_size,       # noqa: E731
                                                                  text_encoder="native", tokenizer=tokenizer)
    with sweep.session(args, {"sd1": SD1, "small64": SMALL64}, make_pipeline) as s:
        bld = BlendedLatnetDiffusion(pipe=s.pipe)
        side = s.cfg.sample_size * s.cfg.vae_scale
        instructions = sweep.read_mapping(args)
        for method in args.edit_method_list:
            todo = plan_work(args, instructions, method, s.rank, s.world)
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
                    sweep.save_panel(Image.fromarray(np.concatenate(panel, 1)), c[2])


if __name__ == "__main__":
    main()
