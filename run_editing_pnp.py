#!/usr/bin/env python
"""PIE-Bench sweep driver with the CLI of the reference's run_editing_pnp.py (same five flags, output folders `ddim+pnp` /
`directinversion+pnp`, skip-if-exists resume): Plug-and-Play editing on NativePipeline.  Weight / model-config flags and rank sharding as
run_editing_p2p.py.

Per image (run_editing_pnp.py:414-462): DDIM inversion with the source prompt (one row, no CFG, 50 steps on the timesteps 1 .. 981), then
the Plug-and-Play loop towards the editing prompt from the inversion latents (directinversion+pnp) or from the reversed DDIM
reconstruction latents (ddim+pnp): guidance 7.5, feature injection on the first 40 steps, self-attention q/k injection on the first 25.
Panel [instruction, source image, reconstruction, edit]; for ddim+pnp the third column is the decoded DDIM reconstruction, for
directinversion+pnp it is latent2image(inverted_x[1]), as in the reference."""
import argparse

import numpy as np
from PIL import Image

from pnpinversion_amd import sweep
from pnpinversion_amd.sweep import mask_decode, setup_seed  # noqa: F401  (mask_decode: part of the reference script's surface)

image_save_paths = {
    "ddim+pnp": "ddim+pnp",
    "directinversion+pnp": "directinversion+pnp",
}
NUM_DDIM_STEPS = 50


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    sweep.add_sweep_args(ap, ["ddim+pnp", "directinversion+pnp"])
    args = ap.parse_args(argv)
    sweep.check_methods(ap, args, image_save_paths)
    return args


def plan_work(args, instructions, method, rank=0, world=1, log=print):
    """This rank's share of the mapping file for `method`, without what is already on disk (:507-521 + round-robin sharding)
    -> [(original_prompt, editing_prompt, image_path, out_path)]"""
    return [(sweep.clean_prompt(item["original_prompt"]), sweep.clean_prompt(item["editing_prompt"]), image_path, out_path)
            for item, image_path, out_path in sweep.plan(args, instructions, image_save_paths[method], rank, world, log, method)]


def _u8(img01):
    return np.uint8(255 * np.array(img01[0].permute(1, 2, 0).cpu().detach()))


def edit_image_ddim_PnP(model, pnp, image_path, prompt_src, prompt_tar, guidance_scale=7.5, image_shape=(512, 512)):
    """:414-436"""
    from pnpinversion_amd.utils.utils import load_512, txt_draw
    image_gt = load_512(image_path)
    _, rgb_reconstruction, latent_reconstruction = model.extract_latents(data_path=image_path, num_steps=NUM_DDIM_STEPS,
                                                                         inversion_prompt=prompt_src)
    edited_image = pnp.run_pnp(image_path, latent_reconstruction, prompt_tar, guidance_scale)
    image_instruct = txt_draw(f"source prompt: {prompt_src}\ntarget prompt: {prompt_tar}")
    return Image.fromarray(np.concatenate((image_instruct, image_gt, _u8(rgb_reconstruction), _u8(edited_image)), 1))


def edit_image_directinversion_PnP(model, pnp, image_path, prompt_src, prompt_tar, guidance_scale=7.5, image_shape=(512, 512)):
    """:440-462 (third column: latent2image(inverted_x[1]), as the reference has it)"""
    from pnpinversion_amd.utils.utils import latent2image, load_512, txt_draw
    image_gt = load_512(image_path)
    inverted_x, _, _ = model.extract_latents(data_path=image_path, num_steps=NUM_DDIM_STEPS, inversion_prompt=prompt_src)
    edited_image = pnp.run_pnp(image_path, inverted_x, prompt_tar, guidance_scale)
    image_instruct = txt_draw(f"source prompt: {prompt_src}\ntarget prompt: {prompt_tar}")
    return Image.fromarray(np.concatenate((image_instruct, image_gt, np.uint8(np.array(latent2image(model=pnp.vae, latents=inverted_x[1])[0])),
                                           _u8(edited_image)), 1))


def main(argv=None):
    args = parse_args(argv)
    from pnpinversion_amd.config import SD1, SMALL64
    from pnpinversion_amd.pipeline import NativePipeline
    from pnpinversion_amd.pnp import PNP, Preprocess
    make_pipeline = lambda cfg, device, tokenizer: NativePipeline(cfg, device=device, max_unet_rows=3, text_encoder="native",   # noqa: E731
                                                                  tokenizer=tokenizer)
    with sweep.session(args, {"sd1": SD1, "small64": SMALL64}, make_pipeline) as s:
        model = Preprocess(pipe=s.pipe)
        pnp = PNP(pipe=s.pipe, n_timesteps=NUM_DDIM_STEPS)
        instructions = sweep.read_mapping(args)
        for method in args.edit_method_list:
            for prompt_src, prompt_tar, image_path, out_path in plan_work(args, instructions, method, s.rank, s.world):
                print(f"editing image [{image_path}] with [{method}]")
                setup_seed()
                fn = edit_image_ddim_PnP if method == "ddim+pnp" else edit_image_directinversion_PnP
                edited_image = fn(model, pnp, image_path=image_path, prompt_src=prompt_src, prompt_tar=prompt_tar, guidance_scale=7.5)
                sweep.save_panel(edited_image, out_path)


if __name__ == "__main__":
    main()
