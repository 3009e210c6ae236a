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
import json
import os

import numpy as np
import torch
from PIL import Image

from pnpinversion_amd.checkpoint import add_weight_args, resolve_weights
from pnpinversion_amd.distributed import broadcast_weights, prepare_env, shard_items
from run_editing_p2p import mask_decode, setup_seed  # noqa: F401  (mask_decode: part of the reference script's surface)

image_save_paths = {
    "ddim+pnp": "ddim+pnp",
    "directinversion+pnp": "directinversion+pnp",
}
NUM_DDIM_STEPS = 50


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rerun_exist_images", action="store_true")
    ap.add_argument("--data_path", type=str, default="data")
    ap.add_argument("--output_path", type=str, default="output")
    ap.add_argument("--edit_category_list", nargs="+", type=str, default=[str(i) for i in range(10)])
    ap.add_argument("--edit_method_list", nargs="+", type=str, default=["ddim+pnp", "directinversion+pnp"])
    ap.add_argument("--model_config", choices=("sd1", "small64"), default="sd1", help="small64: reduced-width test configuration")
    add_weight_args(ap)
    args = ap.parse_args(argv)
    unknown = [m for m in args.edit_method_list if m not in image_save_paths]
    if unknown:
        ap.error("unknown edit method(s) %s; this script runs %s" % (unknown, list(image_save_paths)))
    return args


def plan_work(args, instructions, method, rank=0, world=1, log=print):
    """This rank's share of the mapping file for `method`, without what is already on disk (:507-521 + round-robin sharding)
    -> [(original_prompt, editing_prompt, image_path, out_path)]"""
    work = [(k, v) for k, v in instructions.items() if v["editing_type_id"] in args.edit_category_list]
    todo = []
    for key, item in shard_items(work, rank, world):
        original_prompt = item["original_prompt"].replace("[", "").replace("]", "")
        editing_prompt = item["editing_prompt"].replace("[", "").replace("]", "")
        image_path = os.path.join(args.data_path, "annotation_images", item["image_path"])
        out_path = image_path.replace(args.data_path, os.path.join(args.output_path, image_save_paths[method]))
        if os.path.exists(out_path) and not args.rerun_exist_images:
            log(f"skip image [{image_path}] with [{method}]")
            continue
        todo.append((original_prompt, editing_prompt, image_path, out_path))
    return todo


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
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    prepare_env()
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    from pnpinversion_amd.config import SD1, SMALL64
    from pnpinversion_amd.pipeline import NativePipeline
    from pnpinversion_amd.pnp import PNP, Preprocess
    cfg = SD1 if args.model_config == "sd1" else SMALL64
    unet_sd, vae_sd, clip_sd, tokenizer = resolve_weights(args, cfg, rank)
    pipe = NativePipeline(cfg, device="cuda:%d" % local_rank, max_unet_rows=3, text_encoder="native", tokenizer=tokenizer)
    if rank == 0:
        pipe.load_state_dict(unet_sd, vae_sd, clip_sd=clip_sd)
    if world > 1:
        broadcast_weights(pipe.engine, src=0)
    model = Preprocess(pipe=pipe)
    pnp = PNP(pipe=pipe, n_timesteps=NUM_DDIM_STEPS)

    with open(os.path.join(args.data_path, "mapping_file.json")) as f:
        instructions = json.load(f)
    for method in args.edit_method_list:
        for prompt_src, prompt_tar, image_path, out_path in plan_work(args, instructions, method, rank, world):
            print(f"editing image [{image_path}] with [{method}]")
            setup_seed()
            fn = edit_image_ddim_PnP if method == "ddim+pnp" else edit_image_directinversion_PnP
            edited_image = fn(model, pnp, image_path=image_path, prompt_src=prompt_src, prompt_tar=prompt_tar, guidance_scale=7.5)
            os.makedirs(os.path.dirname(out_path), exist_ok=True)
            edited_image.save(out_path)
            print("finish")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
