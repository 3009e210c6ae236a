#!/usr/bin/env python
"""PIE-Bench sweep driver with the CLI of the reference's run_editing_edit_friendly_p2p.py (same flags, output tree and skip-if-exists
resume): edit-friendly DDPM inversion (eta = 1) + Prompt-to-Prompt, on NativePipeline.  Weight / model-config flags and rank sharding as
run_editing_p2p.py.

Per image (run_editing_edit_friendly_p2p.py:64-118): w0 = 0.18215 * VAE posterior mode; inversion_forward_process with the source prompt at
guidance 1 (50 steps); inversion_reverse_process from xts[50 - 12] over the last 38 steps with [source, target] at guidance [1, 7.5] and
AttentionReplace (equal word counts) or AttentionRefine; panel [instruction, image, decode(source row), decode(target row)].
The reference also runs a target-prompt reconstruction pass (:86-89) whose decoded image is not in the panel: it is skipped here.
--batch_size N runs N images per set of launches (pnpi_ef_invert / pnpi_ef_edit with N images); every image gets the noise its sequential
run would draw -- after setup_seed(1234) the same stream for each."""
import argparse

import numpy as np
import torch
from PIL import Image

from pnpinversion_amd import sweep
from pnpinversion_amd.edit_friendly_ddm import inversion_utils as iu
from pnpinversion_amd.edit_friendly_ddm.ptp_classes import AttentionRefine, AttentionReplace
from pnpinversion_amd.sweep import mask_decode, setup_seed  # noqa: F401  (mask_decode: part of the reference script's surface, :19-35)
from pnpinversion_amd.utils.utils import image2latent, latent2image, load_512, txt_draw

image_save_paths = {
    "edit-friendly-inversion+p2p": "edit-friendly-inversion+p2p",
}
NUM_DDIM_STEPS = 50
ETA = 1
SKIP = 12
ldm_stable = None          # the NativePipeline of main(); edit_image_EF's default


def controller_class(prompt_src, prompt_tar):
    """:92-96: AttentionReplace when the prompts have the same number of words, AttentionRefine otherwise"""
    return AttentionReplace if len(prompt_src.split(" ")) == len(prompt_tar.split(" ")) else AttentionRefine


def edit_images_EF(pipe, image_paths, prompts_src, prompts_tar, source_guidance_scale=1, target_guidance_scale=7.5,
                   cross_replace_steps=0.4, self_replace_steps=0.6, num_ddim_steps=NUM_DDIM_STEPS, skip=SKIP, eta=ETA, noise=None):
    """edit_image_EF for len(image_paths) images in one set of launches -> list of PIL panels.  noise: the draws of one image
    [num_ddim_steps, 1, 4, h, w] (default: torch.randn_like on the device, the stream a sequential run would draw), used for every image."""
    n = len(image_paths)
    pipe.scheduler.set_timesteps(num_ddim_steps)
    ts = [int(t) for t in pipe.scheduler.timesteps]
    gts = [load_512(p) for p in image_paths]
    w0 = torch.cat([image2latent(pipe.vae, g) for g in gts])                  # :74-75 (posterior mode = mean)
    if noise is None:
        noise = iu.draw_noise(w0[:1], num_ddim_steps)
    noise = noise.to(pipe.device).float().reshape(num_ddim_steps, 1, *w0.shape[1:]).expand(num_ddim_steps, n, *w0.shape[1:])
    enc = lambda p: iu.encode_text(pipe, p)                                   # noqa: E731
    unc = enc("")
    cond = torch.cat([enc(s) for s in prompts_src])
    eng = pipe.unet.engine
    xts, zs = eng.ef_invert(w0, noise, unc.expand(n, -1, -1), cond, source_guidance_scale, eta, ts)
    ctrls = [controller_class(s, t)([s, t], num_ddim_steps, cross_replace_steps=cross_replace_steps, self_replace_steps=self_replace_steps,
                                    model=pipe).tables() for s, t in zip(prompts_src, prompts_tar)]
    ctx = torch.stack([torch.cat([unc, unc, enc([s, t])]) for s, t in zip(prompts_src, prompts_tar)])
    run = num_ddim_steps - skip
    lat = eng.ef_edit(xts[run], zs[:run], ctx, [source_guidance_scale, target_guidance_scale], ctrls, eta, ts)     # [n, 2, 4, h, w]
    panels = []
    for i in range(n):
        dec = latent2image(pipe.vae, lat[i])                                  # [source row, target row]
        gt = torch.from_numpy(gts[i]).float() / 127.5 - 1                     # the panel's image column as the reference computes it (:113)
        gt = np.uint8((gt.numpy() / 2 + 0.5) * 255)
        instruct = txt_draw(f"source prompt: {prompts_src[i]}\ntarget prompt: {prompts_tar[i]}")
        panels.append(Image.fromarray(np.concatenate((instruct, gt, dec[0], dec[1]), 1)))
    return panels


def edit_image_EF(edit_method, image_path, prompt_src, prompt_tar, source_guidance_scale=1, target_guidance_scale=7.5,
                  cross_replace_steps=0.4, self_replace_steps=0.6, pipe=None):
    """:64-118 -> PIL panel [instruction, image, source reconstruction, edit] (512 x 2048)"""
    if edit_method != "edit-friendly-inversion+p2p":
        raise NotImplementedError(f"No edit method named {edit_method}")
    return edit_images_EF(pipe or ldm_stable, [image_path], [prompt_src], [prompt_tar], source_guidance_scale, target_guidance_scale,
                          cross_replace_steps, self_replace_steps)[0]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    sweep.add_sweep_args(ap, ["edit-friendly-inversion+p2p"])
    ap.add_argument("--batch_size", type=int, default=1, help="images per set of launches and GPU (not in the reference: it edits one by one)")
    args = ap.parse_args(argv)
    sweep.check_methods(ap, args, image_save_paths)
    if args.batch_size < 1:
        ap.error("--batch_size must be >= 1")
    return args


def main(argv=None):
    global ldm_stable
    args = parse_args(argv)
    from pnpinversion_amd.config import SD1, SMALL64
    from pnpinversion_amd.pipeline import NativePipeline
    make_pipeline = lambda cfg, device, tokenizer: NativePipeline(cfg, device=device, max_unet_rows=4 * args.batch_size,       # noqa: E731
                                                                  text_encoder="native", tokenizer=tokenizer)
    with sweep.session(args, {"sd1": SD1, "small64": SMALL64}, make_pipeline) as s:
        ldm_stable = s.pipe
        instructions = sweep.read_mapping(args)
        for method in args.edit_method_list:
            todo = sweep.plan(args, instructions, image_save_paths[method], s.rank, s.world, method=method)
            for b0 in range(0, len(todo), args.batch_size):
                chunk = todo[b0:b0 + args.batch_size]
                for _, image_path, _ in chunk:
                    print(f"editing image [{image_path}] with [{method}]")
                setup_seed()
                panels = edit_images_EF(s.pipe, [c[1] for c in chunk], [sweep.clean_prompt(c[0]["original_prompt"]) for c in chunk],
                                        [sweep.clean_prompt(c[0]["editing_prompt"]) for c in chunk], source_guidance_scale=1,
                                        target_guidance_scale=7.5, cross_replace_steps=0.4, self_replace_steps=0.6)
                for panel, c in zip(panels, chunk):
                    sweep.save_panel(panel, c[2])


if __name__ == "__main__":
    main()
