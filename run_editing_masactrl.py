#!/usr/bin/env python
"""MasaCtrl editing driver with the CLI and the MasaCtrlEditor class of the reference's run_editing_masactrl.py (methods
"ddim+masactrl" and "directinversion+masactrl"), on the MI355X-native pipeline: inversion, direct-inversion offsets and the
mutual-self-attention sampling loop are device-resident libpnpi loops; the attention editor is a kernel-side row table.  Under
torch.distributed.run the work list is sharded over the ranks exactly like run_editing_p2p.py."""
import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image

from pnpinversion_amd.masactrl.diffuser_utils import MasaCtrlPipeline
from pnpinversion_amd.masactrl.masactrl import MutualSelfAttentionControl, MutualSelfAttentionControlMask
from pnpinversion_amd.masactrl.masactrl_utils import AttentionBase, regiter_attention_editor_diffusers
from pnpinversion_amd.p2p.inversion import DirectInversion
from pnpinversion_amd import sweep
from pnpinversion_amd.sweep import mask_decode, setup_seed  # noqa: F401  (same helpers as the reference's copy, :21-46)
from pnpinversion_amd.utils.utils import load_512, txt_draw


def load_image(image_path, device):
    """run_editing_masactrl.py:49-54: RGB -> float [-1, 1] [1,3,H,W] -> nearest resize to 512 x 512"""
    arr = np.array(Image.open(image_path).convert("RGB")) if isinstance(image_path, str) else np.asarray(image_path)[:, :, :3]
    image = torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1)[:3].unsqueeze(0).float() / 127.5 - 1.
    return F.interpolate(image, (512, 512)).to(device)


class MasaCtrlEditor:
    """run_editing_masactrl.py:57-175"""

    def __init__(self, method_list, device, num_ddim_steps=50, *, pipeline=None, weight_seed=0):
        self.device = device
        self.method_list = method_list
        self.num_ddim_steps = num_ddim_steps
        if pipeline is None:   # the reference loads CompVis/stable-diffusion-v1-4 here; no checkpoint exists offline
            pipeline = MasaCtrlPipeline.synthetic(seed=weight_seed, device=device)
        self.model = pipeline
        self.scheduler = pipeline.scheduler
        self.model.scheduler.set_timesteps(self.num_ddim_steps)

    def __call__(self, edit_method, image_path, prompt_src, prompt_tar, guidance_scale, step=4, layper=10, mask=None):
        """mask (beyond the reference's signature): a binary (h, w) array -> mask-guided MasaCtrl with it as source AND target mask"""
        kw = dict(mask=mask) if mask is not None else {}
        if edit_method == "ddim+masactrl":
            return self.edit_image_ddim_MasaCtrl(image_path, prompt_src, prompt_tar, guidance_scale, step=step, layper=layper, **kw)
        elif edit_method == "directinversion+masactrl":
            return self.edit_image_directinversion_MasaCtrl(image_path, prompt_src, prompt_tar, guidance_scale, step=step, layper=layper, **kw)
        raise NotImplementedError(f"No edit method named {edit_method}")

    def _side(self):
        return self.model.engine.cfg.sample_size * self.model.engine.cfg.vae_scale

    def _sample(self, prompt_tar, start, guidance_scale, step, layper, noise_loss_list, mask=None):
        prompts = ["", prompt_tar]
        regiter_attention_editor_diffusers(self.model, AttentionBase())
        image_fixed = self.model([prompt_tar], latents=start[-1:], num_inference_steps=self.num_ddim_steps,
                                 guidance_scale=guidance_scale)                                   # "direct synthesis" (:104-110)
        total = max(50, self.num_ddim_steps)
        if mask is None:
            editor = MutualSelfAttentionControl(step, layper, total_steps=total)
        else:
            m = torch.as_tensor(np.asarray(mask), dtype=torch.float32)
            editor = MutualSelfAttentionControlMask(step, layper, total_steps=total, mask_s=m, mask_t=m)
        regiter_attention_editor_diffusers(self.model, editor)
        image_masactrl = self.model(prompts, latents=start, num_inference_steps=self.num_ddim_steps, guidance_scale=guidance_scale,
                                    noise_loss_list=noise_loss_list)
        return image_fixed, image_masactrl

    def _panel(self, source_image, image_masactrl, prompt_src, prompt_tar):
        side = source_image.shape[-1]
        u8 = lambda t: (t.permute(1, 2, 0).detach().cpu().numpy() * 255).astype(np.uint8)
        instruct = txt_draw(f"source prompt: {prompt_src}\ntarget prompt: {prompt_tar}", target_size=(side, side))
        src = ((source_image[0].permute(1, 2, 0).detach().cpu().numpy() * 0.5 + 0.5) * 255).astype(np.uint8)
        return Image.fromarray(np.concatenate((np.array(instruct), src, u8(image_masactrl[0]), u8(image_masactrl[-1])), 1))

    def _images(self, image_path):
        source_image = load_image(image_path, self.model.device)
        image_gt = load_512(image_path)
        side = self._side()
        if side != 512:   # reduced test configurations only
            source_image = F.interpolate(source_image, (side, side))
            image_gt = np.array(Image.fromarray(image_gt).resize((side, side)))
        return source_image, image_gt

    def edit_image_directinversion_MasaCtrl(self, image_path, prompt_src, prompt_tar, guidance_scale, step=4, layper=10,
                                            return_stages=False, mask=None):
        """run_editing_masactrl.py:87-133"""
        source_image, image_gt = self._images(image_path)
        inv = DirectInversion(model=self.model, num_ddim_steps=self.num_ddim_steps)
        _, _, x_stars, noise_loss_list = inv.invert(image_gt=image_gt, prompt=["", prompt_tar], guidance_scale=guidance_scale)
        x_t = x_stars[-1]
        _, image_masactrl = self._sample(prompt_tar, x_t.expand(2, -1, -1, -1), guidance_scale, step, layper, noise_loss_list, mask)
        panel = self._panel(source_image, image_masactrl, prompt_src, prompt_tar)
        return (panel, dict(x_stars=x_stars, noise_loss_list=noise_loss_list, images=image_masactrl)) if return_stages else panel

    def edit_image_ddim_MasaCtrl(self, image_path, prompt_src, prompt_tar, guidance_scale, step=4, layper=10, return_stages=False,
                                 mask=None):
        """run_editing_masactrl.py:135-175"""
        source_image, _ = self._images(image_path)
        start_code, latents_list = self.model.invert(source_image, "", guidance_scale=guidance_scale,
                                                     num_inference_steps=self.num_ddim_steps, return_intermediates=True)
        _, image_masactrl = self._sample(prompt_tar, start_code.expand(2, -1, -1, -1), guidance_scale, step, layper, None, mask)
        panel = self._panel(source_image, image_masactrl, prompt_src, prompt_tar)
        return (panel, dict(x_stars=latents_list, images=image_masactrl)) if return_stages else panel


def latent_mask(rle, side=64):
    """The PIE-Bench mask of an item (run-length list over the 512 x 512 image) as a binary (side, side) array: mask_decode, then PIL
    NEAREST to the latent grid, as run_editing_blended_latent_diffusion.py reads its mask."""
    m = Image.fromarray(np.uint8(mask_decode(rle)) * 255).resize((side, side), Image.NEAREST)
    return (np.array(m) > 127).astype(np.uint8)


def output_folder(method, mask_guided):
    """<method> as in the reference; --mask_guided runs go to <method>-mask"""
    return method + ("-mask" if mask_guided else "")


def output_dir(output_path, method, mask_guided):
    return os.path.join(output_path, output_folder(method, mask_guided))


def build_parser():
    ap = argparse.ArgumentParser()
    sweep.add_sweep_args(ap, ["ddim+masactrl", "directinversion+masactrl"])
    ap.add_argument("--num_ddim_steps", type=int, default=50)
    ap.add_argument("--mask_guided", action="store_true",
                    help="mask-guided MasaCtrl (MutualSelfAttentionControlMask): the item's PIE-Bench mask at 64 x 64 is source and target "
                         "mask; outputs go to <method>-mask.  Not an option of the reference's script.")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from pnpinversion_amd.config import SD1, SMALL64
    make_pipeline = lambda cfg, device, tokenizer: MasaCtrlPipeline(cfg, device=device, text_encoder="native", tokenizer=tokenizer)  # noqa: E731
    with sweep.session(args, {"sd1": SD1, "small64": SMALL64}, make_pipeline) as s:
        editor = MasaCtrlEditor(args.edit_method_list, s.device, num_ddim_steps=args.num_ddim_steps, pipeline=s.pipe)
        for item, image_path in sweep.shard(args, sweep.read_mapping(args), s.rank, s.world):     # images outside, methods inside
            for method in args.edit_method_list:
                out_path = sweep.pending(args, image_path, output_folder(method, args.mask_guided), method=method)
                if out_path is None:
                    continue
                print(f"editing image [{image_path}] with [{method}]")
                setup_seed()
                torch.cuda.empty_cache()
                kw = dict(mask=latent_mask(item["mask"], s.cfg.sample_size)) if args.mask_guided else {}
                edited = editor(method, image_path=image_path, prompt_src=sweep.clean_prompt(item["original_prompt"]),
                                prompt_tar=sweep.clean_prompt(item["editing_prompt"]), guidance_scale=7.5, step=4, layper=10, **kw)
                sweep.save_panel(edited, out_path)


if __name__ == "__main__":
    main()
