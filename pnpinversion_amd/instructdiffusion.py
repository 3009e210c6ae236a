"""InstructDiffusion on NativePipeline: the sampler of the reference's run_editing_instructdiffusion.py (instruct_diffusion_edit :90-130), the
benchmark's second instruction-driven editor.  The UNet is the function InstructPix2Pix runs (config.SD1_IP2P: instruct_diffusion.yaml is the
SD-1.x graph with in_channels = 8, GroupNorm eps 1e-6 as ldm's; force_type_convert only moves dtypes under autocast), the schedule, the
fractional timesteps and the Euler-ancestral move are the same (instructpix2pix.py: SigmaSchedule, step_table, get_ancestral_step).  What
differs (CFGDenoiser :37-48):

  rows     [instruction + image, null text + image, instruction + zero image]: the third row keeps the TEXT and drops the image
  combine  0.5 * (out_img_cond + out_txt_cond) + text_cfg_scale * (out_cond - out_img_cond) + image_cfg_scale * (out_cond - out_txt_cond):
           symmetric around the mean of the two single-condition rows, no chain from an unconditional row
  defaults cfg_text = 5.0, cfg_image = 1.25; the edit is ImageOps.fit back to the original's size before the panel is built (:127)

euler_ancestral_step is the step in eager fp32 torch: what the HIP kernel (pnpi_instdiff_step) is tested against bit for bit.

Random draws are inputs: `noise=(start [4, h, w], steps [nsteps - 1, 4, h, w])`.  Without it they are drawn with torch on the host from
the GLOBAL generator in the reference's order (z0 :119, then one randn_like per step whose sigma_next > 0).  There is no device RNG.

Deviations from the reference, the same as InstructPix2Pix's:
  * fp32 latents and step arithmetic (the reference runs under autocast);
  * the image must fit the context's SQUARE latent: ImageOps.fit to (side, side), where the reference fits to a multiple of 64 near 512
    and keeps the aspect ratio; an image that fits to another size is refused.  The final ImageOps.fit(edited, original.size) is kept: it is
    the identity for an original of (side, side) (PIE-Bench: 512 x 512) and resamples a square original of another size."""
import numpy as np
import torch
from PIL import Image, ImageOps

from .instructpix2pix import InstructPix2Pix, SigmaSchedule, fit_size, get_ancestral_step, step_table  # noqa: F401  (the shared restatements)


def euler_ancestral_step(z, eps, noise, sigma, sigma_next, cfg_text, cfg_image):
    """CompVisDenoiser.forward on the three rows, CFGDenoiser's combine (:46-48) and one iteration of sample_euler_ancestral in eager fp32:
    z [n, C, h, w], eps [n, 3, C, h, w] (cond, image-cond, text-cond), noise [n, C, h, w] (unread when sigma_next == 0) -> z'"""
    sigma, sigma_next = torch.as_tensor(sigma, dtype=torch.float32), torch.as_tensor(sigma_next, dtype=torch.float32)
    c_out = -sigma
    out_cond, out_img_cond, out_txt_cond = (z + eps[:, k] * c_out for k in range(3))
    denoised = 0.5 * (out_img_cond + out_txt_cond) + \
        cfg_text * (out_cond - out_img_cond) + \
        cfg_image * (out_cond - out_txt_cond)
    sigma_down, sigma_up = get_ancestral_step(sigma, sigma_next)
    d = (z - denoised) / sigma
    dt = sigma_down - sigma
    z = z + d * dt
    if sigma_next > 0:
        z = z + noise * 1.0 * sigma_up
    return z


class InstructDiffusion(InstructPix2Pix):
    """pipe: a loaded NativePipeline on an 8-channel configuration (config.SD1_IP2P); max_unet_rows: 3 per image of an edit_images call"""

    def _rows(self, cond, null_token):
        return torch.stack([cond, null_token, cond], 1)                                         # :41

    def _loop(self, *args):
        return self.engine.instdiff_edit(*args)                                                 # :120

    def _edited(self, x, original):
        return np.array(ImageOps.fit(Image.fromarray(x), original.size, method=Image.Resampling.LANCZOS))        # :127

    def edit_images(self, images, instructions, steps=50, cfg_text=5.0, cfg_image=1.25, noise=None, return_latents=False):
        """instruct_diffusion_edit for len(images) (image, instruction) pairs in one loop call -> list of panels (uint8 [H, 4 W, 3])"""
        return super().edit_images(images, instructions, steps, cfg_text, cfg_image, noise, return_latents)

    def edit(self, image, instruction, steps=50, cfg_text=5.0, cfg_image=1.25, noise=None):
        """instruct_diffusion_edit (:90-130) -> the panel instruction | source | black | edit as a PIL image"""
        return super().edit(image, instruction, steps, cfg_text, cfg_image, noise)
