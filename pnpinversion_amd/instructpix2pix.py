"""InstructPix2Pix on NativePipeline: the sampler of the reference's run_editing_instructpix2pix.py (edit_instruct_pix2pix :92-142), the
benchmark's only instruction-driven editor.  The UNet is the SD-1.x graph with an 8-channel conv_in (config.SD1_IP2P): it reads the noisy
latent scaled by c_in next to the UNSCALED image latent, at a fractional timestep, on three rows per image
[edit text + image, null text + image, null text + zero image] (CFGDenoiser :33-46).

k_diffusion is not a dependency: the three things the reference takes from it are restated here in fp32 eager torch, operation by operation
  DiscreteEpsDDPMDenoiser / CompVisDenoiser   sigmas, t_to_sigma, get_sigmas, sigma_to_t (quantize = False), c_in / c_out
  get_ancestral_step, sample_euler_ancestral  eta = 1, s_noise = 1
and the device loop (pnpi_ip2p_edit) takes their per-step scalars as a host table (step_table).  euler_ancestral_step is the step in
eager torch: what the HIP kernel is tested against bit for bit.

Random draws are inputs: `noise=(start [4, h, w], steps [nsteps - 1, 4, h, w])`.  Without it they are drawn with torch on the host from
the GLOBAL generator in the reference's order (z0 :133, then one randn_like per step whose sigma_next > 0).  There is no device RNG.

Deviations from the reference:
  * fp32 latents and step arithmetic (the reference runs under autocast);
  * the sinusoid of a fractional timestep is evaluated as ldm's timestep_embedding does (fp32 freqs, fp32 t * freqs), with the C
    library's expf / cosf / sinf; an INTEGER timestep (the schedule's two ends) takes the library's table row (fp64, rounded once);
  * the image must fit the context's square latent: ImageOps.fit to (side, side), where the reference fits to a multiple of 64 near 512;
    the panel puts the ORIGINAL image next to the edit as the reference does, so it must already have that size (PIE-Bench: 512 x 512)."""
import math

import numpy as np
import torch
from PIL import Image, ImageOps

from .utils.utils import txt_draw

VAE_SCALING = 0.18215


def ldm_alphas_cumprod(n=1000, linear_start=0.00085, linear_end=0.012):
    """ldm's register_schedule (ddpm_edit.py:117-148, make_beta_schedule "linear"): fp64 throughout, stored as an fp32 buffer"""
    betas = (torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n, dtype=torch.float64) ** 2).numpy()
    return torch.tensor(np.cumprod(1.0 - betas, axis=0), dtype=torch.float32)


class SigmaSchedule:
    """K.external.DiscreteEpsDDPMDenoiser's schedule on the fp32 alphas_cumprod buffer"""

    def __init__(self, alphas_cumprod=None):
        ac = ldm_alphas_cumprod() if alphas_cumprod is None else torch.as_tensor(alphas_cumprod, dtype=torch.float32)
        self.sigmas = ((1 - ac) / ac) ** 0.5
        self.log_sigmas = self.sigmas.log()

    def t_to_sigma(self, t):
        t = torch.as_tensor(t).float()
        low_idx, high_idx, w = t.floor().long(), t.ceil().long(), t.frac()
        log_sigma = (1 - w) * self.log_sigmas[low_idx] + w * self.log_sigmas[high_idx]
        return log_sigma.exp()

    def get_sigmas(self, n):
        t = torch.linspace(len(self.sigmas) - 1, 0, n)
        return torch.cat([self.t_to_sigma(t), torch.zeros(1)])                  # n + 1 values

    def sigma_to_t(self, sigma):
        """quantize = False: a FRACTIONAL timestep, [n] -> [n]"""
        sigma = torch.as_tensor(sigma, dtype=torch.float32).reshape(-1)
        log_sigma = sigma.log()
        dists = log_sigma - self.log_sigmas[:, None]
        low_idx = dists.ge(0).cumsum(dim=0).argmax(dim=0).clamp(max=self.log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = self.log_sigmas[low_idx], self.log_sigmas[high_idx]
        w = ((low - log_sigma) / (low - high)).clamp(0, 1)
        return (1 - w) * low_idx + w * high_idx


def get_ancestral_step(sigma_from, sigma_to):
    """k-diffusion's get_ancestral_step at eta = 1 on 0-dim fp32 tensors -> (sigma_down, sigma_up)"""
    sigma_up = min(sigma_to, (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


def step_table(sigmas, schedule=None):
    """The per-step host scalars of pnpi_ip2p_edit, [nsteps, 6] fp32: sigma, sigma_down - sigma, sigma_up, c_in, t = sigma_to_t(sigma),
    sigma_next > 0.  sigmas: get_sigmas(nsteps) (or its first k + 1 values: the first k steps)."""
    schedule = schedule or SigmaSchedule()
    sigmas = torch.as_tensor(sigmas, dtype=torch.float32)
    n = len(sigmas) - 1
    out = np.zeros((n, 6), np.float32)
    for i in range(n):
        s, s1 = sigmas[i], sigmas[i + 1]
        down, up = get_ancestral_step(s, s1)
        c_in = 1 / (s.reshape(1) ** 2 + 1) ** 0.5                                # get_scalings on the [batch] sigma
        out[i] = [s.item(), (down - s).item(), up.item(), c_in.item(), schedule.sigma_to_t(s.reshape(1)).item(), float(s1 > 0)]
    return out


def euler_ancestral_step(z, eps, noise, sigma, sigma_next, cfg_text, cfg_image):
    """CompVisDenoiser.forward on the three rows, CFGDenoiser's combine (:46) and one iteration of sample_euler_ancestral in eager fp32:
    z [n, C, h, w], eps [n, 3, C, h, w] (cond, image-cond, uncond), noise [n, C, h, w] (unread when sigma_next == 0) -> z'"""
    sigma, sigma_next = torch.as_tensor(sigma, dtype=torch.float32), torch.as_tensor(sigma_next, dtype=torch.float32)
    c_out = -sigma
    out_cond, out_img_cond, out_uncond = (z + eps[:, k] * c_out for k in range(3))
    denoised = out_uncond + cfg_text * (out_cond - out_img_cond) + cfg_image * (out_img_cond - out_uncond)
    sigma_down, sigma_up = get_ancestral_step(sigma, sigma_next)
    d = (z - denoised) / sigma
    dt = sigma_down - sigma
    z = z + d * dt
    if sigma_next > 0:
        z = z + noise * 1.0 * sigma_up
    return z


def fit_size(width, height, resolution=512):
    """:107-111: the size the reference fits the input image to"""
    factor = resolution / max(width, height)
    factor = math.ceil(min(width, height) * factor / 64) * 64 / min(width, height)
    return int((width * factor) // 64) * 64, int((height * factor) // 64) * 64


class InstructPix2Pix:
    def __init__(self, pipe, schedule=None):
        """pipe: a loaded NativePipeline on an 8-channel configuration (config.SD1_IP2P); max_unet_rows: 3 per image of an edit_images call"""
        cfg = pipe.engine.cfg
        if cfg.in_channels != 8 or cfg.out_channels != 4:
            raise ValueError("%s needs a model with in_channels = 8 and out_channels = 4 (config.SD1_IP2P), got in_channels = %d, "
                             "out_channels = %d" % (type(self).__name__, cfg.in_channels, cfg.out_channels))
        self.pipe, self.engine = pipe, pipe.engine
        self.schedule = schedule or SigmaSchedule()
        self.side = self.engine.lat_hw * cfg.vae_scale

    def _encode(self, prompts):
        """model.get_learned_conditioning: the tokenizer / text-encoder calls (FrozenCLIPEmbedder.forward)"""
        ids = self.pipe.tokenizer(prompts, padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
        with torch.no_grad():
            return self.pipe.text_encoder(ids.to(self.pipe.device))[0]

    def _draw(self, sigmas):
        """the reference's draws of one image from the global generator, in its order"""
        shape = (4, self.engine.lat_hw, self.engine.lat_hw)
        start = torch.randn(1, *shape)[0]                                                       # :133
        n = int((sigmas[1:] > 0).sum())
        return start, torch.stack([torch.randn(1, *shape)[0] for _ in range(n)]) if n else torch.zeros(0, *shape)

    def _fit(self, image):
        image = Image.open(image) if isinstance(image, str) else image
        original = image.convert("RGB")                                                         # :106
        width, height = fit_size(*original.size, resolution=self.side)
        if (width, height) != (self.side, self.side):
            raise ValueError("the image fits to %d x %d, this context's latent needs %d x %d" % (width, height, self.side, self.side))
        return original, ImageOps.fit(original, (width, height), method=Image.Resampling.LANCZOS)          # :112

    # what InstructDiffusion (instructdiffusion.py) does differently: the third text row, the loop's combine, the edit's way into the panel
    def _rows(self, cond, null_token):
        """[n, 77, D] each -> the three text rows per image [n, 3, 77, D] (:42)"""
        return torch.stack([cond, null_token, null_token], 1)

    def _loop(self, *args):
        return self.engine.ip2p_edit(*args)

    def _edited(self, x, original):
        """the decoded uint8 [H, W, 3] edit as it enters the panel"""
        return x

    @torch.no_grad()
    def edit_images(self, images, instructions, steps=50, cfg_text=7.5, cfg_image=1.5, noise=None, return_latents=False):
        """edit for len(images) (image, instruction) pairs in one loop call -> list of panels (uint8 [H, 4 W, 3])"""
        n = len(images)
        if len(instructions) != n:
            raise ValueError("one instruction per image")
        eng = self.engine
        originals, fitted = zip(*[self._fit(im) for im in images])
        null_token = self._encode([""])                                                         # :104
        cond = torch.cat([self._encode([e]) for e in instructions])                             # :116
        context = self._rows(cond, null_token.expand(n, -1, -1))                                # :42
        x = torch.stack([2 * torch.tensor(np.array(f)).float() / 255 - 1 for f in fitted]).permute(0, 3, 1, 2)     # :117-118
        m = eng.max_vae_images
        c_concat = torch.cat([eng.vae_encode(x[i:i + m]) for i in range(0, n, m)])              # :119 encode_first_stage(...).mode()
        sigmas = self.schedule.get_sigmas(steps)                                                # :125
        if noise is None:
            noise = [self._draw(sigmas) for _ in range(n)]
        elif isinstance(noise, tuple):
            noise = [noise] * n
        lat = c_concat.shape[1:]
        start = torch.stack([torch.as_tensor(s).float().reshape(lat) for s, _ in noise])
        draws = torch.zeros(steps, n, *lat)                                                     # the step at sigma_next == 0 draws nothing
        for i, (_, d) in enumerate(noise):
            d = torch.as_tensor(d).float()
            draws[:d.shape[0], i] = d.reshape(-1, *lat)[:steps]
        z0 = start * sigmas[0]                                                                  # :133
        z = self._loop(z0, c_concat, draws, context, step_table(sigmas, self.schedule), cfg_text, cfg_image)      # :134
        scaled = 1. / VAE_SCALING * z                                                           # decode_first_stage
        x = torch.cat([eng.vae_decode(scaled[i:i + m]) for i in range(0, n, m)])                # :135
        x = torch.clamp((x + 1.0) / 2.0, min=0.0, max=1.0)                                      # :136
        x = (255.0 * x.permute(0, 2, 3, 1)).type(torch.uint8).cpu().numpy()                     # :137-138
        panels = []
        for i in range(n):
            source, edited = np.array(originals[i]), self._edited(x[i], originals[i])
            image_instruct = txt_draw(f"edit prompt: {instructions[i]}", target_size=source.shape[:2])      # :140 (512 x 512 there)
            if source.shape != edited.shape:
                raise ValueError("the panel needs a source image of the edit's size %s, got %s" % (edited.shape, source.shape))
            panels.append(np.concatenate((image_instruct, source, np.zeros_like(image_instruct), edited), axis=1))   # :142
        return (panels, z) if return_latents else panels

    @torch.no_grad()
    def edit(self, image, instruction, steps=50, cfg_text=7.5, cfg_image=1.5, noise=None):
        """edit_instruct_pix2pix (:92-142) -> the panel instruction | source | black | edit as a PIL image"""
        return Image.fromarray(self.edit_images([image], [instruction], steps, cfg_text, cfg_image, noise)[0])
