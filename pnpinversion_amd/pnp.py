"""Plug-and-Play editing on NativePipeline: the two classes of the reference's run_editing_pnp.py (`Preprocess` :40-156, `PNP` :296-400)
with its method names and signatures.  Feature injection (register_conv_control_efficient :239-294) and self-attention q/k injection
(register_attention_control_efficient :176-236) run inside libpnpi, selected per step by a pnpi_pnp_desc; there are no Python hooks.

  Preprocess.extract_latents   VAE encode, DDIM inversion with the source prompt at one row (pnpi_ddim_invert on the scheduler's
                               steps_offset = 1 timesteps 1, 21, .., 981 -> 51 latents), DDIM reconstruction from the last one (50 latents,
                               returned reversed) and its decoded image
  PNP.run_pnp / sample_loop    pnpi_pnp_edit: one UNet launch of the rows [source latent of this level, x, x] and one CFG + DDIM launch per
                               step, device-resident, text K / V projected once
  PNP.denoise_step             the same step through the level-1 calls pnpi_unet_forward_pnp + pnpi_pnp_step

The source-latent list is indexed exactly as the reference does: step i reads noisy_latent[-1 - i] and the start latent is
noisy_latent[-1].  `directinversion+pnp` passes the 51 inversion latents (step i reads the latent of ITS level); `ddim+pnp` passes the 50
reversed reconstruction latents, so its start latent is the one AFTER the first sampling step while the first timestep is still 981, and
step i reads the reconstruction one level below its own (source_list).

Deviations from the reference, deliberate: latents and the step arithmetic are fp32, as in every other loop of this project (the
reference runs an fp16 pipeline with xformers attention under a float32 autocast); images are loaded with PIL only (the reference goes
through torchvision's Resize / ToTensor, which for PIL images are PIL's own BILINEAR / LANCZOS resize and a division by 255); with several
images the rows of a launch are [img][source, negative, target] rather than the reference's [sources, negatives, targets] (every row's
arithmetic is the same).  A request the loop cannot honour raises: there is no CPU path."""
import numpy as np
import torch
from PIL import Image

from .p2p.scheduler_dev import DDIMSchedulerDev

NUM_DDIM_STEPS = 50
NEGATIVE_PROMPT = "ugly, blurry, black, low res, unrealistic"          # run_pnp :383
VAE_SCALING = 0.18215


def injection_counts(n_timesteps, pnp_f_t=0.8, pnp_attn_t=0.5):
    """run_pnp :386-387 -> (conv_steps, qk_steps): the number of leading timesteps that inject"""
    return int(n_timesteps * pnp_f_t), int(n_timesteps * pnp_attn_t)


def source_list(noisy_latent, n_timesteps):
    """sample_loop :395-396 / run_pnp :381 -> (source latents in step order [noisy_latent[-1 - i] for i < n], start latent noisy_latent[-1]).
    Holds for both lists the reference passes: the 51 inversion latents and the 50 reversed reconstruction latents."""
    if len(noisy_latent) < n_timesteps:
        raise ValueError("noisy_latent holds %d latents, the loop reads %d" % (len(noisy_latent), n_timesteps))
    return [noisy_latent[-1 - i] for i in range(n_timesteps)], noisy_latent[-1]


def _make_scheduler(engine):
    """DDIMScheduler.from_pretrained(model_key, subfolder="scheduler") of SD-1.5: scaled_linear 0.00085 -> 0.012, clip_sample False,
    set_alpha_to_one False, steps_offset 1"""
    s = DDIMSchedulerDev(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False,
                         steps_offset=1)
    s.bind(engine)
    return s


def _pipe_from(model_key, device, max_unet_rows):
    if model_key is None:
        raise ValueError("needs pipe= (a loaded NativePipeline) or model_key= (an SD-1.x checkpoint directory in the diffusers layout); "
                         "there is nothing to download from")
    from .checkpoint import load_checkpoint_dir
    from .config import SD1
    from .pipeline import NativePipeline
    unet_sd, vae_sd, clip_sd, tok = load_checkpoint_dir(model_key)
    pipe = NativePipeline(SD1, device=None if str(device) == "cuda" else device, max_unet_rows=max_unet_rows, text_encoder="native", tokenizer=tok)
    pipe.load_state_dict(unet_sd, vae_sd, clip_sd=clip_sd)
    return pipe


class _Parts:
    """what both classes take from the pipeline (:49-57, :307-313)"""

    def _bind(self, pipe):
        self.pipe = pipe
        self.engine = pipe.engine
        self.device = pipe.device
        self.vae = pipe.vae
        self.tokenizer = pipe.tokenizer
        self.text_encoder = pipe.text_encoder
        self.unet = pipe.unet
        self.scheduler = _make_scheduler(pipe.engine)

    def _side(self):
        return self.engine.lat_hw * self.engine.cfg.vae_scale

    def _encode(self, prompt):
        ids = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                             return_tensors="pt").input_ids
        return self.text_encoder(ids.to(self.device))[0]

    def _timesteps(self):
        return [int(t) for t in self.scheduler.timesteps]


class Preprocess(_Parts):
    def __init__(self, device="cuda", model_key=None, *, pipe=None):
        self.use_depth = False
        self._bind(pipe if pipe is not None else _pipe_from(model_key, device, 3))

    @torch.no_grad()
    def get_text_embeds(self, prompt, negative_prompt, device="cuda"):
        """:61-69 -> cat([negative, prompt])"""
        return torch.cat([self._encode(negative_prompt), self._encode(prompt)])

    @torch.no_grad()
    def decode_latents(self, latents):
        """:72-77"""
        imgs = self.vae.decode(1 / VAE_SCALING * latents)["sample"]
        return (imgs / 2 + 0.5).clamp(0, 1)

    def load_img(self, image_path):
        """:79-82: Resize(512) (the shorter side, PIL BILINEAR) and ToTensor -> [1, 3, H, W] in 0 .. 1"""
        im = (Image.open(image_path) if isinstance(image_path, str) else image_path).convert("RGB")
        side = self._side()
        w, h = im.size
        if min(w, h) != side:
            im = im.resize((side, int(side * h / w)) if w <= h else (int(side * w / h), side), Image.BILINEAR)
        if im.size != (side, side):
            raise ValueError("the context encodes %d x %d images; %s resizes to %s" % (side, side, image_path, im.size))
        return torch.from_numpy(np.asarray(im, dtype=np.float32) / 255.0).permute(2, 0, 1)[None].to(self.device)

    @torch.no_grad()
    def encode_imgs(self, imgs):
        """:85-90"""
        return self.vae.encode(2 * imgs - 1)["latent_dist"].mean * VAE_SCALING

    @torch.no_grad()
    def ddim_inversion(self, cond, latent):
        """:93-116 -> [latent, .. n more]: DirectInversion.next_step's arithmetic on reversed(scheduler.timesteps), one row, no CFG"""
        cond_batch = cond.repeat(latent.shape[0], 1, 1)
        lat = self.engine.ddim_invert(latent, cond_batch, self._timesteps())
        return [lat[i] for i in range(lat.shape[0])]

    @torch.no_grad()
    def ddim_sample(self, x, cond):
        """:119-141 -> the latent after every sampling step"""
        cond_batch = cond.repeat(x.shape[0], 1, 1)
        self.engine.text_kv_precompute(cond_batch)
        latent_list = []
        for t in self._timesteps():
            eps = self.engine.unet(x, t, None)
            x = self.engine.ddim_prev_step(eps, t, self.scheduler.step_ratio, x)
            latent_list.append(x)
        return latent_list

    @torch.no_grad()
    def extract_latents(self, num_steps, data_path, inversion_prompt=""):
        """:144-156 -> (inverted_x [num_steps + 1], rgb_reconstruction [1, 3, H, W], latent_reconstruction [num_steps], reversed)"""
        self.scheduler.set_timesteps(num_steps)
        cond = self.get_text_embeds(inversion_prompt, "")[1].unsqueeze(0)
        image = self.load_img(data_path)
        latent = self.encode_imgs(image)
        inverted_x = self.ddim_inversion(cond, latent)
        latent_reconstruction = self.ddim_sample(inverted_x[-1], cond)
        rgb_reconstruction = self.decode_latents(latent_reconstruction[-1])
        latent_reconstruction.reverse()
        return inverted_x, rgb_reconstruction, latent_reconstruction


class PNP(_Parts):
    def __init__(self, model_key=None, n_timesteps=NUM_DDIM_STEPS, device="cuda", *, pipe=None):
        self._bind(pipe if pipe is not None else _pipe_from(model_key, device, 3))
        if self.engine.max_unet_rows < 3:
            raise ValueError("Plug-and-Play launches three UNet rows per image: the pipeline needs max_unet_rows >= 3")
        self.scheduler.set_timesteps(n_timesteps, device=self.device)
        self.n_timesteps = n_timesteps
        self.desc = None

    @torch.no_grad()
    def get_text_embeds(self, prompt, negative_prompt, batch_size=1):
        """:318-332 -> cat([negative] * batch_size + [prompt] * batch_size)"""
        return torch.cat([self._encode(negative_prompt)] * batch_size + [self._encode(prompt)] * batch_size)

    @torch.no_grad()
    def decode_latent(self, latent):
        """:335-340"""
        img = self.vae.decode(1 / VAE_SCALING * latent)["sample"]
        return (img / 2 + 0.5).clamp(0, 1)

    def get_data(self, image_path):
        """:343-348: LANCZOS resize to the context's image size, ToTensor -> [3, H, W]"""
        image = (Image.open(image_path) if isinstance(image_path, str) else image_path).convert("RGB")
        side = self._side()
        image = image.resize((side, side), resample=Image.LANCZOS)
        return torch.from_numpy(np.asarray(image, dtype=np.float32) / 255.0).permute(2, 0, 1).to(self.device)

    def init_pnp(self, conv_injection_t, qk_injection_t):
        """:371-375: the first conv_injection_t / qk_injection_t timesteps inject (negative: none) at the reference's sites, derived from
        this model's structure (pnpi_pnp_desc_default)"""
        ts = self.scheduler.timesteps
        self.qk_injection_timesteps = ts[:qk_injection_t] if qk_injection_t >= 0 else []
        self.conv_injection_timesteps = ts[:conv_injection_t] if conv_injection_t >= 0 else []
        self.desc = self.engine.pnp_desc(self.n_timesteps, len(self.conv_injection_timesteps), len(self.qk_injection_timesteps))

    def _context(self):
        """denoise_step :358: ["", negative prompt, target prompt] -> [1, 3, 77, D]"""
        return torch.cat([self.pnp_guidance_embeds, self.text_embeds], dim=0)[None]

    @torch.no_grad()
    def denoise_step(self, x, t, guidance_scale, noisy_latent):
        """:351-369 through the level-1 calls: one hooked forward of [noisy_latent, x, x], CFG over rows 1 and 2, the DDIM step"""
        if self.desc is None:
            raise RuntimeError("init_pnp has not been called")
        t = int(t)
        latent_model_input = torch.cat([noisy_latent] + [x] * 2)[None]
        conv_on = t in [int(v) for v in self.conv_injection_timesteps] or t == 1000              # register_time + :276
        qk_on = t in [int(v) for v in self.qk_injection_timesteps] or t == 1000                  # :190-191
        noise_pred = self.engine.unet_pnp(latent_model_input, t, self._context(), self.desc, conv_on, qk_on)
        return self.engine.pnp_step(noise_pred, x, t, self.scheduler.step_ratio, guidance_scale)

    def run_pnp(self, image_path, noisy_latent, target_prompt, guidance_scale=7.5, pnp_f_t=0.8, pnp_attn_t=0.5):
        """:377-391"""
        self.image = self.get_data(image_path)
        self.eps = noisy_latent[-1]
        self.text_embeds = self.get_text_embeds(target_prompt, NEGATIVE_PROMPT)
        self.pnp_guidance_embeds = self.get_text_embeds("", "").chunk(2)[0]
        pnp_f_t, pnp_attn_t = injection_counts(self.n_timesteps, pnp_f_t, pnp_attn_t)
        self.init_pnp(conv_injection_t=pnp_f_t, qk_injection_t=pnp_attn_t)
        return self.sample_loop(self.eps, guidance_scale, noisy_latent)

    @torch.no_grad()
    def sample_latents(self, x, guidance_scale, noisy_latent):
        """the loop of sample_loop (:395-396) -> the final latent [1, C, h, w], device-resident"""
        if self.desc is None:
            raise RuntimeError("init_pnp has not been called")
        src, _ = source_list(noisy_latent, self.n_timesteps)
        return self.engine.pnp_edit(torch.stack([s.reshape(x.shape) for s in src]), x, self._context(), self.desc, self._timesteps(),
                                    guidance_scale)

    @torch.no_grad()
    def sample_loop(self, x, guidance_scale, noisy_latent):
        """:393-400 -> the decoded edit [1, 3, H, W] in 0 .. 1"""
        return self.decode_latent(self.sample_latents(x, guidance_scale, noisy_latent))
