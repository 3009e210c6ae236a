"""Blended Latent Diffusion on NativePipeline: the class of the reference's run_editing_blended_latent_diffusion.py (:42-173, its spelling
`BlendedLatnetDiffusion`), the benchmark's only mask-driven editor.  One prompt, one user-supplied region; after every CFG + DDIM step the
latent outside the region is replaced by the source latent noised to that step's level, so the background is preserved by construction.

edit_image mirrors the reference line by line (file:line comments below); the step loop runs device-resident in libpnpi (pnpi_bld_edit:
one UNet launch of the [uncond, cond] rows per step, one fused CFG + DDIM + add_noise + blend launch, text K / V cached).  edit_images
batches several (image, mask, prompt) triples into one loop call (2 rows per image and launch).

Random draws are inputs: `noise=(start [4, h, w], blend [nsteps_run, 4, h, w])`.  Without it they are drawn with torch on the host from
the GLOBAL generator in the reference's order (the start latent :102-105, then one torch.randn_like per executed step :137) -- the
reference's default argument `generator=torch.manual_seed(42)` (:74) IS the global generator, re-seeded per image by the script's
setup_seed().  Any other generator is refused.  There is no device RNG.

Deviations from the reference, both deliberate:
  * latents and the step arithmetic are fp32, as in every other loop of this project (the reference keeps fp16 latents, :106, :158);
  * the model is the context's SD-1.x architecture.  The reference's default stabilityai/stable-diffusion-2-1-base (other head layout,
    linear projections, OpenCLIP) is out of scope; model_path takes an SD-1.x checkpoint directory in the diffusers layout.
The reference calls _read_mask with its default dest_size (64, 64) (:81), which only fits height = width = 512; here the destination is
the latent size (height // 8, width // 8), the same 64 x 64 at 512."""
import numpy as np
import torch
from PIL import Image

from .utils.utils import txt_draw

VAE_SCALING = 0.18215


def timestep_slice(timesteps, blending_percentage):
    """:110-112: timesteps[int(len(timesteps) * blending_percentage):]"""
    return timesteps[int(len(timesteps) * blending_percentage):]


def nearest_source_index(dst, src):
    """PIL NEAREST: destination pixel i of `dst` reads source pixel floor((i + 0.5) * src / dst) of `src`"""
    return np.minimum(((2 * np.arange(dst, dtype=np.int64) + 1) * src) // (2 * dst), src - 1)


def host_mask(mask_u8, dest_size):
    """The rule of pnpi_bld_mask on the host: uint8 [H, W] -> fp32 0/1 [h, w], dest_size = (w, h) as PIL takes it"""
    m = np.asarray(mask_u8)
    w, h = dest_size
    m = m[nearest_source_index(h, m.shape[0])][:, nearest_source_index(w, m.shape[1])]
    return (m >= 0.5).astype(np.float32)


class BlendedLatnetDiffusion:
    def __init__(self, model_path=None, device="cuda", *, pipe=None, max_unet_rows=2):
        """pipe: a loaded NativePipeline to run on; otherwise model_path is an SD-1.x checkpoint directory (diffusers layout) loaded into
        a new one (:43-62 without the download).  max_unet_rows: 2 per image of an edit_images call."""
        self.model_path = model_path
        self.device = device
        if pipe is None:
            if model_path is None:
                raise ValueError("BlendedLatnetDiffusion needs pipe= (a loaded NativePipeline) or model_path= (an SD-1.x checkpoint "
                                 "directory in the diffusers layout); there is nothing to download from")
            from .checkpoint import load_checkpoint_dir
            from .config import SD1
            from .pipeline import NativePipeline
            unet_sd, vae_sd, clip_sd, tok = load_checkpoint_dir(model_path)
            pipe = NativePipeline(SD1, device=None if device == "cuda" else device, max_unet_rows=max_unet_rows, text_encoder="native",
                                  tokenizer=tok)
            pipe.load_state_dict(unet_sd, vae_sd, clip_sd=clip_sd)
        self.load_models(pipe)

    def load_models(self, pipe):
        """:48-62: the pipeline's parts; its scheduler already is DDIMScheduler(beta 0.00085 -> 0.012 scaled_linear, clip_sample=False,
        set_alpha_to_one=False), bound to the engine's tables"""
        self.pipe = pipe
        self.engine = pipe.engine
        self.vae = pipe.vae
        self.tokenizer = pipe.tokenizer
        self.text_encoder = pipe.text_encoder
        self.unet = pipe.unet
        self.scheduler = pipe.scheduler

    # ---- helpers
    def _size(self, height, width):
        side = self.engine.lat_hw * self.engine.cfg.vae_scale
        if (height, width) != (side, side):
            raise ValueError("height / width must be the context's %d x %d, got %d x %d" % (side, side, height, width))

    def _encode(self, prompts):
        """:83-99: the tokenizer / text-encoder calls of the reference"""
        ids = self.tokenizer(prompts, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                             return_tensors="pt").input_ids
        with torch.no_grad():
            return self.text_encoder(ids.to(self.pipe.device))[0]

    def _draw(self, n_run, height, width):
        """the reference's draws of one image from the global generator, in its order: :102-105, then :137 once per executed step"""
        shape = (1, self.unet.in_channels, height // 8, width // 8)
        start = torch.randn(shape)
        return start[0], torch.stack([torch.randn(shape)[0] for _ in range(n_run)])

    @torch.no_grad()
    def edit_images(self, image_paths, masks, prompts, height=512, width=512, num_inference_steps=50, guidance_scale=7.5, generator=None,
                    blending_percentage=0.25, *, noise=None, return_latents=False):
        """edit_image for len(image_paths) (image, mask, prompt) triples in one loop call -> list of the reference's 4-panel lists.
        prompts: one editing prompt (str) per image.  noise: None | (start, blend) used for every image | list of such pairs per image."""
        if generator is not None and generator is not torch.default_generator:
            raise ValueError("generator= other than the global generator is not supported: the reference's default "
                             "torch.manual_seed(42) is the global generator; seed it (setup_seed) or pass noise=")
        self._size(height, width)
        n = len(image_paths)
        if len(masks) != n or len(prompts) != n:
            raise ValueError("one mask and one prompt per image")
        images, src, lat_masks = [], [], []
        for path, mask in zip(image_paths, masks):
            image_ori = Image.open(path) if isinstance(path, str) else path
            image_ori = image_ori.resize((height, width), Image.BILINEAR)                      # :78 (not load_512's crop)
            image_ori = np.array(image_ori)[:, :, :3]                                          # :79
            images.append(image_ori)
            src.append(self._image2latent(image_ori))                                          # :80
            lat_masks.append(self._read_mask(mask, (width // 8, height // 8))[0])              # :81
        src = torch.cat(src)
        lat_mask = torch.cat(lat_masks)[:, 0]                                                  # [n, h, w], broadcast over the 4 channels
        cond = torch.cat([self._encode([p]) for p in prompts])                                 # :83-90
        uncond = self._encode([""]).expand(n, -1, -1)                                          # :92-99
        self.scheduler.set_timesteps(num_inference_steps)                                      # :108
        ts = [int(t) for t in self.scheduler.timesteps]
        n_run = len(timestep_slice(ts, blending_percentage))                                   # :110-112
        if n_run < 1:
            raise ValueError("blending_percentage %r leaves no step to run" % blending_percentage)
        if noise is None:
            noise = [self._draw(n_run, height, width) for _ in range(n)]                       # :102-105, :137
        elif isinstance(noise, tuple):
            noise = [noise] * n
        start = torch.stack([torch.as_tensor(s).float().reshape(src.shape[1:]) for s, _ in noise])
        blend = torch.stack([torch.as_tensor(b).float().reshape(n_run, *src.shape[1:]) for _, b in noise], 1)
        latents = self.engine.bld_edit(start, src, blend, lat_mask, uncond, cond, guidance_scale, ts)      # :110-139
        scaled = 1 / VAE_SCALING * latents                                                     # :141
        m = self.engine.max_vae_images
        image = torch.cat([self.vae.decode(scaled[i:i + m])["sample"] for i in range(0, n, m)])            # :144
        image = (image / 2 + 0.5).clamp(0, 1)                                                  # :146
        image = image.detach().cpu().permute(0, 2, 3, 1).numpy()                               # :147
        decoded = (image * 255).round().astype("uint8")                                        # :148 (rounds; utils.latent2image truncates)
        panels = []
        for i in range(n):
            image_instruct = txt_draw(f"edit prompt: {[prompts[i]]}")                          # :150
            panels.append([image_instruct, images[i], np.zeros_like(image_instruct), decoded[i]])          # :152
        return (panels, latents) if return_latents else panels

    @torch.no_grad()
    def edit_image(self, image_path, mask, prompts, height=512, width=512, num_inference_steps=50, guidance_scale=7.5, generator=None,
                   blending_percentage=0.25, *, noise=None):
        """:64-152 -> [instruction, source image, zeros, edited] (uint8 [height, width, 3] each).  prompts: the reference's list with the
        one editing prompt (or that prompt)."""
        if not isinstance(prompts, str):
            if len(prompts) != 1:
                raise ValueError("blended latent diffusion edits with ONE prompt (the reference passes [editing_prompt] * 1)")
            prompts = prompts[0]
        return self.edit_images([image_path], [mask], [prompts], height, width, num_inference_steps, guidance_scale, generator,
                                blending_percentage, noise=noise)[0]

    @torch.no_grad()
    def _image2latent(self, image):
        """:154-162: uint8 [H, W, 3] -> 0.18215 * posterior mean [1, 4, H / 8, W / 8] (fp32)"""
        return self.vae.image2latent_u8(np.ascontiguousarray(image))

    def _read_mask(self, mask, dest_size=(64, 64)):
        """:164-173: PIL image (1 = edit region) -> ([1, 1, h, w] fp32 0/1 on the device, the original mask)"""
        org_mask = mask
        mask = org_mask.resize(dest_size, Image.NEAREST)
        mask = np.array(mask)
        mask[mask < 0.5] = 0
        mask[mask >= 0.5] = 1
        mask = mask[np.newaxis, np.newaxis, ...]
        pipe = self.__dict__.get("pipe")                    # no pipeline (host tests): the mask stays on the CPU
        mask = torch.from_numpy(mask).float().to(pipe.device if pipe is not None else "cpu")
        return mask, org_mask
