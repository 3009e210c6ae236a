"""CLIP similarity on the device: what the reference's evaluation gets from torchmetrics' CLIPScore("openai/clip-vit-large-patch14")
(evaluation/matrics_calculator.py:274,290-302), from uint8 panels and prompts in to scores out.

    scorer = ClipScore(pipe)                       # pipe: a NativePipeline whose text encoder is the native CLIP text tower
    scorer.load_state_dict(clip_model_sd)          # transformers CLIPModel keys (checkpoint.load_clip_model_dir), or scorer.load_synthetic(seed)
    scorer.score(images, prompts, masks=None)      # -> fp32 tensor [n]: max(100 * cos(image, text), 0)

The text tower is the one Stable Diffusion 1.x conditions on and the pipeline already holds; the image tower (ViT-L/14: 257 tokens x 1024
channels x 24 layers) and the two projection matrices are attached to the same context (pnpi_clipv_attach).  Preprocessing is
CLIPProcessor's: PIL's bicubic resize to 224 (bit-exact, fixed point), / 255, CLIP mean / std; a mask is applied first as uint8(img * mask).

EOS rule.  The pooled text row is the FIRST position holding the row's largest id.  That is transformers' `input_ids.argmax(-1)` and it
is the end-of-text token for every tokenizer of this package: WordTokenizer and ClipBPETokenizer both close a prompt with EOS = 49407 =
vocab - 1 (the largest id there is) and pad with the same id, so the first maximum is the prompt's own EOS (text.eos_positions).

Real clip-vit-large-patch14 weights load through checkpoint.load_clip_model_dir; no such checkpoint exists offline, so that loader is
untested here and the tests run seeded synthetic towers (weights.clipv_state_dict)."""
import torch

from . import _capi
from .image_batches import chunks, stack_images, stack_masks


class ClipScore:
    def __init__(self, pipe, vcfg=None, max_images=8):
        """vcfg: _capi.ClipvConfig (default: ViT-L/14).  max_images: images per launch set; longer batches are split."""
        self.pipe, self.engine = pipe, pipe.engine
        if vcfg is None:
            vcfg = _capi.ClipvConfig()
            self.engine.lib.pnpi_clipv_config_vitl14(vcfg)
        self.engine.clipv_attach(vcfg, max_images)
        self.vcfg, self.max_images = vcfg, int(max_images)

    # ---- weights
    def load_state_dict(self, clip_model_sd):
        self.engine.load_clipv_state_dict(clip_model_sd)

    def load_synthetic(self, seed=0):
        from . import weights
        v = self.vcfg
        sd = weights.clipv_state_dict(v.image_size, v.patch, v.width, v.layers, v.heads, v.intermediate, v.proj_dim,
                                      text_hidden=self.engine.cfg.cross_dim, seed=seed)
        self.load_state_dict(sd)
        return sd

    # ---- inputs
    def tokenize(self, prompts):
        """prompts (str or list) -> int64 ids [n, 77], padded and truncated as CLIPProcessor does for CLIPScore"""
        if isinstance(prompts, str):
            prompts = [prompts]
        L = self.engine.cfg.ctx_len
        return torch.as_tensor(self.pipe.tokenizer(list(prompts), padding="max_length", max_length=L, truncation=True).input_ids)

    # ---- outputs
    def image_embed(self, images, masks=None):
        """uint8 [n, S, S, 3] (numpy / torch / list of PIL images), masks None or 0 / 1 [n, S, S] -> fp32 [n, proj_dim], not normalised"""
        img = stack_images(images)
        m = stack_masks(masks, img)
        return torch.cat([self.engine.clip_image_embed(img[a:b], None if m is None else m[a:b]) for a, b in chunks(len(img), self.max_images)])

    def text_embed(self, prompts=None, input_ids=None):
        ids = self.tokenize(prompts) if input_ids is None else torch.as_tensor(input_ids)
        return torch.cat([self.engine.clip_text_embed(ids[a:b]) for a, b in chunks(len(ids), self.max_images)])

    def score(self, images, prompts=None, masks=None, input_ids=None):
        """CLIPScore per (image, prompt) pair, one launch set per max_images pairs"""
        img = stack_images(images)
        m = stack_masks(masks, img)
        ids = self.tokenize(prompts) if input_ids is None else torch.as_tensor(input_ids)
        if len(ids) != len(img):
            raise ValueError("%d images but %d prompts" % (len(img), len(ids)))
        return torch.cat([self.engine.clip_score(img[a:b], ids[a:b], None if m is None else m[a:b]) for a, b in chunks(len(img), self.max_images)])
