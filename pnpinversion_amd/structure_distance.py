"""Structure distance on the device: what the reference's evaluation gets from LossG.calculate_global_ssim_loss with dino_vitb8
(evaluation/matrics_calculator.py:385-405 -> :237-246 -> :154-171), from uint8 panels in to one float per pair out.

    scorer = StructureDistance(pipe_or_engine)     # a NativePipeline or a NativeEngine; no text tower, UNet rows or VAE images needed
    scorer.load_state_dict(dino_sd)                # DINO's own keys (checkpoint.load_dino_checkpoint), or scorer.load_synthetic(seed)
    scorer.distance(pred, gt, mask_pred, mask_gt)  # -> fp32 tensor [n]

What is computed, quirks included: the images as float 0..255 (NOT divided by 255), times a 0 / 1 mask; torchvision 0.13's Resize(224) on
a tensor, i.e. two-tap bilinear interpolation without antialiasing; ImageNet Normalize applied to those 0..255 values; DINO ViT-B/8 up to
the output of blocks.11.attn.qkv; the cosine self-similarity of its 785 keys (768 wide, the heads side by side), clamped at 1e-8 on the
product of the norms; the mean squared difference of the two 785 x 785 maps.  On the device the two maps are never written: one fused
kernel forms both per tile and reduces (csrc/structdist.hip).

Real dino_vitbase8_pretrain.pth weights load through checkpoint.load_dino_checkpoint; no such file exists offline, so that loader is
untested here and the tests run seeded synthetic weights (weights.dino_state_dict).  Whether the real patch embedding keeps the
~1.1e3-valued normalised pixels inside fp16's range is likewise unverified offline."""
import torch

from . import _capi
from .image_batches import chunks, stack_images, stack_masks


class StructureDistance:
    def __init__(self, pipe_or_engine, cfg=None, max_pairs=4):
        """cfg: _capi.DinoConfig (default: ViT-B/8).  max_pairs: pairs per launch set; longer batches are split."""
        self.engine = getattr(pipe_or_engine, "engine", pipe_or_engine)
        if cfg is None:
            cfg = _capi.DinoConfig()
            self.engine.lib.pnpi_dino_config_vitb8(cfg)
        self.engine.dino_attach(cfg, max_pairs)
        self.cfg, self.max_pairs = cfg, int(max_pairs)

    # ---- weights
    def load_state_dict(self, sd):
        self.engine.load_dino_state_dict(sd)

    def load_synthetic(self, seed=0):
        from . import weights
        g = self.cfg
        sd = weights.dino_state_dict(g.image_size, g.patch, g.width, g.layers, g.heads, g.intermediate, seed=seed)
        self.load_state_dict(sd)
        return sd

    # ---- outputs
    def keys(self, images, masks=None):
        """uint8 [n, S, S, 3], masks None or 0 / 1 -> fp32 [n, T, width]: the concatenated keys of the last block"""
        img = stack_images(images)
        m = stack_masks(masks, img)
        return torch.cat([self.engine.dino_keys(img[a:b], None if m is None else m[a:b]) for a, b in chunks(len(img), 2 * self.max_pairs)])

    def distance(self, pred, gt, mask_pred=None, mask_gt=None):
        """structure distance per (pred, gt) pair, one launch set per max_pairs pairs -> fp32 [n]"""
        a, b = stack_images(pred), stack_images(gt)
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError("Image shapes should be the same.")
        ma, mb = stack_masks(mask_pred, a), stack_masks(mask_gt, b)
        return torch.cat([self.engine.structure_distance(a[i:j], b[i:j], None if ma is None else ma[i:j], None if mb is None else mb[i:j])
                          for i, j in chunks(len(a), self.max_pairs)])
