"""LPIPS (SqueezeNet) on the device: what the reference's evaluation gets from torchmetrics'
LearnedPerceptualImagePatchSimilarity(net_type='squeeze') (evaluation/matrics_calculator.py:324-342), from uint8 panels in to one float
per pair out.

    scorer = Lpips(pipe_or_engine)               # a NativePipeline or a NativeEngine; no text tower, UNet rows or VAE images needed
    scorer.load_state_dict(sd)                   # checkpoint.load_lpips_checkpoint(squeezenet_pth, lin_pth), or scorer.load_synthetic(seed)
    scorer.score(pred, gt, mask_pred, mask_gt)   # -> fp32 tensor [n]

What is computed: the images as float / 255, times a 0 / 1 mask, then * 2 - 1 (a cleared pixel is -1, not 0); the ScalingLayer
(x - shift) / scale; torchvision's squeezenet1_1().features 0 .. 12 at the image's own size (no resize; the max pools are ceil_mode);
the seven taps behind features 1, 4, 7, 9, 10, 11, 12; per tap and pixel the channel-normalised difference, squared, weighted by the
non-negative `lin` layer and averaged over the pixels; the sum of the seven.

The normalisation is torchmetrics >= 1.0's own: a / sqrt(1e-8 + sum_c a_c^2).  torchmetrics 0.11 wraps the lpips package, which divides
by sqrt(sum_c a_c^2) + 1e-10; the reference pins no version.  The two differ only where a feature vector is ~0.

Neither torchvision's squeezenet1_1 weights nor the lpips package's squeeze.pth exists offline: checkpoint.load_lpips_checkpoint's key
mapping is tested on stand-in files, real weights are unverified, and so is whether the real network's activations stay inside fp16's
range (the device keeps them in fp16).  The tests run seeded synthetic weights (weights.lpips_state_dict)."""
import torch

from .image_batches import chunks, stack_images, stack_masks


class Lpips:
    def __init__(self, pipe_or_engine, max_pairs=4):
        """max_pairs: pairs per launch set; longer batches are split."""
        self.engine = getattr(pipe_or_engine, "engine", pipe_or_engine)
        self.engine.lpips_attach(max_pairs)
        self.max_pairs = int(max_pairs)

    # ---- weights
    def load_state_dict(self, sd):
        self.engine.load_lpips_state_dict(sd)

    def load_synthetic(self, seed=0):
        from . import weights
        sd = weights.lpips_state_dict(seed)
        self.load_state_dict(sd)
        return sd

    # ---- outputs
    def features(self, images, masks=None, tap=0):
        """uint8 [n, S, S, 3], masks None or 0 / 1 -> fp32 [n, H, H, C]: the feature map of tap 0 .. 6"""
        img = stack_images(images)
        m = stack_masks(masks, img)
        return torch.cat([self.engine.lpips_features(img[a:b], None if m is None else m[a:b], tap) for a, b in chunks(len(img), 2 * self.max_pairs)])

    def score(self, pred, gt, mask_pred=None, mask_gt=None):
        """LPIPS per (pred, gt) pair, one launch set per max_pairs pairs -> fp32 [n]"""
        a, b = stack_images(pred), stack_images(gt)
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError("Image shapes should be the same.")
        ma, mb = stack_masks(mask_pred, a), stack_masks(mask_gt, b)
        return torch.cat([self.engine.lpips(a[i:j], b[i:j], None if ma is None else ma[i:j], None if mb is None else mb[i:j])
                          for i, j in chunks(len(a), self.max_pairs)])
