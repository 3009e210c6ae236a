"""MutualSelfAttentionControl / MutualSelfAttentionControlMask with the constructors of models/masactrl/masactrl.py:14-39, :114-136.
Semantics (:57-69): at denoising steps >= start_step and transformer blocks >= start_layer (execution order 0..15), every self-attention
row of a CFG half reads the K and V of the half's FIRST row (the source image) -- in the kernel a row-indirection table of the
flash-attention launch.  `layer_idx` / `step_idx` lists (any subsets) replace the windows, as in the reference.  The mask-guided class
(:138-193) further restricts each target query to the source keys of its own class (foreground / background): one class-restricted
softmax in the kernel, equal to the reference's two masked passes + blend for binary masks."""
import os

from ..engine import MasaCtrlMaskTables, MasaCtrlTables
from .masactrl_utils import AttentionBase


class MutualSelfAttentionControl(AttentionBase):
    MODEL_TYPE = {"SD": 16, "SDXL": 70}

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, model_type="SD"):
        super().__init__()
        self.total_steps = total_steps
        self.total_layers = self.MODEL_TYPE.get(model_type, 16)
        self.start_step = start_step
        self.start_layer = start_layer
        self.layer_idx = layer_idx if layer_idx is not None else list(range(start_layer, self.total_layers))
        self.step_idx = step_idx if step_idx is not None else list(range(start_step, total_steps))

    def _windows(self):
        # the reference tests membership (`cur_step not in self.step_idx`, `cur_att_layer // 2 not in self.layer_idx`, masactrl.py:61):
        # the lists travel as a 16-bit block mask and a per-step byte array; the default windows keep their two integers
        win_l = self.layer_idx == list(range(self.start_layer, self.total_layers))
        win_s = self.step_idx == list(range(self.start_step, self.total_steps))
        return self.start_step, self.start_layer, None if win_l else self.layer_idx, None if win_s else self.step_idx

    def tables(self):
        return MasaCtrlTables(*self._windows())


def save_mask_png(mask, path):
    """torchvision.utils.save_image(mask[None, None], path) for a 0 / 1 (h, w) mask (masactrl.py:135-136) with PIL: one grey channel
    replicated to RGB, value * 255 + 0.5 clamped and truncated to uint8."""
    import numpy as np
    from PIL import Image
    a = mask.detach().cpu().numpy() if hasattr(mask, "detach") else np.asarray(mask)
    g = np.clip(np.asarray(a, dtype=np.float32) * 255.0 + 0.5, 0, 255).astype(np.uint8)
    Image.fromarray(np.repeat(g[:, :, None], 3, axis=2)).save(path)


class MutualSelfAttentionControlMask(MutualSelfAttentionControl):
    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, mask_s=None, mask_t=None,
                 mask_save_dir=None, model_type="SD"):
        """masactrl.py:115-136.  mask_s / mask_t: binary (h, w) masks of the source / target foreground, same shape.  The reference
        accepts None and then runs plain mutual self-attention through this class; here that is an error naming the plain class."""
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps, model_type)
        if mask_s is None or mask_t is None:
            raise ValueError("MutualSelfAttentionControlMask needs both mask_s and mask_t; for mutual self-attention without masks "
                             "use MutualSelfAttentionControl")
        self.mask_s = mask_s
        self.mask_t = mask_t
        self._tables = MasaCtrlMaskTables(*self._windows(), mask_s=mask_s, mask_t=mask_t)     # validates: binary, same shape
        if self._tables.mask_s.shape[0] != 1:
            raise ValueError("mask_s / mask_t have shape (h, w): one image per editor, as in the reference")
        if mask_save_dir is not None:
            os.makedirs(mask_save_dir, exist_ok=True)
            save_mask_png(self.mask_s, os.path.join(mask_save_dir, "mask_s.png"))
            save_mask_png(self.mask_t, os.path.join(mask_save_dir, "mask_t.png"))

    def tables(self):
        return self._tables
