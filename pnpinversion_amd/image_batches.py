"""What the device-side image metrics (clip_score.ClipScore, structure_distance.StructureDistance) accept as images and masks, brought
to the batches the engine takes: uint8 [n, S, S, 3] images and 0 / 1 uint8 [n, S, S] masks, cut into chunks of what one call holds."""
import numpy as np
import torch


def plane(mask):
    """one mask as evaluate.py builds it ([S, S, 3], the plane repeated) or [S, S] -> uint8 [S, S]"""
    a = np.asarray(mask)
    if a.ndim == 3:
        if not (a == a[..., :1]).all():
            raise ValueError("a mask with different channel planes is not supported")
        a = a[..., 0]
    if not np.isin(a, (0, 1)).all():
        raise ValueError("masks must hold 0 / 1 only")
    return a.astype(np.uint8)


def rgb(img):
    """one image (PIL or array) -> uint8 [S, S, 3]"""
    a = np.asarray(img)
    if (a.ndim != 3 or a.shape[2] != 3) and hasattr(img, "convert"):
        a = np.asarray(img.convert("RGB"))
    return a.astype(np.uint8)


def stack_images(images):
    """a numpy array or torch tensor [n, S, S, 3] or [S, S, 3], or a list of PIL images / arrays -> [n, S, S, 3]"""
    if isinstance(images, (list, tuple)):
        images = np.stack([rgb(i) for i in images])
    a = images if isinstance(images, torch.Tensor) else np.asarray(images)
    return a[None] if a.ndim == 3 else a


def stack_masks(masks, img):
    """None, [n, S, S], [n, S, S, 3] or a list whose entries are None (whole image), [S, S] or the [S, S, 3] repeat -> uint8 [n, S, S]"""
    if masks is None:
        return None
    if isinstance(masks, torch.Tensor):
        masks = masks.cpu().numpy()
    if not isinstance(masks, (list, tuple)):
        masks = np.asarray(masks)
        one = masks.ndim == 2 or (masks.ndim == 3 and tuple(masks.shape) == tuple(img.shape[1:]))      # [S, S], or one [S, S, 3] repeat
        masks = [masks] if one else list(masks)
    if all(k is None for k in masks):
        return None
    S = img.shape[1]
    return np.stack([np.ones((S, S), np.uint8) if k is None else plane(k) for k in masks])


def chunks(n, per):
    return [(i, min(i + per, n)) for i in range(0, n, per)]
