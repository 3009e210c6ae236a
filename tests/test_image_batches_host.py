"""The image and mask forms ClipScore and StructureDistance accept (pnpinversion_amd/image_batches.py), on the host: both classes
hand the engine the same uint8 batches for the same input, in chunks of what one call holds, and refuse the same inputs with the same
words.  The engine is a recorder; nothing here needs a GPU."""
import types

import numpy as np
import pytest
import torch

from pnpinversion_amd.clip_score import ClipScore
from pnpinversion_amd.structure_distance import StructureDistance

N, S = 3, 12


class _Recorder:
    """stands in for NativeEngine: keeps what the metric classes pass down"""
    def __init__(self):
        self.seen = []

    def clipv_attach(self, *a):
        pass

    def dino_attach(self, *a):
        pass

    def _rec(self, img, m):
        self.seen.append((np.asarray(img), None if m is None else np.asarray(m)))
        return torch.zeros(len(img))

    def clip_image_embed(self, img, m=None):
        return self._rec(img, m)[:, None]

    def clip_score(self, img, ids, m=None):
        assert len(ids) == len(img)
        return self._rec(img, m)

    def dino_keys(self, img, m=None):
        return self._rec(img, m)[:, None, None]

    def structure_distance(self, a, b, ma=None, mb=None):
        self._rec(a, ma)
        return self._rec(b, mb)[:len(a)]

    def batches(self):
        """everything seen so far as one (images, masks) pair; a call without a mask counts as all ones"""
        imgs = np.concatenate([i for i, _ in self.seen])
        masks = None if all(m is None for _, m in self.seen) else np.concatenate([np.ones(i.shape[:3], np.uint8) if m is None else m for i, m in self.seen])
        self.seen = []
        return imgs, masks


@pytest.fixture()
def both():
    ec, ed = _Recorder(), _Recorder()
    clip = ClipScore(types.SimpleNamespace(engine=ec, tokenizer=None), vcfg=object(), max_images=2)
    dino = StructureDistance(ed, cfg=object(), max_pairs=1)
    return clip, ec, dino, ed


def _inputs():
    from PIL import Image
    g = np.random.Generator(np.random.Philox(key=[7, S]))
    imgs = g.integers(0, 256, (N, S, S, 3), dtype=np.uint8)
    masks = (g.random((N, S, S)) < 0.5).astype(np.uint8)
    grey = Image.fromarray(imgs[1, :, :, 0], "L")
    image_forms = {
        "numpy": (imgs, imgs),
        "torch": (torch.from_numpy(imgs), imgs),
        "one image": (imgs[0], imgs[:1]),
        "list of arrays": ([i for i in imgs], imgs),
        "tuple of PIL": (tuple(Image.fromarray(i) for i in imgs), imgs),
        "list with a grey PIL image": ([imgs[0], grey, imgs[2]], np.stack([imgs[0], np.asarray(grey.convert("RGB")), imgs[2]])),
    }
    ones = np.ones((S, S), np.uint8)
    mask_forms = {
        "none": (None, None),
        "[n, S, S]": (masks, masks),
        "int64 tensor": (torch.from_numpy(masks).long(), masks),
        "bool": (masks.astype(bool), masks),
        "[n, S, S, 3] repeat": (np.repeat(masks[..., None], 3, -1), masks),
        "list with None": ([masks[0], None, np.repeat(masks[2][..., None], 3, -1)], np.stack([masks[0], ones, masks[2]])),
        "list of None": ([None] * N, None),
    }
    return imgs, masks, image_forms, mask_forms


def _same(got, want, what):
    gi, gm = got
    assert gi.dtype == np.uint8 and np.array_equal(gi, want[0]), what
    if want[1] is None:
        assert gm is None, what
    else:
        assert gm.dtype == np.uint8 and np.array_equal(gm, want[1]), what


def test_both_classes_accept_the_same_forms(both):
    clip, ec, dino, ed = both
    imgs, masks, image_forms, mask_forms = _inputs()
    for iname, (iform, iwant) in image_forms.items():
        n = len(iwant)
        for mname, (mform, mwant) in mask_forms.items():
            if n == 1:      # the one-image form takes one mask: [S, S], the [S, S, 3] repeat or a one-entry list
                mform = None if mform is None else mform[0] if not isinstance(mform, list) else mform[:1]
                mwant = None if mwant is None else mwant[:1]
            what = "%s / %s" % (iname, mname)
            want = (iwant, mwant)
            clip.image_embed(iform, mform)
            _same(ec.batches(), want, "ClipScore.image_embed: " + what)
            assert len(clip.score(iform, masks=mform, input_ids=torch.zeros(n, 77, dtype=torch.int64))) == n
            _same(ec.batches(), want, "ClipScore.score: " + what)
            dino.keys(iform, mform)
            _same(ed.batches(), want, "StructureDistance.keys: " + what)
            assert len(dino.distance(iform, iform, mform, mform)) == n
            gi, gm = ed.batches()       # one pair per call: pred, gt, pred, gt ...
            _same((gi[0::2], None if gm is None else gm[0::2]), want, "StructureDistance.distance, pred: " + what)
            _same((gi[1::2], None if gm is None else gm[1::2]), want, "StructureDistance.distance, gt: " + what)


def test_chunks_are_what_one_call_holds(both):
    clip, ec, dino, ed = both
    imgs = _inputs()[0]
    clip.image_embed(imgs)
    assert [len(i) for i, _ in ec.seen] == [2, 1]                  # max_images = 2
    dino.keys(imgs)
    assert [len(i) for i, _ in ed.seen] == [2, 1]                  # 2 * max_pairs images
    ed.seen = []
    dino.distance(imgs, imgs)
    assert [len(i) for i, _ in ed.seen] == [1] * 6                 # max_pairs = 1: pred and gt of each pair


def test_both_classes_refuse_the_same_inputs(both):
    clip, ec, dino, ed = both
    imgs, masks = _inputs()[:2]
    ids = torch.zeros(N, 77, dtype=torch.int64)
    planes = np.repeat(masks[..., None], 3, -1)
    planes[1, 2, 3, 1] ^= 1
    two = masks.copy()
    two[2, 0, 0] = 2
    for bad, words in ((planes, "different channel planes"), (list(planes), "different channel planes"), (two, "0 / 1"), ([None, None, two[2]], "0 / 1")):
        for fn in (lambda: clip.image_embed(imgs, bad), lambda: clip.score(imgs, masks=bad, input_ids=ids), lambda: dino.keys(imgs, bad),
                   lambda: dino.distance(imgs, imgs, bad, None), lambda: dino.distance(imgs, imgs, None, bad)):
            with pytest.raises(ValueError, match=words):
                fn()
    with pytest.raises(ValueError, match="3 images but 2 prompts"):
        clip.score(imgs, input_ids=ids[:2])
    with pytest.raises(ValueError, match="Image shapes should be the same"):
        dino.distance(imgs, imgs[:2])
    assert not ec.seen and not ed.seen, "a refused input reached the engine"
