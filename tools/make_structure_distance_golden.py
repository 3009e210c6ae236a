"""Writes tests/golden/structure_distance_tiny.npz: the tiny DINO tower's seed and config, three uint8 images with two masks, the pairs, and
the float64 restatement's keys and distances (tests/test_structure_distance_host.py; the weights are weights.dino_state_dict(seed)).

    python tools/make_structure_distance_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_structure_distance_host as H      # noqa: E402


def main():
    seed, S = 5, 45
    imgs, masks = H.make_images(seed, S)
    pairs = np.array([[a, b, -1 if m is None else m, int(c)] for a, b, m, c in H.PAIRS], np.int32)
    np.savez_compressed(H.GOLDEN, seed=seed, cfg=np.array([H.TINY[k] for k in ("image_size", "patch", "width", "layers", "heads", "intermediate")]),
                        images=imgs, masks=masks, pairs=pairs, keys=np.zeros(0), dist=np.zeros(0))
    fx = H.Fixture()
    ref = fx.reference()
    np.savez_compressed(H.GOLDEN, seed=seed, cfg=fx.z["cfg"], images=imgs, masks=masks, pairs=pairs, keys=ref["keys"].numpy(), dist=ref["dist"])
    print("%s: %d bytes, distances %s" % (H.GOLDEN, os.path.getsize(H.GOLDEN), ref["dist"]))


if __name__ == "__main__":
    main()
