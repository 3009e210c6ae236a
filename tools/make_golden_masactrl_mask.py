#!/usr/bin/env python
"""Golden fixtures of mask-guided MasaCtrl, produced by the reference's OWN MutualSelfAttentionControlMask (models/masactrl/masactrl.py:
114-193) and regiter_attention_editor_diffusers (masactrl_utils.py:79-144), imported from the reference tree through oracle/ref_shim.py, on
the CPU in fp32.  Build container only (needs the reference tree); the fixtures are committed under tests/golden/.

  masactrl_mask_attn.npz   kernel level: the class's forward on one head at the SD-1.x head widths and map sizes (d = 40 at 64^2, 80 at 32^2,
                           160 at 16^2) and the narrow test width (d = 16 at 16^2), five mask pairs each; q / k / v are small integers
                           (N(0, 1) rounded: fp16-exact, stored as int8), the outputs of a fixed sample of 48 query rows are kept (fp32), plus the plain
                           mutual self-attention output of the same rows (the parent class's attn_batch)
  e2e_masactrl_mask.npz    SMALL64 (weight seed 2, the model of e2e_masactrl.npz), the reference's MasaCtrlPipeline.__call__ on ["", tgt] from
                           the inverted latent of e2e_masactrl.npz's ddim+masactrl run, 4 steps, control from step 1 in blocks 8..15
                           (16^2, 32^2 and 64^2 maps), a 64 x 64 rectangle pair; the latent after every step; and the same for a second
                           mask pair whose foreground vanishes at the 16^2 level (the uniform fall-back inside a whole edit)

Patches, and nothing else of the reference is restated:
  1. torchvision / cv2 are not installed: ref_shim._install_fake_vision() provides empty modules; torchvision.utils.save_image is a no-op
     (only mask_save_dir would call it, and it is None here).
  2. ref_shim.build_masactrl_editor: from_pretrained is skipped (seeded weights), the fork's CrossAttention modules get the class name
     `Attention` the hook looks for, the UNet's dict output gains attribute access, `.to("cuda")` stays on the CPU (ref_shim.cuda_to_cpu).
  3. MasaCtrlPipeline.step is wrapped to RECORD the latent it returns (the per-step latents); it computes what it always does.
  4. builtins.print is silenced inside the class's forward (it prints "masked attention" per call).

    python tools/make_golden_masactrl_mask.py [attn] [e2e]"""
import builtins
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SMALL64  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder, WordTokenizer  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIZES = (("d40", 40, 64), ("d80", 80, 32), ("d160", 160, 16), ("d16", 16, 16))       # tag, head width, map side
CASES = ("rect", "empty_fg", "full_fg", "single_key", "full_t")
NSEL = 48


@contextlib.contextmanager
def quiet():
    p = builtins.print
    builtins.print = lambda *a, **k: None
    try:
        yield
    finally:
        builtins.print = p


def masks_for(case, side, rng):
    """(mask_s, mask_t) at the map's own size (F.interpolate to the same size is the identity)"""
    s, t = np.zeros((side, side), np.float32), np.zeros((side, side), np.float32)
    a, b = side // 4 + 1, (3 * side) // 4 - 2          # rectangle edges off the 64-key tile grid (rows are `side` keys long)
    if case == "rect":
        s[a:b, a + 1:b + 2] = 1
        t[a - 1:b - 3, a + 2:b] = 1
    elif case == "empty_fg":                            # no foreground key: the foreground queries of mask_t fall back to uniform
        t[a:b, a:b] = 1
    elif case == "full_fg":                             # no background key: the background queries fall back
        s[:] = 1
        t[a:b, a:b] = 1
    elif case == "single_key":
        s[side // 2 + 1, side // 3] = 1
        t[a:b, a:b] = 1
    elif case == "full_t":
        s[:] = (rng.random((side, side)) < 0.3).astype(np.float32)
        t[:] = 1
    return s, t


def run_attn():
    ref_shim.install()
    ref_shim._install_fake_vision()                                                              # patch 1
    from models.masactrl.masactrl import MutualSelfAttentionControl, MutualSelfAttentionControlMask
    rng = np.random.default_rng(11)
    out = dict(cases=np.array(CASES), tags=np.array([s[0] for s in SIZES]))
    for tag, d, side in SIZES:
        n = side * side
        q8, k8, v8 = (np.clip(np.rint(rng.standard_normal((2, n, d))), -3, 3).astype(np.int8) for _ in range(3))
        q, k, v = (torch.from_numpy(x.astype(np.float32)) for x in (q8, k8, v8))          # [2 (src, tgt), n, d]
        scale = d ** -0.5
        sel = np.sort(rng.choice(n, NSEL, replace=False))
        # rows [u_src, u_tgt, c_src, c_tgt], one head (masactrl.py:170-181)
        q4, k4, v4 = (torch.cat([x, x]) for x in (q, k, v))
        dummy = torch.zeros(4, 1, 1)
        out.update({tag + "_q": q8, tag + "_k": k8, tag + "_v": v8, tag + "_sel": sel.astype(np.int64), tag + "_side": np.int64(side),
                    tag + "_scale": np.float32(scale)})
        with quiet():
            plain_ed = MutualSelfAttentionControl(start_step=0, start_layer=0, total_steps=1)
            plain = plain_ed.forward(q4, k4, v4, dummy, dummy, False, "up", 1, scale=scale)      # [4, n, d]; row 1 = tgt over src K / V
        out[tag + "_plain"] = plain[1][sel].numpy()
        for case in CASES:
            ms, mt = masks_for(case, side, rng)
            with quiet():
                ed = MutualSelfAttentionControlMask(start_step=0, start_layer=0, total_steps=1, mask_s=torch.from_numpy(ms),
                                                    mask_t=torch.from_numpy(mt))
                o = ed.forward(q4, k4, v4, dummy, dummy, False, "up", 1, scale=scale)
            assert torch.equal(o[1], o[3]) and torch.equal(o[0], plain[0]) and torch.isfinite(o).all()
            out["%s_%s_mask_s" % (tag, case)] = ms.astype(np.uint8)
            out["%s_%s_mask_t" % (tag, case)] = mt.astype(np.uint8)
            out["%s_%s_out" % (tag, case)] = o[1][sel].numpy()
            print(tag, case, "max |masked - plain| on the kept rows: %.3f" % float((o[1][sel] - plain[1][sel]).abs().max()))
    np.savez_compressed(os.path.join(OUT, "masactrl_mask_attn.npz"), **out)


def run_e2e(steps=4, start_step=1, start_layer=8):
    cfg, seed = SMALL64, 2
    usd, vsd = weights.unet_state_dict(cfg, seed), weights.vae_state_dict(cfg, seed)
    ed = ref_shim.build_masactrl_editor(cfg, usd, vsd, WordTokenizer(), SyntheticTextEncoder(cfg.cross_dim, seed=7), steps)   # patches 1, 2
    from models.masactrl.masactrl import MutualSelfAttentionControlMask
    from models.masactrl.masactrl_utils import regiter_attention_editor_diffusers
    g = np.load(os.path.join(OUT, "e2e_masactrl.npz"))
    x_t = torch.from_numpy(g["ddim+masactrl/x_stars"][-1])
    tgt = str(g["tgt"])
    side = cfg.sample_size
    mask_s, mask_t = np.zeros((2, side, side), np.float32), np.zeros((2, side, side), np.float32)
    mask_s[0, 13:41, 19:50] = 1          # image 0: two overlapping rectangles, edges off every level's 2x / 4x grid
    mask_t[0, 17:47, 11:45] = 1
    mask_s[1, 21, 33] = 1                # image 1: a one-pixel source foreground at odd coordinates: gone at 32^2 and 16^2 (nearest reads
    mask_t[1, 9:30, 30:60] = 1           # even pixels) -> the foreground queries of those levels take the uniform fall-back
    rec = []
    pipe = ed.model
    step = pipe.step

    def rec_step(*a, **k):                                                                       # patch 3
        r = step(*a, **k)
        rec.append(r[0].clone())
        return r

    pipe.step = rec_step
    out = dict(steps=np.int64(steps), start_step=np.int64(start_step), start_layer=np.int64(start_layer), tgt=np.array(tgt),
               weight_seed=np.int64(seed), x_t=x_t.numpy(), mask_s=mask_s.astype(np.uint8), mask_t=mask_t.astype(np.uint8))
    try:
        with ref_shim.cuda_to_cpu(), torch.no_grad(), quiet():                                   # patch 4
            for im in range(2):
                del rec[:]
                editor = MutualSelfAttentionControlMask(start_step, start_layer, total_steps=steps, mask_s=torch.from_numpy(mask_s[im]),
                                                        mask_t=torch.from_numpy(mask_t[im]))
                regiter_attention_editor_diffusers(pipe, editor)
                pipe(["", tgt], latents=x_t.expand(2, -1, -1, -1), num_inference_steps=steps, guidance_scale=7.5)
                assert len(rec) == steps
                out["latents_steps_%d" % im] = torch.stack(rec).numpy()                          # [steps, 2, 4, 64, 64]
    finally:
        pipe.step = step
    np.savez_compressed(os.path.join(OUT, "e2e_masactrl_mask.npz"), **out)
    for im in range(2):
        print("e2e image", im, out["latents_steps_%d" % im].shape,
              "target rows of the two images differ by %.3f" % float(np.abs(out["latents_steps_0"][-1, 1] - out["latents_steps_%d" % im][-1, 1]).mean()))


if __name__ == "__main__":
    torch.set_num_threads(8)          # tests/test_masactrl_mask_host.py restates the attention bit for bit under the same thread count
    which = sys.argv[1:] or ["attn", "e2e"]
    if "attn" in which:
        run_attn()
    if "e2e" in which:
        run_e2e()
