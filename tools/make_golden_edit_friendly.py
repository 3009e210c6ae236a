#!/usr/bin/env python
"""Golden fixtures of the edit-friendly DDPM inversion + P2P editor (run_editing_edit_friendly_p2p.py), produced by the reference's OWN
models/edit_friendly_ddm/{inversion_utils,ptp_classes,ptp_utils}.py on the oracle's fp32 model (oracle/ref_shim.py, CPU, seeded weights).
Build container only (needs the reference tree); the fixtures are committed under tests/golden/.

  e2e_edit_friendly.npz      SMALL64, 6 steps, skip 2: one AttentionReplace pair and one AttentionRefine pair
  e2e_edit_friendly_sd1.npz  SD-1.x width, 10 steps, skip 2, AttentionReplace

Both cases share the source prompt, so the forward process is stored once: w0 (the encoded source latent, fp32), xts[1:] (fp32; xts[0] is
NaN in the reference and not stored; levels `xts_index` only for the full-width file), zs (fp16).  Per case: the edited latents [src, tgt]
(fp16) and the decoded images 4x subsampled.  fp16 storage rounds at ~5e-4 relative, far inside the 1.5e-2 bars of those quantities; every
committed file stays under 1 MiB.  The noise of sample_xts_from_x0 is the CPU generator's stream after torch.manual_seed(noise_seed):
the seed is stored, not the draws.  ETA = 1, source / target guidance 1 / 7.5, cross / self replace 0.4 / 0.6, as the script.

    python tools/make_golden_edit_friendly.py [small64] [sd1]"""
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_shim  # noqa: E402
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SD1, SMALL64  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder, WordTokenizer  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
PAIRS = {
    "replace": ("a cat sitting on a wooden chair", "a dog sitting on a wooden chair"),
    "refine": ("a cat sitting on a wooden chair", "a cat sitting on a big wooden chair"),
}


class _Out(dict):
    __getattr__ = dict.__getitem__


def build_model(cfg, seed, steps):
    ref_shim.install()
    if "cv2" not in sys.modules:                    # ptp_utils.py imports cv2 (only its display helpers use it)
        sys.modules["cv2"] = types.ModuleType("cv2")
    import diffusers
    h = ref_shim._Holder()
    unet = ref_shim.build_unet(cfg, weights.unet_state_dict(cfg, seed))
    unet.sample_size = cfg.sample_size
    fwd = unet.forward
    unet.forward = lambda *a, **k: _Out(fwd(*a, **k))          # the fork returns a dict; inversion_utils reads .sample
    h.unet = unet
    h.vae = ref_shim.build_vae(cfg, weights.vae_state_dict(cfg, seed))
    h.tokenizer = WordTokenizer()
    h.text_encoder = SyntheticTextEncoder(cfg.cross_dim, seed=7)
    h.scheduler = diffusers.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                                          set_alpha_to_one=False)
    h.scheduler.set_timesteps(steps)
    h.device = torch.device("cpu")
    return h


def run_case(model, img, src, tgt, steps, skip, noise_seed):
    from models.edit_friendly_ddm.inversion_utils import inversion_forward_process, inversion_reverse_process
    from models.edit_friendly_ddm.ptp_classes import AttentionRefine, AttentionReplace, AttentionStore
    from models.edit_friendly_ddm.ptp_utils import register_attention_control
    image_gt = torch.from_numpy(img).float() / 127.5 - 1
    image_gt = image_gt.permute(2, 0, 1).unsqueeze(0)
    with torch.no_grad():
        w0 = (model.vae.encode(image_gt)["latent_dist"].mode() * 0.18215).float()
        register_attention_control(model, AttentionStore())
        torch.manual_seed(noise_seed)
        _, zs, wts = inversion_forward_process(model, w0, etas=1, prompt=src, cfg_scale=1, prog_bar=False, num_inference_steps=steps)
        cls = AttentionReplace if len(src.split(" ")) == len(tgt.split(" ")) else AttentionRefine
        controller = cls([src, tgt], steps, cross_replace_steps=0.4, self_replace_steps=0.6, model=model)
        register_attention_control(model, controller)
        lat, _ = inversion_reverse_process(model, xT=wts[steps - skip], etas=1, prompts=[src, tgt], cfg_scales=[1, 7.5], prog_bar=False,
                                           zs=zs[:(steps - skip)], controller=controller)
        dec = model.vae.decode(1 / 0.18215 * lat)
        dec = dec["sample"] if isinstance(dec, dict) else dec.sample
    imgs = np.uint8(np.clip(dec.permute(0, 2, 3, 1).numpy() / 2 + 0.5, 0, 1) * 255)
    return dict(w0=w0.numpy(), xts=wts[1:].numpy(), zs=zs.numpy(), edited_latents=lat.numpy().astype(np.float16),
                images_small=imgs[:, ::4, ::4], is_replace=np.bool_(cls is AttentionReplace))


def make(name, cfg, steps, skip, cases, weight_seed=2, noise_seed=1234, xts_index=None):
    from PIL import Image
    t0 = time.time()
    model = build_model(cfg, weight_seed, steps)
    img = np.array(Image.open(os.path.join(OUT, "example_cat_512.png")))[:, :, :3]
    out = dict(steps=np.int64(steps), skip=np.int64(skip), weight_seed=np.int64(weight_seed), noise_seed=np.int64(noise_seed),
               cases=np.array(cases))
    xi = np.arange(steps) if xts_index is None else np.asarray(xts_index, np.int64)      # into xts[1:]
    for c in cases:
        src, tgt = PAIRS[c]
        r = run_case(model, img, src, tgt, steps, skip, noise_seed)
        shared = dict(w0=r.pop("w0"), xts=r.pop("xts")[xi], zs=r.pop("zs").astype(np.float16))
        if "w0" in out:     # same source prompt and image: the forward process must be the same computation
            assert all(np.array_equal(out[k], v) for k, v in shared.items())
        out.update(shared)
        out.update({"%s_%s" % (c, k): v for k, v in r.items()})
        out["%s_tgt" % c] = np.array(tgt)
        out["src"] = np.array(src)
        print(name, c, "%.1fs" % (time.time() - t0), flush=True)
    out["xts_index"] = xi
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["small64", "sd1"]
    torch.set_num_threads(os.cpu_count() or 1)
    if "small64" in which:
        make("e2e_edit_friendly", SMALL64, 6, 2, ["replace", "refine"])
    if "sd1" in which:
        make("e2e_edit_friendly_sd1", SD1, 10, 2, ["replace"], xts_index=[0, 2, 4, 6, 7, 9])
