"""Record tests/golden/e2e_ip2p_tiny.npz from the reference's own modules (build container only; needs the reference tree):

    python tools/make_golden_ip2p.py --reference /path/to/PnPInversion [--out tests/golden/e2e_ip2p_tiny.npz]

The reference's ldm `UNetModel` (openaimodel.py) at the TINY16_IP2P shape and its `Encoder` / `Decoder` (diffusionmodules/model.py) run on
the CPU in fp32 inside the sampler of run_editing_instructpix2pix.py (:33-46, :125-135) with k-diffusion's three functions restated
(pnpinversion_amd/instructpix2pix.py -- k_diffusion is not part of the reference tree).  The weights are this project's seeded synthetic
ones, renamed BY HAND here into ldm's layout and loaded with strict=True: the fixture keeps the (ldm key, source key) lists -- names only
-- so that a test can rebuild the ldm-layout state dict and check checkpoint.convert_ldm_state_dict against what ldm itself accepted.

The fixture holds data only: key lists, draws, sigmas, fractional timesteps, the three eps rows and z of every step, the image latent and
the decoded image.  omegaconf is not installed: openaimodel.py imports ListConfig from it for one isinstance test, so a three-line stand-in
is registered before the import (here, never in the package)."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pnpinversion_amd import instructpix2pix as ip  # noqa: E402
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import TINY16_IP2P  # noqa: E402

SEED, NSTEPS, GT, GI = 2, 8, 7.5, 1.5
RES = {"norm1": "in_layers.0", "conv1": "in_layers.2", "time_emb_proj": "emb_layers.1", "norm2": "out_layers.0", "conv2": "out_layers.3",
       "conv_shortcut": "skip_connection"}


def unet_to_ldm(cfg, keys):
    """project (diffusers-layout) UNet key -> ldm key, written out level by level"""
    lpb, nb, out = cfg.layers_per_block, cfg.n_blocks, {}
    for k in keys:
        p = k.split(".")
        if p[0] == "time_embedding":
            n = "time_embed.%d.%s" % ({"linear_1": 0, "linear_2": 2}[p[1]], p[2])
        elif p[0] == "conv_in":
            n = "input_blocks.0.0." + p[1]
        elif p[0] == "conv_norm_out":
            n = "out.0." + p[1]
        elif p[0] == "conv_out":
            n = "out.2." + p[1]
        elif p[0] == "down_blocks":
            b = int(p[1])
            if p[2] == "downsamplers":
                n = "input_blocks.%d.0.op.%s" % (1 + b * (lpb + 1) + lpb, p[5])
            else:
                i = 1 + b * (lpb + 1) + int(p[3])
                n = "input_blocks.%d.0.%s.%s" % (i, RES[p[4]], p[5]) if p[2] == "resnets" else "input_blocks.%d.1.%s" % (i, ".".join(p[4:]))
        elif p[0] == "mid_block":
            n = "middle_block.%d.%s.%s" % (2 * int(p[2]), RES[p[3]], p[4]) if p[1] == "resnets" else "middle_block.1." + ".".join(p[3:])
        elif p[0] == "up_blocks":
            b = int(p[1])
            has_attn = cfg.block_has_attn[nb - 1 - b]
            if p[2] == "upsamplers":
                n = "output_blocks.%d.%d.conv.%s" % (b * (lpb + 1) + lpb, 2 if has_attn else 1, p[5])
            else:
                i = b * (lpb + 1) + int(p[3])
                n = "output_blocks.%d.0.%s.%s" % (i, RES[p[4]], p[5]) if p[2] == "resnets" else "output_blocks.%d.1.%s" % (i, ".".join(p[4:]))
        else:
            raise KeyError(k)
        out[n] = k
    return out


def vae_to_ldm(cfg, keys):
    nb, out = len(cfg.vae_block_out_channels), {}
    attn = {"group_norm": "norm", "query": "q", "key": "k", "value": "v", "proj_attn": "proj_out"}
    for k in keys:
        p = k.split(".")
        if p[0] in ("quant_conv", "post_quant_conv"):
            n = k
        elif p[1] in ("conv_in", "conv_out"):
            n = k
        elif p[1] == "conv_norm_out":
            n = "%s.norm_out.%s" % (p[0], p[2])
        elif p[1] == "mid_block":
            n = "%s.mid.block_%d.%s" % (p[0], int(p[3]) + 1, ".".join(p[4:])) if p[2] == "resnets" else "%s.mid.attn_1.%s.%s" % (p[0], attn[p[4]], p[5])
        elif p[1] == "down_blocks":
            n = ("encoder.down.%s.block.%s.%s.%s" % (p[2], p[4], "nin_shortcut" if p[5] == "conv_shortcut" else p[5], p[6]) if p[3] == "resnets"
                 else "encoder.down.%s.downsample.conv.%s" % (p[2], p[6]))
        elif p[1] == "up_blocks":
            lvl = nb - 1 - int(p[2])
            n = ("decoder.up.%d.block.%s.%s.%s" % (lvl, p[4], "nin_shortcut" if p[5] == "conv_shortcut" else p[5], p[6]) if p[3] == "resnets"
                 else "decoder.up.%d.upsample.conv.%s" % (lvl, p[6]))
        else:
            raise KeyError(k)
        out[n] = k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "e2e_ip2p_tiny.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.reference, "models", "instructpix2pix", "stable_diffusion"))
    oc, lc = types.ModuleType("omegaconf"), types.ModuleType("omegaconf.listconfig")
    lc.ListConfig = type("ListConfig", (list,), {})
    oc.listconfig = lc
    sys.modules.setdefault("omegaconf", oc), sys.modules.setdefault("omegaconf.listconfig", lc)
    from ldm.modules.diffusionmodules.model import Decoder, Encoder
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from PIL import Image

    torch.set_num_threads(8)
    cfg = TINY16_IP2P
    S = cfg.sample_size
    usd, vsd = weights.unet_state_dict(cfg, SEED), weights.vae_state_dict(cfg, SEED)
    unet = UNetModel(image_size=S, in_channels=8, out_channels=4, model_channels=32, attention_resolutions=[1, 2, 4], num_res_blocks=2,
                     channel_mult=(1, 2, 2, 2), num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=64,
                     use_checkpoint=False, legacy=False).eval()
    umap = unet_to_ldm(cfg, usd)
    unet.load_state_dict({n: usd[k].float() for n, k in umap.items()}, strict=True)
    dd = dict(double_z=True, z_channels=4, resolution=S * 8, in_channels=3, out_ch=3, ch=32, ch_mult=(1, 1, 2, 2), num_res_blocks=2,
              attn_resolutions=[], dropout=0.0)
    enc, dec = Encoder(**dd).eval(), Decoder(**dd).eval()
    vmap = vae_to_ldm(cfg, vsd)

    def conv_w(n, k):                                            # ldm's VAE attention is made of 1 x 1 convolutions
        w = vsd[k].float()
        return w[:, :, None, None] if ".mid.attn_1." in n and n.endswith("weight") and "norm" not in n else w
    enc.load_state_dict({n[len("encoder."):]: conv_w(n, k) for n, k in vmap.items() if n.startswith("encoder.")}, strict=True)
    dec.load_state_dict({n[len("decoder."):]: conv_w(n, k) for n, k in vmap.items() if n.startswith("decoder.")}, strict=True)
    F = torch.nn.functional
    quant = lambda h: F.conv2d(h, vsd["quant_conv.weight"].float(), vsd["quant_conv.bias"].float())              # noqa: E731
    post_quant = lambda z: F.conv2d(z, vsd["post_quant_conv.weight"].float(), vsd["post_quant_conv.bias"].float())    # noqa: E731

    side = S * 8
    image = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "example_cat_512.png")).convert("RGB").resize((side, side), Image.BILINEAR))
    g = torch.Generator().manual_seed(1234)
    sched = ip.SigmaSchedule()
    sigmas = sched.get_sigmas(NSTEPS)
    ts = sched.sigma_to_t(sigmas[:-1])
    ctx2 = weights.synth_context(cfg, 2, seed=77)
    context = torch.stack([ctx2[0], ctx2[1], ctx2[1]])                                             # [edit, null, null]
    draw0 = torch.randn(1, 4, S, S, generator=g)
    draws = torch.stack([torch.randn(1, 4, S, S, generator=g)[0] for _ in range(NSTEPS - 1)])
    with torch.no_grad():
        x = (2 * torch.tensor(image).float() / 255 - 1).permute(2, 0, 1)[None]                     # :117-118
        c_concat = quant(enc(x))[:, :4]                                                            # :119 encode_first_stage(...).mode()
        z = draw0 * sigmas[0]                                                                      # :133
        eps_all, z_all = [], []
        for i in range(NSTEPS):
            s_in = sigmas[i] * torch.ones(3)
            c_in = 1 / (s_in ** 2 + 1) ** 0.5
            zin = torch.cat([z] * 3) * c_in[:, None, None, None]
            cc = torch.cat([c_concat, c_concat, torch.zeros_like(c_concat)])
            eps = unet(torch.cat([zin, cc], 1), sched.sigma_to_t(s_in), context=context)
            noise = draws[i][None] if i < NSTEPS - 1 else torch.full_like(z, float("nan"))
            z = ip.euler_ancestral_step(z, eps[None], noise, sigmas[i], sigmas[i + 1], GT, GI)
            eps_all.append(eps)
            z_all.append(z[0])
        decoded = dec(post_quant(1. / 0.18215 * z))                                                # :135 decode_first_stage
        # a one-row forward at a fractional t on 8 random channels, for the op-level checks
        lat8 = torch.randn(3, 8, S, S, generator=g)
        eps8 = unet(lat8, ts[3].expand(3), context=context)
    assert torch.isfinite(torch.stack(z_all)).all() and all(float(t) != round(float(t)) for t in ts[1:-1])
    sig50 = sched.get_sigmas(50)
    np.savez_compressed(
        args.out, weight_seed=SEED, nsteps=NSTEPS, cfg_text=GT, cfg_image=GI, context_seed=77,
        unet_ldm_keys=np.array(list(umap)), unet_src_keys=np.array(list(umap.values())),
        vae_ldm_keys=np.array(list(vmap)), vae_src_keys=np.array(list(vmap.values())),
        sigmas=sigmas.numpy(), timesteps=ts.numpy(), sigmas50=sig50.numpy(), timesteps50=sched.sigma_to_t(sig50[:-1]).numpy(),
        roundtrip_k=sched.sigma_to_t(sched.t_to_sigma(torch.arange(1000).float())).numpy(),
        image=image, c_concat=c_concat.numpy(), draw0=draw0[0].numpy(), draws=draws.numpy(), context=context.numpy(),
        eps=torch.stack(eps_all).numpy(), z=torch.stack(z_all).numpy(), decoded=decoded[0].numpy(),
        lat8=lat8.numpy(), t8=np.float32(ts[3]), eps8=eps8.numpy())
    print("wrote", args.out, os.path.getsize(args.out), "bytes; t:", ts.numpy())


if __name__ == "__main__":
    main()
