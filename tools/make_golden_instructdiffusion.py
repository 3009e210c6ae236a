"""Record tests/golden/e2e_instdiff_tiny.npz from the reference's own modules (build container only; needs the reference tree):

    python tools/make_golden_instructdiffusion.py --reference /path/to/PnPInversion [--out tests/golden/e2e_instdiff_tiny.npz]

The reference's InstructDiffusion `UNetModel` (models/InstructDiffusion/stable_diffusion/ldm/.../openaimodel.py, force_type_convert=True as
instruct_diffusion.yaml has it) at the TINY16_IP2P shape and its `Encoder` / `Decoder` run on the CPU in fp32 under the reference's own
`CFGDenoiser.forward`, imported from run_editing_instructdiffusion.py (:32-48), inside k-diffusion's CompVisDenoiser and
sample_euler_ancestral restated here (k_diffusion is not part of the reference tree; the schedule is pnpinversion_amd/instructpix2pix.py's,
which the InstructPix2Pix fixture pins bit for bit).  The step is written out here from k-diffusion's loop and does not call
pnpinversion_amd.instructdiffusion: tests/test_instdiff_host.py checks that module against what this run recorded.

Weights, image, context seed, draws' seed and step count are those of tools/make_golden_ip2p.py (whose key maps are imported), the scales
are the reference's defaults cfg_text = 5.0, cfg_image = 1.25.  The fixture holds data only: key lists, draws, sigmas, fractional
timesteps, the three eps rows and z of every step, the image latent and the decoded image.

force_type_convert = True makes SpatialTransformer.forward run its GroupNorm in fp32 and cast the result with `.half()` for the fp16 weights
that autocast / DeepSpeed give it; against fp32 weights that cast raises (dtype mismatch at proj_in).  For this fp32 run `Tensor.half` is the
identity while the UNet runs (keep_fp32), and the first step's rows are checked bit for bit against the same weights in a UNetModel built
with force_type_convert = False: the flag moves dtypes and nothing else.

k_diffusion, omegaconf and deepspeed are not installed and the reference's modules import them at the top (none is called on this path):
stand-in modules are registered before the import (here, never in the package); `requests` is stood in for only where it is missing."""
import argparse
import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from make_golden_ip2p import unet_to_ldm, vae_to_ldm  # noqa: E402  (tools/ is this script's directory)
from pnpinversion_amd import instructpix2pix as ip  # noqa: E402
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import TINY16_IP2P  # noqa: E402

SEED, NSTEPS, GT, GI = 2, 8, 5.0, 1.25


def stand_ins():
    oc, lc = types.ModuleType("omegaconf"), types.ModuleType("omegaconf.listconfig")
    lc.ListConfig = type("ListConfig", (list,), {})
    oc.listconfig, oc.OmegaConf = lc, type("OmegaConf", (), {})
    mods = {"omegaconf": oc, "omegaconf.listconfig": lc, "k_diffusion": types.ModuleType("k_diffusion"),
            "deepspeed": types.ModuleType("deepspeed")}
    try:
        importlib.import_module("requests")
    except ImportError:
        mods["requests"] = types.ModuleType("requests")
    for name, m in mods.items():
        sys.modules.setdefault(name, m)


@contextlib.contextmanager
def keep_fp32():
    half = torch.Tensor.half
    torch.Tensor.half = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.half = half


class CompVisDenoiser(torch.nn.Module):
    """K.external.CompVisDenoiser (quantize = False) around ldm's DiffusionWrapper with conditioning_key "hybrid": forward is
    DiscreteEpsDDPMDenoiser.forward, get_eps is apply_model.  Keeps the eps of every call."""

    def __init__(self, unet, schedule):
        super().__init__()
        self.unet, self.schedule, self.sigma_data, self.eps = unet, schedule, 1., []

    def get_eps(self, x, t, cond):
        xc = torch.cat([x] + cond["c_concat"], dim=1)
        cc = torch.cat(cond["c_crossattn"], 1)
        with keep_fp32():
            return self.unet(xc, t, context=cc)

    def forward(self, input, sigma, **kwargs):
        c_out = -sigma
        c_in = 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5
        c_out, c_in = (x[(...,) + (None,) * (input.ndim - x.ndim)] for x in (c_out, c_in))          # utils.append_dims
        eps = self.get_eps(input * c_in, self.schedule.sigma_to_t(sigma), **kwargs)
        self.eps.append(eps)
        return input + eps * c_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "e2e_instdiff_tiny.npz"))
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    sys.path.insert(0, os.path.join(ref, "models", "InstructDiffusion", "stable_diffusion"))
    sys.path.insert(1, ref)                                      # run_editing_instructdiffusion.py and its utils.utils
    stand_ins()
    from ldm.modules.diffusionmodules.model import Decoder, Encoder
    from ldm.modules.diffusionmodules.openaimodel import UNetModel
    from PIL import Image
    from run_editing_instructdiffusion import CFGDenoiser

    torch.set_num_threads(8)
    cfg = TINY16_IP2P
    S = cfg.sample_size
    usd, vsd = weights.unet_state_dict(cfg, SEED), weights.vae_state_dict(cfg, SEED)
    shape = dict(image_size=S, in_channels=8, out_channels=4, model_channels=32, attention_resolutions=[1, 2, 4], num_res_blocks=2,
                 channel_mult=(1, 2, 2, 2), num_heads=8, use_spatial_transformer=True, transformer_depth=1, context_dim=64,
                 use_checkpoint=False, legacy=False)
    unet, plain = UNetModel(force_type_convert=True, **shape).eval(), UNetModel(force_type_convert=False, **shape).eval()
    umap = unet_to_ldm(cfg, usd)
    for m in (unet, plain):
        m.load_state_dict({n: usd[k].float() for n, k in umap.items()}, strict=True)
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
    sigmas = sched.get_sigmas(NSTEPS)                                                              # :110
    ts = sched.sigma_to_t(sigmas[:-1])
    ctx2 = weights.synth_context(cfg, 2, seed=77)                                                  # [instruction, null]
    draw0 = torch.randn(1, 4, S, S, generator=g)
    draws = torch.stack([torch.randn(1, 4, S, S, generator=g)[0] for _ in range(NSTEPS - 1)])
    model_wrap = CompVisDenoiser(unet, sched)
    model_wrap_cfg = CFGDenoiser(model_wrap)                                                       # the reference's class
    with torch.no_grad():
        x = (2 * torch.tensor(image).float() / 255 - 1).permute(2, 0, 1)[None]                     # :102-103
        c_concat = quant(enc(x))[:, :4]                                                            # :104 encode_first_stage(...).mode()
        cond = {"c_crossattn": [ctx2[0:1]], "c_concat": [c_concat]}
        uncond = {"c_crossattn": [ctx2[1:2]], "c_concat": [torch.zeros_like(c_concat)]}            # :106-108
        extra_args = {"cond": cond, "uncond": uncond, "text_cfg_scale": GT, "image_cfg_scale": GI}
        z = draw0 * sigmas[0]                                                                      # :119
        z_all = []
        s_in = z.new_ones([z.shape[0]])
        for i in range(NSTEPS):                                                                    # K.sampling.sample_euler_ancestral, eta = s_noise = 1
            denoised = model_wrap_cfg(z, sigmas[i] * s_in, **extra_args)
            sigma_down, sigma_up = ip.get_ancestral_step(sigmas[i], sigmas[i + 1])
            d = (z - denoised) / sigmas[i]                                                         # to_d
            dt = sigma_down - sigmas[i]
            z = z + d * dt
            if sigmas[i + 1] > 0:
                z = z + draws[i][None] * 1.0 * sigma_up
            z_all.append(z[0])
        decoded = dec(post_quant(1. / 0.18215 * z))                                                # :121 decode_first_stage
    eps = torch.stack(model_wrap.eps)
    with torch.no_grad():
        z0 = draw0 * sigmas[0]
        rows = torch.cat([torch.cat([z0] * 3) * (1 / (sigmas[0] ** 2 + 1) ** 0.5),torch.cat([c_concat, c_concat, torch.zeros_like(c_concat)])], 1)
        assert torch.equal(plain(rows, ts[:1].expand(3), context=torch.stack([ctx2[0], ctx2[1], ctx2[0]])), eps[0])
    assert eps.shape == (NSTEPS, 3, 4, S, S) and torch.isfinite(torch.stack(z_all)).all()
    assert all(float(t) != round(float(t)) for t in ts[1:-1])
    context = torch.stack([ctx2[0], ctx2[1], ctx2[0]])                                             # the rows of :41: [instruction, null, instruction]
    np.savez_compressed(
        args.out, weight_seed=SEED, nsteps=NSTEPS, cfg_text=GT, cfg_image=GI, context_seed=77,
        unet_ldm_keys=np.array(list(umap)), unet_src_keys=np.array(list(umap.values())),
        vae_ldm_keys=np.array(list(vmap)), vae_src_keys=np.array(list(vmap.values())),
        sigmas=sigmas.numpy(), timesteps=ts.numpy(),
        image=image, c_concat=c_concat.numpy(), draw0=draw0[0].numpy(), draws=draws.numpy(), context=context.numpy(),
        eps=eps.numpy(), z=torch.stack(z_all).numpy(), decoded=decoded[0].numpy())
    print("wrote", args.out, os.path.getsize(args.out), "bytes; t:", ts.numpy())


if __name__ == "__main__":
    main()
