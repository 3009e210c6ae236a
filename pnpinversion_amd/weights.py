"""Synthetic, seeded Stable-Diffusion-1.x weights in the diffusers state-dict layout (keys of UNet2DConditionModel /
AutoencoderKL, identical in diffusers 0.3.0 .. 0.10.0 for this architecture; see models/edict/my_diffusers/models/*).

There are no SD checkpoints on the build / GPU boxes (no network), so parity and benchmarks use these.  Every tensor is drawn
from a counter-based generator keyed by (seed, key name), so any process regenerates the identical value without shipping
files, and every value is exactly representable in fp16 (the device arithmetic type), which keeps the CPU oracle and the HIP
path on bit-identical parameters.  A real checkpoint loads through the same `load_state_dict` path unchanged."""
import zlib

import numpy as np
import torch

from .config import ModelConfig


def _gen(seed, name):
    return np.random.Generator(np.random.Philox(key=[seed & 0xFFFFFFFF, zlib.crc32(name.encode())]))


def _fp16_round(a):
    return a.astype(np.float16).astype(np.float32)


def _w(sd, seed, name, shape, fan_in, gain=1.0):
    # variance-preserving uniform init: var = gain^2 / fan_in
    bound = gain * np.sqrt(3.0 / fan_in)
    a = _gen(seed, name).uniform(-bound, bound, size=shape).astype(np.float32)
    sd[name] = torch.from_numpy(_fp16_round(a))


def _b(sd, seed, name, n, scale=0.05):
    a = (_gen(seed, name).standard_normal(n) * scale).astype(np.float32)
    sd[name] = torch.from_numpy(_fp16_round(a))


def _norm(sd, seed, pre, n):
    g = (1.0 + 0.1 * _gen(seed, pre + ".weight").standard_normal(n)).astype(np.float32)
    sd[pre + ".weight"] = torch.from_numpy(_fp16_round(g))
    _b(sd, seed, pre + ".bias", n, 0.1)


def _conv(sd, seed, pre, cin, cout, k, gain=1.0):
    _w(sd, seed, pre + ".weight", (cout, cin, k, k), cin * k * k, gain)
    _b(sd, seed, pre + ".bias", cout)


def _lin(sd, seed, pre, cin, cout, bias=True, gain=1.0):
    _w(sd, seed, pre + ".weight", (cout, cin), cin, gain)
    if bias:
        _b(sd, seed, pre + ".bias", cout)


def _resnet(sd, seed, pre, cin, cout, temb):
    _norm(sd, seed, pre + ".norm1", cin)
    _conv(sd, seed, pre + ".conv1", cin, cout, 3)
    if temb:
        _lin(sd, seed, pre + ".time_emb_proj", temb, cout)
    _norm(sd, seed, pre + ".norm2", cout)
    _conv(sd, seed, pre + ".conv2", cout, cout, 3, gain=0.7)
    if cin != cout:
        _conv(sd, seed, pre + ".conv_shortcut", cin, cout, 1)


def _transformer(sd, seed, pre, c, cross):
    _norm(sd, seed, pre + ".norm", c)
    _conv(sd, seed, pre + ".proj_in", c, c, 1)
    tb = pre + ".transformer_blocks.0"
    for n in ("norm1", "norm2", "norm3"):
        _norm(sd, seed, tb + "." + n, c)
    for a, kdim in (("attn1", c), ("attn2", cross)):
        _lin(sd, seed, tb + "." + a + ".to_q", c, c, bias=False, gain=1.2)
        _lin(sd, seed, tb + "." + a + ".to_k", kdim, c, bias=False, gain=1.2)
        _lin(sd, seed, tb + "." + a + ".to_v", kdim, c, bias=False)
        _lin(sd, seed, tb + "." + a + ".to_out.0", c, c, gain=0.7)
    _lin(sd, seed, tb + ".ff.net.0.proj", c, 8 * c)
    _lin(sd, seed, tb + ".ff.net.2", 4 * c, c, gain=0.7)
    _conv(sd, seed, pre + ".proj_out", c, c, 1, gain=0.7)


def unet_state_dict(cfg: ModelConfig, seed=0):
    sd = {}
    boc = cfg.block_out_channels
    n = len(boc)
    c0, te = boc[0], 4 * boc[0]
    _conv(sd, seed, "conv_in", cfg.in_channels, c0, 3)
    _lin(sd, seed, "time_embedding.linear_1", c0, te)
    _lin(sd, seed, "time_embedding.linear_2", te, te)
    out = c0
    for i in range(n):
        cin, out = out, boc[i]
        for j in range(cfg.layers_per_block):
            _resnet(sd, seed, "down_blocks.%d.resnets.%d" % (i, j), cin if j == 0 else out, out, te)
            if cfg.block_has_attn[i]:
                _transformer(sd, seed, "down_blocks.%d.attentions.%d" % (i, j), out, cfg.cross_dim)
        if i != n - 1:
            _conv(sd, seed, "down_blocks.%d.downsamplers.0.conv" % i, out, out, 3)
    cl = boc[-1]
    _resnet(sd, seed, "mid_block.resnets.0", cl, cl, te)
    _transformer(sd, seed, "mid_block.attentions.0", cl, cfg.cross_dim)
    _resnet(sd, seed, "mid_block.resnets.1", cl, cl, te)
    rev = list(reversed(boc))
    out = rev[0]
    for i in range(n):
        prev, out = out, rev[i]
        cin = rev[min(i + 1, n - 1)]
        for j in range(cfg.layers_per_block + 1):
            skip = cin if j == cfg.layers_per_block else out
            rin = prev if j == 0 else out
            _resnet(sd, seed, "up_blocks.%d.resnets.%d" % (i, j), rin + skip, out, te)
            if cfg.block_has_attn[n - 1 - i]:
                _transformer(sd, seed, "up_blocks.%d.attentions.%d" % (i, j), out, cfg.cross_dim)
        if i != n - 1:
            _conv(sd, seed, "up_blocks.%d.upsamplers.0.conv" % i, out, out, 3)
    _norm(sd, seed, "conv_norm_out", c0)
    _conv(sd, seed, "conv_out", c0, cfg.out_channels, 3)
    return sd


def _vae_attn(sd, seed, pre, c):
    _norm(sd, seed, pre + ".group_norm", c)
    for n in ("query", "key"):
        _lin(sd, seed, pre + "." + n, c, c, gain=1.2)
    _lin(sd, seed, pre + ".value", c, c)
    _lin(sd, seed, pre + ".proj_attn", c, c, gain=0.7)


def vae_state_dict(cfg: ModelConfig, seed=0):
    sd = {}
    vb = cfg.vae_block_out_channels
    n = len(vb)
    L = cfg.vae_latent_channels
    _conv(sd, seed, "encoder.conv_in", cfg.vae_in_channels, vb[0], 3)
    out = vb[0]
    for i in range(n):
        cin, out = out, vb[i]
        for j in range(cfg.vae_layers_per_block):
            _resnet(sd, seed, "encoder.down_blocks.%d.resnets.%d" % (i, j), cin if j == 0 else out, out, 0)
        if i != n - 1:
            _conv(sd, seed, "encoder.down_blocks.%d.downsamplers.0.conv" % i, out, out, 3)
    cl = vb[-1]
    _resnet(sd, seed, "encoder.mid_block.resnets.0", cl, cl, 0)
    _vae_attn(sd, seed, "encoder.mid_block.attentions.0", cl)
    _resnet(sd, seed, "encoder.mid_block.resnets.1", cl, cl, 0)
    _norm(sd, seed, "encoder.conv_norm_out", cl)
    _conv(sd, seed, "encoder.conv_out", cl, 2 * L, 3)
    _conv(sd, seed, "quant_conv", 2 * L, 2 * L, 1)
    _conv(sd, seed, "post_quant_conv", L, L, 1)
    _conv(sd, seed, "decoder.conv_in", L, cl, 3)
    _resnet(sd, seed, "decoder.mid_block.resnets.0", cl, cl, 0)
    _vae_attn(sd, seed, "decoder.mid_block.attentions.0", cl)
    _resnet(sd, seed, "decoder.mid_block.resnets.1", cl, cl, 0)
    rev = list(reversed(vb))
    out = rev[0]
    for i in range(n):
        prev, out = out, rev[i]
        for j in range(cfg.vae_layers_per_block + 1):
            _resnet(sd, seed, "decoder.up_blocks.%d.resnets.%d" % (i, j), prev if j == 0 else out, out, 0)
        if i != n - 1:
            _conv(sd, seed, "decoder.up_blocks.%d.upsamplers.0.conv" % i, out, out, 3)
    _norm(sd, seed, "decoder.conv_norm_out", vb[0])
    _conv(sd, seed, "decoder.conv_out", vb[0], cfg.vae_in_channels, 3)
    return sd


def synth_context(cfg: ModelConfig, rows, seed=0, name="context"):
    """Stand-in text-encoder output [rows, ctx_len, cross_dim] (fp16-representable), LayerNorm-like statistics."""
    a = _gen(seed, name).standard_normal((rows, cfg.ctx_len, cfg.cross_dim)).astype(np.float32)
    return torch.from_numpy(_fp16_round(a))


def clip_state_dict(cfg: ModelConfig, seed=0):
    """transformers CLIPTextModel state dict (key names of transformers >= 5; older releases prefix them with "text_model."),
    seeded, fp16-representable.  Scales follow the HF initialisation loosely; values only need to keep activations O(1)."""
    sd = {}
    H, I = cfg.cross_dim, cfg.clip_intermediate
    e = _gen(seed, "clip.tok").standard_normal((cfg.clip_vocab, H)).astype(np.float32) * 0.02
    sd["embeddings.token_embedding.weight"] = torch.from_numpy(_fp16_round(e))
    e = _gen(seed, "clip.pos").standard_normal((cfg.ctx_len, H)).astype(np.float32) * 0.02
    sd["embeddings.position_embedding.weight"] = torch.from_numpy(_fp16_round(e))
    for l in range(cfg.clip_layers):
        pre = "encoder.layers.%d" % l
        _norm(sd, seed, "clip." + pre + ".layer_norm1", H)
        _norm(sd, seed, "clip." + pre + ".layer_norm2", H)
        for n in ("q_proj", "k_proj", "v_proj"):
            _lin(sd, seed, "clip." + pre + ".self_attn." + n, H, H, gain=1.2)
        _lin(sd, seed, "clip." + pre + ".self_attn.out_proj", H, H, gain=0.5)
        _lin(sd, seed, "clip." + pre + ".mlp.fc1", H, I)
        _lin(sd, seed, "clip." + pre + ".mlp.fc2", I, H, gain=0.5)
    _norm(sd, seed, "clip.final_layer_norm", H)
    return {(k[5:] if k.startswith("clip.") else k): v for k, v in sd.items()}


def clipv_state_dict(image_size=224, patch=14, width=1024, layers=24, heads=16, intermediate=4096, proj_dim=768, text_hidden=768, seed=0):
    """The image tower and the two projections of transformers' CLIPModel (its state-dict keys: vision_model.*, visual_projection.weight,
    text_projection.weight), seeded and fp16-representable like clip_state_dict -- no clip-vit-large-patch14 checkpoint exists offline.
    Scales keep the activations O(1): the patch embedding is variance-preserving over normalised pixels, the residual branches shrink."""
    del heads                                        # the head count shapes no tensor
    sd = {}
    vm = "vision_model."
    T = (image_size // patch) ** 2 + 1
    e = _gen(seed, "clipv.cls").standard_normal(width).astype(np.float32) * 0.5
    sd[vm + "embeddings.class_embedding"] = torch.from_numpy(_fp16_round(e))
    _w(sd, seed, vm + "embeddings.patch_embedding.weight", (width, 3, patch, patch), 3 * patch * patch)
    e = _gen(seed, "clipv.pos").standard_normal((T, width)).astype(np.float32) * 0.5
    sd[vm + "embeddings.position_embedding.weight"] = torch.from_numpy(_fp16_round(e))
    _norm(sd, seed, vm + "pre_layrnorm", width)      # upstream's spelling
    for l in range(layers):
        pre = vm + "encoder.layers.%d" % l
        _norm(sd, seed, pre + ".layer_norm1", width)
        _norm(sd, seed, pre + ".layer_norm2", width)
        for n in ("q_proj", "k_proj", "v_proj"):
            _lin(sd, seed, pre + ".self_attn." + n, width, width, gain=1.2)
        _lin(sd, seed, pre + ".self_attn.out_proj", width, width, gain=0.5)
        _lin(sd, seed, pre + ".mlp.fc1", width, intermediate)
        _lin(sd, seed, pre + ".mlp.fc2", intermediate, width, gain=0.5)
    _norm(sd, seed, vm + "post_layernorm", width)
    _lin(sd, seed, "visual_projection", width, proj_dim, bias=False)
    _lin(sd, seed, "text_projection", text_hidden, proj_dim, bias=False)
    return sd


def dino_state_dict(image_size=224, patch=8, width=768, layers=12, heads=12, intermediate=3072, seed=0):
    """facebookresearch/dino VisionTransformer state dict (its own keys: cls_token, pos_embed, patch_embed.proj.*, blocks.N.*, norm.*),
    seeded and fp16-representable like clipv_state_dict -- no dino_vitbase8_pretrain.pth exists offline.  The structure distance feeds
    the ViT 0..255 pixels normalised with ImageNet mean / std (values of ~5.6e2 +- 3.3e2, up to 1.13e3), so the patch embedding is scaled
    to give O(1) tokens from them: |w| uniform in 0.8e-4 .. 2.4e-4 with a random sign (rms 1.7e-4 -> tokens of ~1.5 rms over 3 p^2 = 192
    inputs; the scale follows 192 / fan_in for other patch sizes).  Every weight stays in fp16's normal range, above 6.1e-5."""
    del heads                                        # the head count shapes no tensor
    sd = {}
    T = (image_size // patch) ** 2 + 1
    K = 3 * patch * patch
    sd["cls_token"] = torch.from_numpy(_fp16_round(_gen(seed, "dino.cls").standard_normal((1, 1, width)).astype(np.float32) * 0.5))
    sd["pos_embed"] = torch.from_numpy(_fp16_round(_gen(seed, "dino.pos").standard_normal((1, T, width)).astype(np.float32) * 0.5))
    g = _gen(seed, "dino.patch_embed.proj.weight")
    mag = g.uniform(0.8e-4, 2.4e-4, size=(width, 3, patch, patch)) * np.sqrt(192.0 / K)
    sign = np.where(g.integers(0, 2, size=mag.shape) == 0, -1.0, 1.0)
    sd["patch_embed.proj.weight"] = torch.from_numpy(_fp16_round((mag * sign).astype(np.float32)))
    _b(sd, seed, "dino.patch_embed.proj.bias", width)
    sd["patch_embed.proj.bias"] = sd.pop("dino.patch_embed.proj.bias")
    for l in range(layers):
        pre = "blocks.%d" % l
        _norm(sd, seed, pre + ".norm1", width)
        _lin(sd, seed, pre + ".attn.qkv", width, 3 * width, gain=1.2)
        _lin(sd, seed, pre + ".attn.proj", width, width, gain=0.5)
        _norm(sd, seed, pre + ".norm2", width)
        _lin(sd, seed, pre + ".mlp.fc1", width, intermediate)
        _lin(sd, seed, pre + ".mlp.fc2", intermediate, width, gain=0.5)
    _norm(sd, seed, "norm", width)
    return sd


# squeezenet1_1().features' Fire blocks: (index, in, squeeze, expand) -- each of expand1x1 / expand3x3 gives `expand` channels
LPIPS_FIRES = ((3, 64, 16, 64), (4, 128, 16, 64), (6, 128, 32, 128), (7, 256, 32, 128), (9, 256, 48, 192), (10, 384, 48, 192),
               (11, 384, 64, 256), (12, 512, 64, 256))
LPIPS_TAP_CHANNELS = (64, 128, 256, 384, 384, 512, 512)       # the outputs of features 1, 4, 7, 9, 10, 11, 12


def lpips_state_dict(seed=0):
    """What lpips.Lpips.load_state_dict takes: torchvision's squeezenet1_1 keys (features.0.*, features.N.{squeeze, expand1x1,
    expand3x3}.*) and the lpips package's lin layers as lin{k}.weight [1, C, 1, 1], seeded and fp16-representable -- neither file exists
    offline.  The convolutions are He-scaled (variance 2 / fan_in) so that the ReLU activations neither die nor leave fp16's range over
    the 17 layers; features.0 sees the ScalingLayer's output (|x| up to 2.7).  The lin weights are non-negative, as the trained ones
    are (the kernel does not assume it)."""
    sd = {}
    he = float(np.sqrt(2.0))
    _conv(sd, seed, "features.0", 3, 64, 3, gain=he)
    for idx, cin, sq, ex in LPIPS_FIRES:
        pre = "features.%d" % idx
        _conv(sd, seed, pre + ".squeeze", cin, sq, 1, gain=he)
        _conv(sd, seed, pre + ".expand1x1", sq, ex, 1, gain=he)
        _conv(sd, seed, pre + ".expand3x3", sq, ex, 3, gain=he)
    for k, ch in enumerate(LPIPS_TAP_CHANNELS):
        a = _gen(seed, "lpips.lin%d" % k).uniform(0.0, 1.0, size=(1, ch, 1, 1)).astype(np.float32)
        sd["lin%d.weight" % k] = torch.from_numpy(_fp16_round(a))
    return sd
