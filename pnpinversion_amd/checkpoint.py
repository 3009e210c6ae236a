"""Loading a Stable-Diffusion-1.x checkpoint directory in the diffusers layout -- what the reference gets from
`StableDiffusionPipeline.from_pretrained("CompVis/stable-diffusion-v1-4", ...)` (models/p2p_editor.py:23-24):

    <dir>/unet/diffusion_pytorch_model.{safetensors,bin}      UNet2DConditionModel state dict
    <dir>/vae/diffusion_pytorch_model.{safetensors,bin}       AutoencoderKL state dict
    <dir>/text_encoder/{model.safetensors,pytorch_model.bin}  transformers CLIPTextModel state dict
    <dir>/tokenizer/{vocab.json,merges.txt}                   CLIP byte-level BPE vocabulary -> text.ClipBPETokenizer

No checkpoint exists on the build / GPU boxes (no network), so the runs there use seeded synthetic weights; this module is the
path a user with a real checkpoint takes (`--checkpoint_dir` of the drivers, `P2PEditor(..., checkpoint_dir=...)`)."""
import os
import sys

import torch


def _load_sd(folder, names):
    for n in names:
        p = os.path.join(folder, n)
        if os.path.exists(p):
            if p.endswith(".safetensors"):
                from safetensors.torch import load_file
                return load_file(p)
            return torch.load(p, map_location="cpu", weights_only=True)
    raise FileNotFoundError("none of %s under %s" % (", ".join(names), folder))


def load_checkpoint_dir(path):
    """-> (unet_sd, vae_sd, clip_sd, tokenizer)"""
    from .text import ClipBPETokenizer
    if not os.path.isdir(path):
        raise FileNotFoundError("checkpoint directory %r does not exist" % path)
    model_files = ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors", "diffusion_pytorch_model.bin")
    unet = _load_sd(os.path.join(path, "unet"), model_files)
    vae = _load_sd(os.path.join(path, "vae"), model_files)
    clip = _load_sd(os.path.join(path, "text_encoder"), ("model.safetensors", "model.fp16.safetensors", "pytorch_model.bin"))
    clip = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in clip.items() if "position_ids" not in k}
    tok = ClipBPETokenizer(os.path.join(path, "tokenizer", "vocab.json"), os.path.join(path, "tokenizer", "merges.txt"))
    return unet, vae, clip, tok


def load_clip_model_dir(path, text_sd=None, atol=1e-3):
    """A local `openai/clip-vit-large-patch14` directory (model.safetensors or pytorch_model.bin: transformers CLIPModel) -> the state
    dict ClipScore.load_state_dict takes: vision_model.*, visual_projection.weight, text_projection.weight.
    text_sd: the CLIPTextModel state dict already loaded from the SD checkpoint (load_checkpoint_dir's third value).  CLIP similarity
    runs the image tower of THIS directory against the text tower of THAT one, which is right only if they are the same network (SD-1.x
    conditions on clip-vit-large-patch14's text tower): every text_model.* tensor here must match it within atol (fp16 checkpoints), or
    ValueError names the first that does not.
    Nothing offline can exercise this function -- no clip-vit-large-patch14 checkpoint exists on the build / GPU boxes; the tests run
    seeded towers (weights.clipv_state_dict) through the same ClipScore.load_state_dict."""
    if not os.path.isdir(path):
        raise FileNotFoundError("CLIP model directory %r does not exist" % path)
    sd = _load_sd(path, ("model.safetensors", "pytorch_model.bin"))
    out = {k: v for k, v in sd.items() if (k.startswith("vision_model.") and "position_ids" not in k) or k in ("visual_projection.weight", "text_projection.weight")}
    for need in ("vision_model.embeddings.class_embedding", "vision_model.pre_layrnorm.weight", "visual_projection.weight", "text_projection.weight"):
        if need not in out:
            raise KeyError("%s: no %s -- not a transformers CLIPModel checkpoint" % (path, need))
    if text_sd is not None:
        for k, v in text_sd.items():
            mine = sd.get("text_model." + k)
            if mine is None or mine.shape != v.shape or float((mine.float() - v.float()).abs().max()) > atol:
                raise ValueError("the text tower of %s differs from the loaded Stable-Diffusion text encoder at %r: CLIP similarity would pair "
                                 "an image tower with a text tower it was not trained with" % (path, k))
    return out


# ---- CompVis-layout checkpoints (what run_editing_instructpix2pix.py loads: one .ckpt whose state_dict holds model.diffusion_model.*,
# first_stage_model.* and cond_stage_model.transformer.*) -> the diffusers-layout names load_state_dict takes
_LDM_RES = {"in_layers.0": "norm1", "in_layers.2": "conv1", "emb_layers.1": "time_emb_proj", "out_layers.0": "norm2", "out_layers.3": "conv2",
            "skip_connection": "conv_shortcut"}
_LDM_VAE_ATTN = {"norm": "group_norm", "q": "query", "k": "key", "v": "value", "proj_out": "proj_attn"}
_LDM_VAE_RES = {"nin_shortcut": "conv_shortcut"}


def _ldm_res(rest):
    for a, b in _LDM_RES.items():
        if rest.startswith(a + "."):
            return b + rest[len(a):]
    raise KeyError(rest)


def _ldm_unet_key(k, lpb, ups):
    """one openaimodel.UNetModel key -> UNet2DConditionModel key.  lpb: ResNets per level; ups: output blocks whose LAST member upsamples"""
    p = k.split(".")
    if p[0] == "time_embed":
        return "time_embedding.linear_%d.%s" % ({"0": 1, "2": 2}[p[1]], p[2])
    if p[0] == "out":
        return {"0": "conv_norm_out", "2": "conv_out"}[p[1]] + "." + p[2]
    if p[0] == "input_blocks":
        i, j, rest = int(p[1]), int(p[2]), ".".join(p[3:])
        if i == 0:
            return "conv_in." + rest
        b, l = (i - 1) // (lpb + 1), (i - 1) % (lpb + 1)
        if l == lpb:
            return "down_blocks.%d.downsamplers.0.conv.%s" % (b, rest[len("op."):])
        return "down_blocks.%d.resnets.%d.%s" % (b, l, _ldm_res(rest)) if j == 0 else "down_blocks.%d.attentions.%d.%s" % (b, l, rest)
    if p[0] == "middle_block":
        j, rest = int(p[1]), ".".join(p[2:])
        return "mid_block.attentions.0." + rest if j == 1 else "mid_block.resnets.%d.%s" % (j // 2, _ldm_res(rest))
    if p[0] == "output_blocks":
        i, j, rest = int(p[1]), int(p[2]), ".".join(p[3:])
        b, l = i // (lpb + 1), i % (lpb + 1)
        if j == 0:
            return "up_blocks.%d.resnets.%d.%s" % (b, l, _ldm_res(rest))
        if (i, j) in ups:
            return "up_blocks.%d.upsamplers.0.%s" % (b, rest)
        return "up_blocks.%d.attentions.%d.%s" % (b, l, rest)
    raise KeyError(k)


def _ldm_vae_key(k, v, n_up):
    p = k.split(".")
    if p[0] in ("quant_conv", "post_quant_conv"):
        return k, v
    side, p = p[0], p[1:]
    if side not in ("encoder", "decoder"):
        raise KeyError(k)
    if p[0] in ("conv_in", "conv_out"):
        return side + "." + ".".join(p), v
    if p[0] == "norm_out":
        return side + ".conv_norm_out." + p[1], v
    if p[0] == "mid":
        if p[1].startswith("block_"):
            return "%s.mid_block.resnets.%d.%s" % (side, int(p[1][6:]) - 1, ".".join(p[2:])), v
        if p[1] == "attn_1":
            return "%s.mid_block.attentions.0.%s.%s" % (side, _LDM_VAE_ATTN[p[2]], p[3]), (v.reshape(v.shape[0], v.shape[1]) if v.dim() == 4 else v)
    if p[0] in ("down", "up"):
        b = int(p[1]) if p[0] == "down" else n_up - 1 - int(p[1])                 # ldm's decoder lists its levels from the output side
        pre = "%s.%s_blocks.%d." % (side, p[0], b)
        if p[2] == "block":
            return pre + "resnets.%s.%s.%s" % (p[3], _LDM_VAE_RES.get(p[4], p[4]), p[5]), v
        if p[2] in ("downsample", "upsample"):
            return pre + "%ssamplers.0.conv.%s" % (p[0], p[4]), v
    raise KeyError(k)


def convert_ldm_state_dict(sd):
    """CompVis-layout state dict -> (unet_sd, vae_sd, clip_sd) in the names load_state_dict takes.  Every key under the three model
    prefixes is consumed (an unknown one raises KeyError); what a training checkpoint holds besides (EMA copies, schedule buffers) is
    left alone.  The block structure is read from the keys themselves."""
    U, V, T = "model.diffusion_model.", "first_stage_model.", "cond_stage_model.transformer."
    uk = [k[len(U):] for k in sd if k.startswith(U)]
    unet, vae, clip = {}, {}, {}
    if uk:
        downs = sorted(int(k.split(".")[1]) for k in uk if k.startswith("input_blocks.") and k.endswith(".0.op.weight"))
        n_in = 1 + max(int(k.split(".")[1]) for k in uk if k.startswith("input_blocks."))
        lpb = downs[0] - 1 if downs else n_in - 1
        ups = {(int(k.split(".")[1]), int(k.split(".")[2])) for k in uk if k.startswith("output_blocks.") and k.endswith(".conv.weight")
               and k.count(".") == 4}
        for k in uk:
            unet[_ldm_unet_key(k, lpb, ups)] = sd[U + k]
    vk = [k[len(V):] for k in sd if k.startswith(V)]
    if vk:
        n_up = 1 + max(int(k.split(".")[2]) for k in vk if k.startswith("decoder.up."))
        for k in vk:
            if k.startswith("loss."):
                continue                                                           # the training discriminator of an autoencoder checkpoint
            nk, nv = _ldm_vae_key(k, sd[V + k], n_up)
            vae[nk] = nv
    for k in sd:
        if k.startswith(T):
            r = k[len(T):]
            if "position_ids" in r:
                continue
            clip[r[len("text_model."):] if r.startswith("text_model.") else r] = sd[k]
    for name, d, n in (("UNet", unet, len(uk)), ("VAE", vae, len([k for k in vk if not k.startswith("loss.")]))):
        if len(d) != n:
            raise KeyError("%s: two checkpoint keys map to one name" % name)
    return unet, vae, clip


def load_ldm_checkpoint(path):
    """a CompVis .ckpt as the reference's load_model_from_config reads it (:49-70) -> (unet_sd, vae_sd, clip_sd)"""
    pl_sd = torch.load(path, map_location="cpu", weights_only=False)
    return convert_ldm_state_dict(pl_sd["state_dict"] if "state_dict" in pl_sd else pl_sd)


def load_dino_checkpoint(path):
    """dino_vitbase8_pretrain.pth (what torch.hub's facebookresearch/dino:main dino_vitb8 downloads): a plain state dict with DINO's own
    keys -- cls_token, pos_embed, patch_embed.proj.*, blocks.N.*, norm.* -- as structure_distance.StructureDistance.load_state_dict
    takes it.  A training checkpoint's "teacher" / "student" wrapper and its "module." / "backbone." prefixes are stripped; head.* is
    dropped.  No such file exists offline, so this loader is untested here (the tests run weights.dino_state_dict)."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    for wrap in ("teacher", "student", "state_dict"):
        if isinstance(sd, dict) and wrap in sd and isinstance(sd[wrap], dict):
            sd = sd[wrap]
            break
    out = {}
    for k, v in sd.items():
        for pre in ("module.", "backbone."):
            if k.startswith(pre):
                k = k[len(pre):]
        if not k.startswith("head."):
            out[k] = v
    if "cls_token" not in out or "pos_embed" not in out:
        raise KeyError("%s holds no DINO VisionTransformer state dict (no cls_token / pos_embed)" % path)
    return out


def lpips_keys():
    """the state-dict keys lpips.Lpips.load_state_dict needs"""
    from . import weights
    keys = ["features.0.weight", "features.0.bias"]
    for idx, _, _, _ in weights.LPIPS_FIRES:
        keys += ["features.%d.%s.%s" % (idx, part, t) for part in ("squeeze", "expand1x1", "expand3x3") for t in ("weight", "bias")]
    return keys + ["lin%d.weight" % k for k in range(len(weights.LPIPS_TAP_CHANNELS))]


def load_lpips_checkpoint(squeezenet_pth, lin_pth):
    """The two files torchmetrics' LPIPS(net_type="squeeze") rests on, merged into what lpips.Lpips.load_state_dict takes:
      squeezenet_pth  torchvision's squeezenet1_1 state dict (squeezenet1_1-b8a52dc0.pth): features.N.{weight, bias} and
                      features.N.{squeeze, expand1x1, expand3x3}.{weight, bias} are kept under their own names, classifier.* is ignored
      lin_pth         the lpips package's squeeze.pth: lin{k}.model.1.weight [1, C, 1, 1] -> lin{k}.weight
    Any other key of either file, and any needed key that neither holds, raises KeyError with the names.  Neither file exists
    offline: the key mapping is tested on stand-ins written with torch.save, real weights are unverified, and so is whether the real
    network's activations stay inside fp16's range."""
    import re
    out, unknown = {}, []
    for k, v in torch.load(squeezenet_pth, map_location="cpu", weights_only=True).items():
        if k.startswith("classifier."):
            continue
        (out.__setitem__(k, v) if k.startswith("features.") else unknown.append("%s: %s" % (os.path.basename(squeezenet_pth), k)))
    for k, v in torch.load(lin_pth, map_location="cpu", weights_only=True).items():
        m = re.fullmatch(r"lin(\d)\.model\.1\.weight", k)
        (out.__setitem__("lin%s.weight" % m.group(1), v) if m else unknown.append("%s: %s" % (os.path.basename(lin_pth), k)))
    want = lpips_keys()
    unknown += [k for k in out if k not in want]
    out = {k: v for k, v in out.items() if k in want}
    missing = [k for k in want if k not in out]
    if unknown or missing:
        raise KeyError("LPIPS checkpoint: unknown keys %s; missing keys %s" % (sorted(set(unknown)), missing))
    return out


SYNTHETIC_WARNING = ("WARNING: running on SEEDED SYNTHETIC (random) Stable-Diffusion weights and a word-level stand-in tokenizer -- the "
                     "saved panels are numerically meaningful (parity / timing) but are NOT edits of a trained model.  Pass "
                     "--checkpoint_dir <diffusers SD-1.x directory> for real weights.")


def add_weight_args(ap):
    ap.add_argument("--checkpoint_dir", type=str, default=None,
                    help="Stable-Diffusion-1.x checkpoint in the diffusers layout (unet/, vae/, text_encoder/, tokenizer/): what the "
                         "reference downloads as CompVis/stable-diffusion-v1-4")
    ap.add_argument("--synthetic_weights", action="store_true",
                    help="explicit opt-in: seeded random weights + word-level stand-in tokenizer (no checkpoint exists offline)")


def resolve_weights(args, cfg, rank=0):
    """-> (unet_sd, vae_sd, clip_sd, tokenizer or None).  Exactly one of --checkpoint_dir / --synthetic_weights must be given;
    state dicts are None on ranks other than `rank` 0 (they receive the packed arena by the start-up broadcast)."""
    if args.checkpoint_dir and args.synthetic_weights:
        raise SystemExit("--checkpoint_dir and --synthetic_weights are mutually exclusive")
    if args.checkpoint_dir:
        unet, vae, clip, tok = load_checkpoint_dir(args.checkpoint_dir)
        return (unet, vae, clip, tok) if rank == 0 else (None, None, None, tok)
    if not args.synthetic_weights:
        raise SystemExit("no weights: pass --checkpoint_dir <diffusers SD-1.x directory> (the reference loads CompVis/stable-diffusion-v1-4), "
                         "or --synthetic_weights to run on seeded random weights")
    if rank == 0:
        print(SYNTHETIC_WARNING, file=sys.stderr, flush=True)
        from . import weights
        return weights.unet_state_dict(cfg, 0), weights.vae_state_dict(cfg, 0), weights.clip_state_dict(cfg, 0), None
    return None, None, None, None
