"""NativeEngine: thin Python owner of one pnpi_ctx (one per process / GPU).  PyTorch is used for device memory, the HIP
stream and (elsewhere) torch.distributed only; every FLOP of the hot path runs inside libpnpi.so."""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .config import ModelConfig


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class ControllerTables:
    """Host tables of one image's Prompt-to-Prompt controller -> pnpi_ctrl_desc (see include/pnpi.h)."""

    def __init__(self, cross_alpha, mapper, alphas, equalizer, self_range, lb_alpha=None, lb_start=0, lb_threshold=0.3,
                 self_max_tokens=32 ** 2, lb_sub_alpha=None, lb_threshold_sub=0.3):
        f = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        self.cross_alpha = f(cross_alpha)      # [steps+1, 77]
        self.mapper = f(mapper)                # [77, 77]
        self.alphas = f(alphas)                # [77]
        self.equalizer = f(equalizer)          # [77]
        self.self_range = (int(self_range[0]), int(self_range[1]))
        self.lb_alpha = f(lb_alpha) if lb_alpha is not None else None   # [2, 77]
        self.lb_start = int(lb_start)
        self.lb_threshold = float(lb_threshold)
        self.self_max_tokens = int(self_max_tokens)
        self.lb_sub_alpha = f(lb_sub_alpha) if lb_sub_alpha is not None else None   # [2, 77] LocalBlend substruct_layers
        self.lb_threshold_sub = float(lb_threshold_sub)
        if self.lb_sub_alpha is not None and self.lb_alpha is None:
            raise ValueError("lb_sub_alpha (LocalBlend substruct_words) without lb_alpha (LocalBlend words)")

    def desc(self):
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        d = _capi.CtrlDesc()
        d.kind = 1
        d.n_alpha_rows = self.cross_alpha.shape[0]
        d.cross_alpha_host = fp(self.cross_alpha)
        d.mapper_host = fp(self.mapper)
        d.alphas_host = fp(self.alphas)
        d.equalizer_host = fp(self.equalizer)
        d.self_replace_lo, d.self_replace_hi = self.self_range
        d.self_replace_max_tokens = self.self_max_tokens
        d.lb_enabled = 1 if self.lb_alpha is not None else 0
        d.lb_start = self.lb_start
        d.lb_threshold = self.lb_threshold
        d.lb_alpha_host = fp(self.lb_alpha) if self.lb_alpha is not None else None
        d.lb_sub_alpha_host = fp(self.lb_sub_alpha) if self.lb_sub_alpha is not None else None
        d.lb_threshold_sub = self.lb_threshold_sub
        return d


class MasaCtrlTables:
    """MutualSelfAttentionControl (models/masactrl/masactrl.py:14-72) -> pnpi_ctrl_desc kind 2."""

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None):
        """layer_idx / step_idx: explicit lists (any subset of transformer blocks 0..15 / denoising steps); None = the window."""
        self.start_step, self.start_layer = int(start_step), int(start_layer)
        self.layer_mask = 0
        if layer_idx is not None:
            for b in layer_idx:
                if 0 <= int(b) < 32:                      # blocks past the UNet's 16 never match, as in the reference's `in` test
                    self.layer_mask |= 1 << int(b)
            self.layer_mask |= 1 << 31                    # "a list was given" (an empty list switches the control off everywhere)
        self.step_on = None
        if step_idx is not None:
            n = max([int(x) for x in step_idx if int(x) >= 0], default=-1) + 1
            self.step_on = (C.c_ubyte * max(n, 1))()
            for x in step_idx:
                if int(x) >= 0:
                    self.step_on[int(x)] = 1

    def desc(self):
        d = _capi.CtrlDesc()
        d.kind = 2
        d.masa_start_step, d.masa_start_layer = self.start_step, self.start_layer
        d.masa_layer_mask = self.layer_mask
        if self.step_on is not None:
            d.masa_n_steps = len(self.step_on)
            d.masa_step_on_host = C.cast(self.step_on, C.POINTER(C.c_ubyte))
        return d


def masa_masks_u8(mask_s, mask_t):
    """MutualSelfAttentionControlMask's mask_s / mask_t (models/masactrl/masactrl.py:124-131: (h, w) tensors, same shape) -> two contiguous
    uint8 arrays [nimg, h, w] for pnpi_masa_set_masks ((h, w) is one image).  Only 0 / 1 values pass: the library runs the reference's two
    masked passes + blend as one class-restricted softmax, which equals them for binary masks only."""
    if mask_s is None or mask_t is None:
        raise ValueError("mask-guided MasaCtrl needs both mask_s and mask_t; without masks use MutualSelfAttentionControl")
    out = []
    for name, m in (("mask_s", mask_s), ("mask_t", mask_t)):
        a = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3 or a.size == 0:
            raise ValueError("%s must have shape (h, w) or (nimg, h, w), got %s" % (name, tuple(a.shape)))
        if not np.isin(a, (0.0, 1.0)).all():
            raise ValueError("%s must be binary (0 / 1): the blend of two masked passes for fractional masks is not built" % name)
        out.append(np.ascontiguousarray(a.astype(np.uint8)))
    if out[0].shape != out[1].shape:
        raise ValueError("mask_s %s and mask_t %s must have the same shape" % (out[0].shape, out[1].shape))
    return out[0], out[1]


class MasaCtrlMaskTables(MasaCtrlTables):
    """MutualSelfAttentionControlMask (models/masactrl/masactrl.py:114-193): the kind-2 descriptor plus the two masks, which travel
    through pnpi_masa_set_masks (NativeEngine.masa_set_masks) when the editor is registered -- pnpi_ctrl_desc keeps its layout."""

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, mask_s=None, mask_t=None):
        super().__init__(start_step, start_layer, layer_idx, step_idx)
        self.mask_s, self.mask_t = masa_masks_u8(mask_s, mask_t)


def _desc_array(ctrls):
    """list[ControllerTables | None] -> (ctypes array of pnpi_ctrl_desc, keep-alive)"""
    if ctrls is None:
        return None
    arr = (_capi.CtrlDesc * len(ctrls))()
    for i, c in enumerate(ctrls):
        if c is None:
            arr[i].kind = 0
        else:
            arr[i] = c.desc()
    return arr


class NativeEngine:
    def __init__(self, cfg: ModelConfig, device=None, max_unet_rows=4, max_vae_images=2, share_weights_with=None):
        """share_weights_with: another NativeEngine on the same device -- this context then borrows its packed weight arena
        (pnpi_create_shared: no second copy of the 1.9 GB) and is ready without load_state_dict; the other engine must outlive it."""
        if not torch.cuda.is_available():
            raise RuntimeError("NativeEngine needs an AMD GPU (gfx950); there is no CPU fallback")
        self.lib = _capi.load_library()
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self._ccfg = cfg.to_c()
        self.h = C.c_void_p()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            if share_weights_with is not None:
                if share_weights_with.device != self.device or share_weights_with.cfg != cfg:
                    raise ValueError("share_weights_with: same device and model configuration required")
                self._weights_owner = share_weights_with          # keep the owner alive as long as this context
                st = self.lib.pnpi_create_shared(C.byref(self.h), share_weights_with.h, C.c_void_p(stream), max_unet_rows, max_vae_images)
            else:
                st = self.lib.pnpi_create(C.byref(self.h), C.byref(self._ccfg), self.device.index or 0, C.c_void_p(stream),
                                          max_unet_rows, max_vae_images)
        if st != 0:
            msg = self.lib.pnpi_last_error(self.h if self.h else (share_weights_with.h if share_weights_with is not None else self.h))
            text = msg.decode() if msg else "?"
            self.close()                 # the half-built context only serves pnpi_last_error: free it
            raise _capi.PnpiError(st, text)
        self.max_unet_rows = max_unet_rows
        self.max_vae_images = max_vae_images
        self.lat_hw = cfg.sample_size
        self.ac = None
        self.final_alpha = None

    # ---- plumbing
    def _call(self, name, *args):
        st = getattr(self.lib, name)(self.h, *args)
        _capi.check(self.lib, self.h, st)

    def close(self):
        if self.h:
            self.lib.pnpi_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _f32(self, t):
        return t.to(device=self.device, dtype=torch.float32).contiguous()

    # ---- weights
    def load_state_dict(self, unet_sd=None, vae_sd=None, chunk_bytes=1 << 30, clip_sd=None, clipv_sd=None, dino_sd=None, lpips_sd=None):
        """diffusers-layout state dicts (CPU or GPU tensors, fp32 or fp16); repacked on the device into the fp16 arena.
        clip_sd: transformers CLIPTextModel state dict (optional; only pnpi_text_encode needs it).
        clipv_sd: transformers CLIPModel keys of the image tower and the two projections (after clipv_attach; see load_clipv_state_dict).
        dino_sd: facebookresearch/dino VisionTransformer keys (after dino_attach; see load_dino_state_dict).
        lpips_sd: squeezenet1_1 features.* keys and lin{k}.weight (after lpips_attach; see load_lpips_state_dict)."""
        items = []
        for prefix, sd in (("unet.", unet_sd), ("vae.", vae_sd), ("clip.", clip_sd), ("clipv.", clipv_sd), ("dino.", dino_sd),
                           ("lpips.", lpips_sd)):
            if sd:
                items += [(prefix + k, v) for k, v in sd.items()]
        batch, keep, size = [], [], 0

        def flush():
            nonlocal batch, keep, size
            if not batch:
                return
            arr = (_capi.NamedTensor * len(batch))(*batch)
            self._call("pnpi_load_weights", arr, len(batch))
            torch.cuda.synchronize(self.device)
            batch, keep, size = [], [], 0

        for name, v in items:
            t = v.detach()
            if t.dtype not in (torch.float32, torch.float16):
                t = t.float()
            t = t.to(self.device).contiguous()
            nt = _capi.NamedTensor()
            nt.name = name.encode()
            nt.data = t.data_ptr()
            nt.dtype = 1 if t.dtype == torch.float16 else 0
            nt.ndim = t.dim()
            for i, s in enumerate(t.shape):
                nt.shape[i] = s
            batch.append(nt)
            keep.append((t, nt.name))
            size += t.numel() * t.element_size()
            if size >= chunk_bytes:
                flush()
        flush()

    def missing_weights(self):
        buf = C.create_string_buffer(1 << 16)
        n = self.lib.pnpi_missing_weights(self.h, buf, len(buf))
        return n, buf.value.decode().split("\n")[:-1]

    def weight_arena(self):
        """The packed weight arena as a uint8 CUDA tensor view (for the one start-up RCCL broadcast)."""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._call("pnpi_weight_arena", C.byref(ptr), C.byref(nbytes))
        return ptr.value, nbytes.value

    def mark_all_loaded(self):
        self._call("pnpi_mark_all_loaded")

    def set_scheduler(self, alphas_cumprod, final_alpha_cumprod):
        ac = np.ascontiguousarray(np.asarray(alphas_cumprod, dtype=np.float32))
        self.ac = ac
        self.final_alpha = float(np.float32(final_alpha_cumprod))
        self._call("pnpi_set_scheduler", ac.ctypes.data_as(C.POINTER(C.c_float)), len(ac), self.final_alpha)

    def counters(self):
        c = _capi.Counters()
        self._call("pnpi_get_counters", C.byref(c))
        return {k: getattr(c, k) for k, _ in c._fields_}

    def reset_counters(self):
        self._call("pnpi_reset_counters")

    def tuning(self, **knobs):
        """with eng.tuning(key=value, ...): process-wide tuning knobs for the block (_capi.tuning)"""
        return _capi.tuning(self.lib, **knobs)

    def masa_set_masks(self, mask_s=None, mask_t=None):
        """pnpi_masa_set_masks: attach binary masks [nimg, h, w] (or (h, w)) to the kind-2 controllers of this context; no arguments clears them."""
        if mask_s is None and mask_t is None:
            self._call("pnpi_masa_set_masks", None, None, 0, 0, 0)
            self._masa_nimg = 0
            return
        s, t = masa_masks_u8(mask_s, mask_t)
        self._masa_nimg = 0
        self._call("pnpi_masa_set_masks", s.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), s.shape[0], s.shape[1], s.shape[2])
        self._masa_nimg = s.shape[0]

    def masa_level_masks(self, level):
        """the resized masks of self-attention level `level` (side = sample_size >> level) -> (mask_s, mask_t) uint8 [nimg, side, side]"""
        side = self.cfg.sample_size >> level
        n = max(getattr(self, "_masa_nimg", 0), 1)
        s, t = np.zeros((n, side, side), np.uint8), np.zeros((n, side, side), np.uint8)
        got = C.c_int()
        self._call("pnpi_masa_get_level_masks", int(level), s.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), C.byref(got))
        assert got.value == side
        return s, t

    def clock_probe(self, iters=100000):
        """effective matrix-pipe clock (GHz) under back-to-back MFMAs on every SIMD, and the probe's duration (ms)"""
        ghz, ms = C.c_float(), C.c_float()
        self._call("pnpi_clock_probe", int(iters), C.byref(ghz), C.byref(ms))
        return float(ghz.value), float(ms.value)

    def profile_begin(self):
        self._call("pnpi_profile_begin")

    def profile_end(self):
        arr = (_capi.KernelStats * len(_capi.KC_NAMES))()
        self._call("pnpi_profile_end", arr)
        return {n: dict(launches=int(arr[i].launches), total_ms=arr[i].total_ms, flops=arr[i].flops, bytes=arr[i].bytes)
                for i, n in enumerate(_capi.KC_NAMES)}

    # ---- level 1
    def text_kv_precompute(self, context):
        """Project the text context to the 16 cross-attention K / V pairs once; unet(..., context=None) then reads them."""
        ctx = self._f32(context)
        self._call("pnpi_text_kv_precompute", _p(ctx), ctx.shape[0])
        self._keep_ctx = ctx

    # ---- level-1 fallback: materialise-and-call-back attention (controllers without a kernel descriptor)
    def attention_sites(self):
        """(tokens, keys) of the 32 attention sites in call order -- sizes the call-back buffer"""
        cfg, S, sites = self.cfg, self.cfg.sample_size, []
        def level(i):
            n = (S >> i) ** 2
            return [(n, n), (n, cfg.ctx_len)]
        for i in range(cfg.n_blocks):
            if cfg.block_has_attn[i]:
                sites += level(i) * cfg.layers_per_block
        sites += level(cfg.n_blocks - 1)
        for i in reversed(range(cfg.n_blocks)):
            if cfg.block_has_attn[i]:
                sites += level(i) * (cfg.layers_per_block + 1)
        return sites

    def set_attention_callback(self, fn, rows=None):
        """fn(attn, is_cross: bool, place: 'down'|'mid'|'up', layer: int) -> None | tensor: called at every attention site of unet()
        with the softmax probabilities as a float32 CUDA tensor [rows*heads, Nq, Nk] (the reference's hooked forward,
        models/p2p/attention_control.py:40-44); it may modify the tensor in place or return a replacement.  fn = None removes it."""
        if fn is None:
            self._call("pnpi_set_attention_callback", None, None, None, 0)
            self._cb_keep = None
            return
        rows = rows or self.max_unet_rows
        heads = self.cfg.heads
        need = max(rows * heads * nq * nk * 4 + nq * ((nk + 7) // 8 * 8) * 2 + 512 for nq, nk in self.attention_sites())
        buf = torch.empty(need, dtype=torch.uint8, device=self.device)
        base = buf.data_ptr()
        places = ("down", "mid", "up")
        err = []

        def trampoline(user, attn_ptr, B, H, Nq, Nk, is_cross, place, layer):
            try:
                n = B * H * Nq * Nk
                off = attn_ptr - base
                view = buf[off:off + 4 * n].view(torch.float32).view(B * H, Nq, Nk)
                with torch.cuda.device(self.device):
                    new = fn(view, bool(is_cross), places[place], layer)
                    if new is not None and new is not view:
                        view.copy_(new.reshape(view.shape))
                    torch.cuda.current_stream().synchronize()
                return 0
            except Exception as e:       # never let an exception cross the C boundary
                err.append(e)
                return 1

        cb = _capi.ATTN_CALLBACK(trampoline)
        self._call("pnpi_set_attention_callback", cb, None, C.c_void_p(base), need)
        self._cb_keep = (cb, buf, err)

    def unet(self, latents, t, context, rows_per_image=1, ctrls=None, cur_step=0):
        lat, ctx = self._f32(latents), (self._f32(context) if context is not None else None)
        rows = lat.shape[0]
        out = torch.empty_like(lat)
        arr = _desc_array(ctrls)
        try:
            self._call("pnpi_unet_forward", _p(lat), rows, rows_per_image, int(t), _p(ctx), arr, int(cur_step), _p(out))
        except _capi.PnpiError:
            keep = getattr(self, "_cb_keep", None)
            if keep and keep[2]:
                raise keep[2].pop()          # the exception raised inside the attention callback
            raise
        self._keep = (lat, ctx, arr, ctrls)
        return out

    def text_encode(self, input_ids):
        """CLIPTextModel(input_ids)[0] on the device: int ids [n, 77] -> fp32 [n, 77, cross_dim]"""
        ids = torch.as_tensor(input_ids).to(self.device, dtype=torch.int32).contiguous()
        n, T = ids.shape
        if T != self.cfg.ctx_len:
            raise ValueError("input_ids must have %d positions" % self.cfg.ctx_len)
        out = torch.empty(n, T, self.cfg.cross_dim, device=self.device)
        self._call("pnpi_text_encode", _p(ids), n, _p(out))
        self._keep = ids
        return out

    # ---- CLIP similarity (pnpi_clipv_attach and the pnpi_clip_* entry points; clip_score.ClipScore is the user-facing object)
    def clipv_attach(self, vcfg=None, max_images=8):
        """Attach the CLIP image tower + projections (vcfg: _capi.ClipvConfig, default ViT-L/14) for up to max_images images per call."""
        if vcfg is None:
            vcfg = _capi.ClipvConfig()
            self.lib.pnpi_clipv_config_vitl14(C.byref(vcfg))
        self._call("pnpi_clipv_attach", C.byref(vcfg), int(max_images))
        self.clipv_cfg, self.clipv_max_images = vcfg, int(max_images)

    def load_clipv_state_dict(self, sd):
        """transformers CLIPModel keys (vision_model.*, visual_projection.weight, text_projection.weight; text_model.* is ignored here)"""
        wanted = {k: v for k, v in sd.items() if k.startswith("vision_model.") or k in ("visual_projection.weight", "text_projection.weight")}
        self.load_state_dict(clipv_sd={k: v for k, v in wanted.items() if "position_ids" not in k})

    def _tower_images(self, images, masks):
        img = torch.as_tensor(images)
        if img.dim() == 3:
            img = img[None]
        if img.dtype != torch.uint8 or img.dim() != 4 or img.shape[-1] != 3 or img.shape[1] != img.shape[2]:
            raise ValueError("images must be uint8 [n, S, S, 3] (square panels), got %s %s" % (img.dtype, tuple(img.shape)))
        img = img.to(self.device).contiguous()
        m = None
        if masks is not None:
            m = torch.as_tensor(masks)
            if m.dim() == 2:
                m = m[None]
            if m.dim() == 4:                      # evaluate.py's [S, S, 3] masks: one plane, broadcast over the channels by the kernel
                if not bool((m == m[..., :1]).all()):
                    raise ValueError("a mask with different channel planes is not supported")
                m = m[..., 0]
            if tuple(m.shape) != tuple(img.shape[:3]):
                raise ValueError("masks must be [n, S, S], got %s for images %s" % (tuple(m.shape), tuple(img.shape)))
            if not bool(((m == 0) | (m == 1)).all()):
                raise ValueError("masks must hold 0 / 1 only")
            m = m.to(self.device, dtype=torch.uint8).contiguous()
        return img, m

    def _clip_ids(self, input_ids):
        ids = torch.as_tensor(input_ids).to(self.device, dtype=torch.int32).contiguous()
        if ids.dim() != 2 or ids.shape[1] != self.cfg.ctx_len:
            raise ValueError("input_ids must be [n, %d]" % self.cfg.ctx_len)
        return ids

    def clip_preprocess(self, images, masks=None, out_size=None, want_resized=True, want_patches=True):
        """pnpi_op_clip_preprocess -> (resized uint8 [n, out, out, 3] or None, patch rows fp16 [n, (out / patch)^2, Kp] or None)"""
        img, m = self._tower_images(images, masks)
        n, S = img.shape[0], img.shape[1]
        out = int(out_size or self.clipv_cfg.image_size)
        p = self.clipv_cfg.patch
        kp = (3 * p * p + 63) // 64 * 64
        res = torch.empty(n, out, out, 3, dtype=torch.uint8, device=self.device) if want_resized else None
        pat = torch.empty(n, max(out // p, 1) ** 2, kp, dtype=torch.float16, device=self.device) if want_patches else None
        self._call("pnpi_op_clip_preprocess", _p(img), _p(m), n, S, out, _p(res), _p(pat))
        return res, pat

    def clip_image_embed(self, images, masks=None):
        img, m = self._tower_images(images, masks)
        out = torch.empty(img.shape[0], self.clipv_cfg.proj_dim, device=self.device)
        self._call("pnpi_clip_image_embed", _p(img), _p(m), img.shape[0], img.shape[1], _p(out))
        return out

    def clip_text_embed(self, input_ids):
        ids = self._clip_ids(input_ids)
        out = torch.empty(ids.shape[0], self.clipv_cfg.proj_dim, device=self.device)
        self._call("pnpi_clip_text_embed", _p(ids), ids.shape[0], _p(out))
        return out

    def clip_score(self, images, input_ids, masks=None):
        img, m = self._tower_images(images, masks)
        ids = self._clip_ids(input_ids)
        if ids.shape[0] != img.shape[0]:
            raise ValueError("%d images but %d prompts" % (img.shape[0], ids.shape[0]))
        out = torch.empty(img.shape[0], device=self.device)
        self._call("pnpi_clip_score", _p(img), _p(m), _p(ids), img.shape[0], img.shape[1], _p(out))
        return out

    # ---- DINO structure distance (pnpi_dino_attach and the entry points behind it; structure_distance.StructureDistance is the user-facing object)
    def dino_attach(self, cfg=None, max_pairs=4):
        """Attach the DINO ViT (cfg: _capi.DinoConfig, default ViT-B/8) for up to max_pairs image pairs (2 * max_pairs images) per call."""
        if cfg is None:
            cfg = _capi.DinoConfig()
            self.lib.pnpi_dino_config_vitb8(C.byref(cfg))
        self._call("pnpi_dino_attach", C.byref(cfg), int(max_pairs))
        self.dino_cfg, self.dino_max_pairs = cfg, int(max_pairs)

    def load_dino_state_dict(self, sd):
        """DINO's own state-dict keys.  The tensors the metric never reads (the last block's attn.proj / norm2 / mlp, norm.*, head.*) are dropped."""
        self.load_state_dict(dino_sd=dict(sd))

    def dino_tokens(self):
        return (self.dino_cfg.image_size // self.dino_cfg.patch) ** 2 + 1

    def dino_preprocess(self, images, masks=None, out_size=None, want_resized=True, want_patches=True):
        """pnpi_op_dino_preprocess -> (resized fp32 [n, 3, out, out] in 0..255 or None, patch rows fp16 [n, (out / patch)^2, 3 patch^2] or None)"""
        img, m = self._tower_images(images, masks)
        n, S = img.shape[0], img.shape[1]
        out = int(out_size or self.dino_cfg.image_size)
        p = self.dino_cfg.patch
        res = torch.empty(n, 3, out, out, dtype=torch.float32, device=self.device) if want_resized else None
        pat = torch.empty(n, max(out // p, 1) ** 2, 3 * p * p, dtype=torch.float16, device=self.device) if want_patches else None
        self._call("pnpi_op_dino_preprocess", _p(img), _p(m), n, S, out, _p(res), _p(pat))
        return res, pat

    def dino_keys(self, images, masks=None):
        """-> fp32 [n, T, width]: the concatenated keys of the last block (the output of blocks[-1].attn.qkv, K third)"""
        img, m = self._tower_images(images, masks)
        out = torch.empty(img.shape[0], self.dino_tokens(), self.dino_cfg.width, device=self.device)
        self._call("pnpi_dino_keys", _p(img), _p(m), img.shape[0], img.shape[1], _p(out))
        return out

    def structure_distance(self, pred, gt, mask_pred=None, mask_gt=None):
        """-> fp32 [n]: calculate_structure_distance per pair, one tower pass over the 2 n images"""
        a, ma = self._tower_images(pred, mask_pred)
        b, mb = self._tower_images(gt, mask_gt)
        if a.shape != b.shape:
            raise ValueError("Image shapes should be the same: %s and %s" % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty(a.shape[0], device=self.device)
        self._call("pnpi_structure_distance", _p(a), _p(ma), _p(b), _p(mb), a.shape[0], a.shape[1], _p(out))
        return out

    def keys_selfsim_mse(self, keys_a, keys_b, want_map=False):
        """pnpi_op_keys_selfsim_mse on fp16 [n, T, D] key matrices -> (distance fp32 [n], the map of keys_a fp32 [n, T, T] or None)"""
        ka = torch.as_tensor(keys_a).to(self.device, dtype=torch.float16).contiguous()
        kb = torch.as_tensor(keys_b).to(self.device, dtype=torch.float16).contiguous()
        if ka.dim() != 3 or ka.shape != kb.shape:
            raise ValueError("keys must be two [n, T, D] tensors of one shape")
        n, T, D = ka.shape
        dist = torch.empty(n, device=self.device)
        sim = torch.empty(n, T, T, device=self.device) if want_map else None
        self._call("pnpi_op_keys_selfsim_mse", _p(ka), _p(kb), n, T, D, _p(dist), _p(sim))
        return dist, sim

    # ---- LPIPS (pnpi_lpips_attach and the entry points behind it; lpips.Lpips is the user-facing object)
    def lpips_attach(self, max_pairs=4):
        """Attach SqueezeNet 1.1's features and the seven lin layers for up to max_pairs image pairs (2 * max_pairs images) per call."""
        self._call("pnpi_lpips_attach", int(max_pairs))
        self.lpips_max_pairs = int(max_pairs)

    def load_lpips_state_dict(self, sd):
        """torchvision's squeezenet1_1 keys (features.*) and lin{k}.weight (checkpoint.load_lpips_checkpoint, weights.lpips_state_dict)"""
        self.load_state_dict(lpips_sd=dict(sd))

    @staticmethod
    def lpips_tap_shape(S, tap):
        """(map side, channels) of tap 0 .. 6 at image side S: the stride-2 convolution, then ceil-mode 3 x 3 stride-2 pools"""
        def pool(h):
            o = (h - 2) // 2 + 1
            return o - 1 if (o - 1) * 2 >= h else o
        h = (S - 3) // 2 + 1
        sides = [h]
        for _ in range(3):
            h = pool(h)
            sides.append(h)
        from .weights import LPIPS_TAP_CHANNELS
        return sides[min(tap, 3)], LPIPS_TAP_CHANNELS[tap]

    def lpips_features(self, images, masks=None, tap=0):
        """-> fp32 [n, H, H, C]: the feature map of tap 0 .. 6 (the outputs of features 1, 4, 7, 9, 10, 11, 12), NHWC"""
        img, m = self._tower_images(images, masks)
        H, Cc = self.lpips_tap_shape(img.shape[1], int(tap))
        out = torch.empty(img.shape[0], H, H, Cc, device=self.device)
        self._call("pnpi_lpips_features", _p(img), _p(m), img.shape[0], img.shape[1], int(tap), _p(out))
        return out

    def lpips(self, pred, gt, mask_pred=None, mask_gt=None):
        """-> fp32 [n]: calculate_lpips per pair, one pass of the network over the 2 n images"""
        a, ma = self._tower_images(pred, mask_pred)
        b, mb = self._tower_images(gt, mask_gt)
        if a.shape != b.shape:
            raise ValueError("Image shapes should be the same: %s and %s" % (tuple(a.shape), tuple(b.shape)))
        out = torch.empty(a.shape[0], device=self.device)
        self._call("pnpi_lpips", _p(a), _p(ma), _p(b), _p(mb), a.shape[0], a.shape[1], _p(out))
        return out

    def lpips_layer(self, feat_a, feat_b, w):
        """pnpi_op_lpips_layer on fp16 [n, HW, C] feature maps and fp32 [C] weights -> fp32 [n]"""
        fa = torch.as_tensor(feat_a).to(self.device, dtype=torch.float16).contiguous()
        fb = torch.as_tensor(feat_b).to(self.device, dtype=torch.float16).contiguous()
        wv = self._f32(torch.as_tensor(w))
        if fa.dim() != 3 or fa.shape != fb.shape or tuple(wv.shape) != (fa.shape[2],):
            raise ValueError("features must be two [n, HW, C] tensors of one shape and w [C]")
        out = torch.empty(fa.shape[0], device=self.device)
        self._call("pnpi_op_lpips_layer", _p(fa), _p(fb), _p(wv), fa.shape[0], fa.shape[1], fa.shape[2], _p(out))
        return out

    def maxpool3s2_ceil(self, x):
        """pnpi_op_maxpool3s2_ceil on fp16 NHWC [n, H, H, C] -> fp16 [n, Ho, Ho, C]"""
        x = torch.as_tensor(x).to(self.device, dtype=torch.float16).contiguous()
        n, H, _, Cc = x.shape
        Ho = (H - 2) // 2 + 1
        Ho -= (Ho - 1) * 2 >= H
        out = torch.empty(n, Ho, Ho, Cc, dtype=torch.float16, device=self.device)
        self._call("pnpi_op_maxpool3s2_ceil", _p(x), n, H, Cc, _p(out))
        return out

    def local_blend(self, latents, step_index):
        lat = self._f32(latents)
        self._call("pnpi_local_blend", _p(lat), lat.shape[0] // 2, int(step_index))
        return lat

    def vae_encode(self, x):
        x = self._f32(x)
        n, _, H, W = x.shape
        f = self.cfg.vae_scale
        out = torch.empty(n, self.cfg.vae_latent_channels, H // f, W // f, device=self.device)
        self._call("pnpi_vae_encode", _p(x), n, H, W, _p(out))
        self._keep = x
        return out

    def vae_decode(self, z):
        z = self._f32(z)
        n, _, h, w = z.shape
        f = self.cfg.vae_scale
        out = torch.empty(n, 3, h * f, w * f, device=self.device)
        self._call("pnpi_vae_decode", _p(z), n, h, w, _p(out))
        self._keep = z
        return out

    def image2latent(self, img_u8):
        """uint8 [n,H,W,3] (or [H,W,3]) -> 0.18215 * posterior mean, fp32 [n,4,H/8,W/8]."""
        img = torch.as_tensor(img_u8)
        if img.dim() == 3:
            img = img[None]
        img = img.to(self.device).contiguous()
        n, H, W, _ = img.shape
        f = self.cfg.vae_scale
        out = torch.empty(n, self.cfg.vae_latent_channels, H // f, W // f, device=self.device)
        self._call("pnpi_image2latent", _p(img), n, H, W, _p(out))
        self._keep = img
        return out

    def latent2image(self, z):
        z = self._f32(z)
        n, _, h, w = z.shape
        f = self.cfg.vae_scale
        out = torch.empty(n, h * f, w * f, 3, dtype=torch.uint8, device=self.device)
        self._call("pnpi_latent2image", _p(z), n, h, w, _p(out))
        self._keep = z
        return out

    def ddim_next_step(self, eps, t, ratio, sample):
        e, s = self._f32(eps), self._f32(sample)
        out = torch.empty_like(s)
        self._call("pnpi_ddim_next_step", _p(e), int(t), int(ratio), _p(s), s.numel(), _p(out))
        self._keep = (e, s)
        return out

    def ddim_prev_step(self, eps, t, ratio, sample):
        e, s = self._f32(eps), self._f32(sample)
        out = torch.empty_like(s)
        self._call("pnpi_ddim_prev_step", _p(e), int(t), int(ratio), _p(s), s.numel(), _p(out))
        self._keep = (e, s)
        return out

    def cfg_ddim_prev(self, eps, x, t, ratio, guidance_scale, noise_loss=None, offset_rows=0):
        """One image's CFG combine + DDIM step (+ the direct-inversion offset on the first offset_rows rows): eps [2R, 4, h, w]
        (R unconditional rows, then R conditional), x [R, 4, h, w] -> [R, 4, h, w]   (p2p_guidance_forward.py:108-114)"""
        e, xs = self._f32(eps), self._f32(x)
        R = xs.shape[0]
        assert e.shape[0] == 2 * R
        nl = self._f32(noise_loss) if noise_loss is not None else None
        out = torch.empty_like(xs)
        self._call("pnpi_cfg_ddim_prev", _p(e), _p(xs), 1, R, xs[0].numel(), float(guidance_scale), int(t), int(ratio), _p(nl),
                   int(offset_rows) if nl is not None else 0, None, 1.0, None, _p(out), None, 0, None)
        self._keep = (e, xs, nl)
        return out

    def ddim_prev_step_recon(self, eps, t, ratio, sample, ref_image, recon_lr, recon_mask=None):
        """DDIMSchedulerDev.step with ref_image / recon_lr / recon_mask (scheduler_dev.py:68-76) -> (prev_sample, pred_original_sample)"""
        e, s = self._f32(eps), self._f32(sample)
        ref = self._f32(ref_image.to(self.device).expand_as(s))
        mask = None if recon_mask is None else self._f32(recon_mask.to(self.device).expand_as(s).float())
        out, x0 = torch.empty_like(s), torch.empty_like(s)
        self._call("pnpi_ddim_prev_step_recon", _p(e), int(t), int(ratio), _p(s), s.numel(), _p(ref), float(recon_lr),
                   _p(mask) if mask is not None else None, _p(out), _p(x0))
        self._keep = (e, s, ref, mask)
        return out, x0

    # ---- level 2
    def _ts(self, timesteps):
        ts = np.ascontiguousarray(np.asarray(timesteps, dtype=np.int32))
        return ts, ts.ctypes.data_as(C.POINTER(C.c_int))

    def _recon_desc(self, recon, nimg, xT, nsteps):
        """recon dict -> (pnpi_recon_desc, tensors to keep alive).  ref_image: [nimg,4,h,w] encoded source latent or None; x_stars: None
        or the inversion trajectory [nsteps+1, 1 | nimg, 4, h, w] (inversion guidance, proximal_guidance_forward.py:73-75)."""
        if recon is None:
            return None, None
        ref = inv = None
        if recon.get("ref_image") is not None:
            ref = self._f32(recon["ref_image"]).reshape(nimg, *xT.shape[1:]).contiguous()
        if recon.get("x_stars") is not None:
            xs = recon["x_stars"]
            xs = torch.stack([x for x in xs]) if isinstance(xs, (list, tuple)) else xs
            inv = self._f32(xs).reshape(nsteps + 1, -1, *xT.shape[1:])
            inv = inv.expand(nsteps + 1, nimg, *xT.shape[1:]).contiguous()
        rd = _capi.ReconDesc.make(ref.data_ptr() if ref is not None else None, recon["recon_lr"], recon["recon_t"],
                                  int(recon.get("dilate_mask") or 0), inv.data_ptr() if inv is not None else None)
        return rd, (ref, inv)

    def edit_loop_uncond_steps(self, x_T, context4, uncond_steps, ctrls, timesteps, guidance_scale, first_only=False, prox=None, quantile=0.7,
                               recon=None):
        """edit_loop with per-step unconditional embeddings [steps, nimg, 77, D] (null-text inversion); recon as in edit_loop."""
        xT, ctx, us = self._f32(x_T), self._f32(context4), self._f32(uncond_steps)
        nimg = xT.shape[0]
        out = torch.empty(nimg, 2, *xT.shape[1:], device=self.device)
        ts, tsp = self._ts(timesteps)
        arr = _desc_array(ctrls)
        mode = {None: 0, "l0": 1, "l1": 2}[prox]
        rd, ref = self._recon_desc(recon, nimg, xT, len(timesteps))
        self._call("pnpi_edit_loop_uncond_steps_recon", _p(xT), nimg, _p(ctx), arr, len(timesteps), tsp, float(guidance_scale), mode, float(quantile),
                   _p(us), int(bool(first_only)), C.byref(rd) if rd is not None else None, _p(out))
        self._keep = (xT, ctx, us, ts, arr, ctrls, ref, rd)
        return out

    def unet_context_grad(self, latents, t, context, d_eps):
        """eps and d loss / d context for ONE row (null-text path groundwork): latents [1,4,h,w], context [1,77,D], d_eps like eps."""
        lat, ctx, de = self._f32(latents), self._f32(context), self._f32(d_eps)
        eps, dctx = torch.empty_like(lat), torch.empty_like(ctx)
        self._call("pnpi_unet_context_grad", _p(lat), int(t), _p(ctx), _p(de), _p(eps), _p(dctx))
        return eps, dctx

    def null_text_optimize(self, ddim_latents, ctx_uncond, ctx_cond, timesteps, guidance_scale, num_inner_steps=10, epsilon=1e-5,
                           return_losses=False):
        """NullInversion.null_optimization for one image -> ([steps, 1, 77, D] embeddings, [steps] Adam iterations run[, per-step lists
        of every iteration's loss])."""
        lat = self._f32(ddim_latents)
        n = lat.shape[0] - 1
        cu, cc = self._f32(ctx_uncond), self._f32(ctx_cond)
        out = torch.empty(n, 1, cu.shape[-2], cu.shape[-1], device=self.device, dtype=torch.float32)
        its = (C.c_int * n)()
        losses = (C.c_float * max(1, n * int(num_inner_steps)))()
        ts_keep, ts_ptr = self._ts(timesteps)
        self._call("pnpi_null_text_optimize", _p(lat), _p(cu), _p(cc), n, ts_ptr, float(guidance_scale), int(num_inner_steps),
                   float(epsilon), _p(out), its, losses)
        del ts_keep
        if return_losses:
            return out, list(its), [[losses[i * num_inner_steps + j] for j in range(its[i])] for i in range(n)]
        return out, list(its)

    def null_latent_calculate(self, ddim_latents, context4, timesteps, guidance_scale, num_inner_steps=10, epsilon=1e-5, return_losses=False):
        """DirectInversion.null_latent_calculate for one prompt pair -> [steps, 2, 4, h, w] latent offsets (context4 rows:
        unc_src, unc_tgt, cond_src, cond_tgt)."""
        lat = self._f32(ddim_latents)
        n = lat.shape[0] - 1
        c4 = self._f32(context4)
        assert c4.shape[0] == 4, "null_latent_calculate handles one (source, target) prompt pair"
        out = torch.empty(n, 2, *lat.shape[-3:], device=self.device, dtype=torch.float32)
        its = (C.c_int * n)()
        losses = (C.c_float * max(1, n * int(num_inner_steps)))()
        ts_keep, ts_ptr = self._ts(timesteps)
        self._call("pnpi_null_latent_calculate", _p(lat), _p(c4), n, ts_ptr, float(guidance_scale), int(num_inner_steps), float(epsilon),
                   _p(out), its, losses)
        del ts_keep
        if return_losses:
            return out, list(its), [[losses[i * num_inner_steps + j] for j in range(its[i])] for i in range(n)]
        return out, list(its)

    def ddim_invert(self, z0, ctx_cond, timesteps):
        z0, ctx = self._f32(z0), self._f32(ctx_cond)
        n = len(timesteps)
        nimg = z0.shape[0]
        out = torch.empty(n + 1, *z0.shape, device=self.device)
        ts, tsp = self._ts(timesteps)
        self._call("pnpi_ddim_invert", _p(z0), nimg, _p(ctx), n, tsp, _p(out))
        self._keep = (z0, ctx, ts)
        return out

    @staticmethod
    def _scales(offset_scale, n):
        """None | float | sequence[n] -> (keep-alive array, float* or None): per-step factor on the direct-inversion offset"""
        if offset_scale is None:
            return None, None
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(offset_scale, dtype=np.float32), (n,)))
        return sc, sc.ctypes.data_as(C.POINTER(C.c_float))

    def ddim_invert_cfg(self, z0, ctx_uncond, ctx_cond, timesteps, guidance_scale):
        """DDIM inversion under classifier-free guidance (inversion.py:334-347) -> [steps+1, nimg, 4, h, w]"""
        z0, cu, cc = self._f32(z0), self._f32(ctx_uncond), self._f32(ctx_cond)
        n, nimg = len(timesteps), z0.shape[0]
        out = torch.empty(n + 1, *z0.shape, device=self.device)
        ts, tsp = self._ts(timesteps)
        self._call("pnpi_ddim_invert_cfg", _p(z0), nimg, _p(cu), _p(cc), float(guidance_scale), n, tsp, _p(out))
        self._keep = (z0, cu, cc, ts)
        return out

    def offset_calculate(self, ddim_latents, context4, timesteps, guidance_scale, offset_scale=None):
        lat, ctx = self._f32(ddim_latents), self._f32(context4)
        n = len(timesteps)
        nimg = lat.shape[1]
        out = torch.empty(n, nimg, 2, *lat.shape[2:], device=self.device)
        ts, tsp = self._ts(timesteps)
        sc, scp = self._scales(offset_scale, n)
        self._call("pnpi_offset_calculate", _p(lat), nimg, _p(ctx), n, tsp, float(guidance_scale), scp, _p(out))
        self._keep = (lat, ctx, ts, sc)
        return out

    def direct_edit(self, ddim_latents, context4, ctrls_per_pass, timesteps, guidance_scale, offset_rows=1, offset_scale=None):
        """offset_calculate + len(ctrls_per_pass) guidance-forward passes in lock step (pnpi_direct_edit).
        ctrls_per_pass: list (passes) of None | list[ControllerTables | None] (images).  -> (noise_loss, latents[npass])"""
        lat, ctx = self._f32(ddim_latents), self._f32(context4)
        n = len(timesteps)
        nimg = lat.shape[1]
        npass = len(ctrls_per_pass)
        flat = []
        for cp in ctrls_per_pass:
            flat += list(cp) if cp is not None else [None] * nimg
        assert len(flat) == npass * nimg
        arr = _desc_array(flat)
        nl = torch.empty(n, nimg, 2, *lat.shape[2:], device=self.device)
        out = torch.empty(npass, nimg, 2, *lat.shape[2:], device=self.device)
        ts, tsp = self._ts(timesteps)
        sc, scp = self._scales(offset_scale, n)
        self._call("pnpi_direct_edit", _p(lat), nimg, _p(ctx), npass, arr, int(offset_rows), n, tsp, float(guidance_scale), scp, _p(nl), _p(out))
        self._keep = (lat, ctx, ts, arr, flat, sc)
        return nl, out

    def direct_edit_pruned(self, ddim_latents, context4, ctrls, timesteps, guidance_scale):
        """The pruned-equivalent schedule (SURVEY Note D): 3 rows per image and step, source latent assigned from the trajectory.
        ctrls: None | list[ControllerTables | None] per image.  -> latents [nimg, 2, 4, h, w] = (x*_0, edited)"""
        lat, ctx = self._f32(ddim_latents), self._f32(context4)
        n, nimg = len(timesteps), lat.shape[1]
        arr = _desc_array(ctrls)
        out = torch.empty(nimg, 2, *lat.shape[2:], device=self.device)
        ts, tsp = self._ts(timesteps)
        self._call("pnpi_direct_edit_pruned", _p(lat), nimg, _p(ctx), arr, n, tsp, float(guidance_scale), _p(out))
        self._keep = (lat, ctx, ts, arr, ctrls)
        return out

    def edit_loop(self, x_T, context4, noise_loss, ctrls, timesteps, guidance_scale, offset_rows=1, prox=None, quantile=0.7,
                  recon=None):
        """recon: None | dict(ref_image=[nimg,4,h,w] encoded source latent, recon_lr, recon_t, dilate_mask): reconstruction guidance
        (proximal_guidance_forward.py:48-51 + scheduler_dev.py:68-76), applied with prox 'l0' / 'l1' only."""
        xT, ctx = self._f32(x_T), self._f32(context4)
        nl = self._f32(noise_loss) if noise_loss is not None else None
        n = len(timesteps)
        nimg = xT.shape[0]
        out = torch.empty(nimg, 2, *xT.shape[1:], device=self.device)
        ts, tsp = self._ts(timesteps)
        arr = _desc_array(ctrls)
        mode = {None: 0, "l0": 1, "l1": 2}[prox]
        rd, ref = self._recon_desc(recon, nimg, xT, n)
        self._call("pnpi_edit_loop", _p(xT), nimg, _p(ctx), _p(nl), int(offset_rows), arr, n, tsp, float(guidance_scale), mode,
                   float(quantile), C.byref(rd) if rd is not None else None, _p(out))
        self._keep = (xT, ctx, nl, ts, arr, ctrls, ref, rd)
        return out

    # ---- edit-friendly DDPM inversion (models/edit_friendly_ddm/inversion_utils.py, eta > 0)
    @staticmethod
    def _etas(etas, n):
        """the reference's `etas`: a number (repeated, :121-122 / :231) or a per-step list indexed by idx"""
        if isinstance(etas, (int, float)):
            etas = [etas] * n
        e = np.ascontiguousarray(np.asarray(etas, dtype=np.float32))
        if e.shape != (n,):
            raise ValueError("etas: one value per inference step (%d), got shape %s" % (n, e.shape))
        return e, e.ctypes.data_as(C.POINTER(C.c_float))

    def ef_step_scalars(self, t, ratio, eta):
        """host scalars of one step: (sqrt(ab_t), sqrt(1-ab_t), sqrt(ab_prev), sqrt(1-ab_prev-eta*var), eta*sqrt(var), var)"""
        return ef_step_scalars(self.lib, self.ac, self.final_alpha, t, ratio, eta)

    def ef_sample_xts(self, x0, noise, timesteps):
        """sample_xts_from_x0 (:31-55): x0 [nimg,4,h,w], noise [nsteps, nimg, 4, h, w] in draw order -> xts [nsteps+1, nimg, 4, h, w]"""
        x, nz = self._f32(x0), self._f32(noise)
        n, nimg = len(timesteps), x.shape[0]
        assert nz.shape == (n, *x.shape)
        out = torch.empty(n + 1, *x.shape, device=self.device)
        out[0] = x
        ts, tsp = self._ts(timesteps)
        self._call("pnpi_ef_sample_xts", _p(x), nimg, _p(nz), x[0].numel(), n, tsp, _p(out))
        self._keep = (x, nz, ts)
        return out

    def ef_noise_map(self, eps, xt, xprev, t, ratio, eta, cfg_scale=None):
        """One forward-process step (:151-171).  eps [nimg, 2, 4, h, w] (uncond, cond) with cfg_scale, or [nimg, 1, ...] without;
        xt = xts[idx+1], xprev = xts[idx] [nimg, 4, h, w] -> (z, corrected xprev), new tensors."""
        e, x = self._f32(eps), self._f32(xt)
        xp = self._f32(xprev).clone()
        nimg = x.shape[0]
        z = torch.empty_like(x)
        self._call("pnpi_ef_noise_map", _p(e), 1 if cfg_scale is not None else 0, float(cfg_scale or 0.0), _p(x), _p(xp), _p(z), nimg,
                   x[0].numel(), int(t), int(ratio), float(eta))
        self._keep = (e, x)
        return z, xp

    def ef_reverse_step(self, eps, x, z, t, ratio, eta, cfg_scales):
        """CFG per prompt row + reverse_step (:179-208, :254-258): eps [nimg, 2P, 4, h, w], x [nimg, P, 4, h, w], z [nimg, 4, h, w]"""
        e, xs, zz = self._f32(eps), self._f32(x), self._f32(z)
        nimg, P = xs.shape[:2]
        sc = np.ascontiguousarray(np.asarray(cfg_scales, dtype=np.float32))
        assert sc.shape == (P,) and e.shape[1] == 2 * P
        out = torch.empty_like(xs)
        self._call("pnpi_ef_reverse_step", _p(e), _p(xs), _p(zz), nimg, P, xs[0, 0].numel(), sc.ctypes.data_as(C.POINTER(C.c_float)), int(t),
                   int(ratio), float(eta), _p(out))
        self._keep = (e, xs, zz, sc)
        return out

    def ef_invert(self, x0, noise, ctx_uncond, ctx_cond, cfg_scale, etas, timesteps):
        """inversion_forward_process (:100-176) for nimg images, device-resident (pnpi_ef_invert).  x0 [nimg,4,h,w], noise
        [nsteps, nimg, 4, h, w] (the draws in the reference's order), ctx_* [nimg, 77, D] (ctx_cond None: prompt "").
        -> (xts [nsteps+1, nimg, 4, h, w], zs [nsteps, nimg, 4, h, w])"""
        x, nz, cu = self._f32(x0), self._f32(noise), self._f32(ctx_uncond)
        cc = self._f32(ctx_cond) if ctx_cond is not None else None
        n, nimg = len(timesteps), x.shape[0]
        if nz.shape != (n, *x.shape):
            raise ValueError("noise must be [nsteps, nimg, 4, h, w] = %s, got %s" % ((n, *x.shape), tuple(nz.shape)))
        e, ep = self._etas(etas, n)
        ts, tsp = self._ts(timesteps)
        xts = torch.empty(n + 1, *x.shape, device=self.device)
        zs = torch.empty(n, *x.shape, device=self.device)
        self._call("pnpi_ef_invert", _p(x), nimg, _p(nz), _p(cu), _p(cc), float(cfg_scale), ep, n, tsp, _p(xts), _p(zs))
        self._keep = (x, nz, cu, cc, e, ts)
        return xts, zs

    def ef_edit(self, xT, zs, context, cfg_scales, ctrls, etas, timesteps):
        """inversion_reverse_process (:210-262) with stored noise maps, device-resident (pnpi_ef_edit).  xT [nimg,4,h,w],
        zs [nsteps_run, nimg, 4, h, w] (the first nsteps_run maps), context [nimg, 2P, 77, D] (P uncond rows, then P cond rows),
        cfg_scales [P], ctrls None | [nimg] ControllerTables (P == 2), etas: number or [len(timesteps)], timesteps: the full schedule.
        -> latents [nimg, P, 4, h, w]"""
        x, z, ctx = self._f32(xT), self._f32(zs), self._f32(context)
        nimg, P = x.shape[0], ctx.shape[1] // 2
        n_run, n_tot = z.shape[0], len(timesteps)
        if z.shape[1:] != x.shape or ctx.shape[:2] != (nimg, 2 * P):
            raise ValueError("zs [nsteps_run, nimg, 4, h, w] and context [nimg, 2 * nprompts, 77, D] expected")
        sc = np.ascontiguousarray(np.asarray(cfg_scales, dtype=np.float32))
        if sc.shape != (P,):
            raise ValueError("one guidance scale per prompt row (%d), got %s" % (P, sc.shape))
        e, ep = self._etas(etas, n_tot)
        ts, tsp = self._ts(timesteps)
        arr = _desc_array(ctrls)
        out = torch.empty(nimg, P, *x.shape[1:], device=self.device)
        self._call("pnpi_ef_edit", _p(x), _p(z), nimg, P, _p(ctx), sc.ctypes.data_as(C.POINTER(C.c_float)), arr, ep, n_run, n_tot, tsp, _p(out))
        self._keep = (x, z, ctx, sc, e, ts, arr, ctrls)
        return out

    # ---- Blended Latent Diffusion (run_editing_blended_latent_diffusion.py)
    def bld_mask(self, mask_u8):
        """_read_mask (:164-173) on the device: uint8 [n, H, W] (or [H, W]) full-resolution masks -> fp32 0/1 [n, h, w] at the latent size
        (PIL-nearest source pixel floor((i + 0.5) * H / h), non-zero -> 1)."""
        m = torch.as_tensor(mask_u8)
        if m.dim() == 2:
            m = m[None]
        if m.dim() != 3 or m.dtype != torch.uint8:
            raise ValueError("mask must be uint8 [n, H, W], got %s %s" % (m.dtype, tuple(m.shape)))
        m = m.to(self.device).contiguous()
        n, H, W = m.shape
        out = torch.empty(n, self.lat_hw, self.lat_hw, device=self.device)
        self._call("pnpi_bld_mask", _p(m), n, H, W, _p(out))
        self._keep = m
        return out

    def bld_step(self, eps, x, src, noise, mask, t, ratio, guidance_scale, inplace=False):
        """One step of edit_image's loop (:127-139): eps [nimg, 2, C, h, w] (uncond, cond), x / src / noise [nimg, C, h, w], mask [nimg, h, w]
        fp32 0/1 -> CFG, DDIM step t -> t - ratio, source noised to level t, blend by the mask.  inplace: the result overwrites (the
        device copy of) x and that tensor is returned."""
        e, xs, s, nz, m = self._f32(eps), self._f32(x), self._f32(src), self._f32(noise), self._f32(mask)
        if xs.dim() != 4:
            raise ValueError("x must be [nimg, C, h, w], got %s" % (tuple(xs.shape),))
        nimg, _, h, w = xs.shape
        if e.shape != (nimg, 2, *xs.shape[1:]):
            raise ValueError("eps must be [nimg, 2, C, h, w] = %s, got %s" % ((nimg, 2, *xs.shape[1:]), tuple(e.shape)))
        if s.shape != xs.shape or nz.shape != xs.shape:
            raise ValueError("src and noise must be [nimg, C, h, w] = %s, got %s and %s" % (tuple(xs.shape), tuple(s.shape), tuple(nz.shape)))
        if m.shape != (nimg, h, w):
            raise ValueError("mask must be [nimg, h, w] = %s, got %s" % ((nimg, h, w), tuple(m.shape)))
        out = xs if inplace else torch.empty_like(xs)
        self._call("pnpi_bld_step", _p(e), _p(xs), _p(s), _p(nz), _p(m), nimg, xs[0].numel(), h * w, float(guidance_scale), int(t), int(ratio),
                   _p(out))
        self._keep = (e, xs, s, nz, m)
        return out

    def bld_edit(self, x_start, src, noise, mask, ctx_uncond, ctx_cond, guidance_scale, timesteps):
        """BlendedLatnetDiffusion.edit_image's loop (:110-139) for nimg images, device-resident (pnpi_bld_edit).  x_start [nimg, 4, h, w] the
        N(0,1) start latents, src [nimg, 4, h, w] the encoded sources, noise [nsteps_run, nimg, 4, h, w] the blending draws in step order,
        mask [nimg, h, w] fp32 0/1, ctx_* [nimg, 77, D], timesteps: the full schedule (its last nsteps_run entries are executed).
        -> latents [nimg, 4, h, w]"""
        x, s, nz, m = self._f32(x_start), self._f32(src), self._f32(noise), self._f32(mask)
        cu, cc = self._f32(ctx_uncond), self._f32(ctx_cond)
        if x.dim() != 4 or x.shape[1:] != (self.cfg.in_channels, self.lat_hw, self.lat_hw):
            raise ValueError("x_start must be [nimg, %d, %d, %d], got %s" % (self.cfg.in_channels, self.lat_hw, self.lat_hw, tuple(x.shape)))
        nimg = x.shape[0]
        if s.shape != x.shape:
            raise ValueError("src must be [nimg, 4, h, w] = %s, got %s" % (tuple(x.shape), tuple(s.shape)))
        if nz.dim() != 5 or nz.shape[1:] != x.shape:
            raise ValueError("noise must be [nsteps_run, nimg, 4, h, w] = (nsteps_run, %s), got %s" % (", ".join(map(str, x.shape)), tuple(nz.shape)))
        if m.shape != (nimg, self.lat_hw, self.lat_hw):
            raise ValueError("mask must be [nimg, h, w] = %s, got %s" % ((nimg, self.lat_hw, self.lat_hw), tuple(m.shape)))
        want = (nimg, self.cfg.ctx_len, self.cfg.cross_dim)
        if cu.shape != want or cc.shape != want:
            raise ValueError("ctx_uncond and ctx_cond must be [nimg, 77, D] = %s, got %s and %s" % (want, tuple(cu.shape), tuple(cc.shape)))
        ts, tsp = self._ts(timesteps)
        out = torch.empty_like(x)
        self._call("pnpi_bld_edit", _p(x), nimg, _p(s), _p(nz), _p(m), _p(cu), _p(cc), float(guidance_scale), len(ts), nz.shape[0], tsp, _p(out))
        self._keep = (x, s, nz, m, cu, cc, ts)
        return out

    # ---- Plug-and-Play (run_editing_pnp.py)
    def pnp_desc(self, nsteps, conv_steps=None, qk_steps=None):
        """The reference's injection sites for this model (pnp_desc_default) with its schedule int(n * 0.8) / int(n * 0.5), or the given
        numbers of leading steps that inject"""
        d = pnp_desc_default(self.lib, self.cfg, nsteps)
        if conv_steps is not None:
            d.conv_steps = int(conv_steps)
        if qk_steps is not None:
            d.qk_steps = int(qk_steps)
        return d

    def pnp_step(self, eps, x, t, ratio, guidance_scale):
        """denoise_step :363-368: eps [nimg, 3, C, h, w] (source row unread, negative, target), x [nimg, C, h, w] -> CFG over rows 1 and 2,
        then DDIMScheduler.step t -> t - ratio"""
        e, xs = self._f32(eps), self._f32(x)
        if xs.dim() != 4 or e.shape != (xs.shape[0], 3, *xs.shape[1:]):
            raise ValueError("eps must be [nimg, 3, C, h, w] and x [nimg, C, h, w], got %s and %s" % (tuple(e.shape), tuple(xs.shape)))
        out = torch.empty_like(xs)
        self._call("pnpi_pnp_step", _p(e), _p(xs), xs.shape[0], xs[0].numel(), float(guidance_scale), int(t), int(ratio), _p(out))
        self._keep = (e, xs)
        return out

    def unet_pnp(self, latents, t, context, desc, conv_on, qk_on):
        """One hooked forward of denoise_step (:361): latents [nimg, 3, C, h, w] = [source, x, x] per image, context [nimg, 3, 77, D]
        (None: the rows of text_kv_precompute) -> eps [nimg, 3, C, h, w] with desc's conv site / q/k blocks injecting or not"""
        lat = self._f32(latents)
        if lat.dim() != 5 or lat.shape[1] != 3:
            raise ValueError("latents must be [nimg, 3, C, h, w], got %s" % (tuple(lat.shape),))
        ctx = self._f32(context) if context is not None else None
        if ctx is not None and ctx.shape != (lat.shape[0], 3, self.cfg.ctx_len, self.cfg.cross_dim):
            raise ValueError("context must be [nimg, 3, %d, %d], got %s" % (self.cfg.ctx_len, self.cfg.cross_dim, tuple(ctx.shape)))
        out = torch.empty_like(lat)
        self._call("pnpi_unet_forward_pnp", _p(lat), lat.shape[0], int(t), _p(ctx), C.byref(desc), int(bool(conv_on)), int(bool(qk_on)), _p(out))
        self._keep = (lat, ctx, desc)
        return out

    def pnp_edit(self, src_latents, x_start, context, desc, timesteps, guidance_scale):
        """PNP.sample_loop (:393-396) for nimg images, device-resident (pnpi_pnp_edit).  src_latents [nsteps, nimg, C, h, w]: the source
        latent of every step in step order, x_start [nimg, C, h, w], context [nimg, 3, 77, D] -> latents [nimg, C, h, w]"""
        src, x, ctx = self._f32(src_latents), self._f32(x_start), self._f32(context)
        ts, tsp = self._ts(timesteps)
        if x.dim() != 4 or x.shape[1:] != (self.cfg.in_channels, self.lat_hw, self.lat_hw):
            raise ValueError("x_start must be [nimg, %d, %d, %d], got %s" % (self.cfg.in_channels, self.lat_hw, self.lat_hw, tuple(x.shape)))
        nimg = x.shape[0]
        if src.shape != (len(ts), *x.shape):
            raise ValueError("src_latents must be [nsteps, nimg, C, h, w] = %s, got %s" % ((len(ts), *x.shape), tuple(src.shape)))
        if ctx.shape != (nimg, 3, self.cfg.ctx_len, self.cfg.cross_dim):
            raise ValueError("context must be [nimg, 3, %d, %d], got %s" % (self.cfg.ctx_len, self.cfg.cross_dim, tuple(ctx.shape)))
        out = torch.empty_like(x)
        self._call("pnpi_pnp_edit", _p(src), _p(x), nimg, _p(ctx), C.byref(desc), len(ts), tsp, float(guidance_scale), _p(out))
        self._keep = (src, x, ctx, ts, desc)
        return out


    # ---- InstructPix2Pix (run_editing_instructpix2pix.py)
    def unet_t(self, latents, t, context):
        """pnpi_unet_forward at a float timestep: latents [rows, in_channels, h, w], context [rows, 77, D] (None: the rows of
        text_kv_precompute) -> eps [rows, out_channels, h, w]"""
        lat, ctx = self._f32(latents), (self._f32(context) if context is not None else None)
        want = (self.cfg.in_channels, self.lat_hw, self.lat_hw)
        if lat.dim() != 4 or lat.shape[1:] != want:
            raise ValueError("latents must be [rows, %d, %d, %d], got %s" % (*want, tuple(lat.shape)))
        out = torch.empty(lat.shape[0], self.cfg.out_channels, self.lat_hw, self.lat_hw, device=self.device)
        self._call("pnpi_unet_forward_t", _p(lat), lat.shape[0], float(t), _p(ctx), _p(out))
        self._keep = (lat, ctx)
        return out

    def ip2p_step(self, eps, z, noise, image, scalars, cfg_text, cfg_image, c_in_next=None, _symbol="pnpi_ip2p_step"):
        """One step for nimg images (CFGDenoiser :46 + one iteration of sample_euler_ancestral): eps [nimg, 3, C, h, w], z / noise / image
        [nimg, C, h, w], scalars the step's 6 floats (instructpix2pix.step_table) -> z' , or (z', inputs [nimg, 2, 2 C, h, w]) when c_in_next
        is given: the next launch's [z' * c_in_next | image] and [z' * c_in_next | 0].  noise is not read when scalars[5] == 0."""
        e, zs = self._f32(eps), self._f32(z)
        if zs.dim() != 4 or e.shape != (zs.shape[0], 3, *zs.shape[1:]):
            raise ValueError("eps must be [nimg, 3, C, h, w] and z [nimg, C, h, w], got %s and %s" % (tuple(e.shape), tuple(zs.shape)))
        nz = self._f32(noise) if noise is not None else None
        im = self._f32(image) if image is not None else None
        for name, x in (("noise", nz), ("image", im)):
            if x is not None and x.shape != zs.shape:
                raise ValueError("%s must be [nimg, C, h, w] = %s, got %s" % (name, tuple(zs.shape), tuple(x.shape)))
        sc = np.ascontiguousarray(np.asarray(scalars, dtype=np.float32).reshape(6))
        out = torch.empty_like(zs)
        nimg, ch = zs.shape[:2]
        nxt = torch.empty(nimg, 2, 2 * ch, *zs.shape[2:], device=self.device) if c_in_next is not None else None
        self._call(_symbol, _p(e), _p(zs), _p(nz), _p(im), nimg, zs[0].numel(), float(cfg_text), float(cfg_image),
                   sc.ctypes.data_as(C.POINTER(C.c_float)), float(c_in_next) if c_in_next is not None else 0.0, _p(out), _p(nxt))
        self._keep = (e, zs, nz, im, sc)
        return out if nxt is None else (out, nxt)

    def ip2p_edit(self, z0, image, noise, context, scalars, cfg_text=7.5, cfg_image=1.5, trajectory=False, _symbol="pnpi_ip2p_edit"):
        """edit_instruct_pix2pix's sampler (:125-134) for nimg images, device-resident (pnpi_ip2p_edit).  z0 [nimg, 4, h, w] = randn *
        sigmas[0], image [nimg, 4, h, w] the encoder's posterior mean (unscaled), noise [nsteps, nimg, 4, h, w] the draws in step order,
        context [nimg, 3, 77, D] = [edit, null, null], scalars [nsteps, 6] (instructpix2pix.step_table) -> z [nimg, 4, h, w], or
        (z, z after every step [nsteps, nimg, 4, h, w]) with trajectory"""
        z, im, nz, ctx = self._f32(z0), self._f32(image), self._f32(noise), self._f32(context)
        sc = np.ascontiguousarray(np.asarray(scalars, dtype=np.float32))
        if sc.ndim != 2 or sc.shape[1] != 6:
            raise ValueError("scalars must be [nsteps, 6], got %s" % (sc.shape,))
        nsteps = sc.shape[0]
        want = (self.cfg.out_channels, self.lat_hw, self.lat_hw)
        if z.dim() != 4 or z.shape[1:] != want:
            raise ValueError("z0 must be [nimg, %d, %d, %d], got %s" % (*want, tuple(z.shape)))
        nimg = z.shape[0]
        if im.shape != z.shape:
            raise ValueError("image must be [nimg, 4, h, w] = %s, got %s" % (tuple(z.shape), tuple(im.shape)))
        if nz.shape != (nsteps, *z.shape):
            raise ValueError("noise must be [nsteps, nimg, 4, h, w] = %s, got %s" % ((nsteps, *z.shape), tuple(nz.shape)))
        if ctx.shape != (nimg, 3, self.cfg.ctx_len, self.cfg.cross_dim):
            raise ValueError("context must be [nimg, 3, %d, %d], got %s" % (self.cfg.ctx_len, self.cfg.cross_dim, tuple(ctx.shape)))
        out = torch.empty_like(z)
        traj = torch.empty(nsteps, *z.shape, device=self.device) if trajectory else None
        self._call(_symbol, _p(z), _p(im), _p(nz), nimg, _p(ctx), float(cfg_text), float(cfg_image), nsteps,
                   sc.ctypes.data_as(C.POINTER(C.c_float)), _p(out), _p(traj))
        self._keep = (z, im, nz, ctx, sc)
        return (out, traj) if trajectory else out

    # ---- InstructDiffusion (run_editing_instructdiffusion.py): the same arguments, another third row and combine
    def instdiff_step(self, eps, z, noise, image, scalars, cfg_text, cfg_image, c_in_next=None):
        """ip2p_step with InstructDiffusion's combine (pnpi_instdiff_step): eps rows (text + image, null + image, text + zero image),
        0.5 * (den_1 + den_2) + cfg_text * (den_0 - den_1) + cfg_image * (den_0 - den_2)"""
        return self.ip2p_step(eps, z, noise, image, scalars, cfg_text, cfg_image, c_in_next, _symbol="pnpi_instdiff_step")

    def instdiff_edit(self, z0, image, noise, context, scalars, cfg_text=5.0, cfg_image=1.25, trajectory=False):
        """instruct_diffusion_edit's sampler (:110-120), device-resident (pnpi_instdiff_edit): ip2p_edit's arguments with context
        [nimg, 3, 77, D] = [edit, null, edit]"""
        return self.ip2p_edit(z0, image, noise, context, scalars, cfg_text, cfg_image, trajectory, _symbol="pnpi_instdiff_edit")


def pnp_desc_default(lib, cfg, nsteps):
    """pnpi_pnp_desc_default without a context (host only, no GPU): the reference's conv site, q/k blocks and schedule for this model"""
    d = _capi.PnpDesc()
    ccfg = cfg.to_c()
    st = lib.pnpi_pnp_desc_default(C.byref(ccfg), int(nsteps), C.byref(d))
    if st != 0:
        raise _capi.PnpiError(st, "pnpi_pnp_desc_default: this model has no decoder level with attention, or nsteps <= 0")
    return d



def ef_step_scalars(lib, alphas_cumprod, final_alpha, t, ratio, eta):
    """pnpi_ef_step_scalars without a context (host only, no GPU): the six fp32 scalars of one edit-friendly step."""
    ac = np.ascontiguousarray(np.asarray(alphas_cumprod, dtype=np.float32))
    out = np.zeros(6, dtype=np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))       # noqa: E731
    st = lib.pnpi_ef_step_scalars(fp(ac), len(ac), float(final_alpha), int(t), int(ratio), float(eta), fp(out))
    if st != 0:
        raise _capi.PnpiError(st, "pnpi_ef_step_scalars: invalid arguments")
    return out
