"""CLIP similarity, host side (no GPU): a float64 restatement of the whole path -- uint8(img * mask), PIL's fixed-point bicubic resize,
rescale + normalise, the ViT image tower, the text tower's EOS row, the two projections, the clamped cosine -- held against the
transformers fixture tests/golden/clip_score_tiny.npz (tools/make_clip_score_golden.py) and, where transformers is installed, against a
freshly built CLIPModel; the library's host-side coefficient tables against PIL.Image.resize; evaluation/evaluate.py's CSV; the C ABI.

tests/test_gpu_clip_score.py imports the restatement (rs_*) and the tolerance from here.

Tolerance of the fp16 device path (embeddings and scores; the float64 restatement is the truth).  ENVELOPE is how far the restatement
itself moves when its weights and every layer's output go through fp16 (`.half().double()`), measured on the CPU over the fixture's tiny
towers and over the full-width 2-layer towers of the GPU test, three seeds each (test_fp16_envelope_and_bar prints the figures):
  embeddings: max |moved - exact| / max |exact| per embedding   tiny 4.9e-4 .. 1.01e-3 (image and text, seeds 5 / 6 / 7),
                                                                 full width 3.7e-4 .. 5.4e-4 (seeds 31 / 32 / 33)      -> ENVELOPE_EMB   = 1.1e-3
  scores (100 * cos, before the clamp):                          tiny 0.013 .. 0.032                                   -> ENVELOPE_SCORE = 0.035
(the largest figure measured, rounded up).  The bars are 3 x the envelope: BAR_EMB = 3.3e-3, BAR_SCORE = 0.105: one factor for the accumulation order of the MFMA GEMMs / flash attention, one for the exp / quick-GELU
approximations.  test_bar_can_fail checks that dropping the position embedding, swapping two patches and pooling the text row one
position off each move the result by more than the bar."""
import csv
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_score_tiny.npz")

ENVELOPE_EMB, ENVELOPE_SCORE = 1.1e-3, 0.035         # measured, see the module docstring
BAR_EMB, BAR_SCORE = 3 * ENVELOPE_EMB, 3 * ENVELOPE_SCORE

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
NEW_SYMBOLS = ("pnpi_clipv_config_vitl14", "pnpi_clipv_attach", "pnpi_clip_image_embed", "pnpi_clip_text_embed", "pnpi_clip_score",
               "pnpi_op_clip_preprocess", "pnpi_clip_resize_tables")


# ------------------------------------------------------------------------------------------------------------------ restatement
def rs_bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def rs_tables(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for BICUBIC -> [(first, int64 weights)] per output pixel"""
    if in_size == out_size:
        return [(i, np.array([1 << 22], np.int64)) for i in range(out_size)]
    scale = in_size / out_size
    fscale = max(scale, 1.0)
    support = 2.0 * fscale
    tabs = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = np.array([rs_bicubic((x + xmin - center + 0.5) / fscale) for x in range(xmax)], np.float64)
        w = w / w.sum()
        tabs.append((xmin, np.where(w < 0, np.trunc(-0.5 + w * (1 << 22)), np.trunc(0.5 + w * (1 << 22))).astype(np.int64)))
    return tabs


def rs_apply_tables(img, tabs_first, tabs_w):
    """one pass along axis 1 of an integer array [R, S, C] with per-output (first, weights)"""
    out = np.empty((img.shape[0], len(tabs_first), img.shape[2]), np.int64)
    for o, (f, w) in enumerate(zip(tabs_first, tabs_w)):
        acc = (1 << 21) + np.tensordot(img[:, f:f + len(w), :].astype(np.int64), w, axes=([1], [0]))
        out[:, o, :] = np.clip(acc >> 22, 0, 255)
    return out


def rs_resize(img_u8, out_size, tabs=None):
    """PIL Image.resize((out, out), BICUBIC) of a square uint8 [S, S, 3] image: horizontal pass, uint8, vertical pass, uint8"""
    tabs = tabs or rs_tables(img_u8.shape[0], out_size)
    f, w = [t[0] for t in tabs], [t[1] for t in tabs]
    h = rs_apply_tables(img_u8, f, w)
    v = rs_apply_tables(h.transpose(1, 0, 2), f, w).transpose(1, 0, 2)
    return v.astype(np.uint8)


def rs_preprocess(img_u8, mask, out_size):
    """-> (resized uint8 [out, out, 3], pixel values float64 [3, out, out])"""
    src = img_u8 if mask is None else np.uint8(img_u8 * np.asarray(mask)[:, :, None])
    r = rs_resize(src, out_size)
    x = (torch.from_numpy(r.astype(np.float64)) / 255.0 - torch.tensor(CLIP_MEAN, dtype=torch.float64)) / torch.tensor(CLIP_STD, dtype=torch.float64)
    return r, x.permute(2, 0, 1).contiguous()


def rs_patch_rows(pix, patch):
    """[3, S, S] -> [(S / p)^2, 3 p p] in the patch-embedding weight's (c, ky, kx) order, patches row-major"""
    C, S, _ = pix.shape
    g = S // patch
    return pix.reshape(C, g, patch, g, patch).permute(1, 3, 0, 2, 4).reshape(g * g, C * patch * patch)


def _ln(x, w, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5) * w + b


def rs_layer(x, sd, pre, heads, causal, rnd):
    """one CLIPEncoderLayer on x [T, H] (float64); rnd rounds the layer's output"""
    W = lambda k: rnd(sd[pre + k].double())
    T, H = x.shape
    dh = H // heads
    h = _ln(x, W(".layer_norm1.weight"), W(".layer_norm1.bias"))
    q = (h @ W(".self_attn.q_proj.weight").T + W(".self_attn.q_proj.bias")) * dh ** -0.5
    k = h @ W(".self_attn.k_proj.weight").T + W(".self_attn.k_proj.bias")
    v = h @ W(".self_attn.v_proj.weight").T + W(".self_attn.v_proj.bias")
    q, k, v = (t.reshape(T, heads, dh).transpose(0, 1) for t in (q, k, v))
    s = q @ k.transpose(1, 2)
    if causal:
        s = s + torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    a = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(T, H)
    x = x + a @ W(".self_attn.out_proj.weight").T + W(".self_attn.out_proj.bias")
    h = _ln(x, W(".layer_norm2.weight"), W(".layer_norm2.bias"))
    f = h @ W(".mlp.fc1.weight").T + W(".mlp.fc1.bias")
    f = f * torch.sigmoid(1.702 * f)
    return rnd(x + f @ W(".mlp.fc2.weight").T + W(".mlp.fc2.bias"))


_ident = lambda t: t
rs_fp16 = lambda t: t.half().double()


def rs_vision_tokens(vsd, vcfg, pix, rnd=_ident, drop_pos=False, swap=None):
    """pixel values [3, S, S] -> the tokens behind pre_layrnorm [T, W]"""
    W = lambda k: rnd(vsd["vision_model." + k].double())
    rows = rs_patch_rows(pix, vcfg["patch"])
    if swap is not None:
        rows = rows.clone()
        rows[[swap[0], swap[1]]] = rows[[swap[1], swap[0]]]
    pe = rows @ W("embeddings.patch_embedding.weight").reshape(vcfg["width"], -1).T
    x = torch.cat([W("embeddings.class_embedding")[None], pe])
    if not drop_pos:
        x = x + W("embeddings.position_embedding.weight")
    return rnd(_ln(x, W("pre_layrnorm.weight"), W("pre_layrnorm.bias")))


def rs_image_embed(vsd, vcfg, pix, rnd=_ident, layers=None, hidden=False, **kw):
    x = rs_vision_tokens(vsd, vcfg, pix, rnd, **kw)
    for l in range(vcfg["layers"] if layers is None else layers):
        x = rs_layer(x, vsd, "vision_model.encoder.layers.%d" % l, vcfg["heads"], False, rnd)
    if hidden:
        return x
    p = _ln(x[0], rnd(vsd["vision_model.post_layernorm.weight"].double()), rnd(vsd["vision_model.post_layernorm.bias"].double()))
    return rnd(rnd(p) @ rnd(vsd["visual_projection.weight"].double()).T)


def rs_text_embed(csd, tcfg, ids, tproj, rnd=_ident, shift=0):
    """ids int [T] -> text_projection of the final-LayerNorm row at the first position of the largest id (+ shift)"""
    x = rnd(csd["embeddings.token_embedding.weight"].double())[ids] + rnd(csd["embeddings.position_embedding.weight"].double())
    x = rnd(x)
    for l in range(tcfg.clip_layers):
        x = rs_layer(x, csd, "encoder.layers.%d" % l, tcfg.clip_heads, True, rnd)
    y = rnd(_ln(x, rnd(csd["final_layer_norm.weight"].double()), rnd(csd["final_layer_norm.bias"].double())))
    eos = int((ids == ids.max()).nonzero()[0]) + shift
    return rnd(y[eos] @ rnd(tproj.double()).T)


def rs_score(ie, te):
    c = (ie * te).sum(-1) / (ie.norm(dim=-1) * te.norm(dim=-1))
    return torch.clamp(100.0 * c, min=0.0), c


def emb_err(got, ref):
    """max |got - ref| / max |ref| per embedding (rows), the worst row"""
    got, ref = torch.as_tensor(got).double().reshape(-1, ref.shape[-1]), torch.as_tensor(ref).double().reshape(-1, ref.shape[-1])
    return float(((got - ref).abs().amax(-1) / ref.abs().amax(-1)).max())


# ------------------------------------------------------------------------------------------------------------------ fixture
class Fixture:
    def __init__(self):
        from pnpinversion_amd import weights
        from pnpinversion_amd.config import TINY16
        z = np.load(GOLDEN)
        self.z = z
        self.tcfg = TINY16
        self.vcfg = dict(zip(("image_size", "patch", "width", "layers", "heads", "intermediate", "proj_dim"), (int(v) for v in z["vcfg"])))
        self.vsd = {k[2:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith("w:")}
        self.csd = weights.clip_state_dict(TINY16, int(z["text_seed"]))
        self.images, self.masks = z["images"], z["masks"]
        self.variants = [(int(i), None if m < 0 else int(m)) for i, m in zip(z["variant_image"], z["variant_mask"])]
        self.ids = torch.from_numpy(z["input_ids"])
        self.pair_prompt = [int(p) for p in z["pair_prompt"]]
        self._ref = None

    def variant(self, r):
        i, m = self.variants[r]
        return self.images[i], (None if m is None else self.masks[m])

    def reference(self):
        """the float64 restatement of every fixture row, computed once: pixel values, image / text embeddings, cosines, scores"""
        if self._ref is None:
            pix = [rs_preprocess(*self.variant(r), self.vcfg["image_size"]) for r in range(len(self.variants))]
            ie = torch.stack([rs_image_embed(self.vsd, self.vcfg, p[1]) for p in pix])
            te = torch.stack([rs_text_embed(self.csd, self.tcfg, self.ids[p], self.vsd["text_projection.weight"]) for p in range(len(self.ids))])
            sc, cos = rs_score(ie, te[self.pair_prompt])
            self._ref = dict(resized=np.stack([p[0] for p in pix]), pix=torch.stack([p[1] for p in pix]), ie=ie, te=te, scores=sc, cos=cos)
        return self._ref


@pytest.fixture(scope="module")
def fx():
    return Fixture()


# ------------------------------------------------------------------------------------------------------------------ tests
def test_restatement_reproduces_fixture(fx):
    z, ref = fx.z, fx.reference()
    assert (ref["resized"] == z["resized"]).all(), "the restated PIL resize differs from the fixture's PIL output"
    assert float((ref["pix"] - torch.from_numpy(z["pixel_values"]).double()).abs().max()) < 1e-6       # fp32 rounding of O(1) values
    e_i, e_t = emb_err(z["image_embeds"], ref["ie"]), emb_err(z["text_embeds"], ref["te"])
    print("fixture (fp32 transformers) vs float64 restatement: image %.3g, text %.3g" % (e_i, e_t))
    assert e_i < 2e-5 and e_t < 2e-5
    assert float((ref["scores"] - torch.from_numpy(z["scores"]).double()).abs().max()) < 2e-3
    # the clamp is exercised: a pair of the fixture has a negative cosine, and one a positive
    assert float(ref["cos"].min()) < -0.02 and float(ref["cos"].max()) > 0.02
    assert float(ref["scores"][ref["cos"] < 0].abs().max()) == 0.0
    # vision hidden states behind the last layer
    hid = torch.stack([rs_image_embed(fx.vsd, fx.vcfg, ref["pix"][r], hidden=True) for r in range(len(fx.variants))])
    assert float((hid - torch.from_numpy(z["vision_hidden"]).double()).abs().max()) < 1e-4


def test_restatement_reproduces_fresh_clipmodel(fx):
    tr = pytest.importorskip("transformers")
    from pnpinversion_amd import weights
    v, t = fx.vcfg, fx.tcfg
    tc = tr.CLIPTextConfig(vocab_size=t.clip_vocab, hidden_size=t.cross_dim, intermediate_size=t.clip_intermediate, num_hidden_layers=t.clip_layers,
                           num_attention_heads=t.clip_heads, max_position_embeddings=t.ctx_len, hidden_act="quick_gelu", projection_dim=v["proj_dim"])
    vc = tr.CLIPVisionConfig(hidden_size=v["width"], intermediate_size=v["intermediate"], num_hidden_layers=v["layers"], num_attention_heads=v["heads"],
                             image_size=v["image_size"], patch_size=v["patch"], hidden_act="quick_gelu", projection_dim=v["proj_dim"])
    m = tr.CLIPModel(tr.CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=v["proj_dim"])).eval().double()
    csd = weights.clip_state_dict(t, 21)
    vsd = weights.clipv_state_dict(text_hidden=t.cross_dim, seed=22, **v)
    sd = {"text_model." + k: x for k, x in csd.items()}
    sd.update(vsd)
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k or k == "logit_scale" for k in missing)
    pix = fx.reference()["pix"][:3]
    with torch.no_grad():
        ie = m.visual_projection(m.vision_model(pixel_values=pix).pooler_output)
        te = m.text_projection(m.text_model(input_ids=fx.ids).pooler_output)
    mine_i = torch.stack([rs_image_embed(vsd, v, p) for p in pix])
    mine_t = torch.stack([rs_text_embed(csd, t, i, vsd["text_projection.weight"]) for i in fx.ids])
    assert emb_err(mine_i, ie) < 1e-9 and emb_err(mine_t, te) < 1e-9


def _lib_tables(in_size, out_size):
    import ctypes as C
    from pnpinversion_amd import _capi
    lib = _capi.load_library()
    ks = lib.pnpi_clip_resize_tables(in_size, out_size, None, None)
    assert ks > 0
    b, c = (C.c_int * (2 * out_size))(), (C.c_int * (ks * out_size))()
    assert lib.pnpi_clip_resize_tables(in_size, out_size, b, c) == ks
    b, c = np.array(b).reshape(out_size, 2), np.array(c).reshape(out_size, ks)
    return [(int(f), c[o, :n].astype(np.int64)) for o, (f, n) in enumerate(b)]


def test_library_tables_reproduce_pil(fx):
    """the coefficient tables the kernels apply, applied here with integer numpy: bit-exact against PIL.Image.resize (the fallback bar of
    one level per pixel is not needed)"""
    from PIL import Image
    cases = [(fx.variant(r), 28) for r in range(len(fx.variants))]
    cat = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "example_cat_512.png")).convert("RGB"))
    cases.append(((cat, None), 224))
    cases.append(((fx.images[1][:28, :28], None), 28))          # same size: PIL copies
    for (img, mask), out in cases:
        src = img if mask is None else np.uint8(img * mask[:, :, None])
        pil = np.asarray(Image.fromarray(src).resize((out, out), Image.BICUBIC))
        tabs = _lib_tables(src.shape[0], out)
        got = rs_resize(src, out, tabs)
        ndiff = int((got != pil).sum())
        print("%d -> %d: %d of %d values differ from PIL" % (src.shape[0], out, ndiff, pil.size))
        assert ndiff == 0
        mine = rs_tables(src.shape[0], out)
        assert all(a[0] == b[0] and (a[1] == b[1]).all() for a, b in zip(tabs, mine)), "library tables differ from the restated ones"
    from pnpinversion_amd import _capi
    assert _capi.load_library().pnpi_clip_resize_tables(28, 64, None, None) == _capi.PNPI_ESHAPE


def _full_width_case(seed, n_img=1):
    """the full-width 2-layer towers of the GPU test: weights, inputs and the float64 restatement"""
    from pnpinversion_amd import weights
    vcfg = dict(image_size=224, patch=14, width=1024, layers=2, heads=16, intermediate=4096, proj_dim=768)
    vsd = weights.clipv_state_dict(text_hidden=64, seed=seed, **vcfg)
    g = np.random.Generator(np.random.Philox(key=[seed, 224]))
    imgs = g.integers(0, 256, (n_img, 224, 224, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:224, 0:224]
    imgs[0] = np.clip(np.stack([xx, yy, 255 - xx], -1) + g.normal(0, 20, (224, 224, 3)), 0, 255).astype(np.uint8)
    return vcfg, vsd, imgs


def test_fp16_envelope_and_bar(fx):
    """measures the envelope the module docstring quotes (printed) and holds the constants against it"""
    from pnpinversion_amd import weights
    emb, sc = [], []
    for seed in (5, 6, 7):           # the tiny towers, three seeds (5 = the fixture's)
        vsd = weights.clipv_state_dict(text_hidden=fx.tcfg.cross_dim, seed=seed, **fx.vcfg)
        csd = weights.clip_state_dict(fx.tcfg, seed - 2)
        pix = fx.reference()["pix"]
        ie = torch.stack([rs_image_embed(vsd, fx.vcfg, p) for p in pix])
        ie16 = torch.stack([rs_image_embed(vsd, fx.vcfg, rs_fp16(p), rs_fp16) for p in pix])
        te = torch.stack([rs_text_embed(csd, fx.tcfg, i, vsd["text_projection.weight"]) for i in fx.ids])
        te16 = torch.stack([rs_text_embed(csd, fx.tcfg, i, vsd["text_projection.weight"], rs_fp16) for i in fx.ids])
        emb += [emb_err(ie16, ie), emb_err(te16, te)]
        s, _ = rs_score(ie, te[fx.pair_prompt]); s16, _ = rs_score(ie16, te16[fx.pair_prompt])
        raw = 100 * (rs_score(ie, te[fx.pair_prompt])[1] - rs_score(ie16, te16[fx.pair_prompt])[1]).abs().max()
        sc.append(float(raw))
    print("tiny: embedding envelope %s, score envelope %s" % (["%.2e" % e for e in emb], ["%.3f" % s for s in sc]))
    assert max(emb) <= ENVELOPE_EMB and max(sc) <= ENVELOPE_SCORE
    assert max(emb) > ENVELOPE_EMB / 10 and max(sc) > ENVELOPE_SCORE / 10, "the constants are far above what was measured: re-measure"


def test_fp16_envelope_full_width():
    emb = []
    for seed in (31, 32, 33):
        vcfg, vsd, imgs = _full_width_case(seed)
        _, pix = rs_preprocess(imgs[0], None, 224)
        e = rs_image_embed(vsd, vcfg, pix)
        e16 = rs_image_embed(vsd, vcfg, rs_fp16(pix), rs_fp16)
        emb.append(emb_err(e16, e))
    print("full width, 2 layers: embedding envelope %s" % ["%.2e" % e for e in emb])
    assert max(emb) <= ENVELOPE_EMB


def test_bar_can_fail(fx):
    """each mistake the issue names moves the result by more than the bar, on the fixture's inputs"""
    ref = fx.reference()
    pix = ref["pix"]
    nopos = torch.stack([rs_image_embed(fx.vsd, fx.vcfg, p, drop_pos=True) for p in pix])
    swapped = torch.stack([rs_image_embed(fx.vsd, fx.vcfg, p, swap=(0, 3)) for p in pix])
    tproj = fx.vsd["text_projection.weight"]
    off = torch.stack([rs_text_embed(fx.csd, fx.tcfg, i, tproj, shift=-1) for i in fx.ids])
    per_row = lambda a, b: ((a - b).abs().amax(-1) / b.abs().amax(-1))
    for name, e in (("no position embedding", per_row(nopos, ref["ie"])), ("patches 0 and 3 swapped", per_row(swapped, ref["ie"])),
                    ("text row one position early", per_row(off, ref["te"]))):
        print("%s: embedding moves by %s (bar %.1e)" % (name, ["%.3f" % float(x) for x in e], BAR_EMB))
        assert float(e.min()) > BAR_EMB, name
    for name, ie, te in (("no position embedding", nopos, ref["te"]), ("patches swapped", swapped, ref["te"]), ("text row early", ref["ie"], off)):
        d = 100 * (rs_score(ie, te[fx.pair_prompt])[1] - ref["cos"]).abs()
        print("%s: 100 cos moves by %s (bar %.2f)" % (name, ["%.2f" % float(x) for x in d], BAR_SCORE))
        assert float(d.max()) > BAR_SCORE, name


def test_eos_rule_agrees_between_tokenizers(fx):
    from pnpinversion_amd.text import EOS, WordTokenizer, eos_positions
    ids = WordTokenizer()(["a cat", "", "x " * 100], padding="max_length", max_length=77).input_ids
    pos = eos_positions(ids.numpy())
    assert (pos == ids.argmax(-1).numpy()).all()                      # transformers' rule for the real vocabulary
    assert all(int(ids[r, p]) == EOS and (ids[r, :p] != EOS).all() for r, p in enumerate(pos))
    assert list(pos) == [3, 1, 76]


def test_tower_gemm_shapes_have_a_plan():
    """every GEMM the image tower launches at full width (M = n * 257 tails, the padded K = 640 patch embedding, the projection with
    M = n) is accepted by the launcher's host-side plan, with the LDS-DMA kernels, for n = 1, 3, 8"""
    import ctypes as C
    from pnpinversion_amd import _capi
    lib = _capi.load_library()
    W, I, P, T, NP, Kp = 1024, 4096, 768, 257, 256, 640
    for n in (1, 3, 8):
        shapes = [(n * NP, W, Kp, 0), (n * T, 3 * W, W, 1), (n * T, W, W, 0), (n * T, I, W, 0), (n * T, W, I, 0), (n, P, W, 0), (n, P, 768, 0)]
        for M, N, K, vt in shapes:
            d = _capi.IgemmLaunchDesc()
            d.M, d.N, d.K, d.ksize, d.C1, d.C2 = M, N, K, 1, K, 0
            d.ldx1, d.ldw, d.ldo, d.ldres = K, K, (2 * W if vt else N), N
            d.bias, d.bias_aligned16 = 1, 1
            d.vt_col0, d.vt_ld, d.rows_per_batch, d.nbatch = (2 * W if vt else N), (264 if vt else 0), (T if vt else 1), 1
            d.ws_bytes, d.force_cfg = 96 << 20, -1
            pl = _capi.IgemmPlan()
            assert lib.pnpi_igemm_plan_query(C.byref(d), C.byref(pl)) == 0
            assert pl.err == 0 and pl.dma == 1 and pl.gx * pl.bm >= M and pl.gy * pl.bn >= N, (M, N, K, pl.err, pl.id)


def test_new_symbols_everywhere():
    from pnpinversion_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "pnpi.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _capi.SYMBOLS and hasattr(lib, s) and s in doc, s
    import ctypes as C
    g = _capi.ClipvConfig()
    lib.pnpi_clipv_config_vitl14(C.byref(g))
    assert [getattr(g, f) for f, _ in g._fields_] == [C.sizeof(g), 224, 14, 1024, 24, 16, 4096, 768]


# ------------------------------------------------------------------------------------------------------------------ evaluate.py
class _StubScorer:
    def __init__(self):
        self.calls = []

    def score(self, images, prompts, masks=None):
        self.calls.append((len(images), list(prompts), None if masks is None else [m is not None for m in masks]))
        return torch.arange(len(images), dtype=torch.float32) + 1.0


def _bench_dir(tmp_path):
    from PIL import Image
    import json
    g = np.random.default_rng(0)
    src = tmp_path / "data" / "annotation_images"
    out = tmp_path / "output" / "directinversion+p2p" / "annotation_images"
    src.mkdir(parents=True); out.mkdir(parents=True)
    mapping = {}
    for key, mask in (("000000000000", [512 * 100 + 50, 300]), ("000000000001", [])):
        Image.fromarray(g.integers(0, 256, (512, 512, 3), dtype=np.uint8)).save(src / (key + ".png"))
        Image.fromarray(g.integers(0, 256, (512, 2048, 3), dtype=np.uint8)).save(out / (key + ".png"))      # a four-panel output
        mapping[key] = dict(image_path=key + ".png", mask=mask, original_prompt="a [cat] on a chair", editing_prompt="a [dog] on a chair",
                            editing_type_id="1")
    (tmp_path / "data" / "mapping_file.json").write_text(json.dumps(mapping))
    return tmp_path


def test_evaluate_csv_layout_and_nan(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    d = _bench_dir(tmp_path)
    monkeypatch.chdir(d)
    metrics = ["psnr_unedit_part", "mse_unedit_part", "ssim_unedit_part", "clip_similarity_source_image", "clip_similarity_target_image",
               "clip_similarity_target_image_edit_part", "psnr_edit_part"]
    stub = _StubScorer()
    evaluate.run(evaluate.parse_args(["--metrics"] + metrics + ["--tgt_methods", "1_directinversion+p2p", "--result_path", "r.csv"]), scorer=stub)
    rows = list(csv.reader(open(d / "r.csv", newline="")))
    assert rows[0] == ["file_id"] + ["1_directinversion+p2p|" + m for m in metrics]
    assert [r[0] for r in rows[1:]] == ["000000000000", "000000000001"]
    # the mask of image 1 is its one-pixel border only: not empty, so nothing is "nan" there; one CLIP launch set per image
    assert all(len(r) == 1 + len(metrics) for r in rows[1:])
    assert len(stub.calls) == 2 and stub.calls[0][0] == 3 and stub.calls[0][1] == ["a cat on a chair", "a dog on a chair", "a dog on a chair"]
    assert stub.calls[0][2] == [False, False, True]
    assert rows[1][4:7] == ["1.0", "2.0", "3.0"]
    # "nan" cells: a mask that covers the whole image has an empty unedited part
    full = evaluate.calculate_metric(None, "psnr_unedit_part", None, None, np.ones((4, 4, 3)), np.ones((4, 4, 3)), "", "")
    empty = evaluate.calculate_metric(None, "clip_similarity_target_image_edit_part", None, None, np.zeros((4, 4, 3)), np.zeros((4, 4, 3)), "", "")
    assert full == "nan" and empty == "nan"
    assert evaluate.all_tgt_image_folders["4_null-text-inverse+p2p_a800"] == "output/null-text-inversion+p2p_a800/annotation_images"
    assert evaluate.all_tgt_image_folders["6_ablation_directinversion_interval_2"] == "output/ablation_directinversion_interval_2+p2p/annotation_images"
    assert len(evaluate.all_tgt_image_folders) == 60


@pytest.mark.parametrize("metric", ["lpips_unedit_part", "structure_distance", "lpips", "structure_distance_edit_part"])
def test_evaluate_refuses_unbuilt_columns_by_name(metric):
    """the run ends (SystemExit with a message, i.e. exit status 1 and the message on stderr) before any file is opened"""
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.run(evaluate.parse_args(["--metrics", "psnr", metric, "--annotation_mapping_file", "/nonexistent.json"]))
    assert isinstance(e.value.code, str) and repr(metric) in e.value.code and "not built" in e.value.code
