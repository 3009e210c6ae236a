"""DINO structure distance, host side (no GPU): a float64 restatement of the reference's whole path
(evaluation/matrics_calculator.py of the reference):
  1. calculate_structure_distance :385-405   the images as float32 0..255 (no / 255), times a 0 / 1 mask, CHW
  2. LossG.global_transform :182-187         Resize(224, max_size=480) on a TENSOR = interpolate(bilinear, align_corners=False), no
                                             antialiasing (torchvision 0.13.1); Normalize(ImageNet mean, std) on the 0..255 values
  3. VitExtractor :154-164, :140-145         dino_vitb8 up to the hook on blocks[11].attn.qkv; keys = the K third, heads side by side
  4. attn_cosine_sim :166-171                sim = x x^T / clamp(|x| |x|^T, min=1e-8)
  5. calculate_global_ssim_loss :237-246     F.mse_loss(sim_pred, sim_gt): the mean over all T^2 entries
held against torch (interpolate on CPU float32; a transcription of attn_cosine_sim + F.mse_loss in float64), the library's host-side tap
table, the fixture tests/golden/structure_distance_tiny.npz, and evaluation/evaluate.py's CSV.

tests/test_gpu_structure_distance.py imports the restatement (rs_*) and the bars from here.

Bars of the fp16 device path (the float64 restatement is the truth).  The ENVELOPE is how far the restatement itself moves when its
input pixels, its weights, every layer's output and its keys go through fp16 (`.half().double()`), measured on the CPU
(test_fp16_envelope_* print the figures and hold the constants against them):
  keys, max |moved - exact| / max |exact row| per element:  tiny tower (3 layers, the fixture's image variants) 9.05e-4 / 7.72e-4 / 8.89e-4
                                                            for seeds 5 / 6 / 7; full width (ViT-B/8 with 2 layers, one 512 x 512 pair,
                                                            seed 41) 6.73e-4                                       -> ENVELOPE_KEYS = 1.0e-3
  distance, |moved - exact| / exact:                        the fixture's pairs 4.02e-4 / 3.64e-4 / 6.75e-4, the full-width pair
                                                            (distance 1.93e-2) 3.51e-4                             -> ENVELOPE_DIST = 7e-4
BAR_KEYS = 3.0e-3 and BAR_DIST = 2.1e-3 are 3 x the largest figure (rounded up): one factor for the accumulation order of the MFMA GEMMs / flash
attention, one for the exp / erf approximations.  A relative bar on the distance means something only where the distance is far above
its own movement: test_pairs_are_well_conditioned holds every test pair at distance >= 100 x the absolute movement seen."""
import csv
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "structure_distance_tiny.npz")

ENVELOPE_KEYS, ENVELOPE_DIST = 1.0e-3, 7e-4           # measured, see the module docstring and DESIGN 7i
BAR_KEYS, BAR_DIST = 3 * ENVELOPE_KEYS, 3 * ENVELOPE_DIST

IMNET_MEAN = (0.485, 0.456, 0.406)
IMNET_STD = (0.229, 0.224, 0.225)
TINY = dict(image_size=32, patch=8, width=64, layers=3, heads=2, intermediate=256)
NEW_SYMBOLS = ("pnpi_dino_config_vitb8", "pnpi_dino_attach", "pnpi_dino_keys", "pnpi_structure_distance", "pnpi_op_dino_preprocess",
               "pnpi_op_keys_selfsim_mse", "pnpi_dino_resize_taps")


# ------------------------------------------------------------------------------------------------------------------ restatement
def rs_taps(in_size, out_size):
    """PyTorch's compute_source_index_and_lambda, align_corners=False, in its fp32 arithmetic -> (idx0, idx1 int64 [out], lambda1 fp32 [out])"""
    o = np.arange(out_size)
    if in_size == out_size:
        return o.copy(), o.copy(), np.zeros(out_size, np.float32)
    f = np.float32
    scale = f(in_size) / f(out_size)
    src = scale * (o.astype(f) + f(0.5)) - f(0.5)
    src = np.maximum(src, f(0)).astype(f)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    lam = np.clip(src - i0.astype(f), f(0), f(1)).astype(f)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, lam


def rs_resize(x, out_size):
    """x float64 [3, S, S] -> [3, out, out]: the two-tap formula with the fp32 weights (lambda0 = 1 - lambda1 formed in fp32), in float64"""
    i0, i1, l1 = rs_taps(x.shape[1], out_size)
    l0 = (np.float32(1) - l1).astype(np.float64)
    l1 = l1.astype(np.float64)
    rows = x[:, i0, :] * l0[None, :, None] + x[:, i1, :] * l1[None, :, None]
    return rows[:, :, i0] * l0[None, None, :] + rows[:, :, i1] * l1[None, None, :]


def rs_preprocess(img_u8, mask, out_size):
    """-> (resized float64 [3, out, out] in 0..255, normalised pixel values float64 torch [3, out, out])"""
    x = img_u8.astype(np.float64)
    if mask is not None:
        x = x * np.asarray(mask, np.float64)[:, :, None]
    r = rs_resize(x.transpose(2, 0, 1), out_size)
    pix = (r - np.array(IMNET_MEAN)[:, None, None]) / np.array(IMNET_STD)[:, None, None]
    return r, torch.from_numpy(pix)


def rs_patch_rows(pix, patch):
    """[3, S, S] -> [(S / p)^2, 3 p p] in the patch-embedding weight's (c, ky, kx) order, patches row-major"""
    C, S, _ = pix.shape
    g = S // patch
    return pix.reshape(C, g, patch, g, patch).permute(1, 3, 0, 2, 4).reshape(g * g, C * patch * patch)


def _ln(x, w, b):
    m = x.mean(-1, keepdim=True)
    v = ((x - m) ** 2).mean(-1, keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-6) * w + b


_ident = lambda t: t
rs_fp16 = lambda t: t.half().double()


def rs_block(x, sd, pre, heads, rnd):
    """one DINO Block on x [T, W] (float64): x += proj(attn(norm1(x))); x += fc2(gelu(fc1(norm2(x)))); rnd rounds the block's output"""
    W_ = lambda k: rnd(sd[pre + k].double())
    T, W = x.shape
    dh = W // heads
    qkv = _ln(x, W_(".norm1.weight"), W_(".norm1.bias")) @ W_(".attn.qkv.weight").T + W_(".attn.qkv.bias")
    q, k, v = (t.transpose(0, 1) for t in qkv.reshape(T, 3, heads, dh).unbind(1))      # output columns [3][heads][dh]
    a = (torch.softmax(q @ k.transpose(1, 2) * dh ** -0.5, -1) @ v).transpose(0, 1).reshape(T, W)
    x = x + a @ W_(".attn.proj.weight").T + W_(".attn.proj.bias")
    f = _ln(x, W_(".norm2.weight"), W_(".norm2.bias")) @ W_(".mlp.fc1.weight").T + W_(".mlp.fc1.bias")
    f = 0.5 * f * (1.0 + torch.erf(f / 2.0 ** 0.5))
    return rnd(x + f @ W_(".mlp.fc2.weight").T + W_(".mlp.fc2.bias"))


def rs_keys(sd, cfg, pix, rnd=_ident, drop_pos=False):
    """normalised pixel values [3, S, S] -> the concatenated keys of the last block [T, W]: blocks 0 .. L - 2 in full, then norm1 and the
    K rows (W .. 2 W - 1) of the last block's qkv"""
    W = cfg["width"]
    P = lambda k: rnd(sd[k].double())
    pe = rs_patch_rows(pix, cfg["patch"]) @ P("patch_embed.proj.weight").reshape(W, -1).T + P("patch_embed.proj.bias")
    x = torch.cat([P("cls_token")[0], pe])
    if not drop_pos:
        x = x + P("pos_embed")[0]
    x = rnd(x)
    L = cfg["layers"]
    for l in range(L - 1):
        x = rs_block(x, sd, "blocks.%d" % l, cfg["heads"], rnd)
    pre = "blocks.%d" % (L - 1)
    h = _ln(x, P(pre + ".norm1.weight"), P(pre + ".norm1.bias"))
    return rnd(h @ P(pre + ".attn.qkv.weight")[W:2 * W].T + P(pre + ".attn.qkv.bias")[W:2 * W])


def rs_selfsim(x):
    n = torch.sqrt((x * x).sum(-1))
    return (x @ x.T) / torch.clamp(n[:, None] * n[None, :], min=1e-8)


def rs_distance(ka, kb):
    return float(((rs_selfsim(ka) - rs_selfsim(kb)) ** 2).mean())


def keys_err(got, ref):
    """max |got - ref| / max |ref row| per element, the worst element"""
    got, ref = torch.as_tensor(got).double().reshape(ref.shape), torch.as_tensor(ref).double()
    return float(((got - ref).abs() / ref.abs().amax(-1, keepdim=True)).max())


# ------------------------------------------------------------------------------------------------------------------ test inputs
def make_images(seed=5, S=45):
    """three uint8 [S, S, 3] images with structure (gradients, a disc, stripes + noise) and two 0 / 1 masks [S, S]"""
    g = np.random.Generator(np.random.Philox(key=[seed, S]))
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64) / (S - 1)
    a = np.stack([255 * xx, 255 * yy, 255 * (1 - xx)], -1) + g.normal(0, 12, (S, S, 3))
    b = a.copy()
    disc = (xx - 0.6) ** 2 + (yy - 0.4) ** 2 < 0.07
    b[disc] = [250, 30, 40]
    c = 127 + 100 * np.sin(14 * xx + 5 * yy)[:, :, None] * np.array([1.0, -1.0, 0.5]) + g.normal(0, 25, (S, S, 3))
    imgs = np.clip(np.stack([a, b, c]), 0, 255).astype(np.uint8)
    m0 = np.zeros((S, S), np.uint8)
    m0[S // 5: S // 5 + S // 2, S // 3: S // 3 + S // 2] = 1
    m1 = (disc | (yy > 0.8)).astype(np.uint8)
    return imgs, np.stack([m0, m1])


# pairs of the fixture: (pred image, gt image, mask index or None for both sides, complement?)
PAIRS = [(0, 1, None, False), (0, 1, 1, True), (0, 1, 1, False), (0, 2, None, False), (2, 1, 0, False), (1, 1, None, False)]


def pair_inputs(imgs, masks, p):
    a, b, m, comp = p
    mk = None if m is None else ((1 - masks[m]) if comp else masks[m])
    return imgs[a], imgs[b], mk, mk


def full_width_case(seed=41):
    """ViT-B/8 with 2 layers (T = 785, D = 768 as in the real model), seeded weights, one 512 x 512 pair"""
    from pnpinversion_amd import weights
    cfg = dict(image_size=224, patch=8, width=768, layers=2, heads=12, intermediate=3072)
    sd = weights.dino_state_dict(seed=seed, **cfg)
    imgs, _ = make_images(seed, 512)
    return cfg, sd, imgs[0], imgs[1]


class Fixture:
    def __init__(self):
        from pnpinversion_amd import weights
        z = np.load(GOLDEN)
        self.z = z
        self.cfg = dict(zip(("image_size", "patch", "width", "layers", "heads", "intermediate"), (int(v) for v in z["cfg"])))
        self.seed = int(z["seed"])
        self.sd = weights.dino_state_dict(seed=self.seed, **self.cfg)
        self.images, self.masks = z["images"], z["masks"]
        self.pairs = [(int(a), int(b), None if m < 0 else int(m), bool(c)) for a, b, m, c in z["pairs"]]
        self._ref = None

    def variants(self):
        """every distinct (image, mask) the pairs use -> index"""
        out = {}
        for p in self.pairs:
            for img in p[:2]:
                out.setdefault((img, p[2], p[3]), len(out))
        return out

    def variant_inputs(self, key):
        img, m, comp = key
        return self.images[img], None if m is None else ((1 - self.masks[m]) if comp else self.masks[m])

    def reference(self, sd=None, rnd=_ident):
        """the float64 restatement of every fixture pair, computed once: keys per (image, mask) variant, distance per pair"""
        if sd is None and rnd is _ident and self._ref is not None:
            return self._ref
        var = self.variants()
        keys = [None] * len(var)
        for key, i in var.items():
            pix = rs_preprocess(*self.variant_inputs(key), self.cfg["image_size"])[1]
            keys[i] = rs_keys(sd or self.sd, self.cfg, rnd(pix), rnd)
        dist = [rs_distance(keys[var[(a, m, c)]], keys[var[(b, m, c)]]) for a, b, m, c in self.pairs]
        ref = dict(keys=torch.stack(keys), dist=np.array(dist))
        if sd is None and rnd is _ident:
            self._ref = ref
        return ref


@pytest.fixture(scope="module")
def fx():
    return Fixture()


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("S,out", [(512, 224), (224, 224), (32, 224), (225, 224), (45, 32), (16, 32)])
def test_resize_restatement_against_torch_interpolate(S, out):
    """the reference's Resize on a tensor.  torch evaluates the same taps in fp32: the index arithmetic of the two may differ where the
    compiler contracts scale * (o + 0.5) - 0.5 into one FMA (one rounding of a value below S: 2^-24 S in lambda, 255 times that in the
    pixel), and the interpolation itself carries a few fp32 roundings of values up to 255 (4 x 2^-24 x 255)"""
    g = np.random.default_rng(S)
    img = g.integers(0, 256, (S, S, 3)).astype(np.uint8)
    got = rs_resize(img.astype(np.float64).transpose(2, 0, 1), out)
    x = torch.from_numpy(img.astype(np.float32)).permute(2, 0, 1)[None]
    ref = torch.nn.functional.interpolate(x, size=(out, out), mode="bilinear", align_corners=False, antialias=False)[0].double().numpy()
    d = float(np.abs(got - ref).max())
    tol = 255 * 2.0 ** -24 * (4 + 2 * S)
    print("%d -> %d: restatement vs torch float32 interpolate: max |diff| %.3g (tolerance %.3g)" % (S, out, d, tol))
    assert d <= tol
    if S == out:
        assert (got == img.transpose(2, 0, 1)).all()


def test_selfsim_and_mse_against_torch_transcription():
    """attn_cosine_sim (:166-171) and F.mse_loss as the reference writes them, in float64, zero row included"""
    g = torch.Generator().manual_seed(3)
    for T, D in ((17, 64), (40, 96)):
        xa, xb = torch.randn(T, D, generator=g, dtype=torch.float64), torch.randn(T, D, generator=g, dtype=torch.float64)
        xa[3] = 0

        def attn_cosine_sim(x, eps=1e-08):
            x = x[0]
            norm1 = x.norm(dim=2, keepdim=True)
            factor = torch.clamp(norm1 @ norm1.permute(0, 2, 1), min=eps)
            return (x @ x.permute(0, 2, 1)) / factor

        sa, sb = attn_cosine_sim(xa[None, None]), attn_cosine_sim(xb[None, None])
        assert float((rs_selfsim(xa) - sa[0]).abs().max()) < 1e-14 and (rs_selfsim(xa)[3] == 0).all()
        assert abs(rs_distance(xa, xb) - float(torch.nn.functional.mse_loss(sa, sb))) < 1e-15


def _lib_taps(in_size, out_size):
    import ctypes as C
    from pnpinversion_amd import _capi
    lib = _capi.load_library()
    i0, i1, lam = (C.c_int * out_size)(), (C.c_int * out_size)(), (C.c_float * out_size)()
    assert lib.pnpi_dino_resize_taps(in_size, out_size, i0, i1, lam) == 0
    return np.array(i0), np.array(i1), np.array(lam, np.float32)


@pytest.mark.parametrize("S,out", [(512, 224), (224, 224), (32, 224), (225, 224), (45, 32), (16, 32), (8192, 224)])
def test_library_taps(S, out):
    """the tap table the preprocess kernel applies, from the library with no GPU: indices exact, weights within 1 ulp of fp32"""
    i0, i1, lam = _lib_taps(S, out)
    r0, r1, rl = rs_taps(S, out)
    assert (i0 == r0).all() and (i1 == r1).all()
    assert (np.abs(lam.astype(np.float64) - rl.astype(np.float64)) <= np.spacing(np.maximum(rl, np.float32(2.0 ** -126)))).all()
    assert i0.min() >= 0 and i1.max() <= S - 1 and (lam >= 0).all() and (lam <= 1).all()
    if S == out:
        assert (i0 == np.arange(out)).all() and (i1 == i0).all() and (lam == 0).all()
    from pnpinversion_amd import _capi
    assert _capi.load_library().pnpi_dino_resize_taps(9000, 224, None, None, None) == _capi.PNPI_ESHAPE


def test_restatement_reproduces_fixture(fx):
    """passes whether the values are read or recomputed: the fixture's inputs are make_images' and its results the restatement's"""
    z, ref = fx.z, fx.reference()
    imgs, masks = make_images(fx.seed, fx.images.shape[1])
    assert (imgs == fx.images).all() and (masks == fx.masks).all() and fx.cfg == TINY and fx.pairs == PAIRS
    assert float((ref["keys"] - torch.from_numpy(z["keys"])).abs().max()) < 1e-9
    assert np.abs(ref["dist"] - z["dist"]).max() < 1e-12
    # two pairs are identical after masking (the same image twice; images 0 and 1 differ only inside mask 1, which the unedited part
    # clears): exactly 0.  Every other pair is far from it.
    same = np.array([bool((np.asarray(a) * (1 if m is None else m[:, :, None]) == np.asarray(b) * (1 if m is None else m[:, :, None])).all())
                     for a, b, m, _ in (pair_inputs(fx.images, fx.masks, p) for p in fx.pairs)])
    assert list(same) == [False, True, False, False, False, True]
    assert (ref["dist"][same] == 0.0).all() and (ref["dist"][~same] > 1e-3).all()


def _envelope(keys, keys16, dist, dist16):
    ek = max(keys_err(a, b) for a, b in zip(keys16, keys))
    nz = dist > 0
    return ek, float((np.abs(dist16 - dist)[nz] / dist[nz]).max()), float(np.abs(dist16 - dist).max())


def test_fp16_envelope_tiny(fx):
    from pnpinversion_amd import weights
    ek, ed = [], []
    for seed in (5, 6, 7):
        sd = weights.dino_state_dict(seed=seed, **fx.cfg)
        a, b = fx.reference(sd if seed != fx.seed else None), fx.reference(sd, rs_fp16)
        k, d, _ = _envelope(a["keys"], b["keys"], a["dist"], b["dist"])
        ek.append(k); ed.append(d)
    print("tiny: keys envelope %s, distance envelope %s" % (["%.2e" % e for e in ek], ["%.2e" % e for e in ed]))
    assert max(ek) <= ENVELOPE_KEYS and max(ed) <= ENVELOPE_DIST


def _full_width_reference(rnd=_ident):
    cfg, sd, a, b = full_width_case()
    keys = [rs_keys(sd, cfg, rnd(rs_preprocess(im, None, 224)[1]), rnd) for im in (a, b)]
    return torch.stack(keys), rs_distance(*keys)


def test_fp16_envelope_full_width_and_constants():
    k, d = _full_width_reference()
    k16, d16 = _full_width_reference(rs_fp16)
    ek, ed = keys_err(k16, k), abs(d16 - d) / d
    print("full width, 2 layers: keys envelope %.2e, distance %.4e moved by %.2e relative" % (ek, d, ed))
    assert ek <= ENVELOPE_KEYS and ed <= ENVELOPE_DIST
    assert d >= 100 * abs(d16 - d)
    assert max(ek / ENVELOPE_KEYS, ed / ENVELOPE_DIST) > 0.05, "the constants are far above what was measured: re-measure"


def test_pairs_are_well_conditioned(fx):
    """every non-identical test pair's restated distance is at least 100 x the absolute movement under fp16 rounding"""
    a, b = fx.reference(), fx.reference(fx.sd, rs_fp16)
    for p, d, d16 in zip(fx.pairs, a["dist"], b["dist"]):
        print("pair %s: distance %.4e, moved by %.2e" % (p, d, abs(d16 - d)))
        assert (d16 == 0.0) if d == 0.0 else d >= 100 * abs(d16 - d), p


def test_bar_can_fail(fx):
    """mistakes the issue warns of move the result by more than the bars: no position embedding; the reference's 0..255 input divided by 255"""
    ref = fx.reference()
    var = fx.variants()
    key = (0, None, False)
    img, _ = fx.variant_inputs(key)
    pix = rs_preprocess(img, None, fx.cfg["image_size"])[1]
    nopos = rs_keys(fx.sd, fx.cfg, pix, drop_pos=True)
    r = rs_resize(img.astype(np.float64).transpose(2, 0, 1) / 255.0, fx.cfg["image_size"])
    unit = rs_keys(fx.sd, fx.cfg, torch.from_numpy((r - np.array(IMNET_MEAN)[:, None, None]) / np.array(IMNET_STD)[:, None, None]))
    for name, k in (("no position embedding", nopos), ("pixels / 255", unit)):
        e = keys_err(k, ref["keys"][var[key]])
        print("%s: keys move by %.3f (bar %.1e)" % (name, e, BAR_KEYS))
        assert e > BAR_KEYS
    other = ref["keys"][var[(1, None, False)]]
    d0 = ref["dist"][0]
    for name, k in (("no position embedding", nopos), ("pixels / 255", unit)):
        d = rs_distance(k, other)
        print("%s: distance moves by %.3f relative (bar %.1e)" % (name, abs(d - d0) / d0, BAR_DIST))
        assert abs(d - d0) / d0 > BAR_DIST


def test_new_symbols_everywhere():
    import ctypes as C
    from pnpinversion_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "pnpi.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _capi.SYMBOLS and hasattr(lib, s) and s in doc, s
    g = _capi.DinoConfig()
    lib.pnpi_dino_config_vitb8(C.byref(g))
    assert [getattr(g, f) for f, _ in g._fields_] == [C.sizeof(g), 224, 8, 768, 12, 12, 3072]


def test_seeded_weights_and_dropped_tensors():
    """the seeded state dict carries DINO's own keys, block 11's unused tensors and norm.* included (the loader drops them), and its patch
    embedding turns 0..255-normalised pixels into O(1) tokens, the all-255 image included"""
    from pnpinversion_amd import weights
    sd = weights.dino_state_dict(seed=5, **TINY)
    for k in ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "blocks.2.attn.proj.weight", "blocks.2.mlp.fc2.bias",
              "blocks.2.norm2.weight", "norm.weight", "norm.bias", "blocks.0.attn.qkv.weight"):
        assert k in sd, k
    assert all(bool((v == v.half().float()).all()) for v in sd.values())
    assert float(sd["patch_embed.proj.weight"].abs().min()) > 6.2e-5           # fp16 normal range
    imgs, _ = make_images(5, 45)
    for img in (imgs[0], np.full((45, 45, 3), 255, np.uint8)):
        pix = rs_preprocess(img, None, 32)[1]
        pe = rs_patch_rows(pix, 8) @ sd["patch_embed.proj.weight"].double().reshape(64, -1).T
        assert 0.05 < float(pe.abs().mean()) < 20 and float(pe.abs().max()) < 100


# ------------------------------------------------------------------------------------------------------------------ evaluate.py
class _StubStruct:
    def __init__(self):
        self.calls = []

    def distance(self, pred, gt, mask_pred=None, mask_gt=None):
        self.calls.append((len(pred), [None if m is None else float(np.asarray(m).mean()) for m in mask_pred],
                           [np.asarray(p).shape for p in pred], [np.asarray(p).shape for p in gt]))
        return torch.arange(len(pred), dtype=torch.float32) + 0.5


def _bench_dir(tmp_path):
    from PIL import Image
    import json
    g = np.random.default_rng(0)
    src = tmp_path / "data" / "annotation_images"
    out = tmp_path / "output" / "directinversion+p2p" / "annotation_images"
    src.mkdir(parents=True); out.mkdir(parents=True)
    mapping = {}
    for key, mask in (("000000000000", [512 * 100 + 50, 300]), ("000000000001", [0, 512 * 512])):      # the second mask covers everything
        Image.fromarray(g.integers(0, 256, (512, 512, 3), dtype=np.uint8)).save(src / (key + ".png"))
        Image.fromarray(g.integers(0, 256, (512, 2048, 3), dtype=np.uint8)).save(out / (key + ".png"))
        mapping[key] = dict(image_path=key + ".png", mask=mask, original_prompt="a [cat]", editing_prompt="a [dog]", editing_type_id="1")
    (tmp_path / "data" / "mapping_file.json").write_text(json.dumps(mapping))
    return tmp_path


def test_evaluate_structure_columns(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    d = _bench_dir(tmp_path)
    monkeypatch.chdir(d)
    metrics = ["structure_distance", "psnr_unedit_part", "structure_distance_unedit_part", "structure_distance_edit_part"]
    stub = _StubStruct()
    evaluate.run(evaluate.parse_args(["--metrics"] + metrics + ["--tgt_methods", "1_directinversion+p2p", "--result_path", "r.csv"]), struct_scorer=stub)
    rows = list(csv.reader(open(d / "r.csv", newline="")))
    assert rows[0] == ["file_id"] + ["1_directinversion+p2p|" + m for m in metrics]
    # image 0: the three columns arrive in ONE call -- whole (no mask), unedited part (1 - mask), edited part (mask); (src, tgt) order
    assert len(stub.calls) == 2 and stub.calls[0][0] == 3
    assert stub.calls[0][1][0] is None and stub.calls[0][1][1] > 0.9 and stub.calls[0][1][2] < 0.1
    assert all(s == (512, 512, 3) for s in stub.calls[0][2] + stub.calls[0][3])                    # the right-hand 512 crop of the panel
    assert [rows[1][1], rows[1][3], rows[1][4]] == ["0.5", "1.5", "2.5"]
    # image 1: its mask covers the whole image, so the unedited part is empty: "nan" there, and only two pairs reach the device
    assert stub.calls[1][0] == 2 and rows[2][3] == "nan" and rows[2][2] == "nan" and [rows[2][1], rows[2][4]] == ["0.5", "1.5"]
    # single cells through the Calculator protocol, the reference's "nan" rule
    calc = evaluate.Calculator(None, stub)
    ones, zeros = np.ones((4, 4, 3)), np.zeros((4, 4, 3))
    img = np.zeros((4, 4, 3), np.uint8)
    assert evaluate.calculate_metric(calc, "structure_distance_unedit_part", img, img, ones, ones, "", "") == "nan"
    assert evaluate.calculate_metric(calc, "structure_distance_edit_part", img, img, zeros, zeros, "", "") == "nan"
    assert evaluate.calculate_metric(calc, "structure_distance", img, img, zeros, zeros, "", "") == 0.5


@pytest.mark.parametrize("metric", ["structure_distance", "structure_distance_unedit_part", "structure_distance_edit_part", "lpips"])
def test_evaluate_refusals(metric):
    """without DINO weights the column is refused by name before any file is opened; lpips stays refused with them"""
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.run(evaluate.parse_args(["--metrics", "psnr", metric, "--annotation_mapping_file", "/nonexistent.json"]))
    assert isinstance(e.value.code, str) and repr(metric) in e.value.code and "not built" in e.value.code
    if metric == "lpips":
        with pytest.raises(SystemExit) as e:
            evaluate.run(evaluate.parse_args(["--metrics", metric, "--dino_checkpoint", "/nonexistent.pth"]))
        assert "not built" in e.value.code
    else:
        evaluate.check_metrics(["psnr", metric], dino=True)                       # computable once weights are named
        assert evaluate.has_dino_weights(evaluate.parse_args(["--dino_checkpoint", "x.pth"]))
        assert metric in evaluate.STRUCT_METRICS and evaluate.DEFAULT_METRICS[0] == "structure_distance"
