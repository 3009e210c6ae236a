"""CLIP similarity on the device (pnpi_clipv_attach, pnpi_clip_*; pnpinversion_amd/csrc/clipscore.hip, api_clipscore.inc) against the
float64 restatement of tests/test_clip_score_host.py and against PIL.

Bars (derived on the CPU in test_clip_score_host.py, not from the device): embeddings BAR_EMB = 3.3e-3 of the embedding's largest
magnitude per element, scores BAR_SCORE = 0.105 -- 3 x the envelope by which the restatement itself moves under fp16 rounding of its
weights and layer outputs.  The resized image is compared with PIL bit for bit.  Patch rows: the device rounds an fp32 value to fp16
(half an ulp) and its fp32 arithmetic may sit on the other side of a rounding boundary from the float64 restatement: one fp16 ulp,
2^-10 relative (+ the smallest normal's spacing near zero)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from pnpinversion_amd import _capi, weights
from pnpinversion_amd.config import TINY16
from tests.test_clip_score_host import (BAR_EMB, BAR_SCORE, ROOT, Fixture, _full_width_case, rs_image_embed, rs_patch_rows, rs_preprocess,
                                        rs_score)

pytestmark = pytest.mark.gpu


def _vc(v, layers=None):
    return _capi.ClipvConfig.make(v["image_size"], v["patch"], v["width"], v["layers"] if layers is None else layers, v["heads"],
                                  v["intermediate"], v["proj_dim"])


def _engine(cfg=TINY16, seed=None):
    from pnpinversion_amd.engine import NativeEngine
    eng = NativeEngine(cfg, max_unet_rows=4, max_vae_images=1)
    if seed is not None:
        eng.load_state_dict(clip_sd=weights.clip_state_dict(cfg, seed))
    return eng


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture(scope="module")
def tiny(fx):
    """the fixture's towers on the device: TINY16 text tower + the tiny image tower, up to 3 images per call"""
    eng = _engine(seed=int(fx.z["text_seed"]))
    eng.clipv_attach(_vc(fx.vcfg), 3)
    eng.load_clipv_state_dict(fx.vsd)
    yield eng
    eng.close()


def _per_element(got, ref, bar, what):
    """every element within bar x the largest magnitude of its row of the reference; prints the worst ratio"""
    got, ref = got.detach().cpu().double().reshape(ref.shape), ref.double()
    lim = bar * ref.abs().amax(-1, keepdim=True)
    worst = float(((got - ref).abs() / lim).max())
    print("%s: worst element at %.3f of the bar (%.1e of the row's largest magnitude)" % (what, worst, bar))
    assert torch.isfinite(got).all() and worst <= 1.0, what


# ---- 1. preprocessing
def _check_preprocess(eng, imgs, masks, out, patch):
    from PIL import Image
    res, pat = eng.clip_preprocess(imgs, masks, out_size=out)
    torch.cuda.synchronize()
    res, pat = res.cpu().numpy(), pat.cpu()
    K, ndiff = 3 * patch * patch, 0
    for i in range(len(imgs)):
        src = imgs[i] if masks is None else np.uint8(imgs[i] * masks[i][:, :, None])
        pil = np.asarray(Image.fromarray(src).resize((out, out), Image.BICUBIC))
        ndiff += int((res[i] != pil).sum())
        _, pix = rs_preprocess(imgs[i], None if masks is None else masks[i], out)
        ref = rs_patch_rows(pix, patch)
        got = pat[i].double()
        assert (got[:, K:] == 0).all(), "pad columns of the patch rows are not zero"
        bound = ref.abs() * 2.0 ** -10 + 2.0 ** -14
        assert ((got[:, :K] - ref).abs() <= bound).all(), "patch rows differ from the restatement by more than one fp16 ulp"
    print("%d images %d -> %d%s: %d values differ from PIL" % (len(imgs), imgs.shape[1], out, "" if masks is None else " (masked)", ndiff))
    assert ndiff == 0


def test_preprocess_fixture_images(tiny, fx):
    _check_preprocess(tiny, fx.images, None, 28, 14)
    _check_preprocess(tiny, fx.images[[0, 2]], fx.masks, 28, 14)


def test_preprocess_512_to_224(tiny):
    from PIL import Image
    cat = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "example_cat_512.png")).convert("RGB"))[None]
    mask = np.zeros((1, 512, 512), np.uint8)
    mask[0, 100:333, 57:401] = 1
    _check_preprocess(tiny, cat, None, 224, 14)
    _check_preprocess(tiny, cat, mask, 224, 14)


# ---- 2. one encoder layer, the full tiny tower
def test_one_layer_and_tiny_tower_per_element(tiny, fx):
    ref = fx.reference()
    got = tiny.clip_image_embed(fx.images)
    _per_element(got, ref["ie"][:3], BAR_EMB, "tiny tower, 2 layers")
    got_m = tiny.clip_image_embed(fx.images[[0, 2]], fx.masks)
    _per_element(got_m, ref["ie"][3:], BAR_EMB, "tiny tower, masked images")
    eng1 = _engine(seed=int(fx.z["text_seed"]))
    try:
        eng1.clipv_attach(_vc(fx.vcfg, layers=1), 3)
        eng1.load_clipv_state_dict(fx.vsd)
        one = torch.stack([rs_image_embed(fx.vsd, fx.vcfg, p, layers=1) for p in ref["pix"][:3]])
        _per_element(eng1.clip_image_embed(fx.images), one, BAR_EMB, "tiny tower, 1 layer")
    finally:
        eng1.close()
    te = tiny.clip_text_embed(fx.ids)
    _per_element(te, ref["te"], BAR_EMB, "text tower -> EOS row -> text_projection")


# ---- 3. the full-width shapes: 257 tokens, width 1024, 16 heads, intermediate 4096, 2 layers, projection 768
@pytest.fixture(scope="module")
def full():
    vcfg, vsd, imgs = _full_width_case(31, n_img=3)
    eng = _engine()
    eng.clipv_attach(_vc(vcfg), 3)
    eng.load_clipv_state_dict(vsd)
    ref = torch.stack([rs_image_embed(vsd, vcfg, rs_preprocess(imgs[i], None, 224)[1]) for i in range(3)])
    yield eng, imgs, ref
    eng.close()


@pytest.mark.parametrize("n", [1, 3])
def test_full_width_two_layers(full, n):
    eng, imgs, ref = full
    _per_element(eng.clip_image_embed(imgs[:n]), ref[:n], BAR_EMB, "full width, n = %d" % n)


# ---- 4. scores, the clamp, the masked variant
def test_scores_on_fixture(tiny, fx):
    ref = fx.reference()
    ids = fx.ids[fx.pair_prompt]
    plain = tiny.clip_score(fx.images, ids[:3]).cpu().double()
    masked = tiny.clip_score(fx.images[[0, 2]], ids[3:], fx.masks).cpu().double()
    got = torch.cat([plain, masked])
    print("scores: device %s, restatement %s" % (["%.3f" % v for v in got], ["%.3f" % v for v in ref["scores"]]))
    assert float((got - ref["scores"]).abs().max()) <= BAR_SCORE
    neg = ref["cos"] < 0
    assert bool(neg.any()) and float(ref["cos"][neg].max()) * 100 < -BAR_SCORE        # checked on the CPU: clearly negative pairs exist
    assert (got[neg] == 0).all(), "a negative cosine must clamp to exactly 0"
    # the cosine before the clamp, from the embeddings
    ie = torch.cat([tiny.clip_image_embed(fx.images), tiny.clip_image_embed(fx.images[[0, 2]], fx.masks)]).cpu().double()
    te = torch.cat([tiny.clip_text_embed(ids[:3]), tiny.clip_text_embed(ids[3:])]).cpu().double()
    assert float((100 * (rs_score(ie, te)[1] - ref["cos"])).abs().max()) <= BAR_SCORE


# ---- 5. rows do not mix
def test_rows_are_independent(tiny, fx):
    ids = fx.ids[[2, 0, 1]]                        # three different images with three different prompts
    batch = tiny.clip_score(fx.images, ids).cpu()
    emb = tiny.clip_image_embed(fx.images).cpu()
    for i in range(3):
        one = tiny.clip_score(fx.images[i:i + 1], ids[i:i + 1]).cpu()
        e1 = tiny.clip_image_embed(fx.images[i:i + 1]).cpu()
        assert abs(float(one[0] - batch[i])) <= BAR_SCORE, i
        assert float((e1[0] - emb[i]).abs().max()) <= BAR_EMB * float(emb[i].abs().max()), i
    assert len({round(float(v), 3) for v in batch}) > 1, "identical rows would hide a mix-up"


# ---- 6. refusals, all before a launch
def _refused(fn, status, *words):
    with pytest.raises(_capi.PnpiError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    torch.cuda.synchronize()                        # nothing faulted behind the refusal


def test_refusals(tiny, fx):
    img, ids = fx.images, fx.ids
    eng = _engine(seed=int(fx.z["text_seed"]))
    try:
        eng.clipv_cfg = _vc(fx.vcfg)
        _refused(lambda: eng.clip_score(img, ids), _capi.PNPI_ESTATE, "pnpi_clipv_attach")
        _refused(lambda: eng.clip_image_embed(img), _capi.PNPI_ESTATE, "pnpi_clipv_attach")
        _refused(lambda: eng.clip_text_embed(ids), _capi.PNPI_ESTATE, "pnpi_clipv_attach")
        _refused(lambda: eng.clip_preprocess(img), _capi.PNPI_ESTATE, "pnpi_clipv_attach")
        n0, names0 = eng.missing_weights()
        eng.clipv_attach(_vc(fx.vcfg), 2)
        assert eng.missing_weights() == (n0, names0), "pnpi_missing_weights must not count the image tower's slots"
        _refused(lambda: eng.clip_score(img[:2], ids[:2]), _capi.PNPI_ESTATE, "not loaded", "clipv.visual_projection.weight",
                 "clipv.text_projection.weight", "clipv.vision_model.pre_layrnorm.weight", "clipv.vision_model.encoder.layers.1.mlp.fc2.bias")
        _refused(lambda: eng.clipv_attach(_vc(fx.vcfg), 2), _capi.PNPI_ESTATE, "already")
        eng.load_clipv_state_dict(fx.vsd)
        _refused(lambda: eng.clip_score(img, ids), _capi.PNPI_EINVAL, "max_images")              # 3 > 2
        _refused(lambda: eng.clip_image_embed(img[:1, :24, :24]), _capi.PNPI_ESHAPE, "image side")   # 24 < 28
        bad = fx.masks.copy()
        bad[1, 5, 7] = 2
        m = torch.from_numpy(bad).cuda()
        ii, dd = torch.from_numpy(img[:2]).cuda(), ids[:2].to("cuda", torch.int32)
        out = torch.zeros(2, device="cuda")
        st = eng.lib.pnpi_clip_score(eng.h, C.c_void_p(ii.data_ptr()), C.c_void_p(m.data_ptr()), C.c_void_p(dd.data_ptr()), 2, 64, C.c_void_p(out.data_ptr()))
        assert st == _capi.PNPI_EINVAL and b"0 / 1" in eng.lib.pnpi_last_error(eng.h)
        torch.cuda.synchronize()
        assert (out == 0).all()
        assert float((eng.clip_score(img[:2], ids[:2]).cpu() - tiny.clip_score(img[:2], ids[:2]).cpu()).abs().max()) == 0.0
    finally:
        eng.close()
    no_text = _engine(dataclasses.replace(TINY16, clip_layers=0))
    try:
        _refused(lambda: no_text.clipv_attach(_vc(fx.vcfg), 2), _capi.PNPI_ESTATE, "text tower")
    finally:
        no_text.close()


def test_refused_attach_leaves_nothing_behind(tiny, fx):
    """an attach that fails validation leaves the context without a tower: calls still say so, the slots are gone, a good attach works"""
    img = fx.images
    assert fx.vcfg["width"] % 7
    eng = _engine(seed=int(fx.z["text_seed"]))
    try:
        eng.clipv_cfg = _vc(fx.vcfg)
        missing = eng.missing_weights()
        _refused(lambda: eng.clipv_attach(_vc(dict(fx.vcfg, heads=7)), 3), _capi.PNPI_ESHAPE, "heads")
        _refused(lambda: eng.clip_image_embed(img), _capi.PNPI_ESTATE, "pnpi_clipv_attach")
        assert eng.missing_weights() == missing
        eng.clipv_attach(_vc(fx.vcfg), 3)
        eng.load_clipv_state_dict(fx.vsd)
        assert torch.equal(eng.clip_image_embed(img), tiny.clip_image_embed(img))
        assert torch.equal(eng.clip_score(img[[0, 2]], fx.ids[:2], fx.masks), tiny.clip_score(img[[0, 2]], fx.ids[:2], fx.masks))
    finally:
        eng.close()


# ---- 7. the CLIP image tower and the DINO ViT on one context: each swaps its arena and its workspaces in and out of the same context
@pytest.fixture(scope="module")
def dino_alone():
    """the DINO fixture's tiny tower on a context of its own, built as the `tiny` fixture of tests/test_gpu_structure_distance.py is"""
    from pnpinversion_amd.structure_distance import StructureDistance
    from tests import test_gpu_structure_distance as d
    dfx = d.Fixture()
    eng = d._engine()
    sc = StructureDistance(eng, d._dc(dfx.cfg), max_pairs=2)
    sc.load_state_dict(dfx.sd)
    yield dfx, eng
    eng.close()


def test_both_towers_on_one_context(tiny, fx, dino_alone):
    from tests.test_gpu_structure_distance import _dc
    dfx, dino = dino_alone
    ids = fx.ids[[2, 0]]
    pair = (dfx.images[:1], dfx.images[1:2], dfx.masks[:1], dfx.masks[:1])
    want = [tiny.clip_score(fx.images[:2], ids), dino.structure_distance(*pair), dino.dino_keys(dfx.images[1:3]),
            tiny.clip_score(fx.images[[0, 2]], ids, fx.masks), tiny.text_encode(fx.ids), tiny.clip_image_embed(fx.images[1:2])]
    for life in range(2):                           # build, attach both, load, compute, destroy -- twice
        eng = _engine(seed=int(fx.z["text_seed"]))
        try:
            missing = eng.missing_weights()
            eng.clipv_attach(_vc(fx.vcfg), 2)
            assert eng.missing_weights() == missing
            eng.dino_attach(_dc(dfx.cfg), 1)
            assert eng.missing_weights() == missing
            eng.load_clipv_state_dict(fx.vsd)
            eng.load_dino_state_dict(dfx.sd)
            got = [eng.clip_score(fx.images[:2], ids), eng.structure_distance(*pair), eng.dino_keys(dfx.images[1:3]),
                   eng.clip_score(fx.images[[0, 2]], ids, fx.masks), eng.text_encode(fx.ids), eng.clip_image_embed(fx.images[1:2])]
            for i, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), "life %d, call %d differs from the single-tower context" % (life, i)
        finally:
            eng.close()


def test_text_tower_unchanged_by_the_image_tower(tiny, fx):
    """a context without the tower behaves as before, and attaching one changes neither the text encoder's bits nor its launches"""
    plain = _engine(seed=int(fx.z["text_seed"]))
    try:
        a = plain.text_encode(fx.ids)
        plain.profile_begin()
        plain.text_encode(fx.ids)
        prof = plain.profile_end()
        tiny.profile_begin()
        b = tiny.text_encode(fx.ids)
        prof_t = tiny.profile_end()
        assert torch.equal(a, b)
        L = TINY16.clip_layers
        launches = {k: v["launches"] for k, v in prof.items() if v["launches"]}
        assert launches == {k: v["launches"] for k, v in prof_t.items() if v["launches"]}
        assert launches.pop("layernorm") == 2 * L + 1 and launches.pop("attn_flash") == L and sum(launches.values()) == 4 * L, launches
        assert not any(n.startswith("clipv.") for n in plain.missing_weights()[1])
    finally:
        plain.close()
