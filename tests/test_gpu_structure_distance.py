"""DINO structure distance on the device (pnpi_dino_attach, pnpi_dino_keys, pnpi_structure_distance, pnpi_op_dino_preprocess,
pnpi_op_keys_selfsim_mse; pnpinversion_amd/csrc/structdist.hip, api_structdist.inc) against the float64 restatement of
tests/test_structure_distance_host.py.

Bars, none of them taken from the device:
  resized pixels     2 ulp of fp32 of the restatement's value (the issue's bar; the kernel rounds once, from double).
  patch rows         one fp16 ulp of the restatement's value: the device rounds an fp32 value to fp16 (half an ulp) and its fp32
                     normalisation may sit on the other side of a rounding boundary.
  similarity map     per element, from the operands (u = 2^-24, fp16 keys are exact inputs to both sides):
                       |sim_dev - sim_64| <= 2 D u * sum_k |x_ik x_jk| / max(|x_i| |x_j|, 1e-8)     fp32 accumulation of D products, any order,
                                                                                                     round-to-nearest or truncating adders
                                           + (2 D u + 4 u) * |sim_64|                                the two norms (D squares each, a square
                                                                                                     root) , their product, one division
  distance           from the map's bars e = e_a + e_b per element: mean(2 |d| e + e^2) + 64 u * distance -- the squares and the fixed-order
                     fp32 sum (16 terms per lane, 6 shuffle steps, 3 adds, ceil(blocks / 256) + 8 adds, one division).
  keys, end to end   BAR_KEYS / BAR_DIST of the host test: 3 x the fp16 envelope of the restatement."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from pnpinversion_amd import _capi, metrics
from pnpinversion_amd.config import TINY16
from pnpinversion_amd.structure_distance import StructureDistance
from tests.test_structure_distance_host import (BAR_DIST, BAR_KEYS, Fixture, full_width_case, make_images, pair_inputs, rs_distance, rs_keys,
                                                rs_patch_rows, rs_preprocess)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _dc(cfg, layers=None):
    return _capi.DinoConfig.make(cfg["image_size"], cfg["patch"], cfg["width"], cfg["layers"] if layers is None else layers, cfg["heads"],
                                 cfg["intermediate"])


def _engine():
    """a context with nothing but what the metric needs: no text tower, no UNet rows, no VAE images"""
    from pnpinversion_amd.engine import NativeEngine
    return NativeEngine(dataclasses.replace(TINY16, clip_layers=0), max_unet_rows=0, max_vae_images=0)


@pytest.fixture(scope="module")
def fx():
    return Fixture()


@pytest.fixture(scope="module")
def tiny(fx):
    """the fixture's tiny tower on the device, 2 pairs (4 images) per call"""
    eng = _engine()
    sc = StructureDistance(eng, _dc(fx.cfg), max_pairs=2)
    sc.load_state_dict(fx.sd)
    yield sc
    eng.close()


@pytest.fixture(scope="module")
def full():
    """ViT-B/8 with 2 layers: T = 785, D = 768 as in the real model; one 512 x 512 pair"""
    cfg, sd, a, b = full_width_case()
    eng = _engine()
    sc = StructureDistance(eng, _dc(cfg), max_pairs=1)
    sc.load_state_dict(sd)
    yield sc, cfg, sd, a, b
    eng.close()


# ---- 1. preprocessing
def _check_preprocess(eng, imgs, masks, out, patch):
    res, pat = eng.dino_preprocess(imgs, masks, out_size=out)
    torch.cuda.synchronize()
    res, pat = res.cpu().numpy().astype(np.float64), pat.cpu().double()
    worst_r = worst_p = 0.0
    for i in range(len(imgs)):
        r, pix = rs_preprocess(imgs[i], None if masks is None else masks[i], out)
        lim = 2 * np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
        worst_r = max(worst_r, float((np.abs(res[i] - r) / lim).max()))
        ref = rs_patch_rows(pix, patch)
        ulp16 = torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float16)).astype(np.float64))
        worst_p = max(worst_p, float(((pat[i] - ref).abs() / ulp16).max()))
    print("%d images %d -> %d%s: resized at %.2f of 2 fp32 ulp, patch rows at %.2f of one fp16 ulp"
          % (len(imgs), imgs.shape[1], out, "" if masks is None else " (masked)", worst_r, worst_p))
    assert worst_r <= 1.0 and worst_p <= 1.0


@pytest.mark.parametrize("S", [32, 45, 64, 16])
def test_preprocess_tiny(tiny, S):
    imgs, masks = make_images(5, S)
    imgs = np.concatenate([imgs, np.full((1, S, S, 3), 255, np.uint8)])       # all-255: the largest normalised values (~1.13e3)
    _check_preprocess(tiny.engine, imgs, None, 32, 8)
    _check_preprocess(tiny.engine, imgs[:2], masks, 32, 8)


def test_preprocess_512_to_224(full):
    sc = full[0]
    imgs, masks = make_images(41, 512)
    _check_preprocess(sc.engine, imgs[:2], None, 224, 8)
    _check_preprocess(sc.engine, imgs[1:2], masks[1:2], 224, 8)
    _check_preprocess(sc.engine, np.full((1, 512, 512, 3), 255, np.uint8), None, 224, 8)


# ---- 2. the fused self-similarity distance on given keys
def _keys(n, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, 1, D, generator=g) * 0.6                            # a shared component: similarities away from 0
    return (base + torch.randn(n, T, D, generator=g)).half(), (base + 0.8 * torch.randn(n, T, D, generator=g)).half()


def _sim_bar(x):
    """x fp16 keys [T, D] -> (sim float64, per-element bar): the formula of the module docstring"""
    x = x.double()
    D = x.shape[1]
    n = torch.sqrt((x * x).sum(-1))
    den = torch.clamp(n[:, None] * n[None, :], min=1e-8)
    sim = (x @ x.T) / den
    return sim, 2 * D * U * (x.abs() @ x.abs().T) / den + (2 * D * U + 4 * U) * sim.abs()


def _check_selfsim(eng, ka, kb, what):
    dist, sim = eng.keys_selfsim_mse(ka, kb, want_map=True)
    dist2, _ = eng.keys_selfsim_mse(ka, kb)
    torch.cuda.synchronize()
    assert torch.equal(dist, dist2), "the same call twice must give the same bits"
    dist, sim = dist.cpu().double(), sim.cpu().double()
    assert torch.isfinite(sim).all() and torch.isfinite(dist).all()
    worst_s = worst_d = 0.0
    for p in range(ka.shape[0]):
        sa, ea = _sim_bar(ka[p])
        sb, eb = _sim_bar(kb[p])
        err = (sim[p] - sa).abs()
        assert (err <= ea).all(), "%s: a similarity-map element is outside its bar (worst %.3g x)" % (what, float((err / ea.clamp(min=1e-300)).max()))
        worst_s = max(worst_s, float((err / ea.clamp(min=1e-300))[ea > 0].max()) if bool((ea > 0).any()) else 0.0)
        d = sa - sb
        ref = float((d * d).mean())
        e = ea + eb
        lim = float((2 * d.abs() * e + e * e).mean()) + 64 * U * ref
        assert abs(float(dist[p]) - ref) <= lim, (what, p, float(dist[p]), ref, lim)
        worst_d = max(worst_d, abs(float(dist[p]) - ref) / lim if lim > 0 else 0.0)
    print("%s: map at %.3f of its bar, distance at %.3f of its bound" % (what, worst_s, worst_d))
    return dist, sim


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("D", [64, 768])
@pytest.mark.parametrize("T", [1, 17, 64, 65, 197, 785])
def test_selfsim_per_element(tiny, T, D, n):
    ka, kb = _keys(n, T, D, 1000 * T + D + n)
    _check_selfsim(tiny.engine, ka, kb, "T = %d, D = %d, n = %d" % (T, D, n))


def test_selfsim_hostile_rows(tiny):
    eng = tiny.engine
    ka, kb = _keys(2, 197, 768, 7)
    ka[0, 5] = 0                                   # an all-zero key row: sim 0 along its row and column (the eps clamp), never NaN
    ka[1, 196] = 0
    dist, sim = _check_selfsim(eng, ka, kb, "zero rows")
    assert (sim[0, 5] == 0).all() and (sim[0, :, 5] == 0).all() and (sim[1, 196] == 0).all() and (sim[1, :, 196] == 0).all()
    # rows scaled by 2^+-7: exact in fp16 (no overflow or subnormal at these magnitudes), in the fp32 dot products and in the norms
    # (2^14 under the square root), so every quotient sees the same operands times a power of two: the map does not change by a bit
    kc, kd = _keys(2, 65, 64, 11)
    kc = (torch.sign(kc.float()) * (0.25 + kc.float().abs())).half()          # magnitudes 0.25 .. ~6: / 128 stays normal in fp16, * 128 finite
    _, ref = eng.keys_selfsim_mse(kc, kd, want_map=True)
    ks = kc.clone()
    ks[:, 0::3] *= 128.0
    ks[:, 1::3] /= 128.0
    assert torch.equal(ks[:, 0::3] / 128.0, kc[:, 0::3]) and torch.equal(ks[:, 1::3] * 128.0, kc[:, 1::3])          # the scaling was exact
    _, got = eng.keys_selfsim_mse(ks, kd, want_map=True)
    assert torch.equal(got, ref)
    # keys_a == keys_b, as one buffer and as two
    for T, D in ((785, 768), (17, 64)):
        ke, _ = _keys(3, T, D, 13)
        d1, _ = eng.keys_selfsim_mse(ke, ke)
        d2, _ = eng.keys_selfsim_mse(ke, ke.clone())
        assert (d1 == 0).all() and (d2 == 0).all()


# ---- 3. keys of the tiny tower
def test_keys_per_element_and_batch_independence(tiny, fx):
    S = fx.images.shape[1]
    imgs = np.concatenate([fx.images, np.full((1, S, S, 3), 255, np.uint8)])
    ref = torch.stack([rs_keys(fx.sd, fx.cfg, rs_preprocess(im, None, fx.cfg["image_size"])[1]) for im in imgs])
    one = tiny.keys(imgs[3:4])                                                  # n = 1
    four = tiny.keys(imgs)                                                      # n = 2 * max_pairs
    torch.cuda.synchronize()
    for what, got, r in (("n = 1", one, ref[3:4]), ("n = 4", four, ref)):
        err = ((got.cpu().double() - r).abs() / r.abs().amax(-1, keepdim=True)).max()
        print("keys, %s: worst element at %.3f of the bar (%.1e of the row's largest magnitude)" % (what, float(err) / BAR_KEYS, BAR_KEYS))
        assert torch.isfinite(got).all() and float(err) <= BAR_KEYS
    assert torch.equal(one[0], four[3]), "an image's keys must not depend on the batch it is in"
    masked = tiny.keys(fx.images[:2], fx.masks)
    rm = torch.stack([rs_keys(fx.sd, fx.cfg, rs_preprocess(fx.images[i], fx.masks[i], fx.cfg["image_size"])[1]) for i in range(2)])
    assert float(((masked.cpu().double() - rm).abs() / rm.abs().amax(-1, keepdim=True)).max()) <= BAR_KEYS


# ---- 4. end to end
def test_distance_on_fixture_pairs(tiny, fx):
    ref = fx.reference()["dist"]
    ins = [pair_inputs(fx.images, fx.masks, p) for p in fx.pairs]             # whole, unedited-part and edited-part masks
    got = tiny.distance([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], [i[3] for i in ins]).cpu().double().numpy()
    print("distances: device %s, restatement %s" % (["%.5e" % v for v in got], ["%.5e" % v for v in ref]))
    for p, g, r in zip(fx.pairs, got, ref):
        if r == 0.0:
            assert g == 0.0, "a pair that is identical after masking must give exactly 0.0: %s" % (p,)
        else:
            print("pair %s at %.3f of the bar" % (p, abs(g - r) / r / BAR_DIST))
            assert abs(g - r) <= BAR_DIST * r, p
    for i in (0, 2):
        a, b, ma, mb = ins[i]
        assert metrics.calculate_structure_distance(a, b, ma, mb, scorer=tiny) == float(got[i])
    m3 = None if ins[2][2] is None else np.repeat(ins[2][2][:, :, None], 3, 2)                      # evaluate.py's [S, S, 3] repeat
    assert metrics.calculate_structure_distance(ins[2][0], ins[2][1], m3, m3, scorer=tiny) == float(got[2])


def test_full_width(full):
    sc, cfg, sd, a, b = full
    ka, kb = (rs_keys(sd, cfg, rs_preprocess(im, None, 224)[1]) for im in (a, b))
    ref = rs_distance(ka, kb)
    keys = sc.keys(np.stack([a, b])).cpu().double()
    err = float(((keys - torch.stack([ka, kb])).abs() / torch.stack([ka, kb]).abs().amax(-1, keepdim=True)).max())
    got = float(sc.distance(a[None], b[None])[0])
    print("full width: keys at %.3f of BAR_KEYS, distance %.5e vs %.5e at %.3f of BAR_DIST" % (err / BAR_KEYS, got, ref, abs(got - ref) / ref / BAR_DIST))
    assert err <= BAR_KEYS and abs(got - ref) <= BAR_DIST * ref
    assert float(sc.distance(a[None], a[None])[0]) == 0.0


# ---- 5. life cycle and refusals, all before a launch
def _refused(fn, status, *words):
    with pytest.raises(_capi.PnpiError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    torch.cuda.synchronize()                        # nothing faulted behind the refusal


def test_lifecycle_and_refusals(tiny, fx):
    img, S = fx.images, fx.images.shape[1]
    eng = _engine()
    try:
        eng.dino_cfg = _dc(fx.cfg)
        _refused(lambda: eng.dino_keys(img), _capi.PNPI_ESTATE, "pnpi_dino_attach")
        _refused(lambda: eng.structure_distance(img[:1], img[1:2]), _capi.PNPI_ESTATE, "pnpi_dino_attach")
        _refused(lambda: eng.dino_preprocess(img), _capi.PNPI_ESTATE, "pnpi_dino_attach")
        n0, names0 = eng.missing_weights()
        eng.dino_attach(_dc(fx.cfg), 1)
        assert eng.missing_weights() == (n0, names0), "pnpi_missing_weights must not count the ViT's slots"
        with pytest.raises(_capi.PnpiError) as e:
            eng.dino_keys(img[:2])
        msg = str(e.value)
        assert e.value.status == _capi.PNPI_ESTATE and "not loaded" in msg
        assert all(w in msg for w in ("dino.cls_token", "dino.pos_embed", "dino.patch_embed.proj.bias", "dino.blocks.0.mlp.fc2.weight",
                                      "dino.blocks.2.norm1.weight", "dino.blocks.2.attn.qkv.bias"))
        # the hooked block's other tensors and the final norm are neither missing ...
        assert not any(w in msg for w in ("dino.blocks.2.attn.proj", "dino.blocks.2.norm2", "dino.blocks.2.mlp", "dino.norm."))
        _refused(lambda: eng.dino_attach(_dc(fx.cfg), 1), _capi.PNPI_ESTATE, "already")
        eng.load_dino_state_dict(fx.sd)             # ... nor rejected as unknown: the full state dict loads
        _refused(lambda: eng.dino_keys(img), _capi.PNPI_EINVAL, "n out of range")                            # 3 images > 2
        _refused(lambda: eng.structure_distance(img[:2], img[1:3]), _capi.PNPI_EINVAL, "n out of range")    # 2 pairs > 1
        _refused(lambda: eng.dino_keys(img[:1, :8, :8]), _capi.PNPI_ESHAPE, "image side")                    # 8 < 16
        with pytest.raises(ValueError):
            eng.dino_keys(img[:1, :40])                                                                      # not square
        bad = fx.masks.copy()
        bad[1, 5, 7] = 2
        m = torch.from_numpy(bad).cuda()
        ii = torch.from_numpy(img[:2]).cuda()
        out = torch.zeros(2, 17, 64, device="cuda")
        st = eng.lib.pnpi_dino_keys(eng.h, C.c_void_p(ii.data_ptr()), C.c_void_p(m.data_ptr()), 2, S, C.c_void_p(out.data_ptr()))
        assert st == _capi.PNPI_EINVAL and b"0 / 1" in eng.lib.pnpi_last_error(eng.h)
        d = torch.zeros(1, device="cuda")
        st = eng.lib.pnpi_structure_distance(eng.h, C.c_void_p(ii.data_ptr()), None, C.c_void_p(ii.data_ptr()), C.c_void_p(m[1:].data_ptr()), 1, S,
                                             C.c_void_p(d.data_ptr()))
        assert st == _capi.PNPI_EINVAL and b"0 / 1" in eng.lib.pnpi_last_error(eng.h)
        for name, args in (("pnpi_dino_keys", (C.c_void_p(ii.data_ptr()), None, 1, S, None)),
                           ("pnpi_structure_distance", (C.c_void_p(ii.data_ptr()), None, C.c_void_p(ii.data_ptr()), None, 1, S, None)),
                           ("pnpi_op_dino_preprocess", (C.c_void_p(ii.data_ptr()), None, 1, S, 32, None, None)),
                           ("pnpi_op_keys_selfsim_mse", (C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr()), 1, 17, 64, None, None))):
            assert getattr(eng.lib, name)(eng.h, *args) == _capi.PNPI_EINVAL, name
            err = eng.lib.pnpi_last_error(eng.h)
            assert b"NULL" in err or b"no output" in err, (name, err)
        k = torch.zeros(1, 4, 48, dtype=torch.float16, device="cuda")
        _refused(lambda: eng.keys_selfsim_mse(k, k), _capi.PNPI_ESHAPE, "multiple of 32")
        torch.cuda.synchronize()
        assert (out == 0).all() and (d == 0).all(), "a refused call launched something"
        got = eng.dino_keys(img[:2])                # after all the refusals the context still computes: the same keys as the fixture tower
        want = tiny.engine.dino_keys(img[:2])
        assert float((got - want).abs().max()) <= BAR_KEYS * float(want.abs().max())
    finally:
        eng.close()
    again = _engine()                               # attach, destroy, attach again
    try:
        again.dino_attach(_dc(fx.cfg), 1)
        again.load_dino_state_dict(fx.sd)
        assert torch.equal(again.dino_keys(img[:2]), got)
    finally:
        again.close()


def test_refused_attach_leaves_nothing_behind(tiny, fx):
    """an attach that fails validation leaves the context without a ViT: calls still say so, the slots are gone, a good attach works"""
    img = fx.images
    assert fx.cfg["width"] % 3
    eng = _engine()
    try:
        eng.dino_cfg = _dc(fx.cfg)
        missing = eng.missing_weights()
        _refused(lambda: eng.dino_attach(_dc(dict(fx.cfg, heads=3)), 2), _capi.PNPI_ESHAPE, "heads")
        _refused(lambda: eng.dino_keys(img), _capi.PNPI_ESTATE, "pnpi_dino_attach")
        assert eng.missing_weights() == missing
        eng.dino_attach(_dc(fx.cfg), 2)
        eng.load_dino_state_dict(fx.sd)
        assert torch.equal(eng.dino_keys(img), tiny.engine.dino_keys(img))
        pair = (img[:2], img[1:3], fx.masks, fx.masks)
        assert torch.equal(eng.structure_distance(*pair), tiny.engine.structure_distance(*pair))
    finally:
        eng.close()
