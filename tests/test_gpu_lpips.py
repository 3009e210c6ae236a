"""LPIPS (SqueezeNet) on the device (pnpi_lpips_attach, pnpi_lpips, pnpi_lpips_features, pnpi_op_lpips_layer, pnpi_op_maxpool3s2_ceil;
pnpinversion_amd/csrc/lpips.hip, api_lpips.inc) against the float64 restatement of tests/test_lpips_host.py.

Bars, none of them taken from the device (u = 2^-24):
  conv1 (tap 0)      per element.  The kernel forms every input value in double and rounds it to fp32 once (relative error u), starts its
                     accumulator at the bias and adds the 27 products by FMAs, one rounding each: with A = |bias| + sum_k |w_k x_k| the
                     fp32 value is within (1 + 27 + 1) u A = 29 u A of the exact one (the last u covers the second-order terms).  ReLU does
                     not enlarge an error; the fp16 store adds half an ulp of the stored value: 2^-11 of it, or 2^-25 below fp16's normal range.
                       bar = e + 2^-11 (relu(ref) + e) + 2^-25,  e = 29 u A
  pool               bit-exact: a maximum of fp16 values rounds nothing.
  tap distance       per pair, from the fp16 operands (exact inputs to both sides), C channels:
                       norms      C squares summed in fp32 (any order: C u), + 1e-8 in fp32 (2 u), the root halves it and adds u / 2
                       quotient   one more rounding:                           |a^_dev - a^| <= eq |a^|,  eq = (C / 2 + 3) u
                       difference one rounding:                                e_df = eq (|a^| + |b^|) + u |df|
                       square     one rounding:                                e_t  = 2 |df| e_df + e_df^2 + u (|df| + e_df)^2
                       weighted sum over C, FMAs and shuffle adds:             e_d  = sum_c |w_c| e_t + (C + 1) u sum_c |w_c| (df^2 + e_t)
                       mean       at most 64 pixels per lane in walk order, an 8-level tree, ceil(blocks / 256) + 8 adds in the second
                                  kernel, one division: under 96 roundings:    bar = mean(e_d) + 96 u mean(sum_c |w_c| (df^2 + e_t))
  taps, end to end   BAR_FEAT / BAR_SCORE of the host test: 3 x the fp16 envelope of the restatement."""
import ctypes as C
import dataclasses
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pnpinversion_amd import _capi, metrics
from pnpinversion_amd.config import TINY16
from pnpinversion_amd.lpips import Lpips
from tests.test_lpips_host import (BAR_FEAT, BAR_SCORE, PAIRS, ROOT, SEED, TAP_CHANNELS, ZERO_PAIRS, case, feat_err, make_images, pair_inputs,
                                   rs_conv1, rs_input, rs_score, rs_taps)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _engine(cfg=None):
    """a context with nothing but what the metric needs: no text tower, no UNet rows, no VAE images"""
    from pnpinversion_amd.engine import NativeEngine
    return NativeEngine(cfg or dataclasses.replace(TINY16, clip_layers=0), max_unet_rows=0, max_vae_images=0)


@pytest.fixture(scope="module")
def sc():
    """the seeded network on the device, 4 pairs (8 images) per call"""
    eng = _engine()
    s = Lpips(eng, max_pairs=4)
    s.sd = s.load_synthetic(SEED)
    yield s
    eng.close()


# ---- 1. the first convolution with the preprocessing in front (tap 0)
@pytest.mark.parametrize("S", [17, 32, 34, 65])
def test_conv1_per_element(sc, S):
    imgs, masks = make_images(SEED, S)
    w, b = sc.sd["features.0.weight"].double(), sc.sd["features.0.bias"].double()
    worst = 0.0
    for batch, mk in ((imgs, None), (imgs[:1], None), (imgs, np.stack([masks[0], masks[1], 1 - masks[1]])), (imgs[1:2], masks[1:2]),
                      (np.stack([np.full((S, S, 3), 255, np.uint8), np.zeros((S, S, 3), np.uint8)]), None)):
        got = sc.features(batch, mk, tap=0).cpu().double().permute(0, 3, 1, 2)
        for i in range(len(batch)):
            x = rs_input(batch[i], None if mk is None else mk[i])
            ref = rs_conv1(x, w, b)[0]
            e = 29 * U * rs_conv1(x.abs(), w.abs(), b.abs())[0]
            bar = e + 2.0 ** -11 * (torch.relu(ref) + e) + 2.0 ** -25
            assert got[i].shape == ref.shape
            worst = max(worst, float(((got[i] - torch.relu(ref)).abs() / bar).max()))
    print("conv1 at S = %d: at %.3f of the per-element bar" % (S, worst))
    assert worst <= 1.0


# ---- 2. the ceil-mode pool, bit-exact
@pytest.mark.parametrize("H", [3, 4, 7, 8, 15, 16, 2])
def test_maxpool_bit_exact(sc, H):
    for Cc in (8, 64, 136):
        for n in (1, 2):
            g = torch.Generator().manual_seed(H * 1000 + Cc + n)
            x = (torch.randn(n, H, H, Cc, generator=g) * 3 - 1).half()              # negative values too: no maximum starts at zero
            ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, ceil_mode=True).permute(0, 2, 3, 1).half()
            got = sc.engine.maxpool3s2_ceil(x).cpu()
            assert got.shape == ref.shape and torch.equal(got, ref), (H, Cc, n)
    assert H % 2 == 1 or (F.max_pool2d(torch.zeros(1, 1, H, H), 3, 2, ceil_mode=True).shape[-1] - 1) * 2 + 3 > H     # even sides: the last window overhangs


# ---- 3. the fused tap distance on given feature maps
def _layer_ref(a, b, w):
    """fp16 [n, HW, C] x 2, w [C] -> (exact value, bar) per pair in float64, as the module docstring derives it"""
    a, b, w = a.double(), b.double(), w.double()
    Cc = a.shape[-1]
    ah = a / torch.sqrt(1e-8 + (a * a).sum(-1, keepdim=True))
    bh = b / torch.sqrt(1e-8 + (b * b).sum(-1, keepdim=True))
    df = ah - bh
    eq = (Cc / 2 + 3) * U
    e_df = eq * (ah.abs() + bh.abs()) + U * df.abs()
    e_t = 2 * df.abs() * e_df + e_df ** 2 + U * (df.abs() + e_df) ** 2
    mag = (w.abs() * (df ** 2 + e_t)).sum(-1)
    e_d = (w.abs() * e_t).sum(-1) + (Cc + 1) * U * mag
    return (w * df ** 2).sum(-1).mean(-1), e_d.mean(-1) + 96 * U * mag.mean(-1)


@pytest.mark.parametrize("Cc", [8, 64, 384, 512])
def test_lpips_layer_per_pair(sc, Cc):
    worst = 0.0
    for HW in (1, 9, 961, 1023):
        for n in (1, 3):
            g = torch.Generator().manual_seed(Cc * 7 + HW + n)
            a = torch.relu(torch.randn(n, HW, Cc, generator=g) * 2).half()
            b = torch.relu(a.float() + torch.randn(n, HW, Cc, generator=g)).half()
            w = torch.randn(Cc, generator=g)                                         # mixed signs: the kernel must not assume w >= 0
            a[0, 0] = 0                                                              # an all-zero vector on one side ...
            if HW > 1:
                a[-1, HW // 2] = 0; b[-1, HW // 2] = 0                               # ... and on both: that pixel adds nothing
            ref, bar = _layer_ref(a, b, w)
            got = sc.engine.lpips_layer(a, b, w).cpu().double()
            assert bool(torch.isfinite(got).all())
            worst = max(worst, float(((got - ref).abs() / bar).max()))
            assert float(sc.engine.lpips_layer(a, a, w).abs().max()) == 0.0          # a == b as two buffers (lpips_layer copies each) ...
            ad, wd = a.cuda(), w.cuda()
            out = torch.full((n,), 7.0, device="cuda")
            sc.engine._call("pnpi_op_lpips_layer", C.c_void_p(ad.data_ptr()), C.c_void_p(ad.data_ptr()), C.c_void_p(wd.data_ptr()), n, HW, Cc,
                            C.c_void_p(out.data_ptr()))
            assert float(out.abs().max()) == 0.0                                     # ... and as one
    z = torch.zeros(2, 5, Cc, dtype=torch.float16)
    assert float(sc.engine.lpips_layer(z, z, torch.ones(Cc)).abs().max()) == 0.0     # both sides all zero everywhere: exactly 0
    print("tap distance at C = %d: at %.3f of the per-pair bar" % (Cc, worst))
    assert worst <= 1.0


# ---- 4. the seven taps
@pytest.mark.parametrize("S", [34, 65])
def test_tap_features(sc, S):
    c = case(S)
    mk = np.stack([c.masks[1], c.masks[1], c.masks[1]])
    for masks in (None, mk):
        worst = 0.0
        for tap in range(7):
            got = sc.features(c.imgs, masks, tap=tap).cpu().double().permute(0, 3, 1, 2)
            for i in range(3):
                ref = c.taps(i, None if masks is None else masks[i])[tap][0]
                assert got[i].shape == ref.shape and ref.shape[0] == TAP_CHANNELS[tap]
                worst = max(worst, feat_err(got[i], ref))
        print("S = %d%s: taps at %.3f of BAR_FEAT" % (S, "" if masks is None else " (masked)", worst / BAR_FEAT))
        assert worst <= BAR_FEAT
    for tap in (0, 3, 6):                                                            # an image's features do not depend on the batch it is in
        full = sc.features(c.imgs, None, tap=tap)
        for i in range(3):
            assert torch.equal(sc.features(c.imgs[i:i + 1], None, tap=tap)[0], full[i]), (tap, i)


# ---- 5. the score
def test_scores_end_to_end(sc):
    c = case(65)
    ref = c.scores()
    ins = [pair_inputs(c.imgs, c.masks, p) for p in PAIRS]
    args = [np.stack([i[0] for i in ins]), np.stack([i[1] for i in ins]), [i[2] for i in ins], [i[3] for i in ins]]
    got = sc.score(*args).cpu().double().numpy()
    again = sc.score(*args).cpu().double().numpy()
    assert (got == again).all(), "the same call twice must give the same bits"
    for i, p in enumerate(PAIRS):
        print("pair %s: %.6e vs %.6e%s" % (p, got[i], ref[i], "" if i in ZERO_PAIRS else " at %.3f of BAR_SCORE" % (abs(got[i] - ref[i]) / ref[i] / BAR_SCORE)))
        if i in ZERO_PAIRS:
            assert got[i] == 0.0 and ref[i] == 0.0, p                               # identical, or identical after masking: exactly 0
        else:
            assert abs(got[i] - ref[i]) <= BAR_SCORE * ref[i], p
    for i in (1, 2):                                                                 # one cell through metrics: the same bits, either mask layout
        a, b, ma, mb = ins[i]
        assert metrics.calculate_lpips(a, b, ma, mb, scorer=sc) == float(np.float32(got[i]))
        assert metrics.calculate_lpips(a, b, ma[:, :, None].repeat(3, 2), mb[:, :, None].repeat(3, 2), scorer=sc) == float(np.float32(got[i]))
    assert float(sc.score(args[0][:1], args[1][:1])[0]) == float(np.float32(got[0]))    # nor on the batch it is in


@pytest.fixture(scope="module")
def real_shape():
    """one 512 x 512 pair (maps of 255 / 127 / 63 / 31), restated once"""
    c = case(512)
    ta, tb = rs_taps(c.sd, rs_input(c.imgs[0])), rs_taps(c.sd, rs_input(c.imgs[2]))
    return c, ta, tb, rs_score(c.sd, ta, tb)


def test_real_shape_512(sc, real_shape):
    c, ta, tb, ref = real_shape
    assert [t.shape[-1] for t in ta] == [255, 127, 63, 31, 31, 31, 31]
    got = float(sc.score(c.imgs[0:1], c.imgs[2:3])[0])
    f6 = sc.features(c.imgs[[0, 2]], None, tap=6).cpu().double().permute(0, 3, 1, 2)
    ef = max(feat_err(f6[0], ta[6][0]), feat_err(f6[1], tb[6][0]))
    print("512 x 512: score %.6e vs %.6e at %.3f of BAR_SCORE; last tap at %.3f of BAR_FEAT" % (got, ref, abs(got - ref) / ref / BAR_SCORE, ef / BAR_FEAT))
    assert abs(got - ref) <= BAR_SCORE * ref and ef <= BAR_FEAT
    assert float(sc.score(c.imgs[0:1], c.imgs[0:1])[0]) == 0.0


# ---- 6. life cycle and refusals, all before a launch
def _refused(fn, status, *words):
    with pytest.raises(_capi.PnpiError) as e:
        fn()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)
    torch.cuda.synchronize()                        # nothing faulted behind the refusal


def test_lifecycle_and_refusals(sc):
    S = 34
    img, masks = make_images(SEED, S)
    eng = _engine()
    try:
        _refused(lambda: eng.lpips_features(img), _capi.PNPI_ESTATE, "pnpi_lpips_attach")
        _refused(lambda: eng.lpips(img[:1], img[1:2]), _capi.PNPI_ESTATE, "pnpi_lpips_attach")
        n0, names0 = eng.missing_weights()
        _refused(lambda: eng.lpips_attach(0), _capi.PNPI_EINVAL, "max_pairs")                           # a refused attach leaves nothing behind
        _refused(lambda: eng.lpips_features(img), _capi.PNPI_ESTATE, "pnpi_lpips_attach")
        eng.lpips_attach(1)
        assert eng.missing_weights() == (n0, names0), "pnpi_missing_weights must not count the network's slots"
        with pytest.raises(_capi.PnpiError) as e:
            eng.lpips(img[:1], img[1:2])
        msg = str(e.value)
        assert e.value.status == _capi.PNPI_ESTATE and "not loaded (57)" in msg
        assert all(w in msg for w in ("lpips.features.0.weight", "lpips.features.12.expand3x3.bias", "lpips.features.9.squeeze.weight", "lpips.lin6.weight"))
        _refused(lambda: eng.lpips_attach(1), _capi.PNPI_ESTATE, "already")
        eng.load_lpips_state_dict(sc.sd)
        _refused(lambda: eng.lpips_features(img), _capi.PNPI_EINVAL, "n out of range")                  # 3 images > 2
        _refused(lambda: eng.lpips(img[:2], img[1:3]), _capi.PNPI_EINVAL, "n out of range")             # 2 pairs > 1
        _refused(lambda: eng.lpips_features(img[:1, :16, :16]), _capi.PNPI_ESHAPE, "image side")        # 16 < 17
        with pytest.raises(ValueError):
            eng.lpips_features(img[:1, :30])                                                            # not square
        bad = masks.copy()
        bad[1, 5, 7] = 2
        m = torch.from_numpy(bad).cuda()
        ii = torch.from_numpy(img[:2]).cuda()
        p = lambda t: C.c_void_p(t.data_ptr())
        out = torch.zeros(2, 16, 16, 64, device="cuda")
        d = torch.zeros(1, device="cuda")
        assert eng.lib.pnpi_lpips_features(eng.h, p(ii), p(m), 2, S, 0, p(out)) == _capi.PNPI_EINVAL and b"0 / 1" in eng.lib.pnpi_last_error(eng.h)
        assert eng.lib.pnpi_lpips(eng.h, p(ii), None, p(ii), p(m[1:]), 1, S, p(d)) == _capi.PNPI_EINVAL and b"0 / 1" in eng.lib.pnpi_last_error(eng.h)
        assert eng.lib.pnpi_lpips_features(eng.h, p(ii), None, 1, S, 7, p(out)) == _capi.PNPI_EINVAL and b"tap" in eng.lib.pnpi_last_error(eng.h)
        assert eng.lib.pnpi_lpips_features(eng.h, p(ii), None, 1, 8193, 0, p(out)) == _capi.PNPI_ESHAPE
        f16 = torch.zeros(1, 4, 64, dtype=torch.float16, device="cuda")
        for name, a in (("pnpi_lpips_features", (p(ii), None, 1, S, 0, None)), ("pnpi_lpips", (p(ii), None, p(ii), None, 1, S, None)),
                        ("pnpi_op_lpips_layer", (p(f16), p(f16), p(out), 1, 4, 64, None)), ("pnpi_op_maxpool3s2_ceil", (p(f16), 1, 2, 64, None))):
            assert getattr(eng.lib, name)(eng.h, *a) == _capi.PNPI_EINVAL, name
            assert b"NULL" in eng.lib.pnpi_last_error(eng.h), name
        k = torch.zeros(1, 4, 12, dtype=torch.float16)
        _refused(lambda: eng.lpips_layer(k, k, torch.ones(12)), _capi.PNPI_ESHAPE, "multiple of 8")
        _refused(lambda: eng.maxpool3s2_ceil(torch.zeros(1, 4, 4, 12)), _capi.PNPI_ESHAPE, "multiple of 8")
        torch.cuda.synchronize()
        assert (out == 0).all() and (d == 0).all(), "a refused call launched something"
        got = eng.lpips(img[:1], img[2:3], masks[:1], masks[:1])        # after all the refusals the context still computes: the module network's bits
        assert torch.equal(got, sc.score(img[:1], img[2:3], masks[:1], masks[:1]))
    finally:
        eng.close()
    again = _engine()                               # attach, destroy, attach again
    try:
        again.lpips_attach(1)
        again.load_lpips_state_dict(sc.sd)
        assert torch.equal(again.lpips(img[:1], img[2:3], masks[:1], masks[:1]), got)
    finally:
        again.close()


def test_attaching_lpips_leaves_dino_and_clip_bits(sc):
    """LPIPS next to the two ViTs on one context: their outputs do not move by a bit, and LPIPS gives the module network's bits there"""
    from tests.test_clip_score_host import Fixture as ClipFx
    from tests.test_structure_distance_host import Fixture as DinoFx
    from pnpinversion_amd import weights
    dfx, cfx = DinoFx(), ClipFx()
    dcfg = _capi.DinoConfig.make(*(dfx.cfg[k] for k in ("image_size", "patch", "width", "layers", "heads", "intermediate")))
    vcfg = _capi.ClipvConfig.make(*(cfx.vcfg[k] for k in ("image_size", "patch", "width", "layers", "heads", "intermediate", "proj_dim")))
    img, _ = make_images(SEED, 34)
    out = []
    for with_lpips in (False, True):
        eng = _engine(TINY16)
        try:
            eng.load_state_dict(clip_sd=weights.clip_state_dict(TINY16, int(cfx.z["text_seed"])))
            if with_lpips:
                eng.lpips_attach(2)
                eng.load_lpips_state_dict(sc.sd)
            eng.dino_attach(dcfg, 1)
            eng.load_dino_state_dict(dfx.sd)
            eng.clipv_attach(vcfg, 3)
            eng.load_clipv_state_dict(cfx.vsd)
            if with_lpips:
                assert torch.equal(eng.lpips(img[:2], img[1:3]), sc.score(img[:2], img[1:3]))
            out.append((eng.dino_keys(dfx.images[:2]).cpu(), eng.clip_image_embed(cfx.images).cpu()))
        finally:
            eng.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---- 7. the evaluation script with seeded weights: the three LPIPS columns of two 512 x 512 images (the smallest context, built by the script)
def test_evaluate_lpips_columns_synthetic(tmp_path, monkeypatch, real_shape):
    from PIL import Image
    import csv
    import json
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    c = real_shape[0]
    src = tmp_path / "data" / "annotation_images"
    dst = tmp_path / "output" / "directinversion+p2p" / "annotation_images"
    src.mkdir(parents=True); dst.mkdir(parents=True)
    Image.fromarray(c.imgs[0]).save(src / "a.png")
    Image.fromarray(c.imgs[2]).save(dst / "a.png")
    (tmp_path / "data" / "mapping_file.json").write_text(json.dumps({"a": dict(
        image_path="a.png", mask=[512 * 100 + 50, 3000], original_prompt="a [cat]", editing_prompt="a [dog]", editing_type_id="1")}))
    monkeypatch.chdir(tmp_path)
    cols = ["lpips", "psnr_unedit_part", "lpips_unedit_part", "lpips_edit_part"]
    evaluate.run(evaluate.parse_args(["--synthetic_weights", "--metrics"] + cols + ["--tgt_methods", "1_directinversion+p2p", "--result_path", "r.csv"]))
    rows = list(csv.reader(open(tmp_path / "r.csv", newline="")))
    assert rows[0][1:] == ["1_directinversion+p2p|" + m for m in cols] and len(rows) == 2
    vals = [float(rows[1][i]) for i in (1, 3, 4)]
    assert all(np.isfinite(v) and v > 0 for v in vals) and len(set(vals)) == 3
