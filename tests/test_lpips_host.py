"""LPIPS (SqueezeNet), host side (no GPU): a float64 restatement of what the reference's calculate_lpips computes
(evaluation/matrics_calculator.py:324-342 of the reference -> torchmetrics >= 1.0 LearnedPerceptualImagePatchSimilarity(net_type='squeeze')):
  1. input      x = ((u8 / 255) * mask) * 2 - 1 (a cleared pixel is -1), then the ScalingLayer (x - shift_c) / scale_c; no resize
  2. network    torchvision squeezenet1_1().features 0 .. 12: Conv 3 -> 64 (3 x 3, stride 2, no padding) + ReLU, three ceil-mode max pools,
                eight Fire blocks (squeeze 1 x 1 + ReLU, cat(ReLU(expand 1 x 1), ReLU(expand 3 x 3 pad 1)))
  3. taps       the outputs of layers 1, 4, 7, 9, 10, 11, 12 (64, 128, 256, 384, 384, 512, 512 channels)
  4. score      per tap and pixel a^ = a / sqrt(1e-8 + sum_c a_c^2), d = sum_c w_c (a^_c - b^_c)^2; the sum over the taps of mean_pixels(d)
Neither torchmetrics, lpips nor torchvision is installed: the definition above is the specification.  The restatement's own convolution
and pool are held against torch.nn.functional; the loader, evaluation/evaluate.py's CSV and the C symbols are tested here too.

tests/test_gpu_lpips.py imports the restatement (rs_*), the test pairs and the bars from here.

Bars of the fp16 device path (the float64 restatement is the truth).  The ENVELOPE is how far the restatement itself moves when its
weights and every convolution / pool output go through fp16 (`.half().double()`), measured on the CPU over the test pairs of sides 34
and 65 with seeds 3 and 4 (test_fp16_envelope prints the figures and holds the constants against them):
  tap features, max over taps and pixels of max_c |moved - exact| / max(max_c |exact|, 1e-3 max |tap|):  1.37e-3 / 1.81e-3 (seed 3, S = 34 / 65),
                                                                               1.61e-3 / 2.14e-3 (seed 4)   -> ENVELOPE_FEAT = 2.2e-3
  score, |moved - exact| / exact over the pairs with a non-zero score:         6.38e-4 / 4.93e-4 (seed 3), 5.39e-4 / 8.28e-5 (seed 4)
                                                                                                          -> ENVELOPE_SCORE = 6.5e-4
BAR_FEAT = 6.6e-3 and BAR_SCORE = 1.95e-3 are 3 x the envelope: one factor for the accumulation order of the MFMA GEMMs, one for the fp32
(device) versus float64 (restatement) score arithmetic -- the structure-distance test's convention.  A relative bar on the score means
something only where the score is far above its own movement: test_pairs_are_well_conditioned holds every non-identical test pair at
score >= 100 x the absolute movement seen."""
import csv
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_structure_distance_host import make_images  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENVELOPE_FEAT, ENVELOPE_SCORE = 2.2e-3, 6.5e-4         # measured, see the module docstring and DESIGN 7j
BAR_FEAT, BAR_SCORE = 3 * ENVELOPE_FEAT, 3 * ENVELOPE_SCORE

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
FIRES = (3, 4, 6, 7, 9, 10, 11, 12)
POOL_BEFORE = (3, 6, 9)                                # features.2, 5, 8 sit in front of these Fire blocks
TAP_AFTER = (4, 7, 9, 10, 11, 12)                      # taps 1 .. 6; tap 0 is features.1
TAP_CHANNELS = (64, 128, 256, 384, 384, 512, 512)
NEW_SYMBOLS = ("pnpi_lpips_attach", "pnpi_lpips", "pnpi_lpips_features", "pnpi_op_lpips_layer", "pnpi_op_maxpool3s2_ceil")
SEED = 3
# test pairs: (pred image, gt image, mask index or None for both sides, complement?) on make_images(SEED, S).  Image 1 is image 0 with a
# disc painted over and mask 1 covers the disc: pair 5 is identical after masking with the complement.
PAIRS = [(0, 1, None, False), (0, 2, 1, True), (0, 2, 1, False), (0, 2, None, False), (2, 1, 0, False), (0, 1, 1, True), (1, 1, None, False)]
ZERO_PAIRS = (5, 6)


def pair_inputs(imgs, masks, p):
    a, b, m, comp = p
    mk = None if m is None else ((1 - masks[m]) if comp else masks[m])
    return imgs[a], imgs[b], mk, mk


# ------------------------------------------------------------------------------------------------------------------ restatement
_ident = lambda t: t
rs_fp16 = lambda t: t.half().double()


def rs_input(img_u8, mask=None):
    """uint8 [S, S, 3] (* 0 / 1 mask [S, S]) -> float64 torch [1, 3, S, S]: ((u8 / 255) * mask) * 2 - 1, then (x - shift) / scale"""
    x = img_u8.astype(np.float64) / 255.0
    if mask is not None:
        x = x * np.asarray(mask, np.float64)[:, :, None]
    x = (x * 2.0 - 1.0 - np.array(SHIFT)) / np.array(SCALE)
    return torch.from_numpy(x.transpose(2, 0, 1)[None].copy())


def rs_conv1(x, w, b):
    """Conv2d(3, 64, 3, stride 2, no padding) written out: nine strided slices, each a [64, 3] x [3, Ho, Ho] product"""
    S = x.shape[-1]
    Ho = (S - 3) // 2 + 1
    out = b[None, :, None, None].expand(x.shape[0], -1, Ho, Ho).clone()
    for ky in range(3):
        for kx in range(3):
            out = out + torch.einsum("oc,bcyx->boyx", w[:, :, ky, kx], x[:, :, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Ho - 1:2])
    return out


def rs_pool_out(H):
    """MaxPool2d(3, stride 2, ceil_mode=True): ceil((H - 3) / 2) + 1 windows, one less if the last would start outside the input"""
    Ho = -((H - 3) // -2) + 1
    return Ho - 1 if (Ho - 1) * 2 >= H else Ho


def rs_pool(x):
    """[B, C, H, H] -> [B, C, Ho, Ho]: every window clipped to the input"""
    H = x.shape[-1]
    Ho = rs_pool_out(H)
    rows = [torch.stack([x[:, :, 2 * i:min(2 * i + 3, H), 2 * j:min(2 * j + 3, H)].amax((-2, -1)) for j in range(Ho)], -1) for i in range(Ho)]
    return torch.stack(rows, -2)


def rs_fire(x, sd, pre, rnd):
    P = lambda k: rnd(sd[pre + k].double())
    s = torch.relu(rnd(F.conv2d(x, P(".squeeze.weight"), P(".squeeze.bias"))))
    e1 = rnd(F.conv2d(s, P(".expand1x1.weight"), P(".expand1x1.bias")))
    e3 = rnd(F.conv2d(s, P(".expand3x3.weight"), P(".expand3x3.bias"), padding=1))
    return torch.relu(torch.cat([e1, e3], 1))


def rs_taps(sd, x, rnd=_ident, pool=rs_pool):
    """x [B, 3, S, S] (rs_input) -> the seven tap maps [B, C_k, H_k, H_k]; rnd rounds the weights and every convolution / pool output"""
    h = torch.relu(rnd(rs_conv1(x, rnd(sd["features.0.weight"].double()), rnd(sd["features.0.bias"].double()))))
    taps = [h]
    for idx in FIRES:
        if idx in POOL_BEFORE:
            h = rnd(pool(h))
        h = rs_fire(h, sd, "features.%d" % idx, rnd)
        if idx in TAP_AFTER:
            taps.append(h)
    return taps


def rs_tap_term(a, b, w):
    """[C, H, H] x 2, w [C] -> the tap's term: mean over the pixels of sum_c w_c (a^_c - b^_c)^2"""
    an = a / torch.sqrt(1e-8 + (a * a).sum(0, keepdim=True))
    bn = b / torch.sqrt(1e-8 + (b * b).sum(0, keepdim=True))
    return float((w[:, None, None] * (an - bn) ** 2).sum(0).mean())


def rs_score(sd, taps_a, taps_b):
    return sum(rs_tap_term(a[0], b[0], sd["lin%d.weight" % k].double().reshape(-1)) for k, (a, b) in enumerate(zip(taps_a, taps_b)))


def feat_err(got, ref):
    """[C, H, H] each -> max over the pixels of max_c |got - ref| / max(max_c |ref|, 1e-3 max |ref|): relative to each pixel's largest
    magnitude, with a floor so that an all-but-dead pixel does not set the scale"""
    den = torch.clamp(ref.abs().amax(0), min=1e-3 * float(ref.abs().max()))
    return float(((got - ref).abs().amax(0) / den).max())


class Case:
    """the seeded weights, the test images of one side and the restated taps / scores of every test pair, exact or fp16-rounded"""

    def __init__(self, S, seed=SEED):
        from pnpinversion_amd import weights
        self.S, self.seed = S, seed
        self.sd = weights.lpips_state_dict(seed)
        self.imgs, self.masks = make_images(seed, S)
        self._memo = {}

    def taps(self, img, mask, rnd=_ident):
        key = (img, None if mask is None else bytes(mask), rnd is _ident)
        if key not in self._memo:
            self._memo[key] = rs_taps(self.sd, rs_input(self.imgs[img], mask), rnd)
        return self._memo[key]

    def scores(self, rnd=_ident):
        out = []
        for p in PAIRS:
            _, _, ma, mb = pair_inputs(self.imgs, self.masks, p)
            out.append(rs_score(self.sd, self.taps(p[0], ma, rnd), self.taps(p[1], mb, rnd)))
        return np.array(out)


_cases = {}


def case(S, seed=SEED):
    if (S, seed) not in _cases:
        _cases[(S, seed)] = Case(S, seed)
    return _cases[(S, seed)]


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("H", [2, 3, 4, 7, 8, 15, 16, 31, 127])
def test_pool_restatement_against_torch(H):
    g = torch.Generator().manual_seed(H)
    x = torch.randn(2, 5, H, H, generator=g, dtype=torch.float64)
    ref = F.max_pool2d(x, 3, 2, ceil_mode=True)
    got = rs_pool(x)
    assert got.shape == ref.shape and rs_pool_out(H) == ref.shape[-1] and bool((got == ref).all())


def test_pool_sizes_of_the_real_shape_and_the_smallest():
    """512 x 512: 255, 127, 63, 31 with no overhanging window; 17 is the smallest side whose third pool has a window"""
    h = [(512 - 3) // 2 + 1]
    for _ in range(3):
        assert (h[-1] - 3) % 2 == 0
        h.append(rs_pool_out(h[-1]))
    assert h == [255, 127, 63, 31]
    sides = lambda S: [rs_pool_out(rs_pool_out((S - 3) // 2 + 1))]
    assert sides(17) == [2] and rs_pool_out(2) == 1 and sides(16) == [1]
    with pytest.raises(RuntimeError):
        F.max_pool2d(torch.zeros(1, 1, 1, 1), 3, 2, ceil_mode=True)


@pytest.mark.parametrize("S", [17, 32, 65])
def test_conv1_restatement_against_torch(S):
    g = torch.Generator().manual_seed(S)
    x = torch.randn(2, 3, S, S, generator=g, dtype=torch.float64)
    w, b = torch.randn(64, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    ref = F.conv2d(x, w, b, stride=2)
    got = rs_conv1(x, w, b)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_masked_pixel_is_minus_one_before_scaling():
    img = np.full((4, 4, 3), 200, np.uint8)
    mask = np.ones((4, 4), np.uint8)
    mask[1, 2] = 0
    x = rs_input(img, mask)[0]
    for c in range(3):
        assert float(x[c, 1, 2]) == (-1.0 - SHIFT[c]) / SCALE[c]                       # -1, not 0, goes through the ScalingLayer
        assert abs(float(x[c, 0, 0]) - ((200 / 255 * 2 - 1) - SHIFT[c]) / SCALE[c]) < 1e-15
    assert float(rs_input(np.zeros((4, 4, 3), np.uint8))[0, 0, 0, 0]) == (-1.0 - SHIFT[0]) / SCALE[0]   # and so does a black pixel


def _envelope(c):
    ef = 0.0
    for i in range(3):
        for m in (None, c.masks[1]):
            ef = max(ef, max(feat_err(a[0], b[0]) for a, b in zip(c.taps(i, m, rs_fp16), c.taps(i, m))))
    s, s16 = c.scores(), c.scores(rs_fp16)
    nz = s > 0
    return ef, float((np.abs(s16 - s)[nz] / s[nz]).max()), s, s16


def test_fp16_envelope():
    worst_f = worst_s = 0.0
    for seed in (3, 4):
        for S in (34, 65):
            ef, es, _, _ = _envelope(case(S, seed))
            print("seed %d, S = %d: feature envelope %.2e, score envelope %.2e" % (seed, S, ef, es))
            worst_f, worst_s = max(worst_f, ef), max(worst_s, es)
    assert worst_f <= ENVELOPE_FEAT and worst_s <= ENVELOPE_SCORE
    assert worst_f >= 0.5 * ENVELOPE_FEAT and worst_s >= 0.5 * ENVELOPE_SCORE, "the constants are far above what was measured: re-measure"


@pytest.mark.parametrize("S", [34, 65])
def test_pairs_are_well_conditioned(S):
    """every non-identical test pair's restated score is at least 100 x the absolute movement under fp16 rounding; the identical ones give 0"""
    _, _, s, s16 = _envelope(case(S))
    for i, (p, d, d16) in enumerate(zip(PAIRS, s, s16)):
        print("S = %d pair %s: score %.4e, moved by %.2e" % (S, p, d, abs(d16 - d)))
        if i in ZERO_PAIRS:
            assert d == 0.0 and d16 == 0.0, p
        else:
            assert d >= 100 * abs(d16 - d) and d > 1e-3, p


def test_activations_neither_die_nor_overflow():
    """the seeded network on a test image and on the all-255 / all-0 images: every tap keeps a usable share of live channels and stays far
    inside fp16's range"""
    c = case(65)
    for x in (rs_input(c.imgs[0]), rs_input(np.full((65, 65, 3), 255, np.uint8)), rs_input(np.zeros((65, 65, 3), np.uint8))):
        for k, t in enumerate(rs_taps(c.sd, x)):
            assert t.shape[1] == TAP_CHANNELS[k]
            assert float((t > 0).double().mean()) > 0.2 and 0.05 < float(t.abs().max()) < 1000, k


def test_bar_can_fail():
    """mistakes the issue warns of move the result by more than the bars: a cleared pixel taken as 0 instead of -1; floor-mode pools"""
    c = case(65)
    m = c.masks[1]
    ref = c.taps(0, m)
    x0 = rs_input(c.imgs[0])
    keep = torch.from_numpy(np.asarray(m, np.float64))[None, None]
    zero = (0.0 - torch.tensor(SHIFT, dtype=torch.float64)) / torch.tensor(SCALE, dtype=torch.float64)
    wrong = rs_taps(c.sd, x0 * keep + (1 - keep) * zero[None, :, None, None])
    e = max(feat_err(a[0], b[0]) for a, b in zip(wrong, ref))
    print("cleared pixel = 0: features move by %.3f (bar %.1e)" % (e, BAR_FEAT))
    assert e > BAR_FEAT
    floor = rs_taps(c.sd, rs_input(c.imgs[0], m), pool=lambda t: F.max_pool2d(t, 3, 2))
    assert floor[1].shape[-1] != ref[1].shape[-1]                                  # 65 -> 32 -> 16 (ceil) but 15 (floor): an overhanging window
    s0 = rs_score(c.sd, c.taps(0, None), c.taps(2, None))
    s1 = rs_score(c.sd, rs_taps(c.sd, x0, pool=lambda t: F.max_pool2d(t, 3, 2)), rs_taps(c.sd, rs_input(c.imgs[2]), pool=lambda t: F.max_pool2d(t, 3, 2)))
    print("floor-mode pools: score moves by %.3f relative (bar %.1e)" % (abs(s1 - s0) / s0, BAR_SCORE))
    assert abs(s1 - s0) / s0 > BAR_SCORE


def test_new_symbols_everywhere():
    from pnpinversion_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "pnpi.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _capi.load_library()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _capi.SYMBOLS and hasattr(lib, s) and s in doc, s


def test_seeded_weights():
    from pnpinversion_amd import checkpoint, weights
    sd = weights.lpips_state_dict(5)
    assert sorted(sd) == sorted(checkpoint.lpips_keys()) and len(sd) == 2 + 8 * 6 + 7
    assert all(bool((v == v.half().float()).all()) for v in sd.values())
    assert tuple(sd["features.0.weight"].shape) == (64, 3, 3, 3) and tuple(sd["features.9.expand3x3.weight"].shape) == (192, 48, 3, 3)
    for k, ch in enumerate(TAP_CHANNELS):
        w = sd["lin%d.weight" % k]
        assert tuple(w.shape) == (1, ch, 1, 1) and float(w.min()) >= 0.0
    assert any(not torch.equal(sd[k], weights.lpips_state_dict(6)[k]) for k in sd)


def test_checkpoint_loader_key_mapping(tmp_path):
    """torchvision's squeezenet1_1 file (classifier.* ignored) + the lpips package's squeeze.pth (lin{k}.model.1.weight), on stand-ins"""
    from pnpinversion_amd import checkpoint, weights
    sd = weights.lpips_state_dict(7)
    net = {k: v for k, v in sd.items() if k.startswith("features.")}
    net["classifier.1.weight"], net["classifier.1.bias"] = torch.zeros(1000, 512, 1, 1), torch.zeros(1000)
    lin = {"lin%d.model.1.weight" % k: sd["lin%d.weight" % k] for k in range(7)}
    torch.save(net, tmp_path / "net.pth")
    torch.save(lin, tmp_path / "lin.pth")
    got = checkpoint.load_lpips_checkpoint(str(tmp_path / "net.pth"), str(tmp_path / "lin.pth"))
    assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    bad_net = dict(net)
    del bad_net["features.7.expand3x3.bias"]
    bad_net["features.13.weight"] = torch.zeros(1)
    bad_lin = dict(lin)
    del bad_lin["lin4.model.1.weight"]
    bad_lin["lin4.model.0.weight"] = torch.zeros(1)
    torch.save(bad_net, tmp_path / "bad_net.pth")
    torch.save(bad_lin, tmp_path / "bad_lin.pth")
    with pytest.raises(KeyError) as e:
        checkpoint.load_lpips_checkpoint(str(tmp_path / "bad_net.pth"), str(tmp_path / "bad_lin.pth"))
    for name in ("features.13.weight", "lin4.model.0.weight", "features.7.expand3x3.bias", "lin4.weight"):
        assert name in str(e.value), name
    assert "classifier" not in str(e.value)


# ------------------------------------------------------------------------------------------------------------------ evaluate.py
class _StubLpips:
    def __init__(self):
        self.calls = []

    def score(self, pred, gt, mask_pred=None, mask_gt=None):
        self.calls.append((len(pred), [None if m is None else float(np.asarray(m).mean()) for m in mask_pred],
                           [np.asarray(p).shape for p in pred], [np.asarray(p).shape for p in gt],
                           [float(np.asarray(p).mean()) for p in pred], [float(np.asarray(p).mean()) for p in gt]))
        return torch.arange(len(pred), dtype=torch.float32) + 0.25


def _bench_dir(tmp_path):
    from PIL import Image
    import json
    g = np.random.default_rng(0)
    src = tmp_path / "data" / "annotation_images"
    out = tmp_path / "output" / "directinversion+p2p" / "annotation_images"
    src.mkdir(parents=True); out.mkdir(parents=True)
    mapping = {}
    for key, mask in (("000000000000", [512 * 100 + 50, 300]), ("000000000001", [0, 512 * 512])):      # the second mask covers everything
        Image.fromarray(g.integers(0, 100, (512, 512, 3), dtype=np.uint8)).save(src / (key + ".png"))
        panel = g.integers(0, 100, (512, 2048, 3), dtype=np.uint8)
        panel[:, -512:] += 150                                                                         # the right-hand panel is the bright one
        Image.fromarray(panel).save(out / (key + ".png"))
        mapping[key] = dict(image_path=key + ".png", mask=mask, original_prompt="a [cat]", editing_prompt="a [dog]", editing_type_id="1")
    (tmp_path / "data" / "mapping_file.json").write_text(json.dumps(mapping))
    return tmp_path


def test_evaluate_lpips_columns(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    d = _bench_dir(tmp_path)
    monkeypatch.chdir(d)
    metrics = ["lpips", "psnr_unedit_part", "lpips_unedit_part", "lpips_edit_part"]
    stub = _StubLpips()
    evaluate.run(evaluate.parse_args(["--metrics"] + metrics + ["--tgt_methods", "1_directinversion+p2p", "--result_path", "r.csv"]), lpips_scorer=stub)
    rows = list(csv.reader(open(d / "r.csv", newline="")))
    assert rows[0] == ["file_id"] + ["1_directinversion+p2p|" + m for m in metrics]
    # image 0: the three columns arrive in ONE call -- whole (no mask), unedited part (1 - mask), edited part (mask)
    assert len(stub.calls) == 2 and stub.calls[0][0] == 3
    assert stub.calls[0][1][0] is None and stub.calls[0][1][1] > 0.9 and stub.calls[0][1][2] < 0.1
    assert all(s == (512, 512, 3) for s in stub.calls[0][2] + stub.calls[0][3])
    assert all(v < 60 for v in stub.calls[0][4]) and all(v > 190 for v in stub.calls[0][5])          # (src, tgt) order; the right-hand 512 crop
    assert [rows[1][1], rows[1][3], rows[1][4]] == ["0.25", "1.25", "2.25"]
    # image 1: its mask covers the whole image, so the unedited part is empty: "nan" there, and only two pairs reach the device
    assert stub.calls[1][0] == 2 and rows[2][3] == "nan" and rows[2][2] == "nan" and [rows[2][1], rows[2][4]] == ["0.25", "1.25"]
    # single cells through the Calculator protocol, the reference's "nan" rule
    calc = evaluate.Calculator(None, None, stub)
    ones, zeros = np.ones((4, 4, 3)), np.zeros((4, 4, 3))
    img = np.zeros((4, 4, 3), np.uint8)
    assert evaluate.calculate_metric(calc, "lpips_unedit_part", img, img, ones, ones, "", "") == "nan"
    assert evaluate.calculate_metric(calc, "lpips_edit_part", img, img, zeros, zeros, "", "") == "nan"
    assert evaluate.calculate_metric(calc, "lpips", img, img, zeros, zeros, "", "") == 0.25
    assert evaluate.Calculator(None, None).lpips_scorer is None
    with pytest.raises(SystemExit):                                                                   # no scorer in the calculator: refused by name
        evaluate.calculate_metric(evaluate.Calculator(None, None), "lpips", img, img, zeros, zeros, "", "")


def test_evaluate_default_metrics_with_stubs(tmp_path, monkeypatch):
    """the default metric list writes a CSV once every scorer is there"""
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    d = _bench_dir(tmp_path)
    monkeypatch.chdir(d)

    class Clip:
        def score(self, imgs, prompts, masks=None):
            return torch.full((len(imgs),), 20.0)

    class Struct:
        def distance(self, pred, gt, mp=None, mg=None):
            return torch.full((len(pred),), 0.5)

    evaluate.run(evaluate.parse_args(["--tgt_methods", "1_directinversion+p2p", "--result_path", "r.csv"]), scorer=Clip(), struct_scorer=Struct(),
                 lpips_scorer=_StubLpips())
    rows = list(csv.reader(open(d / "r.csv", newline="")))
    assert rows[0][1:] == ["1_directinversion+p2p|" + m for m in evaluate.DEFAULT_METRICS] and len(rows) == 3
    assert rows[1][1 + evaluate.DEFAULT_METRICS.index("lpips_unedit_part")] == "0.25"


@pytest.mark.parametrize("metric", ["lpips", "lpips_unedit_part", "lpips_edit_part"])
def test_evaluate_refusals(metric):
    """without LPIPS weights the column is refused by name before any file is opened; DINO weights alone do not help"""
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    for extra in ([], ["--dino_checkpoint", "/nonexistent.pth"], ["--squeezenet_checkpoint", "/nonexistent.pth"], ["--lpips_checkpoint", "/nonexistent.pth"]):
        with pytest.raises(SystemExit) as e:
            evaluate.run(evaluate.parse_args(["--metrics", "psnr", metric, "--annotation_mapping_file", "/nonexistent.json"] + extra))
        assert isinstance(e.value.code, str) and repr(metric) in e.value.code and "not built" in e.value.code and "LPIPS" in e.value.code
    evaluate.check_metrics(["psnr", metric], lpips=True)                                   # computable once weights are named
    with pytest.raises(SystemExit):
        evaluate.check_metrics(["psnr", metric], dino=True)
    assert evaluate.has_lpips_weights(evaluate.parse_args(["--squeezenet_checkpoint", "a.pth", "--lpips_checkpoint", "b.pth"]))
    assert evaluate.has_lpips_weights(evaluate.parse_args(["--synthetic_weights"]))
    assert not evaluate.has_lpips_weights(evaluate.parse_args(["--squeezenet_checkpoint", "a.pth"]))
    assert metric in evaluate.LPIPS_METRICS and "lpips_unedit_part" in evaluate.DEFAULT_METRICS


def test_default_metrics_pass_once_weights_are_named():
    sys.path.insert(0, ROOT)
    from evaluation import evaluate
    evaluate.check_metrics(evaluate.DEFAULT_METRICS, dino=True, lpips=True)
    a = evaluate.parse_args(["--synthetic_weights"])
    evaluate.check_metrics(a.metrics, dino=evaluate.has_dino_weights(a), lpips=evaluate.has_lpips_weights(a))
    with pytest.raises(SystemExit) as e:
        evaluate.check_metrics(evaluate.DEFAULT_METRICS, dino=True)
    assert repr("lpips_unedit_part") in e.value.code
    with pytest.raises(SystemExit, match="unknown metric column"):
        evaluate.check_metrics(["lpips_part"], dino=True, lpips=True)


def test_metrics_calculate_lpips_masks():
    """[S, S] and [S, S, 3] masks reach the scorer as given; shapes must agree"""
    from pnpinversion_amd import metrics
    stub = _StubLpips()
    img = np.zeros((8, 8, 3), np.uint8)
    m2 = np.zeros((8, 8)); m2[:4] = 1
    assert metrics.calculate_lpips(img, img, m2, m2, scorer=stub) == 0.25
    assert metrics.calculate_lpips(img, img, m2[:, :, None].repeat(3, 2), None, scorer=stub) == 0.25
    assert stub.calls[0][1] == [0.5] and stub.calls[1][1] == [0.5]
    with pytest.raises(ValueError):
        metrics.calculate_lpips(img, np.zeros((9, 9, 3), np.uint8), scorer=stub)
