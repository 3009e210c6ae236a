"""Time of pnpi_clip_score at full width (ViT-L/14 image tower, 24 layers; SD-1.x text tower) on seeded weights, for the record in
DESIGN.md 7h: device events around each call on the context's stream, warmed up, median of several calls, for 1 and 8 pairs of
512 x 512 panels; the FLOPs the call executes (2 M N K of every GEMM launch from the library's counters, attention from the shapes), over the median,
as a whole-call rate and its share of the dense fp16 peak (2.5 PFLOP/s); and the numpy SSIM of pnpinversion_amd.metrics per call on
the host for comparison.  Prints one JSON line.

    python tools/clip_score_time.py [--calls 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pnpinversion_amd import metrics, weights                    # noqa: E402
from pnpinversion_amd.clip_score import ClipScore                # noqa: E402
from pnpinversion_amd.config import SD1                          # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline             # noqa: E402

PEAK_FP16 = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken elsewhere says nothing")
    pipe = NativePipeline(SD1, max_unet_rows=1, max_vae_images=1, text_encoder="native")
    pipe.engine.load_state_dict(clip_sd=weights.clip_state_dict(SD1, 0))
    scorer = ClipScore(pipe, max_images=8)
    scorer.load_synthetic(0)
    eng = pipe.engine
    g = np.random.default_rng(0)
    res = {"weights": "synthetic", "panel": 512, "calls": a.calls, "peak_fp16_flops": PEAK_FP16}
    for n in (1, 8):
        imgs = torch.from_numpy(g.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)).cuda()
        ids = scorer.tokenize(["a photo of a cat sitting on a chair %d" % i for i in range(n)]).cuda()
        for _ in range(3):
            eng.clip_score(imgs, ids)
        torch.cuda.synchronize()
        eng.reset_counters()
        eng.clip_score(imgs, ids)
        torch.cuda.synchronize()
        c = eng.counters()
        v, t = scorer.vcfg, SD1
        T = (v.image_size // v.patch) ** 2 + 1
        attn = 4.0 * n * (v.layers * v.width * T * T + t.clip_layers * t.cross_dim * t.ctx_len * t.ctx_len)      # QK^T and PV of both towers, from the shapes
        flops = c["executed_gemm_flops"] + attn
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.clip_score(imgs, ids)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        res["n%d" % n] = dict(median_ms=round(med, 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), gemm_flops=c["executed_gemm_flops"],
                              attn_flops=attn, whole_call_tflops=round(flops / med / 1e9, 1),
                              share_of_fp16_peak=round(flops / (med * 1e-3) / PEAK_FP16, 4))
    a8, b8 = g.integers(0, 256, (512, 512, 3), dtype=np.uint8), g.integers(0, 256, (512, 512, 3), dtype=np.uint8)
    keep = np.ones((512, 512, 3), np.float32)
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        metrics.calculate_ssim(a8, b8, keep, keep)
        t.append((time.perf_counter() - t0) * 1e3)
    res["numpy_ssim_ms_per_call"] = round(statistics.median(t), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
