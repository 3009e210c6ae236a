"""Time of pnpi_lpips (SqueezeNet 1.1 features + the seven fused tap distances) on seeded weights, for the record in DESIGN.md 7j:
device events around each call on the context's stream, warmed up, median of several calls, for 1 and max_pairs pairs of 512 x 512 panels:
  ms per pair of the whole call;
  the network's share (pnpi_lpips_features over the same 2 n images, last tap) against the fused distance's (pnpi_op_lpips_layer on the
  seven taps' shapes);
  the time of the float64 CPU restatement of the tests for one pair (host clock).
One process, no child processes; prints one JSON line and writes it to --out.

    python tools/time_lpips.py [--calls 20] [--max_pairs 4] [--out profiles/lpips.json]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pnpinversion_amd.config import TINY16                                   # noqa: E402
from pnpinversion_amd.engine import NativeEngine                             # noqa: E402
from pnpinversion_amd.lpips import Lpips                                     # noqa: E402


def timed(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--max_pairs", type=int, default=4)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: a time taken elsewhere says nothing")
    eng = NativeEngine(dataclasses.replace(TINY16, clip_layers=0), max_unet_rows=0, max_vae_images=0)
    sc = Lpips(eng, max_pairs=a.max_pairs)
    sd = sc.load_synthetic(0)
    g = np.random.default_rng(0)
    clk = eng.clock_probe(20000)      # (GHz the matrix pipe holds under back-to-back MFMAs, probe ms): the clock the times below were taken at
    res = {"weights": "synthetic", "model": "squeezenet1_1 features 0..12 + 7 lin", "panel": 512, "calls": a.calls, "max_pairs": a.max_pairs, "clock": clk}
    for n in sorted({1, a.max_pairs}):
        pred = torch.from_numpy(g.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)).cuda()
        gt = torch.from_numpy(g.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)).cuda()
        both = torch.cat([pred, gt])
        taps = [eng.lpips_features(both, None, k).half().flatten(1, 2) for k in range(7)]
        lins = [sd["lin%d.weight" % k].reshape(-1).cuda() for k in range(7)]
        whole = timed(lambda: eng.lpips(pred, gt), a.calls)
        net = timed(lambda: eng.lpips_features(both, None, 6), a.calls)
        dist = timed(lambda: [eng.lpips_layer(t[:n], t[n:], w) for t, w in zip(taps, lins)], a.calls)
        res["n%d" % n] = dict(whole_call=whole, ms_per_pair=round(whole["median_ms"] / n, 4), network=net, fused_distance_7_taps=dist,
                              network_share=round(net["median_ms"] / whole["median_ms"], 4),
                              distance_share=round(dist["median_ms"] / whole["median_ms"], 4))
    eng.close()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_lpips_host import rs_input, rs_score, rs_taps
    img = g.integers(0, 256, (2, 512, 512, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    rs_score(sd, rs_taps(sd, rs_input(img[0])), rs_taps(sd, rs_input(img[1])))
    res["cpu_float64_restatement_one_pair_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
