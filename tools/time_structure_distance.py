"""Time of pnpi_structure_distance at full size (DINO ViT-B/8, 12 layers: T = 785, D = 768) on seeded weights, for the record in
DESIGN.md 7i: device events around each call on the context's stream, warmed up, median of several calls, for 1 and max_pairs pairs of
512 x 512 panels:
  ms per pair of the whole call;
  the tower's share (pnpi_dino_keys over the same 2 n images) against the fused distance kernel's (pnpi_op_keys_selfsim_mse on the keys);
  the fused kernel against the unfused composition: its own debug-map variant once per input (two T x T fp32 maps written) plus a
  difference reduction over them (torch).
One process, no child processes; prints one JSON line and writes it to --out.

    python tools/time_structure_distance.py [--calls 20] [--max_pairs 4] [--out profiles/structure_distance.json]"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pnpinversion_amd.config import TINY16                                   # noqa: E402
from pnpinversion_amd.engine import NativeEngine                             # noqa: E402
from pnpinversion_amd.structure_distance import StructureDistance            # noqa: E402


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
    sc = StructureDistance(eng, max_pairs=a.max_pairs)
    sc.load_synthetic(0)
    g = np.random.default_rng(0)
    clk = eng.clock_probe(20000)      # (GHz the matrix pipe holds under back-to-back MFMAs, probe ms): the clock the times below were taken at
    res = {"weights": "synthetic", "model": "ViT-B/8, 12 layers", "panel": 512, "calls": a.calls, "max_pairs": a.max_pairs, "clock": clk}
    for n in sorted({1, a.max_pairs}):
        pred = torch.from_numpy(g.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)).cuda()
        gt = torch.from_numpy(g.integers(0, 256, (n, 512, 512, 3), dtype=np.uint8)).cuda()
        both = torch.cat([pred, gt])
        keys = eng.dino_keys(both).half()
        ka, kb = keys[:n].contiguous(), keys[n:].contiguous()
        whole = timed(lambda: eng.structure_distance(pred, gt), a.calls)
        tower = timed(lambda: eng.dino_keys(both), a.calls)
        fused = timed(lambda: eng.keys_selfsim_mse(ka, kb), a.calls)

        def unfused():
            _, sa = eng.keys_selfsim_mse(ka, ka, want_map=True)
            _, sb = eng.keys_selfsim_mse(kb, kb, want_map=True)
            return ((sa - sb) ** 2).mean((1, 2))

        # want_map also runs the fused launch set: take it out again (measured just above) to leave the two map launches + the reduction
        unf = timed(unfused, a.calls)
        d_f = eng.keys_selfsim_mse(ka, kb)[0]
        d_u = unfused()
        res["n%d" % n] = dict(whole_call=whole, ms_per_pair=round(whole["median_ms"] / n, 4), tower=tower, fused_distance=fused,
                              unfused_maps_plus_reduction=dict(unf, median_ms_less_fused=round(unf["median_ms"] - 2 * fused["median_ms"], 4)),
                              tower_share=round(tower["median_ms"] / whole["median_ms"], 4),
                              fused_share=round(fused["median_ms"] / whole["median_ms"], 4),
                              fused_vs_unfused_max_rel_diff=float(((d_f - d_u).abs() / d_u.abs().clamp(min=1e-30)).max()))
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
