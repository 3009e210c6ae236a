"""Time one whole InstructPix2Pix edit loop (pnpi_ip2p_edit, 50 steps, one image, SD1_IP2P width, synthetic weights) with the compact
text-independent prefix (tuning "cfg_dedup" = 1, the default) and without it (0): wall clock around a device synchronise after a warm-up,
the two settings interleaved.  Text encoding, VAE and host table are outside the timed region.

    python tools/ip2p_ab.py [--runs 4] [--steps 50] [--out profiles/ip2p_ab.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pnpinversion_amd import instructpix2pix as ip  # noqa: E402
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SD1_IP2P  # noqa: E402
from pnpinversion_amd.engine import NativeEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "ip2p_ab.json"))
    args = ap.parse_args()
    cfg = SD1_IP2P
    eng = NativeEngine(cfg, max_unet_rows=3, max_vae_images=1)
    eng.load_state_dict(weights.unet_state_dict(cfg, 0), weights.vae_state_dict(cfg, 0))
    S = cfg.sample_size
    g = torch.Generator().manual_seed(0)
    sched = ip.SigmaSchedule()
    sigmas = sched.get_sigmas(args.steps)
    tab = ip.step_table(sigmas, sched)
    ctx = weights.synth_context(cfg, 2, seed=1)
    a = [x.to(eng.device) for x in (torch.randn(1, 4, S, S, generator=g) * sigmas[0], torch.randn(1, 4, S, S, generator=g),
                                    torch.randn(args.steps, 1, 4, S, S, generator=g), torch.stack([ctx[0], ctx[1], ctx[1]])[None])]

    def run(mode):
        assert eng.lib.pnpi_set_tuning(b"cfg_dedup", mode) == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.ip2p_edit(a[0], a[1], a[2], a[3], tab)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for mode in (1, 0):
        run(mode)                                                   # warm-up of both settings
    times, outs = {1: [], 0: []}, {}
    for _ in range(args.runs):
        for mode in (1, 0):
            dt, outs[mode] = run(mode)
            times[mode].append(dt)
    eng.lib.pnpi_set_tuning(b"cfg_dedup", 1)
    c = eng.counters()
    res = {"what": "pnpi_ip2p_edit, one image, %d steps, SD1_IP2P width, synthetic weights; seconds of wall clock around a device "
                   "synchronise, after one warm-up run of each setting, settings interleaved" % args.steps,
           "device": torch.cuda.get_device_name(0), "arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None), "steps": args.steps, "runs": args.runs,
           "cfg_dedup_1_s": times[1], "cfg_dedup_0_s": times[0],
           "cfg_dedup_1_median_s": sorted(times[1])[len(times[1]) // 2], "cfg_dedup_0_median_s": sorted(times[0])[len(times[0]) // 2],
           "rel_l2_between_settings": ((outs[1] - outs[0]).norm() / outs[0].norm()).item(),
           "finite": bool(torch.isfinite(outs[1]).all()),
           "not_timed": "text encoding, VAE encode / decode, the host scalar table, image files; more than one image per call"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
