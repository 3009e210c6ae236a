"""Records which kernel instance launch_igemm runs over a sweep of tile ids, tuning knobs, occupancies and K -> tests/golden/igemm_instances.json,
which tests/test_igemm_instances_host.py replays through pnpi_igemm_plan_query.  Host only: no GPU is needed.

The recording was made at the commit before the instance table (kInstances, csrc/gemm.hip): the plan came from that commit's library and the
instance name from instance_of() below, that commit's igemm_dispatch switch written out as its test file had it.  The plan query now names
the instance itself; instance_of() works from the plan's other fields only, so running this script again must reproduce the file byte for
byte -- the two ways to the name are held against each other.

    python tools/make_igemm_instance_golden.py [output path]

Sweep.  Per tile id 0, 1, 3 ... 20 (force_cfg) at N = BN and M = 200 / 300 / 600 BM + 2 rows (201 / 301 / 601 tile units: sparse 2 / 1 / 0 under
deep rings): K = 320 under igemm_deep_rings x igemm_dma in {0, 1}^2 and, where the tile has a variant knob, every value its rules name plus
one they do not (7); K = 72 (the generic register-staged kernels) under the defaults.  Tile 0 under v128_bk64_tiles = 1 and 300 (below and
above 301 units).  The ping-pong tiles under igemm_vpp = 1: a product library refuses the value at pnpi_set_tuning (the record holds the
refusal), an ablation library plans with it.  The table / cost-model path (force_cfg = -1) on the shapes of test_gemm_bound_host.CASES, with
deep rings on and off."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pnpinversion_amd import _capi  # noqa: E402
from tests.test_gemm_bound_host import CASES, query_plan  # noqa: E402

TILES = {0: (128, 128), 1: (64, 64), 3: (256, 128), 4: (128, 320), 5: (128, 256), 6: (256, 320), 7: (256, 256), 8: (64, 64), 9: (128, 128),
         10: (128, 128), 11: (64, 64), 12: (64, 320), 13: (128, 128), 14: (128, 128), 15: (128, 256), 16: (256, 256), 17: (192, 320),
         18: (128, 128), 19: (128, 320), 20: (192, 256)}
KNOBS = {0: ("igemm_v128", (0, 1, 2, 3, 4, 8, 7)), 1: ("igemm_v64", (0, 1, 2, 3, 8, 7)), 3: ("igemm_v256", (0, 1)), 4: ("igemm_v320", (0, 1, 2, 3)),
         5: ("igemm_v256n", (0, 1, 2, 3)), 16: ("igemm_vpp", (0, 1)), 17: ("igemm_vpp", (0, 1)), 19: ("igemm_vpp", (0, 1)), 20: ("igemm_vpp", (0, 1))}
UNITS = (200, 300, 600)
_ONE_INSTANCE = {6: "dma<256,320,64,2,wgm4>", 7: "dma<256,256,64,2,wgm4>", 8: "dma<64,64,64,2,kg4>", 9: "dma<128,128,32,3,kg2>",
                 10: "dma<128,128,64,2,kg2>", 11: "dma<64,64,64,2,kg2>", 12: "dma<64,320,32,2>", 13: "dma<128,128,32,2>",
                 14: "dma<128,128,64,2>", 15: "dma<128,256,64,2>", 16: "pp<256,256>", 17: "pp<192,320>", 18: "dma<128,128,64,3>",
                 19: "pp<128,320>", 20: "pp<192,256>"}


def instance_of(pl):
    """the kernel instance a product library launches for a plan, from the fields id, variant, sparse, dma, fastk, bm of pnpi_igemm_plan"""
    if not pl.dma:
        return "v1<%s,%s>" % ("64,64" if pl.bm == 64 else "128,128", "fast" if pl.fastk else "generic")
    if pl.id in _ONE_INSTANCE:
        return _ONE_INSTANCE[pl.id]
    if pl.id == 0:
        return "dma<128,128,%s>" % {1: "64,3", 2: "32,3", 3: "32,4", 4: "32,2", 8: "32,8"}.get(pl.variant, "64,2")
    if pl.id == 1:
        return "dma<64,64,%s>" % {8: "64,8", 1: "64,2", 2: "64,4", 3: "32,4"}.get(pl.variant, "64,3")
    if pl.id == 3:
        return "dma<256,128,32,2>" if pl.variant == 1 else "dma<256,128,32,3>"
    if pl.id in (4, 5):
        bn, deep = (320, 5) if pl.id == 4 else (256, 6)
        if pl.sparse == 2 and pl.variant == 1:
            return "dma<128,%d,32,%d>" % (bn, deep)
        return "dma<128,%d,%s>" % (bn, {0: "32,3", 2: "64,2"}.get(pl.variant, "32,2"))
    raise ValueError("no instance for tile id %d" % pl.id)


def record(lib, M, N, K, cfg, tune):
    """one launch description under `tune` -> a record; a knob value the library refuses is recorded as refused, and nothing is planned"""
    rec = {"M": M, "N": N, "K": K, "cfg": cfg, "tune": tune}
    try:
        with _capi.tuning(lib, **tune):
            pl = query_plan(lib, M, N, K, cfg=cfg, bias="a16")
    except ValueError:
        rec["refused"] = True
        return rec
    rec["plan"] = [pl.err, pl.id, pl.variant, pl.sparse, pl.split, pl.gx, pl.gy, pl.gz]
    rec["instance"] = instance_of(pl) if pl.err == 0 else None
    return rec


def sweep(lib):
    recs = []
    for cfg, (bm, bn) in TILES.items():
        knob, values = KNOBS.get(cfg, (None, (None,)))
        for units in UNITS:
            M = units * bm + 2
            for v in values:
                for deep in (1, 0):
                    for dma in (1, 0):
                        tune = {"igemm_deep_rings": deep, "igemm_dma": dma}
                        if knob:
                            tune[knob] = v
                        recs.append(record(lib, M, bn, 320, cfg, tune))
            recs.append(record(lib, M, bn, 72, cfg, {}))
            if cfg == 0:
                for v in (2, 3):
                    for at in (1, 300):
                        recs.append(record(lib, M, bn, 320, cfg, {"igemm_v128": v, "v128_bk64_tiles": at}))
    for M, N, K in sorted(set((c.M, c.N, c.K) for c in CASES)):
        for deep in (1, 0):
            recs.append(record(lib, M, N, K, -1, {"igemm_deep_rings": deep}))
    return recs


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                             "igemm_instances.json")
    recs = sweep(_capi.load_library())
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True, separators=(",", ":")) for r in recs) + "\n]\n")
    print("%d records, %d instances, %d refused -> %s" % (len(recs), len(set(r.get("instance") for r in recs) - {None}), sum("refused" in r for r in recs), out))


if __name__ == "__main__":
    main()
