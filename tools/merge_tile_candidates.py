"""Patch csrc/tile_table.inc with NEW tile configurations measured after the table was generated: each input is a tools/fwd_tune.py
JSON of a partial sweep (FWD_TUNE_CFGS=...: `auto` = what the current table runs for the shape + the new configurations, all timed in
the same process on the same box); an entry is replaced when a new configuration beats `auto` by more than --margin (default 3 %:
interleaved arms of one process repeat to about 1 - 2 %).  Entries the sweeps did not see, or did not beat, stay as they are.
--spread: the bar is the shape's own run-to-run spread in the sweep instead (its "spread_us": max - min of the repeated `auto` arms of
tools/fwd_tune.py FWD_TUNE_WORK=edit), taken twice -- the difference of two timings that each move by it -- and against the better of
`auto` and the forced arm of the configuration `auto` ran (single launches move with their place in the sweep by more than the
repeated arms show).  Shapes the table does not list yet are ADDED, and a candidate that is what `auto` already ran is no candidate.  The shorter ping-pong row heights (pp320r128, pp256r192) are no table ids: the table names the family (17 / 16) and
pp_rowtile picks the height on the launched M, so a ping-pong timing counts only where pnpi_pp_rowtile_query picks that height.
usage: merge_tile_candidates.py [--margin 0.03 | --spread] table.inc sweep.json [sweep.json ...]"""
import json, os, re, sys
CFG = {"128": 0, "64": 1, "256m": 3, "320": 4, "256n": 5, "256x320": 6, "256x256": 7, "64k4": 8, "128k2": 9, "128k2b": 10, "64k2": 11, "64x320": 12, "128n2": 13, "128b64": 14,
       "256nb64": 15, "pp256": 16, "pp320": 17, "128b64x3": 18}      # tools/gen_tile_table.py's names
PP = {"pp320": (17, 192), "pp320r128": (17, 128), "pp256": (16, 256), "pp256r192": (16, 192)}      # name -> (table id, row height)
args = sys.argv[1:]
margin, spread = 0.03, False
if args[0] == "--margin":
    margin = float(args[1]); args = args[2:]
elif args[0] == "--spread":
    spread = True; args = args[1:]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from pnpinversion_amd import _capi
    lib = _capi.load_library()
table, sweeps = args[0], args[1:]
best = {}
for path in sweeps:
    d = json.load(open(path))
    for sh in d["shapes"]:
        auto = sh["us"].get("auto")
        if not auto:
            continue
        cands = {k: v for k, v in sh["us"].items() if k != "auto" and k.partition("/s")[0] in CFG}
        if spread:
            cands = {}
            for k, v in sh["us"].items():
                base, _, sp = k.partition("/s")
                sp = int(sp) if sp else 1
                if base in PP:
                    if lib.pnpi_pp_rowtile_query(PP[base][0], sh["M"], sh["N"], sp) == PP[base][1]:
                        cands[(PP[base][0], sp)] = v
                elif base in CFG:
                    cands[(CFG[base], sp)] = v
            ab, _, asp = (sh.get("auto_cfg") or "").partition("/s")
            same = cands.pop((PP[ab][0] if ab in PP else CFG.get(ab, -1), int(asp) if asp else 1), None)
            if same is not None and same < auto: auto = same
        if not cands:
            continue
        key, us = min(cands.items(), key=lambda kv: kv[1])
        if (us < auto - 2.0 * sh.get("spread_us", auto)) if spread else (us < (1.0 - margin) * auto):
            if spread:
                cfg, sp = key
            else:
                base, _, sp = key.partition("/s"); cfg = CFG[base]
            k = (sh["M"], sh["N"], sh["K"], sh["ks"])
            if k not in best or us / auto < best[k][3]:
                best[k] = (cfg, int(sp) if sp else 1, us, us / auto, auto, d["rows"])
out, n = [], 0
for line in open(table):
    m = re.match(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},", line)
    if m:
        k = tuple(int(x) for x in m.groups()[:4])
        if k in best:
            cfg, split, us, _, auto, rows = best[k]
            line = "{%d, %d, %d, %d, %d, %d},   // %d rows: %.1f us (was %.1f us under {%s, %s}; tools/merge_tile_candidates.py)\n" % (k + (cfg, split, rows, us, auto, m.group(5), m.group(6)))
            n += 1
            best[k] += (True,)
    out.append(line)
if spread:      # new shapes, in the table's order: rows sorted by {M, N, K, ksize} behind the header comment
    add = ["{%d, %d, %d, %d, %d, %d},   // %d rows: %.1f us (was %.1f us without an entry; tools/merge_tile_candidates.py)\n" % (k + (v[0], v[1], v[5], v[2], v[4]))
           for k, v in best.items() if len(v) == 6]
    n += len(add)
    head = [l for l in out if not l.startswith("{")]
    out = head + sorted([l for l in out if l.startswith("{")] + add, key=lambda l: tuple(int(x) for x in re.match(r"\{(\d+), (\d+), (\d+), (\d+),", l).groups()))
open(table, "w").writelines(out)
print("%d of %d candidate shapes replaced in %s" % (n, len(best), table))
for k, v in sorted(best.items()):
    print("  %s -> cfg %d split %d: %.1f us against %.1f" % (k, v[0], v[1], v[2], v[4]))
