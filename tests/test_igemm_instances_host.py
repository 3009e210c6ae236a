"""Which kernel instance launch_igemm runs, held to a recording: tests/golden/igemm_instances.json is a sweep over tile ids, variant knobs,
occupancy classes and K, recorded by tools/make_igemm_instance_golden.py (its docstring lists the sweep) at the commit before the instance
table kInstances and its rules kInstRules (csrc/gemm.hip) replaced the launcher's switch.  Every record is planned again through
pnpi_igemm_plan_query; err, tile id, variant, sparse, split-K, the grid and the name of the instance row have to be the recorded ones.

The recording is checked too: all 36 product instances occur, and every (tile id, knob value) pair the sweep promises.  A product library
cannot be brought to the -10 of "this variant has no row" from outside: the only knob that reaches it is igemm_vpp, and pnpi_set_tuning
refuses every igemm_vpp but 0 there (tests/test_tuning_host.py), so the recording holds no err = -10; its igemm_vpp = 1 records hold the
refusal, which is replayed.  The rule behind -10 (no row for the short ping-pong tiles' ablations in any build, rows for the tall tiles'
in an ablation library only) is a static_assert next to kInstRules, compiled into both libraries."""
import json
import os

import pytest

from pnpinversion_amd import _capi
from tests.test_gemm_bound_host import PRODUCT_INSTANCES, instance_name, query_plan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "igemm_instances.json")
TILE_IDS = (0, 1) + tuple(range(3, 21))
KNOB_VALUES = {("igemm_v128", 0): (0, 1, 2, 3, 4, 8, 7), ("igemm_v64", 1): (0, 1, 2, 3, 8, 7), ("igemm_v256", 3): (0, 1), ("igemm_v320", 4): (0, 1, 2, 3),
               ("igemm_v256n", 5): (0, 1, 2, 3), ("igemm_vpp", 16): (0, 1), ("igemm_vpp", 17): (0, 1), ("igemm_vpp", 19): (0, 1), ("igemm_vpp", 20): (0, 1)}


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


@pytest.fixture(scope="module")
def records():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_covers_the_sweep(records):
    planned = [r for r in records if "plan" in r]
    assert set(r["instance"] for r in planned if r["plan"][0] == 0) == PRODUCT_INSTANCES
    for (knob, cfg), values in KNOB_VALUES.items():
        for v in values:
            for deep in (0, 1):
                for dma in (0, 1):
                    want = {knob: v, "igemm_deep_rings": deep, "igemm_dma": dma}
                    assert any(r["cfg"] == cfg and r["tune"] == want for r in records), (cfg, want)
    for cfg in TILE_IDS:
        mine = [r for r in planned if r["cfg"] == cfg and r["K"] == 320 and r["tune"].get("igemm_deep_rings") == 1 and r["tune"].get("igemm_dma") == 1]
        assert set(r["plan"][3] for r in mine) == {0, 1, 2}, cfg                        # the three occupancy classes
        assert any(r["cfg"] == cfg and r["K"] == 72 and r["instance"].endswith("generic>") for r in planned), cfg
    assert set(r["tune"].get("v128_bk64_tiles", 0) for r in records if r["cfg"] == 0) >= {0, 1}
    assert sum(r["cfg"] == -1 for r in planned) >= 100                                  # the table / cost-model path
    # igemm_vpp = 1: refused by the product library the recording was made with (module docstring), never planned
    vpp = [r for r in records if r["tune"].get("igemm_vpp") == 1]
    assert vpp and all(r.get("refused") for r in vpp) and not any(r.get("refused") for r in records if r not in vpp)


def test_the_library_replays_the_recording(lib, records):
    for r in records:
        try:
            with _capi.tuning(lib, **r["tune"]):
                pl = query_plan(lib, r["M"], r["N"], r["K"], cfg=r["cfg"], bias="a16")
        except ValueError:
            assert r.get("refused"), r
            continue
        assert not r.get("refused"), r
        got = [pl.err, pl.id, pl.variant, pl.sparse, pl.split, pl.gx, pl.gy, pl.gz]
        assert got == r["plan"], (r, got)
        assert (instance_name(lib, pl) if pl.err == 0 else None) == r["instance"], (r, pl.instance)
        assert pl.err == 0 or pl.instance == -1, r
