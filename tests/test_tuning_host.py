"""The tuning-knob table (csrc/tuning.h, tuning.hip): its surface, the built-in defaults, set / get / reset, the environment variables
that seed it at load, and the scoped setter _capi.tuning.  CPU only.  What depends on the state at load runs in a child process that
loads the library with ctypes alone (no torch, no context) under an environment of its own and answers a list of operations."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

from pnpinversion_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every key pnpi_set_tuning accepts, with its built-in default
DEFAULTS = {
    "text_kv": 1, "temb_cache": 1, "ff_fold": 1, "cfg_dedup": 1, "src_share": 1, "attn_aug": 1, "attn_vt_perm": 1, "attn_bwd_flash": 1,
    "op_attention_aug": 0, "op_gemm_vt_perm16": 0, "op_attention_vt_perm": 0, "gn_inline_rows": 0, "attn_pipe": 0,
    "igemm_dma": 1, "igemm_v128": 2, "igemm_v64": 0, "igemm_v256": 0, "igemm_v320": 1, "igemm_v256n": 1, "igemm_wide": 1, "tile_order": -1,
    "igemm_force_cfg": -1, "igemm_force_split": 0, "igemm_bias_init": 1, "igemm_sched": 0, "igemm_vpp": 0, "igemm_tapin": 0,
    "igemm_pp_only_n": 0, "igemm_pp_only_k": 0, "igemm_pp_only_m": 0, "igemm_deep_rings": 1, "igemm_vt_lds": 1, "igemm_res_late": 0,
    "igemm_table": 1, "igemm_table_near": 1, "pp_rowtile": 1,
    # the switches that were environment variables only
    "attn_nodma": 0, "attn_ksq4": 0, "attn_noaug": 0, "abf_prefetch": 1, "gn_small_max": 24576, "gn_wide_below": 1 << 30, "gn_small_min": 0,
    "gn_nofuse": 0, "v128_bk64_tiles": 0,
}
# values a product library rejects: outside the range, or selectors of instances only a `build --ablations` library has
REJECTED = {"cfg_dedup": (-1, 3, 7), "src_share": (-1, 3), "igemm_vpp": (1, 4), "igemm_sched": (1, 2), "attn_pipe": (1, 2),
            "igemm_v128": (11, 12, 15), "igemm_v320": (11, 12, 15)}
NO_OTHER_VALUE = ("igemm_vpp", "igemm_sched", "attn_pipe")      # the product library accepts their default only
STORED_AS_BOOL = ("op_gemm_vt_perm16", "pp_rowtile")


def other_value(key):
    """an accepted value that is not the default"""
    d = DEFAULTS[key]
    return {"cfg_dedup": 2, "src_share": 0}.get(key, 1 - d if d in (0, 1) else d + 3)


CHILD = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
def info():
    out, k, a, b, i = {}, C.c_char_p(), C.c_int(), C.c_int(), 0
    while lib.pnpi_tuning_info(i, C.byref(k), C.byref(a), C.byref(b)) == 0:
        assert k.value.decode() not in out
        out[k.value.decode()] = [a.value, b.value]
        i += 1
    assert lib.pnpi_tuning_info(-1, None, None, None) != 0 and lib.pnpi_tuning_info(i, None, None, None) != 0
    assert lib.pnpi_tuning_info(0, None, None, None) == 0                   # every output is optional
    return out
def get(key):
    v = C.c_int(-12345)
    return [lib.pnpi_get_tuning(key.encode(), C.byref(v)), v.value]
ops = {"info": info, "set": lambda key, v: lib.pnpi_set_tuning(key.encode(), v), "get": get, "reset": lib.pnpi_reset_tuning}
print(json.dumps([ops[op[0]](*op[1:]) for op in json.loads(sys.argv[2])]))
"""


def child(ops, **env):
    """run ops in a fresh process that sees no PNPI_* variable but those given; -> one result per op"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("PNPI_")}
    e.update(env)
    lib_path = os.environ.get("PNPI_LIBRARY") or _capi.LIB_PATH
    r = subprocess.run([sys.executable, "-c", CHILD, lib_path, json.dumps(ops)], env=e, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def table(lib):
    """[(key, initial, current)] of the loaded library"""
    rows, k, a, b = [], C.c_char_p(), C.c_int(), C.c_int()
    while lib.pnpi_tuning_info(len(rows), C.byref(k), a, b) == 0:
        rows.append((k.value.decode(), a.value, b.value))
    return rows


def test_surface():
    lib = _capi.load_library()
    keys = [r[0] for r in table(lib)]
    assert len(set(keys)) == len(keys)
    assert set(keys) == set(DEFAULTS), set(keys) ^ set(DEFAULTS)
    assert lib.pnpi_tuning_info(len(keys), None, None, None) != 0 and lib.pnpi_tuning_info(-1, None, None, None) != 0
    hdr = open(os.path.join(ROOT, "include", "pnpi.h")).read()
    assert not [k for k in keys if '"%s"' % k not in hdr]
    for k, _, cur in table(lib):
        assert _capi.get_tuning(lib, k) == cur


def test_built_in_defaults():
    got = child([["info"]])[0]
    assert got == {k: [v, v] for k, v in DEFAULTS.items()}, {k: (got.get(k), DEFAULTS.get(k)) for k in set(got) | set(DEFAULTS) if got.get(k) != [DEFAULTS.get(k)] * 2}


def test_round_trip_rejections_and_reset():
    ops, want = [], []
    for key, d in DEFAULTS.items():
        if key not in NO_OTHER_VALUE:
            v = other_value(key)
            assert v != d
            ops += [["set", key, v], ["get", key]]
            want += [0, [0, v]]
            if key in STORED_AS_BOOL:
                ops += [["set", key, 5], ["get", key], ["set", key, v]]
                want += [0, [0, 1], 0]
        stored = d if key in NO_OTHER_VALUE else other_value(key)
        for bad in REJECTED.get(key, ()):
            ops += [["set", key, bad], ["get", key]]
            want += [_capi.PNPI_EINVAL, [0, stored]]
    for key in ("no_such_knob", "gn_slab", ""):
        ops += [["set", key, 1], ["get", key]]
        want += [_capi.PNPI_EINVAL, [_capi.PNPI_EINVAL, -12345]]
    n = len(ops)
    ops += [["info"], ["reset"], ["info"]]
    got = child(ops)
    assert got[:n] == want, [(o, g, w) for o, g, w in zip(ops, got, want) if g != w]
    changed, rc, after = got[n:]
    assert {k: v[0] for k, v in changed.items()} == DEFAULTS                              # `initial` does not move with the knob
    assert all(changed[k][1] != DEFAULTS[k] for k in DEFAULTS if k not in NO_OTHER_VALUE)
    assert rc == 0 and after == {k: [v, v] for k, v in DEFAULTS.items()}


@pytest.mark.parametrize("env,key,want", [
    ({"PNPI_CFG_DEDUP": "0"}, "cfg_dedup", 0), ({"PNPI_SRC_SHARE": "2"}, "src_share", 2), ({"PNPI_PP_ROWTILE": "0"}, "pp_rowtile", 0),
    ({"PNPI_IGEMM_V128": "3"}, "igemm_v128", 3), ({"PNPI_CFG_DEDUP": "7"}, "cfg_dedup", 1), ({"PNPI_PP_ROWTILE": "5"}, "pp_rowtile", 1),
    ({"PNPI_ATTN_NOAUG": "1"}, "attn_noaug", 1), ({"PNPI_GN_NOFUSE": "0"}, "gn_nofuse", 1),      # switched on by being set, as before
    ({"PNPI_ABF_PREFETCH": "0"}, "abf_prefetch", 0), ({"PNPI_GN_SMALL_MAX": "8192"}, "gn_small_max", 8192),
    ({"PNPI_V128_BK64_TILES": "512"}, "v128_bk64_tiles", 512),
    ({"PNPI_IGEMM_V320": "12"}, "igemm_v320", 1),                                              # an ablation selector: not in this library
], ids=lambda p: "-".join("%s=%s" % kv for kv in p.items()) if isinstance(p, dict) else None)
def test_environment_seeds_the_knob_at_load(env, key, want):
    # the variable gives `initial` of its knob alone and is not read again: a set value stays, reset goes back to what the variable gave
    v = other_value(key)
    res = child([["info"], ["set", key, v], ["get", key], ["reset"], ["get", key]], **env)
    assert {k: i for k, (i, _) in res[0].items()} == dict(DEFAULTS, **{key: want})
    assert res[1:] == [0, [0, v], 0, [0, want]]


def test_scoped_setter_nests_and_restores():
    lib = _capi.load_library()
    before = table(lib)
    a, b = other_value("igemm_v64"), other_value("igemm_v64") + 1
    with _capi.tuning(lib, igemm_v64=a, cfg_dedup=2):
        assert (_capi.get_tuning(lib, "igemm_v64"), _capi.get_tuning(lib, "cfg_dedup")) == (a, 2)
        with _capi.tuning(lib, igemm_v64=b):
            assert (_capi.get_tuning(lib, "igemm_v64"), _capi.get_tuning(lib, "cfg_dedup")) == (b, 2)
        assert _capi.get_tuning(lib, "igemm_v64") == a
        with _capi.tuning(lib):
            pass
    assert table(lib) == before


def test_scoped_setter_restores_when_the_block_raises():
    lib = _capi.load_library()
    before = table(lib)
    with pytest.raises(KeyError):
        with _capi.tuning(lib, ff_fold=0, igemm_force_cfg=4):
            assert _capi.get_tuning(lib, "igemm_force_cfg") == 4
            raise KeyError("from the block")
    assert table(lib) == before


@pytest.mark.parametrize("knobs", [{"ff_fold": 0, "cfg_dedup": 3}, {"igemm_tapin": 1, "igemm_vpp": 1}, {"ff_fold": 0, "no_such_knob": 1}])
def test_scoped_setter_rejected_value_raises_and_changes_nothing(knobs):
    lib = _capi.load_library()
    before = table(lib)
    ran = False
    with pytest.raises(ValueError):
        with _capi.tuning(lib, **knobs):
            ran = True
    assert not ran and table(lib) == before
