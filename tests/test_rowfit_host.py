"""The table rows measured for the shapes the lock-step step launches (8 rows on 4 latents under src_share = 1 / cfg_dedup = 1;
profiles/rowfit_fwd_tune_b8edit.json -> tools/merge_tile_candidates.py --spread -> csrc/tile_table.inc), through the host-only
pnpi_igemm_plan_query / pnpi_tile_table_lookup: the launched M finds the new row, the logical row count (sel_M, what src_share = 2 and
cfg_dedup = 2 hand the plan) still finds the 12-row choice, no 12-row or 1-row shape is sent to a new row by the nearest-M rule, and no
new row's split-K is clamped by the workspace of a context sized for 12 or for 96 rows."""
import ctypes as C
import os
import re

import pytest

from pnpinversion_amd import _capi

MiB = 1 << 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "pnpinversion_amd", "csrc", "tile_table.inc")
# {M at 8 rows, N, K, ksize}: (tile id, split-K) of the new row, (tile id, split-K) of the same layer's 12-row row (M * 3 / 2), GEGLU epilogue
ROWS = {
    (512, 1280, 6400, 1): ((18, 6), (18, 4), 0),
    (512, 1280, 11520, 3): ((18, 6), (18, 4), 0),
    (2048, 640, 5760, 3): ((18, 3), (18, 2), 0),
    (2048, 1280, 2560, 1): ((18, 1), (18, 1), 0),
    (2048, 3840, 1280, 1): ((17, 1), (17, 1), 0),
    (2048, 10240, 1280, 1): ((16, 1), (17, 1), 1),
    (8192, 320, 2880, 3): ((1, 1), (11, 1), 0),
    (8192, 640, 1920, 1): ((14, 1), (14, 1), 0),
    (8192, 1280, 11520, 3): ((17, 1), (16, 1), 0),
    (8192, 2304, 640, 1): ((16, 1), (16, 1), 0),
    (32768, 320, 320, 1): ((17, 1), (17, 1), 0),
    (32768, 2560, 320, 1): ((16, 1), (0, 1), 1),
}
FAMILY = {16: (16, 20), 17: (17, 19)}      # a ping-pong row names its family; pp_rowtile picks the row height on the launched M


def ws_of(max_unet_rows):
    """the split-K workspace of a context (pnpi_create): 96 MiB, 8 MiB more for every row beyond 12"""
    return 96 * MiB + max(max_unet_rows - 12, 0) * 8 * MiB


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def plan(lib, M, N, K, ks, geglu=0, sel_M=0, ws_bytes=ws_of(12)):
    C1 = K // (ks * ks)
    d = _capi.IgemmLaunchDesc(M=M, N=N, K=K, ksize=ks, C1=C1, C2=0, ldx1=C1, ldx2=0, ldw=K, ldo=N // 2 if geglu else N, ldres=N, bias=1, bias_aligned16=1,
                              residual=0, geglu=geglu, stats=0, vt_col0=1 << 30, vt_ld=0, vt_f32=0, rows_per_batch=1, vt_perm16=0, nbatch=1,
                              ws_bytes=ws_bytes, force_cfg=-1, force_split=0, sel_M=sel_M)
    pl = _capi.IgemmPlan()
    assert lib.pnpi_igemm_plan_query(d, pl) == 0 and pl.err == 0
    return pl


def lookup(lib, M, N, K, ks):
    cfg, split, em = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    how = lib.pnpi_tile_table_lookup(M, N, K, ks, C.byref(cfg), C.byref(split), C.byref(em))
    return how, cfg.value, split.value, em.value


def check_choice(lib, pl, want, M, N):
    cfg, split = want
    assert pl.split == split, (pl.id, pl.split, want)
    assert pl.id in FAMILY.get(cfg, (cfg,)), (pl.id, pl.split, want)
    if cfg in FAMILY:
        assert pl.bm == lib.pnpi_pp_rowtile_query(cfg, M, N, split)


@pytest.mark.parametrize("shape", sorted(ROWS))
def test_launched_rows_find_the_new_row_and_the_logical_rows_the_old_choice(lib, shape):
    M, N, K, ks = shape
    new, old, geglu = ROWS[shape]
    assert lookup(lib, M, N, K, ks) == (1,) + new + (M,)
    check_choice(lib, plan(lib, M, N, K, ks, geglu), new, M, N)
    # src_share = 2 / cfg_dedup = 2: the launch of 8 rows is planned as the 12 logical rows it serves
    assert M * 3 % 2 == 0 and lookup(lib, M * 3 // 2, N, K, ks) == (1,) + old + (M * 3 // 2,)
    check_choice(lib, plan(lib, M, N, K, ks, geglu, sel_M=M * 3 // 2), old, M, N)


def test_no_twelve_row_or_one_row_shape_goes_to_a_new_row(lib):
    """the nearest-M rule applies to shapes without a row of their own: the layers of the new rows at 1 and 12 rows (an eighth and one
    and a half times the 8-row M), and every row the table's comments mark as measured in a 1-row or a 12-row forward, resolve elsewhere"""
    new = set(ROWS)
    for (M, N, K, ks) in ROWS:
        for m in (M // 8, M * 3 // 2):
            how, _, _, em = lookup(lib, m, N, K, ks)
            assert how == 0 or (em, N, K, ks) not in new, (m, N, K, ks, em)
    n = 0
    for line in open(INC):
        r = re.match(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\},\s+// (1|12) rows:", line)
        if r:
            M, N, K, ks, cfg, split = (int(x) for x in r.groups()[:6])
            assert (M, N, K, ks) not in new
            assert lookup(lib, M, N, K, ks) == (1, cfg, split, M)
            n += 1
    assert n > 100


@pytest.mark.parametrize("max_unet_rows", [12, 96])
def test_split_k_of_the_new_rows_fits_the_workspace(lib, max_unet_rows):
    """8-row launches on a context sized for the lock-step edit (12 rows) and for 96 rows: the plan keeps the row's split-K.  The same
    layers launched at 96 rows on the 96-row context keep the split of the entry they resolve to."""
    ws = ws_of(max_unet_rows)
    for (M, N, K, ks), (new, _, geglu) in ROWS.items():
        assert new[1] == 1 or new[1] * M * N * 4 <= ws      # split-K 1 writes no slabs
        assert plan(lib, M, N, K, ks, geglu, ws_bytes=ws).split == new[1]
        if max_unet_rows == 96:
            how, _, split, _ = lookup(lib, M * 12, N, K, ks)
            if how:
                assert plan(lib, M * 12, N, K, ks, geglu, ws_bytes=ws).split == (1 if geglu else split)


def test_the_old_eight_row_row_of_the_32x32_upsampler_was_clamped(lib):
    """why {8192, 1280, 11520, 3} changed most: its former row {16, 3} needs three fp32 slabs of 8192 x 1280 = 120 MiB, more than the 96 MiB
    of a 12-row context, so the plan fell to the cost model (128 x 320, split-K 2: 277 us against 224 us for the new row)"""
    assert 3 * 8192 * 1280 * 4 > ws_of(12) >= 1 * 8192 * 1280 * 4


def test_a_launch_configured_as_at_fewer_rows_still_fits_its_slabs(lib):
    """the full 12-row launch of a tape-holding context is configured as the 8-row launch (sel_M below M): {512, 1280, 11520, 3} -> split-K 6,
    but the slabs are written for the 768 launched rows -- with room for six slabs of 512 rows only, the split must come down"""
    ws = 6 * 512 * 1280 * 4
    assert plan(lib, 512, 1280, 11520, 3, ws_bytes=ws).split == 6
    pl = plan(lib, 768, 1280, 11520, 3, sel_M=512, ws_bytes=ws)
    assert pl.split * 768 * 1280 * 4 <= ws and pl.split < 6
    pl = plan(lib, 768, 1280, 11520, 3, sel_M=512)
    assert (pl.id, pl.split) == (18, 6) and pl.gx == 6       # room for all: the 8-row choice on the 12-row grid
