"""What launch_igemm decides before it launches (igemm_plan, csrc/gemm.hip), through the host-only pnpi_igemm_plan_query: the measured
table, the cost model behind it, and the fall-backs between them.  Every expectation is worked out here from the rule it tests.

Tile ids (the descriptor table kTileDesc): 0 = 128 x 128, 1 = 64 x 64, 4 = 128 x 320, 5 = 128 x 256, 8 / 11 = 64 x 64 with 4 / 2 k-groups,
10 = 128 x 128 with 2 k-groups, 17 / 19 = the 192 / 128 x 320 ping-pong tiles, 16 / 20 = the 256 / 192 x 256 ones."""
import pytest

from pnpinversion_amd import _capi

MiB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def plan(lib, M, N, K, ks=1, *, bias=0, bias_aligned16=1, residual=0, geglu=0, stats=0, vt_col0=1 << 30, vt_ld=0, vt_f32=0, rows_per_batch=1,
         vt_perm16=0, nbatch=1, ws_bytes=256 * MiB, force_cfg=-1, force_split=0, sel_M=0, ldx1=None):
    C1 = K // (ks * ks)
    d = _capi.IgemmLaunchDesc(M=M, N=N, K=K, ksize=ks, C1=C1, C2=0, ldx1=C1 if ldx1 is None else ldx1, ldx2=0, ldw=K, ldo=N // 2 if geglu else N, ldres=N,
                              bias=bias, bias_aligned16=bias_aligned16, residual=residual, geglu=geglu, stats=stats, vt_col0=vt_col0, vt_ld=vt_ld,
                              vt_f32=vt_f32, rows_per_batch=rows_per_batch, vt_perm16=vt_perm16, nbatch=nbatch, ws_bytes=ws_bytes,
                              force_cfg=force_cfg, force_split=force_split, sel_M=sel_M)
    pl = _capi.IgemmPlan()
    assert lib.pnpi_igemm_plan_query(d, pl) == 0
    return pl


def cdiv(a, b):
    return -(-a // b)


def cost_model(M, N, K, ws_bytes):
    """The cost model of igemm_plan for a plain launch (no transposed columns, no GEGLU, DMA-able), transcribed from its description:
    time = rounds on the busiest of 256 CUs x (t_fix + K-chunks per split x padded tile FLOPs / per-CU rate) / (0.82 + 0.18 fill)
    + under split-K the slab traffic (2 s + 1) M N 4 bytes at 8.14 TB/s and a 4.97 us combine launch.  Returns (id, split)."""
    tiles = [(0, 128, 128, 868e12, 1.22e-6, 3), (1, 64, 64, 572e12, 0.25e-6, 4), (4, 128, 320, 1228e12, 5.15e-6, 2), (5, 128, 256, 1178e12, 3.61e-6, 2)]
    nchunks = cdiv(K, 64)
    best = (1e30, None, None)
    for tid, bm, bn, rate, t_fix, bpc in tiles:
        for s in (1, 2, 3, 4, 6, 8, 12, 16):
            if s > 1 and (nchunks // s < 4 or s * M * N * 4 > ws_bytes):
                continue
            unit = t_fix + cdiv(nchunks, s) * (2.0 * bm * bn * 64) / (rate / 256.0)
            units = cdiv(M, bm) * cdiv(N, bn) * s
            per_cu = units / 256.0
            fill = 1.0 if per_cu >= bpc else (0.0 if per_cu <= 1.0 else (per_cu - 1.0) / (bpc - 1.0))
            t = cdiv(units, 256) * unit / (0.82 + 0.18 * fill)
            if s > 1:
                t += (2 * s + 1) * M * N * 4.0 / 8.14e12 + 4.97e-6
            if t < best[0]:
                best = (t, tid, s)
    return best[1], best[2]


def test_exact_table_hit(lib):
    """tile_table.inc lists {256, 1280, 1280, 1} -> {11, 3}: 64 x 64 tiles with two k-groups, split-K 3"""
    pl = plan(lib, 256, 1280, 1280, bias=1)
    assert (pl.err, pl.id, pl.split) == (0, 11, 3)
    assert (pl.bm, pl.bn, pl.gx, pl.gy, pl.gz) == (64, 64, 4, 20, 3)
    assert pl.kchunks_per_split == 7                      # 20 chunks of 64 over 3 splits
    assert pl.cls == 2 and pl.dma == 1                    # split-K launches report as igemm64_splitk
    assert pl.epi_lds == 0 and pl.bias_init == 0          # slabs: the combine kernel adds the bias
    assert pl.stats == 0 and pl.stats_tile_rows == 0


def test_nearest_row_hit(lib):
    """(20 * 4096, 320, 2880, ks 3) is not listed; the layer is, at 49152 rows (1.67x away) and 98304 (1.2x): the nearer entry is
    {17, 1}.  At the launched 81920 rows 427 tiles of 192 rows take two rounds of 256 and 640 of 128 rows three: the tile stays 192."""
    pl = plan(lib, 20 * 4096, 320, 2880, 3, bias=1, stats=1)
    assert (pl.err, pl.id, pl.split) == (0, 17, 1)
    assert (pl.bm, pl.bn, pl.gx, pl.gy, pl.gz) == (192, 320, 427, 1, 1)
    assert pl.cls == 9 and pl.epi_lds == 1
    assert pl.bias_init == 0                              # the ping-pong kernel adds its bias in the epilogue
    assert pl.stats == 1 and pl.stats_tile_rows == 64     # its statistics partials are per 64-row sub-block


def test_ineligible_ping_pong_entry_goes_to_the_cost_model(lib):
    """{49152, 320, 1280, 1} -> {17, 1}; the ping-pong kernel has no scalar epilogue, so a bias that is not 16-byte aligned takes the
    entry away and the cost model chooses: 384 tiles of 128 x 320 in two rounds (59 us) beat 1152 of 128 x 128 (68 us)"""
    assert plan(lib, 49152, 320, 1280, bias=1).id == 17
    pl = plan(lib, 49152, 320, 1280, bias=1, bias_aligned16=0)
    assert (pl.id, pl.split) == cost_model(49152, 320, 1280, 256 * MiB) == (4, 1)
    assert pl.epi_lds == 1 and pl.bias_init == 0          # LDS epilogue; the 16-byte bias loads of bias_init need the alignment too
    # an entry with split-K ({12288, 320, 5760, 3} -> {17, 4}) lost to a row pitch beyond the 2 GiB buffer descriptor (2 * 12288 * 90000
    # bytes): tile AND split come from the cost model, not the entry's split 4 on another tile
    assert (plan(lib, 12288, 320, 5760, 3, bias=1).id, plan(lib, 12288, 320, 5760, 3, bias=1).split) == (17, 4)
    pl = plan(lib, 12288, 320, 5760, 3, bias=1, ldx1=90000)
    want = cost_model(12288, 320, 5760, 256 * MiB)
    assert (pl.id, pl.split) == want and want[0] in (0, 1, 4, 5) and want[1] != 4


def test_forced_ping_pong_tile_on_a_shape_without_dma(lib):
    """K = 72 (3 x 3 over 8 channels) is no multiple of 64: only the register-staged kernels take it, and they exist as 128 x 128
    and 64 x 64; a forced 192 x 320 falls to 128 x 128"""
    pl = plan(lib, 4096, 320, 72, 3, bias=1, force_cfg=17)
    assert (pl.err, pl.id, pl.split, pl.dma, pl.fastk) == (0, 0, 1, 0, 0)
    assert (pl.bm, pl.bn, pl.gx, pl.gy, pl.gz) == (128, 128, 32, 3, 1)
    assert pl.bias_init == 0 and pl.stats_tile_rows == 0


def test_forced_192x256_takes_no_statistics_launch(lib):
    """the 192 x 256 tile cannot reproduce the 256 x 256 tile's statistics tree: with statistics requested it falls to 128 x 128, which
    produces them per 128-row tile; without, it stays"""
    pl = plan(lib, 2048, 1280, 1280, bias=1, stats=1, force_cfg=20)
    assert (pl.err, pl.id, pl.stats, pl.stats_tile_rows) == (0, 0, 1, 128)
    pl = plan(lib, 2048, 1280, 1280, bias=1, force_cfg=20)
    assert (pl.err, pl.id, pl.bm, pl.bn) == (0, 20, 192, 256)


def test_batched_launch_loses_k_groups_and_split(lib):
    """nbatch > 1: grid z is the problem index, so no split-K and no k-groups: id 8 (64 x 64, 4 k-groups) becomes id 1"""
    pl = plan(lib, 1024, 1280, 1280, nbatch=4, force_cfg=8, force_split=3)
    assert (pl.err, pl.id, pl.split) == (0, 1, 1)
    assert (pl.gx, pl.gy, pl.gz) == (16, 20, 4)
    assert plan(lib, 1024, 1280, 1280, nbatch=4, force_cfg=8, bias=1).err == -8      # batched launches are plain products


def test_forced_split_is_clamped_to_the_workspace(lib):
    need = 8 * 256 * 1280 * 4                             # eight fp32 slabs
    pl = plan(lib, 256, 1280, 1280, force_cfg=0, force_split=8, ws_bytes=need)
    assert (pl.id, pl.split, pl.gz, pl.kchunks_per_split) == (0, 8, 8, 3)
    pl = plan(lib, 256, 1280, 1280, force_cfg=0, force_split=8, ws_bytes=need - 1)
    assert (pl.id, pl.split, pl.gz, pl.kchunks_per_split) == (0, 1, 1, 20)
    assert plan(lib, 256, 1280, 1280, force_cfg=0, force_split=8, ws_bytes=0).split == 1
    assert plan(lib, 256, 1280, 1280, force_cfg=0, force_split=64).split == 20      # at most one 64-wide chunk per split


def test_rejections(lib):
    """GEGLU pairs 32-column groups: N % 64; the permuted V^T moves whole 16-token groups"""
    pl = plan(lib, 4096, 2592, 320, bias=1, geglu=1)
    assert pl.err == -7 and pl.id >= 0 and pl.stats_tile_rows == -1
    assert plan(lib, 4096, 2560, 320, bias=1, geglu=1).err == 0
    kw = dict(bias=1, vt_col0=640, vt_ld=4096)
    assert plan(lib, 4096, 960, 320, rows_per_batch=8, vt_perm16=1, **kw).err == -9
    assert plan(lib, 4096, 960, 320, rows_per_batch=16, vt_perm16=1, **kw).err == 0
    assert plan(lib, 0, 320, 320).err == -2 and plan(lib, 0, 320, 320).id == -1
    assert plan(lib, 64, 320, 324).err == -3                                        # K % 8
    assert plan(lib, 64, 320, 320, force_cfg=21).err == -2 and plan(lib, 64, 320, 320, force_cfg=20).err == 0


def test_misaligned_transposed_columns_clear_the_lds_epilogue(lib):
    """q | k | v of a 320-wide block with V transposed from column 640: the table's {4096, 960, 320, 1} -> {10, 1} is 128 wide and 640 is
    a tile boundary, so V^T goes through the LDS epilogue; from column 648 no tile is whole and the launch takes the scalar epilogue"""
    kw = dict(bias=1, vt_ld=4096, rows_per_batch=4096, stats=1)
    pl = plan(lib, 4096, 960, 320, vt_col0=640, **kw)
    assert (pl.err, pl.id, pl.epi_lds) == (0, 10, 1)
    assert pl.stats == 0 and pl.stats_tile_rows == 0      # a launch whose V^T columns take the LDS epilogue produces no statistics
    pl = plan(lib, 4096, 960, 320, vt_col0=648, **kw)
    assert pl.err == 0 and pl.epi_lds == 0 and pl.stats == 0
    assert pl.id in (0, 1, 4, 5)                          # the entry needs vt_col0 on its tile boundary: the cost model chose
    assert plan(lib, 4096, 960, 320, vt_col0=5000, **kw).vt_col0 == 960      # clamped to N: no transposed columns


def test_sel_m_pins_the_choice_and_the_row_height_follows_the_launch(lib):
    """(32768, 320, 2880, ks 3) configured as at 49152 rows ({49152, 320, 2880, 3} -> {17, 1}): the family and the ring depth are the
    49152-row launch's, the row height is picked on the 32768 launched rows -- 171 tiles of 192 rows or 256 of 128, one round each"""
    full = plan(lib, 49152, 320, 2880, 3, bias=1)
    assert (full.id, full.split, full.gx, full.sparse) == (17, 1, 256, 2)
    pl = plan(lib, 32768, 320, 2880, 3, bias=1, sel_M=49152)
    assert (pl.err, pl.id, pl.split) == (0, 19, 1)
    assert (pl.bm, pl.bn, pl.gx, pl.gy, pl.gz) == (128, 320, 256, 1, 1)
    assert pl.sparse == 1                                 # occupancy is counted at sel_M: 384 units of 128 rows, two per CU
    with _capi.tuning(lib, pp_rowtile=0):
        assert plan(lib, 32768, 320, 2880, 3, bias=1, sel_M=49152).id == 17
