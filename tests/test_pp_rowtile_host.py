"""The row-height rule of the ping-pong GEMM launches (launch_igemm's pp_rowtile_pick, csrc/gemm.hip), through its host-only query.

Tile and split-K of a launch are chosen as ever (the table entry at sel_M); the rule then picks, inside the family of the chosen BN and
for the LAUNCHED M, the shorter tile when its W = ceil(M / bm) * ceil(N / BN) * split workgroups need no more rounds of 256 (one
workgroup per CU) than the taller tile's.  The rule's first form, "minimise ceil(W / 256) * bm", differs only where the shorter tile
adds a round: the kernel trace showed four rounds of 128 rows losing to three of 192 (profiles/pp_rowtile_ab.json), so those launches
keep the taller tile.  cfg 17 / 19 = 192 / 128 x 320, cfg 16 / 20 = 256 / 192 x 256."""
import pytest

from pnpinversion_amd import _capi


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def _by_hand(M, N, split, bn, tall, short):
    rounds = lambda bm: -(-(-(-M // bm) * -(-N // bn) * split) // 256)      # noqa: E731
    return short if rounds(short) <= rounds(tall) else tall


@pytest.mark.parametrize("cfg,M,N,split,want", [
    (17, 32768, 320, 1, 128),      # 8 rows at 64 x 64: 171 tiles of 192 rows on two thirds of the CUs -> exactly 256 of 128
    (17, 49152, 320, 1, 192),      # 12 rows: exactly 256 tiles of 192, one round; 384 of 128 would take two
    (17, 16384, 320, 1, 128),      # the compact CFG prefix (4 latents): 86 -> 128 workgroups, one round either way
    (16, 2048, 1280, 4, 192),      # 8 rows at 16 x 16, split-K 4: 8 x 5 x 4 = 160 -> 11 x 5 x 4 = 220 workgroups, one round
    (16, 3072, 1280, 4, 256),      # 12 rows: 240 workgroups, one round; 320 of 192 rows would take two
    # 8 rows at 32 x 32, N = 5120: 43 x 16 = 688 workgroups = three rounds of 192 against 64 x 16 = 1024 = four of 128 (0.89 on paper,
    # 1.08 measured): the rule as shipped keeps 192
    (17, 8192, 5120, 1, 192),
])
def test_rule_on_the_shapes_of_the_lock_step(lib, cfg, M, N, split, want):
    assert lib.pnpi_pp_rowtile_query(cfg, M, N, split) == want
    assert want == (_by_hand(M, N, split, 320, 192, 128) if cfg == 17 else _by_hand(M, N, split, 256, 256, 192))


def test_other_row_counts_keep_their_tile(lib):
    """96 rows (8 rounds of 192 against 12 of 128) stay; 12-row launches of the 32 x 32 and 16 x 16 levels stay"""
    assert lib.pnpi_pp_rowtile_query(17, 96 * 4096, 320, 1) == 192
    assert lib.pnpi_pp_rowtile_query(17, 12288, 640, 2) == 192
    assert lib.pnpi_pp_rowtile_query(16, 96 * 256, 1280, 1) == 256
    assert lib.pnpi_pp_rowtile_query(17, 8192, 2560, 1) == 128       # 344 workgroups: 1.35 rounds of 192 -> two full rounds of 128


def test_family_ids(lib):
    """the short tiles' own ids name the same families and get the same answer; anything else is no ping-pong tile"""
    assert lib.pnpi_pp_rowtile_query(19, 32768, 320, 1) == 128 and lib.pnpi_pp_rowtile_query(19, 49152, 320, 1) == 192
    assert lib.pnpi_pp_rowtile_query(20, 2048, 1280, 4) == 192 and lib.pnpi_pp_rowtile_query(20, 3072, 1280, 4) == 256
    assert lib.pnpi_pp_rowtile_query(17, 96 * 4096, 320, 1) == 192 and lib.pnpi_pp_rowtile_query(19, 96 * 4096, 320, 1) == 192
    for cfg in (-1, 0, 4, 15, 18, 21):
        assert lib.pnpi_pp_rowtile_query(cfg, 32768, 320, 1) == 0
    assert lib.pnpi_pp_rowtile_query(17, 0, 320, 1) == 0


def test_knob_is_a_tuning_key(lib):
    with _capi.tuning(lib, pp_rowtile=0), _capi.tuning(lib, pp_rowtile=1):      # both accepted (a rejected value raises)
        assert _capi.get_tuning(lib, "pp_rowtile") == 1
