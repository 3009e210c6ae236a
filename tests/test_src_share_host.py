"""The row maps of pnpi_direct_edit's shared-row launch (tuning "src_share"; pnpi_src_share_maps is the host-only export of the builder the
loop itself calls, csrc/api_loops.inc src_share_maps).

Logical rows of a step: pseudo-image q = p * nimg + im (pass p = 0 the offset pass O, 1 .. npass the guidance passes R, E) owns the rows
4 q + [unc_src, unc_tgt, cond_src, cond_tgt], on the latents 2 q (source) and 2 q + 1 (target), with the context rows 4 im + k.  The
source latents of every pass of an image are one latent (same x_T, same update), so a logical row's identity is the pair
(latent with the passes' source latents identified, context row).  Checked for nimg 1 - 3 and npass 1 - 2:
every logical row maps to a compact row with the same identity, no two compact rows share one (nothing is launched twice), the counts,
O1 (the offset pass's own target row: `prev + (x* - prev)` on another `prev`) is nobody else's row, and each pass's Prompt-to-Prompt pair
source is the compact row of its image's O2."""
import ctypes as C

import pytest


def _maps(nimg, npass):
    from pnpinversion_amd import _capi
    lib = _capi.load_library()
    rows = (1 + npass) * 4 * nimg
    bufs = [(C.c_int * n)() for n in (rows, rows, rows, rows)]            # lsel / cmap / cctx never exceed the logical row count
    crows, nlat = C.c_int(-1), C.c_int(-1)
    assert lib.pnpi_src_share_maps(nimg, npass, bufs[0], bufs[1], bufs[2], bufs[3], C.byref(crows), C.byref(nlat)) == 0
    lsel, cmap, cctx, omap = (list(b) for b in bufs)
    return lsel[:nlat.value], cmap[:crows.value], cctx[:crows.value], omap, crows.value, nlat.value


def _canon_latent(lat, nimg):
    """logical latent 2 q + s -> the same with every pass's source latent named as the offset pass's"""
    q, s = divmod(lat, 2)
    return 2 * (q % nimg) if s == 0 else lat


@pytest.mark.parametrize("nimg", [1, 2, 3])
@pytest.mark.parametrize("npass", [1, 2])
def test_maps(nimg, npass):
    lsel, cmap, cctx, omap, crows, nlat = _maps(nimg, npass)
    rows = (1 + npass) * 4 * nimg
    assert crows == (4 + 2 * npass) * nimg and nlat == (2 + npass) * nimg
    if npass == 2:
        assert crows == 8 * nimg and nlat == 4 * nimg
    else:
        assert crows == 6 * nimg
    assert len(set(lsel)) == nlat and all(_canon_latent(x, nimg) == x for x in lsel)            # distinct, canonical latents
    assert all(0 <= x < nlat for x in cmap) and set(cmap) == set(range(nlat))
    compact_key = [(lsel[cmap[r]], cctx[r]) for r in range(crows)]
    assert len(set(compact_key)) == crows                                                        # no compact row repeats another
    for r in range(rows):
        q, k = divmod(r, 4)
        im = q % nimg
        key = (_canon_latent(2 * q + k % 2, nimg), 4 * im + k)
        assert 0 <= omap[r] < crows and compact_key[omap[r]] == key, (r, omap[r])
    assert set(omap) == set(range(crows))                                                        # every compact row serves someone
    for im in range(nimg):
        o1 = omap[4 * im + 1]
        assert omap.count(o1) == 1                                                               # O1 is never shared
        for k in (0, 2):                                                                         # O0 / O2 serve every pass
            assert omap.count(omap[4 * im + k]) == 1 + npass
        for p in range(1, npass + 1):
            q = p * nimg + im
            assert omap[4 * q + 2] == omap[4 * im + 2]                                           # the pass's pair source is O2 of its image
            assert omap[4 * q] == omap[4 * im]
            assert omap.count(omap[4 * q + 1]) == 1 and omap.count(omap[4 * q + 3]) == 1


def test_the_documented_example_and_bad_arguments():
    from pnpinversion_amd import _capi
    lib = _capi.load_library()
    lsel, cmap, cctx, omap, crows, nlat = _maps(1, 2)
    assert omap == [0, 1, 2, 3, 0, 4, 2, 5, 0, 6, 2, 7]
    assert cmap == [0, 1, 0, 1, 2, 2, 3, 3] and cctx == [0, 1, 2, 3, 1, 3, 1, 3] and lsel == [0, 1, 3, 5]
    assert lib.pnpi_src_share_maps(0, 2, None, None, None, None, None, None) != 0
    assert lib.pnpi_src_share_maps(1, 0, None, None, None, None, None, None) != 0
    n = C.c_int(-1)
    assert lib.pnpi_src_share_maps(2, 2, None, None, None, None, C.byref(n), None) == 0 and n.value == 16
