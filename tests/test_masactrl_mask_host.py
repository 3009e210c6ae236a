"""Host side of mask-guided MasaCtrl (no GPU): the MutualSelfAttentionControlMask class and its tables, the refusals, the driver's
--mask_guided flag, the new C-ABI symbols, and the arithmetic the kernel is built on -- ONE class-restricted softmax per query equals the
reference's two masked passes + blend (models/masactrl/masactrl.py:138-193) for binary masks, including the uniform fall-back of an empty
class -- against tests/golden/masactrl_mask_attn.npz (the reference's own class, tools/make_golden_masactrl_mask.py)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def one_pass(q, k, v, mask_s, mask_t, scale):
    """Query i attends to the keys j with mask_s[j] == mask_t[i]; no such key: uniform over all keys.  The foreground pass of the reference
    adds mask_s == 1 to the kept logits (a constant shift); it is kept here so that the comparison can be exact.  For the same reason P V
    runs in the reference's shape -- a batch of two [N, N] x [N, d] products (foreground pass, background pass): the CPU GEMM splits its
    work by the batch's shape, and another split sums the 4096 terms of a row in another order (~1e-8 absolute)."""
    ks, qt = mask_s.reshape(-1).bool(), mask_t.reshape(-1).bool()
    sim = torch.einsum("h i d, h j d -> h i j", q[None], k[None]) * scale
    allowed = (ks[None, :] == qt[:, None])[None]
    logits = torch.where(allowed, sim + qt[None, :, None].to(sim.dtype), torch.full_like(sim, float("-inf")))
    empty = ~allowed.any(-1, keepdim=True)
    logits = torch.where(empty, torch.zeros_like(sim), logits)
    attn = logits.softmax(-1)
    return torch.einsum("h i j, h j d -> h i d", torch.cat([attn, attn]), torch.cat([v[None], v[None]]))[0]


def ulp_distance(a, b):
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = torch.where(ib < 0, -(ib & 0x7fffffff), ib)
    return (ia - ib).abs().max().item()


@pytest.fixture(scope="module")
def attn_fixture():
    n = torch.get_num_threads()
    torch.set_num_threads(8)          # the fixture's thread count (tools/make_golden_masactrl_mask.py): the GEMM's split follows it
    yield np.load(os.path.join(GOLD, "masactrl_mask_attn.npz"))
    torch.set_num_threads(n)


@pytest.mark.parametrize("tag", ["d40", "d80", "d160", "d16"])
def test_one_softmax_per_query_equals_the_references_two_passes(attn_fixture, tag):
    g = attn_fixture
    q, k, v = (torch.from_numpy(g[tag + "_" + n].astype(np.float32)) for n in "qkv")       # [2 (src, tgt), N, d]
    sel, scale = torch.from_numpy(g[tag + "_sel"]), float(g[tag + "_scale"])
    for case in [str(c) for c in g["cases"]]:
        ms, mt = torch.from_numpy(g["%s_%s_mask_s" % (tag, case)]), torch.from_numpy(g["%s_%s_mask_t" % (tag, case)])
        got = one_pass(q[1], k[0], v[0], ms, mt, scale)[sel]
        ref = torch.from_numpy(g["%s_%s_out" % (tag, case)])
        assert torch.isfinite(got).all()
        assert torch.equal(got, ref) or ulp_distance(got, ref) <= 1, (tag, case, ulp_distance(got, ref), (got - ref).abs().max().item())
    # the empty class really is the mean of V, and the fixture's rectangle case discriminates masked from plain mutual self-attention
    ms, mt = g[tag + "_empty_fg_mask_s"], torch.from_numpy(g[tag + "_empty_fg_mask_t"]).reshape(-1).bool()
    assert ms.sum() == 0 and mt.any() and not mt.all()
    fg_rows = mt[sel]
    ref = torch.from_numpy(g[tag + "_empty_fg_out"])
    assert fg_rows.any()
    assert (ref[fg_rows] - v[0].mean(0)).abs().max().item() < 1e-5
    assert np.abs(g[tag + "_rect_out"] - g[tag + "_plain"]).max() >= 10 * 3e-3


def test_class_constructor_and_tables_against_the_fixture():
    from pnpinversion_amd.engine import MasaCtrlMaskTables
    from pnpinversion_amd.masactrl.masactrl import MutualSelfAttentionControl, MutualSelfAttentionControlMask
    g = np.load(os.path.join(GOLD, "e2e_masactrl_mask.npz"))
    ms, mt = torch.from_numpy(g["mask_s"][0]).float(), torch.from_numpy(g["mask_t"][0]).float()
    steps, start_step, start_layer = int(g["steps"]), int(g["start_step"]), int(g["start_layer"])
    # the reference's argument order (masactrl.py:115)
    ed = MutualSelfAttentionControlMask(start_step, start_layer, None, None, steps, ms, mt, None, "SD")
    assert isinstance(ed, MutualSelfAttentionControl)
    assert ed.step_idx == list(range(start_step, steps)) and ed.layer_idx == list(range(start_layer, 16))
    assert ed.mask_s is ms and ed.mask_t is mt
    t = ed.tables()
    assert isinstance(t, MasaCtrlMaskTables)
    assert t.mask_s.dtype == np.uint8 and t.mask_s.shape == (1, 64, 64)
    assert np.array_equal(t.mask_s[0], g["mask_s"][0]) and np.array_equal(t.mask_t[0], g["mask_t"][0])
    d = t.desc()
    plain = MutualSelfAttentionControl(start_step, start_layer, total_steps=steps).tables().desc()
    assert (d.kind, d.masa_start_step, d.masa_start_layer, d.masa_layer_mask, d.masa_n_steps) == \
        (2, plain.masa_start_step, plain.masa_start_layer, plain.masa_layer_mask, plain.masa_n_steps) == (2, start_step, start_layer, 0, 0)
    lists = MutualSelfAttentionControlMask(layer_idx=[10, 12], step_idx=[1, 3], total_steps=steps, mask_s=ms, mask_t=mt).tables().desc()
    assert lists.masa_layer_mask == (1 << 31) | (1 << 10) | (1 << 12) and lists.masa_n_steps == 4


def test_mask_save_dir_writes_the_two_pngs(tmp_path):
    from PIL import Image
    from pnpinversion_amd.masactrl.masactrl import MutualSelfAttentionControlMask
    ms = torch.zeros(8, 8)
    ms[2:5, 1:4] = 1
    mt = torch.zeros(8, 8)
    mt[0, 0] = 1
    MutualSelfAttentionControlMask(mask_s=ms, mask_t=mt, mask_save_dir=str(tmp_path / "masks"))
    for name, m in (("mask_s.png", ms), ("mask_t.png", mt)):
        img = np.array(Image.open(str(tmp_path / "masks" / name)))
        assert img.shape == (8, 8, 3) and np.array_equal(img[:, :, 0], (m.numpy() * 255).astype(np.uint8))


def test_refusals():
    from pnpinversion_amd.engine import masa_masks_u8
    from pnpinversion_amd.masactrl.masactrl import MutualSelfAttentionControlMask
    ok = torch.zeros(16, 16)
    ok[3:9, 2:7] = 1
    with pytest.raises(ValueError, match="MutualSelfAttentionControl"):          # a missing mask names the plain class
        MutualSelfAttentionControlMask(mask_s=ok, mask_t=None)
    with pytest.raises(ValueError, match="MutualSelfAttentionControl"):
        MutualSelfAttentionControlMask()
    with pytest.raises(ValueError, match="binary"):
        MutualSelfAttentionControlMask(mask_s=ok * 0.5, mask_t=ok)
    with pytest.raises(ValueError, match="binary"):
        MutualSelfAttentionControlMask(mask_s=ok, mask_t=ok * 255)
    with pytest.raises(ValueError, match="same shape"):
        MutualSelfAttentionControlMask(mask_s=ok, mask_t=torch.zeros(16, 8))
    with pytest.raises(ValueError, match="shape"):
        masa_masks_u8(torch.zeros(16), torch.zeros(16))
    s, t = masa_masks_u8(np.ones((2, 4, 6)), np.zeros((2, 4, 6), bool))
    assert s.shape == t.shape == (2, 4, 6) and s.dtype == np.uint8 and s.flags["C_CONTIGUOUS"]


def test_foreign_editor_objects_are_read_off_their_attributes():
    """an object with the attributes of the reference's class and no .tables() (models/masactrl/masactrl.py:129-131)"""
    from pnpinversion_amd.engine import MasaCtrlMaskTables, MasaCtrlTables
    from pnpinversion_amd.masactrl.masactrl_utils import adapt_foreign_editor
    m = torch.zeros(8, 8)
    m[1:4, 2:6] = 1
    Foreign = type("MutualSelfAttentionControlMask", (), {})
    f = Foreign()
    f.layer_idx, f.step_idx, f.mask_s, f.mask_t, f.cur_step = [10, 11], [4, 5, 6], m, 1 - m, 0
    a = adapt_foreign_editor(f)
    t = a.tables()
    assert isinstance(t, MasaCtrlMaskTables) and np.array_equal(t.mask_t[0], (1 - m).numpy().astype(np.uint8))
    assert t.desc().masa_layer_mask == (1 << 31) | (1 << 10) | (1 << 11) and t.desc().masa_n_steps == 7
    a.cur_step += 3
    assert f.cur_step == 3                         # bookkeeping stays on the wrapped object
    f.mask_s = f.mask_t = None                     # the reference then runs plain mutual self-attention
    assert type(adapt_foreign_editor(f).tables()) is MasaCtrlTables
    f.mask_t = m
    with pytest.raises(ValueError, match="only one"):
        adapt_foreign_editor(f)
    with pytest.raises(TypeError, match="no kernel descriptor"):
        adapt_foreign_editor(type("MutualSelfAttentionControlMaskAuto", (), {})())


def load_driver():
    """this repository's run_editing_masactrl.py, whatever else of that name an earlier test (the oracle's reference shim) left importable"""
    import importlib
    import sys
    names = ("run_editing_masactrl", "run_editing_p2p")
    saved_path, saved = list(sys.path), {n: sys.modules.get(n) for n in names}
    try:
        for n, m in saved.items():
            if m is not None and os.path.dirname(os.path.abspath(getattr(m, "__file__", "") or "")) != ROOT:
                del sys.modules[n]
        sys.path.insert(0, ROOT)
        return importlib.import_module("run_editing_masactrl")
    finally:
        sys.path[:] = saved_path
        for n, m in saved.items():
            if m is not None:
                sys.modules[n] = m


def test_cli_flag_and_output_paths():
    drv = load_driver()
    assert os.path.dirname(os.path.abspath(drv.__file__)) == ROOT
    ap = drv.build_parser()
    off = ap.parse_args(["--synthetic_weights"])
    on = ap.parse_args(["--synthetic_weights", "--mask_guided"])
    assert off.mask_guided is False and on.mask_guided is True
    for m in ("ddim+masactrl", "directinversion+masactrl"):
        assert drv.output_dir("output", m, False) == os.path.join("output", m)          # the reference's tree, unchanged
        assert drv.output_dir("output", m, True) == os.path.join("output", m + "-mask")
    # the PIE-Bench mask at the latent size: mask_decode (border forced to 1), then PIL NEAREST (pixel 8 i + 4 of the 512 grid)
    rle = []
    for r in range(100, 164):
        rle += [r * 512 + 44, 281]
    lm = drv.latent_mask(rle, 64)
    full = drv.mask_decode(rle)
    assert lm.shape == (64, 64) and lm.dtype == np.uint8 and set(np.unique(lm)) <= {0, 1}
    assert np.array_equal(lm, full[4::8, 4::8].astype(np.uint8))
    assert lm[13:20, 6:40].all() and not lm[30:, 1:-1].any()


def test_new_symbols_in_header_and_bindings():
    from pnpinversion_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "pnpi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("pnpi_masa_set_masks", "pnpi_op_attention_masked", "pnpi_op_masa_mask_level", "pnpi_masa_get_level_masks"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _capi.SYMBOLS
    m = re.search(r"pnpi_masa_set_masks\s*\(([^)]*)\)", hdr).group(1)
    assert [a.split()[-1].lstrip("*") for a in m.split(",")] == ["ctx", "mask_s_u8_host", "mask_t_u8_host", "nimg", "h", "w"]
    assert len(_capi.SYMBOLS["pnpi_masa_set_masks"][1]) == 6
    assert len(_capi.SYMBOLS["pnpi_op_attention_masked"][1]) == len(_capi.SYMBOLS["pnpi_op_attention"][1]) + 3
    # pnpi_ctrl_desc keeps its layout: the masks do not travel in the descriptor
    assert [f for f, _ in _capi.CtrlDesc._fields_][-3:] == ["masa_layer_mask", "masa_n_steps", "masa_step_on_host"]
