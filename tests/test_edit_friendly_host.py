"""Host side of the edit-friendly DDPM inversion + P2P editor (no GPU): controller tables against the reference's
models/edit_friendly_ddm/ptp_classes.py imported live, the library's per-step scalars against torch-CPU fp32 evaluation of the
reference's expressions (bit for bit), and the script's CLI."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pnpinversion_amd import _capi  # noqa: E402
from pnpinversion_amd.edit_friendly_ddm import ptp_classes as pc  # noqa: E402
from pnpinversion_amd.engine import ef_step_scalars  # noqa: E402
from pnpinversion_amd.p2p.scheduler_dev import DDIMSchedulerDev  # noqa: E402
from pnpinversion_amd.text import WordTokenizer  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def load_script():
    """this repository's run_editing_edit_friendly_p2p.py (by path: the reference tree, when on sys.path, has a script of that name)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pnpi_run_editing_edit_friendly_p2p", os.path.join(ROOT, "run_editing_edit_friendly_p2p.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _Model:
    def __init__(self):
        self.tokenizer = WordTokenizer()
        self.device = torch.device("cpu")


def _pairs():
    """the prompt pairs of host_tables.json (the P2P copy's table fixture)"""
    with open(os.path.join(GOLD, "host_tables.json")) as f:
        return [(c["src"], c["tgt"]) for c in json.load(f)]


def _ref_ptp():
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("reference tree not present")
    ref_shim.install()
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    import models.edit_friendly_ddm.ptp_classes as rp
    return rp


@pytest.mark.parametrize("steps", [50, 10])
def test_controller_tables_equal_reference(steps):
    rp = _ref_ptp()
    model = _Model()
    for src, tgt in _pairs():
        same = len(src.split(" ")) == len(tgt.split(" "))
        for kind in (["replace"] if same else []) + ["refine"]:
            mine_cls, ref_cls = (pc.AttentionReplace, rp.AttentionReplace) if kind == "replace" else (pc.AttentionRefine, rp.AttentionRefine)
            try:
                ref = ref_cls([src, tgt], steps, cross_replace_steps=0.4, self_replace_steps=0.6, model=model)
            except Exception as e:           # the reference refuses this pair: so must the product
                with pytest.raises(type(e)):
                    mine_cls([src, tgt], steps, cross_replace_steps=0.4, self_replace_steps=0.6, model=model)
                continue
            mine = mine_cls([src, tgt], steps, cross_replace_steps=0.4, self_replace_steps=0.6, model=model)
            t = mine.tables()
            assert t.self_max_tokens == 256
            assert t.self_range == tuple(ref.num_self_replace)
            assert np.array_equal(t.cross_alpha, ref.cross_replace_alpha.reshape(steps + 1, 77).numpy())
            if kind == "replace":
                assert np.array_equal(t.mapper, ref.mapper[0].numpy())
                assert np.array_equal(t.alphas, np.ones(77, np.float32))
            else:
                assert np.array_equal(mine.mapper.numpy(), ref.mapper.numpy())
                assert np.array_equal(t.alphas, ref.alphas.reshape(-1).numpy())


def sq(x):
    """`x ** 0.5` of a 0-dim fp32 tensor, correctly rounded (as on the GPU the reference runs on).  torch's CPU sqrt goes through a
    vectorised approximation that is 1 ulp off for some operands (e.g. the variance at t = 740 of 50 steps), so only the ** 0.5 is not
    torch-CPU's; every + - * / is."""
    return torch.from_numpy(np.asarray(np.sqrt(np.asarray(x.numpy(), dtype=np.float32))))


@pytest.mark.parametrize("steps", [50, 10])
def test_step_scalars_bit_exact(steps):
    lib = _capi.load_library()
    s = DDIMSchedulerDev(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=False)
    s.set_timesteps(steps)
    ratio = 1000 // steps
    ac = s.alphas_cumprod
    for t in [int(x) for x in s.timesteps]:
        for eta in (1, 0.5, 0.83):
            ab_t = ac[t]
            ab_p = ac[t - ratio] if t - ratio >= 0 else s.final_alpha_cumprod
            var = ((1 - ab_p) / (1 - ab_t)) * (1 - ab_t / ab_p)               # get_variance, inversion_utils.py:91-98
            ref = torch.stack([sq(ab_t), sq(1 - ab_t), sq(ab_p), sq(1 - ab_p - eta * var), eta * sq(var), var])
            got = ef_step_scalars(lib, ac.numpy(), float(s.final_alpha_cumprod), t, ratio, eta)
            assert np.array_equal(got.view(np.uint32), ref.numpy().astype(np.float32).view(np.uint32)), (t, eta, got, ref)
            if t == 0:
                assert got[5] == 0.0 and got[4] == 0.0


def test_cli_flags_and_controller_choice():
    ef = load_script()
    a = ef.parse_args(["--data_path", "d", "--output_path", "o", "--edit_category_list", "0", "3", "--rerun_exist_images",
                       "--synthetic_weights"])
    assert a.data_path == "d" and a.output_path == "o" and a.edit_category_list == ["0", "3"] and a.rerun_exist_images
    assert a.edit_method_list == ["edit-friendly-inversion+p2p"] and a.batch_size == 1
    assert ef.image_save_paths == {"edit-friendly-inversion+p2p": "edit-friendly-inversion+p2p"}
    assert (ef.NUM_DDIM_STEPS, ef.ETA, ef.SKIP) == (50, 1, 12)
    with pytest.raises(SystemExit):
        ef.parse_args(["--edit_method_list", "ddim+p2p", "--synthetic_weights"])
    with pytest.raises(NotImplementedError):
        ef.edit_image_EF("ddim+p2p", "x.png", "a", "b")
    assert ef.controller_class("a cat on a chair", "a dog on a chair") is pc.AttentionReplace
    assert ef.controller_class("a cat on a chair", "a big dog on a chair") is pc.AttentionRefine


def test_local_blend_and_eta_zero_refused():
    with pytest.raises(NotImplementedError):
        pc.LocalBlend(["a cat", "a dog"], [["cat"], ["dog"]], tokenizer=WordTokenizer())
    with pytest.raises(NotImplementedError):
        pc.AttentionReplace(["a cat", "a dog"], 50, 0.4, 0.6, local_blend=object(), model=_Model())
    from pnpinversion_amd.edit_friendly_ddm import inversion_utils as iu
    with pytest.raises(NotImplementedError):
        iu.inversion_forward_process(None, torch.zeros(1, 4, 8, 8), etas=0)
