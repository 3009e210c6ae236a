"""pnpinversion_amd/sweep.py, what the eight run_editing_*.py drivers share (no GPU): the parsers against the defaults recorded before the
drivers were rewritten on it, the work plan (category filter, then round-robin, then skip-if-exists) against lists written out by hand,
the drivers' plan_work adapters, the start-up / shutdown order of sweep.session, and that no driver keeps a start-up path of its own."""
import argparse
import importlib.util
import json
import os
import sys
import types

import pytest

from pnpinversion_amd import sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DRIVERS = ("run_editing_blended_latent_diffusion", "run_editing_edit_friendly_p2p", "run_editing_instructdiffusion",
           "run_editing_instructpix2pix", "run_editing_masactrl", "run_editing_p2p", "run_editing_p2p_one_image", "run_editing_pnp")


def load_script(name):
    """this repository's script of that name, by path (the reference tree, when an earlier test put it on sys.path, has scripts of the same
    names); run_editing_p2p_one_image.py imports run_editing_p2p by name, so that name means this repository's copy while it loads"""
    def by_path(n):
        spec = importlib.util.spec_from_file_location("pnpi_sweep_test_" + n, os.path.join(ROOT, n + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m
    if name != "run_editing_p2p_one_image":
        return by_path(name)
    saved = sys.modules.get("run_editing_p2p")
    sys.modules["run_editing_p2p"] = by_path("run_editing_p2p")
    try:
        return by_path(name)
    finally:
        if saved is None:
            del sys.modules["run_editing_p2p"]
        else:
            sys.modules["run_editing_p2p"] = saved


@pytest.fixture(scope="module")
def scripts():
    return {name: load_script(name) for name in DRIVERS}


# ---------------------------------------------------------------------------------------------- CLI defaults
@pytest.mark.parametrize("name", DRIVERS)
def test_cli_defaults_are_the_recorded_ones(scripts, name):
    """tests/golden/sweep_cli_defaults.json: vars(parse_args([])) of every driver, recorded on the commit before sweep.py"""
    with open(os.path.join(GOLD, "sweep_cli_defaults.json")) as f:
        want = json.load(f)[name]
    m = scripts[name]
    got = vars(m.build_parser().parse_args([]) if name == "run_editing_masactrl" else m.parse_args([]))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


# ---------------------------------------------------------------------------------------------- the work plan
CATEGORIES = ["0", "2"]


def _items():
    """7 items over 3 categories (i % 3); item 2's prompts carry [brackets]"""
    return {"%03d" % i: {"editing_type_id": str(i % 3), "image_path": "c%d/%03d.jpg" % (i % 3, i), "mask": [5, 3], "blended_word": "",
                         "original_prompt": "a [blue] bird" if i == 2 else "a bird %d" % i,
                         "editing_prompt": "a [red] bird" if i == 2 else "a dog %d" % i, "editing_instruction": "make it %d" % i}
            for i in range(7)}


def _args(tmp_path, rerun=False):
    return argparse.Namespace(data_path=str(tmp_path / "data"), output_path=str(tmp_path / "out"), edit_category_list=CATEGORIES,
                              rerun_exist_images=rerun)


def _image(args, i):
    return os.path.join(args.data_path, "annotation_images", "c%d" % (i % 3), "%03d.jpg" % i)


def _panel(args, folder, i):
    return os.path.join(args.output_path, folder, "annotation_images", "c%d" % (i % 3), "%03d.jpg" % i)


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "w").close()


# categories 0 and 2 keep items 0 2 3 5 6; rank r of W takes every W-th of those from the r-th on; item 3's panel exists for "alpha"
SHARE = {(1, 0): [0, 2, 3, 5, 6],
         (2, 0): [0, 3, 6], (2, 1): [2, 5],
         (3, 0): [0, 5], (3, 1): [2, 6], (3, 2): [3]}
ALPHA = {(1, 0): [0, 2, 5, 6],
         (2, 0): [0, 6], (2, 1): [2, 5],
         (3, 0): [0, 5], (3, 1): [2, 6], (3, 2): []}


def test_plan_filters_shards_then_skips(tmp_path):
    args, items = _args(tmp_path), _items()
    _touch(_panel(args, "alpha", 3))
    assert sweep.clean_prompt("a [red] bird") == "a red bird"
    for (world, rank), share in SHARE.items():
        log = []
        got = sweep.plan(args, items, "alpha", rank, world, log.append)
        assert got == [(items["%03d" % i], _image(args, i), _panel(args, "alpha", i)) for i in ALPHA[world, rank]], (world, rank)
        assert log == (["skip image [%s] with [alpha]" % _image(args, 3)] if 3 in share else []), (world, rank)
        # another method: nothing of it on disk; a folder that is not the method's name (MasaCtrl's -mask runs)
        got = sweep.plan(args, items, "beta-mask", rank, world, log.append, method="beta")
        assert got == [(items["%03d" % i], _image(args, i), _panel(args, "beta-mask", i)) for i in share], (world, rank)
        assert [(item, path) for item, path, _ in got] == sweep.shard(args, items, rank, world)
    for world in (1, 2, 3):                   # the ranks' shares are a partition of the filtered list, in its order
        assert sorted(i for r in range(world) for i in SHARE[world, r]) == SHARE[1, 0]
    _touch(_panel(args, "beta-mask", 5))
    log = []
    assert [p for _, p, _ in sweep.plan(args, items, "beta-mask", 0, 3, log.append, method="beta")] == [_image(args, 0)]
    assert log == ["skip image [%s] with [beta]" % _image(args, 5)]                       # the message names the method, not the folder
    rerun, log = _args(tmp_path, rerun=True), []
    for (world, rank), share in SHARE.items():
        assert [p for _, p, _ in sweep.plan(rerun, items, "alpha", rank, world, log.append)] == [_image(args, i) for i in share]
    assert log == []


ADAPTERS = {      # driver -> (method, the driver's tuple from sweep.plan's (item, image_path, out_path))
    "run_editing_pnp": ("ddim+pnp", lambda it, p, o: (sweep.clean_prompt(it["original_prompt"]), sweep.clean_prompt(it["editing_prompt"]), p, o)),
    "run_editing_instructpix2pix": ("instruct-pix2pix", lambda it, p, o: (it["editing_instruction"], p, o)),
    "run_editing_instructdiffusion": ("instruct-diffusion", lambda it, p, o: (it["editing_instruction"], p, o)),
    "run_editing_blended_latent_diffusion": ("blended-latent-diffusion", lambda it, p, o: (sweep.clean_prompt(it["editing_prompt"]), p, o, it)),
}


@pytest.mark.parametrize("name", sorted(ADAPTERS))
def test_plan_work_adapters(scripts, tmp_path, name):
    method, project = ADAPTERS[name]
    args, items = _args(tmp_path), _items()
    _touch(_panel(args, method, 3))
    for (world, rank), share in SHARE.items():
        log, log_plan = [], []
        got = scripts[name].plan_work(args, items, method, rank, world, log.append)
        assert got == [project(*t) for t in sweep.plan(args, items, method, rank, world, log_plan.append)]
        assert [t[-2 if name.endswith("blended_latent_diffusion") else -1] for t in got] == [_panel(args, method, i) for i in ALPHA[world, rank]]
        assert log == log_plan == (["skip image [%s] with [%s]" % (_image(args, 3), method)] if 3 in share else [])
    pnp = scripts["run_editing_pnp"].plan_work(args, items, "directinversion+pnp", 1, 3, print)
    assert pnp[0][:2] == ("a blue bird", "a red bird")                                    # item 2, brackets stripped


# ---------------------------------------------------------------------------------------------- rank, device and weight start-up
class _Recorder:
    def __init__(self, monkeypatch, capsys):
        import torch
        import pnpinversion_amd.distributed as pd
        self.calls, self.capsys = [], capsys
        note = lambda name, ret=None: lambda *a, **k: (self.calls.append((name, a, k)), ret)[1]          # noqa: E731
        monkeypatch.setattr(torch.cuda, "set_device", note("set_device"))
        monkeypatch.setattr(torch, "distributed", types.SimpleNamespace(
            init_process_group=note("init_process_group"), barrier=note("barrier"), destroy_process_group=note("destroy_process_group")))
        monkeypatch.setattr(pd, "prepare_env", note("prepare_env"))

        def broadcast(engine, src=0, stats=None):
            self.calls.append(("broadcast", (engine,), dict(src=src)))
            stats.update(bytes=5_000_000, ms=2.5, ranks=2)
        monkeypatch.setattr(pd, "broadcast_weights", broadcast)
        self.pipe = types.SimpleNamespace(engine=object(), load_state_dict=note("load"))
        self.load_weights = note("weights", ("unet", "vae", "clip", "tok"))
        self.make_pipeline = note("make_pipeline", self.pipe)
        self.setenv = monkeypatch.setenv

    def run(self, rank, world, local_rank, body=lambda s: None):
        del self.calls[:]
        for k, v in (("RANK", rank), ("WORLD_SIZE", world), ("LOCAL_RANK", local_rank)):
            self.setenv(k, str(v))
        args = argparse.Namespace(model_config="small64")
        with sweep.session(args, {"sd1": "CFG-SD1", "small64": "CFG-SMALL64"}, self.make_pipeline, self.load_weights) as s:
            self.calls.append(("body", (), {}))
            body(s)
        return s, args, self.capsys.readouterr().out


def test_session_call_order(monkeypatch, capsys):
    import torch
    rec = _Recorder(monkeypatch, capsys)
    names = lambda: [c[0] for c in rec.calls]                                              # noqa: E731
    s, args, out = rec.run(0, 1, 0)
    assert names() == ["prepare_env", "set_device", "weights", "make_pipeline", "load", "body"] and out == ""
    assert (s.pipe, s.cfg, s.rank, s.world, s.local_rank, s.device) == (rec.pipe, "CFG-SMALL64", 0, 1, 0, torch.device("cuda", 0))
    s, args, out = rec.run(0, 2, 0)
    assert names() == ["prepare_env", "set_device", "init_process_group", "weights", "make_pipeline", "load", "broadcast", "body", "barrier",
                       "destroy_process_group"]
    by = {c[0]: c for c in rec.calls}
    assert by["init_process_group"][1:] == (("nccl",), dict(device_id=torch.device("cuda", 0)))
    assert by["weights"][1] == (args, "CFG-SMALL64", 0) and by["make_pipeline"][1] == ("CFG-SMALL64", "cuda:0", "tok")
    assert by["load"][1:] == (("unet", "vae"), dict(clip_sd="clip")) and by["broadcast"][1:] == ((rec.pipe.engine,), dict(src=0))
    assert out == "weight arena broadcast over RCCL: 5.0 MB to 2 ranks in 2.5 ms\n"
    s, args, out = rec.run(1, 2, 1)                                                        # rank 1: no load, no report, its own device
    assert names() == ["prepare_env", "set_device", "init_process_group", "weights", "make_pipeline", "broadcast", "body", "barrier",
                       "destroy_process_group"] and out == ""
    by = {c[0]: c for c in rec.calls}
    assert by["set_device"][1] == (1,) and by["make_pipeline"][1][1] == "cuda:1" and by["weights"][1][2] == 1
    assert (s.rank, s.world, s.local_rank, s.device) == (1, 2, 1, torch.device("cuda", 1))

    def fail(s):
        raise KeyError("from the block")
    with pytest.raises(KeyError, match="from the block"):
        rec.run(0, 2, 0, fail)
    assert names()[-2:] == ["broadcast", "body"]                                           # no barrier on the way out of an exception


def test_session_default_weights_are_resolve_weights(monkeypatch, capsys):
    import pnpinversion_amd.checkpoint as ck
    rec = _Recorder(monkeypatch, capsys)
    monkeypatch.setattr(ck, "resolve_weights", rec.load_weights)
    rec.load_weights = None
    rec.run(0, 1, 0)
    assert [c[0] for c in rec.calls] == ["prepare_env", "set_device", "weights", "make_pipeline", "load", "body"]


# ---------------------------------------------------------------------------------------------- one path for every driver
@pytest.mark.parametrize("name", DRIVERS)
def test_no_driver_keeps_its_own_start_up(name):
    with open(os.path.join(ROOT, name + ".py")) as f:
        src = f.read()
    for word in ("init_process_group", "destroy_process_group", "mapping_file.json"):
        assert word not in src, word
    if name not in ("run_editing_p2p_one_image", "run_editing_instructdiffusion"):         # one image, no sweep / its sibling's main
        assert "sweep.session(" in src


def test_sweep_module_imports_no_torch_at_module_level():
    import ast
    with open(sweep.__file__) as f:
        top = [n for n in ast.parse(f.read()).body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name for n in top if isinstance(n, ast.Import) for a in n.names} | {n.module for n in top if isinstance(n, ast.ImportFrom)}
    assert names == {"contextlib", "json", "os", "random", "types", "numpy"}     # torch, and the modules that import it, only inside functions
