"""No call leaves anything behind for the next one (csrc/api_graph.inc: UNetCall, UNetFlight).

What belongs to ONE UNet forward -- the text K/V cache switch, row sharing and its GEMM pin, the Plug-and-Play injection, the recording
switch, the block counters -- travels in that forward's call record and lives on its stack.  The property pinned here: whatever ran on a
context before, a plain pnpi_unet_forward(latents, rows = 4, t, context) on it gives the bits and the per-launch (tile configuration,
split-K) sequence of the same call on a fresh context.

PROBE is that call; `fresh` runs it on a context of its own.  Every test runs one sequence on a second context (`used`, shared by the
tests: what one sequence leaves behind would show in every later probe too), then the probe.  pnpi_unet_context_grad has a context of
its own: the activation tape stays with a context for good.  TINY16, synthetic seeded weights, two-step loops."""
import csv
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi, weights  # noqa: E402
from pnpinversion_amd import instructpix2pix as ip  # noqa: E402
from pnpinversion_amd.config import TINY16  # noqa: E402
from pnpinversion_amd.p2p import attention_control as ac  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

CFG = TINY16
S = CFG.sample_size
STEPS = 2
T = 481
GS = 7.5


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


LAT = randn(3, 4, 4, S, S)                                # the probe's four rows: all different
CTX = weights.synth_context(CFG, 4, seed=31)
CTX4 = weights.synth_context(CFG, 4, seed=40)[None]       # [1 image][unc_src, unc_tgt, cond_src, cond_tgt]
CTX3 = weights.synth_context(CFG, 3, seed=50)[None]       # [1 image][3 rows] of the three-row editors


def make_pipe():
    p = NativePipeline(CFG, max_unet_rows=12, max_vae_images=1, text_encoder=SyntheticTextEncoder(CFG.cross_dim, seed=7))
    p.load_state_dict(weights.unet_state_dict(CFG, 2), weights.vae_state_dict(CFG, 2))
    p.scheduler.set_timesteps(STEPS)
    return p


def probe(eng, dump):
    """(eps, [(cfg, split) per launch]) of the probe call, the sequence read from the per-launch profile dump"""
    os.environ["PNPI_PROFILE_DUMP"] = dump
    try:
        eng.profile_begin()
        eps = eng.unet(LAT, T, CTX).clone()
        eng.profile_end()
    finally:
        del os.environ["PNPI_PROFILE_DUMP"]
    with open(dump) as f:
        seq = [(int(r["cfg"]), int(r["split"])) for r in csv.DictReader(f)]
    return eps, seq


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return str(tmp_path_factory.mktemp("call_state") / "launches.csv")


@pytest.fixture(scope="module")
def fresh(dump):
    p = make_pipe()
    try:
        eps0, seq0 = probe(p.engine, dump)
    finally:
        p.engine.close()
    assert torch.isfinite(eps0).all() and not torch.equal(eps0[0], eps0[1])
    assert len(seq0) > 100 and any(c >= 0 for c, _ in seq0)      # the GEMM launches carry their configuration
    return eps0, seq0


@pytest.fixture(scope="module")
def used():
    p = make_pipe()
    p.ts = p.scheduler.timesteps.numpy()
    p.traj = p.engine.ddim_invert(randn(11, 1, 4, S, S), CTX4[:, 2], p.ts).clone()      # [STEPS + 1][1][4][S][S]
    yield p
    p.engine.close()


def same_as_fresh(eng, fresh, dump):
    eps, seq = probe(eng, dump)
    assert seq == fresh[1], [(i, a, b) for i, (a, b) in enumerate(zip(seq, fresh[1])) if a != b][:8]
    assert torch.equal(eps, fresh[0]), (eps - fresh[0]).abs().max().item()


def refine(pipe):
    c = ac.make_controller(pipe, ["a cat sitting on a wooden chair", "a small cat sitting on a old wooden chair"], False, {"default_": 0.4}, 0.6,
                           None, {"words": ("small",), "values": (2,)}, num_ddim_steps=STEPS)
    return [c.tables()]


def direct_edit(p, share, ts=None, passes=None):
    eng = p.engine
    with eng.tuning(src_share=share):
        eng.reset_counters()
        eng.direct_edit(p.traj, CTX4, passes or [None, refine(p)], p.ts if ts is None else ts, GS)
        return eng.counters()


@pytest.mark.parametrize("share", [1, 2])
def test_after_direct_edit_with_shared_rows(used, fresh, dump, share):
    assert direct_edit(used, share)["unet_shared_rows"] == 4 * STEPS      # the compact launches ran (pinned under 2)
    same_as_fresh(used.engine, fresh, dump)


def test_after_direct_edit_that_fails_at_its_second_step(used, fresh, dump):
    """timesteps[1] out of range: the host-side timestep check refuses step 1's forward after step 0 ran with pinned shared rows"""
    eng = used.engine
    with eng.tuning(src_share=2):
        eng.reset_counters()
        with pytest.raises(_capi.PnpiError, match="timestep out of range") as e:
            eng.direct_edit(used.traj, CTX4, [None, None], [int(used.ts[0]), CFG.n_train_timesteps], GS)
        assert e.value.status == _capi.PNPI_EINVAL and eng.counters()["unet_calls"] == 1
    same_as_fresh(eng, fresh, dump)


def test_after_plug_and_play(used, fresh, dump):
    eng = used.engine
    desc = eng.pnp_desc(STEPS, STEPS, STEPS)                  # both injections at every step
    assert desc.conv_site >= 0 and desc.qk_block_mask != 0
    rows = randn(21, 1, 3, 4, S, S)
    on = eng.unet_pnp(rows, T, CTX3, desc, 1, 1).clone()
    off = eng.unet_pnp(rows, T, CTX3, desc, 0, 0)
    assert torch.isfinite(on).all() and not torch.equal(on, off)       # the injections acted
    same_as_fresh(eng, fresh, dump)
    out = eng.pnp_edit(randn(22, STEPS, 1, 4, S, S), randn(23, 1, 4, S, S), CTX3, desc, used.ts, GS)
    assert torch.isfinite(out).all()
    same_as_fresh(eng, fresh, dump)


def test_after_cached_text_kv(used, fresh, dump):
    eng = used.engine
    eng.text_kv_precompute(CTX)
    eng.reset_counters()
    cached = eng.unet(LAT, T, None)
    assert eng.counters()["unet_sample_forwards_cached_kv"] == 4
    assert torch.equal(cached, fresh[0])                      # the same projections, read from the cache
    same_as_fresh(eng, fresh, dump)                           # and the next forward with a context projects its own again
    eng.unet(LAT, T, None)                                    # the cache is the caller's until a loop takes it
    eng.ddim_invert(randn(11, 4, 4, S, S), CTX, used.ts)      # four rows, like the cache: the loop's projections must not stay behind
    with pytest.raises(_capi.PnpiError, match="pnpi_text_kv_precompute") as e:
        eng.unet(LAT, T, None)
    assert e.value.status == _capi.PNPI_ESTATE
    same_as_fresh(eng, fresh, dump)


def test_after_fractional_timestep(used, fresh, dump):
    eng = used.engine
    frac = eng.unet_t(LAT, T + 0.5, CTX).clone()
    assert torch.isfinite(frac).all() and not torch.equal(frac, fresh[0])
    assert torch.equal(eng.unet_t(LAT, float(T), CTX), fresh[0])          # a whole timestep reproduces pnpi_unet_forward
    same_as_fresh(eng, fresh, dump)


def test_after_context_grad(fresh, dump):
    p = make_pipe()
    try:
        p.ts = p.scheduler.timesteps.numpy()
        p.traj = p.engine.ddim_invert(randn(11, 1, 4, S, S), CTX4[:, 2], p.ts).clone()
        eps, d_ctx = p.engine.unet_context_grad(LAT[:1], T, CTX[:1], torch.ones(1, 4, S, S))
        assert torch.isfinite(d_ctx).all() and d_ctx.abs().max() > 0
        same_as_fresh(p.engine, fresh, dump)
        assert direct_edit(p, 1)["unet_shared_rows"] == 0      # the tape-holding context keeps the full launch
        same_as_fresh(p.engine, fresh, dump)
    finally:
        p.engine.close()


def test_after_instruct_pix2pix_loop():
    """the 8-channel twin: a loop at fractional timesteps (its own sinusoid rows and bias row), and the same forward before and after it"""
    from pnpinversion_amd.config import TINY16_IP2P
    p = NativePipeline(TINY16_IP2P, max_unet_rows=12, max_vae_images=1, text_encoder=SyntheticTextEncoder(CFG.cross_dim, seed=7))
    p.load_state_dict(weights.unet_state_dict(TINY16_IP2P, 2), weights.vae_state_dict(TINY16_IP2P, 2))
    try:
        eng, lat8 = p.engine, randn(5, 4, 8, S, S)
        want = eng.unet_t(lat8, float(T), CTX).clone()
        sched = ip.SigmaSchedule()
        sigmas = sched.get_sigmas(STEPS)
        out = eng.ip2p_edit(randn(6, 1, 4, S, S) * sigmas[0], randn(7, 1, 4, S, S), randn(8, STEPS, 1, 4, S, S), CTX3, ip.step_table(sigmas, sched))
        assert torch.isfinite(out).all()
        assert torch.equal(eng.unet_t(lat8, float(T), CTX), want)
    finally:
        p.engine.close()
