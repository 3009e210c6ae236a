"""Free tile choice as the default of the lock-step step (tuning "src_share" = 1 and "cfg_dedup" = 1: every GEMM of the 8-row launch and of
its 4-latent prefix is planned on the rows it launches, csrc/tile_table.inc) against the pinned form (2 / 2: planned as the 12 logical
rows) at full SD-1.x width.  Free choice is not bit-identical to the pinned path -- other tiles and split-K factors sum in another
order -- so the bar is the reference: tests/golden/e2e_sd1.npz, the reference's own fp32 run that tests/test_gpu_headline_parity.py uses,
with that test's controller (Refine + Reweight + LocalBlend) on the edit pass.  One 2-step pnpi_direct_edit per mode, shared by the tests.

(a) the offsets of step 0 are one 8-row UNet forward on 4 latents with the lock-step row maps (the target minus the DDIM step from that
    forward's prediction): mode 1's rel-L2 error may exceed mode 2's by at most MARGIN_A, the spread (max - min) of that error over
    fourteen whole-forward tile choices (every tile family without split-K, five with), profiles/rowfit_ab.json "error_spread":
    8.436e-3 ... 8.682e-3.  Measured: mode 2 8.547e-3, mode 1 8.523e-3 (8.562e-3 before the new table rows).
(b) per step, the offsets' error (as a share of the whole offset tensor's norm, the quantity the headline test bounds: a later step's own
    offsets are too small to carry a relative error) and the final latents' error: under the bars the headline test holds
    this fixture to (1.5e-2) and at most 1.25 x the pinned path's (the margin tests/test_gpu_src_share.py gives mode 1: independent
    fp16 roundings of the same math); the source branches of the reconstruction and the edit pass bit-equal.
(c) the same edit twice: bit-equal.
(d) SMALL64 (where mode 1 and mode 0 choose different tiles): a context that holds an activation tape keeps the full 12-row launch; under
    mode 1 that launch is configured as the compact one, so the context gives the bits it gave before the tape, for both cfg_dedup forms."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SD1, SMALL64  # noqa: E402
from pnpinversion_amd.p2p import attention_control as ac  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MARGIN_A = 2.46e-4          # spread of the step-0 offset error over the sweep's tile choices (profiles/rowfit_ab.json)
BAR, MARGIN = 1.5e-2, 1.25  # tests/test_gpu_headline_parity.py on this fixture; tests/test_gpu_src_share.py for mode 1 against the pinned path


def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def runs():
    g = np.load(os.path.join(GOLD, "e2e_sd1.npz"))
    steps, seed = int(g["steps"]), int(g["weight_seed"])
    pipe = NativePipeline(SD1, max_unet_rows=12, max_vae_images=1, text_encoder=SyntheticTextEncoder(SD1.cross_dim, seed=7))
    pipe.load_state_dict(weights.unet_state_dict(SD1, seed), weights.vae_state_dict(SD1, seed))
    eng = pipe.engine
    pipe.scheduler.set_timesteps(steps)
    ts = pipe.scheduler.timesteps.numpy()
    ctx, x_stars = torch.from_numpy(g["context"]).float(), torch.from_numpy(g["x_stars"])
    w0, w1 = [str(x) for x in g["blend"]]
    ctrl = ac.make_controller(pipe, [str(g["src"]), str(g["tgt"])], bool(g["is_replace"]), {"default_": 0.4}, 0.6, ((w0,), (w1,)),
                              {"words": (w1,), "values": (2,)}, num_ddim_steps=steps)
    got = []
    try:
        for mode in (2, 1, 1):
            with eng.tuning(src_share=mode, cfg_dedup=mode):
                eng.reset_counters()
                nl, lats = eng.direct_edit(x_stars, ctx[None], [None, [ctrl.tables()]], ts, 7.5)
                c = eng.counters()
            assert c["unet_shared_rows"] == 4 * steps and c["unet_dedup_prefix_rows"] == 6 * steps, c      # 8 rows on 4 latents serve 12 on 6
            got.append((nl.cpu(), lats.cpu()))
    finally:
        eng.close()
    return {"g": g, "steps": steps, "x_stars": x_stars, 2: got[0], 1: got[1], "again": got[2]}


def test_one_eight_row_forward_against_the_fixture(runs):
    g = runs["g"]
    e2, e1 = rel(runs[2][0][0, 0], g["noise_loss"][0]), rel(runs[1][0][0, 0], g["noise_loss"][0])
    print("step-0 offsets (one 8-row forward on 4 latents) rel-L2 against the fp32 fixture: mode 2 %.4e, mode 1 %.4e, margin %.3e" % (e2, e1, MARGIN_A))
    assert torch.isfinite(runs[1][0]).all() and e2 < BAR
    assert e1 <= e2 + MARGIN_A, (e1, e2)


def test_two_step_edit_within_the_bars_of_mode_one(runs):
    g, steps = runs["g"], runs["steps"]
    ref_nl = torch.from_numpy(g["noise_loss"])

    def errors(mode):
        nl, lats = runs[mode]
        off = [((nl[i, 0] - ref_nl[i]).norm() / ref_nl.norm()).item() for i in range(steps)]
        return off + [rel(lats[0, 0][1], g["reconstruct_latent"][1]), rel(lats[1, 0][1], torch.from_numpy(g["edited_latents"])[1])]

    e2, e1 = errors(2), errors(1)
    print("per-step offsets, reconstruction, edit against the fixture: mode 2 %s, mode 1 %s" % (["%.3e" % v for v in e2], ["%.3e" % v for v in e1]))
    nl, lats = runs[1]
    assert torch.isfinite(nl).all() and torch.isfinite(lats).all()
    for a, b in zip(e1, e2):
        assert a < BAR and a <= MARGIN * b, (e1, e2)
    assert torch.equal(lats[0, 0][0], lats[1, 0][0])           # the source branches are one launch row: bit-equal
    assert not torch.equal(lats[0, 0][1], lats[1, 0][1])       # the controller acts on the edit pass


def test_the_same_edit_twice_is_bit_equal(runs):
    assert torch.equal(runs[1][0], runs["again"][0]) and torch.equal(runs[1][1], runs["again"][1])


@pytest.mark.parametrize("dedup", [1, 2])
def test_a_context_with_a_tape_gives_the_bits_it_gave_without(dedup):
    cfg, steps = SMALL64, 3
    pipe = NativePipeline(cfg, max_unet_rows=12, max_vae_images=1, text_encoder=SyntheticTextEncoder(cfg.cross_dim, seed=7))
    pipe.load_state_dict(weights.unet_state_dict(cfg, 2), weights.vae_state_dict(cfg, 2))
    eng, S = pipe.engine, cfg.sample_size
    pipe.scheduler.set_timesteps(steps)
    ts = pipe.scheduler.timesteps.numpy()
    z0 = torch.randn(1, 4, S, S, generator=torch.Generator().manual_seed(11))
    ctx = weights.synth_context(cfg, 4, seed=40)[None]
    c = ac.make_controller(pipe, ["a photograph of a mountain", "a watercolor photograph of a snowy mountain"], False, {"default_": 0.4}, 0.6,
                           (("mountain",), ("mountain",)), {"words": ("snowy",), "values": (2,)}, num_ddim_steps=steps)

    def run(share):
        with eng.tuning(src_share=share, cfg_dedup=dedup):
            eng.reset_counters()
            nl, lats = eng.direct_edit(traj, ctx, [None, [c.tables()]], ts, 7.5)
            return nl.cpu(), lats.cpu(), eng.counters()["unet_shared_rows"]

    try:
        traj = eng.ddim_invert(z0, ctx[:, 2], ts).clone()
        free, pinned = run(1), run(2)
        eng.unet_context_grad(z0, int(ts[0]), ctx[0, 2:3], torch.ones(1, 4, S, S))      # the context holds a tape from here on
        free_t, pinned_t = run(1), run(2)
    finally:
        eng.close()
    assert free[2] == pinned[2] == 4 * steps and free_t[2] == pinned_t[2] == 0          # compact before, the full launch after
    print("SMALL64: mode 1 %s mode 2" % ("equals" if torch.equal(free[1], pinned[1]) else "differs from"))
    assert torch.equal(pinned_t[0], pinned[0]) and torch.equal(pinned_t[1], pinned[1])
    assert torch.equal(free_t[0], free[0]) and torch.equal(free_t[1], free[1]), (free_t[1] - free[1]).abs().max().item()
