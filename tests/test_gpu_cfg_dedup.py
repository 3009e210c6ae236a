"""The CFG-duplicated rows' shared UNet prefix, once per latent (tuning "cfg_dedup", csrc/api_graph.inc unet_fwd / transformer_fwd).

In the CFG loops every latent feeds two UNet rows (its unconditional and its conditional one).  Up to the first cross-attention the
UNet reads no text, so conv_in, down_res[0][0] and the first half of down_attn[0][0] run once per distinct latent and are expanded
to the rows of the launch (three fp16 row gathers); at a step where block 0's self-attention redirects rows (self-replace) the prefix
ends behind the ResNet instead.

cfg_dedup = 2 pins every compact GEMM to the tile / split-K of its full-row form: per-element accumulation order does not depend on
which tile owns the element, GroupNorm partial sums stay image-aligned, attention and the norms are per row -- so the bar against
cfg_dedup = 0 is BIT-IDENTITY, here for every loop layout: [unc_src, unc_tgt, cond_src, cond_tgt] x two passes (pnpi_direct_edit,
24 rows of 12 latents), the pruned schedule (map [1, 0, 1] per image), a P = 1 CFG loop (pnpi_ddim_invert_cfg) and a loop without a
map (pnpi_ddim_invert: no compact launch at all, counter unet_dedup_prefix_rows stays 0).

Two images with different latents, different prompt pairs and random per-row contexts: a row mix-up cannot hide behind equal rows.
SMALL64: 4096 level-0 tokens > self_replace_max_tokens, the long prefix at every step.  TINY16: 256 level-0 tokens, so step 0 (inside
the self-replace window of 0.6 x 3 steps) takes the short prefix and steps 1, 2 the long one -- one loop switches between them.
LocalBlend needs 64 x 64 latents, so the TINY16 controllers are Refine + Reweight only.

cfg_dedup = 1 (free tile choice): at these narrow widths no launch is in the measured tile table and the cost model picks the same
tile and split-K for the compact and the full row count, so the comparison against the oracle collapses to bit-identity as well
(measured: equal at SMALL64 and TINY16) and is asserted as such below.  At the SD-1.x width it does not collapse: conv_in's compact
launch takes another tile and the edited panel moves by up to 2 / 255 (profiles/cfg_dedup_ab.json), which is why the default is 2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SMALL64, TINY16  # noqa: E402
from pnpinversion_amd.p2p import attention_control as ac  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

STEPS = 3
PROMPTS = [("a photograph of a mountain", "a watercolor photograph of a snowy mountain", "mountain", "snowy"),
           ("a cat sitting on a wooden chair", "a small cat sitting on a old wooden chair", "cat", "small")]


class Case:
    def __init__(self, cfg, blend):
        self.cfg = cfg
        self.pipe = NativePipeline(cfg, max_unet_rows=24, max_vae_images=1, text_encoder=SyntheticTextEncoder(cfg.cross_dim, seed=7))
        self.pipe.load_state_dict(weights.unet_state_dict(cfg, 2), weights.vae_state_dict(cfg, 2))
        self.eng = self.pipe.engine
        self.pipe.scheduler.set_timesteps(STEPS)
        self.ts = self.pipe.scheduler.timesteps.numpy()
        S = cfg.sample_size
        self.z0 = torch.randn(2, 4, S, S, generator=torch.Generator().manual_seed(11))
        self.ctx = torch.stack([weights.synth_context(cfg, 4, seed=40 + i) for i in range(2)])      # [2 images][4 rows][77][X], all different
        self.ctrls = []
        for src, tgt, bw, ew in PROMPTS:
            c = ac.make_controller(self.pipe, [src, tgt], False, {"default_": 0.4}, 0.6, ((bw,), (bw,)) if blend else None,
                                   {"words": (ew,), "values": (2,)}, num_ddim_steps=STEPS)
            self.ctrls.append(c.tables())
        with self.eng.tuning(cfg_dedup=0):
            self.traj = self.eng.ddim_invert(self.z0, self.ctx[:, 2], self.ts).clone()      # [STEPS + 1][2][4][S][S]
        self.memo = {}

    def direct_edit(self, mode, fresh=False):
        """(noise_loss, latents, rows through the compact prefix) of the two-pass lock-step edit of both images under cfg_dedup = mode"""
        if fresh or mode not in self.memo:
            with self.eng.tuning(cfg_dedup=mode):
                self.eng.reset_counters()
                nl, lats = self.eng.direct_edit(self.traj, self.ctx, [None, self.ctrls], self.ts, 7.5)
                got = (nl.clone(), lats.clone(), self.eng.counters()["unet_dedup_prefix_rows"])
            if fresh:
                return got
            self.memo[mode] = got
        return self.memo[mode]

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module")
def small64():
    c = Case(SMALL64, blend=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny16():
    c = Case(TINY16, blend=False)
    yield c
    c.close()


def _check_direct_edit(case, mode):
    nl0, lat0, n0 = case.direct_edit(0)
    nl1, lat1, n1 = case.direct_edit(mode)
    assert torch.isfinite(nl0).all() and torch.isfinite(lat0).all()
    assert n0 == 0 and n1 == STEPS * 12, (n0, n1)              # 24 rows (offset pass + two edit passes, two images) of 12 distinct latents per step
    assert not torch.equal(lat0[1, 0], lat0[1, 1]) and not torch.equal(lat0[0], lat0[1])       # images and passes differ
    assert not torch.equal(lat0[1, 0, 0], lat0[1, 0, 1])                                        # so do source and target
    assert torch.equal(nl1, nl0), (nl1 - nl0).abs().max().item()
    assert torch.equal(lat1, lat0), (lat1 - lat0).abs().max().item()


def test_pinned_prefix_is_bit_identical_small64(small64):
    """1. pnpi_direct_edit, two images, Refine + Reweight + LocalBlend, 3 steps, the long prefix: cfg_dedup = 2 against 0"""
    _check_direct_edit(small64, 2)


def test_fallback_prefix_and_the_switch_between_steps_tiny16(tiny16):
    """2. TINY16: step 0 self-replaces at level 0 (short prefix, expanded behind the ResNet), steps 1 and 2 take the long one"""
    _check_direct_edit(tiny16, 2)


def test_other_row_maps(small64):
    """3. the pruned schedule (map [1, 0, 1], U = 2 of 3 per image), a P = 1 CFG loop and a loop without a map"""
    eng, got = small64.eng, {}
    for mode in (0, 2):
        with eng.tuning(cfg_dedup=mode):
            eng.reset_counters()
            pr = eng.direct_edit_pruned(small64.traj, small64.ctx, small64.ctrls, small64.ts, 7.5).clone()
            n_pr = eng.counters()["unet_dedup_prefix_rows"]
            eng.reset_counters()
            inv = eng.ddim_invert_cfg(small64.z0, small64.ctx[:, 0], small64.ctx[:, 2], small64.ts, 2.5).clone()
            n_inv = eng.counters()["unet_dedup_prefix_rows"]
            eng.reset_counters()
            plain = eng.ddim_invert(small64.z0, small64.ctx[:, 2], small64.ts).clone()
            c = eng.counters()
            got[mode] = (pr, inv, plain, n_pr, n_inv, c["unet_dedup_prefix_rows"], c["unet_sample_forwards"])
    assert got[0][3:] == (0, 0, 0, 2 * STEPS), got[0][3:]
    assert got[2][3:] == (STEPS * 4, STEPS * 2, 0, 2 * STEPS), got[2][3:]        # 6 rows of 4 latents; 4 rows of 2; no map, nothing compact
    for a, b in zip(got[0][:3], got[2][:3]):
        assert torch.isfinite(a).all() and torch.equal(a, b), (a - b).abs().max().item()
    assert torch.equal(got[2][2], small64.traj)
    assert not torch.equal(got[0][0][0, 1], got[0][0][1, 1])


@pytest.mark.parametrize("which", ["small64", "tiny16"])
def test_free_tile_choice(which, request):
    """4. cfg_dedup = 1: the cost model picks the same tile and split-K for the compact and the full row count at these widths (see the
    module docstring), so the bar is bit-identity here too"""
    _check_direct_edit(request.getfixturevalue(which), 1)


def test_knob_on_a_live_context(tiny16):
    """5. 0 -> 1 -> 0 between loops of one context: no arena overflow (the sizing run covers both paths), equal settings give equal
    results; values outside 0 .. 2 are rejected and leave the setting alone"""
    a = tiny16.direct_edit(0, fresh=True)
    b = tiny16.direct_edit(1, fresh=True)
    c = tiny16.direct_edit(0, fresh=True)
    assert a[2] == 0 and b[2] == STEPS * 12 and c[2] == 0
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert torch.equal(b[1], tiny16.direct_edit(1)[1])
    lib = tiny16.eng.lib
    assert lib.pnpi_set_tuning(b"cfg_dedup", 3) != 0 and lib.pnpi_set_tuning(b"cfg_dedup", -1) != 0
    assert tiny16.direct_edit(1, fresh=True)[2] == STEPS * 12
