"""pnpi_direct_edit with each step's repeated source rows launched once (tuning "src_share", csrc/api_loops.inc).

The lock-step loop's logical rows are [unc_src, unc_tgt, cond_src, cond_tgt] x (offset pass O + npass guidance passes) x nimg.  The
source rows of the guidance passes repeat O's bit for bit (same x_T, same context rows, no controller writes a source row, the same
fp32 add advances every pass's source latent), so the launch holds them once: (4 + 2 npass) nimg rows on (2 + npass) nimg latents, and
eps is expanded to the logical rows behind the UNet (tests/test_src_share_host.py checks the maps on the host).

src_share = 2 configures every GEMM as at the logical row count (tile, split-K, ring depth: launch_igemm's sel_M); per-element
accumulation order does not depend on the row count then, GroupNorm statistics are per image, attention and the norms per row -- so the
bar against src_share = 0 is BIT-IDENTITY of latents_out and noise_loss_out, for every controller kind and both cfg_dedup forms.
src_share = 1 lets the compact launch choose its own tiles: bit-identical where both row counts choose alike, otherwise judged against
the fp32 CPU oracle with the bar and the margin of tests/test_gpu_ff_fold.py (4e-3 rel-L2, 1.25 x the error of src_share = 0).

Two images with different latents, prompts and random per-row contexts: a row mix-up cannot hide behind equal rows.  Four DDIM steps:
the self-replace window (0.6) covers steps 0 - 2, the cross-replace window (0.4) steps 0 - 1, MasaCtrl starts at step 1 / block 2.
TINY16 (256 level-0 tokens: self-replace at level 0, so block 0 redirects rows) and SMALL64 (LocalBlend needs 64 x 64 latents)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sd_oracle  # noqa: E402  (checker only)
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import SMALL64, TINY16  # noqa: E402
from pnpinversion_amd.engine import MasaCtrlTables  # noqa: E402
from pnpinversion_amd.p2p import attention_control as ac  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

STEPS = 4
GS = 7.5
BAR, MARGIN = 4e-3, 1.25          # tests/test_gpu_ff_fold.py (the UNet parity bar of tests/test_gpu_model.py)
PROMPTS = [("a photograph of a mountain", "a watercolor photograph of a snowy mountain", "mountain", "snowy"),
           ("a cat sitting on a wooden chair", "a small cat sitting on a old wooden chair", "cat", "small")]


class Case:
    def __init__(self, cfg, blend):
        self.cfg = cfg
        self.usd = weights.unet_state_dict(cfg, 2)
        self.pipe = NativePipeline(cfg, max_unet_rows=24, max_vae_images=1, text_encoder=SyntheticTextEncoder(cfg.cross_dim, seed=7))
        self.pipe.load_state_dict(self.usd, weights.vae_state_dict(cfg, 2))
        self.eng = self.pipe.engine
        self.pipe.scheduler.set_timesteps(STEPS)
        self.ts = self.pipe.scheduler.timesteps.numpy()
        S = cfg.sample_size
        self.z0 = torch.randn(2, 4, S, S, generator=torch.Generator().manual_seed(11))
        self.ctx = torch.stack([weights.synth_context(cfg, 4, seed=40 + i) for i in range(2)])      # [2 images][4 rows][77][X], all different
        self.p2p = []
        for src, tgt, bw, ew in PROMPTS:
            c = ac.make_controller(self.pipe, [src, tgt], False, {"default_": 0.4}, 0.6, ((bw,), (bw,)) if blend else None,
                                   {"words": (ew,), "values": (2,)}, num_ddim_steps=STEPS)
            self.p2p.append(c.tables())
        self.masa = [MasaCtrlTables(start_step=1, start_layer=2), MasaCtrlTables(start_step=1, start_layer=2)]
        self.traj = self.eng.ddim_invert(self.z0, self.ctx[:, 2], self.ts).clone()      # [STEPS + 1][2][4][S][S]
        self.memo = {}

    def passes(self, kind, nimg, npass):
        """ctrls_per_pass of a loop: the reconstruction pass without a controller, the last pass with the controllers of `kind`"""
        last = {"p2p": self.p2p[:nimg], "masa": self.masa[:nimg], "none": None}[kind]
        return [None] * (npass - 1) + [last]

    def run(self, share, kind="p2p", nimg=2, npass=2, dedup=2, offset_rows=1, fresh=False):
        """(noise_loss, latents, counters) of the lock-step edit under src_share = share"""
        key = (share, kind, nimg, npass, dedup, offset_rows)
        if fresh or key not in self.memo:
            with self.eng.tuning(src_share=share, cfg_dedup=dedup):
                self.eng.reset_counters()
                nl, lats = self.eng.direct_edit(self.traj[:, :nimg], self.ctx[:nimg], self.passes(kind, nimg, npass), self.ts, GS,
                                                offset_rows=offset_rows)
                got = (nl.clone(), lats.clone(), self.eng.counters())
            if fresh:
                return got
            self.memo[key] = got
        return self.memo[key]

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


def _same(case, share, **kw):
    nimg, npass = kw.get("nimg", 2), kw.get("npass", 2)
    nl0, lat0, c0 = case.run(0, **kw)
    nl1, lat1, c1 = case.run(share, **kw)
    assert torch.isfinite(nl0).all() and torch.isfinite(lat0).all()
    assert c0["unet_shared_rows"] == 0 and c1["unet_shared_rows"] == 2 * npass * nimg * STEPS, (c0, c1)
    assert c1["unet_sample_forwards"] == c0["unet_sample_forwards"] == (1 + npass) * 4 * nimg * STEPS
    assert c1["unet_dedup_prefix_rows"] == c0["unet_dedup_prefix_rows"] and c1["unet_calls"] == c0["unet_calls"] == STEPS
    assert c1["unet_sample_forwards_cached_kv"] == c0["unet_sample_forwards_cached_kv"]
    assert c1["executed_gemm_flops"] < c0["executed_gemm_flops"]                         # fewer rows really went through the GEMMs
    assert not torch.equal(lat0[-1, 0, 0], lat0[-1, 0, 1])                               # source and target differ
    if nimg > 1:
        assert not torch.equal(lat0[-1, 0], lat0[-1, 1])                                 # so do the images
    assert torch.equal(nl1, nl0), (nl1 - nl0).abs().max().item()
    assert torch.equal(lat1, lat0), (lat1 - lat0).abs().max().item()


@pytest.mark.parametrize("dedup", [2, 0])
def test_refine_reweight_localblend_small64(small64, dedup):
    """two images, two passes, Refine + Reweight + LocalBlend; steps on both sides of the self- and cross-replace windows"""
    _same(small64, 2, dedup=dedup)
    if dedup == 2:
        assert not torch.equal(small64.run(0)[1][1], small64.run(0)[1][0])               # the edit pass differs from the reconstruction pass


@pytest.mark.parametrize("nimg,npass,dedup", [(2, 2, 2), (2, 2, 0), (1, 2, 2), (2, 1, 2), (1, 1, 0)])
def test_refine_reweight_tiny16(tiny16, nimg, npass, dedup):
    """TINY16: self-replace redirects rows in block 0 at steps 0 - 2 (short cfg_dedup prefix), step 3 takes the long one"""
    _same(tiny16, 2, nimg=nimg, npass=npass, dedup=dedup)


def test_no_controller_tiny16(tiny16):
    _same(tiny16, 2, kind="none")
    _same(tiny16, 2, kind="none", nimg=1, dedup=0)


@pytest.mark.parametrize("masks", [False, True])
def test_masactrl_tiny16(tiny16, masks):
    """kind 2: every target row reads K and V of its half's (shared) source row; with masks the target rows take the class-restricted kernel"""
    eng, S = tiny16.eng, TINY16.sample_size
    if masks:
        g = torch.Generator().manual_seed(5)
        ms = (torch.rand(2, S, S, generator=g) > 0.5).to(torch.uint8).numpy()
        mt = (torch.rand(2, S, S, generator=g) > 0.5).to(torch.uint8).numpy()
        eng.masa_set_masks(ms, mt)
    try:
        got = {s: tiny16.run(s, kind="masa", fresh=True) for s in (0, 2)}
        plain = tiny16.run(0, kind="none")
    finally:
        eng.masa_set_masks()
    assert got[2][2]["unet_shared_rows"] == 4 * 2 * STEPS and got[0][2]["unet_shared_rows"] == 0
    assert torch.isfinite(got[0][1]).all() and not torch.equal(got[0][1][1], plain[1][1])        # the controller acts on the last pass
    assert torch.equal(got[2][0], got[0][0]) and torch.equal(got[2][1], got[0][1]), (got[2][1] - got[0][1]).abs().max().item()


def _one_step_eps(case, share):
    """The conditional predictions a one-step loop of image 0 computed, recovered from its outputs: [O cond_src (the shared row), O cond_tgt,
    last pass cond_tgt].  With guidance scale 1 the CFG mix is the conditional eps itself, and the step is affine in it:
    prev = c_x x + c_e eps (DDIM, eta = 0), so eps = (prev - c_x x) / c_e in float64; the offset pass stores loss = target - prev."""
    eng, t = case.eng, int(case.ts[0])
    x, target = case.traj[-1, :1], case.traj[0, :1]                       # any start latent and any target serve
    with eng.tuning(src_share=share):
        eng.reset_counters()
        nl, lats = eng.direct_edit(torch.stack([target, x]), case.ctx[:1], [None, None], case.ts[:1], 1.0)
        assert eng.counters()["unet_shared_rows"] == (4 if share else 0)
    a_t, a_p = float(eng.ac[t]), float(eng.final_alpha)                     # one step of a one-step schedule ends at final_alpha_cumprod
    c_x, c_e = (a_p / a_t) ** 0.5, (1 - a_p) ** 0.5 - (a_p * (1 - a_t) / a_t) ** 0.5
    x, target, nl, lats = (v.cpu().double() for v in (x[0], target[0], nl, lats))
    prev = torch.stack([target - nl[0, 0, 0], target - nl[0, 0, 1], lats[-1, 0, 1]])
    return (prev - c_x * x) / c_e, t


@pytest.mark.parametrize("which", ["small64", "tiny16"])
def test_free_tile_choice(which, request):
    """src_share = 1: bit-identical to 0 where the compact and the logical row count choose the same tiles at this width.  Where they do
    not: the bar of tests/test_gpu_ff_fold.py on what it is a bar for, the eps of ONE UNet forward against the fp32 oracle -- both knob
    values under 4e-3 rel-L2 and 1 at most 1.25 x the error of 0 (independent fp16 roundings, nothing else).
    Measured on MI355X: TINY16 bit-identical; SMALL64 not (see the figures this test prints)."""
    case = request.getfixturevalue(which)
    kw = dict(kind="none", nimg=1)
    nl0, lat0, c0 = case.run(0, **kw)
    nl1, lat1, c1 = case.run(1, **kw)
    assert c1["unet_shared_rows"] == 4 * STEPS and c1["unet_sample_forwards"] == c0["unet_sample_forwards"]
    if torch.equal(lat1, lat0) and torch.equal(nl1, nl0):
        print("%s: src_share = 1 is bit-identical to 0" % which)
        return
    e_0, t = _one_step_eps(case, 0)
    e_1, _ = _one_step_eps(case, 1)
    with torch.no_grad():
        ref = sd_oracle.unet_forward(case.usd, case.cfg, case.traj[-1, :1].cpu().expand(2, -1, -1, -1), t, case.ctx[0, 2:4]).double()
    ref = torch.stack([ref[0], ref[1], ref[1]])
    e0, e1 = ((e_0 - ref).norm() / ref.norm()).item(), ((e_1 - ref).norm() / ref.norm()).item()
    msg = "%s rel-L2(eps) of one forward vs oracle: src_share 1 %.3e, 0 %.3e" % (which, e1, e0)
    print(msg)
    assert e0 < BAR and e1 < BAR, msg
    assert e1 <= MARGIN * e0, msg


def test_fallbacks(tiny16):
    """offset_rows = 0 (the guidance passes' source latents no longer follow the offset pass's) and a recording context (one that holds
    an activation tape: pnpi_unet_context_grad ran on it) run the full launch, whatever the knob says"""
    for share in (1, 2):
        a = tiny16.run(0, offset_rows=0)
        b = tiny16.run(share, offset_rows=0)
        assert b[2]["unet_shared_rows"] == 0 and b[2]["executed_gemm_flops"] == a[2]["executed_gemm_flops"]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(tiny16.run(0, offset_rows=0)[1], tiny16.run(0)[1])
    rec = Case(TINY16, blend=False)           # a context of its own: the tape stays with a context for good
    try:
        kw = dict(kind="none", nimg=1)
        before = rec.run(2, fresh=True, **kw)
        assert before[2]["unet_shared_rows"] == 4 * STEPS
        S = TINY16.sample_size
        rec.eng.unet_context_grad(rec.z0[:1], int(rec.ts[0]), rec.ctx[0, 2:3], torch.ones(1, 4, S, S))
        got = {share: rec.run(share, fresh=True, **kw) for share in (0, 2)}
    finally:
        rec.close()
    assert got[2][2]["unet_shared_rows"] == 0 and got[2][2]["executed_gemm_flops"] == got[0][2]["executed_gemm_flops"]
    assert torch.equal(got[0][0], got[2][0]) and torch.equal(got[0][1], got[2][1])
    assert torch.equal(got[0][0], before[0]) and torch.equal(got[0][1], before[1])


def test_knob_on_a_live_context(tiny16):
    """0 -> 2 -> 0 -> 1 -> 2 between loops of one context: no arena overflow either way, equal settings give equal results; values
    outside 0 .. 2 are rejected and leave the setting alone"""
    runs = [(s, tiny16.run(s, fresh=True)) for s in (0, 2, 0, 1, 2)]
    for s, (nl, lat, c) in runs:
        assert c["unet_shared_rows"] == (8 * STEPS if s else 0), (s, c)
        assert torch.isfinite(nl).all() and torch.isfinite(lat).all()
        want = tiny16.run(1) if s == 1 else runs[0][1]          # equal settings give equal results (1 need not equal 0: test_free_tile_choice)
        assert torch.equal(nl, want[0]) and torch.equal(lat, want[1]), s
    lib = tiny16.eng.lib
    assert lib.pnpi_set_tuning(b"src_share", 3) != 0 and lib.pnpi_set_tuning(b"src_share", -1) != 0
    assert tiny16.run(2, fresh=True)[2]["unet_shared_rows"] == 8 * STEPS
