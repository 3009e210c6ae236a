"""ff2 folded into proj_out (tuning "ff_fold", csrc/api_graph.inc transformer_fwd): each transformer block ends in ONE two-source 1 x 1
convolution over f2 | hs2 with the derived weights [Wp W2 | Wp] and bias Wp b2 + bp instead of the ff2 GEMM followed by proj_out.

Configuration: two levels of width 64 / 128 (multiples of 64, so the fold is active in all 11 transformer blocks) on 12 x 12 latents:
144 and 36 tokens per row, so M = 144 / 432 and 36 / 108 at one / three rows -- no multiple of any GEMM tile (64, 128, 192, 256 rows).
Bar: the UNet parity bar of tests/test_gpu_model.py (rel-L2(eps) < 4e-3 against the fp32 CPU oracle on identical seeded weights)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sd_oracle  # noqa: E402  (checker only)
from pnpinversion_amd import weights  # noqa: E402
from pnpinversion_amd.config import ModelConfig  # noqa: E402
from pnpinversion_amd.engine import NativeEngine  # noqa: E402

CFG = ModelConfig(block_out_channels=(64, 128), block_has_attn=(1, 1), cross_dim=64, sample_size=12, layers_per_block=2,
                  vae_block_out_channels=(32, 64), vae_layers_per_block=2, clip_layers=0)
N_TRANSFORMERS = 2 * 2 + 1 + 2 * 3
VSD = weights.vae_state_dict(CFG, 20)          # a forward refuses to run before every UNet and VAE tensor is loaded
BAR = 4e-3
IGEMM_CLASSES = ("igemm128", "igemm64", "igemm64_splitk", "igemm_wide")


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


def _inputs(rows, seed):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randn(rows, CFG.in_channels, CFG.sample_size, CFG.sample_size, generator=g)
    return lat, weights.synth_context(CFG, rows, seed=seed + 1)


def _forward(eng, fold, lat, t, ctx):
    with eng.tuning(ff_fold=fold):
        return eng.unet(lat, t, ctx).clone()


def _igemm_launches(eng, fold, lat, t, ctx):
    with eng.tuning(ff_fold=fold):
        eng.profile_begin()
        eng.unet(lat, t, ctx)
        st = eng.profile_end()
    return sum(st[k]["launches"] for k in IGEMM_CLASSES)


@pytest.fixture(scope="module")
def model():
    usd = weights.unet_state_dict(CFG, 21)
    eng = NativeEngine(CFG, max_unet_rows=4, max_vae_images=1)
    eng.load_state_dict(usd, VSD)
    refs = {}
    for rows in (1, 3):
        lat, ctx = _inputs(rows, 30 + rows)
        with torch.no_grad():
            refs[rows] = (lat, ctx, sd_oracle.unet_forward(usd, CFG, lat, 500, ctx))
    yield eng, refs
    eng.close()


@pytest.mark.parametrize("rows", [1, 3])
def test_fold_and_two_launches_against_the_oracle(model, rows):
    """eps_out of the whole forward (it passes through the GroupNorm partial sums the folded launch's epilogue leaves for the next
    ResNet): both knob settings meet the parity bar, and the folded error is at most 1.25 x the unfolded one -- the two differ by
    independent fp16 roundings only, a wrong weight column would not fit under that."""
    eng, refs = model
    lat, ctx, ref = refs[rows]
    on, off = _forward(eng, 1, lat, 500, ctx), _forward(eng, 0, lat, 500, ctx)
    e_on, e_off = rel(on, ref), rel(off, ref)
    msg = "rows=%d rel-L2 vs oracle: folded %.3e, two launches %.3e" % (rows, e_on, e_off)
    print(msg)
    assert torch.isfinite(on).all() and torch.isfinite(off).all(), msg
    assert not torch.equal(on, off), "the knob changed nothing: " + msg
    assert e_on < BAR and e_off < BAR, msg
    assert e_on <= 1.25 * e_off, msg


def test_rows_stay_independent(model):
    """rows 0 and 2 of a three-row launch fed identical inputs come out bit-identical (M = 432 / 108: the rows share GEMM tiles)"""
    eng, refs = model
    lat, ctx, _ = refs[3]
    lat, ctx = lat.clone(), ctx.clone()
    lat[2], ctx[2] = lat[0], ctx[0]
    out = _forward(eng, 1, lat, 500, ctx)
    assert torch.equal(out[0], out[2])
    assert not torch.equal(out[0], out[1])


def test_counters_and_launch_count(model):
    eng, refs = model
    lat, ctx, _ = refs[3]
    got = {}
    for fold in (0, 1):
        eng.reset_counters()
        _forward(eng, fold, lat, 500, ctx)
        c = eng.counters()
        got[fold] = (c["unet_sample_forwards"], c["unet_calls"], c["executed_gemm_flops"])
    assert got[0] == got[1] and got[0][0] == 3 and got[0][2] > 0, got
    n_off, n_on = _igemm_launches(eng, 0, lat, 500, ctx), _igemm_launches(eng, 1, lat, 500, ctx)
    assert n_off - n_on == N_TRANSFORMERS, (n_off, n_on)


def test_reload_rebuilds_the_folded_weights():
    """Stale-weight guard: seed A, a forward, then seed B into the same context -- the folded forward must follow the new weights (a
    stale fold would be eleven blocks of seed-A weights inside a seed-B network), also on a context sharing the arena."""
    lat, ctx = _inputs(3, 50)
    eng = NativeEngine(CFG, max_unet_rows=4, max_vae_images=1)
    try:
        eng.load_state_dict(weights.unet_state_dict(CFG, 22), VSD)
        a_on = _forward(eng, 1, lat, 500, ctx)
        usd_b = weights.unet_state_dict(CFG, 23)
        eng.load_state_dict(usd_b, None)
        with torch.no_grad():
            ref_b = sd_oracle.unet_forward(usd_b, CFG, lat, 500, ctx)
        b_on, b_off = _forward(eng, 1, lat, 500, ctx), _forward(eng, 0, lat, 500, ctx)
        msg = "folded vs two launches %.3e, vs oracle %.3e / %.3e, seed A vs seed B %.3e" % (
            rel(b_on, b_off), rel(b_on, ref_b), rel(b_off, ref_b), rel(a_on, b_off))
        print(msg)
        assert rel(b_on, b_off) < BAR and rel(b_on, ref_b) < BAR and rel(b_off, ref_b) < BAR, msg
        assert rel(a_on, b_off) > 100 * BAR, msg          # the two seeds are different networks
        assert _igemm_launches(eng, 0, lat, 500, ctx) - _igemm_launches(eng, 1, lat, 500, ctx) == N_TRANSFORMERS      # folded again after the reload
        child = NativeEngine(CFG, max_unet_rows=4, max_vae_images=1, share_weights_with=eng)
        try:
            c_on = _forward(child, 1, lat, 500, ctx)
            assert rel(c_on, b_off) < BAR, rel(c_on, b_off)
            assert torch.equal(c_on, b_on)                # the same launches on the same folded weights
            assert _igemm_launches(child, 0, lat, 500, ctx) - _igemm_launches(child, 1, lat, 500, ctx) == N_TRANSFORMERS
        finally:
            child.close()
    finally:
        eng.close()


def test_fold_follows_a_checkpoint_loaded_in_pieces():
    """The folded weights are built once all four sources of every block are there, whichever load call brings the last one: a
    checkpoint without one proj_out bias leaves the context unusable (a forward refuses to run), the missing tensor loaded on its own
    completes it, and the forward then runs folded on weights that match."""
    lat, ctx = _inputs(1, 60)
    usd = weights.unet_state_dict(CFG, 24)
    part = {k: v for k, v in usd.items() if k != "mid_block.attentions.0.proj_out.bias"}
    eng = NativeEngine(CFG, max_unet_rows=4, max_vae_images=1)
    try:
        eng.load_state_dict(part, VSD)
        assert eng.missing_weights() == (1, ["unet.mid_block.attentions.0.proj_out.bias"])
        with pytest.raises(Exception, match="weights not loaded"):
            eng.unet(lat, 500, ctx)
        eng.load_state_dict({k: v for k, v in usd.items() if k not in part}, None)
        assert _igemm_launches(eng, 0, lat, 500, ctx) - _igemm_launches(eng, 1, lat, 500, ctx) == N_TRANSFORMERS
        with torch.no_grad():
            ref = sd_oracle.unet_forward(usd, CFG, lat, 500, ctx)
        assert rel(_forward(eng, 1, lat, 500, ctx), ref) < BAR
    finally:
        eng.close()


def test_recording_forward_ignores_the_knob(model):
    """The taping forward (null-text path) keeps ff2 and proj_out apart -- the backward walks them as two records: same launches (the
    tape's length: one record per launch), same counters, bit-identical eps and context gradient under both knob settings."""
    eng, refs = model
    lat, ctx, _ = refs[1]
    d_eps = torch.randn(lat.shape, generator=torch.Generator().manual_seed(70)) * 64
    got = {}
    eng.unet_context_grad(lat, 500, ctx, d_eps)          # the first recording forward of a context also sizes the tape's arenas (a counted dry run)
    for fold in (0, 1):
        with eng.tuning(ff_fold=fold):
            eng.reset_counters()
            eng.profile_begin()
            eps, dctx = eng.unet_context_grad(lat, 500, ctx, d_eps)
            st = eng.profile_end()
            c = eng.counters()
        got[fold] = (eps.clone(), dctx.clone(), {k: v["launches"] for k, v in st.items()}, c["executed_gemm_flops"], c["unet_backward_rows"])
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert got[0][2:] == got[1][2:] and sum(got[0][2].values()) > 0, (got[0][2:], got[1][2:])
    assert torch.isfinite(got[1][1]).all() and got[1][1].abs().max() > 0
