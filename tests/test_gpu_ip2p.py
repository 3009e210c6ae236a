"""InstructPix2Pix (run_editing_instructpix2pix.py) on the MI355X: the step kernel bit-exact against the eager fp32 restatement
(pnpinversion_amd/instructpix2pix.py), the UNet forward at a float timestep (an integer t reproduces pnpi_unet_forward, a fractional t and 8
real input channels against the CPU oracle), the device-resident loop against its level-1 composition, against the run without the compact
prefix and against an fp32 CPU run of the same sampler around the oracle UNet, batching, counters and the refusals.  TINY16 shapes; one
two-step run at 64 x 64 latents for the 4096-token attention sites under this row layout.

The reference run is tests/golden/e2e_ip2p_tiny.npz (tools/make_golden_ip2p.py): the reference's own ldm UNetModel / Encoder / Decoder on
the CPU in fp32 inside the restated sampler, on this project's seeded weights (seed 2, the weights every context here loads)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi, weights  # noqa: E402
from pnpinversion_amd import instructpix2pix as ip  # noqa: E402
from pnpinversion_amd.config import SMALL64_IP2P, TINY16, TINY16_IP2P  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

CFG = TINY16_IP2P
S = CFG.sample_size
MAX_ROWS = 9                     # three images of three rows
GT, GI = 7.5, 1.5
NSTEPS = 8
LAT_BAR = 1.5e-2                 # tests/test_gpu_loops.py: latents against an fp32 reference run
BATCH_BAR = 3e-2                 # tests/test_gpu_blended.py: one call of three images against three calls


def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "e2e_ip2p_tiny.npz"))
    assert int(g["weight_seed"]) == 2 and int(g["nsteps"]) == NSTEPS and float(g["cfg_text"]) == GT and float(g["cfg_image"]) == GI
    return g


@pytest.fixture(scope="module")
def usd():
    return weights.unet_state_dict(CFG, 2)


@pytest.fixture(scope="module")
def pipe(usd):
    p = NativePipeline(CFG, max_unet_rows=MAX_ROWS, max_vae_images=2, text_encoder=SyntheticTextEncoder(CFG.cross_dim, seed=7))
    p.load_state_dict(usd, weights.vae_state_dict(CFG, 2))
    yield p
    p.engine.close()


@pytest.fixture(scope="module")
def sched():
    return ip.SigmaSchedule()


@pytest.fixture(scope="module")
def table(sched):
    sigmas = sched.get_sigmas(NSTEPS)
    return sigmas, ip.step_table(sigmas, sched)


def loop_inputs(nimg, seed, sigmas, nsteps=NSTEPS):
    ctx = weights.synth_context(CFG, 2 * nimg, seed=seed).reshape(nimg, 2, CFG.ctx_len, CFG.cross_dim)
    return dict(z0=randn(seed + 1, nimg, 4, S, S) * sigmas[0], image=randn(seed + 2, nimg, 4, S, S),
                noise=randn(seed + 3, nsteps, nimg, 4, S, S), ctx=torch.stack([ctx[:, 0], ctx[:, 1], ctx[:, 1]], 1))


def run_loop(eng, a, tab, **kw):
    return eng.ip2p_edit(a["z0"], a["image"], a["noise"], a["ctx"], tab, GT, GI, **kw)


# ---------------------------------------------------------------------------------------------- the step kernel
@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("step", ["first", "middle", "last"])
def test_ip2p_step_bit_exact(pipe, sched, step, nimg):
    """50-step schedule: step 0, step 25, and step 49 (sigma_next = 0: the draw is NaN and must not be read).  C x h x w = 4 x 5 x 7
    (E = 140: the float4 path, more than one wavefront) and 3 x 5 x 7 (E = 105: no multiple of the vector width, the scalar path)."""
    eng = pipe.engine
    sigmas = sched.get_sigmas(50)
    tab = ip.step_table(sigmas, sched)
    i = {"first": 0, "middle": 25, "last": 49}[step]
    assert (tab[i][5] == 0) == (step == "last") and (sigmas[i + 1] == 0) == (step == "last")
    c_in_next = float(tab[i + 1][3]) if i + 1 < 50 else 0.25
    for ch in (4, 3):
        eps, z = randn(1, nimg, 3, ch, 5, 7), randn(2, nimg, ch, 5, 7) * sigmas[i]
        noise, image = randn(3, nimg, ch, 5, 7), randn(4, nimg, ch, 5, 7)
        want = ip.euler_ancestral_step(z, eps, noise, sigmas[i], sigmas[i + 1], GT, GI)
        given = torch.full_like(noise, float("nan")) if step == "last" else noise
        got, nxt = eng.ip2p_step(eps, z, given, image, tab[i], GT, GI, c_in_next=c_in_next)
        assert torch.equal(got.cpu(), want), (ch, (got.cpu() - want).abs().max())
        scaled = want * torch.tensor(np.float32(c_in_next))
        assert torch.equal(nxt[:, 0].cpu(), torch.cat([scaled, image], 1)), ch
        assert torch.equal(nxt[:, 1].cpu(), torch.cat([scaled, torch.zeros_like(image)], 1)), ch
        assert torch.equal(eng.ip2p_step(eps, z, given, None, tab[i], GT, GI).cpu(), want), ch          # without the next inputs
        if step != "last":
            with pytest.raises(_capi.PnpiError, match="needs its draw"):
                eng.ip2p_step(eps, z, None, image, tab[i], GT, GI)
        else:
            assert torch.equal(eng.ip2p_step(eps, z, None, image, tab[i], GT, GI).cpu(), want), ch
    with pytest.raises(ValueError, match=r"eps must be \[nimg, 3, C, h, w\]"):
        eng.ip2p_step(eps[:, :2], z, noise, image, tab[i], GT, GI)


# ---------------------------------------------------------------------------------------------- the forward at a float timestep
def packed(eng, out, rows):
    """pnpi_unet_forward writes [rows][out_channels][h][w] packed at the start of engine.unet's input-shaped buffer"""
    return out.flatten()[:rows * 4 * S * S].reshape(rows, 4, S, S)


def test_unet_forward_t_integer_t_reproduces_unet_forward(pipe):
    eng = pipe.engine
    lat, ctx = randn(20, 3, 8, S, S), weights.synth_context(CFG, 3, seed=21)
    for t in (0, 500, 999):
        first = packed(eng, eng.unet(lat, t, ctx), 3).clone()          # fills the per-timestep bias row
        again = packed(eng, eng.unet(lat, t, ctx), 3).clone()          # reads it
        got = eng.unet_t(lat, float(t), ctx)
        assert torch.equal(first, again) and torch.equal(got, first), (t, (got - first).abs().max())
    ref500 = packed(eng, eng.unet(lat, 500, ctx), 3).clone()
    eng.text_kv_precompute(ctx)
    assert torch.equal(eng.unet_t(lat, 500.0, None), ref500)
    with pytest.raises(_capi.PnpiError, match="timestep out of range"):
        eng.unet_t(lat, 999.5, ctx)
    with pytest.raises(_capi.PnpiError, match="timestep out of range"):
        eng.unet_t(lat, float("nan"), ctx)


def test_unet_forward_t_fractional_t_eight_channels_against_oracle(pipe, usd, sched):
    """the op-level bar of tests/test_gpu_model.py::test_unet_tiny (rel-L2 < 4e-3) at timesteps of the 8-step schedule"""
    from oracle import sd_oracle
    eng = pipe.engine
    lat, ctx = randn(30, 3, 8, S, S), weights.synth_context(CFG, 3, seed=31)
    ts = sched.sigma_to_t(sched.get_sigmas(NSTEPS)[:-1])
    for t in (float(ts[1]), float(ts[5])):
        assert t != round(t)
        got = eng.unet_t(lat, t, ctx).cpu()
        with torch.no_grad():
            ref = sd_oracle.unet_forward(usd, CFG, lat, t, ctx)
        r = rel(got, ref)
        print("unet_t at t = %.4f: rel-L2 %.3g against the oracle" % (t, r))
        assert got.shape == ref.shape == (3, 4, S, S) and r < 4e-3, (t, r)
        # the neighbouring integer timesteps are another function: the fraction is not dropped
        lo, hi = packed(eng, eng.unet(lat, int(t), ctx), 3).cpu(), packed(eng, eng.unet(lat, int(t) + 1, ctx), 3).cpu()
        print("  the integer neighbours against it: %.3g, %.3g" % (rel(lo, ref), rel(hi, ref)))
        assert not torch.equal(lo, got) and not torch.equal(hi, got)
    # conv_in reads channels 4 .. 7
    cut = lat.clone()
    cut[:, 4:] = 0
    moved = rel(eng.unet_t(cut, t, ctx).cpu(), got)
    assert moved > 1e-2, moved


def test_unet_forward_t_and_vae_against_the_reference_modules(pipe, gold):
    """ldm's UNetModel at the recorded fractional t on 8 real channels (its own fp32 sinusoid), and its Encoder / Decoder: the op-level
    bars of tests/test_gpu_model.py for a TINY16 forward (UNet and encoder 4e-3, decoder 6e-3)"""
    eng = pipe.engine
    t8 = float(gold["t8"])
    assert t8 != round(t8)
    got = eng.unet_t(torch.from_numpy(gold["lat8"]), t8, torch.from_numpy(gold["context"])).cpu()
    r = rel(got, gold["eps8"])
    x = (2 * torch.tensor(gold["image"]).float() / 255 - 1).permute(2, 0, 1)[None]
    r_e = rel(eng.vae_encode(x), gold["c_concat"])
    r_d = rel(eng.vae_decode(1. / 0.18215 * torch.from_numpy(gold["z"][-1])[None])[0], gold["decoded"])
    print("against ldm's modules: unet_t at t = %.4f %.3g, encoder mean %.3g, decoder %.3g" % (t8, r, r_e, r_d))
    assert r < 4e-3 and r_e < 4e-3 and r_d < 6e-3, (r, r_e, r_d)


def test_ip2p_edit_against_the_reference_run(pipe, gold, sched):
    """per-step z against the run recorded from ldm's UNetModel, from the reference's image latent and draws (bar: tests/test_gpu_loops.py)"""
    eng = pipe.engine
    sigmas = torch.from_numpy(gold["sigmas"])
    tab = ip.step_table(sigmas, sched)
    # sigma_to_t goes through torch's vectorised log, which differs by an ulp between host CPUs (tests/test_ip2p_host.py pins the bits on
    # the machine class the fixture was made on): the loop is given the reference's own timesteps
    assert np.abs(tab[:, 4] - gold["timesteps"]).max() < 1e-3
    tab[:, 4] = gold["timesteps"]
    draws = torch.cat([torch.from_numpy(gold["draws"]), torch.full((1, 4, S, S), float("nan"))])[:, None]     # the last step draws nothing
    z0 = torch.from_numpy(gold["draw0"])[None] * sigmas[0]
    got, traj = eng.ip2p_edit(z0, torch.from_numpy(gold["c_concat"]), draws, torch.from_numpy(gold["context"])[None], tab, GT, GI, trajectory=True)
    d = [rel(traj[i, 0], gold["z"][i]) for i in range(NSTEPS)]
    print("ip2p parity per step against the reference run:", " ".join("%.3g" % v for v in d))
    for i, v in enumerate(d):
        assert v < LAT_BAR, (i, v)
    assert torch.equal(got, traj[-1])


def test_edit_mirrors_edit_instruct_pix2pix(pipe, gold):
    """InstructPix2Pix.edit end to end on a 128 x 128 image: panel layout, the draws' order, and the loop it runs"""
    from PIL import Image
    ed = ip.InstructPix2Pix(pipe)
    img = Image.fromarray(gold["image"])
    side = S * 8
    shape = (4, S, S)
    torch.manual_seed(1234)
    a = np.array(ed.edit(img, "make it snowy", steps=4))
    torch.manual_seed(1234)
    start, steps = torch.randn(1, *shape)[0], torch.stack([torch.randn(1, *shape)[0] for _ in range(3)])      # z0, then one draw per step but the last
    b = np.array(ed.edit(img, "make it snowy", steps=4, noise=(start, steps)))
    assert a.shape == (side, 4 * side, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
    assert np.array_equal(a[:, side:2 * side], gold["image"]) and not a[:, 2 * side:3 * side].any()          # instruction | source | black | edit
    panels, z = ed.edit_images([img], ["make it snowy"], 4, noise=(start, steps), return_latents=True)
    sigmas = ed.schedule.get_sigmas(4)
    x = (2 * torch.tensor(gold["image"]).float() / 255 - 1).permute(2, 0, 1)[None]
    ctx = torch.cat([ed._encode(["make it snowy"]), ed._encode([""]), ed._encode([""])])[None]
    draws = torch.cat([steps, torch.zeros(1, *shape)])[:, None]
    want = pipe.engine.ip2p_edit(start[None] * sigmas[0], pipe.engine.vae_encode(x), draws, ctx, ip.step_table(sigmas, ed.schedule))
    assert torch.equal(z, want) and np.array_equal(panels[0], a)
    other = np.array(ed.edit(img, "make it a painting", steps=4, noise=(start, steps)))
    assert not np.array_equal(other[:, 3 * side:], a[:, 3 * side:])
    with pytest.raises(ValueError, match="fits to"):
        ed.edit(img.resize((side, 2 * side)), "x", steps=2)


# ---------------------------------------------------------------------------------------------- the loop
def test_ip2p_edit_equals_level1_steps_and_the_run_without_the_compact_prefix(pipe, table):
    """two images with different contexts, latents, image latents and draws"""
    eng = pipe.engine
    sigmas, tab = table
    nimg = 2
    a = loop_inputs(nimg, 100, sigmas)
    with eng.tuning(cfg_dedup=2):
        got, traj = run_loop(eng, a, tab, trajectory=True)
        got, traj = got.cpu(), traj.cpu()
        eng.reset_counters()
        again = run_loop(eng, a, tab).cpu()
        c2 = eng.counters()
    with eng.tuning(cfg_dedup=0):
        eng.reset_counters()
        plain = run_loop(eng, a, tab).cpu()
        c0 = eng.counters()
    assert torch.equal(got, again) and torch.equal(got, traj[-1])
    assert torch.equal(got, plain), (got - plain).abs().max()
    assert c2["unet_dedup_prefix_rows"] == 2 * nimg * NSTEPS and c0["unet_dedup_prefix_rows"] == 0, (c2, c0)
    # level 1: one float-timestep forward of the 3 * nimg rows and one step launch per step
    eng.text_kv_precompute(a["ctx"].flatten(0, 1))
    z = a["z0"]
    scaled = z * torch.tensor(tab[0][3])
    two = torch.stack([torch.cat([scaled, a["image"]], 1), torch.cat([scaled, torch.zeros_like(scaled)], 1)], 1)
    for i in range(NSTEPS):
        rows = two[:, [0, 0, 1]].flatten(0, 1)
        eps = eng.unet_t(rows, float(tab[i][4]), None).unflatten(0, (nimg, 3))
        last = i + 1 == NSTEPS
        out = eng.ip2p_step(eps, z, a["noise"][i], a["image"], tab[i], GT, GI, c_in_next=None if last else float(tab[i + 1][3]))
        z, two = (out, None) if last else out
        assert torch.equal(z.cpu(), traj[i]), (i, (z.cpu() - traj[i]).abs().max())
    assert torch.equal(z.cpu(), got)


def test_ip2p_edit_against_fp32_cpu_run_counters_and_draws(pipe, usd, table):
    """per-step z against the same sampler in fp32 on the CPU around the oracle UNet: the bar of the other loops against fp32 runs"""
    from oracle import sd_oracle
    eng = pipe.engine
    sigmas, tab = table
    a = loop_inputs(1, 200, sigmas)
    ts = ip.SigmaSchedule().sigma_to_t(sigmas[:-1])
    assert all(float(t) != round(float(t)) for t in ts[1:-1])
    z, ref = a["z0"], []
    with torch.no_grad():
        for i in range(NSTEPS):
            c_in = 1 / (sigmas[i].reshape(1) ** 2 + 1) ** 0.5
            x = torch.cat([torch.cat([z * c_in] * 3), torch.cat([a["image"], a["image"], torch.zeros_like(a["image"])])], 1)
            eps = sd_oracle.unet_forward(usd, CFG, x, float(ts[i]), a["ctx"][0])
            z = ip.euler_ancestral_step(z, eps[None], a["noise"][i], sigmas[i], sigmas[i + 1], GT, GI)
            ref.append(z)
    torch.cuda.synchronize()
    eng.reset_counters()
    got, traj = run_loop(eng, a, tab, trajectory=True)
    c = eng.counters()
    d = [rel(traj[i], ref[i]) for i in range(NSTEPS)]
    print("ip2p parity per step against the fp32 CPU run:", " ".join("%.3g" % v for v in d))
    for i, v in enumerate(d):
        assert v < LAT_BAR, (i, v)
    assert c["unet_sample_forwards"] == 3 * NSTEPS and c["unet_sample_forwards_cached_kv"] == 3 * NSTEPS, c
    assert c["unet_calls"] == NSTEPS and c["text_kv_rows"] == 3, c
    # the last step's sigma_next is 0: its draw is not read; every other draw is
    nan_last = a["noise"].clone()
    nan_last[-1] = float("nan")
    assert torch.equal(run_loop(eng, dict(a, noise=nan_last), tab), got)
    other = a["noise"].clone()
    other[3] += 1.0
    assert not torch.equal(run_loop(eng, dict(a, noise=other), tab), got)
    # the image latent reaches the UNet unscaled through rows 0 and 1
    assert rel(run_loop(eng, dict(a, image=a["image"] * 0.5), tab), got) > 1e-2


def test_three_images_in_one_call_equal_single_calls(pipe, table):
    """Rows are independent in every kernel; only the per-launch tile / split-K choice could differ with the row count (9 rows against
    3); at these widths it does not and the results have so far been bit-equal (printed), the asserted bar stays the batching bar"""
    eng = pipe.engine
    sigmas, tab = table
    a = loop_inputs(3, 300, sigmas)
    both = run_loop(eng, a, tab).cpu()
    singles = [run_loop(eng, {k: (v[:, i:i + 1] if k == "noise" else v[i:i + 1]) for k, v in a.items()}, tab).cpu()[0] for i in range(3)]
    d = [rel(both[i], singles[i]) for i in range(3)]
    wrong = [rel(both[i], singles[(i + 1) % 3]) for i in range(3)]
    print("batched vs single:", d, "against the next image's:", wrong)
    for i in range(3):
        assert d[i] < BATCH_BAR, (i, d[i])
        assert not wrong[i] < BATCH_BAR, (i, wrong[i])


def test_ip2p_edit_refusals_launch_nothing(pipe, table):
    eng = pipe.engine
    sigmas, tab = table
    torch.cuda.synchronize()
    before = eng.counters()
    too_many = loop_inputs(MAX_ROWS // 3 + 1, 400, sigmas)
    with pytest.raises(_capi.PnpiError, match=r"3 \* nimg exceeds max_unet_rows") as e:
        run_loop(eng, too_many, tab)
    assert e.value.status == _capi.PNPI_EINVAL
    a = loop_inputs(1, 410, sigmas)
    with pytest.raises(_capi.PnpiError, match="nsteps") as e:
        run_loop(eng, dict(a, noise=a["noise"][:0]), tab[:0])
    assert e.value.status == _capi.PNPI_EINVAL
    bad = tab.copy()
    bad[2, 4] = 1000.0
    with pytest.raises(_capi.PnpiError, match="timestep out of range"):
        run_loop(eng, a, bad)
    bad = tab.copy()
    bad[1, 0] = 0.0
    with pytest.raises(_capi.PnpiError, match="sigma and c_in must be positive"):
        run_loop(eng, a, bad)
    assert eng.counters() == before
    with pytest.raises(ValueError, match=r"noise must be \[nsteps, nimg, 4, h, w\]"):
        run_loop(eng, dict(a, noise=a["noise"][:-1]), tab)


def test_four_channel_context_is_refused(table):
    sigmas, tab = table
    p = NativePipeline(TINY16, max_unet_rows=3, max_vae_images=1, text_encoder=SyntheticTextEncoder(TINY16.cross_dim, seed=7))
    try:
        p.load_state_dict(weights.unet_state_dict(TINY16, 2), weights.vae_state_dict(TINY16, 2))
        before = p.engine.counters()
        with pytest.raises(_capi.PnpiError, match="in_channels") as e:
            run_loop(p.engine, loop_inputs(1, 500, sigmas), tab)
        assert e.value.status == _capi.PNPI_EINVAL and p.engine.counters() == before
        with pytest.raises(ValueError, match="in_channels"):
            ip.InstructPix2Pix(p)
    finally:
        p.engine.close()


def test_loops_that_step_a_latent_by_its_prediction_refuse_the_eight_channel_model(pipe):
    eng = pipe.engine
    before = eng.counters()
    pipe.scheduler.set_timesteps(2)
    with pytest.raises(_capi.PnpiError, match="in_channels == out_channels"):
        eng.ddim_invert(randn(600, 1, 8, S, S), weights.synth_context(CFG, 1, seed=601), pipe.scheduler.timesteps.numpy())
    assert eng.counters() == before


# ---------------------------------------------------------------------------------------------- 64 x 64 latents
def test_small64_two_steps_compact_prefix_is_bit_identical(sched):
    """4096-token self-attention and the compacted prefix under the rows [0, 0, 1]: cfg_dedup = 2 against 0"""
    cfg = SMALL64_IP2P
    p = NativePipeline(cfg, max_unet_rows=3, max_vae_images=1, text_encoder=SyntheticTextEncoder(cfg.cross_dim, seed=7))
    try:
        p.load_state_dict(weights.unet_state_dict(cfg, 2), weights.vae_state_dict(cfg, 2))
        eng = p.engine
        sigmas = sched.get_sigmas(50)[:3]
        tab = ip.step_table(sigmas, sched)
        ctx = weights.synth_context(cfg, 2, seed=700)
        args = (randn(701, 1, 4, 64, 64) * sigmas[0], randn(702, 1, 4, 64, 64), randn(703, 2, 1, 4, 64, 64), torch.stack([ctx[0], ctx[1], ctx[1]])[None], tab)
        out = {}
        for mode in (2, 0):
            with eng.tuning(cfg_dedup=mode):
                eng.reset_counters()
                out[mode] = eng.ip2p_edit(*args, GT, GI).cpu()
                c = eng.counters()
                assert c["unet_dedup_prefix_rows"] == (4 if mode else 0) and c["unet_sample_forwards"] == 6, (mode, c)
        assert torch.isfinite(out[0]).all() and torch.equal(out[2], out[0]), (out[2] - out[0]).abs().max()
    finally:
        p.engine.close()
