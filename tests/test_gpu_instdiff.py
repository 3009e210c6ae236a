"""InstructDiffusion (run_editing_instructdiffusion.py) on the MI355X: the step kernel's symmetric combine bit-exact against the eager fp32
restatement (pnpinversion_amd/instructdiffusion.py), the forward on the rows [instruction + image, null + image, instruction + zero image]
and the device-resident loop against the run recorded from the reference, the loop against its level-1 composition and against the run
without the compact prefix, batching, InstructDiffusion.edit and the refusals.  TINY16 shapes; one two-step run at 64 x 64 latents.

The reference run is tests/golden/e2e_instdiff_tiny.npz (tools/make_golden_instructdiffusion.py): the reference's own CFGDenoiser.forward
around its InstructDiffusion ldm UNetModel, Encoder and Decoder on the CPU in fp32 inside the restated k-diffusion sampler, on this project's
seeded weights (seed 2, the weights every context here loads).  The bars are those tests/test_gpu_ip2p.py asserts for the same UNet, width,
step count and arithmetic."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

from pnpinversion_amd import _capi, weights  # noqa: E402
from pnpinversion_amd import instructdiffusion as idf  # noqa: E402
from pnpinversion_amd import instructpix2pix as ip  # noqa: E402
from pnpinversion_amd.config import SMALL64_IP2P, TINY16, TINY16_IP2P  # noqa: E402
from pnpinversion_amd.pipeline import NativePipeline  # noqa: E402
from pnpinversion_amd.text import SyntheticTextEncoder  # noqa: E402

CFG = TINY16_IP2P
S = CFG.sample_size
MAX_ROWS = 9                     # three images of three rows
GT, GI = 5.0, 1.25
NSTEPS = 8
FWD_BAR = 4e-3                   # tests/test_gpu_ip2p.py: one TINY16 forward against ldm's UNetModel
LAT_BAR = 1.5e-2                 # tests/test_gpu_ip2p.py: per-step latents against the reference run
DEC_BAR = 6e-3                   # tests/test_gpu_ip2p.py: the decoded image against ldm's Decoder


def rel(a, b):
    a, b = torch.as_tensor(a).float().cpu(), torch.as_tensor(b).float().cpu()
    return ((a - b).norm() / b.norm()).item()


def randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "e2e_instdiff_tiny.npz"))
    assert int(g["weight_seed"]) == 2 and int(g["nsteps"]) == NSTEPS and float(g["cfg_text"]) == GT and float(g["cfg_image"]) == GI
    return g


@pytest.fixture(scope="module")
def pipe():
    p = NativePipeline(CFG, max_unet_rows=MAX_ROWS, max_vae_images=2, text_encoder=SyntheticTextEncoder(CFG.cross_dim, seed=7))
    p.load_state_dict(weights.unet_state_dict(CFG, 2), weights.vae_state_dict(CFG, 2))
    yield p
    p.engine.close()


@pytest.fixture(scope="module")
def sched():
    return ip.SigmaSchedule()


@pytest.fixture(scope="module")
def table(sched):
    sigmas = sched.get_sigmas(NSTEPS)
    return sigmas, ip.step_table(sigmas, sched)


def loop_inputs(nimg, seed, sigmas, nsteps=NSTEPS, cfg=CFG):
    s = cfg.sample_size
    ctx = weights.synth_context(cfg, 2 * nimg, seed=seed).reshape(nimg, 2, cfg.ctx_len, cfg.cross_dim)
    return dict(z0=randn(seed + 1, nimg, 4, s, s) * sigmas[0], image=randn(seed + 2, nimg, 4, s, s),
                noise=randn(seed + 3, nsteps, nimg, 4, s, s), ctx=torch.stack([ctx[:, 0], ctx[:, 1], ctx[:, 0]], 1))     # [instruction, null, instruction]


def run_loop(eng, a, tab, **kw):
    return eng.instdiff_edit(a["z0"], a["image"], a["noise"], a["ctx"], tab, GT, GI, **kw)


def single(a, i):
    return {k: (v[:, i:i + 1] if k == "noise" else v[i:i + 1]) for k, v in a.items()}


@pytest.fixture(scope="module")
def reference_run(pipe, gold, sched):
    """pnpi_instdiff_edit on the fixture's inputs, once: (z, trajectory) on the host"""
    sigmas = torch.from_numpy(gold["sigmas"])
    tab = ip.step_table(sigmas, sched)
    # sigma_to_t goes through torch's vectorised log, which differs by an ulp between host CPUs: the loop is given the reference's timesteps
    assert np.abs(tab[:, 4] - gold["timesteps"]).max() < 1e-3
    tab[:, 4] = gold["timesteps"]
    draws = torch.cat([torch.from_numpy(gold["draws"]), torch.full((1, 4, S, S), float("nan"))])[:, None]     # the last step draws nothing
    z0 = torch.from_numpy(gold["draw0"])[None] * sigmas[0]
    got, traj = pipe.engine.instdiff_edit(z0, torch.from_numpy(gold["c_concat"]), draws, torch.from_numpy(gold["context"])[None], tab, GT, GI,
                                          trajectory=True)
    return got.cpu(), traj.cpu()


# ---------------------------------------------------------------------------------------------- the step kernel
@pytest.mark.parametrize("nimg", [1, 3])
@pytest.mark.parametrize("step", ["first", "middle", "last"])
def test_instdiff_step_bit_exact(pipe, sched, step, nimg):
    """50-step schedule: step 0, step 25, and step 49 (sigma_next = 0: the draw pointer is NULL).  C x h x w = 4 x 5 x 7 (E = 140: the
    float4 path, more than one wavefront) and 3 x 5 x 7 (E = 105: no multiple of the vector width, the scalar path)."""
    eng = pipe.engine
    sigmas = sched.get_sigmas(50)
    tab = ip.step_table(sigmas, sched)
    i = {"first": 0, "middle": 25, "last": 49}[step]
    assert (tab[i][5] == 0) == (step == "last") and (sigmas[i + 1] == 0) == (step == "last")
    c_in_next = float(tab[i + 1][3]) if i + 1 < 50 else 0.25
    for ch in (4, 3):
        eps, z = randn(1, nimg, 3, ch, 5, 7), randn(2, nimg, ch, 5, 7) * sigmas[i]
        noise, image = randn(3, nimg, ch, 5, 7), randn(4, nimg, ch, 5, 7)
        want = idf.euler_ancestral_step(z, eps, noise, sigmas[i], sigmas[i + 1], GT, GI)
        given = None if step == "last" else noise
        got, nxt = eng.instdiff_step(eps, z, given, image, tab[i], GT, GI, c_in_next=c_in_next)
        assert torch.equal(got.cpu(), want), (ch, (got.cpu() - want).abs().max())
        scaled = want * torch.tensor(np.float32(c_in_next))
        assert torch.equal(nxt[:, 0].cpu(), torch.cat([scaled, image], 1)), ch
        assert torch.equal(nxt[:, 1].cpu(), torch.cat([scaled, torch.zeros_like(image)], 1)), ch
        assert torch.equal(eng.instdiff_step(eps, z, given, None, tab[i], GT, GI).cpu(), want), ch          # without the next inputs
        # the other editor's combine on the same rows is another result: the entry point selects the kernel variant
        assert not torch.equal(eng.ip2p_step(eps, z, given, None, tab[i], GT, GI).cpu(), want), ch
        if step == "last":                                                                                   # a NaN draw is not read either
            assert torch.equal(eng.instdiff_step(eps, z, torch.full_like(noise, float("nan")), None, tab[i], GT, GI).cpu(), want), ch


def device_floats(n, offset):
    """n floats on the device starting `offset` floats into an allocation: offset = 1 is 4-byte but not 16-byte aligned"""
    return torch.zeros(n + 4, device="cuda")[offset:offset + n]


def test_instdiff_step_scalar_path_row_of_1023_on_offset_pointers(pipe, sched):
    """row_elems = 1023 and every pointer one float past a 16-byte boundary, through the C entry point itself: the scalar path, several
    blocks (2 x 1023 elements, 256 threads each)"""
    import ctypes as C
    eng = pipe.engine
    sigmas = sched.get_sigmas(50)
    tab = ip.step_table(sigmas, sched)
    nimg, E, i = 2, 1023, 25
    eps, z, noise, image = randn(11, nimg, 3, E), randn(12, nimg, E) * sigmas[i], randn(13, nimg, E), randn(14, nimg, E)
    want = idf.euler_ancestral_step(z, eps, noise, sigmas[i], sigmas[i + 1], GT, GI)
    c_in_next = float(tab[i + 1][3])
    dev = {}
    for name, t in (("eps", eps), ("z", z), ("noise", noise), ("image", image)):
        dev[name] = device_floats(t.numel(), 1)
        dev[name].copy_(t.flatten())
    out, nxt = device_floats(nimg * E, 1), device_floats(nimg * 4 * E, 1)
    guard = [t.storage_offset() for t in (*dev.values(), out, nxt)]
    assert guard == [1] * 6 and all(t.data_ptr() % 16 == 4 for t in (*dev.values(), out, nxt))
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    sc = np.ascontiguousarray(tab[i], dtype=np.float32)
    eng._call("pnpi_instdiff_step", p(dev["eps"]), p(dev["z"]), p(dev["noise"]), p(dev["image"]), nimg, E, GT, GI,
              sc.ctypes.data_as(C.POINTER(C.c_float)), c_in_next, p(out), p(nxt))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().reshape(nimg, E), want), (out.cpu().reshape(nimg, E) - want).abs().max()
    scaled = want * torch.tensor(np.float32(c_in_next))
    rows = nxt.cpu().reshape(nimg, 2, 2, E)
    assert torch.equal(rows[:, 0, 0], scaled) and torch.equal(rows[:, 0, 1], image)
    assert torch.equal(rows[:, 1, 0], scaled) and not rows[:, 1, 1].any()


def test_prologue_form_writes_both_input_rows(pipe, table):
    """eps = NULL is the loop's first launch: z' = z and the two 8-channel inputs [z * c_in | image] and [z * c_in | 0] with the zero half
    exactly zero.  pnpi_instdiff_step refuses a NULL eps as pnpi_ip2p_step does, so the form is observed where it runs: a one-step loop
    whose sigma_next is 0 moves z by its single step, which the level-1 step reproduces only from the inputs the prologue wrote."""
    eng = pipe.engine
    sigmas, tab = table
    a = loop_inputs(2, 50, sigmas, nsteps=1)
    one = tab[-1:].copy()                                        # sigma_next = 0: no draw
    got = run_loop(eng, a, one).cpu()
    c_in = torch.tensor(one[0][3])
    scaled = a["z0"] * c_in
    two = torch.stack([torch.cat([scaled, a["image"]], 1), torch.cat([scaled, torch.zeros_like(scaled)], 1)], 1)
    assert not two[:, 1, 4:].any()
    eps = eng.unet_t(two[:, [0, 0, 1]].flatten(0, 1), float(one[0][4]), a["ctx"].flatten(0, 1)).unflatten(0, (2, 3))
    want = eng.instdiff_step(eps, a["z0"], None, a["image"], one[0], GT, GI).cpu()
    assert torch.equal(got, want), (got - want).abs().max()
    # a prologue that left anything but zero in the second input's image half, or the unscaled z, gives another eps row
    dirty = two.clone()
    dirty[:, 1, 4:] = 1e-3
    assert not torch.equal(eng.unet_t(dirty[:, [0, 0, 1]].flatten(0, 1), float(one[0][4]), a["ctx"].flatten(0, 1)).unflatten(0, (2, 3))[:, 2], eps[:, 2])
    import ctypes as C
    sc = np.ascontiguousarray(one[0], dtype=np.float32)
    zd = a["z0"].cuda()
    st = eng.lib.pnpi_instdiff_step(eng.h, None, C.c_void_p(zd.data_ptr()), None, None, 2, zd[0].numel(), GT, GI,
                                    sc.ctypes.data_as(C.POINTER(C.c_float)), 1.0, C.c_void_p(zd.data_ptr()), None)
    assert st == _capi.PNPI_EINVAL


# ---------------------------------------------------------------------------------------------- against the reference's run
def test_forward_on_the_three_rows_of_step_0_against_the_reference(pipe, gold):
    """[instruction + image, null + image, instruction + zero image] at t = 999 from the fixture's z0, image latent and contexts: the third
    row is a (text, image) pairing only this editor launches"""
    eng = pipe.engine
    sigmas = torch.from_numpy(gold["sigmas"])
    z0 = torch.from_numpy(gold["draw0"])[None] * sigmas[0]
    cc = torch.from_numpy(gold["c_concat"])
    c_in = 1 / (sigmas[0].reshape(1) ** 2 + 1) ** 0.5
    rows = torch.cat([torch.cat([z0 * c_in] * 3), torch.cat([cc, cc, torch.zeros_like(cc)])], 1)
    got = eng.unet_t(rows, float(gold["timesteps"][0]), torch.from_numpy(gold["context"])).cpu()
    d = [rel(got[k], gold["eps"][0][k]) for k in range(3)]
    print("step-0 rows against the reference's eps: %.3g %.3g %.3g" % tuple(d))
    for k in range(3):
        assert d[k] < FWD_BAR, (k, d[k])
    # the three rows are three functions of the inputs: none passes for another within the bar
    assert not rel(gold["eps"][0][2], gold["eps"][0][0]) < FWD_BAR and not rel(gold["eps"][0][1], gold["eps"][0][0]) < FWD_BAR
    assert not rel(got[2], gold["eps"][0][0]) < FWD_BAR and not rel(got[2], gold["eps"][0][1]) < FWD_BAR


def test_instdiff_edit_against_the_reference_run(pipe, gold, reference_run):
    """per-step z and the decoded image against the run recorded from the reference's CFGDenoiser and ldm modules"""
    got, traj = reference_run
    d = [rel(traj[i, 0], gold["z"][i]) for i in range(NSTEPS)]
    print("instdiff parity per step against the reference run:", " ".join("%.3g" % v for v in d))
    dec_own = rel(pipe.engine.vae_decode(1. / 0.18215 * got)[0], gold["decoded"])
    dec_ref = rel(pipe.engine.vae_decode(1. / 0.18215 * torch.from_numpy(gold["z"][-1])[None])[0], gold["decoded"])
    print("decoded image: from the loop's z %.3g, from the reference's z %.3g" % (dec_own, dec_ref))
    for i, v in enumerate(d):
        assert v < LAT_BAR, (i, v)
    assert torch.equal(got, traj[-1])
    assert dec_ref < DEC_BAR and dec_own < DEC_BAR, (dec_ref, dec_own)
    # the other editor's loop on the same inputs does not pass for this run: the bar tells the two combines apart
    assert not rel(pipe.engine.ip2p_edit(torch.from_numpy(gold["draw0"])[None] * float(gold["sigmas"][0]), torch.from_numpy(gold["c_concat"]),
                                     torch.cat([torch.from_numpy(gold["draws"]), torch.zeros(1, 4, S, S)])[:, None],
                                     torch.from_numpy(gold["context"])[None], ip.step_table(torch.from_numpy(gold["sigmas"])), GT, GI),
                   gold["z"][-1]) < LAT_BAR


def test_edit_mirrors_instruct_diffusion_edit(pipe, gold, reference_run):
    """InstructDiffusion.edit end to end on the fixture's 128 x 128 image with the fixture's contexts and draws: panel instruction | source |
    black | edit, the edit quarter against the reference's decoded image quantised as the reference does (:122-125).

    Bar, in units of the clamped reference image's norm: the decoder's output is held to DEC_BAR of the UNCLAMPED image's norm (above) and
    clamping moves no two values apart; both images are then truncated to uint8, which moves the reference's own image by q, measured on
    the fixture.  So the two quarters may differ by DEC_BAR * |decoded| / |clamped| + 2 q (triangle inequality), no more."""
    from PIL import Image
    ed = idf.InstructDiffusion(pipe)
    ctx = torch.from_numpy(gold["context"]).to(pipe.device)
    ed._encode = lambda prompts: ctx[1:2] if prompts == [""] else ctx[0:1]
    img = Image.fromarray(gold["image"])
    side = S * 8
    noise = (torch.from_numpy(gold["draw0"]), torch.from_numpy(gold["draws"]))
    panel = np.array(ed.edit(img, "make it snowy", steps=NSTEPS, noise=noise))
    assert panel.shape == (side, 4 * side, 3) and panel.dtype == np.uint8
    assert np.array_equal(panel[:, side:2 * side], gold["image"]) and not panel[:, 2 * side:3 * side].any()
    assert panel[:, :side].any()                                                                          # the instruction is drawn
    decoded = torch.from_numpy(gold["decoded"])
    ref = decoded.clamp(-1, 1)                                                                            # :122, in the decoder's [-1, 1]
    want = (255.0 * ((ref + 1.0) / 2.0).permute(1, 2, 0)).type(torch.uint8)                               # :123-125
    back = lambda u8: 2 * torch.as_tensor(u8).float().permute(2, 0, 1) / 255 - 1      # noqa: E731
    q = ((back(want) - ref).norm() / ref.norm()).item()
    r = ((back(panel[:, 3 * side:]) - back(want)).norm() / ref.norm()).item()
    bar = DEC_BAR * (decoded.norm() / ref.norm()).item() + 2 * q
    print("edit quarter against the reference's quantised image: %.3g of the clamped image's norm (quantisation alone %.3g, bar %.3g), "
          "max level difference %d" % (r, q, bar, np.abs(panel[:, 3 * side:].astype(int) - want.numpy().astype(int)).max()))
    assert r < bar, (r, q, bar)
    # the defaults are the reference's scales, the draws come from the global generator in its order, and the latents are the loop's
    panels, z = ed.edit_images([img], ["make it snowy"], NSTEPS, noise=noise, return_latents=True)
    assert np.array_equal(panels[0], panel)
    sigmas = ed.schedule.get_sigmas(NSTEPS)
    x_in = (2 * torch.tensor(gold["image"]).float() / 255 - 1).permute(2, 0, 1)[None]
    draws = torch.cat([noise[1], torch.zeros(1, 4, S, S)])[:, None]
    want_z = pipe.engine.instdiff_edit(noise[0][None] * sigmas[0], pipe.engine.vae_encode(x_in), draws, ctx[None], ip.step_table(sigmas, ed.schedule), 5.0, 1.25)
    assert torch.equal(z, want_z)
    shape = (4, S, S)
    torch.manual_seed(1234)
    a = np.array(ed.edit(img, "make it snowy", steps=4))
    torch.manual_seed(1234)
    start, steps = torch.randn(1, *shape)[0], torch.stack([torch.randn(1, *shape)[0] for _ in range(3)])
    assert np.array_equal(a, np.array(ed.edit(img, "make it snowy", steps=4, noise=(start, steps))))
    with pytest.raises(ValueError, match="fits to"):
        ed.edit(img.resize((side, 2 * side)), "x", steps=2)


# ---------------------------------------------------------------------------------------------- the loop equals its parts
def test_instdiff_edit_equals_level1_steps_and_the_run_without_the_compact_prefix(pipe, table):
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
    assert c2["unet_sample_forwards"] == 3 * nimg * NSTEPS and c2["unet_calls"] == NSTEPS, c2
    # level 1: one float-timestep forward of the explicitly assembled 3 * nimg rows and one step launch per step
    eng.text_kv_precompute(a["ctx"].flatten(0, 1))
    z = a["z0"]
    scaled = z * torch.tensor(tab[0][3])
    two = torch.stack([torch.cat([scaled, a["image"]], 1), torch.cat([scaled, torch.zeros_like(scaled)], 1)], 1)
    for i in range(NSTEPS):
        rows = two[:, [0, 0, 1]].flatten(0, 1)
        eps = eng.unet_t(rows, float(tab[i][4]), None).unflatten(0, (nimg, 3))
        last = i + 1 == NSTEPS
        out = eng.instdiff_step(eps, z, None if last else a["noise"][i], a["image"], tab[i], GT, GI, c_in_next=None if last else float(tab[i + 1][3]))
        z, two = (out, None) if last else out
        assert torch.equal(z.cpu(), traj[i]), (i, (z.cpu() - traj[i]).abs().max())
    assert torch.equal(z.cpu(), got)
    # the third row reads the instruction: with the null text there the loop is another one
    null3 = a["ctx"].clone()
    null3[:, 2] = a["ctx"][:, 1]
    assert not rel(run_loop(eng, dict(a, ctx=null3), tab), got) < LAT_BAR


def test_three_images_in_one_call_equal_their_single_calls_bit_for_bit(pipe, table):
    """three different images, instructions and draws; swapping two instructions changes exactly those two outputs"""
    eng = pipe.engine
    sigmas, tab = table
    a = loop_inputs(3, 300, sigmas)
    assert not torch.equal(a["ctx"][0], a["ctx"][1]) and not torch.equal(a["image"][0], a["image"][1]) and not torch.equal(a["noise"][:, 0], a["noise"][:, 1])
    both = run_loop(eng, a, tab).cpu()
    singles = [run_loop(eng, single(a, i), tab).cpu()[0] for i in range(3)]
    print("batched vs single:", [rel(both[i], singles[i]) for i in range(3)], "against the next image's:", [rel(both[i], singles[(i + 1) % 3]) for i in range(3)])
    for i in range(3):
        assert torch.equal(both[i], singles[i]), (i, (both[i] - singles[i]).abs().max())
        assert not torch.equal(both[i], singles[(i + 1) % 3])
    swapped_ctx = a["ctx"].clone()
    swapped_ctx[0, [0, 2]], swapped_ctx[2, [0, 2]] = a["ctx"][2, [0, 2]], a["ctx"][0, [0, 2]]           # the instruction sits in rows 0 and 2
    swapped = run_loop(eng, dict(a, ctx=swapped_ctx), tab).cpu()
    assert torch.equal(swapped[1], both[1])
    assert not torch.equal(swapped[0], both[0]) and not torch.equal(swapped[2], both[2])


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(pipe, table):
    eng = pipe.engine
    sigmas, tab = table
    a = loop_inputs(1, 410, sigmas)
    good = run_loop(eng, a, tab).cpu()
    torch.cuda.synchronize()
    before = eng.counters()
    with pytest.raises(_capi.PnpiError, match=r"3 \* nimg exceeds max_unet_rows \(InstructDiffusion runs \[edit \+ image, null \+ image, edit \+ no image\]") as e:
        run_loop(eng, loop_inputs(MAX_ROWS // 3 + 1, 400, sigmas), tab)
    assert e.value.status == _capi.PNPI_EINVAL
    for col, value, message in ((0, 0.0, "InstructDiffusion step scalars: sigma and c_in must be positive"),
                                (0, -1.0, "sigma and c_in must be positive"), (3, 0.0, "sigma and c_in must be positive"),
                                (3, float("nan"), "sigma and c_in must be positive"),
                                (4, 1000.0, "timestep out of range"), (4, -0.5, "timestep out of range")):
        bad = tab.copy()
        bad[2, col] = value
        with pytest.raises(_capi.PnpiError, match=message) as e:
            run_loop(eng, a, bad)
        assert e.value.status == _capi.PNPI_EINVAL
    with pytest.raises(_capi.PnpiError, match="nsteps"):
        run_loop(eng, dict(a, noise=a["noise"][:0]), tab[:0])
    # level 1: a missing draw when sigma_next > 0, a non-positive sigma
    eps, z, image = randn(1, 1, 3, 4, 5, 7), randn(2, 1, 4, 5, 7), randn(4, 1, 4, 5, 7)
    with pytest.raises(_capi.PnpiError, match="needs its draw") as e:
        eng.instdiff_step(eps, z, None, image, tab[0], GT, GI)
    assert e.value.status == _capi.PNPI_EINVAL
    bad = tab[0].copy()
    bad[0] = 0.0
    with pytest.raises(_capi.PnpiError, match="InstructDiffusion step scalars"):
        eng.instdiff_step(eps, z, z, image, bad, GT, GI)
    assert eng.counters() == before
    with pytest.raises(ValueError, match=r"eps must be \[nimg, 3, C, h, w\]"):
        eng.instdiff_step(eps[:, :2], z, z, image, tab[0], GT, GI)
    assert torch.equal(run_loop(eng, a, tab).cpu(), good)                                                # the context is as usable as before


def test_four_channel_context_is_refused(table):
    sigmas, tab = table
    p = NativePipeline(TINY16, max_unet_rows=3, max_vae_images=1, text_encoder=SyntheticTextEncoder(TINY16.cross_dim, seed=7))
    try:
        p.load_state_dict(weights.unet_state_dict(TINY16, 2), weights.vae_state_dict(TINY16, 2))
        before = p.engine.counters()
        with pytest.raises(_capi.PnpiError, match="InstructDiffusion needs a model with in_channels == 8") as e:
            run_loop(p.engine, loop_inputs(1, 500, sigmas), tab)
        assert e.value.status == _capi.PNPI_EINVAL and p.engine.counters() == before
        with pytest.raises(ValueError, match="InstructDiffusion needs a model with in_channels"):
            idf.InstructDiffusion(p)
        lat, ctx = randn(501, 1, 4, S, S), weights.synth_context(TINY16, 1, seed=502)
        assert torch.isfinite(p.engine.unet(lat, 500, ctx)).all()                                        # the context still runs
    finally:
        p.engine.close()


# ---------------------------------------------------------------------------------------------- 64 x 64 latents
def test_small64_two_steps_compact_prefix_is_bit_identical(sched):
    """4096-token self-attention and the compacted prefix under the rows [0, 0, 1] with the instruction in the third: cfg_dedup = 2 against 0"""
    cfg = SMALL64_IP2P
    p = NativePipeline(cfg, max_unet_rows=3, max_vae_images=1, text_encoder=SyntheticTextEncoder(cfg.cross_dim, seed=7))
    try:
        p.load_state_dict(weights.unet_state_dict(cfg, 2), weights.vae_state_dict(cfg, 2))
        eng = p.engine
        sigmas = sched.get_sigmas(50)[:3]
        tab = ip.step_table(sigmas, sched)
        a = loop_inputs(1, 700, sigmas, nsteps=2, cfg=cfg)
        out = {}
        for mode in (2, 0):
            with eng.tuning(cfg_dedup=mode):
                eng.reset_counters()
                out[mode] = run_loop(eng, a, tab).cpu()
                c = eng.counters()
                assert c["unet_dedup_prefix_rows"] == (4 if mode else 0) and c["unet_sample_forwards"] == 6, (mode, c)
        assert torch.isfinite(out[0]).all() and torch.equal(out[2], out[0]), (out[2] - out[0]).abs().max()
    finally:
        p.engine.close()
