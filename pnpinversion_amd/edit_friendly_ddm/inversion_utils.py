"""models/edit_friendly_ddm/inversion_utils.py on NativePipeline: the edit-friendly DDPM inversion (stochastic forward process with one
stored noise map per step) and its reverse process.  Same signatures as the reference, plus one keyword-only `noise=`: the draws of
sample_xts_from_x0 [num_inference_steps, 4, h, w] (or [.., nimg, 4, h, w]) in the reference's order (reversed(timesteps), i.e. xts[1] first).
Without it they come from torch.randn_like on the pipeline's device, in that order.

The step loops run device-resident in libpnpi (pnpi_ef_invert / pnpi_ef_edit): one UNet launch per step, both CFG branches (and both
prompts) as rows of that launch.  Deviation (not read by anything): the reference's xts[0] is NaN (its t = 0 step divides by a zero
variance); here it is x0, and zs[0] = 0 as in the reference."""
import torch

from ..p2p.attention_control import controller_tables


def encode_text(model, prompts):
    """:58-68"""
    if isinstance(prompts, str):
        prompts = [prompts]
    tok = model.tokenizer
    ids = tok(list(prompts), padding="max_length", max_length=tok.model_max_length, truncation=True, return_tensors="pt").input_ids
    with torch.no_grad():
        return model.text_encoder(ids.to(model.device))[0]


def get_variance(model, timestep):
    """:91-98 (host scalar; the loops evaluate the same expression inside libpnpi, pnpi_ef_step_scalars)"""
    s = model.scheduler
    prev_timestep = timestep - s.config.num_train_timesteps // s.num_inference_steps
    alpha_prod_t = s.alphas_cumprod[timestep]
    alpha_prod_t_prev = s.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else s.final_alpha_cumprod
    beta_prod_t = 1 - alpha_prod_t
    beta_prod_t_prev = 1 - alpha_prod_t_prev
    return (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)


def _schedule(model, num_inference_steps):
    s = model.scheduler
    if s.num_inference_steps != num_inference_steps:
        raise ValueError("scheduler.set_timesteps(%d) first: the reference indexes its tables by the scheduler's timesteps"
                         % num_inference_steps)
    return [int(t) for t in s.timesteps]


def _images(x):
    """[4,h,w] / [1,4,h,w] (the reference's single image) or [nimg,4,h,w] -> ([nimg,4,h,w], single)"""
    if x.dim() == 3:
        return x[None], True
    return x, x.shape[0] == 1


def draw_noise(x0, num_inference_steps):
    """the draws of sample_xts_from_x0 (:50-53): torch.randn_like(x0) once per level, xts[1] first -> [n, *x0.shape]"""
    return torch.stack([torch.randn_like(x0) for _ in range(num_inference_steps)])


def sample_xts_from_x0(model, x0, num_inference_steps=50, *, noise=None):
    """:31-55 (one launch).  xts[0] = x0."""
    ts = _schedule(model, num_inference_steps)
    x, single = _images(x0.to(model.device).float())
    if noise is None:
        noise = draw_noise(x, num_inference_steps)
    noise = noise.reshape(num_inference_steps, *x.shape)
    xts = model.unet.engine.ef_sample_xts(x, noise, ts)
    return xts[:, 0] if single else xts


def inversion_forward_process(model, x0, etas=None, prog_bar=False, prompt="", cfg_scale=3.5, num_inference_steps=50, eps=None, *,
                              noise=None):
    """:100-176 -> (xt, zs, xts): xts [n+1, 4, h, w], zs [n, 4, h, w] (an image axis after the first when x0 holds several images),
    xt = xts[1][None].  eta = 0 (the deterministic branch, :115-117, :165-167) is not implemented: it stores no noise maps."""
    if etas is None or (type(etas) in [int, float] and etas == 0):
        raise NotImplementedError("inversion_forward_process with eta = 0 is not implemented (edit-friendly inversion needs eta > 0)")
    ts = _schedule(model, num_inference_steps)
    x, single = _images(x0.to(model.device).float())
    nimg = x.shape[0]
    if noise is None:
        noise = draw_noise(x, num_inference_steps)
    noise = noise.to(model.device).float().reshape(num_inference_steps, nimg, *x.shape[1:])
    uncond = encode_text(model, "").expand(nimg, -1, -1)
    cond = encode_text(model, prompt).expand(nimg, -1, -1) if prompt != "" else None
    xts, zs = model.unet.engine.ef_invert(x, noise, uncond, cond, cfg_scale, etas, ts)
    if single:
        xts, zs = xts[:, 0], zs[:, 0]
    return xts[1][None], zs, xts


def inversion_reverse_process(model, xT, etas=0, prompts="", cfg_scales=None, prog_bar=False, zs=None, controller=None, asyrp=False):
    """:210-262 -> (xt [len(prompts), 4, h, w], zs).  The attention edit is the controller registered on the model
    (register_attention_control), as in the reference; `controller` is the one whose step_callback the reference calls.
    Several images: xT [nimg, 4, h, w], zs [n_run, nimg, 4, h, w] -> xt [nimg, len(prompts), 4, h, w]."""
    if zs is None:
        raise ValueError("inversion_reverse_process needs the noise maps zs of inversion_forward_process (the reference fails on zs=None)")
    if isinstance(prompts, str) or len(prompts) not in (1, 2):
        raise ValueError("prompts: a list of one or two prompts")
    if controller is not None and getattr(controller, "local_blend", None) is not None:
        raise NotImplementedError("edit_friendly_ddm LocalBlend is not supported")
    batch_size = len(prompts)
    s = model.scheduler
    ts = [int(t) for t in s.timesteps]
    if etas is None:
        etas = 0
    if type(etas) in [int, float]:
        etas = [etas] * s.num_inference_steps
    assert len(etas) == s.num_inference_steps
    x = xT.to(model.device).float()
    z = zs.to(model.device).float()
    batched = x.dim() == 4 and z.dim() == 5
    if not batched:
        x, z = x.reshape(1, *z.shape[1:]), z[:, None]
    nimg = x.shape[0]
    text = encode_text(model, prompts)
    uncond = encode_text(model, [""] * batch_size)
    context = torch.cat([uncond, text])[None].expand(nimg, -1, -1, -1)
    registered = model.unet.controller
    tables = controller_tables(registered)
    if tables is not None and batch_size != 2:
        raise ValueError("an attention edit needs two prompts (source, target)")
    out = model.unet.engine.ef_edit(x, z, context, cfg_scales if cfg_scales is not None else [1.0] * batch_size,
                                    None if tables is None else [tables] * nimg, etas, ts)
    for c in {id(registered): registered, id(controller): controller}.values():
        if c is not None and hasattr(c, "cur_step"):
            c.cur_step += z.shape[0]         # LOW_RESOURCE: one step per (uncond, cond) call pair
    return (out if batched else out[0]), zs
