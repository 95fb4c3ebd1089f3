"""The reference's inference() + step() (src/pipe_FRESCO.py:14-234) restated for any dtype, and the stand-ins the loop's
tests run it and fresco_amd.inference on.

`inference_model` performs the reference's torch operations in the reference's order; the rounding hook `q` is applied after
every one of them (identity: the reference's own arithmetic in the tensors' dtype; `round_half` on float64 tensors: every
operation rounded to fp16, which is what fp16 tensors compute, since a float64 result rounded to half is the correctly
rounded half result).  The scheduler's coefficients are 0-dim tensors of the scheduler's dtype and are not rounded, as
diffusers keeps alphas_cumprod in fp32 beside fp16 latents.  warp_tensor is injected.

The stand-ins are small deterministic networks whose output depends on everything the loop hands them (the latents, the
timestep, each text row, each residual, the conditioning scale) with a gain below 1; they log their calls into one trace.
They never read a device value on the host, so they run under torch.cuda.set_sync_debug_mode("error").
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if _GOLDEN not in sys.path:
    sys.path.insert(0, _GOLDEN)
import closed_form as cf  # noqa: E402

GOLDEN_FILE = "loop_golden.npz"
STEPS = [901, 751, 601, 451, 301, 151]
COND_SCALE = [0.7, 0.6, 0.9, 0.5, 0.8, 1.0]
GUIDANCE = 7.5
SIDE = 64  # images; latents are SIDE // 8

# name -> (frames, keyword arguments of inference); propagation cases read the recorded `<name>_rec_in` list
CASES = {
    "first": (3, dict(num_warmup_steps=1, seed=3, repeat_noise=True)),
    "prop": (3, dict(num_warmup_steps=1, seed=4, propagation_mode=True)),
    "warm2": (3, dict(num_warmup_steps=2, seed=5)),
    "warm0": (3, dict(num_warmup_steps=0, seed=6)),
    "warmneg": (3, dict(num_warmup_steps=-1, seed=7)),
    "smooth": (3, dict(num_warmup_steps=0, seed=8, bg_smoothing_steps=[3, 4], smoothing=True)),
    "nocn": (3, dict(num_warmup_steps=1, seed=9, use_controlnet=False)),
    "nocfg": (3, dict(num_warmup_steps=1, seed=10, do_classifier_free_guidance=False)),
    "prop2": (2, dict(num_warmup_steps=1, seed=11, propagation_mode=True)),
}
PREDECESSOR = {"prop": "first", "prop2": None}  # prop2 follows an unrecorded first batch of two frames (seed 12)


def round_half(x):
    return x.to(torch.float16).to(x.dtype)


def identity(x):
    return x


class Scheduler:
    """What inference() and step() read of a DDPMScheduler: SD-1.5's scaled-linear schedule, six steps 150 apart."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, dtype=torch.float64):
        betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0).to(dtype)
        self.one = torch.tensor(1.0, dtype=dtype)
        self.timesteps = torch.tensor(STEPS)

    def previous_timestep(self, timestep):
        return timestep - 150

    def add_noise(self, original_samples, noise, timesteps):
        """DDPMScheduler.add_noise for one timestep: the schedule cast to the samples' dtype first"""
        a = self.alphas_cumprod.to(dtype=original_samples.dtype)[timesteps.cpu()].to(original_samples.device)
        return a ** 0.5 * original_samples + (1 - a) ** 0.5 * noise


class VAE:
    """Deterministic: decode is a bounded channel mix enlarged eight times, encode an 8 x 8 mean and a fourth channel."""
    config = types.SimpleNamespace(scaling_factor=0.18215)

    def decode(self, z):
        img = torch.tanh(0.2 * (z[:, :3] + 0.25 * z[:, 3:4]))
        return types.SimpleNamespace(sample=img.repeat_interleave(8, 2).repeat_interleave(8, 3))

    def encode(self, img):
        p = F.avg_pool2d(img, 8)
        z = 2.0 * torch.cat([p, p.mean(1, keepdim=True)], 1)
        return types.SimpleNamespace(latent_dist=types.SimpleNamespace(sample=lambda: z))


def _time(timestep, like):
    return torch.as_tensor(timestep, device=like.device).to(like.dtype) / 1000


def _text(encoder_hidden_states):
    return encoder_hidden_states.mean(dim=(1, 2)).view(-1, 1, 1, 1)


class _UpBlock(torch.nn.Module):
    def forward(self, hidden_states):
        return hidden_states


class UNet(torch.nn.Module):
    """eps = f(latents, timestep, text row, residuals); an nn.Module with up_blocks, so fresco_amd.apply_FRESCO_opt
    installs on it.  on_call runs at the top of every call (the sync test switches the debug mode on there)."""

    def __init__(self, trace, dtype):
        super().__init__()
        self.config = types.SimpleNamespace(in_channels=4)
        self.dtype = dtype
        self.trace = trace
        self.inputs = []
        self.on_call = None
        self.up_blocks = torch.nn.ModuleList([_UpBlock(), _UpBlock()])

    def forward(self, sample, timestep, encoder_hidden_states=None, cross_attention_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None, return_dict=True):
        if self.on_call is not None:
            self.on_call()
        assert cross_attention_kwargs is None and return_dict is False
        self.trace.append(["unet", timestep, torch.is_tensor(timestep) and timestep.dim() == 0 and
                           timestep.device == sample.device])
        self.inputs.append(sample.detach().clone())
        tt = _time(timestep, sample)
        h = 0.5 * sample.roll(1, -1) + 0.15 * torch.sin(3.0 * sample.roll(1, 1))
        h = h + 0.2 * _text(encoder_hidden_states) + 0.1 * torch.cos(6.0 * tt)
        if down_block_additional_residuals is not None:
            r0, r1 = down_block_additional_residuals
            h = h + 0.25 * r0 + 0.25 * r1 + 0.25 * mid_block_additional_residual
        for blk in self.up_blocks:
            h = blk(hidden_states=h)
        return (h,)


class ControlNet:
    def __init__(self, trace):
        self.trace = trace

    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0,
                 guess_mode=None, return_dict=True):
        assert guess_mode is False and return_dict is False
        self.trace.append(["controlnet", timestep, float(conditioning_scale)])
        tt = _time(timestep, sample)
        e = F.avg_pool2d(controlnet_cond, 8).mean(1, keepdim=True)
        r0 = conditioning_scale * (0.3 * sample.flip(-2) + 0.2 * e)
        r1 = conditioning_scale * (0.2 * _text(encoder_hidden_states) * torch.cos(sample))
        mid = conditioning_scale * (0.3 * torch.sin(4.0 * tt) * sample.mean(dim=(2, 3), keepdim=True))
        return [r0, r1], mid


class Controller:
    def __init__(self, trace):
        self.trace = trace

    def disable_intraattn(self):
        self.trace.append(["disable_intraattn"])

    def disable_interattn(self):
        self.trace.append(["disable_interattn"])


class Pipe:
    def __init__(self, device, dtype, sched_dtype=torch.float64):
        self.trace = []
        self._execution_device = torch.device(device)
        self.unet = UNet(self.trace, dtype)
        self.vae = VAE()
        self.scheduler = Scheduler(sched_dtype)
        self.controlnet = ControlNet(self.trace)
        self.frescoProc = types.SimpleNamespace(controller=Controller(self.trace))
        self.progress = []

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        assert latents is None
        shape = (batch_size, num_channels_latents, height // 8, width // 8)
        return torch.randn(shape, generator=generator, device=device, dtype=dtype) * self.scheduler.init_noise_sigma

    @contextlib.contextmanager
    def progress_bar(self, total=None):
        self.progress.append(["total", total])
        yield types.SimpleNamespace(update=lambda: self.progress.append(["update"]))


def finish_trace(trace):
    """the trace with its timesteps as host ints (read after the run: the stand-ins log what they were handed)"""
    out = []
    for ev in trace:
        ev = list(ev)
        if len(ev) > 1:
            ev[1] = int(ev[1])
        if ev[0] == "unet":
            ev = ev[:2]
        out.append(ev)
    return out


def make_inputs(name, device, dtype):
    """(positional arguments after frescoProc, keyword arguments) of inference for a case, closed forms throughout"""
    B, kw = CASES[name]
    kw = dict(kw)
    copies = 2 if kw.get("do_classifier_free_guidance", True) else 1
    imgs = cf.feat(B, 3, SIDE, SIDE, 0.5).double()
    embeds = 0.7 * cf.feat(copies * B, 1, 5, 16, 0.3).double()[:, 0]
    embeds[B:] += 0.4  # (with guidance: the text rows)
    edges = torch.sigmoid(cf.feat(copies * B, 3, SIDE, SIDE, 1.3).double())
    to = lambda x: x.to(device=device, dtype=dtype)  # noqa: E731
    if kw.pop("smoothing", False):
        f32 = lambda x: x.to(device=device, dtype=torch.float32)  # noqa: E731  (the warp computes in fp32)
        kw["flows"] = [f32(cf.flow(B, SIDE, SIDE, +1.0)), f32(cf.flow(B, SIDE, SIDE, -1.0))]
        kw["occs"] = [f32(cf.occ(B, SIDE, SIDE, 5)), f32(cf.occ(B, SIDE, SIDE, 7))]
        kw["saliency"] = f32(torch.sigmoid(cf.feat(B, 1, SIDE // 2, SIDE // 2, 1.0)))
    kw.update(cond_scale=list(COND_SCALE), num_inference_steps=len(STEPS), guidance_scale=GUIDANCE)
    return (to(imgs), to(embeds), to(edges)), kw


def _cast(x, dtype):
    if torch.is_tensor(x) and x.is_floating_point():
        return x.to(dtype)
    if isinstance(x, (list, tuple)):
        return type(x)(_cast(v, dtype) for v in x)
    return x


def net(fn, net_dtype, like):
    """fn with its floating tensors cast to net_dtype and its results cast back to `like`'s dtype: the stand-in networks
    computing in fp16 inside a float64 restatement (net_dtype None: fn itself)"""
    if net_dtype is None:
        return fn
    return lambda *a, **k: _cast(fn(*_cast(a, net_dtype), **{n: _cast(v, net_dtype) for n, v in k.items()}), like.dtype)


def step_model(pipe, model_output, timestep, sample, generator, q, warp_tensor, flows=None, occs=None, saliency=None,
               net_dtype=None):
    """step() (pipe_FRESCO.py:14-77) without its debug view; repeat_noise is never passed by inference()"""
    scheduler = pipe.scheduler
    prev_timestep = scheduler.previous_timestep(timestep)
    alpha_prod_t = scheduler.alphas_cumprod[timestep]
    alpha_prod_t_prev = scheduler.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else scheduler.one
    beta_prod_t = 1 - alpha_prod_t
    beta_prod_t_prev = 1 - alpha_prod_t_prev
    current_alpha_t = alpha_prod_t / alpha_prod_t_prev
    current_beta_t = 1 - current_alpha_t
    x0 = q(q(sample - q(beta_prod_t ** 0.5 * model_output)) / alpha_prod_t ** 0.5)
    if saliency is not None and flows is not None and occs is not None:
        sf = pipe.vae.config.scaling_factor
        image = q(net(lambda z: pipe.vae.decode(z).sample, net_dtype, sample)(q(x0 / sf)))
        image = q(warp_tensor(image, flows, occs, saliency, unet_chunk_size=1))
        x0 = q(sf * q(net(lambda im: pipe.vae.encode(im).latent_dist.sample(), net_dtype, sample)(image)))
    c_x0 = (alpha_prod_t_prev ** 0.5 * current_beta_t) / beta_prod_t
    c_xt = current_alpha_t ** 0.5 * beta_prod_t_prev / beta_prod_t
    mean = q(q(c_x0 * x0) + q(c_xt * sample))
    variance = torch.clamp(beta_prod_t_prev / beta_prod_t * current_beta_t, min=1e-20)
    noise = q(torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype))
    return q(mean + q(variance ** 0.5 * noise)), x0


@torch.no_grad()
def inference_model(pipe, controlnet, frescoProc, imgs, prompt_embeds, edges, timesteps, cond_scale=[0.7] * 20,
                    num_inference_steps=20, num_warmup_steps=6, do_classifier_free_guidance=True, seed=0, guidance_scale=7.5,
                    use_controlnet=True, record_latents=None, propagation_mode=False, flows=None, occs=None, saliency=None,
                    repeat_noise=False, num_intraattn_steps=1, step_interattn_end=350, bg_smoothing_steps=[16, 17],
                    q=identity, warp_tensor=None, net_dtype=None, step_fn=None):
    """inference() (pipe_FRESCO.py:80-234); `timesteps` lives where the scheduler's alphas_cumprod lives (the CPU).
    net_dtype: the dtype the stand-in networks compute in when it is not the tensors' own (see `net`).  step_fn: a step()
    with the reference's signature in place of step_model (tools/bench_loop.py: the route before fresco_amd.inference)."""
    record_latents = [] if record_latents is None else record_latents
    device = pipe._execution_device
    generator = torch.Generator(device=device).manual_seed(seed)
    B, C, H, W = imgs.shape
    latents = q(pipe.prepare_latents(B, pipe.unet.config.in_channels, H, W, prompt_embeds.dtype, device, generator,
                                     latents=None))
    if repeat_noise:
        latents = latents[0:1].repeat(B, 1, 1, 1)
    if num_warmup_steps < 0:
        num_warmup_steps = 0
    else:
        encode = net(lambda im: pipe.vae.encode(im).latent_dist.sample(), net_dtype, imgs)
        latent_x0 = q(pipe.vae.config.scaling_factor * q(encode(imgs.to(pipe.unet.dtype))))
        latents = q(pipe.scheduler.add_noise(latent_x0, latents, timesteps[num_warmup_steps]))
    with pipe.progress_bar(total=num_inference_steps - num_warmup_steps) as progress_bar:
        for i, t in enumerate(timesteps[num_warmup_steps:]):
            if i >= num_intraattn_steps:
                frescoProc.controller.disable_intraattn()
            if t < step_interattn_end:
                frescoProc.controller.disable_interattn()
            if propagation_mode:
                latents[0:2] = record_latents[i].detach().clone()
                record_latents[i] = latents[[0, len(latents) - 1]].detach().clone()
            else:
                record_latents += [latents[[0, len(latents) - 1]].detach().clone()]
            model_input = torch.cat([latents] * 2) if do_classifier_free_guidance else latents
            down, mid = None, None
            if use_controlnet:
                down, mid = net(controlnet, net_dtype, latents)(model_input, t, encoder_hidden_states=prompt_embeds, controlnet_cond=edges,
                                       conditioning_scale=cond_scale[i + num_warmup_steps], guess_mode=False,
                                       return_dict=False)
                down, mid = [q(r) for r in down], q(mid)
            unet = net(pipe.unet, net_dtype, latents)
            noise_pred = q(unet(model_input, t, encoder_hidden_states=prompt_embeds, cross_attention_kwargs=None,
                                down_block_additional_residuals=down, mid_block_additional_residual=mid, return_dict=False)[0])
            if do_classifier_free_guidance:
                uncond, text = noise_pred.chunk(2)
                noise_pred = q(uncond + q(guidance_scale * q(text - uncond)))
            smooth = dict(flows=flows, occs=occs, saliency=saliency) if i + num_warmup_steps in bg_smoothing_steps else {}
            if step_fn is not None:
                latents = step_fn(pipe, noise_pred, t, latents, generator, **smooth)[0]
            else:
                latents = step_model(pipe, noise_pred, t, latents, generator, q, warp_tensor, net_dtype=net_dtype, **smooth)[0]
            if i == len(timesteps) - 1 or ((i + 1) > 0 and (i + 1) % pipe.scheduler.order == 0):
                progress_bar.update()
    return latents


def image_to_frames_model(img):
    """tensor2numpy (src/utils.py:17-21) on a CPU tensor, restated; fp16 and fp32 take the same steps in their format"""
    image = (img / 2 + 0.5).clamp(0, 1)
    image = image.detach().cpu().permute(0, 2, 3, 1).numpy()
    with np.errstate(invalid="ignore"):
        return (image * 255).round().astype("uint8")


def all_half_patterns():
    """every fp16 bit pattern, as a (1, 1, 256, 256) tensor"""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.float16).reshape(1, 1, 256, 256).copy())


def replay_randn(draws, device=None):
    """a torch.randn that hands out the recorded draws in order, in the dtype and on the device asked for"""
    it = iter(draws)

    def randn(shape, generator=None, device=device, dtype=None, **kw):
        z = next(it)
        z = z if torch.is_tensor(z) else torch.from_numpy(z)
        assert tuple(z.shape) == tuple(shape), (tuple(z.shape), tuple(shape))
        return z.to(device=device, dtype=dtype)

    return randn
