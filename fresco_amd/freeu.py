"""FreeU on the HIP kernels, behind the names and signatures of the reference's src/free_lunch_utils.py.

``apply_freeu(pipe, b1, b2, s1, s2)`` replaces the forward of every ``UpBlock2D`` / ``CrossAttnUpBlock2D`` of
``pipe.unet.up_blocks`` (recognised by class name, as the reference does).  At a resnet whose incoming hidden state has
1280 or 640 channels the replacement makes two library calls that write straight into the concat tensor
(ops.freeu_site): the backbone scaling of the first half of the channels, in place like the reference's slice
assignment, and the skip connection's Fourier filter in closed form.  Anywhere else it is a plain ``torch.cat``.

Deviations from the reference, all in DESIGN.md section 11: fp32 arithmetic with one rounding at the store (the reference
keeps fp16 through its FFT on power-of-two planes), ``s == 1`` copies the skip (the reference returns it up to FFT
noise), and only ``threshold == 1`` -- the one value the reference passes -- is built.  The training /
gradient-checkpointing branch is not.
"""
from typing import Any, Dict, Optional, Tuple

import torch

from . import ops

# channels of the incoming hidden state -> (channels scaled, name of the backbone factor, name of the skip factor)
_SITES = {1280: (640, "b1", "s1"), 640: (320, "b2", "s2")}


def isinstance_str(x, cls_name):
    """True if a class *named* cls_name is in x's ancestry (no access to the class itself needed)."""
    return any(c.__name__ == cls_name for c in type(x).__mro__)


def Fourier_filter(x_in, threshold, scale):
    """free_lunch_utils.Fourier_filter for threshold == 1: same dtype out as in, no FFT."""
    if threshold != 1:
        raise NotImplementedError("fresco_amd Fourier_filter: threshold %r (only 1, the value FreeU passes, is built)"
                                  % (threshold,))
    return ops.freeu_fourier(x_in, scale)


def _join(block, hidden, skip):
    """what the reference does between popping a skip and calling the resnet: FreeU at a 1280 / 640 channel site, then
    the concat"""
    site = _SITES.get(hidden.shape[1])
    if site is None:
        return torch.cat([hidden, skip], dim=1)
    n_scaled, b_name, s_name = site
    b, s = getattr(block, b_name), getattr(block, s_name)
    if hidden.is_contiguous():
        return ops.freeu_site(hidden, skip, n_scaled, b, s)
    work = hidden.contiguous()
    cat = ops.freeu_site(work, skip, n_scaled, b, s)
    hidden.copy_(work)  # the in-place update reaches whoever holds the incoming tensor
    return cat


def _run(block, hidden, skips, temb, upsample_size, attn_kwargs):
    if block.training and getattr(block, "gradient_checkpointing", False):
        raise NotImplementedError("fresco_amd FreeU: the gradient-checkpointing (training) branch is not built")
    skips = tuple(skips)
    attentions = block.attentions if attn_kwargs is not None else [None] * len(block.resnets)
    for resnet, attn in zip(block.resnets, attentions):
        skip, skips = skips[-1], skips[:-1]
        hidden = resnet(_join(block, hidden, skip), temb)
        if attn is not None:
            hidden = attn(hidden, return_dict=False, **attn_kwargs)[0]
    if block.upsamplers is not None:
        for upsampler in block.upsamplers:
            hidden = upsampler(hidden, upsample_size)
    return hidden


def _up_forward(block):
    def forward(hidden_states, res_hidden_states_tuple, temb=None, upsample_size=None):
        return _run(block, hidden_states, res_hidden_states_tuple, temb, upsample_size, None)

    return forward


def _crossattn_up_forward(block):
    def forward(
        hidden_states: torch.FloatTensor,
        res_hidden_states_tuple: Tuple[torch.FloatTensor, ...],
        temb: Optional[torch.FloatTensor] = None,
        encoder_hidden_states: Optional[torch.FloatTensor] = None,
        cross_attention_kwargs: Optional[Dict[str, Any]] = None,
        upsample_size: Optional[int] = None,
        attention_mask: Optional[torch.FloatTensor] = None,
        encoder_attention_mask: Optional[torch.FloatTensor] = None,
    ):
        kwargs = dict(encoder_hidden_states=encoder_hidden_states, cross_attention_kwargs=cross_attention_kwargs,
                      attention_mask=attention_mask, encoder_attention_mask=encoder_attention_mask)
        return _run(block, hidden_states, res_hidden_states_tuple, temb, upsample_size, kwargs)

    return forward


def _register(model, cls_name, make_forward, b1, b2, s1, s2):
    for block in model.unet.up_blocks:
        if isinstance_str(block, cls_name):
            block.forward = make_forward(block)
            block.b1, block.b2, block.s1, block.s2 = b1, b2, s1, s2


def register_free_upblock2d(model, b1=1.2, b2=1.4, s1=0.9, s2=0.2):
    """free_lunch_utils.register_free_upblock2d: FreeU forward on every UpBlock2D of model.unet.up_blocks."""
    _register(model, "UpBlock2D", _up_forward, b1, b2, s1, s2)


def register_free_crossattn_upblock2d(model, b1=1.2, b2=1.4, s1=0.9, s2=0.2):
    """free_lunch_utils.register_free_crossattn_upblock2d: FreeU forward on every CrossAttnUpBlock2D."""
    _register(model, "CrossAttnUpBlock2D", _crossattn_up_forward, b1, b2, s1, s2)


def apply_freeu(pipe, b1=1.0, b2=1.0, s1=1.0, s2=1.0):
    register_free_upblock2d(pipe, b1, b2, s1, s2)
    register_free_crossattn_upblock2d(pipe, b1, b2, s1, s2)


def patch_free_lunch(flu):
    """Rebind Fourier_filter, the two register_free_* functions and apply_freeu on a module object (the reference's
    src.free_lunch_utils, or a module that imported those names from it) -- the zero-diff form of INTEGRATION.md recipe F."""
    flu.Fourier_filter = Fourier_filter
    flu.register_free_upblock2d = register_free_upblock2d
    flu.register_free_crossattn_upblock2d = register_free_crossattn_upblock2d
    flu.apply_freeu = apply_freeu
    return flu
