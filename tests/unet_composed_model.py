"""One SD-1.5-shaped stand-in of the UNet and the ControlNet, shared by tests/golden/make_unet_composed_golden.py,
tests/test_unet_composed_cpu.py and tests/test_gpu_unet_composed.py: what the four patches (patch_unet_resnets,
patch_unet_transformers, patch_unet_attention, patch_unet_shell), the FRESCO processors, the up-block hook and inference()
are tried on TOGETHER.

The parts are the restated modules the per-module tests already have -- unet_resnet_model.Resnet, unet_transformer_model's
Transformer (its attention layers replaced by unet_attention_model.Attention, which calls a processor), unet_shell_model's
Downsample2D, Upsample2D, Timesteps, TimestepEmbedding and CondEmbedding -- under diffusers' attribute names
(down_blocks.N.resnets / attentions / downsamplers, mid_block, up_blocks.N.resnets / attentions / upsamplers, conv_in,
time_proj, time_embedding, conv_norm_out, conv_act, conv_out, controlnet_cond_embedding, controlnet_down_blocks,
controlnet_mid_block), so the reference's name rule applies as written: `up_blocks.2` and `up_blocks.3` carry the FRESCO
processor (src/diffusion_hacked.py:156, :398).

The forwards restate, in this file's own words,
  * the UNet forward the reference runs (src/diffusion_hacked.py: the timestep :570-605, conv_in :700, the down blocks and
    their skips :707-729, the ControlNet residuals added to the skips :731-740, the mid block and its residual :743-754,
    the up-block hook :757-779, the up blocks :762-800, the output end :803-806, the tuple with the decoder inputs
    :811-812), with the block forwards of diffusers 0.19.3 (models/unet_2d_blocks.py: CrossAttnDownBlock2D, DownBlock2D,
    UNetMidBlock2DCrossAttn, CrossAttnUpBlock2D, UpBlock2D);
  * ControlNetModel.forward of diffusers 0.19.3 (models/controlnet.py; it is not part of the reference tree): conv_in + the
    condition embedding, the down blocks, the mid block, the zero convolutions, `sample * conditioning_scale`.
diffusers is NOT installed where these tests run: names and forwards come from its published source and are UNVERIFIED
against the real modules or a checkpoint.

SHAPE.  Widths 320 (8 heads, head dim 40), 640 (head dim 80) and 1280 (head dim 160); latents 16 x 16 (frames 128 x 128), so
the planes are 16^2, 8^2, 4^2 and 2^2; the text is 77 tokens of width 64.

  level   UNet down_blocks                     ControlNet down_blocks               UNet up_blocks (in call order 0 .. 3)
  16^2    0: resnet 320, transformer, down     0: the same                          3: cat 960->320, tf, cat 640->320, tf
   8^2    1: resnet 320->640, transformer, dn  1: the same                          2: cat 960->640, transformer, up 640
   4^2    2: down 640 (no resnet)              2: the same                          1: cat 1920->640, up 640 (no attention)
   2^2    3: resnet 640->1280 (no attention)   -- (stops at 640)                    0: cat 1920->1280, up 1280 (no attention)
  mid     transformer 1280 (no resnet)         resnet 640, transformer 640; its zero convolution is 640 -> 1280

WHAT WAS CUT, and why: both models together must stay below 250 M parameters (PARAM_LIMIT; SD-1.5's pair has 1.2 G) and
one 1280-wide 3 x 3 convolution alone has 14.7 M.  layers_per_block is 1 (an up block then has as many resnets as it has
skips to take).  The depth at 1280 is cut to one of each KIND of site: one resnet that enters the width (640 -> 1280), one
transformer (the mid block, without the resnet in front of it), one concatenating resnet (1920 -> 1280) and one
Upsample2D.  The third level is 640 wide and holds only its Downsample2D, `up_blocks.1` is 640 wide without attention, and
the ControlNet stops at 640: its mid zero convolution maps 640 -> 1280.  No kind of site is missing: concatenating resnets
at 640 -> 320, 960 -> 320, 960 -> 640, 1920 -> 640 and 1920 -> 1280 (a channels_last tensor and a skip tensor through
torch.cat), a transformer at 320, 640 and 1280, Downsample2D at 320 and 640, Upsample2D at 1280 and 640, conv_in, the
output end, the time MLP, the condition embedding, five zero convolutions and the mid one.

  * weights: `standin_state_dict`: unet_transformer_model.standin_value's closed forms seeded by (tag, parameter name),
    to_q / to_k times unet_attention_model.QK_GAIN, the zero convolutions times ZERO_GAIN (a trained ControlNet's are not
    zero), the condition embedding's convolutions times COND_GAIN (with plain fan-in scaling its eight layers damp the
    edges to 2 % of its output and an embedding of the wrong edges could not show), rounded to fp16 once: the float64, fp32, fp16 and bf16-rounded builds carry the same values;
  * `q`: the rounding hook of the other restatements, applied to every layer's output (the models keep it as the attribute
    `q`, so that loop_model.inference_model, which knows nothing of it, drives them): the identity for the float64 record,
    a round trip through fp16 for the reference arithmetic's noise (fp32, every layer's output rounded), through bf16 for
    the bf16 noise;
  * `fresco`: a `Fresco` object switches the UNet's FRESCO sites on for the record: oracle.fresco_oracle's
    fresco_attention on `attn1` of up_blocks.2 / up_blocks.3 (cross-frame keys and the temporal pass), and adain +
    warp_tensor at the input of every up block (optimize_feature with iters = 0 is its AdaIN epilogue).  All three run in
    the dtype they are given: float64 for the record.  The same object is the restatement's controller: the store pass
    (`store_pass`, what get_intraframe_paras does) fills its list of reference features, the spatial-guided pass reads them
    through a cyclic index, and loop_model.inference_model switches it as the reference's loop switches AttentionControl
    (`SeqModels`, `derive_seq`: the records `store`, `full` and `seq` of unet_composed_seq_golden.npz);
  * `fault`: one planted fault of FAULTS, for the discrimination checks of tests/test_unet_composed_cpu.py.
"""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

import loop_model as L
import unet_attention_model as A
import unet_resnet_model as R
import unet_shell_model as S
import unet_transformer_model as T
from vae_model import round16  # noqa: F401

GOLDEN_FILE = "unet_composed_golden.npz"
PARAM_LIMIT = 250_000_000
HEADS = 8
TEXT_TOKENS, TEXT_WIDTH = 77, 64
FRAMES, SIDE = 2, 128            # frames per CFG half; latents are SIDE // 8
LAT = SIDE // 8
ZERO_GAIN = 0.5
COND_GAIN = 1.75                 # on the condition embedding's convolutions: eight layers behind SiLUs would damp the edges away
ACT_LIMIT = 65504.0 / 8
COND_SCALE = 0.75                # of the single calls
STEPS3 = L.STEPS[3:]             # the loop case: num_warmup_steps = 3 of loop_model's six steps
LOOP_KW = dict(num_warmup_steps=3, seed=21, cond_scale=list(L.COND_SCALE), num_inference_steps=len(L.STEPS),
               guidance_scale=L.GUIDANCE)
FAULTS = ("stale_input", "swapped_text", "edited_edges", "swapped_cat", "no_mid_residual", "timestep_off")
TAPS = ("mid", "up2")            # the UNet's mid block output with its residual; the output of up_blocks.2

_ident = lambda t: t  # noqa: E731


def round_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _call(m, q, *args, **kw):
    """a patched module takes no q"""
    return m(*args, **kw) if q is _ident else m(*args, q=q, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# processors of the restatement
# ---------------------------------------------------------------------------------------------------------------------
class Fresco:
    """what the record's FRESCO sites read: flows / occs / saliency of the hook, per token count the cross-frame mask and
    the trajectory map of the processor, and the controller: its three switches, and the store of the spatial-guided pass --
    a list of reference features, a read index and a store switch that behave as fresco_amd/control.py's do (append when
    storing; read store[index], advance, wrap to 0), under the method names the loop calls.
    hook_steps: the timesteps the hook is active on (None: on every call), as apply_FRESCO_opt's `steps`."""

    def __init__(self, flows, occs, saliency, cf_masks, fwd_maps, tmasks):
        self.flows, self.occs, self.saliency = flows, occs, saliency
        self.cf_masks = {m.shape[1]: m for m in cf_masks}
        self.fwd_maps = {f.shape[2]: f[:, 0] for f in fwd_maps}
        self.tmasks = {f.shape[2]: t[:, 0] for f, t in zip(fwd_maps, tmasks)}
        self.use_cfattn = self.use_interattn = self.hook = True
        self.use_intraattn = self.store = False
        self.stored, self.index = [], 0
        self.intra_scale, self.intra_bias = 0.2, 0.0     # AttentionControl's intraattn_scale_factor and intraattn_bias
        self.hook_steps = None
        self.own_refs = False                            # the planted fault "own_refs"

    def flags(self):
        return (int(self.use_intraattn), int(self.use_interattn), int(self.use_cfattn), int(self.index))

    def clear_store(self):
        self.stored = []
        self.disable_intraattn()

    def enable_store(self):
        self.store = True

    def disable_store(self):
        self.store = False

    def enable_intraattn(self):
        self.index, self.store = 0, False
        self.use_intraattn = len(self.stored) > 0        # nothing recorded: stays off

    def disable_intraattn(self):
        self.index, self.use_intraattn, self.store = 0, False, False

    def disable_interattn(self):
        self.use_interattn = False

    def disable_controller(self):
        self.disable_intraattn()
        self.use_interattn = self.use_cfattn = False

    def enable_controller(self):
        self.enable_intraattn()
        self.use_interattn = self.use_cfattn = True

    def read(self):
        """AttentionControl.forward(None) with use_intraattn on"""
        ref = self.stored[self.index]
        self.index += 1
        if self.index >= len(self.stored):
            self.index, self.store = 0, False
        return ref


class OracleFrescoProcessor:
    """FRESCOAttnProcessor2_0 restated through the oracle: self-attention is fresco_oracle.fresco_attention with whatever
    `fresco` has switched on (the spatial-guided pass reads the next stored reference); while `fresco` stores, the
    self-attention input is appended first (diffusion_hacked.py:206-207); cross-attention is the plain processor"""

    def __init__(self, fresco, q=_ident):
        self.fresco, self.q, self.plain = fresco, q, A.RefProcessor(q)

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        from oracle import fresco_oracle as O
        f = self.fresco
        if encoder_hidden_states is None and f.store:
            f.stored.append(hidden_states.detach().clone())
        if encoder_hidden_states is not None or not (f.use_cfattn or f.use_interattn or f.use_intraattn):
            return self.plain(attn, hidden_states, encoder_hidden_states, attention_mask, temb)
        assert attention_mask is None
        hw = hidden_states.shape[1]
        dt = hidden_states.dtype
        kw = {}
        if f.use_intraattn:
            ref = f.read()
            if f.own_refs:
                ref = hidden_states
            assert ref.shape == hidden_states.shape, (tuple(ref.shape), tuple(hidden_states.shape))
            kw.update(ref=ref.to(dt), intra_scale=f.intra_scale, intra_bias=f.intra_bias)
        if f.use_cfattn:
            kw.update(use_cf=True, cf_mask=f.cf_masks[hw])
        if f.use_interattn:
            kw.update(fwd_map=f.fwd_maps[hw], tmask=f.tmasks[hw])
        W = [m.weight.to(dt) for m in (attn.to_q, attn.to_k, attn.to_v, attn.to_out[0])]
        rd = None if self.q is _ident else (torch.bfloat16 if self.q is round_bf16 else torch.float16)
        return O.fresco_attention(hidden_states, W[0], W[1], W[2], W[3], attn.to_out[0].bias.to(dt), attn.heads,
                                  round_dtype=rd, chunk=2, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# blocks (diffusers 0.19.3, models/unet_2d_blocks.py, restated)
# ---------------------------------------------------------------------------------------------------------------------
def transformer(c, cross_dim=TEXT_WIDTH):
    """unet_transformer_model.Transformer whose attention layers are unet_attention_model.Attention modules (same parameter
    names): they hand their call to a processor, as diffusers' do"""
    tf = T.Transformer(c, HEADS, cross_dim)
    for blk in tf.transformer_blocks:
        blk.attn1 = A.Attention(c, HEADS)
        blk.attn2 = A.Attention(c, HEADS, cross_dim)
    return tf


class DownBlock(nn.Module):
    """CrossAttnDownBlock2D / DownBlock2D: resnet [, transformer] per layer, then the downsamplers; every output is a skip"""

    def __init__(self, cin, cout, resnet=True, attention=True, down=True, skip_layers=True):
        super().__init__()
        self.has_cross_attention = attention
        self.skip_layers = skip_layers     # (cut: False keeps only the downsampler's output as a skip)
        self.resnets = nn.ModuleList([R.Resnet(cin, cout)] if resnet else [])
        if attention:
            self.attentions = nn.ModuleList([transformer(cout)])
        self.downsamplers = nn.ModuleList([S.Downsample2D(cout)]) if down else None

    def forward(self, hidden_states, temb=None, encoder_hidden_states=None, cross_attention_kwargs=None, q=_ident):
        skips = ()
        for i, resnet in enumerate(self.resnets):
            hidden_states = _call(resnet, q, hidden_states, temb)
            if self.has_cross_attention:
                hidden_states = _call(self.attentions[i], q, hidden_states, encoder_hidden_states=encoder_hidden_states,
                                      cross_attention_kwargs=cross_attention_kwargs, return_dict=False)[0]
            if self.skip_layers:
                skips += (hidden_states,)
        if self.downsamplers is not None:
            for d in self.downsamplers:
                hidden_states = _call(d, q, hidden_states)
            skips += (hidden_states,)
        return hidden_states, skips


class MidBlock(nn.Module):
    """UNetMidBlock2DCrossAttn, cut: [one resnet,] one transformer"""

    def __init__(self, c, resnet):
        super().__init__()
        self.has_cross_attention = True
        self.resnets = nn.ModuleList([R.Resnet(c, c)] if resnet else [])
        self.attentions = nn.ModuleList([transformer(c)])

    def forward(self, hidden_states, temb=None, encoder_hidden_states=None, cross_attention_kwargs=None, q=_ident):
        for resnet in self.resnets:
            hidden_states = _call(resnet, q, hidden_states, temb)
        return _call(self.attentions[0], q, hidden_states, encoder_hidden_states=encoder_hidden_states,
                     cross_attention_kwargs=cross_attention_kwargs, return_dict=False)[0]


class UpBlock(nn.Module):
    """CrossAttnUpBlock2D / UpBlock2D: per layer torch.cat([hidden_states, the last skip]), resnet [, transformer]; then the
    upsamplers.  skip_channels: the widths of the skips in the order they are taken"""

    def __init__(self, cin, cout, skip_channels, attention=True, up=True):
        super().__init__()
        self.has_cross_attention = attention
        self.resnets = nn.ModuleList([R.Resnet((cin if i == 0 else cout) + s, cout) for i, s in enumerate(skip_channels)])
        if attention:
            self.attentions = nn.ModuleList([transformer(cout) for _ in skip_channels])
        self.upsamplers = nn.ModuleList([S.Upsample2D(cout)]) if up else None
        self.swap_cat = False     # the planted fault "swapped_cat"

    def forward(self, hidden_states, res_hidden_states_tuple=(), temb=None, encoder_hidden_states=None,
                cross_attention_kwargs=None, upsample_size=None, q=_ident):
        for i, resnet in enumerate(self.resnets):
            res = res_hidden_states_tuple[-1]
            res_hidden_states_tuple = res_hidden_states_tuple[:-1]
            pair = [res, hidden_states] if self.swap_cat and i == 0 else [hidden_states, res]
            hidden_states = _call(resnet, q, torch.cat(pair, dim=1), temb)
            if self.has_cross_attention:
                hidden_states = _call(self.attentions[i], q, hidden_states, encoder_hidden_states=encoder_hidden_states,
                                      cross_attention_kwargs=cross_attention_kwargs, return_dict=False)[0]
        if self.upsamplers is not None:
            for u in self.upsamplers:
                hidden_states = _call(u, q, hidden_states, upsample_size)
        return hidden_states


class _Model(nn.Module):
    """what both models share: conv_in, the time MLP, the processors' table, the attributes of the restatement"""

    def _shared(self):
        self.conv_in = nn.Conv2d(4, 320, 3, padding=1)
        self.time_proj = S.Timesteps(320, True, 0)
        self.time_embedding = S.TimestepEmbedding(320, 1280)
        self.config = types.SimpleNamespace(in_channels=4)
        self.q = _ident
        self.fault = None

    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    # ---- diffusers' processor table (models/unet_2d_condition.py: attn_processors, set_attn_processor) ----------------
    def _attention_modules(self):
        return [(name, m) for name, m in self.named_modules() if isinstance(m, A.Attention)]

    @property
    def attn_processors(self):
        return OrderedDict((name + ".processor", m.processor) for name, m in self._attention_modules())

    def set_attn_processor(self, processor):
        mods = self._attention_modules()
        if isinstance(processor, dict):
            assert len(processor) == len(mods), (len(processor), len(mods))
        for name, m in mods:
            m.set_processor(processor[name + ".processor"] if isinstance(processor, dict) else processor)

    def _emb(self, sample, timestep, q):
        """:570-605: a 0-dim timestep becomes one per image; the sinusoid is fp32 (float64 beside float64 samples) and is cast to
        the sample's dtype"""
        timesteps = timestep
        if not torch.is_tensor(timesteps):
            timesteps = torch.tensor([timesteps], device=sample.device)
        elif timesteps.dim() == 0:
            timesteps = timesteps[None].to(sample.device)
        timesteps = timesteps.expand(sample.shape[0])
        t_emb = self.time_proj(timesteps.to(torch.float64 if sample.dtype == torch.float64 else torch.float32))
        t_emb = q(t_emb.to(dtype=sample.dtype))
        return self.time_embedding(t_emb) if q is _ident else self.time_embedding(t_emb, None, q)


class UNet(_Model):
    def __init__(self):
        super().__init__()
        self._shared()
        self.down_blocks = nn.ModuleList([DownBlock(320, 320), DownBlock(320, 640, skip_layers=False),
                                          DownBlock(640, 640, resnet=False, attention=False),
                                          DownBlock(640, 1280, attention=False, down=False)])
        self.mid_block = MidBlock(1280, resnet=False)
        # the skips, first to last: conv_in 320 @16, resnet 320 @16, down 320 @8, down 640 @4, down 640 @2, resnet 1280 @2 --
        # the last is the mid block's input and no block takes it as a skip (dropped in forward); down_blocks.1's resnet
        # output is no skip either (skip_layers=False), so that up_blocks.2 holds one resnet, 640 + 320 -> 640
        self.up_blocks = nn.ModuleList([UpBlock(1280, 1280, [640], attention=False), UpBlock(1280, 640, [640], attention=False),
                                        UpBlock(640, 640, [320]), UpBlock(640, 320, [320, 320], up=False)])
        self.conv_norm_out = nn.GroupNorm(32, 320, eps=1e-5)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(320, 4, 3, padding=1)
        self.fresco = None
        self.taps = None          # a dict that receives TAPS
        self.ups = None           # a list that receives every up block's input, before the hook (:773-774, :811-812)
        self.inputs = []          # every call's sample, as loop_model.UNet keeps them
        self.on_call = None

    def forward(self, sample, timestep, encoder_hidden_states=None, cross_attention_kwargs=None,
                down_block_additional_residuals=None, mid_block_additional_residual=None, return_dict=True, q=None):
        q = self.q if q is None else q
        if self.on_call is not None:
            self.on_call()
        self.inputs.append(sample.detach().clone())
        if self.fault == "stale_input" and len(self.inputs) > 1:
            sample = self.inputs[-2]                                       # conv_in reads the previous call's input
        if self.fault == "timestep_off":
            timestep = timestep - 150                                      # one step of loop_model.Scheduler
        if self.fault == "swapped_text":
            encoder_hidden_states = torch.cat(list(encoder_hidden_states.chunk(2))[::-1])
        emb = self._emb(sample, timestep, q)
        sample = q(self.conv_in(sample))                                   # :700
        skips = (sample,)
        for blk in self.down_blocks:                                       # :707-729
            kw = dict(encoder_hidden_states=encoder_hidden_states, cross_attention_kwargs=cross_attention_kwargs) \
                if blk.has_cross_attention else {}
            sample, res = _call(blk, q, hidden_states=sample, temb=emb, **kw)
            skips += res
        skips = skips[:-1]        # (cut: down_blocks.3's resnet output feeds the mid block only)
        if down_block_additional_residuals is not None:                    # :731-740
            assert len(down_block_additional_residuals) == len(skips)
            skips = tuple(q(s + r) for s, r in zip(skips, down_block_additional_residuals))
        sample = _call(self.mid_block, q, sample, emb, encoder_hidden_states=encoder_hidden_states,
                       cross_attention_kwargs=cross_attention_kwargs)     # :743-751
        if mid_block_additional_residual is not None and self.fault != "no_mid_residual":
            sample = q(sample + mid_block_additional_residual)             # :753-754
        if self.taps is not None:
            self.taps["mid"] = sample
        for i, blk in enumerate(self.up_blocks):                           # :762-800
            n = len(blk.resnets)
            res, skips = skips[-n:], skips[:-n]
            if self.ups is not None:
                self.ups.append(sample)
            sample = self._hook(sample, q, timestep)                       # :773-779
            kw = dict(encoder_hidden_states=encoder_hidden_states, cross_attention_kwargs=cross_attention_kwargs) \
                if blk.has_cross_attention else {}
            sample = _call(blk, q, hidden_states=sample, temb=emb, res_hidden_states_tuple=res, **kw)
            if self.taps is not None and i == 2:
                self.taps["up2"] = sample
        assert not skips
        sample = q(self.conv_act(q(self.conv_norm_out(sample))))           # :803-805
        sample = q(self.conv_out(sample))
        return types.SimpleNamespace(sample=sample) if return_dict else (sample,)

    def _hook(self, sample, q, timestep=None):
        """optimize_feature with iters = 0 (its AdaIN epilogue) and warp_tensor with the saliency, in the sample's dtype; with
        hook_steps only on those timesteps (`timestep in steps`, :775)"""
        f = self.fresco
        if f is None or not f.hook or (f.hook_steps is not None and int(timestep) not in f.hook_steps):
            return sample
        from oracle import fresco_oracle as O
        sample = q(O.adain(q(sample), sample))
        return q(O.warp_tensor(sample, f.flows, f.occs, f.saliency, 2, compute_dtype=sample.dtype))


class ControlNet(_Model):
    def __init__(self):
        super().__init__()
        self._shared()
        self.controlnet_cond_embedding = S.CondEmbedding(320)
        self.down_blocks = nn.ModuleList([DownBlock(320, 320), DownBlock(320, 640, skip_layers=False),
                                          DownBlock(640, 640, resnet=False, attention=False)])
        self.mid_block = MidBlock(640, resnet=True)
        self.controlnet_down_blocks = nn.ModuleList([nn.Conv2d(c, c, 1) for c in (320, 320, 320, 640, 640)])
        self.controlnet_mid_block = nn.Conv2d(640, 1280, 1)
        self.edges_seen = 0

    def forward(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, conditioning_scale=1.0,
                guess_mode=False, return_dict=True, q=None):
        q = self.q if q is None else q
        assert guess_mode is False
        self.edges_seen += 1
        if self.fault == "edited_edges" and self.edges_seen > 1:
            controlnet_cond = controlnet_cond * 0.5                        # the embedding of edges edited after the first call
        emb = self._emb(sample, timestep, q)
        sample = q(self.conv_in(sample))
        cond = _call(self.controlnet_cond_embedding, q, controlnet_cond)
        sample = q(sample + cond)
        skips = (sample,)
        for blk in self.down_blocks:
            kw = dict(encoder_hidden_states=encoder_hidden_states) if blk.has_cross_attention else {}
            sample, res = _call(blk, q, hidden_states=sample, temb=emb, **kw)
            skips += res
        sample = _call(self.mid_block, q, sample, emb, encoder_hidden_states=encoder_hidden_states)
        down = [q(q(z(s)) * conditioning_scale) for z, s in zip(self.controlnet_down_blocks, skips)]
        assert len(down) == len(skips) == len(self.controlnet_down_blocks)
        mid = q(q(self.controlnet_mid_block(sample)) * conditioning_scale)
        return types.SimpleNamespace(down_block_res_samples=down, mid_block_res_sample=mid) if return_dict else (down, mid)


# ---------------------------------------------------------------------------------------------------------------------
# weights and builds
# ---------------------------------------------------------------------------------------------------------------------
def standin_state_dict(module, tag):
    """float64 values, each rounded to fp16 once: unet_transformer_model.standin_value per (tag, name); to_q / to_k carry
    unet_attention_model.QK_GAIN, the zero convolutions ZERO_GAIN, the condition embedding's COND_GAIN"""
    sd = OrderedDict()
    for name, v in module.state_dict().items():
        val = np.asarray(T.standin_value("%s.%s" % (tag, name), name, tuple(v.shape)), np.float64)
        if name.endswith(("to_q.weight", "to_k.weight")):
            val = val * A.QK_GAIN
        if name.startswith(("controlnet_down_blocks", "controlnet_mid_block")):
            val = val * ZERO_GAIN
        if name.startswith("controlnet_cond_embedding") and name.endswith(".weight"):
            val = val * COND_GAIN
        sd[name] = torch.from_numpy(val.astype(np.float16).astype(np.float64))
    return sd


_WEIGHTS = {}


def weights(kind):
    """the float64 state dict of a model, drawn once per process"""
    if kind not in _WEIGHTS:
        with torch.device("meta"):
            shapes = {"unet": UNet, "controlnet": ControlNet}[kind]()
        _WEIGHTS[kind] = standin_state_dict(shapes, "composed_" + kind)
    return _WEIGHTS[kind]


def build(kind, dtype=torch.float32, device=None):
    """the model with its stand-in weights in eval mode; every attention module carries a plain RefProcessor"""
    with torch.device("meta"):
        net = {"unet": UNet, "controlnet": ControlNet}[kind]()
    net = net.to_empty(device="cpu").to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in weights(kind).items()})
    if device is not None:
        net = net.to(device)
    return net.eval()


def parameters_of(net):
    return sum(p.numel() for p in net.parameters())


def set_rounding(net, q):
    """the rounding hook on the model and on every plain processor of it"""
    net.q = q
    for _, m in net._attention_modules():
        m.set_processor(A.RefProcessor(q))


def fresco_names(unet):
    """the attention modules the reference's name rule gives the FRESCO processor"""
    return [name for name, _ in unet._attention_modules() if name.startswith(("up_blocks.2", "up_blocks.3"))]


def set_fresco(unet, fresco, q=_ident):
    """the record's FRESCO sites: OracleFrescoProcessor on up_blocks.2 / up_blocks.3, the hook on every up block"""
    unet.fresco = fresco
    proc = OracleFrescoProcessor(fresco, q)
    for name, m in unet._attention_modules():
        if name.startswith(("up_blocks.2", "up_blocks.3")):
            m.set_processor(proc)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def call_inputs():
    """one ControlNet + UNet call on 2 frames x 2 CFG halves, fp16 values: latents (4, 4, 16, 16) with both halves equal (as
    the loop's torch.cat([latents] * 2)), the last frame scaled and shifted; a 0-dim timestep; the text (4, 77, 64), the
    halves different; the edges (4, 3, 128, 128) in [0, 1], both halves equal"""
    rs = np.random.RandomState(77)
    x = rs.standard_normal((FRAMES, 4, LAT, LAT))
    x[-1] = x[-1] * 0.5 + 0.5
    text = rs.standard_normal((2 * FRAMES, TEXT_TOKENS, TEXT_WIDTH))
    text[FRAMES:] = text[FRAMES:] * 0.75 + 0.4
    edges = rs.uniform(0.0, 1.0, (FRAMES, 3, SIDE, SIDE))
    h = lambda a: torch.from_numpy(np.concatenate([a, a]) if a.shape[0] == FRAMES else a).to(torch.float16)  # noqa: E731
    return h(x), torch.tensor(451), h(text), h(edges)


def fresco_inputs():
    """as tests/test_gpu_integration.py makes them: synth.make_flows, the oracle's mapping_ind and cross_frame_masks at the
    token counts of up_blocks.2 (8 x 8, scale 16) and up_blocks.3 (16 x 16, scale 8) -> dict of CPU tensors"""
    import synth
    from oracle import fresco_oracle as O
    g = synth.gen(41)
    flows, occs = synth.make_flows(FRAMES, SIDE, g)
    sal = torch.rand(FRAMES, 1, SIDE // 2, SIDE // 2, generator=g)
    imgs = torch.rand(FRAMES, 3, SIDE, SIDE, generator=g)
    maps = [O.mapping_ind(flows[1], occs[1], imgs, scale=s) for s in (8.0, 16.0)]
    cfm = O.cross_frame_masks(occs[1], scales=(8.0, 16.0))
    return dict(flows=flows, occs=occs, saliency=sal, cf_masks=list(cfm), fwd_maps=[m[0] for m in maps],
                bwd_maps=[m[1] for m in maps], tmasks=[m[2] for m in maps])


def make_fresco(dtype):
    fi = fresco_inputs()
    c = lambda ts: [t.to(dtype) for t in ts]  # noqa: E731
    return Fresco(c(fi["flows"]), c(fi["occs"]), fi["saliency"].to(dtype), fi["cf_masks"], fi["fwd_maps"], fi["tmasks"])


def loop_inputs(device="cpu", dtype=torch.float64):
    """(imgs, prompt_embeds, edges) of the loop case: 2 frames of 128 x 128 in [-1, 1], call_inputs' text and edges"""
    rs = np.random.RandomState(78)
    imgs = torch.from_numpy(np.tanh(rs.standard_normal((FRAMES, 3, SIDE, SIDE)))).to(torch.float16)
    _, _, text, edges = call_inputs()
    return tuple(t.to(device=device, dtype=dtype) for t in (imgs, text, edges))


# ---------------------------------------------------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------------------------------------------------
def run_call(unet, controlnet, x, t, text, edges, scale=COND_SCALE):
    """the ControlNet and then the UNet with its residuals, as one step of inference() calls them -> (noise prediction, down
    residuals, mid residual)"""
    down, mid = controlnet(x, t, encoder_hidden_states=text, controlnet_cond=edges, conditioning_scale=scale, guess_mode=False,
                           return_dict=False)
    out = unet(x, t, encoder_hidden_states=text, cross_attention_kwargs=None, down_block_additional_residuals=down,
               mid_block_additional_residual=mid, return_dict=False)[0]
    return out, down, mid


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def call_record(unet, controlnet, dtype, edges_gain=1.0, text_gain=1.0, device="cpu", inputs=None, input_q=_ident):
    """{"out": the noise prediction (n, 4, H, W), "res": every ControlNet residual thinned and flattened, TAPS thinned} of
    one call in `dtype` on call_inputs (or on `inputs`, tensors the caller keeps, as they are), as float64 numpy.  input_q: a
    rounding of call_inputs' fp16 values (round_bf16 for the bf16 case: what a cast of them to bf16 gives)"""
    if inputs is None:
        x, t, text, edges = call_inputs()
        inputs = (input_q(x.to(device, dtype)), t.to(device), input_q(text.to(device, dtype)) * text_gain,
                  input_q(edges.to(device, dtype)) * edges_gain)
    unet.taps = {}
    with torch.no_grad():
        out, down, mid = run_call(unet, controlnet, *inputs)
    taps, unet.taps = unet.taps, None
    rec = {"out": out.double().cpu().numpy(),
           "res": np.concatenate([R.thin(nhwc(r).double()).reshape(-1) for r in list(down) + [mid]])}
    for k in TAPS:
        rec[k] = R.thin(nhwc(taps[k]).double())
    return rec


class Pipe(L.Pipe):
    """loop_model.Pipe with its UNet and ControlNet replaced by the composed stand-ins"""

    def __init__(self, device, dtype, unet, controlnet, sched_dtype=torch.float64):
        super().__init__(device, dtype, sched_dtype)
        self.unet, self.controlnet = unet, controlnet
        unet.inputs = []
        controlnet.edges_seen = 0


def recording_randn(draws):
    """a torch.randn that records what it hands out (the golden maker), in float64 rounded to fp16 values"""
    def randn(shape, generator=None, device=None, dtype=None, **kw):
        z = torch.empty(tuple(shape), dtype=torch.float64).normal_(generator=generator)
        z = z.to(torch.float16).to(torch.float64)
        draws.append(z.numpy().copy())
        return z.to(dtype=dtype)
    return randn


def loop_record(unet, controlnet, dtype, randn, loop_q=L.identity):
    """three steps of loop_model.inference_model on the stand-ins in `dtype` -> {"steps": every UNet input's first half
    (3, 2, 4, 16, 16), "final": the returned latents}, float64 numpy.  randn: what torch.randn is during the run.
    loop_q: the loop's own rounding (loop_model.round_half for the noise run: fp16 tensors round every operation)"""
    pipe = Pipe("cpu", dtype, unet, controlnet)
    imgs, text, edges = loop_inputs("cpu", dtype)
    keep, torch.randn = torch.randn, randn
    try:
        final = L.inference_model(pipe, pipe.controlnet, pipe.frescoProc, imgs, text, edges, pipe.scheduler.timesteps,
                                  q=loop_q, **LOOP_KW)
    finally:
        torch.randn = keep
    assert len(unet.inputs) == len(STEPS3)
    return {"steps": torch.stack([s[:FRAMES] for s in unet.inputs]).double().numpy(), "final": final.double().numpy()}


def distance(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


if os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden") not in sys.path:   # (closed_form, for loop_model)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


# ---------------------------------------------------------------------------------------------------------------------
# the records
# ---------------------------------------------------------------------------------------------------------------------
CALL_KEYS = ("out", "res") + TAPS          # the order of a call case's *_noise and *_peak entries
CALL_CASES = {"plain": {}, "fresco": {}, "halfedges": dict(edges_gain=0.5), "halftext": dict(text_gain=0.5)}


class Models:
    """the float64 pair and the fp32 pair whose layers round (to fp16, or to bf16), built once"""

    def __init__(self):
        self.u64, self.c64 = build("unet", torch.float64), build("controlnet", torch.float64)
        self.u32, self.c32 = build("unet", torch.float32), build("controlnet", torch.float32)

    def load(self, weight_q=_ident):
        """the stand-in weights again, through `weight_q` (round_bf16: what a bf16 pipeline holds of them)"""
        for kind, nets in (("unet", (self.u64, self.u32)), ("controlnet", (self.c64, self.c32))):
            for net in nets:
                net.load_state_dict({k: weight_q(v).to(net.dtype) for k, v in weights(kind).items()})

    def reset(self, q=round16):
        for net in (self.u64, self.c64):
            set_rounding(net, _ident)
        for net in (self.u32, self.c32):
            set_rounding(net, q)
        for net in (self.u64, self.c64, self.u32, self.c32):
            net.fault = None
        for u in (self.u64, self.u32):
            u.fresco = None
            u.up_blocks[2].swap_cat = False

    def call(self, case, q=round16, fault=None, input_q=_ident):
        """(float64 record, rounded run's record) of a call case; fault: planted into the float64 pair only"""
        self.reset(q)
        if case == "fresco":
            set_fresco(self.u64, make_fresco(torch.float64))
            set_fresco(self.u32, make_fresco(torch.float32), q)
        if fault == "swapped_cat":
            self.u64.up_blocks[2].swap_cat = True
        elif fault is not None:
            self.u64.fault = self.c64.fault = fault
        kw = dict(CALL_CASES[case], input_q=input_q)
        r64 = call_record(self.u64, self.c64, torch.float64, **kw)
        r16 = None if fault is not None else call_record(self.u32, self.c32, torch.float32, **kw)
        self.reset()
        return r64, r16

    def loop(self, draws=None, fault=None):
        """(float64 record, rounded run's record, the draws) of the loop case; draws None: drawn and recorded here"""
        self.reset()
        if fault is not None:
            self.u64.fault = self.c64.fault = fault
        if draws is None:
            draws = []
            r64 = loop_record(self.u64, self.c64, torch.float64, recording_randn(draws))
        else:
            r64 = loop_record(self.u64, self.c64, torch.float64, L.replay_randn(list(draws), "cpu"))
        r16 = None if fault is not None else loop_record(self.u32, self.c32, torch.float32, L.replay_randn(list(draws), "cpu"),
                                                         loop_q=L.round_half)
        self.reset()
        return r64, r16, draws


def noise_and_peak(r64, r16, keys):
    peak = [float(np.abs(r64[k]).max()) for k in keys]
    return [distance(r64[k], r16[k]) / p for k, p in zip(keys, peak)], peak


def loop_noise_and_peak(r64, r16):
    peak = max(float(np.abs(r64[k]).max()) for k in ("steps", "final"))
    return max(distance(r64[k], r16[k]) for k in ("steps", "final")) / peak, peak


def loop_distance(a, b):
    return max(distance(a[k], b[k]) for k in ("steps", "final"))


def derive(models, draws=None):
    """every entry of the golden file, from scratch (draws: the loop's recorded draws, or None to draw them)"""
    out = {}
    for case in CALL_CASES:
        r64, r16 = models.call(case)
        for k in CALL_KEYS:
            out["%s_%s" % (case, k)] = r64[k]
        noise, peak = noise_and_peak(r64, r16, CALL_KEYS)
        out[case + "_noise"], out[case + "_peak"] = np.array(noise), np.array(peak)
    # bf16: plain on what a bf16 pipeline holds -- the weights and the inputs rounded to bf16 once (as
    # unet_resnet_bf16_model does) -- and the noise of the layers rounding to bf16
    models.load(round_bf16)
    r64, rb = models.call("plain", q=round_bf16, input_q=round_bf16)
    models.load()
    for k in CALL_KEYS:
        out["bf16_%s" % k] = r64[k]
    noise, peak = noise_and_peak(r64, rb, CALL_KEYS)
    out["bf16_noise"], out["bf16_peak"] = np.array(noise), np.array(peak)
    r64, r16, draws = models.loop(draws)
    out["loop_steps"], out["loop_final"], out["loop_draws"] = r64["steps"], r64["final"], np.stack(draws)
    noise, peak = loop_noise_and_peak(r64, r16)
    out["loop_noise"], out["loop_peak"] = np.array([noise]), np.array([peak])
    return out


def fault_distance(models, fault, gold):
    """(distance of the float64 model with `fault` planted from the record, the case's bar 4 x noise x peak): the three
    faults of a single call on `plain`'s noise prediction, the three that need several steps on the loop case"""
    if fault in ("swapped_text", "swapped_cat", "no_mid_residual"):
        r64, _ = models.call("plain", fault=fault)
        return distance(r64["out"], gold["plain_out"]), 4 * float(gold["plain_noise"][0]) * float(gold["plain_peak"][0])
    r64, _, _ = models.loop(gold["loop_draws"], fault=fault)
    d = loop_distance(r64, {"steps": gold["loop_steps"], "final": gold["loop_final"]})
    return d, 4 * float(gold["loop_noise"][0]) * float(gold["loop_peak"][0])


# ---------------------------------------------------------------------------------------------------------------------
# the store pass, the spatial-guided call and the controller's sequence (tests/golden/unet_composed_seq_golden.npz)
# ---------------------------------------------------------------------------------------------------------------------
SEQ_GOLDEN_FILE = "unet_composed_seq_golden.npz"
STORE_STEP = L.STEPS[-1]         # get_intraframe_paras runs at the scheduler's last timestep
STORE_SEED, STALE_SEED = 79, 81  # of the store pass's inputs, and of the pass a store that was not cleared still holds
STORED = 3                       # attn1 calls of up_blocks.2 / up_blocks.3 in this model
END_OPT_STEP = 4                 # run_fresco.py: apply_FRESCO_opt(steps=timesteps[:end_opt_step]) -- 901 .. 451
STEPS2 = L.STEPS[2:]             # the seq case: num_warmup_steps = 2 of loop_model's six steps
SEQ_KW = dict(num_warmup_steps=2, seed=22, cond_scale=list(L.COND_SCALE), num_inference_steps=len(L.STEPS),
              guidance_scale=L.GUIDANCE, num_intraattn_steps=1)
# (use_intraattn, use_interattn, use_cfattn, index) at the UNet call of 601, 451, 301, 151: intra on the first step only,
# temporal off once t < step_interattn_end = 350, cross-frame throughout, the index back at 0 each time
SEQ_FLAGS = ((1, 1, 1, 0), (0, 1, 1, 0), (0, 0, 1, 0), (0, 0, 1, 0))
FULL_FAULTS = ("rotated_refs", "no_intra", "uncleared_store", "own_refs")
SEQ_FAULTS = ("intra_every_step", "temporal_never_off")
GRAM_FAULTS = ("gram_unnormalised", "gram_transposed")


def seq_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, SEQ_GOLDEN_FILE)))


def thin_tokens(t):
    """(n, h * w, C) tokens of a square plane, kept as R.thin keeps the (n, h, w, C) map"""
    n, hw, C = t.shape
    side = int(round(hw ** 0.5))
    assert side * side == hw
    return R.thin(t.reshape(n, side, side, C).double())


def thin_gram(g):
    """(B, hw, hw) kept as R.thin keeps a one-channel map: every s-th row and column plus the last ones"""
    return R.thin(g.double()[..., None])


def store_inputs(seed=STORE_SEED):
    """(imgs (2, 3, 128, 128) in [-1, 1], the draw of prepare_latents (2, 4, 16, 16)) of the store pass, fp16 values.  The
    images carry a level per frame and channel under the texture (an 8 x 8 mean of texture alone is next to nothing), so that
    the latents are another set than call_inputs' and the loop's, and not noise alone"""
    rs = np.random.RandomState(seed)
    level = rs.uniform(-1.2, 1.2, (FRAMES, 3, 1, 1))
    imgs = np.tanh(level + 0.6 * rs.standard_normal((FRAMES, 3, SIDE, SIDE)))
    draw = rs.standard_normal((FRAMES, 4, LAT, LAT))
    return torch.from_numpy(imgs).to(torch.float16), torch.from_numpy(draw).to(torch.float16)


def store_latents(dtype, q=L.identity, seed=STORE_SEED):
    """what get_intraframe_paras hands the UNet on `Pipe` (diffusion_hacked.py:863-877): the draw, loop_model.VAE's encoding of
    the images times the scaling factor, add_noise at the last timestep, both CFG halves"""
    imgs, draw = store_inputs(seed)
    vae, sched = L.VAE(), L.Scheduler()
    x0 = q(vae.config.scaling_factor * q(vae.encode(imgs.to(dtype)).latent_dist.sample()))
    lat = q(sched.add_noise(x0, q(draw.to(dtype) * sched.init_noise_sigma), torch.tensor(STORE_STEP)))
    return torch.cat([lat] * 2)


def gram(feat, fault=None):
    """oracle.gram_target of a (B, C, h, w) feature in float64; fault: a Gram a kernel at fault would give"""
    from oracle import fresco_oracle as O
    feat = feat.double()
    if fault == "gram_transposed":         # the pixels enumerated column by column
        feat = feat.transpose(2, 3)
    if fault == "gram_unnormalised":
        X = feat.reshape(feat.shape[0], feat.shape[1], -1).transpose(1, 2)
        return X @ X.transpose(1, 2)
    return O.gram_target(feat).double()


def store_pass(unet, fresco, dtype, loop_q=L.identity, seed=STORE_SEED, clear=True, gram_fault=None):
    """the pass get_intraframe_paras makes (diffusion_hacked.py:842-901) on `unet`, whose FRESCO sites read `fresco`: every
    flag off, the hook collecting and optimising nothing, the store cleared (clear=False: the fault of a store that was not)
    and storing; ONE UNet call without ControlNet residuals at STORE_STEP -> {"attn<i>": the i-th stored tensor thinned,
    "gram<i>": gram_target of the i-th up block's input thinned}; the whole stored tensors stay in fresco.stored"""
    fresco.disable_controller()
    fresco.hook = False
    if clear:
        fresco.clear_store()
    before = len(fresco.stored)
    fresco.enable_store()
    _, _, text, _ = call_inputs()
    unet.ups = []
    with torch.no_grad():
        unet(store_latents(dtype, loop_q, seed), torch.tensor(STORE_STEP), encoder_hidden_states=text.to(dtype),
             cross_attention_kwargs=None, return_dict=False)
    ups, unet.ups = unet.ups, None
    fresco.disable_store()
    assert len(fresco.stored) == before + STORED and len(ups) == len(unet.up_blocks)
    rec = {"attn%d" % i: thin_tokens(t) for i, t in enumerate(fresco.stored[before:])}
    rec.update({"gram%d" % i: thin_gram(gram(u, gram_fault)) for i, u in enumerate(ups)})
    return rec


STORE_KEYS = tuple("attn%d" % i for i in range(STORED)) + tuple("gram%d" % i for i in range(4))


def seq_record(unet, controlnet, fresco, dtype, randn, loop_q=L.identity, **overrides):
    """four steps of loop_model.inference_model on the stand-ins with `fresco` as the working controller (its store filled
    by store_pass), everything switched on as run_fresco.py does before inference(): enable_controller, the hook on
    timesteps[:END_OPT_STEP] with iters = 0 -> {"steps": every UNet input's first half (4, 2, 4, 16, 16), "final": the
    returned latents, "flags": Fresco.flags() at each UNet call (4, 4)}.  flows / occs / saliency are given, as run_fresco.py
    gives them: with six steps no bg_smoothing_step is reached."""
    pipe = Pipe("cpu", dtype, unet, controlnet)
    pipe.frescoProc = types.SimpleNamespace(controller=fresco)
    imgs, text, edges = loop_inputs("cpu", dtype)
    fresco.enable_controller()
    fresco.hook, fresco.hook_steps = True, set(L.STEPS[:END_OPT_STEP])
    flags = []
    keep, torch.randn, unet.on_call = torch.randn, randn, lambda: flags.append(fresco.flags())
    try:
        final = L.inference_model(pipe, pipe.controlnet, pipe.frescoProc, imgs, text, edges, pipe.scheduler.timesteps,
                                  flows=fresco.flows, occs=fresco.occs, saliency=fresco.saliency, q=loop_q,
                                  **dict(SEQ_KW, **overrides))
    finally:
        torch.randn, unet.on_call = keep, None
    assert len(unet.inputs) == len(STEPS2)
    return {"steps": torch.stack([s[:FRAMES] for s in unet.inputs]).double().numpy(), "final": final.double().numpy(),
            "flags": np.array(flags)}


class SeqModels:
    """the store pass, `full` and `seq` on a Models' two pairs"""

    def __init__(self, models):
        self.m = models

    def _sites(self, q=round16):
        m = self.m
        m.reset(q)
        f64, f32 = make_fresco(torch.float64), make_fresco(torch.float32)
        set_fresco(m.u64, f64)
        set_fresco(m.u32, f32, q)
        return f64, f32

    def store(self, rounded=True, gram_fault=None):
        """(float64 record, the rounded run's, the two Fresco objects with their stores filled and the sites installed)"""
        f64, f32 = self._sites()
        s64 = store_pass(self.m.u64, f64, torch.float64, gram_fault=gram_fault)
        s16 = store_pass(self.m.u32, f32, torch.float32, L.round_half) if rounded else None
        return s64, s16, f64, f32

    def full(self, fault=None):
        """(float64 record, the rounded run's) of `full`: the store pass, then call_inputs() through ControlNet + UNet with
        intra, cross-frame and temporal attention on and the hook as in `fresco`.  fault (float64 pair only):
          rotated_refs     the references one layer off: up_blocks.3's two, the only ones of one shape, change places
                           (store[0], 64 x 640, has no peer: a rotation that reaches it cannot compute, the shapes differ)
          no_intra         the spatial pass skipped
          uncleared_store  six entries: the three of an earlier pass on other images are read, the index ends at 3
          own_refs         the references are the call's own features"""
        _, _, f64, f32 = self.store(rounded=fault is None)
        m = self.m
        if fault == "uncleared_store":
            f64.clear_store()
            store_pass(m.u64, f64, torch.float64, seed=STALE_SEED)
            store_pass(m.u64, f64, torch.float64, clear=False)
            assert len(f64.stored) == 2 * STORED
        if fault == "rotated_refs":
            f64.stored = [f64.stored[0], f64.stored[2], f64.stored[1]]
        f64.own_refs = fault == "own_refs"
        for f in (f64, f32):
            f.enable_controller()
            f.hook, f.hook_steps = True, None
        if fault == "no_intra":
            f64.disable_intraattn()
        r64 = call_record(m.u64, m.c64, torch.float64)
        r16 = call_record(m.u32, m.c32, torch.float32) if fault is None else None
        if fault is None:
            assert f64.flags() == (1, 1, 1, 0) and f32.flags() == (1, 1, 1, 0)
        m.reset()
        return r64, r16

    def seq(self, draws=None, fault=None):
        """(float64 record, the rounded run's, the draws) of `seq`.  fault: intra_every_step (num_intraattn_steps never
        reached), temporal_never_off (step_interattn_end = 0)"""
        _, _, f64, f32 = self.store(rounded=fault is None)
        m = self.m
        over = {"intra_every_step": dict(num_intraattn_steps=len(STEPS2) + 1), "temporal_never_off": dict(step_interattn_end=0),
                None: {}}[fault]
        if draws is None:
            draws = []
            r64 = seq_record(m.u64, m.c64, f64, torch.float64, recording_randn(draws), **over)
        else:
            r64 = seq_record(m.u64, m.c64, f64, torch.float64, L.replay_randn(list(draws), "cpu"), **over)
        r16 = None
        if fault is None:
            r16 = seq_record(m.u32, m.c32, f32, torch.float32, L.replay_randn(list(draws), "cpu"), loop_q=L.round_half)
            assert (r16["flags"] == r64["flags"]).all()
        m.reset()
        return r64, r16, draws


def derive_seq(models, draws=None):
    """every entry of the second golden file (draws: seq's recorded draws, or None to draw them)"""
    sm = SeqModels(models)
    out = {}
    s64, s16, _, _ = sm.store()
    models.reset()
    noise, peak = noise_and_peak(s64, s16, STORE_KEYS)
    for k in STORE_KEYS:
        out["store_" + k] = s64[k]
    out["store_noise"], out["store_peak"] = np.array(noise), np.array(peak)
    r64, r16 = sm.full()
    for k in CALL_KEYS:
        out["full_" + k] = r64[k]
    noise, peak = noise_and_peak(r64, r16, CALL_KEYS)
    out["full_noise"], out["full_peak"] = np.array(noise), np.array(peak)
    r64, r16, draws = sm.seq(draws)
    out["seq_steps"], out["seq_final"], out["seq_draws"], out["seq_flags"] = r64["steps"], r64["final"], np.stack(draws), r64["flags"]
    noise, peak = loop_noise_and_peak(r64, r16)
    out["seq_noise"], out["seq_peak"] = np.array([noise]), np.array([peak])
    return out


def store_bars(gold):
    """per STORE_KEYS entry 4 x noise x peak"""
    return [4 * float(n) * float(p) for n, p in zip(gold["store_noise"], gold["store_peak"])]


def seq_fault_distance(models, fault, gold):
    """(distance of the float64 model with `fault` planted from its record, that record's bar): FULL_FAULTS on `full`'s noise
    prediction, SEQ_FAULTS on `seq`'s step inputs and final latents, GRAM_FAULTS on the worst of the four Gram targets (in
    its own bars: -> (the ratio, 1.0))"""
    sm = SeqModels(models)
    if fault in FULL_FAULTS:
        r64, _ = sm.full(fault)
        return distance(r64["out"], gold["full_out"]), 4 * float(gold["full_noise"][0]) * float(gold["full_peak"][0])
    if fault in SEQ_FAULTS:
        r64, _, _ = sm.seq(gold["seq_draws"], fault)
        d = loop_distance(r64, {"steps": gold["seq_steps"], "final": gold["seq_final"]})
        return d, 4 * float(gold["seq_noise"][0]) * float(gold["seq_peak"][0])
    s64, _, _, _ = sm.store(rounded=False, gram_fault=fault)
    models.reset()
    bars = dict(zip(STORE_KEYS, store_bars(gold)))
    return min(distance(s64[k], gold["store_" + k]) / bars[k] for k in STORE_KEYS if k.startswith("gram")), 1.0
