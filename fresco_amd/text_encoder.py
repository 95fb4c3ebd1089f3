"""CLIPTextModel of SD-1.5 pipelines (`pipe.text_encoder`) on this package's kernels, for fp16 pipelines (DESIGN.md section
24): the module that `pipe._encode_prompt` calls for the prompts and the negative prompts.

`CLIPTextEncoder.from_module(text_encoder)` reads a module's parameters, `CLIPTextEncoder.from_state_dict(sd, config)` a state
dict's; `patch_text_encoder(pipe)` binds the native forward on `pipe.text_encoder`, which stays in place (its `dtype`,
`config` and `device` keep working), `unpatch_text_encoder(pipe)` removes it.  A call of a model of N layers is 2 + 7 N
launches into libfresco_hip.so (include/fresco_text.h, fresco_unet_tf.h, fresco_vae.h), 86 at the 12 layers of SD-1.5:

  1. clip_embed(ids)                                 token_embedding[ids] + position_embedding[:L], one rounding
  per layer:
  2. unet_layernorm(h)                               layer_norm1
  3. vae_conv 1 x 1 + bias                           q_proj | k_proj | v_proj as ONE (3 C, C) matrix; q, k, v are column slices
  4. clip_attention(q, k, v)                         causal softmax attention at head dim 64, the mask a selection
  5. vae_conv 1 x 1 + bias + residual h              out_proj; h = h + attention, rounded once
  6. unet_layernorm(h)                               layer_norm2
  7. clip_fc1(y)                                     quick_gelu(fc1): the pre-activation is never written
  8. vae_conv 1 x 1 + bias + residual h              fc2; h = h + mlp, rounded once
  last:
  9. unet_layernorm(h)                               final_layer_norm

This is transformers' `CLIPTextModel.forward` for `hidden_act="quick_gelu"`, no `attention_mask` and no `position_ids`.
Against PyTorch's fp16 module each residual sum is rounded to fp16 once from the fp32 accumulator, and fc1's pre-activation
is never rounded.

PARAMETER LAYOUTS.  transformers 4.x (what diffusers 0.19.3 installs) nests the parameters under `text_model.`
(`text_model.embeddings.token_embedding.weight`), transformers 5.x is flat (`embeddings.token_embedding.weight`): both are
accepted, after the caller's own `prefix`.

PACKED COPIES.  The stacked q | k | v weight, the fp32 biases and the fp32 LayerNorm parameters are COPIES, keyed by the
source parameters' identity and `_version`, as UNetAttnProcessor's are: an in-place weight update (load_state_dict, an
optimiser step) is seen on the next call and the copy is made again.  The token table, the position table, out_proj, fc1 and
fc2 weights are read where they live (a weight that is not dense or not 16-byte aligned is copied under the same rule).

RESULT.  What `CLIPTextModel` returns: a `BaseModelOutputWithPooling` where transformers imports, otherwise `TextOutput`, a
tuple type with `last_hidden_state` / `pooler_output` / `hidden_states` attributes; with `return_dict=False` a plain tuple.
`[0]` is the last hidden state in every case.  `output_hidden_states=True` adds the N + 1 residual streams (the embedding and
every layer's output, the last one BEFORE final_layer_norm, as transformers has it).  `pooler_output` follows transformers'
rule: row `ids.argmax(-1)` where `eos_token_id == 2` (the legacy rule that SD-1.5's config selects), otherwise the first
position equal to `eos_token_id`.  It is taken with torch indexing on the device, without a host synchronisation: a BOUNDARY
COPY of B rows by PyTorch's index kernels, not part of the model's arithmetic.

REFUSALS, each a NotImplementedError that names its cause, the module's before anything is patched: a non-None
attention_mask or position_ids; output_attentions=True; hidden_act other than quick_gelu; a head dim other than 64; more
tokens than max_position_embeddings or than 128; widths that are no multiple of 64; parameters that are not fp16 or not on the
GPU (bf16 and fp32 text encoders are not built); ids that are not int64 (B, L).  There is no fallback to PyTorch.

VERIFIED against transformers 5.15's `CLIPTextModel` where this package is built and tested (tests/test_text_encoder_cpu.py:
the restated model that every record comes from equals the real module in float64): the parameter names, `config`'s
`hidden_size`, `intermediate_size`, `num_hidden_layers`, `num_attention_heads`, `max_position_embeddings`, `hidden_act`,
`layer_norm_eps` and `eos_token_id`, the hidden-state list and the pooling rule.  UNVERIFIED: the `text_model.` nesting of
transformers 4.x (from its published source), and `pipe._encode_prompt` itself (diffusers is not installed): that it calls
`self.text_encoder(ids, attention_mask=None)`, takes `[0]`, and reads `text_encoder.dtype` and `config.use_attention_mask`.
"""
import collections
import math

import torch

from . import _dropin, _lib, ops
from ._dropin import rows16 as _rows16

HEAD_DIM = ops.CLIP_ATTN_HEAD_DIM
MAX_TOKENS = ops.CLIP_ATTN_MAX_L
WIDTH_STEP = 64
NESTED = "text_model."                  # transformers 4.x
_ATTR = "_fresco_text_encoder"
_WHO = "fresco_amd.text_encoder"
_CONFIG = ("hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads", "max_position_embeddings",
           "hidden_act", "layer_norm_eps", "eos_token_id")

TextOutput = collections.namedtuple("TextOutput", ["last_hidden_state", "pooler_output", "hidden_states"])
TextOutput.__doc__ = "what a call returns where transformers does not import: [0] is the last hidden state"


def _cfg(config, name):
    if isinstance(config, dict):
        return config[name]
    return getattr(config, name)


def _layer_names(i):
    b = "encoder.layers.%d." % i
    return [b + n for n in ("layer_norm1", "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj",
                            "layer_norm2", "mlp.fc1", "mlp.fc2")]


def _config_refusal(config):
    """why a configuration is outside what the kernels compute, or None"""
    try:
        C, inner, layers, heads, maxpos, act = (_cfg(config, n) for n in _CONFIG[:6])
        float(_cfg(config, "layer_norm_eps"))
        _cfg(config, "eos_token_id")
    except (KeyError, AttributeError) as e:
        return "has a config without %s" % e
    C, inner, layers, heads, maxpos = int(C), int(inner), int(layers), int(heads), int(maxpos)
    if act != "quick_gelu":
        return "has hidden_act %r, only quick_gelu" % (act,)
    if layers <= 0 or heads <= 0 or C % heads or C // heads != HEAD_DIM:
        return "has head dim %s (%d channels on %d heads), only %d" % (C // heads if heads > 0 and C % heads == 0 else "?", C, heads,
                                                                      HEAD_DIM)
    if C % WIDTH_STEP or inner <= 0 or inner % WIDTH_STEP or not ops.unet_ln_channels(C):
        return "is %d wide and %d inside, the kernels take multiples of %d (the width in %d .. %d)" \
            % (C, inner, WIDTH_STEP, ops.UNET_LN_MIN, ops.UNET_LN_MAX)
    if maxpos <= 0:
        return "has max_position_embeddings %d" % maxpos
    return None


class CLIPTextEncoder:
    """One CLIPTextModel on HIP kernels (see the module docstring).  The constructor takes a state dict as from_state_dict
    does but does not ask where the parameters live; the two factories and patch_text_encoder do."""

    def __init__(self, state_dict, config, prefix=""):
        _lib.load()  # fail here, loudly, when the HIP library is absent
        why = _config_refusal(config)
        if why:
            raise _dropin.refusal(_WHO, "the text encoder", why)
        C, inner, layers, heads, maxpos = (int(_cfg(config, n)) for n in _CONFIG[:5])
        if prefix and not prefix.endswith("."):
            prefix += "."
        if not any(k.startswith(prefix + "embeddings.") for k in state_dict) and \
                any(k.startswith(prefix + NESTED + "embeddings.") for k in state_dict):
            prefix += NESTED
        names = ["final_layer_norm"] + [n for i in range(layers) for n in _layer_names(i)]
        need = ["embeddings.token_embedding.weight", "embeddings.position_embedding.weight"] \
            + [n + s for n in names for s in (".weight", ".bias")]
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        what = "%s: %s" % (_WHO, prefix[:-1] or "the text encoder")
        missing = [k for k in need if k not in sd]
        if missing:
            raise ValueError("%s: missing parameters %s" % (what, missing[:4]))
        for k in need:
            if sd[k].dtype != torch.float16:
                raise _dropin.refusal(_WHO, prefix[:-1] or "the text encoder",
                                      "has %s parameters (%s), fp16 only: bf16 and fp32 text encoders are not built" % (sd[k].dtype, k))
        vocab = int(sd["embeddings.token_embedding.weight"].shape[0]) if sd["embeddings.token_embedding.weight"].dim() == 2 else 0
        shapes = {"embeddings.token_embedding.weight": (vocab, C), "embeddings.position_embedding.weight": (maxpos, C),
                  "final_layer_norm.weight": (C,), "final_layer_norm.bias": (C,)}
        for i in range(layers):
            ln1, q, k, v, o, ln2, fc1, fc2 = _layer_names(i)
            for n in (ln1, ln2):
                shapes.update({n + ".weight": (C,), n + ".bias": (C,)})
            for n in (q, k, v, o):
                shapes.update({n + ".weight": (C, C), n + ".bias": (C,)})
            shapes.update({fc1 + ".weight": (inner, C), fc1 + ".bias": (inner,), fc2 + ".weight": (C, inner), fc2 + ".bias": (C,)})
        _dropin.check_shapes(sd, shapes, what, only=False)
        if vocab <= 0:
            raise ValueError("%s: an empty token table" % what)
        self.width, self.inner, self.layers, self.heads, self.max_positions, self.vocab = C, inner, layers, heads, maxpos, vocab
        self.eps = float(_cfg(config, "layer_norm_eps"))
        self.eos_token_id = _cfg(config, "eos_token_id")
        self.scale = 1.0 / math.sqrt(HEAD_DIM)
        self._sd = sd
        self._packed = {}        # slot -> ([(parameter, version)], value)
        try:
            from transformers.modeling_outputs import BaseModelOutputWithPooling
            self._output = BaseModelOutputWithPooling
        except Exception:        # transformers is absent (or does not import here): the tuple type of this module
            self._output = None

    # ---- what the module must be ------------------------------------------------------------------------------------
    @staticmethod
    def refusal(text_encoder):
        """why `text_encoder` is outside what this class computes, or None; reads the config, shapes, dtypes and devices"""
        config = getattr(text_encoder, "config", None)
        if config is None:
            return "has no config"
        why = _config_refusal(config)
        if why:
            return why
        params = list(text_encoder.parameters())
        if not params:
            return "has no parameters"
        dtypes = {p.dtype for p in params}
        if dtypes != {torch.float16}:
            return "is %s, fp16 modules only (bf16 and fp32 text encoders are not built)" % "/".join(sorted(str(d) for d in dtypes))
        for p in params:
            if not p.is_cuda:
                return "has parameters on %s, GPU modules only" % p.device
        return None

    @classmethod
    def from_module(cls, text_encoder, name="the text encoder"):
        """the native forward of a CLIPTextModel (or a module with its parameter names and `config`); it keeps the module's
        Parameters, so their in-place updates are seen"""
        why = cls.refusal(text_encoder)
        if why:
            raise _dropin.refusal(_WHO, name, why)
        return cls(text_encoder.state_dict(keep_vars=True), text_encoder.config)

    @classmethod
    def from_state_dict(cls, state_dict, config, prefix=""):
        """from fp16 GPU tensors under transformers' names (flat, or nested under `text_model.`), after `prefix`; `config`: a
        CLIPTextConfig, any object with its attributes, or a dict"""
        self = cls(state_dict, config, prefix)
        for k, v in self._sd.items():
            if not v.is_cuda:
                raise _dropin.refusal(_WHO, "the text encoder", "has parameters on %s (%s), GPU tensors only" % (v.device, k))
        return self

    # ---- packed copies ----------------------------------------------------------------------------------------------
    def _pack(self, slot, names, build):
        params = [self._sd[n] for n in names]
        hit = self._packed.get(slot)
        if hit is not None and all(p is s and p._version == ver for p, (s, ver) in zip(params, hit[0])):
            return hit[1]
        with torch.no_grad():
            value = build(*[p.detach() for p in params])
        self._packed[slot] = ([(p, p._version) for p in params], value)
        return value

    def _f32(self, name):
        return self._pack(name, [name], lambda p: p.to(torch.float32).contiguous())

    def _in_place(self, name):
        """the weight where it lives (dense rows at a 16-byte aligned address), otherwise one copy under the version rule"""
        return self._pack(name, [name], _rows16)

    # ---- the call ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, input_ids=None, attention_mask=None, position_ids=None, output_attentions=None, output_hidden_states=None,
                 return_dict=None, *, taps=None):
        """input_ids int64 (B, L) on the GPU -> CLIPTextModel.forward's result (see the module docstring).  taps: a dict that
        receives "attn", layer 0's attention output before out_proj, and "fc1", layer 0's quick_gelu(fc1), both (B, L, .)."""
        def refuse(why):
            raise _dropin.refusal(_WHO, "", why)
        if attention_mask is not None:
            refuse("an attention_mask is not supported (the pipeline passes None: the SD-1.5 config has no use_attention_mask)")
        if position_ids is not None:
            refuse("position_ids are not supported (the pipeline passes None)")
        if output_attentions:
            refuse("output_attentions is not supported: the attention probabilities are never written")
        ids = input_ids
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 2 or ids.numel() == 0:
            refuse("input_ids must be an int64 (B, L) tensor, got %s"
                   % ((str(ids.dtype), tuple(ids.shape)) if isinstance(ids, torch.Tensor) else type(ids).__name__,))
        B, L = ids.shape
        if L > self.max_positions or L > MAX_TOKENS:
            refuse("%d tokens, at most %d (max_position_embeddings %d, the attention kernel %d)"
                   % (L, min(self.max_positions, MAX_TOKENS), self.max_positions, MAX_TOKENS))
        if not ids.is_cuda:
            refuse("input_ids are on %s, GPU tensors only" % ids.device)
        ids = ids if ids.is_contiguous() else ids.contiguous()
        C, eps = self.width, self.eps
        h = ops.clip_embed(ids, self._in_place("embeddings.token_embedding.weight"),
                           self._in_place("embeddings.position_embedding.weight"))
        streams = [h] if output_hidden_states else None
        for i in range(self.layers):
            ln1, q, k, v, o, ln2, fc1, fc2 = _layer_names(i)
            y = ops.unet_layernorm(h, self._f32(ln1 + ".weight"), self._f32(ln1 + ".bias"), eps)
            w_qkv = self._pack(q + "|k|v.weight", [q + ".weight", k + ".weight", v + ".weight"],
                               lambda *p: torch.cat(p, dim=0).contiguous())
            b_qkv = self._pack(q + "|k|v.bias", [q + ".bias", k + ".bias", v + ".bias"],
                               lambda *p: torch.cat(p, dim=0).to(torch.float32).contiguous())
            qkv = ops.conv_rows(y, w_qkv, b_qkv)
            a = ops.clip_attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], self.heads, self.scale)
            h = ops.conv_rows(a, self._in_place(o + ".weight"), self._f32(o + ".bias"), residual=h)
            y = ops.unet_layernorm(h, self._f32(ln2 + ".weight"), self._f32(ln2 + ".bias"), eps)
            g = ops.clip_fc1(y, self._in_place(fc1 + ".weight"), self._f32(fc1 + ".bias"))
            if taps is not None and i == 0:
                taps["attn"], taps["fc1"] = a, g
            h = ops.conv_rows(g, self._in_place(fc2 + ".weight"), self._f32(fc2 + ".bias"), residual=h)
            if streams is not None:
                streams.append(h)
        last = ops.unet_layernorm(h, self._f32("final_layer_norm.weight"), self._f32("final_layer_norm.bias"), eps)
        # the boundary copy: B rows by torch indexing on the device, no host synchronisation
        if self.eos_token_id == 2:
            at = ids.to(torch.int).argmax(dim=-1)
        else:
            at = (ids.to(torch.int) == self.eos_token_id).int().argmax(dim=-1)
        pooled = last[torch.arange(B, device=last.device), at]
        hidden = tuple(streams) if streams is not None else None
        if return_dict is not None and not return_dict:
            return (last, pooled) + ((hidden,) if hidden is not None else ())
        if self._output is not None:
            return self._output(last_hidden_state=last, pooler_output=pooled, hidden_states=hidden)
        return TextOutput(last, pooled, hidden)


def patch_text_encoder(pipe):
    """bind a CLIPTextEncoder built from `pipe.text_encoder` as that module's `forward` (in its __dict__: the module object,
    its `dtype`, `config` and `device` stay); a module outside the supported configuration raises NotImplementedError before
    anything is patched.  Returns the number of modules patched (1).  The module's own forward stays on its class:
    unpatch_text_encoder removes the binding."""
    te = getattr(pipe, "text_encoder", None)
    if not isinstance(te, torch.nn.Module):
        raise TypeError("%s: pipe.text_encoder must be a module, got %s" % (_WHO, type(te).__name__))
    _dropin.unpatch(te, _ATTR)
    native = CLIPTextEncoder.from_module(te, name="pipe.text_encoder")
    te.__dict__[_ATTR] = native
    te.__dict__["forward"] = native
    return 1


def unpatch_text_encoder(pipe):
    """the module's own forward again; returns the number of modules restored"""
    return _dropin.unpatch(pipe.text_encoder, _ATTR)
