#!/usr/bin/env python
"""The CLIP text model of SD-1.5 (12 layers, width 768, 12 heads, intermediate 3072, the real vocabulary of 49408, fp16) at 1, 2
and 10 sequences of 77 tokens -- `pipe._encode_prompt` calls it once for the N prompts and once for the N negative prompts of
a key-frame batch -- with stand-in weights (the restated model of tests/clip_text_model.py under a fixed seed: the time does
not depend on the values).

  native    fresco_amd.CLIPTextEncoder.from_module on the model: 86 launches per call
  pytorch   the same weights in fp16 on PyTorch's kernels: transformers.CLIPTextModel where transformers imports, otherwise the
            restated model with scaled_dot_product_attention(is_causal=True); `baseline` in the result says which
  kernel    the three kernels of csrc/text.hip alone at each batch, each beside PyTorch's own operation on the same operands
            (embedding + add, scaled_dot_product_attention(is_causal=True), Linear + x sigmoid(1.702 x))

Every mode is a child process of its own under a time limit; a child that fails ends the run.  Per measurement: two warm-up
calls, then the median of five timed blocks (a host clock around several calls that end in a device synchronise): `ms`; and
`gpu_us`, device events around calls queued behind 10 ms of matrix products, so that the host is ahead and what is timed is
the GPU's work with its dispatch gaps (tools/bench_unet_resnet.py's measure).  No ratio is fixed in advance: every case where
PyTorch wins is listed as such.

    python tools/bench_text_encoder.py [--out profiles/text_encoder_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_unet_resnet import queued_us  # noqa: E402
from bench_vae import timed  # noqa: E402

LAYERS, WIDTH, HEADS, INNER, VOCAB, TOKENS = 12, 768, 12, 3072, 49408, 77
BATCHES = (1, 2, 10)
MODES = ("native", "pytorch", "kernel")
LIMITS = dict(native=240, pytorch=300, kernel=240)  # seconds per child


def _config():
    return types.SimpleNamespace(vocab_size=VOCAB, hidden_size=WIDTH, intermediate_size=INNER, num_hidden_layers=LAYERS,
                                 num_attention_heads=HEADS, max_position_embeddings=TOKENS, hidden_act="quick_gelu",
                                 layer_norm_eps=1e-5, eos_token_id=2, bos_token_id=VOCAB - 2, pad_token_id=1, attention_dropout=0.0)


def _model(dev):
    import torch
    import clip_text_model as M
    torch.manual_seed(0)
    return M.TextModel(_config()).half().eval().to(dev)


def _ids(B, dev):
    import torch
    g = torch.Generator().manual_seed(B)
    ids = torch.randint(0, VOCAB - 2, (B, TOKENS), generator=g)
    ids[:, 0] = VOCAB - 2
    ids[:, 20:] = VOCAB - 1     # BOS, 19 words, EOS and its padding
    return ids.to(dev)


def child(mode):
    import torch
    import torch.nn.functional as F
    import fresco_amd
    from fresco_amd import ops
    if not torch.cuda.is_available():
        sys.exit("bench_text_encoder.py needs a GPU")
    dev = "cuda:0"
    res = dict(mode=mode, device=torch.cuda.get_device_name(0))
    mod = _model(dev)
    rows = []
    if mode == "native":
        enc = fresco_amd.CLIPTextEncoder.from_module(mod)
        for B in BATCHES:
            ids = _ids(B, dev)
            ms, _ = timed(lambda: enc(ids), 10)
            rows.append(dict(sequences=B, ms=ms, gpu_us=queued_us(lambda: enc(ids), 20)))
    elif mode == "pytorch":
        res["baseline"] = "tests/clip_text_model.py with scaled_dot_product_attention(is_causal=True)"
        base = mod
        try:
            import transformers
            c = _config()
            cfg = transformers.CLIPTextConfig(**{k: v for k, v in vars(c).items()})
            real = transformers.CLIPTextModel(cfg)
            nested = next(iter(real.state_dict())).startswith("text_model.")
            real.load_state_dict({("text_model." + k if nested else k): v for k, v in mod.state_dict().items()})
            base = real.half().eval().to(dev)
            res["baseline"] = "transformers.CLIPTextModel %s (attention: %s)" % (transformers.__version__,
                                                                                getattr(cfg, "_attn_implementation", "default"))
        except ImportError:
            pass
        with torch.no_grad():
            for B in BATCHES:
                ids = _ids(B, dev)
                ms, _ = timed(lambda: base(ids), 10)
                rows.append(dict(sequences=B, ms=ms, gpu_us=queued_us(lambda: base(ids), 20)))
    else:
        sd = mod.state_dict()
        tok, pos = sd["embeddings.token_embedding.weight"], sd["embeddings.position_embedding.weight"]
        w1, b1 = sd["encoder.layers.0.mlp.fc1.weight"], sd["encoder.layers.0.mlp.fc1.bias"]
        b1f = b1.float()
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for B in BATCHES:
                ids = _ids(B, dev)
                qkv = torch.randn(B, TOKENS, 3 * WIDTH, generator=g).half().to(dev)
                q, k, v = qkv[..., :WIDTH], qkv[..., WIDTH:2 * WIDTH], qkv[..., 2 * WIDTH:]
                q4, k4, v4 = (t.reshape(B, TOKENS, HEADS, 64).transpose(1, 2) for t in (q, k, v))
                y = torch.randn(B, TOKENS, WIDTH, generator=g).half().to(dev)
                pairs = dict(
                    clip_embed=(lambda: ops.clip_embed(ids, tok, pos), lambda: tok[ids] + pos[:TOKENS]),
                    clip_attention=(lambda: ops.clip_attention(q, k, v, HEADS, 0.125),
                                    lambda: F.scaled_dot_product_attention(q4, k4, v4, is_causal=True)),
                    clip_fc1=(lambda: ops.clip_fc1(y, w1, b1f), lambda: (lambda t: t * torch.sigmoid(1.702 * t))(F.linear(y, w1, b1))))
                row = dict(sequences=B)
                for name, (ours, theirs) in pairs.items():
                    for fn in (ours, theirs, ours, theirs):     # warm-up: PyTorch's GEMM and SDPA choose their kernels on a first call
                        fn()
                    us, tus = queued_us(ours, 40), queued_us(theirs, 40)
                    row[name] = dict(gpu_us=us, pytorch_gpu_us=tus, pytorch_over_native_gpu=tus / us, pytorch_wins=bool(tus < us))
                rows.append(row)
    res["rows"] = rows
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the result as JSON here as well")
    ap.add_argument("--mode", choices=MODES, default=None, help="(internal) run one mode in this process")
    args = ap.parse_args()
    if args.mode:
        return child(args.mode)
    got = {}
    for mode in MODES:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode], stdout=subprocess.PIPE,
                           timeout=LIMITS[mode], text=True)
        if p.returncode != 0:
            sys.exit("bench_text_encoder.py: mode %s ended with status %d; nothing further is started" % (mode, p.returncode))
        got[mode] = json.loads(p.stdout.strip().splitlines()[-1])
        print(mode, got[mode], flush=True)
    cases = []
    for nat, pt, ker in zip(got["native"]["rows"], got["pytorch"]["rows"], got["kernel"]["rows"]):
        cases.append(dict(sequences=nat["sequences"], native_ms=nat["ms"], native_gpu_us=nat["gpu_us"], pytorch_ms=pt["ms"],
                          pytorch_gpu_us=pt["gpu_us"], pytorch_over_native=pt["ms"] / nat["ms"],
                          pytorch_over_native_gpu=pt["gpu_us"] / nat["gpu_us"], pytorch_wins=bool(pt["ms"] < nat["ms"]),
                          pytorch_wins_gpu=bool(pt["gpu_us"] < nat["gpu_us"]),
                          kernels={k: v for k, v in ker.items() if k != "sequences"}))
    result = dict(bench="text_encoder", device=got["native"]["device"], dtype="float16",
                  model=dict(layers=LAYERS, width=WIDTH, heads=HEADS, intermediate=INNER, vocabulary=VOCAB, tokens=TOKENS),
                  launches_per_call=2 + 7 * LAYERS, baseline=got["pytorch"]["baseline"], cases=cases,
                  cases_where_pytorch_wins=[c["sequences"] for c in cases if c["pytorch_wins"]],
                  cases_where_pytorch_wins_gpu=[c["sequences"] for c in cases if c["pytorch_wins_gpu"]])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
