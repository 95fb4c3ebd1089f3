"""Generate tests/golden/freeu_golden.npz: records of the UNMODIFIED reference src/free_lunch_utils.py on the CPU.

Run (build container, where the reference tree is present):  python tests/golden/make_freeu_golden.py

The reference module imports three names from diffusers, which is not installed: `is_torch_version` (only reached in the
gradient-checkpointing branch) and the module loggers of unet_2d_condition / unet_3d_condition (`.debug` only).  Stubs
for exactly these are registered here; _ref_harness.py is not involved.

Recorded, from seeded inputs that tests/freeu_model.py rebuilds (their sha256 is stored, they are not):
  (a) Fourier_filter(x, 1, s) for freeu_model.FOURIER_SHAPES x FOURIER_SCALES, run in float64 (`*_f64`, every shape) and
      in float32 (`*_f32`, planes up to 32 x 32);
  (b) register_free_upblock2d / register_free_crossattn_upblock2d run on the stand-in blocks of freeu_model
      (BLOCK_CONFIGS x BLOCK_SIZES, b1 = 1.2, b2 = 1.5, s1 = 0.9, s2 = 0.2) in float64 and float32: every resnet input,
      the block output and the incoming hidden_states after the call (the reference scales it in place).  Of these the
      channels freeu_model.kept_channels names are kept -- both ends of the scaled range, the end of the hidden part and
      all skip channels -- which keeps the file small; the untouched middle is covered by the kernel tests.
"""
import importlib.util
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import freeu_model as M  # noqa: E402

REF = "/root/reference/src/free_lunch_utils.py"
OUT = os.path.join(HERE, "freeu_golden.npz")


def load_reference():
    sys.dont_write_bytecode = True
    stubs = {}
    for name in ("diffusers", "diffusers.utils", "diffusers.models", "diffusers.models.unet_2d_condition",
                 "diffusers.models.unet_3d_condition"):
        if name not in sys.modules:
            stubs[name] = sys.modules[name] = types.ModuleType(name)
    if "diffusers.utils" in stubs:
        stubs["diffusers.utils"].is_torch_version = lambda op, v: True
    for name in ("diffusers.models.unet_2d_condition", "diffusers.models.unet_3d_condition"):
        if name in stubs:
            stubs[name].logger = logging.getLogger(name)
    spec = importlib.util.spec_from_file_location("reference_free_lunch_utils", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    flu = load_reference()
    out = {}
    for shape in M.FOURIER_SHAPES:
        x = M.fourier_input(shape)
        out["fourier_%s_sha256" % "x".join(map(str, shape))] = np.array(M.digest(x))
        for s in M.FOURIER_SCALES:
            key = M.fourier_key(shape, s)
            out[key + "_f64"] = flu.Fourier_filter(torch.from_numpy(x), 1, s).numpy()
            if shape[2] * shape[3] <= M.FOURIER_F32_MAX_HW:
                out[key + "_f32"] = flu.Fourier_filter(torch.from_numpy(x).float(), 1, s).numpy()
    registers = {"UpBlock2D": flu.register_free_upblock2d, "CrossAttnUpBlock2D": flu.register_free_crossattn_upblock2d}
    for kind in M.BLOCK_KINDS:
        for name, (C, outs, _) in M.BLOCK_CONFIGS.items():
            for size in M.BLOCK_SIZES:
                key = M.block_key(kind, name, size)
                hidden, skips = M.block_inputs(name, size)
                out[key + "_sha256"] = np.array(M.digest(hidden, *skips))
                for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
                    r = M.run_block(registers[kind], kind, name, size, dt)
                    stage = C
                    for k, t in enumerate(r["resnet_in"]):
                        out["%s_in%d_%s" % (key, k, tag)] = t.numpy()[:, M.kept_of(name, stage, t.shape[1])]
                        stage = outs[k]
                    out["%s_out_%s" % (key, tag)] = r["out"].numpy()[:, M.kept_of(name, stage, stage)]
                    out["%s_hidden_%s" % (key, tag)] = r["hidden_after"].numpy()[:, M.kept_of(name, C, C)]
                    if kind == "CrossAttnUpBlock2D":  # the attentions ran, once per resnet, on the resnet's output
                        assert [len(a.inputs) for a in r["block"].attentions] == [1] * len(outs)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes, %d arrays)" % (OUT, os.path.getsize(OUT), len(out)))


if __name__ == "__main__":
    main()
