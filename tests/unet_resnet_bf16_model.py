"""The bf16 side of tests/unet_resnet_model.py (imported, not edited): what tests/golden/make_unet_resnet_bf16_golden.py,
tests/test_bf16_net_cpu.py and tests/test_gpu_bf16_net.py share.

The restated ResnetBlock2D, its cases, its closed-form stand-in values and its thinning rule are unet_resnet_model's.  What
changes is the ONE rounding of the stand-in weights and of the inputs -- drawn in float64 from the same seeds and rounded to
bf16 here, where unet_resnet_model rounds them to fp16 -- and the reference arithmetic of the noise: the fp32 module with
every layer's output sent through a bf16 round trip (DESIGN.md sections 16 and 17's rule with bf16 in fp16's place).  bf16
has fp32's range, so no activation limit is asserted.
"""
import os
import zlib
from collections import OrderedDict

import numpy as np
import torch

import unet_resnet_model as M

GOLDEN_FILE = "unet_resnet_bf16_golden.npz"
CASES, TENSORS, TEMB_CHANNELS = M.CASES, M.TENSORS, M.TEMB_CHANNELS
case_key, thin = M.case_key, M.thin


def to_bf16(a):
    """float64 numpy -> torch bf16, one rounding to nearest even"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.bfloat16)


def round_bf16(t):
    """the bf16 round trip of a layer's output"""
    return t.to(torch.bfloat16).to(t.dtype)


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN_FILE)))


def inputs(case):
    """unet_resnet_model.inputs' draw (same seed, same order, the LAST image scaled and shifted), rounded to bf16"""
    cin, _, n, H, W = case
    rs = np.random.RandomState(zlib.crc32(case_key(case).encode()) & 0x7FFFFFFF)
    x = rs.standard_normal((n, cin, H, W)) * 1.5
    x[-1] = x[-1] * 0.5 + 1.0
    t = rs.standard_normal((n, TEMB_CHANNELS))
    t[-1] = t[-1] * 0.5 - 0.25
    return to_bf16(x), to_bf16(t)


def standin_state_dict(module, tag, dtype=torch.float64):
    """unet_resnet_model.standin_value for every parameter, rounded to bf16 once, here"""
    return OrderedDict((name, to_bf16(M.standin_value("%s.%s" % (tag, name), name, tuple(v.shape))).to(dtype))
                       for name, v in module.state_dict().items())


def build(cin, cout, dtype=torch.float32):
    net = M.Resnet(cin, cout)
    net.load_state_dict(standin_state_dict(net, "%dto%d" % (cin, cout)))
    return net.to(dtype).eval()


def build_tree(dtype=torch.float32, c=320):
    net = M.Tree(c)
    net.load_state_dict(standin_state_dict(net, "tree%d" % c))
    return net.to(dtype).eval()


def record(case):
    """(float64 tap (n, H, W, cout), float64 output (n, H, W, cout), noise [tap, out], peak [tap, out]): the float64 run of
    the case on the bf16-rounded weights and inputs, and the reference arithmetic's noise against it = max|difference| /
    max|float64| of the fp32 run with every layer's output rounded to bf16"""
    cin, cout = case[:2]
    x, temb = inputs(case)
    net64, net32 = build(cin, cout, torch.float64), build(cin, cout, torch.float32)
    t64, t16 = {}, {}
    with torch.no_grad():
        o64 = net64(x.double(), temb.double(), taps=t64).permute(0, 2, 3, 1)
        o16 = net32(x.float(), temb.float(), round_bf16, t16).permute(0, 2, 3, 1)
    peaks = [float(t64["tap"].abs().max()), float(o64.abs().max())]
    noise = [float((t16["tap"].double() - t64["tap"]).abs().max() / peaks[0]), float((o16.double() - o64).abs().max() / peaks[1])]
    return t64["tap"].contiguous(), o64.contiguous(), noise, peaks
