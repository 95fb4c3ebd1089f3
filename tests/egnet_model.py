"""Stand-ins and restatements shared by tests/golden/make_egnet_golden.py, tests/test_egnet_cpu.py and tests/test_gpu_egnet.py.

The published EGNet checkpoint is not available to the tests:

  * weights: closed-form stand-ins, seeded by parameter name, drawn in float64 and cast --
      convolution weights  sqrt(2 / fan_in) N(0, 1), the stem `base.conv1.weight` additionally / 64 (its pixels are +-128);
      convolution biases   0.1 N(0, 1);
      BatchNorm weight     U(0.75, 1.25), x 0.25 for every bn3 (the residual branch: 16 blocks must not double the
                           activation each);  bias and running_mean 0.1 N(0, 1);  running_var U(0.75, 1.25);
    activations stay below 500 of the 1015 the operand planes hold at scale 64, the logits span about -14 .. +5 and the
    saliency map has saturated, empty and graded regions (tests/golden/make_egnet_golden.py asserts all of that);
  * frames: hed_model.frames(case).

`cv2sod64`, `dilate` and `saliency_from_logit` restate src/utils.py's cv2sod / Dilate / the last line of get_saliency in the
precision of their input; `param_shapes` the reference's state dict (the golden file keeps the reference's own list).
"""
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import hed_model

CASES = [(2, 64, 64), (1, 96, 128), (1, 72, 88)]
# recorded in a file of its own: the stem map is 32 x 32 = whole 16 x 16 patches, so the merge layers' 3 x 3 convolutions at
# that scale take the window-in-LDS form
WIDE_CASES = [(1, 128, 128)]
GOLDEN_FILES = ("egnet_golden.npz", "egnet_wide_golden.npz")  # under tests/golden: CASES, WIDE_CASES
MEANS = (104.00699, 116.66877, 122.67892)
TAPS = ("stem", "layer1", "layer2", "layer3", "layer4", "convert0", "convert1", "convert2", "convert3", "convert4",
        "edge_feature", "sal_feature0", "sal_feature1", "sal_feature2", "sal_feature3", "tmp_fea")
TAP_STRIDE = 16  # the golden files keep every 16th channel of a tap
K_DILATE = 7
STEM_GAIN, BIAS_STD, BN3_GAIN = 1.0 / 64.0, 0.1, 0.25
# Prefix of every parameter name where it seeds its draw.  Whether the saliency map has empty, saturated AND graded regions
# hangs on the last layers' draws: of the prefixes "" and "1:" .. "59:" this is the only one with which all four recorded
# cases meet the conditions tests/golden/make_egnet_golden.py asserts (most give a map that is zero everywhere).
SEED_SALT = "48:"

frames = hed_model.frames
digest = hed_model.digest


def load_golden(golden_dir):
    gold = {}
    for name in GOLDEN_FILES:
        gold.update(np.load(os.path.join(golden_dir, name)))
    return gold


def case_key(case):
    return "egnet_%dx%dx%d" % case


def _bn(prefix, c):
    return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)),
            (prefix + ".running_var", (c,)), (prefix + ".num_batches_tracked", ())]


def param_shapes():
    """name -> shape of the reference's TUN_bone('resnet') state dict, in its registration order"""
    out = []
    for i, (a, b) in enumerate(zip((64, 256, 512, 1024, 2048), (128, 256, 512, 512, 512))):
        out.append(("convert.convert0.%d.0.weight" % i, (b, a, 1, 1)))
    out.append(("base.conv1.weight", (64, 3, 7, 7)))
    out += _bn("base.bn1", 64)
    inplanes = 64
    for layer, (planes, blocks) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), 1):
        for b in range(blocks):
            p = "base.layer%d.%d" % (layer, b)
            out.append((p + ".conv1.weight", (planes, inplanes, 1, 1)))
            out += _bn(p + ".bn1", planes)
            out.append((p + ".conv2.weight", (planes, planes, 3, 3)))
            out += _bn(p + ".bn2", planes)
            out.append((p + ".conv3.weight", (4 * planes, planes, 1, 1)))
            out += _bn(p + ".bn3", 4 * planes)
            if b == 0:
                out.append((p + ".downsample.0.weight", (4 * planes, inplanes, 1, 1)))
                out += _bn(p + ".downsample.1", 4 * planes)
            inplanes = 4 * planes
    merge1 = ((128, 256, 128, 3), (256, 512, 256, 3), (512, 0, 512, 5), (512, 0, 512, 5), (512, 0, 512, 7))
    for i, (cin, cout) in enumerate(((256, 128), (512, 256), (512, 128))):
        out.append(("merge1.trans.%d.0.weight" % i, (cout, cin, 1, 1)))
    for i, (a, _, c, k) in enumerate(merge1):
        for idx, cin in ((0, a), (2, c), (4, c)):
            out.append(("merge1.up.%d.%d.weight" % (i, idx), (c, cin, k, k)))
            out.append(("merge1.up.%d.%d.bias" % (i, idx), (c,)))
    for i, (_, _, c, _) in enumerate(merge1):
        out.append(("merge1.score.%d.weight" % i, (1, c, 3, 3)))
        out.append(("merge1.score.%d.bias" % i, (1,)))
    for j, cin in enumerate((256, 512, 512, 512)):
        out.append(("merge2.trans.0.%d.0.weight" % j, (128, cin, 1, 1)))
    for j, k in enumerate((3, 5, 5, 7)):
        for idx in (0, 2, 4):
            out.append(("merge2.up.0.%d.%d.weight" % (j, idx), (128, 128, k, k)))
            out.append(("merge2.up.0.%d.%d.bias" % (j, idx), (128,)))
    for j in range(4):
        out.append(("merge2.score.0.%d.weight" % j, (1, 128, 3, 3)))
        out.append(("merge2.score.0.%d.bias" % j, (1,)))
    out += [("merge2.final_score.0.weight", (128, 128, 5, 5)), ("merge2.final_score.0.bias", (128,)),
            ("merge2.final_score.2.weight", (1, 128, 3, 3)), ("merge2.final_score.2.bias", (1,))]
    return dict(out)


def _rs(name):
    return np.random.RandomState(zlib.crc32((SEED_SALT + name).encode()) & 0x7FFFFFFF)


_IS_BN = (".bn1.", ".bn2.", ".bn3.", ".downsample.1.")


def standin_state_dict(dtype=torch.float32):
    sd = {}
    for name, shape in param_shapes().items():
        rs = _rs(name)
        bn = any(t in name for t in _IS_BN)
        if name.endswith("num_batches_tracked"):
            sd[name] = torch.zeros((), dtype=torch.int64)
            continue
        if bn and name.endswith((".weight", ".running_var")):
            v = rs.uniform(0.75, 1.25, shape)
            if name.endswith(".weight") and ".bn3." in name:
                v = v * BN3_GAIN
        elif bn or name.endswith(".bias"):  # BatchNorm bias / running_mean, convolution biases
            v = BIAS_STD * rs.standard_normal(shape)
        else:
            fan_in = shape[1] * shape[2] * shape[3]
            v = np.sqrt(2.0 / fan_in) * rs.standard_normal(shape)
            if name == "base.conv1.weight":
                v = v * STEM_GAIN
        sd[name] = torch.from_numpy(np.asarray(v, np.float64)).to(dtype)
    return sd


def weights_digest():
    sd = standin_state_dict()
    return digest(*[sd[k].numpy() for k in sd])


def cv2sod64(frames_u8, dtype=torch.float64):
    """cv2sod of every frame, (n, 3, H // 2, W // 2): channel means subtracted (in float64, as numpy subtracts a float64
    array from a float32 image, then rounded to `dtype`), the 2 x 2 block mean in `dtype`.  dtype=torch.float32 gives
    utils.cv2sod's own tensor."""
    x = torch.from_numpy(np.asarray(frames_u8)).double() - torch.tensor(MEANS, dtype=torch.float64)
    return F.interpolate(x.to(dtype).permute(0, 3, 1, 2), scale_factor=0.5, mode="bilinear")


def dilate(x, k):
    """utils.Dilate(kernel_size=k): replicate padding, k x k box sum, clamp to [0, 1]; x (n, 1, h, w)"""
    r = (k - 1) // 2
    x = F.pad(x, (r, r, r, r), "replicate")
    return torch.clamp(F.conv2d(x, torch.ones(1, 1, k, k, dtype=x.dtype)), 0, 1)


def saliency_from_logit(logit, k=K_DILATE):
    """get_saliency's last line on a logit (n, 1, h, w), in the logit's precision"""
    return 1 - dilate(torch.sigmoid(logit), k)


def golden_pair(gold, key):
    """-> (the fp32 record, the float64 one) of `key`; float64 records are stored as the float32 record plus a float32
    difference"""
    f32 = gold[key + "_f32"]
    return f32, f32.astype(np.float64) + gold[key + "_d64"].astype(np.float64)
