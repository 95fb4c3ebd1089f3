"""Ebsynth on the GPU: propagate a stylised keyframe to another frame by guided patch-based synthesis (the second stage
of FRESCO, video_blend.py, which runs the reference's Ebsynth binary once per in-between frame).

``ebsynth_run`` is the Python entry point: one call into libfresco_hip.so (``fresco_ebsynth_run``) runs the whole
pyramid on the current stream.  ``ebsynth_run_batch`` runs n problems of one shape in one launch sequence
(``fresco_ebsynth_run_batch``), each equal to its own ``ebsynth_run``; ``edge_guide`` and ``warp_nearest`` build
video_blend.py's edge and warped guides on the GPU (fresco_amd.propagate drives all of them for the whole stage).  ``python -m fresco_amd.ebsynth`` (and the shell shim ``fresco_amd/bin/ebsynth``) is a
drop-in for the reference binary's command line: same flags, channel counting and default weights, and the same
``<output>.png`` + ``<output>.bin`` files (recipe C).
"""
import struct
import sys

import numpy as np
import torch

from .. import _lib, ops
from .._lib import FrescoHipError

VOTE_MODES = {"plain": 1, "weighted": 2}
MAX_STYLE_CHANNELS = 8
MAX_GUIDE_CHANNELS = 24


def max_pyramid_levels(source_hw, target_hw, patch_size):
    """The level count the binary picks for ``-pyramidlevels`` unset: the most levels whose coarsest one keeps the
    shorter side of min(source, target) >= 2 * patch_size + 1 (0 if even the full size is smaller)."""
    (sh, sw), (th, tw) = source_hw, target_hw
    return int(_lib.load().fresco_ebsynth_max_levels(int(sw), int(sh), int(tw), int(th), int(patch_size)))


def _per_level(name, v, levels):
    if isinstance(v, (list, tuple)):
        if len(v) != levels:
            raise ValueError("%s: %d values given for %d pyramid levels" % (name, len(v), levels))
        vals = [int(x) for x in v]
    else:
        vals = [int(v)] * levels
    if any(x < 0 for x in vals):
        raise ValueError("%s must be >= 0, got %r" % (name, v))
    return (_lib._c.c_int * max(levels, 1))(*(vals or [0]))


def _check_image(name, t, channels=None, hw=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError("%s must be a uint8 (H, W, C) tensor" % name)
    if channels is not None and t.shape[2] != channels:
        raise ValueError("%s has %d channels, expected %d" % (name, t.shape[2], channels))
    if hw is not None and tuple(t.shape[:2]) != tuple(hw):
        raise ValueError("%s is %dx%d, expected %dx%d" % ((name,) + tuple(t.shape[:2]) + tuple(hw)))


def _prepare(style, source_guide, target_guide, target_modulation, style_weights, guide_weights, patch_size,
             vote_mode, pyramid_levels, search_vote_iters, patchmatch_iters, stop_threshold):
    """Checks and ctypes arguments shared by ebsynth_run and ebsynth_run_batch; images are (h, w, c) per problem (the
    batch dimension already stripped from the shapes given)."""
    if vote_mode not in VOTE_MODES:
        raise ValueError("vote_mode must be one of %s, got %r" % (sorted(VOTE_MODES), vote_mode))
    sh, sw, ns = (int(v) for v in style)
    th, tw, ng = (int(v) for v in target_guide)
    sweights = [1.0 / ns] * ns if style_weights is None else [float(v) for v in style_weights]
    gweights = [1.0 / ng] * ng if guide_weights is None else [float(v) for v in guide_weights]
    if len(sweights) != ns or len(gweights) != ng:
        raise ValueError("style_weights / guide_weights need %d / %d values, got %d / %d"
                         % (ns, ng, len(sweights), len(gweights)))
    pyramid_levels = int(pyramid_levels)
    if pyramid_levels != -1 and pyramid_levels < 1:
        raise ValueError("pyramid_levels must be -1 or >= 1, got %d" % pyramid_levels)
    top = max_pyramid_levels((sh, sw), (th, tw), patch_size)
    levels = top if pyramid_levels == -1 else min(pyramid_levels, top)
    c = _lib._c
    return dict(sh=sh, sw=sw, ns=ns, th=th, tw=tw, ng=ng, levels=levels, top=top,
                svi=_per_level("search_vote_iters", search_vote_iters, levels),
                pmi=_per_level("patchmatch_iters", patchmatch_iters, levels),
                stop=_per_level("stop_threshold", stop_threshold, levels),
                sw_arr=(c.c_float * ns)(*sweights), gw_arr=(c.c_float * ng)(*gweights))


def ebsynth_run(style, source_guide, target_guide, *, target_modulation=None, style_weights=None, guide_weights=None,
                uniformity=3500.0, patch_size=5, vote_mode="plain", pyramid_levels=-1, search_vote_iters=6,
                patchmatch_iters=4, stop_threshold=5, extra_pass_3x3=False, seed=0, return_nnf=False):
    """Synthesise the target frame in the style of ``style``.

    style (sh, sw, ns), source_guide (sh, sw, ng), target_guide (th, tw, ng) and target_modulation (th, tw, ng, optional)
    are uint8 GPU tensors.  Weights default to the binary's for one style and one guide image: 1 / ns per style
    channel, 1 / ng per guide channel.  ``pyramid_levels`` -1
    picks the most levels (``max_pyramid_levels``); larger requests are capped to it, like the binary does.  The
    per-level arguments take an int (every level) or one value per level, coarse first.

    Returns (image uint8 (th, tw, ns), error float32 (th, tw)) and, with ``return_nnf``, the NNF int32 (th, tw, 2):
    the (x, y) centre of the source patch each target pixel maps to.  Raises FrescoHipError on CPU tensors and on
    what the library refuses (more than 8 style / 24 guide channels, an even patch, an image side below
    2 * patch_size + 1)."""
    _check_image("style", style)
    _check_image("source_guide", source_guide, hw=style.shape[:2])
    _check_image("target_guide", target_guide, channels=source_guide.shape[2])
    if target_modulation is not None:
        _check_image("target_modulation", target_modulation, channels=target_guide.shape[2],
                     hw=target_guide.shape[:2])
    a = _prepare(style.shape, source_guide.shape, target_guide.shape, target_modulation, style_weights, guide_weights,
                 patch_size, vote_mode, pyramid_levels, search_vote_iters, patchmatch_iters, stop_threshold)
    sh, sw, ns, th, tw, ng, levels = (a[k] for k in ("sh", "sw", "ns", "th", "tw", "ng", "levels"))
    ops._need_gpu(style, source_guide, target_guide, target_modulation)

    lib = _lib.load()
    dev = target_guide.device
    style, source_guide, target_guide = (t.contiguous() for t in (style, source_guide, target_guide))
    if target_modulation is not None:
        target_modulation = target_modulation.contiguous()
    nbytes = lib.fresco_ebsynth_workspace_bytes(ns, ng, sw, sh, tw, th, int(patch_size), levels,
                                                int(target_modulation is not None))
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    out = torch.empty((th, tw, ns), dtype=torch.uint8, device=dev)
    err = torch.empty((th, tw), dtype=torch.float32, device=dev)
    nnf = torch.empty((th, tw, 2), dtype=torch.int32, device=dev) if return_nnf else None
    rc = lib.fresco_ebsynth_run(style.data_ptr(), source_guide.data_ptr(), target_guide.data_ptr(),
                                ops._ptr(target_modulation), a["sw_arr"], a["gw_arr"], ns, ng, sw, sh, tw, th,
                                float(uniformity), int(patch_size), VOTE_MODES[vote_mode],
                                levels if a["top"] else -1, a["svi"], a["pmi"], a["stop"], int(bool(extra_pass_3x3)),
                                int(seed) & (2 ** 64 - 1), ops._ptr(nnf), out.data_ptr(), err.data_ptr(),
                                ws.data_ptr(), ws.numel(), ops._stream())
    _lib.check(rc, "fresco_ebsynth_run(style %dx%dx%d, target %dx%dx%d, patch %s)" % (sh, sw, ns, th, tw, ng,
                                                                                      patch_size))
    return (out, err, nnf) if return_nnf else (out, err)


MAX_BATCH = 64  # FRESCO_EBSYNTH_MAX_BATCH


def batch_workspace_bytes(n, n_style, n_guide, source_hw, target_hw, patch_size=5, with_modulation=False):
    """Device bytes ``ebsynth_run_batch`` allocates for n problems of these shapes (0 if the library refuses them)."""
    (sh, sw), (th, tw) = source_hw, target_hw
    return int(_lib.load().fresco_ebsynth_batch_workspace_bytes(int(n), int(n_style), int(n_guide), int(sw), int(sh),
                                                                 int(tw), int(th), int(patch_size), -1,
                                                                 int(bool(with_modulation))))


def _check_batch(name, t, channels=None, shape=None):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 4:
        raise ValueError("%s must be a uint8 (N, H, W, C) tensor" % name)
    if channels is not None and t.shape[3] != channels:
        raise ValueError("%s has %d channels, expected %d" % (name, t.shape[3], channels))
    if shape is not None and tuple(t.shape[:3]) != tuple(shape):
        raise ValueError("%s is %s, expected %s x H x W = %s" % (name, tuple(t.shape[:3]), name, tuple(shape)))


def ebsynth_run_batch(style, source_guide, target_guide, *, target_modulation=None, style_weights=None,
                      guide_weights=None, uniformity=3500.0, patch_size=5, vote_mode="plain", pyramid_levels=-1,
                      search_vote_iters=6, patchmatch_iters=4, stop_threshold=5, extra_pass_3x3=False, seeds=0,
                      return_nnf=False, workspace=None):
    """n ``ebsynth_run`` problems of one shape and one set of arguments in one launch sequence.

    style (n, sh, sw, ns), source_guide (n, sh, sw, ng), target_guide (n, th, tw, ng) and target_modulation
    (n, th, tw, ng, optional) are uint8 GPU tensors; ``seeds`` is one int for every problem or n ints.  Every other
    argument is ``ebsynth_run``'s and applies to every problem.  Returns (images (n, th, tw, ns), errors (n, th, tw))
    and, with ``return_nnf``, the NNFs (n, th, tw, 2): problem b equals ``ebsynth_run`` on its inputs and seed, bit for
    bit.  1 <= n <= MAX_BATCH.  ``workspace``: an optional uint8 GPU tensor of at least ``batch_workspace_bytes``
    (a caller running many batches of one shape can keep one)."""
    _check_batch("style", style)
    n = int(style.shape[0])
    _check_batch("source_guide", source_guide, shape=style.shape[:3])
    _check_batch("target_guide", target_guide, channels=source_guide.shape[3])
    if int(target_guide.shape[0]) != n:
        raise ValueError("target_guide holds %d problems, style %d" % (target_guide.shape[0], n))
    if target_modulation is not None:
        _check_batch("target_modulation", target_modulation, channels=target_guide.shape[3],
                     shape=target_guide.shape[:3])
    seeds = [int(seeds)] * n if isinstance(seeds, int) else [int(s) for s in seeds]
    if len(seeds) != n:
        raise ValueError("%d seeds given for %d problems" % (len(seeds), n))
    a = _prepare(style.shape[1:], source_guide.shape[1:], target_guide.shape[1:], target_modulation, style_weights,
                 guide_weights, patch_size, vote_mode, pyramid_levels, search_vote_iters, patchmatch_iters,
                 stop_threshold)
    sh, sw, ns, th, tw, ng, levels = (a[k] for k in ("sh", "sw", "ns", "th", "tw", "ng", "levels"))
    ops._need_gpu(style, source_guide, target_guide, target_modulation)

    lib = _lib.load()
    dev = target_guide.device
    style, source_guide, target_guide = (t.contiguous() for t in (style, source_guide, target_guide))
    if target_modulation is not None:
        target_modulation = target_modulation.contiguous()
    if workspace is None:
        nbytes = lib.fresco_ebsynth_batch_workspace_bytes(max(n, 1), ns, ng, sw, sh, tw, th, int(patch_size), levels,
                                                          int(target_modulation is not None))
        workspace = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    out = torch.empty((n, th, tw, ns), dtype=torch.uint8, device=dev)
    err = torch.empty((n, th, tw), dtype=torch.float32, device=dev)
    nnf = torch.empty((n, th, tw, 2), dtype=torch.int32, device=dev) if return_nnf else None
    seed_arr = (_lib._c.c_uint64 * max(n, 1))(*[s & (2 ** 64 - 1) for s in seeds])
    rc = lib.fresco_ebsynth_run_batch(n, style.data_ptr(), source_guide.data_ptr(), target_guide.data_ptr(),
                                      ops._ptr(target_modulation), a["sw_arr"], a["gw_arr"], ns, ng, sw, sh, tw, th,
                                      float(uniformity), int(patch_size), VOTE_MODES[vote_mode],
                                      levels if a["top"] else -1, a["svi"], a["pmi"], a["stop"],
                                      int(bool(extra_pass_3x3)), seed_arr, ops._ptr(nnf), out.data_ptr(),
                                      err.data_ptr(), workspace.data_ptr(), workspace.numel(), ops._stream())
    _lib.check(rc, "fresco_ebsynth_run_batch(n %d, style %dx%dx%d, target %dx%dx%d, patch %s)"
               % (n, sh, sw, ns, th, tw, ng, patch_size))
    return (out, err, nnf) if return_nnf else (out, err)


def _check_guide_input(name, img):
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() not in (3, 4):
        raise ValueError("%s must be a uint8 (H, W, C) or (N, H, W, C) tensor" % name)
    ops._need_gpu(img)
    return img.contiguous() if img.dim() == 4 else img.contiguous()[None]


def edge_guide(img):
    """video_blend.py's edge guide on the GPU: cv2.filter2D(img, -1, [[0,-1,0],[-1,4,-1],[0,-1,0]]) with
    BORDER_REFLECT_101, saturated, of a uint8 (h, w, c) or (n, h, w, c) tensor (sides >= 2, c <= 16)."""
    x = _check_guide_input("img", img)
    n, h, w, c = (int(v) for v in x.shape)
    out = torch.empty_like(x)
    rc = _lib.load().fresco_edge_guide(x.data_ptr(), out.data_ptr(), n, w, h, c, ops._stream())
    _lib.check(rc, "fresco_edge_guide(%dx%dx%dx%d)" % (n, h, w, c))
    return out if img.dim() == 4 else out[0]


def warp_nearest(img, flow):
    """flow_calc.warp(img, flow, 'nearest') on the GPU for a uint8 (h, w, c) or (n, h, w, c) tensor: grid_sample
    (nearest, zeros, align_corners=True) at pixel + flow.  flow: float32 (2, h, w) / (1, 2, h, w) per image, or
    (n, 2, h, w) for a batch (x plane first, as read_flow gives it)."""
    x = _check_guide_input("img", img)
    n, h, w, c = (int(v) for v in x.shape)
    if not isinstance(flow, torch.Tensor) or flow.dtype != torch.float32 or flow.numel() != n * 2 * h * w \
            or tuple(flow.shape[-3:]) != (2, h, w):
        raise ValueError("flow must be float32 (n, 2, %d, %d) for %d image(s), got %s"
                         % (h, w, n, tuple(getattr(flow, "shape", ()))))
    ops._need_gpu(flow)
    f = flow.contiguous()
    out = torch.empty_like(x)
    rc = _lib.load().fresco_warp_nearest(x.data_ptr(), f.data_ptr(), out.data_ptr(), n, w, h, c, ops._stream())
    _lib.check(rc, "fresco_warp_nearest(%dx%dx%dx%d)" % (n, h, w, c))
    return out if img.dim() == 4 else out[0]


def _stage_ws(w, h, ow, oh, dev):
    return torch.empty(max(int(_lib.load().fresco_ebsynth_stage_workspace_bytes(w, h, ow, oh)), 256),
                       dtype=torch.uint8, device=dev)


def resample(img, out_hw):
    """The run's pyramid downsample of one uint8 (h, w, c <= 16) GPU image to out_hw (bilinear, sample point
    (x, y) * w / out_w, clamped taps, truncated)."""
    _check_image("img", img)
    ops._need_gpu(img)
    img = img.contiguous()
    (h, w, c), (oh, ow) = img.shape, out_hw
    out = torch.empty((oh, ow, c), dtype=torch.uint8, device=img.device)
    ws = _stage_ws(w, h, ow, oh, img.device)
    rc = _lib.load().fresco_ebsynth_resample(img.data_ptr(), w, h, c, out.data_ptr(), ow, oh, ws.data_ptr(),
                                             ws.numel(), ops._stream())
    _lib.check(rc, "fresco_ebsynth_resample(%dx%dx%d -> %dx%d)" % (h, w, c, oh, ow))
    return out


def stop_mask(style_new, style_old, stop_threshold, patch_size):
    """The run's stop mask between two votes: uint8 (h, w), 255 where some style channel changed by >= stop_threshold,
    dilated by the patch."""
    _check_image("style_new", style_new)
    _check_image("style_old", style_old, channels=style_new.shape[2], hw=style_new.shape[:2])
    ops._need_gpu(style_new, style_old)
    a, b = style_new.contiguous(), style_old.contiguous()
    h, w, c = a.shape
    mask = torch.empty((h, w), dtype=torch.uint8, device=a.device)
    ws = _stage_ws(w, h, w, h, a.device)
    rc = _lib.load().fresco_ebsynth_stop_mask(a.data_ptr(), b.data_ptr(), w, h, c, int(stop_threshold),
                                              int(patch_size), mask.data_ptr(), ws.data_ptr(), ws.numel(),
                                              ops._stream())
    _lib.check(rc, "fresco_ebsynth_stop_mask(%dx%dx%d)" % (h, w, c))
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# the reference binary's command line (src/ebsynth/deps/ebsynth/src/ebsynth.cpp, main)
# ---------------------------------------------------------------------------------------------------------------------
class CliError(Exception):
    pass


_INT_FLAGS = {"-patchsize": "patchsize", "-pyramidlevels": "pyramidlevels", "-searchvoteiters": "searchvoteiters",
              "-patchmatchiters": "patchmatchiters", "-stopthreshold": "stopthreshold"}


def parse_cli(argv):
    """argv (without the program name) -> dict of settings, with the binary's defaults and checks."""
    cfg = dict(style=None, style_weight=-1.0, guides=[], output="output.png", uniformity=3500.0, patchsize=5,
               pyramidlevels=-1, searchvoteiters=6, patchmatchiters=4, stopthreshold=5, extrapass3x3=False)
    weight_target = None  # the -style (None key) or the guide index a following -weight applies to
    i = 0

    def value(flag, n=1):
        if i + n >= len(argv):
            raise CliError("missing argument for the %s option" % flag)
        return argv[i + 1:i + 1 + n]

    while i < len(argv):
        a = argv[i]
        if a == "-style":
            cfg["style"], = value(a)
            cfg["style_weight"] = -1.0
            weight_target = "style"
            i += 2
        elif a == "-guide":
            src, tgt = value(a, 2)
            cfg["guides"].append([src, tgt, -1.0])
            weight_target = len(cfg["guides"]) - 1
            i += 3
        elif a == "-output":
            cfg["output"], = value(a)
            i += 2
        elif a == "-weight":
            w = _parse_float(a, value(a)[0])
            if weight_target is None:
                raise CliError("at least one -style or -guide option must precede the -weight option!")
            if w < 0:
                raise CliError("weights must be non-negative!")
            if weight_target == "style":
                cfg["style_weight"] = w
            else:
                cfg["guides"][weight_target][2] = w
            i += 2
        elif a == "-uniformity":
            cfg["uniformity"] = _parse_float(a, value(a)[0])
            i += 2
        elif a in _INT_FLAGS:
            v = _parse_int(a, value(a)[0])
            if a == "-patchsize" and v < 3:
                raise CliError("patchsize is too small!")
            if a == "-patchsize" and v % 2 == 0:
                raise CliError("patchsize must be an odd number!")
            if a == "-pyramidlevels" and v < 1:
                raise CliError("bad argument for -pyramidlevels!")
            if a != "-patchsize" and a != "-pyramidlevels" and v < 0:
                raise CliError("bad argument for %s!" % a)
            cfg[_INT_FLAGS[a]] = v
            i += 2
        elif a == "-backend":  # accepted for compatibility; there is one backend
            value(a)
            i += 2
        elif a == "-extrapass3x3":
            cfg["extrapass3x3"] = True
            i += 1
        else:
            raise CliError("unrecognized option '%s'" % a)
    if cfg["style"] is None:
        raise CliError("a -style image is required")
    if not cfg["guides"]:
        raise CliError("at least one -guide pair is required")
    return cfg


def _parse_int(flag, s):
    try:
        return int(s)
    except ValueError:
        raise CliError("bad %s argument '%s'" % (flag, s))


def _parse_float(flag, s):
    try:
        return float(s)
    except ValueError:
        raise CliError("bad %s argument '%s'" % (flag, s))


def num_channels(rgba):
    """ebsynth.cpp evalNumChannels on an (H, W, 4) uint8 array: 1 if r == g == b everywhere else 3, +1 if any alpha is
    below 255."""
    gray = bool(np.all((rgba[..., 0] == rgba[..., 1]) & (rgba[..., 1] == rgba[..., 2])))
    alpha = bool(np.any(rgba[..., 3] < 255))
    return (1 if gray else 3) + (1 if alpha else 0)


def pick_channels(rgba, n):
    """The channels the binary keeps of an image counted as n channels: gray -> R, gray+alpha -> R, A."""
    return rgba[..., {1: [0], 2: [0, 3], 3: [0, 1, 2], 4: [0, 1, 2, 3]}[n]]


def pack_inputs(style_rgba, guides_rgba, style_weight=-1.0, guide_weights=None):
    """style_rgba (sh, sw, 4); guides_rgba [(source (sh, sw, 4), target (th, tw, 4))]; weights as given on the command
    line (-1 = default) -> (style, source_guide, target_guide, style_weights, guide_weights) packed like the binary:
    style weight 1 and guide weight 1 / number of guides by default, each divided by its image's channel count."""
    ns = num_channels(style_rgba)
    style = pick_channels(style_rgba, ns)
    guide_weights = guide_weights or [-1.0] * len(guides_rgba)
    srcs, tgts, gw = [], [], []
    for (s, t), w in zip(guides_rgba, guide_weights):
        n = max(num_channels(s), num_channels(t))
        srcs.append(pick_channels(s, n))
        tgts.append(pick_channels(t, n))
        w = 1.0 / len(guides_rgba) if w < 0 else w
        gw += [np.float32(w) / np.float32(n)] * n
    sw_ = 1.0 if style_weight < 0 else style_weight
    sweights = [np.float32(sw_) / np.float32(ns)] * ns
    return (np.ascontiguousarray(style), np.concatenate(srcs, -1), np.concatenate(tgts, -1),
            [float(v) for v in sweights], [float(v) for v in gw])


def bin_path(output):
    """<output without its last extension>.bin -- ebsynth.cpp cuts at the last '.' of the whole path."""
    k = output.rfind(".")
    return (output if k < 0 else output[:k]) + ".bin"


def write_error_bin(path, err):
    """int64 pixel count, then the fp32 error map row by row (what video_blend.py's load_error reads)."""
    e = np.ascontiguousarray(err, dtype=np.float32)
    with open(path, "wb") as f:
        f.write(struct.pack("<q", e.size))
        f.write(e.tobytes())


def _load_rgba(path):
    from PIL import Image
    try:
        return np.asarray(Image.open(path).convert("RGBA"))
    except (OSError, ValueError) as e:
        raise CliError("failed to load '%s': %s" % (path, e))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        print("usage: ebsynth -style <style.png> -guide <source.png> <target.png> [-weight <value>] ... "
              "[-output <output.png>] [-uniformity <value>] [-patchsize <size>] [-pyramidlevels <number>] "
              "[-searchvoteiters <number>] [-patchmatchiters <number>] [-stopthreshold <value>] [-extrapass3x3]")
        return 1
    try:
        cfg = parse_cli(argv)
        style = _load_rgba(cfg["style"])
        guides = [(_load_rgba(s), _load_rgba(t)) for s, t, _ in cfg["guides"]]
        for (s, t), (sn, tn, _) in zip(guides, cfg["guides"]):
            if s.shape[:2] != style.shape[:2]:
                raise CliError("source guide '%s' doesn't match the resolution of '%s'" % (sn, cfg["style"]))
            if t.shape[:2] != guides[0][1].shape[:2]:
                raise CliError("target guide '%s' doesn't match the resolution of '%s'" % (tn, cfg["guides"][0][1]))
        st, sg, tg, swt, gwt = pack_inputs(style, guides, cfg["style_weight"], [g[2] for g in cfg["guides"]])
        if st.shape[2] > MAX_STYLE_CHANNELS:
            raise CliError("too many style channels (%d), maximum number is %d" % (st.shape[2], MAX_STYLE_CHANNELS))
        if sg.shape[2] > MAX_GUIDE_CHANNELS:
            raise CliError("too many guide channels (%d), maximum number is %d" % (sg.shape[2], MAX_GUIDE_CHANNELS))
    except CliError as e:
        print("error: %s" % e)
        return 1
    dev = torch.device("cuda", torch.cuda.current_device())
    img, err = ebsynth_run(torch.from_numpy(st).to(dev), torch.from_numpy(sg).to(dev), torch.from_numpy(tg).to(dev),
                           style_weights=swt, guide_weights=gwt, uniformity=cfg["uniformity"],
                           patch_size=cfg["patchsize"], pyramid_levels=cfg["pyramidlevels"],
                           search_vote_iters=cfg["searchvoteiters"], patchmatch_iters=cfg["patchmatchiters"],
                           stop_threshold=cfg["stopthreshold"], extra_pass_3x3=cfg["extrapass3x3"])
    img = img.cpu().numpy()
    err = err.cpu().numpy()
    from PIL import Image
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(cfg["output"], format="PNG")
    write_error_bin(bin_path(cfg["output"]), err)
    print("image result was written to %s" % cfg["output"])
    print("binary result was written to %s" % bin_path(cfg["output"]))
    return 0


__all__ = ["ebsynth_run", "ebsynth_run_batch", "batch_workspace_bytes", "edge_guide", "warp_nearest",
           "max_pyramid_levels", "parse_cli", "pack_inputs", "num_channels", "write_error_bin",
           "bin_path", "main", "FrescoHipError"]
