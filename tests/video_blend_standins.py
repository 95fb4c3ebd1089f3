"""Stand-ins for what video_blend.py's Ebsynth stage reaches outside Python: cv2, flow_calc.get_flow, the Ebsynth
process (subprocess.run), and the path layout of blender.video_sequence.VideoSequence.  Shared by
tests/golden/make_propagate_golden.py (the reference's own process_one_sequence and guide classes on CPU) and
tests/test_gpu_propagate.py (fresco_amd.propagate with the same stand-ins), so both sides see the same I/O.

* cv2: imread / imwrite of real image files (PNG containers, so the shim's PIL loader reads them), with a
  deterministic lossy transform on ``.jpg`` writes: a driver that skips a round trip sees other bytes.  filter2D
  restated; inpaint a deterministic function of image and mask; cvtColor BGR -> gray.
* flow_calc.get_flow: fixed flows per save path (half-pixel ties, out-of-range and large values), saved with their
  occlusion masks as the real one saves them.
* answer(job): the Ebsynth stand-in, a deterministic function of the packed inputs (fresco_amd.propagate.load_job).
"""
import os
import shlex
import types
import zlib

import numpy as np
import torch
from PIL import Image

from fresco_amd import propagate as P

# ---------------------------------------------------------------------------------------------------------------------
# cv2
IMREAD_COLOR = 1
COLOR_BGR2GRAY = 6
INPAINT_TELEA = 1


def _to_u8(img):
    a = np.asarray(img)
    if a.dtype != np.uint8:
        a = np.clip(np.rint(a.astype(np.float64)), 0, 255).astype(np.uint8)  # convertTo(CV_8U): round, saturate
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    return a


def lossy(a):
    """the stand-in's 'JPEG': 8 grey levels per step, and a one-pixel blur along x of the low bits"""
    q = (a.astype(np.int32) >> 3) << 3
    return np.clip(q + (np.roll(a, 1, axis=1).astype(np.int32) & 7), 0, 255).astype(np.uint8)


def imwrite(path, img):
    a = _to_u8(img)
    if path.lower().endswith((".jpg", ".jpeg")):
        a = lossy(a)
    im = Image.fromarray(a if a.ndim == 2 else a[..., ::-1].copy())
    im.save(path, format="PNG")
    return True


def imread(path, flags=IMREAD_COLOR):
    if not os.path.exists(path):
        return None
    return np.ascontiguousarray(np.asarray(Image.open(path).convert("RGB"))[..., ::-1])


def cvtColor(img, code):
    assert code == COLOR_BGR2GRAY
    a = img.astype(np.int64)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def filter2D(img, ddepth, kernel):
    assert ddepth == -1
    k = np.asarray(kernel, np.int64)
    h, w = img.shape[:2]
    ys = np.concatenate([[1], np.arange(h), [h - 2]])
    xs = np.concatenate([[1], np.arange(w), [w - 2]])
    pad = img.astype(np.int64)[ys][:, xs]
    acc = np.zeros(img.shape, np.int64)
    for dy in range(3):
        for dx in range(3):
            acc += k[dy, dx] * pad[dy:dy + h, dx:dx + w]
    return np.clip(acc, 0, 255).astype(np.uint8)


def inpaint(img, mask, radius, flags):
    assert img.dtype == np.uint8 and mask.dtype == np.uint8 and flags == INPAINT_TELEA
    out = img.copy()
    m = mask != 0
    mean = img.reshape(-1, img.shape[-1]).astype(np.int64).sum(0) // (img.shape[0] * img.shape[1])
    out[m] = ((img[m].astype(np.int64) + mean * 3 + radius) // 4).astype(np.uint8)
    return out


cv2 = types.SimpleNamespace(IMREAD_COLOR=IMREAD_COLOR, COLOR_BGR2GRAY=COLOR_BGR2GRAY, INPAINT_TELEA=INPAINT_TELEA,
                            imread=imread, imwrite=imwrite, cvtColor=cvtColor, filter2D=filter2D, inpaint=inpaint)


# ---------------------------------------------------------------------------------------------------------------------
# flows
def fixed_flow(save_path, h, w):
    """float32 (1, 2, h, w) and the occlusion mask (h, w) of 0 / 1, a function of the file name alone"""
    rng = np.random.default_rng(zlib.crc32(os.path.basename(save_path).encode()))
    f = rng.integers(-6, 7, (2, h, w)).astype(np.float32) * np.float32(0.5)
    f[:, : h // 3] += np.float32(0.25) * rng.integers(-2, 3, (2, h // 3, w)).astype(np.float32)
    f[0, -1, : w // 2] = np.float32(3 * w)
    f[1, : h // 2, -1] = np.float32(-2.5 * h)
    occ = (rng.random((h, w)) < 0.15).astype(np.int64)
    return f[None], occ


def get_flow(image1, image2, save_path=None):
    """flow_calc.get_flow: an existing save path is read back; else the fixed flow is saved (npy) with its mask
    (<path>.png, 0 / 255) as the real one does"""
    if save_path is not None and os.path.exists(save_path):
        return read_flow(save_path)
    f, occ = fixed_flow(save_path or "", *image1.shape[:2])
    if save_path is not None:
        np.save(save_path, f)
        imwrite(os.path.splitext(save_path)[0] + ".png", occ[..., None] * 255)
    return torch.from_numpy(f)


def read_flow(save_path):
    return torch.from_numpy(np.load(save_path))


def read_mask(save_path):
    return cvtColor(imread(os.path.splitext(save_path)[0] + ".png"), COLOR_BGR2GRAY)


# ---------------------------------------------------------------------------------------------------------------------
# Ebsynth
def answer(job):
    """the Ebsynth stand-in: image and error map from the packed inputs of one frame"""
    st, tg = job["style"].astype(np.int64), job["target_guide"].astype(np.int64)
    sg = job["source_guide"].astype(np.int64)
    ns = st.shape[2]
    wsum = int(round(1000 * (sum(job["style_weights"]) + sum(job["guide_weights"]))))
    img = (st * 3 + tg[..., :ns] * 5 + np.roll(tg, 1, axis=2)[..., :ns] + sg[..., -ns:] + wsum) % 256
    err = (np.abs(tg - sg).sum(-1) * np.float32(job["style_weights"][0])).astype(np.float32)
    return img.astype(np.uint8), err


def answer_all(jobs):
    """propagate.run_ebsynth(synth=...): the stand-in for every job of a batch"""
    return [answer(j) for j in jobs]


class SubprocessStandin:
    """video_blend.subprocess: run(cmd, shell=True, ...) answers an Ebsynth command line as the shim would, through
    the same parse / decode / pack steps, and records the argv."""

    def __init__(self):
        self.argvs = []

    def run(self, cmd, shell=False, capture_output=False, **kw):
        argv = shlex.split(cmd)[1:]
        self.argvs.append(argv)
        job = P.load_job(argv)
        img, err = answer(job)
        P.write_output(job["cfg"]["output"], img, err)
        return types.SimpleNamespace(returncode=0)


# ---------------------------------------------------------------------------------------------------------------------
# the synthetic video and video_blend's path layout
def make_video(base, key_ind, h=24, w=28, seed=3):
    """frames video/%04d.png and keys keys/%04d.png (PNG: lossless in and out) under base"""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(base, "video"), exist_ok=True)
    os.makedirs(os.path.join(base, "keys"), exist_ok=True)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    for t in range(key_ind[0], key_ind[-1] + 1):
        frame = np.stack([(xs * 9 + t * 7) % 256, (ys * 11 + t * 3) % 256,
                          rng.integers(0, 256, (h, w))], -1).astype(np.uint8)
        imwrite(os.path.join(base, "video", "%04d.png" % t), frame)
    for k in key_ind:
        key = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        imwrite(os.path.join(base, "keys", "%04d.png" % k), key)


class VideoSequence:
    """blender.video_sequence.VideoSequence's paths as video_blend.create_sequence configures it (inputs and keys
    %04d.png, outputs %04d.jpg, out_<key> and tmp/out_<key> directories)"""

    def __init__(self, base_dir, key_ind, input_subdir="video", key_subdir="keys"):
        self.base, self.key_ind = base_dir, list(key_ind)
        self.input_dir = os.path.join(base_dir, input_subdir)
        self.key_dir = os.path.join(base_dir, key_subdir)
        self.tmp_dir = os.path.join(base_dir, "tmp")
        self.n_seq = len(key_ind) - 1
        for i in range(self.n_seq + 1):
            os.makedirs(self._out(i), exist_ok=True)
            os.makedirs(self._tmp(i), exist_ok=True)
        os.makedirs(os.path.join(base_dir, "blend"), exist_ok=True)

    def _out(self, i):
        return os.path.join(self.base, "out_%d" % self.key_ind[i])

    def _tmp(self, i):
        return os.path.join(self.tmp_dir, "out_%d" % self.key_ind[i])

    def get_sequence_beg_id(self, i):
        return self.key_ind[i]

    def interval(self, i):
        return self.key_ind[i + 1] - self.key_ind[i]

    def _ids(self, i, fwd):
        b, e = self.key_ind[i], self.key_ind[i + 1]
        return list(range(b, e)) if fwd else list(range(e, b, -1))

    def get_input_sequence(self, i, is_forward=True):
        return [os.path.join(self.input_dir, "%04d.png" % k) for k in self._ids(i, is_forward)]

    def get_output_sequence(self, i, is_forward=True):
        d = self._out(i if is_forward else i + 1)
        return [os.path.join(d, "%04d.jpg" % k) for k in self._ids(i, is_forward)]

    def _tmp_seq(self, i, fwd, prefix):
        d = self._tmp(i if fwd else i + 1)
        return [os.path.join(d, prefix + "%04d.jpg" % k) for k in self._ids(i, fwd)]

    def get_temporal_sequence(self, i, is_forward=True):
        return self._tmp_seq(i, is_forward, "temporal_")

    def get_edge_sequence(self, i, is_forward=True):
        return self._tmp_seq(i, is_forward, "edge_")

    def get_pos_sequence(self, i, is_forward=True):
        return self._tmp_seq(i, is_forward, "pos_")

    def get_flow_sequence(self, i, is_forward=True):
        b, e = self.key_ind[i], self.key_ind[i + 1]
        if is_forward:
            return [os.path.join(self.tmp_dir, "flow_f_%04d.npy" % k) for k in range(b, e - 1)]
        return [os.path.join(self.tmp_dir, "flow_b_%04d.npy" % k) for k in range(e, b + 1, -1)]

    def get_key_img(self, i):
        return os.path.join(self.key_dir, "%04d.png" % self.key_ind[i])


def snapshot(base):
    """{relative path: decoded pixels (images) or raw bytes (.bin)} of every file the stage writes under base"""
    out = {}
    for root, _, files in os.walk(base):
        for f in sorted(files):
            p = os.path.join(root, f)
            rel = os.path.relpath(p, base)
            if rel.startswith(("video" + os.sep, "keys" + os.sep)) or f.endswith(".npy"):
                continue
            if f.endswith(".bin"):
                out[rel] = np.frombuffer(open(p, "rb").read(), np.uint8)
            else:
                out[rel] = np.asarray(Image.open(p))
    return out


def inputs_digest(base):
    """sha256 of the decoded frames and keys under base (the golden keeps it: the synthetic video is rebuilt, not
    stored)"""
    import hashlib
    h = hashlib.sha256()
    for d in ("video", "keys"):
        for f in sorted(os.listdir(os.path.join(base, d))):
            h.update(np.ascontiguousarray(imread(os.path.join(base, d, f))).tobytes())
    return h.hexdigest()


def relative_argv(argv, base):
    return [os.path.relpath(a, base) if os.path.isabs(a) else a for a in argv]


KEY_IND = [0, 3, 7]  # two intervals of lengths 3 and 4
