"""Key-frame selection (reference: src/keyframe_selection.py get_keyframe_ind, src/utils.py resize_image) with the per-frame
work on the GPU.

The reference runs, for every frame of the video, resize_image (cv2.resize, INTER_AREA or INTER_LANCZOS4) ->
cv2.GaussianBlur(img, (9, 9), 0) -> numpy2tensor(...).cuda() -> F.mse_loss(prev, cur).cpu(): one upload and one device
synchronisation per frame.  Here a chunk of frames is uploaded once and goes through

    ops.resize_area_u8 or, where the geometry enlarges, ops.resize_taps_u8 (one launch) -> ops.frame_sq_diffs (two launches: the blur of both frames of every pair in LDS and
    the integer sum of their squared differences; the last resized frame is carried into the next chunk)

and the sums of all chunks come back in one copy at the end.  The greedy choice over the error curve (select_keyframes)
stays on the host, restated with its quirks.  DESIGN.md section 15 has the rules and what is verified; INTEGRATION.md
recipe J the ways to use it.
"""
import numpy as np
import torch

from . import ops
from ._lib import FrescoHipError

CHUNK = 32  # frames decoded, uploaded and measured at a time


def resize_size(H0, W0, resolution):
    """resize_image's arithmetic: (H, W, k) -- the sides scaled by k = resolution / min(H0, W0) and rounded (np.round: half
    to even) to multiples of 64"""
    H, W = float(H0), float(W0)
    k = float(resolution) / min(H, W)
    H *= k
    W *= k
    return int(np.round(H / 64.0)) * 64, int(np.round(W / 64.0)) * 64, k


def _check_batch(frames, what):
    if not isinstance(frames, torch.Tensor):
        raise TypeError("%s: expected a uint8 tensor (n, H, W, 3), got %s" % (what, type(frames).__name__))
    if frames.dtype != torch.uint8:
        raise TypeError("%s: frames are uint8, got %s" % (what, frames.dtype))
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("%s: frames must be (n, H, W, 3) with three channels, got %s" % (what, tuple(frames.shape)))
    return frames


def resize_frames(frames, resolution=512, enlarge=False):
    """frames: uint8 (n, H0, W0, 3) on the GPU -> resize_image of every frame, uint8 (n, H, W, 3) on the GPU.  By default
    only the shrinking INTER_AREA case is taken: k > 1 (the reference switches to Lanczos) and a side that the rounding to
    64 would enlarge raise NotImplementedError.  enlarge=True takes every geometry as resize_image and cv2.resize do
    together: k > 1 -> INTER_LANCZOS4 on both sides, whatever each does; otherwise INTER_AREA, which is the area rule when no
    side grows and its two-tap rule on both sides when one does.  There is no host fallback."""
    _check_batch(frames, "resize_frames")
    _, H0, W0, _ = frames.shape
    H, W, k = resize_size(H0, W0, resolution)
    if H <= 0 or W <= 0:
        raise NotImplementedError("resize_frames: %d x %d to resolution %s gives %d x %d after the rounding to multiples "
                                  "of 64; an empty image is not built" % (H0, W0, resolution, H, W))
    if k > 1:
        if not enlarge:
            raise NotImplementedError("resize_frames: %d x %d to resolution %s enlarges (k = %.4f > 1): the reference "
                                      "resizes with INTER_LANCZOS4 there, which only enlarge=True takes"
                                      % (H0, W0, resolution, k))
        return ops.resize_taps_u8(frames.contiguous(), H, W, ops.RESIZE_LANCZOS4)
    if H > H0 or W > W0:
        if not enlarge:
            raise NotImplementedError("resize_frames: %d x %d to resolution %s gives %d x %d after the rounding to "
                                      "multiples of 64; INTER_AREA that enlarges a side is another rule, which only "
                                      "enlarge=True takes" % (H0, W0, resolution, H, W))
        return ops.resize_taps_u8(frames.contiguous(), H, W, ops.RESIZE_LINEAR_AREA)
    return ops.resize_area_u8(frames.contiguous(), H, W)


def resize_image(input_image, resolution):
    """The reference's resize_image protocol: an (H0, W0, 3) uint8 array in, the resized array out (through the GPU)."""
    if not isinstance(input_image, np.ndarray) or input_image.dtype != np.uint8 or input_image.ndim != 3 \
            or input_image.shape[2] != 3:
        raise TypeError("resize_image: the image is an (H, W, 3) uint8 array")
    frames = torch.from_numpy(np.ascontiguousarray(input_image)[None]).cuda()
    return resize_frames(frames, resolution, enlarge=True)[0].cpu().numpy()


def _as_chunk(chunk):
    """one chunk (a uint8 tensor (n, H, W, 3) / (H, W, 3), an array of those shapes, or a list of (H, W, 3) arrays) -> the
    uint8 tensor (n, H, W, 3) on the GPU: host data is uploaded in one piece"""
    if isinstance(chunk, (list, tuple)):
        if not chunk:
            raise ValueError("frame_errors: an empty chunk")
        if isinstance(chunk[0], torch.Tensor):
            chunk = torch.stack(list(chunk), 0)
        else:
            chunk = np.stack([np.asarray(f) for f in chunk], 0)
    if isinstance(chunk, np.ndarray):
        if chunk.dtype != np.uint8:
            raise TypeError("frame_errors: frames are uint8, got %s" % chunk.dtype)
        if chunk.ndim == 3:
            chunk = chunk[None]
        chunk = torch.from_numpy(np.ascontiguousarray(chunk)).cuda()
    if isinstance(chunk, torch.Tensor) and chunk.dim() == 3:
        chunk = chunk[None]
    return _check_batch(chunk, "frame_errors").contiguous()


def _chunks_of(source):
    """a tensor / array batch -> itself as the one chunk; anything else iterable -> its items as chunks"""
    if isinstance(source, (torch.Tensor, np.ndarray)):
        return [source]
    return source


def _sq_diff_chunks(chunks, resolution, keep_frames, measure=True):
    """-> (device int64 sums of all chunks concatenated or None, (H, W), the list of resized chunks if keep_frames);
    measure=False only resizes"""
    sums, kept, carry, size = [], [], None, None
    for chunk in chunks:
        frames = _as_chunk(chunk)
        if resolution is not None:
            frames = resize_frames(frames, resolution, enlarge=True)
        if size is None:
            size = tuple(frames.shape[1:3])
        elif tuple(frames.shape[1:3]) != size:
            raise ValueError("frame_errors: the chunks hold frames of one size, got %s after %s"
                             % (tuple(frames.shape[1:3]), size))
        if measure:
            sums.append(ops.frame_sq_diffs(frames, carry))
            carry = frames[-1]  # (a view of this chunk: it stays alive through the next call)
        if keep_frames:
            kept.append(frames)
    return (torch.cat(sums) if sums else None), size, kept


def _curve(sums, size):
    """the sums of squared 8-bit differences -> the reference's errors: mse_loss of x / 255 * 2 - 1 over 3 H W elements is
    S * 4 / (65025 * 3 H W); float32 as the reference's loss is"""
    if sums is None:
        return np.zeros(1)  # the reference's curve starts as [0] whether or not a frame could be read
    H, W = size
    s = sums.cpu().numpy()  # the one device-to-host copy
    err = np.array([float(np.float32(int(v) * 4 / (65025 * 3 * H * W))) for v in s], dtype=np.float64)
    err[0] = 0.0
    return err


def frame_errors(frames_or_chunks, resolution=None):
    """The error curve of get_keyframe_ind: err[0] = 0, err[i] = the MSE between the blurred frames i - 1 and i in the
    reference's [-1, 1] scale, as the nearest fp32 to S_i * 4 / (65025 * 3 H W).  frames_or_chunks: a uint8 tensor or array
    (n, H, W, 3), or an iterable of such chunks of one frame size (the last frame of a chunk is carried into the next);
    resolution: resize_image's, applied first when given.  One device-to-host copy, at the end."""
    sums, size, _ = _sq_diff_chunks(_chunks_of(frames_or_chunks), resolution, False)
    return _curve(sums, size)


def select_keyframes(err, mininterv, maxinterv):
    """The reference's greedy loop on the error curve, quirks kept: keys start as [0, n - 1]; the first and last mininterv
    entries become the sentinel -1 (err[-0:] at mininterv = 0 is the whole curve); while the largest gap between keys
    exceeds maxinterv the first index of the maximum becomes a key and err[ind - mininterv : ind + mininterv] is blanked
    (a negative start wraps as numpy slices do); the loop ends when the maximum is a sentinel."""
    err = np.array(err, dtype=np.float64)
    n = len(err)
    keys = [0, n - 1]
    err[0:mininterv] = -1
    err[-mininterv:] = -1

    def gap(keys):
        return max([1] + [keys[i + 1] - keys[i] for i in range(len(keys) - 1)])

    while gap(keys) > maxinterv:
        ind = int(np.argmax(err))
        if err[ind] == -1:
            break
        err[ind - mininterv:ind + mininterv] = -1
        for i, k in enumerate(keys):  # insert_key: before the first larger key, nowhere if there is none
            if ind < k:
                keys.insert(i, ind)
                break
    return keys


def _video_chunks(filename, n_limit):
    """decode `filename` with cv2 in chunks of CHUNK frames, at most n_limit frames"""
    try:
        import cv2
    except ImportError:
        raise FrescoHipError("get_keyframe_ind: decoding %r needs cv2 (opencv-python), which cannot be imported here; "
                             "pass the decoded frames (or an iterable of chunks of frames) instead" % (filename,))
    cap = cv2.VideoCapture(filename)
    n_frames = max(1, min(int(cap.get(cv2.CAP_PROP_FRAME_COUNT)), n_limit))
    chunk = []
    for _ in range(int(n_frames)):
        success, frame = cap.read()
        if not success:
            break
        # no BGR -> RGB swap: resize, blur and the squared error treat the three channels alike and sum over them, so the
        # curve is the same for either order (with return_frames the caller gets the frames in the decoder's BGR order)
        chunk.append(frame)
        if len(chunk) == CHUNK:
            yield chunk
            chunk = []
    if chunk:
        yield chunk


def _frame_chunks(source, n_limit):
    """frames (a tensor / array (n, H0, W0, 3), or an iterable of (H0, W0, 3) frames) -> chunks of CHUNK frames, at most
    n_limit frames"""
    if isinstance(source, (torch.Tensor, np.ndarray)):
        if source.ndim != 4:
            raise ValueError("get_keyframe_ind: a batch of frames is (n, H, W, 3), got %s" % (tuple(source.shape),))
        n = int(min(len(source), n_limit))
        for i in range(0, n, CHUNK):
            yield source[i:min(i + CHUNK, n)]
        return
    chunk, taken = [], 0
    for frame in source:
        if taken >= n_limit:
            break
        chunk.append(frame)
        taken += 1
        if len(chunk) == CHUNK:
            yield chunk
            chunk = []
    if chunk:
        yield chunk


def get_keyframe_ind(source, lastframen=1e10, mininterv=5, maxinterv=20, viz=False, return_frames=False):
    """The reference's get_keyframe_ind(filename, lastframen, mininterv, maxinterv, viz).  source: a file name (decoded
    with cv2, imported only then) or the decoded frames -- a uint8 tensor / array (n, H0, W0, 3) or an iterable of
    (H0, W0, 3) frames; at most max(1, min(count, lastframen)) of them are used.  Frames are resized to resolution 512,
    as the reference does.  return_frames=True returns (keys, the resized frames as a uint8 tensor (n, H, W, 3) on the
    GPU, or None when there was no frame), which spares run_fresco.py its second read-and-resize pass."""
    if viz:
        raise NotImplementedError("get_keyframe_ind: viz=True (the reference's matplotlib plot) is not built")
    same = maxinterv == mininterv
    if same and not return_frames:
        return list(range(0, lastframen, mininterv))
    n_limit = max(1, lastframen)
    chunks = _video_chunks(source, n_limit) if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__") \
        else _frame_chunks(source, n_limit)
    sums, size, kept = _sq_diff_chunks(chunks, 512, return_frames, measure=not same)
    keys = list(range(0, lastframen, mininterv)) if same else select_keyframes(_curve(sums, size), mininterv, maxinterv)
    if return_frames:
        return keys, (torch.cat(kept) if kept else None)
    return keys


def patch_keyframe_selection(module=None):
    """Rebind get_keyframe_ind on the reference's src.keyframe_selection (default) or on a module that imported the name
    from it (run_fresco, webUI)."""
    if module is None:
        import src.keyframe_selection as module
    module.get_keyframe_ind = get_keyframe_ind
    return module
