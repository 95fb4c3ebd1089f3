"""Tensor-level entry points over the C ABI (include/fresco_hip.h).

PyTorch is used for device memory, the current HIP stream and dtype casts only; every arithmetic op
below is one call into libfresco_hip.so.  All functions require HIP ("cuda") tensors and raise on
CPU tensors -- there is no fallback path.
"""
import ctypes
import math

import torch

from . import _lib
from ._lib import FrescoHipError


try:  # raw handle of the current HIP stream without building a torch.cuda.Stream object (~10x cheaper per call)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except AttributeError:  # pragma: no cover
    _raw_stream = None


def _stream():
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise FrescoHipError("fresco_amd operators run on the GPU only (got a %s tensor); "
                                 "there is no CPU fallback" % t.device)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _planes(rows, C, device, want=True):
    """a pair of uninitialised (hi, lo) fp16 operand planes of (rows, C), or (None, None) when they are not wanted"""
    if not want:
        return None, None
    return (torch.empty(rows, C, dtype=torch.float16, device=device), torch.empty(rows, C, dtype=torch.float16, device=device))


def _f32c(t):
    return t.to(torch.float32).contiguous()


def _split_scale(scale):
    """the power of two a pair of (hi, lo) operand planes is written with, as a float"""
    scale = float(scale)
    if not (scale > 0 and math.isfinite(scale) and math.frexp(scale)[0] == 0.5):
        raise ValueError("split scale %r must be a power of two" % (scale,))
    return scale


def _dense(t, name, dtype, shape=None, align=1):
    """the kernels read raw words: dtype, density and (where they move 16-byte pieces) alignment are checked here, on the
    host; the caller ends its checks with _need_gpu"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a tensor, got %s" % (name, type(t).__name__))
    if t.dtype != dtype:
        raise TypeError("%s: dtype %s, expected %s" % (name, t.dtype, dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s: shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    if not t.is_contiguous():
        raise ValueError("%s: must be contiguous" % name)
    if t.data_ptr() % align:
        raise ValueError("%s: must be %d-byte aligned" % (name, align))
    return t


def _rows(t):
    """(tensor, row stride in elements, rows) for a (..., C) tensor whose rows are uniformly strided
    (dense, or a column slice of a dense (..., k*C) tensor such as a fused projection output);
    anything else is made dense first."""
    C = t.shape[-1]
    if t.is_contiguous() and C % 8 == 0 and t.dim() >= 2 and t.data_ptr() % 16 == 0:  # the common case
        return t, C, t.numel() // C
    ok = t.stride(-1) == 1 and t.dim() >= 2
    if ok:
        ld = t.stride(-2)
        exp = ld
        for d in range(t.dim() - 2, -1, -1):  # leading dims must nest without gaps
            if t.shape[d] != 1 and t.stride(d) != exp:
                ok = False
                break
            exp *= t.shape[d]
        ok = ok and ld >= C and ld % 8 == 0 and t.data_ptr() % 16 == 0
    if not ok:
        t = t.contiguous()
        ld = C
    return t, ld, t.numel() // C


class Workspace:
    """Grow-only device scratch buffer (the C ABI never allocates)."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        return self.buf


class OptContext:
    """A fresco_ctx (include/fresco_hip.h): the side stream + events the two-pipeline form of fresco_opt_run uses.  Owned
    by the caller -- the library keeps no process-wide stream table; one context per host thread and device."""

    def __init__(self):
        p = ctypes.c_void_p()
        _lib.check(_lib.load().fresco_ctx_create(ctypes.byref(p)), "fresco_ctx_create")
        self.ptr = p

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                _lib.load().fresco_ctx_destroy(self.ptr)
                self.ptr = None
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass


class _PerThreadContexts:
    def __init__(self):
        import threading
        self._tls = threading.local()

    def get(self, device):
        table = getattr(self._tls, "table", None)
        if table is None:
            table = self._tls.table = {}
        ctx = table.get(device)
        if ctx is None:
            ctx = table[device] = OptContext()
        return ctx


_opt_contexts = _PerThreadContexts()


class _PerStreamWorkspace:
    """Default scratch when the caller passes none: one grow-only buffer per (thread, device, stream), so
    that concurrent callers on different streams or threads never share scratch memory."""

    def __init__(self):
        import threading

        self._tls = threading.local()

    def get(self, nbytes, device):
        table = getattr(self._tls, "table", None)
        if table is None:
            table = self._tls.table = {}
        key = (device, _stream())
        ws = table.get(key)
        if ws is None:
            ws = table[key] = Workspace()
        return ws.get(nbytes, device)


_default_ws = _PerStreamWorkspace()


# ---------------------------------------------------------------------------------------------
# fused linear projections
# ---------------------------------------------------------------------------------------------
# element types of the 16-bit MFMA kernels (linear, attention, temporal attention) -> dtype code of their entry points
_MFMA_DTYPES = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


_linear_supported = {}


def linear_plan(nw, M, N, K):
    """(rc, row_blocks, splits, tiles_per_split) of the launch `linear` would make for nw weights of (N, K) and M rows
    (fresco_linear_plan: host arithmetic, no GPU needed); rc != 0 (the library's refusal) leaves the rest at 0"""
    rb, sp, tps = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.load().fresco_linear_plan(int(nw), int(M), int(N), int(K), ctypes.byref(rb), ctypes.byref(sp),
                                        ctypes.byref(tps))
    return rc, rb.value, sp.value, tps.value


def linear_supported(K, N, dtype, nw=1):
    """shapes / dtype fresco_linear takes for a launch of `nw` weights (SD-1.5 up_blocks.2/3 attention widths; nw * N is
    bounded by the kernel's LDS plan); others keep torch's GEMM.  The library answers (fresco_linear_plan), not a copy of
    its rules; the answer per (K, N, nw) is kept, the processor asks on every layer call)."""
    if dtype not in _MFMA_DTYPES:
        return False
    key = (K, N, nw)
    ok = _linear_supported.get(key)
    if ok is None:
        ok = _linear_supported[key] = linear_plan(nw, 1, N, K)[0] == _lib.OK
    return ok


def linear(x, weights, biases=None, outs=None, x_rows=None, x_rows_trusted=False):
    """out_j = x W_j^T (+ b_j) for the 1..3 weight matrices in `weights` (each (N, K) fp16, read where it lives --
    nothing is stacked or cached), x (..., K) fp16 read once; `biases`: None or a list of (N,) fp16 / None.
    All-bf16 operands are taken the same way (bf16 MFMA, fp32 accumulation, bf16 outputs); mixed dtypes raise.
    Returns len(weights) tensors shaped x.shape[:-1] + (N,); `outs` may supply them (dense in the last dim,
    uniformly strided rows -- e.g. the two halves of a fused K|V buffer).
    x_rows (int32, (M',)): gathered form -- output row m is the projection of x's flat row x_rows[m]; the outputs are
    (M', N).  The table is bounds-checked once (a host synchronisation; cached with the tensor) unless the caller vouches
    for it (`x_rows_trusted`: tables derived from a mask's non-zero positions)."""
    if torch.is_tensor(weights):
        weights = [weights]
    weights = list(weights)
    nw = len(weights)
    if biases is None:
        biases = [None] * nw
    elif torch.is_tensor(biases):
        biases = [biases]
    _need_gpu(x, *weights, *[b for b in biases if b is not None])
    K = x.shape[-1]
    N = weights[0].shape[0]
    if not 1 <= nw <= 3 or len(biases) != nw:
        raise ValueError("linear: 1..3 weights and as many biases (or None)")
    dt = x.dtype
    if dt not in _MFMA_DTYPES:
        raise ValueError("linear: x must be fp16 or bf16 (got %s)" % dt)
    for W in weights:
        if W.dtype != dt or tuple(W.shape) != (N, K) or not W.is_contiguous():
            raise ValueError("linear: x (...,K) and every W (N,K) must be contiguous, of one dtype (fp16 or bf16), with "
                             "matching shapes")
    for b in biases:
        if b is not None and (b.dtype != dt or tuple(b.shape) != (N,) or not b.is_contiguous()):
            raise ValueError("linear: a bias must be a contiguous (N,) tensor of x's dtype")
    x2, x_ld, M = _rows(x)
    if x_rows is not None:
        _need_gpu(x_rows)
        if x_rows.dtype != torch.int32 or x_rows.dim() != 1 or not x_rows.is_contiguous():
            raise TypeError("linear: x_rows must be a contiguous 1-D int32 tensor")
        n_x = M

        def run(x_rows=x_rows, n_x=n_x):
            lo, hi = int(x_rows.min()), int(x_rows.max())
            if lo < 0 or hi >= n_x:
                raise ValueError("linear: x_rows address rows %d..%d but x has %d rows" % (lo, hi, n_x))
        if not x_rows_trusted:
            _check_once(("xrows", x_rows.data_ptr(), x_rows.numel(), x_rows._version, n_x), x_rows, run)
        M = x_rows.numel()
    if outs is None:
        shape = (M, N) if x_rows is not None else x.shape[:-1] + (N,)
        outs = [torch.empty(shape, dtype=dt, device=x.device) for _ in range(nw)]
    ptrs, lds = [], []
    for t in outs:
        t2, ld, rows = _rows(t)
        if t2 is not t or rows != M or t.shape[-1] != N or t.dtype != dt:
            raise ValueError("linear: every output must be a (M,N) tensor of x's dtype with uniformly strided rows")
        ptrs.append(t.data_ptr())
        lds.append(ld)
    wp = [W.data_ptr() for W in weights] + [None] * (3 - nw)
    bp = [_ptr(b) for b in biases] + [None] * (3 - nw)
    while len(ptrs) < 3:
        ptrs.append(None)
        lds.append(0)
    rc = _lib.load().fresco_linear(x2.data_ptr(), x_ld, _ptr(x_rows), wp[0], wp[1], wp[2], bp[0], bp[1], bp[2], ptrs[0],
                                   ptrs[1], ptrs[2], lds[0], lds[1], lds[2], nw, M, N, K, _MFMA_DTYPES[dt], _stream())
    _lib.check(rc, "fresco_linear(M=%d,N=%d,K=%d,nw=%d)" % (M, N, K, nw))
    return outs


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def attention(q, k, v, heads, scale, *, kv_rows=None, n_groups=None, M=None, group_rows=None,
              diag_bias=0.0, workspace=None):
    """softmax(scale * q k^T + diag_bias*I) v with grouped keys (fresco_attn_fwd).

    q: (B, Lq, C) fp16.  k, v: (..., C) fp16 whose leading dims flatten to rows.  Or all three bf16 (bf16 MFMA kernels:
    fp32 scores and softmax, the scale applied in fp32, bf16 output).
    Default grouping: one key group per batch element (plain attention): k, v are (B, Lk, C).
    """
    _need_gpu(q, k, v, kv_rows)
    if q.dtype not in _MFMA_DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError("fresco_amd.attention: q, k, v must all be fp16 or all bf16 (got %s/%s/%s)"
                        % (q.dtype, k.dtype, v.dtype))
    B, Lq, C = q.shape
    D = C // heads
    if D * heads != C:
        raise ValueError("channels %d not divisible by heads %d" % (C, heads))
    q, q_ld, _ = _rows(q)
    k, kv_ld, k_rows = _rows(k)
    v, v_ld, v_rows = _rows(v)
    if v_ld != kv_ld:
        v = v.contiguous()
        k = k.contiguous()
        kv_ld = C
    if n_groups is None:
        if k_rows != v_rows or k_rows % B != 0:
            raise ValueError("k and v must have the same number of rows, a multiple of the batch")
        n_groups = B
        group_rows = k_rows // B
        M = group_rows
    if kv_rows is not None:
        if kv_rows.dtype != torch.int32:
            raise TypeError("kv_rows must be int32")
        kv_rows = kv_rows.contiguous()
        M = kv_rows.numel()
        limit = min(k_rows, v_rows)

        def run(kv_rows=kv_rows, limit=limit):
            lo, hi = int(kv_rows.min()), int(kv_rows.max())
            if lo < 0 or hi + (n_groups - 1) * group_rows >= limit:
                raise ValueError("kv_rows address rows %d..%d (+%d groups of %d) but k/v have %d rows"
                                 % (lo, hi, n_groups, group_rows, limit))
        _check_once(("rows", kv_rows.data_ptr(), M, kv_rows._version, n_groups, int(group_rows), limit), kv_rows, run)
    if kv_rows is None and ((n_groups - 1) * group_rows + M > min(k_rows, v_rows)):
        raise ValueError("k/v have %d/%d rows, grouping needs %d" % (k_rows, v_rows, (n_groups - 1) * group_rows + M))
    lib = _lib.load()
    ws_bytes = lib.fresco_attn_workspace_bytes(n_groups, heads, M, D)
    ws = (workspace or _default_ws).get(ws_bytes, q.device)
    out = torch.empty((B, Lq, C), dtype=q.dtype, device=q.device)
    rc = lib.fresco_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), _ptr(kv_rows), out.data_ptr(),
                             ws.data_ptr(), ws.numel(), B, heads, Lq, D, n_groups, M, group_rows,
                             float(scale), float(diag_bias), q_ld, kv_ld, _MFMA_DTYPES[q.dtype], _stream())
    _lib.check(rc, "fresco_attn_fwd(B=%d,H=%d,Lq=%d,D=%d,groups=%d,M=%d)" % (B, heads, Lq, D, n_groups, M))
    return out


def attention_kvproj_supported(heads, head_dim, in_features):
    return bool(_lib.load().fresco_attn_kvproj_supported(int(heads), int(head_dim), int(in_features)))


def attention_kvproj(q, hidden, x_rows, w_k, w_v, heads, scale, n_groups, M, workspace=None):
    """Cross-frame pass whose K | V projection of the selected rows is fused into the key pack (fresco_attn_fwd_kvproj).

    q (B, Lq, C) fp16; hidden (..., K_in) fp16 whose leading dims flatten to rows; x_rows int32 (n_groups * M): key m of
    group g = row x_rows[g * M + m] of `hidden` (in range: the caller's table, checked once where it is built);
    w_k, w_v (C, K_in) fp16 contiguous -- the live weights of bias-free nn.Linear modules.  Or all four bf16 (bf16 MFMA,
    K and V rounded to bf16 once, the bf16 flash kernels); a mix raises.  Returns (B, Lq, C) of q's dtype."""
    _need_gpu(q, hidden, x_rows, w_k, w_v)
    dt = q.dtype
    if dt not in _MFMA_DTYPES or any(t.dtype != dt for t in (hidden, w_k, w_v)) or x_rows.dtype != torch.int32:
        raise TypeError("fresco_amd.attention_kvproj: q, hidden, w_k, w_v all fp16 or all bf16 and an int32 row table "
                        "required (got %s/%s/%s/%s, %s)" % (q.dtype, hidden.dtype, w_k.dtype, w_v.dtype, x_rows.dtype))
    B, Lq, C = q.shape
    D = C // heads
    K_in = hidden.shape[-1]
    if w_k.shape != (C, K_in) or w_v.shape != (C, K_in) or not (w_k.is_contiguous() and w_v.is_contiguous()):
        raise ValueError("attention_kvproj: contiguous (%d, %d) weights expected" % (C, K_in))
    if x_rows.numel() != n_groups * M or not x_rows.is_contiguous():
        raise ValueError("attention_kvproj: x_rows must hold n_groups * M = %d entries" % (n_groups * M))
    q, q_ld, _ = _rows(q)
    hidden, x_ld, _ = _rows(hidden)
    lib = _lib.load()
    ws_bytes = lib.fresco_attn_workspace_bytes(n_groups, heads, M, D)
    ws = (workspace or _default_ws).get(ws_bytes, q.device)
    out = torch.empty((B, Lq, C), dtype=q.dtype, device=q.device)
    rc = lib.fresco_attn_fwd_kvproj(q.data_ptr(), hidden.data_ptr(), x_ld, x_rows.data_ptr(), w_k.data_ptr(),
                                    w_v.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), B, heads, Lq, D, n_groups,
                                    M, K_in, float(scale), q_ld, _MFMA_DTYPES[dt], _stream())
    _lib.check(rc, "fresco_attn_fwd_kvproj(B=%d,H=%d,Lq=%d,D=%d,groups=%d,M=%d,K=%d)" % (B, heads, Lq, D, n_groups, M, K_in))
    return out


def attention_f32(q, k, v, scale):
    """softmax(scale * q k^T) v at fp32 accuracy (fresco_attn_f32 with a flag): q (B,Lq,D), k (B,Lk,D), v (B,Lk,Dv) ->
    (B,Lq,Dv).  One head; batch entries are independent problems (windows).  When several 128-query workgroups share a
    key set (Lq >= 256) K and V are converted to the kernel's operand images once per launch, into a workspace taken from
    the caching allocator PER CALL (stream-safe: two streams running the flow network never share it; nothing is kept).
    No range limit: the split-fp16 kernels need |q scale log2 e|, |k|, |v| < 1000; a range pass on the device raises a
    flag otherwise and the exact-fp32 MFMA kernel recomputes the launch (no host sync either way)."""
    _need_gpu(q, k, v)
    q, k, v = _f32c(q), _f32c(k), _f32c(v)
    B, Lq, D = q.shape
    Lk, Dv = k.shape[1], v.shape[2]
    if k.shape != (B, Lk, D) or v.shape[:2] != (B, Lk):
        raise ValueError("attention_f32: q (B,Lq,D), k (B,Lk,D), v (B,Lk,Dv) expected")
    out = torch.empty(B, Lq, Dv, dtype=torch.float32, device=q.device)
    lib = _lib.load()
    need = lib.fresco_attn_f32_workspace_bytes(B, Lk, D, Dv) if Lq >= 256 else 0
    if need:
        # workspace form: the range tests ride in the split pass and the attention prologue; the flag is a word of a
        # zero-filled pool, handed out once (no memset, no range pass: 20 us of short launches per call)
        ws = torch.empty(need, dtype=torch.uint8, device=q.device)
        flag = _a32_zero_flag(q.device)
    else:
        ws = None
        fresh = torch.empty(1, dtype=torch.int32, device=q.device)  # (the call clears it and runs the range pass)
        flag = fresh.data_ptr()
    rc = lib.fresco_attn_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(ws), need, flag,
                             1 if need else 0, B, Lq, Lk, D, Dv, float(scale), _stream())
    _lib.check(rc, "fresco_attn_f32(B=%d,Lq=%d,Lk=%d,D=%d,Dv=%d)" % (B, Lq, Lk, D, Dv))
    return out


_A32_POOL_WORDS = 4096
_a32_pools = None  # a threading.local with a dict keyed by (device index, stream), made on first use


def _a32_zero_flag(device):
    """address of an int32 that is zero in the current stream's order and has never been handed out: word i of a pool that
    torch.zeros created ON THIS STREAM (one fill per 4096 calls).  A pool that runs out is dropped: its memory goes back to
    the caching allocator, which re-issues it in this stream's order (the kernels that still read its words come first).
    Under stream capture a word is handed out once per CAPTURE and read by every replay: a replay whose operands left the
    range leaves it set, and later replays of that graph take the exact-fp32 kernel as well (correct, slower) -- the flow
    network is not captured anywhere in this package."""
    global _a32_pools
    if _a32_pools is None:
        _a32_pools = _threading.local()
    pools = getattr(_a32_pools, "d", None)
    if pools is None:
        pools = _a32_pools.d = {}
    key = (device.index, _stream())
    ent = pools.get(key)
    if ent is None or ent[1] >= _A32_POOL_WORDS:
        ent = pools[key] = [torch.zeros(_A32_POOL_WORDS, dtype=torch.int32, device=device), 0]
    ptr = ent[0].data_ptr() + 4 * ent[1]
    ent[1] += 1
    return ptr


# ---- the flow network's dense layers (csrc/flownet.hip): fp32 tensors in NHWC / token layout, products on the fp16 matrix
# pipe from (hi, lo) fp16 planes.  A "split" below is a pair of fp16 tensors (M, ld) with x * scale = hi + lo (scale: FN_A_SCALE
# for activations, FN_W_SCALE for weights -- powers of two that keep the lo pieces normal fp16 numbers, csrc/flownet.hip).
FN_A_SCALE, FN_W_SCALE = 64.0, 1024.0
_fn_zero_page = {}  # per device: 128 bytes of zeros, the LDS-DMA source of rows outside a GEMM (padding, tails)

# Range guard of the split planes: |x * scale| beyond 65000 saturates -- finite, wrong.  Every producer ORs 1
# into the int32 word of the innermost `fn_range_guard` of the calling thread; whoever opened the guard reads the word once
# (one host sync per flow-network forward) and recomputes with library ops when it is set.
import threading as _threading

_fn_guard = _threading.local()


class fn_range_guard:
    """with fn_range_guard(device) as g: ... producers ...;  g.tripped() -> bool (synchronises)"""

    def __init__(self, device):
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)

    def __enter__(self):
        self._outer = getattr(_fn_guard, "cur", None)
        _fn_guard.cur = self
        return self

    def __exit__(self, *exc):
        _fn_guard.cur = self._outer
        return False

    def tripped(self):
        return bool(int(self.flag.item()) != 0)


def _fn_flag_ptr(device):
    g = getattr(_fn_guard, "cur", None)
    if g is None:
        return None
    if g.flag.device != device:
        raise ValueError("fn_range_guard on %s, operands on %s" % (g.flag.device, device))
    return g.flag.data_ptr()


def _fn_f32_operand(t, name, like):
    """optional fp32 side operand (bias, gamma, mean, residual ...) of a flownet.hip kernel: the kernels read raw fp32 words,
    so a .half() module or a strided view must not get through as it is"""
    if t is None:
        return None
    if not t.is_cuda or t.device != like.device:
        raise ValueError("fresco_amd: %s on %s, operands on %s" % (name, t.device, like.device))
    return _f32c(t)


def _fn_rows_table(t, name, like, n=None):
    if t is None:
        return None
    if t.dtype != torch.int32 or not t.is_contiguous() or t.device != like.device or (n is not None and t.numel() != n):
        raise ValueError("fresco_amd: %s must be a contiguous int32 table%s on the operands' device"
                         % (name, "" if n is None else " of %d rows" % n))
    return t


def fn_prep(x, mean=None, rstd=None, residual=None, rows_per_img=0, relu_a=False, relu_b=False, want_f32=False,
            want_split=True, ld=None, out_split=None, scale=FN_A_SCALE):
    """y = relu_b?(relu_a?((x - mean) * rstd) + residual) on (M, C) fp32 rows (fresco_fn_prep).  Returns (y or None,
    (hi, lo) or None); the planes have row stride ld >= C with channels C .. ld-1 zeroed.  out_split: planes to write into
    (views with a row stride are fine: (hi, lo, ld))."""
    _need_gpu(x)
    x = _f32c(x)
    M, C = x.shape
    mean, rstd, residual = (_fn_f32_operand(t, n_, x) for t, n_ in ((mean, "mean"), (rstd, "rstd"), (residual, "residual")))
    y = torch.empty_like(x) if want_f32 else None
    hi = lo = None
    ldo = C
    if out_split is not None:
        hi, lo, ldo = out_split
    elif want_split:
        ldo = ld or C
        hi, lo = _planes(M, ldo, x.device)
    rc = _lib.load().fresco_fn_prep(x.data_ptr(), _ptr(mean), _ptr(rstd), _ptr(residual), _ptr(y), _ptr(hi), _ptr(lo), M, C,
                                    int(ldo), int(rows_per_img), int(relu_a), int(relu_b), float(scale),
                                    _fn_flag_ptr(x.device), _stream())
    _lib.check(rc, "fresco_fn_prep(M=%d,C=%d,ld=%d)" % (M, C, ldo))
    return y, ((hi, lo) if hi is not None else None)


def fn_colstats(x, n_img, eps=1e-5):
    """InstanceNorm2d statistics of x (n_img * rows, C) fp32 -> (mean, rstd), (n_img, C) each (fresco_fn_colstats)"""
    _need_gpu(x)
    M, C = x.shape
    rows = M // n_img
    lib = _lib.load()
    nbytes = lib.fresco_fn_colstats_workspace_bytes(n_img, rows, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    mean = torch.empty(n_img, C, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n_img, C, dtype=torch.float32, device=x.device)
    rc = lib.fresco_fn_colstats(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), nbytes, n_img, rows, C,
                                float(eps), _stream())
    _lib.check(rc, "fresco_fn_colstats(n=%d,rows=%d,C=%d)" % (n_img, rows, C))
    return mean, rstd


def conv_out_size(H, W, kh, kw, stride, pad, dilation=1):
    """nn.Conv2d's output size (floor)"""
    return ((H + 2 * pad - dilation * (kh - 1) - 1) // stride + 1, (W + 2 * pad - dilation * (kw - 1) - 1) // stride + 1)


def fn_gemm(a, w, N, K, bias=None, act=0, conv=None, M=None, want_f32=True, want_split=False, out_split=None,
            instance_norm_eps=None, a_rows=None, out_rows=None, out_f32=None, out_blocks=0, a_scale=FN_A_SCALE,
            out_scale=FN_A_SCALE):
    """act(A W^T + bias) (fresco_fn_gemm).  a = (hi, lo) planes, (rows, lda); w = (hi, lo) planes (N, K).
    a_scale / out_scale: the power of two the planes of `a` were written with / the output planes are written with.
    conv = (n_img, H, W, kh, kw, stride, pad[, dilation = 1]): implicit im2col of the NHWC tensor behind `a` (K = kh kw cin).
    a_rows / out_rows (linear layers): int32 (M) tables -- problem row m reads input row a_rows[m], writes output row
    out_rows[m] (the rows of `out` not named by the table keep whatever they held: pass a full permutation).
    instance_norm_eps (convolutions): also return InstanceNorm2d statistics (mean, rstd) of the result, from partial sums
    the kernel's epilogue leaves behind (no second pass over the output).
    Returns (out fp32 (M, N) or None, (hi, lo) (M, N) or None[, (mean, rstd)])."""
    ah, al = a
    wh, wl = w
    _need_gpu(ah, wh)
    lda = ah.stride(0)
    if conv is None:
        M = (ah.shape[0] if a_rows is None else a_rows.numel()) if M is None else M
        cargs = (0, 0, 0, 0, 0, 1, 0, 1)
    else:
        if len(conv) not in (7, 8):
            raise ValueError("fn_gemm: conv = (n_img, H, W, kh, kw, stride, pad[, dilation]), got %r" % (conv,))
        n_img, H, W, kh, kw, stride, pad = conv[:7]
        dilation = int(conv[7]) if len(conv) == 8 else 1
        if dilation < 1:
            raise ValueError("fn_gemm: dilation %r" % (conv[7],))
        OH, OW = conv_out_size(H, W, kh, kw, stride, pad, dilation)
        M = n_img * OH * OW
        cargs = (n_img, H, W, kh, kw, stride, pad, dilation)
    dev = ah.device
    bias = _fn_f32_operand(bias, "bias", ah)
    a_rows = _fn_rows_table(a_rows, "a_rows", ah, M)
    out_rows = _fn_rows_table(out_rows, "out_rows", ah, M)
    # out_blocks = n > 1: W holds n stacked projections; the result is (n, M, N / n) fp32 -- every projection's rows contiguous
    ocb, obs, ldc = 0, 0, N
    if out_blocks and out_blocks > 1:
        if N % out_blocks or out_f32 is not None or want_split or out_split is not None or conv is not None:
            raise ValueError("fn_gemm: out_blocks needs a plain fp32 linear product whose N divides into the blocks")
        ocb = N // out_blocks
        out = torch.empty(out_blocks, M, ocb, dtype=torch.float32, device=dev)
        obs, ldc = M * ocb, ocb
    else:
        out = out_f32 if out_f32 is not None else (torch.empty(M, N, dtype=torch.float32, device=dev) if want_f32 else None)
    ldo = N
    if out_split is not None:
        oh, ol, ldo = out_split
    else:
        oh, ol = _planes(M, N, dev, want_split)
    stats = None
    fused = instance_norm_eps is not None and conv is not None and (M // conv[0]) % 256 == 0
    if fused:
        stats = torch.empty((M // 64) * N * 2, dtype=torch.float64, device=dev)
    zeros = _fn_zero_page.get(dev)
    if zeros is None:
        zeros = _fn_zero_page[dev] = torch.zeros(64, dtype=torch.float16, device=dev)
    lib = _lib.load()
    rc = lib.fresco_fn_gemm(ah.data_ptr(), al.data_ptr(), lda, wh.data_ptr(), wl.data_ptr(), _ptr(bias), _ptr(out),
                            _ptr(oh), _ptr(ol), int(ldc), int(ldo), M, N, K, int(act), 1.0 / (float(a_scale) * FN_W_SCALE),
                            float(out_scale), *cargs, _ptr(stats), zeros.data_ptr(), _ptr(a_rows), _ptr(out_rows),
                            _fn_flag_ptr(dev), int(ocb), int(obs), _stream())
    _lib.check(rc, "fresco_fn_gemm(M=%d,N=%d,K=%d,conv=%s)" % (M, N, K, conv))
    res = (out, ((oh, ol) if oh is not None else None))
    if instance_norm_eps is None:
        return res
    if not fused:
        return res + (fn_colstats(out, conv[0], instance_norm_eps),)
    mean = torch.empty(conv[0], N, dtype=torch.float32, device=dev)
    rstd = torch.empty(conv[0], N, dtype=torch.float32, device=dev)
    rc = lib.fresco_fn_colstats_finish(stats.data_ptr(), mean.data_ptr(), rstd.data_ptr(), conv[0], M // conv[0], N,
                                       float(instance_norm_eps), _stream())
    _lib.check(rc, "fresco_fn_colstats_finish")
    return res + ((mean, rstd),)


def fn_layernorm(x, gamma, beta, residual=None, eps=1e-5, want_f32=True, want_split=False, out_split=None):
    """residual + LayerNorm(x) over the 128 channels of (M, 128) fp32 rows (fresco_fn_layernorm) -> (y or None, split or None)"""
    _need_gpu(x)
    x = _f32c(x)
    M, C = x.shape
    gamma, beta, residual = (_fn_f32_operand(t, n_, x) for t, n_ in ((gamma, "gamma"), (beta, "beta"), (residual, "residual")))
    y = torch.empty_like(x) if want_f32 else None
    ldo = C
    if out_split is not None:
        oh, ol, ldo = out_split
    else:
        oh, ol = _planes(M, C, x.device, want_split)
    rc = _lib.load().fresco_fn_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(residual), _ptr(y), _ptr(oh),
                                         _ptr(ol), C, int(ldo), M, C, float(eps), FN_A_SCALE, _fn_flag_ptr(x.device),
                                         _stream())
    _lib.check(rc, "fresco_fn_layernorm(M=%d,C=%d)" % (M, C))
    return y, ((oh, ol) if oh is not None else None)


def fn_conv7_weight(weight):
    """(hi, lo) planes of the stem's weight as fresco_fn_conv7_rgb reads it: (64, 3, 7, 7) -> W'[cout][32 ky + 3 kx + ci],
    the 11 surplus positions of every kernel row zero"""
    w = weight.detach().float().permute(0, 2, 3, 1).reshape(64, 7, 21)
    w = torch.nn.functional.pad(w, (0, 11)).reshape(64, 224).contiguous()
    _, planes = fn_prep(w, scale=FN_W_SCALE)
    return planes


def fn_conv7_rgb(x_nhwc, w_split, instance_norm_eps=None):
    """Conv2d(3, 64, 7, stride 2, padding 3, bias=False) on (n, H, W, 3) fp32 NHWC, w_split = fn_conv7_weight(weight)
    -> (n, OH, OW, 64); instance_norm_eps: also the (mean, rstd) of the InstanceNorm2d that follows (partial sums out of
    the epilogue where the map allows it, a second pass otherwise)"""
    _need_gpu(x_nhwc, *w_split)
    x_nhwc = _f32c(x_nhwc)
    wh, wl = w_split
    if tuple(wh.shape) != (64, 224) or tuple(wl.shape) != (64, 224) or wh.dtype != torch.float16 or wl.dtype != torch.float16 \
            or not wh.is_contiguous() or not wl.is_contiguous():
        raise ValueError("fn_conv7_rgb: w_split must be the (64, 224) fp16 planes of fn_conv7_weight")
    n, H, W, c = x_nhwc.shape
    if c != 3:
        raise ValueError("fn_conv7_rgb: x must be (n, H, W, 3)")
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dev = x_nhwc.device
    out = torch.empty(n, OH, OW, 64, dtype=torch.float32, device=dev)
    fused = instance_norm_eps is not None and OW % 64 == 0 and (OH * OW) % 256 == 0
    stats = torch.empty((n * OH * OW // 64) * 64 * 2, dtype=torch.float64, device=dev) if fused else None
    lib = _lib.load()
    rc = lib.fresco_fn_conv7_rgb(x_nhwc.data_ptr(), wh.data_ptr(), wl.data_ptr(), out.data_ptr(), _ptr(stats), n, H, W,
                                 _fn_flag_ptr(dev), _stream())
    _lib.check(rc, "fresco_fn_conv7_rgb(n=%d,H=%d,W=%d)" % (n, H, W))
    if instance_norm_eps is None:
        return out
    if not fused:
        return out, fn_colstats(out.view(n * OH * OW, 64), n, instance_norm_eps)
    mean = torch.empty(n, 64, dtype=torch.float32, device=dev)
    rstd = torch.empty(n, 64, dtype=torch.float32, device=dev)
    rc = lib.fresco_fn_colstats_finish(stats.data_ptr(), mean.data_ptr(), rstd.data_ptr(), n, OH * OW, 64,
                                       float(instance_norm_eps), _stream())
    _lib.check(rc, "fresco_fn_colstats_finish")
    return out, (mean, rstd)


def fn_convex_upsample(logits, flow_tok, B, h, w):
    """convex upsampling by 8 (gmflow.py:75-90): logits (B h w, 576) fp32 rows of the mask head, flow_tok (B, h w, 2) ->
    (B, 2, 8 h, 8 w) (fresco_fn_convex_upsample)"""
    _need_gpu(logits, flow_tok)
    logits, flow_tok = _f32c(logits), _f32c(flow_tok)
    out = torch.empty(B, 2, 8 * h, 8 * w, dtype=torch.float32, device=logits.device)
    rc = _lib.load().fresco_fn_convex_upsample(logits.data_ptr(), flow_tok.data_ptr(), out.data_ptr(), B, h, w, _stream())
    _lib.check(rc, "fresco_fn_convex_upsample(B=%d,h=%d,w=%d)" % (B, h, w))
    return out


_checked_tables = {}


def _check_once(key, tensor, fn):
    """Run the (synchronising) validity check `fn` once per index table; the verdict is cached with the table
    (address, size, version; a weak reference guards against a recycled address)."""
    import weakref
    hit = _checked_tables.get(key)
    if hit is not None and hit() is tensor:
        return
    if len(_checked_tables) > 64:
        _checked_tables.clear()
    fn()
    _checked_tables[key] = weakref.ref(tensor)


def _check_permutations(owner, fwd_map, HW):
    """every row of fwd_map (N, HW) must be a permutation of 0..HW-1: the temporal kernel writes
    out[f][fwd_map[f][p]], so anything else leaves rows of the result unwritten (the reference's
    get_mapping_ind always produces permutations, src/flow_utils.py:99-101, 134-135).  `owner` is the tensor
    object the caller holds (the verdict is cached with IT: views made here are new objects every call)."""
    def run():
        srt = torch.sort(fwd_map, dim=1).values
        ok = bool((srt == torch.arange(HW, device=fwd_map.device, dtype=fwd_map.dtype)).all())
        if not ok:
            raise ValueError("fresco_amd.temporal_attention: fwd_mapping rows must be permutations of 0..%d" % (HW - 1))
    _check_once(("perm", owner.data_ptr(), tuple(owner.shape), owner._version), owner, run)


def _prep_fwd_map(fwd_map, N, HW):
    """the kernels read the row table as raw contiguous (N, HW) int64 words (N = -1: as many frames as it holds)"""
    fwd_map = fwd_map.reshape(N, HW)
    if fwd_map.dtype != torch.int64:
        fwd_map = fwd_map.to(torch.int64)
    return fwd_map.contiguous()


def _prep_maps(fwd_map, mask, N, HW):
    if fwd_map is not None:
        fwd_map = _prep_fwd_map(fwd_map, N, HW)
    mask = mask.reshape(-1, N, N)
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)
    elif mask.dtype != torch.uint8:
        mask = (mask != 0).contiguous().view(torch.uint8)
    return fwd_map, mask.contiguous()


def temporal_attention(q, k, v, fwd_map, mask, heads, scale, chunk):
    """fresco_temporal_attn: q, k, v (chunk*N, HW, C) all fp16 or all bf16; fwd_map (N,HW) int64 (a permutation per
    frame, checked once per table); mask (HW,N,N) bool."""
    _need_gpu(q, k, v, fwd_map, mask)
    if q.dtype not in _MFMA_DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError("fresco_amd.temporal_attention: q, k, v must all be fp16 or all bf16 (got %s/%s/%s)"
                        % (q.dtype, k.dtype, v.dtype))
    Bt, HW, C = q.shape
    N = Bt // chunk
    D = C // heads
    q, q_ld, _ = _rows(q)
    k, k_ld, _ = _rows(k)
    v, v_ld, _ = _rows(v)
    owner = fwd_map
    fwd_map, mask = _prep_maps(fwd_map, mask, N, HW)
    _check_permutations(owner, fwd_map, HW)
    out = torch.empty((Bt, HW, C), dtype=q.dtype, device=q.device)
    rc = _lib.load().fresco_temporal_attn(q.data_ptr(), k.data_ptr(), v.data_ptr(), fwd_map.data_ptr(),
                                          mask.data_ptr(), out.data_ptr(), chunk, N, HW, heads, D,
                                          float(scale), q_ld, k_ld, v_ld, _MFMA_DTYPES[q.dtype], _stream())
    _lib.check(rc, "fresco_temporal_attn(chunk=%d,N=%d,HW=%d,H=%d,D=%d)" % (chunk, N, HW, heads, D))
    return out


def temporal_pack(q, k, v, fwd_map, chunk, n_loc, f0, world):
    """Multi-GPU, way out (fresco_temporal_pack): this rank's frames [f0, f0+n_loc) of q, k, v (chunk*n_loc, HW, C)
    gathered along the trajectories into per-destination ranges: returns (world, n_loc, chunk, HW/world, 3C).  q, k, v
    all fp16 or all bf16 (the kernel copies 16-byte pieces: no arithmetic); the buffer is of their dtype."""
    _need_gpu(q, k, v, fwd_map)
    if q.dtype not in _MFMA_DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        raise TypeError("fresco_amd.temporal_pack: q, k, v must all be fp16 or all bf16 (got %s/%s/%s)"
                        % (q.dtype, k.dtype, v.dtype))
    Bl, HW, C = q.shape
    q, q_ld, _ = _rows(q)
    k, k_ld, _ = _rows(k)
    v, v_ld, _ = _rows(v)
    fwd_map = _prep_fwd_map(fwd_map, -1, HW)
    if fwd_map.shape[0] < f0 + n_loc:
        raise ValueError("fresco_amd.temporal_pack: fwd_map has %d frames, frames [%d, %d) asked for"
                         % (fwd_map.shape[0], f0, f0 + n_loc))
    buf = torch.empty((world, n_loc, chunk, HW // world, 3 * C), dtype=q.dtype, device=q.device)
    rc = _lib.load().fresco_temporal_pack(q.data_ptr(), k.data_ptr(), v.data_ptr(), fwd_map.data_ptr(), buf.data_ptr(),
                                          chunk, n_loc, f0, HW, C, world, q_ld, k_ld, v_ld, _stream())
    _lib.check(rc, "fresco_temporal_pack(chunk=%d,n_loc=%d,HW=%d,C=%d,world=%d)" % (chunk, n_loc, HW, C, world))
    return buf


def temporal_attention_packed(qkv, mask, heads, scale, chunk):
    """fresco_temporal_attn_packed: qkv (N, chunk, P, 3C) fp16 or bf16 = q | k | v rows already in trajectory order
    for a range of P trajectories, mask (P, N, N) for that range -> (N, chunk, P, C) of qkv's dtype."""
    _need_gpu(qkv, mask)
    N, ch, P, C3 = qkv.shape
    C = C3 // 3
    D = C // heads
    if ch != chunk or qkv.dtype not in _MFMA_DTYPES or not qkv.is_contiguous():
        raise ValueError("temporal_attention_packed: contiguous fp16 or bf16 (N, chunk, P, 3C) expected")
    _, mask = _prep_maps(None, mask, N, 1)
    if mask.shape[0] != P:
        raise ValueError("temporal_attention_packed: mask must cover the %d trajectories of the range" % P)
    out = torch.empty((N, chunk, P, C), dtype=qkv.dtype, device=qkv.device)
    rc = _lib.load().fresco_temporal_attn_packed(qkv.data_ptr(), mask.data_ptr(), out.data_ptr(), chunk, N, P, heads,
                                                 D, float(scale), _MFMA_DTYPES[qkv.dtype], _stream())
    _lib.check(rc, "fresco_temporal_attn_packed(chunk=%d,N=%d,P=%d,H=%d,D=%d)" % (chunk, N, P, heads, D))
    return out


def temporal_unpack(buf, fwd_map, chunk, n_loc, f0, world):
    """Multi-GPU, way back (fresco_temporal_unpack): buf (world, n_loc, chunk, HW/world, C) = this rank's frames'
    result rows per trajectory range -> (chunk*n_loc, HW, C) in frame order, fp16 or bf16 like buf (copies)."""
    _need_gpu(buf, fwd_map)
    if buf.dtype not in _MFMA_DTYPES:
        raise TypeError("fresco_amd.temporal_unpack: buf must be fp16 or bf16 (got %s)" % buf.dtype)
    w, nl, ch, Pw, C = buf.shape
    HW = Pw * world
    fwd_map = _prep_fwd_map(fwd_map, -1, HW)
    if fwd_map.shape[0] < f0 + n_loc:
        raise ValueError("fresco_amd.temporal_unpack: fwd_map has %d frames, frames [%d, %d) asked for"
                         % (fwd_map.shape[0], f0, f0 + n_loc))
    out = torch.empty((chunk * n_loc, HW, C), dtype=buf.dtype, device=buf.device)
    rc = _lib.load().fresco_temporal_unpack(buf.contiguous().data_ptr(), fwd_map.data_ptr(), out.data_ptr(), chunk,
                                            n_loc, f0, HW, C, world, _stream())
    _lib.check(rc, "fresco_temporal_unpack(chunk=%d,n_loc=%d,HW=%d,C=%d,world=%d)" % (chunk, n_loc, HW, C, world))
    return out


# ---------------------------------------------------------------------------------------------
# warp family (fp32)
# ---------------------------------------------------------------------------------------------
def flow_warp(x, flow):
    """(B,C,h,w) fp32 sampled at pixel + flow[b % Bf] (bilinear, zeros, align_corners=True)."""
    _need_gpu(x, flow)
    x, flow = _f32c(x), _f32c(flow)
    B, C, h, w = x.shape
    Bf = flow.shape[0]
    if flow.shape[1:] != (2, h, w) or B % Bf != 0:
        raise ValueError("flow %s does not match feature %s" % (tuple(flow.shape), tuple(x.shape)))
    out = torch.empty_like(x)
    rc = _lib.load().fresco_flow_warp(x.data_ptr(), flow.data_ptr(), out.data_ptr(), B, C, h, w, Bf, _stream())
    _lib.check(rc, "fresco_flow_warp")
    return out


def resize_bilinear(x, scale_factor, mul=1.0):
    """F.interpolate(x * mul, scale_factor=s, mode='bilinear') for (B,C,H,W)."""
    _need_gpu(x)
    x = _f32c(x)
    B, C, H, W = x.shape
    ho, wo = int(math.floor(H * scale_factor)), int(math.floor(W * scale_factor))
    if ho <= 0 or wo <= 0:
        raise ValueError("resize to empty output")
    out = torch.empty(B, C, ho, wo, dtype=torch.float32, device=x.device)
    r = 1.0 / scale_factor
    rc = _lib.load().fresco_resize_bilinear(x.data_ptr(), out.data_ptr(), B * C, H, W, ho, wo, r, r,
                                            float(mul), _stream())
    _lib.check(rc, "fresco_resize_bilinear")
    return out


def max_pool(x, k):
    """F.max_pool2d(x, kernel_size=k) for (B,C,H,W)."""
    _need_gpu(x)
    x = _f32c(x)
    B, C, H, W = x.shape
    out = torch.empty(B, C, H // k, W // k, dtype=torch.float32, device=x.device)
    rc = _lib.load().fresco_max_pool(x.data_ptr(), out.data_ptr(), B * C, H, W, k, _stream())
    _lib.check(rc, "fresco_max_pool")
    return out


def dilate(x, k):
    _need_gpu(x)
    x = _f32c(x)
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    rc = _lib.load().fresco_dilate(x.data_ptr(), out.data_ptr(), B * C, H, W, k, _stream())
    _lib.check(rc, "fresco_dilate")
    return out


def flow_occlusion(fwd_flow, bwd_flow, images=None, alpha=0.01, beta=0.5, color_thr=255 * 0.25):
    """(fwd_occ, bwd_occ) fp32 (N,H,W) for the frame pairs (n, n+1 mod N); images (N,C,H,W) in 0..255 adds
    the colour-difference test, None = forward_backward_consistency_check alone."""
    _need_gpu(fwd_flow)
    fwd_flow, bwd_flow = _f32c(fwd_flow), _f32c(bwd_flow)
    N, two, H, W = fwd_flow.shape
    if two != 2 or bwd_flow.shape != fwd_flow.shape:
        raise ValueError("flows must be (N,2,H,W) and of equal shape")
    C, ip = 0, None
    if images is not None:
        images = _f32c(images)
        if images.shape[0] != N or tuple(images.shape[2:]) != (H, W):
            raise ValueError("images must be (N,C,H,W) matching the flows")
        C, ip = images.shape[1], images.data_ptr()
    fo = torch.empty(N, H, W, dtype=torch.float32, device=fwd_flow.device)
    bo = torch.empty_like(fo)
    rc = _lib.load().fresco_flow_occlusion(ip, fwd_flow.data_ptr(), bwd_flow.data_ptr(), fo.data_ptr(), bo.data_ptr(),
                                           N, C, H, W, alpha, beta, color_thr, _stream())
    _lib.check(rc, "fresco_flow_occlusion")
    return fo, bo


def warp_fuse_chain(lat, bwd_flow, fwd_flow, bwd_occ, fwd_occ, sal, warp_sal, warp_sal_last, chunk):
    """In-place frame chain of warp_tensor on lat (chunk*N, C, h, w) fp32 contiguous."""
    _need_gpu(lat)
    assert lat.dtype == torch.float32 and lat.is_contiguous()
    Bt, C, h, w = lat.shape
    N = Bt // chunk
    args = [_f32c(t) for t in (bwd_flow, fwd_flow, bwd_occ, fwd_occ, sal, warp_sal, warp_sal_last)]
    rc = _lib.load().fresco_warp_fuse_chain(lat.data_ptr(), *[t.data_ptr() for t in args], chunk, N, C, h, w,
                                            _stream())
    _lib.check(rc, "fresco_warp_fuse_chain(N=%d)" % N)
    return lat


# storage types of the elementwise / reduction kernels that carry a dtype code (fp32 arithmetic inside, one rounding at the store)
_ELEMWISE_DTYPES = {torch.float16: _lib.F16, torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def adain(content, style, eps_content=1e-5, eps_style=1.0):
    _need_gpu(content, style)
    if content.shape != style.shape:
        raise ValueError("AdaIN: content %s vs style %s" % (tuple(content.shape), tuple(style.shape)))
    dt = torch.result_type(content, style)
    if dt not in _ELEMWISE_DTYPES:
        dt = torch.float32
    c, s = content.to(dt).contiguous(), style.to(dt).contiguous()
    rows = c.shape[0] * c.shape[1]
    L = c.numel() // rows
    out = torch.empty_like(c)
    rc = _lib.load().fresco_adain(c.data_ptr(), s.data_ptr(), out.data_ptr(), rows, L, float(eps_content),
                                  float(eps_style), _ELEMWISE_DTYPES[dt], _stream())
    _lib.check(rc, "fresco_adain")
    return out


def chan_mean_std(feat, eps=1e-5):
    """-> (mean, std) fp32 of shape (N*C,): per-plane mean and sqrt(unbiased variance + eps)  (src/utils.py:58-67)."""
    _need_gpu(feat)
    dt = feat.dtype if feat.dtype in _ELEMWISE_DTYPES else torch.float32
    x = feat.to(dt).contiguous()
    rows = x.shape[0] * x.shape[1]
    L = x.numel() // rows
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    std = torch.empty(rows, dtype=torch.float32, device=x.device)
    rc = _lib.load().fresco_chan_mean_std(x.data_ptr(), mean.data_ptr(), std.data_ptr(), rows, L, float(eps),
                                          _ELEMWISE_DTYPES[dt], _stream())
    _lib.check(rc, "fresco_chan_mean_std")
    return mean, std


# ---------------------------------------------------------------------------------------------
# FreeU (src/free_lunch_utils.py): closed-form skip filter and backbone scaling at the up-block sites
# ---------------------------------------------------------------------------------------------
def _freeu_dense_nchw(t, name):
    """(batch stride in elements) of a 4-D tensor whose samples are dense (C, H, W) blocks: a contiguous tensor or a
    channel slice of one (the tail of a concat buffer)."""
    B, C, H, W = t.shape
    if t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W or (B > 1 and t.stride(0) < C * H * W):
        raise ValueError("%s: samples must be dense (C, H, W) blocks, got strides %s" % (name, tuple(t.stride())))
    return t.stride(0) if B > 1 else C * H * W


def freeu_fourier(x, scale, out=None):
    """Fourier_filter(x, threshold=1, scale) (free_lunch_utils.py:25-52) in closed form; x (B, C, H, W) fp16 / bf16 / fp32.
    out: a (B, C, H, W) tensor of the same dtype with dense samples (e.g. buf[:, C0:] of a concat buffer); default a new
    tensor.  scale == 1 copies."""
    _need_gpu(x, out)
    if x.dim() != 4:
        raise ValueError("freeu_fourier: expected (B, C, H, W), got %s" % (tuple(x.shape),))
    if x.dtype not in _ELEMWISE_DTYPES:
        raise ValueError("freeu_fourier: dtype %s (fp16, bf16 or fp32)" % x.dtype)
    x = x.contiguous()
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device:
        raise ValueError("freeu_fourier: out %s %s vs x %s %s" % (tuple(out.shape), out.dtype, tuple(x.shape), x.dtype))
    if x.numel() == 0:
        return out
    rc = _lib.load().fresco_freeu_fourier(x.data_ptr(), out.data_ptr(), _freeu_dense_nchw(out, "freeu_fourier: out"), B, C,
                                          H, W, float(scale), _ELEMWISE_DTYPES[x.dtype], _stream())
    _lib.check(rc, "fresco_freeu_fourier")
    return out


def freeu_backbone(hidden, n_scaled, b, cat=None, workspace=None):
    """hidden[:, :n_scaled] *= (b - 1) * normalised channel mean + 1, IN PLACE (free_lunch_utils.py:130-135); hidden must
    be contiguous (B, C, H, W) fp16 / bf16 / fp32.  cat: a tensor of the same dtype whose first C channels receive hidden
    after the update (dense samples of >= C channels)."""
    _need_gpu(hidden, cat)
    if hidden.dim() != 4 or not hidden.is_contiguous():
        raise ValueError("freeu_backbone: hidden must be a contiguous (B, C, H, W) tensor")
    if hidden.dtype not in _ELEMWISE_DTYPES:
        raise ValueError("freeu_backbone: dtype %s (fp16, bf16 or fp32)" % hidden.dtype)
    B, C, H, W = hidden.shape
    cat_bs = 0
    if cat is not None:
        if (cat.dim() != 4 or cat.dtype != hidden.dtype or cat.device != hidden.device or cat.shape[0] != B
                or cat.shape[1] < C or tuple(cat.shape[2:]) != (H, W)):
            raise ValueError("freeu_backbone: cat %s %s vs hidden %s %s" % (tuple(cat.shape), cat.dtype,
                                                                          tuple(hidden.shape), hidden.dtype))
        cat_bs = _freeu_dense_nchw(cat, "freeu_backbone: cat")
    if hidden.numel() == 0:
        return hidden
    lib = _lib.load()
    nbytes = lib.fresco_freeu_workspace_bytes(B, C, H, W)
    ws = (workspace or _default_ws).get(nbytes, hidden.device)
    rc = lib.fresco_freeu_backbone(hidden.data_ptr(), _ptr(cat), cat_bs, B, C, int(n_scaled), H, W, float(b),
                                   ws.data_ptr(), ws.numel(), _ELEMWISE_DTYPES[hidden.dtype], _stream())
    _lib.check(rc, "fresco_freeu_backbone")
    return hidden


def freeu_site(hidden, skip, n_scaled, b, s, workspace=None):
    """One FreeU site (free_lunch_utils.py:127-149): scales hidden[:, :n_scaled] in place, filters skip, and returns
    cat([hidden, filtered skip], dim=1) -- two library calls that write straight into the concat tensor."""
    _need_gpu(hidden, skip)
    B, C, H, W = hidden.shape
    if skip.dim() != 4 or skip.shape[0] != B or tuple(skip.shape[2:]) != (H, W) or skip.dtype != hidden.dtype:
        raise ValueError("freeu_site: skip %s %s vs hidden %s %s" % (tuple(skip.shape), skip.dtype, tuple(hidden.shape),
                                                                    hidden.dtype))
    cat = torch.empty((B, C + skip.shape[1], H, W), dtype=hidden.dtype, device=hidden.device)
    freeu_backbone(hidden, n_scaled, b, cat=cat, workspace=workspace)
    if skip.shape[1]:
        freeu_fourier(skip, s, out=cat[:, C:])
    return cat


# ---------------------------------------------------------------------------------------------
# HED annotator (src/ControlNet/annotator/hed/__init__.py): the pieces around the fn_gemm convolutions (csrc/hed.hip)
# ---------------------------------------------------------------------------------------------
HED_CHANNELS = (64, 128, 256, 512)


def hed_input(frames, norm, scale=FN_A_SCALE):
    """frames (n, H, W, 3) uint8 RGB, norm 3 fp32 values on the device -> (hi, lo) planes (n H W, 32) of
    (frames - norm) * scale, channels 3..31 zero (fresco_hed_input)"""
    _dense(frames, "hed_input: frames", torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("hed_input: frames must be (n, H, W, 3), got %s" % (tuple(frames.shape),))
    norm = _dense(norm, "hed_input: norm", torch.float32)
    if norm.numel() != 3 or norm.device != frames.device:
        raise ValueError("hed_input: norm must hold 3 values on the frames' device")
    scale = _split_scale(scale)
    _need_gpu(frames)
    n, H, W, _ = frames.shape
    hi, lo = _planes(n * H * W, 32, frames.device)
    rc = _lib.load().fresco_hed_input(frames.data_ptr(), norm.data_ptr(), hi.data_ptr(), lo.data_ptr(), n, H, W, scale,
                                      _fn_flag_ptr(frames.device), _stream())
    _lib.check(rc, "fresco_hed_input(n=%d,H=%d,W=%d)" % (n, H, W))
    return hi, lo


def hed_side_pool(h, n, H, W, weight, bias=None, want_proj=True, want_pool=True, scale=FN_A_SCALE):
    """h (n H W, C) fp32 NHWC rows (post-ReLU), weight (C) / bias (1) of the block's 1 x 1 projection -> (proj (n, H, W)
    fp32 or None, (hi, lo) planes (n (H//2) (W//2), C) of max_pool2d(h, 2, 2) * scale or None) (fresco_hed_side_pool)"""
    _dense(h, "hed_side_pool: h", torch.float32, align=16)
    if h.dim() != 2 or h.shape[0] != n * H * W or n <= 0 or H <= 0 or W <= 0:
        raise ValueError("hed_side_pool: h %s is not (n H W, C) rows for n, H, W = %d, %d, %d" % (tuple(h.shape), n, H, W))
    C = h.shape[1]
    if C not in HED_CHANNELS:
        raise ValueError("hed_side_pool: C = %d (built for %s)" % (C, HED_CHANNELS))
    if not (want_proj or want_pool):
        raise ValueError("hed_side_pool: nothing asked for")
    if want_pool and (H < 2 or W < 2):
        raise ValueError("hed_side_pool: a %d x %d map has no pooled pixel" % (H, W))
    weight = _dense(weight, "hed_side_pool: weight", torch.float32, align=16)
    if weight.numel() != C or weight.device != h.device:
        raise ValueError("hed_side_pool: weight must hold C = %d values on h's device" % C)
    if bias is not None:
        bias = _dense(bias, "hed_side_pool: bias", torch.float32)
        if bias.numel() != 1 or bias.device != h.device:
            raise ValueError("hed_side_pool: bias must hold one value on h's device")
    scale = _split_scale(scale)
    _need_gpu(h)
    proj = torch.empty(n, H, W, dtype=torch.float32, device=h.device) if want_proj else None
    hi, lo = _planes(n * (H // 2) * (W // 2), C, h.device, want_pool)
    rc = _lib.load().fresco_hed_side_pool(h.data_ptr(), weight.data_ptr(), _ptr(bias), _ptr(proj), _ptr(hi), _ptr(lo), n, H,
                                          W, C, scale, _fn_flag_ptr(h.device), _stream())
    _lib.check(rc, "fresco_hed_side_pool(n=%d,H=%d,W=%d,C=%d)" % (n, H, W, C))
    return proj, ((hi, lo) if want_pool else None)


def hed_level_sizes(H, W):
    """the five block resolutions of an (H, W) frame: halved with floor four times"""
    return [(H >> k, W >> k) for k in range(5)]


def hed_fuse(sides, want_logit=False, cond_dtype=None):
    """five side maps, level k (n, H >> k, W >> k) fp32 -> (edge map (n, H, W) uint8, fused logit (n, H, W) fp32 or None,
    ControlNet condition (n, 3, H, W) of cond_dtype or None) (fresco_hed_fuse)"""
    if len(sides) != 5:
        raise ValueError("hed_fuse: five side maps, got %d" % len(sides))
    s0 = _dense(sides[0], "hed_fuse: side 1", torch.float32)
    if s0.dim() != 3 or s0.numel() == 0:
        raise ValueError("hed_fuse: side maps are (n, h, w), got %s" % (tuple(s0.shape),))
    n, H, W = s0.shape
    if H < 16 or W < 16:
        raise ValueError("hed_fuse: frames of at least 16 x 16 (level 5 is the size halved four times), got %d x %d" % (H, W))
    for k, (hk, wk) in enumerate(hed_level_sizes(H, W)):
        _dense(sides[k], "hed_fuse: side %d" % (k + 1), torch.float32, (n, hk, wk))
        if sides[k].device != s0.device:
            raise ValueError("hed_fuse: side maps on different devices")
    if cond_dtype is not None and cond_dtype not in _ELEMWISE_DTYPES:
        raise TypeError("hed_fuse: cond_dtype %s (fp16, bf16 or fp32)" % (cond_dtype,))
    _need_gpu(s0)
    out = torch.empty(n, H, W, dtype=torch.uint8, device=s0.device)
    logit = torch.empty(n, H, W, dtype=torch.float32, device=s0.device) if want_logit else None
    cond = torch.empty(n, 3, H, W, dtype=cond_dtype, device=s0.device) if cond_dtype is not None else None
    rc = _lib.load().fresco_hed_fuse(*[t.data_ptr() for t in sides], out.data_ptr(), _ptr(logit), _ptr(cond),
                                     _ELEMWISE_DTYPES.get(cond_dtype, _lib.F32), n, H, W, _stream())
    _lib.check(rc, "fresco_hed_fuse(n=%d,H=%d,W=%d)" % (n, H, W))
    return out, logit, cond


# ---------------------------------------------------------------------------------------------
# EGNet saliency detector (src/EGNet/model.py, src/utils.py::get_saliency): the pieces around the fn_gemm convolutions
# (csrc/egnet.hip)
# ---------------------------------------------------------------------------------------------
EGNET_MAX_K = 15


def egnet_input(frames):
    """frames (n, H, W, 3) uint8 -> cv2sod's tensor as (n, H // 2, W // 2, 3) fp32 NHWC: channel means subtracted, each
    2 x 2 block averaged (fresco_egnet_input)"""
    _dense(frames, "egnet_input: frames", torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0 or frames.shape[1] < 2 or frames.shape[2] < 2:
        raise ValueError("egnet_input: frames must be (n, H >= 2, W >= 2, 3), got %s" % (tuple(frames.shape),))
    _need_gpu(frames)
    n, H, W, _ = frames.shape
    out = torch.empty(n, H // 2, W // 2, 3, dtype=torch.float32, device=frames.device)
    rc = _lib.load().fresco_egnet_input(frames.data_ptr(), out.data_ptr(), n, H, W, _stream())
    _lib.check(rc, "fresco_egnet_input(n=%d,H=%d,W=%d)" % (n, H, W))
    return out


def egnet_pool_size(size):
    """MaxPool2d(3, stride 2, padding 1, ceil_mode=True): the output size of one axis (PyTorch's rule: the last window
    starts inside the input or its left padding)"""
    o = (size + 2 - 3 + 1) // 2 + 1
    return o - 1 if (o - 1) * 2 >= size + 1 else o


def egnet_pool(x, want_f32=False, scale=FN_A_SCALE):
    """x (n, H, W, 64) fp32 NHWC -> (pooled fp32 (n, OH, OW, 64) or None, (hi, lo) planes (n OH OW, 64)) of
    MaxPool2d(3, 2, 1, ceil_mode=True) (fresco_egnet_pool)"""
    _dense(x, "egnet_pool: x", torch.float32, align=16)
    if x.dim() != 4 or x.shape[3] != 64 or x.numel() == 0:
        raise ValueError("egnet_pool: x must be (n, H, W, 64), got %s" % (tuple(x.shape),))
    scale = _split_scale(scale)
    _need_gpu(x)
    n, H, W, C = x.shape
    OH, OW = egnet_pool_size(H), egnet_pool_size(W)
    out = torch.empty(n, OH, OW, C, dtype=torch.float32, device=x.device) if want_f32 else None
    hi, lo = _planes(n * OH * OW, C, x.device)
    rc = _lib.load().fresco_egnet_pool(x.data_ptr(), _ptr(out), hi.data_ptr(), lo.data_ptr(), n, H, W, C, scale,
                                       _fn_flag_ptr(x.device), _stream())
    _lib.check(rc, "fresco_egnet_pool(n=%d,H=%d,W=%d,C=%d)" % (n, H, W, C))
    return out, (hi, lo)


def egnet_resize_add(x, size, addend=None, relu=False, want_f32=True, want_split=False, scale=FN_A_SCALE):
    """[relu](F.interpolate(x, size, bilinear, align_corners=True) [+ addend]) on NHWC fp32: x (n, h, w, C), addend
    (n, H, W, C) -> (fp32 (n, H, W, C) or None, (hi, lo) planes (n H W, C) or None) (fresco_egnet_resize_add)"""
    _dense(x, "egnet_resize_add: x", torch.float32, align=16)
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("egnet_resize_add: x must be (n, h, w, C), got %s" % (tuple(x.shape),))
    n, h, w, C = x.shape
    H, W = int(size[0]), int(size[1])
    if H <= 0 or W <= 0:
        raise ValueError("egnet_resize_add: size %r" % (size,))
    if C % 32 or C > 512:
        raise ValueError("egnet_resize_add: C = %d (a multiple of 32 up to 512)" % C)
    if addend is not None:
        _dense(addend, "egnet_resize_add: addend", torch.float32, (n, H, W, C), align=16)
        if addend.device != x.device:
            raise ValueError("egnet_resize_add: addend on another device")
    if not (want_f32 or want_split):
        raise ValueError("egnet_resize_add: nothing asked for")
    scale = _split_scale(scale)
    _need_gpu(x)
    out = torch.empty(n, H, W, C, dtype=torch.float32, device=x.device) if want_f32 else None
    hi, lo = _planes(n * H * W, C, x.device, want_split)
    rc = _lib.load().fresco_egnet_resize_add(x.data_ptr(), _ptr(addend), _ptr(out), _ptr(hi), _ptr(lo), n, h, w, H, W, C,
                                             int(bool(relu)), scale, _fn_flag_ptr(x.device), _stream())
    _lib.check(rc, "fresco_egnet_resize_add(n=%d,%dx%d->%dx%d,C=%d)" % (n, h, w, H, W, C))
    return out, ((hi, lo) if want_split else None)


def egnet_saliency(logit, size, k=7, want_logit=False):
    """logit (n, h, w) fp32 -> (1 - clamp(box_k(sigmoid(resize(logit, size))), 0, 1) as (n, 1, Hs, Ws) fp32, the resized logit
    (n, Hs, Ws) or None): align_corners=True resize, k x k box sum with replicate padding (fresco_egnet_saliency)"""
    _dense(logit, "egnet_saliency: logit", torch.float32)
    if logit.dim() != 3 or logit.numel() == 0:
        raise ValueError("egnet_saliency: logit must be (n, h, w), got %s" % (tuple(logit.shape),))
    Hs, Ws, k = int(size[0]), int(size[1]), int(k)
    if Hs <= 0 or Ws <= 0:
        raise ValueError("egnet_saliency: size %r" % (size,))
    if k < 1 or k % 2 == 0 or k > EGNET_MAX_K:
        raise ValueError("egnet_saliency: k = %d (odd, at most %d)" % (k, EGNET_MAX_K))
    _need_gpu(logit)
    n, h, w = logit.shape
    out = torch.empty(n, 1, Hs, Ws, dtype=torch.float32, device=logit.device)
    lg = torch.empty(n, Hs, Ws, dtype=torch.float32, device=logit.device) if want_logit else None
    rc = _lib.load().fresco_egnet_saliency(logit.data_ptr(), out.data_ptr(), _ptr(lg), n, h, w, Hs, Ws, k, _stream())
    _lib.check(rc, "fresco_egnet_saliency(n=%d,%dx%d->%dx%d,k=%d)" % (n, h, w, Hs, Ws, k))
    return out, lg


# ---------------------------------------------------------------------------------------------
# Canny edge detector (src/ControlNet/annotator/canny: cv2.Canny per frame) (csrc/canny.hip)
# ---------------------------------------------------------------------------------------------
def canny_classify(frames, low, high):
    """frames (n, H, W, 3) uint8 RGB -> the class map (n, H, W) uint8 of OpenCV's Canny at aperture 3 with the L1 magnitude:
    0 no edge, 1 weak (a local maximum above `low`), 2 strong (above `high` too); integer thresholds, low > high swapped
    (fresco_canny_classify)"""
    _dense(frames, "canny_classify: frames", torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("canny_classify: frames must be (n, H, W, 3), got %s" % (tuple(frames.shape),))
    low, high = int(low), int(high)
    _need_gpu(frames)
    n, H, W, _ = frames.shape
    cls = torch.empty(n, H, W, dtype=torch.uint8, device=frames.device)
    rc = _lib.load().fresco_canny_classify(frames.data_ptr(), cls.data_ptr(), n, H, W, low, high, _stream())
    _lib.check(rc, "fresco_canny_classify(n=%d,H=%d,W=%d)" % (n, H, W))
    return cls


def canny_hysteresis(cls, cond_dtype=None):
    """class map (n, H, W) uint8 -> (edge map (n, H, W) uint8: 255 on the weak and strong pixels of every 8-connected
    component that holds a strong one, ControlNet condition (n, 3, H, W) of cond_dtype or None) (fresco_canny_hysteresis)"""
    _dense(cls, "canny_hysteresis: cls", torch.uint8)
    if cls.dim() != 3 or cls.numel() == 0:
        raise ValueError("canny_hysteresis: the class map is (n, H, W), got %s" % (tuple(cls.shape),))
    if cond_dtype is not None and cond_dtype not in _ELEMWISE_DTYPES:
        raise TypeError("canny_hysteresis: cond_dtype %s (fp16, bf16 or fp32)" % (cond_dtype,))
    _need_gpu(cls)
    n, H, W = cls.shape
    lib = _lib.load()
    need = lib.fresco_canny_workspace_bytes(n, H, W)
    if need == 0:
        raise FrescoHipError("canny_hysteresis: n H W = %d x %d x %d is beyond what the kernels index (2^31)" % (n, H, W))
    ws = torch.empty(need, dtype=torch.uint8, device=cls.device)
    out = torch.empty(n, H, W, dtype=torch.uint8, device=cls.device)
    cond = torch.empty(n, 3, H, W, dtype=cond_dtype, device=cls.device) if cond_dtype is not None else None
    rc = lib.fresco_canny_hysteresis(cls.data_ptr(), out.data_ptr(), _ptr(cond), _ELEMWISE_DTYPES.get(cond_dtype, _lib.F32),
                                     ws.data_ptr(), need, n, H, W, _stream())
    _lib.check(rc, "fresco_canny_hysteresis(n=%d,H=%d,W=%d)" % (n, H, W))
    return out, cond


# ---------------------------------------------------------------------------------------------
# key-frame selection (src/keyframe_selection.py: resize_image, cv2.GaussianBlur, mse_loss per frame) (csrc/keyframe.hip)
# ---------------------------------------------------------------------------------------------
def _u8_frames(frames, name):
    _dense(frames, name, torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("%s must be (n, H, W, 3), got %s" % (name, tuple(frames.shape)))
    return frames


def _cached_table(cache, cache_max, key, what, nbytes, build, args, device):
    """the int32 table the library builds on the host for `args` (nbytes(*args) sizes it, build(*args, buffer, bytes) fills
    it), uploaded once per `key` and kept in `cache`, the oldest entry going first beyond cache_max"""
    tab = cache.get(key)
    if tab is None:
        need = nbytes(*args)
        if need == 0:  # the geometry is refused: let the call say why
            _lib.check(build(*args, None, 0), what)
            raise FrescoHipError("%s: no table for this geometry" % what)
        host = (ctypes.c_int32 * (need // 4))()
        _lib.check(build(*args, ctypes.addressof(host), need), what)
        tab = torch.frombuffer(host, dtype=torch.int32).to(device)  # (a blocking copy: `host` may go afterwards)
        while len(cache) >= cache_max:
            cache.pop(next(iter(cache)))
        cache[key] = tab
    return tab


_AREA_TABLES = {}      # (H0, W0, H, W, device) -> the coverage tables of the geometry on that device, int32 words
_AREA_TABLES_MAX = 32  # geometries kept; the oldest goes first


def _area_table(H0, W0, H, W, device):
    """the two coverage tables of INTER_AREA for one geometry: built on the host by the library (keyframe_resize_table),
    uploaded once and kept; the kernel walks them in their order"""
    lib = _lib.load()
    return _cached_table(_AREA_TABLES, _AREA_TABLES_MAX, (H0, W0, H, W, str(device)),
                         "keyframe_resize_table(%dx%d->%dx%d)" % (H0, W0, H, W), lib.keyframe_resize_table_bytes,
                         lib.keyframe_resize_table, (H0, W0, H, W), device)


def resize_area_u8(frames, H, W):
    """frames (n, H0, W0, 3) uint8 -> (n, H, W, 3) uint8: OpenCV's INTER_AREA where no side is enlarged; a side that would
    be is refused (keyframe_resize_area_u8)"""
    _u8_frames(frames, "resize_area_u8: frames")
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError("resize_area_u8: the size %d x %d is not positive" % (H, W))
    _need_gpu(frames)
    n, H0, W0, _ = frames.shape
    tab = _area_table(H0, W0, H, W, frames.device)
    out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=frames.device)
    rc = _lib.load().keyframe_resize_area_u8(frames.data_ptr(), out.data_ptr(), tab.data_ptr(), tab.numel() * 4, n, H0, W0, H,
                                             W, _stream())
    _lib.check(rc, "keyframe_resize_area_u8(n=%d,%dx%d->%dx%d)" % (n, H0, W0, H, W))
    return out


RESIZE_LANCZOS4, RESIZE_LINEAR_AREA = _lib.RESIZE_LANCZOS4, _lib.RESIZE_LINEAR_AREA
_TAP_TABLES = {}      # (H0, W0, H, W, method, device) -> the tap table of the geometry on that device, int32 words
_TAP_TABLES_MAX = 32  # geometries kept; the oldest goes first


def _tap_table(H0, W0, H, W, method, device):
    """the tap table of one geometry and method (per axis and output index the first source index and the 8 or 2 fixed-point
    coefficients): built on the host by the library (frame_resize_table), uploaded once and kept"""
    lib = _lib.load()
    return _cached_table(_TAP_TABLES, _TAP_TABLES_MAX, (H0, W0, H, W, method, str(device)),
                         "frame_resize_table(%dx%d->%dx%d, method %d)" % (H0, W0, H, W, method), lib.frame_resize_table_bytes,
                         lib.frame_resize_table, (H0, W0, H, W, method), device)


def resize_taps_u8(frames, H, W, method):
    """frames (n, H0, W0, 3) uint8 -> (n, H, W, 3) uint8 through OpenCV's fixed-point tap resizes: method RESIZE_LANCZOS4 is
    cv2.INTER_LANCZOS4, RESIZE_LINEAR_AREA what cv2.INTER_AREA does when a side is enlarged.  A side that shrinks by more
    than a factor 2 is refused (frame_resize_u8)"""
    _u8_frames(frames, "resize_taps_u8: frames")
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError("resize_taps_u8: the size %d x %d is not positive" % (H, W))
    if method not in (RESIZE_LANCZOS4, RESIZE_LINEAR_AREA):
        raise ValueError("resize_taps_u8: method %r (RESIZE_LANCZOS4 or RESIZE_LINEAR_AREA)" % (method,))
    _need_gpu(frames)
    n, H0, W0, _ = frames.shape
    tab = _tap_table(H0, W0, H, W, method, frames.device)
    out = torch.empty(n, H, W, 3, dtype=torch.uint8, device=frames.device)
    rc = _lib.load().frame_resize_u8(frames.data_ptr(), out.data_ptr(), tab.data_ptr(), tab.numel() * 4, n, H0, W0, H, W,
                                     method, _stream())
    _lib.check(rc, "frame_resize_u8(n=%d,%dx%d->%dx%d, method %d)" % (n, H0, W0, H, W, method))
    return out


def frame_sq_diffs(frames, carry=None):
    """frames (n, H, W, 3) uint8, carry (H, W, 3) uint8 or None -> (n,) int64 on the device: entry i is the sum of squared
    differences of the 9 x 9 blurred frames i - 1 and i (frame -1 is the carry; entry 0 is 0 without one)
    (keyframe_frame_errors)"""
    _u8_frames(frames, "frame_sq_diffs: frames")
    n, H, W, _ = frames.shape
    if carry is not None:
        _dense(carry, "frame_sq_diffs: carry", torch.uint8, (H, W, 3))
        if carry.device != frames.device:
            raise ValueError("frame_sq_diffs: carry on %s, frames on %s" % (carry.device, frames.device))
    _need_gpu(frames, carry)
    lib = _lib.load()
    need = lib.keyframe_workspace_bytes(n, H, W)
    if need == 0:
        raise FrescoHipError("frame_sq_diffs: frames of %d x %d x %d are outside what the kernels take (sides >= 5, "
                             "n H W 3 < 2^40)" % (n, H, W))
    ws = torch.empty(need // 8, dtype=torch.int64, device=frames.device)
    out = torch.empty(n, dtype=torch.int64, device=frames.device)  # the kernel's uint64; the sums stay far below 2^63
    rc = lib.keyframe_frame_errors(frames.data_ptr(), _ptr(carry), out.data_ptr(), ws.data_ptr(), need, n, H, W, _stream())
    _lib.check(rc, "keyframe_frame_errors(n=%d,H=%d,W=%d)" % (n, H, W))
    return out


# ---------------------------------------------------------------------------------------------
# feature optimisation (fp32)
# ---------------------------------------------------------------------------------------------
def _opt_args(cs, prep, target, chunk):
    Bt, C, h, w = cs.shape
    N = Bt // chunk
    if prep is not None:
        fwd_flow, bwd_flow, fwd_occ, bwd_occ = [_f32c(t) for t in prep]
        assert fwd_flow.shape == (N, 2, h, w) and bwd_flow.shape == (N, 2, h, w), (fwd_flow.shape, (N, 2, h, w))
        assert fwd_occ.numel() == N * h * w and bwd_occ.numel() == N * h * w
        keep = (fwd_flow, bwd_flow, fwd_occ, bwd_occ)
    else:
        keep = (None, None, None, None)
    if target is not None:
        target = _f32c(target)
        assert target.shape == (Bt, h * w, h * w), (target.shape, (Bt, h * w, h * w))
    return N, C, h, w, keep, target


def opt_run(cs, prep, target, intra_weight, iters, chunk, lr=0.2, betas=(0.9, 0.999), eps=1e-8,
            workspace=None, context=None):
    """`iters` Adam steps on cs (chunk*N, C, h, w) fp32 contiguous, in place (fresco_opt_run).
    prep = (fwd_flow, bwd_flow, fwd_occ, bwd_occ) at feature resolution, or None."""
    _need_gpu(cs)
    assert cs.dtype == torch.float32 and cs.is_contiguous()
    N, C, h, w, keep, target = _opt_args(cs, prep, target, chunk)
    lib = _lib.load()
    has_t, has_s = int(prep is not None), int(target is not None and intra_weight > 0)
    nbytes = lib.fresco_opt_workspace_bytes(chunk, N, C, h, w, has_t, has_s)
    ws = (workspace or _default_ws).get(nbytes, cs.device)
    ctx = context or _opt_contexts.get(cs.device)
    rc = lib.fresco_opt_run(ctx.ptr, cs.data_ptr(), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]),
                            _ptr(target), ws.data_ptr(), ws.numel(), chunk, N, C, h, w, float(intra_weight),
                            int(iters), float(lr), float(betas[0]), float(betas[1]), float(eps), _stream())
    _lib.check(rc, "fresco_opt_run(chunk=%d,N=%d,C=%d,h=%d,w=%d)" % (chunk, N, C, h, w))
    return cs


def opt_run_sharded(cs, prep_pairs, target, intra_weight, iters, chunk, N_total, exchange, lr=0.2,
                    betas=(0.9, 0.999), eps=1e-8, workspace=None):
    """Frame-sharded optimize_feature loop (fresco_opt_sharded_begin / _step_part).

    cs: local (chunk*n_loc, C, h, w) fp32 contiguous, updated in place.
    prep_pairs = (fwd_flow, bwd_flow, fwd_occ, bwd_occ) for the n_loc+1 local frame pairs, or None.
    exchange: where the inter-GPU traffic happens.  Either an object with `halo_start(cs) -> handle` and
    `halo_finish(handle) -> (halo_l, halo_r)` (fresco_amd.dist.FrameShard): the exchange of the frames Adam(it-1) left
    behind is started, the launches of step `it` that read no halo frame run (part 1), then the halos are waited for and
    the boundary pairs' signs + Adam follow (part 2).  Or a plain callable `exchange(cs) -> (halo_l, halo_r)` (blocking,
    called before every undivided step).  halo_l / halo_r: the current frame before / after the owned range,
    (chunk, C, h, w) each.  Both forms give identical bits."""
    _need_gpu(cs)
    assert cs.dtype == torch.float32 and cs.is_contiguous()
    Bt, C, h, w = cs.shape
    n_loc = Bt // chunk
    keep = (None, None, None, None)
    if prep_pairs is not None:
        keep = tuple(_f32c(t) for t in prep_pairs)
        assert keep[0].shape == (n_loc + 1, 2, h, w) and keep[2].numel() == (n_loc + 1) * h * w
    if target is not None:
        target = _f32c(target)
        assert target.shape == (Bt, h * w, h * w)
    lib = _lib.load()
    has_t, has_s = int(prep_pairs is not None), int(target is not None and intra_weight > 0)
    nbytes = lib.fresco_opt_sharded_workspace_bytes(chunk, n_loc, C, h, w, has_t, has_s)
    ws = (workspace or _default_ws).get(nbytes, cs.device)
    rc = lib.fresco_opt_sharded_begin(_ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]), ws.data_ptr(),
                                      ws.numel(), chunk, n_loc, N_total, C, h, w, has_s, _stream())
    _lib.check(rc, "fresco_opt_sharded_begin")
    overlapped = hasattr(exchange, "halo_start") and hasattr(exchange, "halo_finish")

    def step(it, halo_l, halo_r, part):
        rc = lib.fresco_opt_sharded_step(cs.data_ptr(), _ptr(halo_l), _ptr(halo_r), _ptr(keep[0]), _ptr(keep[1]),
                                         _ptr(keep[2]), _ptr(keep[3]), _ptr(target), ws.data_ptr(), ws.numel(),
                                         chunk, n_loc, N_total, C, h, w, float(intra_weight), it, float(lr),
                                         float(betas[0]), float(betas[1]), float(eps), part, _stream())
        _lib.check(rc, "fresco_opt_sharded_step(it=%d, part=%d)" % (it, part))

    for it in range(1, iters + 1):
        if not has_t:
            step(it, None, None, 3)
        elif overlapped:
            handle = exchange.halo_start(cs)           # asynchronous: the frames Adam(it-1) produced
            step(it, None, None, 1)                    # normalise, interior signs, Gram, S V: under the transfer
            halo_l, halo_r = exchange.halo_finish(handle)
            halo_l, halo_r = _f32c(halo_l), _f32c(halo_r)
            step(it, halo_l, halo_r, 2)                # boundary signs + Adam
        else:
            halo_l, halo_r = exchange(cs)
            halo_l, halo_r = _f32c(halo_l), _f32c(halo_r)
            step(it, halo_l, halo_r, 3)
    return cs


def opt_loss_grad(cs, prep, target, intra_weight, chunk, workspace=None):
    """One closure evaluation: returns (loss_temporal, loss_spatial) device tensor (2,) and grad."""
    _need_gpu(cs)
    cs = _f32c(cs)
    N, C, h, w, keep, target = _opt_args(cs, prep, target, chunk)
    lib = _lib.load()
    has_t, has_s = int(prep is not None), int(target is not None and intra_weight > 0)
    nbytes = lib.fresco_opt_workspace_bytes(chunk, N, C, h, w, has_t, has_s)
    ws = (workspace or _default_ws).get(nbytes, cs.device)
    grad = torch.empty_like(cs)
    loss = torch.zeros(2, dtype=torch.float32, device=cs.device)
    rc = lib.fresco_opt_loss_grad(cs.data_ptr(), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]), _ptr(keep[3]),
                                  _ptr(target), grad.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                  chunk, N, C, h, w, float(intra_weight), _stream())
    _lib.check(rc, "fresco_opt_loss_grad")
    return loss, grad


def gram_target(x, workspace=None):
    """Cosine Gram matrix of (B,C,h,w) features -> (B,hw,hw) fp32 (fresco_gram_target)."""
    _need_gpu(x)
    x = _f32c(x)
    B, C, h, w = x.shape
    hw = h * w
    out = torch.empty(B, hw, hw, dtype=torch.float32, device=x.device)
    nbytes = _lib.load().fresco_gram_target_workspace_bytes(B, C, hw)
    ws = (workspace or _default_ws).get(nbytes, x.device)
    rc = _lib.load().fresco_gram_target(x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), B, C, hw,
                                        _stream())
    _lib.check(rc, "fresco_gram_target")
    return out


# ---------------------------------------------------------------------------------------------
# MiDaS depth annotator (src/ControlNet/annotator/midas): the pieces around fn_gemm / attention_f32 / egnet_resize_add
# (csrc/midas.hip, include/fresco_midas.h)
# ---------------------------------------------------------------------------------------------
MIDAS_GN_CHANNELS = (64, 128, 256, 512, 1024)


def midas_input(frames):
    """frames (n, H, W, 3) uint8 -> x / 127.5 - 1 as (n, H, W, 3) fp32 NHWC (midas_input)"""
    _dense(frames, "midas_input: frames", torch.uint8)
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("midas_input: frames must be (n, H, W, 3), got %s" % (tuple(frames.shape),))
    _need_gpu(frames)
    n, H, W, _ = frames.shape
    out = torch.empty(n, H, W, 3, dtype=torch.float32, device=frames.device)
    _lib.check(_lib.load().midas_input(frames.data_ptr(), out.data_ptr(), n, H, W, _stream()),
               "midas_input(n=%d,H=%d,W=%d)" % (n, H, W))
    return out


def midas_stem_conv(x_nhwc, w_split):
    """StdConv2dSame(3, 64, 7, stride 2) at even sizes (padding 2 before, 3 after) on (n, H, W, 3) fp32 NHWC, w_split =
    fn_conv7_weight(the standardised weight) -> (n, H / 2, W / 2, 64) fp32 (midas_stem_conv)"""
    _dense(x_nhwc, "midas_stem_conv: x", torch.float32)
    wh, wl = w_split
    for w in (wh, wl):
        _dense(w, "midas_stem_conv: weight planes", torch.float16, (64, 224), align=16)
    if x_nhwc.dim() != 4 or x_nhwc.shape[3] != 3 or x_nhwc.shape[1] % 2 or x_nhwc.shape[2] % 2 or x_nhwc.numel() == 0:
        raise ValueError("midas_stem_conv: x must be (n, even H, even W, 3), got %s" % (tuple(x_nhwc.shape),))
    _need_gpu(x_nhwc, wh, wl)
    n, H, W, _ = x_nhwc.shape
    out = torch.empty(n, H // 2, W // 2, 64, dtype=torch.float32, device=x_nhwc.device)
    rc = _lib.load().midas_stem_conv(x_nhwc.data_ptr(), wh.data_ptr(), wl.data_ptr(), out.data_ptr(), n, H, W,
                                     _fn_flag_ptr(x_nhwc.device), _stream())
    _lib.check(rc, "midas_stem_conv(n=%d,H=%d,W=%d)" % (n, H, W))
    return out


def midas_groupnorm(x, gamma, beta, relu=False, residual=None, eps=1e-5, want_f32=True, want_split=False, far_border=False,
                    scale=FN_A_SCALE):
    """GroupNorm(32, C) on x (n, H, W, C) fp32 NHWC: (x - mean) rstd gamma + beta [ReLU] [+ residual, ReLU]
    (midas_groupnorm_stats + midas_groupnorm_apply).  -> (y (n, H, W, C) fp32 or None, (hi, lo) planes or None).
    far_border: the planes are (n (H + 1) (W + 1), C) rows of a map with one zero row below and one zero column to the right
    -- what a "same" 3 x 3 stride-2 convolution reads with fn_gemm's pad = 0."""
    _dense(x, "midas_groupnorm: x", torch.float32, align=16)
    if x.dim() != 4 or x.numel() == 0 or x.shape[3] not in MIDAS_GN_CHANNELS:
        raise ValueError("midas_groupnorm: x must be (n, H, W, C), C in %s, got %s" % (MIDAS_GN_CHANNELS, tuple(x.shape)))
    n, H, W, C = x.shape
    if not (want_f32 or want_split):
        raise ValueError("midas_groupnorm: nothing asked for")
    if residual is not None:
        _dense(residual, "midas_groupnorm: residual", torch.float32, (n, H, W, C), align=16)
    scale = _split_scale(scale)
    _need_gpu(x)
    gamma, beta = _fn_f32_operand(gamma, "gamma", x), _fn_f32_operand(beta, "beta", x)
    if gamma.numel() != C or beta.numel() != C:
        raise ValueError("midas_groupnorm: gamma / beta of %d channels" % C)
    lib = _lib.load()
    dev = x.device
    nbytes = lib.midas_groupnorm_workspace_bytes(n, H * W, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mean = torch.empty(n, 32, dtype=torch.float32, device=dev)
    rstd = torch.empty(n, 32, dtype=torch.float32, device=dev)
    rc = lib.midas_groupnorm_stats(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ws.data_ptr(), nbytes, n, H * W, C,
                                   float(eps), _stream())
    _lib.check(rc, "midas_groupnorm_stats(n=%d,P=%d,C=%d)" % (n, H * W, C))
    y = torch.empty_like(x) if want_f32 else None
    ph, pw = (H + 1, W + 1) if far_border else (H, W)
    if want_split and far_border:  # the border rows and columns are never written: zeros
        hi = torch.zeros(n * ph * pw, C, dtype=torch.float16, device=dev)
        lo = torch.zeros(n * ph * pw, C, dtype=torch.float16, device=dev)
    else:
        hi, lo = _planes(n * ph * pw, C, dev, want_split)
    rc = lib.midas_groupnorm_apply(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                   _ptr(residual), _ptr(y), _ptr(hi), _ptr(lo), n, H, W, C, ph, pw, int(bool(relu)), scale,
                                   _fn_flag_ptr(dev), _stream())
    _lib.check(rc, "midas_groupnorm_apply(n=%d,H=%d,W=%d,C=%d)" % (n, H, W, C))
    return y, ((hi, lo) if want_split else None)


def midas_pool(x, want_f32=False, scale=FN_A_SCALE):
    """MaxPool2dSame(3, stride 2) at even sizes on x (n, H, W, 64) fp32 NHWC -> (fp32 (n, H / 2, W / 2, 64) or None, planes)"""
    _dense(x, "midas_pool: x", torch.float32, align=16)
    if x.dim() != 4 or x.shape[3] != 64 or x.numel() == 0 or x.shape[1] % 2 or x.shape[2] % 2:
        raise ValueError("midas_pool: x must be (n, even H, even W, 64), got %s" % (tuple(x.shape),))
    scale = _split_scale(scale)
    _need_gpu(x)
    n, H, W, C = x.shape
    out = torch.empty(n, H // 2, W // 2, C, dtype=torch.float32, device=x.device) if want_f32 else None
    hi, lo = _planes(n * (H // 2) * (W // 2), C, x.device, True)
    rc = _lib.load().midas_pool(x.data_ptr(), _ptr(out), hi.data_ptr(), lo.data_ptr(), n, H, W, C, scale,
                                _fn_flag_ptr(x.device), _stream())
    _lib.check(rc, "midas_pool(n=%d,H=%d,W=%d)" % (n, H, W))
    return out, (hi, lo)


def midas_layernorm(x, gamma, beta, eps=1e-6, want_f32=False, want_split=True, scale=FN_A_SCALE):
    """nn.LayerNorm(C) on (M, C) fp32 rows, C % 4 == 0 and C <= 1024 -> (y or None, planes or None) (midas_layernorm)"""
    _dense(x, "midas_layernorm: x", torch.float32, align=16)
    if x.dim() != 2 or x.numel() == 0 or x.shape[1] % 4 or x.shape[1] > 1024:
        raise ValueError("midas_layernorm: x must be (M, C), C a multiple of 4 up to 1024, got %s" % (tuple(x.shape),))
    if not (want_f32 or want_split):
        raise ValueError("midas_layernorm: nothing asked for")
    scale = _split_scale(scale)
    _need_gpu(x)
    M, C = x.shape
    gamma, beta = _fn_f32_operand(gamma, "gamma", x), _fn_f32_operand(beta, "beta", x)
    if gamma.numel() != C or beta.numel() != C:
        raise ValueError("midas_layernorm: gamma / beta of %d channels" % C)
    y = torch.empty_like(x) if want_f32 else None
    hi, lo = _planes(M, C, x.device, want_split)
    rc = _lib.load().midas_layernorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(y), _ptr(hi), _ptr(lo), M, C,
                                     float(eps), scale, _fn_flag_ptr(x.device), _stream())
    _lib.check(rc, "midas_layernorm(M=%d,C=%d)" % (M, C))
    return y, ((hi, lo) if want_split else None)


def midas_tokens(grid, cls, pos):
    """grid (n, L - 1, C) fp32, cls (C), pos (L, C) -> [cls | grid] + pos, (n, L, C) fp32 (midas_tokens)"""
    _dense(grid, "midas_tokens: grid", torch.float32, align=16)
    if grid.dim() != 3 or grid.numel() == 0 or grid.shape[2] % 4:
        raise ValueError("midas_tokens: grid must be (n, L - 1, C), C a multiple of 4, got %s" % (tuple(grid.shape),))
    n, L, C = grid.shape[0], grid.shape[1] + 1, grid.shape[2]
    _need_gpu(grid)
    cls, pos = _fn_f32_operand(cls, "cls", grid), _fn_f32_operand(pos, "pos", grid)
    if cls.numel() != C or pos.numel() != L * C:
        raise ValueError("midas_tokens: cls of %d values and pos of %d x %d expected" % (C, L, C))
    out = torch.empty(n, L, C, dtype=torch.float32, device=grid.device)
    rc = _lib.load().midas_tokens(grid.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), n, L, C, _stream())
    _lib.check(rc, "midas_tokens(n=%d,L=%d,C=%d)" % (n, L, C))
    return out


def midas_head_merge(x, n, want_f32=False, want_split=True, scale=FN_A_SCALE):
    """attention output x (heads * n, L, 64) fp32, batch = head * n + image -> rows (n L, heads 64): (fp32 or None, planes or
    None) (midas_head_merge)"""
    _dense(x, "midas_head_merge: x", torch.float32, align=16)
    if x.dim() != 3 or x.shape[2] != 64 or x.numel() == 0 or x.shape[0] % int(n):
        raise ValueError("midas_head_merge: x must be (heads * n, L, 64), got %s with n = %r" % (tuple(x.shape), n))
    if not (want_f32 or want_split):
        raise ValueError("midas_head_merge: nothing asked for")
    scale = _split_scale(scale)
    _need_gpu(x)
    heads, L = x.shape[0] // int(n), x.shape[1]
    out = torch.empty(n * L, heads * 64, dtype=torch.float32, device=x.device) if want_f32 else None
    hi, lo = _planes(n * L, heads * 64, x.device, want_split)
    rc = _lib.load().midas_head_merge(x.data_ptr(), _ptr(out), _ptr(hi), _ptr(lo), int(n), L, heads, scale,
                                      _fn_flag_ptr(x.device), _stream())
    _lib.check(rc, "midas_head_merge(n=%d,L=%d,heads=%d)" % (n, L, heads))
    return out, ((hi, lo) if want_split else None)


def midas_rowbias_gelu(x, rowbias, rows_per_img, want_f32=False, want_split=True, scale=FN_A_SCALE):
    """GELU(x[m] + rowbias[m // rows_per_img]) (erf form) on (M, C) fp32 rows -> (fp32 or None, planes or None)"""
    _dense(x, "midas_rowbias_gelu: x", torch.float32, align=16)
    if x.dim() != 2 or x.numel() == 0 or x.shape[1] % 4 or int(rows_per_img) < 1 or x.shape[0] % int(rows_per_img):
        raise ValueError("midas_rowbias_gelu: x must be (images * rows_per_img, C), got %s" % (tuple(x.shape),))
    M, C = x.shape
    _dense(rowbias, "midas_rowbias_gelu: rowbias", torch.float32, (M // int(rows_per_img), C), align=16)
    if not (want_f32 or want_split):
        raise ValueError("midas_rowbias_gelu: nothing asked for")
    scale = _split_scale(scale)
    _need_gpu(x, rowbias)
    out = torch.empty_like(x) if want_f32 else None
    hi, lo = _planes(M, C, x.device, want_split)
    rc = _lib.load().midas_rowbias_gelu(x.data_ptr(), rowbias.data_ptr(), _ptr(out), _ptr(hi), _ptr(lo), M, C,
                                        int(rows_per_img), scale, _fn_flag_ptr(x.device), _stream())
    _lib.check(rc, "midas_rowbias_gelu(M=%d,C=%d)" % (M, C))
    return out, ((hi, lo) if want_split else None)


def midas_tail(depth, a, bg_th, cond_dtype=None):
    """depth (n, H, W) fp32 -> (depth image (n, H, W) uint8, normal image (n, H, W, 3) uint8, ControlNet condition
    (n, 3, H, W) of cond_dtype or None): the lines after the network of annotator/midas/__init__.py (midas_tail)"""
    _dense(depth, "midas_tail: depth", torch.float32)
    if depth.dim() != 3 or depth.numel() == 0 or depth.shape[1] < 2 or depth.shape[2] < 2:
        raise ValueError("midas_tail: depth must be (n, H >= 2, W >= 2), got %s" % (tuple(depth.shape),))
    if cond_dtype is not None and cond_dtype not in _ELEMWISE_DTYPES:
        raise TypeError("midas_tail: cond_dtype %s (fp16, bf16 or fp32)" % (cond_dtype,))
    _need_gpu(depth)
    n, H, W = depth.shape
    dev = depth.device
    lib = _lib.load()
    nbytes = lib.midas_tail_workspace_bytes(n, H, W)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    dimg = torch.empty(n, H, W, dtype=torch.uint8, device=dev)
    nimg = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
    cond = torch.empty(n, 3, H, W, dtype=cond_dtype, device=dev) if cond_dtype is not None else None
    rc = lib.midas_tail(depth.data_ptr(), dimg.data_ptr(), nimg.data_ptr(), _ptr(cond), _ELEMWISE_DTYPES.get(cond_dtype, _lib.F32),
                        ws.data_ptr(), nbytes, n, H, W, float(a), float(bg_th), _stream())
    _lib.check(rc, "midas_tail(n=%d,H=%d,W=%d)" % (n, H, W))
    return dimg, nimg, cond


# ---------------------------------------------------------------------------------------------------------------------
# the VAE decoder's kernels (include/fresco_vae.h): fp16 NHWC activations, plain-fp16 implicit-GEMM convolutions
# ---------------------------------------------------------------------------------------------------------------------
VAE_GN_CHANNELS = (128, 256, 512)
# vae_conv, unet_groupnorm and unet_temb take fp16 or bf16 operands: the flag OR-ed into the C call's int argument
# (VAE_ELEM_BF16 / UNET_ELEM_BF16 of the headers) and unet_temb_dt's dtype code
_ELEM16_FLAG = {torch.float16: 0, torch.bfloat16: _lib.ELEM_BF16}
_ELEM16_CODE = {torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}


def _elem16(x, name):
    """the element type of a call, taken from its first operand: fp16 or bf16"""
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: expected a tensor, got %s" % (name, type(x).__name__))
    if x.dtype not in _ELEM16_FLAG:
        raise TypeError("%s: dtype %s, expected torch.float16 or torch.bfloat16" % (name, x.dtype))
    return x.dtype


def _same_elem(t, name, et, first):
    """a 16-bit operand of another type than the call's first one: both types are named"""
    if isinstance(t, torch.Tensor) and t.dtype != et and t.dtype in _ELEM16_FLAG:
        raise TypeError("%s: dtype %s, but %s is %s: one element type per call" % (name, t.dtype, first, et))
VAE_CIN_PAD = 32  # conv_in's four input channels padded to the convolution's K chunk


def vae_input(z, weight, bias, cpad=VAE_CIN_PAD):
    """latents (n, 4, h, w) fp16 NCHW -> post_quant_conv (weight (4, 4), bias (4) fp32) -> (n, h, w, cpad) fp16 NHWC, channels
    4 .. zero (vae_input)"""
    _dense(z, "vae_input: z", torch.float16)
    if z.dim() != 4 or z.shape[1] != 4 or z.numel() == 0:
        raise ValueError("vae_input: z must be (n, 4, h, w), got %s" % (tuple(z.shape),))
    _dense(weight, "vae_input: weight", torch.float32, (4, 4))
    _dense(bias, "vae_input: bias", torch.float32, (4,))
    _need_gpu(z, weight, bias)
    n, _, h, w = z.shape
    out = torch.empty(n, h, w, cpad, dtype=torch.float16, device=z.device)
    rc = _lib.load().vae_input(z.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), n, h, w, cpad, _stream())
    _lib.check(rc, "vae_input(n=%d,h=%d,w=%d,cpad=%d)" % (n, h, w, cpad))
    return out


def vae_conv(x, w, bias, n, H, W, cin, cout, ksize, up2=False, residual=None, out_kind=_lib.VAE_OUT_F16, x_img_stride=None,
             w_img_stride=0, bias_rows=False, ldo=None, out=None):
    """out = [residual +] conv(x) + bias on the plain 16-bit implicit GEMM (vae_conv of include/fresco_vae.h).  x: fp16 or
    bf16 (the element type of the call: w, residual and a 16-bit out must have it too), ksize 3: (n, H, W, cin) NHWC, or
    (n, H / 2, W / 2, cin) with up2; ksize 1: H * W rows of cin per image, x_img_stride elements apart (default H W cin;
    0 = shared).  w: (cout, ksize^2 cin) with k = (ky, kx, ci), or n such matrices w_img_stride elements apart.  -> `out`,
    or a new (n, H, W, cout) tensor of x's type / fp32 (VAE_OUT_F32) of row stride ldo, (n, cout, H, W) for VAE_OUT_F16_NCHW."""
    et = _elem16(x, "vae_conv: x")
    _dense(x, "vae_conv: x", et, align=16)
    _same_elem(w, "vae_conv: w", et, "x")
    _dense(w, "vae_conv: w", et, align=16)
    if bias is not None:
        _dense(bias, "vae_conv: bias", torch.float32, align=16)
    K = ksize * ksize * cin
    Hs, Ws = (H // 2, W // 2) if up2 else (H, W)
    if x_img_stride is None:
        x_img_stride = Hs * Ws * cin
    need_x = (n - 1) * x_img_stride + Hs * Ws * cin
    need_w = (n - 1) * w_img_stride + cout * K
    if x.numel() < need_x or w.numel() < need_w:
        raise ValueError("vae_conv: x holds %d elements (needs %d), w %d (needs %d)" % (x.numel(), need_x, w.numel(), need_w))
    if bias is not None and bias.numel() < (H * W if bias_rows else cout):
        raise ValueError("vae_conv: bias of %d values" % bias.numel())
    ldo = cout if ldo is None else int(ldo)
    odt = torch.float32 if out_kind == _lib.VAE_OUT_F32 else et
    if out is None:
        if out_kind == _lib.VAE_OUT_F16_NCHW:
            out = torch.empty(n, cout, H, W, dtype=odt, device=x.device)
        elif ldo == cout:
            out = torch.empty(n, H, W, cout, dtype=odt, device=x.device)
        else:
            out = torch.empty(n, H * W, ldo, dtype=odt, device=x.device)
    else:
        if odt is et:
            _same_elem(out, "vae_conv: out", et, "x")
        _dense(out, "vae_conv: out", odt, align=8)
    if out.numel() < n * H * W * (cout if out_kind == _lib.VAE_OUT_F16_NCHW else ldo):
        raise ValueError("vae_conv: out holds %d elements" % out.numel())
    if residual is not None:
        _same_elem(residual, "vae_conv: residual", et, "x")
        _dense(residual, "vae_conv: residual", et, align=8)
        if residual.numel() < n * H * W * ldo:
            raise ValueError("vae_conv: residual holds %d elements" % residual.numel())
    _need_gpu(x, w, bias, residual, out)
    rc = _lib.load().vae_conv(x.data_ptr(), x_img_stride, w.data_ptr(), w_img_stride, _ptr(bias), _ptr(residual),
                              out.data_ptr(), n, H, W, cin, cout, ksize, int(bool(up2)), out_kind | _ELEM16_FLAG[et],
                              int(bool(bias_rows)), ldo, _stream())
    _lib.check(rc, "vae_conv(n=%d,H=%d,W=%d,cin=%d,cout=%d,k=%d,up2=%d,kind=%d)" % (n, H, W, cin, cout, ksize, up2, out_kind))
    return out


def conv_rows(x, w, bias=None, residual=None):
    """a linear layer on vae_conv's 1 x 1 form, all rows of all images as ONE run of rows (n = 1, H = rows, W = 1): x fp16 or
    bf16 (..., K) dense, w (N, K) packed and residual (..., N) of x's type, bias fp32 (N) -> [residual +] x w^T + bias, of
    x's type (..., N)"""
    K = x.shape[-1]
    if w.dim() != 2 or w.shape[1] != K:     # what vae_conv cannot see: it is handed K; everything else it checks itself
        raise ValueError("conv_rows: x (..., K) and w (N, K), got %s and %s" % (tuple(x.shape), tuple(w.shape)))
    N = w.shape[0]
    return vae_conv(x, w, bias, 1, x.numel() // K, 1, K, N, 1, residual=residual).view(*x.shape[:-1], N)


_vae_gn_ws = _PerStreamWorkspace()


def vae_groupnorm(x, gamma, beta, eps=1e-6, silu=False):
    """GroupNorm(32, C, eps) [+ SiLU] on x (n, ..., C) fp16 NHWC, C in VAE_GN_CHANNELS; gamma / beta fp32 -> fp16 like x
    (vae_groupnorm)"""
    _dense(x, "vae_groupnorm: x", torch.float16, align=16)
    if x.dim() < 3 or x.numel() == 0 or x.shape[-1] not in VAE_GN_CHANNELS:
        raise ValueError("vae_groupnorm: x must be (n, ..., C), C in %s, got %s" % (VAE_GN_CHANNELS, tuple(x.shape)))
    n, C = x.shape[0], x.shape[-1]
    P = x.numel() // (n * C)
    _dense(gamma, "vae_groupnorm: gamma", torch.float32, (C,))
    _dense(beta, "vae_groupnorm: beta", torch.float32, (C,))
    _need_gpu(x, gamma, beta)
    lib = _lib.load()
    nbytes = lib.vae_groupnorm_workspace_bytes(n, P, C)
    ws = _vae_gn_ws.get(nbytes, x.device)
    y = torch.empty_like(x)
    rc = lib.vae_groupnorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes, n, P, C,
                           float(eps), int(bool(silu)), _stream())
    _lib.check(rc, "vae_groupnorm(n=%d,P=%d,C=%d)" % (n, P, C))
    return y


def vae_softmax(scores, Lk, scale, ld_out=None):
    """scores (rows, ld_in) fp32, the first Lk columns of a row its logits -> softmax(scale * logits) as (rows, ld_out) fp16,
    columns Lk .. zero (vae_softmax)"""
    _dense(scores, "vae_softmax: scores", torch.float32)
    if scores.dim() != 2 or scores.numel() == 0 or not 0 < Lk <= scores.shape[1]:
        raise ValueError("vae_softmax: scores (rows, ld_in >= Lk), got %s, Lk %d" % (tuple(scores.shape), Lk))
    rows, ld_in = scores.shape
    ld_out = Lk if ld_out is None else int(ld_out)
    if ld_out < Lk:
        raise ValueError("vae_softmax: ld_out %d < Lk %d" % (ld_out, Lk))
    _need_gpu(scores)
    p = torch.empty(rows, ld_out, dtype=torch.float16, device=scores.device)
    rc = _lib.load().vae_softmax(scores.data_ptr(), p.data_ptr(), rows, Lk, ld_in, ld_out, float(scale), _stream())
    _lib.check(rc, "vae_softmax(rows=%d,Lk=%d)" % (rows, Lk))
    return p


# ---------------------------------------------------------------------------------------------------------------------
# the UNet resnet block's kernels (include/fresco_unet.h): GroupNorm at the UNet's widths with the time embedding folded in
# ---------------------------------------------------------------------------------------------------------------------
UNET_GN_MIN, UNET_GN_MAX, UNET_GN_STEP = 64, 2560, 64   # C of unet_groupnorm: the multiples of 64 in this range
UNET_TEMB_MAX_N = 64

_unet_gn_ws = _PerStreamWorkspace()


def unet_gn_channels(C):
    return UNET_GN_MIN <= C <= UNET_GN_MAX and C % UNET_GN_STEP == 0


def unet_groupnorm(x, gamma, beta, eps=1e-5, silu=False, addend=None):
    """[SiLU] GroupNorm(32, C, eps)(x + addend) on x (n, ..., C) fp16 or bf16 NHWC, C a multiple of 64 in 64 .. 2560; gamma /
    beta fp32 (C); addend: fp32 (n, C), one term per image and channel, or None -> like x, in x's type (unet_groupnorm)"""
    et = _elem16(x, "unet_groupnorm: x")
    _dense(x, "unet_groupnorm: x", et, align=16)
    if x.dim() < 3 or x.numel() == 0 or not unet_gn_channels(x.shape[-1]):
        raise ValueError("unet_groupnorm: x must be (n, ..., C), C a multiple of %d in %d .. %d, got %s"
                         % (UNET_GN_STEP, UNET_GN_MIN, UNET_GN_MAX, tuple(x.shape)))
    n, C = x.shape[0], x.shape[-1]
    P = x.numel() // (n * C)
    _dense(gamma, "unet_groupnorm: gamma", torch.float32, (C,), align=16)
    _dense(beta, "unet_groupnorm: beta", torch.float32, (C,), align=16)
    if addend is not None:
        _dense(addend, "unet_groupnorm: addend", torch.float32, (n, C), align=16)
    _need_gpu(x, gamma, beta, addend)
    lib = _lib.load()
    nbytes = lib.unet_groupnorm_workspace_bytes(n, P, C)
    ws = _unet_gn_ws.get(nbytes, x.device)
    y = torch.empty_like(x)
    rc = lib.unet_groupnorm(x.data_ptr(), _ptr(addend), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes,
                            n, P, C, float(eps), int(bool(silu)) | _ELEM16_FLAG[et], _stream())
    _lib.check(rc, "unet_groupnorm(n=%d,P=%d,C=%d)" % (n, P, C))
    return y


def unet_temb(temb, weight, bias, conv_bias):
    """bias + conv_bias + SiLU(temb) W^T: temb fp16 or bf16 (n, K), n <= 64, weight (cout, K) of temb's type, bias / conv_bias
    fp32 (cout) -> fp32 (n, cout) (unet_temb_dt)"""
    et = _elem16(temb, "unet_temb: temb")
    _dense(temb, "unet_temb: temb", et, align=16)
    if temb.dim() != 2 or temb.numel() == 0:
        raise ValueError("unet_temb: temb must be (n, K), got %s" % (tuple(temb.shape),))
    n, K = temb.shape
    _same_elem(weight, "unet_temb: weight", et, "temb")
    _dense(weight, "unet_temb: weight", et, align=16)
    if weight.dim() != 2 or weight.shape[1] != K or weight.shape[0] == 0:
        raise ValueError("unet_temb: weight must be (cout, %d), got %s" % (K, tuple(weight.shape)))
    cout = weight.shape[0]
    _dense(bias, "unet_temb: bias", torch.float32, (cout,))
    _dense(conv_bias, "unet_temb: conv_bias", torch.float32, (cout,))
    _need_gpu(temb, weight, bias, conv_bias)
    out = torch.empty(n, cout, dtype=torch.float32, device=temb.device)
    rc = _lib.load().unet_temb_dt(temb.data_ptr(), weight.data_ptr(), bias.data_ptr(), conv_bias.data_ptr(), out.data_ptr(), n,
                                  K, cout, _ELEM16_CODE[et], _stream())
    _lib.check(rc, "unet_temb(n=%d,K=%d,cout=%d)" % (n, K, cout))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what the UNet transformer blocks add (include/fresco_unet_tf.h): LayerNorm with the residual add, the fused GEGLU
# ---------------------------------------------------------------------------------------------------------------------
UNET_LN_MIN, UNET_LN_MAX, UNET_LN_STEP = 64, 2560, 8   # C of unet_layernorm: the multiples of 8 in this range
UNET_GEGLU_STEP = 32                                   # K and inner of unet_geglu


def unet_ln_channels(C):
    return UNET_LN_MIN <= C <= UNET_LN_MAX and C % UNET_LN_STEP == 0


def _uniform_rows(t, name, C, dims=None):
    """(row stride ld, rows) of a fp16 (..., C) tensor (of `dims` dimensions, where given) whose row i starts i ld elements
    after the first: the last stride is 1 and the leading dimensions nest without gaps -- a dense tensor, or a column slice of
    a dense wider one -- with ld >= C, ld a multiple of 8 and a 16-byte aligned base.  Nothing is copied (_rows copies where
    this raises): the kernels only see ld."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a tensor, got %s" % (name, type(t).__name__))
    if t.dtype != torch.float16:
        raise TypeError("%s: dtype %s, expected %s (bf16 is not built)" % (name, t.dtype, torch.float16))
    if (t.dim() < 2 if dims is None else t.dim() != dims) or t.shape[-1] != C or t.numel() == 0:
        raise ValueError("%s: shape %s, expected (%s, %d)" % (name, tuple(t.shape), "B, L" if dims == 3 else "...", C))
    ld, ok = C, True
    if not t.is_contiguous():
        span = None
        for size, stride in zip(t.shape[-2::-1], t.stride()[-2::-1]):   # outwards from the rows; a dimension of 1 says nothing
            if size != 1:
                if span is None:            # (not `not span`: a stride of 0, an expanded dimension, is a value like any other)
                    ld = span = stride
                ok = ok and stride == span
                span *= size
        ok = ok and t.stride(-1) == 1
    if not ok:
        raise ValueError("%s: rows must be dense and uniformly strided (a dense tensor or a column slice of one)" % name)
    if ld < C or ld % 8 or t.data_ptr() % 16:
        raise ValueError("%s: rows must be 16-byte aligned, a multiple of 8 elements and at least %d apart" % (name, C))
    return ld, t.numel() // C


def unet_layernorm(x, gamma, beta, eps=1e-5, residual=None, want_sum=False):
    """LayerNorm(C, eps)(x [+ residual]) * gamma + beta on fp16 rows (..., C), C a multiple of 8 in 64 .. 2560; gamma / beta fp32
    (C).  x and residual may be column slices of dense wider tensors, 2-D or with leading dimensions (a row stride above C: the
    kernel only sees the stride).  -> y fp16, dense, shaped like x; with want_sum, (y, x + residual rounded once to fp16)
    (unet_layernorm)"""
    if not isinstance(x, torch.Tensor) or x.dim() < 2 or not unet_ln_channels(x.shape[-1]):
        raise ValueError("unet_layernorm: x must be (..., C), C a multiple of %d in %d .. %d, got %s"
                         % (UNET_LN_STEP, UNET_LN_MIN, UNET_LN_MAX, tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)))
    C = x.shape[-1]
    ldx, rows = _uniform_rows(x, "unet_layernorm: x", C)
    ldr = 0
    if residual is not None:
        ldr, rrows = _uniform_rows(residual, "unet_layernorm: residual", C)
        if rrows != rows:
            raise ValueError("unet_layernorm: residual of %d rows, x of %d" % (rrows, rows))
    _dense(gamma, "unet_layernorm: gamma", torch.float32, (C,), align=16)
    _dense(beta, "unet_layernorm: beta", torch.float32, (C,), align=16)
    _need_gpu(x, residual, gamma, beta)
    y = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    total = torch.empty(x.shape, dtype=torch.float16, device=x.device) if want_sum else None
    rc = _lib.load().unet_layernorm(x.data_ptr(), ldx, _ptr(residual), ldr, gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), C,
                                    _ptr(total), C, rows, C, float(eps), _stream())
    _lib.check(rc, "unet_layernorm(rows=%d,C=%d)" % (rows, C))
    return (y, total) if want_sum else y


def unet_geglu(x, w, bias, out=None):
    """(x Wv^T + bv) * gelu(x Wg^T + bg), the exact GELU: x fp16 (..., K) dense, w fp16 (2 inner, K) and bias fp32 (2 inner) in
    pack_geglu_weight's order, K % 32 == 0 and inner % 32 == 0 -> fp16 (..., inner), or into `out`, a 2-D (M, inner) tensor
    that may be a column slice (unet_geglu)"""
    _dense(x, "unet_geglu: x", torch.float16, align=16)
    _dense(w, "unet_geglu: w", torch.float16, align=16)
    if x.dim() < 2 or x.numel() == 0 or w.dim() != 2 or w.shape[1] != x.shape[-1] or w.shape[0] == 0 or w.shape[0] % 2:
        raise ValueError("unet_geglu: x (..., K) and w (2 inner, K), got %s and %s" % (tuple(x.shape), tuple(w.shape)))
    K, inner = x.shape[-1], w.shape[0] // 2
    if K % UNET_GEGLU_STEP or inner % UNET_GEGLU_STEP:
        raise ValueError("unet_geglu: K = %d and inner = %d must be multiples of %d" % (K, inner, UNET_GEGLU_STEP))
    M = x.numel() // K
    _dense(bias, "unet_geglu: bias", torch.float32, (2 * inner,), align=16)
    if out is None:
        out = torch.empty(x.shape[:-1] + (inner,), dtype=torch.float16, device=x.device)
        ldo = inner
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float16 or out.dim() != 2 or tuple(out.shape) != (M, inner):
            raise ValueError("unet_geglu: out must be a fp16 (%d, %d) tensor" % (M, inner))
        ldo = inner if M == 1 else out.stride(0)
        if out.stride(1) != 1 or ldo < inner or ldo % 4 or out.data_ptr() % 8:
            raise ValueError("unet_geglu: out rows must be dense, 8-byte aligned and a multiple of 4 elements apart")
    _need_gpu(x, w, bias, out)
    rc = _lib.load().unet_geglu(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), M, K, inner, ldo, _stream())
    _lib.check(rc, "unet_geglu(M=%d,K=%d,inner=%d)" % (M, K, inner))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# flash attention at head dim 160 (include/fresco_unet_attn.h): the 1280-wide layers of the UNet and the ControlNet
# ---------------------------------------------------------------------------------------------------------------------
UNET_ATTN_HEAD_DIM = 160


def unet_attention(q, k, v, heads, scale, out=None):
    """softmax(scale q k^T) v per (batch, head) at head dim 160: q (B, Lq, heads * 160), k and v (B, Lk, heads * 160), fp16;
    each may be a column slice of a wider buffer (q | k | v of a fused projection), k and v with one row stride.  Any Lq and
    Lk.  -> `out`, or a new dense (B, Lq, heads * 160) fp16 tensor (unet_attention).  Nothing is copied or made dense: what
    the kernel would refuse raises here."""
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise ValueError("unet_attention: q must be (B, Lq, C), got %s" % (tuple(q.shape) if isinstance(q, torch.Tensor) else type(q),))
    heads = int(heads)
    B, Lq, C = q.shape
    if heads <= 0 or C != heads * UNET_ATTN_HEAD_DIM:
        raise NotImplementedError("unet_attention: head dim %s (%d channels on %d heads), only %d is built"
                                  % (C // heads if heads > 0 and C % heads == 0 else "?", C, heads, UNET_ATTN_HEAD_DIM))
    if not (float(scale) > 0 and math.isfinite(float(scale))):
        raise ValueError("unet_attention: scale %r must be positive and finite" % (scale,))
    q_ld = _uniform_rows(q, "unet_attention: q", C, 3)[0]
    kv_ld = _uniform_rows(k, "unet_attention: k", C, 3)[0]
    v_ld = _uniform_rows(v, "unet_attention: v", C, 3)[0]
    if k.shape != v.shape or k.shape[0] != B or v_ld != kv_ld:
        raise ValueError("unet_attention: k %s and v %s must be (%d, Lk, %d) with one row stride (got %d and %d)"
                         % (tuple(k.shape), tuple(v.shape), B, C, kv_ld, v_ld))
    Lk = k.shape[1]
    if out is None:
        out = torch.empty(B, Lq, C, dtype=torch.float16, device=q.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, Lq, C):
        raise ValueError("unet_attention: out must be a fp16 (%d, %d, %d) tensor" % (B, Lq, C))
    out_ld = _uniform_rows(out, "unet_attention: out", C, 3)[0]
    _need_gpu(q, k, v, out)
    rc = _lib.load().unet_attention(q.data_ptr(), q_ld, k.data_ptr(), v.data_ptr(), kv_ld, out.data_ptr(), out_ld, B, heads, Lq,
                                    Lk, UNET_ATTN_HEAD_DIM, float(scale), _lib.F16, _stream())
    _lib.check(rc, "unet_attention(B=%d,H=%d,Lq=%d,Lk=%d)" % (B, heads, Lq, Lk))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the CLIP text model (include/fresco_text.h): token + position embedding, causal attention at head dim 64, quick-GELU fc1
# ---------------------------------------------------------------------------------------------------------------------
CLIP_ATTN_HEAD_DIM = 64
CLIP_ATTN_MAX_L = 128
CLIP_FC1_K_STEP, CLIP_FC1_N_STEP = 32, 64


def clip_embed(ids, tok, pos):
    """tok[ids] + pos[:L], fp16 + fp16 rounded once: ids int64 (B, L) dense, tok fp16 (vocab, C) and pos fp16 (>= L, C) dense
    and read where they live, C a multiple of 8 -> fp16 (B, L, C).  An id outside [0, vocab) gives a NaN row (clip_embed)."""
    if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int64 or ids.dim() != 2 or ids.numel() == 0:
        raise ValueError("clip_embed: ids must be an int64 (B, L) tensor, got %s"
                         % ((ids.dtype, tuple(ids.shape)) if isinstance(ids, torch.Tensor) else type(ids).__name__,))
    _dense(ids, "clip_embed: ids", torch.int64, align=8)
    _dense(tok, "clip_embed: tok", torch.float16, align=16)
    _dense(pos, "clip_embed: pos", torch.float16, align=16)
    B, L = ids.shape
    if tok.dim() != 2 or pos.dim() != 2 or tok.shape[0] == 0 or tok.shape[1] != pos.shape[1] or tok.shape[1] % 8 or tok.shape[1] == 0:
        raise ValueError("clip_embed: tok (vocab, C) and pos (positions, C), C a multiple of 8, got %s and %s"
                         % (tuple(tok.shape), tuple(pos.shape)))
    if pos.shape[0] < L:
        raise ValueError("clip_embed: %d tokens, the position table has %d rows" % (L, pos.shape[0]))
    vocab, C = tok.shape
    _need_gpu(ids, tok, pos)
    out = torch.empty(B, L, C, dtype=torch.float16, device=tok.device)
    rc = _lib.load().clip_embed(tok.data_ptr(), pos.data_ptr(), ids.data_ptr(), out.data_ptr(), B, L, C, vocab, _stream())
    _lib.check(rc, "clip_embed(B=%d,L=%d,C=%d,vocab=%d)" % (B, L, C, vocab))
    return out


def clip_attention(q, k, v, heads, scale, out=None):
    """causal softmax(scale q k^T) v per (sequence, head) at head dim 64: q, k, v (B, L, heads * 64) fp16 with ONE row stride
    -- dense, or the column slices of one (B, L, 3 heads 64) q | k | v buffer; 1 <= L <= 128.  -> `out`, or a new dense
    (B, L, heads * 64) fp16 tensor (clip_attention).  Nothing is copied or made dense: what the kernel would refuse raises
    here."""
    if not isinstance(q, torch.Tensor) or q.dim() != 3:
        raise ValueError("clip_attention: q must be (B, L, C), got %s" % (tuple(q.shape) if isinstance(q, torch.Tensor) else type(q),))
    heads = int(heads)
    B, L, C = q.shape
    if heads <= 0 or C != heads * CLIP_ATTN_HEAD_DIM:
        raise NotImplementedError("clip_attention: head dim %s (%d channels on %d heads), only %d is built"
                                  % (C // heads if heads > 0 and C % heads == 0 else "?", C, heads, CLIP_ATTN_HEAD_DIM))
    if L > CLIP_ATTN_MAX_L:
        raise NotImplementedError("clip_attention: %d tokens, at most %d" % (L, CLIP_ATTN_MAX_L))
    if B > 65535 or heads > 65535:
        raise NotImplementedError("clip_attention: %d sequences on %d heads, at most 65535 of each" % (B, heads))
    if not (float(scale) > 0 and math.isfinite(float(scale))):
        raise ValueError("clip_attention: scale %r must be positive and finite" % (scale,))
    lds = [_uniform_rows(t, "clip_attention: " + nm, C, 3)[0] for t, nm in ((q, "q"), (k, "k"), (v, "v"))]
    if k.shape != q.shape or v.shape != q.shape or len(set(lds)) != 1:
        raise ValueError("clip_attention: q %s, k %s and v %s must have one shape and one row stride (got %s)"
                         % (tuple(q.shape), tuple(k.shape), tuple(v.shape), lds))
    if out is None:
        out = torch.empty(B, L, C, dtype=torch.float16, device=q.device)
    elif not isinstance(out, torch.Tensor) or tuple(out.shape) != (B, L, C):
        raise ValueError("clip_attention: out must be a fp16 (%d, %d, %d) tensor" % (B, L, C))
    out_ld = _uniform_rows(out, "clip_attention: out", C, 3)[0]
    _need_gpu(q, k, v, out)
    rc = _lib.load().clip_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), lds[0], out.data_ptr(), out_ld, B, heads, L,
                                    CLIP_ATTN_HEAD_DIM, float(scale), _lib.F16, _stream())
    _lib.check(rc, "clip_attention(B=%d,H=%d,L=%d)" % (B, heads, L))
    return out


def clip_fc1(x, w, bias, out=None):
    """quick_gelu(x w^T + bias), quick_gelu(g) = g sigmoid(1.702 g): x fp16 (..., K) dense, w fp16 (N, K) dense and read where
    it lives, bias fp32 (N); K % 32 == 0 and N % 64 == 0 -> fp16 (..., N), or into `out`, a 2-D (M, N) tensor that may be a
    column slice (clip_fc1)"""
    _dense(x, "clip_fc1: x", torch.float16, align=16)
    _dense(w, "clip_fc1: w", torch.float16, align=16)
    if x.dim() < 2 or x.numel() == 0 or w.dim() != 2 or w.shape[1] != x.shape[-1] or w.shape[0] == 0:
        raise ValueError("clip_fc1: x (..., K) and w (N, K), got %s and %s" % (tuple(x.shape), tuple(w.shape)))
    K, N = x.shape[-1], w.shape[0]
    if K % CLIP_FC1_K_STEP or N % CLIP_FC1_N_STEP:
        raise ValueError("clip_fc1: K = %d must be a multiple of %d and N = %d of %d" % (K, CLIP_FC1_K_STEP, N, CLIP_FC1_N_STEP))
    M = x.numel() // K
    _dense(bias, "clip_fc1: bias", torch.float32, (N,), align=16)
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float16, device=x.device)
        ldo = N
    else:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float16 or out.dim() != 2 or tuple(out.shape) != (M, N):
            raise ValueError("clip_fc1: out must be a fp16 (%d, %d) tensor" % (M, N))
        ldo = N if M == 1 else out.stride(0)
        if out.stride(1) != 1 or ldo < N or ldo % 4 or out.data_ptr() % 8:
            raise ValueError("clip_fc1: out rows must be dense, 8-byte aligned and a multiple of 4 elements apart")
    _need_gpu(x, w, bias, out)
    rc = _lib.load().clip_fc1(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), M, K, N, ldo, _stream())
    _lib.check(rc, "clip_fc1(M=%d,K=%d,N=%d)" % (M, K, N))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what the VAE encoder adds (include/fresco_vae_enc.h)
# ---------------------------------------------------------------------------------------------------------------------
def vaeenc_input(image, cpad=VAE_CIN_PAD):
    """image (n, 3, H, W) fp16 NCHW -> (n, H, W, cpad) fp16 NHWC, channels 3 .. zero (vaeenc_input)"""
    _dense(image, "vaeenc_input: image", torch.float16)
    if image.dim() != 4 or image.shape[1] != 3 or image.numel() == 0:
        raise ValueError("vaeenc_input: image must be (n, 3, H, W), got %s" % (tuple(image.shape),))
    _need_gpu(image)
    n, _, H, W = image.shape
    out = torch.empty(n, H, W, cpad, dtype=torch.float16, device=image.device)
    rc = _lib.load().vaeenc_input(image.data_ptr(), out.data_ptr(), n, H, W, cpad, _stream())
    _lib.check(rc, "vaeenc_input(n=%d,H=%d,W=%d,cpad=%d)" % (n, H, W, cpad))
    return out


def vaeenc_conv_down(x, w, bias):
    """Downsample2D(padding=0): x (n, H, W, cin) fp16 NHWC, w (cout, 9 cin) fp16 with k = (ky, kx, ci), bias (cout) fp32 ->
    (n, H // 2, W // 2, cout) fp16 NHWC: the 3 x 3, stride-2 convolution behind a zero row at the bottom and a zero column on
    the right (vaeenc_conv_down)"""
    _dense(x, "vaeenc_conv_down: x", torch.float16, align=16)
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("vaeenc_conv_down: x must be (n, H, W, cin), got %s" % (tuple(x.shape),))
    n, H, W, cin = x.shape
    _dense(w, "vaeenc_conv_down: w", torch.float16, align=16)
    if w.dim() != 2 or w.shape[0] == 0 or w.shape[1] != 9 * cin:
        raise ValueError("vaeenc_conv_down: w must be (cout, %d), got %s" % (9 * cin, tuple(w.shape)))
    cout = w.shape[0]
    _dense(bias, "vaeenc_conv_down: bias", torch.float32, (cout,), align=16)
    _need_gpu(x, w, bias)
    out = torch.empty(n, H // 2, W // 2, cout, dtype=torch.float16, device=x.device)
    rc = _lib.load().vaeenc_conv_down(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), n, H, W, cin, cout, _stream())
    _lib.check(rc, "vaeenc_conv_down(n=%d,H=%d,W=%d,cin=%d,cout=%d)" % (n, H, W, cin, cout))
    return out


def vaeenc_moments(h, weight, bias):
    """h (n, hh, ww, 8) fp32 NHWC (conv_out through vae_conv with VAE_OUT_F32) -> quant_conv (weight (8, 8), bias (8) fp32) ->
    the distribution's parameters (n, 8, hh, ww) fp16 NCHW (vaeenc_moments)"""
    _dense(h, "vaeenc_moments: h", torch.float32, align=16)
    if h.dim() != 4 or h.shape[3] != 8 or h.numel() == 0:
        raise ValueError("vaeenc_moments: h must be (n, hh, ww, 8), got %s" % (tuple(h.shape),))
    _dense(weight, "vaeenc_moments: weight", torch.float32, (8, 8))
    _dense(bias, "vaeenc_moments: bias", torch.float32, (8,))
    _need_gpu(h, weight, bias)
    n, hh, ww, _ = h.shape
    params = torch.empty(n, 8, hh, ww, dtype=torch.float16, device=h.device)
    rc = _lib.load().vaeenc_moments(h.data_ptr(), weight.data_ptr(), bias.data_ptr(), params.data_ptr(), n, hh, ww, _stream())
    _lib.check(rc, "vaeenc_moments(n=%d,h=%d,w=%d)" % (n, hh, ww))
    return params


def vaeenc_sample(parameters, noise, scale=1.0):
    """parameters (n, 8, h, w) fp16 (mean | logvar), noise (n, 4, h, w) fp16 -> scale (mean + exp(0.5 clamp(logvar, -30, 20))
    noise) as (n, 4, h, w) fp16, computed in fp32 and rounded once (vaeenc_sample)"""
    _dense(parameters, "vaeenc_sample: parameters", torch.float16)
    if parameters.dim() != 4 or parameters.shape[1] != 8 or parameters.numel() == 0:
        raise ValueError("vaeenc_sample: parameters must be (n, 8, h, w), got %s" % (tuple(parameters.shape),))
    n, _, hh, ww = parameters.shape
    _dense(noise, "vaeenc_sample: noise", torch.float16, (n, 4, hh, ww))
    _need_gpu(parameters, noise)
    out = torch.empty_like(noise)
    rc = _lib.load().vaeenc_sample(parameters.data_ptr(), noise.data_ptr(), out.data_ptr(), n, hh, ww, float(scale), _stream())
    _lib.check(rc, "vaeenc_sample(n=%d,h=%d,w=%d)" % (n, hh, ww))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# what is left of the UNet and the ControlNet (include/fresco_unet_shell.h): the padded 3 x 3 convolution at both strides,
# the NCHW -> padded NHWC input, the time-embedding linear layers
# ---------------------------------------------------------------------------------------------------------------------
UNET_TIME_MAX_N = 64


def unet_conv3(x, w, bias, stride=1, silu=False):
    """Conv2d(cin, cout, 3, stride, padding 1) [+ SiLU]: x (n, H, W, cin) fp16 NHWC, w (cout, 9 cin) fp16 with k = (ky, kx, ci),
    bias (cout) fp32 -> (n, (H - 1) // stride + 1, (W - 1) // stride + 1, cout) fp16 NHWC (unet_conv3)"""
    _dense(x, "unet_conv3: x", torch.float16, align=16)
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError("unet_conv3: x must be (n, H, W, cin), got %s" % (tuple(x.shape),))
    n, H, W, cin = x.shape
    _dense(w, "unet_conv3: w", torch.float16, align=16)
    if w.dim() != 2 or w.shape[0] == 0 or w.shape[1] != 9 * cin:
        raise ValueError("unet_conv3: w must be (cout, %d), got %s" % (9 * cin, tuple(w.shape)))
    cout = w.shape[0]
    _dense(bias, "unet_conv3: bias", torch.float32, (cout,), align=16)
    if stride not in (1, 2):
        raise ValueError("unet_conv3: stride %r, only 1 or 2" % (stride,))
    _need_gpu(x, w, bias)
    out = torch.empty(n, (H - 1) // stride + 1, (W - 1) // stride + 1, cout, dtype=torch.float16, device=x.device)
    rc = _lib.load().unet_conv3(x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), n, H, W, cin, cout, stride,
                                _lib.UNET_ACT_SILU if silu else _lib.UNET_ACT_NONE, _stream())
    _lib.check(rc, "unet_conv3(n=%d,H=%d,W=%d,cin=%d,cout=%d,stride=%d,silu=%d)" % (n, H, W, cin, cout, stride, bool(silu)))
    return out


def unet_input(x, cpad=VAE_CIN_PAD):
    """x (n, c, H, W) fp16 NCHW, c <= cpad -> (n, H, W, cpad) fp16 NHWC, channels c .. zero (unet_input)"""
    _dense(x, "unet_input: x", torch.float16)
    if x.dim() != 4 or x.numel() == 0 or x.shape[1] > cpad:
        raise ValueError("unet_input: x must be (n, c <= %d, H, W), got %s" % (cpad, tuple(x.shape)))
    _need_gpu(x)
    n, c, H, W = x.shape
    out = torch.empty(n, H, W, cpad, dtype=torch.float16, device=x.device)
    rc = _lib.load().unet_input(x.data_ptr(), out.data_ptr(), n, c, H, W, cpad, _stream())
    _lib.check(rc, "unet_input(n=%d,c=%d,H=%d,W=%d,cpad=%d)" % (n, c, H, W, cpad))
    return out


def unet_time_linear(src, weight, bias, want_sin=False):
    """round16(bias + f(src) W^T) -> fp16 (n, cout), n <= 64 (unet_time_linear).  src fp32 (n): the timesteps, f their
    sinusoid of K = weight.shape[1] columns ([cos | sin], flip_sin_to_cos, no frequency shift) rounded to fp16; with want_sin
    -> (out, sinusoid fp16 (n, K)).  src fp16 (n, K): f = SiLU."""
    _dense(weight, "unet_time_linear: weight", torch.float16, align=16)
    if weight.dim() != 2 or weight.numel() == 0:
        raise ValueError("unet_time_linear: weight must be (cout, K), got %s" % (tuple(weight.shape),))
    cout, K = weight.shape
    _dense(bias, "unet_time_linear: bias", torch.float32, (cout,))
    if isinstance(src, torch.Tensor) and src.dtype == torch.float32:
        _dense(src, "unet_time_linear: timesteps", torch.float32)
        if src.dim() != 1 or src.numel() == 0:
            raise ValueError("unet_time_linear: timesteps must be (n), got %s" % (tuple(src.shape),))
        kind, n = _lib.UNET_SRC_TIMESTEPS, src.shape[0]
    else:
        _dense(src, "unet_time_linear: rows", torch.float16, align=16)
        if src.dim() != 2 or src.numel() == 0 or src.shape[1] != K:
            raise ValueError("unet_time_linear: rows must be (n, %d), got %s" % (K, tuple(src.shape)))
        if want_sin:
            raise ValueError("unet_time_linear: want_sin goes with timesteps")
        kind, n = _lib.UNET_SRC_SILU_ROWS, src.shape[0]
    _need_gpu(src, weight, bias)
    out = torch.empty(n, cout, dtype=torch.float16, device=src.device)
    sin = torch.empty(n, K, dtype=torch.float16, device=src.device) if want_sin else None
    rc = _lib.load().unet_time_linear(src.data_ptr(), kind, weight.data_ptr(), bias.data_ptr(), out.data_ptr(), _ptr(sin), n, K,
                                      cout, _stream())
    _lib.check(rc, "unet_time_linear(kind=%d,n=%d,K=%d,cout=%d)" % (kind, n, K, cout))
    return (out, sin) if want_sin else out
