"""bf16 at the C ABI and the Python gate, without a GPU: the dtype code, and argument checks that must answer before
any HIP call."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


def test_bf16_dtype_code_in_header_and_binding():
    from fresco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fresco_hip.h")).read()
    assert re.search(r"^#define\s+FRESCO_BF16\s+2\b", hdr, re.M)
    assert _lib.BF16 == 2 and _lib.F16 == 0 and _lib.F32 == 1


def test_linear_supported_takes_bf16():
    import fresco_amd.ops as ops
    assert ops.linear_supported(320, 320, torch.bfloat16)
    assert ops.linear_supported(640, 640, torch.bfloat16)
    assert not ops.linear_supported(256, 256, torch.bfloat16)
    assert not ops.linear_supported(320, 320, torch.float32)


def _buf():
    b = ctypes.create_string_buffer(4096)  # a host buffer: never dereferenced, the calls below return before any launch
    return ctypes.addressof(b), b


def _calls(lib, p, dtype, null):
    """every dtype-carrying entry point with valid shapes; `null`: the first operand is NULL"""
    x = None if null else p
    return {
        "fresco_linear": lambda: lib.fresco_linear(x, 320, None, p, None, None, None, None, None, p, None, None, 320, 0, 0,
                                                   1, 4, 320, 320, dtype, None),
        "fresco_linear-x_rows": lambda: lib.fresco_linear(x, 320, p, p, None, None, None, None, None, p, None, None, 320, 0,
                                                          0, 1, 4, 320, 320, dtype, None),
        "fresco_attn_fwd": lambda: lib.fresco_attn_fwd(x, p, p, None, p, p, 1 << 30, 1, 8, 64, 40, 1, 64, 64, 0.158, 0.0, 320,
                                                       320, dtype, None),
        "fresco_temporal_attn": lambda: lib.fresco_temporal_attn(x, p, p, p, p, p, 2, 4, 64, 8, 40, 0.03, 320, 320, 320,
                                                                 dtype, None),
    }


@pytest.mark.parametrize("name", ["fresco_linear", "fresco_linear-x_rows", "fresco_attn_fwd", "fresco_temporal_attn"])
def test_new_entry_points_reject_bad_dtype_and_null_without_a_device(lib, name):
    from fresco_amd import _lib
    p, keep = _buf()
    assert _calls(lib, p, 7, False)[name]() == EINVAL            # unknown dtype code
    assert _calls(lib, p, _lib.F32, False)[name]() == EINVAL     # fp32 is not an element type of these kernels
    for dt in (_lib.F16, _lib.BF16):
        assert _calls(lib, p, dt, True)[name]() == EINVAL        # null operand
    del keep
