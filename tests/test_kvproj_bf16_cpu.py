"""The entry points of the fused K | V projection-pack and of the packed temporal pass at the C ABI, without a
GPU: declared, bound, and every argument check answers before any HIP call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
NAMES = ["fresco_attn_fwd_kvproj", "fresco_temporal_attn_packed"]


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_declared_and_bound(lib, name):
    from fresco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fresco_hip.h")).read()
    assert re.search(r"^int\s+%s\(" % name, hdr, re.M)
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    # the dtype code sits in front of the stream in both
    assert _lib.SIGNATURES[name][1][-2:] == [ctypes.c_int, ctypes.c_void_p]


def _buf():
    b = ctypes.create_string_buffer(4096)  # a host buffer: never dereferenced, the calls below return before any launch
    return ctypes.addressof(b), b


def _calls(lib, p, dtype, null, hdk=(8, 40, 320)):
    """both entry points with valid shapes; `null`: the first operand is NULL"""
    x = None if null else p
    H, D, K = hdk
    return {
        "fresco_attn_fwd_kvproj": lambda: lib.fresco_attn_fwd_kvproj(x, p, K, p, p, p, p, p, 1 << 30, 2, H, 64, D, 2, 64, K,
                                                                     0.158, H * D, dtype, None),
        "fresco_temporal_attn_packed": lambda: lib.fresco_temporal_attn_packed(x, p, p, 2, 4, 64, 8, 40, 0.03, dtype, None),
    }


@pytest.mark.parametrize("name", NAMES)
def test_entry_points_reject_bad_dtype_and_null_without_a_device(lib, name):
    from fresco_amd import _lib
    p, keep = _buf()
    assert _calls(lib, p, 7, False)[name]() == EINVAL            # unknown dtype code
    assert _calls(lib, p, _lib.F32, False)[name]() == EINVAL     # fp32 is not an element type of these kernels
    for dt in (_lib.F16, _lib.BF16):
        assert _calls(lib, p, dt, True)[name]() == EINVAL        # null operand
    del keep


def test_kvproj_dt_unsupported_shape_without_a_device(lib):
    from fresco_amd import _lib
    p, keep = _buf()
    for dt in (_lib.F16, _lib.BF16):
        assert _calls(lib, p, dt, False, hdk=(8, 64, 512))["fresco_attn_fwd_kvproj"]() == EUNSUPPORTED
    del keep


def test_version_is_0_5_0(lib):
    """(0.3.0 added the bf16 K | V pack entry points; 0.4.0, fresco_linear_plan; 0.5.0 left one entry point per operation)"""
    assert "0.5.0" in lib.fresco_version().decode()
