"""The C ABI as a surface, without a GPU: the ctypes binding against the header's prototypes (argument lists, not only names),
one exported symbol per operation, the mode checks of fresco_attn_f32 and the workspace query of fresco_gram_target (fake
pointers: every check answers before any HIP call), and the refusal of a library of another version."""
import ctypes
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
RETIRED = ["fresco_attn_fwd_ld", "fresco_attn_fwd_dt", "fresco_attn_fwd_kvproj_dt", "fresco_linear_rows", "fresco_linear_dt",
           "fresco_linear_rows_dt", "fresco_temporal_attn_ld", "fresco_temporal_attn_dt", "fresco_temporal_attn_packed_dt",
           "fresco_attn_f32_ws", "fresco_attn_f32_guarded", "fresco_attn_f32_guarded_ws", "fresco_opt_run_ctx",
           "fresco_opt_sharded_step_part"]
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}


@pytest.fixture(scope="module")
def lib():
    from fresco_amd import _lib
    return _lib.load()


def _ctype(decl, is_return=False):
    """ctypes type of one C parameter / return declaration: any pointer is a c_void_p (a returned const char* a c_char_p)"""
    decl = decl.strip()
    if "*" in decl:
        return ctypes.c_char_p if is_return and re.match(r"const\s+char\s*\*", decl) else ctypes.c_void_p
    words = [w for w in re.sub(r"\bconst\b", " ", decl).split()]
    return SCALARS[words[0]]  # (the parameter name, if any, follows the type)


def _prototypes():
    header = open(os.path.join(ROOT, "include", "fresco_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"^\s*#.*$", "", header, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s]*?\*?)\s*\b(fresco_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        params = params.strip()
        args = [] if params in ("", "void") else [_ctype(a) for a in params.split(",")]
        assert name not in protos, name
        protos[name] = (_ctype(ret + " ", is_return=True) if "*" in ret else SCALARS[ret.split()[-1]], args)
    return protos


def test_binding_matches_the_header_prototypes():
    from fresco_amd import _lib
    protos = _prototypes()
    assert set(protos) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.SIGNATURES)
    for name, (res, args) in protos.items():
        assert _lib.SIGNATURES[name][0] is res, (name, res)
        assert list(_lib.SIGNATURES[name][1]) == args, name


def _exported_fresco_functions(path):
    """names of the defined global functions `fresco_*` in the .dynsym of an ELF64 shared object"""
    data = open(path, "rb").read()
    assert data[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, off, size, link, _, _, entsize in sections:
        if sh_type != 11:  # SHT_DYNSYM
            continue
        str_off = sections[link][4]
        for i in range(size // entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", data, off + i * entsize)
            name = data[str_off + st_name:data.index(b"\0", str_off + st_name)].decode()
            if st_shndx != 0 and st_info >> 4 in (1, 2) and st_info & 15 == 2 and name.startswith("fresco_"):
                names.add(name)
    return names


def test_retired_names_are_gone(lib):
    import fresco_amd
    from fresco_amd import _lib
    for name in RETIRED:
        assert not hasattr(lib, name), name
        assert name not in _lib.SIGNATURES
    exported = _exported_fresco_functions(fresco_amd.LIB_PATH)
    assert exported == set(_lib.SIGNATURES), exported ^ set(_lib.SIGNATURES)
    assert len(exported) == 78  # 84 - 14 retired + fresco_gram_target_workspace_bytes = 71, + 4 egnet + 3 canny


def test_one_library_holds_the_process_wide_state():
    """fresco_amd/lib holds one libfresco_*.so, and fresco_version / fresco_last_error are each exported once among its
    files: a second library would carry its own last error, dynamic-LDS table, CU cache and fresco_prof_* recorder"""
    import glob
    lib_dir = os.path.join(ROOT, "fresco_amd", "lib")
    assert glob.glob(os.path.join(lib_dir, "libfresco_*.so")) == [os.path.join(lib_dir, "libfresco_hip.so")]
    exporters = {"fresco_version": [], "fresco_last_error": []}
    for name in sorted(os.listdir(lib_dir)):
        path = os.path.join(lib_dir, name)
        if os.path.isfile(path) and open(path, "rb").read(6) == b"\x7fELF\x02\x01":
            for symbol in exporters:
                if symbol in _exported_fresco_functions(path):
                    exporters[symbol].append(name)
    assert exporters == {"fresco_version": ["libfresco_hip.so"], "fresco_last_error": ["libfresco_hip.so"]}


def test_attn_f32_mode_checks_without_a_device(lib):
    p = 4096  # fake, aligned, never touched
    B, Lq, Lk, D, Dv = 2, 300, 70, 32, 5
    need = lib.fresco_attn_f32_workspace_bytes(B, Lk, D, Dv)
    assert need > 0

    def call(ws=p, wsb=need, flag=p, zero=1, B=B, D=D, Dv=Dv, q=p):
        return lib.fresco_attn_f32(q, p, p, p, ws, wsb, flag, zero, B, Lq, Lk, D, Dv, 0.17, None)

    assert call(ws=None, wsb=0) == EINVAL            # only the workspace kernels carry the in-kernel range test
    assert call(flag=None) == EINVAL                 # a zero word that is not there
    assert call(q=None) == EINVAL
    for flag, zero in ((None, 0), (p, 0), (p, 1)):
        assert call(wsb=need - 1, flag=flag, zero=zero) == EWORKSPACE
        assert call(D=48, flag=flag, zero=zero) == EUNSUPPORTED
        assert call(Dv=129, flag=flag, zero=zero) == EUNSUPPORTED
        assert call(B=65536, wsb=1 << 40, flag=flag, zero=zero) == EUNSUPPORTED
    for flag in (None, p):                           # ... and without a workspace, before the memset and the range pass
        assert call(ws=None, wsb=0, flag=flag, zero=0, B=65536) == EUNSUPPORTED
        assert call(ws=None, wsb=0, flag=flag, zero=0, D=48) == EUNSUPPORTED
    assert lib.fresco_attn_f32_workspace_bytes(B, Lk, 48, Dv) == 0


def test_gram_target_workspace_query(lib):
    p = 4096
    for bad in ((0, 64, 256), (2, 0, 256), (2, 64, -1)):
        assert lib.fresco_gram_target_workspace_bytes(*bad) == 0
    need = lib.fresco_gram_target_workspace_bytes(2, 64, 256)
    assert need >= (2 * 64 * 256 + 33 * 2 * 256) * 4
    assert lib.fresco_gram_target(p, p, p, need - 1, 2, 64, 256, None) == EWORKSPACE


def test_stale_library_is_refused(lib, monkeypatch):
    from fresco_amd import _lib

    class Stale:
        """the built library, except that it reports the version before this binding's"""
        def __getattr__(self, name):
            return getattr(lib, name)

        @staticmethod
        def fresco_version():
            return b"fresco_hip 0.4.0 gfx950"

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: Stale())
    with pytest.raises(_lib.FrescoHipError, match="stale build"):
        _lib.load()
    assert _lib._lib is None
