"""CPU tests of the file-to-file round trip's entry points of the C ABI
(pfb_roundtrip_execute_dada_to_dada and its two halves): declared in include/pfb_api.h, exported
by the library, bound by ``_lib.SYMBOLS`` with the header's argument types, and rejecting null
plans and bad section formats before any device is touched."""
import ctypes
import os
import re
from ctypes import POINTER, c_float, c_int32, c_int64, c_void_p

from conftest import REPO

WHOLE = "pfb_roundtrip_execute_dada_to_dada"
ANA = "pfb_roundtrip_analysis_execute_dada"
SYN = "pfb_roundtrip_synthesis_execute_to_dada"

# the issue's signatures, after the two plans
IN_ARGS = [c_void_p, c_int32, c_int32, c_int32, c_int64]            # in, nbit, ndim, order, n_dat
CHAN_ARGS = [c_void_p, c_int64, POINTER(c_int64), c_int64]          # chan, capacity, n_chan_rows, sample_offset
OUT_ARGS = [c_void_p, c_int32, c_float, c_int64, POINTER(c_int64)]  # out, out_nbit, out_scale, capacity, n_out
ARGTYPES = {
    WHOLE: [c_void_p, c_void_p] + IN_ARGS + CHAN_ARGS + OUT_ARGS + [c_void_p],
    ANA: [c_void_p, c_void_p] + IN_ARGS + CHAN_ARGS + [c_void_p],
    SYN: [c_void_p, c_void_p, c_int64, c_int64] + OUT_ARGS + [c_void_p],
}
C_NAMES = {c_void_p: ("void*", "pfb_analysis_plan*", "pfb_synthesis_plan*"), c_int32: ("int32_t",),
           c_int64: ("int64_t",), c_float: ("float",), POINTER(c_int64): ("int64_t*",)}


def _header():
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        return f.read()


def test_symbols_declared_exported_and_bound():
    from ska_pst_dsp_model_amd import _lib
    text = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name, want in ARGTYPES.items():
        m = re.search(r"^pfb_status\s+%s\s*\(([^)]*)\)" % name, text, flags=re.M)
        assert m, f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound"
        assert bound[name][0] is c_int32 and bound[name][1] == want, name
        # the header's parameter types, one by one
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert len(params) == len(want), name
        for p, t in zip(params, want):
            ctype = p.replace("const ", "").rsplit(" ", 1)[0].replace(" *", "*")
            assert ctype in C_NAMES[t], (name, p)
    decl = re.search(r"%s\s*\(([^)]*)\)" % WHOLE, text).group(1)
    for part in ("int64_t chan_capacity_bytes", "int64_t* n_chan_rows", "int64_t sample_offset", "float out_scale",
                 "int64_t out_capacity_bytes", "int64_t* n_out", "void* stream"):
        assert part in " ".join(decl.split()), part
    # declared together, the whole call first
    pos = [text.index(name + "(") for name in (WHOLE, ANA, SYN)]
    assert pos == sorted(pos)


def _calls(lib, L, pa, ps, nbit=16, ndim=2, order=0, out_nbit=16):
    buf = (ctypes.c_int16 * 64)()
    chan = (ctypes.c_float * 64)()
    out = (ctypes.c_int16 * 64)()
    k, n = c_int64(-7), c_int64(-7)
    sts = [
        lib.pfb_roundtrip_execute_dada_to_dada(pa, ps, buf, nbit, ndim, order, 16, chan, 256, ctypes.byref(k), 1, out,
                                               out_nbit, 1.0, 128, ctypes.byref(n), None),
        lib.pfb_roundtrip_analysis_execute_dada(pa, ps, buf, nbit, ndim, order, 16, chan, 256, ctypes.byref(k), 1,
                                                None),
        lib.pfb_roundtrip_synthesis_execute_to_dada(pa, ps, 16, 1, out, out_nbit, 1.0, 128, ctypes.byref(n), None),
    ]
    assert (k.value, n.value) == (-7, -7), "a rejected call reported lengths"
    return sts


def test_null_plans_are_rejected_without_a_device():
    from ska_pst_dsp_model_amd import _lib as L
    lib = L.load()
    for st in _calls(lib, L, None, None):
        assert st == L.PFB_ERR_INVALID_ARG and b"null" in lib.pfb_last_error()


def test_bad_formats_are_rejected_without_a_device():
    """A bad NBIT, NDIM or order is PFB_ERR_INVALID_ARG with a message, no device needed (no
    plan exists without one, so the null-plan check answers here; the GPU tests reject the
    same formats on real plans)."""
    from ska_pst_dsp_model_amd import _lib as L
    lib = L.load()
    E = L.PFB_ERR_INVALID_ARG
    for kw in (dict(nbit=12), dict(nbit=0), dict(ndim=3), dict(ndim=0), dict(order=5), dict(out_nbit=24)):
        assert _calls(lib, L, None, None, **kw) == [E, E, E], kw
        assert lib.pfb_last_error()


def test_api_version_unchanged():
    from ska_pst_dsp_model_amd import _lib
    assert _lib.load().pfb_api_version() == 1
    assert re.search(r"#define PFB_API_VERSION 1\b", _header())
