"""CPU tests of the analysis-to-DADA entry points of the C ABI: declared in
include/pfb_api.h, exported by the library, bound by ``_lib.SYMBOLS``, and rejecting a null
plan before any device is touched."""
import ctypes
import os
import re

from conftest import REPO

NEW = ("pfb_analysis_execute_to_dada", "pfb_filterbank_execute_to_dada",
       "pfb_analysis_execute_dada_to_dada", "pfb_filterbank_execute_dada_to_dada",
       "pfb_analysis_last_dada_output")


def test_symbols_declared_exported_and_bound():
    from ska_pst_dsp_model_amd import _lib
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        text = f.read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"^(?:pfb_status|int32_t)\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in bound, name
    # the bindings' arity is the header's
    for name in NEW:
        decl = re.search(r"^(?:pfb_status|int32_t)\s+%s\s*\(([^)]*)\)" % name, text, flags=re.M).group(1)
        assert len(decl.split(",")) == len(bound[name][1]), name
    # out_scale is a float32, the capacity counts bytes
    for name in NEW[:4]:
        assert ctypes.c_float in bound[name][1], name
        decl = re.search(r"%s\s*\(([^)]*)\)" % name, text).group(1)
        assert "float out_scale" in decl and "int64_t out_capacity_bytes" in decl, name


def test_enum_values():
    from ska_pst_dsp_model_amd import _lib
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        text = f.read()
    for k, v in (("NONE", 0), ("FUSED", 1), ("STAGED", 2)):
        assert re.search(r"PFB_DADA_OUTPUT_%s = %d\b" % (k, v), text)
        assert getattr(_lib, "PFB_DADA_OUTPUT_" + k) == v
    assert len(re.findall(r"typedef enum pfb_dada_output\b", text)) == 1


def test_null_plan_is_rejected_without_a_device():
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    n_out = ctypes.c_int64(-7)
    buf = (ctypes.c_int16 * 64)()
    out = (ctypes.c_int16 * 64)()
    E = _lib.PFB_ERR_INVALID_ARG
    st = lib.pfb_analysis_execute_to_dada(None, buf, 8, 8, out, 16, 1.0, 128, ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_filterbank_execute_to_dada(None, buf, 8, 8, out, 8, 0.5, 128, ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_analysis_execute_dada_to_dada(None, buf, 16, 2, _lib.PFB_DADA_TFP, 16, out, 16, 1.0, 128,
                                               ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_filterbank_execute_dada_to_dada(None, buf, 16, 2, _lib.PFB_DADA_LOWCBF, 32, out, 32, 1.0, 128,
                                                 ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    assert n_out.value == -7
    assert lib.pfb_analysis_last_dada_output(None) == -1


def test_api_version_unchanged():
    from ska_pst_dsp_model_amd import _lib
    assert _lib.load().pfb_api_version() == 1
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        assert re.search(r"#define PFB_API_VERSION 1\b", f.read())
