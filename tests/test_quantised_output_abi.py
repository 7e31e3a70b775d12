"""CPU tests of the quantised to-DADA entry points of the C ABI: declared in include/pfb_api.h,
exported by the library, bound by ``_lib.SYMBOLS``, and rejecting a null plan before any device
is touched."""
import ctypes
import os
import re

from conftest import REPO

EXEC = ("pfb_analysis_execute_quantised_to_dada", "pfb_filterbank_execute_quantised_to_dada",
        "pfb_analysis_execute_dada_quantised_to_dada", "pfb_filterbank_execute_dada_quantised_to_dada")
NEW = EXEC + ("pfb_analysis_set_quantiser_moments", "pfb_analysis_last_quantiser")


def _header():
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        return f.read()


def test_symbols_declared_exported_and_bound():
    from ska_pst_dsp_model_amd import _lib
    text = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in NEW:
        decl = re.search(r"^(?:pfb_status|int32_t)\s+%s\s*\(([^)]*)\)" % name, text, flags=re.M)
        assert decl, name
        assert hasattr(lib, name), name
        assert name in bound, name
        # the bindings' arity is the header's
        assert len(decl.group(1).split(",")) == len(bound[name][1]), name
    for name in EXEC:
        decl = re.search(r"%s\s*\(([^)]*)\)" % name, text).group(1)
        # rms and the returned scale are doubles, out_scale a float32, the capacity counts bytes
        assert "double rms" in decl and "double* scale" in decl, name
        assert "float out_scale" in decl and "int64_t out_capacity_bytes" in decl, name
        args = bound[name][1]
        assert args.count(ctypes.c_double) == 1 and args.count(ctypes.c_float) == 1, name
        assert ctypes.POINTER(ctypes.c_double) in args, name


def test_enum_values():
    from ska_pst_dsp_model_amd import _lib
    text = _header()
    for k, v in (("AUTO", 0), ("FUSED", 1), ("STAGED", 2)):
        assert re.search(r"PFB_QUANTISER_MOMENTS_%s = %d\b" % (k, v), text)
        assert getattr(_lib, "PFB_QUANTISER_MOMENTS_" + k) == v
    for k, v in (("NONE", 0), ("FUSED", 1), ("STAGED", 2)):
        assert re.search(r"PFB_QUANTISER_%s = %d\b" % (k, v), text)
        assert getattr(_lib, "PFB_QUANTISER_" + k) == v
    assert len(re.findall(r"typedef enum pfb_quantiser_moments\b", text)) == 1
    assert len(re.findall(r"typedef enum pfb_quantiser\b", text)) == 1


def test_null_plan_is_rejected_without_a_device():
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    n_out = ctypes.c_int64(-7)
    scale = ctypes.c_double(-3.0)
    buf = (ctypes.c_int16 * 64)()
    out = (ctypes.c_int16 * 64)()
    E = _lib.PFB_ERR_INVALID_ARG
    tail = (ctypes.byref(n_out), ctypes.byref(scale), None)
    st = lib.pfb_analysis_execute_quantised_to_dada(None, buf, 8, 8, 30.0, out, 16, 1.0, 128, *tail)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_filterbank_execute_quantised_to_dada(None, buf, 8, 8, 0.0, out, 8, 0.5, 128, *tail)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_analysis_execute_dada_quantised_to_dada(None, buf, 16, 2, _lib.PFB_DADA_TFP, 16, 30.0, out, 16, 1.0,
                                                         128, *tail)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_filterbank_execute_dada_quantised_to_dada(None, buf, 16, 2, _lib.PFB_DADA_TFP, 32, 30.0, out, 32,
                                                           1.0, 128, *tail)
    assert st == E and b"null" in lib.pfb_last_error()
    assert n_out.value == -7 and scale.value == -3.0
    assert lib.pfb_analysis_set_quantiser_moments(None, _lib.PFB_QUANTISER_MOMENTS_STAGED) == E
    assert lib.pfb_analysis_last_quantiser(None) == -1


def test_api_version_unchanged():
    from ska_pst_dsp_model_amd import _lib
    assert _lib.load().pfb_api_version() == 1
    assert re.search(r"#define PFB_API_VERSION 1\b", _header())
