"""CPU tests of the synthesis-to-DADA entry points of the C ABI: declared in
include/pfb_api.h, exported by the library, bound by ``_lib.SYMBOLS``, reusing the analysis's
``pfb_dada_output`` enum, and rejecting a null plan before any device is touched."""
import ctypes
import os
import re

from conftest import REPO

NEW = ("pfb_synthesis_execute_to_dada", "pfb_inverse_filterbank_execute_to_dada",
       "pfb_synthesis_execute_dada_to_dada", "pfb_inverse_filterbank_execute_dada_to_dada",
       "pfb_synthesis_last_dada_output")


def _header():
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        return f.read()


def test_symbols_declared_exported_and_bound():
    from ska_pst_dsp_model_amd import _lib
    text = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"^(?:pfb_status|int32_t)\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in bound, name
        # the binding's arity is the header's
        decl = re.search(r"^(?:pfb_status|int32_t)\s+%s\s*\(([^)]*)\)" % name, text, flags=re.M).group(1)
        assert len(decl.split(",")) == len(bound[name][1]), name
    # out_scale is a float32, the capacity counts bytes; the stateless calls take a sample offset
    for name in NEW[:4]:
        assert ctypes.c_float in bound[name][1], name
        decl = re.search(r"%s\s*\(([^)]*)\)" % name, text).group(1)
        assert "float out_scale" in decl and "int64_t out_capacity_bytes" in decl, name
        assert ("int64_t sample_offset" in decl) == name.startswith("pfb_synthesis_"), name
    # declared in the order of their analysis twins
    pos = [text.index(name + "(") for name in NEW]
    assert pos == sorted(pos)


def test_enum_is_reused():
    """No second enum: pfb_synthesis_last_dada_output reports pfb_dada_output's values."""
    from ska_pst_dsp_model_amd import _lib
    text = _header()
    assert len(re.findall(r"typedef enum pfb_dada_output\b", text)) == 1
    assert not re.search(r"typedef enum pfb_(synthesis|synth)\w*dada_output", text)
    assert len(re.findall(r"PFB_DADA_OUTPUT_FUSED\s*=", text)) == 1
    assert (_lib.PFB_DADA_OUTPUT_NONE, _lib.PFB_DADA_OUTPUT_FUSED, _lib.PFB_DADA_OUTPUT_STAGED) == (0, 1, 2)


def test_null_plan_is_rejected_without_a_device():
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    n_out = ctypes.c_int64(-7)
    buf = (ctypes.c_int16 * 64)()
    out = (ctypes.c_int16 * 64)()
    E = _lib.PFB_ERR_INVALID_ARG
    st = lib.pfb_synthesis_execute_to_dada(None, buf, 8, 8, 1, out, 16, 1.0, 128, ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_inverse_filterbank_execute_to_dada(None, buf, 8, 8, out, 8, 0.5, 128, ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_synthesis_execute_dada_to_dada(None, buf, 16, 2, _lib.PFB_DADA_TFP, 16, 1, out, 16, 1.0, 128,
                                                ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    st = lib.pfb_inverse_filterbank_execute_dada_to_dada(None, buf, 16, 2, _lib.PFB_DADA_LOWCBF, 32, out, 32, 1.0,
                                                         128, ctypes.byref(n_out), None)
    assert st == E and b"null" in lib.pfb_last_error()
    assert n_out.value == -7
    assert lib.pfb_synthesis_last_dada_output(None) == -1


def test_api_version_unchanged():
    from ska_pst_dsp_model_amd import _lib
    assert _lib.load().pfb_api_version() == 1
    assert re.search(r"#define PFB_API_VERSION 1\b", _header())
