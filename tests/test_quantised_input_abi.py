"""CPU tests of the input quantiser's entry points of the C ABI (pfb_analysis_set_input_quantiser
and its three companions): declared in include/pfb_api.h, exported by the library, bound by
``_lib.SYMBOLS``, and rejecting a null plan before any device is touched."""
import ctypes
import os
import re

from conftest import REPO

NEW = ("pfb_analysis_set_input_quantiser", "pfb_analysis_set_input_quantiser_mode",
       "pfb_analysis_last_input_quantiser", "pfb_analysis_last_input_scale")


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
    # the rms and the scale read back are doubles
    assert bound["pfb_analysis_set_input_quantiser"][1] == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_double]
    assert ctypes.POINTER(ctypes.c_double) in bound["pfb_analysis_last_input_scale"][1]
    decl = re.search(r"^pfb_status\s+pfb_analysis_set_input_quantiser\s*\(([^)]*)\)", text, flags=re.M).group(1)
    assert "int32_t enable" in decl and "double rms" in decl


def test_enum_values():
    from ska_pst_dsp_model_amd import _lib
    text = _header()
    for k, v in (("NONE", 0), ("FUSED", 1), ("STAGED", 2)):
        assert re.search(r"PFB_INPUT_QUANTISER_%s = %d\b" % (k, v), text)
        assert getattr(_lib, "PFB_INPUT_QUANTISER_" + k) == v
    assert len(re.findall(r"typedef enum pfb_input_quantiser\b", text)) == 1


def test_null_plan_is_rejected_without_a_device():
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    E = _lib.PFB_ERR_INVALID_ARG
    assert lib.pfb_analysis_set_input_quantiser(None, 1, 20.0) == E and b"null" in lib.pfb_last_error()
    assert lib.pfb_analysis_set_input_quantiser_mode(None, _lib.PFB_QUANTISER_MOMENTS_STAGED) == E
    assert b"null" in lib.pfb_last_error()
    scale = ctypes.c_double(-3.0)
    assert lib.pfb_analysis_last_input_scale(None, ctypes.byref(scale), None) == E
    assert scale.value == -3.0
    assert lib.pfb_analysis_last_input_quantiser(None) == -1


def test_api_version_unchanged():
    from ska_pst_dsp_model_amd import _lib
    assert _lib.load().pfb_api_version() == 1
    assert re.search(r"#define PFB_API_VERSION 1\b", _header())
