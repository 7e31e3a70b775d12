"""CPU tests of the strided-input synthesis entry points of the C ABI: declared in
include/pfb_api.h, exported by the library, bound by ``_lib.SYMBOLS``, and rejecting a null
plan before any device is touched."""
import ctypes
import os
import re

from conftest import REPO

NEW = ("pfb_synthesis_execute_strided", "pfb_inverse_filterbank_execute_strided",
       "pfb_synthesis_last_strided_input")


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
    for k, v in (("NONE", 0), ("IN_PLACE", 1), ("STAGED", 2)):
        assert re.search(r"PFB_STRIDED_INPUT_%s = %d\b" % (k, v), text)
        assert getattr(_lib, "PFB_STRIDED_INPUT_" + k) == v


def test_null_plan_is_rejected_without_a_device():
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    n_out = ctypes.c_int64(-7)
    buf = (ctypes.c_float * 64)()
    out = (ctypes.c_float * 64)()
    st = lib.pfb_synthesis_execute_strided(None, buf, 8, 16, 1, 32, 2, 1, out, 8, 8,
                                           ctypes.byref(n_out), None)
    assert st == _lib.PFB_ERR_INVALID_ARG and b"null" in lib.pfb_last_error()
    st = lib.pfb_inverse_filterbank_execute_strided(None, buf, 8, 16, 1, 32, 2, out, 8, 8,
                                                    ctypes.byref(n_out), None)
    assert st == _lib.PFB_ERR_INVALID_ARG and b"null" in lib.pfb_last_error()
    assert n_out.value == -7
    assert lib.pfb_synthesis_last_strided_input(None) == -1


def test_api_version_unchanged():
    from ska_pst_dsp_model_amd import _lib
    assert _lib.load().pfb_api_version() == 1
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        assert re.search(r"#define PFB_API_VERSION 1\b", f.read())
