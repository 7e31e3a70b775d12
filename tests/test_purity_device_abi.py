"""CPU tests of the verification entry points of the C ABI (pfb_testvec_generate,
pfb_purity_score_spurious, pfb_purity_score_difference): declared in include/pfb_api.h, exported
by the library, bound by ``_lib.SYMBOLS`` with the header's argument types, and rejecting every
bad argument before any device is touched."""
import ctypes
import math
import os
import re
from ctypes import POINTER, c_double, c_int32, c_int64, c_void_p

import pytest

from conftest import REPO

GEN = "pfb_testvec_generate"
SPUR = "pfb_purity_score_spurious"
DIFF = "pfb_purity_score_difference"

ARGTYPES = {
    # kind, param, n_vec, n, out, out_stride, stream
    GEN: [POINTER(c_int32), POINTER(c_double), c_int32, c_int64, c_void_p, c_int64, c_void_p],
    # a, dtype, stride, n, n_vec, scale, domain, expected, result, stream
    SPUR: [c_void_p, c_int32, c_int64, c_int64, c_int32, c_double, c_int32, POINTER(c_int64), POINTER(c_double),
           c_void_p],
    # a, a_stride, b, b_stride, n, n_vec, result, stream
    DIFF: [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int32, POINTER(c_double), c_void_p],
}
C_NAMES = {c_void_p: ("void*", "pfb_cf32*"), c_int32: ("int32_t",), c_int64: ("int64_t",), c_double: ("double",),
           POINTER(c_int32): ("int32_t*",), POINTER(c_int64): ("int64_t*",), POINTER(c_double): ("double*",)}


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
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert len(params) == len(want), name
        for p, t in zip(params, want):
            ctype = p.replace("const ", "").rsplit(" ", 1)[0].replace(" *", "*")
            assert ctype in C_NAMES[t], (name, p)
    # a section of their own, before the utilities
    pos = [text.index(s) for s in ("- verification */", GEN + "(", SPUR + "(", DIFF + "(", "- utilities */")]
    assert pos == sorted(pos)
    assert re.search(r"PFB_TESTVEC_IMPULSE = 0, PFB_TESTVEC_SINUSOID = 1", text)
    assert (_lib.PFB_TESTVEC_IMPULSE, _lib.PFB_TESTVEC_SINUSOID) == (0, 1)


class _Args:
    """Valid host-side arguments of the three calls; the 'device' buffers are fake non-null,
    8-byte aligned addresses no accepted call would get as far as using on this machine."""

    def __init__(self):
        self.kind = (c_int32 * 2)(0, 1)
        self.param = (c_double * 8)(5, 1, 0, 0, 3, math.pi / 4, 0, 0)
        self.expected = (c_int64 * 2)(1, 2)
        self.result = (c_double * 12)(*([-7.0] * 12))
        self.buf = c_void_p(0x10000)
        self.buf2 = c_void_p(0x20000)

    def gen(self, lib, **kw):
        a = dict(kind=self.kind, param=self.param, n_vec=2, n=16, out=self.buf, out_stride=16)
        a.update(kw)
        return lib.pfb_testvec_generate(a["kind"], a["param"], a["n_vec"], a["n"], a["out"], a["out_stride"], None)

    def spur(self, lib, **kw):
        a = dict(a=self.buf, dtype=0, stride=16, n=16, n_vec=2, scale=1.0, domain=30, expected=self.expected,
                 result=self.result)
        a.update(kw)
        return lib.pfb_purity_score_spurious(a["a"], a["dtype"], a["stride"], a["n"], a["n_vec"], a["scale"],
                                             a["domain"], a["expected"], a["result"], None)

    def diff(self, lib, **kw):
        a = dict(a=self.buf, a_stride=16, b=self.buf2, b_stride=16, n=16, n_vec=2, result=self.result)
        a.update(kw)
        return lib.pfb_purity_score_difference(a["a"], a["a_stride"], a["b"], a["b_stride"], a["n"], a["n_vec"],
                                               a["result"], None)


def _params(*vals):
    return (c_double * 8)(*vals)


GEN_BAD = [dict(n=0), dict(n=-3), dict(n_vec=0), dict(n_vec=-1), dict(n_vec=65536), dict(out_stride=15),
           dict(kind=None), dict(param=None), dict(out=None), dict(out=c_void_p(0x10004)),
           dict(kind=(c_int32 * 2)(0, 2)), dict(kind=(c_int32 * 2)(-1, 1)),
           dict(param=_params(math.nan, 1, 0, 0, 3, 0.5, 0, 0)), dict(param=_params(5, math.inf, 0, 0, 3, 0.5, 0, 0)),
           dict(param=_params(5, 1, 0, 0, math.inf, 0.5, 0, 0)), dict(param=_params(5, 1, 0, 0, 3, math.nan, 0, 0)),
           dict(param=_params(5, 1, 0, 0, 3, 0.5, -math.inf, 0))]
SPUR_BAD = [dict(n=0), dict(n=-1), dict(n_vec=0), dict(n_vec=65536), dict(stride=15), dict(a=None),
            dict(result=None), dict(a=c_void_p(0x10004)), dict(domain=-1), dict(dtype=2), dict(dtype=-1),
            dict(scale=math.nan), dict(scale=math.inf)]
DIFF_BAD = [dict(n=0), dict(n=-1), dict(n_vec=0), dict(n_vec=65536), dict(a_stride=15), dict(b_stride=15),
            dict(a=None), dict(b=None), dict(result=None), dict(b=c_void_p(0x20004))]


@pytest.mark.parametrize("call, cases", [("gen", GEN_BAD), ("spur", SPUR_BAD), ("diff", DIFF_BAD)])
def test_bad_arguments_are_rejected_without_a_device(call, cases):
    from ska_pst_dsp_model_amd import _lib as L
    lib = L.load()
    args = _Args()
    for kw in cases:
        st = getattr(args, call)(lib, **kw)
        assert st == L.PFB_ERR_INVALID_ARG, (call, kw, st)
        msg = lib.pfb_last_error()
        assert msg and msg.startswith(b"pfb_"), (call, kw, msg)
    assert list(args.result) == [-7.0] * 12, "a rejected call wrote results"


SAN_LIB = os.path.join(REPO, "ska-pst-dsp-model_amd", "lib", "libpfb_hip_san.so")


@pytest.mark.skipif(not os.path.exists(SAN_LIB),
                    reason="sanitizer build not present (make -C ska-pst-dsp-model_amd SANITIZE=1)")
def test_argument_checks_under_asan_ubsan():
    """tools/verify_args_check.c — a stand-alone program with its own main, built with ASan +
    UBSan and linked against the sanitizer build of the library — calls the three entry points
    with every kind of bad argument (`make SANITIZE=1 check-verify-args`; the library itself is
    taken as it is, not rebuilt)."""
    import subprocess
    r = subprocess.run(["make", "-C", os.path.join(REPO, "ska-pst-dsp-model_amd"), "SANITIZE=1",
                        "-o", "lib/libpfb_hip_san.so", "check-verify-args"],
                       capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
    assert r.returncode == 0, out[-3000:]
    assert re.search(r"verify_args_check: \d+ calls, 0 failures", out), out[-3000:]


def test_purity_sweep_rejects_an_unknown_scoring():
    from ska_pst_dsp_model_amd import verify
    with pytest.raises(ValueError, match="scoring"):
        verify.purity_sweep(scoring="bogus")


def test_device_functions_are_exported():
    from ska_pst_dsp_model_amd import verify
    assert {"device_vectors", "score_vectors_device"} <= set(verify.__all__)
    with pytest.raises(ValueError):
        verify.device_vectors([("comb", 32)], 16)


def test_api_version_unchanged():
    from ska_pst_dsp_model_amd import _lib
    assert _lib.load().pfb_api_version() == 1
