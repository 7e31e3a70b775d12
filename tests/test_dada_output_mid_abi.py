"""CPU tests that the 4096-channel to-DADA path added no C ABI: the functions declared in
include/pfb_api.h, bound by ``_lib.SYMBOLS`` and exported by the library are the 81 there were,
the path enums keep their values, and the analysis ``_to_dada`` prototypes are unchanged."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

from conftest import REPO

N_FUNCTIONS = 81
NAMES_SHA256 = "4a6f0b3aa22b8cd1cb2acc7ab0f5002c27f4754471ba0a8c7f1955a551ea1cf1"  # "\n".join(sorted(names))

PROTOTYPES = (
    "pfb_status pfb_analysis_execute_to_dada(pfb_analysis_plan* plan, const pfb_cf32* in, int64_t in_pol_stride, "
    "int64_t n_dat, void* out, int32_t out_nbit, float out_scale, int64_t out_capacity_bytes, int64_t* n_out, "
    "void* stream)",
    "pfb_status pfb_filterbank_execute_to_dada(pfb_analysis_plan* plan, const pfb_cf32* in, int64_t in_pol_stride, "
    "int64_t n_in, void* out, int32_t out_nbit, float out_scale, int64_t out_capacity_bytes, int64_t* n_out, "
    "void* stream)",
    "pfb_status pfb_analysis_execute_dada_to_dada(pfb_analysis_plan* plan, const void* in, int32_t nbit, "
    "int32_t ndim, int32_t order, int64_t n_dat, void* out, int32_t out_nbit, float out_scale, "
    "int64_t out_capacity_bytes, int64_t* n_out, void* stream)",
    "pfb_status pfb_filterbank_execute_dada_to_dada(pfb_analysis_plan* plan, const void* in, int32_t nbit, "
    "int32_t ndim, int32_t order, int64_t n_in, void* out, int32_t out_nbit, float out_scale, "
    "int64_t out_capacity_bytes, int64_t* n_out, void* stream)",
    "pfb_status pfb_analysis_execute_quantised_to_dada(pfb_analysis_plan* plan, const pfb_cf32* in, "
    "int64_t in_pol_stride, int64_t n_dat, double rms, void* out, int32_t out_nbit, float out_scale, "
    "int64_t out_capacity_bytes, int64_t* n_out, double* scale, void* stream)",
    "int32_t pfb_analysis_last_dada_output(const pfb_analysis_plan* plan)",
)


def _header():
    with open(os.path.join(REPO, "include", "pfb_api.h")) as f:
        return f.read()


def _declared(text):
    return sorted(set(re.findall(r"^(?:pfb_status|int32_t|int64_t|double|const char\*|void)\s+(pfb_\w+)\s*\(", text,
                                 flags=re.M)))


def _digest(names):
    return hashlib.sha256("\n".join(names).encode()).hexdigest()


def test_no_function_was_added_or_removed():
    from ska_pst_dsp_model_amd import _lib
    names = _declared(_header())
    assert len(names) == N_FUNCTIONS and _digest(names) == NAMES_SHA256, names
    assert sorted(n for n, _, _ in _lib.SYMBOLS) == names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    # the library's own export list, where a symbol lister is at hand
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True,
                             text=True).stdout
        exported = sorted({ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("pfb_")})
        assert exported == names, sorted(set(exported) ^ set(names))


def test_to_dada_prototypes_unchanged():
    flat = " ".join(_header().split())
    for proto in PROTOTYPES:
        assert proto + ";" in flat, proto


def test_path_enums_unchanged():
    from ska_pst_dsp_model_amd import _lib
    text = _header()
    for enum, values in (("PFB_DADA_OUTPUT", (("NONE", 0), ("FUSED", 1), ("STAGED", 2))),
                         ("PFB_DADA_INPUT", (("NONE", 0), ("FUSED", 1), ("STAGED", 2))),
                         ("PFB_INPUT_QUANTISER", (("NONE", 0), ("FUSED", 1), ("STAGED", 2)))):
        for k, v in values:
            assert re.search(r"%s_%s = %d\b" % (enum, k, v), text), (enum, k)
            assert getattr(_lib, f"{enum}_{k}") == v
    assert _lib.load().pfb_api_version() == 1 and re.search(r"#define PFB_API_VERSION 1\b", text)
