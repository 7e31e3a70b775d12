"""Analysis straight from a single-channel DADA data section (pfb_analysis_execute_dada,
pfb_filterbank_execute_dada): the analysis kernels load the file's NBIT 8 / 16 / 32 samples,
polarisations interleaved, themselves (analysis_stream_dada_kernel, fir_lds_dada_kernel)
instead of the packed complex float32 series pfb_dada_unpack would make.

The contract is bit-identity with the pair pfb_dada_unpack + pfb_analysis_execute /
pfb_filterbank_execute, so every comparison against the pair is np.array_equal on samples
drawn over the type's full range; the two oracle cases keep the project's 1e-6
(conftest.assert_pfb_close).  Shapes are the smallest that reach each path: a few dozen
output rows.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

DESIGN_MAX_TAPS = 8192  # above: random taps (the host firls design takes seconds)


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _file_samples(rng, nbit, count):
    """Samples over the full range of the file's type (test_gpu_dada_synthesis._file_samples)."""
    t = orc._NBIT_NP[nbit]
    if np.issubdtype(t, np.integer):
        info = np.iinfo(t)
        return rng.integers(info.min, info.max + 1, size=count).astype(t)
    return rng.standard_normal(count).astype(t)


@functools.lru_cache(maxsize=None)
def _taps(N, os_, tpc, cut=None):
    if N * tpc > DESIGN_MAX_TAPS:
        taps = np.random.default_rng(9400 + N + tpc).standard_normal(N * tpc + 1) / N
    else:
        taps = _pfb().design_PFB_FIR_filter(N, os_, tpc)
    if cut:
        taps = taps[:cut].copy()
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def _pst_taps():
    pfb = _pfb()
    taps = pfb.read_fir_filter_coeff(pfb.config.config_dir + "/PST_filtertaps.txt")
    taps.setflags(write=False)
    return taps


def _plan(kind, n_pol):
    """kind: (N, os, tpc[, cut][, variant]) or "lowcbf"."""
    pfb = _pfb()
    if kind == "lowcbf":
        return pfb.AnalysisPlan(_pst_taps(), 256, "4/3", "polyphase_analysis_lowcbf", n_pol)
    N, os_, tpc, cut, variant = kind
    return pfb.AnalysisPlan(_taps(N, os_, tpc, cut), N, os_, variant, n_pol)


C2 = (256, "8/7", 12, None, "polyphase_analysis")          # 3073 taps: 13 phases


def _section(gpu, seed, nbit, n_dat, n_pol, ndim=2):
    import torch
    raw = _file_samples(np.random.default_rng(seed), nbit, n_dat * n_pol * ndim)
    return raw, torch.from_numpy(raw.view(np.uint8)).to(gpu)


def _unpacked(rawd, nbit, n_pol, ndim=2, lowcbf=False):
    """pfb_dada_unpack into the packed [pol][t] series."""
    from ska_pst_dsp_model_amd import layout
    return layout.dada_unpack(rawd, nbit, ndim, 1, n_pol, lowcbf=lowcbf)[:, :, 0].contiguous()


def _pair(plan, rawd, nbit, ndim=2, lowcbf=False, stateful=False):
    """The staged pair through the C ABI: pfb_dada_unpack, then the cf32 call."""
    out = plan.execute(_unpacked(rawd, nbit, plan.n_pol, ndim, lowcbf), stateful=stateful).cpu().numpy()
    assert plan.last_dada_input() == "none"
    return out


def _kernel_name(which):
    from ska_pst_dsp_model_amd import _lib
    buf = ctypes.create_string_buffer(1024)
    assert _lib.load().pfb_profile_kernel_name(which, buf, len(buf)) == 0
    return buf.value.decode()


@pytest.fixture
def profiling(gpu):
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    assert lib.pfb_profile_reset() == 0 and lib.pfb_profile_enable(1) == 0
    try:
        yield lib
    finally:
        lib.pfb_profile_enable(0)
        lib.pfb_profile_reset()


def _n_dat(kind, rows, extra):
    """Samples that give `rows` output rows of a stateless Bunton call (+ a ragged tail)."""
    N, os_, tpc, cut, _ = kind
    nu, de = (int(v) for v in os_.split("/"))
    n_taps = cut or N * tpc + 1
    return -(-n_taps // N) * N + rows * (N * de // nu) + extra


# ------------------------------------------------------------------ 1. fused == the pair
# (id, plan kind, nbit, n_pol, rows)
STREAM_CASES = [
    # a: K = 53 rows — three 16-row steps and a ragged one
    ("a-c2-nbit16-1pol", C2, 16, 1, 53),
    ("b-4over3-nbit8-2pol", (256, "4/3", 12, None, "polyphase_analysis"), 8, 2, 37),
    # c: 3072 taps, 12 phases
    ("c-c2-p12-nbit32-2pol", (256, "8/7", 12, 3072, "polyphase_analysis"), 32, 2, 37),
    # e: fewer samples than the taps span: OK, 0 rows
    ("e-c2-short", C2, 16, 2, None),
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: c[0])
def test_fused_stream_kernel_matches_unpack_then_execute(gpu, profiling, case):
    name, kind, nbit, n_pol, rows = case
    plan = _plan(kind, n_pol)
    n_dat = _n_dat(kind, rows, 17) if rows is not None else 13 * 256 - 1
    _, rawd = _section(gpu, 100 + len(name) + nbit, nbit, n_dat, n_pol)
    ref = _pair(plan, rawd, nbit)
    cf32_kernel = _kernel_name(0)
    got = plan.execute_dada(rawd, nbit).cpu().numpy()
    assert plan.last_dada_input() == "fused"
    assert got.shape == ref.shape == (n_pol, rows or 0, 256)
    assert np.array_equal(got, ref)
    if rows is None:
        return
    assert np.abs(ref).max() > 0
    dada_kernel = _kernel_name(0)
    print(f"class 0: cf32 {cf32_kernel!r}, DADA {dada_kernel!r}")
    assert "analysis_stream_kernel<" in cf32_kernel
    assert "analysis_stream_dada_kernel<" in dada_kernel and dada_kernel != cf32_kernel


def test_fused_lowcbf_first_and_stream_calls(gpu, profiling):
    """d: PFB_ANALYSIS_LOWCBF with the PST taps, NBIT 8, two pols: the first call (the
    pre-padding due: window rows before the section read as zeros), a stream call with nothing
    buffered, and one that reads its carry through the cf32 descriptor."""
    plan, twin = _plan("lowcbf", 2), _plan("lowcbf", 2)
    n = 3072 - 1536 + 41 * 192 + 5
    _, rawd = _section(gpu, 140, 8, n, 2)
    ref = _pair(twin, rawd, 8)
    cf32_kernel = _kernel_name(0)
    got = plan.execute_dada(rawd, 8).cpu().numpy()
    assert plan.last_dada_input() == "fused"
    assert ref.shape == (2, 41, 216) and np.abs(ref).max() > 0
    assert np.array_equal(got, ref)
    dada_kernel = _kernel_name(0)
    print(f"class 0: cf32 {cf32_kernel!r}, DADA {dada_kernel!r}")
    assert "analysis_stream_kernel<256, 12, 4, 3, 0, true" in cf32_kernel
    assert "analysis_stream_dada_kernel<256, 12, 4, 3, true" in dada_kernel
    for i, n in enumerate((3072 + 23 * 192 + 7, 19 * 192 + 3)):
        _, rawd = _section(gpu, 141 + i, 8, n, 2)
        ref = _pair(twin, rawd, 8, stateful=True)
        got = plan.execute_dada(rawd, 8, stateful=True).cpu().numpy()
        assert plan.last_dada_input() == "fused", i
        assert ref.shape[1] > 0 and ref.shape[1] % 4 == 0 and np.array_equal(got, ref), i
        assert plan.buffered_samples == twin.buffered_samples > 0, i


# f: the smallest Bunton and the smallest padded N > 256 cell of test_gpu_dispatch_matrix.py's
# family C that launches fir_lds_kernel; 40 output rows as there
FIR_CASES = [
    ("f-n512-4over3-tpc12-bunton", (512, "4/3", 12, None, "polyphase_analysis"), 16, 2),
    ("f-n512-4over3-tpc28-padded", (512, "4/3", 28, None, "polyphase_analysis_padded"), 16, 2),
]


@pytest.mark.parametrize("case", FIR_CASES, ids=lambda c: c[0])
def test_fused_fir_matches_unpack_then_execute(gpu, profiling, case):
    name, kind, nbit, n_pol = case
    plan = _plan(kind, n_pol)
    n_dat = _n_dat(kind, 40, 3)
    _, rawd = _section(gpu, 160 + len(name), nbit, n_dat, n_pol)
    ref = _pair(plan, rawd, nbit)
    cf32_kernel = _kernel_name(4)
    got = plan.execute_dada(rawd, nbit).cpu().numpy()
    assert plan.last_dada_input() == "fused"
    assert ref.shape[0] == n_pol and ref.shape[1] >= 40 and ref.shape[2] == 512 and np.abs(ref).max() > 0
    assert np.array_equal(got, ref)
    dada_kernel = _kernel_name(4)
    print(f"class 4: cf32 {cf32_kernel!r}, DADA {dada_kernel!r}")
    assert "fir_lds_dada_kernel<" in dada_kernel and dada_kernel != cf32_kernel


def test_fused_many_series_one_workgroup_walks_several_steps(gpu):
    """g: launch_stream gives each series min(steps, max(1, 2 CU / n_pol)) workgroups
    (csrc/pfb_analysis.hip; tests/test_gpu_partition.py RANGES["stream"]): with more series than
    CUs it is one, which walks all three steps — the window slide converting the prefetched
    file values, at a step of n_pol x 4 bytes between a series' samples."""
    import torch
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    S, rows = cu + 1, 41
    steps = -(-(-(-rows // 8)) // 2)
    assert steps == 3 and min(steps, max(1, 2 * cu // S)) == 1
    plan = _plan(C2, S)
    _, rawd = _section(gpu, 170, 16, _n_dat(C2, rows, 9), S)
    ref = plan.execute(_unpacked(rawd, 16, S))
    got = plan.execute_dada(rawd, 16)
    assert plan.last_dada_input() == "fused"
    assert tuple(ref.shape) == (S, rows, 256) and float(ref.abs().max()) > 0
    assert torch.equal(got, ref)


# ------------------------------------------------------------------ 2. stream
# five uneven chunks: one shorter than one output row (M = 224 / 192 samples), one odd
CHUNKS = (9000, 100, 7777, 6001, 9001)


def _stream_run(gpu, kind, nbit, n_pol, dada_calls):
    """CHUNKS through one plan — chunk i by pfb_filterbank_execute_dada where dada_calls[i],
    else by pfb_filterbank_execute on the unpacked chunk — against pfb_filterbank_execute on the
    unpacked chunks; output and buffered count compared after every call."""
    plan, ref_plan = _plan(kind, n_pol), _plan(kind, n_pol)
    paths, total_rows = [], 0
    for i, n in enumerate(CHUNKS):
        _, rawd = _section(gpu, 200 + i, nbit, n, n_pol)
        x = _unpacked(rawd, nbit, n_pol)
        assert plan.stream_rows(n) == ref_plan.stream_rows(n), i
        ref = ref_plan.execute(x, stateful=True).cpu().numpy()
        if dada_calls[i]:
            got = plan.execute_dada(rawd, nbit, stateful=True).cpu().numpy()
        else:
            got = plan.execute(x, stateful=True).cpu().numpy()
        paths.append(plan.last_dada_input())
        assert got.shape == ref.shape, (i, got.shape, ref.shape)
        assert np.array_equal(got, ref), i
        assert plan.buffered_samples == ref_plan.buffered_samples, i
        total_rows += ref.shape[1]
    print(kind, paths, total_rows, plan.buffered_samples)
    assert total_rows > 64 and plan.buffered_samples > 0
    return paths


@pytest.mark.parametrize("kind,nbit", [(C2, 16), ("lowcbf", 8)], ids=["c2-nbit16", "lowcbf-nbit8"])
def test_stream_chunks_match_unpacked_stream(gpu, kind, nbit):
    paths = _stream_run(gpu, kind, nbit, 2, (True,) * 5)
    # chunk 2 (100 samples after a carry) completes no row: carry and chunk are concatenated
    # (unpacked behind the carry); every other call reads its section in place
    assert paths == ["fused", "staged", "fused", "fused", "fused"]


@pytest.mark.parametrize("kind,nbit", [(C2, 16), ("lowcbf", 8)], ids=["c2-nbit16", "lowcbf-nbit8"])
def test_stream_alternating_cf32_and_dada_calls(gpu, kind, nbit):
    paths = _stream_run(gpu, kind, nbit, 2, (True, False, True, False, True))
    assert paths == ["fused", "none", "fused", "none", "fused"]


@pytest.mark.parametrize("rnd", [False, True], ids=["plain", "rndInput"])
def test_filterbank_object_execute_dada(gpu, rnd):
    """FilterBank.execute_dada == FilterBank.execute of the unpacked chunks; with rndInput it
    unpacks and quantises first (the quantiser needs the variance), so the plan sees cf32."""
    pfb = _pfb()
    cfg = dict(analysis_function="polyphase_analysis", filt_coeff=_taps(256, "8/7", 12), channels=256,
               os_factor="8/7", rndInput=rnd, rmsInput=33.8)
    fb, ref_fb = pfb.FilterBank(cfg), pfb.FilterBank(cfg)
    for i, n in enumerate((9000, 7777)):
        _, rawd = _section(gpu, 250 + i, 16, n, 2)
        _, got = fb.execute_dada(rawd, 16, n_pol=2)
        _, ref = ref_fb.execute(_unpacked(rawd, 16, 2))
        assert tuple(got.shape) == tuple(ref.shape) and ref.shape[2] > 0 and ref.shape[1] == 256
        assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy()), i
        assert fb.buffered_samples == ref_fb.buffered_samples > 0
        assert fb._plan.last_dada_input() == ("none" if rnd else "fused")


# ------------------------------------------------------------------ 3. no outside sample
EMBED_CASES = [
    ("c2-nbit16-2pol", C2, 16, 2),
    ("c2-nbit8-1pol", C2, 8, 1),
    ("c2-nbit32-2pol", C2, 32, 2),
    ("lowcbf-nbit8-2pol", "lowcbf", 8, 2),
    ("fir-n512-nbit16-2pol", FIR_CASES[0][1], 16, 2),
]


@pytest.mark.parametrize("case", EMBED_CASES, ids=lambda c: c[0])
def test_no_sample_outside_the_section_contributes(gpu, case):
    """The section in the middle of a larger allocation whose bytes before and after it hold
    the type's extreme values: the window rows before sample 0 (LowCBF pre-padding), the rows
    past n_dat and the unconditional last prefetch must all read as zero."""
    import torch
    name, kind, nbit, n_pol = case
    n_dat = 3072 - 1536 + 21 * 192 + 5 if kind == "lowcbf" else _n_dat(kind, 21, 5)
    raw, rawd = _section(gpu, 300 + len(name), nbit, n_dat, n_pol)
    t = orc._NBIT_NP[nbit]
    lo, hi = (np.iinfo(t).min, np.iinfo(t).max) if np.issubdtype(t, np.integer) else (-3.0e38, 3.0e38)
    guard = 1 << 16                                      # values on each side (a multiple of 16 bytes)
    pattern = np.where(np.arange(guard) % 3 == 0, lo, hi).astype(t)
    big = torch.from_numpy(np.concatenate([pattern, raw, pattern[::-1]]).view(np.uint8)).to(gpu)
    off = guard * t().itemsize
    inner = big[off:off + raw.nbytes]
    assert inner.data_ptr() == big.data_ptr() + off and torch.equal(inner, rawd)
    ref = _pair(_plan(kind, n_pol), rawd, nbit)
    plan = _plan(kind, n_pol)
    got = plan.execute_dada(inner, nbit).cpu().numpy()
    assert plan.last_dada_input() == "fused"
    assert ref.shape[1] >= 21 and np.isfinite(ref).all() and np.abs(ref).max() > 0
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------ 4. staged
N8 = (8, "8/7", 10, None, "polyphase_analysis")
# (id, plan kind, nbit, ndim, lowcbf order, byte offset)
STAGED_CASES = [
    ("nbit64", C2, 64, 2, False, 0),
    ("ndim1", C2, 16, 1, False, 0),
    ("one-byte-offset-nbit16", C2, 16, 2, False, 1),
    ("lowcbf-order", C2, 16, 2, True, 0),
    ("n8-plan", N8, 16, 2, False, 0),
]


@pytest.mark.parametrize("case", STAGED_CASES, ids=lambda c: c[0])
def test_staged_matches_unpack_then_execute(gpu, case):
    import torch
    name, kind, nbit, ndim, lowcbf, shift = case
    plan = _plan(kind, 2)
    n_dat = _n_dat(kind, 37, 0)
    n_dat += -n_dat % 32                                  # whole LowCBF heaps
    raw, rawd = _section(gpu, 400 + len(name), nbit, n_dat, 2, ndim)
    if shift:
        holder = torch.zeros(raw.nbytes + 16, dtype=torch.uint8, device=gpu)
        holder[shift:shift + raw.nbytes] = rawd
        rawd = holder[shift:shift + raw.nbytes]
        assert rawd.data_ptr() % 2 == 1
    ref = _pair(plan, rawd, nbit, ndim, lowcbf)
    got = plan.execute_dada(rawd, nbit, ndim=ndim, lowcbf=lowcbf).cpu().numpy()
    assert plan.last_dada_input() == "staged"
    assert ref.shape[1] >= 37 and np.abs(ref).max() > 0
    assert np.array_equal(got, ref)
    plan.execute(_unpacked(rawd, nbit, 2, ndim, lowcbf))
    assert plan.last_dada_input() == "none"


# ------------------------------------------------------------------ 5. rejections
def _raw_call(plan, stateful, rawd, nbit, ndim, order, n, out, cap, n_out, null_in=False):
    import torch
    fn = plan._lib.pfb_filterbank_execute_dada if stateful else plan._lib.pfb_analysis_execute_dada
    stream = ctypes.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
    src = ctypes.c_void_p(0 if null_in else rawd.data_ptr())
    return fn(plan._h, src, nbit, ndim, order, n, ctypes.c_void_p(out.data_ptr()), out.shape[1] * out.shape[2],
              cap, ctypes.byref(n_out), stream)


@pytest.mark.parametrize("kind,nbit", [(C2, 16), ("lowcbf", 8)], ids=["c2-nbit16", "lowcbf-nbit8"])
@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "stream"])
def test_rejections_leave_output_and_state_alone(gpu, kind, nbit, stateful):
    import torch
    from ska_pst_dsp_model_amd import _lib
    plan, twin = _plan(kind, 2), _plan(kind, 2)
    if stateful and kind != "lowcbf":
        # something buffered (a LowCBF plan stays fresh: its first call is what a retry must equal)
        for p in (plan, twin):
            p.execute_dada(_section(gpu, 500, nbit, 6000, 2)[1], nbit, stateful=True)
        assert plan.buffered_samples > 0
    buffered = plan.buffered_samples
    n = 9001
    _, rawd = _section(gpu, 501, nbit, n, 2)
    rows = plan.stream_rows(n) if stateful else plan.output_length(n)
    assert rows > 16
    out = torch.full((2, rows, plan.out_chan), -7.5, dtype=torch.complex64, device=gpu)
    n_out = ctypes.c_int64(-1)
    TFP = _lib.PFB_DADA_TFP
    bad = _lib.PFB_ERR_INVALID_ARG
    assert _raw_call(plan, stateful, rawd, 12, 2, TFP, n, out, rows, n_out) == bad           # NBIT 12
    assert _raw_call(plan, stateful, rawd, nbit, 3, TFP, n, out, rows, n_out) == bad         # NDIM 3
    assert _raw_call(plan, stateful, rawd, nbit, 2, 7, n, out, rows, n_out) == bad           # order 7
    assert _raw_call(plan, stateful, rawd, nbit, 2, TFP, n, out, rows, n_out, null_in=True) == bad
    assert n_out.value == -1
    assert _raw_call(plan, stateful, rawd, nbit, 2, TFP, n, out, rows - 1, n_out) == _lib.PFB_ERR_BUFFER_TOO_SMALL
    assert n_out.value == rows
    torch.cuda.synchronize(gpu)
    assert bool((out == -7.5).all()), "a rejected call wrote output"
    assert plan.buffered_samples == buffered
    assert (plan.stream_rows(n) if stateful else plan.output_length(n)) == rows
    # the corrected retry: what the twin, which saw no rejected call, returns (a LowCBF plan:
    # exactly a first call's rows, the pre-padding still pending)
    ref = _pair(twin, rawd, nbit, stateful=stateful)
    assert _raw_call(plan, stateful, rawd, nbit, 2, TFP, n, out, rows, n_out) == _lib.PFB_OK
    assert n_out.value == rows == ref.shape[1]
    assert np.array_equal(out.cpu().numpy(), ref)
    assert plan.buffered_samples == twin.buffered_samples


# ------------------------------------------------------------------ 6. oracle parity
def test_fused_matches_oracle_c2(gpu):
    name, kind, nbit, n_pol, rows = STREAM_CASES[0]
    plan = _plan(kind, n_pol)
    raw, rawd = _section(gpu, 100 + len(name) + nbit, nbit, _n_dat(kind, rows, 17), n_pol)
    got = plan.execute_dada(rawd, nbit).cpu().numpy()
    assert plan.last_dada_input() == "fused"
    x = orc.reshape_dada_data(raw, 2, n_pol, 1).astype(np.complex64)          # (n_pol, 1, n_dat)
    ref = orc.polyphase_analysis(x, _taps(256, "8/7", 12), 256, "8/7")
    assert ref.shape == (n_pol, 256, rows)
    assert_pfb_close(got.transpose(0, 2, 1), ref, what="DADA analysis a")


def test_fused_matches_oracle_lowcbf(gpu):
    plan = _plan("lowcbf", 2)
    n = 3072 - 1536 + 41 * 192 + 5
    raw, rawd = _section(gpu, 140, 8, n, 2)
    got = plan.execute_dada(rawd, 8).cpu().numpy()
    assert plan.last_dada_input() == "fused"
    x = orc.reshape_dada_data(raw, 2, 2, 1).astype(np.complex64)
    ref = orc.polyphase_analysis_lowcbf(x, _pst_taps(), do_padding=True)
    assert ref.shape == (2, 216, 41)
    assert_pfb_close(got.transpose(0, 2, 1), ref, what="DADA analysis d")


# ------------------------------------------------------------------ 7. harness
def test_harness_channelize_reads_nbit16_file(gpu, tmp_path):
    """harness.channelize of a two-pol NBIT-16 single-channel file == polyphase_analysis of
    read_dada_file's data, byte for byte, with the analysis reading the file's own bytes."""
    pfb = _pfb()
    taps = _taps(256, "8/7", 12)
    fir = tmp_path / "fir.npy"
    pfb.firio.save_fir_filter_coeff(str(fir), taps)
    rng = np.random.default_rng(78)
    n = _n_dat(C2, 37, 11)
    x = 3000.0 * (rng.standard_normal((2, 1, n)) + 1j * rng.standard_normal((2, 1, n)))
    src = tmp_path / "series16.dump"
    pfb.dada.write_dada_file(src, x.astype(np.complex64), {"HDR_SIZE": "4096", "TSAMP": "1.0"}, nbit=16)
    f = pfb.harness.channelize(str(src), 256, "8/7", str(fir), output_file_name="chan.dump",
                               output_dir=str(tmp_path))
    plan = pfb.core.analysis_plan(pfb.read_fir_filter_coeff(str(fir)), 256, "8/7", "polyphase_analysis", 2)
    assert plan.last_dada_input() == "fused"
    data, hdr = pfb.dada.read_dada_file(src)
    assert hdr["NBIT"] == "16" and tuple(data.shape) == (2, 1, n)
    ref = pfb.polyphase_analysis(data[:, 0, :], taps, 256, "8/7")
    assert tuple(ref.shape) == (2, 256, 37) and float(ref.abs().max()) > 0
    expect = tmp_path / "expect.dump"
    ch = dict(hdr)
    with open(f.file_path, "rb") as fh:
        got_hdr = pfb.dada.read_header(fh)
    for k in ("TSAMP", "PFB_DC_CHAN", "NCHAN_PFB_0", "OS_FACTOR"):
        ch[k] = got_hdr[k]
    pfb.dada.add_fir_filter_to_header(ch, taps, pfb.config.as_rational("8/7"))
    pfb.dada.write_dada_file(expect, ref, ch)
    with open(f.file_path, "rb") as a, open(expect, "rb") as b:
        assert a.read() == b.read()
