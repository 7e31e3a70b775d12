"""Oracle parity of the persistent kernels' loop-carried code: workgroups that run SEVERAL
steps or blocks, and plans of many series.

Every persistent launcher gives a workgroup a contiguous range of steps (16 output rows) or
synthesis blocks, and the kernel carries state from one to the next: the streaming analysis
slides its register window and prefetches the next step's rows, the wave and block synthesis
kernels prefetch the next block and reuse its overlap rows, the register-window FIR slides
along a residue's rows.  The number of ranges comes from the CU count and the plan's series
count (n_pol); with one or two series of a few hundred rows on a 256-CU part it exceeds the
number of steps, so a workgroup runs exactly one and none of that code executes.  A LARGE
series count drives the per-series range count down to 1 instead: one workgroup then walks
all steps of a short series, with a few MB of input.

The launchers' range expressions, restated (RANGES below; CU = multi_processor_count, the
attribute cu_count() of csrc/pfb_common.hpp reads; S = the plan's series count):

  stream    csrc/pfb_analysis.hip : launch_stream        min(steps, max(1, 2 CU / S))
            (the LowCBF filterbank too: launch_lowcbf -> launch_lowcbf_stream -> launch_stream)
  wave      csrc/pfb_synth_wave.hip : launch_wave_t      min(blocks, max(1, 3 CU / (N/16 S)))
  wave512   csrc/pfb_synth_wave512.hip : launch_w5       min(blocks, max(1, ceil(6 CU / (N/8 S))))
  block     csrc/pfb_synth.hip : launch_sb               min(blocks, max(1, per_cu CU / (groups S))),
            groups = N / (2 PAIRS), per_cu <= 512 / threads <= 4 (the LDS-limited count)
  firwin    csrc/pfb_analysis.hip : launch_fir_window_t  max(1, ceil(4096 / (N/256 nu S)))
  (the descriptor-extent lower bounds of launch_stream and launch_fir_window_t are 1 at
  these lengths.)  All kernels split n steps / blocks / rows over nw ranges as
  [n w / nw, n (w + 1) / nw).

Two regimes per case, each ASSERTED from that table (a launcher change that lets the shape no
longer force the loop fails the case; nothing is skipped):
  one    the expression gives 1 range per series: one workgroup runs all 7 steps or blocks;
  three  it gives 3: 7 steps or blocks split 2, 2, 3, the last one partial.

Every case: three distinct seeded complex-noise series base[0..2], expanded on the device to
x[p] = base[p % 3]; lengths no multiple of M, N or keep; and three checks —
  1. out[0:3] against oracle.pfb_oracle with conftest.assert_pfb_close at 1e-6 (RMS scale;
     raw for round-trip outputs);
  2. out[p] bit-identical to out[p % 3] for every p (compared on the device);
  3. out[0:3] bit-identical to a plan of the same configuration with n_pol = 3 fed `base`,
     which is partitioned one step or block per workgroup (the invariance the stream-versus-
     one-shot and chunking tests already claim).
The kernel (or multi-launch path) of each case is pinned with the C ABI's profiler, as in
test_gpu_dispatch_matrix.py.  No PFB_* environment knob is read or set.

Not here: the 4096-point row-FFT persistent kernels (>= 3072 rows of 4096 channels per series;
the full-size tests run their loops) and fir_lds_kernel (its range count depends on neither
CU nor n_pol).
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

SEED = 9300
DESIGN_MAX_TAPS = 8192  # above: random taps (the host firls design takes seconds)
REGIMES = ("one", "three")


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _rat(os_):
    nu, de = os_.split("/")
    return int(nu), int(de)


@functools.lru_cache(maxsize=None)
def _taps(N, os_, tpc):
    if N * tpc > DESIGN_MAX_TAPS:
        taps = np.random.default_rng(SEED + N + N * tpc + 1).standard_normal(N * tpc + 1) / N
    else:
        taps = _pfb().design_PFB_FIR_filter(N, os_, tpc)
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def _pst_taps():
    pfb = _pfb()
    taps = pfb.read_fir_filter_coeff(pfb.config.config_dir + "/PST_filtertaps.txt")
    taps.setflags(write=False)
    return taps


def _noise(seed, shape):
    rng = np.random.default_rng(seed)
    x = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)
    x.setflags(write=False)
    return x


def _cu(gpu):
    import torch
    return torch.cuda.get_device_properties(gpu).multi_processor_count


# ----------------------------------------------------------------- the launchers' ranges
def _ceil(a, b):
    return -(-a // b)


def _steps(rows, nu):
    """16-row steps of `rows` output rows: QS = 16 / nu rows of each residue per step
    (launch_stream: n_steps = ceil(ceil(K / NU) / QS))."""
    return _ceil(_ceil(rows, nu), 16 // nu)


RANGES = {
    # csrc/pfb_analysis.hip, launch_stream: per_pol = max(1, 2 CU / n_pol), wgs = min(n_steps, per_pol)
    "stream": lambda cu, s, n: min(n, max(1, 2 * cu // s)),
    # csrc/pfb_synth_wave.hip, launch_wave_t: max(1, 3 CU / (N/16 n_pol)), capped at n_blocks
    "wave": lambda cu, s, n, N: min(n, max(1, 3 * cu // (N // 16 * s))),
    # csrc/pfb_synth_wave512.hip, launch_w5: ceil(2 (3 CU) / (N/8 n_pol)), capped at n_blocks
    "wave512": lambda cu, s, n, N: min(n, max(1, _ceil(6 * cu, N // 8 * s))),
    # csrc/pfb_synth.hip, launch_sb (persistent branch): max(1, CU per_cu / (groups n_pol)) with
    # per_cu = min(512 / threads, 160 KB / LDS bytes) <= 4 — the bound below is the largest count
    # any per_cu gives; more than 16 blocks per range would switch to ranges of ~18 blocks
    "block": lambda cu, s, n, groups: min(n, max(1, 4 * cu // (groups * s))),
    # csrc/pfb_analysis.hip, launch_fir_window_t: ceil(4096 / (N/256 nu n_pol)) ranges per residue
    "firwin": lambda cu, s, n, N, nu: max(1, _ceil(4096, N // 256 * nu * s)),
}


def _split(n, nw):
    """Sizes of the kernels' ranges [n w / nw, n (w + 1) / nw)."""
    return [n * (w + 1) // nw - n * w // nw for w in range(nw)]


def _assert_partition(regime, n, nw, what):
    """The precondition of a case (a condition, not a skip): `n` steps / blocks / rows over
    `nw` ranges run the loop-carried code in the claimed regime."""
    sizes = _split(n, nw)
    print(f"{what}: {n} over {nw} ranges -> {sizes}")
    assert max(sizes) >= 2, f"{what}: no range of {sizes} holds two steps — the shape no longer forces the loop"
    if regime == "one":
        assert nw == 1, f"{what}: {nw} ranges, the case claims one workgroup for all {n}"
    elif regime == "three":
        assert nw == 3 and min(sizes) >= 2 and len(set(sizes)) > 1, (
            f"{what}: ranges {sizes}, the case claims three uneven ranges of two or more")
    else:  # "many": several uneven ranges of two or more each
        assert nw > 1 and min(sizes) >= 2 and len(set(sizes)) > 1, f"{what}: ranges {sizes}"


def _assert_single(n, nw, what):
    """The n_pol = 3 twin runs one step or block per workgroup."""
    assert max(_split(n, nw)) == 1, f"{what}: the n_pol 3 plan is not partitioned one per workgroup"


# ----------------------------------------------------------------- series and comparisons
def _expand(base_d, S):
    """x[p] = base[p % 3] on the device."""
    import torch
    idx = torch.arange(S, device=base_d.device) % 3
    return base_d[idx].contiguous()


def _bits(t):
    import torch
    return torch.view_as_real(t).view(torch.int32)  # (a view, also of a row-sliced buffer)


def _assert_series_repeat(out, what):
    """out[p] bit-identical to out[p % 3], compared on the device (no copy of `out`)."""
    b = _bits(out)
    assert out.shape[0] > 3
    for r in range(3):
        assert bool((b[r::3] == b[r]).all()), f"{what}: a series with p % 3 == {r} differs from series {r}"


def _assert_same_bits(a, b, what):
    import torch
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), what


# ----------------------------------------------------------------- the kernel that ran
class _Launches:
    """Kernel names and launch records of the C ABI's profiler classes."""

    def __init__(self, lib):
        self.lib = lib

    def reset(self):
        assert self.lib.pfb_profile_reset() == 0

    def name(self, which):
        buf = ctypes.create_string_buffer(1024)
        assert self.lib.pfb_profile_kernel_name(which, buf, len(buf)) == 0
        return buf.value.decode()

    def records(self, which):
        n = ctypes.c_int64()
        assert self.lib.pfb_profile_read(which, None, ctypes.byref(n), None) == 0
        return n.value

    def assert_kernel(self, which, expect, threads=None):
        """The class's last single launch was pfb::<expect...> (`expect`: the template name
        with its leading template arguments, `threads` the last one)."""
        name = self.name(which)
        print(f"class {which}: {name}")
        head = "void pfb::" + expect
        assert name.startswith(head) and name[len(head)] in ",>", (
            f"class {which} ran {name!r}, the case claims {expect!r}")
        if threads is not None:
            assert f", {threads}>(" in name, f"class {which} ran {name!r}, the case claims {threads} threads"
        self.reset()

    def assert_multi_launch(self, which):
        """The class ran as one multi-launch record: no single-kernel name."""
        name, n = self.name(which), self.records(which)
        assert name == "" and n == 1, (
            f"class {which}: {n} records, single-kernel name {name!r}; the case claims one "
            "multi-launch path")
        self.reset()


@pytest.fixture
def launches(gpu):
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    assert lib.pfb_profile_reset() == 0
    assert lib.pfb_profile_enable(1) == 0
    try:
        yield _Launches(lib)
    finally:
        lib.pfb_profile_enable(0)
        lib.pfb_profile_reset()


def _bool(v):
    return "true" if v else "false"


# =============================================================== A. streaming analysis, N 256
ROWS = 107  # 7 steps of 16 rows, the last one partial


def _series_count(cu, regime):
    """A / B: per_pol = max(1, 2 CU / S) is 1 from S = 2 CU + 1 on and 3 at S = 2 CU / 3."""
    return 2 * cu + 1 if regime == "one" else 2 * cu // 3


@functools.lru_cache(maxsize=None)
def _ana_ref(os_, tpc):
    """Input of ROWS rows plus a ragged tail, and its oracle product (shared, read-only)."""
    nu, de = _rat(os_)
    taps = _taps(256, os_, tpc)
    P = -(-len(taps) // 256)
    base = _noise(SEED + 10 * tpc + nu, (3, P * 256 + ROWS * (256 * de // nu) + 11))
    ref = orc.polyphase_analysis(base[:, None, :], taps, 256, os_)
    assert ref.shape == (3, 256, ROWS)
    ref.setflags(write=False)
    return base, ref


STREAM_CASES = [("8/7", 12), ("8/7", 11), ("4/3", 12), ("4/3", 11)]  # tpc 12 / 11: 13 / 12 phases
_stream_ids = lambda c: f"{c[0].replace('/', 'over')}-tpc{c[1]}"  # noqa: E731


def _stream_kernel(os_, tpc):
    nu, de = _rat(os_)
    return f"analysis_stream_kernel<256, {tpc + 1}, {nu}, {de}, 0, false, 0"


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_stream_ids)
def test_stream_analysis_multi_step(gpu, launches, case, regime):
    """AnalysisPlan.execute, stateless: the plain-store streaming kernel behind
    pfb_analysis_execute, 8/7 and 4/3 with 13 and 12 phases."""
    import torch
    pfb = _pfb()
    os_, tpc = case
    nu, _ = _rat(os_)
    cu = _cu(gpu)
    S = _series_count(cu, regime)
    steps = _steps(ROWS, nu)
    assert steps == 7 and ROWS % 16
    _assert_partition(regime, steps, RANGES["stream"](cu, S, steps), f"stream {case} S {S}")
    _assert_single(steps, RANGES["stream"](cu, 3, steps), f"stream {case}")
    base, ref = _ana_ref(os_, tpc)
    taps = _taps(256, os_, tpc)
    base_d = torch.from_numpy(base.copy()).to(gpu)  # (the shared array is read-only)
    plan = pfb.AnalysisPlan(taps, 256, os_, "polyphase_analysis", S, 0)
    launches.reset()
    out = plan.execute(_expand(base_d, S))
    launches.assert_kernel(0, _stream_kernel(os_, tpc))
    assert out.shape == (S, ROWS, 256)
    assert_pfb_close(out[:3].cpu().numpy().transpose(0, 2, 1), ref, what=f"stream {case} {regime}")
    _assert_series_repeat(out, f"stream {case} {regime}")
    twin = pfb.AnalysisPlan(taps, 256, os_, "polyphase_analysis", 3, 0)
    _assert_same_bits(out[:3], twin.execute(base_d), f"stream {case} {regime}: S {S} vs n_pol 3")
    plan.close()
    twin.close()


def _stream_chunks(plan, twin, chunks_d, S, cu, regime, nu, win_lo, win_hi, M, kernel, launches, what):
    """execute(stateful=True) over the chunks: per-call preconditions from the table, the rows
    of both plans; returns ([rows of plan], [rows of twin], [carries before each call])."""
    outs, outs3, carries = [], [], []
    for i, c in enumerate(chunks_d):
        B = plan.buffered_samples
        assert B == twin.buffered_samples
        carries.append(B)
        rows = plan.stream_rows(c.shape[1])
        steps = _steps(rows, nu)
        _assert_partition(regime, steps, RANGES["stream"](cu, S, steps), f"{what} chunk {i} ({rows} rows)")
        _assert_single(steps, RANGES["stream"](cu, 3, steps), f"{what} chunk {i}")
        if i and win_lo is not None:
            # the one-launch carry path of filterbank_exec (its one-launch path): the carried samples
            # lie in the kernel's first window (read through AnalysisArgs::pre), more of them
            # than P N, and the kernel copies the next carry itself (carry_out)
            assert win_lo < B <= win_hi and rows * M >= B, (i, B, win_lo, win_hi)
        launches.reset()
        y = plan.execute(_expand(c, S), stateful=True)
        launches.assert_kernel(0, kernel)
        assert y.shape[1] == rows
        outs.append(y)
        outs3.append(twin.execute(c, stateful=True))
    return outs, outs3, carries


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("case", STREAM_CASES, ids=_stream_ids)
def test_stream_analysis_multi_step_stateful(gpu, launches, case, regime):
    """execute(stateful=True) on device input over three chunks whose carries exceed P N: the
    one-launch path — carry descriptor (`pre`) in the first window of a workgroup that then
    runs further steps, and the in-kernel copy of the next carry (`carry_out`) — against
    FilterBankOracle, the one-shot call and the n_pol 3 plan."""
    import torch
    pfb = _pfb()
    os_, tpc = case
    nu, de = _rat(os_)
    cu = _cu(gpu)
    S = _series_count(cu, regime)
    taps = _taps(256, os_, tpc)
    M, P = 256 * de // nu, tpc + 1
    lens = (P * 256 + ROWS * M + 11, ROWS * M + 37, ROWS * M + 5)
    base = _noise(SEED + 100 + 10 * tpc + nu, (3, sum(lens)))
    base_d = torch.from_numpy(base.copy()).to(gpu)  # (the shared array is read-only)
    cuts = np.cumsum((0,) + lens)
    chunks_d = [base_d[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    plan = pfb.AnalysisPlan(taps, 256, os_, "polyphase_analysis", S, 0)
    twin = pfb.AnalysisPlan(taps, 256, os_, "polyphase_analysis", 3, 0)
    what = f"stateful stream {case} {regime}"
    outs, outs3, carries = _stream_chunks(plan, twin, chunks_d, S, cu, regime, nu, P * 256,
                                          (de * 16 // nu + P) * 256, M, _stream_kernel(os_, tpc), launches, what)
    ofb = orc.FilterBankOracle(taps, 256, os_)
    whole = pfb.AnalysisPlan(taps, 256, os_, "polyphase_analysis", 3, 0).execute(base_d)
    r0 = 0
    for i, (y, y3) in enumerate(zip(outs, outs3)):
        ref = ofb.execute(base[:, None, cuts[i]:cuts[i + 1]])
        assert ref.shape == (3, 256, y.shape[1]), (i, ref.shape, y.shape)
        assert_pfb_close(y[:3].cpu().numpy().transpose(0, 2, 1), ref, what=f"{what} chunk {i}")
        _assert_series_repeat(y, f"{what} chunk {i}")
        _assert_same_bits(y[:3], y3, f"{what} chunk {i}: S {S} vs n_pol 3")
        _assert_same_bits(y[:3], whole[:, r0:r0 + y.shape[1]], f"{what} chunk {i}: vs the one-shot call")
        r0 += y.shape[1]
    assert plan.buffered_samples == twin.buffered_samples == ofb.buffered_samples
    assert carries[0] == 0 and min(carries[1:]) > P * 256
    plan.close()
    twin.close()


# =============================================================== B. LowCBF filterbank
LOWCBF_KERNEL = "analysis_stream_kernel<256, 12, 4, 3, 0, true"


class _LowCbfOracle(orc.FilterBankOracle):
    """FilterBank.m around polyphase_analysis_lowcbf.m: the 1536 zeros before the first call."""

    def __init__(self, taps):
        super().__init__(taps, 256, "4/3")
        self.first = True
        self.pfb_analysis = self._call

    def _call(self, x, filt, n_chan, os_factor):
        y = orc.polyphase_analysis_lowcbf(x, filt, do_padding=self.first)
        self.first = False
        return y


@pytest.mark.parametrize("regime", REGIMES)
def test_lowcbf_multi_step(gpu, launches, regime):
    """The LowCBF filterbank's production path, analysis_stream_kernel<256, 12, 4, 3, 0, true>
    (launch_lowcbf forwards to launch_lowcbf_stream): the plan's first call pre-padded with
    1536 zeros (107 rows), the second on the same input not (99 rows), 7 steps each."""
    import torch
    pfb = _pfb()
    cu = _cu(gpu)
    S = _series_count(cu, regime)
    taps = _pst_taps()
    base = _noise(SEED + 200, (3, 3072 - 1536 + 192 * ROWS + 11))
    base_d = torch.from_numpy(base.copy()).to(gpu)  # (the shared array is read-only)
    x = _expand(base_d, S)
    plan = pfb.AnalysisPlan(taps, 256, "4/3", "polyphase_analysis_lowcbf", S, 0)
    twin = pfb.AnalysisPlan(taps, 256, "4/3", "polyphase_analysis_lowcbf", 3, 0)
    assert plan.out_chan == 216
    for call, rows in enumerate((ROWS, ROWS - 8)):
        what = f"lowcbf {regime} call {call}"
        steps = _steps(rows, 4)
        assert steps == 7 and rows % 16 and plan.output_length(base.shape[1]) == rows
        _assert_partition(regime, steps, RANGES["stream"](cu, S, steps), what)
        _assert_single(steps, RANGES["stream"](cu, 3, steps), what)
        launches.reset()
        out = plan.execute(x)
        launches.assert_kernel(0, LOWCBF_KERNEL)
        ref = orc.polyphase_analysis_lowcbf(base[:, None, :], taps, do_padding=(call == 0))
        assert ref.shape == (3, 216, rows) and out.shape == (S, rows, 216)
        assert_pfb_close(out[:3].cpu().numpy().transpose(0, 2, 1), ref, what=what)
        _assert_series_repeat(out, what)
        _assert_same_bits(out[:3], twin.execute(base_d), what + f": S {S} vs n_pol 3")
    plan.close()
    twin.close()


@pytest.mark.parametrize("regime", REGIMES)
def test_lowcbf_multi_step_stateful(gpu, launches, regime):
    """A fresh LowCBF plan, execute(stateful=True) over three chunks (nu-trim to multiples of
    4 and the carried samples, as FilterBank.m does) against the streaming oracle."""
    import torch
    pfb = _pfb()
    cu = _cu(gpu)
    S = _series_count(cu, regime)
    taps = _pst_taps()
    lens = (3072 - 1536 + 192 * ROWS + 11, 192 * ROWS + 37, 192 * ROWS + 5)
    base = _noise(SEED + 201, (3, sum(lens)))
    base_d = torch.from_numpy(base.copy()).to(gpu)  # (the shared array is read-only)
    cuts = np.cumsum((0,) + lens)
    chunks_d = [base_d[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    plan = pfb.AnalysisPlan(taps, 256, "4/3", "polyphase_analysis_lowcbf", S, 0)
    twin = pfb.AnalysisPlan(taps, 256, "4/3", "polyphase_analysis_lowcbf", 3, 0)
    what = f"stateful lowcbf {regime}"
    outs, outs3, _ = _stream_chunks(plan, twin, chunks_d, S, cu, regime, 4, None, None, 192, LOWCBF_KERNEL,
                                    launches, what)
    ofb = _LowCbfOracle(taps)
    for i, (y, y3) in enumerate(zip(outs, outs3)):
        ref = ofb.execute(base[:, None, cuts[i]:cuts[i + 1]])
        assert ref.shape == (3, 216, y.shape[1]), (i, ref.shape, y.shape)
        assert_pfb_close(y[:3].cpu().numpy().transpose(0, 2, 1), ref, what=f"{what} chunk {i}")
        _assert_series_repeat(y, f"{what} chunk {i}")
        _assert_same_bits(y[:3], y3, f"{what} chunk {i}: S {S} vs n_pol 3")
    assert plan.buffered_samples == twin.buffered_samples == ofb.buffered_samples
    plan.close()
    twin.close()


# =============================================================== C. fused round trip
BLOCKS = 7
NF, OV, KEEP = 256, 48, 160
RT_ROWS = BLOCKS * KEEP + 2 * OV + 5  # 7 synthesis blocks and a ragged tail


@functools.lru_cache(maxsize=None)
def _rt_ref(os_, tpc):
    nu, de = _rat(os_)
    taps = _taps(256, os_, tpc)
    P = tpc + 1
    base = _noise(SEED + 300 + 10 * tpc + nu, (3, P * 256 + RT_ROWS * (256 * de // nu) + 11))
    chan = orc.polyphase_analysis(base[:, None, :], taps, 256, os_)
    assert chan.shape == (3, 256, RT_ROWS)
    out = orc.polyphase_synthesis(chan, 1, NF, os_, {"apply_deripple": 1, "filter_coeff": taps}, 1, OV,
                                  orc.pfb_window("tukey", NF, OV))
    assert out.shape == (3, 1, BLOCKS * KEEP * de // nu * 256)
    chan.setflags(write=False)
    out.setflags(write=False)
    return base, chan, out


@pytest.mark.parametrize("case", [("4/3", 12), ("4/3", 11), ("8/7", 11)], ids=_stream_ids)
def test_roundtrip_multi_block(gpu, launches, case):
    """pfb_roundtrip_execute, N 256, Nf 256, Ov 48, tukey, deripple on, sample offset 1, with
    3 CU / 16 + 1 series: ONE block range per series and phase group in the wave kernel (all 7
    blocks in one workgroup) and about ten uneven step ranges per series in the analysis.
    Stored rows (the analysis' zblk 2 variant + the wave kernel), recomputed rows (the wave
    kernel's FIR variants), and the chunked pipeline with set_chunk_blocks(3)."""
    import torch
    pfb = _pfb()
    os_, tpc = case
    nu, de = _rat(os_)
    cu = _cu(gpu)
    S = 3 * cu // 16 + 1
    what = f"round trip {case} S {S}"
    _assert_partition("one", BLOCKS, RANGES["wave"](cu, S, BLOCKS, 256), what + " wave")
    _assert_single(BLOCKS, RANGES["wave"](cu, 3, BLOCKS, 256), what + " wave")
    steps = _steps(RT_ROWS, nu)
    _assert_partition("many", steps, RANGES["stream"](cu, S, steps), what + " analysis")
    _assert_single(steps, RANGES["stream"](cu, 3, steps), what + " analysis")
    base, ref_chan, ref_out = _rt_ref(os_, tpc)
    taps = _taps(256, os_, tpc)
    base_d = torch.from_numpy(base.copy()).to(gpu)  # (the shared array is read-only)
    x = _expand(base_d, S)
    rw = 14 if os_ == "8/7" else 12

    def run(xin, n_pol, mode, chunk=0, pin=False):
        ana = pfb.AnalysisPlan(taps, 256, os_, "polyphase_analysis", n_pol, 0)
        syn = pfb.SynthesisPlan(256, os_, NF, OV, True, 1, True, taps, "tukey", None, n_pol, 0)
        syn.set_stage1_rows(mode)
        if chunk:
            syn.set_chunk_blocks(chunk)
        launches.reset()
        chan, out = pfb.roundtrip(ana, syn, xin, sample_offset=1)
        torch.cuda.synchronize()
        if not chunk:
            assert syn.last_stage1_rows == mode
        if pin:
            launches.assert_kernel(2, f"synth_wave_kernel<{rw}, true, 10")
        ana.close()
        syn.close()
        return chan, out

    fused = {}
    for mode in ("stored", "recomputed"):
        w = f"{what} {mode}"
        chan, out = run(x, S, mode, pin=True)
        assert chan.shape == (S, RT_ROWS, 256) and out.shape == (S, ref_out.shape[2])
        assert_pfb_close(chan[:3].cpu().numpy().transpose(0, 2, 1), ref_chan, what=w + " chan")
        assert_pfb_close(out[:3].cpu().numpy()[:, None, :], ref_out, scale=1.0, what=w + " out (raw)")
        _assert_series_repeat(chan, w + " chan")
        _assert_series_repeat(out, w + " out")
        chan3, out3 = run(base_d, 3, mode)
        _assert_same_bits(chan[:3], chan3, w + f" chan: S {S} vs n_pol 3")
        _assert_same_bits(out[:3], out3, w + f" out: S {S} vs n_pol 3")
        fused[mode] = (chan[:3].clone(), out[:3].clone())
        del chan, out
    # the recomputed rows are the same FIR sums in the same order: bit-identical round trips
    _assert_same_bits(fused["stored"][0], fused["recomputed"][0], what + " chan: stored vs recomputed")
    _assert_same_bits(fused["stored"][1], fused["recomputed"][1], what + " out: stored vs recomputed")
    # chunked pipeline: separate analysis and synthesis kernels, 3 + 3 + 1 blocks
    w = what + " chunked"
    chan, out = run(x, S, "stored", chunk=3)
    _assert_same_bits(chan[:3], fused["stored"][0], w + " chan vs fused")
    assert_pfb_close(out[:3].cpu().numpy(), fused["stored"][1].cpu().numpy(), scale=1.0, what=w + " out vs fused (raw)")
    assert_pfb_close(chan[:3].cpu().numpy().transpose(0, 2, 1), ref_chan, what=w + " chan")
    assert_pfb_close(out[:3].cpu().numpy()[:, None, :], ref_out, scale=1.0, what=w + " out (raw)")
    _assert_series_repeat(chan, w + " chan")
    _assert_series_repeat(out, w + " out")
    chan3, out3 = run(base_d, 3, "stored", chunk=3)
    _assert_same_bits(chan[:3], chan3, w + f" chan: S {S} vs n_pol 3")
    _assert_same_bits(out[:3], out3, w + f" out: S {S} vs n_pol 3")


# =============================================================== D-F. stand-alone synthesis
SO = 3  # sample offset (1-based first row)


@functools.lru_cache(maxsize=None)
def _synth_ref(N, nf, ov, os_, spans, taper):
    """Channelised noise (3, rows, N) of 7 blocks and a ragged tail, and its oracle output."""
    keep = nf - 2 * ov
    base = _noise(SEED + 400 + 7 * N + nf + ov, (3, (SO - 1) + BLOCKS * keep + 2 * ov + 5, N))
    taps = _taps(N, os_, 12)
    ref = orc.polyphase_synthesis(base.transpose(0, 2, 1), spans, nf, os_,
                                  {"apply_deripple": 1, "filter_coeff": taps}, SO, ov,
                                  orc.pfb_window(taper, nf, ov))
    nu, de = _rat(os_)
    assert ref.shape == (3, 1, BLOCKS * keep * de * N // nu)
    ref.setflags(write=False)
    return base, ref


def _synth_case(gpu, launches, N, nf, ov, os_, spans, taper, S, kernel, what, threads=None):
    import torch
    pfb = _pfb()
    base, ref = _synth_ref(N, nf, ov, os_, spans, taper)
    taps = _taps(N, os_, 12)
    base_d = torch.from_numpy(base.copy()).to(gpu)  # (the shared array is read-only)
    plan = pfb.SynthesisPlan(N, os_, nf, ov, bool(spans), 1, True, taps, taper, None, S, 0)
    launches.reset()
    out = plan.execute(_expand(base_d, S), sample_offset=SO, layout="ptc")
    launches.assert_kernel(2, kernel, threads)
    assert out.shape == (S, ref.shape[2])
    assert_pfb_close(out[:3].cpu().numpy()[:, None, :], ref, what=what)
    _assert_series_repeat(out, what)
    twin = pfb.SynthesisPlan(N, os_, nf, ov, bool(spans), 1, True, taps, taper, None, 3, 0)
    _assert_same_bits(out[:3], twin.execute(base_d, sample_offset=SO, layout="ptc"), what + f": S {S} vs n_pol 3")
    plan.close()
    twin.close()


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("taper", ["tukey", "hann"])  # the flat-window and the general kernel
@pytest.mark.parametrize("spans", [1, 0])
@pytest.mark.parametrize("os_", ["8/7", "4/3"])
def test_wave_synthesis_multi_block(gpu, launches, os_, spans, taper, regime):
    """SynthesisPlan.execute, N 256, Nf 256, Ov 48: the wave kernel on stored rows (RW 14 and
    12, SPANS, flat and general window) with 7 blocks in one range, or 2 + 2 + 3 in three."""
    cu = _cu(gpu)
    S = 3 * cu // 16 + 1 if regime == "one" else 3 * cu // (16 * 3)
    what = f"wave {os_} spans {spans} {taper} {regime} S {S}"
    _assert_partition(regime, BLOCKS, RANGES["wave"](cu, S, BLOCKS, 256), what)
    _assert_single(BLOCKS, RANGES["wave"](cu, 3, BLOCKS, 256), what)
    rw = 14 if os_ == "8/7" else 12
    _synth_case(gpu, launches, 256, NF, OV, os_, spans, taper, S, f"synth_wave_kernel<{rw}, {_bool(spans)}, 10", what)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("taper", ["tukey", "hann"])
@pytest.mark.parametrize("spans", [1, 0])
def test_wave512_synthesis_multi_block(gpu, launches, spans, taper, regime):
    """N 64, Nf 512, Ov 128, 8/7: the Nf 512 wave kernel, 8 phase groups per series."""
    cu = _cu(gpu)
    S = _ceil(6 * cu, 8) if regime == "one" else 70 * cu // 256
    what = f"wave512 spans {spans} {taper} {regime} S {S}"
    _assert_partition(regime, BLOCKS, RANGES["wave512"](cu, S, BLOCKS, 64), what)
    _assert_single(BLOCKS, RANGES["wave512"](cu, 3, BLOCKS, 64), what)
    _synth_case(gpu, launches, 64, 512, 128, "8/7", spans, taper, S, f"synth_wave512_kernel<{_bool(spans)}", what)


# (Nf, W, N, os, Ov, PAIRS, DK, threads)
BLOCK_ROWS = [
    (128, 96, 8, "4/3", 16, 1, 6, 128),      # overlap reuse
    (128, 96, 16, "4/3", 8, 8, 0, 128),      # no reuse
    (1024, 896, 8, "8/7", 128, 4, 0, 256),   # 256 threads
]


@pytest.mark.parametrize("spans", [1, 0])
@pytest.mark.parametrize("row", BLOCK_ROWS, ids=lambda r: f"Nf{r[0]}-N{r[2]}-Ov{r[4]}")
def test_block_synthesis_one_range(gpu, launches, row, spans):
    """The block kernel's persistent branch with ONE range walking every block of a series
    (the shape the inverse cascades produce): the other extreme of dispatch-matrix family E."""
    nf, W, N, os_, ov, pairs, dk, threads = row
    cu = _cu(gpu)
    groups = N // (2 * pairs)  # launch_sb
    S = 4 * cu // groups + 1
    what = f"block kernel {row} spans {spans} S {S}"
    _assert_partition("one", BLOCKS, RANGES["block"](cu, S, BLOCKS, groups), what)
    # (n_pol 3: at least CU / (3 groups) ranges whatever per_cu is — one block each)
    assert max(1, cu // (groups * 3)) >= BLOCKS
    _synth_case(gpu, launches, N, nf, ov, os_, spans, "tukey", S,
                f"synth_block_kernel<{nf}, {W}, {pairs}, {_bool(spans)}, true, {dk}", what, threads)


# =============================================================== G. register-window FIR
@pytest.mark.parametrize("regime", REGIMES)
def test_fir_window_multi_row(gpu, launches, regime):
    """N 512, 32/27, 28 taps per channel (random), Bunton: fir_window_kernel<32, 27, kBunton>
    (the only register-window FIR of a release build) + row FFT, 32 * 7 + 5 rows — 7 or 8 rows
    per residue, walked by one workgroup per column slice (64 series) or split 2, 2, 3 (22)."""
    import torch
    pfb = _pfb()
    N, os_, tpc, nu, M = 512, "32/27", 28, 32, 432
    rows = nu * 7 + 5
    S = 64 if regime == "one" else 22
    cu = _cu(gpu)
    what = f"fir window {regime} S {S}"
    nw, nw3 = RANGES["firwin"](cu, S, rows, N, nu), RANGES["firwin"](cu, 3, rows, N, nu)
    per_residue = sorted({_ceil(rows - s, nu) for s in range(nu)})
    assert per_residue == [7, 8]
    _assert_partition(regime, 7, nw, what)
    _assert_partition(regime if regime == "one" else "many", 8, nw, what)
    _assert_single(8, nw3, what)
    taps = _taps(N, os_, tpc)
    P = -(-len(taps) // N)
    assert P == 29
    base = _noise(SEED + 500, (3, P * N + rows * M + 11))
    ref = orc.polyphase_analysis(base[:, None, :], taps, N, os_)
    assert ref.shape == (3, N, rows)
    base_d = torch.from_numpy(base.copy()).to(gpu)  # (the shared array is read-only)
    plan = pfb.AnalysisPlan(taps, N, os_, "polyphase_analysis", S, 0)
    launches.reset()
    out = plan.execute(_expand(base_d, S))
    launches.assert_multi_launch(0)
    assert out.shape == (S, rows, N)
    assert_pfb_close(out[:3].cpu().numpy().transpose(0, 2, 1), ref, what=what)
    _assert_series_repeat(out, what)
    twin = pfb.AnalysisPlan(taps, N, os_, "polyphase_analysis", 3, 0)
    _assert_same_bits(out[:3], twin.execute(base_d), what + f": S {S} vs n_pol 3")
    plan.close()
    twin.close()
