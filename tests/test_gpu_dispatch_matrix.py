"""Oracle parity of every kernel instantiation the dispatch code can reach but no other
test launches: one case per reachable cell, at the smallest shape that reaches it.

Every case: two polarisations, complex noise from a fixed seed, a ragged length (not a
multiple of M, N or keep), more than one workgroup or block range, through the public
Python API, against oracle.pfb_oracle with conftest.assert_pfb_close at the project's 1e-6.

The cell is pinned, not only the shape: the module-local ``launches`` fixture enables the
C ABI's profiler (pfb_profile_enable / pfb_profile_kernel_name, _lib.py), which records the
demangled name of the last single-kernel launch of class 0 (analysis), 1 (channel IFFT)
and 2 (block or wave kernel); each case asserts the template and the leading template
arguments it claims to cover.  Paths of several launches record no name (ProfScope,
pfb_host.hpp, single = false): the non-fused analysis (FIR + row FFT: families B and C) and
the spectral-taper synthesis (six launches per polarisation: family F).  Their cases
assert exactly that — one multi-launch record in the class and no single-kernel name, i.e.
neither the fused analysis kernel nor the channel-IFFT / block / wave kernels ran — and
cite the dispatch lines, which switch on the shape alone.

Taps: design_PFB_FIR_filter(N, os, tpc) gives N tpc + 1 taps, so P = tpc + 1; where the
host design takes seconds (more than 8192 taps) the taps are rng.standard_normal(n) / N,
as in test_analysis_4096_persistent_row_fft ("random" below).

Cell -> dispatch line -> case (csrc/ file : function)

A. Fused analysis, pfb_analysis.hip : launch_fused_p / launch_analysis N switch.
   Input length P N + R M + 3 with R = max(150, 8192 / N + 22) rows (at least three
   workgroups of T = 4096 / N rows).  Name: analysis_fused_kernel<N, PMAX, variant, 1, EXACT>.
     N 32   8/7   tpc 12  both     exact P 13, the N = 32 case of the switch
     N 128  4/3   tpc 11  both     exact P 12, the N = 128 case of the switch
     N 16   8/7   tpc 10  padded   exact P 11
     N 256  8/7   tpc 11  padded   N 256 fused (stream_shape declines the padded variant)
     N 256  32/27 tpc 12  bunton   N 256 fused (stream_shape declines 32/27)
     N 64   8/7   tpc 15  both     PMAX 16 clamped, P 16
     N 128  8/7   tpc 13  bunton   PMAX 16 clamped, P 14
     N 32   4/3   tpc 5 cut to 4 N taps  padded   PMAX 16, P 4, tap count a multiple of N
     N 128  32/27 tpc 16  padded   PMAX 32, P 17
     N 8    8/7   tpc 31  bunton   PMAX 32, P 32
     N 16   5/3   random 12 N + 1  both   M = floor(N de / nu) = 9, nu M != de N (the padded
                                          barrel index is ((nu - k mod nu)(N - M)) mod N, not (M k) mod N)
B. Non-fused, N <= 256, pfb_analysis.hip : analysis_supported clears `fused` for P > 32;
   launch_analysis then runs fir_generic_kernel + row_fft_kernel<N, -1 / +1> through the
   plan's scratch.  Same input length as A.  Two launches: no name.
     N 8    8/7   tpc 40  bunton
     N 64   4/3   tpc 33  padded
     N 256  8/7   tpc 33  bunton  (random taps)
C. Generic path, N >= 512, pfb_analysis.hip : launch_fir_window_de / fir_window_applies /
   launch_analysis; 40 output rows (P N + 40 M + 3 samples).  Two launches: no name.
     N 512  8/7   tpc 15  bunton   fir_lds_kernel PW 16, DE 7
     N 1024 4/3   tpc 13  padded   fir_lds_kernel PW 16, DE 3 (random taps)
     N 512  4/3   tpc 28  padded   fir_lds_kernel PW 32, DE 3 (random taps)
     N 512  4/3   tpc 12  bunton   fir_lds_kernel PW 13, DE 3, Bunton
     N 512  8/7   tpc 24  bunton   fir_lds_kernel PW 25, DE 7, Bunton (random taps)
     N 512  32/27 tpc 28  bunton   fir_window_kernel<32, 27, kBunton> (random taps)
     N 512  32/27 tpc 12  bunton   fir_generic_kernel<kBunton>, P 13 < DE 27
     N 512  16/15 tpc 12  bunton   fir_generic_kernel, de 15 has no window instance
     N 512  8/7   tpc 33  padded   fir_generic_kernel, P 34 > 32 (random taps)
     N 512  5/3   random 12 N + 1  both   fir_generic_kernel, M = 307 with a remainder
     N 2048 8/7   random 12 N + 1  bunton   row_fft_kernel<2048, -1>
     N 2048 4/3   random 12 N + 1  padded   row_fft_kernel<2048, +1>
D. Stage-1 channel IFFT, pfb_rowfft.hip : dispatch_row_fft<+1> / launch_row_fft.  Nf 128,
   Ov 16, 8/7, spans 1, sample offset 3, three blocks and a ragged tail, tukey.
   Name (class 1): row_fft_kernel<N, 1, PERM, GAIN>.
     every N of mixed_chan_supported (pfb_common.hpp): 14 28 56 112 192 216 224 384 432
       448 768 864 896 1536 1792 3072 3584, and N = 32 128 512 1024 2048
       (deripple on with designed taps for N <= 256, off above)
     N 56 and N 216: combine 2 (PERM), temporal hann (GAIN), both (PERM + GAIN)
E. Stage-2 kernels, spans 1 and 0 each, tukey, deripple on, sample offset 3.  The block
   counts leave every block range more than one block on 256 CUs (the persistent loop, its
   prefetch and the overlap reuse run).
   Block kernel, pfb_synth.hip : launch_sb_p / launch_sb.
   Name (class 2): synth_block_kernel<Nf, W, PAIRS, SPANS, true, DK, ..., threads>.
     Nf 128  W 96   N 8   4/3 Ov 16    PAIRS 1, reuse DK 6
     Nf 128  W 96   N 16  4/3 Ov 8     POPT 8, keep 112: no reuse
     Nf 1024 W 896  N 8   8/7 Ov 128   P2 4, 256 threads
     Nf 1024 W 896  N 28  8/7 Ov 128   POPT 2
     Nf 1024 W 896  N 14  8/7 Ov 256   PAIRS 1
     Nf 512  W 448  N 8   8/7 Ov 64    P2 4, 256 threads (the wave kernel declines keep 384)
     Nf 512  W 448  N 28  8/7 Ov 128   POPT 2, reuse DK 4 (the wave kernel needs N % 8 == 0)
     Nf 512  W 448  N 14  8/7 Ov 128   PAIRS 1, reuse DK 4
     Nf 256  W 224  N 8   8/7 Ov 48    PAIRS 1, reuse DK 10
     Nf 256  W 224  N 216 8/7 Ov 48    PAIRS 1 (N % 16 != 0), reuse DK 10
     Nf 256  W 192  N 8   4/3 Ov 48    PAIRS 1, reuse DK 10
   Wave kernels with a non-power-of-two number of phase groups, pfb_synth_wave.hip :
   launch_synth_wave and pfb_synth_wave512.hip : launch_synth_wave512; each also bit-
   identical between the one-chunk call and set_chunk_blocks(2).
   Name (class 2): synth_wave_kernel<RW, SPANS, 10, ...> / synth_wave512_kernel<SPANS, ...>.
     Nf 256 Ov 48   N 224 8/7   14 phase groups (RW 14)
     Nf 256 Ov 48   N 448 8/7   28 phase groups (RW 14)
     Nf 256 Ov 48   N 192 4/3   12 phase groups (RW 12)
     Nf 512 Ov 128  N 56  8/7   7 phase groups
F. Spectral taper 'hann', pfb_spectral.hip : dispatch_w_out / launch_spectral_synth (forward
   Nf row FFT, channel IFFT over N, w_out_kernel<W>); spans 1 and 0 each, tukey, deripple
   on, sample offset 3.  Six launches per polarisation: no name in class 1 or 2.
     Nf 128  4/3   Ov 16   N 8     w_out_kernel<96>
     Nf 256  32/27 Ov 16   N 8     w_out_kernel<216>
     Nf 256  8/7   Ov 48   N 8     w_out_kernel<224>
     Nf 512  8/7   Ov 128  N 8     w_out_kernel<448>, forward row FFT 512
     Nf 1024 8/7   Ov 128  N 8     w_out_kernel<896>, forward row FFT 1024
     Nf 128  8/7   Ov 16   N 14    mixed channel IFFT row_fft_kernel<14, +1> in the spectral path
     Nf 128  8/7   Ov 16   N 216   mixed channel IFFT row_fft_kernel<216, +1> in the spectral path
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

SEED = 9100
DESIGN_MAX_TAPS = 8192  # above: random taps (the host firls design takes seconds)
MIXED_N = (14, 28, 56, 112, 192, 216, 224, 384, 432, 448, 768, 864, 896, 1536, 1792, 3072, 3584)


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _rat(os_):
    nu, de = os_.split("/")
    return int(nu), int(de)


@functools.lru_cache(maxsize=None)
def _designed(N, os_, tpc):
    taps = _pfb().design_PFB_FIR_filter(N, os_, tpc)
    taps.setflags(write=False)
    return taps


def _random_taps(N, n):
    return np.random.default_rng(SEED + N + n).standard_normal(n) / N


def _taps(N, os_, spec):
    """spec: tpc (designed, or random N tpc + 1 above DESIGN_MAX_TAPS), ("cut", tpc, n):
    the first n designed taps, ("random", n)."""
    if isinstance(spec, int):
        if N * spec > DESIGN_MAX_TAPS:
            return _random_taps(N, N * spec + 1)
        return _designed(N, os_, spec)
    if spec[0] == "cut":
        return _designed(N, os_, spec[1])[:spec[2]]
    return _random_taps(N, spec[1])


def _noise(seed, shape):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) /
            np.sqrt(2)).astype(np.complex64)


# ----------------------------------------------------------------------------- the cell
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
        """The class's last single launch was pfb::<expect...>: `expect` is the template
        name with its leading (or all) template arguments, `threads` the last one."""
        name = self.name(which)
        print(f"class {which}: {name}")
        head = "void pfb::" + expect
        assert name.startswith(head) and name[len(head)] in ",>", (
            f"class {which} ran {name!r}, the case claims {expect!r}")
        if threads is not None:
            assert f", {threads}>(" in name, f"class {which} ran {name!r}, the case claims {threads} threads"

    def assert_multi_launch(self, which):
        """The class ran as one multi-launch record: no single-kernel name."""
        name, n = self.name(which), self.records(which)
        assert name == "" and n == 1, (
            f"class {which}: {n} records, single-kernel name {name!r}; the case claims one "
            "multi-launch path")


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


# ----------------------------------------------------------------------------- analysis
def _run_analysis(gpu, N, os_, taps, variant, rows):
    """GPU and oracle products of `rows` output rows' worth of noise plus a ragged tail."""
    import torch
    pfb = _pfb()
    nu, de = _rat(os_)
    M = N * de // nu
    P = -(-len(taps) // N)
    n_dat = P * N + rows * M + 3
    x = _noise(SEED + N + P, (2, 1, n_dat))
    name = "polyphase_analysis" if variant == "bunton" else "polyphase_analysis_padded"
    ref = getattr(orc, name)(x, taps, N, os_)
    assert ref.shape[2] >= rows
    got = getattr(pfb, name)(torch.from_numpy(x).to(gpu), taps, N, os_).cpu().numpy()
    return got, ref, P


def _variants(rows):
    out = []
    for r in rows:
        for v in (("bunton", "padded") if r[3] == "both" else (r[3],)):
            out.append(r[:3] + (v,) + r[4:])
    return out


def _ana_id(c):
    spec = c[2] if isinstance(c[2], int) else "-".join(str(s) for s in c[2])
    return f"N{c[0]}-{c[1].replace('/', 'over')}-taps{spec}-{c[3]}"


# (N, os, taps, variant, PMAX, EXACT)
A_CASES = _variants([
    (32, "8/7", 12, "both", 13, True),
    (128, "4/3", 11, "both", 12, True),
    (16, "8/7", 10, "padded", 11, True),
    (256, "8/7", 11, "padded", 12, True),
    (256, "32/27", 12, "bunton", 13, True),
    (64, "8/7", 15, "both", 16, False),
    (128, "8/7", 13, "bunton", 16, False),
    (32, "4/3", ("cut", 5, 4 * 32), "padded", 16, False),
    (128, "32/27", 16, "padded", 32, False),
    (8, "8/7", 31, "bunton", 32, False),
    (16, "5/3", ("random", 12 * 16 + 1), "both", 13, True),
])


@pytest.mark.parametrize("case", A_CASES, ids=_ana_id)
def test_fused_analysis_cell(gpu, launches, case):
    N, os_, spec, variant, pmax, exact = case
    taps = _taps(N, os_, spec)
    got, ref, P = _run_analysis(gpu, N, os_, taps, variant, max(150, 8192 // N + 22))
    assert (P == pmax) if exact else (P <= pmax and P not in (11, 12, 13) and (pmax == 16 or P > 16))
    launches.assert_kernel(0, f"analysis_fused_kernel<{N}, {pmax}, {0 if variant == 'bunton' else 1}, 1, "
                              f"{'true' if exact else 'false'}")
    assert_pfb_close(got, ref, what=f"fused analysis {case}")


B_CASES = [
    (8, "8/7", 40, "bunton"),
    (64, "4/3", 33, "padded"),
    (256, "8/7", 33, "bunton"),
]


@pytest.mark.parametrize("case", B_CASES, ids=_ana_id)
def test_nonfused_small_n_analysis_cell(gpu, launches, case):
    N, os_, spec, variant = case
    taps = _taps(N, os_, spec)
    got, ref, P = _run_analysis(gpu, N, os_, taps, variant, max(150, 8192 // N + 22))
    assert P > 32
    launches.assert_multi_launch(0)
    assert_pfb_close(got, ref, what=f"non-fused analysis {case}")


C_CASES = _variants([
    (512, "8/7", 15, "bunton"),
    (1024, "4/3", 13, "padded"),
    (512, "4/3", 28, "padded"),
    (512, "4/3", 12, "bunton"),
    (512, "8/7", 24, "bunton"),
    (512, "32/27", 28, "bunton"),
    (512, "32/27", 12, "bunton"),
    (512, "16/15", 12, "bunton"),
    (512, "8/7", 33, "padded"),
    (512, "5/3", ("random", 12 * 512 + 1), "both"),
    (2048, "8/7", ("random", 12 * 2048 + 1), "bunton"),
    (2048, "4/3", ("random", 12 * 2048 + 1), "padded"),
])


@pytest.mark.parametrize("case", C_CASES, ids=_ana_id)
def test_generic_analysis_cell(gpu, launches, case):
    N, os_, spec, variant = case
    taps = _taps(N, os_, spec)
    got, ref, _ = _run_analysis(gpu, N, os_, taps, variant, 40)
    launches.assert_multi_launch(0)
    assert_pfb_close(got, ref, what=f"generic analysis {case}")


# ----------------------------------------------------------------------------- synthesis
SO = 3  # sample offset (1-based first row)


def _synth_input(N, nf, ov, blocks):
    keep = nf - 2 * ov
    return _noise(SEED + 7 * N + nf + blocks, (2, N, (SO - 1) + blocks * keep + 2 * ov + 5))


def _synth_ref(x, nf, ov, os_, spans, taps, taper="tukey", spectral=None, combine=1):
    dr = {"apply_deripple": 1, "filter_coeff": taps} if taps is not None else None
    s = orc.pfb_window(spectral, nf, ov) if spectral else None
    return orc.polyphase_synthesis(x, spans, nf, os_, dr, SO, ov, orc.pfb_window(taper, nf, ov), s, combine)


def _synth_gpu(x, nf, ov, os_, spans, taps, taper="tukey", spectral=None, combine=1):
    import torch
    pfb = _pfb()
    w = pfb.PFBWindow()
    dr = {"apply_deripple": 1, "filter_coeff": taps} if taps is not None else None
    s = w.lookup[spectral](nf, ov) if spectral else None
    return pfb.polyphase_synthesis(torch.from_numpy(x).cuda(), spans, nf, os_, dr, SO, ov,
                                   w.lookup[taper](nf, ov), s, combine).cpu().numpy()


def _bool(v):
    return "true" if v else "false"


# (N, combine, temporal taper)
D_CASES = ([(n, 1, "tukey") for n in MIXED_N + (32, 128, 512, 1024, 2048)] +
           [(n, c, t) for n in (56, 216) for c, t in ((2, "tukey"), (1, "hann"), (2, "hann"))])


@pytest.mark.parametrize("case", D_CASES, ids=lambda c: f"N{c[0]}-combine{c[1]}-{c[2]}")
def test_chan_ifft_cell(gpu, launches, case):
    N, combine, taper = case
    taps = _designed(N, "8/7", 12) if N <= 256 else None
    x = _synth_input(N, 128, 16, 3)
    ref = _synth_ref(x, 128, 16, "8/7", 1, taps, taper, None, combine)
    assert ref.shape[2] == 3 * 84 * N
    got = _synth_gpu(x, 128, 16, "8/7", 1, taps, taper, None, combine)
    launches.assert_kernel(1, f"row_fft_kernel<{N}, 1, {_bool(combine > 1)}, {_bool(taper == 'hann')}>"[:-1])
    assert_pfb_close(got, ref, what=f"chan IFFT {case}")


# (Nf, W, N, os, Ov, PAIRS, DK, threads, blocks)
E_BLOCK_ROWS = [
    (128, 96, 8, "4/3", 16, 1, 6, 128, 300),
    (128, 96, 16, "4/3", 8, 8, 0, 128, 600),
    (1024, 896, 8, "8/7", 128, 4, 0, 256, 300),
    (1024, 896, 28, "8/7", 128, 2, 0, 128, 100),
    (1024, 896, 14, "8/7", 256, 1, 0, 128, 100),
    (512, 448, 8, "8/7", 64, 4, 0, 256, 300),
    (512, 448, 28, "8/7", 128, 2, 4, 128, 100),
    (512, 448, 14, "8/7", 128, 1, 4, 128, 100),
    (256, 224, 8, "8/7", 48, 1, 10, 128, 300),
    (256, 224, 216, "8/7", 48, 1, 10, 128, 12),
    (256, 192, 8, "4/3", 48, 1, 10, 128, 300),
]
E_BLOCK_CASES = [r + (s,) for r in E_BLOCK_ROWS for s in (1, 0)]


@pytest.mark.parametrize("case", E_BLOCK_CASES,
                         ids=lambda c: f"Nf{c[0]}-W{c[1]}-N{c[2]}-Ov{c[4]}-spans{c[9]}")
def test_synth_block_cell(gpu, launches, case):
    nf, W, N, os_, ov, pairs, dk, threads, blocks, spans = case
    nu, de = _rat(os_)
    assert W == nf * de // nu
    taps = _designed(N, os_, 12)
    x = _synth_input(N, nf, ov, blocks)
    ref = _synth_ref(x, nf, ov, os_, spans, taps)
    assert ref.shape[2] == blocks * (nf - 2 * ov) * de * N // nu
    got = _synth_gpu(x, nf, ov, os_, spans, taps)
    launches.assert_kernel(2, f"synth_block_kernel<{nf}, {W}, {pairs}, {_bool(spans)}, true, {dk}", threads)
    assert_pfb_close(got, ref, what=f"block kernel {case}")


# (Nf, Ov, N, os, kernel and its leading arguments before SPANS, after SPANS, blocks)
E_WAVE_ROWS = [
    (256, 48, 224, "8/7", "synth_wave_kernel<14, ", ", 10", 60),
    (256, 48, 448, "8/7", "synth_wave_kernel<14, ", ", 10", 30),
    (256, 48, 192, "4/3", "synth_wave_kernel<12, ", ", 10", 70),
    (512, 128, 56, "8/7", "synth_wave512_kernel<", "", 230),
]
E_WAVE_CASES = [r + (s,) for r in E_WAVE_ROWS for s in (1, 0)]


@pytest.mark.parametrize("case", E_WAVE_CASES, ids=lambda c: f"Nf{c[0]}-N{c[2]}-spans{c[7]}")
def test_synth_wave_cell(gpu, launches, case):
    import torch
    pfb = _pfb()
    nf, ov, N, os_, head, tail, blocks, spans = case
    groups = N // (16 if nf == 256 else 8)  # kCols / kW5Cols output phases per workgroup
    assert groups & (groups - 1), f"{groups} phase groups: a power of two"
    taps = _designed(N, os_, 12)
    x = _synth_input(N, nf, ov, blocks)
    ref = _synth_ref(x, nf, ov, os_, spans, taps)
    plan = pfb.SynthesisPlan(N, os_, nf, ov, bool(spans), 1, True, taps, "tukey", None, 2)
    xd = torch.from_numpy(x).cuda()
    one = plan.execute(xd, sample_offset=SO)
    launches.assert_kernel(2, head + _bool(spans) + tail)
    launches.reset()
    plan.set_chunk_blocks(2)
    two = plan.execute(xd, sample_offset=SO)
    launches.assert_kernel(2, head + _bool(spans) + tail)
    assert torch.equal(one, two), "set_chunk_blocks(2) differs from the one-chunk call"
    plan.close()
    assert_pfb_close(one.cpu().numpy()[:, None, :], ref, what=f"wave kernel {case}")


# (Nf, os, Ov, N, blocks)
F_ROWS = [
    (128, "4/3", 16, 8, 9),
    (256, "32/27", 16, 8, 9),
    (256, "8/7", 48, 8, 9),
    (512, "8/7", 128, 8, 9),
    (1024, "8/7", 128, 8, 9),
    (128, "8/7", 16, 14, 9),
    (128, "8/7", 16, 216, 4),
]
F_CASES = [r + (s,) for r in F_ROWS for s in (1, 0)]


@pytest.mark.parametrize("case", F_CASES,
                         ids=lambda c: f"Nf{c[0]}-{c[1].replace('/', 'over')}-N{c[3]}-spans{c[5]}")
def test_spectral_taper_cell(gpu, launches, case):
    nf, os_, ov, N, blocks, spans = case
    taps = _designed(N, os_, 12)
    x = _synth_input(N, nf, ov, blocks)
    ref = _synth_ref(x, nf, ov, os_, spans, taps, "tukey", "hann")
    got = _synth_gpu(x, nf, ov, os_, spans, taps, "tukey", "hann")
    launches.assert_multi_launch(2)
    assert launches.name(1) == "" and launches.records(1) == 0
    assert_pfb_close(got, ref, what=f"spectral taper {case}")
