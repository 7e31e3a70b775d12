"""The 32-bit offset limits of the host layer on the GPU: bases 2^32 bytes apart, and the
largest extents every accept/reject check lets through, with the first one it does not.

Every hot kernel addresses HBM through raw buffer descriptors with 32-bit byte offsets; the
host layer cuts ranges, rejects shapes or falls back to a staged path so that no offset
reaches 2^31.  The limits, restated (LIMITS / the helpers below; K_RSRC = pfb::kRsrcMaxBytes
of csrc/pfb_kernels.hpp; every shape in this module is derived from these, none is a literal):

  name           expression (accepted when true)                      csrc file : function
  strided        (64 rs + jn cs + 1) 8 <= K_RSRC  (else UNSUPPORTED)  pfb_api_analysis.hip :
                                                                      pfb_filterbank_execute_strided
  dada_in        n_pol (nbit/4) N 512 <= K_RSRC   (else STAGED)       pfb_analysis.hip : analysis_reads_dada
  fit_steps      (K_RSRC / (sstep N) - WIN) / NEW steps per range,    pfb_ana_stream.hpp : stream_grid
                 sstep = n_pol (nbit/4) for a section, 8 for cf32;
                 ranges = max(min(steps, max(1, 2 CU / n_pol)), ceil(steps / fit_steps))
  wave_dadaout   L n_pol (nbit/4) <= K_RSRC       (else STAGED)       pfb_synth_wave_dadaout.hip :
                                                                      synth_wave_dadaout_supported
  wave_fir       (n_dat + 512 N) 8 < K_RSRC       (else STORED)       pfb_synth_wave.hip : synth_wave_fir_supported
  ana_dadaout    16 C n_pol (nbit/4) <= K_RSRC    (else an error)     pfb_ana_stream_dadaout.hip : launch_stream_dadaout
                 (n_pol <= 65535, the grid's y extent, keeps it true for every plan)

Not tested: the `fit_rows` branch of launch_fir_lds_t, the `fit` branch of launch_fir_window_t
(csrc/pfb_analysis.hip) and `fit_steps` for cf32 input need one series of K_RSRC bytes per
range on top of the CU-derived range count — hundreds of GB on one card.

A. FAR BASES.  Two polarisations (or outer slices) FAR = 2^29 + 3 elements = 2^32 + 24 bytes
apart inside ONE allocation, with an odd lead (a base 8-byte but not 16-byte aligned).  A base
truncated to 32 bits lands 24 bytes into series 0, inside the same tensor: it shows as a wrong
value, a NaN or a changed guard, never as an access outside the allocation.  Inputs are
NaN outside the mapped samples, outputs one finite sentinel.  Every case: bit-identical to the
packed contiguous call, no NaN, the WHOLE frame outside the mapped regions unchanged
(compared on the device).  The frames are allocated once (class-scoped) and handed back
clean by every case.

B. LARGEST ACCEPTED EXTENTS, AND ONE BEYOND.  Many-series cases follow
tests/test_gpu_partition.py: three seeded series base[0..2], x[p] = base[p % 3] expanded on the
device; out[0:3] against oracle.pfb_oracle at 1e-6 (cf32 outputs), out[p] bit-identical to
out[p % 3], out[0:3] bit-identical to an n_pol = 3 plan.  Quantised sections: the
bit-identities are the check.

Every case asserts — and prints — the quantity that makes it meaningful (base distance,
largest offset formed, range counts, the path flag): a launcher change that empties a case
fails it.  Every case asserts at its start that the device memory it needs is free (at most
16 GiB; one stated exception, the NBIT 8 wave-synthesis limit) and frees what it allocated.
No PFB_* knob is read or set.
"""
import functools
from ctypes import byref, c_double, c_int32, c_int64, c_void_p

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

OK, UNSUPPORTED = 0, 2
DEVICE = 0
SENTINEL = complex(7.0, -7.0)
NAN = complex(float("nan"), float("nan"))
SEED = 9700
DESIGN_MAX_TAPS = 8192  # above: random taps (the host firls design takes seconds)
GIB = 1 << 30

# ------------------------------------------------------------------------- the limits
K_RSRC = 0x7FFFFFF0                      # csrc/pfb_kernels.hpp : kRsrcMaxBytes
FAR = (1 << 29) + 3                      # elements between two far bases: 2^32 + 24 bytes
NEAR_2_31 = (1 << 31) - (1 << 24)        # "within 2^24 of 2^31"
GRID_Y_MAX = 65535                       # launch_stream: dim3 grid(wgs, n_pol)

LIMITS = {
    # pfb_api_analysis.hip, pfb_filterbank_execute_strided (Bunton streaming kernel)
    "strided": lambda rs, cs, jn: (64 * rs + jn * cs + 1) * 8 <= K_RSRC,
    # pfb_analysis.hip, analysis_reads_dada
    "dada_in": lambda n_pol, nbit, N: n_pol * (nbit // 4) * N * 512 <= K_RSRC,
    # pfb_synth_wave_dadaout.hip, synth_wave_dadaout_supported
    "wave_dadaout": lambda L, n_pol, nbit: L * n_pol * (nbit // 4) <= K_RSRC,
    # pfb_synth_wave.hip, synth_wave_fir_supported
    "wave_fir": lambda n_dat, N: (n_dat + 512 * N) * 8 < K_RSRC,
    # pfb_ana_stream_dadaout.hip, launch_stream_dadaout
    "ana_dadaout": lambda C, n_pol, nbit: 16 * C * n_pol * (nbit // 4) <= K_RSRC,
}


def _largest(pred, lo=1, hi=1 << 40):
    """The largest v in [lo, hi) with pred(v) (pred is true up to a threshold, false beyond)."""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def _ceil(a, b):
    return -(-a // b)


def _stream_shape(P, nu, de):
    """pfb_ana_stream.hpp, StreamShape: (QS, NEW, WIN) — periods per 16-row step, input rows
    a step consumes, rows of the register window."""
    qs = 16 // nu
    new = de * qs
    return qs, new, new + P - 1


def _fit_steps(sstep, N, P, nu, de):
    """pfb_ana_stream.hpp, stream_grid: steps of one range that fit a descriptor."""
    _, new, win = _stream_shape(P, nu, de)
    return (K_RSRC // (sstep * N) - win) // new


def _stream_ranges(cu, S, n_steps, fit):
    """pfb_ana_stream.hpp, stream_grid: -> (CU-derived count, the launch's count)."""
    by_cu = min(n_steps, max(1, 2 * cu // S))
    return by_cu, max(by_cu, _ceil(n_steps, fit))


def _steps(rows, nu):
    return _ceil(_ceil(rows, nu), 16 // nu)


# ------------------------------------------------------------------------- small helpers
def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _lib():
    from ska_pst_dsp_model_amd import _lib as L
    return L.load()


def _err(lib):
    m = lib.pfb_last_error()
    return m.decode() if m else ""


def _rat(os_):
    nu, de = os_.split("/")
    return int(nu), int(de)


def _stream(dev):
    import torch
    return c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _cu(gpu):
    import torch
    return torch.cuda.get_device_properties(gpu).multi_processor_count


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
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def _dnoise(gpu, seed, shape):
    import torch
    return torch.from_numpy(_noise(seed, shape)).to(gpu)


def _bits(t):
    """complex64 tensor -> its int32 bit patterns (NaN payloads and signed zeros included)."""
    import torch
    return torch.view_as_real(t.contiguous()).view(torch.int32)


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _no_nan(t):
    import torch
    return not torch.isnan(torch.view_as_real(t)).any().item()


def _need(gpu, nbytes, what, budget=16 * GIB):
    """The case's memory precondition: a failure with a clear message, not a skip."""
    import torch
    assert nbytes <= budget, f"{what}: the case would hold {nbytes / GIB:.1f} GiB, the budget is {budget / GIB:.0f} GiB"
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(gpu)
    print(f"{what}: needs {nbytes / GIB:.2f} GiB, {free / GIB:.1f} of {total / GIB:.1f} GiB free")
    assert free >= nbytes, (f"{what}: needs {nbytes / GIB:.2f} GiB of device memory, only "
                            f"{free / GIB:.2f} GiB are free")


@pytest.fixture(autouse=True)
def _memory(gpu):
    import torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(gpu)
    yield
    torch.cuda.synchronize(gpu)
    print(f"peak allocation {torch.cuda.max_memory_allocated(gpu) / GIB:.2f} GiB")
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------- far frames
EXTENT = 1 << 20  # elements each far region may hold (8 MiB)


class _FarFrame:
    """Two regions FAR elements apart in one flat complex64 tensor:

        [lead 1][region 0 ... up to EXTENT][fill ..................][region 1 ... up to EXTENT][tail]

    filled with `fill` (NaN for inputs, the sentinel for outputs).  `clean()` puts the fill
    back into what a case mapped and then compares the WHOLE tensor with the fill on the
    device: the guard check and the hand-over to the next case in one pass."""

    LEAD, TAIL = 1, 5

    def __init__(self, dev, fill):
        import torch
        self.fill = fill
        n = self.LEAD + FAR + EXTENT + self.TAIL
        self.flat = torch.full((n,), fill, dtype=torch.complex64, device=dev)
        self.fill_bits = int(self._i64()[0].item())
        assert self.flat.data_ptr() % 16 == 0 and self.ptr % 16 == 8
        d = self.region(1, 1).data_ptr() - self.region(0, 1).data_ptr()
        assert d == 8 * FAR and d >= 1 << 32

    def _i64(self):
        import torch
        return torch.view_as_real(self.flat).view(torch.int64).reshape(-1)

    @property
    def ptr(self):
        return self.flat.data_ptr() + 8 * self.LEAD

    @property
    def capacity(self):
        """Elements available from `ptr`."""
        return self.flat.numel() - self.LEAD

    def region(self, p, n):
        assert 0 <= n <= EXTENT, f"a far region holds {EXTENT} elements, the case wants {n}"
        o = self.LEAD + p * FAR
        return self.flat[o:o + int(n)]

    def put(self, x):
        """x: (2, n) device tensor."""
        for p in range(2):
            self.region(p, x.shape[1]).copy_(x[p])
        return self

    def get(self, n):
        import torch
        return torch.stack([self.region(p, n) for p in range(2)])

    # elements of a strided layout, relative to `ptr`
    def take(self, idx):
        return self.flat[idx + self.LEAD]

    def scatter(self, idx, values):
        self.flat[idx + self.LEAD] = values

    def whole(self):
        return bool((self._i64() == self.fill_bits).all().item())

    def clean(self, n=0, idx=None):
        """Refill regions [0, n) of both bases (and the elements `idx`), then: is every
        element of the frame the fill?"""
        v = self._i64()
        for p in range(2):
            o = self.LEAD + p * FAR
            v[o:o + int(n)] = self.fill_bits
        if idx is not None:
            v[idx.reshape(-1) + self.LEAD] = self.fill_bits
        return self.whole()


def _distance(frame, what):
    d = frame.region(1, 1).data_ptr() - frame.region(0, 1).data_ptr()
    print(f"{what}: bases {d} bytes apart (2^32 + {d - (1 << 32)})")
    assert d >= 1 << 32, f"{what}: the bases are {d} bytes apart, the case claims >= 2^32"


def _far_pair(far, what, x, olen, call, dirty=None, packed_call=None):
    """One cf32 -> cf32 two-series entry point on packed buffers and on the far frames.

    call(k, in_ptr, in_stride, out_ptr, out_stride): k = 0 the packed run, 1 the far run (a
    stateful case keeps one plan for each).  olen: elements per series compared; dirty (>=
    olen): elements per series the contract lets the call write (scratch rows)."""
    import torch
    fin, fout = far
    n = int(x.shape[1])
    dirty = olen if dirty is None else dirty
    assert x.shape[0] == 2 and 0 < olen <= dirty
    packed = torch.full((2, dirty), SENTINEL, dtype=torch.complex64, device=x.device)
    xc = x.contiguous()
    (packed_call or call)(0, xc.data_ptr(), n, packed.data_ptr(), dirty)
    _distance(fin, what + " in")
    _distance(fout, what + " out")
    fin.put(x)
    call(1, fin.ptr, FAR, fout.ptr, FAR)
    torch.cuda.synchronize(x.device)
    got = fout.get(olen)
    assert not _same_bits(packed[:, :olen], torch.full_like(packed[:, :olen], SENTINEL)), what + ": nothing written"
    assert _no_nan(got), what + ": NaN from outside the input reached the result"
    assert _same_bits(got, packed[:, :olen]), what + ": far bases changed a value"
    assert _same_bits(fin.get(n), xc), what + ": the input samples changed"
    assert fout.clean(dirty), what + ": output frame changed outside the mapped regions"
    assert fin.clean(n), what + ": input frame changed"
    return packed[:, :olen]


class TestFarBases:
    """A. Small workloads whose bases lie 2^32 + 24 bytes apart."""

    @pytest.fixture(scope="class")
    def far_frames(self, gpu):
        import torch
        _need(gpu, 2 * 8 * (FAR + EXTENT + 6) + GIB, "far frames")
        frames = (_FarFrame(gpu, NAN), _FarFrame(gpu, SENTINEL))
        yield frames
        del frames
        torch.cuda.empty_cache()

    @pytest.fixture
    def far(self, far_frames):
        """(input frame, output frame); a case that failed half-way does not hand its
        leftovers to the next one."""
        yield far_frames
        for f in far_frames:
            if not f.whole():
                f.flat.fill_(f.fill)
                assert f.whole()

    # ---------------------------------------------------------------- analysis, stateless
    # (id, N, os, taps per channel | "pst", variant, rows): the smallest cell of each family
    # of tests/test_gpu_dispatch_matrix.py / test_gpu_partition.py that forms its own base
    ANALYSIS = [
        ("stream-c2", 256, "8/7", 12, "polyphase_analysis", 53),
        ("lowcbf", 256, "4/3", "pst", "polyphase_analysis_lowcbf", 20),
        ("fused-n32-bunton", 32, "8/7", 12, "polyphase_analysis", 150),
        ("fused-n32-padded", 32, "8/7", 12, "polyphase_analysis_padded", 150),
        ("nonfused-n8-tpc40", 8, "8/7", 40, "polyphase_analysis", 150),
        ("fir-lds-n512", 512, "8/7", 15, "polyphase_analysis", 40),
        ("fir-window-n512", 512, "32/27", 28, "polyphase_analysis", 40),
        ("fir-generic-n512", 512, "16/15", 12, "polyphase_analysis", 40),
        ("rowfft4096", 4096, "8/7", 12, "polyphase_analysis", 40),
    ]

    @pytest.mark.parametrize("case", ANALYSIS, ids=lambda c: c[0])
    def test_analysis_stateless(self, gpu, far, case):
        """pfb_analysis_execute with in_pol_stride = out_pol_stride = FAR."""
        pfb, lib = _pfb(), _lib()
        name, N, os_, tpc, variant, rows = case
        nu, de = _rat(os_)
        taps = _pst_taps() if tpc == "pst" else _taps(N, os_, tpc)
        plan = pfb.AnalysisPlan(taps, N, os_, variant, 2, 0)
        C, M, P = plan.out_chan, plan.step, plan.phases
        n_dat = (3072 - 1536 if tpc == "pst" else P * N) + rows * M + 7
        plan.reset()
        K = plan.output_length(n_dat)
        assert K >= rows
        x = _dnoise(gpu, SEED + N + P, (2, n_dat))

        def call(k, ip, ips, op, ops):
            plan.reset()  # (LowCBF: the 1536 leading zeros are due again)
            n = c_int64(-1)
            st = lib.pfb_analysis_execute(plan._h, c_void_p(ip), ips, n_dat, c_void_p(op), ops, K, byref(n),
                                          DEVICE, _stream(gpu))
            assert st == OK and n.value == K, (name, st, n.value, _err(lib))

        _far_pair(far, f"analysis {name}", x, K * C, call)
        plan.close()

    # ---------------------------------------------------------------- stream objects
    @pytest.mark.parametrize("case", [("stream-c2", 256, "polyphase_analysis", (20000, 33333, 15001)),
                                      ("padded-n16", 16, "polyphase_analysis_padded", (1000, 1500, 777))],
                             ids=lambda c: c[0])
    def test_filterbank_carry(self, gpu, far, case):
        """pfb_filterbank_execute over three chunks (a carry from the second on): the
        streaming kernel's one-launch carry path, and a padded fused plan writing all K rows
        (rows [T_out, K) are scratch) straight behind the far base."""
        pfb, lib = _pfb(), _lib()
        name, N, variant, chunks = case
        taps = _taps(N, "8/7", 12 if N > 16 else 10)
        plans = [pfb.AnalysisPlan(taps, N, "8/7", variant, 2, 0) for _ in range(2)]
        M = plans[0].step
        for i, n_in in enumerate(chunks):
            B = plans[1].buffered_samples
            assert B == plans[0].buffered_samples and (i == 0) == (B == 0)
            Kt = plans[1].stream_rows(n_in)
            K = (B + n_in) // M if variant.endswith("padded") else Kt
            assert 0 < Kt <= K
            x = _dnoise(gpu, SEED + 20 + i + N, (2, n_in))

            def call(k, ip, ips, op, ops):
                n = c_int64(-1)
                st = lib.pfb_filterbank_execute(plans[k]._h, c_void_p(ip), ips, n_in, c_void_p(op), ops, K + 1,
                                                byref(n), DEVICE, _stream(gpu))
                assert st == OK and n.value == Kt, (name, i, st, n.value, _err(lib))

            _far_pair(far, f"filterbank {name} chunk {i} (carry {B})", x, Kt * N, call, dirty=(K + 1) * N)
            assert plans[0].buffered_samples == plans[1].buffered_samples
        for p in plans:
            p.close()

    def test_filterbank_strided_far_pol(self, gpu, far):
        """pfb_filterbank_execute_strided, Bunton streaming kernel, packed rows with
        out_pol_stride = FAR, two chunks (the second with a carry)."""
        pfb, lib = _pfb(), _lib()
        taps = _taps(256, "8/7", 12)
        plans = [pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", 2, 0) for _ in range(2)]
        for i, n_in in enumerate((20000, 15001)):
            Kt = plans[1].stream_rows(n_in)
            x = _dnoise(gpu, SEED + 30 + i, (2, n_in))

            def call(k, ip, ips, op, ops):
                n = c_int64(-1)
                cap = far[1].capacity if k else 2 * Kt * 256
                st = lib.pfb_filterbank_execute_strided(plans[k]._h, c_void_p(ip), ips, n_in, c_void_p(op), ops, 256,
                                                        1, 0, 0, 0, cap, byref(n), _stream(gpu))
                assert st == OK and n.value == Kt, (i, st, n.value, _err(lib))

            _far_pair(far, f"strided filterbank chunk {i}", x, Kt * 256, call)
        for p in plans:
            p.close()

    # ---------------------------------------------------------------- synthesis
    # (id, N, Nf, Ov, os, temporal taper, spectral taper, blocks)
    SYNTHESIS = [
        ("wave-nf256-n256", 256, 256, 48, "8/7", "tukey", None, 3),
        ("wave512-nf512-n56", 56, 512, 128, "8/7", "tukey", None, 3),
        ("block-nf128-n8", 8, 128, 16, "8/7", "tukey", None, 5),
        ("spectral-hann-nf128-n8", 8, 128, 16, "8/7", "tukey", "hann", 5),
        ("mixed-ifft-n14", 14, 128, 16, "8/7", "tukey", None, 5),
    ]

    @staticmethod
    def _synth_plan(N, nf, ov, os_, taper, spectral, deripple=True):
        pfb = _pfb()
        w = pfb.PFBWindow()
        return pfb.SynthesisPlan(N, os_, nf, ov, True, 1, deripple, _taps(N, os_, 12 if N > 8 else 10), taper,
                                 w.lookup[spectral](nf, ov) if spectral else None, 2, 0)

    @pytest.mark.parametrize("case", SYNTHESIS, ids=lambda c: c[0])
    def test_synthesis_stateless(self, gpu, far, case):
        """pfb_synthesis_execute (sample_offset 3) with both pol strides FAR."""
        lib = _lib()
        name, N, nf, ov, os_, taper, spectral, blocks = case
        so = 3
        plan = self._synth_plan(N, nf, ov, os_, taper, spectral)
        n_dat = (so - 1) + blocks * (nf - 2 * ov) + 2 * ov + 5
        olen = plan.output_length(n_dat - (so - 1))
        assert olen == blocks * plan.output_keep
        x = _dnoise(gpu, SEED + 40 + N + nf, (2, n_dat * N))

        def call(k, ip, ips, op, ops):
            n = c_int64(-1)
            st = lib.pfb_synthesis_execute(plan._h, c_void_p(ip), ips, n_dat, so, c_void_p(op), ops, olen, byref(n),
                                           DEVICE, _stream(gpu))
            assert st == OK and n.value == olen, (name, st, n.value, _err(lib))

        _far_pair(far, f"synthesis {name}", x, olen, call)
        plan.close()

    def test_inverse_filterbank_carry(self, gpu, far):
        """pfb_inverse_filterbank_execute, N 256 wave plan, three chunks with carried rows."""
        lib = _lib()
        plans = [self._synth_plan(256, 256, 48, "8/7", "tukey", None, deripple=False) for _ in range(2)]
        for i, n_in in enumerate((1000, 700, 1300)):
            B = plans[1].buffered_samples
            assert (i == 0) == (B == 0)
            x = _dnoise(gpu, SEED + 50 + i, (2, n_in * 256))
            cap = plans[1].output_length(B + n_in)
            got_n = []

            def call(k, ip, ips, op, ops):
                n = c_int64(-1)
                st = lib.pfb_inverse_filterbank_execute(plans[k]._h, c_void_p(ip), ips, n_in, c_void_p(op), ops, cap,
                                                        byref(n), DEVICE, _stream(gpu))
                assert st == OK and 0 < n.value <= cap, (i, st, n.value, _err(lib))
                got_n.append(n.value)

            _far_pair(far, f"inverse filterbank chunk {i} (carry {B} rows)", x, cap, call)
            assert got_n[0] == got_n[1]
            assert plans[0].buffered_samples == plans[1].buffered_samples
        for p in plans:
            p.close()

    # ---------------------------------------------------------------- round trip
    @pytest.mark.parametrize("chunk_blocks", [0, 2], ids=["fused", "chunked"])
    def test_roundtrip(self, gpu, far, chunk_blocks):
        """pfb_roundtrip_execute, C2 (N 256, 8/7, Nf 256, Ov 48): in, chan and out all FAR
        apart — the fused path (streaming analysis + wave kernel), and the chunked pipeline
        (set_chunk_blocks(2): analysis chunks on the plan's own stream)."""
        import torch
        pfb, lib = _pfb(), _lib()
        _need(gpu, 8 * (FAR + EXTENT + 6) + GIB, "third far frame")
        fchan = _FarFrame(gpu, SENTINEL)
        fin, fout = far
        taps = _taps(256, "8/7", 12)
        ana = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", 2, 0)
        syn = self._synth_plan(256, 256, 48, "8/7", "tukey", None)
        if chunk_blocks:
            syn.set_chunk_blocks(chunk_blocks)
        n_dat, so = 13 * 256 + (5 * 160 + 96 + 5) * 224 + 11, 1
        K = ana.output_length(n_dat)
        olen = syn.output_length(K - (so - 1))
        assert K * 256 <= EXTENT and 0 < olen <= EXTENT
        x = _dnoise(gpu, SEED + 60, (2, n_dat))

        def call(ip, ips, cp, cps, op, ops):
            kr, no = c_int64(-1), c_int64(-1)
            st = lib.pfb_roundtrip_execute(ana._h, syn._h, c_void_p(ip), ips, n_dat, c_void_p(cp), cps, K, byref(kr),
                                           so, c_void_p(op), ops, olen, byref(no), _stream(gpu))
            torch.cuda.synchronize(gpu)
            assert st == OK and kr.value == K and no.value == olen, (st, kr.value, no.value, _err(lib))

        pchan = torch.full((2, K * 256), SENTINEL, dtype=torch.complex64, device=gpu)
        pout = torch.full((2, olen), SENTINEL, dtype=torch.complex64, device=gpu)
        call(x.data_ptr(), n_dat, pchan.data_ptr(), K * 256, pout.data_ptr(), olen)
        what = f"round trip chunk_blocks {chunk_blocks}"
        for f, w in ((fin, "in"), (fchan, "chan"), (fout, "out")):
            _distance(f, f"{what} {w}")
        fin.put(x)
        call(fin.ptr, FAR, fchan.ptr, FAR, fout.ptr, FAR)
        chan, out = fchan.get(K * 256), fout.get(olen)
        assert _no_nan(chan) and _no_nan(out), what + ": NaN from outside the input reached a result"
        assert _same_bits(chan, pchan), what + ": far bases changed a channelised value"
        assert _same_bits(out, pout), what + ": far bases changed a synthesised value"
        assert fchan.clean(K * 256), what + ": chan frame changed outside the mapped regions"
        assert fout.clean(olen), what + ": out frame changed outside the mapped regions"
        assert fin.clean(n_dat), what + ": input frame changed"
        ana.close()
        syn.close()
        del fchan, pchan, pout

    # ---------------------------------------------------------------- mixed-format entries
    def test_analysis_to_dada_far_input(self, gpu, far):
        """pfb_analysis_execute_to_dada (C2, NBIT 16, fused store) with in_pol_stride = FAR."""
        import torch
        pfb, lib = _pfb(), _lib()
        fin, _ = far
        plan = pfb.AnalysisPlan(_taps(256, "8/7", 12), 256, "8/7", "polyphase_analysis", 2, 0)
        n_dat = 13 * 256 + 53 * 224 + 7
        K = plan.output_length(n_dat)
        x = _dnoise(gpu, SEED + 70, (2, n_dat))
        nbytes = K * 256 * 2 * 2 * 2
        secs = []
        for ip, ips in ((x.data_ptr(), n_dat), (fin.put(x).ptr, FAR)):
            sec = torch.full((nbytes // 2 + 8,), 0x5555, dtype=torch.int16, device=gpu)
            n = c_int64(-1)
            st = lib.pfb_analysis_execute_to_dada(plan._h, c_void_p(ip), ips, n_dat, c_void_p(sec.data_ptr()), 16,
                                                  30.0, nbytes, byref(n), _stream(gpu))
            assert st == OK and n.value == K, (st, n.value, _err(lib))
            assert plan.last_dada_output() == "fused"
            secs.append(sec)
        _distance(fin, "analysis to DADA in")
        torch.cuda.synchronize(gpu)
        assert torch.equal(secs[0], secs[1]), "far input bases changed a stored value"
        assert bool((secs[1][nbytes // 2:] == 0x5555).all()) and bool((secs[1][:nbytes // 2] != 0x5555).any())
        assert fin.clean(n_dat), "input frame changed"
        plan.close()

    def test_synthesis_from_dada_far_output(self, gpu, far):
        """pfb_synthesis_execute_dada (N 256 wave plan, NBIT 8 section read in place) with
        out_pol_stride = FAR."""
        import torch
        pfb, lib = _pfb(), _lib()
        _, fout = far
        plan = pfb.SynthesisPlan(256, "8/7", 256, 48, True, 1, False, None, "tukey", None, 2, 0)
        n_dat = 3 * 160 + 96 + 5
        olen = plan.output_length(n_dat)
        raw = torch.from_numpy(np.random.default_rng(SEED + 71).integers(-128, 128, n_dat * 256 * 2 * 2)
                               .astype(np.int8)).to(gpu)
        packed = torch.full((2, olen), SENTINEL, dtype=torch.complex64, device=gpu)
        for op, ops in ((packed.data_ptr(), olen), (fout.ptr, FAR)):
            n = c_int64(-1)
            st = lib.pfb_synthesis_execute_dada(plan._h, c_void_p(raw.data_ptr()), 8, 2, 0, n_dat, 1, c_void_p(op), ops,
                                                olen, byref(n), _stream(gpu))
            assert st == OK and n.value == olen, (st, n.value, _err(lib))
            assert plan.last_dada_input() == "fused"
        _distance(fout, "synthesis from DADA out")
        torch.cuda.synchronize(gpu)
        got = fout.get(olen)
        assert _no_nan(got) and _same_bits(got, packed), "far output bases changed a value"
        assert float(packed.abs().max()) > 0
        assert fout.clean(olen), "output frame changed outside the mapped regions"
        plan.close()

    @pytest.mark.parametrize("taper,path", [("tukey", "in_place"), ("hann", "staged")])
    def test_synthesis_strided_far_pol(self, gpu, far, taper, path):
        """pfb_synthesis_execute_strided with packed rows and in_pol_stride = FAR: the channel
        IFFT loading through the layout, and (Hann temporal taper) the staging copy."""
        lib = _lib()
        fin, _ = far
        N, nf, ov, so = 8, 128, 16, 3
        plan = self._synth_plan(N, nf, ov, "8/7", taper, None)
        n_dat = (so - 1) + 5 * 96 + 2 * ov + 5
        olen = plan.output_length(n_dat - (so - 1))

        def call(k, ip, ips, op, ops):
            n = c_int64(-1)
            cap = fin.capacity if k else 2 * n_dat * N
            st = lib.pfb_synthesis_execute_strided(plan._h, c_void_p(ip), ips, N, 1, cap, n_dat, so, c_void_p(op), ops,
                                                   olen, byref(n), _stream(gpu))
            assert st == OK and n.value == olen, (taper, st, n.value, _err(lib))
            assert plan.last_strided_input() == path

        def packed_call(k, ip, ips, op, ops):
            n = c_int64(-1)
            st = lib.pfb_synthesis_execute(plan._h, c_void_p(ip), ips, n_dat, so, c_void_p(op), ops, olen, byref(n),
                                           DEVICE, _stream(gpu))
            assert st == OK and n.value == olen, (taper, st, n.value, _err(lib))

        x = _dnoise(gpu, SEED + 72, (2, n_dat * N))
        ref = _far_pair(far, f"strided synthesis {taper} vs packed entry", x, olen, call, packed_call=packed_call)
        assert _same_bits(ref, _far_pair(far, f"strided synthesis {taper}", x, olen, call))
        plan.close()

    # ---------------------------------------------------------------- utilities
    @pytest.mark.parametrize("nbit", [8, 16])
    def test_dada_unpack_pack(self, gpu, far, nbit):
        """pfb_dada_unpack writing pols FAR apart and pfb_dada_pack reading them there: the
        section comes back byte for byte (the integer cast is exact)."""
        import torch
        lib = _lib()
        fin, fout = far
        n_dat, n_chan = 1001, 4
        t = {8: np.int8, 16: np.int16}[nbit]
        info = np.iinfo(t)
        raw = torch.from_numpy(np.random.default_rng(SEED + 80 + nbit)
                               .integers(info.min, info.max + 1, n_dat * n_chan * 2 * 2).astype(t)).to(gpu)
        length = n_dat * n_chan
        packed = torch.full((2, length), SENTINEL, dtype=torch.complex64, device=gpu)
        for op, ops in ((packed.data_ptr(), length), (fout.ptr, FAR)):
            st = lib.pfb_dada_unpack(c_void_p(raw.data_ptr()), nbit, 2, 0, n_dat, n_chan, 2, c_void_p(op), ops,
                                     _stream(gpu))
            assert st == OK, _err(lib)
        _distance(fout, f"unpack NBIT {nbit} out")
        torch.cuda.synchronize(gpu)
        got = fout.get(length)
        assert _same_bits(got, packed), "far output bases changed an unpacked value"
        ref = raw.view(n_dat, n_chan, 2, 2).permute(2, 0, 1, 3).to(torch.float32).contiguous()
        assert torch.equal(torch.view_as_real(got).reshape(2, n_dat, n_chan, 2), ref)
        assert fout.clean(length), "unpack: output frame changed outside the mapped regions"
        # pack: the same samples read from the NaN-filled input frame
        fin.put(got)
        _distance(fin, f"pack NBIT {nbit} in")
        back = torch.full((raw.numel() + 16,), 0x55, dtype=raw.dtype, device=gpu)
        st = lib.pfb_dada_pack(c_void_p(fin.ptr), FAR, n_dat, n_chan, 2, c_void_p(back.data_ptr()), nbit, _stream(gpu))
        assert st == OK, _err(lib)
        torch.cuda.synchronize(gpu)
        assert torch.equal(back[:raw.numel()], raw), "far input bases changed a packed value"
        assert bool((back[raw.numel():] == 0x55).all())
        assert fin.clean(length), "pack: input frame changed"

    def test_gather_and_corner_turn(self, gpu, far):
        """pfb_gather_channels and pfb_corner_turn with both outer strides FAR."""
        import torch
        lib = _lib()
        fin, fout = far
        rows, cols = 97, 24
        x = _dnoise(gpu, SEED + 82, (2, rows * cols))
        xm = x.view(2, rows, cols)
        # gather: 20 bins from bin 1 on, 3 dropped behind the 9th kept one
        n_sel, src0, split, shift = 17, 1, 9, 3

        def gather(k, ip, ips, op, ops):
            st = lib.pfb_gather_channels(c_void_p(ip), ips, cols, c_void_p(op), ops, n_sel, 2, rows, n_sel, src0,
                                         split, shift, _stream(gpu))
            assert st == OK, _err(lib)

        got = _far_pair(far, "gather", x, rows * n_sel, gather)
        j = torch.arange(n_sel, device=gpu)
        assert _same_bits(got.view(2, rows, n_sel), xm[:, :, src0 + j + (j >= split) * shift])

        def turn(k, ip, ips, op, ops):
            st = lib.pfb_corner_turn(c_void_p(ip), ips, cols, 2, rows, cols, c_void_p(op), ops, rows, _stream(gpu))
            assert st == OK, _err(lib)

        got = _far_pair(far, "corner turn", x, rows * cols, turn)
        assert _same_bits(got.view(2, cols, rows), xm.transpose(1, 2))

    def test_quantize(self, gpu, far):
        """pfb_quantize with both strides FAR.  The scale comes from double partial sums
        combined by atomicAdd in launch order (pfb_layout.hip, moments_kernel), so two
        launches agree to the reordering error of an n-term double sum, n 2^-53 relative —
        asserted at n 2^-52; the values to the bounds of test_quantize_gapped_strides (at most
        one unit, at most 1e-4 of the samples).  A NaN read from between the series would make
        the scale NaN."""
        import torch
        lib = _lib()
        n, rms = 40001, 33.8
        x = _dnoise(gpu, SEED + 84, (2, n)) * 3.0 + complex(0.25, -0.5)
        scales = []

        def call(k, ip, ips, op, ops):
            sc = c_double(-1.0)
            st = lib.pfb_quantize(c_void_p(ip), ips, n, 2, rms, c_void_p(op), ops, byref(sc), _stream(gpu))
            assert st == OK, _err(lib)
            scales.append(sc.value)

        fin, fout = far
        packed = torch.full((2, n), SENTINEL, dtype=torch.complex64, device=gpu)
        call(0, x.data_ptr(), n, packed.data_ptr(), n)
        _distance(fin, "quantize in")
        _distance(fout, "quantize out")
        call(1, fin.put(x).ptr, FAR, fout.ptr, FAR)
        torch.cuda.synchronize(gpu)
        print(f"quantize scales: packed {scales[0]!r}, far {scales[1]!r}")
        ref_sc = orc.quantize_scale(x.cpu().numpy(), rms)
        assert abs(scales[0] - ref_sc) <= 1e-9 * ref_sc
        assert abs(scales[1] - scales[0]) <= 2 * n * 2.0 ** -52 * scales[0], scales
        got = fout.get(n)
        assert _no_nan(got)
        d = (got - packed).abs()
        assert float(d.max()) <= 1.0 and float((d > 0).float().mean()) < 1e-4
        assert fout.clean(n), "quantize: output frame changed outside the mapped regions"
        assert fin.clean(n), "quantize: input frame changed"

    def test_testvec_and_purity_scores(self, gpu, far):
        """pfb_testvec_generate with out_stride FAR; pfb_purity_score_spurious and
        pfb_purity_score_difference with their row strides FAR (deterministic scores: the
        same bits as on packed rows)."""
        import torch
        lib = _lib()
        fin, fout = far
        n = 5003
        kind = (c_int32 * 2)(0, 1)
        param = (c_double * 8)(17.0, 3.0, 0.0, 0.0, 41.0, 0.3, 0.25, 0.0)
        packed = torch.full((2, n), SENTINEL, dtype=torch.complex64, device=gpu)
        for op, ops in ((packed.data_ptr(), n), (fout.ptr, FAR)):
            st = lib.pfb_testvec_generate(kind, param, 2, n, c_void_p(op), ops, _stream(gpu))
            assert st == OK, _err(lib)
        _distance(fout, "testvec out")
        torch.cuda.synchronize(gpu)
        got = fout.get(n)
        assert _same_bits(got, packed) and _no_nan(got), "far rows changed a generated value"
        assert float(packed[0].abs().sum()) == 3.0 and abs(float(packed[1].abs().mean()) - 1.0) < 1e-6
        assert fout.clean(n), "testvec: output frame changed outside the mapped regions"
        # scores of noisy rows, read from the NaN-filled frame.  The scoring kernels sum a row
        # in slots laid out from its 16-byte boundary (pfb_verify.hip), so the bits of a sum
        # depend on each row's alignment: the packed rows get the far rows' (8, then 0 mod 16)
        def lead1(t):
            flat = torch.empty(2 * n + 1, dtype=torch.complex64, device=gpu)
            rows = flat[1:].view(2, n)
            rows.copy_(t)
            return rows

        assert n % 2 == 1 and FAR % 2 == 1
        y = lead1(packed + _dnoise(gpu, SEED + 86, (2, n)) * 1e-3)
        b = lead1(packed)
        assert [r.data_ptr() % 16 for r in y] == [fin.region(p, 1).data_ptr() % 16 for p in range(2)] == [8, 0]
        fin.put(y)
        _distance(fin, "purity in")
        expected = (c_int64 * 2)(17, 41)
        res = [(c_double * 12)(), (c_double * 12)()]
        for r, (ip, ips) in zip(res, ((y.data_ptr(), n), (fin.ptr, FAR))):
            st = lib.pfb_purity_score_spurious(c_void_p(ip), 0, ips, n, 2, 1.0, 2, expected, r, _stream(gpu))
            assert st == OK, _err(lib)
        print("spurious scores:", list(res[1]))
        assert bytes(res[0]) == bytes(res[1]), (list(res[0]), list(res[1]))
        assert not np.isnan(np.array(list(res[1]))).any() and res[1][1] > 0
        fout.put(b)  # (the second operand in the other frame: both row strides far)
        dif = [(c_double * 4)(), (c_double * 4)()]
        for r, (ap, aps, bp, bps) in zip(dif, ((y.data_ptr(), n, b.data_ptr(), n), (fin.ptr, FAR, fout.ptr, FAR))):
            st = lib.pfb_purity_score_difference(c_void_p(ap), aps, c_void_p(bp), bps, n, 2, r, _stream(gpu))
            assert st == OK, _err(lib)
        print("difference scores:", list(dif[1]))
        assert bytes(dif[0]) == bytes(dif[1]), (list(dif[0]), list(dif[1]))
        assert not np.isnan(np.array(list(dif[1]))).any() and dif[1][1] > 0
        assert fin.clean(n), "purity: input frame changed"
        assert fout.clean(n), "purity: second operand's frame changed"

    # ------------------------------------------------- strides that carry the distance themselves
    @pytest.mark.parametrize("case", [("fused-n16", 16, 10, (1000, 1500)),
                                      ("fir-rowfft-n512", 512, 12, (20000, 33333))], ids=lambda c: c[0])
    def test_padded_strided_far_chan_stride(self, gpu, far, case):
        """pfb_filterbank_execute_strided on padded plans (guarded plain stores with 64-bit
        addresses), channel-major with chan_stride = FAR / (N - 1) + 1: the last channel lies
        beyond 2^32 bytes.  Two chunks, the second with a carry."""
        import torch
        pfb, lib = _pfb(), _lib()
        _, fout = far
        name, N, tpc, chunks = case
        taps = _taps(N, "8/7", tpc)
        plans = [pfb.AnalysisPlan(taps, N, "8/7", "polyphase_analysis_padded", 2, 0) for _ in range(2)]
        cs = FAR // (N - 1) + 1
        for i, n_in in enumerate(chunks):
            Kt = plans[1].stream_rows(n_in)
            K = (plans[1].buffered_samples + n_in) // plans[1].step
            ops = Kt + 1
            assert 0 < Kt and 2 * ops <= cs
            last = ops + (Kt - 1) + (N - 1) * cs
            print(f"padded strided {name} chunk {i}: chan_stride {cs}, furthest element at byte {8 * last}")
            assert 8 * (N - 1) * cs >= 1 << 32 and last < fout.capacity
            x = _dnoise(gpu, SEED + 90 + i + N, (2, n_in))
            packed = torch.full((2, (K + 1) * N), SENTINEL, dtype=torch.complex64, device=gpu)
            n = c_int64(-1)
            st = lib.pfb_filterbank_execute(plans[0]._h, c_void_p(x.data_ptr()), n_in, n_in,
                                            c_void_p(packed.data_ptr()), (K + 1) * N, K + 1, byref(n), DEVICE,
                                            _stream(gpu))
            assert st == OK and n.value == Kt, (st, n.value, _err(lib))
            st = lib.pfb_filterbank_execute_strided(plans[1]._h, c_void_p(x.data_ptr()), n_in, n_in, c_void_p(fout.ptr),
                                                    ops, 1, cs, 0, 0, 0, fout.capacity, byref(n), _stream(gpu))
            assert st == OK and n.value == Kt, (st, n.value, _err(lib))
            torch.cuda.synchronize(gpu)
            p, k, c = torch.meshgrid(torch.arange(2, device=gpu), torch.arange(Kt, device=gpu),
                                     torch.arange(N, device=gpu), indexing="ij")
            idx = p * ops + k + c * cs
            got = fout.take(idx)
            assert _no_nan(got) and _same_bits(got, packed[:, :Kt * N].reshape(2, Kt, N)), \
                f"{name} chunk {i}: the far channel stride changed a value"
            assert fout.clean(idx=idx), f"{name} chunk {i}: output frame changed outside the mapped elements"
            assert plans[0].buffered_samples == plans[1].buffered_samples
        for pl in plans:
            pl.close()

    def test_synthesis_strided_far_chan_stride(self, gpu, far):
        """pfb_synthesis_execute_strided, channel-major rows (in_row_stride 1) with
        in_chan_stride = FAR / (N - 1) + 1: the last channel lies beyond 2^32 bytes."""
        import torch
        lib = _lib()
        fin, _ = far
        N, nf, ov, so = 8, 128, 16, 3
        plan = self._synth_plan(N, nf, ov, "8/7", "tukey", None)
        n_dat = (so - 1) + 5 * 96 + 2 * ov + 5
        olen = plan.output_length(n_dat - (so - 1))
        cs, ips = FAR // (N - 1) + 1, n_dat + 1
        last = ips + (n_dat - 1) + (N - 1) * cs
        print(f"strided synthesis: in_chan_stride {cs}, furthest element at byte {8 * last}")
        assert 8 * (N - 1) * cs >= 1 << 32 and 2 * ips <= cs and last < fin.capacity
        x = _dnoise(gpu, SEED + 95, (2, n_dat, N))
        p, t, c = torch.meshgrid(torch.arange(2, device=gpu), torch.arange(n_dat, device=gpu),
                                 torch.arange(N, device=gpu), indexing="ij")
        idx = p * ips + t + c * cs
        fin.scatter(idx, x)
        outs = []
        for k in range(2):
            out = torch.full((2, olen + 3), SENTINEL, dtype=torch.complex64, device=gpu)
            n = c_int64(-1)
            if k == 0:
                st = lib.pfb_synthesis_execute(plan._h, c_void_p(x.data_ptr()), n_dat * N, n_dat, so,
                                               c_void_p(out.data_ptr()), olen + 3, olen, byref(n), DEVICE, _stream(gpu))
            else:
                st = lib.pfb_synthesis_execute_strided(plan._h, c_void_p(fin.ptr), ips, 1, cs, fin.capacity, n_dat, so,
                                                       c_void_p(out.data_ptr()), olen + 3, olen, byref(n), _stream(gpu))
                assert plan.last_strided_input() == "in_place"
            assert st == OK and n.value == olen, (k, st, n.value, _err(lib))
            outs.append(out)
        torch.cuda.synchronize(gpu)
        assert _no_nan(outs[1][:, :olen]) and _same_bits(outs[0], outs[1]), "the far channel stride changed a value"
        assert float(outs[0][:, :olen].abs().max()) > 0
        assert _same_bits(fin.take(idx), x), "the input elements changed"
        assert fin.clean(idx=idx), "input frame changed"
        plan.close()


# ================================================================= B. largest accepted extents
def _expand(base_d, S):
    """x[p] = base[p % 3] on the device."""
    import torch
    return base_d[torch.arange(S, device=base_d.device) % 3].contiguous()


def _interleave(base_sec_d, S):
    """The single-channel TFP section [t][p][re, im] of x[p] = base[p % 3] (base: (3, n, 2))."""
    import torch
    idx = torch.arange(S, device=base_sec_d.device) % 3
    return base_sec_d.permute(1, 0, 2)[:, idx, :].contiguous()


def _assert_repeat(out, dim, what):
    """out[p] (p along `dim`) bit-identical to out[p % 3], compared on the device (integer
    tensors: _int_bits)."""
    S = out.shape[dim]
    assert S > 3
    for r in range(3):
        every_third = [slice(None)] * out.dim()
        every_third[dim] = slice(r, None, 3)
        assert bool((out[tuple(every_third)] == out.narrow(dim, r, 1)).all()), (
            f"{what}: a series with p % 3 == {r} differs from series {r}")


def _int_bits(t):
    """Any tensor compared as integers (floats and complex by their bit patterns)."""
    import torch
    if t.dtype == torch.complex64:
        return torch.view_as_real(t).view(torch.int32)
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t


_FILE_NP = {8: np.int8, 16: np.int16, 32: np.float32}


def _base_section(gpu, seed, nbit, n_dat):
    """Three seeded single-channel series as file samples: -> (device (3, n_dat, 2) of the
    file's type, host complex64 (3, n_dat) — the exact values the kernels convert to)."""
    import torch
    rng = np.random.default_rng(seed)
    t = _FILE_NP[nbit]
    if nbit == 32:
        raw = (rng.standard_normal((3, n_dat, 2)) / np.sqrt(2)).astype(t)
    else:
        info = np.iinfo(t)
        raw = rng.integers(info.min, info.max + 1, (3, n_dat, 2)).astype(t)
    x = raw[..., 0].astype(np.float32) + 1j * raw[..., 1].astype(np.float32)
    return torch.from_numpy(raw).to(gpu), x.astype(np.complex64)


C2 = dict(N=256, os="8/7", tpc=12, P=13, nu=8, de=7, M=224)


def _c2_n_dat(rows, extra=11):
    return C2["P"] * C2["N"] + rows * C2["M"] + extra


def _dada_in_limit(nbit, N):
    return _largest(lambda s: LIMITS["dada_in"](s, nbit, N))


def _c2_dada_case(gpu, nbit, S, rows, expect_path, what):
    """C2 execute_dada of an S-series section of `rows` rows, cf32 output, checked by the
    reference scheme.  Returns nothing; asserts the path flag."""
    import torch
    pfb = _pfb()
    taps = _taps(256, "8/7", 12)
    n_dat = _c2_n_dat(rows)
    sec_bytes = n_dat * S * 2 * (nbit // 8)
    out_bytes = S * rows * 256 * 8
    # (section + its gather temporary, output, and the staged path's unpacked copy)
    _need(gpu, 2 * sec_bytes + out_bytes + (S * n_dat * 8 if expect_path == "staged" else 0) + GIB, what)
    base_d, base = _base_section(gpu, SEED + 100 + nbit, nbit, n_dat)
    plan = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", S, 0)
    sec = _interleave(base_d, S)
    out = plan.execute_dada(sec, nbit)
    path = plan.last_dada_input()
    print(f"{what}: n_pol {S}, NBIT {nbit}: last_dada_input {path!r}")
    assert path == expect_path, f"{what}: n_pol {S} NBIT {nbit} took {path!r}, the case claims {expect_path!r}"
    assert out.shape == (S, rows, 256)
    del sec
    ref = orc.polyphase_analysis(base[:, None, :], taps, 256, "8/7")
    assert ref.shape == (3, 256, rows)
    assert_pfb_close(out[:3].cpu().numpy().transpose(0, 2, 1), ref, what=what)
    _assert_repeat(_int_bits(out), 0, what)
    twin = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", 3, 0)
    out3 = twin.execute_dada(_interleave(base_d, 3), nbit)
    assert twin.last_dada_input() == "fused"
    assert _same_bits(out[:3], out3), f"{what}: n_pol {S} vs n_pol 3"
    plan.close()
    twin.close()
    del out, out3, base_d
    torch.cuda.empty_cache()


@pytest.mark.parametrize("side", ["limit", "beyond"])
@pytest.mark.parametrize("nbit", [32, 16, 8])
def test_dada_analysis_stream_flag_sides(gpu, nbit, side):
    """B1, flag sides.  C2 reading a section in place at the largest n_pol analysis_reads_dada
    accepts (NBIT 32 / 16 / 8: the step between a series' samples is n_pol 2 NBIT / 8 bytes)
    and one above: 'fused' at the limit, 'staged' beyond, 53 rows, both by the reference
    scheme."""
    lim = _dada_in_limit(nbit, 256)
    assert LIMITS["dada_in"](lim, nbit, 256) and not LIMITS["dada_in"](lim + 1, nbit, 256)
    assert lim + 1 <= GRID_Y_MAX
    rows = 53
    sstep = lim * (nbit // 4)
    _, new, win = _stream_shape(13, 8, 7)
    steps = _steps(rows, 8)
    # one workgroup per series (n_pol > 2 CU) walks all four steps
    r_last = (steps - 1) * new + win - 1
    print(f"flag sides NBIT {nbit}: limit n_pol {lim}, sample step {sstep} B, largest load offset "
          f"{(r_last * 256 + 255) * sstep} B over {steps} steps")
    S = lim if side == "limit" else lim + 1
    _c2_dada_case(gpu, nbit, S, rows, "fused" if side == "limit" else "staged", f"C2 section {side}")


@pytest.mark.parametrize("extra_steps", [0, 1], ids=["one-range", "split-ranges"])
def test_dada_analysis_stream_largest_range(gpu, extra_steps):
    """B1, largest single range and split ranges.  NBIT 32 at its n_pol limit with a series of
    exactly fit_steps steps (the last one ragged): ONE workgroup per series walks them all and
    loads at offsets up to the largest stream_grid admits; with fit_steps + 1 steps
    stream_grid's "more, shorter ranges" branch yields 2 ranges per series although the
    CU-derived count is 1."""
    nbit = 32
    S = _dada_in_limit(nbit, 256)
    sstep = S * (nbit // 4)
    fit = _fit_steps(sstep, 256, 13, 8, 7)
    n_steps = fit + extra_steps
    rows = (n_steps - 1) * 16 + 5
    assert _steps(rows, 8) == n_steps and rows % 16
    by_cu, ranges = _stream_ranges(_cu(gpu), S, n_steps, fit)
    _, new, win = _stream_shape(13, 8, 7)
    per_range = _ceil(n_steps, ranges)
    off = (((per_range - 1) * new + win - 1) * 256 + 255) * sstep
    # (the ragged series ends inside the last window: the offsets beyond its last sample are
    # formed and dropped by the descriptor; the largest one that loads a sample, per range
    # [n w / nw, n (w + 1) / nw) whose descriptor starts at its first window row:)
    n_dat = _c2_n_dat(rows)
    loaded = 0
    for w in range(ranges):
        st0, st1 = n_steps * w // ranges, n_steps * (w + 1) // ranges
        window = ((st1 - st0 - 1) * new + win) * 256
        loaded = max(loaded, (min(window, n_dat - st0 * new * 256) - 1) * sstep)
    print(f"largest range: n_pol {S}, fit_steps {fit}, {n_steps} steps -> CU-derived {by_cu}, launched {ranges} "
          f"range(s); largest load offset formed {off} B = {off / 2 ** 31:.4f} x 2^31, largest that loads a "
          f"sample {loaded} B = {loaded / 2 ** 31:.4f} x 2^31")
    assert loaded <= off < K_RSRC
    if extra_steps == 0:
        assert by_cu == 1 and ranges == 1, (by_cu, ranges)
        # the window of one more step would no longer fit the descriptor's rows
        assert (K_RSRC // (sstep * 256) - win) // new == n_steps and off >= 0.95 * 2 ** 31
        assert loaded >= 0.93 * 2 ** 31
    else:
        assert _ceil(n_steps, fit) > by_cu and ranges == 2, (by_cu, ranges)
    _c2_dada_case(gpu, nbit, S, rows, "fused", f"C2 section, {n_steps} steps")


def test_dada_to_dada_input_and_output_limits(gpu):
    """B1, input and output limits together.  NBIT 8 -> 8 through execute_dada_to_dada at
    n_pol 8191 with fit_steps steps: section in and section out both in place.  Quantised
    output: the bit-identities are the check."""
    import torch
    pfb = _pfb()
    nbit = 8
    S = _dada_in_limit(nbit, 256)
    fit = _fit_steps(S * (nbit // 4), 256, 13, 8, 7)
    rows = (fit - 1) * 16 + 5
    by_cu, ranges = _stream_ranges(_cu(gpu), S, fit, fit)
    assert LIMITS["ana_dadaout"](256, S, nbit) and (by_cu, ranges) == (1, 1)
    print(f"dada to dada: n_pol {S}, fit_steps {fit}, {rows} rows, 1 range per series")
    n_dat = _c2_n_dat(rows)
    _need(gpu, 2 * n_dat * S * 2 + 2 * rows * 256 * S * 2 + GIB, "dada to dada")
    taps = _taps(256, "8/7", 12)
    base_d, _ = _base_section(gpu, SEED + 130, nbit, n_dat)
    twin = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", 3, 0)
    sec3 = _interleave(base_d, 3)
    rms = float(twin.execute_dada(sec3, nbit).abs().pow(2).mean().sqrt())
    scale = 30.0 / rms  # int8 codes of ~30 rms: neither all zero nor saturated
    out3 = twin.execute_dada_to_dada(sec3, nbit, nbit, scale)
    assert (twin.last_dada_input(), twin.last_dada_output()) == ("fused", "fused")
    plan = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", S, 0)
    out = plan.execute_dada_to_dada(_interleave(base_d, S), nbit, nbit, scale)
    flags = (plan.last_dada_input(), plan.last_dada_output())
    print(f"dada to dada: last_dada_input / output {flags}")
    assert flags == ("fused", "fused")
    assert out.shape == (rows, 256, S, 2) and out.dtype == torch.int8
    assert 5 < float(out3.float().std()) < 60 and int(out3.abs().max()) <= 127
    _assert_repeat(out, 2, "dada to dada")
    assert torch.equal(out[:, :, :3], out3), "dada to dada: n_pol limit vs n_pol 3"
    plan.close()
    twin.close()


@pytest.mark.parametrize("side", ["limit", "beyond"])
@pytest.mark.parametrize("nbit", [32, 16])
def test_dada_analysis_fir_lds_flag_sides(gpu, nbit, side):
    """B2.  fir_lds (N 512, 4/3, 12 taps per channel, Bunton) reading a section in place at the
    largest n_pol analysis_reads_dada accepts and one above, 40 rows, by the reference scheme."""
    import torch
    pfb = _pfb()
    N, os_, tpc, rows = 512, "4/3", 12, 40
    lim = _dada_in_limit(nbit, N)
    assert LIMITS["dada_in"](lim, nbit, N) and not LIMITS["dada_in"](lim + 1, nbit, N)
    S = lim if side == "limit" else lim + 1
    expect = "fused" if side == "limit" else "staged"
    taps = _taps(N, os_, tpc)
    n_dat = 13 * N + rows * 384 + 3
    what = f"fir_lds section {side}"
    _need(gpu, 2 * n_dat * S * 2 * (nbit // 8) + 3 * S * (rows + 2) * N * 8 + S * n_dat * 8 + GIB, what)
    base_d, base = _base_section(gpu, SEED + 140 + nbit, nbit, n_dat)
    plan = pfb.AnalysisPlan(taps, N, os_, "polyphase_analysis", S, 0)
    out = plan.execute_dada(_interleave(base_d, S), nbit)
    path = plan.last_dada_input()
    print(f"{what}: n_pol {S}, NBIT {nbit}, sample step {S * (nbit // 4)} B: last_dada_input {path!r}")
    assert path == expect
    ref = orc.polyphase_analysis(base[:, None, :], taps, N, os_)
    assert out.shape == (S, ref.shape[2], N) and ref.shape[2] >= rows
    assert_pfb_close(out[:3].cpu().numpy().transpose(0, 2, 1), ref, what=what)
    _assert_repeat(_int_bits(out), 0, what)
    twin = pfb.AnalysisPlan(taps, N, os_, "polyphase_analysis", 3, 0)
    out3 = twin.execute_dada(_interleave(base_d, 3), nbit)
    assert twin.last_dada_input() == "fused"
    assert _same_bits(out[:3], out3), f"{what}: n_pol {S} vs n_pol 3"
    plan.close()
    twin.close()
    del out, out3
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B3. wave synthesis -> DADA
WAVE = dict(N=256, nf=256, ov=48, os="8/7", nu=8, de=7, keep=160, L=224 * 256, SO=3)


def _ifb_lens(total, so0, nf, ov, keep, nu, de, N):
    """pfb_api_synthesis.hip, ifb_lens / synth_blocks for a stream call with nothing buffered:
    -> (blocks B, carried rows, samples returned).  The carry is rounded up to a multiple of nu
    (InverseFilterBank.m:104-135), which trims the last block's output."""
    B = max((total - so0 - 2 * ov) // keep, 0)
    full = B * keep * N * de // nu
    buffered = total - B * keep
    if buffered % nu:
        buffered += nu - buffered % nu
        return B, buffered, min(max(0, (total - buffered) * N * de // nu), full)
    return B, buffered, full


@pytest.mark.parametrize("case", [(32, "limit", 2), (32, "beyond", 2), (8, "limit", 1)],
                         ids=lambda c: f"nbit{c[0]}-{c[1]}")
def test_wave_synthesis_dada_store_limits(gpu, case):
    """B3.  The Nf 256 wave synthesis storing a DADA section (N 256, Ov 48, 8/7, L = 224 x 256)
    at the largest n_pol synth_wave_dadaout_supported accepts ('fused') and one above
    ('staged').  A STREAM call (pfb_inverse_filterbank_execute_to_dada, stream sample offset
    2 = Matlab's 3) whose carry is rounded up to a multiple of nu: it returns fewer samples
    than its blocks make, so the last block is ragged (asserted from the restated ifb_lens)
    and takes store_block's non-uniform branch (pfb_synth_wave.hpp) — the one that forms the
    negative offsets of the discarded head, which must wrap above the descriptor's range at
    this largest sample step; the blocks before it take the uniform branch.  NBIT 32
    (float): out[0:3] against InverseFilterBankOracle; NBIT 8: bit-identities; both against
    an n_pol = 3 plan through the same stream call, with the carried row count checked.
    Memory: the NBIT 8 case needs 18 724 series of one block — 9.4 GiB of rows, 9.1 GiB for the
    plan's stage-1 rows (Nf rows per series), 3.7 GiB of carry and the section, 24 GiB in all:
    above the module's 16 GiB, and no smaller shape reaches this limit, so this one case
    asserts 26 GiB."""
    import torch
    pfb = _pfb()
    nbit, side, blocks = case
    N, nf, ov, os_, L, so = WAVE["N"], WAVE["nf"], WAVE["ov"], WAVE["os"], WAVE["L"], WAVE["SO"]
    keep, nu, de = WAVE["keep"], WAVE["nu"], WAVE["de"]
    lim = _largest(lambda s: LIMITS["wave_dadaout"](L, s, nbit))
    assert lim + 1 <= GRID_Y_MAX
    S = lim if side == "limit" else lim + 1
    expect = "fused" if side == "limit" else "staged"
    rows = (so - 1) + blocks * keep + 2 * ov + 5
    B, carry, olen = _ifb_lens(rows, so - 1, nf, ov, keep, nu, de, N)
    lkeep, lov = keep * N * de // nu, ov * N * de // nu
    nk_last = olen - (B - 1) * lkeep
    sb = S * (nbit // 4)
    what = f"wave DADA store NBIT {nbit} {side}"
    print(f"{what}: n_pol {S}, sample step {sb} B; {rows} rows -> {B} blocks, carry {carry} rows, {olen} of "
          f"{B * lkeep} samples returned: the last block keeps {nk_last} of {lkeep}")
    print(f"{what}: offsets of the ragged block: from {-lov * sb} B (wraps to {(-lov * sb) % 2 ** 32}) to "
          f"{(L - lov - 1) * sb} B, in range up to {(nk_last - 1) * sb} B; L sb = {L * sb} B = "
          f"{L * sb / 2 ** 31:.5f} x 2^31")
    assert B == blocks and 0 < nk_last < lkeep, "the last block is not ragged: the non-uniform store branch is idle"
    assert (B > 1) == (blocks > 1)
    if side == "limit":
        assert NEAR_2_31 <= L * sb <= K_RSRC and (-lov * sb) % 2 ** 32 >= 1 << 31
    # the rows, the plan's stage-1 rows (Nf rows per block and series), the carry, the section
    in_bytes, z_bytes, out_bytes = S * rows * N * 8, S * blocks * nf * N * 8, B * lkeep * S * 2 * (nbit // 8)
    _need(gpu, in_bytes + z_bytes + S * carry * N * 8 + out_bytes + (S * olen * 8 if expect == "staged" else 0) + GIB,
          what, budget=(16 if nbit == 32 else 26) * GIB)
    taps = _taps(N, os_, 12)
    base = _noise(SEED + 150 + nbit, (3, rows, N))
    base_d = torch.from_numpy(base).to(gpu)

    def mk(s):  # (InverseFilterBank.m:90 forces the deripple off)
        plan = pfb.SynthesisPlan(N, os_, nf, ov, True, 1, False, taps, "tukey", None, s, 0)
        plan.set_stream_sample_offset(so - 1)
        return plan

    scale = 1.0
    if nbit == 8:
        probe = mk(3)
        scale = 30.0 / float(probe.execute(base_d, stateful=True, layout="ptc").abs().pow(2).mean().sqrt())
        probe.close()
    twin = mk(3)
    out3 = twin.execute_to_dada(base_d, nbit, scale, stateful=True, layout="ptc")
    assert twin.last_dada_output() == "fused" and twin.buffered_samples == carry
    plan = mk(S)
    out = plan.execute_to_dada(_expand(base_d, S), nbit, scale, stateful=True, layout="ptc")
    path = plan.last_dada_output()
    print(f"{what}: last_dada_output {path!r}, {out.shape[0]} samples, {plan.buffered_samples} rows carried")
    assert path == expect
    assert out.shape == (olen, 1, S, 2) and plan.buffered_samples == carry
    if nbit == 32:
        ref = orc.InverseFilterBankOracle(taps, N, os_, nf, ov, "tukey", sample_offset=so - 1).execute(
            base.transpose(0, 2, 1))
        assert ref.shape == (3, 1, olen)
        got = torch.view_as_complex(out[:, 0, :3, :].contiguous()).cpu().numpy().T
        assert_pfb_close(got[:, None, :], ref, what=what)
    else:
        assert 5 < float(out3.float().std()) < 60
    _assert_repeat(_int_bits(out), 2, what)
    assert torch.equal(_int_bits(out[:, :, :3]), _int_bits(out3)), f"{what}: n_pol {S} vs n_pol 3"
    plan.close()
    twin.close()
    del out, out3
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B4. Bunton strided output
def _strided_idx(gpu, n_pol, Kt, ops, rs, cs, sel):
    """-> (element index (n_pol, Kt, kept bins), the kept bins) of the strided layout."""
    import torch
    split, shift, sel_n = sel
    c = torch.arange(256, device=gpu)
    if sel_n > 0:
        keep = (c < split) | (c >= split + shift)
        j = torch.where(c < split, c, c - shift)
        keep &= j < sel_n
        c, j = c[keep], j[keep]
    else:
        j = c
    p = torch.arange(n_pol, device=gpu)[:, None, None]
    k = torch.arange(Kt, device=gpu)[None, :, None]
    return p * ops + k * rs + j[None, None, :] * cs, c


def _strided_limit_case(gpu, layout, sel):
    import torch
    pfb, lib = _pfb(), _lib()
    jn = sel[2] if sel[2] > 0 else 256
    if layout == "channel-major":
        rs = 1
        cs = _largest(lambda v: LIMITS["strided"](rs, v, jn))
        rows, beyond = 56, (rs, cs + 1)
    else:
        cs = 1
        rs = _largest(lambda v: LIMITS["strided"](v, cs, jn))
        # rows up to the first 16-row step whose base k0 rs lies beyond 2^32 bytes, and half of it
        rows, beyond = _ceil(1 << 29, 16 * rs) * 16 + 8, (rs + 1, cs)
    assert LIMITS["strided"](rs, cs, jn) and not LIMITS["strided"](*beyond, jn)
    n_pol = 2
    taps = _taps(256, "8/7", 12)
    n_in = _c2_n_dat(rows, 7)
    x = _dnoise(gpu, SEED + 160 + jn, (n_pol, n_in))
    plan = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", n_pol, 0)
    fresh = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", n_pol, 0)
    Kt = plan.stream_rows(n_in)
    assert Kt == rows and Kt % 8 == 0
    # pols interleave inside the layout: pol 1 sits Kt + 3 rows (channel-major) or half a row
    # (row-major) behind pol 0
    ops = (Kt + 3) * rs if layout == "channel-major" else 1024
    idx, kept = _strided_idx(gpu, n_pol, Kt, ops, rs, cs, sel)
    assert idx.unique().numel() == idx.numel()
    # (room for the rejected layout too: even an unchecked call would stay inside the buffer)
    margin = 1024
    assert (beyond[0] - rs) * Kt + (beyond[1] - cs) * jn < margin
    total = int(idx.max()) + 1 + margin
    step_off = (15 * rs + (jn - 1) * cs) * 8
    print(f"strided {layout} sel {sel}: rs {rs}, cs {cs}; largest store offset in a step {step_off} B = "
          f"{step_off / 2 ** 31:.4f} x 2^31; furthest element at byte {(total - margin - 1) * 8}; "
          f"rejected: rs, cs {beyond}")
    if layout == "channel-major":
        assert step_off >= NEAR_2_31
    else:
        k0 = (Kt - 1) // 16 * 16
        print(f"strided {layout}: {Kt} rows, the last step's base at byte {k0 * rs * 8}")
        assert k0 * rs * 8 >= 1 << 32 > (k0 - 16) * rs * 8, "no step's base crosses 2^32 bytes"
    what = f"strided {layout} sel {sel}"
    _need(gpu, 8 * total + total + GIB, what)
    buf = torch.full((total,), SENTINEL, dtype=torch.complex64, device=gpu)
    sent = int(torch.view_as_real(buf[:1]).view(torch.int64).item())
    i64 = torch.view_as_real(buf).view(torch.int64).reshape(-1)

    # 1. one beyond: PFB_ERR_UNSUPPORTED, nothing written, the stream state untouched
    half = n_in // 2
    first = plan.execute(x[:, :half], stateful=True)     # (a carry to keep)
    first_f = fresh.execute(x[:, :half], stateful=True)
    B = plan.buffered_samples
    assert B > 0 and _same_bits(first, first_f)
    n = c_int64(-7)
    st = lib.pfb_filterbank_execute_strided(plan._h, c_void_p(x[:, half:].data_ptr()), x.stride(0), n_in - half,
                                            c_void_p(buf.data_ptr()), ops, beyond[0], beyond[1], *sel, total,
                                            byref(n), _stream(gpu))
    torch.cuda.synchronize(gpu)
    print(f"{what}: one beyond -> status {st} ({_err(lib)!r}), *n_out {n.value}")
    assert st == UNSUPPORTED, (st, _err(lib))
    # (pfb_api.h: a call refused for its layout leaves *n_out as it was)
    assert n.value == -7, what + ": a call refused for its layout wrote *n_out"
    assert bool((i64 == sent).all()), what + ": a rejected call wrote to the buffer"
    assert plan.buffered_samples == B == fresh.buffered_samples, what + ": a rejected call changed the stream state"
    # a following valid call equals a fresh plan's
    nxt, nxt_f = plan.execute(x[:, half:], stateful=True), fresh.execute(x[:, half:], stateful=True)
    assert nxt.shape[1] > 0 and _same_bits(nxt, nxt_f), what + ": the call after a rejected one differs"
    # 2. at the limit: bit-identical to the packed call, guards intact
    plan.reset()
    fresh.reset()
    packed = fresh.execute(x, stateful=True)
    assert packed.shape == (n_pol, Kt, 256)
    got_rows = plan.execute_strided(x, buf, ops, rs, cs, sel)
    torch.cuda.synchronize(gpu)
    assert got_rows == Kt
    got = buf[idx]
    assert _no_nan(got) and _same_bits(got, packed[:, :, kept]), what + ": a strided element differs"
    i64[idx.reshape(-1)] = sent
    assert bool((i64 == sent).all()), what + ": the buffer changed outside the mapped elements"
    assert plan.buffered_samples == fresh.buffered_samples
    plan.close()
    fresh.close()
    del buf, i64, got, idx
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layout", ["channel-major", "row-major"])
def test_bunton_strided_extent_limit(gpu, layout):
    """B4.  pfb_filterbank_execute_strided on the Bunton streaming kernel (C2) at the largest
    chan_stride (row_stride 1) and the largest row_stride (chan_stride 1) its extent check
    accepts — bit-identical to the packed call, guards intact — and one beyond:
    PFB_ERR_UNSUPPORTED, the buffer bit-unchanged, the stream state untouched, a following
    valid call equal to a fresh plan's."""
    _strided_limit_case(gpu, layout, (0, 0, 0))


def test_bunton_strided_extent_limit_chomp(gpu):
    """B4 with the cascade's channel chomp (bins [127, 155) dropped, 228 kept): the extent
    check counts sel_n channel strides, so the limit lies higher than the full row's."""
    jn = 228
    assert _largest(lambda v: LIMITS["strided"](1, v, jn)) > _largest(lambda v: LIMITS["strided"](1, v, 256))
    _strided_limit_case(gpu, "channel-major", (127, 28, jn))


# ------------------------------------------------------------------ B5. recomputed stage-1 rows
@pytest.mark.parametrize("side", ["limit", "beyond"])
def test_recomputed_stage1_rows_series_limit(gpu, side):
    """B5.  The C2 round trip with set_stage1_rows('recomputed') at the largest n_dat
    synth_wave_fir_supported accepts — (n_dat + 512 x 256) x 8 < K_RSRC — and one beyond: the
    limit reports RECOMPUTED and is bit-identical (out and chan) to a STORED run of the same
    input, one beyond reports STORED; head (and at the limit tail) against the oracle as
    test_c2_series_beyond_2gib does."""
    import torch
    pfb = _pfb()
    lim = _largest(lambda v: LIMITS["wave_fir"](v, 256))
    n = lim if side == "limit" else lim + 1
    expect = "recomputed" if side == "limit" else "stored"
    print(f"recomputed rows {side}: n_dat {n} = {n * 8} B of series, (n_dat + 512 N) 8 = {(n + 512 * 256) * 8}")
    assert LIMITS["wave_fir"](lim, 256) and not LIMITS["wave_fir"](lim + 1, 256)
    M, PN, keep, lkeep = 224, 13 * 256, 160, 35840
    K = (n - PN) // M
    B = (K - 96) // keep
    # input, chan, out, the plan's stage-1 rows (a STORED run), and one kept copy of out
    need = n * 8 + K * 256 * 8 * 3 + B * lkeep * 8 * 2 + GIB
    _need(gpu, need, f"recomputed rows {side}")
    taps = _taps(256, "8/7", 12)
    g = torch.Generator(device=gpu).manual_seed(7)
    xd = torch.complex(torch.randn((1, n), device=gpu, generator=g),
                       torch.randn((1, n), device=gpu, generator=g)).to(torch.complex64) / np.sqrt(2.0)
    win = pfb.PFBWindow().lookup["tukey"](256, 48)

    def run(mode):
        ana = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", 1, 0)
        syn = pfb.SynthesisPlan(256, "8/7", 256, 48, True, 1, True, taps, win, None, 1, 0)
        syn.set_stage1_rows(mode)
        chan, out = pfb.roundtrip(ana, syn, xd)
        torch.cuda.synchronize()
        got = syn.last_stage1_rows
        ana.close()
        syn.close()
        return chan, out, got

    chan, out, got = run("recomputed")
    print(f"recomputed rows {side}: last_stage1_rows {got!r}")
    assert got == expect
    assert out.shape == (1, B * lkeep)
    dr = {"apply_deripple": 1, "filter_coeff": taps}
    w = orc.pfb_window("tukey", 256, 48)

    def ref_from(s0, s1):
        xs = xd[:, s0:s1].cpu().numpy()[:, None, :]
        c = orc.polyphase_analysis(xs, taps, 256, "8/7")
        return orc.polyphase_synthesis(c, 1, 256, "8/7", dr, 1, 48, w)[:, 0, :]

    head = ref_from(0, 1 << 21)
    assert_pfb_close(out[:, :head.shape[1]].cpu().numpy(), head, scale=1.0, what=f"recomputed rows {side}: head")
    if side == "limit":
        b0 = B - 40
        k0 = b0 * keep
        assert k0 % 8 == 0
        tail = ref_from(k0 * M, n)
        assert tail.shape[1] == 40 * lkeep
        assert_pfb_close(out[:, b0 * lkeep:].cpu().numpy(), tail, scale=1.0, what="recomputed rows limit: tail")
        out_keep = out
        chan_r = chan
        chan, out, got = run("stored")
        assert got == "stored"
        assert torch.equal(out, out_keep), "recomputed vs stored rows: out differs"
        assert torch.equal(chan, chan_r), "recomputed vs stored rows: chan differs"
        del out_keep, chan_r
    del chan, out, xd
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ B6. analysis -> DADA, largest plan
def test_analysis_dada_store_largest_plan(gpu):
    """B6.  C2 storing a NBIT 32 section for n_pol 65535 — the largest plan the launch grid
    takes — 17 rows (one full step and a ragged one): the largest store offset is
    ((15 x 256 + 255) x 65535 + 65534) x 8 = 2 147 450 872, within 2^15 of K_RSRC.  By the
    reference scheme (float section: out[0:3] against the oracle)."""
    import torch
    pfb = _pfb()
    S, rows, nbit = GRID_Y_MAX, 17, 32
    assert LIMITS["ana_dadaout"](256, S, nbit) and not LIMITS["ana_dadaout"](256, S + 1, nbit)
    off = ((15 * 256 + 255) * S + S - 1) * (nbit // 4)
    print(f"analysis DADA store: n_pol {S}, largest store offset {off} B = {off / 2 ** 31:.5f} x 2^31")
    assert NEAR_2_31 <= off < K_RSRC
    n_dat = _c2_n_dat(rows)
    what = "analysis DADA store, largest plan"
    _need(gpu, 2 * S * n_dat * 8 + rows * 256 * S * 8 + 2 * GIB, what)
    taps = _taps(256, "8/7", 12)
    base = _noise(SEED + 180, (3, n_dat))
    base_d = torch.from_numpy(base).to(gpu)
    plan = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", S, 0)
    out = plan.execute_to_dada(_expand(base_d, S), nbit)
    path = plan.last_dada_output()
    print(f"{what}: last_dada_output {path!r}")
    assert path == "fused" and out.shape == (rows, 256, S, 2)
    ref = orc.polyphase_analysis(base[:, None, :], taps, 256, "8/7")
    assert ref.shape == (3, 256, rows)
    got = torch.view_as_complex(out[:, :, :3, :].contiguous()).permute(2, 1, 0).cpu().numpy()
    assert_pfb_close(got, ref, what=what)
    _assert_repeat(_int_bits(out), 2, what)
    twin = pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", 3, 0)
    out3 = twin.execute_to_dada(base_d, nbit)
    assert torch.equal(_int_bits(out[:, :, :3]), _int_bits(out3)), f"{what}: n_pol {S} vs n_pol 3"
    plan.close()
    twin.close()
    del out, out3
    torch.cuda.empty_cache()
