"""The C ABI's stride, capacity and alignment contract (include/pfb_api.h) on the GPU.

Every execute entry point takes a base pointer, a polarisation stride and an output
capacity that a C caller may choose freely; the Python wrappers always pass the tightest,
best-aligned layout.  These tests call the C ABI directly with framed buffers: an odd lead
(a base that is 8-B but not 16-B aligned), pols spaced wider than the data, a capacity
larger than what is written and guard samples after the last pol.

What each case asserts (``_Frame`` below):
  1. the status is PFB_OK and *n_out equals the length query;
  2. the framed result equals, BIT FOR BIT, the same entry point on contiguous, freshly
     allocated buffers with exact strides and exact capacity (the form the rest of the suite
     ties to the oracle) — stride and base select no kernel and change no arithmetic order;
     the only alignment-selected paths in csrc/ are pfb_layout.hip's launch_unpack (the TFP
     fast path) and moments_kernel / quantize_kernel (16-B loads), see the format tests;
  3. the framed result also passes conftest.assert_pfb_close against oracle/pfb_oracle.py
     at the project's 1e-6;
  4. every sample the contract does not hand to the library still holds the sentinel bit
     pattern (lead, inter-pol gaps, rows past n_out up to the capacity, tail), and no NaN
     from the NaN-filled input frames reaches a result;
  5. stateful entry points: a plan fed framed chunks against a plan fed contiguous chunks,
     chunk by chunk, with pfb_*_buffered compared after every call.

Bit-identity exceptions: pfb_quantize only — its scale comes from double atomicAdd partial
sums (pfb_layout.hip, moments_kernel's last lines), whose order differs from launch to
launch, so it is held to the existing test's bounds (scale 1e-9, values one unit / 1e-4).
"""
from ctypes import byref, c_double, c_int64, c_void_p

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

SENTINEL = complex(7.0, -7.0)
NAN = complex(float("nan"), float("nan"))
OK, INVALID_ARG = 0, 1
DEVICE, HOST = 0, 1


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _lib():
    from ska_pst_dsp_model_amd import _lib as L
    return L.load()


def _noise(rng, shape, scale=1.0):
    return (scale * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) /
            np.sqrt(2)).astype(np.complex64)


def _stream(dev):
    import torch
    return c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _bits(t):
    """complex64 tensor -> its int32 bit patterns (NaN payloads and signed zeros included)."""
    import torch
    return torch.view_as_real(t.contiguous()).view(torch.int32)


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _err(lib):
    m = lib.pfb_last_error()
    return m.decode() if m else ""


# ----------------------------------------------------------------------------- framing
class _Frame:
    """n_pol pols of ``length`` samples inside one flat complex64 device tensor:

        [lead][pol 0 ....][gap][pol 1 ....] ... [up to `extent` samples of the last pol][tail]

    ``stride = length + gap`` is the pol stride handed to the C ABI, ``extent`` (>= length)
    the samples per pol the header lets the call touch (capacity x row), so the allocation
    holds lead + (n_pol - 1) stride + extent + tail samples: a layout defect shows as a
    changed guard or a NaN, never as an access outside this tensor.  Everything is filled
    with ``fill``: NaN for inputs (a read outside [0, n) of a pol that reaches a result is
    visible, 0 * NaN included), one finite sentinel for outputs.  An odd ``lead`` gives a
    base that is 8-B but not 16-B aligned."""

    def __init__(self, dev, n_pol, length, lead=0, gap=0, tail=0, fill=SENTINEL, extent=None):
        import torch
        self.n_pol, self.length = int(n_pol), int(length)
        self.stride = self.length + int(gap)
        self.extent = max(int(extent) if extent is not None else 0, self.length)
        self.lead, self.tail, self.fill = int(lead), int(tail), fill
        total = self.lead + (self.n_pol - 1) * self.stride + self.extent + self.tail
        self.flat = torch.full((max(total, 1),), fill, dtype=torch.complex64, device=dev)
        assert self.flat.data_ptr() % 16 == 0
        if self.lead % 2:
            assert self.ptr % 16 == 8

    @property
    def ptr(self):
        return self.flat.data_ptr() + 8 * self.lead

    def pol(self, p, n=None):
        o = self.lead + p * self.stride
        return self.flat[o:o + (self.length if n is None else int(n))]

    def put(self, x):
        """x: (n_pol, n) host array or device tensor."""
        import torch
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        for p in range(self.n_pol):
            self.pol(p, x.shape[1]).copy_(x[p])
        return self

    def get(self, n):
        import torch
        return torch.stack([self.pol(p, n) for p in range(self.n_pol)])

    def guards_intact(self, n, scratch=(0, 0)):
        """Every sample outside [0, n) of each pol — and outside the documented scratch
        range [scratch[0], scratch[1]) of each pol — still holds the fill pattern."""
        import torch
        mask = torch.ones(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        for p in range(self.n_pol):
            o = self.lead + p * self.stride
            mask[o:o + int(n)] = False
            mask[o + int(scratch[0]):o + int(scratch[1])] = False
        ref = torch.full_like(self.flat, self.fill)
        return torch.equal(_bits(self.flat)[mask], _bits(ref)[mask])


def _no_nan(t):
    import torch
    return not torch.isnan(torch.view_as_real(t)).any().item()


# Input and output layouts of the device cases.  A gap is a + b rows (row = n_chan samples;
# the input's row is taken as 64 samples).  The three stride regimes: exact (the input
# lengths are odd, so pol 1 starts 8-B aligned only), length + an odd gap, length + a gap of
# a few rows.  out: (lead, a, b, tail, extra capacity in rows)
LAYOUTS = [
    dict(name="exact-in/odd-gap-out", inp=(1, 0, 0, 3), out=(3, 1, 0, 33, 0)),
    dict(name="odd-gap-in/row-gap-out", inp=(3, 5, 0, 1), out=(1, 0, 3, 17, 2)),
    dict(name="row-gap-in/odd-gap-out", inp=(5, 0, 3, 7), out=(5, 129, 0, 64, 1)),
]


def _in_frame(dev, lay, n_pol, n, row=64):
    lead, a, b, tail = lay["inp"]
    return _Frame(dev, n_pol, n, lead, a + b * row, tail, fill=NAN)


def _out_frame(dev, lay, n_pol, rows, row):
    lead, a, b, tail, extra = lay["out"]
    cap = rows + extra
    return _Frame(dev, n_pol, rows * row, lead, a + b * row, tail, extent=cap * row), cap


# ----------------------------------------------------------------------------- analysis
def _analysis_exec(lib, plan, fin, n_dat, fout, cap, dev, mem=DEVICE):
    plan.reset()  # (LowCBF: the 1536 leading zeros are due again; a no-op otherwise)
    n = c_int64(-1)
    st = lib.pfb_analysis_execute(plan._h, c_void_p(fin.ptr), fin.stride, n_dat, c_void_p(fout.ptr),
                                  fout.stride, cap, byref(n), mem, _stream(dev))
    return st, int(n.value)


def _analysis_case(dev, taps, N, os_, variant, n_dat, n_pol, seed, ref_fn, layouts=LAYOUTS):
    import torch
    pfb, lib = _pfb(), _lib()
    plan = pfb.AnalysisPlan(taps, N, os_, variant, n_pol, 0)
    C = plan.out_chan
    x = _noise(np.random.default_rng(seed), (n_pol, n_dat))
    plan.reset()
    K = int(lib.pfb_analysis_output_length(plan._h, n_dat))
    assert K > 0
    # the contiguous form: fresh allocations, exact strides, exact capacity
    cin = _Frame(dev, n_pol, n_dat, fill=NAN).put(x)
    cout = _Frame(dev, n_pol, K * C)
    st, n = _analysis_exec(lib, plan, cin, n_dat, cout, K, dev)
    assert st == OK, _err(lib)
    assert n == K
    base = cout.get(K * C)
    ref = ref_fn(x[:, None, :])
    assert ref.shape == (n_pol, C, K), (ref.shape, (n_pol, C, K))
    what = f"{variant} N={N} {os_} n_pol={n_pol}"
    assert_pfb_close(base.cpu().numpy().reshape(n_pol, K, C).transpose(0, 2, 1), ref, what=what + " contiguous")
    for lay in layouts:
        w = f"{what} [{lay['name']}]"
        fin = _in_frame(dev, lay, n_pol, n_dat).put(x)
        fout, cap = _out_frame(dev, lay, n_pol, K, C)
        st, n = _analysis_exec(lib, plan, fin, n_dat, fout, cap, dev)
        torch.cuda.synchronize(dev)
        assert st == OK, (w, _err(lib))
        assert n == K, w
        got = fout.get(K * C)
        assert _no_nan(got), w + ": NaN from outside the input reached the result"
        assert _same_bits(got, base), w + ": layout changed a value"
        assert_pfb_close(got.cpu().numpy().reshape(n_pol, K, C).transpose(0, 2, 1), ref, what=w)
        assert fout.guards_intact(K * C), w + ": output guard changed"
        assert fin.guards_intact(n_dat), w + ": input frame changed"
    return K


def _orc_analysis(taps, N, os_, variant):
    fn = {"polyphase_analysis": orc.polyphase_analysis,
          "polyphase_analysis_padded": orc.polyphase_analysis_padded}[variant]
    return lambda x: fn(x, taps, N, os_)


VARIANTS = ["polyphase_analysis", "polyphase_analysis_padded"]


@pytest.mark.parametrize("variant", VARIANTS)
def test_analysis_fused_kernel_layout(gpu, variant):
    """N 8, 8/7, 81 taps (P 11), n_dat 4101: the fused one-launch kernel —
    analysis_supported sets `fused` for 8 <= N <= 256 (pfb_analysis.hip) and
    launch_analysis takes launch_fused_v<8>, P 11 exact instance (launch_fused_p)."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(8, "8/7", 10)
    assert len(taps) == 81
    _analysis_case(gpu, taps, 8, "8/7", variant, 4101, 2, 101, _orc_analysis(taps, 8, "8/7", variant))


@pytest.mark.parametrize("os_", ["8/7", "4/3"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_analysis_streaming_kernel_layout(gpu, variant, os_):
    """N 256, 3073 taps (P 13), n_dat 2^16 + 3.  Bunton: the streaming kernel — stream_shape
    (pfb_analysis.hip: N 256, Bunton, (nu 8, M 224) or (nu 4, M 192), P 12/13) makes
    launch_analysis take launch_stream_any.  Padded: stream_shape is false, so
    the same shape runs the fused one-launch kernel launch_fused_v<256>."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(256, os_, 12)
    assert len(taps) == 3073
    _analysis_case(gpu, taps, 256, os_, variant, (1 << 16) + 3, 2, 102, _orc_analysis(taps, 256, os_, variant))


@pytest.mark.parametrize("variant", VARIANTS)
def test_analysis_fir_lds_row_fft_layout(gpu, variant):
    """N 512, 8/7, 12 taps per channel (P 13), n_dat 60 037: not fused (N > 256,
    analysis_supported), so FIR into scratch + row FFT (launch_analysis, generic branch); the FIR is
    fir_lds_kernel: fir_window_applies (DE 7, P in [7, 32]) and NU 8 divides the
    workgroup (fir_lds_shape)."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(512, "8/7", 12)
    _analysis_case(gpu, taps, 512, "8/7", variant, 60037, 2, 103, _orc_analysis(taps, 512, "8/7", variant))


def test_analysis_fir_window_layout(gpu):
    """N 512, 32/27, padded, 28 taps per channel (P 29): the register-window FIR
    fir_window_kernel — fir_window_applies needs DE 27 <= P <= 32 (pfb_analysis.hip;
    12 taps per channel, P 13 < DE, would run fir_generic_kernel) and DE 27 has no LDS form
    (fir_lds_shape)."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(512, "32/27", 28)
    assert -(-len(taps) // 512) == 29
    v = "polyphase_analysis_padded"
    _analysis_case(gpu, taps, 512, "32/27", v, 60037, 2, 104, _orc_analysis(taps, 512, "32/27", v))


def test_analysis_lowcbf_layout(gpu):
    """PFB_ANALYSIS_LOWCBF with PST_filtertaps.txt, n_dat 3072 + 192 * 20 + 7: analysis_run
    launches launch_lowcbf (its LowCBF branch), 216 output channels, the 1536 leading zeros
    of the plan's first call (restored by pfb_filterbank_reset before every call here)."""
    pfb = _pfb()
    taps = pfb.read_fir_filter_coeff(pfb.config.config_dir + "/PST_filtertaps.txt")
    n_dat = 3072 + 192 * 20 + 7
    K = _analysis_case(gpu, taps, 256, "4/3", "polyphase_analysis_lowcbf", n_dat, 2, 105,
                       lambda x: orc.polyphase_analysis_lowcbf(x, taps, do_padding=True))
    assert K == (n_dat + 1536 - 3072) // 192


@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("variant", VARIANTS)
def test_analysis_4096_odd_row_count(gpu, variant, n_pol):
    """4096 channels with an ODD row count (9 Bunton, 23 padded): launch_row_fft_t takes the
    !RUN pair kernel row_fft4096_pair_kernel<.., RUN = false> for rows [row][N] with
    n_rows >= 2 (pfb_rowfft.hip:354-361, the `if constexpr (!GAIN)` block of launch_row_fft_t), whose
    last workgroup has a row A without a row B: row A's values, the skipped r4k_row of row B
    and — with two pols — pol 0's last pair next to pol 1's first row in the exactly sized
    scratch (analysis_run).  Row B's loads of that last pair are pointed at
    row A (they used to read past the last row through the scalar offset, which the buffer
    range check does not cover; the values are discarded, so no value test can see that
    read — this test checks the values of the odd-count branch only)."""
    taps = np.random.default_rng(41).standard_normal(4096 * 12 + 1) / 64.0
    n_dat = 13 * 4096 + 9 * 3584 + 100
    K = _analysis_case(gpu, taps, 4096, "8/7", variant, n_dat, n_pol, 106,
                       _orc_analysis(taps, 4096, "8/7", variant), layouts=LAYOUTS[1:])
    assert K % 2 == 1 and K >= 3
    assert K == (9 if variant == "polyphase_analysis" else 23)


# ----------------------------------------------------------------------------- FilterBank
def _fb_exec(lib, plan, fin, n_in, fout, cap, dev, mem=DEVICE):
    n = c_int64(-1)
    st = lib.pfb_filterbank_execute(plan._h, c_void_p(fin.ptr), fin.stride, n_in, c_void_p(fout.ptr),
                                    fout.stride, cap, byref(n), mem, _stream(dev))
    return st, int(n.value)


def _filterbank_case(dev, taps, N, os_, variant, chunks, out_layout, seed, n_pol=2):
    """Two plans, one fed contiguous chunks and one framed chunks; out_layout(K, Kt, C) ->
    (lead, stride, capacity rows, tail, scratch rows allowed)."""
    import torch
    pfb, lib = _pfb(), _lib()
    plan_c = pfb.AnalysisPlan(taps, N, os_, variant, n_pol, 0)
    plan_f = pfb.AnalysisPlan(taps, N, os_, variant, n_pol, 0)
    ofb = orc.FilterBankOracle(taps, N, os_, variant)
    C = plan_f.out_chan
    M = plan_f.step
    rng = np.random.default_rng(seed)
    lay_in = LAYOUTS[1]
    scratch_seen = 0
    for i, n_in in enumerate(chunks):
        w = f"{variant} N={N} chunk {i} ({n_in} samples)"
        x = _noise(rng, (n_pol, n_in))
        B = plan_f.buffered_samples
        assert B == plan_c.buffered_samples == ofb.buffered_samples, w
        Kt = int(lib.pfb_filterbank_output_rows(plan_f._h, n_in))
        assert Kt == int(lib.pfb_filterbank_output_rows(plan_c._h, n_in)) and Kt > 0, w
        # rows the padded variant computes (the circular shift spans all K = floor(total / M)
        # rows, polyphase_analysis_padded.m:75); Bunton computes only the Kt kept rows
        K = (B + n_in) // M if variant == "polyphase_analysis_padded" else Kt
        assert Kt <= K < Kt + plan_f.os_factor.nu
        ref = ofb.execute(x[:, None, :])
        assert ref.shape == (n_pol, C, Kt), (w, ref.shape)
        cin = _Frame(dev, n_pol, n_in, fill=NAN).put(x)
        cout = _Frame(dev, n_pol, Kt * C)
        st, n = _fb_exec(lib, plan_c, cin, n_in, cout, Kt, dev)
        assert st == OK and n == Kt, (w, _err(lib))
        base = cout.get(Kt * C)
        lead, stride, cap, tail, scratch_ok = out_layout(K, Kt, C)
        fin = _in_frame(dev, lay_in, n_pol, n_in).put(x)
        fout = _Frame(dev, n_pol, Kt * C, lead, stride - Kt * C, tail, extent=cap * C)
        st, n = _fb_exec(lib, plan_f, fin, n_in, fout, cap, dev)
        torch.cuda.synchronize(dev)
        assert st == OK, (w, _err(lib))
        assert n == Kt, w
        got = fout.get(Kt * C)
        assert _no_nan(got), w + ": NaN from outside the input reached the result"
        assert _same_bits(got, base), w + ": layout changed a value"
        assert_pfb_close(got.cpu().numpy().reshape(n_pol, Kt, C).transpose(0, 2, 1), ref, what=w)
        # the padded FilterBank's documented scratch rows [T_out, K) — only where the header
        # grants them (capacity >= K and stride >= K rows); everywhere else nothing but rows
        # [0, T_out) of each pol may change
        scratch = (Kt * C, K * C) if scratch_ok else (0, 0)
        if scratch_ok:
            assert cap >= K and stride >= K * C
            scratch_seen += K - Kt
        assert fout.guards_intact(Kt * C, scratch), w + ": output guard changed"
        assert fin.guards_intact(n_in), w + ": input frame changed"
        assert plan_f.buffered_samples == plan_c.buffered_samples == ofb.buffered_samples, w
    return scratch_seen


@pytest.mark.parametrize("os_", ["8/7", "4/3"])
def test_filterbank_streaming_carry_layout(gpu, os_):
    """N 256 Bunton, three ragged chunks: the first call reads the input in place
    (filterbank_exec, concatenate-or-in-place path), the later ones carry B <= (DE 16/NU + P) N
    samples and take the one-launch carry path of the streaming kernel (the
    `analysis_offset_ok && input_idat >= B` branch: filterbank_exec, one-launch path; carry read through
    AnalysisArgs::pre).
    Input framed with a gap, capacity larger than T_out, out_pol_stride larger than
    capacity x n_chan.  Bunton computes only the kept rows: no scratch rows anywhere."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(256, os_, 12)
    lay = lambda K, Kt, C: (3, (Kt + 3) * C + 5, Kt + 2, 40, False)  # noqa: E731
    _filterbank_case(gpu, taps, 256, os_, "polyphase_analysis", (20000, 33333, 15001), lay, 201)


# (a) roomy: stride >= K rows and capacity >= K — rows [T_out, K) are scratch;
# (b) capacity exactly T_out; (c) PACKED: out_pol_stride = T_out n_chan with capacity >= K —
# pol p's rows [T_out, K) would land on pol p + 1's first rows, so the call must stage: pol
# 1's first rows equal the reference and nothing at or beyond n_pol T_out n_chan changes
# (the tail holds (K - T_out) n_chan + a guard)
PADDED_LAYOUTS = {
    "roomy": lambda K, Kt, C: (1, (K + 1) * C + 3, K + 1, 19, True),
    "exact-capacity": lambda K, Kt, C: (3, Kt * C + 1, Kt, 19, False),
    "packed": lambda K, Kt, C: (1, Kt * C, K + 1, (K - Kt) * C + 23, False),
}


@pytest.mark.parametrize("layout", list(PADDED_LAYOUTS))
def test_filterbank_padded_fused_carry_layout(gpu, layout):
    """N 16, 8/7, 10 taps per channel, padded, chunks 1000 / 1500 / 777: K 71 with T_out 64
    on the first call (filterbank_exec, concatenate-or-in-place path, input in place), K 114 with T_out 112
    on the second with a carry of 104 <= input_idat (the fused-carry branch:
    `p->fused && analysis_fused_carry_ok(p) && input_idat >= B`: filterbank_exec, fused-with-pre path), K 58 / T_out 56 on the third.
    All K rows are computed (the circular shift); they go straight into the caller's buffer
    only when capacity >= K AND out_pol_stride >= K n_chan (fb_rows_dst), else through stage_out."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(16, "8/7", 10)
    seen = _filterbank_case(gpu, taps, 16, "8/7", "polyphase_analysis_padded", (1000, 1500, 777),
                            PADDED_LAYOUTS[layout], 202)
    assert seen == ((7 + 2 + 2) if layout == "roomy" else 0)


@pytest.mark.parametrize("layout", list(PADDED_LAYOUTS))
def test_filterbank_padded_generic_layout(gpu, layout):
    """N 512, 8/7, padded: not fused (N > 256), so every call concatenates carry + input and
    takes filterbank_exec's concatenate-or-in-place path (FIR + row FFT over all K rows): K 44 / 79 / 42
    with T_out 40 / 72 / 40.  The same three layouts."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(512, "8/7", 12)
    seen = _filterbank_case(gpu, taps, 512, "8/7", "polyphase_analysis_padded", (20000, 33333, 16000),
                            PADDED_LAYOUTS[layout], 203)
    assert seen == ((4 + 7 + 2) if layout == "roomy" else 0)


# ------------------------------------------------------------------- rejected LowCBF calls
BUFFER_TOO_SMALL = 5
LOWCBF_REJECTS = {
    # name -> (capacity rows, out_pol_stride, null out) from the call's (K, C), expected status
    "capacity-one-row-short": (lambda K, C: (K - 1, K * C, False), BUFFER_TOO_SMALL),
    "pol-stride-one-short": (lambda K, C: (K, K * C - 1, False), INVALID_ARG),
    "null-out": (lambda K, C: (K, K * C, True), INVALID_ARG),
}


def _lowcbf_rejected_case(dev, entry, reject):
    """A fresh LowCBF plan whose FIRST call is rejected, then the corrected call: the one-time
    1536-zero pre-padding (polyphase_analysis_lowcbf.m:27-34) must still be pending — the
    length query unchanged, the output bit-identical to a twin plan that never saw the
    rejected call and equal to the oracle with do_padding=True.  (The parent consumed the
    padding in the rejected call: the retry then returned K - 8 rows of unpadded data.)"""
    import torch
    pfb, lib = _pfb(), _lib()
    taps = pfb.read_fir_filter_coeff(pfb.config.config_dir + "/PST_filtertaps.txt")
    n_pol, C = 2, 216
    n_dat = 3072 - 1536 + 192 * 20 + 7
    K = 20  # floor((n_dat + 1536 - 3072) / 192), a multiple of nu = 4: no row trimmed
    x = _noise(np.random.default_rng(301), (n_pol, n_dat))
    plan = pfb.AnalysisPlan(taps, 256, "4/3", "polyphase_analysis_lowcbf", n_pol, 0)
    twin = pfb.AnalysisPlan(taps, 256, "4/3", "polyphase_analysis_lowcbf", n_pol, 0)
    assert plan.out_chan == C
    if entry == "analysis":
        fn, query = lib.pfb_analysis_execute, lambda p: int(lib.pfb_analysis_output_length(p._h, n_dat))
    else:
        fn, query = lib.pfb_filterbank_execute, lambda p: int(lib.pfb_filterbank_output_rows(p._h, n_dat))

    def call(p, fout, cap, out_ps, null=False):
        n = c_int64(-1)
        st = fn(p._h, c_void_p(fin.ptr), fin.stride, n_dat, c_void_p(0 if null else fout.ptr), out_ps, cap,
                byref(n), DEVICE, _stream(dev))
        torch.cuda.synchronize(dev)
        return st, int(n.value)

    fin = _Frame(dev, n_pol, n_dat, fill=NAN).put(x)
    assert query(plan) == K and query(twin) == K
    layout, status = LOWCBF_REJECTS[reject]
    cap, out_ps, null = layout(K, C)
    bad = _Frame(dev, n_pol, K * C)
    st, n = call(plan, bad, cap, out_ps, null)
    assert st == status, (st, _err(lib))
    assert bad.guards_intact(0), "a rejected call wrote output"
    assert query(plan) == K, "a rejected call changed the length query (pre-padding consumed)"
    assert plan.buffered_samples == 0
    good, ref_out = _Frame(dev, n_pol, K * C), _Frame(dev, n_pol, K * C)
    st, n = call(plan, good, K, K * C)
    assert st == OK and n == K, (st, n, _err(lib))
    st, n = call(twin, ref_out, K, K * C)
    assert st == OK and n == K, (st, n, _err(lib))
    got = good.get(K * C)
    assert _no_nan(got)
    assert _same_bits(got, ref_out.get(K * C)), "the call after a rejected one differs from a first call"
    ref = orc.polyphase_analysis_lowcbf(x[:, None, :], taps, do_padding=True)
    assert ref.shape == (n_pol, C, K)
    assert_pfb_close(got.cpu().numpy().reshape(n_pol, K, C).transpose(0, 2, 1), ref,
                     what=f"lowcbf {entry} after {reject}")
    # and the padding is consumed exactly once: the next query is the unpadded one
    assert query(plan) == query(twin)
    assert plan.buffered_samples == twin.buffered_samples


@pytest.mark.parametrize("reject", list(LOWCBF_REJECTS))
def test_analysis_lowcbf_rejected_call_keeps_padding(gpu, reject):
    """pfb_analysis_execute on a fresh LowCBF plan, first call rejected for (a) a capacity one
    row short (PFB_ERR_BUFFER_TOO_SMALL), (b) an out_pol_stride one element short, (c) a null
    output (both PFB_ERR_INVALID_ARG): see _lowcbf_rejected_case."""
    _lowcbf_rejected_case(gpu, "analysis", reject)


def test_filterbank_lowcbf_rejected_call_keeps_padding(gpu):
    """pfb_filterbank_execute on a fresh LowCBF plan, first call rejected for a capacity one
    row short (PFB_ERR_BUFFER_TOO_SMALL; filterbank_exec's generic branch): nothing buffered,
    the padding still pending, the corrected call equal to a first call."""
    _lowcbf_rejected_case(gpu, "filterbank", "capacity-one-row-short")


# ----------------------------------------------------------------------------- synthesis
SYNTH_LAYOUTS = [
    # inp: (lead, a, b rows, tail); out: (lead, gap, tail, extra capacity in samples)
    dict(name="odd-gap", inp=(1, 7, 0, 3), out=(3, 5, 33, 65)),
    dict(name="row-gap", inp=(3, 0, 3, 5), out=(1, 1291, 17, 1000)),
]


def _synth_plan(pfb, N, os_, nf, ov, taps, n_pol, spectral=None, deripple=True):
    w = pfb.PFBWindow()
    return pfb.SynthesisPlan(N, os_, nf, ov, True, 1, deripple, taps, w.lookup["tukey"](nf, ov),
                             w.lookup[spectral](nf, ov) if spectral else None, n_pol, 0)


def _synth_exec(lib, plan, fin, n_dat, so, fout, cap, dev, mem=DEVICE):
    n = c_int64(-1)
    st = lib.pfb_synthesis_execute(plan._h, c_void_p(fin.ptr), fin.stride, n_dat, so, c_void_p(fout.ptr),
                                   fout.stride, cap, byref(n), mem, _stream(dev))
    return st, int(n.value)


def _synthesis_case(dev, N, os_, nf, ov, n_dat, seed, spectral=None, n_pol=2):
    import torch
    pfb, lib = _pfb(), _lib()
    taps = pfb.design_PFB_FIR_filter(N, os_, 12 if N > 8 else 10)
    plan = _synth_plan(pfb, N, os_, nf, ov, taps, n_pol, spectral)
    x = _noise(np.random.default_rng(seed), (n_pol, N, n_dat))               # Matlab (pol, chan, t)
    ptc = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(n_pol, n_dat * N)  # engine rows
    for so in (1, 4):
        olen = int(lib.pfb_synthesis_output_length(plan._h, n_dat - (so - 1)))
        assert olen > 0
        ref = orc.polyphase_synthesis(x, 1, nf, os_, {"apply_deripple": 1, "filter_coeff": taps}, so, ov,
                                      orc.pfb_window("tukey", nf, ov),
                                      orc.pfb_window(spectral, nf, ov) if spectral else None)
        assert ref.shape == (n_pol, 1, olen), (ref.shape, olen)
        cin = _Frame(dev, n_pol, n_dat * N, fill=NAN).put(ptc)
        cout = _Frame(dev, n_pol, olen)
        st, n = _synth_exec(lib, plan, cin, n_dat, so, cout, olen, dev)
        assert st == OK and n == olen, _err(lib)
        base = cout.get(olen)
        for lay in SYNTH_LAYOUTS:
            w = f"synthesis N={N} Nf={nf} offset {so} [{lay['name']}]"
            fin = _in_frame(dev, lay, n_pol, n_dat * N, row=N).put(ptc)
            lead, gap, tail, extra = lay["out"]
            fout = _Frame(dev, n_pol, olen, lead, gap, tail, extent=olen + extra)
            st, n = _synth_exec(lib, plan, fin, n_dat, so, fout, olen + extra, dev)
            torch.cuda.synchronize(dev)
            assert st == OK, (w, _err(lib))
            assert n == olen, w
            got = fout.get(olen)
            assert _no_nan(got), w + ": NaN from outside the input reached the result"
            assert _same_bits(got, base), w + ": layout changed a value"
            assert_pfb_close(got.cpu().numpy()[:, None, :], ref, what=w)
            assert fout.guards_intact(olen), w + ": output guard changed"
            assert fin.guards_intact(n_dat * N), w + ": input frame changed"


def test_synthesis_block_kernel_layout(gpu):
    """N 8, Nf 128, Ov 16, 8/7: no wave kernel (synth_wave_supported needs Nf 256,
    pfb_synth_wave.hip:34-39; synth_wave512_supported Nf 512), so launch_synth_block falls to
    the block kernel's size table (pfb_synth.hip:243-247).  Five blocks and a ragged tail."""
    _synthesis_case(gpu, 8, "8/7", 128, 16, 5 * 96 + 32 + 7, 301)


def test_synthesis_wave_kernel_layout(gpu):
    """N 256, Nf 256, Ov 48, 8/7 (W 224, keep 160): synth_wave_supported
    (pfb_synth_wave.hip:34-39) makes synthesis_chunk write the stage-1 rows in 2-row runs
    (synthesis_chunk, `l.zblk`) and launch_synth_block take synth_wave_kernel (pfb_synth.hip:242).
    Six blocks plus a ragged tail."""
    _synthesis_case(gpu, 256, "8/7", 256, 48, 6 * 160 + 96 + 5, 302)


def test_synthesis_wave512_kernel_layout(gpu):
    """N 64, Nf 512, Ov 128, 8/7 (W 448, keep 256): synth_wave512_supported
    (pfb_synth_wave512.hip:403-412), launch_synth_block's first branch (pfb_synth.hip:240)."""
    _synthesis_case(gpu, 64, "8/7", 512, 128, 3 * 256 + 256 + 11, 303)


def test_synthesis_spectral_taper_layout(gpu):
    """N 8, Nf 128, Ov 16 with the `hann` spectral taper: synthesis_chunk's has_spectral
    branch (synthesis_spectral: per-channel FFT, stitch x taper, row IFFTs)."""
    _synthesis_case(gpu, 8, "8/7", 128, 16, 5 * 96 + 32 + 7, 304, spectral="hann")


def _ifb_exec(lib, plan, fin, n_in, fout, cap, dev, mem=DEVICE):
    n = c_int64(-1)
    st = lib.pfb_inverse_filterbank_execute(plan._h, c_void_p(fin.ptr), fin.stride, n_in, c_void_p(fout.ptr),
                                            fout.stride, cap, byref(n), mem, _stream(dev))
    return st, int(n.value)


@pytest.mark.parametrize("N,nf,ov,chunks", [
    (8, 128, 16, (500, 333, 1000)),
    (256, 256, 48, (1000, 700, 1300)),
])
def test_inverse_filterbank_layout(gpu, N, nf, ov, chunks):
    """pfb_inverse_filterbank_execute over three chunks, framed against contiguous: the first
    call reads the input in place, the later ones carry rows and take the in-place carry
    path (`Bc > 0 && !has_spectral && input_idat >= Bc`: ifb_go, split path): the first blocks from a stitched
    buffer of carry + input head, the rest from the input with a row shift.  There is no
    length query for this entry point: *n_out must equal the InverseFilterBank.m oracle's
    length, which is also the contiguous run's exact stride and capacity."""
    import torch
    pfb, lib = _pfb(), _lib()
    n_pol = 2
    taps = pfb.design_PFB_FIR_filter(N, "8/7", 12 if N > 8 else 10)
    # (InverseFilterBank.m:90 forces the deripple off)
    plan_c = _synth_plan(pfb, N, "8/7", nf, ov, taps, n_pol, deripple=False)
    plan_f = _synth_plan(pfb, N, "8/7", nf, ov, taps, n_pol, deripple=False)
    oifb = orc.InverseFilterBankOracle(taps, N, "8/7", nf, ov, "tukey")
    rng = np.random.default_rng(310 + N)
    for i, n_in in enumerate(chunks):
        w = f"inverse stream N={N} chunk {i} ({n_in} rows)"
        x = _noise(rng, (n_pol, N, n_in))
        ptc = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(n_pol, n_in * N)
        ref = oifb.execute(x)
        olen = ref.shape[2]
        assert olen > 0, w
        cin = _Frame(gpu, n_pol, n_in * N, fill=NAN).put(ptc)
        cout = _Frame(gpu, n_pol, olen)
        st, n = _ifb_exec(lib, plan_c, cin, n_in, cout, olen, gpu)
        assert st == OK and n == olen, (w, n, olen, _err(lib))
        base = cout.get(olen)
        lay = SYNTH_LAYOUTS[i % 2]
        fin = _in_frame(gpu, lay, n_pol, n_in * N, row=N).put(ptc)
        lead, gap, tail, extra = lay["out"]
        fout = _Frame(gpu, n_pol, olen, lead, gap, tail, extent=olen + extra)
        st, n = _ifb_exec(lib, plan_f, fin, n_in, fout, olen + extra, gpu)
        torch.cuda.synchronize(gpu)
        assert st == OK, (w, _err(lib))
        assert n == olen, w
        got = fout.get(olen)
        assert _no_nan(got), w + ": NaN from outside the input reached the result"
        assert _same_bits(got, base), w + ": layout changed a value"
        assert_pfb_close(got.cpu().numpy()[:, None, :], ref, what=w)
        assert fout.guards_intact(olen), w + ": output guard changed"
        assert fin.guards_intact(n_in * N), w + ": input frame changed"
        assert plan_f.buffered_samples == plan_c.buffered_samples == oifb.buffered_samples, w


# ----------------------------------------------------------------------------- round trip
def _rt_exec(lib, ana, syn, fin, n_dat, fchan, ccap, so, fout, ocap, dev):
    kr, no = c_int64(-1), c_int64(-1)
    st = lib.pfb_roundtrip_execute(ana._h, syn._h, c_void_p(fin.ptr), fin.stride, n_dat, c_void_p(fchan.ptr),
                                   fchan.stride, ccap, byref(kr), so, c_void_p(fout.ptr), fout.stride, ocap,
                                   byref(no), _stream(dev))
    return st, int(kr.value), int(no.value)


def _roundtrip_case(dev, N, tpc, nf, ov, n_dat, so, seed, chunk_blocks=0, split=False):
    import torch
    pfb, lib = _pfb(), _lib()
    n_pol, os_, variant = 2, "8/7", "polyphase_analysis"
    taps = pfb.design_PFB_FIR_filter(N, os_, tpc)
    ana = pfb.AnalysisPlan(taps, N, os_, variant, n_pol, 0)
    syn = _synth_plan(pfb, N, os_, nf, ov, taps, n_pol)
    if chunk_blocks:
        syn.set_chunk_blocks(chunk_blocks)
    x = _noise(np.random.default_rng(seed), (n_pol, n_dat))
    K = int(lib.pfb_analysis_output_length(ana._h, n_dat))
    olen = int(lib.pfb_synthesis_output_length(syn._h, K - (so - 1)))
    assert K > 0 and olen > 0
    ref_chan = orc.polyphase_analysis(x[:, None, :], taps, N, os_)
    ref = orc.polyphase_synthesis(ref_chan, 1, nf, os_, {"apply_deripple": 1, "filter_coeff": taps}, so, ov,
                                  orc.pfb_window("tukey", nf, ov))
    assert ref_chan.shape == (n_pol, N, K) and ref.shape == (n_pol, 1, olen)
    cin = _Frame(dev, n_pol, n_dat, fill=NAN).put(x)
    cchan = _Frame(dev, n_pol, K * N)
    cout = _Frame(dev, n_pol, olen)
    st, kr, no = _rt_exec(lib, ana, syn, cin, n_dat, cchan, K, so, cout, olen, dev)
    assert st == OK and kr == K and no == olen, _err(lib)
    torch.cuda.synchronize(dev)
    base_chan, base_out = cchan.get(K * N), cout.get(olen)
    for lay in LAYOUTS[:2]:
        w = f"round trip N={N} Nf={nf} chunk_blocks={chunk_blocks} split={split} [{lay['name']}]"
        fin = _in_frame(dev, lay, n_pol, n_dat).put(x)
        fchan, ccap = _out_frame(dev, lay, n_pol, K, N)
        lead, a, b, tail, extra = lay["out"]
        fout = _Frame(dev, n_pol, olen, lead + 2, a + 2 + b * N, tail, extent=olen + extra * 77)
        ocap = olen + extra * 77
        if split:
            kr, no = c_int64(-1), c_int64(-1)
            st = lib.pfb_roundtrip_analysis_execute(ana._h, syn._h, c_void_p(fin.ptr), fin.stride, n_dat,
                                                    c_void_p(fchan.ptr), fchan.stride, ccap, byref(kr), so,
                                                    _stream(dev))
            assert st == OK, (w, _err(lib))
            st = lib.pfb_roundtrip_synthesis_execute(ana._h, syn._h, n_dat, so, c_void_p(fout.ptr), fout.stride,
                                                     ocap, byref(no), _stream(dev))
            kr, no = int(kr.value), int(no.value)
        else:
            st, kr, no = _rt_exec(lib, ana, syn, fin, n_dat, fchan, ccap, so, fout, ocap, dev)
        torch.cuda.synchronize(dev)
        assert st == OK, (w, _err(lib))
        assert kr == K and no == olen, w
        chan, out = fchan.get(K * N), fout.get(olen)
        assert _no_nan(chan) and _no_nan(out), w + ": NaN from outside the input reached a result"
        assert _same_bits(chan, base_chan), w + ": layout changed a channelised value"
        assert _same_bits(out, base_out), w + ": layout changed a synthesised value"
        assert_pfb_close(chan.cpu().numpy().reshape(n_pol, K, N).transpose(0, 2, 1), ref_chan, what=w + " chan")
        assert_pfb_close(out.cpu().numpy()[:, None, :], ref, scale=1.0, what=w + " out (raw)")
        assert fchan.guards_intact(K * N), w + ": chan guard changed"
        assert fout.guards_intact(olen), w + ": out guard changed"
        assert fin.guards_intact(n_dat), w + ": input frame changed"


def test_roundtrip_fused_stream_layout(gpu):
    """N 256, 8/7, Nf 256, Ov 48: the fused round trip (roundtrip_run: analysis_emits_z, no
    chunk size), the streaming kernel writing the stage-1 rows in runs for synth_wave_kernel;
    sample_offset 1 (off % 16 == 0, the zblk layout)."""
    _roundtrip_case(gpu, 256, 12, 256, 48, 150003, 1, 401)


def test_roundtrip_chunked_layout(gpu):
    """N 8 with a chunk size set: roundtrip_run's chunked pipeline (analysis chunks on the
    plan's second stream, synthesis_chunk on the caller's)."""
    _roundtrip_case(gpu, 8, 10, 128, 16, 9001, 4, 402, chunk_blocks=2)


def test_roundtrip_fused_fir_layout(gpu):
    """N 512, 8/7, Nf 128, Ov 16: the fused path of the generic analysis (roundtrip_run's
    `!pa->fused` arm of its fused path: the FIR writes the stage-1 rows, the row FFT makes the channelised
    product from them, the block kernel reads them)."""
    _roundtrip_case(gpu, 512, 12, 128, 16, 200003, 4, 403)


def test_roundtrip_split_halves_layout(gpu):
    """pfb_roundtrip_analysis_execute + pfb_roundtrip_synthesis_execute on the N 256 fused
    shape with framed in / chan / out: bit-identical to the contiguous whole round trip."""
    _roundtrip_case(gpu, 256, 12, 256, 48, 150003, 1, 404, split=True)


# ----------------------------------------------------------------------------- rejections
def _reject(lib, st, frames, what):
    assert st == INVALID_ARG, (what, st, _err(lib))
    assert len(_err(lib)) > 0, what
    for f in frames:
        assert f.guards_intact(0), what + ": a rejected call wrote to its output"


@pytest.mark.parametrize("entry", ["analysis", "filterbank", "filterbank_strided", "synthesis",
                                   "inverse_filterbank", "roundtrip"])
def test_execute_rejects_bad_strides(gpu, entry):
    """Every device-memory execute entry point returns PFB_ERR_INVALID_ARG with a message,
    writes nothing and keeps its stream state for: an in_pol_stride smaller than one pol's
    input samples, an out_pol_stride smaller than the samples returned, a negative n_in.
    (The frames are sized for the proper strides, so even an unchecked call would stay
    inside them.)"""
    import torch
    pfb, lib = _pfb(), _lib()
    dev, n_pol, s = gpu, 2, _stream(gpu)
    n = c_int64(-1)
    if entry in ("analysis", "filterbank", "filterbank_strided"):
        N = 256 if entry == "filterbank_strided" else 8
        taps = pfb.design_PFB_FIR_filter(N, "8/7", 12 if N > 8 else 10)
        plan = pfb.AnalysisPlan(taps, N, "8/7", "polyphase_analysis", n_pol, 0)
        n_dat = 20001 if N > 8 else 4101
        K = int(lib.pfb_filterbank_output_rows(plan._h, n_dat) if entry != "analysis"
                else lib.pfb_analysis_output_length(plan._h, n_dat))
        assert K > 0
        fin = _Frame(dev, n_pol, n_dat, 1, 3, 3, fill=NAN).put(_noise(np.random.default_rng(5), (n_pol, n_dat)))
        fout = _Frame(dev, n_pol, K * N, 1, 3, 9)
        if entry == "filterbank_strided":
            cap = fout.flat.numel() - fout.lead

            def call(ips, nd, ops):
                return lib.pfb_filterbank_execute_strided(plan._h, c_void_p(fin.ptr), ips, nd, c_void_p(fout.ptr),
                                                          fout.stride, 1, K, 0, 0, 0, cap, byref(n), s)
            cases = [("in stride", n_dat - 1, n_dat, 0), ("negative n_in", fin.stride, -1, 0)]
        else:
            fn = lib.pfb_analysis_execute if entry == "analysis" else lib.pfb_filterbank_execute

            def call(ips, nd, ops):
                return fn(plan._h, c_void_p(fin.ptr), ips, nd, c_void_p(fout.ptr), ops, K, byref(n), DEVICE, s)
            cases = [("in stride", n_dat - 1, n_dat, fout.stride), ("out stride", fin.stride, n_dat, K * N - 1),
                     ("negative n_in", fin.stride, -1, fout.stride)]
        for what, ips, nd, ops in cases:
            _reject(lib, call(ips, nd, ops), [fout], f"{entry}: {what}")
            torch.cuda.synchronize(dev)
            assert plan.buffered_samples == 0
        return
    N, nf, ov = 8, 128, 16
    taps = pfb.design_PFB_FIR_filter(N, "8/7", 10)
    syn = _synth_plan(pfb, N, "8/7", nf, ov, taps, n_pol, deripple=(entry != "inverse_filterbank"))
    if entry == "roundtrip":
        ana = pfb.AnalysisPlan(taps, N, "8/7", "polyphase_analysis", n_pol, 0)
        n_dat = 9001
        K = int(lib.pfb_analysis_output_length(ana._h, n_dat))
        olen = int(lib.pfb_synthesis_output_length(syn._h, K))
        assert K > 0 and olen > 0
        fin = _Frame(dev, n_pol, n_dat, 1, 3, 3, fill=NAN).put(_noise(np.random.default_rng(6), (n_pol, n_dat)))
        fchan = _Frame(dev, n_pol, K * N, 1, 3, 9)
        fout = _Frame(dev, n_pol, olen, 1, 3, 9)
        kr, no = c_int64(-1), c_int64(-1)

        def call(ips, nd, cps, ops):
            return lib.pfb_roundtrip_execute(ana._h, syn._h, c_void_p(fin.ptr), ips, nd, c_void_p(fchan.ptr), cps,
                                             K, byref(kr), 1, c_void_p(fout.ptr), ops, olen, byref(no), s)
        for what, ips, nd, cps, ops in [("in stride", n_dat - 1, n_dat, fchan.stride, fout.stride),
                                        ("chan stride", fin.stride, n_dat, K * N - 1, fout.stride),
                                        ("out stride", fin.stride, n_dat, fchan.stride, olen - 1),
                                        ("negative n_dat", fin.stride, -1, fchan.stride, fout.stride)]:
            _reject(lib, call(ips, nd, cps, ops), [fchan, fout], f"roundtrip: {what}")
            torch.cuda.synchronize(dev)
        return
    n_dat = 5 * 96 + 32 + 7
    olen = int(lib.pfb_synthesis_output_length(syn._h, n_dat))
    assert olen > 0
    x = _noise(np.random.default_rng(7), (n_pol, n_dat * N))
    fin = _Frame(dev, n_pol, n_dat * N, 1, 3, 3, fill=NAN).put(x)
    fout = _Frame(dev, n_pol, olen, 1, 3, 9)

    def call(ips, nd, ops):
        if entry == "synthesis":
            return lib.pfb_synthesis_execute(syn._h, c_void_p(fin.ptr), ips, nd, 1, c_void_p(fout.ptr), ops, olen,
                                             byref(n), DEVICE, s)
        return lib.pfb_inverse_filterbank_execute(syn._h, c_void_p(fin.ptr), ips, nd, c_void_p(fout.ptr), ops,
                                                  olen, byref(n), DEVICE, s)
    n_ret = olen
    if entry == "inverse_filterbank":
        # the stream call trims its output with the carry's rounding to a multiple of nu
        # (InverseFilterBank.m:104-135) and has no length query: a valid call on a second,
        # identical plan tells how many samples this one would return
        probe = _synth_plan(pfb, N, "8/7", nf, ov, taps, n_pol, deripple=False)
        pout = _Frame(dev, n_pol, olen)
        assert lib.pfb_inverse_filterbank_execute(probe._h, c_void_p(fin.ptr), fin.stride, n_dat, c_void_p(pout.ptr),
                                                  pout.stride, olen, byref(n), DEVICE, s) == OK, _err(lib)
        n_ret = int(n.value)
        assert 0 < n_ret <= olen
    for what, ips, nd, ops in [("in stride", n_dat * N - 1, n_dat, fout.stride),
                               ("out stride", fin.stride, n_dat, n_ret - 1),
                               ("negative n_in", fin.stride, -1, fout.stride)]:
        _reject(lib, call(ips, nd, ops), [fout], f"{entry}: {what}")
        torch.cuda.synchronize(dev)
        assert syn.buffered_samples == 0


# ----------------------------------------------------------------------------- host memory
def _host_frame(n_pol, length, lead, gap, tail, fill):
    stride = length + gap
    flat = np.full(lead + (n_pol - 1) * stride + length + tail, fill, dtype=np.complex64)
    return flat, stride


def _host_guards_intact(flat, n_pol, length, lead, stride, fill):
    mask = np.ones(flat.size, dtype=bool)
    for p in range(n_pol):
        mask[lead + p * stride:lead + p * stride + length] = False
    ref = np.full(flat.size, fill, dtype=np.complex64)
    return np.array_equal(flat.view(np.int32).reshape(-1, 2)[mask], ref.view(np.int32).reshape(-1, 2)[mask])


@pytest.mark.parametrize("kind", ["analysis", "synthesis"])
def test_host_memory_strided_pols(gpu, kind):
    """PFB_MEM_HOST with strided numpy pols and guard values: copy_pols stages in_ps /
    out_ps different from the lengths (pfb_analysis_execute / pfb_synthesis_execute, the
    host branches).  Against the contiguous host call (bit for bit) and the oracle."""
    pfb, lib = _pfb(), _lib()
    n_pol, N = 2, 8
    taps = pfb.design_PFB_FIR_filter(N, "8/7", 10)
    rng = np.random.default_rng(501)
    if kind == "analysis":
        plan = pfb.AnalysisPlan(taps, N, "8/7", "polyphase_analysis", n_pol, 0)
        n_dat = 4101
        x = _noise(rng, (n_pol, n_dat))
        n_in, olen = n_dat, int(lib.pfb_analysis_output_length(plan._h, n_dat)) * N
        cap_c, cap_f = olen // N, olen // N + 3
        ref = orc.polyphase_analysis(x[:, None, :], taps, N, "8/7").transpose(0, 2, 1).reshape(n_pol, olen)
        n_expect = olen // N

        def call(ip, ips, op, ops, cap, n):
            return lib.pfb_analysis_execute(plan._h, c_void_p(ip), ips, n_dat, c_void_p(op), ops, cap, byref(n),
                                            HOST, None)
    else:
        nf, ov, n_dat = 128, 16, 5 * 96 + 32 + 7
        plan = _synth_plan(pfb, N, "8/7", nf, ov, taps, n_pol)
        xm = _noise(rng, (n_pol, N, n_dat))
        x = np.ascontiguousarray(xm.transpose(0, 2, 1)).reshape(n_pol, n_dat * N)
        n_in, olen = n_dat * N, int(lib.pfb_synthesis_output_length(plan._h, n_dat))
        cap_c, cap_f = olen, olen + 50
        ref = orc.polyphase_synthesis(xm, 1, nf, "8/7", {"apply_deripple": 1, "filter_coeff": taps}, 1, ov,
                                      orc.pfb_window("tukey", nf, ov))[:, 0, :]
        n_expect = olen

        def call(ip, ips, op, ops, cap, n):
            return lib.pfb_synthesis_execute(plan._h, c_void_p(ip), ips, n_dat, 1, c_void_p(op), ops, cap,
                                             byref(n), HOST, None)
    assert olen > 0 and ref.shape == (n_pol, olen)
    n = c_int64(-1)
    cin = np.ascontiguousarray(x)
    cout = np.full((n_pol, olen), SENTINEL, dtype=np.complex64)
    assert call(cin.ctypes.data, n_in, cout.ctypes.data, olen, cap_c, n) == OK, _err(lib)
    assert n.value == n_expect
    assert_pfb_close(cout, ref, what=f"host {kind} contiguous")
    for lead_i, gap_i, lead_o, gap_o in ((1, 0, 3, 1), (3, 37, 1, 5 * N)):
        w = f"host {kind} lead {lead_i}/{lead_o} gap {gap_i}/{gap_o}"
        fi, ips = _host_frame(n_pol, n_in, lead_i, gap_i, 5, NAN)
        for p in range(n_pol):
            fi[lead_i + p * ips:lead_i + p * ips + n_in] = x[p]
        fo, ops = _host_frame(n_pol, olen, lead_o, gap_o, 11, SENTINEL)
        n = c_int64(-1)
        st = call(fi.ctypes.data + 8 * lead_i, ips, fo.ctypes.data + 8 * lead_o, ops, cap_f, n)
        assert st == OK, (w, _err(lib))
        assert n.value == n_expect, w
        got = np.stack([fo[lead_o + p * ops:lead_o + p * ops + olen] for p in range(n_pol)])
        assert not np.isnan(got).any(), w
        assert np.array_equal(got.view(np.int32), cout.view(np.int32)), w + ": layout changed a value"
        assert_pfb_close(got, ref, what=w)
        assert _host_guards_intact(fo, n_pol, olen, lead_o, ops, SENTINEL), w + ": output guard changed"
        assert _host_guards_intact(fi, n_pol, n_in, lead_i, ips, NAN), w + ": input frame changed"


# ----------------------------------------------------------------------------- data formats
def _file_samples(rng, nbit, count):
    t = orc._NBIT_NP[nbit]
    info = np.iinfo(t)
    return rng.integers(info.min, info.max + 1, size=count).astype(t)


@pytest.mark.parametrize("nbit", [8, 16])
@pytest.mark.parametrize("layout", ["aligned", "odd-stride", "input-advanced", "odd-lead"])
def test_dada_unpack_layouts(gpu, nbit, layout):
    """pfb_dada_unpack, dual-pol TFP, NDIM 2.  launch_unpack (pfb_layout.hip) takes the
    4-sample fast path dada_unpack_tfp4_kernel (16-B loads and stores) only when the input
    and output bases are 16-B aligned and the pol stride is even: `aligned` is that path;
    an odd out_pol_stride, an input pointer advanced by one sample pair (4 or 8 bytes) and
    an odd output lead must each take the generic kernel.  All equal reshape_dada_data.m
    exactly and leave the guards intact."""
    import torch
    lib = _lib()
    n_pol, n_chan, n_dat = 2, 4, 1001
    count = n_dat * n_chan * n_pol * 2
    pair = 2 * n_pol  # file values of one (t, c) sample pair
    adv = pair if layout == "input-advanced" else 0
    raw = _file_samples(np.random.default_rng(600 + nbit), nbit, count + adv)
    dev_raw = torch.from_numpy(raw.view(np.uint8)).to(gpu)
    in_ptr = dev_raw.data_ptr() + adv * raw.itemsize
    assert dev_raw.data_ptr() % 16 == 0 and (in_ptr % 16 == 0) == (adv == 0)
    length = n_dat * n_chan
    fout = _Frame(gpu, n_pol, length, lead=1 if layout == "odd-lead" else 0,
                  gap=1 if layout == "odd-stride" else 0, tail=9)
    assert (fout.stride % 2 == 1) == (layout == "odd-stride")
    st = lib.pfb_dada_unpack(c_void_p(in_ptr), nbit, 2, 0, n_dat, n_chan, n_pol, c_void_p(fout.ptr), fout.stride,
                             _stream(gpu))
    torch.cuda.synchronize(gpu)
    assert st == OK, _err(lib)
    ref = orc.reshape_dada_data(raw[adv:], 2, n_pol, n_chan).transpose(0, 2, 1).astype(np.complex64)
    assert np.array_equal(fout.get(length).cpu().numpy(), ref.reshape(n_pol, length))
    assert fout.guards_intact(length)


@pytest.mark.parametrize("nbit", [8, 16])
def test_dada_pack_gapped_stride(gpu, nbit):
    """pfb_dada_pack reading pols `in_pol_stride` = length + an odd gap apart from an
    8-B-aligned base, NaN between them: exactly write_dada_data.m, output guard intact."""
    import torch
    lib = _lib()
    n_pol, n_dat, n_chan = 2, 333, 16
    x = _noise(np.random.default_rng(610 + nbit), (n_pol, n_dat, n_chan), scale=300.0)
    x[0, 0, :4] = [0.5, -0.5, 1.5 - 2.5j, 1e6]                      # ties and saturation
    fin = _Frame(gpu, n_pol, n_dat * n_chan, 1, 5, 3, fill=NAN).put(x.reshape(n_pol, -1))
    t = orc._NBIT_NP[nbit]
    count = n_dat * n_chan * n_pol * 2
    out = torch.full((count + 16,), 0x55, dtype=torch.int8 if nbit == 8 else torch.int16, device=gpu)
    st = lib.pfb_dada_pack(c_void_p(fin.ptr), fin.stride, n_dat, n_chan, n_pol, c_void_p(out.data_ptr()), nbit,
                           _stream(gpu))
    torch.cuda.synchronize(gpu)
    assert st == OK, _err(lib)
    got = out.cpu().numpy()
    assert np.array_equal(got[:count], orc.write_dada_data(x.transpose(0, 2, 1), nbit).astype(t))
    assert (got[count:] == 0x55).all()
    assert fin.guards_intact(n_dat * n_chan)


@pytest.mark.parametrize("in_place", [False, True])
def test_quantize_gapped_strides(gpu, in_place):
    """pfb_quantize with gapped strides and an odd lead — pol rows that are not 16-B aligned,
    the scalar branches of moments_kernel and quantize_kernel (pfb_layout.hip, `vec`) — and
    with in == out.  The scale comes from double atomicAdd partial sums (moments_kernel's
    last lines), whose order varies, so values are held to test_quantize_rms_scale's bounds
    (scale within 1e-9 relative of orc.quantize_scale; at most one unit, at most 1e-4 of the
    samples differing) rather than to bit-identity.  A NaN read from between the pols would
    make the scale NaN."""
    import torch
    lib = _lib()
    n_pol, n, rms = 2, 40001, 33.8
    x = _noise(np.random.default_rng(620), (n_pol, n), scale=3.0) + np.complex64(0.25 - 0.5j)
    if in_place:
        fin = fout = _Frame(gpu, n_pol, n, 1, 5, 9).put(x)
    else:
        fin = _Frame(gpu, n_pol, n, 1, 3, 3, fill=NAN).put(x)
        fout = _Frame(gpu, n_pol, n, 3, 1, 9)
    assert fin.pol(1).data_ptr() % 16 == 8 or fin.pol(0).data_ptr() % 16 == 8
    sc = c_double(-1.0)
    st = lib.pfb_quantize(c_void_p(fin.ptr), fin.stride, n, n_pol, rms, c_void_p(fout.ptr), fout.stride, byref(sc),
                          _stream(gpu))
    torch.cuda.synchronize(gpu)
    assert st == OK, _err(lib)
    ref_sc = orc.quantize_scale(x, rms)
    assert abs(sc.value - ref_sc) <= 1e-9 * ref_sc, (sc.value, ref_sc)
    got = fout.get(n)
    assert _no_nan(got)
    d = np.abs(got.cpu().numpy() - orc.quantize(x, ref_sc))
    assert d.max() <= 1.0 and (d > 0).mean() < 1e-4
    assert fout.guards_intact(n)
    if not in_place:
        assert fin.guards_intact(n)
