"""Synthesis of strided channelised rows (pfb_synthesis_execute_strided,
pfb_inverse_filterbank_execute_strided): the channel IFFT's first pass loads element (pol,
row, chan) from in[pol ps + row rs + chan cs] (row_fft_strided_kernel) instead of from a
packed [pol][t][chan] copy.

The contract is bit-identity with the packed call on a contiguous copy of the mapped
elements, so every comparison against it is np.array_equal; only the oracle cases of the
two-stage inversion keep the project's 1e-6 (conftest.assert_pfb_close).  Every input is
noise scattered into a larger buffer whose unmapped elements are NaN: an output equal to the
reference holds no NaN, so no unmapped element was used, and the buffer must be bit-unchanged
after the call.  Shapes are the smallest that reach each path: a few hundred rows, two or
three blocks.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


@functools.lru_cache(maxsize=None)
def _taps(N, os_):
    taps = _pfb().design_PFB_FIR_filter(N, os_, 12)
    taps.setflags(write=False)
    return taps


def _noise(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def _plan(N, os_, nf, ov, n_pol, taper="tukey", spectral=None, deripple=False, spans=True, combine=1):
    pfb = _pfb()
    w = pfb.PFBWindow()
    return pfb.SynthesisPlan(N, os_, nf, ov, spans, combine, deripple, _taps(N, os_) if deripple else None,
                             w.lookup[taper](nf, ov), w.lookup[spectral](nf, ov) if spectral else None,
                             n_pol)


class Scattered:
    """Noise of shape (n_pol, rows, N) behind element strides (ps, rs, cs), `lead` elements
    into a NaN-filled device buffer with `tail` NaN elements after the furthest one."""

    def __init__(self, gpu, seed, shape, strides, lead=3, tail=5):
        import torch
        n_pol, rows, N = shape
        ps, rs, cs = strides
        self.need = (n_pol - 1) * ps + (rows - 1) * rs + (N - 1) * cs + 1
        self.packed = _noise(np.random.default_rng(seed), shape)
        host = np.full(lead + self.need + tail, np.nan + 1j * np.nan, dtype=np.complex64)
        mapped = np.lib.stride_tricks.as_strided(host[lead:], shape, tuple(8 * s for s in strides))
        mapped[...] = self.packed
        assert np.isnan(host).sum() == host.size - self.packed.size, "the strides overlap"
        self.host = host
        self.dev = torch.from_numpy(host).to(gpu)
        self.view = torch.as_strided(self.dev, shape, strides, lead)
        self.ref_in = torch.from_numpy(self.packed).to(gpu)      # the contiguous copy

    def assert_unchanged(self):
        assert np.array_equal(self.dev.cpu().numpy().view(np.uint64), self.host.view(np.uint64))


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


def _check(plan, sc, sample_offset, expect):
    """Packed call on the contiguous copy, then the strided call on the view."""
    ref = plan.execute(sc.ref_in, sample_offset=sample_offset, layout="ptc").cpu().numpy()
    assert plan.last_strided_input() == "none"
    got = plan.execute_view(sc.view, sample_offset=sample_offset).cpu().numpy()
    assert plan.last_strided_input() == expect
    assert ref.shape[1] >= 2 * plan.output_keep and np.abs(ref).max() > 0
    assert got.shape == ref.shape
    assert np.array_equal(got, ref)
    sc.assert_unchanged()
    return ref


# ------------------------------------------------------------------ 1. cascade slices
@pytest.mark.parametrize("critical,combine", [(False, 1), (True, 1), (True, 2)])
def test_cascade_slices_in_place(gpu, profiling, critical, combine):
    """The inverse cascade's layout (test_two_stage_inverse_matches_oracle's shapes): 4 coarse
    channels of nch_in = 16 / 14 / 28 fine channels interleaved in every row, 3 spare
    channels per row.  14 and 28 are mixed-radix sizes, combine 2 the permuted loader."""
    nch_in = (14 if critical else 16) * combine
    plan = _plan(nch_in, "8/7", 128, 16, 4, spans=not critical, combine=combine)
    sc = Scattered(gpu, 10 + nch_in, (4, 700, nch_in), (nch_in, 4 * nch_in + 3, 1))
    plan.execute(sc.ref_in, layout="ptc")
    packed_kernel = _kernel_name(1)
    _check(plan, sc, 1, "in_place")
    strided_kernel = _kernel_name(1)
    print(f"class 1: packed {packed_kernel!r}, strided {strided_kernel!r}")
    assert "row_fft_kernel<" in packed_kernel
    assert "row_fft_strided_kernel<" in strided_kernel and strided_kernel != packed_kernel
    # a packed call after a strided one: the diagnostic goes back to 'none'
    plan.execute(sc.ref_in, layout="ptc")
    assert plan.last_strided_input() == "none"


# ------------------------------------------------------------------ 2. the C2 kernels
def test_c2_interleaved_pols_in_place(gpu):
    """N 256, Nf 256: row_fft<256>, the 2-row-run Z and the wave synthesis; the two
    polarisations interleave inside each 512-channel row."""
    plan = _plan(256, "8/7", 256, 48, 2, deripple=True)
    sc = Scattered(gpu, 21, (2, 576, 256), (256, 512, 1))
    _check(plan, sc, 1, "in_place")


# ------------------------------------------------------------------ 3. channel-major rows
# (id, N, os, Nf, Ov, n_pol, rows, sample_offset)
CHANNEL_MAJOR = [
    # 512 rows per workgroup and 320 rows: one ragged workgroup, kept in range by the clamp
    ("n8", 8, "8/7", 128, 16, 2, 320, 1),
    # W = 192 and an odd first row
    ("n256-4over3", 256, "4/3", 256, 48, 1, 2 + 2 * 160 + 96 + 5, 3),
]


@pytest.mark.parametrize("case", CHANNEL_MAJOR, ids=lambda c: c[0])
def test_channel_major_in_place(gpu, case):
    _, N, os_, nf, ov, n_pol, rows, so = case
    plan = _plan(N, os_, nf, ov, n_pol)
    cs = rows + 5
    sc = Scattered(gpu, 30 + N, (n_pol, rows, N), (N * cs, 1, cs))
    _check(plan, sc, so, "in_place")


# ------------------------------------------------------------------ 4. staged plans
# (id, N, os, Nf, Ov, taper, spectral, n_pol, rows, row stride)
STAGED = [
    # the 4096-point pair kernels keep their descriptor loads: 2 blocks
    ("n4096", 4096, "8/7", 512, 128, "tukey", None, 1, 769, 4096 + 8),
    # the spectral path's six passes read `in` themselves
    ("spectral-hann", 8, "4/3", 128, 16, "tukey", "hann", 2, 3 * 96 + 32 + 5, 8 + 3),
    # a Hann temporal taper is a per-channel gain of the channel IFFT's loader
    ("temporal-hann-n56", 56, "8/7", 128, 16, "hann", None, 2, 3 * 96 + 32 + 5, 56 + 3),
]


@pytest.mark.parametrize("case", STAGED, ids=lambda c: c[0])
def test_staged_plans(gpu, case):
    _, N, os_, nf, ov, taper, spectral, n_pol, rows, rs = case
    plan = _plan(N, os_, nf, ov, n_pol, taper=taper, spectral=spectral)
    sc = Scattered(gpu, 40 + N, (n_pol, rows, N), (rows * rs + 7, rs, 1))
    _check(plan, sc, 2, "staged")


# ------------------------------------------------------------------ 5. stream
C2_CFG = dict(channels=256, os_factor="8/7", input_fft_length=256, input_overlap=48, deripple=False,
              temporal_taper="tukey")
STREAM_OFFSET = 5


def _stream_pair():
    pfb = _pfb()
    cfg = dict(C2_CFG, filt_coeff=_taps(256, "8/7"))
    a, b = pfb.InverseFilterBank(cfg), pfb.InverseFilterBank(cfg)
    a.sample_offset = b.sample_offset = STREAM_OFFSET
    return a, b


def _stream_input(gpu, seed, rows):
    # two polarisations interleaved in every row, one spare channel
    return Scattered(gpu, seed, (2, rows, 256), (256, 513, 1))


def _stream_chunk(gpu, ifb, ref_ifb, seed, rows):
    """One chunk through both objects: the view to one, its contiguous copy to the other."""
    sc = _stream_input(gpu, seed, rows)
    _, got = ifb.execute_view(sc.view)
    path = ifb._plan.last_strided_input()
    _, ref = ref_ifb.execute(sc.ref_in.transpose(1, 2))
    assert got.shape == ref.shape, (rows, got.shape, ref.shape)
    assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy()), rows
    assert ifb.buffered_samples == ref_ifb.buffered_samples, rows
    sc.assert_unchanged()
    return path, got.shape[2], ifb.buffered_samples


def test_stream_chunks_match_packed_stream(gpu):
    import torch
    from ska_pst_dsp_model_amd import _lib
    ifb, ref_ifb = _stream_pair()
    seen = []
    # 384 rows: nothing carried, every block in place; 32: no block completes (carry + chunk
    # concatenated); 224: both blocks start in the carry (stitched); 672: one stitched block,
    # three in place
    for i, rows in enumerate((384, 32, 224, 672)):
        seen.append(_stream_chunk(gpu, ifb, ref_ifb, 500 + i, rows))
    print(seen)
    assert [s[0] for s in seen] == ["in_place", "staged", "staged", "in_place"]
    assert [s[1] > 0 for s in seen] == [True, False, True, True]
    assert [s[2] for s in seen] == [224, 256, 160, 192], "carries of several lengths"

    # a call rejected for a short output capacity leaves both objects as they were ...
    sc = _stream_input(gpu, 510, 289)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    for obj, strided in ((ifb, True), (ref_ifb, False)):
        plan = obj._plan
        buffered = plan.buffered_samples
        width = plan.output_length(buffered + 289)
        assert width > 1
        sentinel = complex(-7.0, 7.0)
        out = torch.full((2, width), sentinel, dtype=torch.complex64, device=gpu)
        n_out = ctypes.c_int64(-1)
        if strided:
            st = plan._lib.pfb_inverse_filterbank_execute_strided(
                plan._h, ctypes.c_void_p(sc.view.data_ptr()), 256, 513, 1, sc.need, 289,
                ctypes.c_void_p(out.data_ptr()), width, 1, ctypes.byref(n_out), stream)
        else:
            st = plan._lib.pfb_inverse_filterbank_execute(
                plan._h, ctypes.c_void_p(sc.ref_in.data_ptr()), 289 * 256, 289,
                ctypes.c_void_p(out.data_ptr()), width, 1, ctypes.byref(n_out), _lib.PFB_MEM_DEVICE, stream)
        assert st == _lib.PFB_ERR_BUFFER_TOO_SMALL
        assert n_out.value > 1
        assert plan.buffered_samples == buffered == 192
        assert bool((out == sentinel).all())
    # ... and the retry returns what the call would have
    _, got = ifb.execute_view(sc.view)
    _, ref = ref_ifb.execute(sc.ref_in.transpose(1, 2))
    assert got.shape == ref.shape and got.shape[2] > 0
    assert np.array_equal(got.cpu().numpy(), ref.cpu().numpy())
    assert ifb.buffered_samples == ref_ifb.buffered_samples
    sc.assert_unchanged()


# ------------------------------------------------------------------ 6. TwoStageInverseFilterBank
def _two_stage(critical, combine, taper, strided_input):
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(16, "8/7", 10)
    cfg = dict(filt_coeff=taps, channels=16, os_factor="8/7", input_fft_length=128,
               input_overlap=16, deripple=False, temporal_taper="tukey")
    nch2 = 14 if critical else 16
    ti = pfb.TwoStageInverseFilterBank(cfg)
    ti.nch2 = nch2
    ti.combine = combine
    ti.strided_input = strided_input
    if taper:
        ti.frequency_taper(taper)

    def factory():
        o = orc.InverseFilterBankOracle(taps, 16, "8/7", 128, 16, "tukey")
        return o.frequency_taper(taper) if taper else o

    return ti, orc.TwoStageInverseFilterBankOracle(factory, nch2, combine=combine), nch2


TWO_STAGE = [(False, 1, None), (True, 1, None), (True, 2, None), (True, 2, "hann")]


@functools.lru_cache(maxsize=None)
def _two_stage_inputs(nch2):
    rng = np.random.default_rng(22 + nch2)
    return tuple(_noise(rng, (1, 4 * nch2, n)) for n in (700, 450))   # shared: never written


@pytest.mark.parametrize("critical,combine,taper", TWO_STAGE)
def test_two_stage_inverse_without_gather(gpu, monkeypatch, critical, combine, taper):
    """The strided path makes no Python-level gather, and matches the oracle."""
    from ska_pst_dsp_model_amd import layout

    def no_gather(*a, **k):
        raise AssertionError("layout.gather_channels called on the strided path")

    monkeypatch.setattr(layout, "gather_channels", no_gather)
    ti, oti, nch2 = _two_stage(critical, combine, taper, True)
    for x in _two_stage_inputs(nch2):
        ti, got = ti.execute(x)
        ref = oti.execute(x)
        assert got.shape[2] > 0
        assert_pfb_close(got, ref, what=f"two-stage inverse, strided input, n={x.shape[2]}")
        assert ti.stage2._plan.last_strided_input() == ("staged" if taper else "in_place")


@pytest.mark.parametrize("critical,combine,taper", TWO_STAGE)
def test_two_stage_inverse_equals_gather_path(gpu, critical, combine, taper):
    a, _, nch2 = _two_stage(critical, combine, taper, True)
    b, _, _ = _two_stage(critical, combine, taper, False)
    for x in _two_stage_inputs(nch2):
        a, got = a.execute(x)
        b, ref = b.execute(x)
        assert got.shape == ref.shape and got.shape[2] > 0
        assert np.array_equal(got, ref)
        assert b.stage2._plan.last_strided_input() == "none"


# ------------------------------------------------------------------ 7. argument checks
def test_argument_checks(gpu):
    import torch
    from ska_pst_dsp_model_amd import _lib
    plan = _plan(8, "8/7", 128, 16, 2)
    rows, rs, ps = 320, 8 + 3, 320 * 11 + 7
    sc = Scattered(gpu, 70, (2, rows, 8), (ps, rs, 1))
    width = plan.output_length(rows)
    sentinel = complex(-7.0, 7.0)
    out = torch.full((2, width), sentinel, dtype=torch.complex64, device=gpu)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    src, dst = ctypes.c_void_p(sc.view.data_ptr()), ctypes.c_void_p(out.data_ptr())
    n_out = ctypes.c_int64(-1)

    def stateless(ps_, rs_, cs_, in_cap, cap=width):
        return plan._lib.pfb_synthesis_execute_strided(plan._h, src, ps_, rs_, cs_, in_cap, rows, 1, dst,
                                                       width, cap, ctypes.byref(n_out), stream)

    def stream_call(ps_, rs_, cs_, in_cap, cap=width):
        return plan._lib.pfb_inverse_filterbank_execute_strided(plan._h, src, ps_, rs_, cs_, in_cap, rows,
                                                                dst, width, cap, ctypes.byref(n_out), stream)

    for call in (stateless, stream_call):
        for bad in ((0, rs, 1), (ps, 0, 1), (ps, rs, 0), (-ps, rs, 1), (ps, -rs, 1), (ps, rs, -1)):
            assert call(*bad, sc.need) == _lib.PFB_ERR_INVALID_ARG, bad
        assert call(ps, rs, 1, sc.need - 1) == _lib.PFB_ERR_INVALID_ARG      # one element short
        assert call(ps, rs, 1, sc.need, cap=width - 1) == _lib.PFB_ERR_BUFFER_TOO_SMALL
        torch.cuda.synchronize()
        assert bool((out == sentinel).all()), "a rejected call wrote"
        assert plan.buffered_samples == 0
    # the exact capacity is accepted, by both, and the stream call then holds a carry
    ref = plan.execute(sc.ref_in, layout="ptc").cpu().numpy()
    assert stateless(ps, rs, 1, sc.need) == _lib.PFB_OK and n_out.value == width
    assert np.array_equal(out.cpu().numpy(), ref)
    assert stream_call(ps, rs, 1, sc.need) == _lib.PFB_OK and n_out.value == width
    assert np.array_equal(out.cpu().numpy(), ref)
    assert plan.buffered_samples == rows - 3 * 96
    sc.assert_unchanged()
