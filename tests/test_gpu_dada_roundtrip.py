"""The round trip from file bytes to file bytes (pfb_roundtrip_execute_dada_to_dada and its two
halves): a single-channel DADA section in, the channelised file's float section and the output
file's section out.  FUSED, one analysis launch (analysis_stream_rt_dada_kernel) reads the
section, stores the product section and emits the stage-1 rows, and the wave synthesis
(synth_wave_dadaout_kernel) stores the output section.

The contract is bit-identity with the sequence pfb_dada_unpack -> pfb_roundtrip_execute ->
pfb_dada_pack(32) of the product -> both components of the output times float32(scale) ->
pfb_dada_pack: "the pair" below, built from the existing calls.  Every comparison against it is
np.array_equal on bytes, under a scale at which the pair's own integer output saturates at both
ends and rounds in both directions (asserted).  Both sections are framed by a byte pattern that
must survive.  The shapes are the smallest that exercise the kernel: K = 613 rows (not a
multiple of the 16-row step), 3 synthesis blocks and a ragged tail.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

PAT = 0xA5          # the frames' byte
FRAME = 512         # bytes of frame on each side of a section (keeps its alignment)
SPARE_ROWS = 2      # product capacity beyond the rows due, pattern-filled
SPARE_SAMPLES = 5   # output capacity beyond the samples due, pattern-filled
NF, OV, KEEP = 256, 48, 160
ROWS = 613          # 38 steps of 16 rows and 5 more; 3 blocks at sample_offset 1 and 17
OK, INVALID, UNSUPPORTED, TOO_SMALL = 0, 1, 2, 5


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


@functools.lru_cache(maxsize=None)
def _taps(N, os_, tpc, cut=None):
    taps = _pfb().design_PFB_FIR_filter(N, os_, tpc)
    if cut:
        taps = taps[:cut].copy()
    taps.setflags(write=False)
    return taps


def _n_dat(n_taps, N, os_, rows, extra):
    """Samples that give `rows` rows of a stateless Bunton call, and a ragged tail."""
    nu, de = (int(v) for v in os_.split("/"))
    return -(-n_taps // N) * N + rows * (N * de // nu) + extra


N_DAT = _n_dat(3073, 256, "8/7", ROWS, 5)
assert N_DAT == 3328 + 224 * 613 + 5


def _plans(n_pol, os_="8/7", cut=None, N=256, tpc=12, variant="polyphase_analysis", nf=NF, ov=OV, spectral=None,
           chunk=0):
    pfb = _pfb()
    taps = _taps(N, os_, tpc, cut)
    w = pfb.PFBWindow()
    ana = pfb.AnalysisPlan(taps, N, os_, variant, n_pol, 0)
    syn = pfb.SynthesisPlan(N, os_, nf, ov, True, 1, True, taps, w.lookup["tukey"](nf, ov),
                            w.lookup[spectral](nf, ov) if spectral else None, n_pol, 0)
    if chunk:
        syn.set_chunk_blocks(chunk)
    return ana, syn


def _file_samples(rng, nbit, count):
    """Samples over the full range of the file's type (floats: unit variance)."""
    t = orc._NBIT_NP[nbit]
    if np.issubdtype(t, np.integer):
        info = np.iinfo(t)
        return rng.integers(info.min, info.max + 1, size=count).astype(t)
    return rng.standard_normal(count).astype(t)


def _section(gpu, seed, nbit, n_dat, n_pol, ndim=2, lead=0):
    """A single-channel section on the device, `lead` spare bytes in front of it."""
    import torch
    raw = _file_samples(np.random.default_rng(seed), nbit, n_dat * n_pol * ndim)
    host = np.concatenate([np.zeros(lead, np.uint8), raw.view(np.uint8)])
    return torch.from_numpy(host).to(gpu)[lead:]


def _pair(ana, syn, rawd, nbit, so=1, ndim=2):
    """The sequence's first three steps through the existing calls: pfb_dada_unpack, the cf32
    round trip, pfb_dada_pack(32) of the product.  -> (product section bytes, cf32 output)"""
    import torch
    from ska_pst_dsp_model_amd import layout
    x = layout.dada_unpack(rawd, nbit, ndim, 1, ana.n_pol)[:, :, 0].contiguous()
    chan, out = _pfb().roundtrip(ana, syn, x, sample_offset=so)
    sec = layout.dada_pack(chan, 32)
    torch.cuda.synchronize()
    return sec.cpu().numpy().view(np.uint8), out


def _pack_pair(out, nbit, scale):
    """The sequence's last two steps: both components times float32(scale), pfb_dada_pack with
    one channel.  `out`: the (n_pol, n_out) complex64 device series -> the section's bytes."""
    import torch
    from ska_pst_dsp_model_amd import layout
    scaled = torch.view_as_complex((torch.view_as_real(out.contiguous()) * float(np.float32(scale))).contiguous())
    return layout.dada_pack(scaled[:, :, None], nbit).cpu().numpy().view(np.uint8)


def _scale_for(ref, nbit):
    """A float32 scale, not a power of two, that puts the 97th percentile of the series'
    component magnitudes at the end of the integer range: about three per cent of them
    saturate, whatever their distribution (a round trip returns its input's: uniform for the
    integer sections, Gaussian for the float ones)."""
    comp = np.abs(ref.view(np.float32).ravel().astype(np.float64))
    full = 1.11 if nbit in (32, 64) else float(np.iinfo(orc._NBIT_NP[nbit]).max)
    scale = np.float32(full / np.quantile(comp, 0.97))
    assert np.frexp(scale)[0] != 0.5
    return float(scale)


def _assert_pair_is_demanding(ref, pair_bytes, nbit, scale):
    """Saturation at both ends and both rounding directions occur in the pair's own output."""
    if nbit in (32, 64):
        return
    t = orc._NBIT_NP[nbit]
    info = np.iinfo(t)
    v = (np.float32(scale) * ref.T.reshape(-1).view(np.float32)).astype(np.float64)   # TFP order, float32 product
    q = pair_bytes.view(t).astype(np.float64)
    assert q.shape == v.shape
    hi, lo = v > info.max + 1, v < info.min - 1
    assert hi.any() and (q[hi] == info.max).all() and lo.any() and (q[lo] == info.min).all()
    inside = np.abs(v) < info.max
    frac = np.abs(v) - np.floor(np.abs(v))
    up, down = inside & (frac > 0.5), inside & (frac < 0.5) & (frac > 0)
    assert up.any() and (np.abs(q[up]) == np.floor(np.abs(v[up])) + 1).all()
    assert down.any() and (np.abs(q[down]) == np.floor(np.abs(v[down]))).all()


def _kernel_name(which):
    from ska_pst_dsp_model_amd import _lib
    buf = ctypes.create_string_buffer(1024)
    assert _lib.load().pfb_profile_kernel_name(which, buf, len(buf)) == 0
    return buf.value.decode()


def _launches(lib, which):
    ms, n, b = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
    assert lib.pfb_profile_read(which, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(b)) == 0
    return n.value


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


def _lengths(ana, syn, n_dat, so):
    K = ana.output_length(n_dat)
    return K, syn.output_length(max(K - (so - 1), 0))


def _paths(ana, syn):
    return ana.last_dada_input(), ana.last_dada_output(), syn.last_dada_output()


class _Framed:
    """A device buffer of `cap` bytes between two frames, all pattern-filled."""

    def __init__(self, gpu, cap, offset=0):
        import torch
        self.holder = torch.full((FRAME + offset + cap + FRAME,), PAT, dtype=torch.uint8, device=gpu)
        assert self.holder.data_ptr() % 16 == 0
        self.off, self.cap = FRAME + offset, cap
        self.ptr = ctypes.c_void_p(self.holder.data_ptr() + self.off)

    def written(self, nbytes, what=""):
        """The first nbytes of the section; everything else must still be the pattern."""
        h = self.holder.cpu().numpy()
        assert (h[:self.off] == PAT).all(), f"{what}: bytes before the section were written"
        assert (h[self.off + nbytes:] == PAT).all(), f"{what}: bytes beyond the section's end were written"
        return h[self.off:self.off + nbytes]


def _call(ana, syn, gpu, rawd, nbit, out_nbit, scale, so=1, ndim=2, order=0, n_dat=None, chan_off=0, out_off=0,
          chan_cap=None, out_cap=None, which="whole"):
    """One raw C-ABI call into framed sections; the capacities default to what is due plus the
    spare rows / samples.  -> (status, n_chan_rows, n_out, framed chan, framed out)"""
    import torch
    lib = ana._lib
    P = ana.n_pol
    if n_dat is None:
        n_dat = rawd.numel() // (P * ndim * (nbit // 8))
    K, olen = _lengths(ana, syn, n_dat, so)
    sb = P * 2 * (out_nbit // 8) if out_nbit in (8, 16, 32, 64) else P * 2
    chan = _Framed(gpu, (K + SPARE_ROWS) * ana.n_chan * P * 8 if chan_cap is None else chan_cap, chan_off)
    out = _Framed(gpu, (olen + SPARE_SAMPLES) * sb if out_cap is None else out_cap, out_off)
    k, n = ctypes.c_int64(-1), ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    src = ctypes.c_void_p(rawd.data_ptr()) if rawd is not None else None
    if which == "whole":
        st = lib.pfb_roundtrip_execute_dada_to_dada(ana._h, syn._h, src, nbit, ndim, order, n_dat, chan.ptr, chan.cap,
                                                    ctypes.byref(k), so, out.ptr, out_nbit, scale, out.cap,
                                                    ctypes.byref(n), stream)
    elif which == "analysis":
        st = lib.pfb_roundtrip_analysis_execute_dada(ana._h, syn._h, src, nbit, ndim, order, n_dat, chan.ptr, chan.cap,
                                                     ctypes.byref(k), so, stream)
    else:
        st = lib.pfb_roundtrip_synthesis_execute_to_dada(ana._h, syn._h, n_dat, so, out.ptr, out_nbit, scale, out.cap,
                                                         ctypes.byref(n), stream)
    torch.cuda.synchronize(gpu)
    return st, k.value, n.value, chan, out


def _check_against_pair(ana, syn, gpu, rawd, nbit, out_nbit, so, paths, ndim=2, what="", **kw):
    """The pair, then the call on the same plans: sections, lengths and the reported paths."""
    n_dat = rawd.numel() // (ana.n_pol * ndim * (nbit // 8))
    K, olen = _lengths(ana, syn, n_dat, so)
    assert K > 0 and olen > 0, what
    chan_ref, out_ref = _pair(ana, syn, rawd, nbit, so, ndim)
    cf32_kernels = (_kernel_name(3), _kernel_name(2))
    refh = out_ref.cpu().numpy()
    assert tuple(refh.shape) == (ana.n_pol, olen) and chan_ref.size == K * ana.n_chan * ana.n_pol * 8
    scale = _scale_for(refh, out_nbit)
    pair = _pack_pair(out_ref, out_nbit, scale)
    _assert_pair_is_demanding(refh, pair, out_nbit, scale)
    st, k, n, chan, out = _call(ana, syn, gpu, rawd, nbit, out_nbit, scale, so=so, ndim=ndim, **kw)
    assert (st, k, n) == (OK, K, olen), (what, st, k, n, ana._lib.pfb_last_error())
    assert _paths(ana, syn) == paths, (what, _paths(ana, syn))
    assert syn.last_stage1_rows == "stored", what
    assert np.array_equal(chan.written(chan_ref.size, what + " chan"), chan_ref), what + ": product section"
    assert np.array_equal(out.written(pair.size, what + " out"), pair), what + ": output section"
    return scale, chan_ref, pair, cf32_kernels


def _torch_type(nbit):
    import torch
    return {8: torch.int8, 16: torch.int16, 32: torch.float32, 64: torch.float64}[nbit]


FUSED =("fused", "fused", "fused")
STAGED = ("staged", "staged", "staged")


# ------------------------------------------------------------------ 1. FUSED == the pair, framed
@pytest.mark.parametrize("n_pol", [1, 2], ids=["1pol", "2pol"])
@pytest.mark.parametrize("out_nbit", [8, 16, 32], ids=["out8", "out16", "out32"])
@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["in8", "in16", "in32"])
def test_fused_matches_the_pair(gpu, profiling, nbit, out_nbit, n_pol):
    """Sections equal to the pair's at sample_offset 1 and 17, framed (case 2: rows past K and
    samples past n_out included), lengths, all three diagnostics, and the kernels launched."""
    ana, syn = _plans(n_pol)
    rawd = _section(gpu, 3000 + 7 * nbit + n_pol, nbit, N_DAT, n_pol)
    for so in (1, 17):
        what = f"in {nbit} out {out_nbit} {n_pol} pol offset {so}"
        profiling.pfb_profile_reset()
        cf32 = _check_against_pair(ana, syn, gpu, rawd, nbit, out_nbit, so, FUSED, what=what)[3]
        ak, sk = _kernel_name(3), _kernel_name(2)
        print(f"{what}: class 3 {cf32[0]!r} -> {ak!r}, class 2 {cf32[1]!r} -> {sk!r}")
        # the pair's cf32 round trip takes the path the call fuses: the streaming analysis with
        # 2-row runs and the wave kernel
        assert "analysis_stream_kernel<256, 13, 8, 7, 2," in cf32[0] and "synth_wave_kernel<14, true," in cf32[1]
        assert "analysis_stream_rt_dada_kernel<256, 13, 8, 7," in ak and f"InDada{nbit}>" in ak
        assert "synth_wave_dadaout_kernel<14, true, true," in sk and f"OutDada{out_nbit}>" in sk
        # one analysis and one synthesis launch each for the pair and the call, and neither a
        # plain analysis nor a channel IFFT
        assert (_launches(profiling, 3), _launches(profiling, 2)) == (2, 2)
        assert _launches(profiling, 0) == 0 and _launches(profiling, 1) == 0


@pytest.mark.parametrize("cut", [None, 3072], ids=["13phases", "12phases"])
def test_fused_4over3(gpu, profiling, cut):
    ana, syn = _plans(2, os_="4/3", cut=cut)
    n_dat = _n_dat(cut or 3073, 256, "4/3", ROWS, 5)
    rawd = _section(gpu, 3100 + (cut or 0), 16, n_dat, 2)
    _check_against_pair(ana, syn, gpu, rawd, 16, 8, 17, FUSED, what=f"4/3 cut {cut}")
    ak, sk = _kernel_name(3), _kernel_name(2)
    assert f"analysis_stream_rt_dada_kernel<256, {12 if cut else 13}, 4, 3," in ak and "InDada16>" in ak
    assert "synth_wave_dadaout_kernel<12, true, true," in sk and "OutDada8>" in sk


def test_python_surface(gpu):
    """roundtrip_dada: shapes, dtypes, scale 1.0 and every out_nbit."""
    pfb = _pfb()
    ana, syn = _plans(2)
    rawd = _section(gpu, 3200, 16, N_DAT, 2)
    chan_ref, out_ref = _pair(ana, syn, rawd, 16)
    K, olen = _lengths(ana, syn, N_DAT, 1)
    for out_nbit, dtype in ((8, "torch.int8"), (16, "torch.int16"), (32, "torch.float32"), (64, "torch.float64")):
        scale = _scale_for(out_ref.cpu().numpy(), out_nbit) if out_nbit != 32 else 1.0
        chan, out = pfb.roundtrip_dada(ana, syn, rawd.view(_torch_type(16)), 16, out_nbit, scale=scale)
        assert _paths(ana, syn) == (FUSED if out_nbit != 64 else STAGED)
        assert tuple(chan.shape) == (K, 256, 2, 2) and str(chan.dtype) == "torch.float32"
        assert tuple(out.shape) == (olen, 1, 2, 2) and str(out.dtype) == dtype
        assert np.array_equal(chan.cpu().numpy().view(np.uint8).ravel(), chan_ref)
        assert np.array_equal(out.cpu().numpy().view(np.uint8).ravel(), _pack_pair(out_ref, out_nbit, scale))


def test_fused_call_replays_from_a_graph(gpu):
    """The FUSED call is capturable (its checks allocate nothing once the rows exist): one
    replay fills both framed sections with the pair's bytes."""
    import torch
    ana, syn = _plans(2)
    rawd = _section(gpu, 3250, 16, N_DAT, 2)
    chan_ref, out_ref = _pair(ana, syn, rawd, 16, 17)
    scale = _scale_for(out_ref.cpu().numpy(), 16)
    pair = _pack_pair(out_ref, 16, scale)
    chan, out = _Framed(gpu, chan_ref.size), _Framed(gpu, pair.size)
    k, n = ctypes.c_int64(-1), ctypes.c_int64(-1)

    def call():
        stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
        st = ana._lib.pfb_roundtrip_execute_dada_to_dada(
            ana._h, syn._h, ctypes.c_void_p(rawd.data_ptr()), 16, 2, 0, N_DAT, chan.ptr, chan.cap, ctypes.byref(k), 17,
            out.ptr, 16, scale, out.cap, ctypes.byref(n), stream)
        assert st == OK and _paths(ana, syn) == FUSED

    call()                                                  # eager warm-up: the stage-1 rows exist
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    chan.holder.fill_(PAT)
    out.holder.fill_(PAT)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(chan.written(chan_ref.size, "replayed chan"), chan_ref)
    assert np.array_equal(out.written(pair.size, "replayed out"), pair)


# ------------------------------------------------------------------ 3. STAGED == the pair, framed
def test_staged_other_offset(gpu):
    ana, syn = _plans(2)
    _check_against_pair(ana, syn, gpu, _section(gpu, 3300, 16, N_DAT, 2), 16, 16, 2, STAGED, what="offset 2")


def test_staged_nbit64_out(gpu):
    ana, syn = _plans(2)
    _check_against_pair(ana, syn, gpu, _section(gpu, 3301, 8, N_DAT, 2), 8, 64, 1, STAGED, what="NBIT 64 out")


def test_staged_ndim1_in(gpu):
    ana, syn = _plans(2)
    rawd = _section(gpu, 3302, 16, N_DAT, 2, ndim=1)
    _check_against_pair(ana, syn, gpu, rawd, 16, 16, 1, STAGED, ndim=1, what="NDIM 1 in")


@pytest.mark.parametrize("n_pol", [1, 2], ids=["1pol", "2pol"])
def test_staged_out_aligned_to_a_value_only(gpu, n_pol):
    """`out` one value past a complex-sample boundary (and, with one polarisation, a product
    section the cf32 round trip writes straight into)."""
    ana, syn = _plans(n_pol)
    rawd = _section(gpu, 3303 + n_pol, 16, N_DAT, n_pol)
    _check_against_pair(ana, syn, gpu, rawd, 16, 16, 1, STAGED, out_off=2, what="out offset by one value")


def test_staged_chan_aligned_to_a_value_only(gpu):
    ana, syn = _plans(1)
    rawd = _section(gpu, 3306, 16, N_DAT, 1)
    _check_against_pair(ana, syn, gpu, rawd, 16, 16, 1, STAGED, chan_off=4, what="chan offset by one float")


def test_staged_spectral_taper(gpu):
    """N 8, os 4/3, Nf 128, Ov 16 with a Hann spectral taper (test_gpu_dada_synthesis_output.py's
    spectral pair)."""
    ana, syn = _plans(2, os_="4/3", N=8, tpc=10, nf=128, ov=16, spectral="hann")
    _check_against_pair(ana, syn, gpu, _section(gpu, 3307, 16, 9000, 2), 16, 8, 1, STAGED, what="spectral taper")


def test_staged_chunk_size_set(gpu):
    ana, syn = _plans(2, chunk=2)
    _check_against_pair(ana, syn, gpu, _section(gpu, 3308, 16, N_DAT, 2), 16, 16, 17, STAGED, what="chunk 2")


def test_staged_padded_small_pair(gpu):
    """N 8, os 8/7, padded, Nf 128, Ov 16 (test_gpu_roundtrip.py's smallest pair)."""
    ana, syn = _plans(2, N=8, tpc=10, variant="polyphase_analysis_padded", nf=128, ov=16)
    _check_against_pair(ana, syn, gpu, _section(gpu, 3309, 16, 9000, 2), 16, 16, 3, STAGED, what="padded N 8")


def test_staged_n512_pair(gpu):
    """N 512, Nf 512, Ov 128, padded: the second row of test_gpu_roundtrip.py's split-halves
    table (register-window FIR + row FFT + the Nf 512 wave kernel)."""
    ana, syn = _plans(2, N=512, variant="polyphase_analysis_padded", nf=512, ov=128)
    n_dat = (3 * 256 + 2 * 128 + 5) * 448
    _check_against_pair(ana, syn, gpu, _section(gpu, 3310, 16, n_dat, 2), 16, 16, 1, STAGED, what="N 512")


# ------------------------------------------------------------------ 4. halves
@pytest.mark.parametrize("n_pol,nbit,out_nbit,so", [(2, 16, 16, 17), (1, 8, 32, 1), (2, 32, 8, 2)],
                         ids=["fused-2pol", "fused-1pol", "staged-offset2"])
def test_halves_equal_the_whole_call(gpu, n_pol, nbit, out_nbit, so):
    import torch
    pfb = _pfb()
    ana, syn = _plans(n_pol)
    rawd = _section(gpu, 3400 + nbit, nbit, N_DAT, n_pol)
    typed = rawd.view(_torch_type(nbit))
    chan_ref, out_ref = _pair(ana, syn, rawd, nbit, so)
    scale = _scale_for(out_ref.cpu().numpy(), out_nbit)
    pair = _pack_pair(out_ref, out_nbit, scale)
    want = FUSED if so != 2 else STAGED
    chan_w, out_w = pfb.roundtrip_dada(ana, syn, typed, nbit, out_nbit, scale=scale, sample_offset=so)
    assert _paths(ana, syn) == want
    whole = (chan_w.cpu().numpy().view(np.uint8).ravel(), out_w.cpu().numpy().view(np.uint8).ravel())
    assert np.array_equal(whole[0], chan_ref) and np.array_equal(whole[1], pair)
    # the whole call reused the pair's rows: the synthesis half alone is refused
    with pytest.raises(pfb.PfbError):
        pfb.roundtrip_synthesis_to_dada(ana, syn, N_DAT, out_nbit, scale=scale, sample_offset=so)
    # DADA analysis half + to-DADA synthesis half, on two streams ordered by an event
    ana2, syn2 = _plans(n_pol)
    chan = pfb.roundtrip_analysis_dada(ana2, syn2, typed, nbit, sample_offset=so)
    assert (ana2.last_dada_input(), ana2.last_dada_output()) == want[:2]
    ev, ss = torch.cuda.Event(), torch.cuda.Stream()
    ev.record(torch.cuda.current_stream())
    ss.wait_event(ev)
    with torch.cuda.stream(ss):
        out = pfb.roundtrip_synthesis_to_dada(ana2, syn2, N_DAT, out_nbit, scale=scale, sample_offset=so)
    torch.cuda.synchronize()
    assert syn2.last_dada_output() == want[2] and syn2.last_stage1_rows == "stored"
    assert np.array_equal(chan.cpu().numpy().view(np.uint8).ravel(), whole[0])
    assert np.array_equal(out.cpu().numpy().view(np.uint8).ravel(), whole[1])
    # cf32 analysis half + to-DADA synthesis half == the pair
    from ska_pst_dsp_model_amd import layout
    x = layout.dada_unpack(rawd, nbit, 2, 1, n_pol)[:, :, 0].contiguous()
    ana3, syn3 = _plans(n_pol)
    c3 = pfb.roundtrip_analysis(ana3, syn3, x, sample_offset=so)
    out = pfb.roundtrip_synthesis_to_dada(ana3, syn3, N_DAT, out_nbit, scale=scale, sample_offset=so)
    torch.cuda.synchronize()
    assert syn3.last_dada_output() == want[2]
    assert np.array_equal(layout.dada_pack(c3, 32).cpu().numpy().view(np.uint8), chan_ref)
    assert np.array_equal(out.cpu().numpy().view(np.uint8).ravel(), pair)
    # DADA analysis half + cf32 synthesis half: the rows and the key are the same
    chan = pfb.roundtrip_analysis_dada(ana2, syn2, typed, nbit, sample_offset=so)
    o2 = pfb.roundtrip_synthesis(ana2, syn2, N_DAT, sample_offset=so)
    torch.cuda.synchronize()
    assert torch.equal(o2, out_ref)


def test_synthesis_half_rejects_another_call(gpu):
    """Another n_dat or sample_offset than the analysis half's: PFB_ERR_INVALID_ARG, nothing
    written; the matching call still works afterwards."""
    ana, syn = _plans(2)
    rawd = _section(gpu, 3450, 16, N_DAT, 2)
    _, out_ref = _pair(ana, syn, rawd, 16, 17)
    st, k, _, chan, _ = _call(ana, syn, gpu, rawd, 16, 16, 1.0, so=17, which="analysis")
    assert (st, k) == (OK, ROWS)
    for n_dat, so in ((N_DAT - 224, 17), (N_DAT, 1), (N_DAT, 33)):
        st, _, n, _, out = _call(ana, syn, gpu, None, 16, 16, 1.0, so=so, n_dat=n_dat, which="synthesis")
        assert st == INVALID, (n_dat, so, st)
        out.written(0, f"rejected synthesis half ({n_dat}, {so})")
    st, _, n, _, out = _call(ana, syn, gpu, None, 16, 16, 1.0, so=17, n_dat=N_DAT, which="synthesis")
    assert (st, n) == (OK, out_ref.shape[1])
    assert np.array_equal(out.written(n * 8), _pack_pair(out_ref, 16, 1.0))


def test_halves_of_a_chunked_pair_are_unsupported(gpu):
    ana, syn = _plans(2, chunk=2)
    rawd = _section(gpu, 3460, 16, N_DAT, 2)
    st, _, _, chan, _ = _call(ana, syn, gpu, rawd, 16, 16, 1.0, which="analysis")
    assert st == UNSUPPORTED
    chan.written(0, "analysis half of a chunked pair")
    st, _, _, _, out = _call(ana, syn, gpu, None, 16, 16, 1.0, n_dat=N_DAT, which="synthesis")
    assert st == UNSUPPORTED
    out.written(0, "synthesis half of a chunked pair")


# ------------------------------------------------------------------ 5. rejections
@pytest.mark.parametrize("so,paths", [(1, "fused"), (2, "staged")])
def test_capacity_one_byte_short(gpu, so, paths):
    ana, syn = _plans(2)
    rawd = _section(gpu, 3500, 16, N_DAT, 2)
    K, olen = _lengths(ana, syn, N_DAT, so)
    chan_need, out_need = K * 256 * 2 * 8, olen * 2 * 2 * 2
    for kw in (dict(chan_cap=chan_need - 1), dict(out_cap=out_need - 1)):
        st, k, n, chan, out = _call(ana, syn, gpu, rawd, 16, 16, 1.0, so=so, **kw)
        assert (st, k, n) == (TOO_SMALL, K, olen), (kw, st, k, n)
        chan.written(0, f"{kw} chan")
        out.written(0, f"{kw} out")
    st, k, _, chan, _ = _call(ana, syn, gpu, rawd, 16, 16, 1.0, so=so, chan_cap=chan_need - 1, which="analysis")
    assert (st, k) == (TOO_SMALL, K)
    chan.written(0, "analysis half")
    # exactly enough is enough
    st, k, n, chan, out = _call(ana, syn, gpu, rawd, 16, 16, 1.0, so=so, chan_cap=chan_need, out_cap=out_need)
    assert (st, k, n) == (OK, K, olen)
    assert _paths(ana, syn) == (FUSED if paths == "fused" else STAGED)
    assert (chan.written(chan_need) != PAT).any() and (out.written(out_need) != PAT).any()


def test_bad_arguments(gpu):
    ana, syn = _plans(2)
    rawd = _section(gpu, 3510, 16, N_DAT, 2, lead=16)
    for what, kw in (("NaN scale", dict(scale=float("nan"))), ("infinite scale", dict(scale=float("inf"))),
                     ("nbit 12", dict(nbit=12)), ("ndim 3", dict(ndim=3)), ("order 5", dict(order=5)),
                     ("out_nbit 24", dict(out_nbit=24)), ("offset 0", dict(so=0)),
                     ("chan misaligned", dict(chan_off=2)), ("out misaligned", dict(out_off=1))):
        a = dict(nbit=16, out_nbit=16, scale=1.0, n_dat=N_DAT)
        a.update(kw)
        st, k, n, chan, out = _call(ana, syn, gpu, rawd, a.pop("nbit"), a.pop("out_nbit"), a.pop("scale"), **a)
        assert st == INVALID, (what, st)
        chan.written(0, what)
        out.written(0, what)
    # `in` one byte past an int16 boundary
    import torch
    odd = torch.zeros(rawd.numel() + 1, dtype=torch.uint8, device=gpu)[1:]
    assert odd.data_ptr() % 2 == 1
    for which in ("whole", "analysis"):
        st, _, _, chan, out = _call(ana, syn, gpu, odd, 16, 16, 1.0, n_dat=N_DAT, which=which)
        assert st == INVALID, which
        chan.written(0, "misaligned in")
    # plans that do not belong together, and the LowCBF filterbank
    _, syn1 = _plans(1)
    st, _, _, _, _ = _call(ana, syn1, gpu, rawd, 16, 16, 1.0, n_dat=N_DAT)
    assert st == INVALID
    pfb = _pfb()
    low = pfb.AnalysisPlan(pfb.read_fir_filter_coeff(pfb.config.config_dir + "/PST_filtertaps.txt"), 256, "4/3",
                           "polyphase_analysis_lowcbf", 2)
    st = ana._lib.pfb_roundtrip_execute_dada_to_dada(low._h, syn._h, ctypes.c_void_p(rawd.data_ptr()), 16, 2, 0, 4096,
                                                     None, 0, None, 1, None, 16, 1.0, 0, None, None)
    assert st == UNSUPPORTED


def test_in_aligned_to_a_value_only_is_staged(gpu):
    """`in` on an int16 boundary that is no complex-sample boundary: accepted, STAGED."""
    ana, syn = _plans(1)
    rawd = _section(gpu, 3520, 16, N_DAT, 1, lead=2)
    assert rawd.data_ptr() % 4 == 2
    _check_against_pair(ana, syn, gpu, rawd, 16, 16, 1, STAGED, what="in offset by one value")


def test_too_short_for_a_block(gpu):
    """Rows but no synthesis block: the product section alone, nothing of `out` touched."""
    ana, syn = _plans(2)
    n_dat = _n_dat(3073, 256, "8/7", 50, 3)
    rawd = _section(gpu, 3530, 16, n_dat, 2)
    from ska_pst_dsp_model_amd import layout
    x = layout.dada_unpack(rawd, 16, 2, 1, 2)[:, :, 0].contiguous()
    ref = layout.dada_pack(ana.execute(x), 32).cpu().numpy().view(np.uint8)
    st, k, n, chan, out = _call(ana, syn, gpu, rawd, 16, 16, 1.0)
    assert (st, k, n) == (OK, 50, 0)
    assert np.array_equal(chan.written(ref.size), ref)
    out.written(0, "no block")
    st, k, n, _, _ = _call(ana, syn, gpu, rawd, 16, 16, 1.0, n_dat=100)
    assert (st, k, n) == (OK, 0, 0)


# ------------------------------------------------------------------ 6. work partition
def test_many_series_one_workgroup_walks_all_steps(gpu, profiling):
    """launch_stream's sizing gives each series min(steps, max(1, 2 CU / n_pol)) workgroups
    (csrc/pfb_ana_stream.hpp, stream_grid; tests/test_gpu_partition.py RANGES["stream"]): with
    more series than CUs it is one, which walks all 17 steps of its series — the window slide
    converting the prefetched file values at a step of n_pol x 4 bytes, the product store at
    n_pol x 8 bytes between a series' samples."""
    import torch
    from ska_pst_dsp_model_amd import layout
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    S, rows = cu + 1, KEEP + 2 * OV + 5
    steps = -(-(-(-rows // 8)) // 2)
    assert steps == 17 and min(steps, max(1, 2 * cu // S)) == 1
    ana, syn = _plans(S)
    n_dat = _n_dat(3073, 256, "8/7", rows, 9)
    base = _file_samples(np.random.default_rng(3600), 16, n_dat * 3 * 2).reshape(n_dat, 3, 2)
    raw = np.ascontiguousarray(base[:, np.arange(S) % 3, :])          # series s = base series s mod 3
    rawd = torch.from_numpy(raw).to(gpu)
    x = layout.dada_unpack(rawd, 16, 2, 1, S)[:, :, 0].contiguous()
    chan_ref, out_ref = _pfb().roundtrip(ana, syn, x)
    chan, out = _pfb().roundtrip_dada(ana, syn, rawd, 16, 32)
    assert _paths(ana, syn) == FUSED
    assert "analysis_stream_rt_dada_kernel<" in _kernel_name(3)
    assert tuple(chan.shape) == (rows, 256, S, 2) and tuple(out.shape) == (out_ref.shape[1], 1, S, 2)
    assert float(chan_ref.abs().max()) > 0 and float(out_ref.abs().max()) > 0
    assert torch.equal(torch.view_as_complex(chan).permute(2, 0, 1), chan_ref)
    assert torch.equal(torch.view_as_complex(out)[:, 0, :].permute(1, 0), out_ref)
    # the series repeat with period 3
    assert torch.equal(chan[:, :, 3:], chan[:, :, :-3]) and torch.equal(out[:, :, 3:], out[:, :, :-3])


# ------------------------------------------------------------------ 7. oracle
def test_float_section_matches_the_oracle(gpu):
    """The unit-variance series of test_gpu_roundtrip.py's C2 oracle case (seed 0, at this
    file's length) as an NBIT 32 section, out_nbit 32, scale 1, against the float64 oracle
    with the criterion applied as there: the product on the rms scale, the output raw."""
    import torch
    taps = _taps(256, "8/7", 12)
    rng = np.random.default_rng(0)
    x = ((rng.standard_normal((1, 1, N_DAT)) + 1j * rng.standard_normal((1, 1, N_DAT))) / np.sqrt(2)).astype(np.complex64)
    rawd = torch.from_numpy(np.ascontiguousarray(x[0, 0]).view(np.float32)).to(gpu)
    ana, syn = _plans(1)
    chan, out = _pfb().roundtrip_dada(ana, syn, rawd, 32, 32)
    assert _paths(ana, syn) == FUSED
    ref_chan = orc.polyphase_analysis(x, taps, 256, "8/7")                     # (1, 256, K)
    got_chan = torch.view_as_complex(chan)[:, :, 0].cpu().numpy()              # (K, 256)
    assert_pfb_close(got_chan.T[None], ref_chan, what="file-to-file analysis")
    ref = orc.polyphase_synthesis(ref_chan, 1, NF, "8/7", {"apply_deripple": 1, "filter_coeff": taps}, 1, OV,
                                  orc.pfb_window("tukey", NF, OV))
    got = torch.view_as_complex(out)[:, 0, 0].cpu().numpy()
    assert got.size == 3 * KEEP * 224
    assert_pfb_close(got[None, None, :], ref, scale=1.0, what="file-to-file round trip (raw)")
