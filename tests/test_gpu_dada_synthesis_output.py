"""Synthesis writing its output straight into a DADA data section
(pfb_synthesis_execute_to_dada, pfb_inverse_filterbank_execute_to_dada and their _dada_to_dada
twins): the Nf = 256 wave kernel converts and stores the NBIT 8 / 16 / 32 samples itself
(synth_wave_dadaout_kernel) instead of the packed complex float32 series that pfb_dada_pack
would read back.

The contract is bit-identity with the pair: the corresponding cf32-output call, both
components times float32(scale), pfb_dada_pack with one channel.  Every comparison against
the pair is np.array_equal on bytes, under a scale at which the pair's own integer output
saturates at both ends and rounds in both directions (asserted, so no case passes vacuously).
Every output buffer is framed by a byte pattern that must survive.  The oracle cases bound each
quantised component by half a step plus the project's 1e-6 (conftest.assert_pfb_close's
allowance) of its own sample.  Three to seven blocks per case.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import PARITY_TOL, assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

PAT = 0xA5         # the frame's byte
FRAME = 512        # bytes of frame on each side of the output buffer (keeps its alignment)
SPARE_SAMPLES = 5  # capacity beyond the samples due, pattern-filled
NF, OV, KEEP = 256, 48, 160


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


@functools.lru_cache(maxsize=None)
def _taps(N, os_):
    taps = _pfb().design_PFB_FIR_filter(N, os_, 12)
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def _ramp_window(nf):
    """A temporal window that is 1 nowhere (so the kernel multiplies every row)."""
    w = 0.75 + 0.25 * np.cos(2 * np.pi * (np.arange(nf) + 0.5) / nf)
    assert not (w.astype(np.float32) == 1).any()
    w.setflags(write=False)
    return w


def _plan(N, os_, n_pol, nf=NF, ov=OV, spans=True, taper="tukey", spectral=None, deripple=False):
    pfb = _pfb()
    w = pfb.PFBWindow()
    tt = w.custom(_ramp_window(nf)) if taper == "custom" else w.lookup[taper](nf, ov)
    return pfb.SynthesisPlan(N, os_, nf, ov, spans, 1, deripple, _taps(N, os_) if deripple else None, tt,
                             w.lookup[spectral](nf, ov) if spectral else None, n_pol)


def _rows(blocks, extra=0):
    return blocks * KEEP + 2 * OV + extra


def _section(gpu, seed, nbit, n_dat, N, n_pol):
    """A channelised DADA section (TFP or LowCBF bytes alike) over the integer type's full range."""
    import torch
    info = np.iinfo(orc._NBIT_NP[nbit])
    raw = np.random.default_rng(seed).integers(info.min, info.max + 1, size=n_dat * N * n_pol * 2)
    raw = raw.astype(orc._NBIT_NP[nbit])
    return raw, torch.from_numpy(raw.view(np.uint8)).to(gpu)


def _unpacked(rawd, nbit, N, n_pol, lowcbf=False):
    from ska_pst_dsp_model_amd import layout
    return layout.dada_unpack(rawd, nbit, 2, N, n_pol, lowcbf=lowcbf)          # (n_pol, rows, N)


def _pack_pair(out, nbit, scale):
    """The pair's second half: both components times float32(scale), then pfb_dada_pack with one
    channel.  `out`: the (n_pol, n_out) complex64 device series -> the section's bytes (numpy)."""
    import torch
    from ska_pst_dsp_model_amd import layout
    scaled = torch.view_as_complex((torch.view_as_real(out.contiguous()) * float(np.float32(scale))).contiguous())
    return layout.dada_pack(scaled[:, :, None], nbit).cpu().numpy().view(np.uint8)


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


def _sample_bytes(plan, out_nbit):
    return plan.n_pol * 2 * (out_nbit // 8)


def _call(plan, gpu, out_nbit, scale, x=None, rawd=None, in_nbit=None, lowcbf=False, stateful=False,
          sample_offset=1, cap_bytes=None, offset=0, null_out=False):
    """One raw C-ABI to-DADA call into a framed buffer: cf32 rows `x` (n_pol, n, N) or a DADA
    section `rawd` of in_nbit.  The capacity defaults to the samples due plus SPARE_SAMPLES.
    -> (status, n_out, host bytes of the whole framed buffer, offset of `out` in it)"""
    import torch
    from ska_pst_dsp_model_amd import _lib
    lib = plan._lib
    N = plan.n_chan
    if x is not None:
        n = int(x.shape[1])
    else:
        n = rawd.numel() // (N * plan.n_pol * 2 * (in_nbit // 8))
    # (an upper bound of the samples due, as SynthesisPlan.execute sizes its buffer)
    due = plan.output_length(plan.buffered_samples + n) if stateful else plan.output_length(max(n - sample_offset + 1, 0))
    sb = _sample_bytes(plan, out_nbit) if out_nbit in (8, 16, 32, 64) else plan.n_pol * 2
    cap = (due + SPARE_SAMPLES) * sb if cap_bytes is None else cap_bytes
    holder = torch.full((FRAME + offset + cap + FRAME,), PAT, dtype=torch.uint8, device=gpu)
    assert holder.data_ptr() % 16 == 0
    out = ctypes.c_void_p(0 if null_out else holder.data_ptr() + FRAME + offset)
    n_out = ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    if x is not None:
        src = ctypes.c_void_p(x.data_ptr())
        if stateful:
            st = lib.pfb_inverse_filterbank_execute_to_dada(plan._h, src, n * N, n, out, out_nbit, scale, cap,
                                                            ctypes.byref(n_out), stream)
        else:
            st = lib.pfb_synthesis_execute_to_dada(plan._h, src, n * N, n, sample_offset, out, out_nbit, scale, cap,
                                                   ctypes.byref(n_out), stream)
    else:
        src = ctypes.c_void_p(rawd.data_ptr())
        order = _lib.PFB_DADA_LOWCBF if lowcbf else _lib.PFB_DADA_TFP
        if stateful:
            st = lib.pfb_inverse_filterbank_execute_dada_to_dada(plan._h, src, in_nbit, 2, order, n, out, out_nbit,
                                                                 scale, cap, ctypes.byref(n_out), stream)
        else:
            st = lib.pfb_synthesis_execute_dada_to_dada(plan._h, src, in_nbit, 2, order, n, sample_offset, out,
                                                        out_nbit, scale, cap, ctypes.byref(n_out), stream)
    torch.cuda.synchronize(gpu)
    return st, n_out.value, holder.cpu().numpy(), FRAME + offset


def _written(h, off, nbytes, what=""):
    """The first nbytes of `out`; everything else of the framed buffer must be the pattern."""
    assert (h[:off] == PAT).all(), f"{what}: bytes before the section were written"
    assert (h[off + nbytes:] == PAT).all(), f"{what}: bytes beyond sample n_out were written"
    return h[off:off + nbytes]


def _scale_for(ref, nbit):
    """A float32 scale, not a power of two, that puts the rms of the series' finite components at
    0.4 of the integer range: a few per cent of them saturate."""
    comp = ref.view(np.float32).ravel().astype(np.float64)
    comp = comp[np.isfinite(comp)]
    rms = float(np.sqrt(np.mean(comp ** 2)))
    full = 1.11 if nbit in (32, 64) else float(np.iinfo(orc._NBIT_NP[nbit]).max)
    scale = np.float32(0.4 * full / rms)
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
    fin = np.isfinite(v)
    hi, lo = fin & (v > info.max + 1), fin & (v < info.min - 1)
    assert hi.any() and (q[hi] == info.max).all() and lo.any() and (q[lo] == info.min).all()
    inside = fin & (np.abs(v) < info.max)
    frac = np.abs(v) - np.floor(np.abs(v))
    up, down = inside & (frac > 0.5), inside & (frac < 0.5) & (frac > 0)
    assert up.any() and (np.abs(q[up]) == np.floor(np.abs(v[up])) + 1).all()
    assert down.any() and (np.abs(q[down]) == np.floor(np.abs(v[down]))).all()


# ------------------------------------------------------------------ 1. fused == the pair, framed
# the 8 (RW, SPANS, WFLAT) forms of the kernel; with NBIT 8 / 16 / 32: all 24 instantiations
FORMS = [(os_, spans, taper) for os_ in ("8/7", "4/3") for spans in (True, False) for taper in ("tukey", "custom")]


@pytest.mark.parametrize("n_pol", [1, 2], ids=["1pol", "2pol"])
@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["nbit8", "nbit16", "nbit32"])
@pytest.mark.parametrize("form", range(len(FORMS)), ids=lambda i: "%s-%s-%s" % (
    FORMS[i][0].replace("/", "over"), "spans" if FORMS[i][1] else "critical", FORMS[i][2]))
def test_fused_matches_the_pair(gpu, profiling, form, nbit, n_pol):
    os_, spans, taper = FORMS[form]
    # one phase group or seven (a non-power-of-two count: 112 is the smallest channel count
    # with one that the channel IFFT has a kernel for); 3, 4 or 5 blocks; an odd first row
    N = (16, 112)[(form + n_pol + nbit // 8) % 2]
    blocks = 3 + (form + nbit // 8) % 3
    so = 1 + (form % 2) * 2
    n = _rows(blocks, 7) + so - 1
    _, rawd = _section(gpu, 2000 + 31 * form + nbit + n_pol, 16, n, N, n_pol)
    x = _unpacked(rawd, 16, N, n_pol)
    plan = _plan(N, os_, n_pol, spans=spans, taper=taper)
    ref = plan.execute(x, sample_offset=so, layout="ptc")
    cf32_kernel = _kernel_name(2)
    assert "synth_wave_kernel<" in cf32_kernel
    assert plan.last_dada_output() == "none"
    n_ref = blocks * plan.output_keep
    assert tuple(ref.shape) == (n_pol, n_ref)
    refh = ref.cpu().numpy()
    scale = _scale_for(refh, nbit)
    pair = _pack_pair(ref, nbit, scale)
    sb = _sample_bytes(plan, nbit)
    assert pair.size == n_ref * sb
    _assert_pair_is_demanding(refh, pair, nbit, scale)
    # the _dada twin is the same series (the input side's own contract), so one pair serves both
    assert np.array_equal(plan.execute_dada(rawd, 16, sample_offset=so).cpu().numpy(), refh)
    rw = {"8/7": 14, "4/3": 12}[os_]
    for label, kw in (("cf32", dict(x=x)), ("dada", dict(rawd=rawd, in_nbit=16))):
        profiling.pfb_profile_reset()
        st, n_out, h, off = _call(plan, gpu, nbit, scale, sample_offset=so, **kw)
        assert (st, n_out) == (0, n_ref), (label, st, n_out)
        assert plan.last_dada_output() == "fused"
        assert plan.last_dada_input() == ("fused" if label == "dada" else "none")
        kernel = _kernel_name(2)
        print(f"{label}: class 2 {kernel!r}")
        # the block launch is the DADA-store kernel (so no cf32 series exists for a pack launch
        # to read), one launch for the call's one chunk
        assert kernel.replace("void ", "", 1).replace("pfb::", "", 1).startswith("synth_wave_dadaout_kernel<")
        assert f"<{rw}, {'true' if spans else 'false'}, {'true' if taper == 'tukey' else 'false'}," in kernel
        assert f"OutDada{nbit}>" in kernel
        assert _launches(profiling, 2) == 1
        assert np.array_equal(_written(h, off, n_ref * sb, label), pair), label
    plan.execute(x, layout="ptc")
    assert plan.last_dada_output() == "none"


def test_fused_scale_one_python_surface(gpu):
    """scale = 1.0 through SynthesisPlan.execute_to_dada / execute_dada_to_dada."""
    N, n_pol = 16, 2
    _, rawd = _section(gpu, 2100, 16, _rows(3, 1), N, n_pol)
    x = _unpacked(rawd, 16, N, n_pol)
    plan = _plan(N, "8/7", n_pol, deripple=True)
    ref = plan.execute(x, layout="ptc")
    for nbit, dtype in ((8, "torch.int8"), (16, "torch.int16"), (32, "torch.float32"), (64, "torch.float64")):
        pair = _pack_pair(ref, nbit, 1.0)
        got = plan.execute_to_dada(x, nbit, layout="ptc")
        assert plan.last_dada_output() == ("fused" if nbit != 64 else "staged")
        assert tuple(got.shape) == (ref.shape[1], 1, n_pol, 2) and str(got.dtype) == dtype
        assert np.array_equal(got.cpu().numpy().view(np.uint8).ravel(), pair), nbit
        got = plan.execute_dada_to_dada(rawd, 16, nbit)
        assert plan.last_dada_input() == "fused"
        assert np.array_equal(got.cpu().numpy().view(np.uint8).ravel(), pair), nbit
    # Matlab-shaped (n_pol, n_chan, n_dat) input, the default layout
    got = plan.execute_to_dada(x.transpose(1, 2), 16)
    assert np.array_equal(got.cpu().numpy().view(np.uint8).ravel(), _pack_pair(ref, 16, 1.0))


@pytest.mark.parametrize("nbit", [8, 16], ids=["nbit8", "nbit16"])
def test_nan_in_the_input_becomes_zero_bytes(gpu, nbit):
    """A NaN in one cf32 row spreads over its block of one polarisation: those samples are 0 in
    the section, as pfb_dada_pack writes them; every other block is converted as ever."""
    import torch
    N, n_pol, blocks = 16, 2, 4
    _, rawd = _section(gpu, 2200 + nbit, 16, _rows(blocks), N, n_pol)
    x = _unpacked(rawd, 16, N, n_pol).contiguous()
    x[1, OV + KEEP + 80, 3] = complex(float("nan"), 1.0)          # the middle of block 1 only
    plan = _plan(N, "8/7", n_pol)
    ref = plan.execute(x, layout="ptc")
    refh = ref.cpu().numpy()
    L = plan.output_keep
    bad = np.isnan(refh.view(np.float32).reshape(n_pol, -1, 2)).any(axis=2)
    assert bad[1, L:2 * L].all() and not bad[0].any() and not bad[1, :L].any() and not bad[1, 2 * L:].any()
    scale = _scale_for(refh, nbit)
    pair = _pack_pair(ref, nbit, scale)
    q = pair.view(orc._NBIT_NP[nbit]).reshape(-1, n_pol, 2)
    assert (q[L:2 * L, 1] == 0).all() and (q[:, 0] != 0).any() and (q[2 * L:, 1] != 0).any()
    st, n_out, h, off = _call(plan, gpu, nbit, scale, x=x)
    assert (st, n_out) == (0, blocks * L) and plan.last_dada_output() == "fused"
    assert np.array_equal(_written(h, off, pair.size), pair)
    assert torch.isnan(torch.view_as_real(x)).sum().item() == 1


# ------------------------------------------------------------------ 2. block ranges and chunks
def test_ranges_of_three_and_more_blocks(gpu, profiling):
    """n_chan 256 (16 phase groups) with enough polarisations that the launcher gives each
    workgroup a range of 3 or 4 blocks: the loop-carried register rows and the per-block
    descriptors over a range, two ranges per series."""
    import torch
    N, n_pol, blocks, nbit = 256, 24, 7, 8
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    # csrc/pfb_synth_wave_dadaout.hip, launch_dadaout (= launch_wave_t): max(1, 3 CU / (N/16 n_pol)),
    # capped at n_blocks
    ranges = min(blocks, max(1, 3 * cu // (N // 16 * n_pol)))
    sizes = [blocks * (w + 1) // ranges - blocks * w // ranges for w in range(ranges)]
    print(f"{cu} CUs: {blocks} blocks over {ranges} ranges -> {sizes}")
    assert max(sizes) >= 3, f"ranges {sizes}: no workgroup holds three blocks — pick another n_pol"
    _, rawd = _section(gpu, 2300, 8, _rows(blocks, 3), N, n_pol)
    plan = _plan(N, "8/7", n_pol, deripple=True)
    ref = plan.execute_dada(rawd, 8)
    refh = ref.cpu().numpy()
    scale = _scale_for(refh, nbit)
    pair = _pack_pair(ref, nbit, scale)
    _assert_pair_is_demanding(refh, pair, nbit, scale)
    st, n_out, h, off = _call(plan, gpu, nbit, scale, rawd=rawd, in_nbit=8)
    assert (st, n_out) == (0, blocks * plan.output_keep)
    assert plan.last_dada_output() == "fused" and plan.last_dada_input() == "fused"
    assert "synth_wave_dadaout_kernel<" in _kernel_name(2)
    assert np.array_equal(_written(h, off, pair.size), pair)


@pytest.mark.parametrize("out_nbit", [16, 64], ids=["fused16", "staged64"])
def test_chunked_synthesis_fills_one_section(gpu, profiling, out_nbit):
    """pfb_synthesis_set_chunk_blocks(2) over 7 blocks: four block launches into one section."""
    N, n_pol, blocks = 16, 2, 7
    _, rawd = _section(gpu, 2400, 16, _rows(blocks, 9), N, n_pol)
    x = _unpacked(rawd, 16, N, n_pol)
    plan = _plan(N, "4/3", n_pol)
    ref = plan.execute(x, layout="ptc")
    scale = _scale_for(ref.cpu().numpy(), out_nbit)
    pair = _pack_pair(ref, out_nbit, scale)
    plan.set_chunk_blocks(2)
    profiling.pfb_profile_reset()
    st, n_out, h, off = _call(plan, gpu, out_nbit, scale, x=x)
    assert (st, n_out) == (0, blocks * plan.output_keep)
    assert _launches(profiling, 2) == 4
    assert plan.last_dada_output() == ("fused" if out_nbit == 16 else "staged")
    assert ("synth_wave_dadaout_kernel<" in _kernel_name(2)) == (out_nbit == 16)
    assert np.array_equal(_written(h, off, pair.size), pair)


# ------------------------------------------------------------------ 3. staged
# (id, N, os, Nf, Ov, spectral, out_nbit, byte offset of `out`, rows)
STAGED_CASES = [
    ("nf512", 32, "8/7", 512, 128, None, 16, 0, 3 * 256 + 256 + 3),
    ("spectral-taper", 8, "4/3", 128, 16, "hann", 16, 0, 3 * 96 + 32 + 5),
    ("block-kernel-nf128", 8, "8/7", 128, 16, None, 8, 0, 3 * 96 + 32 + 5),
    ("nbit64", 16, "8/7", NF, OV, None, 64, 0, _rows(3, 2)),
    ("out-offset-one-value", 16, "8/7", NF, OV, None, 16, 2, _rows(3, 2)),
]


@pytest.mark.parametrize("case", STAGED_CASES, ids=lambda c: c[0])
def test_staged_matches_the_pair(gpu, profiling, case):
    name, N, os_, nf, ov, spectral, out_nbit, offset, n = case
    n_pol = 2
    _, rawd = _section(gpu, 2500 + len(name), 16, n, N, n_pol)
    x = _unpacked(rawd, 16, N, n_pol)
    plan, twin = (_plan(N, os_, n_pol, nf=nf, ov=ov, spectral=spectral) for _ in range(2))
    ref = twin.execute(x, sample_offset=2, layout="ptc")
    assert ref.shape[1] == 3 * plan.output_keep and float(ref.abs().max()) > 0
    refh = ref.cpu().numpy()
    scale = _scale_for(refh, out_nbit)
    pair = _pack_pair(ref, out_nbit, scale)
    _assert_pair_is_demanding(refh, pair, out_nbit, scale)
    for kw in (dict(x=x), dict(rawd=rawd, in_nbit=16)):
        st, n_out, h, off = _call(plan, gpu, out_nbit, scale, sample_offset=2, offset=offset, **kw)
        assert (st, n_out) == (0, ref.shape[1])
        assert plan.last_dada_output() == "staged"
        assert "dadaout" not in _kernel_name(2)
        assert np.array_equal(_written(h, off, pair.size, name), pair)
    # stream calls on the same plan
    for i, m in enumerate((n, 8 * 37)):
        _, rd = _section(gpu, 2550 + i, 16, m, N, n_pol)
        xs = _unpacked(rd, 16, N, n_pol)
        ref_s = twin.execute(xs, stateful=True, layout="ptc")
        st, n_out, h, off = _call(plan, gpu, out_nbit, scale, x=xs, stateful=True, offset=offset)
        assert (st, n_out) == (0, int(ref_s.shape[1])), (i, st, n_out)
        assert plan.last_dada_output() == "staged"
        assert np.array_equal(_written(h, off, n_out * _sample_bytes(plan, out_nbit), name),
                              _pack_pair(ref_s, out_nbit, scale)), i
        assert plan.buffered_samples == twin.buffered_samples
    assert ref_s.shape[1] > 0


# ------------------------------------------------------------------ 4. stream sequences
STREAM_OFFSET = 5


def _sequence(gpu, nbit, sizes, modes, lowcbf=False, os_="8/7"):
    """`sizes` rows call by call through one plan in `modes` ("to_dada": cf32 in, DADA out;
    "dada_to_dada"; "cf32": pfb_inverse_filterbank_execute; "dada_in": ..._execute_dada) against
    the cf32 stream of a twin packed call by call."""
    N, n_pol = 16, 2
    plan, twin = _plan(N, os_, n_pol), _plan(N, os_, n_pol)
    for p in (plan, twin):
        p.set_stream_sample_offset(STREAM_OFFSET)
    seen = dict(empty=False, blocks=False, trimmed=False)
    got_all, ref_all = [], []
    for i, (n, mode) in enumerate(zip(sizes, modes)):
        _, rawd = _section(gpu, 2600 + i, 16, n, N, n_pol)
        x = _unpacked(rawd, 16, N, n_pol, lowcbf=lowcbf)
        ref = twin.execute(x, stateful=True, layout="ptc")
        n_ref = int(ref.shape[1])
        seen["empty"] |= n_ref == 0
        seen["blocks"] |= n_ref >= 2 * plan.output_keep
        seen["trimmed"] |= n_ref % plan.output_keep != 0
        scale = 0.0123 if nbit != 32 else 0.37
        ref_b = _pack_pair(ref, nbit, scale)
        if mode == "cf32":
            got_b = _pack_pair(plan.execute(x, stateful=True, layout="ptc"), nbit, scale)
            assert plan.last_dada_output() == "none"
        elif mode == "dada_in":
            got_b = _pack_pair(plan.execute_dada(rawd, 16, lowcbf=lowcbf, stateful=True), nbit, scale)
            assert plan.last_dada_output() == "none"
        else:
            kw = dict(x=x) if mode == "to_dada" else dict(rawd=rawd, in_nbit=16, lowcbf=lowcbf)
            st, n_out, h, off = _call(plan, gpu, nbit, scale, stateful=True, **kw)
            assert (st, n_out) == (0, n_ref), (i, mode, st, n_out)
            got_b = _written(h, off, n_ref * _sample_bytes(plan, nbit), f"call {i}")
            assert plan.last_dada_output() == "fused"
        assert np.array_equal(got_b, ref_b), (i, mode)
        assert plan.buffered_samples == twin.buffered_samples, (i, mode)
        got_all.append(got_b)
        ref_all.append(ref_b)
    assert np.array_equal(np.concatenate(got_all), np.concatenate(ref_all))
    return seen


# first call: no block; then uneven lengths, some no multiple of nu (the output is trimmed)
SIZES = (104, 700, 333, 1001, 250)


@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["nbit8", "nbit16", "nbit32"])
@pytest.mark.parametrize("mode", ["to_dada", "dada_to_dada"])
def test_stream_sequence_to_dada(gpu, mode, nbit):
    seen = _sequence(gpu, nbit, SIZES, (mode,) * len(SIZES), os_="8/7" if nbit != 16 else "4/3")
    assert seen == dict(empty=True, blocks=True, trimmed=True), seen


def test_stream_sequence_alternating_outputs_and_inputs(gpu):
    modes = ("to_dada", "cf32", "dada_to_dada", "dada_in", "to_dada")
    seen = _sequence(gpu, 16, SIZES, modes)
    assert seen["empty"] and seen["blocks"]


def test_stream_sequence_lowcbf_heaps(gpu):
    seen = _sequence(gpu, 16, (96, 704, 320, 1024), ("dada_to_dada", "dada_to_dada", "cf32", "dada_to_dada"),
                     lowcbf=True)
    assert seen["empty"] and seen["blocks"]


# ------------------------------------------------------------------ 5. rejections
@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "stream"])
def test_rejections_leave_output_and_state_alone(gpu, stateful):
    from ska_pst_dsp_model_amd import _lib
    N, n_pol, nbit = 16, 2, 16
    plan, twin = _plan(N, "8/7", n_pol), _plan(N, "8/7", n_pol)
    if stateful:
        _, r0 = _section(gpu, 2700, 16, 400, N, n_pol)
        for p in (plan, twin):
            p.execute(_unpacked(r0, 16, N, n_pol), stateful=True, layout="ptc")
        assert plan.buffered_samples > 0
    buffered = plan.buffered_samples
    n = _rows(3, 24)
    _, rawd = _section(gpu, 2701, 16, n, N, n_pol)
    x = _unpacked(rawd, 16, N, n_pol)
    ref = twin.execute(x, stateful=stateful, layout="ptc")
    due = int(ref.shape[1])
    assert due >= 3 * plan.output_keep
    need = due * _sample_bytes(plan, nbit)
    E, S = _lib.PFB_ERR_INVALID_ARG, _lib.PFB_ERR_BUFFER_TOO_SMALL
    for kw in (dict(x=x), dict(rawd=rawd, in_nbit=16)):
        st, n_out, h, off = _call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need - 1, **kw)
        assert (st, n_out) == (S, due)
        assert (h == PAT).all(), "a call with too small a capacity wrote output"
        for bad in (dict(out_nbit=12), dict(scale=float("nan")), dict(scale=float("inf")), dict(null_out=True)):
            args = dict(out_nbit=nbit, scale=0.01, stateful=stateful, cap_bytes=need)
            args.update(bad)
            args.update(kw)
            st, n_out, h, off = _call(plan, gpu, args.pop("out_nbit"), args.pop("scale"), **args)
            assert st == E, bad
            assert (h == PAT).all(), bad
        # an `out` not aligned to one value
        st, n_out, h, off = _call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need, offset=1, **kw)
        assert st == E and (h == PAT).all()
        assert plan.buffered_samples == buffered
    # the corrected retry: what the twin, which saw no rejected call, returned
    st, n_out, h, off = _call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need, x=x)
    assert (st, n_out) == (0, due) and plan.last_dada_output() == "fused"
    assert np.array_equal(_written(h, off, need), _pack_pair(ref, nbit, 0.01))
    assert plan.buffered_samples == twin.buffered_samples


# ------------------------------------------------------------------ 6. oracle
@functools.lru_cache(maxsize=None)
def _oracle():
    """(raw section NBIT 16, float64 oracle series (n_pol, 1, n_out)) at n_chan 16, 3 blocks."""
    N, n_pol = 16, 2
    info = np.iinfo(np.int16)
    raw = np.random.default_rng(2800).integers(info.min, info.max + 1, size=_rows(3, 4) * N * n_pol * 2).astype(np.int16)
    x = orc.reshape_dada_data(raw, 2, n_pol, N).astype(np.complex64)           # (n_pol, n_chan, n_dat)
    y = orc.polyphase_synthesis(x, 1, NF, "8/7", {"apply_deripple": 1, "filter_coeff": _taps(N, "8/7")}, 1, OV,
                                orc.pfb_window("tukey", NF, OV))
    y = np.asarray(y, dtype=np.complex128)
    y.setflags(write=False)
    raw.setflags(write=False)
    return raw, y


@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["nbit8", "nbit16", "nbit32"])
def test_fused_matches_oracle(gpu, nbit):
    import torch
    N, n_pol = 16, 2
    raw, y = _oracle()
    rawd = torch.from_numpy(raw.view(np.uint8).copy()).to(gpu)
    plan = _plan(N, "8/7", n_pol, deripple=True)
    n_out = 3 * plan.output_keep
    assert y.shape == (n_pol, 1, n_out)
    rms = float(np.sqrt(np.mean(np.abs(y) ** 2)))
    # rms of the magnitudes near a third of the range, and not a power of two
    scale = float(np.float32((np.iinfo(orc._NBIT_NP[nbit]).max if nbit != 32 else 1.11) / 3.0 / rms))
    assert np.frexp(scale)[0] != 0.5
    got = plan.execute_dada_to_dada(rawd, 16, nbit, scale=scale)
    assert plan.last_dada_output() == "fused" and tuple(got.shape) == (n_out, 1, n_pol, 2)
    sy = np.float64(np.float32(scale)) * y[:, 0, :]                            # (n_pol, n_out)
    q = got.cpu().numpy().astype(np.float64)[:, 0]                             # (n_out, n_pol, 2)
    t = sy.T                                                                   # (n_out, n_pol)
    if nbit == 32:
        assert_pfb_close(q[..., 0] + 1j * q[..., 1], t, what="to-DADA synthesis")
        return
    info = np.iinfo(orc._NBIT_NP[nbit])
    delta = PARITY_TOL * (np.sqrt(np.mean(np.abs(sy) ** 2)) + np.abs(t))       # assert_pfb_close's allowance
    worst = 0.0
    for comp, part in ((0, t.real), (1, t.imag)):
        err = np.abs(q[..., comp] - np.clip(part, info.min, info.max))
        worst = max(worst, float((err - delta).max()))
        assert (err <= 0.5 + delta).all(), (nbit, comp, float((err - delta).max()))
    print(f"nbit {nbit}: max (|q - clip(scale y)| - delta) = {worst:.6f} (bound 0.5)")


# ------------------------------------------------------------------ 7. layouts and files
def test_section_feeds_the_analysis(gpu):
    """The synthesised NBIT 16 two-polarisation section read by AnalysisPlan.execute_dada equals
    the analysis of the unpacked section: both sides mean the same layout."""
    from ska_pst_dsp_model_amd import layout
    pfb = _pfb()
    N, n_pol = 16, 2
    _, rawd = _section(gpu, 2900, 16, _rows(3, 2), N, n_pol)
    plan = _plan(N, "8/7", n_pol)
    ref = plan.execute_dada(rawd, 16)
    sec = plan.execute_dada_to_dada(rawd, 16, 16, scale=_scale_for(ref.cpu().numpy(), 16) / 2)
    assert plan.last_dada_output() == "fused" and tuple(sec.shape) == (3 * plan.output_keep, 1, n_pol, 2)
    series = layout.dada_unpack(sec, 16, 2, 1, n_pol)[:, :, 0].contiguous()    # (n_pol, n_out)
    # the unpacked section is the quantised series, polarisation by polarisation
    assert np.array_equal(series.cpu().numpy().view(np.float32).reshape(n_pol, -1, 2),
                          sec.cpu().numpy()[:, 0].transpose(1, 0, 2).astype(np.float32))
    assert float(series[0].abs().max()) > 0 and not np.array_equal(series[0].cpu().numpy(), series[1].cpu().numpy())
    ana = pfb.AnalysisPlan(_taps(16, "8/7"), 16, "8/7", "polyphase_analysis", n_pol)
    want = ana.execute(series).cpu().numpy()
    got = ana.execute_dada(sec, 16).cpu().numpy()
    assert want.shape[1] > 100 and np.abs(want).max() > 0
    assert np.array_equal(got, want)


def test_inverse_filterbank_object_to_dada(gpu):
    """InverseFilterBank.execute_to_dada / execute_dada_to_dada over three calls == execute +
    layout.dada_pack, with the same carry."""
    pfb = _pfb()
    N, n_pol = 16, 2
    cfg = dict(channels=N, os_factor="8/7", input_fft_length=NF, input_overlap=OV, deripple=False,
               temporal_taper="tukey", filt_coeff=_taps(N, "8/7"))
    a, b = pfb.InverseFilterBank(cfg), pfb.InverseFilterBank(cfg)
    a.sample_offset = b.sample_offset = 3
    for i, n in enumerate((600, 104, 777)):
        _, rawd = _section(gpu, 3000 + i, 16, n, N, n_pol)
        x = _unpacked(rawd, 16, N, n_pol).transpose(1, 2)                      # (n_pol, n_chan, n_dat)
        _, ref = b.execute(x)
        if i % 2 == 0:
            _, sec = a.execute_to_dada(x, 8, scale=0.0123)
        else:
            _, sec = a.execute_dada_to_dada(rawd, 16, 8, scale=0.0123, n_pol=n_pol)
        assert tuple(sec.shape) == (ref.shape[2], 1, n_pol, 2) and str(sec.dtype) == "torch.int8"
        assert np.array_equal(sec.cpu().numpy().view(np.uint8).ravel(), _pack_pair(ref[:, 0, :], 8, 0.0123)), i
        assert a.buffered_samples == b.buffered_samples
        assert a._plan.last_dada_output() == "fused"
    assert ref.shape[2] > 0
    # FilterBank's output-quantiser hooks set on the object: execute + pack
    a.rmsOutput = 1.0
    _, rawd = _section(gpu, 3010, 16, 640, N, n_pol)
    x = _unpacked(rawd, 16, N, n_pol).transpose(1, 2)
    _, sec = a.execute_to_dada(x, 16, scale=0.5)
    _, ref = b.execute(x)
    assert a._plan.last_dada_output() == "none"
    assert np.array_equal(sec.cpu().numpy().view(np.uint8).ravel(), _pack_pair(ref[:, 0, :], 16, 0.5))


def test_harness_synthesize_writes_the_section_itself(gpu, tmp_path):
    """harness.synthesize of a two-pol NBIT-16 channelised file == write_dada_file of
    execute_dada's series, byte for byte."""
    pfb = _pfb()
    N, n_pol, os_ = 16, 2, "8/7"
    rng = np.random.default_rng(3100)
    n = _rows(3, 5)
    chan = 3000.0 * (rng.standard_normal((n_pol, N, n)) + 1j * rng.standard_normal((n_pol, N, n)))
    hdr = {"HDR_SIZE": "16384", "TSAMP": "1.0", "OS_FACTOR": os_}
    pfb.dada.add_fir_filter_to_header(hdr, _taps(N, os_), pfb.config.as_rational(os_))
    src = tmp_path / "chan16.dump"
    pfb.dada.write_dada_file(src, chan.astype(np.complex64), hdr, nbit=16)
    f = pfb.harness.synthesize(str(src), NF, OV, "tukey", output_file_name="synth.dump", output_dir=str(tmp_path))
    raw, rhdr = pfb.dada.read_dada_raw(src)
    taps = np.array([float(v) for v in rhdr["COEFF_0"].split(",")])
    plan = pfb.SynthesisPlan(N, os_, NF, OV, True, 1, True, taps, pfb.PFBWindow().lookup["tukey"](NF, OV), None, n_pol)
    ref = plan.execute_dada(raw, 16)
    assert tuple(ref.shape) == (n_pol, 3 * plan.output_keep) and float(ref.abs().max()) > 0
    with open(f.file_path, "rb") as fh:
        got_hdr = pfb.dada.read_header(fh)
    sh = dict(rhdr)
    sh["TSAMP"] = got_hdr["TSAMP"]
    expect = tmp_path / "expect.dump"
    pfb.dada.write_dada_file(expect, ref[:, None, :], sh)
    with open(f.file_path, "rb") as a, open(expect, "rb") as b:
        assert a.read() == b.read()
