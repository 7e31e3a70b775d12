"""The Python plan layer's own behaviour (core.py): which argument errors it raises itself
and which it leaves to the C ABI, what an ``out=`` buffer must be for each synthesis entry,
what a failed constructor and ``close`` leave behind, and the row counts of the stateful
analysis entries.  Kernel results are only compared with themselves, bit for bit.

Everything runs on the smallest configuration the engine has: 8 channels, 8/7, 81 taps
(step 7 samples, 11 phases), a synthesis of Nf 128 and overlap 16 (96 rows in, 672 samples
out per block), inputs of two to three blocks.
"""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, OS, NF, OV = 8, "8/7", 128, 16
# synthesis chunks: 2 blocks with 248 - 192 = 56 rows carried, then (56 + 320 - 32) // 96 = 3
# blocks with 88 carried.  Both carries are multiples of nu = 8 already, so the stream object
# does not round them up (InverseFilterBank.m:104-135) and whole blocks come out.
ROWS_A, ROWS_B = 248, 320
BLOCK_OUT = 672
SENTINEL = complex(7.0, -7.0)


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _lib():
    from ska_pst_dsp_model_amd import _lib
    return _lib


def _syn(n_pol, combine=1):
    return _pfb().SynthesisPlan(N, OS, NF, OV, True, combine, False, None, None, None, n_pol)


def _ana(n_pol, variant="polyphase_analysis"):
    pfb = _pfb()
    return pfb.AnalysisPlan(pfb.design_PFB_FIR_filter(N, OS, 10), N, OS, variant, n_pol)


def _rows(gpu, n_pol, seed=5):
    """(section, rows): ROWS_A + ROWS_B rows of an NBIT-16 DADA section [t][chan][pol][re, im]
    as an int16 device tensor, and the same samples as complex64 (n_pol, rows, N)."""
    import torch
    from ska_pst_dsp_model_amd import layout
    rng = np.random.default_rng(seed + n_pol)
    raw = rng.integers(-3000, 3001, size=(ROWS_A + ROWS_B, N, n_pol, 2)).astype(np.int16)
    sec = torch.from_numpy(raw).to(gpu)
    return sec, layout.dada_unpack(sec, 16, 2, N, n_pol)


def _series(gpu, n_pol, n_dat, seed=9):
    """(section, series): an NBIT-16 single-channel section [t][pol][re, im] and its samples
    as complex64 (n_pol, n_dat)."""
    import torch
    rng = np.random.default_rng(seed + n_pol)
    raw = rng.integers(-3000, 3001, size=(n_dat, n_pol, 2)).astype(np.int16)
    x = (raw[..., 0] + 1j * raw[..., 1]).astype(np.complex64).T
    return torch.from_numpy(raw).to(gpu), torch.from_numpy(np.ascontiguousarray(x)).to(gpu)


def _bits(t):
    import torch
    return torch.view_as_real(t).contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. out= of the synthesis
def _call(entry, plan, sec, rows, a, b, stateful, out):
    if entry == "execute":
        return plan.execute(rows[:, a:b].contiguous(), stateful=stateful, layout="ptc", out=out)
    if entry == "execute_view":
        return plan.execute_view(rows[:, a:b], stateful=stateful, out=out)
    return plan.execute_dada(sec[a:b], 16, stateful=stateful, out=out)


ENTRIES = ["execute", "execute_view", "execute_dada"]


@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "stateful"])
@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("entry", ENTRIES)
def test_out_width(gpu, entry, n_pol, stateful):
    """An ``out`` one sample narrower than the length due is refused — by Python
    (ValueError) in ``execute``, by the C ABI (PFB_ERR_BUFFER_TOO_SMALL) in ``execute_view``
    and ``execute_dada`` — and the stream state is untouched; a wider one receives the same
    samples as the allocating call, and the result is its leading slice."""
    import torch
    pfb = _pfb()
    sec, rows = _rows(gpu, n_pol)
    plan, twin = _syn(n_pol), _syn(n_pol)
    if stateful:
        for p in (plan, twin):
            assert _call(entry, p, sec, rows, 0, ROWS_A, True, None).shape == (n_pol, 2 * BLOCK_OUT)
    a, b = ROWS_A, ROWS_A + ROWS_B
    ref = _call(entry, twin, sec, rows, a, b, stateful, None)
    due = ref.shape[1]
    assert due == 3 * BLOCK_OUT
    carried = plan.buffered_samples
    assert (carried > 0) == stateful
    narrow = torch.full((n_pol, due - 1), SENTINEL, dtype=torch.complex64, device=gpu)
    if entry == "execute":
        with pytest.raises(ValueError):
            _call(entry, plan, sec, rows, a, b, stateful, narrow)
    else:
        with pytest.raises(pfb.PfbError) as e:
            _call(entry, plan, sec, rows, a, b, stateful, narrow)
        assert e.value.status == _lib().PFB_ERR_BUFFER_TOO_SMALL
    assert plan.buffered_samples == carried
    wide = torch.full((n_pol, due + 5), SENTINEL, dtype=torch.complex64, device=gpu)
    got = _call(entry, plan, sec, rows, a, b, stateful, wide)
    torch.cuda.synchronize()
    assert got.data_ptr() == wide.data_ptr() and got.shape == ref.shape
    assert torch.equal(_bits(got), _bits(ref))
    assert bool((narrow == SENTINEL).all()) and bool((wide[:, due:] == SENTINEL).all())
    assert plan.buffered_samples == twin.buffered_samples
    plan.close()
    twin.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_out_must_be_a_contiguous_complex64_buffer_of_the_plans_pols(gpu, entry):
    import torch
    sec, rows = _rows(gpu, 2)
    plan = _syn(2)
    w = 3 * BLOCK_OUT
    bad = {
        "dtype": torch.empty((2, w), dtype=torch.complex128, device=gpu),
        "non-contiguous": torch.empty((2, 2 * w), dtype=torch.complex64, device=gpu)[:, ::2],
        "n_pol": torch.empty((3, w), dtype=torch.complex64, device=gpu),
    }
    for what, out in bad.items():
        with pytest.raises(ValueError):
            _call(entry, plan, sec, rows, 0, ROWS_B, False, out)
            pytest.fail(f"{entry} accepted an out of the wrong {what}")
    plan.close()


# ------------------------------------------------------------------ 2. who rejects what
def test_host_arrays(gpu):
    """The DADA entries are device-only and answer a host array as the C ABI would
    (PFB_ERR_INVALID_ARG); the cf32 round trip raises ValueError."""
    pfb = _pfb()
    ana, syn = _ana(1), _syn(1)
    raw = np.zeros((400, 1, 2), dtype=np.int16)
    x = np.zeros((1, 400), dtype=np.complex64)
    rows_raw = np.zeros((ROWS_B, N, 1, 2), dtype=np.int16)
    rows = np.zeros((1, N, ROWS_B), dtype=np.complex64)
    calls = [
        lambda: ana.execute_dada(raw, 16),
        lambda: ana.execute_to_dada(x, 16),
        lambda: ana.execute_dada_to_dada(raw, 16, 16),
        lambda: syn.execute_dada(rows_raw, 16),
        lambda: syn.execute_to_dada(rows, 16),
        lambda: syn.execute_dada_to_dada(rows_raw, 16, 16),
        lambda: pfb.roundtrip_dada(ana, syn, raw, 16, 16),
        lambda: pfb.roundtrip_analysis_dada(ana, syn, raw, 16),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(pfb.PfbError) as e:
            call()
        assert e.value.status == _lib().PFB_ERR_INVALID_ARG, i
    with pytest.raises(ValueError):
        pfb.roundtrip(ana, syn, x)
    with pytest.raises(ValueError):
        pfb.roundtrip_analysis(ana, syn, x)
    ana.close()
    syn.close()


def test_format_the_c_abi_rejects(gpu):
    """NBIT 12 reaches the C ABI and comes back as PFB_ERR_INVALID_ARG: the Python layer's
    own length and allocation arithmetic does not trip over it first."""
    pfb = _pfb()
    ana, syn = _ana(1), _syn(1)
    raw, x = _series(gpu, 1, 400)
    sec, rows = _rows(gpu, 1)
    calls = [
        lambda: ana.execute_dada(raw, 12),
        lambda: ana.execute_dada(raw, 12, stateful=True),
        lambda: ana.execute_to_dada(x, 12),
        lambda: ana.execute_to_dada(x, 12, stateful=True),
        lambda: ana.execute_dada_to_dada(raw, 12, 16),
        lambda: ana.execute_dada_to_dada(raw, 16, 12),
        lambda: syn.execute_dada(sec, 12),
        lambda: syn.execute_dada(sec, 12, stateful=True),
        lambda: syn.execute_to_dada(rows, 12, layout="ptc"),
        lambda: syn.execute_to_dada(rows, 12, stateful=True, layout="ptc"),
        lambda: syn.execute_dada_to_dada(sec, 12, 16),
        lambda: syn.execute_dada_to_dada(sec, 16, 12),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(pfb.PfbError) as e:
            call()
        assert e.value.status == _lib().PFB_ERR_INVALID_ARG, i
    assert ana.buffered_samples == 0 and syn.buffered_samples == 0
    ana.close()
    syn.close()


def test_roundtrip_preconditions(gpu):
    """Raised by the Python layer before any launch: plans of different n_pol, and
    preallocated ``chan`` / ``out`` of another shape than the call's."""
    import torch
    pfb = _pfb()
    ana, syn, syn2 = _ana(1), _syn(1), _syn(2)
    n_dat = 11 * N + 7 * 320                # 320 rows -> 3 blocks
    raw, x = _series(gpu, 1, n_dat)
    for call in (lambda: pfb.roundtrip(ana, syn2, x),
                 lambda: pfb.roundtrip_analysis(ana, syn2, x),
                 lambda: pfb.roundtrip_dada(ana, syn2, raw, 16, 16),
                 lambda: pfb.roundtrip_analysis_dada(ana, syn2, raw, 16)):
        with pytest.raises(ValueError):
            call()
    assert ana.output_length(n_dat) == 320 and syn.output_length(320) == 3 * BLOCK_OUT

    def buf(*shape):
        return torch.empty(shape, dtype=torch.complex64, device=gpu)

    for kw in ({"chan": buf(1, 321, N)}, {"chan": buf(1, N, 320)}, {"out": buf(1, 3 * BLOCK_OUT + 1)},
               {"out": buf(2, 3 * BLOCK_OUT)}, {"chan": buf(1, 320, N), "out": buf(1, 3 * BLOCK_OUT - 1)}):
        with pytest.raises(ValueError):
            pfb.roundtrip(ana, syn, x, **kw)
    with pytest.raises(ValueError):
        pfb.roundtrip_analysis(ana, syn, x, chan=buf(1, 319, N))
    with pytest.raises(ValueError):
        pfb.roundtrip_synthesis(ana, syn, n_dat, out=buf(1, 3 * BLOCK_OUT + 1))
    for p in (ana, syn, syn2):
        p.close()


# ------------------------------------------------------------------ 3. lifetime
def test_failed_constructor_is_collected_silently(gpu, capfd):
    pfb = _pfb()
    try:
        _syn(1, combine=3)
        raised = None
    except pfb.PfbError as e:
        raised = e.status
    assert raised is not None and raised != _lib().PFB_OK
    gc.collect()
    assert "Exception ignored" not in capfd.readouterr().err


def test_close_twice(gpu):
    for plan in (_ana(1), _syn(1)):
        plan.close()
        plan.close()
        del plan
    gc.collect()


def test_close_is_refused_while_a_capture_holds_the_plan(gpu):
    """tests/test_gpu_roundtrip.py's pattern on one small synthesis plan: ``close`` raises
    while the capture that recorded the plan's launches is open, and works after it ended."""
    import torch
    _, rows = _rows(gpu, 1)
    chan = rows[:, :ROWS_B].contiguous()
    plan = _syn(1)
    ref = plan.execute(chan, layout="ptc").clone()
    out = torch.empty_like(ref)
    plan.execute(chan, layout="ptc", out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            plan.execute(chan, layout="ptc", out=out)
            with pytest.raises(RuntimeError):
                plan.close()
        finally:
            g.capture_end()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(ref))
    del g
    plan.close()
    plan.close()


# ------------------------------------------------------------------ 4. stateful analysis rows
# (variant, first chunk, rows of the two stateful calls): the second chunk is step - 1 = 6
# samples, and completes the sequence's 16th row.  Bunton: K(n) = (n - 88) // 7, so 194
# samples make 15 rows, of which a stream call returns 8 (a multiple of nu = 8) and carries
# 194 - 56 = 138 samples; with 6 more, (144 - 88) // 7 = 8 rows.  Padded: K(n) = n // 7, 106
# samples make 15 rows -> 8, carry 50; 56 // 7 = 8.
STREAMS = [("polyphase_analysis", 194), ("polyphase_analysis_padded", 106)]


@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("variant,first", STREAMS, ids=["bunton", "padded"])
def test_stateful_analysis_rows(gpu, variant, first, n_pol):
    """``execute(stateful=True)`` sizes its buffer by an upper bound of the rows,
    ``execute_to_dada(stateful=True)`` by the exact count: both return what the stateless
    call makes of the whole sequence."""
    _, x = _series(gpu, n_pol, first + 6)
    cf32, dada, whole = _ana(n_pol, variant), _ana(n_pol, variant), _ana(n_pol, variant)
    assert whole.execute(x).shape == (n_pol, 16, N)
    assert whole.execute_to_dada(x, 16).shape == (16, N, n_pol, 2)
    chunks = (x[:, :first].contiguous(), x[:, first:].contiguous())
    assert [tuple(cf32.execute(c, stateful=True).shape) for c in chunks] == [(n_pol, 8, N)] * 2
    assert [tuple(dada.execute_to_dada(c, 16, stateful=True).shape) for c in chunks] == [(8, N, n_pol, 2)] * 2
    assert cf32.buffered_samples == dada.buffered_samples == (first + 6) - 16 * 7
    for p in (cf32, dada, whole):
        p.close()
