"""The FilterBank's quantised input as a property of the analysis plan
(pfb_analysis_set_input_quantiser; FilterBank.m:75-83): the moments of a call's new samples in
one pass where they lie, the scale from a fixed-order sum, and the rounding at the analysis
kernel's load (FUSED) or in a quantising copy (STAGED).

The yardstick throughout is a twin plan with the quantiser off, fed
``q = layout.quantize(float32(s) * x, 0)`` with ``s`` the scale the call took — the project's own
operations; a multiply by 1.0f is exact, so this is roundf(sf * x).  The product must equal the
twin's on ``q`` bit for bit, and ``s`` the oracle's rms / sqrt(var(x, 0, "all")) within 1e-9 (the
bound of test_quantize_rms_scale: a reordered double sum at these sizes moves it by some 1e-10).
Every input carries the DC offset of ``_series``, (0.25 - 0.5j) of its rms, so the mean term of
the variance matters.  A few dozen output rows per case.
"""
import ctypes

import numpy as np
import pytest

import stream_harness as sh
from conftest import PARITY_TOL, assert_pfb_close
from oracle import pfb_oracle as orc
from test_gpu_dada_output import (BUNTON, C2, C2_P12, F43, N64, N512, PADDED, _fb_cfg, _kernel_name, _n_dat, _pfb,
                                  _plan, _taps, _unpacked, profiling)  # noqa: F401  (profiling: a fixture)
from test_gpu_quantised_output import CHUNKS, _bytes, _series

pytestmark = pytest.mark.gpu

RMS_IN = 20.0
SHAPES = {"c2-p12": C2_P12, "c2-p13": C2, "4over3": F43, "lowcbf": "lowcbf"}
# the file's samples: rms of the noise before the cast (NBIT 8 clips a few samples; they are the input)
AMP = {8: 30.0, 16: 2000.0, 32: 100.0}
INT = {8: "int8", 16: "int16"}


def _input(gpu, kind, n_pol, n, seed):
    """kind 'cf32' or an NBIT -> (what the call takes: the (n_pol, n) series or the TFP section's
    bytes; the same samples as the (n_pol, n) complex64 series, the section's exactly cast)."""
    import torch
    if kind == "cf32":
        x = _series(gpu, n_pol, n, seed)
        return x, x
    v = torch.view_as_real(_series(gpu, n_pol, n, seed, amp=AMP[kind]).T.contiguous())   # (n, n_pol, 2): TFP
    if kind == 32:
        raw = v.contiguous()
    else:
        info = np.iinfo(INT[kind])
        raw = v.round().clamp(info.min, info.max).to(getattr(torch, INT[kind])).contiguous()
    rawd = raw.view(torch.uint8).reshape(-1).contiguous()
    return rawd, _unpacked(rawd, kind, n_pol)


def _run(plan, inp, kind, stateful=False):
    if kind == "cf32":
        return plan.execute(inp, stateful=stateful)
    return plan.execute_dada(inp, kind, stateful=stateful)


def _rounded(x, s):
    """q: the project's own operations on the series x with the float32 of the scale s."""
    import torch
    from ska_pst_dsp_model_amd import layout
    if x.shape[1] == 0:
        return x
    scaled = torch.view_as_complex((torch.view_as_real(x.contiguous()) * float(np.float32(s))).contiguous())
    return layout.quantize(scaled, 0.0)


def _distinct(q):
    import torch
    return len(np.unique(torch.view_as_real(q).cpu().numpy()))


def _scale_ok(s, x, rms, what=""):
    ref = orc.quantize_scale(x.cpu().numpy(), rms)
    print(f"{what}: scale {s!r} reference {ref!r} relative difference {abs(s - ref) / ref:.3e}")
    assert abs(s - ref) <= 1e-9 * s, (what, s, ref)


def _qplan(kind, n_pol, rms=RMS_IN, mode=None):
    plan = _plan(kind, n_pol)
    plan.set_input_quantiser(rms)
    if mode:
        plan.set_input_quantiser_mode(mode)
    return plan


# ------------------------------------------------------------------ 1. bytes and scale
@pytest.mark.parametrize("kind", ["cf32", 8, 16, 32], ids=str)
@pytest.mark.parametrize("n_pol", [1, 2])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bytes_are_the_twins_and_the_scale_the_oracles(gpu, profiling, shape, n_pol, kind):
    pk = SHAPES[shape]
    # 37 rows: two full steps of 16 and a ragged one
    inp, x = _input(gpu, kind, n_pol, _n_dat(pk, 37, 11), 4000 + 7 * n_pol + (0 if kind == "cf32" else kind))
    plan, twin = _qplan(pk, n_pol), _plan(pk, n_pol)
    assert plan.last_input_quantiser() == "none"
    y = _run(plan, inp, kind)
    assert plan.last_input_quantiser() == "fused" and y.shape[1] == 37
    kernel = _kernel_name(0)
    assert "analysis_stream_qin_kernel<" in kernel, kernel
    assert ("InCf32" if kind == "cf32" else f"InDada{kind}") in kernel, kernel
    if kind != "cf32":
        assert plan.last_dada_input() == "fused"
    s = plan.last_input_scale()
    _scale_ok(s, x, RMS_IN, f"{shape} {n_pol} pol {kind}")
    q = _rounded(x, s)
    assert _distinct(q) > 20, "the rounded input is degenerate"
    assert sh.same_bits(y, twin.execute(q))
    assert twin.last_input_quantiser() == "none"


# ------------------------------------------------------------------ 2. round only
@pytest.mark.parametrize("kind", ["cf32", 16], ids=str)
def test_round_only(gpu, profiling, kind):
    """rms <= 0: scale 1, no moments; the product is the twin's on round(x)."""
    inp, x = _input(gpu, kind, 2, _n_dat(C2, 37, 11), 4100)
    if kind == "cf32":
        inp = x = (x * 0.2).contiguous()     # rms 20: the fractions matter
    twin = _plan(C2, 2)
    for rms in (0.0, -3.0):
        plan = _qplan(C2, 2, rms)
        y = _run(plan, inp, kind)
        assert plan.last_input_quantiser() == "fused" and plan.last_input_scale() == 1.0
        assert "analysis_stream_qin_kernel<" in _kernel_name(0)
        q = _rounded(x, 1.0)
        assert _distinct(q) > 20
        assert sh.same_bits(y, twin.execute(q))


# ------------------------------------------------------------------ 3. stream sequences
def _sequence(gpu, pk, chunks, kinds, seed, n_pol=2):
    """The chunks through one plan, the twin fed each chunk rounded at that chunk's own scale:
    after every call the output and the buffered count are the twin's.  -> (paths taken, rows)."""
    plan, twin = _qplan(pk, n_pol), _plan(pk, n_pol)
    paths, rows = [], []
    for i, (n, kind) in enumerate(zip(chunks, kinds)):
        inp, x = _input(gpu, kind, n_pol, n, seed + i)
        y = _run(plan, inp, kind, stateful=True)
        s = plan.last_input_scale()
        _scale_ok(s, x, RMS_IN, f"call {i}")
        q = _rounded(x, s)
        assert _distinct(q) > 20
        ref = twin.execute(q, stateful=True)
        assert sh.same_bits(y, ref), f"call {i} ({n} samples, {kind})"
        assert plan.buffered_samples == twin.buffered_samples, i
        paths.append(plan.last_input_quantiser())
        rows.append(int(y.shape[1]))
    return paths, rows


@pytest.mark.parametrize("first", ["cf32", 16], ids=["cf32-first", "section-first"])
@pytest.mark.parametrize("shape", ["c2-p13", "lowcbf"])
def test_stream_sequence(gpu, shape, first):
    """(9000, 100, 7777), cf32 and section calls alternating on one plan.  The 100-sample chunk
    completes no row: it rounds its samples into the carry behind the older carry, which keeps its
    own rounding — the third call's output proves it."""
    other = 16 if first == "cf32" else "cf32"
    paths, rows = _sequence(gpu, SHAPES[shape], CHUNKS, (first, other, first), 4200)
    assert rows[1] == 0 and rows[0] > 0 and rows[2] > 0
    assert paths[0] == "fused" and set(paths) <= {"fused", "staged"}, paths
    if shape == "c2-p13":
        # (the third call reads its samples in place, the carry through the kernel's window)
        assert paths[2] == "fused", paths


def test_stream_sequence_new_carry_inside_the_old(gpu):
    """Chunks so short that the next carry starts inside the old one (0 < input_idat < B): the
    call concatenates (STAGED), and the old carry's samples are not rounded again."""
    plan, twin = _qplan(C2, 2), _plan(C2, 2)
    for i, (n, kind) in enumerate(((9000, "cf32"), (1600, 16), (1800, "cf32"), (7777, 16))):
        inp, x = _input(gpu, kind, 2, n, 4320 + i)
        B = plan.buffered_samples
        rows = plan.stream_rows(n)
        y = _run(plan, inp, kind, stateful=True)
        q = _rounded(x, plan.last_input_scale())
        assert sh.same_bits(y, twin.execute(q, stateful=True)), i
        assert plan.buffered_samples == twin.buffered_samples
        if i in (1, 2):
            assert 0 < rows * 224 < B, (i, rows, B)
            assert plan.last_input_quantiser() == "staged"


# ------------------------------------------------------------------ 4. partition
def test_several_steps_per_workgroup_and_no_stale_partials(gpu):
    """64 series: each workgroup walks several 16-row steps.  Then a short call on the same plan:
    its scale is its own (fewer slots than the long call left behind)."""
    import torch
    from test_gpu_partition import RANGES, _split, _steps
    S = 64
    cu = torch.cuda.get_device_properties(gpu).multi_processor_count
    per_pol = max(1, 2 * cu // S)
    rows_large, rows_small = 16 * 2 * per_pol + 21, 37
    n_steps = _steps(rows_large, 8)
    sizes = _split(n_steps, RANGES["stream"](cu, S, n_steps))
    assert max(sizes) >= 2 and min(sizes) >= 2, sizes
    plan, twin = _qplan(C2, S), _plan(C2, S)
    scales = []
    for i, rows in enumerate((rows_large, rows_small, rows_large)):
        x = _series(gpu, S, _n_dat(C2, rows, 5), 4400 + i, amp=10.0 * (1 + 3 * (i == 1)))
        y = plan.execute(x)
        s = plan.last_input_scale()
        _scale_ok(s, x, RMS_IN, f"{rows} rows x {S} series")
        assert plan.last_input_quantiser() == "fused"
        assert sh.same_bits(y, twin.execute(_rounded(x, s))), rows
        scales.append(s)
    assert scales[1] < 0.5 * scales[0]   # (the short call's input is four times as strong)


# ------------------------------------------------------------------ 5. staged
STAGED = {"padded-n256": (PADDED, None), "bunton-n64": (N64, None), "fir-rowfft-n512": (N512, None),
          "c2-mode-staged": (C2, "staged")}


@pytest.mark.parametrize("kind", ["cf32", 16], ids=str)
@pytest.mark.parametrize("case", list(STAGED))
def test_staged_plans(gpu, case, kind):
    pk, mode = STAGED[case]
    plan, twin = _qplan(pk, 2, mode=mode), _plan(pk, 2)
    inp, x = _input(gpu, kind, 2, _n_dat(pk, 37, 11), 4500 + len(case))
    y = _run(plan, inp, kind)
    assert plan.last_input_quantiser() == "staged" and y.shape[1] == 37
    s = plan.last_input_scale()
    _scale_ok(s, x, RMS_IN, case)
    q = _rounded(x, s)
    assert _distinct(q) > 20
    assert sh.same_bits(y, twin.execute(q))
    # stream calls: with nothing buffered, with a carry, and one that completes no row
    for i, n in enumerate((x.shape[1], 3001, 50, 2500)):
        inp, xs = _input(gpu, kind, 2, n, 4550 + i)
        y = _run(plan, inp, kind, stateful=True)
        q = _rounded(xs, plan.last_input_scale())
        assert sh.same_bits(y, twin.execute(q, stateful=True)), (case, i)
        assert plan.buffered_samples == twin.buffered_samples and plan.last_input_quantiser() == "staged"


def test_host_memory_filterbank_call_is_staged(gpu):
    plan, twin = _qplan(C2, 2), _plan(C2, 2)
    for i, n in enumerate(CHUNKS):
        x = _series(gpu, 2, n, 4600 + i)
        y = plan.execute(x.cpu().numpy(), stateful=True)
        assert plan.last_input_quantiser() == "staged"
        s = plan.last_input_scale()
        _scale_ok(s, x, RMS_IN, f"host call {i}")
        ref = twin.execute(_rounded(x, s).cpu().numpy(), stateful=True)
        assert y.shape == ref.shape and np.array_equal(y.view(np.uint8), ref.view(np.uint8)), i
        assert plan.buffered_samples == twin.buffered_samples
    # the stateless host call
    x = _series(gpu, 2, _n_dat(C2, 37, 11), 4610)
    y = plan.execute(x.cpu().numpy())
    ref = twin.execute(_rounded(x, plan.last_input_scale()).cpu().numpy())
    assert plan.last_input_quantiser() == "staged" and np.array_equal(y.view(np.uint8), ref.view(np.uint8))


def test_execute_strided_is_staged(gpu):
    import torch
    plan, twin = _qplan(C2, 2), _plan(C2, 2)
    for i, n in enumerate(CHUNKS):
        x = _series(gpu, 2, n, 4700 + i)
        rows = plan.stream_rows(n)
        Tc = max(16, (rows + 15) // 16 * 16)
        outs = [torch.full((2, 256, Tc), sh.SENTINEL, dtype=torch.complex64, device=gpu) for _ in range(2)]
        got = plan.execute_strided(x, outs[0], 256 * Tc, 1, Tc)
        assert plan.last_input_quantiser() == "staged"
        q = _rounded(x, plan.last_input_scale())
        assert twin.execute_strided(q, outs[1], 256 * Tc, 1, Tc) == got == rows
        assert sh.same_bits(outs[0], outs[1]), i
        assert plan.buffered_samples == twin.buffered_samples


def test_fused_against_staged(gpu):
    inp, x = _input(gpu, 16, 2, _n_dat(C2, 37, 11), 4800)
    fused, staged = _qplan(C2, 2, mode="fused"), _qplan(C2, 2, mode="staged")
    for kind, arg in (("cf32", x), (16, inp)):
        a, b = _run(fused, arg, kind), _run(staged, arg, kind)
        assert (fused.last_input_quantiser(), staged.last_input_quantiser()) == ("fused", "staged")
        sa, sb = fused.last_input_scale(), staged.last_input_scale()
        assert np.float64(sa).tobytes() == np.float64(sb).tobytes(), (kind, sa, sb)
        assert sh.same_bits(a, b), kind
    with pytest.raises(ValueError):
        staged.set_input_quantiser_mode("sometimes")


def test_mode_fused_on_a_padded_plan_is_unsupported(gpu):
    import torch
    from ska_pst_dsp_model_amd import _lib
    plan, twin = _qplan(PADDED, 2), _plan(PADDED, 2)
    x0 = _series(gpu, 2, 9000, 4900)
    y = plan.execute(x0, stateful=True)
    assert sh.same_bits(y, twin.execute(_rounded(x0, plan.last_input_scale()), stateful=True))
    buffered = plan.buffered_samples
    plan.set_input_quantiser_mode("fused")
    x = _series(gpu, 2, 7777, 4901)
    st, n_out, out = _abi_stream_call(plan, gpu, x)
    assert st == _lib.PFB_ERR_UNSUPPORTED and plan.buffered_samples == buffered
    assert bool((out == sh.SENTINEL).all()) and plan.last_input_quantiser() == "staged"
    with pytest.raises(_lib.PfbError):
        plan.execute(x)
    plan.set_input_quantiser_mode("auto")
    y = plan.execute(x, stateful=True)
    assert sh.same_bits(y, twin.execute(_rounded(x, plan.last_input_scale()), stateful=True))
    del torch


# ------------------------------------------------------------------ 6. with the outputs that exist
@pytest.mark.parametrize("kind", ["cf32", 16], ids=str)
@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "stream"])
def test_to_dada_and_quantised_to_dada(gpu, kind, stateful):
    """_to_dada at NBIT 16 and _quantised_to_dada at NBIT 8 with both quantisers on: the twin's
    same call on q, and the output side's reports are the twin's."""
    calls = {
        "to_dada": (lambda p, a: p.execute_to_dada(a, 16, scale=0.01, stateful=stateful),
                    lambda p, a: p.execute_dada_to_dada(a, 16, 16, scale=0.01, stateful=stateful)),
        "quantised": (lambda p, a: p.execute_quantised_to_dada(a, 8, 20.0, stateful=stateful),
                      lambda p, a: p.execute_dada_quantised_to_dada(a, 16, 8, 20.0, stateful=stateful)),
    }
    for name, (cf, dd) in calls.items():
        plan, twin = _qplan(C2, 2), _plan(C2, 2)
        for i, n in enumerate(CHUNKS if stateful else (_n_dat(C2, 37, 11),)):
            inp, x = _input(gpu, kind, 2, n, 5000 + i)
            sec = (cf if kind == "cf32" else dd)(plan, inp)
            assert plan.last_input_quantiser() in ("fused", "staged")
            if name == "quantised" and sec.shape[0] and (kind == "cf32" or not stateful or i != 1):
                assert plan.last_input_quantiser() == "fused", (name, i)
            q = _rounded(x, plan.last_input_scale())
            assert _distinct(q) > 20
            ref = cf(twin, q)
            assert sec.shape == ref.shape and np.array_equal(_bytes(sec), _bytes(ref)), (name, i)
            assert plan.last_quantiser() == twin.last_quantiser(), (name, i)
            assert plan.last_dada_output() == twin.last_dada_output(), (name, i)
            assert plan.buffered_samples == twin.buffered_samples
        assert sec.shape[0] > 0


def test_round_trip_with_such_a_plan_is_unsupported(gpu):
    from ska_pst_dsp_model_amd import _lib
    pfb = _pfb()
    taps = _taps(256, "8/7", 12)
    plan, twin = _qplan(C2, 2), _plan(C2, 2)
    syn = pfb.SynthesisPlan(256, "8/7", 256, 32, True, 1, False, taps, None, None, 2)
    x0 = _series(gpu, 2, 9000, 5100)
    y = plan.execute(x0, stateful=True)
    assert sh.same_bits(y, twin.execute(_rounded(x0, plan.last_input_scale()), stateful=True))
    buffered = plan.buffered_samples
    x = _series(gpu, 2, 256 * 13 + 224 * 256 * 2, 5101)
    with pytest.raises(_lib.PfbError) as e:
        pfb.roundtrip(plan, syn, x)
    assert e.value.status == _lib.PFB_ERR_UNSUPPORTED
    with pytest.raises(_lib.PfbError) as e:
        pfb.core.roundtrip_analysis(plan, syn, x)
    assert e.value.status == _lib.PFB_ERR_UNSUPPORTED
    # the plan's stream state is as it was
    assert plan.buffered_samples == buffered
    x1 = _series(gpu, 2, 7777, 5102)
    y = plan.execute(x1, stateful=True)
    assert sh.same_bits(y, twin.execute(_rounded(x1, plan.last_input_scale()), stateful=True))


# ------------------------------------------------------------------ 7. guards and rejections
def _abi_stream_call(plan, gpu, x, cap_rows=None):
    """pfb_filterbank_execute into a sentinel buffer -> (status, n_out, the buffer)."""
    import torch
    n = int(x.shape[1])
    room = (plan.buffered_samples + n) // max(plan.step, 1) + 1     # (the buffer and its stride hold every row)
    rows = room if cap_rows is None else cap_rows
    out = torch.full((plan.n_pol, room, plan.out_chan), sh.SENTINEL, dtype=torch.complex64, device=gpu)
    n_out = ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    st = plan._lib.pfb_filterbank_execute(plan._h, ctypes.c_void_p(x.data_ptr()), n, n, ctypes.c_void_p(out.data_ptr()),
                                          room * plan.out_chan, rows, ctypes.byref(n_out), 0, stream)
    torch.cuda.synchronize(gpu)
    return st, n_out.value, out


@pytest.mark.parametrize("mode", ["fused", "staged"])
def test_framed_input_equals_the_contiguous_call(gpu, mode):
    """cf32 with an odd lead (8-byte aligned only) and a gapped, odd polarisation stride; a section
    offset by one complex sample: bit-identical to the contiguous call, same scale bits."""
    import torch
    n_pol, n = 2, _n_dat(C2, 37, 11)
    plan, ref_plan = _qplan(C2, n_pol, mode=mode), _qplan(C2, n_pol, mode=mode)
    lib = plan._lib
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    x = _series(gpu, n_pol, n, 5200)
    ref = ref_plan.execute(x)
    s_ref = ref_plan.last_input_scale()
    lead, ps = 1, n + 3
    holder = torch.full((lead + n_pol * ps + 8,), complex(float("nan"), float("nan")), dtype=torch.complex64, device=gpu)
    assert holder.data_ptr() % 16 == 0
    for p in range(n_pol):
        holder[lead + p * ps: lead + p * ps + n] = x[p]
    out = torch.empty_like(ref)
    n_out = ctypes.c_int64(-1)
    st = lib.pfb_analysis_execute(plan._h, ctypes.c_void_p(holder.data_ptr() + 8 * lead), ps, n,
                                  ctypes.c_void_p(out.data_ptr()), out.shape[1] * out.shape[2], out.shape[1],
                                  ctypes.byref(n_out), 0, stream)
    assert st == 0 and n_out.value == 37 and plan.last_input_quantiser() == mode
    assert np.float64(plan.last_input_scale()).tobytes() == np.float64(s_ref).tobytes()
    assert sh.same_bits(out, ref)
    # a section offset by one complex sample (4 bytes at NBIT 16: not 16-byte aligned)
    rawd, xs = _input(gpu, 16, n_pol, n, 5201)
    ref = ref_plan.execute_dada(rawd, 16)
    s_ref = ref_plan.last_input_scale()
    frame = torch.full((rawd.numel() + 64,), 0x7F, dtype=torch.uint8, device=gpu)
    frame[4: 4 + rawd.numel()] = rawd
    out = torch.empty_like(ref)
    st = lib.pfb_analysis_execute_dada(plan._h, ctypes.c_void_p(frame.data_ptr() + 4), 16, 2, 0, n,
                                       ctypes.c_void_p(out.data_ptr()), out.shape[1] * out.shape[2], out.shape[1],
                                       ctypes.byref(n_out), stream)
    assert st == 0 and n_out.value == 37 and plan.last_input_quantiser() == mode
    assert np.float64(plan.last_input_scale()).tobytes() == np.float64(s_ref).tobytes()
    assert sh.same_bits(out, ref)
    _scale_ok(s_ref, xs, RMS_IN, "offset section")


def test_rejections_leave_everything_untouched(gpu):
    import torch
    from ska_pst_dsp_model_amd import _lib
    plan, twin = _qplan(C2, 2), _plan(C2, 2)
    x0 = _series(gpu, 2, CHUNKS[0], 5300)
    y = plan.execute(x0, stateful=True)
    assert sh.same_bits(y, twin.execute(_rounded(x0, plan.last_input_scale()), stateful=True))
    buffered = plan.buffered_samples
    assert buffered > 0
    x = _series(gpu, 2, CHUNKS[2], 5301)
    # a non-finite rms: the setter refuses, the plan keeps its setting
    for bad in (float("nan"), float("inf")):
        with pytest.raises(_lib.PfbError) as e:
            plan.set_input_quantiser(bad)
        assert e.value.status == _lib.PFB_ERR_INVALID_ARG
    # an output capacity one row short
    st, n_out, out = _abi_stream_call(plan, gpu, x, cap_rows=plan.stream_rows(x.shape[1]) - 1)
    assert st == _lib.PFB_ERR_BUFFER_TOO_SMALL and bool((out == sh.SENTINEL).all())
    assert plan.buffered_samples == buffered
    # the carry is as it was: the corrected call gives the twin's rows
    y = plan.execute(x, stateful=True)
    assert sh.same_bits(y, twin.execute(_rounded(x, plan.last_input_scale()), stateful=True))
    # cnt < 2 with rms > 0: one sample of one polarisation
    one, one_twin = _qplan(C2, 1), _plan(C2, 1)
    x1 = _series(gpu, 1, 5000, 5302)
    y = one.execute(x1, stateful=True)
    assert sh.same_bits(y, one_twin.execute(_rounded(x1, one.last_input_scale()), stateful=True))
    buffered = one.buffered_samples
    st, _, out = _abi_stream_call(one, gpu, x1[:, :1].contiguous())
    assert st == _lib.PFB_ERR_INVALID_ARG and bool((out == sh.SENTINEL).all()) and one.buffered_samples == buffered
    x2 = _series(gpu, 1, 4000, 5303)
    y = one.execute(x2, stateful=True)
    assert sh.same_bits(y, one_twin.execute(_rounded(x2, one.last_input_scale()), stateful=True))
    # (round only takes the single sample)
    one.set_input_quantiser(0.0)
    st, _, _ = _abi_stream_call(one, gpu, x1[:, :1].contiguous())
    assert st == 0 and one.buffered_samples == one_twin.buffered_samples + 1
    # LowCBF: a rejected first call leaves the pre-padding pending
    lplan, ltwin = _qplan("lowcbf", 2), _plan("lowcbf", 2)
    xl = _series(gpu, 2, CHUNKS[0], 5304)
    st, _, out = _abi_stream_call(lplan, gpu, xl, cap_rows=1)
    assert st == _lib.PFB_ERR_BUFFER_TOO_SMALL and bool((out == sh.SENTINEL).all()) and lplan.buffered_samples == 0
    y = lplan.execute(xl, stateful=True)
    assert sh.same_bits(y, ltwin.execute(_rounded(xl, lplan.last_input_scale()), stateful=True))
    del torch


# ------------------------------------------------------------------ 8. determinism and streams
@pytest.mark.parametrize("mode", ["fused", "staged"])
def test_two_calls_give_the_same_bits(gpu, mode):
    x = _series(gpu, 2, _n_dat(C2, 117, 3), 5400)
    plan = _qplan(C2, 2, mode=mode)
    a = plan.execute(x).clone()
    sa = plan.last_input_scale()
    b = plan.execute(x)
    sb = plan.last_input_scale()
    assert np.float64(sa).tobytes() == np.float64(sb).tobytes()
    assert sh.same_bits(a, b) and plan.last_input_quantiser() == mode


def _chunk_sections(gpu, seed):
    return [_input(gpu, 16, 2, n, seed + i)[0] for i, n in enumerate(CHUNKS)]


STREAM_ENTRIES = {
    "analysis": (False, lambda p, x: p.execute(x)),
    "filterbank": (True, lambda p, x: p.execute(x, stateful=True)),
    "filterbank_dada_to_dada": (True, lambda p, x: p.execute_dada_to_dada(x, 16, 16, scale=0.01, stateful=True)),
}


@pytest.mark.parametrize("entry", list(STREAM_ENTRIES))
def test_entries_on_a_side_stream(gpu, entry):
    """tests/stream_harness.py: the call on a non-blocking side stream behind the delay kernel,
    with poisoned input, equals the default-stream call bit for bit (no scale read-back)."""
    stateful, call = STREAM_ENTRIES[entry]
    if "dada" in entry:
        xs = _chunk_sections(gpu, 5500)
    else:
        xs = [_series(gpu, 2, n, 5520 + n) for n in (CHUNKS if stateful else (_n_dat(C2, 117, 3),))]

    def check(p):
        assert p.last_input_quantiser() in ("fused", "staged")

    ref, _ = sh.poison_delay(f"quantised input {entry}", lambda: _qplan(C2, 2),
                             lambda p, xs, outs: [call(p, x) for x in xs], xs,
                             reset=lambda p: p.reset(), buffered=lambda p: p.buffered_samples, check=check)
    assert ref[-1].numel() > 0


@pytest.mark.parametrize("mode", ["fused", "staged"])
def test_replay_from_a_graph(gpu, mode):
    from test_gpu_streams import _captured
    plan = _qplan(C2, 2, mode=mode)
    inputs = [_series(gpu, 2, _n_dat(C2, 117, 3), 5600 + k, amp=10.0 * (k + 1)) for k in range(3)]
    _captured(f"execute with the input quantiser {mode}", plan, lambda x: plan.execute(x), inputs)


# ------------------------------------------------------------------ 9. oracle
def test_matches_the_oracle(gpu):
    """FilterBank(rndInput, rmsInput 20, fused_input_quantiser) over three chunks against
    FilterBankOracle (quantiser off) fed orc.quantize(x, s_dev): the device's scale for the
    oracle's rounding, so that a float32 rounding boundary of the scale cannot flip an input integer
    and hide behind a tolerance; the scale itself is checked apart.  No sample is excluded."""
    pfb = _pfb()
    taps = _taps(256, "8/7", 12)
    ref_fb = orc.FilterBankOracle(taps, 256, "8/7")
    fb = pfb.FilterBank(_fb_cfg(rndInput=True, rmsInput=RMS_IN), fused_input_quantiser=True)
    for i, n in enumerate(CHUNKS):
        x = _series(gpu, 2, n, 5700 + i)
        _, y = fb.execute(x)
        s = fb._plan.last_input_scale()
        _scale_ok(s, x, RMS_IN, f"chunk {i}")
        q = orc.quantize(x.cpu().numpy(), s)
        assert len(np.unique(q.view(np.float32))) > 20
        ref = ref_fb.execute(q)
        assert fb.buffered_samples == ref_fb.buffered_samples
        assert_pfb_close(y.cpu().numpy(), ref, tol=PARITY_TOL, what=f"chunk {i}")
    assert fb._plan.last_input_quantiser() == "fused"


# ------------------------------------------------------------------ 10. Python surface
def _candidates(x, rms):
    s = orc.quantize_scale(x.cpu().numpy(), rms)
    return [_rounded(x, v) for v in (s, s * (1 - 1e-9), s * (1 + 1e-9))]


def test_filterbank_object_with_the_fused_input_quantiser(gpu):
    """With the flag every entry takes the plan's quantiser; the results are the flag-less
    object's, within the scale's float32 rounding boundary (three candidates, as
    test_filterbank_object_with_the_fused_quantiser)."""
    pfb = _pfb()
    cfg = _fb_cfg(rndInput=True, rmsInput=RMS_IN)
    fb, also = pfb.FilterBank(cfg, fused_input_quantiser=True), pfb.FilterBank(dict(cfg, fused_input_quantiser=True))
    plain = pfb.FilterBank(cfg)
    assert fb.fused_input_quantiser and also.fused_input_quantiser and not plain.fused_input_quantiser
    # execute: equal to the plain analysis of one of the candidates, call by call
    twins = [_plan(C2, 2) for _ in range(3)]
    for i, n in enumerate(CHUNKS):
        x = _series(gpu, 2, n, 5800 + i)
        _, y = fb.execute(x)
        _, yp = plain.execute(x)
        assert fb._plan.last_input_quantiser() != "none" and plain._plan.last_input_quantiser() == "none"
        # (the flag-less object rounds with pfb_quantize's scale: one of the candidates too)
        outs = [t.execute(q, stateful=True).transpose(1, 2) for t, q in zip(twins, _candidates(x, RMS_IN))]
        assert any(sh.same_bits(y, o) for o in outs), i
        assert any(sh.same_bits(yp, o) for o in outs), i
        assert fb.buffered_samples == plain.buffered_samples
        # (keep the three twins' carries in step: each has taken its own candidate, which differ
        # at most where the scale sits on a rounding boundary)
    # execute_dada: the section is read in place
    rawd, xs = _input(gpu, 16, 2, 9000, 5810)
    _, y = also.execute_dada(rawd, 16, n_pol=2)
    assert also._plan.last_input_quantiser() == "fused" and also._plan.last_dada_input() == "fused"
    outs = [_plan(C2, 2).execute(q, stateful=True) for q in _candidates(xs, RMS_IN)]
    assert any(sh.same_bits(y.transpose(1, 2), o) for o in outs)
    # the to-DADA calls no longer fall back because of rndInput
    fresh = pfb.FilterBank(cfg, fused_input_quantiser=True)
    _, sec = fresh.execute_dada_to_dada(rawd, 16, 16, scale=0.01, n_pol=2)
    assert fresh._plan.last_input_quantiser() != "none" and fresh._plan.last_dada_output() == "fused"
    refs = [_plan(C2, 2).execute_to_dada(q, 16, scale=0.01, stateful=True) for q in _candidates(xs, RMS_IN)]
    assert any(np.array_equal(_bytes(sec), _bytes(r)) for r in refs)
    fresh = pfb.FilterBank(cfg, fused_input_quantiser=True)
    _, sec = fresh.execute_to_dada(xs, 16, scale=0.01)
    assert fresh._plan.last_input_quantiser() != "none" and fresh._plan.last_dada_output() == "fused"
    assert any(np.array_equal(_bytes(sec), _bytes(r)) for r in refs)
    # both quantisers: the fused output quantiser holds with rndInput as well
    both = pfb.FilterBank(dict(cfg, rndOutput=True, rmsOutput=20.0), fused_quantiser=True, fused_input_quantiser=True)
    assert both._quantiser_fused()
    _, sec = both.execute_to_dada(xs, 8)
    assert both._plan.last_quantiser() == "fused" and both._plan.last_input_quantiser() == "fused"
    refs = [_plan(C2, 2).execute_quantised_to_dada(q, 8, 20.0, stateful=True) for q in _candidates(xs, RMS_IN)]
    assert any(np.array_equal(_bytes(sec), _bytes(r)) for r in refs)


def test_filterbank_object_without_the_flag_is_as_it_was(gpu):
    from ska_pst_dsp_model_amd import layout
    pfb = _pfb()
    cfg = _fb_cfg(rndInput=True, rmsInput=RMS_IN)
    fb = pfb.FilterBank(cfg)
    twin = _plan(C2, 2)
    assert not fb.fused_input_quantiser and not pfb.FilterBank(_fb_cfg()).fused_input_quantiser
    for i, n in enumerate(CHUNKS):
        x = _series(gpu, 2, n, 5900 + i)
        _, y = fb.execute(x)
        assert fb._plan.last_input_quantiser() == "none"
        ref = twin.execute(layout.quantize(x, RMS_IN), stateful=True)
        assert sh.same_bits(y.transpose(1, 2), ref), i
    rawd, xs = _input(gpu, 16, 2, 9000, 5910)
    fb2 = pfb.FilterBank(cfg)
    fb2.execute_dada(rawd, 16, n_pol=2)
    assert fb2._plan.last_input_quantiser() == "none" and fb2._plan.last_dada_input() == "none"
    # the two-stage objects ignore the flag
    ts = pfb.TwoStageFilterBank(dict(cfg, fused_input_quantiser=True))
    assert not ts.stage1.fused_input_quantiser and not ts.build().stage2.fused_input_quantiser
