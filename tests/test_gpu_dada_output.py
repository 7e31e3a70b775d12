"""Analysis writing its product straight into a DADA data section
(pfb_analysis_execute_to_dada, pfb_filterbank_execute_to_dada and their _dada_to_dada twins):
the streaming kernel converts and stores the NBIT 8 / 16 / 32 samples itself
(analysis_stream_dadaout_kernel) instead of the packed complex float32 product that
pfb_dada_pack would read back.

The contract is bit-identity with the pair: the corresponding cf32-output call, both
components times float32(scale), pfb_dada_pack.  Every comparison against the pair is
np.array_equal on bytes, with inputs over the input type's full range and a scale under which
the pair's own output saturates, rounds in both directions and meets exact .5 ties (asserted,
so no case passes vacuously).  Every output buffer is framed by a byte pattern that must
survive.  The oracle cases bound each quantised component by half a step plus the project's
1e-6 (conftest.assert_pfb_close) of its own element.  A few dozen output rows per case.
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import PARITY_TOL, assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

PAT = 0xA5      # the frame's byte
FRAME = 512     # bytes of frame on each side of the output buffer (keeps its alignment)
SPARE_ROWS = 3  # capacity beyond the rows due, pattern-filled


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _file_samples(rng, nbit, count):
    """Samples over the full range of the file's type."""
    t = orc._NBIT_NP[nbit]
    if np.issubdtype(t, np.integer):
        info = np.iinfo(t)
        return rng.integers(info.min, info.max + 1, size=count).astype(t)
    return rng.standard_normal(count).astype(t)


@functools.lru_cache(maxsize=None)
def _taps(N, os_, tpc, cut=None):
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
    """kind: (N, os, tpc, cut, variant) or "lowcbf"."""
    pfb = _pfb()
    if kind == "lowcbf":
        return pfb.AnalysisPlan(_pst_taps(), 256, "4/3", "polyphase_analysis_lowcbf", n_pol)
    N, os_, tpc, cut, variant = kind
    return pfb.AnalysisPlan(_taps(N, os_, tpc, cut), N, os_, variant, n_pol)


BUNTON = "polyphase_analysis"
C2 = (256, "8/7", 12, None, BUNTON)            # 3073 taps: 13 phases
C2_P12 = (256, "8/7", 12, 3072, BUNTON)        # 3072 taps: 12 phases
F43 = (256, "4/3", 12, None, BUNTON)           # 13 phases
F43_P12 = (256, "4/3", 12, 3072, BUNTON)
STREAM_SHAPES = {"c2-p13": C2, "c2-p12": C2_P12, "4over3-p13": F43, "4over3-p12": F43_P12, "lowcbf": "lowcbf"}


def _n_dat(kind, rows, extra):
    """Samples that give `rows` output rows of a stateless (first) call, plus a ragged tail."""
    if kind == "lowcbf":
        return 3072 - 1536 + rows * 192 + extra
    N, os_, tpc, cut, variant = kind
    nu, de = (int(v) for v in os_.split("/"))
    M = N * de // nu
    if variant != BUNTON:
        return rows * M + extra
    n_taps = cut or N * tpc + 1
    return -(-n_taps // N) * N + rows * M + extra


def _section(gpu, seed, nbit, n_dat, n_pol, ndim=2):
    import torch
    raw = _file_samples(np.random.default_rng(seed), nbit, n_dat * n_pol * ndim)
    return raw, torch.from_numpy(raw.view(np.uint8)).to(gpu)


def _unpacked(rawd, nbit, n_pol):
    from ska_pst_dsp_model_amd import layout
    return layout.dada_unpack(rawd, nbit, 2, 1, n_pol)[:, :, 0].contiguous()


def _pack_pair(out, nbit, scale):
    """The pair's second half: both components times float32(scale), then pfb_dada_pack.
    `out`: the (n_pol, rows, chan) complex64 device product -> the section's bytes (numpy)."""
    import torch
    from ska_pst_dsp_model_amd import layout
    scaled = torch.view_as_complex((torch.view_as_real(out.contiguous()) * float(np.float32(scale))).contiguous())
    return layout.dada_pack(scaled, nbit).cpu().numpy().view(np.uint8)


def _kernel_name(which=0):
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


def _row_bytes(plan, out_nbit):
    return plan.out_chan * plan.n_pol * 2 * (out_nbit // 8)


def _call(plan, gpu, out_nbit, scale, x=None, rawd=None, in_nbit=None, stateful=False, cap_bytes=None,
          offset=0, null_out=False):
    """One raw C-ABI to-DADA call into a framed buffer: cf32 input `x` (n_pol, n) or a DADA
    section `rawd` of in_nbit.  The capacity defaults to the rows due plus SPARE_ROWS.
    -> (status, n_out, host bytes of the whole framed buffer, offset of `out` in it, capacity)"""
    import torch
    lib = plan._lib
    if x is not None:
        n = int(x.shape[1])
    else:
        n = rawd.numel() // (plan.n_pol * 2 * (in_nbit // 8))
    rows = plan.stream_rows(n) if stateful else plan.output_length(n)
    rb = _row_bytes(plan, out_nbit) if out_nbit in (8, 16, 32, 64) else plan.out_chan * plan.n_pol * 2
    cap = (rows + SPARE_ROWS) * rb if cap_bytes is None else cap_bytes
    holder = torch.full((FRAME + offset + cap + FRAME,), PAT, dtype=torch.uint8, device=gpu)
    assert holder.data_ptr() % 16 == 0
    out = ctypes.c_void_p(0 if null_out else holder.data_ptr() + FRAME + offset)
    n_out = ctypes.c_int64(-1)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    if x is not None:
        fn = lib.pfb_filterbank_execute_to_dada if stateful else lib.pfb_analysis_execute_to_dada
        st = fn(plan._h, ctypes.c_void_p(x.data_ptr()), n, n, out, out_nbit, scale, cap, ctypes.byref(n_out), stream)
    else:
        from ska_pst_dsp_model_amd import _lib
        fn = lib.pfb_filterbank_execute_dada_to_dada if stateful else lib.pfb_analysis_execute_dada_to_dada
        st = fn(plan._h, ctypes.c_void_p(rawd.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, n, out, out_nbit, scale,
                cap, ctypes.byref(n_out), stream)
    torch.cuda.synchronize(gpu)
    return st, n_out.value, holder.cpu().numpy(), FRAME + offset, cap


def _written(h, off, nbytes, what=""):
    """The first nbytes of `out`; everything else of the framed buffer must be the pattern."""
    assert (h[:off] == PAT).all(), f"{what}: bytes before the section were written"
    assert (h[off + nbytes:] == PAT).all(), f"{what}: bytes beyond row n_out were written"
    return h[off:off + nbytes]


def _tie_scale(ref, nbit):
    """A float32 scale, not a power of two, that puts the rms of the product's components near
    a third of the integer range and makes float32(scale * v) of one component v of `ref`
    (the pair's cf32 product) an exact k + 0.5."""
    comp = np.abs(ref.view(np.float32).ravel())
    comp = comp[(comp > 0) & np.isfinite(comp)]
    rms = float(np.sqrt(np.mean(comp.astype(np.float64) ** 2)))
    if nbit == 32:
        return float(np.float32(0.37 / rms))
    full = float(np.iinfo(orc._NBIT_NP[nbit]).max)
    s0 = full / 3.0 / rms
    k = np.floor(s0 * comp.astype(np.float64))
    cand = ((k + 0.5) / comp.astype(np.float64)).astype(np.float32)
    mant, _ = np.frexp(cand)
    ok = ((cand * comp) == (k + 0.5).astype(np.float32)) & (k >= 20) & (k + 0.5 < full) & (mant != 0.5) & \
         (np.abs(cand / np.float32(s0) - 1) < 0.05)
    assert ok.any(), "no component of the product makes an exact tie near the target scale"
    return float(cand[np.argmax(ok)])


def _assert_pair_is_demanding(ref, pair_bytes, nbit, scale):
    """Saturation, both rounding directions and an exact .5 tie all occur in the pair's output."""
    if nbit == 32:
        return
    t = orc._NBIT_NP[nbit]
    info = np.iinfo(t)
    v = np.float32(scale) * ref.transpose(1, 2, 0).reshape(-1).view(np.float32)  # TFP order, float32 product
    q = pair_bytes.view(t).astype(np.float64)
    assert q.shape == v.shape
    a = np.abs(v.astype(np.float64))
    frac = a - np.floor(a)
    inside = a < info.max
    tie = inside & (frac == 0.5)
    assert tie.any() and (np.abs(q[tie]) == np.floor(a[tie]) + 1).all(), "ties round away from zero"
    assert (inside & (frac > 0.5)).any() and (inside & (frac < 0.5) & (frac > 0)).any()
    sat = a > info.max + 1
    assert sat.any() and ((q[sat] == info.max) | (q[sat] == info.min)).all()
    rms = np.sqrt(np.mean(v.astype(np.float64) ** 2))
    assert 0.25 * info.max < rms < 0.42 * info.max, rms


# ------------------------------------------------------------------ 1 + 4. fused == the pair, framed
# (id, plan kind, rows): rows None = a section shorter than the taps
FUSED_SHAPES = [
    ("a-c2-p13-53rows", C2, 53),          # three 16-row steps and a ragged one
    ("b-4over3-37rows", F43, 37),
    ("c-c2-p12-37rows", C2_P12, 37),
    ("d-lowcbf-first-call", "lowcbf", 41),
    ("e-short", C2, None),
]


@pytest.mark.parametrize("n_pol", [1, 2], ids=["1pol", "2pol"])
@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["nbit8", "nbit16", "nbit32"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda c: c[0])
def test_fused_matches_the_pair(gpu, profiling, shape, nbit, n_pol):
    name, kind, rows = shape
    n = _n_dat(kind, rows, 17) if rows is not None else 13 * 256 - 1
    _, rawd = _section(gpu, 1000 + 7 * len(name) + nbit + n_pol, nbit, n, n_pol)
    x = _unpacked(rawd, nbit, n_pol)
    ref_plan = _plan(kind, n_pol)
    ref = ref_plan.execute(x)
    assert tuple(ref.shape) == (n_pol, rows or 0, ref_plan.out_chan)
    assert ref_plan.last_dada_output() == "none"
    rb = _row_bytes(ref_plan, nbit)
    if rows is None:
        # fewer samples than the taps span: OK, 0 rows, nothing written
        for kw in (dict(x=x), dict(rawd=rawd, in_nbit=nbit)):
            plan = _plan(kind, n_pol)
            st, n_out, h, off, _ = _call(plan, gpu, nbit, 0.37, **kw)
            assert (st, n_out) == (0, 0)
            assert _written(h, off, 0, name).size == 0
            assert plan.last_dada_output() == "fused"
        return
    refh = ref.cpu().numpy()
    scale = _tie_scale(refh, nbit)
    pair = _pack_pair(ref, nbit, scale)
    assert pair.size == rows * rb
    _assert_pair_is_demanding(refh, pair, nbit, scale)
    # the _dada twin is the same product (the input side's own contract), so one pair serves both
    # (a fresh plan: a LowCBF plan pre-pads its first call only)
    assert np.array_equal(_plan(kind, n_pol).execute_dada(rawd, nbit).cpu().numpy(), refh)
    for label, kw, in_cls in (("cf32", dict(x=x), "InCf32"), ("dada", dict(rawd=rawd, in_nbit=nbit), f"InDada{nbit}")):
        plan = _plan(kind, n_pol)
        st, n_out, h, off, _ = _call(plan, gpu, nbit, scale, **kw)
        assert (st, n_out) == (0, rows), (label, st, n_out)
        assert plan.last_dada_output() == "fused"
        assert plan.last_dada_input() == ("fused" if label == "dada" else "none")
        kernel = _kernel_name(0)
        print(f"{name} {label}: class 0 {kernel!r}")
        assert "analysis_stream_dadaout_kernel<" in kernel and in_cls in kernel and f"OutDada{nbit}>" in kernel
        assert np.array_equal(_written(h, off, rows * rb, f"{name} {label}"), pair), label
        # the stream call from a fresh plan: T_out < K (53 -> 48, 37 -> 36, 41 -> 40); the nu-trimmed
        # rows must not appear
        plan, twin = _plan(kind, n_pol), _plan(kind, n_pol)
        ref_s = twin.execute(x, stateful=True)
        t_out = int(ref_s.shape[1])
        assert 0 < t_out < rows
        st, n_out, h, off, _ = _call(plan, gpu, nbit, scale, stateful=True, **kw)
        assert (st, n_out) == (0, t_out), (label, st, n_out)
        assert plan.last_dada_output() == "fused"
        assert np.array_equal(_written(h, off, t_out * rb, f"{name} {label} stream"), _pack_pair(ref_s, nbit, scale))
        assert plan.buffered_samples == twin.buffered_samples > 0


def test_fused_scale_one(gpu):
    """scale = 1.0: the product of full-range int16 input is far beyond the int16 range."""
    _, rawd = _section(gpu, 1100, 16, _n_dat(C2, 21, 5), 1)
    x = _unpacked(rawd, 16, 1)
    plan = _plan(C2, 1)
    ref = plan.execute(x)
    pair = _pack_pair(ref, 16, 1.0)
    q = pair.view(np.int16)
    assert (q == 32767).any() and (q == -32768).any() and (np.abs(q.astype(np.int32)) < 32767).any()
    st, n_out, h, off, _ = _call(plan, gpu, 16, 1.0, x=x)
    assert (st, n_out) == (0, 21) and plan.last_dada_output() == "fused"
    assert np.array_equal(_written(h, off, pair.size), pair)
    got = plan.execute_to_dada(x, 16)                      # the Python surface, default scale
    assert tuple(got.shape) == (21, 256, 1, 2) and np.array_equal(got.cpu().numpy().view(np.uint8).ravel(), pair)


# ------------------------------------------------------------------ 2. mixed NBIT
@pytest.mark.parametrize("in_nbit,out_nbit", [(16, 8), (8, 16)], ids=["16to8", "8to16"])
def test_mixed_nbit_stages_the_input_and_fuses_the_output(gpu, profiling, in_nbit, out_nbit):
    n_pol, rows = 2, 37
    _, rawd = _section(gpu, 1200 + in_nbit, in_nbit, _n_dat(C2, rows, 9), n_pol)
    plan = _plan(C2, n_pol)
    ref = plan.execute_dada(rawd, in_nbit)
    scale = _tie_scale(ref.cpu().numpy(), out_nbit)
    pair = _pack_pair(ref, out_nbit, scale)
    st, n_out, h, off, _ = _call(plan, gpu, out_nbit, scale, rawd=rawd, in_nbit=in_nbit)
    assert (st, n_out) == (0, rows)
    assert plan.last_dada_input() == "staged" and plan.last_dada_output() == "fused"
    kernel = _kernel_name(0)
    assert "analysis_stream_dadaout_kernel<" in kernel and "InCf32" in kernel and f"OutDada{out_nbit}>" in kernel
    assert np.array_equal(_written(h, off, pair.size), pair)


# ------------------------------------------------------------------ 3. staged
PADDED = (256, "8/7", 12, None, "polyphase_analysis_padded")
N64 = (64, "8/7", 10, None, BUNTON)
N512 = (512, "4/3", 12, None, BUNTON)
# (id, plan kind, out_nbit, byte offset of `out`)
STAGED_CASES = [
    ("padded-n256", PADDED, 16, 0),
    ("bunton-n64", N64, 8, 0),
    ("fir-rowfft-n512", N512, 16, 0),
    ("nbit64", C2, 64, 0),
    ("out-offset-one-value", C2, 16, 2),
]


@pytest.mark.parametrize("case", STAGED_CASES, ids=lambda c: c[0])
def test_staged_matches_the_pair(gpu, case):
    name, kind, out_nbit, offset = case
    n_pol, rows = 2, 37
    n = _n_dat(kind, rows, 11)
    _, rawd = _section(gpu, 1300 + len(name), 16, n, n_pol)
    x = _unpacked(rawd, 16, n_pol)
    plan, twin = _plan(kind, n_pol), _plan(kind, n_pol)
    ref = twin.execute(x)
    assert ref.shape[1] == rows and float(ref.abs().max()) > 0
    if kind == PADDED:
        # the circular shift wraps: the last sds rows of the call are the first computed ones
        assert 0 < (len(plan.taps) - 1 + 2 * plan.step - 1) // (2 * plan.step) < rows
    scale = _tie_scale(ref.cpu().numpy(), out_nbit if out_nbit != 64 else 32)
    pair = _pack_pair(ref, out_nbit, scale)
    for kw in (dict(x=x), dict(rawd=rawd, in_nbit=16)):
        st, n_out, h, off, _ = _call(plan, gpu, out_nbit, scale, offset=offset, **kw)
        assert (st, n_out) == (0, rows)
        assert plan.last_dada_output() == "staged"
        assert np.array_equal(_written(h, off, pair.size, name), pair)
    # stream calls: the padded variant computes K rows and returns T_out of them
    for i, m in enumerate((n, 3001)):
        _, rd = _section(gpu, 1350 + i, 16, m, n_pol)
        xs = _unpacked(rd, 16, n_pol)
        ref_s = twin.execute(xs, stateful=True)
        st, n_out, h, off, _ = _call(plan, gpu, out_nbit, scale, x=xs, stateful=True, offset=offset)
        assert (st, n_out) == (0, int(ref_s.shape[1])), (i, st, n_out)
        assert plan.last_dada_output() == "staged"
        assert np.array_equal(_written(h, off, n_out * _row_bytes(plan, out_nbit), name),
                              _pack_pair(ref_s, out_nbit, scale)), i
        assert plan.buffered_samples == twin.buffered_samples
    plan.execute(x)
    assert plan.last_dada_output() == "none"


# ------------------------------------------------------------------ 5. stream sequences
def _sequence(gpu, kind, nbit, n_pol, sizes, modes):
    """`sizes` samples call by call through one plan in `modes` ("to_dada": cf32 in, DADA out;
    "dada_to_dada"; "cf32": pfb_filterbank_execute; "dada_in": pfb_filterbank_execute_dada)
    against the cf32 stream of a twin packed call by call."""
    plan, twin = _plan(kind, n_pol), _plan(kind, n_pol)
    seen = dict(empty=False, ragged=False, trimmed=False)
    got_all, ref_all = [], []
    for i, (n, mode) in enumerate(zip(sizes, modes)):
        _, rawd = _section(gpu, 1400 + i, nbit, n, n_pol)
        x = _unpacked(rawd, nbit, n_pol)
        # the rows computed before the nu-trim (a LowCBF plan: with its pending pre-padding)
        total = twin.buffered_samples + n
        k_full = twin.output_length(total)
        ref = twin.execute(x, stateful=True)
        t_out = int(ref.shape[1])
        seen["empty"] |= i == 0 and t_out == 0
        seen["ragged"] |= t_out % 16 != 0
        seen["trimmed"] |= k_full > t_out
        scale = 0.0123 if nbit != 32 else 0.37
        ref_b = _pack_pair(ref, nbit, scale)
        assert plan.stream_rows(n) == t_out, i
        if mode == "cf32":
            got_b = _pack_pair(plan.execute(x, stateful=True), nbit, scale)
            assert plan.last_dada_output() == "none"
        elif mode == "dada_in":
            got_b = _pack_pair(plan.execute_dada(rawd, nbit, stateful=True), nbit, scale)
            assert plan.last_dada_output() == "none"
        else:
            kw = dict(x=x) if mode == "to_dada" else dict(rawd=rawd, in_nbit=nbit)
            st, n_out, h, off, _ = _call(plan, gpu, nbit, scale, stateful=True, **kw)
            assert (st, n_out) == (0, t_out), (i, mode, st, n_out)
            got_b = _written(h, off, t_out * _row_bytes(plan, nbit), f"call {i}")
            assert plan.last_dada_output() == "fused"
        assert np.array_equal(got_b, ref_b), (i, mode)
        assert plan.buffered_samples == twin.buffered_samples, (i, mode)
        got_all.append(got_b)
        ref_all.append(ref_b)
    assert np.array_equal(np.concatenate(got_all), np.concatenate(ref_all))
    assert sum(b.size for b in ref_all) > 64 * _row_bytes(plan, nbit)
    return seen


# first call: no rows; then 32 + 8 rows (not a multiple of 16); calls whose K is no multiple of nu
SIZES = (1500, 12000, 100, 7777, 6001)


@pytest.mark.parametrize("shape", sorted(STREAM_SHAPES), ids=str)
def test_stream_sequence_to_dada(gpu, shape):
    nbit = {"c2-p13": 16, "c2-p12": 8, "4over3-p13": 32, "4over3-p12": 16, "lowcbf": 16}[shape]
    seen = _sequence(gpu, STREAM_SHAPES[shape], nbit, 2, SIZES, ("to_dada",) * len(SIZES))
    assert seen == dict(empty=True, ragged=True, trimmed=True), seen


@pytest.mark.parametrize("shape", ["c2-p13", "lowcbf"], ids=str)
def test_stream_sequence_alternating_outputs_and_inputs(gpu, shape):
    modes = ("to_dada", "cf32", "dada_to_dada", "dada_in", "to_dada")
    _sequence(gpu, STREAM_SHAPES[shape], 16, 2, SIZES, modes)


# ------------------------------------------------------------------ 6. rejections
@pytest.mark.parametrize("kind", [C2, "lowcbf"], ids=["c2", "lowcbf"])
@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "stream"])
def test_rejections_leave_output_and_state_alone(gpu, kind, stateful):
    from ska_pst_dsp_model_amd import _lib
    nbit, n_pol = 16, 2
    plan, twin = _plan(kind, n_pol), _plan(kind, n_pol)
    if stateful and kind != "lowcbf":
        # something buffered (a LowCBF plan stays fresh: its first call is what a retry must equal)
        _, r0 = _section(gpu, 1500, nbit, 6000, n_pol)
        for p in (plan, twin):
            p.execute(_unpacked(r0, nbit, n_pol), stateful=True)
        assert plan.buffered_samples > 0
    buffered = plan.buffered_samples
    n = 9001
    _, rawd = _section(gpu, 1501, nbit, n, n_pol)
    x = _unpacked(rawd, nbit, n_pol)
    rows = plan.stream_rows(n) if stateful else plan.output_length(n)
    assert rows > 16
    need = rows * _row_bytes(plan, nbit)
    E, S = _lib.PFB_ERR_INVALID_ARG, _lib.PFB_ERR_BUFFER_TOO_SMALL
    for kw in (dict(x=x), dict(rawd=rawd, in_nbit=nbit)):
        st, n_out, h, off, _ = _call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need - 1, **kw)
        assert (st, n_out) == (S, rows)
        assert (h == PAT).all(), "a call with too small a capacity wrote output"
        for bad in (dict(out_nbit=12), dict(scale=float("nan")), dict(scale=float("inf")), dict(null_out=True)):
            args = dict(out_nbit=nbit, scale=0.01, stateful=stateful, cap_bytes=need)
            args.update(bad)
            args.update(kw)
            st, n_out, h, off, _ = _call(plan, gpu, args.pop("out_nbit"), args.pop("scale"), **args)
            assert st == E, bad
            assert (h == PAT).all(), bad
        # an `out` not aligned to one value
        st, n_out, h, off, _ = _call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need, offset=1, **kw)
        assert st == E and (h == PAT).all()
        assert plan.buffered_samples == buffered
        assert (plan.stream_rows(n) if stateful else plan.output_length(n)) == rows
    # the corrected retry: what the twin, which saw no rejected call, returns (a LowCBF plan:
    # exactly a first call's rows, the pre-padding still pending)
    ref = twin.execute(x, stateful=stateful)
    assert ref.shape[1] == rows
    st, n_out, h, off, _ = _call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need, x=x)
    assert (st, n_out) == (0, rows)
    assert np.array_equal(_written(h, off, need), _pack_pair(ref, nbit, 0.01))
    assert plan.buffered_samples == twin.buffered_samples


# ------------------------------------------------------------------ 7. oracle
ORACLE_CASES = [("c2-1pol", C2, 1, 53), ("4over3-2pol", F43, 2, 37), ("lowcbf-2pol", "lowcbf", 2, 41)]


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(raw section NBIT 16, float64 oracle product (n_pol, chan, K)) of an ORACLE_CASES entry."""
    _, kind, n_pol, rows = next(c for c in ORACLE_CASES if c[0] == name)
    raw = _file_samples(np.random.default_rng(1600 + len(name)), 16, _n_dat(kind, rows, 17) * n_pol * 2)
    x = orc.reshape_dada_data(raw, 2, n_pol, 1)
    if kind == "lowcbf":
        y = orc.polyphase_analysis_lowcbf(x, _pst_taps(), do_padding=True)
    else:
        y = orc.polyphase_analysis(x, _taps(*kind[:4]), kind[0], kind[1], round_like_matlab=False)
    assert y.dtype == np.complex128 and y.shape[2] == rows
    y.setflags(write=False)
    raw.setflags(write=False)
    return raw, y


@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["nbit8", "nbit16", "nbit32"])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: c[0])
def test_fused_matches_oracle(gpu, case, nbit):
    import torch
    name, kind, n_pol, rows = case
    raw, y = _oracle(name)
    rawd = torch.from_numpy(raw.view(np.uint8).copy()).to(gpu)
    rms = float(np.sqrt(np.mean(np.abs(y) ** 2)))
    # rms of the magnitudes near a third of the range, and not a power of two
    scale = float(np.float32((np.iinfo(orc._NBIT_NP[nbit]).max if nbit != 32 else 1.11) / 3.0 / rms))
    assert np.frexp(scale)[0] != 0.5
    plan = _plan(kind, n_pol)
    got = plan.execute_to_dada(_unpacked(rawd, 16, n_pol), nbit, scale=scale)
    assert plan.last_dada_output() == "fused" and tuple(got.shape) == (rows, plan.out_chan, n_pol, 2)
    sy = np.float64(np.float32(scale)) * y                                     # (n_pol, chan, K)
    expect = orc.write_dada_data(sy, nbit).reshape(rows, plan.out_chan, n_pol, 2)
    q = got.cpu().numpy().astype(np.float64)
    if nbit == 32:
        e = expect.astype(np.float64)
        assert_pfb_close(q[..., 0] + 1j * q[..., 1], e[..., 0] + 1j * e[..., 1], what=f"to-DADA {name}")
        return
    info = np.iinfo(orc._NBIT_NP[nbit])
    t = sy.transpose(2, 1, 0)                                                  # (K, chan, n_pol)
    delta = PARITY_TOL * (np.sqrt(np.mean(np.abs(sy) ** 2)) + np.abs(t))      # assert_pfb_close's allowance
    worst = 0.0
    for comp, part in ((0, t.real), (1, t.imag)):
        err = np.abs(q[..., comp] - np.clip(part, info.min, info.max))
        worst = max(worst, float((err - delta).max()))
        assert (err <= 0.5 + delta).all(), (name, nbit, comp, float((err - delta).max()))
    # (the oracle's own quantisation can differ only where scale y lies within delta of a tie)
    print(f"{name} nbit {nbit}: max (|q - clip(scale y)| - delta) = {worst:.6f} (bound 0.5); "
          f"{float((expect.astype(np.float64) != q).mean()):.2e} of the samples differ from write_dada_data")


# ------------------------------------------------------------------ 8. Python surface
def _fb_cfg(**kw):
    cfg = dict(analysis_function=BUNTON, filt_coeff=_taps(256, "8/7", 12), channels=256, os_factor="8/7")
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("rnd", [False, True], ids=["plain", "rndOutput"])
def test_filterbank_object_execute_to_dada(gpu, rnd):
    """FilterBank.execute_to_dada over three calls == execute followed by layout.dada_pack; with
    rndOutput it is that fallback (the quantiser needs the variance of the whole output)."""
    from ska_pst_dsp_model_amd import layout
    pfb = _pfb()
    cfg = _fb_cfg(rndOutput=rnd, rmsOutput=20.0 if rnd else 0.0)
    fb, ref_fb = pfb.FilterBank(cfg), pfb.FilterBank(cfg)
    for i, n in enumerate((9000, 100, 7777)):
        _, rawd = _section(gpu, 1700 + i, 16, n, 2)
        x = _unpacked(rawd, 16, 2)
        _, sec = fb.execute_to_dada(x, 8, scale=1.0 if rnd else 0.0123)
        _, view = ref_fb.execute(x)
        buf = view.transpose(1, 2).contiguous()
        expect = _pack_pair(buf, 8, 1.0 if rnd else 0.0123)
        if rnd:
            assert np.array_equal(expect, layout.dada_pack(buf, 8).cpu().numpy().view(np.uint8))
        assert tuple(sec.shape) == (buf.shape[1], 256, 2, 2) and str(sec.dtype) == "torch.int8"
        assert np.array_equal(sec.cpu().numpy().view(np.uint8).ravel(), expect), i
        assert fb.buffered_samples == ref_fb.buffered_samples
        assert fb._plan.last_dada_output() == ("none" if rnd else "fused")
    _, rawd = _section(gpu, 1710, 16, 9000, 2)
    _, sec = fb.execute_dada_to_dada(rawd, 16, 16, scale=0.01, n_pol=2)
    _, view = ref_fb.execute_dada(rawd, 16, n_pol=2)
    assert np.array_equal(sec.cpu().numpy().view(np.uint8).ravel(),
                          _pack_pair(view.transpose(1, 2).contiguous(), 16, 0.01))


def test_harness_channelize_writes_the_section_itself(gpu, tmp_path):
    """harness.channelize of a two-pol NBIT-16 single-channel file == write_dada_file of
    execute_dada's product, byte for byte."""
    pfb = _pfb()
    taps = _taps(256, "8/7", 12)
    fir = tmp_path / "fir.npy"
    pfb.firio.save_fir_filter_coeff(str(fir), taps)
    rng = np.random.default_rng(1800)
    n = _n_dat(C2, 37, 11)
    x = 3000.0 * (rng.standard_normal((2, 1, n)) + 1j * rng.standard_normal((2, 1, n)))
    src = tmp_path / "series16.dump"
    pfb.dada.write_dada_file(src, x.astype(np.complex64), {"HDR_SIZE": "4096", "TSAMP": "1.0"}, nbit=16)
    f = pfb.harness.channelize(str(src), 256, "8/7", str(fir), output_file_name="chan.dump",
                               output_dir=str(tmp_path))
    plan = pfb.core.analysis_plan(pfb.read_fir_filter_coeff(str(fir)), 256, "8/7", BUNTON, 2)
    assert plan.last_dada_input() == "fused" and plan.last_dada_output() == "fused"
    raw, hdr = pfb.dada.read_dada_raw(src)
    ref = _plan(C2, 2).execute_dada(raw, 16).transpose(1, 2)                    # (n_pol, chan, K)
    assert tuple(ref.shape) == (2, 256, 37) and float(ref.abs().max()) > 0
    with open(f.file_path, "rb") as fh:
        got_hdr = pfb.dada.read_header(fh)
    ch = dict(hdr)
    for k in ("TSAMP", "PFB_DC_CHAN", "NCHAN_PFB_0", "OS_FACTOR"):
        ch[k] = got_hdr[k]
    pfb.dada.add_fir_filter_to_header(ch, taps, pfb.config.as_rational("8/7"))
    expect = tmp_path / "expect.dump"
    pfb.dada.write_dada_file(expect, ref, ch)
    with open(f.file_path, "rb") as a, open(expect, "rb") as b:
        assert a.read() == b.read()


@pytest.mark.parametrize("nbit", [8, 32], ids=["nbit8", "nbit32"])
def test_dadawrite_write_section_round_trips(gpu, tmp_path, nbit):
    pfb = _pfb()
    _, rawd = _section(gpu, 1900, 16, _n_dat(C2, 21, 3), 2)
    plan = _plan(C2, 2)
    secs = [plan.execute_dada_to_dada(rawd, 16, nbit, scale=0.0123, stateful=True) for _ in range(2)]
    path = tmp_path / "out.dump"
    w = pfb.dada.DADAWrite(str(path), {"HDR_SIZE": "4096", "TSAMP": "1.0"}, nbit=nbit)
    for s in secs:
        w.write_section(s)
    w.close()
    data, hdr = pfb.dada.read_dada_file(path)                                   # (n_pol, chan, n_dat)
    assert (hdr["NBIT"], hdr["NPOL"], hdr["NCHAN"], hdr["NDIM"]) == (str(nbit), "2", "256", "2")
    import torch
    allsec = torch.cat(secs).to(torch.float32)                                  # (T, chan, n_pol, 2)
    expect = torch.view_as_complex(allsec.contiguous()).permute(2, 1, 0)
    assert tuple(data.shape) == tuple(expect.shape) and data.shape[2] > 16
    assert torch.equal(data, expect)
    with pytest.raises(ValueError):
        w.write_section(secs[0].to(torch.float64))
    one = tmp_path / "one.dump"
    pfb.dada.write_dada_section_file(one, secs[0], {"HDR_SIZE": "4096", "TSAMP": "1.0"})
    d1, h1 = pfb.dada.read_dada_file(one)
    assert h1["NBIT"] == str(nbit) and torch.equal(d1, expect[:, :, :secs[0].shape[0]])
