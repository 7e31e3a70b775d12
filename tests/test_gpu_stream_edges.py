"""Stream objects at the boundaries of their carry paths (filterbank_exec and ifb_go,
ska-pst-dsp-model_amd/csrc/pfb_api_analysis.hip and pfb_api_synthesis.hip), through every entry point of the C ABI.

tests/stream_model.py restates the two host state machines in integers and holds the call
sequences; tests/test_stream_model.py proves on the CPU that each sequence sits on the edges
it claims (input_idat == carry, a one-sample call that completes nu rows out of a maximal
carry, carries shorter than P N or no multiple of N read through `pre`, zero-length calls, an
empty new carry, the synthesis carry rounded up to a multiple of nu with a shortened output,
the rejected call).  Here every sequence runs on the GPU:

  * the plan under test takes call i through entry rotation[i % len]; every cyclic shift of the
    entry list is a case, so each call meets each entry;
  * a twin plan of the same configuration always takes the packed device call;
  * after every call: same shape, bit-identical values (after undoing a strided layout), same
    buffered count, rows / output length and buffered count equal to the model, the
    last_dada_input / last_strided_input value include/pfb_api.h specifies, and for the analysis
    one class-0 profiler record for a call that returns rows and none for one that does not, for the
    synthesis the class-1 and class-2 records of the model's chunks (stream_model.synthesis_launches);
  * every chunk against the float64 oracle stream object at conftest.PARITY_TOL, and a Bunton
    stream against one pfb_analysis_execute of the whole series, bit for bit.

All samples are integers: one seeded section of the file's type per sequence (TFP order, two
polarisations interleaved, the type's full range), unpacked once on the host, so the same
samples go through the cf32, strided, host and DADA entries.  The oracle products are computed
once per sequence and shared by its rotations.
"""
import functools
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest

import stream_model as sm
from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

N_POL = 2
NAN = complex(float("nan"), float("nan"))
SENTINEL = complex(-7.0, 7.0)


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _stream(dev):
    import torch
    return c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _Launches:
    def __init__(self, lib):
        self.lib = lib

    def reset(self):
        assert self.lib.pfb_profile_reset() == 0

    def records(self, which):
        n = c_int64()
        assert self.lib.pfb_profile_read(which, None, byref(n), None) == 0
        return n.value


@pytest.fixture
def launches(gpu):
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    assert lib.pfb_profile_reset() == 0 and lib.pfb_profile_enable(1) == 0
    try:
        yield _Launches(lib)
    finally:
        lib.pfb_profile_enable(0)
        lib.pfb_profile_reset()


# ----------------------------------------------------------------------------- taps and data
@functools.lru_cache(maxsize=None)
def _firls(N, os_, tpc):
    """design_PFB_FIR_filter (N tpc + 1 taps; the 3073-tap designs take a second each)."""
    taps = _pfb().design_PFB_FIR_filter(N, os_, tpc)
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def _pst_taps():
    pfb = _pfb()
    taps = pfb.read_fir_filter_coeff(pfb.config.config_dir + "/PST_filtertaps.txt")
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def _file_values(seed, nbit, *shape):
    """Seeded samples over the full range of the file's integer type, read-only."""
    t = orc._NBIT_NP[nbit]
    info = np.iinfo(t)
    raw = np.random.default_rng(seed).integers(info.min, info.max + 1, size=shape).astype(t)
    raw.setflags(write=False)
    return raw


def _bytes(gpu, arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(gpu)


def _n_calls(chunks):
    return sum(1 for n in chunks if n != "reset")


def _segments(chunks):
    """[(first call index, [chunk lengths])] between resets."""
    segs, cur, i = [], [], 0
    for n in chunks:
        if n == "reset":
            segs.append((i - len(cur), cur))
            cur = []
        else:
            cur.append(n)
            i += 1
    segs.append((i - len(cur), cur))
    return segs


# ============================================================================ analysis
# key -> (model shape, chunks, variant, os, taps, nbit, entries)
BUNTON_ENTRIES = ("packed", "host", "strided_rows", "strided_cm", "dada16", "dada64")
LOWCBF_ENTRIES = ("packed", "host", "dada8")
PADDED_ENTRIES = ("packed", "packed_tight", "host", "strided_chomp")
MODEL_ENTRY = {"packed": "packed", "packed_tight": "packed", "host": "host", "strided_rows": "strided",
               "strided_cm": "strided", "strided_chomp": "strided", "dada16": "dada_fused",
               "dada8": "dada_fused", "dada64": "dada_staged"}
BUNTON_GPU_SHAPES = ("8over7-p13", "4over3-p13", "8over7-p12")


@functools.lru_cache(maxsize=None)
def _analysis_case(key):
    kind = key[0]
    if kind == "bunton":
        _, name, table = key
        shape = sm.STREAM_SHAPES[name]
        os_ = f"{shape.nu}/{shape.de}"
        taps = _firls(256, os_, 12)
        if shape.P == 12:
            taps = taps[:3072].copy()          # 12 phases
            taps.setflags(write=False)
        chunks = sm.bunton_main_chunks(shape) if table == "main" else sm.BUNTON_SHORT_CHUNKS
        return shape, chunks, "polyphase_analysis", os_, taps, 16, BUNTON_ENTRIES
    if kind == "lowcbf":
        return (sm.LOWCBF_SHAPE, sm.LOWCBF_CHUNKS, "polyphase_analysis_lowcbf", "4/3", _pst_taps(), 8,
                LOWCBF_ENTRIES)
    if kind == "padded-fused":
        return (sm.PADDED_FUSED_SHAPE, sm.PADDED_FUSED_CHUNKS, "polyphase_analysis_padded", "8/7",
                _firls(16, "8/7", 10), 16, PADDED_ENTRIES)
    assert kind == "padded-generic"
    taps = np.random.default_rng(505).standard_normal(33 * 64) / 16.0  # test_generic_n64_many_phases
    taps.setflags(write=False)
    return (sm.PADDED_GENERIC_SHAPE, sm.PADDED_GENERIC_CHUNKS, "polyphase_analysis_padded", "4/3", taps, 16,
            PADDED_ENTRIES)


def _analysis_samples(key):
    """(raw (n, n_pol, 2) file values, x (n_pol, n) complex64) of the whole sequence."""
    shape, chunks, *_rest, nbit, _ = _analysis_case(key)
    n = sum(c for c in chunks if c != "reset")
    raw = _file_values(1000 + sum(map(ord, "".join(map(str, key)))), nbit, n, N_POL, 2)
    x = (raw[:, :, 0].astype(np.float32) + 1j * raw[:, :, 1].astype(np.float32)).astype(np.complex64).T
    return raw, np.ascontiguousarray(x)


@functools.lru_cache(maxsize=None)
def _analysis_oracle(key):
    """The oracle stream object's product per call, (n_pol, C, rows) float64, read-only."""
    shape, chunks, variant, os_, taps, _, _ = _analysis_case(key)
    assert shape.P == -(-len(taps) // shape.N)
    _, x = _analysis_samples(key)
    out, a = [], 0
    ofb = orc.FilterBankOracle(taps, shape.N, os_, variant)
    for n in chunks:
        if n == "reset":
            ofb = orc.FilterBankOracle(taps, shape.N, os_, variant)
            continue
        y = ofb.execute(x[:, None, a:a + n])
        y.setflags(write=False)
        out.append((y, int(ofb.buffered_samples)))
        a += n
    return tuple(out)


def _chomp_keep(N, nu, de):
    """(sel, kept bins) of the cascade chomp (TwoStageFilterBank.m:102-105)."""
    nsel = N * de // nu
    split, shift = nsel // 2 - 1, N - nsel
    c = np.arange(N)
    j = np.where(c < split, c, c - shift)
    keep = ((c < split) | (c >= split + shift)) & (j < nsel)
    return (split, shift, nsel), c[keep]


def _analysis_call(gpu, plan, entry, xh, raw, T, shape):
    """One stream call of the plan through `entry` -> ((n_pol, T, bins) ndarray, kept bins or None)."""
    import torch
    n = xh.shape[1]
    C = plan.out_chan
    if entry == "host":
        return np.asarray(plan.execute(xh, stateful=True)), None
    if entry in ("dada16", "dada8"):
        return plan.execute_dada(_bytes(gpu, raw), int(entry[4:]), stateful=True).cpu().numpy(), None
    if entry == "dada64":  # NBIT 64: no fused loader, unpacked behind the carry
        return plan.execute_dada(_bytes(gpu, raw.astype(np.float64)), 64, stateful=True).cpu().numpy(), None
    xd = torch.from_numpy(xh).to(gpu)
    if entry == "packed":
        return plan.execute(xd, stateful=True).cpu().numpy(), None
    if entry == "packed_tight":
        # capacity and pol stride for the T_out returned rows only: a padded call's rows
        # [T_out, K) have no room in `out` and go through the staging buffer
        out = torch.full((N_POL, max(T, 1) * C), NAN, dtype=torch.complex64, device=gpu)
        n_out = c_int64(-1)
        st = plan._lib.pfb_filterbank_execute(plan._h, c_void_p(xd.data_ptr()), n, n, c_void_p(out.data_ptr()),
                                              max(T, 1) * C, T, byref(n_out), 0, _stream(gpu))
        assert st == 0 and n_out.value == T, plan._lib.pfb_last_error()
        return out[:, :T * C].reshape(N_POL, T, C).cpu().numpy(), None
    if entry == "strided_rows":  # the packed layout, spelt as strides
        out = torch.full((N_POL, max(T, 1), C), NAN, dtype=torch.complex64, device=gpu)
        assert plan.execute_strided(xd, out, max(T, 1) * C, C, 1) == T
        return out[:, :T].cpu().numpy(), None
    if entry == "strided_cm":  # channel-major: a cascade's stage-1 product
        Tc = max(16, (T + 15) // 16 * 16)
        out = torch.full((N_POL, C, Tc), NAN, dtype=torch.complex64, device=gpu)
        assert plan.execute_strided(xd, out, C * Tc, 1, Tc) == T
        got = out.cpu().numpy()
        assert np.isnan(got[:, :, T:]).all(), "a column past the returned rows was written"
        return np.ascontiguousarray(got[:, :, :T].transpose(0, 2, 1)), None
    assert entry == "strided_chomp"  # assembled and chomped: a cascade's stage-2 product
    sel, kept = _chomp_keep(shape.N, shape.nu, shape.de)
    out = torch.full((max(T, 1), N_POL, sel[2]), NAN, dtype=torch.complex64, device=gpu)
    assert plan.execute_strided(xd, out, sel[2], N_POL * sel[2], 1, sel) == T
    got = out.cpu().numpy()
    assert np.isnan(got[T:]).all(), "a row past the returned ones was written"
    return np.ascontiguousarray(got[:T].transpose(1, 0, 2)), kept


def _drive_analysis(gpu, launches, key, rot):
    import torch
    pfb = _pfb()
    shape, chunks, variant, os_, taps, nbit, entries = _analysis_case(key)
    rotation = sm.rotations(entries)[rot]
    raw, x = _analysis_samples(key)
    oracle = _analysis_oracle(key)
    plan = pfb.AnalysisPlan(taps, shape.N, os_, variant, N_POL)
    twin = pfb.AnalysisPlan(taps, shape.N, os_, variant, N_POL)
    B, pad_due, a, i = 0, shape.variant == sm.LOWCBF, 0, 0
    produced, seen_paths = [], []
    for n in chunks:
        if n == "reset":
            plan.reset()
            twin.reset()
            B, pad_due = 0, shape.variant == sm.LOWCBF
            assert plan.buffered_samples == twin.buffered_samples == 0
            continue
        entry = rotation[i % len(rotation)]
        w = f"{key} call {i} ({n} samples, carry {B}) via {entry}"
        rec, pad_due = sm.analysis_call(shape, B, n, MODEL_ENTRY[entry], pad_due)
        xh, rw = x[:, a:a + n], raw[a:a + n]
        assert plan.stream_rows(n) == twin.stream_rows(n) == rec.rows, w
        launches.reset()
        got, kept = _analysis_call(gpu, plan, entry, np.ascontiguousarray(xh), rw, rec.rows, shape)
        torch.cuda.synchronize(gpu)
        n_launch = launches.records(0)
        diag = plan.last_dada_input()
        ref = twin.execute(torch.from_numpy(np.ascontiguousarray(xh)).to(gpu), stateful=True).cpu().numpy()
        assert twin.last_dada_input() == "none", w
        assert ref.shape == (N_POL, rec.rows, plan.out_chan), (w, ref.shape)
        want = ref if kept is None else ref[:, :, kept]
        assert got.shape == want.shape, (w, got.shape, want.shape)
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), w
        assert plan.buffered_samples == twin.buffered_samples == rec.carry_after, (
            w, plan.buffered_samples, twin.buffered_samples, rec.carry_after)
        assert diag == sm.analysis_dada_diag(rec), (w, diag, rec.path)
        assert n_launch == sm.analysis_class0_launches(rec), (w, n_launch, rec.path)
        oref, obuf = oracle[i]
        assert obuf == rec.carry_after, (w, obuf)
        oref = oref if kept is None else oref[:, kept, :]
        assert oref.shape == (N_POL, got.shape[2], rec.rows), (w, oref.shape)
        if rec.rows:
            assert np.abs(ref).max() > 0, w
            assert_pfb_close(got.transpose(0, 2, 1), oref, what=w)
        produced.append(ref)
        seen_paths.append(rec.path)
        B, a, i = rec.carry_after, a + n, i + 1
    assert i == _n_calls(chunks) == len(oracle)
    print(key, rotation, seen_paths)
    if shape.variant == sm.BUNTON:
        # the stream of each segment equals one pfb_analysis_execute of its whole series
        for first, seg in _segments(chunks):
            lo = sum([c for c in chunks if c != "reset"][:first])
            whole = twin.execute(torch.from_numpy(np.ascontiguousarray(x[:, lo:lo + sum(seg)])).to(gpu)).cpu().numpy()
            streamed = np.concatenate(produced[first:first + len(seg)], axis=1)
            assert streamed.shape[1] > 0 and streamed.shape[1] <= whole.shape[1]
            assert np.array_equal(streamed, whole[:, :streamed.shape[1]]), (key, first)
    return seen_paths


@pytest.mark.parametrize("rot", range(len(BUNTON_ENTRIES)))
@pytest.mark.parametrize("table", ["main", "short"])
@pytest.mark.parametrize("name", BUNTON_GPU_SHAPES)
def test_bunton_stream_edges(gpu, launches, name, table, rot):
    """Sequence 1: the N 256 streaming kernel (13 and 12 phases, 8/7 and 4/3).  main: carry
    3584 (its 4/3 and 12-phase counterparts) then P N samples (input_idat == carry), a maximal
    carry completed by one sample, a zero-length call, a carry of P N + 1.  short: `pre` holding
    1, 255 and 257 samples.  Entries: packed, host, the packed layout through execute_strided,
    channel-major, DADA NBIT 16 (fused) and NBIT 64 (staged)."""
    _drive_analysis(gpu, launches, ("bunton", name, table), rot)


@pytest.mark.parametrize("rot", range(len(LOWCBF_ENTRIES)))
def test_lowcbf_stream_edges(gpu, launches, rot):
    """Sequence 2: LowCBF with the PST taps: a 1000-sample first call (no rows, the pre-pad
    consumed), the carry on 3072 exactly and on its maximum 3839, a one-sample completing call,
    input_idat == carry, reset() with the pad due again.  Entries: packed, host, DADA NBIT 8."""
    _drive_analysis(gpu, launches, ("lowcbf",), rot)


@pytest.mark.parametrize("rot", range(len(PADDED_ENTRIES)))
@pytest.mark.parametrize("kind", ["padded-fused", "padded-generic"])
def test_padded_stream_edges(gpu, launches, kind, rot):
    """Sequences 3 and 4: polyphase_analysis_padded on the fused kernel (N 16, 8/7: the carry
    read through `pre`) and on the FIR + row-FFT path (N 64, 33 phases: always concatenated):
    an empty new carry, carries 1 and nu M - 1, one sample completing nu rows, a chunk shorter
    than M, a zero-length call.  Entries: packed with room for K rows, packed with capacity
    for the T_out returned rows only (staging), host, execute_strided with the cascade chomp."""
    _drive_analysis(gpu, launches, (kind,), rot)


# ============================================================================ synthesis
SYNTH_ENTRIES = ("packed", "host", "strided_pols", "strided_cm", "dada_tfp", "dada_lowcbf")
SYNTH_MODEL_ENTRY = {"packed": "packed", "host": "host", "strided_pols": "strided", "strided_cm": "strided",
                     "dada_tfp": "dada", "dada_lowcbf": "dada"}


@functools.lru_cache(maxsize=None)
def _synth_case(kind, so):
    """(model shape, rows per call, taper, deripple, taps, the entry reads in place)."""
    if kind == "c2":
        return sm.C2_SYNTH[so], sm.C2_SYNTH_ROWS[so], "tukey", True, _firls(256, "8/7", 12), True
    # Nf 128 block kernel; a Hann temporal taper is a per-channel gain of the channel IFFT's
    # loader, which the strided and DADA loaders do not have: those entries are staged whole
    return sm.SMALL_SYNTH[so], sm.SMALL_SYNTH_ROWS[so], "hann", False, _firls(8, "8/7", 10), False


def _synth_samples(kind, so):
    """(raw (rows, N, n_pol, 2) int16 TFP file values, x (n_pol, rows, N) complex64)."""
    shape, rows, *_ = _synth_case(kind, so)
    raw = _file_values(2000 + shape.N + so, 16, sum(rows), shape.N, N_POL, 2)
    x = (raw[..., 0].astype(np.float32) + 1j * raw[..., 1].astype(np.float32)).astype(np.complex64)
    return raw, np.ascontiguousarray(x.transpose(2, 0, 1))


@functools.lru_cache(maxsize=None)
def _synth_oracle(kind, so):
    """Per call: (product (n_pol, 1, olen), buffered rows), or None where the oracle rejects."""
    shape, rows, taper, deripple, taps, _ = _synth_case(kind, so)
    _, x = _synth_samples(kind, so)
    o = orc.InverseFilterBankOracle(taps, shape.N, f"{shape.nu}/{shape.de}", shape.Nf, shape.Ov, taper,
                                    deripple=deripple, sample_offset=so, honour_deripple=True)
    out, a = [], 0
    for n in rows:
        try:
            y = o.execute(x[:, a:a + n].transpose(0, 2, 1))
            y.setflags(write=False)
            out.append((y, int(o.buffered_samples)))
        except ValueError:
            out.append(None)
        a += n
    return tuple(out)


def _synth_plan(kind, so):
    pfb = _pfb()
    shape, _, taper, deripple, taps, _ = _synth_case(kind, so)
    plan = pfb.SynthesisPlan(shape.N, f"{shape.nu}/{shape.de}", shape.Nf, shape.Ov, True, 1, deripple,
                             taps if deripple else None, pfb.PFBWindow().lookup[taper](shape.Nf, shape.Ov),
                             None, N_POL)
    plan.set_stream_sample_offset(so)
    return plan


def _lowcbf_order(raw):
    """TFP file values (rows, N, n_pol, 2) -> the same samples in LowCBF order: heaps of 32
    rows, [heap][chan][pol][row in heap] (reshape_low_cbf_data.m:14-43)."""
    rows, N, P, _ = raw.shape
    return np.ascontiguousarray(raw.reshape(rows // 32, 32, N, P, 2).transpose(0, 2, 3, 1, 4))


def _synth_call(gpu, plan, entry, xh, raw, out):
    """One stream call through `entry`; `out`: a device buffer to write into (device entries)."""
    import torch
    n_pol, n, N = xh.shape
    if entry == "host":
        return np.asarray(plan.execute(xh, stateful=True, layout="ptc"))
    if entry == "packed":
        return plan.execute(torch.from_numpy(xh).to(gpu), stateful=True, layout="ptc", out=out).cpu().numpy()
    if entry == "dada_tfp" or (entry == "dada_lowcbf" and (n == 0 or n % 32)):
        return plan.execute_dada(_bytes(gpu, raw), 16, stateful=True, out=out).cpu().numpy()
    if entry == "dada_lowcbf":
        return plan.execute_dada(_bytes(gpu, _lowcbf_order(raw)), 16, lowcbf=True, stateful=True,
                                 out=out).cpu().numpy()
    if entry == "strided_pols":  # pols interleaved in every row, one spare channel
        strides, lead = (N, n_pol * N + 1, 1), 3
    else:                        # channel-major rows
        assert entry == "strided_cm"
        cs = n + 5
        strides, lead = (N * cs, 1, cs), 3
    need = (n_pol - 1) * strides[0] + max(n - 1, 0) * strides[1] + (N - 1) * strides[2] + 1
    host = np.full(lead + need + 5, NAN, dtype=np.complex64)
    np.lib.stride_tricks.as_strided(host[lead:], xh.shape, tuple(8 * s for s in strides))[...] = xh
    assert np.isnan(host).sum() == host.size - xh.size, "the strides overlap"
    dev = torch.from_numpy(host).to(gpu)
    view = torch.as_strided(dev, xh.shape, strides, lead)
    got = plan.execute_view(view, stateful=True, out=out).cpu().numpy()
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), host.view(np.uint64)), "the input changed"
    return got


def _drive_synthesis(gpu, launches, kind, so, rot, chunk_blocks=0):
    import torch
    pfb = _pfb()
    shape, rows, _, _, _, in_place = _synth_case(kind, so)
    rotation = sm.rotations(SYNTH_ENTRIES)[rot]
    raw, x = _synth_samples(kind, so)
    oracle = _synth_oracle(kind, so)
    plan, twin = _synth_plan(kind, so), _synth_plan(kind, so)
    if chunk_blocks:
        plan.set_chunk_blocks(chunk_blocks)
        twin.set_chunk_blocks(chunk_blocks)
    assert (plan.input_keep, plan.output_keep) == (shape.keep, shape.Lkeep)
    Bc, a, rejected, paths = 0, 0, 0, []
    for i, n in enumerate(rows):
        entry = rotation[i % len(rotation)]
        w = f"{kind} offset {so} call {i} ({n} rows, carry {Bc}) via {entry}"
        rec = sm.synthesis_call(shape, Bc, n, SYNTH_MODEL_ENTRY[entry])
        xh, rw = np.ascontiguousarray(x[:, a:a + n]), raw[a:a + n]
        xd = torch.from_numpy(xh).to(gpu)
        paths.append(rec.path)
        if rec.path == "rejected":
            # no complete block and the carry rounded past the data: every entry rejects the
            # call and leaves the state and the output buffer alone
            rejected += 1
            assert oracle[i] is None, w
            out = torch.full((N_POL, 64), SENTINEL, dtype=torch.complex64, device=gpu)
            launches.reset()
            with pytest.raises(pfb.PfbError) as e:
                _synth_call(gpu, plan, entry, xh, rw, None if entry == "host" else out)
            assert e.value.status == pfb._lib.PFB_ERR_INVALID_ARG, w
            torch.cuda.synchronize(gpu)
            assert (launches.records(1), launches.records(2)) == sm.synthesis_launches(rec) == (0, 0), w
            with pytest.raises(pfb.PfbError):
                twin.execute(xd, stateful=True, layout="ptc", out=out)
            torch.cuda.synchronize(gpu)
            assert bool((out == SENTINEL).all()), w
            assert plan.buffered_samples == twin.buffered_samples == Bc == rec.carry_after, w
            a += n
            continue
        assert plan.output_length(Bc + n) >= rec.rows, w
        launches.reset()
        got = _synth_call(gpu, plan, entry, xh, rw, None)
        torch.cuda.synchronize(gpu)
        n_launch = (launches.records(1), launches.records(2))
        diag = (plan.last_strided_input(), plan.last_dada_input())
        ref = twin.execute(xd, stateful=True, layout="ptc").cpu().numpy()
        assert (twin.last_strided_input(), twin.last_dada_input()) == ("none", "none"), w
        assert ref.shape == (N_POL, rec.rows), (w, ref.shape, rec.rows)
        assert got.shape == ref.shape, (w, got.shape)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), w
        assert plan.buffered_samples == twin.buffered_samples == rec.carry_after, (
            w, plan.buffered_samples, twin.buffered_samples, rec.carry_after)
        assert diag == sm.synthesis_diag(rec, in_place), (w, diag, rec.path)
        assert n_launch == sm.synthesis_launches(rec, chunk_blocks), (w, n_launch, rec.path)
        oref, obuf = oracle[i]
        assert obuf == rec.carry_after and oref.shape == (N_POL, 1, rec.rows), (w, obuf, oref.shape)
        if rec.rows:
            assert np.abs(ref).max() > 0, w
            assert_pfb_close(got[:, None, :], oref, what=w)
        Bc, a = rec.carry_after, a + n
    print(kind, so, rotation, paths)
    assert rejected == sum(1 for o in oracle if o is None) == 1
    return paths


@pytest.mark.parametrize("rot", range(len(SYNTH_ENTRIES)))
@pytest.mark.parametrize("so", [0, 5])
def test_inverse_filterbank_c2_stream_edges(gpu, launches, so, rot):
    """Sequence 5: 256 channels, Nf 256, Ov 48, tukey, deripple, two pols.  Offset 0: carry 160
    then 96 rows (input_idat == carry, every block stitched, the in-place range empty).  Offset
    5: 165 rows (the carry rounded up to a multiple of nu, the output shorter than the blocks',
    inside the split path).  Both: a zero-length call and a 3-row call every entry rejects.
    Entries: packed, host, pols interleaved in the row with a spare channel, channel-major,
    DADA NBIT 16 TFP, DADA LowCBF order (TFP for the chunks that are no multiple of 32)."""
    _drive_synthesis(gpu, launches, "c2", so, rot)


@pytest.mark.parametrize(
    "so, rot, chunk_blocks",
    [pytest.param(so, rot, 0, id=f"{so}-{rot}") for so in (0, 5) for rot in range(len(SYNTH_ENTRIES))]
    + [pytest.param(so, 0, 1, id=f"{so}-0-chunk1") for so in (0, 5)])
def test_inverse_filterbank_small_block_stream_edges(gpu, launches, so, rot, chunk_blocks):
    """Sequence 6: 8 channels, Nf 128, Ov 16 (the small block kernel) with a Hann temporal
    taper: the strided and DADA entries are staged whole (their loaders have no per-channel
    gain) inside the split path; the same recipe at keep = 96.  chunk_blocks 1 (rotation 0, both
    offsets): every block range runs one chunk per block, so the chunks after the first of a
    range read their rows past a moved first row of the source."""
    _drive_synthesis(gpu, launches, "small", so, rot, chunk_blocks)
