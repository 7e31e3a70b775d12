"""The stream contract of include/pfb_api.h ("Streams"): every entry point off the default
stream.

1. Poison and delay (tests/stream_harness.py): every device-memory entry point runs on a fresh
   non-blocking side stream behind a calibrated delay kernel, its input poisoned until a copy on
   that stream fills it, its output a sentinel, its plan warm from other samples.  The result
   must equal the same call made earlier on the idle default stream bit for bit, and the delay
   must still be running when the call returns to the host (else the test proves nothing).
2. Independent plans, stream objects and host threads at once.
3. pfb_quantize across streams (its moments were one block per device), and the quantiser's
   odd shapes against the oracle.
4. One plan on two streams in turn, ordered by the caller with an event.
5. Graph capture of the stateless device entry points of both plan kinds.

The reference of every comparison is the default-stream call, so no oracle run is needed where
another module compares the shape with the oracle; shapes that are new here get one
assert_pfb_close of the default-stream result, and a check of the kernel the host branch
launched (pfb_profile_kernel_name, as tests/test_gpu_dispatch_matrix.py).
"""
import ctypes
import functools
import threading

import numpy as np
import pytest

import stream_harness as sh
from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _lib():
    from ska_pst_dsp_model_amd import _lib
    return _lib


# ----------------------------------------------------------------------------- data
def _noise(gpu, shape, seed, scale=1.0):
    import torch
    rng = np.random.default_rng(seed)
    x = (scale * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)
    return torch.from_numpy(x).to(gpu)


def _ints(gpu, shape, seed, nbit):
    """File samples of NBIT 8 / 16 well inside the type's range (the products stay unsaturated)."""
    import torch
    rng = np.random.default_rng(seed)
    lim = 100 if nbit == 8 else 3000
    raw = rng.integers(-lim, lim + 1, size=shape).astype(np.int8 if nbit == 8 else np.int16)
    return torch.from_numpy(raw).to(gpu)


def _unit_scale(y):
    """A DADA output scale that brings the cf32 product ``y`` to an RMS of 30 units."""
    import torch
    return float(30.0 / torch.view_as_real(y).float().pow(2).mean().sqrt().item())


@functools.lru_cache(maxsize=None)
def _taps(N, os_, tpc):
    """Designed taps; random ones where the host design takes seconds (N tpc > 4096)."""
    if N * tpc > 4096:
        taps = np.random.default_rng(9700 + N + tpc).standard_normal(N * tpc + 1) / N
    else:
        taps = _pfb().design_PFB_FIR_filter(N, os_, tpc)
    taps.setflags(write=False)
    return taps


@functools.lru_cache(maxsize=None)
def _named_taps(kind):
    pfb = _pfb()
    if kind == "pst":
        taps = pfb.read_fir_filter_coeff(pfb.config.config_dir + "/PST_filtertaps.txt")
    elif kind == "mid":
        taps = pfb.design_PFB_FIR_filter_two_stage(4096, "8/7", 28)
    elif kind == "c2":
        taps = pfb.design_PFB_FIR_filter(256, "8/7", 12)
    else:
        raise KeyError(kind)
    taps = np.asarray(taps, dtype=np.float64)
    taps.setflags(write=False)
    return taps


# ----------------------------------------------------------------------------- which kernel ran
class _Launches:
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        assert self.lib.pfb_profile_reset() == 0 and self.lib.pfb_profile_enable(1) == 0
        return self

    def __exit__(self, *exc):
        self.lib.pfb_profile_enable(0)
        self.lib.pfb_profile_reset()

    def name(self, which):
        buf = ctypes.create_string_buffer(1024)
        assert self.lib.pfb_profile_kernel_name(which, buf, len(buf)) == 0
        return buf.value.decode()

    def records(self, which):
        n = ctypes.c_int64()
        assert self.lib.pfb_profile_read(which, None, ctypes.byref(n), None) == 0
        return n.value


def _assert_branch(call, which, expect):
    """``call()`` on the default stream launched the kernel the row names: ``expect`` is a
    piece of the demangled name, or None for a path of several launches (one record, no name)."""
    import torch
    with _Launches(_lib().load()) as l:
        call()
        torch.cuda.synchronize()
        name = l.name(which)
        print(f"class {which}: {name!r}")
        if expect is None:
            assert name == "" and l.records(which) == 1, f"expected one multi-launch record, got {name!r}"
        else:
            assert expect in name, f"ran {name!r}, the row names {expect!r}"


# ============================================================================ 1. poison and delay
# ---------------------------------------------------------------------------- 1a. AnalysisPlan.execute
# id -> (N, os, taps, variant, n_dat, n_pol, kernel piece or None (several launches), oracle run)
ANALYSIS = {
    "generic-n16": (16, "4/3", 6, "polyphase_analysis", 3000, 2, "analysis_fused_kernel<16,", True),
    "stream-n256": (256, "8/7", "c2", "polyphase_analysis", 1 << 16, 1, "analysis_stream_kernel<256,", True),
    "padded-n512-row-fft": (512, "4/3", 12, "polyphase_analysis_padded", 1 << 16, 2, None, True),
    # tests/test_gpu_parity.py test_analysis_4096_persistent_row_fft: more than 2048 rows
    "padded-n4096-persistent-row-fft": (4096, "8/7", "random41", "polyphase_analysis_padded",
                                        2100 * 3584 + 13 * 4096, 1, None, False),
    "lowcbf": (256, "4/3", "pst", "polyphase_analysis_lowcbf", 3072 - 1536 + 41 * 192 + 5, 2,
               "analysis_stream_kernel<256, 12, 4, 3, 0, true", False),
}


def _analysis_taps(N, os_, spec):
    if spec == "random41":
        return np.random.default_rng(41).standard_normal(4096 * 12 + 1) / 64.0
    if isinstance(spec, str):
        return _named_taps(spec)
    return _taps(N, os_, spec)


@pytest.mark.parametrize("case", list(ANALYSIS), ids=list(ANALYSIS))
def test_analysis_execute_on_a_side_stream(gpu, case):
    pfb = _pfb()
    N, os_, spec, variant, n_dat, n_pol, kernel, oracle = ANALYSIS[case]
    taps = _analysis_taps(N, os_, spec)
    x = _noise(gpu, (n_pol, n_dat), 9800 + N)

    def make():
        return pfb.AnalysisPlan(taps, N, os_, variant, n_pol)

    # (reset: the LowCBF plan pads its first call only, and the warm-up call was one)
    ref, plan = sh.poison_delay(f"AnalysisPlan.execute {case}", make, lambda p, xs, outs: [p.execute(xs[0])], [x],
                                reset=lambda p: p.reset())
    assert ref[0].shape[0] == n_pol and ref[0].shape[1] > (2048 if N == 4096 else 8)
    if variant == "polyphase_analysis_lowcbf":
        plan.reset()  # (the padding of the first call is due again)
    _assert_branch(lambda: plan.execute(x), 0, kernel)
    if oracle:
        want = getattr(orc, variant)(x.cpu().numpy()[:, None, :], taps, N, os_)
        assert_pfb_close(ref[0].transpose(1, 2).cpu().numpy(), want, what=f"analysis {case}")


# ---------------------------------------------------------------------------- 1b. FilterBank.execute x 3
# id -> (analysis function, N, os, taps, chunks, n_pol)
FILTERBANK = {
    # call 2 reads its carry in place behind the new samples, call 3 (shorter than the carry)
    # concatenates: chunks of test_filterbank_stream_carry_in_place
    "carry-in-place-1pol": ("polyphase_analysis", 256, "8/7", "c2", (70000, 40000, 5), 1),
    "carry-in-place-2pol": ("polyphase_analysis", 256, "8/7", "c2", (70000, 40000, 5), 2),
    # carries of 3408 and 4209 samples > P N = 3328: the `pre` descriptor, one launch
    # (test_filterbank_stream_long_carry_one_launch's chunk lengths 50000 + 977 i)
    "long-carry": ("polyphase_analysis", 256, "8/7", "c2", (50000, 50977, 51954), 1),
    # test_filterbank_stream_padded: no row, then the circular shift and the nu-trim
    "padded-n4096": ("polyphase_analysis_padded", 4096, "8/7", "mid", (3000, 131072, 50000), 2),
    # test_fused_lowcbf_first_and_stream_calls' lengths: the padding is applied once
    "lowcbf": ("polyphase_analysis_lowcbf", 256, "4/3", "pst",
               (3072 - 1536 + 41 * 192 + 5, 3072 + 23 * 192 + 7, 19 * 192 + 3), 2),
}


def _fb_run(fb, xs, outs):
    res = []
    fb.carries = []
    for x in xs:
        fb.carries.append(fb.buffered_samples)
        _, y = fb.execute(x)
        res.append(y)
    return res


@pytest.mark.parametrize("case", list(FILTERBANK), ids=list(FILTERBANK))
def test_filterbank_chunks_on_a_side_stream(gpu, case):
    pfb = _pfb()
    fn, N, os_, spec, chunks, n_pol = FILTERBANK[case]
    cfg = dict(analysis_function=fn, filt_coeff=_named_taps(spec), channels=N, os_factor=os_)
    xs = [_noise(gpu, (n_pol, n), 9900 + i) for i, n in enumerate(chunks)]
    ref, fb = sh.poison_delay(f"FilterBank.execute {case}", lambda: pfb.FilterBank(cfg), _fb_run, xs,
                              reset=lambda f: f.reset(), buffered=lambda f: f.buffered_samples)
    assert fb.buffered_samples > 0 and sum(r.shape[2] for r in ref[1:]) > 0
    if case == "long-carry":
        assert fb.carries[1:] == [3408, 4209] and min(fb.carries[1:]) > 13 * 256
    if case.startswith("carry-in-place"):
        assert 0 < fb.carries[1] < chunks[1] and fb.carries[2] > chunks[2]


# ---------------------------------------------------------------------------- 1c. strided, cascades
def test_execute_strided_on_a_side_stream(gpu):
    """pfb_filterbank_execute_strided writing channel-major runs into a sentinel buffer, two
    calls (the second with a carry)."""
    import torch
    pfb = _pfb()
    taps = _named_taps("c2")
    xs = [_noise(gpu, (2, n), 10000 + n) for n in (40000, 30001)]
    T = 256  # samples per channel run: more than either call's rows

    def run(plan, xs, outs):
        res = []
        for i, x in enumerate(xs):
            # (runs longer than the rows: what the call leaves alone keeps the sentinel in both)
            out = outs[i] if outs else torch.full((2, 256, T), sh.SENTINEL, dtype=torch.complex64, device=x.device)
            rows = plan.execute_strided(x, out, 256 * T, 1, T)
            assert 0 < rows < T
            res.append(out)
        return res

    sh.poison_delay("AnalysisPlan.execute_strided", lambda: pfb.AnalysisPlan(taps, 256, "8/7", "polyphase_analysis", 2),
                    run, xs, takes_out=True, reset=lambda p: p.reset(), buffered=lambda p: p.buffered_samples)


def _two_stage(variant, strided):
    pfb = _pfb()
    cfg1 = dict(analysis_function=variant, filt_coeff=_taps(64, "8/7", 12), channels=64, os_factor="8/7")
    cfg2 = dict(analysis_function=variant, filt_coeff=_taps(16, "8/7", 10), channels=16, os_factor="8/7")
    ts = pfb.TwoStageFilterBank(cfg1).set_stage2_config(cfg2)
    ts.critical = 1
    ts.strided = strided
    return ts


def _two_stage_reset(ts):
    ts.stage1.reset()
    if ts.stage2 is not None:
        ts.stage2.reset()


def _cascade_run(ts, xs, outs):
    return [ts.execute(x)[1] for x in xs]


@pytest.mark.parametrize("strided", [True, False], ids=["strided", "turn-gather"])
@pytest.mark.parametrize("variant", ["polyphase_analysis", "polyphase_analysis_padded"], ids=["bunton", "padded"])
def test_two_stage_filterbank_on_a_side_stream(gpu, variant, strided, monkeypatch):
    """The 64 x 16 cascade of test_two_stage_padded_matches_oracle, Bunton and padded, two calls
    (carry in both stages).  Padded stages store strided (pfb_filterbank_execute_strided); with
    ``strided = False``, and for the 64-channel Bunton stages whose kernel has no strided
    store, stage 1 takes the corner turn and stage 2 the gather."""
    from ska_pst_dsp_model_amd import layout
    calls = {"turn": 0, "gather": 0}
    turn, gather = layout.corner_turn, layout.gather_channels

    def counted_turn(*a, **k):
        calls["turn"] += 1
        return turn(*a, **k)

    def counted_gather(*a, **k):
        calls["gather"] += 1
        return gather(*a, **k)

    monkeypatch.setattr(layout, "corner_turn", counted_turn)
    monkeypatch.setattr(layout, "gather_channels", counted_gather)
    xs = [_noise(gpu, (2, n), 10100 + n) for n in (300_000, 123_457)]
    ref, ts = sh.poison_delay(f"TwoStageFilterBank {variant} strided={strided}", lambda: _two_stage(variant, strided),
                              _cascade_run, xs, reset=_two_stage_reset,
                              buffered=lambda t: (t.stage1.buffered_samples, t.stage2.buffered_samples))
    assert all(r.shape[1] == 64 * 14 and r.shape[2] > 0 for r in ref)
    uses_layout = not strided or variant == "polyphase_analysis"
    assert (calls["turn"] > 0) == uses_layout and (calls["gather"] > 0) == uses_layout, calls
    if variant == "polyphase_analysis" and strided:
        # a shape no other module runs: against the oracle's 64 separate stage-2 objects
        t1, t2 = _taps(64, "8/7", 12), _taps(16, "8/7", 10)
        ots = orc.TwoStageFilterBankOracle(orc.FilterBankOracle(t1, 64, "8/7"),
                                           lambda: orc.FilterBankOracle(t2, 16, "8/7"), critical=True, single=False)
        for x, r in zip(xs, ref):
            want = ots.execute(x.cpu().numpy()[:, None, :])
            assert_pfb_close(r.cpu().numpy(), want, what="two-stage 64 x 16 Bunton")


@pytest.mark.parametrize("strided_input", [True, False], ids=["strided", "gather"])
def test_two_stage_inverse_on_a_side_stream(gpu, strided_input):
    """test_two_stage_inverse_matches_oracle's cascade (critical, 4 coarse channels of 14), two
    calls: the coarse-channel slices read in place (pfb_inverse_filterbank_execute_strided) and
    gathered first (pfb_gather_channels + pfb_inverse_filterbank_execute)."""
    pfb = _pfb()
    cfg = dict(filt_coeff=_taps(16, "8/7", 10), channels=16, os_factor="8/7", input_fft_length=128,
               input_overlap=16, deripple=False, temporal_taper="tukey")

    def make():
        ti = pfb.TwoStageInverseFilterBank(cfg)
        ti.nch2 = 14
        ti.strided_input = strided_input
        return ti

    def reset(ti):
        if ti.stage2 is not None:
            ti.stage2.reset()

    xs = [_noise(gpu, (1, 4 * 14, n), 10200 + n) for n in (700, 450)]
    ref, ti = sh.poison_delay(f"TwoStageInverseFilterBank strided_input={strided_input}", make, _cascade_run, xs,
                              reset=reset, buffered=lambda t: t.stage2.buffered_samples)
    assert all(r.shape[1] == 4 and r.shape[2] > 0 for r in ref)
    assert ti.stage2._plan.last_strided_input() == ("in_place" if strided_input else "none")


# ---------------------------------------------------------------------------- 1d. SynthesisPlan
# id -> (N, os, Nf, Ov, combine, deripple taps or None, n_pol, blocks, chunk_blocks, class-2 kernel piece,
#        oracle run)
SYNTHESIS = {
    "block-n8-nf128": (8, "8/7", 128, 16, 1, 10, 2, 3, 0, "synth_block_kernel<128,", False),
    "wave-n256-nf256": (256, "8/7", 256, 48, 1, "c2", 2, 3, 0, "synth_wave_kernel<", False),
    # (no deripple: the host design of 512 x 12 taps takes seconds, and the gains are a table)
    "wave512-n512-nf512": (512, "8/7", 512, 128, 1, None, 1, 3, 0, "synth_wave512_kernel<", True),
    "chunked-n256-nf256": (256, "8/7", 256, 48, 1, "c2", 2, 5, 2, None, False),
    # tests/test_gpu_parity.py test_synthesis_4096_persistent_chan_ifft, combine 2
    "n4096-combine2": (4096, "8/7", 512, 128, 2, "mid", 1, 8, 0, None, False),
}


def _syn_taps(N, os_, spec):
    if spec is None:
        return None
    return _named_taps(spec) if isinstance(spec, str) else _taps(N, os_, spec)


def _syn_plan(case):
    pfb = _pfb()
    N, os_, nf, ov, combine, spec, n_pol, _, chunk, _, _ = SYNTHESIS[case]
    win = pfb.PFBWindow().lookup["tukey"](nf, ov)
    plan = pfb.SynthesisPlan(N, os_, nf, ov, True, combine, spec is not None, _syn_taps(N, os_, spec), win, None, n_pol)
    if chunk:
        plan.set_chunk_blocks(chunk)
    return plan


def _syn_rows(gpu, case, extra=0):
    """(n_pol, rows, N + extra) engine-order rows of the case: whole blocks and a ragged tail."""
    N, _, nf, ov, _, _, n_pol, blocks, _, _, _ = SYNTHESIS[case]
    return _noise(gpu, (n_pol, blocks * (nf - 2 * ov) + 2 * ov + 3, N + extra), 10300 + N + nf)


def test_the_synthesis_has_no_nf64_kernel(gpu):
    """The smallest block-kernel shape is N 8, Nf 128 (the case below): an Nf 64 plan is
    refused when it is built."""
    pfb = _pfb()
    with pytest.raises(pfb.PfbError):
        pfb.SynthesisPlan(8, "8/7", 64, 8, True, 1, False, None, pfb.PFBWindow().lookup["tukey"](64, 8), None, 1)


@pytest.mark.parametrize("entry", ["execute", "execute_view"])
@pytest.mark.parametrize("case", list(SYNTHESIS), ids=list(SYNTHESIS))
def test_synthesis_execute_on_a_side_stream(gpu, case, entry):
    """``execute(out=)`` on packed rows and ``execute_view(out=)`` on a channel window of a
    wider buffer (pfb_synthesis_execute and its strided form), sample offset 3."""
    N, os_, nf, ov, combine, spec, n_pol, blocks, chunk, kernel, oracle = SYNTHESIS[case]
    if entry == "execute":
        x = _syn_rows(gpu, case)

        def run(plan, xs, outs):
            return [plan.execute(xs[0], sample_offset=3, layout="ptc", out=outs[0] if outs else None)]
    else:
        x = _syn_rows(gpu, case, extra=8)

        def run(plan, xs, outs):
            return [plan.execute_view(xs[0][:, :, 4:4 + N], sample_offset=3, out=outs[0] if outs else None)]

    ref, plan = sh.poison_delay(f"SynthesisPlan.{entry} {case}", lambda: _syn_plan(case), run, [x], takes_out=True)
    assert ref[0].shape[0] == n_pol and ref[0].shape[1] > 0
    if combine == 1:
        assert ref[0].shape[1] == blocks * plan.output_keep
    if entry == "execute_view":
        # (the 4096-point channel IFFT keeps its own loads: the view is copied to a packed buffer)
        assert plan.last_strided_input() == ("staged" if N == 4096 else "in_place")
        return
    if kernel:
        _assert_branch(lambda: run(plan, [x], None), 2, kernel)
    if oracle:
        dr = {"apply_deripple": int(spec is not None), "filter_coeff": _syn_taps(N, os_, spec)}
        want = orc.polyphase_synthesis(x.transpose(1, 2).cpu().numpy(), 1, nf, os_, dr, 3, ov,
                                       orc.pfb_window("tukey", nf, ov), None, combine)
        assert_pfb_close(ref[0][:, None, :].cpu().numpy(), want, what=f"synthesis {case}")


# ---------------------------------------------------------------------------- 1e. InverseFilterBank x 3
@pytest.mark.parametrize("N,nf,ov,so,chunks", [(8, 128, 16, 5, (500, 333, 1000)),
                                               (256, 256, 48, 17, (1000, 161, 5000))],
                         ids=["n8-nf128", "n256-nf256"])
def test_inverse_filterbank_chunks_on_a_side_stream(gpu, N, nf, ov, so, chunks):
    """The shapes of test_inverse_filterbank_stream_carry_in_place with a sample offset, two
    polarisations: stitched first blocks, the rest on the new rows in place, the carry moves."""
    pfb = _pfb()
    taps = _taps(8, "8/7", 10) if N == 8 else _named_taps("c2")
    cfg = dict(filt_coeff=taps, channels=N, os_factor="8/7", input_fft_length=nf, input_overlap=ov,
               deripple=True, temporal_taper="tukey")

    def make():
        ifb = pfb.InverseFilterBank(cfg, honour_deripple=True)
        ifb.sample_offset = so
        return ifb

    xs = [_noise(gpu, (2, N, n), 10400 + n) for n in chunks]
    ref, ifb = sh.poison_delay(f"InverseFilterBank.execute N {N}", make,
                               lambda o, xs, outs: [o.execute(x)[1] for x in xs], xs,
                               reset=lambda o: o.reset(), buffered=lambda o: o.buffered_samples)
    assert ifb.buffered_samples > 0 and all(r.shape[2] > 0 for r in ref)


# ---------------------------------------------------------------------------- 1f. DADA sections
C2_ROWS = 2 * 160 + 96          # two synthesis blocks of the 256-channel, Nf 256, Ov 48 plan
C2_SAMPLES = 13 * 256 + C2_ROWS * 224 + 17


def _c2_analysis(n_pol):
    return _pfb().AnalysisPlan(_named_taps("c2"), 256, "8/7", "polyphase_analysis", n_pol)


def _c2_synthesis(n_pol):
    pfb = _pfb()
    return pfb.SynthesisPlan(256, "8/7", 256, 48, True, 1, True, _named_taps("c2"),
                             pfb.PFBWindow().lookup["tukey"](256, 48), None, n_pol)


def _series_section(gpu, nbit, n_dat, n_pol, seed):
    return _ints(gpu, (n_dat, n_pol, 2), seed, nbit)


def _rows_section(gpu, nbit, rows, N, n_pol, seed):
    return _ints(gpu, (rows, N, n_pol, 2), seed, nbit)


def _analysis_scale(raw, nbit, n_pol):
    plan = _c2_analysis(n_pol)
    return _unit_scale(plan.execute_dada(raw, nbit))


# (NBIT in, NBIT out, n_pol, LowCBF order): every NBIT and polarisation count in TFP order, and
# one section in LowCBF heap order (whole heaps of 32 samples)
NBIT_PAIRS = [(8, 8, 1, False), (8, 32, 2, False), (16, 8, 2, False), (16, 32, 1, False), (16, 8, 2, True)]
C2_HEAPS = C2_SAMPLES - C2_SAMPLES % 32   # 3016 heaps: the same 416 rows


def _pair_id(c):
    return f"in{c[0]}-out{c[1]}-{c[2]}pol-{'lowcbf' if c[3] else 'tfp'}"


def _paths(expect_in=None, expect_out=None):
    """check(plan): the host branch its last call took (core.py last_dada_input / _output)."""
    def check(plan):
        if expect_in is not None:
            assert plan.last_dada_input() == expect_in, f"section read {plan.last_dada_input()}, not {expect_in}"
        if expect_out is not None:
            assert plan.last_dada_output() == expect_out, f"section written {plan.last_dada_output()}, not {expect_out}"
    return check


@pytest.mark.parametrize("nbit,n_pol", [(8, 1), (16, 2)])
def test_analysis_execute_dada_on_a_side_stream(gpu, nbit, n_pol):
    """The streaming kernel loads a TFP section itself (analysis_dada_fusable)."""
    raw = _series_section(gpu, nbit, C2_SAMPLES, n_pol, 10500 + nbit)
    ref, _ = sh.poison_delay(f"AnalysisPlan.execute_dada NBIT {nbit}", lambda: _c2_analysis(n_pol),
                             lambda p, xs, outs: [p.execute_dada(xs[0], nbit)], [raw], check=_paths("fused"))
    assert ref[0].shape == (n_pol, C2_ROWS, 256)


def test_analysis_execute_dada_lowcbf_order_on_a_side_stream(gpu):
    """A section in LowCBF heap order is never read in place (analysis_dada_fusable: TFP only):
    pfb_dada_unpack into the plan's staging buffer, then the cf32 launch."""
    raw = _series_section(gpu, 16, C2_HEAPS, 2, 10510)
    ref, _ = sh.poison_delay("AnalysisPlan.execute_dada LowCBF order", lambda: _c2_analysis(2),
                             lambda p, xs, outs: [p.execute_dada(xs[0], 16, lowcbf=True)], [raw],
                             check=_paths("staged"))
    assert ref[0].shape == (2, C2_ROWS, 256)


@pytest.mark.parametrize("out_nbit,n_pol", [(8, 2), (32, 1)])
def test_analysis_execute_to_dada_on_a_side_stream(gpu, out_nbit, n_pol):
    """The streaming kernel stores NBIT 8 / 16 / 32 sections itself (analysis_dada_out_fusable)."""
    x = _noise(gpu, (n_pol, C2_SAMPLES), 10520 + out_nbit)
    scale = _unit_scale(_c2_analysis(n_pol).execute(x))
    ref, _ = sh.poison_delay(f"AnalysisPlan.execute_to_dada NBIT {out_nbit}", lambda: _c2_analysis(n_pol),
                             lambda p, xs, outs: [p.execute_to_dada(xs[0], out_nbit, scale=scale)], [x],
                             check=_paths("none", "fused"))
    assert ref[0].shape == (C2_ROWS, 256, n_pol, 2)
    assert float((ref[0].float().abs() >= 127).float().mean()) < 0.01


@pytest.mark.parametrize("case", NBIT_PAIRS, ids=_pair_id)
def test_analysis_execute_dada_to_dada_on_a_side_stream(gpu, case):
    """The output is stored by the kernel in every case; the input is read in place when the
    DADA-store kernel has a loader for it (the output's own NBIT, or an integer section into
    NBIT 32: pfb::dadaout_reads_dada), else unpacked first — NBIT 16 into NBIT 8, and every
    section in LowCBF order."""
    nbit, out_nbit, n_pol, lowcbf = case
    raw = _series_section(gpu, nbit, C2_HEAPS if lowcbf else C2_SAMPLES, n_pol, 10530 + nbit + out_nbit)
    scale = _unit_scale(_c2_analysis(n_pol).execute_dada(raw, nbit, lowcbf=lowcbf))
    staged = lowcbf or (nbit, out_nbit) == (16, 8)
    ref, _ = sh.poison_delay(
        f"AnalysisPlan.execute_dada_to_dada {_pair_id(case)}", lambda: _c2_analysis(n_pol),
        lambda p, xs, outs: [p.execute_dada_to_dada(xs[0], nbit, out_nbit, scale=scale, lowcbf=lowcbf)], [raw],
        check=_paths("staged" if staged else "fused", "fused"))
    assert ref[0].shape == (C2_ROWS, 256, n_pol, 2)
    assert float((ref[0].float().abs() >= 127).float().mean()) < 0.01


FB_DADA_CHUNKS = (9000, 100, 7777)   # tests/test_gpu_dada_analysis.py CHUNKS: the second completes no row


@pytest.mark.parametrize("entry", ["execute_dada", "execute_to_dada", "execute_dada_to_dada"])
def test_filterbank_dada_chunks_on_a_side_stream(gpu, entry):
    """The three DADA entries of the FilterBank stream object over three chunks, NBIT 16 in,
    NBIT 8 out, two polarisations (the object's DADA entries take TFP sections only).  The last
    call reads its carry through the second descriptor and its section in place, except into
    NBIT 8, which has no NBIT 16 loader."""
    pfb = _pfb()
    cfg = dict(analysis_function="polyphase_analysis", filt_coeff=_named_taps("c2"), channels=256, os_factor="8/7")
    if entry == "execute_to_dada":
        xs = [_noise(gpu, (2, n), 10540 + n) for n in FB_DADA_CHUNKS]
        scale = _unit_scale(_c2_analysis(2).execute(xs[0]))
        call = lambda fb, x: fb.execute_to_dada(x, 8, scale=scale)[1]
        paths = ("none", "fused")
    else:
        xs = [_series_section(gpu, 16, n, 2, 10540 + n) for n in FB_DADA_CHUNKS]
        scale = _analysis_scale(xs[0], 16, 2)
        if entry == "execute_dada":
            call = lambda fb, x: fb.execute_dada(x, 16, n_pol=2)[1]
            paths = ("fused", "none")
        else:
            call = lambda fb, x: fb.execute_dada_to_dada(x, 16, 8, scale=scale, n_pol=2)[1]
            paths = ("staged", "fused")
    ref, fb = sh.poison_delay(f"FilterBank.{entry}", lambda: pfb.FilterBank(cfg),
                              lambda fb, xs, outs: [call(fb, x) for x in xs], xs,
                              reset=lambda f: f.reset(), buffered=lambda f: f.buffered_samples,
                              check=lambda f: _paths(*paths)(f._plan))
    assert fb.buffered_samples > 0 and ref[0].numel() > 0 and ref[2].numel() > 0


@pytest.mark.parametrize("nbit,lowcbf,n_pol", [(8, False, 1), (16, False, 2), (16, True, 2)],
                         ids=["tfp8-1pol", "tfp16-2pol", "lowcbf16-2pol"])
def test_synthesis_execute_dada_on_a_side_stream(gpu, nbit, lowcbf, n_pol):
    """tests/test_gpu_dada_synthesis.py cases a and b: 576 rows TFP, 608 rows (19 heaps) in
    LowCBF order from sample offset 4; three blocks each, into an ``out`` buffer.  The channel
    IFFT reads NBIT 8 / 16 sections of either order itself (dada_fusable)."""
    rows, so = (608, 4) if lowcbf else (576, 1)
    raw = _rows_section(gpu, nbit, rows, 256, n_pol, 10560 + nbit)
    ref, plan = sh.poison_delay(
        f"SynthesisPlan.execute_dada NBIT {nbit} lowcbf={lowcbf}", lambda: _c2_synthesis(n_pol),
        lambda p, xs, outs: [p.execute_dada(xs[0], nbit, lowcbf=lowcbf, sample_offset=so, out=outs[0] if outs else None)],
        [raw], takes_out=True, check=_paths("fused", "none"))
    assert ref[0].shape == (n_pol, 3 * plan.output_keep)


@pytest.mark.parametrize("out_nbit,n_pol", [(8, 2), (32, 1)])
def test_synthesis_execute_to_dada_on_a_side_stream(gpu, out_nbit, n_pol):
    """The wave kernel stores NBIT 8 / 16 / 32 sections itself (synthesis_dada_out_fusable)."""
    x = _noise(gpu, (n_pol, 576, 256), 10570 + out_nbit)
    scale = _unit_scale(_c2_synthesis(n_pol).execute(x, layout="ptc"))
    ref, plan = sh.poison_delay(f"SynthesisPlan.execute_to_dada NBIT {out_nbit}", lambda: _c2_synthesis(n_pol),
                                lambda p, xs, outs: [p.execute_to_dada(xs[0], out_nbit, scale=scale, layout="ptc")], [x],
                                check=_paths("none", "fused"))
    assert ref[0].shape == (3 * plan.output_keep, 1, n_pol, 2)
    assert float((ref[0].float().abs() >= 127).float().mean()) < 0.01


@pytest.mark.parametrize("case", NBIT_PAIRS, ids=_pair_id)
def test_synthesis_execute_dada_to_dada_on_a_side_stream(gpu, case):
    """Section in (either order, read by the channel IFFT), section out (stored by the wave
    kernel); the LowCBF case is 608 rows (19 heaps) from sample offset 4."""
    nbit, out_nbit, n_pol, lowcbf = case
    rows, so = (608, 4) if lowcbf else (576, 1)
    raw = _rows_section(gpu, nbit, rows, 256, n_pol, 10580 + nbit + out_nbit)
    scale = _unit_scale(_c2_synthesis(n_pol).execute_dada(raw, nbit, lowcbf=lowcbf, sample_offset=so))
    ref, plan = sh.poison_delay(
        f"SynthesisPlan.execute_dada_to_dada {_pair_id(case)}", lambda: _c2_synthesis(n_pol),
        lambda p, xs, outs: [p.execute_dada_to_dada(xs[0], nbit, out_nbit, scale=scale, lowcbf=lowcbf,
                                                    sample_offset=so)], [raw], check=_paths("fused", "fused"))
    assert ref[0].shape == (3 * plan.output_keep, 1, n_pol, 2)
    assert float((ref[0].float().abs() >= 127).float().mean()) < 0.01


# rows per chunk: tests/test_gpu_python_surface.py ROWS_A, ROWS_B and a ragged third chunk; in
# LowCBF order whole heaps of 32 rows
IFB_DADA_ROWS = {False: (248, 320, 300), True: (256, 320, 288)}
IFB_DADA_CASES = [("execute_dada", False), ("execute_to_dada", False), ("execute_dada_to_dada", False),
                  ("execute_dada", True), ("execute_dada_to_dada", True)]


@pytest.mark.parametrize("entry,lowcbf", IFB_DADA_CASES,
                         ids=[f"{e}-{'lowcbf' if l else 'tfp'}" for e, l in IFB_DADA_CASES])
def test_inverse_filterbank_dada_chunks_on_a_side_stream(gpu, entry, lowcbf):
    """The three DADA entries of the InverseFilterBank stream object over three chunks of the
    8-channel, Nf 128 synthesis: NBIT 16 in (TFP and LowCBF order), NBIT 8 out, two
    polarisations.  The channel IFFT reads the new rows' section itself and the carry is
    unpacked from it; the block kernel of this shape stores no section, so the output is
    packed by a second launch (synthesis_dada_out_fusable: the wave kernels only)."""
    pfb = _pfb()
    cfg = dict(filt_coeff=_taps(8, "8/7", 10), channels=8, os_factor="8/7", input_fft_length=128,
               input_overlap=16, deripple=False, temporal_taper="tukey")
    probe = pfb.InverseFilterBank(cfg)
    chunks = IFB_DADA_ROWS[lowcbf]
    if entry == "execute_to_dada":
        xs = [_noise(gpu, (2, 8, n), 10590 + n) for n in chunks]
        scale = _unit_scale(probe.execute(xs[0])[1])
        call = lambda o, x: o.execute_to_dada(x, 8, scale=scale)[1]
        paths = ("none", "staged")
    else:
        xs = [_rows_section(gpu, 16, n, 8, 2, 10590 + n) for n in chunks]
        scale = _unit_scale(probe.execute_dada(xs[0], 16, lowcbf=lowcbf, n_pol=2)[1])
        if entry == "execute_dada":
            call = lambda o, x: o.execute_dada(x, 16, lowcbf=lowcbf, n_pol=2)[1]
            paths = ("fused", "none")
        else:
            call = lambda o, x: o.execute_dada_to_dada(x, 16, 8, scale=scale, lowcbf=lowcbf, n_pol=2)[1]
            paths = ("fused", "staged")
    ref, ifb = sh.poison_delay(f"InverseFilterBank.{entry} lowcbf={lowcbf}", lambda: pfb.InverseFilterBank(cfg),
                               lambda o, xs, outs: [call(o, x) for x in xs], xs,
                               reset=lambda o: o.reset(), buffered=lambda o: o.buffered_samples,
                               check=lambda o: _paths(*paths)(o._plan))
    assert ifb.buffered_samples > 0 and all(r.numel() > 0 for r in ref)


@pytest.mark.parametrize("case", NBIT_PAIRS, ids=_pair_id)
def test_roundtrip_dada_on_a_side_stream(gpu, case):
    """pfb_roundtrip_execute_dada_to_dada: both sections of the file-to-file round trip.  TFP
    sections take the FUSED branch (the analysis launch reads and stores the sections, the wave
    kernel stores the output); a section in LowCBF order is never read in place
    (roundtrip_dada_in_fusable), so the whole call takes the STAGED tail: section_unpack, the
    cf32 round trip on plan-owned buffers, pfb_dada_pack of the product and the scaled pack of
    the output."""
    pfb = _pfb()
    from ska_pst_dsp_model_amd import layout
    nbit, out_nbit, n_pol, lowcbf = case
    raw = _series_section(gpu, nbit, C2_HEAPS if lowcbf else C2_SAMPLES, n_pol, 10600 + nbit + out_nbit)
    x = layout.dada_unpack(raw, nbit, 2, 1, n_pol, lowcbf=lowcbf)[:, :, 0].contiguous()
    scale = _unit_scale(pfb.roundtrip(_c2_analysis(n_pol), _c2_synthesis(n_pol), x)[1])
    path = "staged" if lowcbf else "fused"

    def run(pair, xs, outs):
        return list(pfb.roundtrip_dada(pair[0], pair[1], xs[0], nbit, out_nbit, scale=scale, lowcbf=lowcbf))

    def check(pair):
        _paths(path, path)(pair[0])
        _paths(None, path)(pair[1])

    ref, _ = sh.poison_delay(f"roundtrip_dada {_pair_id(case)}",
                             lambda: (_c2_analysis(n_pol), _c2_synthesis(n_pol)), run, [raw], check=check)
    assert ref[0].shape == (C2_ROWS, 256, n_pol, 2) and ref[1].shape == (2 * 160 * 224, 1, n_pol, 2)
    assert float((ref[1].float().abs() >= 127).float().mean()) < 0.01


# ---------------------------------------------------------------------------- 1g. plan-free utilities
def test_dada_unpack_and_pack_on_a_side_stream(gpu):
    from ska_pst_dsp_model_amd import layout
    raw = _ints(gpu, (1000, 6, 2, 2), 10700, 16)
    sh.poison_delay("layout.dada_unpack", lambda: None,
                    lambda _, xs, outs: [layout.dada_unpack(xs[0], 16, 2, 6, 2)], [raw])
    x = _noise(gpu, (2, 333, 16), 10701, scale=300.0)
    sh.poison_delay("layout.dada_pack", lambda: None, lambda _, xs, outs: [layout.dada_pack(xs[0], 16)], [x])


def test_gather_and_corner_turn_on_a_side_stream(gpu):
    import torch
    from ska_pst_dsp_model_amd import layout
    x = _noise(gpu, (3, 1037, 45), 10710)
    sh.poison_delay("layout.corner_turn", lambda: None, lambda _, xs, outs: [layout.corner_turn(xs[0])], [x])

    def gather(_, xs, outs):
        out = outs[0] if outs else torch.zeros((5, 1037, 9), dtype=torch.complex64, device=xs[0].device)
        return [layout.gather_channels(xs[0][0], n_outer=5, in_outer_stride=9, in_row_stride=45, n_rows=1037,
                                       n_sel=9, out=out, out_outer_stride=1037 * 9, out_row_stride=9)]

    ref, _ = sh.poison_delay("layout.gather_channels", lambda: None, gather, [x], takes_out=True)
    assert torch.equal(ref[0], x[0].reshape(1037, 5, 9).permute(1, 0, 2))


def test_quantize_round_on_a_side_stream(gpu):
    """rms = 0: no moments, the rounding pass alone (bit-identical)."""
    from ska_pst_dsp_model_amd import layout
    x = _noise(gpu, (2, 5001), 10720, scale=20.0)
    sh.poison_delay("layout.quantize rms 0", lambda: None,
                    lambda _, xs, outs: [layout.quantize(xs[0], 0.0, out=outs[0] if outs else None)], [x], takes_out=True)


def _assert_quantized(got, x, rms, what):
    """test_quantize_rms_scale's allowance against the oracle: a value may differ by at most one
    unit (a product within an ulp of a .5 tie), in fewer than 1e-4 of the samples."""
    xh = x.cpu().numpy()
    want = orc.quantize(xh, orc.quantize_scale(xh, rms))
    d = np.abs(got.cpu().numpy().reshape(want.shape) - want)
    frac = float((d > 0).mean())
    print(f"{what}: max |diff| {d.max():.3g}, fraction differing {frac:.3g}")
    assert d.max() <= 1.0 and frac < 1e-4, f"{what}: max |diff| {d.max():.3g}, fraction differing {frac:.3g}"


def test_quantize_rms_on_a_side_stream(gpu):
    """rms > 0 (memset, moments, rounding pass; the double atomics make even the serial call
    not bit-reproducible: the oracle under test_quantize_rms_scale's allowance)."""
    import torch
    from ska_pst_dsp_model_amd import layout
    x = _noise(gpu, (2, 1 << 16), 10721, scale=3.0) + complex(0.25, -0.5)
    layout.quantize(x.flip(1), 33.8)  # (the moments block of the default stream exists and is stale)
    (ref,), ref_ms = sh.timed(lambda: [layout.quantize(x, 33.8)])
    _assert_quantized(ref, x, 33.8, "default stream")
    inp, out = sh.poison_(torch.empty_like(x)), sh.sentinel_like(x)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # a stream's first call allocates its moments block: made here,
        layout.quantize(x.flip(1), 33.8)   # on other samples, not behind the delay
    torch.cuda.synchronize()
    with sh.Delayed(ref_ms, "layout.quantize rms 33.8", stream=side) as d:
        inp.copy_(x)
        got = layout.quantize(inp, 33.8, out=out).clone()
        d.assert_pending()
    d.stream.synchronize()
    _assert_quantized(got, x, 33.8, "side stream")
    assert sh.same_bits(inp, x)


def test_testvec_generate_on_a_side_stream(gpu):
    import torch
    from ska_pst_dsp_model_amd import verify
    items = [("time", 17), ("freq", 5), ("time", 900), ("freq", 33)]
    n = 4096
    ref, ref_ms = sh.timed(lambda: verify.device_vectors(items, n).clone())
    out = sh.sentinel_like(ref)
    torch.cuda.synchronize()
    with sh.Delayed(ref_ms, "verify.device_vectors") as d:
        got = verify.device_vectors(items, n, out=out).clone()
        d.assert_pending()
    d.stream.synchronize()
    assert sh.same_bits(got, ref) and abs(float(ref.abs().max()) - 1.0) < 1e-6


# ============================================================================ 2. at once
# input lengths: three blocks of the 256-channel pair (Nf 256, Ov 48), four of the 64-channel one
# (4/3, Nf 128, Ov 16), and a ragged tail
PAIR_SAMPLES = {"n256": 13 * 256 + (3 * 160 + 96) * 224 + 5, "n64": 13 * 64 + (4 * 96 + 32) * 48 + 7}


def _pair(kind, n_pol=1):
    """(analysis plan, synthesis plan) of the two plan pairs of part 2."""
    pfb = _pfb()
    if kind == "n256":
        return _c2_analysis(n_pol), _c2_synthesis(n_pol)
    taps = _taps(64, "4/3", 12)
    ana = pfb.AnalysisPlan(taps, 64, "4/3", "polyphase_analysis", n_pol)
    syn = pfb.SynthesisPlan(64, "4/3", 128, 16, True, 1, True, taps, pfb.PFBWindow().lookup["tukey"](128, 16), None,
                            n_pol)
    return ana, syn


def _pair_inputs(gpu, kind, n_pol=1, calls=4):
    return [_noise(gpu, (n_pol, PAIR_SAMPLES[kind]), 10800 + 7 * i + (0 if kind == "n256" else 100))
            for i in range(calls)]


def _pair_step(ana, syn, x):
    """Two calls: the analysis of ``x`` and the synthesis of its product."""
    chan = ana.execute(x)
    return chan, syn.execute(chan, layout="ptc")


def _serial(ana, syn, xs):
    import torch
    res = []
    for x in xs:
        res.extend(t.clone() for t in _pair_step(ana, syn, x))
    torch.cuda.synchronize()
    return res


def test_the_n64_pair_matches_the_oracle(gpu):
    """The 64-channel 4/3 pair of part 2 is a shape of this module alone."""
    ana, syn = _pair("n64", 2)
    x = _pair_inputs(gpu, "n64", 2, 1)[0]
    chan, out = _pair_step(ana, syn, x)
    taps = _taps(64, "4/3", 12)
    want = orc.polyphase_analysis(x.cpu().numpy()[:, None, :], taps, 64, "4/3")
    assert_pfb_close(chan.transpose(1, 2).cpu().numpy(), want, what="analysis 64 ch 4/3")
    want = orc.polyphase_synthesis(chan.transpose(1, 2).cpu().numpy(), 1, 128, "4/3",
                                   {"apply_deripple": 1, "filter_coeff": taps}, 1, 16, orc.pfb_window("tukey", 128, 16))
    assert out.shape[1] == 4 * 96 * 48
    assert_pfb_close(out[:, None, :].cpu().numpy(), want, what="synthesis 64 ch 4/3 Nf 128")


def test_two_streams_two_plan_pairs(gpu):
    """Eight calls each (four analyses, four syntheses) of a 256-channel 8/7 and a 64-channel
    4/3 plan pair, dealt alternately to two streams from one host thread with nothing in
    between, both streams held behind a gate until all sixteen are enqueued: every output equals
    the serial one."""
    import torch
    kinds = ("n256", "n64")
    xs = {k: _pair_inputs(gpu, k) for k in kinds}
    ref_pairs = {k: _pair(k) for k in kinds}
    refs, ref_ms = sh.timed(lambda: {k: _serial(*ref_pairs[k], xs[k]) for k in kinds})
    pairs = {k: _pair(k) for k in kinds}
    streams = {k: torch.cuda.Stream() for k in kinds}

    def deal(res):
        for i in range(4):
            for k in kinds:
                with torch.cuda.stream(streams[k]):
                    res[k].extend(_pair_step(*pairs[k], xs[k][i]))

    # the same calls on the same streams, not held back: the plans' buffers and the streams'
    # allocator pools exist afterwards, and its time bounds what the host needs to enqueue them
    _, warm_ms = sh.timed(lambda: deal({k: [] for k in kinds}))
    gate = sh.Gate(max(ref_ms, warm_ms), streams.values(), "two plan pairs")
    got = {k: [] for k in kinds}
    deal(got)
    gate.assert_pending()
    torch.cuda.synchronize()
    for k in kinds:
        assert len(got[k]) == 8
        for j, (g, r) in enumerate(zip(got[k], refs[k])):
            assert sh.same_bits(g, r), f"{k}: call {j}"


def _stream_sequence(obj, xs):
    """(outputs, buffered counts after every call) of a stream object over ``xs``; a chunk the
    object refuses (no complete block, carry rounded past the data) leaves an empty output."""
    pfb = _pfb()
    outs, counts = [], []
    for x in xs:
        try:
            outs.append(obj.execute(x)[1])
        except pfb.PfbError:
            outs.append(x.new_empty(0))
        counts.append(obj.buffered_samples)
    return outs, counts


def _interleaved(objs, seqs, ref_ms, streams):
    """objs[k] fed seqs[k], call i of every object before call i + 1 of any, each object on a
    stream of its own, no synchronisation; the streams are held behind a gate until every call
    is enqueued."""
    import torch
    gate = sh.Gate(ref_ms, streams, "stream objects at once")
    outs = [[] for _ in objs]
    counts = [[] for _ in objs]
    pfb = _pfb()
    for i in range(max(len(s) for s in seqs)):
        for k, obj in enumerate(objs):
            if i >= len(seqs[k]):
                continue
            with torch.cuda.stream(streams[k]):
                try:
                    outs[k].append(obj.execute(seqs[k][i])[1])
                except pfb.PfbError:
                    outs[k].append(seqs[k][i].new_empty(0))
                counts[k].append(obj.buffered_samples)
    gate.assert_pending()
    torch.cuda.synchronize()
    return outs, counts


def _assert_sequences(makers, seqs):
    import torch
    refs, ref_ms = [], 0.0
    for make, xs in zip(makers, seqs):
        ref_obj = make()
        (outs, counts), ms = sh.timed(lambda: _stream_sequence(ref_obj, xs))
        refs.append(([o.clone() for o in outs], counts))
        ref_ms += ms
    objs = [make() for make in makers]
    streams = [torch.cuda.Stream() for _ in objs]

    def warm():   # on other samples, on the streams of the run below (their allocator pools fill)
        for obj, xs, s in zip(objs, seqs, streams):
            with torch.cuda.stream(s):
                _stream_sequence(obj, [sh.scrambled(x) for x in xs])

    _, warm_ms = sh.timed(warm)
    for obj in objs:
        obj.reset()
    outs, counts = _interleaved(objs, seqs, max(ref_ms, warm_ms), streams)
    for k, (ref_outs, ref_counts) in enumerate(refs):
        assert counts[k] == ref_counts, f"object {k}: buffered_samples after every call"
        assert sum(o.numel() for o in ref_outs) > 0
        for j, (g, r) in enumerate(zip(outs[k], ref_outs)):
            assert sh.same_bits(g, r), f"object {k}: call {j}"


def test_two_streams_two_filterbanks(gpu):
    pfb = _pfb()
    cfgs = [dict(analysis_function="polyphase_analysis", filt_coeff=_named_taps("c2"), channels=256, os_factor="8/7"),
            dict(analysis_function="polyphase_analysis", filt_coeff=_taps(64, "4/3", 12), channels=64, os_factor="4/3")]
    chunks = [(70000, 5, 3001, 40000, 23457), (9000, 100, 7777, 6001, 9001)]
    seqs = [[_noise(gpu, (2, n), 10900 + 10 * k + i) for i, n in enumerate(c)] for k, c in enumerate(chunks)]
    _assert_sequences([lambda c=c: pfb.FilterBank(c) for c in cfgs], seqs)


def test_two_streams_two_inverse_filterbanks(gpu):
    pfb = _pfb()
    shapes = [(8, 128, 16, (500, 333, 1000, 20, 777)), (256, 256, 48, (1000, 161, 5000, 3, 2222))]
    makers, seqs = [], []
    for k, (N, nf, ov, chunks) in enumerate(shapes):
        cfg = dict(filt_coeff=_taps(8, "8/7", 10) if N == 8 else _named_taps("c2"), channels=N, os_factor="8/7",
                   input_fft_length=nf, input_overlap=ov, deripple=True, temporal_taper="tukey")
        makers.append(lambda c=cfg: pfb.InverseFilterBank(c, honour_deripple=True))
        seqs.append([_noise(gpu, (2, N, n), 10950 + 10 * k + i) for i, n in enumerate(chunks)])
    _assert_sequences(makers, seqs)


def _run_threads(targets, barriers=()):
    """Run the callables in threads of their own; re-raise the first failure (which also
    releases the threads waiting at one of ``barriers``)."""
    errors = []

    def wrap(fn):
        def body():
            try:
                fn()
            except BaseException as e:  # noqa: BLE001 - reported in the main thread
                errors.append(e)
                for b in barriers:
                    b.abort()
        return body

    threads = [threading.Thread(target=wrap(t)) for t in targets]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
        assert not t.is_alive(), "a worker thread did not finish"
    if errors:
        raise errors[0]


def test_two_host_threads(gpu):
    """Each thread has its own stream and plan pair and makes the eight calls of
    test_two_streams_two_plan_pairs (ctypes releases the GIL around every C call).  Thread 0
    then provokes PFB_ERR_BUFFER_TOO_SMALL: its text is thread 0's pfb_last_error only, and
    thread 1's last message, set by an error of its own before, is still what it was."""
    import torch
    pfb, L = _pfb(), _lib()
    kinds = ("n256", "n64")
    xs = {k: _pair_inputs(gpu, k) for k in kinds}
    refs = {k: _serial(*_pair(k), xs[k]) for k in kinds}
    pairs = {k: _pair(k) for k in kinds}
    for k in kinds:
        _pair_step(*pairs[k], xs[k][0].flip(1))
    torch.cuda.synchronize()
    got, msgs = {}, {}
    start, erred = threading.Barrier(2, timeout=60), threading.Barrier(2, timeout=60)

    def last_error():
        return (L.load().pfb_last_error() or b"").decode()

    def worker(k):
        def body():
            ana, syn = pairs[k]
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                if k == "n64":  # an error of this thread's own, first
                    with pytest.raises(pfb.PfbError):
                        ana.execute_dada(torch.zeros(64, dtype=torch.int16, device=gpu), 12)
                    msgs["n64 before"] = last_error()
                start.wait()
                out = []
                for x in xs[k]:
                    out.extend(_pair_step(ana, syn, x))
                s.synchronize()
                got[k] = out
                if k == "n256":
                    chan = out[0]
                    narrow = torch.empty((1, out[1].shape[1] - 1), dtype=torch.complex64, device=gpu)
                    with pytest.raises(pfb.PfbError) as e:
                        syn.execute_view(chan, out=narrow)
                    assert e.value.status == L.PFB_ERR_BUFFER_TOO_SMALL
                    msgs["n256"] = last_error()
                erred.wait()
                if k == "n64":
                    msgs["n64 after"] = last_error()
        return body

    _run_threads([worker(k) for k in kinds], (start, erred))
    for k in kinds:
        for j, (g, r) in enumerate(zip(got[k], refs[k])):
            assert sh.same_bits(g, r), f"thread {k}: call {j}"
    assert "NBIT" in msgs["n64 before"] and msgs["n64 after"] == msgs["n64 before"]
    assert msgs["n256"] and msgs["n256"] != msgs["n64 before"] and "NBIT" not in msgs["n256"]


def test_synchronous_utilities_from_two_threads(gpu):
    """The entry points that wait for their stream — the two purity scores,
    quantize(return_scale=True) and a host-memory analysis — called from two threads at once,
    five rounds each: the scores and the analysis equal the serial results exactly, the
    quantiser's scale to 1e-9 and its output under the oracle's allowance."""
    import torch
    from ska_pst_dsp_model_amd import layout, verify
    pfb = _pfb()
    taps = _taps(8, "8/7", 10)
    data = []
    for k in range(2):
        a = _noise(gpu, (3, 5000 + 7 * k), 11000 + k)
        b = a + _noise(gpu, tuple(a.shape), 11010 + k, scale=1e-3)
        q = _noise(gpu, (2, (1 << 16) + k), 11020 + k, scale=3.0 * (1 + 4 * k))
        h = _noise(gpu, (2, 3000 + k), 11030 + k).cpu().numpy()
        data.append((a, b, q, h))

    def once(k, plan):
        a, b, q, h = data[k]
        n = a.shape[1]
        y, sc = layout.quantize(q, 33.8, return_scale=True)
        return (verify._score_spurious(a, n, 1.0, 30, [5, 17, 4000]), verify._score_difference(a, b, n), y, sc,
                plan.execute(h).copy())

    def plan():
        return pfb.AnalysisPlan(taps, 8, "8/7", "polyphase_analysis", 2)

    serial = [once(k, plan()) for k in range(2)]
    results = {0: [], 1: []}
    start = threading.Barrier(2, timeout=60)

    def worker(k):
        def body():
            p = plan()
            with torch.cuda.stream(torch.cuda.Stream()):
                start.wait()
                for _ in range(5):
                    results[k].append(once(k, p))
        return body

    _run_threads([worker(0), worker(1)], (start,))
    for k in range(2):
        spur, diff, _, sc, chan = serial[k]
        ref_sc = orc.quantize_scale(data[k][2].cpu().numpy(), 33.8)
        assert abs(sc - ref_sc) <= 1e-9 * ref_sc
        assert len(results[k]) == 5
        for r, (g_spur, g_diff, g_y, g_sc, g_chan) in enumerate(results[k]):
            assert np.array_equal(g_spur, spur) and np.array_equal(g_diff, diff), f"thread {k} round {r}: scores"
            assert np.array_equal(g_chan, chan), f"thread {k} round {r}: host-memory analysis"
            assert abs(g_sc - ref_sc) <= 1e-9 * ref_sc, f"thread {k} round {r}: scale {g_sc} vs {ref_sc}"
            _assert_quantized(g_y, data[k][2], 33.8, f"thread {k} round {r}")


# ============================================================================ 3. pfb_quantize
QUANT_N = 1 << 20
QUANT_CALLS = 32
QUANT_RMS = 33.8


def _quantize_inputs(gpu, n=QUANT_N):
    """Two (2, n) inputs whose standard deviations differ 4 x: the other stream's scale moves
    most samples by more than a unit."""
    return [_noise(gpu, (2, n), 11100 + k, scale=s) + complex(0.25, -0.5) for k, s in enumerate((3.0, 12.0))]


def test_quantize_serial_reference_holds(gpu):
    """The allowance itself at this size: one call per input on the idle device."""
    from ska_pst_dsp_model_amd import layout
    for k, x in enumerate(_quantize_inputs(gpu)):
        _assert_quantized(layout.quantize(x, QUANT_RMS), x, QUANT_RMS, f"serial input {k}")


def _quantized_on_device(x, rms):
    """The oracle's quantisation of device tensor ``x`` as a device tensor."""
    import torch
    xh = x.cpu().numpy()
    return torch.from_numpy(orc.quantize(xh, orc.quantize_scale(xh, rms)).astype(np.complex64)).to(x.device)


def _quantize_diff(got, want):
    """(max |difference| of a component, fraction of components that differ), on the device."""
    import torch
    d = (torch.view_as_real(got) - torch.view_as_real(want)).abs()
    return float(d.max()), float((d > 0).float().mean())


def test_quantize_on_two_streams(gpu):
    """32 calls per stream, rms > 0, no scale asked for (so no call waits), dealt alternately
    from one host thread to two streams held behind a gate until all are enqueued: every output
    against the oracle.  With one moments block per device the calls summed into each other's
    moments and scaled by a wrong factor."""
    import torch
    from ska_pst_dsp_model_amd import layout
    xs = _quantize_inputs(gpu)
    want = [_quantized_on_device(x, QUANT_RMS) for x in xs]
    streams = [torch.cuda.Stream() for _ in xs]
    outs = [[torch.empty_like(x) for _ in range(QUANT_CALLS)] for x in xs]

    def deal(on):
        for i in range(QUANT_CALLS):
            for k, x in enumerate(xs):
                with torch.cuda.stream(on[k]):
                    layout.quantize(x, QUANT_RMS, out=outs[k][i])

    deal(streams)  # (each stream's first call allocates: not behind the gate)
    _, ref_ms = sh.timed(lambda: deal([torch.cuda.default_stream()] * len(xs)))
    for o in outs:
        for t in o:
            sh.poison_(t)
    torch.cuda.synchronize()
    gate = sh.Gate(ref_ms, streams, "quantize on two streams")
    deal(streams)
    gate.assert_pending()
    torch.cuda.synchronize()
    diffs = [_quantize_diff(outs[k][i], want[k]) for k in range(len(xs)) for i in range(QUANT_CALLS)]
    worst = (max(d[0] for d in diffs), max(d[1] for d in diffs))
    bad = sum(d[0] > 1.0 or d[1] >= 1e-4 for d in diffs)
    print(f"{bad} of {len(diffs)} calls outside the allowance; worst max |diff| {worst[0]:.3g}, "
          f"worst fraction differing {worst[1]:.3g}")
    assert bad == 0, (f"{bad} of {len(diffs)} calls outside the allowance; worst max |diff| {worst[0]:.3g}, "
                      f"worst fraction differing {worst[1]:.3g}")


@pytest.mark.parametrize("N,n,calls", [(8, QUANT_N, QUANT_CALLS), (256, 1 << 14, 8 * QUANT_CALLS)],
                         ids=["n8-2^20x32", "n256-2^14x256"])
def test_quantising_filterbanks_on_two_streams(gpu, monkeypatch, N, n, calls):
    """Two FilterBank objects with rndInput and rmsInput = 33.8, one per stream, dealt chunks
    alternately behind a gate: 32 chunks of 2^20 samples each through an 8-channel analysis, and
    the denser interleaving of 256 chunks of 2^14 samples through the 256-channel streaming
    kernel, whose launches are as short as the quantiser's.  What an object returns is the
    analysis of its quantised chunk, so the test takes the quantised chunk where the object's
    input hook hands it on: that must be the oracle's quantisation under the allowance, and
    the object's output the analysis of exactly that chunk, bit for bit."""
    import torch
    from ska_pst_dsp_model_amd import filterbank
    pfb = _pfb()
    taps = _taps(8, "8/7", 10) if N == 8 else _named_taps("c2")
    cfg = dict(analysis_function="polyphase_analysis", filt_coeff=taps, channels=N, os_factor="8/7",
               rndInput=True, rmsInput=QUANT_RMS)
    xs = _quantize_inputs(gpu, n)
    want = [_quantized_on_device(x, QUANT_RMS) for x in xs]
    fbs = [pfb.FilterBank(cfg) for _ in xs]
    twins = [pfb.FilterBank(dict(cfg, rndInput=False)) for _ in xs]
    streams = [torch.cuda.Stream() for _ in xs]
    seen = [[] for _ in xs]   # what each object's input hook returned, call by call
    hook = filterbank._quantize

    def spy(x, rms, device=0):
        y = hook(x, rms, device)
        seen[[torch.cuda.current_stream() == s for s in streams].index(True)].append(y)
        return y

    def deal(objs, on, res):
        for i in range(calls):
            for k, x in enumerate(xs):
                with torch.cuda.stream(on[k]):
                    res[k].append(objs[k].execute(x)[1])

    # The same calls on the same streams, not held back, twice: by the objects of the run below
    # on other samples (their buffers, the streams' moments blocks and allocator pools exist
    # afterwards), then by two more objects, timed: what the host needs to enqueue the calls
    # when every allocation is served from the streams' pools, as in the run below.  The hook
    # keeps the quantised chunks in these passes too, so the pools hold room for them.
    monkeypatch.setattr(filterbank, "_quantize", spy)
    flipped = [x.flip(1) for x in xs]
    for i in range(calls):
        for k in range(len(xs)):
            with torch.cuda.stream(streams[k]):
                fbs[k].execute(flipped[k])
    torch.cuda.synchronize()
    for fb in fbs:
        fb.reset()
    warm = [pfb.FilterBank(cfg) for _ in xs]
    for kept in seen:
        kept.clear()
    _, ref_ms = sh.timed(lambda: deal(warm, streams, [[] for _ in xs]))
    del warm
    for kept in seen:
        kept.clear()
    got = [[] for _ in xs]
    torch.cuda.synchronize()
    gate = sh.Gate(ref_ms, streams, "quantising FilterBanks on two streams")
    deal(fbs, streams, got)
    gate.assert_pending()
    torch.cuda.synchronize()
    monkeypatch.undo()
    bad, worst = 0, (0.0, 0.0)
    for k in range(len(xs)):
        assert len(seen[k]) == calls
        for i, q in enumerate(seen[k]):
            d = _quantize_diff(q, want[k])
            bad += d[0] > 1.0 or d[1] >= 1e-4
            worst = (max(worst[0], d[0]), max(worst[1], d[1]))
            assert sh.same_bits(got[k][i], twins[k].execute(q)[1]), (
                f"object {k} call {i}: not the analysis of the quantised chunk")
        assert fbs[k].buffered_samples == twins[k].buffered_samples
    print(f"{bad} of {2 * calls} calls outside the allowance; worst max |diff| {worst[0]:.3g}, "
          f"worst fraction differing {worst[1]:.3g}")
    assert bad == 0, (f"{bad} of {2 * calls} quantised chunks outside the allowance; worst max |diff| "
                      f"{worst[0]:.3g}, worst fraction differing {worst[1]:.3g}")


def test_quantize_does_not_wait_without_a_scale(gpu):
    """rms > 0 and no ``scale``: the call returns with the delay kernel still running."""
    import torch
    from ska_pst_dsp_model_amd import layout
    x = _quantize_inputs(gpu)[0]
    out = torch.empty_like(x)
    _, ref_ms = sh.timed(lambda: layout.quantize(x, QUANT_RMS))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):   # (the stream's first call allocates its moments block)
        layout.quantize(x.flip(1), QUANT_RMS, out=out)
    torch.cuda.synchronize()
    with sh.Delayed(ref_ms, "layout.quantize, no scale", stream=side) as d:
        layout.quantize(x, QUANT_RMS, out=out)
        d.assert_pending()
    d.stream.synchronize()
    _assert_quantized(out, x, QUANT_RMS, "after the delay")


@pytest.mark.parametrize("case", ["odd-n", "n-2", "scalar-path", "three-pols"])
def test_quantize_shapes(gpu, case):
    """Shapes no other test runs, rms > 0, against the oracle: an odd length, two samples, a
    polarisation stride that leaves the second row 8-byte but not 16-byte aligned (the scalar
    path of the moments and the rounding kernel, beside the vector path of row 0) and three
    polarisations."""
    import torch
    from ska_pst_dsp_model_amd import layout
    if case == "odd-n":
        x = _noise(gpu, (2, 100003), 11200, scale=5.0)
        got = layout.quantize(x, QUANT_RMS)
    elif case == "n-2":
        x = _noise(gpu, (1, 2), 11201, scale=5.0)
        got = layout.quantize(x, QUANT_RMS)
    elif case == "three-pols":
        x = _noise(gpu, (3, 70001), 11202, scale=5.0)
        got = layout.quantize(x, QUANT_RMS)
    else:
        n = 70000
        x = _noise(gpu, (2, n + 1), 11203, scale=5.0)[:, :n]
        out = torch.full((2, n + 1), sh.SENTINEL, dtype=torch.complex64, device=gpu)
        assert x.data_ptr() % 16 == 0 and (x.data_ptr() + 8 * x.stride(0)) % 16 == 8
        assert out.data_ptr() % 16 == 0 and out.stride(0) % 2 == 1
        got = layout.quantize(x, QUANT_RMS, out=out[:, :n])
        assert bool((out[:, n] == sh.SENTINEL).all())
    torch.cuda.synchronize()
    xh = x.cpu().numpy()
    sc = orc.quantize_scale(xh, QUANT_RMS)
    want = orc.quantize(xh, sc)
    d = np.abs(got.cpu().numpy() - want)
    # (n = 2: 1e-4 of four components is none)
    assert d.max() <= 1.0 and (d > 0).mean() < 1e-4, f"{case}: max |diff| {d.max()}, fraction {(d > 0).mean()}"
    _, dev_sc = layout.quantize(x, QUANT_RMS, return_scale=True)
    assert abs(dev_sc - sc) <= 1e-9 * sc


# ============================================================================ 4. one plan, two streams in turn
def _in_turn(what, make, call, xs, buffered):
    """``call(obj, x)`` for xs[0] on stream A behind the delay, then for xs[1] on stream B, which
    waits for an event recorded on A after the first call: the caller's ordering.  Both results
    equal the serial ones."""
    import torch
    ref_obj = make()
    ref, ref_ms = sh.timed(lambda: [call(ref_obj, x).clone() for x in xs])
    obj = make()
    for x in xs:
        call(obj, sh.scrambled(x))
    torch.cuda.synchronize()
    obj.reset()
    inp = [sh.poison_(torch.empty_like(x)) for x in xs]
    torch.cuda.synchronize()
    b = torch.cuda.Stream()
    done = torch.cuda.Event()
    with sh.Delayed(ref_ms, what) as d:
        inp[0].copy_(xs[0])
        inp[1].copy_(xs[1])
        got = [call(obj, inp[0]).clone()]
        done.record(d.stream)
        with torch.cuda.stream(b):
            b.wait_event(done)
            got.append(call(obj, inp[1]).clone())
        d.assert_pending()
    torch.cuda.synchronize()
    for k, (g, r) in enumerate(zip(got, ref)):
        assert sh.same_bits(g, r), f"{what}: call {k}"
    assert buffered(obj) == buffered(ref_obj) > 0


def test_one_analysis_plan_on_two_streams_in_turn(gpu):
    xs = [_noise(gpu, (2, n), 11300 + n) for n in (70000, 40000)]
    _in_turn("analysis plan in turn", lambda: _c2_analysis(2), lambda p, x: p.execute(x, stateful=True), xs,
             lambda p: p.buffered_samples)


def test_one_synthesis_plan_on_two_streams_in_turn(gpu):
    xs = [_noise(gpu, (2, n, 256), 11310 + n) for n in (1000, 5000)]
    _in_turn("synthesis plan in turn", lambda: _c2_synthesis(2),
             lambda p, x: p.execute(x, stateful=True, layout="ptc"), xs, lambda p: p.buffered_samples)


# ============================================================================ 5. graph capture
def _captured(what, plan, call, inputs):
    """Warm-up, capture on a side stream (as test_roundtrip_graph_capture), two replays with
    the input's contents changed in place before each: every replay equals the eager call on
    that input.  ``call(x)`` -> the tensor written; the captured call's result is the graph's
    own static output."""
    import torch
    eager = [call(x).clone() for x in inputs]
    x = inputs[0].clone()
    call(x)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = call(x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in (1, 2):
        x.copy_(inputs[k])
        sh.poison_(out)
        g.replay()
        torch.cuda.synchronize()
        assert sh.same_bits(out, eager[k]), f"{what}: replay {k}"
    del g
    plan.close()


GRAPH_ANALYSIS = ["execute", "execute_dada", "execute_to_dada", "execute_dada_to_dada"]


@pytest.mark.parametrize("entry", GRAPH_ANALYSIS)
def test_analysis_entries_replay_from_a_graph(gpu, entry):
    """The stateless device entries of the 256-channel streaming analysis plan: one launch on
    the given stream, no allocation, synchronisation or read-back in the host path."""
    plan = _c2_analysis(2)
    n = 13 * 256 + 100 * 224 + 9
    if entry in ("execute", "execute_to_dada"):
        inputs = [_noise(gpu, (2, n), 11400 + k) for k in range(3)]
    else:
        inputs = [_series_section(gpu, 16, n, 2, 11410 + k) for k in range(3)]
    scale = 1.0 / 64
    call = {"execute": lambda x: plan.execute(x),
            "execute_dada": lambda x: plan.execute_dada(x, 16),
            "execute_to_dada": lambda x: plan.execute_to_dada(x, 32, scale=scale),
            "execute_dada_to_dada": lambda x: plan.execute_dada_to_dada(x, 16, 32, scale=scale)}[entry]
    _captured(f"AnalysisPlan.{entry}", plan, call, inputs)


GRAPH_SYNTHESIS = ["execute", "execute_view", "execute_dada", "execute_to_dada", "execute_dada_to_dada"]


@pytest.mark.parametrize("entry", GRAPH_SYNTHESIS)
def test_synthesis_entries_replay_from_a_graph(gpu, entry):
    """The stateless device entries of the 256-channel wave synthesis plan (channel IFFT into
    the plan's scratch, sized by the warm-up call, then the wave kernel)."""
    import torch
    plan = _c2_synthesis(2)
    rows = 576
    if entry in ("execute", "execute_to_dada"):
        inputs = [_noise(gpu, (2, rows, 256), 11420 + k) for k in range(3)]
    elif entry == "execute_view":
        inputs = [_noise(gpu, (2, rows, 264), 11430 + k) for k in range(3)]
    else:
        inputs = [_rows_section(gpu, 16, rows, 256, 2, 11440 + k) for k in range(3)]
    out = torch.empty((2, 3 * plan.output_keep), dtype=torch.complex64, device=gpu)
    scale = 64.0
    call = {"execute": lambda x: plan.execute(x, layout="ptc", out=out),
            "execute_view": lambda x: plan.execute_view(x[:, :, 4:260], out=out),
            "execute_dada": lambda x: plan.execute_dada(x, 16, out=out),
            "execute_to_dada": lambda x: plan.execute_to_dada(x, 32, scale=scale, layout="ptc"),
            "execute_dada_to_dada": lambda x: plan.execute_dada_to_dada(x, 16, 32, scale=scale)}[entry]
    _captured(f"SynthesisPlan.{entry}", plan, call, inputs)
