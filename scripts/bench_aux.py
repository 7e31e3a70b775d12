"""Secondary measurements (not the bench.py headline): every other kernel of the path on
one MI355X, as algorithmic HBM bytes / time against the 8 TB/s peak.

  * C3 SKA-Mid padded round trip (4096 ch, 8/7, 100 353 taps, 2^26 samples)
  * C2' reference 'low' parity variant (256 ch, 4/3)
  * LowCBF PST filterbank (polyphase_analysis_lowcbf, 2^24 samples x 2 pol)
  * DADA unpack (NBIT 8 / 32) and pack, corner turn, channel gather, quantisation
  * two-stage analysis cascade (256 x 256 ch; stage 2 batched over 256 series)
  * --only-dada: synthesis from a DADA section at the C2 shape, the staged pair
    (pfb_dada_unpack + pfb_synthesis_execute) against pfb_synthesis_execute_dada, interleaved
  * --only-dada-analysis: analysis from a single-channel DADA section (C2, LowCBF, SKA-Mid
    stage 1), the staged pair (pfb_dada_unpack + pfb_analysis_execute) against
    pfb_analysis_execute_dada, interleaved
  * --only-dada-output: analysis into a DADA section (C2, LowCBF, SKA-Mid stage 1), the pair
    (execute, scale, pfb_dada_pack) against pfb_analysis_execute_to_dada /
    pfb_analysis_execute_dada_to_dada, interleaved
  * --only-dada-synthesis-output: synthesis into a DADA section at the C2 shape, the pair
    (pfb_synthesis_execute[_dada], scale, pfb_dada_pack) against pfb_synthesis_execute_to_dada /
    pfb_synthesis_execute_dada_to_dada, interleaved, and the cf32 synthesis alone
  * --only-dada-roundtrip: the round trip from a single-channel DADA section into the
    channelised and the output sections at the C2 unit, the sequence (pfb_dada_unpack,
    pfb_roundtrip_execute, packs) against pfb_roundtrip_execute_dada_to_dada, interleaved, and
    the two halves pipelined over two streams
  * --only-quantised-output: the FilterBank's rms-scaled, rounded output as a DADA section at the
    C2 shape, what the object enqueues today (execute, pfb_quantize, the copy, pfb_dada_pack)
    against pfb_analysis_execute_quantised_to_dada in AUTO and in STAGED mode and the plain
    pfb_analysis_execute_to_dada as the floor, interleaved
  * --only-quantised-input: the FilterBank's rms-scaled, rounded input at the C2 shape, what the
    object enqueues today (pfb_dada_unpack, pfb_quantize, pfb_analysis_execute) against the same
    call with the plan's input quantiser in AUTO and in STAGED mode and with the quantiser off as
    the floor, interleaved
  * --only-twostage-inverse: TwoStageInverseFilterBank with the channel gather against the
    strided input (pfb_inverse_filterbank_execute_strided), interleaved

Prints one JSON object per line.  Usage: python scripts/bench_aux.py [--reps N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "ska-pst-dsp-model_amd"), REPO]
PEAK = 8000.0


def timeit(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def emit(name, ms, alg_bytes, **kw):
    gbs = alg_bytes / (ms * 1e-3) / 1e9
    print(json.dumps({"kernel": name, "ms": round(ms, 4), "alg_bytes": int(alg_bytes),
                      "GB/s": round(gbs, 1), "frac": round(gbs / PEAK, 4), **kw}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-mid", action="store_true")
    ap.add_argument("--only-mid", action="store_true")
    ap.add_argument("--only-twostage", action="store_true")
    ap.add_argument("--only-dada", action="store_true",
                    help="the dada_synthesis A/B alone (--reps: calls per timed window)")
    ap.add_argument("--only-dada-analysis", action="store_true",
                    help="the dada_analysis A/B alone (--reps: calls per timed window)")
    ap.add_argument("--only-dada-output", action="store_true",
                    help="the dada_output A/B alone (--reps: calls per timed window)")
    ap.add_argument("--parent-lib", default=None,
                    help="with --only-dada-output: a libpfb_hip.so built from the parent commit; its to-DADA "
                         "call is timed as a third side P of the SKA-Mid rows")
    ap.add_argument("--only-dada-synthesis-output", action="store_true",
                    help="the dada_synthesis_output A/B alone (--reps: calls per timed window)")
    ap.add_argument("--only-dada-roundtrip", action="store_true",
                    help="the dada_roundtrip A/B alone (--reps: calls per timed window)")
    ap.add_argument("--only-quantised-output", action="store_true",
                    help="the quantised_output A/B alone (--reps: calls per timed window, at least 20; "
                         "--rounds: windows, at least 9)")
    ap.add_argument("--only-quantised-input", action="store_true",
                    help="the quantised_input A/B alone (--reps: calls per timed window, at least 20; "
                         "--rounds: windows, at least 9; --sides A: side A alone, for the parent commit's library)")
    ap.add_argument("--sides", default="A,B,Bs,floor", help="with --only-quantised-input: the sides to run")
    ap.add_argument("--only-twostage-inverse", action="store_true",
                    help="the inverse cascade's gather vs strided-input A/B alone (--reps: calls per window)")
    ap.add_argument("--rounds", type=int, default=15,
                    help="--only-dada / --only-dada-analysis / --only-twostage-inverse: interleaved A/B "
                         "windows per case")
    ap.add_argument("--padded-cascade", default="default",
                    choices=["default", "strided", "no-stage1", "no-stage2", "gather"],
                    help="the SKA-Mid padded cascade's stores: the library default; both stages strided; "
                         "stage 1 through the corner turn (channel-major off); stage 2 through the gather "
                         "(chomp off); or both off (TwoStageFilterBank.strided_stages)")
    ap.add_argument("--inflight", type=int, default=1, help="C3 units in flight (plan pairs/streams)")
    ap.add_argument("--graph", type=int, default=1, help="with --pipeline: capture the steps as one graph")
    ap.add_argument("--pipeline", type=int, default=0,
                    help="with --inflight > 1: the split round trip pipelined over two streams")
    ap.add_argument("--cpu", action="store_true",
                    help="also time the NumPy oracle (1 core) on bounded samples of each config")
    args = ap.parse_args()
    import torch
    import ska_pst_dsp_model_amd as pfb
    from ska_pst_dsp_model_amd import layout
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)

    def noise(*shape):
        return torch.complex(torch.randn(shape, device=dev, generator=g),
                             torch.randn(shape, device=dev, generator=g)).to(torch.complex64)

    if args.cpu:
        cpu_baselines(pfb)
    if args.only_mid:
        return mid(torch, pfb, noise, dev, reps=args.reps, inflight=args.inflight, pipeline=bool(args.pipeline),
                   graph=bool(args.graph))
    if args.only_twostage:
        return twostage(torch, pfb, noise, args.reps, args.padded_cascade)
    if args.only_dada:
        return dada_synthesis(torch, pfb, dev, max(args.reps, 20), args.rounds)
    if args.only_dada_analysis:
        return dada_analysis(torch, pfb, dev, max(args.reps, 20), args.rounds)
    if args.only_dada_output:
        return dada_output(torch, pfb, dev, max(args.reps, 20), args.rounds, args.parent_lib)
    if args.only_dada_synthesis_output:
        return dada_synthesis_output(torch, pfb, dev, max(args.reps, 20), args.rounds)
    if args.only_dada_roundtrip:
        return dada_roundtrip(torch, pfb, dev, max(args.reps, 20), args.rounds)
    if args.only_quantised_output:
        return quantised_output(torch, pfb, dev, max(args.reps, 20), max(args.rounds, 9))
    if args.only_quantised_input:
        return quantised_input(torch, pfb, dev, max(args.reps, 20), max(args.rounds, 9),
                               tuple(args.sides.split(",")))
    if args.only_twostage_inverse:
        return twostage_inverse(torch, pfb, noise, max(args.reps, 20), max(args.rounds, 5))
    # ---- C2' (4/3) round trip
    taps43 = pfb.design_PFB_FIR_filter(256, "4/3", 12)
    n = 1 << 24
    x = noise(1, n)
    ana = pfb.AnalysisPlan(taps43, 256, "4/3", "polyphase_analysis", 1)
    win = pfb.PFBWindow().lookup["tukey"](256, 48)
    syn = pfb.SynthesisPlan(256, "4/3", 256, 48, True, 1, True, taps43, win, None, 1)
    K = ana.output_length(n)
    chan = torch.empty((1, K, 256), dtype=torch.complex64, device=dev)
    out = torch.empty((1, syn.output_length(K)), dtype=torch.complex64, device=dev)
    ms = timeit(torch, lambda: pfb.roundtrip(ana, syn, x, chan=chan, out=out), args.reps)
    emit("roundtrip C2' 256ch 4/3", ms, 16 * (1 + 4 / 3) * n,
         msamples_per_s=round(n / ms / 1e3, 1))

    # ---- LowCBF PST filterbank
    taps_pst = pfb.read_fir_filter_coeff(os.path.join(pfb.config.config_dir, "PST_filtertaps.txt"))
    x2 = noise(2, n)
    low = pfb.AnalysisPlan(taps_pst, 256, "4/3", "polyphase_analysis_lowcbf", 2)
    low.execute(x2)  # consume the one-time padding
    Kl = low.output_length(n)
    ms = timeit(torch, lambda: low.execute(x2), args.reps)
    emit("lowcbf_kernel (PSTFilterbank)", ms, 2 * (8 * n + 8 * 216 * Kl),
         msamples_per_s=round(2 * n / ms / 1e3, 1))

    # ---- layout kernels
    raw8 = torch.randint(-128, 127, (2 * 2 * n,), dtype=torch.int8, device=dev)
    ms = timeit(torch, lambda: layout.dada_unpack(raw8, 8, 2, 1, 2), args.reps)
    emit("dada_unpack NBIT8 2pol", ms, raw8.numel() + 2 * n * 8)
    raw32 = torch.randn((2 * 2 * n,), device=dev)
    ms = timeit(torch, lambda: layout.dada_unpack(raw32, 32, 2, 1, 2), args.reps)
    emit("dada_unpack NBIT32 2pol", ms, raw32.numel() * 4 + 2 * n * 8)
    y = noise(2, n, 1)
    ms = timeit(torch, lambda: layout.dada_pack(y, 32), args.reps)
    emit("dada_pack NBIT32 2pol", ms, 2 * 2 * n * 8)
    rows = noise(1 << 16, 256)
    ms = timeit(torch, lambda: layout.corner_turn(rows), args.reps)
    emit("corner_turn 65536x256", ms, 2 * rows.numel() * 8)
    ms = timeit(torch, lambda: layout.gather_channels(rows, 16, 16, 256, 1 << 16, 16), args.reps)
    emit("gather_channels 16x16", ms, 2 * rows.numel() * 8)
    ms = timeit(torch, lambda: layout.quantize(y, 33.8), args.reps)
    emit("quantize (moments + round)", ms, 3 * y.numel() * 8)

    # ---- two-stage analysis: 256 ch, then 256 ch over each (batched)
    twostage(torch, pfb, noise, 3)

    # ---- C3 SKA-Mid padded round trip
    if not args.skip_mid:
        del x, x2, raw8, raw32, y, rows, chan, out
        torch.cuda.empty_cache()
        mid(torch, pfb, noise, dev)


def twostage(torch, pfb, noise, reps, padded_cascade="default"):
    taps87 = pfb.design_PFB_FIR_filter(256, "8/7", 12)
    cfg = dict(analysis_function="polyphase_analysis", filt_coeff=taps87, channels=256,
               os_factor="8/7")
    ts = pfb.TwoStageFilterBank(cfg)
    xs = noise(1, 1, 1 << 24)
    ts.execute(xs)
    ts2 = pfb.TwoStageFilterBank(cfg)
    ms = timeit(torch, lambda: ts2.execute(xs), reps)
    emit("TwoStageFilterBank 256x256 (stream call)", ms, 16 * (1 + 8 / 7) * (1 << 24),
         msamples_per_s=round((1 << 24) / ms / 1e3, 1),
         note="bytes: the two analyses' input+output; strided stores, no corner turn / gather")
    ts3 = pfb.TwoStageFilterBank(cfg)
    ts3.strided = False
    ts3.execute(xs)
    ms = timeit(torch, lambda: ts3.execute(xs), reps)
    emit("TwoStageFilterBank 256x256 (corner turn + gather path)", ms, 16 * (1 + 8 / 7) * (1 << 24),
         msamples_per_s=round((1 << 24) / ms / 1e3, 1),
         note="bytes: the two analyses' input+output, excluding the corner turn and gather")
    del xs, ts, ts2, ts3
    # BASELINE configs[2]'s cascade: both stages polyphase_analysis_padded (test.config.json
    # `mid`, TwoStageFilterBank.m:27,51-52) — the SKA-Mid stage 1 (4096 ch, 8/7, 100 353 taps)
    # into a 16-ch padded stage 2 over every coarse channel, critical, one 2^26-sample unit
    taps1 = pfb.design_PFB_FIR_filter_two_stage(4096, "8/7", 28)
    taps2 = pfb.design_PFB_FIR_filter(16, "8/7", 10)

    def pcfg(t, n):
        return dict(analysis_function="polyphase_analysis_padded", filt_coeff=t, channels=n, os_factor="8/7")
    nm = 1 << 26
    xm = noise(1, 1, nm)
    tm = pfb.TwoStageFilterBank(pcfg(taps1, 4096)).set_stage2_config(pcfg(taps2, 16))
    tm.critical = 1
    stages = {"strided": [True, True], "no-stage1": [False, True], "no-stage2": [True, False],
              "gather": [False, False]}.get(padded_cascade)
    if stages is not None:
        tm.strided_stages = stages
    tm.execute(xm)
    ms = timeit(torch, lambda: tm.execute(xm), reps)
    emit("TwoStageFilterBank SKA-Mid 4096x16 padded (stream call)", ms, 16 * (1 + 8 / 7) * nm,
         msamples_per_s=round(nm / ms / 1e3, 1),
         note="both stages polyphase_analysis_padded; bytes: the two analyses' input+output",
         **({} if stages is None else {"padded_cascade": padded_cascade}))
    del xm, tm


def dada_synthesis(torch, pfb, dev, reps, rounds):
    """DADA section -> series at the C2 synthesis shape (256 ch, 8/7, Nf 256, Ov 48, tukey,
    deripple; the rows of a 2^24-sample unit).  A: pfb_dada_unpack into a cf32 buffer, then
    pfb_synthesis_execute (the calls a caller had before).  B: pfb_synthesis_execute_dada.
    The outputs are asserted equal first; then `rounds` windows of `reps` calls of each side,
    alternating A and B in one process, after a warm-up of both.  One line per case with the
    median, min, max and quartiles of each side's per-call time over the windows."""
    from ctypes import c_void_p
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    N, rows = 256, ((1 << 24) // 224) // 32 * 32     # whole LowCBF heaps: 74 880 rows
    taps = pfb.design_PFB_FIR_filter(N, "8/7", 12)
    win = pfb.PFBWindow().lookup["tukey"](256, 48)
    g = torch.Generator(device=dev).manual_seed(2)
    for n_pol in (1, 2):
        syn = pfb.SynthesisPlan(N, "8/7", 256, 48, True, 1, True, taps, win, None, n_pol)
        out_a = torch.empty((n_pol, syn.output_length(rows)), dtype=torch.complex64, device=dev)
        out_b = torch.empty_like(out_a)
        x = torch.empty((n_pol, rows, N), dtype=torch.complex64, device=dev)
        for nbit, lowcbf in ((16, False), (16, True), (8, False)):
            dt = torch.int16 if nbit == 16 else torch.int8
            lim = 1 << (nbit - 1)
            raw = torch.randint(-lim, lim, (rows * N * n_pol * 2,), dtype=dt, device=dev, generator=g)
            order = _lib.PFB_DADA_LOWCBF if lowcbf else _lib.PFB_DADA_TFP
            stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)

            def side_a():
                _lib.check(lib.pfb_dada_unpack(c_void_p(raw.data_ptr()), nbit, 2, order, rows, N, n_pol,
                                               c_void_p(x.data_ptr()), rows * N, stream))
                syn.execute(x, layout="ptc", out=out_a)

            def side_b():
                syn.execute_dada(raw, nbit, lowcbf=lowcbf, out=out_b)

            side_a()
            side_b()
            path = syn.last_dada_input()
            torch.cuda.synchronize()
            assert torch.equal(out_a, out_b), f"dada_synthesis {nbit} lowcbf={lowcbf}: outputs differ"
            for _ in range(2):
                timeit(torch, side_a, reps)
                timeit(torch, side_b, reps)
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(timeit(torch, side_a, reps))
                tb.append(timeit(torch, side_b, reps))

            def stats(t):
                q = np.percentile(t, [0, 25, 50, 75, 100])
                return {k: round(float(v), 4) for k, v in zip(("min", "q25", "median", "q75", "max"), q)}
            a, b = stats(ta), stats(tb)
            samples = rows * N * n_pol
            print(json.dumps({
                "kernel": "dada_synthesis", "shape": "256ch 8/7 Nf256 Ov48 tukey deripple", "rows": rows,
                "n_pol": n_pol, "nbit": nbit, "order": "lowcbf" if lowcbf else "tfp", "path": path,
                "calls_per_window": reps, "windows": rounds, "outputs_equal": True,
                "A_unpack_then_execute_ms": a, "B_execute_dada_ms": b,
                "A_spread_ms": round(a["max"] - a["min"], 4),
                "B_below_A_by_ms": round(a["median"] - b["median"], 4),
                "B_over_A": round(b["median"] / a["median"], 4),
                "A_first_pass_bytes_per_sample": 2 * nbit // 8 + 8 + 8,
                "B_first_pass_bytes_per_sample": 2 * nbit // 8,
                "samples": samples}), flush=True)
        del syn, out_a, out_b, x


def dada_analysis(torch, pfb, dev, reps, rounds):
    """Single-channel DADA section (TFP, pols interleaved) -> channelised product.  A:
    pfb_dada_unpack into a packed cf32 [pol][t] buffer, then pfb_analysis_execute (the calls a
    caller had before).  B: pfb_analysis_execute_dada.  Both through the C ABI into
    preallocated buffers.  The outputs are asserted equal first; then `rounds` windows of `reps`
    calls of each side, alternating A and B in one process, after a warm-up of both.  One line
    per case with the median, min, max and quartiles of each side's per-call time."""
    from ctypes import byref, c_int64, c_void_p
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(3)
    taps87 = pfb.design_PFB_FIR_filter(256, "8/7", 12)
    taps_pst = pfb.read_fir_filter_coeff(os.path.join(pfb.config.config_dir, "PST_filtertaps.txt"))
    # (the SKA-Mid stage 1's tap count; the values do not bear on the time)
    taps_mid = np.random.default_rng(4).standard_normal(4096 * 24 + 2049) / 4096
    cases = [("C2 256ch 8/7", taps87, 256, "8/7", "polyphase_analysis", 1 << 24, nbit, n_pol)
             for nbit in (8, 16, 32) for n_pol in (1, 2)]
    cases.append(("LowCBF PST filterbank", taps_pst, 256, "4/3", "polyphase_analysis_lowcbf", 1 << 24, 8, 2))
    cases.append(("SKA-Mid stage 1 4096ch 8/7 padded", taps_mid, 4096, "8/7", "polyphase_analysis_padded",
                  1 << 26, 16, 1))
    dts = {8: torch.int8, 16: torch.int16}
    for shape, taps, N, os_, variant, n, nbit, n_pol in cases:
        plan = pfb.AnalysisPlan(taps, N, os_, variant, n_pol)
        if variant.endswith("lowcbf"):
            plan.execute(torch.zeros((n_pol, 4096), dtype=torch.complex64, device=dev))  # the one-time padding
        K, C = plan.output_length(n), plan.out_chan
        if nbit == 32:
            raw = torch.randn((n * n_pol * 2,), device=dev, generator=g)
        else:
            lim = 1 << (nbit - 1)
            raw = torch.randint(-lim, lim, (n * n_pol * 2,), dtype=dts[nbit], device=dev, generator=g)
        x = torch.empty((n_pol, n), dtype=torch.complex64, device=dev)
        out_a = torch.empty((n_pol, K, C), dtype=torch.complex64, device=dev)
        out_b = torch.empty_like(out_a)
        stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n_out = c_int64(0)

        def side_a():
            _lib.check(lib.pfb_dada_unpack(c_void_p(raw.data_ptr()), nbit, 2, _lib.PFB_DADA_TFP, n, 1, n_pol,
                                           c_void_p(x.data_ptr()), n, stream))
            _lib.check(lib.pfb_analysis_execute(plan._h, c_void_p(x.data_ptr()), n, n, c_void_p(out_a.data_ptr()),
                                                K * C, K, byref(n_out), _lib.PFB_MEM_DEVICE, stream))

        def side_b():
            _lib.check(lib.pfb_analysis_execute_dada(plan._h, c_void_p(raw.data_ptr()), nbit, 2, _lib.PFB_DADA_TFP,
                                                     n, c_void_p(out_b.data_ptr()), K * C, K, byref(n_out),
                                                     stream))

        side_a()
        side_b()
        path = plan.last_dada_input()
        torch.cuda.synchronize()
        assert n_out.value == K and torch.equal(out_a, out_b), f"dada_analysis {shape} {nbit}: outputs differ"
        for _ in range(2):
            timeit(torch, side_a, reps)
            timeit(torch, side_b, reps)
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timeit(torch, side_a, reps))
            tb.append(timeit(torch, side_b, reps))

        def stats(t):
            q = np.percentile(t, [0, 25, 50, 75, 100])
            return {k: round(float(v), 4) for k, v in zip(("min", "q25", "median", "q75", "max"), q)}
        a, b = stats(ta), stats(tb)
        esz = 2 * nbit // 8
        print(json.dumps({
            "kernel": "dada_analysis", "shape": shape, "samples": n, "n_pol": n_pol, "nbit": nbit, "path": path,
            "calls_per_window": reps, "windows": rounds, "outputs_equal": True,
            "A_unpack_then_execute_ms": a, "B_execute_dada_ms": b,
            "A_spread_ms": round(a["max"] - a["min"], 4),
            "B_below_A_by_ms": round(a["median"] - b["median"], 4),
            "B_over_A": round(b["median"] / a["median"], 4),
            "stays_fused": bool(a["median"] - b["median"] > a["max"] - a["min"]),
            "A_bytes": int(n_pol * (n * (esz + 8 + 8) + K * C * 8)),
            "B_bytes": int(n_pol * (n * esz + K * C * 8))}), flush=True)
        del plan, raw, x, out_a, out_b
        torch.cuda.empty_cache()


def dada_output(torch, pfb, dev, reps, rounds, parent_lib=None):
    """Channelised product -> DADA section (TFP, NBIT 8 / 16 / 32).  A: the pair a caller had
    before — the cf32-output call (pfb_analysis_execute, or pfb_analysis_execute_dada for a
    DADA input), both components times the scale in float32 (one elementwise pass), then
    pfb_dada_pack.  B: pfb_analysis_execute_to_dada / pfb_analysis_execute_dada_to_dada.  Both
    through the C ABI into preallocated buffers.  The sections are asserted equal first; then
    `rounds` windows of `reps` calls of each side, alternating A and B in one process, after a
    warm-up of both.  One line per case with the median, min, max and quartiles of each side's
    per-call time.  stays_fused: B's median lies below A's by more than the larger of the two
    sides' interquartile spreads.
    The SKA-Mid rows (the 4096-point row FFT storing the section) have a second comparison side
    when `parent_lib` names a library built from the parent commit: P, that library's own to-DADA
    call on a plan of its own (what a caller of the same entry point had before), alternated with
    A and B in the same windows; those rows stay fused only if B lies below both A and P by more
    than the largest interquartile spread of the three."""
    from ctypes import byref, c_int64, c_void_p
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    plib = _lib.load(parent_lib) if parent_lib else None
    g = torch.Generator(device=dev).manual_seed(5)
    taps87 = pfb.design_PFB_FIR_filter(256, "8/7", 12)
    taps_pst = pfb.read_fir_filter_coeff(os.path.join(pfb.config.config_dir, "PST_filtertaps.txt"))
    # (the SKA-Mid stage 1's tap count; the values do not bear on the time)
    taps_mid = np.random.default_rng(4).standard_normal(4096 * 24 + 2049) / 4096
    c2 = ("C2 256ch 8/7", taps87, 256, "8/7", "polyphase_analysis", 1 << 24)
    # (shape..., input NBIT or 0 for cf32, output NBIT, n_pol)
    cases = [c2 + (0, nbit, n_pol) for nbit in (8, 16, 32) for n_pol in (1, 2)]
    cases += [c2 + (nbit, nbit, n_pol) for nbit in (16, 8) for n_pol in (1, 2)]
    cases.append(("LowCBF PST filterbank", taps_pst, 256, "4/3", "polyphase_analysis_lowcbf", 1 << 24, 16, 16, 2))
    mid = ("SKA-Mid stage 1 4096ch 8/7 padded", taps_mid, 4096, "8/7", "polyphase_analysis_padded", 1 << 26)
    cases += [mid + c for c in ((0, 16, 1), (0, 16, 2), (0, 8, 1), (0, 32, 1), (16, 16, 1))]
    dts = {8: torch.int8, 16: torch.int16, 32: torch.float32}
    for shape, taps, N, os_, variant, n, in_nbit, nbit, n_pol in cases:
        plan = pfb.AnalysisPlan(taps, N, os_, variant, n_pol)
        if variant.endswith("lowcbf"):
            plan.execute(torch.zeros((n_pol, 4096), dtype=torch.complex64, device=dev))  # the one-time padding
        K, C = plan.output_length(n), plan.out_chan
        if in_nbit:
            lim = 1 << (in_nbit - 1)
            src = torch.randint(-lim, lim, (n * n_pol * 2,), dtype=dts[in_nbit], device=dev, generator=g)
        else:
            src = torch.view_as_complex(torch.randn((n_pol, n, 2), device=dev, generator=g))
        cf = torch.empty((n_pol, K, C), dtype=torch.complex64, device=dev)
        scaled = torch.empty_like(cf)
        sec_a = torch.empty((K, C, n_pol, 2), dtype=dts[nbit], device=dev)
        sec_b = torch.empty_like(sec_a)
        nbytes = sec_b.numel() * sec_b.element_size()
        stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n_out = c_int64(0)

        def execute_cf32():
            if in_nbit:
                _lib.check(lib.pfb_analysis_execute_dada(plan._h, c_void_p(src.data_ptr()), in_nbit, 2,
                                                         _lib.PFB_DADA_TFP, n, c_void_p(cf.data_ptr()), K * C, K,
                                                         byref(n_out), stream))
            else:
                _lib.check(lib.pfb_analysis_execute(plan._h, c_void_p(src.data_ptr()), n, n, c_void_p(cf.data_ptr()),
                                                    K * C, K, byref(n_out), _lib.PFB_MEM_DEVICE, stream))

        # the product's component rms at a third of the integer range (0.37 for NBIT 32)
        execute_cf32()
        rms = float(torch.view_as_real(cf).square().mean().sqrt())
        scale = float(np.float32((((1 << (nbit - 1)) - 1) / 3.0 if nbit != 32 else 0.37) / rms))

        def side_a():
            execute_cf32()
            torch.mul(torch.view_as_real(cf), scale, out=torch.view_as_real(scaled))
            _lib.check(lib.pfb_dada_pack(c_void_p(scaled.data_ptr()), K * C, K, C, n_pol, c_void_p(sec_a.data_ptr()),
                                         nbit, stream))

        def side_b():
            if in_nbit:
                _lib.check(lib.pfb_analysis_execute_dada_to_dada(
                    plan._h, c_void_p(src.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, n, c_void_p(sec_b.data_ptr()),
                    nbit, scale, nbytes, byref(n_out), stream))
            else:
                _lib.check(lib.pfb_analysis_execute_to_dada(plan._h, c_void_p(src.data_ptr()), n, n,
                                                            c_void_p(sec_b.data_ptr()), nbit, scale, nbytes,
                                                            byref(n_out), stream))

        # P: the parent commit's library, its own plan and section
        side_p, pplan, sec_p = None, None, None
        if plib is not None and N == 4096:
            arr, ptr = _lib.c_double_array(plan.taps)
            desc = _lib.AnalysisDesc(_lib.PFB_ANALYSIS_PADDED, N, plan.os_factor.nu, plan.os_factor.de, ptr, len(arr),
                                     n_pol, 0)
            pplan = c_void_p()
            assert plib.pfb_analysis_plan_create(byref(desc), byref(pplan)) == 0, plib.pfb_last_error()
            sec_p = torch.empty_like(sec_a)

            def side_p():
                if in_nbit:
                    st = plib.pfb_analysis_execute_dada_to_dada(
                        pplan, c_void_p(src.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, n, c_void_p(sec_p.data_ptr()),
                        nbit, scale, nbytes, byref(n_out), stream)
                else:
                    st = plib.pfb_analysis_execute_to_dada(pplan, c_void_p(src.data_ptr()), n, n,
                                                           c_void_p(sec_p.data_ptr()), nbit, scale, nbytes,
                                                           byref(n_out), stream)
                assert st == 0, plib.pfb_last_error()

        side_a()
        side_b()
        path_in, path = plan.last_dada_input(), plan.last_dada_output()
        torch.cuda.synchronize()
        assert n_out.value == K and torch.equal(sec_a, sec_b), f"dada_output {shape} {in_nbit}->{nbit}: sections differ"
        sides = [side_a, side_b]
        parent_path = None
        if side_p:
            side_p()
            torch.cuda.synchronize()
            parent_path = {0: "none", 1: "fused", 2: "staged"}[int(plib.pfb_analysis_last_dada_output(pplan))]
            assert n_out.value == K and torch.equal(sec_a, sec_p), f"dada_output {shape}: the parent's section differs"
            sides.append(side_p)
        for _ in range(2):
            for f in sides:
                timeit(torch, f, reps)
        times = [[] for _ in sides]
        for _ in range(rounds):
            for t, f in zip(times, sides):
                t.append(timeit(torch, f, reps))
        ta, tb = times[0], times[1]

        def stats(t):
            q = np.percentile(t, [0, 25, 50, 75, 100])
            return {k: round(float(v), 4) for k, v in zip(("min", "q25", "median", "q75", "max"), q)}
        a, b = stats(ta), stats(tb)
        iqr_a, iqr_b = a["q75"] - a["q25"], b["q75"] - b["q25"]
        esz_in, esz = (2 * in_nbit // 8 if in_nbit else 8), 2 * nbit // 8
        prod = K * C * 8
        extra = {}
        stays = bool(path == "fused" and a["median"] - b["median"] > max(iqr_a, iqr_b))
        if side_p:
            pst = stats(times[2])
            iqr = max(iqr_a, iqr_b, pst["q75"] - pst["q25"])
            stays = bool(path == "fused" and min(a["median"], pst["median"]) - b["median"] > iqr)
            extra = {"P_parent_execute_to_dada_ms": pst, "P_iqr_ms": round(pst["q75"] - pst["q25"], 4),
                     "parent_path": parent_path, "B_below_P_by_ms": round(pst["median"] - b["median"], 4),
                     "B_over_P": round(b["median"] / pst["median"], 4)}
            plib.pfb_analysis_plan_destroy(pplan)
        print(json.dumps({
            "kernel": "dada_output", "shape": shape, "samples": n, "n_pol": n_pol,
            "in": f"nbit{in_nbit}" if in_nbit else "cf32", "nbit": nbit, "path": path, "input_path": path_in,
            "calls_per_window": reps, "windows": rounds, "outputs_equal": True,
            "A_execute_scale_pack_ms": a, "B_execute_to_dada_ms": b,
            "A_iqr_ms": round(iqr_a, 4), "B_iqr_ms": round(iqr_b, 4),
            "A_spread_ms": round(a["max"] - a["min"], 4),
            "B_below_A_by_ms": round(a["median"] - b["median"], 4),
            "B_over_A": round(b["median"] / a["median"], 4),
            "stays_fused": stays, **extra,
            # A: the input, the product written, read and rewritten scaled, read again, the section
            "A_bytes": int(n_pol * (n * esz_in + 4 * prod + K * C * esz)),
            "A_bytes_without_scale_pass": int(n_pol * (n * esz_in + 2 * prod + K * C * esz)),
            "B_bytes": int(n_pol * (n * esz_in + (K * C * esz if path == "fused" else 2 * prod + K * C * esz)))}),
            flush=True)
        del plan, src, cf, scaled, sec_a, sec_b, sec_p
        torch.cuda.empty_cache()


def quantised_output(torch, pfb, dev, reps, rounds, sides=("A", "A_nocopy", "B", "Bs", "floor")):
    """The FilterBank's output quantiser (FilterBank.m:106-113) into a DADA section at the C2 shape
    (256 ch, 8/7, 2^24 samples), through the C ABI into preallocated buffers.
    A: what FilterBank enqueues today — the cf32 execute (pfb_analysis_execute, or _dada for an
    NBIT 16 section), pfb_quantize(rms), the contiguous copy, pfb_dada_pack.  A_nocopy: the same
    without the copy (FilterBank's view of a device product is already contiguous when it is
    transposed back).  B: pfb_analysis_execute_quantised_to_dada in AUTO mode.  Bs: the same with
    the moments STAGED.  floor: the plain pfb_analysis_execute_to_dada (no quantiser).
    All sides are warmed, then `rounds` windows of `reps` calls of each side, alternating in one
    process.  One line per case with the median, min, max and max - min of each side, whether the
    sections are equal and whether A's and B's float32 scales have the same bits, and the
    project's rule: the lower median wins when the difference exceeds the larger spread."""
    from ctypes import byref, c_double, c_int64, c_void_p
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(9)
    taps = pfb.design_PFB_FIR_filter(256, "8/7", 12)
    n, N = 1 << 24, 256
    dts = {8: torch.int8, 16: torch.int16}
    for in_nbit in (0, 16):
        for n_pol in (1, 2):
            for nbit in (8, 16):
                plan = pfb.AnalysisPlan(taps, N, "8/7", "polyphase_analysis", n_pol)
                K, C = plan.output_length(n), plan.out_chan
                if in_nbit:
                    src = torch.randint(-3000, 3000, (n * n_pol * 2,), dtype=torch.int16, device=dev, generator=g)
                else:
                    src = torch.view_as_complex(torch.randn((n_pol, n, 2), device=dev, generator=g) + 0.25)
                cf = torch.empty((n_pol, K, C), dtype=torch.complex64, device=dev)
                quant = torch.empty_like(cf)
                copy = torch.empty_like(cf)
                sec = {k: torch.empty((K, C, n_pol, 2), dtype=dts[nbit], device=dev) for k in sides}
                nbytes = K * C * n_pol * 2 * (nbit // 8)
                stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                n_out = c_int64(0)
                rms = 20.0 if nbit == 8 else 3000.0

                def execute_cf32():
                    if in_nbit:
                        _lib.check(lib.pfb_analysis_execute_dada(plan._h, c_void_p(src.data_ptr()), in_nbit, 2,
                                                                 _lib.PFB_DADA_TFP, n, c_void_p(cf.data_ptr()), K * C,
                                                                 K, byref(n_out), stream))
                    else:
                        _lib.check(lib.pfb_analysis_execute(plan._h, c_void_p(src.data_ptr()), n, n,
                                                            c_void_p(cf.data_ptr()), K * C, K, byref(n_out),
                                                            _lib.PFB_MEM_DEVICE, stream))

                def side_a(with_copy, scale=None):
                    execute_cf32()
                    _lib.check(lib.pfb_quantize(c_void_p(cf.data_ptr()), K * C, K * C, n_pol, rms,
                                                c_void_p(quant.data_ptr()), K * C, scale, stream))
                    packed = quant
                    if with_copy:
                        copy.copy_(quant)
                        packed = copy
                    _lib.check(lib.pfb_dada_pack(c_void_p(packed.data_ptr()), K * C, K, C, n_pol,
                                                 c_void_p(sec["A" if with_copy else "A_nocopy"].data_ptr()), nbit,
                                                 stream))

                def side_b(key, scale=None):
                    dst = c_void_p(sec[key].data_ptr())
                    if in_nbit:
                        _lib.check(lib.pfb_analysis_execute_dada_quantised_to_dada(
                            plan._h, c_void_p(src.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, n, rms, dst, nbit, 1.0,
                            nbytes, byref(n_out), scale, stream))
                    else:
                        _lib.check(lib.pfb_analysis_execute_quantised_to_dada(
                            plan._h, c_void_p(src.data_ptr()), n, n, rms, dst, nbit, 1.0, nbytes, byref(n_out), scale,
                            stream))

                def side_bs(scale=None):
                    _lib.check(lib.pfb_analysis_set_quantiser_moments(plan._h, _lib.PFB_QUANTISER_MOMENTS_STAGED))
                    side_b("Bs", scale)
                    _lib.check(lib.pfb_analysis_set_quantiser_moments(plan._h, _lib.PFB_QUANTISER_MOMENTS_AUTO))

                def side_floor():
                    dst = c_void_p(sec["floor"].data_ptr())
                    if in_nbit:
                        _lib.check(lib.pfb_analysis_execute_dada_to_dada(
                            plan._h, c_void_p(src.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, n, dst, nbit, 1e-3,
                            nbytes, byref(n_out), stream))
                    else:
                        _lib.check(lib.pfb_analysis_execute_to_dada(plan._h, c_void_p(src.data_ptr()), n, n, dst, nbit,
                                                                    1e-3, nbytes, byref(n_out), stream))

                fns = {"A": lambda: side_a(True), "A_nocopy": lambda: side_a(False), "B": lambda: side_b("B"),
                       "Bs": side_bs, "floor": side_floor}
                fns = {k: fns[k] for k in sides}
                rec = {"kernel": "quantised_output", "shape": "C2 256ch 8/7", "samples": n, "n_pol": n_pol,
                       "in": f"nbit{in_nbit}" if in_nbit else "cf32", "nbit": nbit, "rms": rms,
                       "calls_per_window": reps, "windows": rounds}
                # the scales and the sections, once
                sa, sb, sbs = c_double(0), c_double(0), c_double(0)
                if "A" in sides:
                    side_a(True, byref(sa))
                    rec["A_scale"] = sa.value
                if "B" in sides:
                    side_b("B", byref(sb))
                    rec["B_scale"], rec["B_path"] = sb.value, plan.last_quantiser()
                    rec["input_path"] = plan.last_dada_input()
                if "Bs" in sides:
                    side_bs(byref(sbs))
                    rec["Bs_scale"], rec["Bs_path"] = sbs.value, plan.last_quantiser()
                for k in sides:
                    fns[k]()
                torch.cuda.synchronize()
                if "A" in sides and "B" in sides:
                    rec["A_B_float32_scale_bits_equal"] = bool(np.float32(sa.value).tobytes() ==
                                                               np.float32(sb.value).tobytes())
                    rec["A_B_outputs_equal"] = bool(torch.equal(sec["A"], sec["B"]))
                    rec["A_B_samples_differing"] = int((sec["A"] != sec["B"]).sum())
                if "B" in sides and "Bs" in sides:
                    rec["B_Bs_float32_scale_bits_equal"] = bool(np.float32(sb.value).tobytes() ==
                                                                np.float32(sbs.value).tobytes())
                    rec["B_Bs_outputs_equal"] = bool(torch.equal(sec["B"], sec["Bs"]))
                if "A" in sides and "A_nocopy" in sides:
                    rec["A_A_nocopy_outputs_equal"] = bool(torch.equal(sec["A"], sec["A_nocopy"]))
                for _ in range(2):
                    for k in sides:
                        timeit(torch, fns[k], reps)
                t = {k: [] for k in sides}
                for _ in range(rounds):
                    for k in sides:
                        t[k].append(timeit(torch, fns[k], reps))
                for k in sides:
                    rec[f"{k}_ms"] = {"median": round(float(np.median(t[k])), 4), "min": round(float(min(t[k])), 4),
                                      "max": round(float(max(t[k])), 4),
                                      "spread": round(float(max(t[k]) - min(t[k])), 4)}

                def wins(x, y):  # x's median below y's by more than the larger spread
                    return bool(rec[f"{y}_ms"]["median"] - rec[f"{x}_ms"]["median"] >
                                max(rec[f"{x}_ms"]["spread"], rec[f"{y}_ms"]["spread"]))
                for x, y in (("B", "A"), ("B", "A_nocopy"), ("B", "Bs"), ("Bs", "B"), ("Bs", "A")):
                    if x in sides and y in sides:
                        rec[f"{x}_below_{y}_by_more_than_spread"] = wins(x, y)
                esz_in, esz, prod = (2 * in_nbit // 8 if in_nbit else 8), 2 * nbit // 8, K * C * 8
                # per polarisation: the input read; the product written and read back
                rec["A_bytes"] = int(n_pol * (n * esz_in + prod + prod + 2 * prod + 2 * prod + prod + K * C * esz))
                rec["A_nocopy_bytes"] = int(n_pol * (n * esz_in + prod + prod + 2 * prod + prod + K * C * esz))
                rec["B_bytes"] = int(n_pol * (n * esz_in + 2 * prod + K * C * esz))
                rec["Bs_bytes"] = int(n_pol * (n * esz_in + 3 * prod + K * C * esz))
                rec["floor_bytes"] = int(n_pol * (n * esz_in + K * C * esz))
                print(json.dumps(rec), flush=True)
                del plan, src, cf, quant, copy, sec
                torch.cuda.empty_cache()


def quantised_input(torch, pfb, dev, reps, rounds, sides=("A", "B", "Bs", "floor")):
    """The FilterBank's input quantiser (FilterBank.m:75-83) at the C2 shape (256 ch, 8/7, 2^24
    samples), through the C ABI into preallocated buffers.
    A: what FilterBank enqueues today — pfb_dada_unpack for an NBIT 16 section, pfb_quantize(rms)
    into a buffer, pfb_analysis_execute.  B: the call with the plan's input quantiser, AUTO.  Bs:
    the same, STAGED.  floor: the same call with the quantiser off.  The cells: cf32 and NBIT 16
    input, one and two polarisations, cf32 output — and one pfb_analysis_execute_dada_quantised_to_dada
    cell (NBIT 16 in and out, both quantisers; its A: unpack, pfb_quantize, execute, pfb_quantize,
    pfb_dada_pack).  `sides`: "A" alone runs on a library without the new entry points (the
    parent commit's, the yardstick).  All sides are warmed, then `rounds` windows of `reps` calls
    of each side, alternating in one process; one line per cell with the median, min, max and
    max - min of each side, whether A's and B's outputs are equal and their float32 scales have
    the same bits, the byte totals from the formulas, and the project's rule: the lower median wins
    when the difference exceeds the larger spread."""
    from ctypes import byref, c_double, c_int64, c_void_p
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(10)
    taps = pfb.design_PFB_FIR_filter(256, "8/7", 12)
    n, N, rms = 1 << 24, 256, 20.0
    AUTO, STAGED = _lib.PFB_QUANTISER_MOMENTS_AUTO, _lib.PFB_QUANTISER_MOMENTS_STAGED
    cells = [(in_nbit, n_pol, 0) for in_nbit in (0, 16) for n_pol in (1, 2)] + [(16, 1, 16)]
    for in_nbit, n_pol, out_nbit in cells:
        plan = pfb.AnalysisPlan(taps, N, "8/7", "polyphase_analysis", n_pol)
        K, C = plan.output_length(n), plan.out_chan
        if in_nbit:
            src = (torch.randn((n * n_pol * 2,), device=dev, generator=g) * 1500 + 400).to(torch.int16)
            unp = torch.empty((n_pol, n), dtype=torch.complex64, device=dev)
        else:
            src = torch.view_as_complex(torch.randn((n_pol, n, 2), device=dev, generator=g) + 0.25)
            unp = src
        qbuf = torch.empty((n_pol, n), dtype=torch.complex64, device=dev)
        cf = torch.empty((n_pol, K, C), dtype=torch.complex64, device=dev)
        if out_nbit:
            quant = torch.empty_like(cf)
            out = {k: torch.empty((K, C, n_pol, 2), dtype=torch.int16, device=dev) for k in sides}
            nbytes = K * C * n_pol * 2 * (out_nbit // 8)
        else:
            out = {k: (cf if k == "A" else torch.empty_like(cf)) for k in sides}
        stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n_out = c_int64(0)

        def side_a(scale=None):
            if in_nbit:
                _lib.check(lib.pfb_dada_unpack(c_void_p(src.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, n, 1, n_pol,
                                               c_void_p(unp.data_ptr()), n, stream))
            _lib.check(lib.pfb_quantize(c_void_p(unp.data_ptr()), n, n, n_pol, rms, c_void_p(qbuf.data_ptr()), n,
                                        scale, stream))
            _lib.check(lib.pfb_analysis_execute(plan._h, c_void_p(qbuf.data_ptr()), n, n, c_void_p(cf.data_ptr()),
                                                K * C, K, byref(n_out), _lib.PFB_MEM_DEVICE, stream))
            if out_nbit:
                _lib.check(lib.pfb_quantize(c_void_p(cf.data_ptr()), K * C, K * C, n_pol, 3000.0,
                                            c_void_p(quant.data_ptr()), K * C, None, stream))
                _lib.check(lib.pfb_dada_pack(c_void_p(quant.data_ptr()), K * C, K, C, n_pol,
                                             c_void_p(out["A"].data_ptr()), out_nbit, stream))

        def new_call(key, on, mode):
            _lib.check(lib.pfb_analysis_set_input_quantiser(plan._h, int(on), rms))
            _lib.check(lib.pfb_analysis_set_input_quantiser_mode(plan._h, mode))
            dst = c_void_p(out[key].data_ptr())
            if out_nbit:
                _lib.check(lib.pfb_analysis_execute_dada_quantised_to_dada(
                    plan._h, c_void_p(src.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, n, 3000.0, dst, out_nbit, 1.0,
                    nbytes, byref(n_out), None, stream))
            elif in_nbit:
                _lib.check(lib.pfb_analysis_execute_dada(plan._h, c_void_p(src.data_ptr()), in_nbit, 2,
                                                         _lib.PFB_DADA_TFP, n, dst, K * C, K, byref(n_out), stream))
            else:
                _lib.check(lib.pfb_analysis_execute(plan._h, c_void_p(src.data_ptr()), n, n, dst, K * C, K,
                                                    byref(n_out), _lib.PFB_MEM_DEVICE, stream))
            _lib.check(lib.pfb_analysis_set_input_quantiser(plan._h, 0, 0.0))

        fns = {"A": side_a, "B": lambda: new_call("B", True, AUTO), "Bs": lambda: new_call("Bs", True, STAGED),
               "floor": lambda: new_call("floor", False, AUTO)}
        fns = {k: fns[k] for k in sides}
        rec = {"kernel": "quantised_input", "shape": "C2 256ch 8/7", "samples": n, "n_pol": n_pol,
               "in": f"nbit{in_nbit}" if in_nbit else "cf32", "out": f"quantised nbit{out_nbit}" if out_nbit else "cf32",
               "rms": rms, "calls_per_window": reps, "windows": rounds}
        # the scales and the outputs, once
        sa, sb = c_double(0), c_double(0)
        if "A" in sides:
            side_a(byref(sa))
            rec["A_scale"] = sa.value
        for key in ("B", "Bs"):
            if key in sides:
                fns[key]()
                # (the setter that switched the quantiser off again touches no device state)
                _lib.check(lib.pfb_analysis_last_input_scale(plan._h, byref(sb), stream))
                rec[f"{key}_scale"] = sb.value
                rec[f"{key}_path"] = plan.last_input_quantiser()
        for k in sides:
            fns[k]()
        torch.cuda.synchronize()
        if "A" in sides and "B" in sides:
            rec["A_B_float32_scale_bits_equal"] = bool(np.float32(rec["A_scale"]).tobytes() ==
                                                       np.float32(rec["B_scale"]).tobytes())
            rec["A_B_outputs_equal"] = bool(torch.equal(out["A"], out["B"]))
        if "B" in sides and "Bs" in sides:
            rec["B_Bs_outputs_equal"] = bool(torch.equal(out["B"], out["Bs"]))
            rec["B_Bs_scale_bits_equal"] = bool(rec["B_scale"] == rec["Bs_scale"])
        for _ in range(2):
            for k in sides:
                timeit(torch, fns[k], reps)
        t = {k: [] for k in sides}
        for _ in range(rounds):
            for k in sides:
                t[k].append(timeit(torch, fns[k], reps))
        for k in sides:
            rec[f"{k}_ms"] = {"median": round(float(np.median(t[k])), 4), "min": round(float(min(t[k])), 4),
                              "max": round(float(max(t[k])), 4), "spread": round(float(max(t[k]) - min(t[k])), 4)}

        def wins(x, y):  # x's median below y's by more than the larger spread
            return bool(rec[f"{y}_ms"]["median"] - rec[f"{x}_ms"]["median"] >
                        max(rec[f"{x}_ms"]["spread"], rec[f"{y}_ms"]["spread"]))
        for x, y in (("B", "A"), ("B", "Bs"), ("Bs", "B"), ("Bs", "A")):
            if x in sides and y in sides:
                rec[f"{x}_below_{y}_by_more_than_spread"] = wins(x, y)
        # bytes per input sample on top of the analysis's own stores, and the stores
        per = {"A": 44 if in_nbit else 32, "B": 8 if in_nbit else 16, "Bs": 24 if in_nbit else 32,
               "floor": 4 if in_nbit else 8}
        stores = K * C * 8 if not out_nbit else K * C * (8 + 8 + 2 * out_nbit // 8)
        for k in sides:
            extra = 4 * K * C * 8 if (out_nbit and k == "A") else 0   # (pfb_quantize's two more passes over the product)
            rec[f"{k}_bytes"] = int(n_pol * (n * per[k] + stores + extra))
        print(json.dumps(rec), flush=True)
        del plan, src, unp, qbuf, cf, out
        torch.cuda.empty_cache()


def dada_synthesis_output(torch, pfb, dev, reps, rounds):
    """Channelised rows -> single-channel DADA section (TFP, NBIT 8 / 16 / 32) at the C2 synthesis
    shape (256 ch, 8/7, Nf 256, Ov 48, tukey, deripple; the rows of a 2^24-sample unit).  A: the
    pair a caller had before — the cf32-output call (pfb_synthesis_execute, or
    pfb_synthesis_execute_dada for an NBIT 16 section), both components times the scale in
    float32 (one elementwise pass), then pfb_dada_pack with one channel.  B:
    pfb_synthesis_execute_to_dada / pfb_synthesis_execute_dada_to_dada.  Both through the C ABI
    into preallocated buffers.  The sections are asserted equal first; then `rounds` windows of
    `reps` calls of each side, alternating A and B in one process, after a warm-up of both.  One
    line per case with the median, min, max and quartiles of each side's per-call time, and
    A_execute_ms: the cf32-output call alone, timed in windows of its own between the two.
    stays_fused: B's median lies below A's by more than A's min-to-max spread (and the larger of
    the two interquartile spreads)."""
    from ctypes import byref, c_int64, c_void_p
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(6)
    N, rows = 256, ((1 << 24) // 224) // 32 * 32
    taps = pfb.design_PFB_FIR_filter(N, "8/7", 12)
    win = pfb.PFBWindow().lookup["tukey"](256, 48)
    dts = {8: torch.int8, 16: torch.int16, 32: torch.float32}
    for n_pol in (1, 2):
        plan = pfb.SynthesisPlan(N, "8/7", 256, 48, True, 1, True, taps, win, None, n_pol)
        n_o = plan.output_length(rows)
        cf = torch.empty((n_pol, n_o), dtype=torch.complex64, device=dev)
        scaled = torch.empty_like(cf)
        for in_nbit in (0, 16):
            if in_nbit:
                src = torch.randint(-(1 << 15), 1 << 15, (rows * N * n_pol * 2,), dtype=torch.int16, device=dev,
                                    generator=g)
            else:
                src = torch.view_as_complex(torch.randn((n_pol, rows, N, 2), device=dev, generator=g))
            stream = c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            n_out = c_int64(0)

            def execute_cf32():
                if in_nbit:
                    _lib.check(lib.pfb_synthesis_execute_dada(plan._h, c_void_p(src.data_ptr()), in_nbit, 2,
                                                              _lib.PFB_DADA_TFP, rows, 1, c_void_p(cf.data_ptr()), n_o,
                                                              n_o, byref(n_out), stream))
                else:
                    _lib.check(lib.pfb_synthesis_execute(plan._h, c_void_p(src.data_ptr()), rows * N, rows, 1,
                                                         c_void_p(cf.data_ptr()), n_o, n_o, byref(n_out),
                                                         _lib.PFB_MEM_DEVICE, stream))

            # the series' component rms at a third of the integer range (0.37 for NBIT 32)
            execute_cf32()
            rms = float(torch.view_as_real(cf).square().mean().sqrt())
            for nbit in (8, 16, 32):
                scale = float(np.float32((((1 << (nbit - 1)) - 1) / 3.0 if nbit != 32 else 0.37) / rms))
                sec_a = torch.empty((n_o, 1, n_pol, 2), dtype=dts[nbit], device=dev)
                sec_b = torch.empty_like(sec_a)
                nbytes = sec_b.numel() * sec_b.element_size()

                def side_a():
                    execute_cf32()
                    torch.mul(torch.view_as_real(cf), scale, out=torch.view_as_real(scaled))
                    _lib.check(lib.pfb_dada_pack(c_void_p(scaled.data_ptr()), n_o, n_o, 1, n_pol,
                                                 c_void_p(sec_a.data_ptr()), nbit, stream))

                def side_b():
                    if in_nbit:
                        _lib.check(lib.pfb_synthesis_execute_dada_to_dada(
                            plan._h, c_void_p(src.data_ptr()), in_nbit, 2, _lib.PFB_DADA_TFP, rows, 1,
                            c_void_p(sec_b.data_ptr()), nbit, scale, nbytes, byref(n_out), stream))
                    else:
                        _lib.check(lib.pfb_synthesis_execute_to_dada(
                            plan._h, c_void_p(src.data_ptr()), rows * N, rows, 1, c_void_p(sec_b.data_ptr()), nbit,
                            scale, nbytes, byref(n_out), stream))

                side_a()
                side_b()
                path_in, path = plan.last_dada_input(), plan.last_dada_output()
                torch.cuda.synchronize()
                assert n_out.value == n_o and torch.equal(sec_a, sec_b), \
                    f"dada_synthesis_output {in_nbit}->{nbit} {n_pol} pol: sections differ"
                for _ in range(2):
                    timeit(torch, side_a, reps)
                    timeit(torch, side_b, reps)
                ta, tb, tc = [], [], []
                for _ in range(rounds):
                    ta.append(timeit(torch, side_a, reps))
                    tb.append(timeit(torch, side_b, reps))
                    tc.append(timeit(torch, execute_cf32, reps))

                def stats(t):
                    q = np.percentile(t, [0, 25, 50, 75, 100])
                    return {k: round(float(v), 4) for k, v in zip(("min", "q25", "median", "q75", "max"), q)}
                a, b, c = stats(ta), stats(tb), stats(tc)
                iqr_a, iqr_b = a["q75"] - a["q25"], b["q75"] - b["q25"]
                spread_a = a["max"] - a["min"]
                esz_in, esz = (2 * in_nbit // 8 if in_nbit else 8), 2 * nbit // 8
                print(json.dumps({
                    "kernel": "dada_synthesis_output", "shape": "256ch 8/7 Nf256 Ov48 tukey deripple", "rows": rows,
                    "n_out": n_o, "n_pol": n_pol, "in": f"nbit{in_nbit}" if in_nbit else "cf32", "nbit": nbit,
                    "path": path, "input_path": path_in, "calls_per_window": reps, "windows": rounds,
                    "outputs_equal": True, "A_execute_scale_pack_ms": a, "B_execute_to_dada_ms": b,
                    "A_execute_ms": c, "A_iqr_ms": round(iqr_a, 4), "B_iqr_ms": round(iqr_b, 4),
                    "A_spread_ms": round(spread_a, 4),
                    "B_below_A_by_ms": round(a["median"] - b["median"], 4),
                    "B_over_A": round(b["median"] / a["median"], 4),
                    "stays_fused": bool(path == "fused" and
                                        a["median"] - b["median"] > max(spread_a, iqr_a, iqr_b)),
                    # per call beyond the channel IFFT: A writes the series, reads and rewrites it
                    # scaled, reads it again and writes the section; B writes the section
                    "A_output_bytes": int(n_pol * n_o * (4 * 8 + esz)),
                    "B_output_bytes": int(n_pol * n_o * (esz if path == "fused" else 2 * 8 + esz)),
                    "input_bytes": int(n_pol * rows * N * esz_in)}), flush=True)
                del sec_a, sec_b
            del src
        del plan, cf, scaled
        torch.cuda.empty_cache()


def dada_roundtrip(torch, pfb, dev, reps, rounds):
    """Single-channel DADA section -> the channelised file's float section and the output file's
    section, the C2 unit (2^24 samples, 256 ch, 8/7, 3073 taps, Nf 256, Ov 48, tukey, deripple).
    A: the sequence a caller had before — pfb_dada_unpack, pfb_roundtrip_execute, pfb_dada_pack at
    NBIT 32 of the product when there are two polarisations (one polarisation's cf32 product is
    the section already), both components of the output times the scale in float32 (one
    elementwise pass), pfb_dada_pack with one channel.  B: pfb_roundtrip_execute_dada_to_dada.
    Both through the C ABI into preallocated buffers.  The sections are asserted equal first;
    then `rounds` windows of `reps` calls of each side, alternating A and B in one process,
    after a warm-up of both.  One line per cell with the median, min, max and quartiles of each
    side's per-call time.  stays_fused: B's median lies below A's by more than the larger of the
    two sides' min-to-max spreads.  The last line is the pipelined row: the two halves over two
    streams on two plan pairs, the steps captured as one graph as bench.py captures its headline
    (A: unpack + cf32 analysis half on one stream, cf32 synthesis half + packs on the other; B:
    the two DADA halves), in windows of replays."""
    from ctypes import byref, c_int64, c_void_p
    from ska_pst_dsp_model_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(8)
    N, n = 256, 1 << 24
    taps = pfb.design_PFB_FIR_filter(N, "8/7", 12)
    win = pfb.PFBWindow().lookup["tukey"](256, 48)
    dts = {8: torch.int8, 16: torch.int16, 32: torch.float32}
    TFP = _lib.PFB_DADA_TFP

    def plans(n_pol):
        return (pfb.AnalysisPlan(taps, N, "8/7", "polyphase_analysis", n_pol),
                pfb.SynthesisPlan(N, "8/7", 256, 48, True, 1, True, taps, win, None, n_pol))

    def section(nbit, n_pol):
        if nbit == 32:
            return torch.randn((n * n_pol * 2,), device=dev, generator=g)
        lim = 1 << (nbit - 1)
        return torch.randint(-lim, lim, (n * n_pol * 2,), dtype=dts[nbit], device=dev, generator=g)

    def stats(t):
        q = np.percentile(t, [0, 25, 50, 75, 100])
        return {k: round(float(v), 4) for k, v in zip(("min", "q25", "median", "q75", "max"), q)}

    def ptr(t):
        return c_void_p(t.data_ptr())

    def cur():
        return c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    class Unit:
        """One plan pair with the buffers of both sides."""

        def __init__(self, n_pol, in_nbit, nbit, src):
            self.n_pol, self.in_nbit, self.nbit, self.src = n_pol, in_nbit, nbit, src
            self.ana, self.syn = plans(n_pol)
            self.K = self.ana.output_length(n)
            self.n_o = self.syn.output_length(self.K)
            self.x = torch.empty((n_pol, n), dtype=torch.complex64, device=dev)
            self.chan = torch.empty((n_pol, self.K, N), dtype=torch.complex64, device=dev)
            self.cf = torch.empty((n_pol, self.n_o), dtype=torch.complex64, device=dev)
            self.scaled = torch.empty_like(self.cf)
            # (one polarisation: the cf32 product is the float section)
            self.chan_a = torch.empty((self.K, N, n_pol, 2), device=dev) if n_pol > 1 else torch.view_as_real(
                self.chan[0])[:, :, None, :]
            self.chan_b = torch.empty((self.K, N, n_pol, 2), device=dev)
            self.sec_a = torch.empty((self.n_o, 1, n_pol, 2), dtype=dts[nbit], device=dev)
            self.sec_b = torch.empty_like(self.sec_a)
            self.kr, self.no = c_int64(0), c_int64(0)
            self.scale = 1.0

        def a_analysis(self, whole):
            _lib.check(lib.pfb_dada_unpack(ptr(self.src), self.in_nbit, 2, TFP, n, 1, self.n_pol, ptr(self.x), n, cur()))
            if whole:
                _lib.check(lib.pfb_roundtrip_execute(self.ana._h, self.syn._h, ptr(self.x), n, n, ptr(self.chan),
                                                     self.K * N, self.K, byref(self.kr), 1, ptr(self.cf), self.n_o,
                                                     self.n_o, byref(self.no), cur()))
            else:
                _lib.check(lib.pfb_roundtrip_analysis_execute(self.ana._h, self.syn._h, ptr(self.x), n, n,
                                                              ptr(self.chan), self.K * N, self.K, byref(self.kr), 1,
                                                              cur()))

        def a_output(self, whole):
            if not whole:
                _lib.check(lib.pfb_roundtrip_synthesis_execute(self.ana._h, self.syn._h, n, 1, ptr(self.cf), self.n_o,
                                                               self.n_o, byref(self.no), cur()))
            if self.n_pol > 1:
                _lib.check(lib.pfb_dada_pack(ptr(self.chan), self.K * N, self.K, N, self.n_pol, ptr(self.chan_a), 32,
                                             cur()))
            torch.mul(torch.view_as_real(self.cf), self.scale, out=torch.view_as_real(self.scaled))
            _lib.check(lib.pfb_dada_pack(ptr(self.scaled), self.n_o, self.n_o, 1, self.n_pol, ptr(self.sec_a),
                                         self.nbit, cur()))

        def side_a(self):
            self.a_analysis(True)
            self.a_output(True)

        def side_b(self):
            _lib.check(lib.pfb_roundtrip_execute_dada_to_dada(
                self.ana._h, self.syn._h, ptr(self.src), self.in_nbit, 2, TFP, n, ptr(self.chan_b),
                self.chan_b.numel() * 4, byref(self.kr), 1, ptr(self.sec_b), self.nbit, self.scale,
                self.sec_b.numel() * self.sec_b.element_size(), byref(self.no), cur()))

        def b_analysis(self):
            _lib.check(lib.pfb_roundtrip_analysis_execute_dada(
                self.ana._h, self.syn._h, ptr(self.src), self.in_nbit, 2, TFP, n, ptr(self.chan_b),
                self.chan_b.numel() * 4, byref(self.kr), 1, cur()))

        def b_output(self):
            _lib.check(lib.pfb_roundtrip_synthesis_execute_to_dada(
                self.ana._h, self.syn._h, n, 1, ptr(self.sec_b), self.nbit, self.scale,
                self.sec_b.numel() * self.sec_b.element_size(), byref(self.no), cur()))

        def set_scale(self):
            # the output's component rms at a third of the integer range (0.37 for NBIT 32)
            self.side_a()
            rms = float(torch.view_as_real(self.cf).square().mean().sqrt())
            self.scale = float(np.float32((((1 << (self.nbit - 1)) - 1) / 3.0 if self.nbit != 32 else 0.37) / rms))

        def check(self, what):
            self.sec_a.zero_()
            self.sec_b.zero_()
            self.chan_b.zero_()
            self.side_a()
            self.side_b()
            paths = (self.ana.last_dada_input(), self.ana.last_dada_output(), self.syn.last_dada_output())
            torch.cuda.synchronize()
            assert (self.kr.value, self.no.value) == (self.K, self.n_o), what
            assert torch.equal(self.sec_a, self.sec_b), f"{what}: output sections differ"
            assert torch.equal(self.chan_a, self.chan_b), f"{what}: product sections differ"
            return paths

        def bytes(self, fused):
            P, K, n_o = self.n_pol, self.K, self.n_o
            e_in, e_out = 2 * self.in_nbit // 8, 2 * self.nbit // 8
            # A: the section read, the series written and read, the product written (and, two
            # polarisations, read and rewritten), the output written, read, rewritten scaled,
            # read again and the section written.  B fused: section read, product and section
            # written.  (The stage-1 rows, written and read once on both sides, are left out.)
            a = P * (n * (e_in + 16) + K * N * (8 + (16 if P > 1 else 0)) + n_o * (32 + e_out))
            b = P * (n * e_in + K * N * 8 + n_o * e_out)
            return int(a), int(b if fused else a)

    for n_pol in (1, 2):
        for in_nbit, nbit in ((16, 16), (8, 8), (16, 32), (32, 32)):
            what = f"dada_roundtrip {in_nbit}->{nbit} {n_pol} pol"
            u = Unit(n_pol, in_nbit, nbit, section(in_nbit, n_pol))
            u.set_scale()
            paths = u.check(what)
            fused = paths == ("fused", "fused", "fused")
            for _ in range(2):
                timeit(torch, u.side_a, reps)
                timeit(torch, u.side_b, reps)
            ta, tb = [], []
            for _ in range(rounds):
                ta.append(timeit(torch, u.side_a, reps))
                tb.append(timeit(torch, u.side_b, reps))
            a, b = stats(ta), stats(tb)
            spread = max(a["max"] - a["min"], b["max"] - b["min"])
            ab, bb = u.bytes(fused)
            print(json.dumps({
                "kernel": "dada_roundtrip", "shape": "C2 2^24 256ch 8/7 Nf256 Ov48 tukey deripple", "n_pol": n_pol,
                "in_nbit": in_nbit, "out_nbit": nbit, "rows": u.K, "n_out": u.n_o, "paths": list(paths),
                "calls_per_window": reps, "windows": rounds, "sections_equal": True,
                "A_unpack_roundtrip_packs_ms": a, "B_roundtrip_dada_to_dada_ms": b,
                "A_spread_ms": round(a["max"] - a["min"], 4), "B_spread_ms": round(b["max"] - b["min"], 4),
                "B_below_A_by_ms": round(a["median"] - b["median"], 4),
                "B_over_A": round(b["median"] / a["median"], 4),
                "stays_fused": bool(fused and a["median"] - b["median"] > spread),
                "A_bytes": ab, "B_bytes": bb}), flush=True)
            del u
            torch.cuda.empty_cache()

    # ---- the pipelined row: two plan pairs, two streams, the steps of a window as one graph
    n_pol, in_nbit, nbit, steps = 1, 16, 16, 8
    units = [Unit(n_pol, in_nbit, nbit, section(in_nbit, n_pol)) for _ in range(2)]
    for u in units:
        u.set_scale()
        u.check("dada_roundtrip pipelined")
    D = len(units)

    def capture(ana_half, out_half):
        def enqueue():
            sa = torch.cuda.current_stream(dev)
            ss = torch.cuda.Stream(device=dev)
            ss.wait_stream(sa)
            ev_a = [torch.cuda.Event() for _ in range(steps)]
            ev_s = [torch.cuda.Event() for _ in range(steps)]
            for i in range(steps):
                u = units[i % D]
                if i >= D:
                    sa.wait_event(ev_s[i - D])
                ana_half(u)
                ev_a[i].record(sa)
                ss.wait_event(ev_a[i])
                with torch.cuda.stream(ss):
                    out_half(u)
                ev_s[i].record(ss)
            sa.wait_stream(ss)
        cs = torch.cuda.Stream(device=dev)
        cs.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(cs):
            enqueue()                                     # warm-up: every buffer the halves need exists
        torch.cuda.current_stream(dev).wait_stream(cs)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            enqueue()
        torch.cuda.synchronize(dev)
        return graph.replay

    pipe_a = capture(lambda u: u.a_analysis(False), lambda u: u.a_output(False))
    pipe_b = capture(lambda u: u.b_analysis(), lambda u: u.b_output())
    for u in units:
        u.sec_a.zero_()
        u.sec_b.zero_()
        u.chan_b.zero_()
    pipe_a()
    pipe_b()
    torch.cuda.synchronize()
    for u in units:
        assert torch.equal(u.sec_a, u.sec_b) and torch.equal(u.chan_a, u.chan_b), "pipelined: sections differ"
    paths = (units[0].ana.last_dada_input(), units[0].ana.last_dada_output(), units[0].syn.last_dada_output())
    w = max(1, reps // steps)
    for _ in range(2):
        timeit(torch, pipe_a, w)
        timeit(torch, pipe_b, w)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timeit(torch, pipe_a, w) / steps)
        tb.append(timeit(torch, pipe_b, w) / steps)
    a, b = stats(ta), stats(tb)
    spread = max(a["max"] - a["min"], b["max"] - b["min"])
    ab, bb = units[0].bytes(paths == ("fused", "fused", "fused"))
    print(json.dumps({
        "kernel": "dada_roundtrip_pipelined", "shape": "C2 2^24 256ch 8/7 Nf256 Ov48 tukey deripple",
        "n_pol": n_pol, "in_nbit": in_nbit, "out_nbit": nbit, "plan_pairs": D, "streams": 2,
        "steps_per_graph": steps, "replays_per_window": w, "windows": rounds, "paths": list(paths),
        "sections_equal": True, "A_ms_per_step": a, "B_ms_per_step": b,
        "A_spread_ms": round(a["max"] - a["min"], 4), "B_spread_ms": round(b["max"] - b["min"], 4),
        "B_below_A_by_ms": round(a["median"] - b["median"], 4), "B_over_A": round(b["median"] / a["median"], 4),
        "meets_rule": bool(a["median"] - b["median"] > spread), "A_bytes": ab, "B_bytes": bb}), flush=True)


def twostage_inverse(torch, pfb, noise, reps, rounds):
    """TwoStageInverseFilterBank stream calls, the gather against the strided input.  Shapes:
    the inverse of BASELINE configs[2]'s cascade (4096 coarse x 14 fine channels, critical,
    stage-2 bank 16 ch 8/7, Nf 128, Ov 16; 1170 rows = one 2^26-sample-equivalent call) and the
    256 x 256 oversampled cascade (stage-2 bank 256 ch 8/7, Nf 256, Ov 48; 1024 rows).
    A: strided_input = False (pfb_gather_channels + the packed call).  B: strided_input = True
    (pfb_inverse_filterbank_execute_strided).  Two objects fed the same calls, so their carries
    agree; the outputs of the first calls are asserted equal; then `rounds` windows of `reps`
    calls of each side, alternating A and B in one process, after a warm-up of both.  One line
    per shape with every window's per-call time and each side's median, min and max."""
    def cfg(n, nf, ov):
        return dict(filt_coeff=pfb.design_PFB_FIR_filter(n, "8/7", 10 if n == 16 else 12), channels=n,
                    os_factor="8/7", input_fft_length=nf, input_overlap=ov, deripple=False,
                    temporal_taper="tukey")
    shapes = [("SKA-Mid inverse 4096x14 critical", cfg(16, 128, 16), 14, 4096, 1170),
              ("256x256 oversampled", cfg(256, 256, 48), 256, 256, 1024)]
    for name, c, nch2, n_coarse, rows in shapes:
        x = noise(1, rows, n_coarse * nch2).transpose(1, 2)      # (1, nchan, T), channel fastest
        sides = []
        for strided in (False, True):
            ti = pfb.TwoStageInverseFilterBank(c)
            ti.nch2 = nch2
            ti.strided_input = strided
            sides.append(ti)
        a_obj, b_obj = sides
        for _ in range(3):
            _, oa = a_obj.execute(x)
            _, ob = b_obj.execute(x)
            torch.cuda.synchronize()
            assert oa.shape == ob.shape and oa.shape[2] > 0 and torch.equal(oa, ob), f"{name}: outputs differ"
        path = b_obj.stage2._plan.last_strided_input()
        side_a, side_b = (lambda: a_obj.execute(x)), (lambda: b_obj.execute(x))
        for _ in range(2):
            timeit(torch, side_a, reps)
            timeit(torch, side_b, reps)
        ta, tb = [], []
        for _ in range(rounds):
            ta.append(timeit(torch, side_a, reps))
            tb.append(timeit(torch, side_b, reps))
        med_a, med_b = float(np.median(ta)), float(np.median(tb))
        print(json.dumps({
            "kernel": "twostage_inverse", "shape": name, "rows": rows, "n_coarse": n_coarse, "nch_in": nch2,
            "path": path, "calls_per_window": reps, "windows": rounds, "outputs_equal": True,
            "A_gather_ms": [round(t, 4) for t in ta], "B_strided_ms": [round(t, 4) for t in tb],
            "A_median_ms": round(med_a, 4), "B_median_ms": round(med_b, 4),
            "A_spread_ms": round(max(ta) - min(ta), 4), "B_spread_ms": round(max(tb) - min(tb), 4),
            "B_below_A_by_ms": round(med_a - med_b, 4),
            "grid_order": os.environ.get("PFB_STRIDED_SHARE", "default"),
            "samples": rows * n_coarse * nch2}), flush=True)
        del x, a_obj, b_obj, sides, oa, ob
        torch.cuda.empty_cache()


def cpu_baselines(pfb):
    """The reference's CPU path stand-in (the NumPy oracle, complex64 where Matlab uses
    single, numpy.fft single-threaded) on bounded samples of the other configurations."""
    import time
    from oracle import pfb_oracle as orc
    rng = np.random.default_rng(0)

    def noise(n, n_pol=1):
        return ((rng.standard_normal((n_pol, 1, n)) + 1j * rng.standard_normal((n_pol, 1, n))) /
                np.sqrt(2)).astype(np.complex64)

    def timed(fn, samples, what, sample):
        t0 = time.perf_counter()
        fn()
        el = time.perf_counter() - t0
        print(json.dumps({"cpu": what, "msamples_per_s": round(samples / el / 1e6, 3),
                          "cores": 1, "kind": "port", "sample": sample,
                          "seconds": round(el, 2)}), flush=True)

    taps43 = pfb.design_PFB_FIR_filter(256, "4/3", 12)
    x = noise(1 << 20)
    win = orc.pfb_window("tukey", 256, 48)
    dr = {"apply_deripple": 1, "filter_coeff": taps43}
    timed(lambda: orc.polyphase_synthesis(
        orc.polyphase_analysis(x, taps43, 256, "4/3", dtype=np.complex64), 1, 256, "4/3", dr, 1,
        48, win, dtype=np.complex64), 1 << 20, "C2' round trip", "2^20 samples")
    pst = pfb.read_fir_filter_coeff(os.path.join(pfb.config.config_dir, "PST_filtertaps.txt"))
    x2 = noise(1 << 18, 2)
    timed(lambda: orc.polyphase_analysis_lowcbf(x2, pst, do_padding=False), 2 << 18,
          "LowCBF PST filterbank", "2 pol x 2^18 samples")
    tm = pfb.design_PFB_FIR_filter_two_stage(4096, "8/7", 28)
    x3 = noise(1 << 22)
    winm = orc.pfb_window("tukey", 512, 128)
    drm = {"apply_deripple": 1, "filter_coeff": tm}
    timed(lambda: orc.polyphase_synthesis(
        orc.polyphase_analysis_padded(x3, tm, 4096, "8/7", dtype=np.complex64), 1, 512, "8/7",
        drm, 1, 128, winm, dtype=np.complex64), 1 << 22, "C3 SKA-Mid round trip",
        "2^22 samples (2 synthesis blocks)")


def mid(torch, pfb, noise, dev, reps=3, inflight=1, pipeline=False, graph=False):
    tm = pfb.design_PFB_FIR_filter_two_stage(4096, "8/7", 28)
    nm = 1 << 26
    xm = noise(1, nm)
    winm = pfb.PFBWindow().lookup["tukey"](512, 128)
    pairs = []
    for _ in range(max(1, inflight)):
        anam = pfb.AnalysisPlan(tm, 4096, "8/7", "polyphase_analysis_padded", 1)
        synm = pfb.SynthesisPlan(4096, "8/7", 512, 128, True, 1, True, tm, winm, None, 1)
        Km = anam.output_length(nm)
        chm = torch.empty((1, Km, 4096), dtype=torch.complex64, device=dev)
        om = torch.empty((1, synm.output_length(Km)), dtype=torch.complex64, device=dev)
        pairs.append((anam, synm, chm, om))
    # each unit in flight reads its own input (no shared input lines between the units)
    xs = [xm] + [noise(1, nm) for _ in pairs[1:]]
    if len(pairs) == 1:
        anam, synm, chm, om = pairs[0]
        ms = timeit(torch, lambda: pfb.roundtrip(anam, synm, xm, chan=chm, out=om), reps)
    elif pipeline:
        # the split round trip as a two-stream pipeline (bench.py --pipeline): unit i's
        # FIR + row FFT on stream A beside unit i-1's synthesis on stream S
        for (a, s_, c, o), xi in zip(pairs, xs):
            pfb.roundtrip(a, s_, xi, chan=c, out=o)
        torch.cuda.synchronize()
        D = len(pairs)

        def enqueue(k):
            sa = torch.cuda.current_stream()
            ss = torch.cuda.Stream(dev)
            ss.wait_stream(sa)
            ev_a = [torch.cuda.Event() for _ in range(k)]
            ev_s = [torch.cuda.Event() for _ in range(k)]
            for i in range(k):
                a, s_, c, o = pairs[i % D]
                if i >= D:
                    sa.wait_event(ev_s[i - D])
                pfb.roundtrip_analysis(a, s_, xs[i % D], chan=c)
                ev_a[i].record(sa)
                ss.wait_event(ev_a[i])
                with torch.cuda.stream(ss):
                    pfb.roundtrip_synthesis(a, s_, nm, out=o)
                ev_s[i].record(ss)
            sa.wait_stream(ss)
        import time
        n_it = reps * D
        enqueue(D)
        torch.cuda.synchronize()
        if graph:
            # the n_it steps captured as one graph (bench.py's form; eager launches of these
            # persistent kernels on two streams interleave destructively)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                enqueue(n_it)
            g.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
        else:
            t0 = time.perf_counter()
            enqueue(n_it)
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / n_it
    else:
        # D units in flight: unit i on plan pair i mod D and stream i mod D (no dependence
        # between the pairs), so one unit's FIR / row FFT can run beside another's synthesis
        streams = [torch.cuda.Stream(dev) for _ in pairs]
        ctr = [0]

        def step():
            i = ctr[0] % len(pairs)
            ctr[0] += 1
            a, s_, c, o = pairs[i]
            with torch.cuda.stream(streams[i]):
                pfb.roundtrip(a, s_, xm, chan=c, out=o)

        def sync_all():
            torch.cuda.synchronize()
        for _ in range(len(pairs)):
            step()
        sync_all()
        import time
        n_it = reps * len(pairs)
        t0 = time.perf_counter()
        for _ in range(n_it):
            step()
        sync_all()
        ms = (time.perf_counter() - t0) * 1e3 / n_it
    emit("roundtrip C3 SKA-Mid padded 4096ch", ms, 16 * (1 + 8 / 7) * nm,
         msamples_per_s=round(nm / ms / 1e3, 1), n_taps=len(tm), units_in_flight=len(pairs),
         pipeline=bool(pipeline and len(pairs) > 1), graph=bool(graph and pipeline and len(pairs) > 1))


if __name__ == "__main__":
    main()
