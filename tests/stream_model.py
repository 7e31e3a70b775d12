"""A plain-integer restatement of the two stream-object state machines of the C ABI:
``filterbank_exec`` (pfb_filterbank_execute / _strided / _dada) and ``ifb_check`` / ``ifb_go``
(pfb_inverse_filterbank_execute / _strided / _dada) in
ska-pst-dsp-model_amd/csrc/pfb_api_analysis.hip and pfb_api_synthesis.hip.

No torch, no GPU, no test in here: given a plan's integers and a list of chunk lengths the
functions return one record per call — which path the call takes, what it returns, what it
leaves buffered and which boundary of the path predicates it sits on.  tests/test_stream_model.py
checks the model against what existing GPU tests assert and proves the reachability bound the
one-launch path rests on; tests/test_gpu_stream_edges.py drives the plans through the sequence
tables below and compares every call with the model.

The comments name the function (and where useful the branch) of those two files that a line
restates, unless they say otherwise.
"""
from collections import namedtuple

BUNTON, PADDED, LOWCBF = "bunton", "padded", "lowcbf"

# how a call hands its samples over (the device entries share one carry):
#   analysis : packed, strided (device cf32 behind pfb_filterbank_execute / _strided), host,
#              dada_fused / dada_staged (pfb_filterbank_execute_dada, by analysis_dada_fusable)
#   synthesis: packed, strided, dada (device), host
ANALYSIS_ENTRIES = ("packed", "strided", "host", "dada_fused", "dada_staged")
SYNTHESIS_ENTRIES = ("packed", "strided", "dada", "host")


def floordiv(a, b):
    return a // b  # Python's // floors like pfb_host.hpp's floordiv


# ============================================================================ analysis
class AnalysisShape(namedtuple("AnalysisShape", "variant N nu de P")):
    """(variant, N, nu, de, P) of an analysis plan; P = ceil(n_taps / N) (analysis_validate)."""

    @property
    def M(self):
        return (self.N * self.de) // self.nu  # analysis_validate

    @property
    def PN(self):
        return self.P * self.N

    @property
    def stream_kernel(self):
        """stream_shape (csrc/pfb_analysis.hip): the N 256 streaming kernel."""
        return (self.variant == BUNTON and self.N == 256 and (self.nu, self.de) in ((8, 7), (4, 3))
                and self.P in (12, 13))

    @property
    def fused(self):
        """pfb_analysis_plan::fused (analysis_validate; analysis_supported, csrc/pfb_analysis.hip)."""
        if self.variant == LOWCBF:
            return True
        return 8 <= self.N <= 256 and self.N & (self.N - 1) == 0 and self.P <= 32

    @property
    def fused_takes_carry(self):
        """analysis_fused_takes_carry (csrc/pfb_analysis.hip)."""
        return self.fused and not self.stream_kernel and self.variant != LOWCBF

    @property
    def window(self):
        """The streaming kernel's first register window in samples (filterbank_exec, one-launch path: `win`)."""
        return (self.de * (16 // self.nu) + self.P) * self.N

    @property
    def max_carry(self):
        """total - Kt M with K - Kt < nu and total - K M < P N + M (the pre-pad of LowCBF
        only shortens what a first call needs)."""
        return self.PN + self.nu * self.M - 1


def analysis_K(shape, n_dat, pad_due=False):
    """analysis_K."""
    if shape.variant == LOWCBF:
        return max(floordiv(n_dat + (1536 if pad_due else 0) - 3072, 192), 0)  # LowCBF branch
    if shape.variant == BUNTON:
        return max(floordiv(n_dat - shape.PN, shape.M), 0)  # Bunton branch
    return max(n_dat // shape.M, 0)  # padded


AnalysisCall = namedtuple(
    "AnalysisCall", "n_in entry carry_before K Kt input_idat rows carry_after path pad pad_due flags")


def analysis_call(shape, B, n_in, entry="packed", pad_due=False):
    """One filterbank_exec call on a state of B buffered samples (its lengths: fb_lens).  Returns the
    record and the pad flag after the call."""
    assert entry in ANALYSIS_ENTRIES and n_in >= 0 and B >= 0
    device = entry != "host"
    sec = entry.startswith("dada")
    fus = entry == "dada_fused"
    total = B + n_in  # fb_lens
    K = analysis_K(shape, total, pad_due)  # fb_lens
    Kt = K - K % shape.nu  # fb_lens: the nu trim (FilterBank.m:93-104)
    input_idat = (Kt * shape.N * shape.de) // shape.nu  # fb_lens (FilterBank.m:119-126)
    pad = 0
    if (device and 0 < B <= shape.window  # filterbank_exec, one-launch path
            and ((shape.variant == BUNTON and shape.stream_kernel) or (fus and shape.variant == LOWCBF))
            and input_idat >= B and not pad_due and (not sec or fus)):
        path, pad = "one_launch", B
    elif (not sec and device and B > 0 and not pad_due and shape.fused and shape.fused_takes_carry
          and input_idat >= B and Kt > 0):  # filterbank_exec, fused-with-pre path
        path, pad = "fused_pre", B
    elif B == 0 and device and (not sec or fus):  # filterbank_exec, `in_place`
        path = "in_place"
    else:
        path = "concat"
    carry_after = max(total - input_idat, 0)  # fb_lens nb, fb_carry
    via_pre = path in ("one_launch", "fused_pre")
    flags = set()
    if B > 0 and input_idat == B:
        flags.add("idat_eq_carry")
    if Kt > 0 and B > 0 and input_idat < B:
        flags.add("rows_from_concat")
    if via_pre and B < shape.PN:
        flags.add("carry_lt_PN")
    if via_pre and B % shape.N:
        flags.add("carry_not_mult_N")
    if n_in == 0 and B > 0:
        flags.add("zero_len_call")
    if total > 0 and carry_after == 0:
        flags.add("empty_new_carry")
    if pad_due:
        flags.add("pad_consumed")  # every accepted call consumes it, rows or not (filterbank_exec: PadConsume::accept)
    rec = AnalysisCall(n_in, entry, B, K, Kt, input_idat, Kt, carry_after, path, pad, pad_due,
                       frozenset(flags))
    return rec, False


def analysis_stream(shape, chunks, entries="packed"):
    """Records of a stream of calls from a fresh (or reset) plan.  ``entries``: one entry name
    for every call or one per call; a chunk given as the string "reset" is
    pfb_filterbank_reset and yields no record."""
    if isinstance(entries, str):
        entries = [entries] * len(chunks)
    B, pad_due, out = 0, shape.variant == LOWCBF, []
    for n, e in zip(chunks, entries):
        if n == "reset":
            B, pad_due = 0, shape.variant == LOWCBF
            continue
        rec, pad_due = analysis_call(shape, B, n, e, pad_due)
        B = rec.carry_after
        out.append(rec)
    return out


def analysis_dada_diag(rec):
    """pfb_analysis_last_dada_input after the call (include/pfb_api.h:386-400): 'none' after a
    cf32 call; FUSED where the kernel read the section in place — nothing buffered (filterbank_exec, `in_place`) or the
    one-launch carry path — else STAGED (filterbank_exec, concatenation: unpacked behind the carry)."""
    if not rec.entry.startswith("dada"):
        return "none"
    if rec.entry == "dada_fused" and rec.path in ("in_place", "one_launch"):
        return "fused"
    return "staged"


def analysis_class0_launches(rec):
    """Launches of the analysis kernel class (profile class 0) the call records: one per
    row-producing call on every path, none when no row completes."""
    return 1 if rec.rows > 0 else 0


def reachable_carries(shape, n_max=None):
    """Every carry length a stream object of this shape can hold: breadth-first from B = 0 over
    every n_in in [0, n_max), n_max = P N + 3 nu M by default.  What a call leaves behind
    depends on B and n_in only through B + n_in (and on whether the pre-pad is due, which it
    is for the first call alone), so a level of the search is the set of totals it can form —
    [0, largest carry so far + n_max) — and not every (B, n_in) pair."""
    if n_max is None:
        n_max = shape.PN + 3 * shape.nu * shape.M

    def after(total, pad_due):
        return analysis_call(shape, 0, total, "packed", pad_due)[0].carry_after

    seen = {after(t, shape.variant == LOWCBF) for t in range(n_max)}  # first calls, from B = 0
    done = 0
    while True:
        hi = max(seen) + n_max
        if hi <= done:
            return seen
        seen |= {after(t, False) for t in range(done, hi)}
        done = hi


# ============================================================================ synthesis
class SynthesisShape(namedtuple("SynthesisShape", "N nu de Nf Ov sample_offset")):
    @property
    def keep(self):
        return self.Nf - 2 * self.Ov  # input rows a block advances by

    @property
    def Lkeep(self):
        """Output samples per block: W N - 2 Lov (SynthesisPlan.__init__)."""
        W = (self.Nf * self.de) // self.nu
        return W * self.N - 2 * ((self.Ov * self.de * self.N) // self.nu)


def synth_blocks(shape, n_dat):
    """synth_blocks."""
    return max(floordiv(n_dat - 2 * shape.Ov, shape.keep), 0)


SynthesisCall = namedtuple(
    "SynthesisCall", "n_in entry carry_before blocks input_idat rows full carry_after path b_s stitched_new "
                     "flags")


def synthesis_call(shape, Bc, n_in, entry="packed", spectral=False):
    """One stream call (ifb_check, ifb_go) on a state of Bc buffered rows (its lengths: ifb_lens).  ``rows`` is the output
    length in samples; a rejected call leaves the carry as it was."""
    assert entry in SYNTHESIS_ENTRIES and n_in >= 0 and Bc >= 0
    total = Bc + n_in  # ifb_lens
    so = min(shape.sample_offset, total)  # ifb_lens
    B = synth_blocks(shape, total - so)  # ifb_lens
    full = B * shape.Lkeep
    input_idat = B * shape.keep
    buffered = total - input_idat
    olen = full
    flags = set()
    rem = buffered % shape.nu  # ifb_lens (Python's % is already non-negative)
    if rem:
        # carry rounded up to a multiple of nu (InverseFilterBank.m:104-135), ifb_lens
        buffered += shape.nu - rem
        input_idat = total - buffered
        olen = min(max(0, floordiv(input_idat * shape.N * shape.de, shape.nu)), full)
        flags.add("rounded_carry")
    if n_in == 0 and Bc > 0:
        flags.add("zero_len_call")
    if input_idat < 0:  # ifb_check: the call is rejected
        flags.discard("rounded_carry")
        return SynthesisCall(n_in, entry, Bc, B, input_idat, 0, full, Bc, "rejected", 0, 0,
                             frozenset(flags | {"rejected"}))
    if olen < full:
        flags.add("olen_lt_full")
    b_s = stitched_new = 0
    if entry != "host" and Bc > 0 and not spectral and input_idat >= Bc:  # ifb_go, split path
        if olen > 0:
            # first block that starts at or after row Bc of the concatenation (ifb_go, split path: b_s)
            b_s = min(B, max(0, (Bc - so + shape.keep - 1) // shape.keep))
            if b_s > 0:
                L = min(total, so + (b_s - 1) * shape.keep + shape.Nf)  # the stitched buffer's rows
                stitched_new = max(L - Bc, 0)
        path = "split(%d, %d)" % (b_s, B)
        if input_idat == Bc:
            flags.add("idat_eq_carry")
    elif Bc == 0 and entry != "host":  # ifb_go, nothing buffered
        path = "in_place"
    else:
        path = "concat"
    if total > 0 and buffered == 0:
        flags.add("empty_new_carry")
    return SynthesisCall(n_in, entry, Bc, B, input_idat, olen, full, max(buffered, 0), path, b_s,
                         stitched_new, frozenset(flags))


def synthesis_stream(shape, chunks, entries="packed", spectral=False):
    if isinstance(entries, str):
        entries = [entries] * len(chunks)
    Bc, out = 0, []
    for n, e in zip(chunks, entries):
        if n == "reset":
            Bc = 0
            continue
        rec = synthesis_call(shape, Bc, n, e, spectral)
        Bc = rec.carry_after
        out.append(rec)
    return out


def synthesis_diag(rec, reads_in_place=True):
    """(last_strided_input, last_dada_input) after an ACCEPTED call (include/pfb_api.h:354-356,
    437-439).  ``reads_in_place``: the plan's channel IFFT can read the layout / the section
    itself (strided_in_place / dada_fusable); otherwise every strided or DADA call
    is staged whole (synth_rows: strided_stage, dada_stage).  In place where any block of new rows is read through the
    entry (blocks [b_s, B) of the split path, every block with nothing buffered); staged where
    only the copy kernel touched the new rows (stitched head, carry, concatenation:
    SynthRows::copy_to); none where nothing of the entry was read."""
    if rec.entry not in ("strided", "dada"):
        return "none", "none"
    if not reads_in_place:
        d = "staged"
    elif rec.path == "in_place":
        d = "in_place" if rec.rows > 0 else "staged" if rec.carry_after > 0 else "none"
    elif rec.path == "concat":
        d = "staged"  # SynthRows::copy_to runs for every concatenation (ifb_go)
    else:
        if rec.rows > 0 and rec.b_s < rec.blocks:
            d = "in_place"
        elif rec.stitched_new > 0 or rec.carry_after > 0:
            d = "staged"
        else:
            d = "none"
    if rec.entry == "strided":
        return d, "none"
    return "none", {"in_place": "fused"}.get(d, d)


def synthesis_launches(rec, chunk_blocks=0):
    """(class-1, class-2) profiler records of the call: every chunk of a block range gives one
    channel-IFFT and one block launch (synthesis_chunk), and a range of nb > 0 blocks is
    ceil(nb / CB) chunks (synthesis_range; CB = chunk_blocks, or the whole range when 0: the default
    chunk is far larger than any range of the tables here).  The split path runs the ranges
    [0, b_s) and [b_s, B), every other path [0, B), each only when the call returns samples; a
    rejected call launches nothing."""
    if rec.path == "rejected" or rec.rows <= 0:
        return 0, 0
    ranges = [(0, rec.b_s), (rec.b_s, rec.blocks)] if rec.path.startswith("split") else [(0, rec.blocks)]
    n = sum(-(-(hi - lo) // (chunk_blocks if chunk_blocks > 0 else hi - lo)) for lo, hi in ranges if hi > lo)
    return n, n


# ============================================================================ sequence tables
# The tables tests/test_gpu_stream_edges.py drives, each with the edges it claims;
# tests/test_stream_model.py asserts every claim on the CPU.


# ---- 1. Bunton on the N 256 streaming kernel
STREAM_SHAPES = {
    "8over7-p13": AnalysisShape(BUNTON, 256, 8, 7, 13),
    "4over3-p13": AnalysisShape(BUNTON, 256, 4, 3, 13),
    "8over7-p12": AnalysisShape(BUNTON, 256, 8, 7, 12),
    "4over3-p12": AnalysisShape(BUNTON, 256, 4, 3, 12),
}
LOWCBF_SHAPE = AnalysisShape(LOWCBF, 256, 4, 3, 12)


def _carry_after(shape, chunks):
    recs = analysis_stream(shape, chunks)
    return recs[-1].carry_after if recs else 0


def bunton_main_chunks(s):
    """The recipe behind 5376, 3328, 1791, 1, 0, 3584, 3327, 1, 255, 1, 1, 20000 (8/7, 13
    phases) at any streaming shape, with R = nu M and B0 the multiple of R in [P N, P N + R):
      B0 + R    nu rows, B0 carried (a multiple of R, so Kt M can equal it)
      P N       total = P N + B0: B0 / M rows, input_idat == B0 (idat_eq_carry), P N carried
      R - 1     no row; the carry at its maximum P N + R - 1
      1         completes nu rows although input_idat = R < B (rows_from_concat)
      0         a zero-length call on P N carried samples
      B0        one launch again, P N carried
      P N - 1   rows out of the concatenation; then 1 and the distance to the maximum
      1, 1      nu rows out of the maximum, then P N + 1 carried: not a multiple of N
      20000     one launch reading P N + 1 samples through `pre`"""
    PN, R = s.PN, s.nu * s.M
    B0 = R * -(-PN // R)
    head = [B0 + R, PN, R - 1, 1, 0, B0, PN - 1, 1]
    head.append(s.max_carry - _carry_after(s, head))
    return tuple(head + [1, 1, 20000])


BUNTON_MAIN_EDGES = ("idat_eq_carry", "rows_from_concat", "zero_len_call", "carry_not_mult_N")
# a stream that starts short, three times over: `pre` holds 1, 255 and 257 samples (fewer than
# P N); the last run is 1, 254, 2, 40000 — the 254- and 2-sample calls complete no row and
# concatenate
BUNTON_SHORT_CHUNKS = (1, 9001, "reset", 255, 8999, "reset", 1, 254, 2, 40000)
BUNTON_SHORT_EDGES = ("carry_lt_PN", "carry_not_mult_N")
BUNTON_SHORT_PADS = (1, 255, 257)

# ---- 2. LowCBF (PST taps, 4/3, 12 phases, the 1536-sample pre-pad)
#   1000   no row; the pad is consumed all the same
#   2840   total 3840 = 3072 + 4 * 192: 4 rows, the carry lands on 3072 exactly
#   767    no row, the carry at its maximum 3839
#   1      completes 4 rows out of it
#   3072   total 6144: 16 rows, input_idat == 3072 == the carry (idat_eq_carry); one launch for a
#          fused section, a concatenation for cf32
#   5000   new carry inside the new samples again
#   reset  the pad is due again: 6000 samples then give (6000 + 1536 - 3072) / 192 -> 20 rows
#   3000, 0, 7000
LOWCBF_CHUNKS = (1000, 2840, 767, 1, 3072, 5000, "reset", 6000, 3000, 0, 7000)
LOWCBF_EDGES = ("pad_consumed", "rows_from_concat", "zero_len_call", "idat_eq_carry")

# ---- 3. padded on the fused kernel (N 16, 8/7, M 14, 10 N + 1 taps: 11 phases)
PADDED_FUSED_SHAPE = AnalysisShape(PADDED, 16, 8, 7, 11)
#   224   = 2 nu M: 16 rows, nothing carried (the next call must read in place)
#   113   8 rows, 1 carried;  120: `pre` holds 1 sample;  214: carry 111, the maximum
#   1     111 carried + 1 sample: 8 rows, nothing carried
#   5     shorter than M;  13: still no row;  0;  1000
PADDED_FUSED_CHUNKS = (224, 113, 120, 214, 1, 5, 13, 0, 1000)
PADDED_FUSED_EDGES = ("empty_new_carry", "carry_lt_PN", "carry_not_mult_N", "zero_len_call")

# ---- 4. padded on the FIR + row-FFT path (N 64, 4/3, M 48, 33 phases): always concatenates
PADDED_GENERIC_SHAPE = AnalysisShape(PADDED, 64, 4, 3, 33)
#   384 = 2 nu M;  193: 1 carried;  200;  182: carry 191, the maximum;  1: 4 rows, nothing carried
PADDED_GENERIC_CHUNKS = (384, 193, 200, 182, 1, 5, 40, 0, 1000)
PADDED_GENERIC_EDGES = ("empty_new_carry", "zero_len_call")

# ---- 5. / 6. InverseFilterBank
C2_SYNTH = {0: SynthesisShape(256, 8, 7, 256, 48, 0), 5: SynthesisShape(256, 8, 7, 256, 48, 5)}
# rows per call; 160 at sample_offset 0, 165 at 5 (the carry then rounds up to a multiple of nu)
C2_SYNTH_ROWS = {0: (384, 32, 224, 672, 128, 96, 0, 160, 3, 1000),
                 5: (384, 32, 224, 672, 128, 96, 0, 165, 3, 1000)}
C2_SYNTH_EDGES = {0: ("idat_eq_carry", "zero_len_call", "rejected"),
                  5: ("rounded_carry", "olen_lt_full", "zero_len_call", "rejected")}


SMALL_SYNTH = {0: SynthesisShape(8, 8, 7, 128, 16, 0), 5: SynthesisShape(8, 8, 7, 128, 16, 5)}
# the same recipe at keep = 96: multiples of nu = 8 except the 101 rows of sample_offset 5; at
# sample_offset 0 the 8-row call brings the carry to 96 = keep and the 56 rows after it make
# one block, all of it stitched, with input_idat == 96
SMALL_SYNTH_ROWS = {0: (224, 16, 136, 400, 80, 8, 56, 0, 96, 3, 600),
                    5: (224, 16, 136, 400, 80, 8, 56, 0, 101, 3, 600)}
SMALL_SYNTH_EDGES = C2_SYNTH_EDGES


def rotations(entries):
    """Every cyclic shift of the entry list: call i of rotation r goes through
    entries[(i + r) % len(entries)], so each call meets each entry once."""
    n = len(entries)
    return [tuple(entries[(i + r) % n] for i in range(n)) for r in range(n)]


def describe(recs):
    """One printable line per record (the pull request's tables are this printout)."""
    lines = []
    for i, r in enumerate(recs):
        line = "%2d  n_in %6d  carry %5d -> %5d  rows %6d  %-13s %s" % (
            i, r.n_in, r.carry_before, r.carry_after, r.rows, r.path, ",".join(sorted(r.flags)))
        lines.append(line.rstrip())
    return "\n".join(lines)


def _printout():
    """Every table with the path and edges per call, and the reachable-carry maxima."""
    for name, s in STREAM_SHAPES.items():
        for tag, chunks in (("main", bunton_main_chunks(s)), ("short", BUNTON_SHORT_CHUNKS)):
            print("bunton %s %s %s" % (name, tag, chunks))
            print(describe(analysis_stream(s, chunks)))
    for tag, s, chunks, entry in (("lowcbf, fused DADA entry", LOWCBF_SHAPE, LOWCBF_CHUNKS, "dada_fused"),
                                  ("lowcbf, cf32 entry", LOWCBF_SHAPE, LOWCBF_CHUNKS, "packed"),
                                  ("padded fused", PADDED_FUSED_SHAPE, PADDED_FUSED_CHUNKS, "packed"),
                                  ("padded generic", PADDED_GENERIC_SHAPE, PADDED_GENERIC_CHUNKS, "packed")):
        print("%s %s" % (tag, chunks))
        print(describe(analysis_stream(s, chunks, entry)))
    for tag, shapes, rows in (("c2", C2_SYNTH, C2_SYNTH_ROWS), ("small", SMALL_SYNTH, SMALL_SYNTH_ROWS)):
        for so in (0, 5):
            print("synthesis %s sample_offset %d %s" % (tag, so, rows[so]))
            print(describe(synthesis_stream(shapes[so], rows[so])))
    for name, s in list(STREAM_SHAPES.items()) + [("lowcbf", LOWCBF_SHAPE)]:
        print("reachable carry %s: max %d, window %d" % (name, max(reachable_carries(s)), s.window))


if __name__ == "__main__":
    _printout()
