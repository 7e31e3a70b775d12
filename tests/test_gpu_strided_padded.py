"""pfb_filterbank_execute_strided on polyphase_analysis_padded plans (include/pfb_api.h).

Case format (``_strided_case``): plans of one descriptor are fed the same sequence of calls.
Plan A goes through pfb_filterbank_execute; a plan B per layout goes through
pfb_filterbank_execute_strided into a buffer pre-filled with a NaN sentinel pattern.  The
expected buffer is built on the host — the sentinel buffer with exactly the mapped elements
of A's result set — and compared with B's buffer as int64 bit patterns (NaNs compare equal):
one assertion proves the values (bit-identical to the contiguous call), the index map, that
the rows [T_out, K) of the padded variant's circular shift and the chomped bins are dropped,
and that nothing else was touched.  ``n_out`` and ``buffered_samples`` are compared after
every call, and A's result is held to oracle.FilterBankOracle(..., "polyphase_analysis_padded")
at the project's 1e-6, so the suite is not self-consistent only.

Layouts, both for every shape (T = the call's T_out, C = N):
  * channel-major — row_stride 1, chan_stride = T rounded up to 16, out_pol_stride = C x that
    (a cascade's stage-1 product);
  * assembled and chomped — row_stride = n_pol nsel, chan_stride 1, out_pol_stride = nsel,
    sel = (nsel / 2 - 1, N - nsel, nsel) with nsel = N de / nu (TwoStageFilterBank.m:102-105).

Kernels: analysis_fused_kernel's strided store (N <= 256, <= 32 tap phases), row_fft_kernel's
(the FIR + row-FFT path: N = 64 with 33 phases, N = 512, 2048) and the 4096-point pair kernel
that pairs by output row (row_fft4096_pair_strided_kernel).
"""
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest

from conftest import assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

PADDED = "polyphase_analysis_padded"
OK, INVALID_ARG, UNSUPPORTED, TOO_SMALL = 0, 1, 2, 5
# two distinct quiet-NaN payloads (re, im): a store of any computed value changes the pattern
_SENT32 = np.array([0x7FC0DEAD, 0x7FC0BEEF], dtype=np.uint32)
SENT64 = int(_SENT32.view(np.int64)[0])
GUARD = 37  # sentinel elements past the furthest mapped one


def _pfb():
    import ska_pst_dsp_model_amd as pfb
    return pfb


def _lib():
    from ska_pst_dsp_model_amd import _lib as L
    return L.load()


def _noise(rng, shape):
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)


def _stream(dev):
    import torch
    return c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _sentinel(dev, n):
    """n complex64 elements holding the sentinel, as an int64 device tensor."""
    import torch
    return torch.full((int(n),), SENT64, dtype=torch.int64, device=dev)


def _chomp(N, nu, de):
    nsel = N * de // nu
    return nsel // 2 - 1, N - nsel, nsel


def _layouts(N, nu, de, n_pol, T):
    """name -> (lead, out_pol_stride, row_stride, chan_stride, sel) for a call returning T rows."""
    Tc = max(16, (T + 15) // 16 * 16)
    split, shift, nsel = _chomp(N, nu, de)
    return {"channel-major": (2, N * Tc, 1, Tc, (0, 0, 0)),
            "assembled": (2, nsel, n_pol * nsel, 1, (split, shift, nsel))}


def _index_map(N, n_pol, T, ps, rs, cs, sel):
    """(flat element offsets (n_pol, T, kept), kept bins c) of the documented store map."""
    split, shift, nsel = sel
    c = np.arange(N)
    if nsel > 0:
        j = np.where(c < split, c, c - shift)
        keep = ((c < split) | (c >= split + shift)) & (j < nsel)
        c, j = c[keep], j[keep]
    else:
        j = c
    idx = (np.arange(n_pol)[:, None, None] * ps + np.arange(T)[None, :, None] * rs + j[None, None, :] * cs)
    return idx.astype(np.int64), c


def _exec_contig(lib, plan, x, dev):
    """pfb_filterbank_execute on exact contiguous buffers -> (T_out, (n_pol, T_out, C) tensor)."""
    import torch
    n_pol, n_in = x.shape
    C = plan.out_chan
    Kt = int(lib.pfb_filterbank_output_rows(plan._h, n_in))
    out = torch.empty((n_pol, max(Kt, 1) * C), dtype=torch.complex64, device=dev)
    n = c_int64(-1)
    st = lib.pfb_filterbank_execute(plan._h, c_void_p(x.data_ptr()), n_in, n_in, c_void_p(out.data_ptr()),
                                    max(Kt, 1) * C, Kt, byref(n), 0, _stream(dev))
    assert st == OK and int(n.value) == Kt, lib.pfb_last_error()
    return Kt, out[:, :Kt * C].reshape(n_pol, Kt, C)


def _exec_strided(lib, plan, x, buf, lead, ps, rs, cs, sel, cap, dev):
    n = c_int64(-1)
    st = lib.pfb_filterbank_execute_strided(
        plan._h, c_void_p(x.data_ptr()), x.shape[1], x.shape[1], c_void_p(buf.data_ptr() + 8 * lead),
        ps, rs, cs, sel[0], sel[1], sel[2], cap, byref(n), _stream(dev))
    return st, int(n.value)


def _strided_case(dev, taps, N, os_, n_pol, calls, seed, check=None, extra_layouts=None):
    """The case format of the module docstring; check(call index, K, T_out, B, plan) asserts
    the shape's stated property.  Returns the number of strided calls compared."""
    import torch
    pfb, lib = _pfb(), _lib()
    plan_a = pfb.AnalysisPlan(taps, N, os_, PADDED, n_pol, 0)
    nu, de = plan_a.os_factor.nu, plan_a.os_factor.de
    M = plan_a.step
    names = list(_layouts(N, nu, de, n_pol, 16)) + list(extra_layouts or ())
    plans_b = {k: pfb.AnalysisPlan(taps, N, os_, PADDED, n_pol, 0) for k in names}
    ofb = orc.FilterBankOracle(taps, N, os_, PADDED)
    rng = np.random.default_rng(seed)
    done = 0
    for i, n_in in enumerate(calls):
        w = f"padded N={N} {os_} n_pol={n_pol} call {i} ({n_in} samples)"
        xh = _noise(rng, (n_pol, n_in))
        x = torch.from_numpy(xh).to(dev)
        B = plan_a.buffered_samples
        assert B == ofb.buffered_samples, w
        K = (B + n_in) // M
        T, base = _exec_contig(lib, plan_a, x, dev)
        assert T == K - K % nu and T > 0, w
        if check:
            check(i, K, T, B, plan_a)
        ref = ofb.execute(xh[:, None, :])
        assert ref.shape == (n_pol, N, T), (w, ref.shape)
        assert_pfb_close(base.cpu().numpy().transpose(0, 2, 1), ref, what=w)
        base64 = torch.view_as_real(base.contiguous()).view(torch.int64).reshape(n_pol, T, N).cpu().numpy()
        lays = _layouts(N, nu, de, n_pol, T)
        for k in extra_layouts or ():
            lays[k] = extra_layouts[k](lays)
        for name, (lead, ps, rs, cs, sel) in lays.items():
            idx, kept = _index_map(N, n_pol, T, ps, rs, cs, sel)
            assert np.unique(idx).size == idx.size, (w, name)
            cap = int(idx.max()) + 1          # exactly the furthest written element
            total = lead + cap + GUARD
            buf = _sentinel(dev, total)
            assert plans_b[name].buffered_samples == B, (w, name)
            st, n = _exec_strided(lib, plans_b[name], x, buf, lead, ps, rs, cs, sel, cap, dev)
            torch.cuda.synchronize(dev)
            assert st == OK, (w, name, lib.pfb_last_error())
            assert n == T, (w, name)
            # (max: with nu M < de N — 5/3 at N = 16 — the reference's input_idat = T N de / nu,
            # FilterBank.m:119, overruns the input and the oracle's count goes negative; the
            # library keeps nothing.  Such a shape is fed one call.)
            assert plans_b[name].buffered_samples == plan_a.buffered_samples == max(ofb.buffered_samples, 0), \
                (w, name)
            exp = np.full(total, SENT64, dtype=np.int64)
            exp[lead + idx] = base64[:, :, kept]
            got = buf.cpu().numpy()
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (f"{w} [{name}]: {bad.size} of {total} elements differ from the mapped "
                                   f"contiguous result (first at {bad[:5] - lead} past the base)")
            done += 1
    return done


# ----------------------------------------------------------------------------- fused kernel
def test_fused_n16_tile_trim_and_carry(gpu):
    """N 16, 8/7, 10 taps per channel, 3 pols, calls of 5000 / 3001 / 4099 samples: K exceeds
    the fused kernel's 256-row workgroup tile, one call has K mod nu != 0 (rows [T_out, K)
    dropped at the store), and calls 2 and 3 carry samples (the fused-carry path, the carry
    read through AnalysisArgs::pre)."""
    taps = _pfb().design_PFB_FIR_filter(16, "8/7", 10)
    seen = {"tile": False, "trim": False, "carry": 0}

    def check(i, K, T, B, plan):
        seen["tile"] |= K > 256
        seen["trim"] |= K % 8 != 0
        if i > 0:
            assert B > 0
            seen["carry"] += 1
    assert _strided_case(gpu, taps, 16, "8/7", 3, (5000, 3001, 4099), 501, check) == 6
    assert seen == {"tile": True, "trim": True, "carry": 2}, seen


def test_fused_n16_shift_wraps_twice(gpu):
    """N 16, 4/3, a first call of 63 samples: K = 5 and T_out = 4 lie below sds = 7, so the
    circular shift wraps more than once; then a 2000-sample call."""
    pfb = _pfb()
    taps = pfb.design_PFB_FIR_filter(16, "4/3", 10)
    sds = int(np.ceil((len(taps) - 1) / 2 / 12))

    def check(i, K, T, B, plan):
        if i == 0:
            assert (K, T, sds) == (5, 4, 7) and sds > K
    _strided_case(gpu, taps, 16, "4/3", 2, (63, 2000), 502, check)


def test_fused_n16_step_with_remainder(gpu):
    """N 16, 5/3, 12 * 16 + 1 random taps: M = floor(16 * 3 / 5) = 9 leaves a remainder (nu M
    != de N), the shape whose barrel shift differs from (M k) mod N.  One call: the stream
    object's carry is not defined for this factor (the reference consumes T N de / nu = 3168 of
    the 3000 samples)."""
    taps = np.random.default_rng(503).standard_normal(12 * 16 + 1) / 8.0

    def check(i, K, T, B, plan):
        assert plan.step == 9 and 5 * plan.step != 3 * 16 and (K, T) == (333, 330)
    _strided_case(gpu, taps, 16, "5/3", 2, (3000,), 503, check)


def test_fused_n256(gpu):
    """N 256, 8/7, 11 taps per channel, 2 pols, two calls of about 60 000 samples (the fused
    kernel's 16-row tile, P = 11 exact instantiation; the second call carries)."""
    taps = _pfb().design_PFB_FIR_filter(256, "8/7", 11)
    _strided_case(gpu, taps, 256, "8/7", 2, (60_000, 59_999), 504)


# ----------------------------------------------------------------------------- FIR + row FFT
def test_generic_n64_many_phases(gpu):
    """N 64, 4/3, 33 taps per channel: P = 33 > 32 sends an N <= 256 plan to the generic FIR +
    row_fft_kernel<64, +1>."""
    taps = np.random.default_rng(505).standard_normal(33 * 64) / 16.0

    def check(i, K, T, B, plan):
        assert plan.phases == 33
    _strided_case(gpu, taps, 64, "4/3", 2, (3000, 2501), 505, check)


@pytest.mark.parametrize("N,n_taps", [(512, 28 * 512), (2048, 12 * 2048 + 1)])
def test_generic_row_fft(gpu, N, n_taps):
    """N 512 (28 random taps per channel) and N 2048 (12 N + 1 random taps), 4/3, about 40 rows
    per call, two calls: row_fft_kernel<N, +1>'s strided store; the second call concatenates
    the carry (the N > 256 path)."""
    taps = np.random.default_rng(506 + N).standard_normal(n_taps) / 32.0
    M = N * 3 // 4

    def check(i, K, T, B, plan):
        assert 36 <= K <= 44
        if i == 1:
            assert B > 0
    _strided_case(gpu, taps, N, "4/3", 2, (40 * M + 100, 41 * M + 7), 506 + N, check)


@pytest.mark.parametrize("n_pol", [1, 2])
def test_generic_n4096_pairs_by_output_row(gpu, n_pol):
    """N 4096, 8/7, 12 N + 1 random taps, about 41 rows per call: the 4096-point pair kernel
    pairs by output row.  sds is odd, so FIR rows (2p, 2p + 1) would land at output rows
    starting odd and straddle the wrap — the misaligned-pair case; K is odd in call 1 and
    even in call 2.  n_pol 1 adds channel-major at an odd (8-B, not 16-B aligned) base: the
    8-byte fallback of the 16-byte pair store."""
    taps = np.random.default_rng(507).standard_normal(12 * 4096 + 1) / 64.0
    M = 3584
    sds = int(np.ceil((len(taps) - 1) / 2 / M))
    assert sds % 2 == 1
    n1 = 41 * M + 100
    n2 = 42 * M - (n1 - 40 * M) + 50
    ks = []

    def check(i, K, T, B, plan):
        ks.append(K)
    extra = None
    if n_pol == 1:
        extra = {"channel-major, odd base": lambda lays: (1,) + lays["channel-major"][1:]}
    _strided_case(gpu, taps, 4096, "8/7", n_pol, (n1, n2), 507, check, extra)
    assert ks == [41, 42], ks


# ----------------------------------------------------------------------------- cascades
def _padded_cfg(taps, n):
    return dict(analysis_function=PADDED, filt_coeff=taps, channels=n, os_factor="8/7")


def _cascade(taps1, nch1, taps2, nch2, critical, single, strided):
    ts = _pfb().TwoStageFilterBank(_padded_cfg(taps1, nch1)).set_stage2_config(_padded_cfg(taps2, nch2))
    ts.critical, ts.single = critical, single
    ts.strided = strided
    # (the comparison is of the two mechanisms, whatever the measured default of a stage is)
    ts.strided_stages = [True, True] if strided else [None, None]
    return ts


@pytest.mark.parametrize("critical,single", [(0, 0), (1, 0), (0, 1)])
def test_two_stage_padded_strided_equals_gather(gpu, critical, single):
    """Padded 64 x 16 cascade, two calls: both stages strided equals the corner-turn / gather
    path bit for bit."""
    import torch
    pfb = _pfb()
    taps1 = pfb.design_PFB_FIR_filter(64, "8/7", 12)
    taps2 = pfb.design_PFB_FIR_filter(16, "8/7", 10)
    a = _cascade(taps1, 64, taps2, 16, critical, single, True)
    b = _cascade(taps1, 64, taps2, 16, critical, single, False)
    rng = np.random.default_rng(510)
    for n in (300_000, 123_457):
        x = torch.from_numpy(_noise(rng, (2, 1, n))).to(gpu)
        _, ya = a.execute(x)
        _, yb = b.execute(x)
        assert ya.shape == yb.shape and ya.shape[2] > 0
        assert torch.equal(ya.contiguous(), yb.contiguous()), f"critical={critical} single={single} n={n}"
        assert a.stage1.buffered_samples == b.stage1.buffered_samples
        assert a.stage2.buffered_samples == b.stage2.buffered_samples


def test_two_stage_padded_needs_no_corner_turn_or_gather(gpu, monkeypatch):
    """The padded 64 x 16 cascade completes with layout.corner_turn and layout.gather_channels
    replaced by functions that raise: both stages store strided."""
    import torch
    pfb = _pfb()
    from ska_pst_dsp_model_amd import layout

    def boom(*a, **k):
        raise AssertionError("the strided cascade called a corner turn / gather")
    monkeypatch.setattr(layout, "corner_turn", boom)
    monkeypatch.setattr(layout, "gather_channels", boom)
    taps1 = pfb.design_PFB_FIR_filter(64, "8/7", 12)
    taps2 = pfb.design_PFB_FIR_filter(16, "8/7", 10)
    ts = _cascade(taps1, 64, taps2, 16, 1, 0, True)
    rng = np.random.default_rng(511)
    for n in (300_000, 123_457):
        x = torch.from_numpy(_noise(rng, (1, 1, n))).to(gpu)
        _, y = ts.execute(x)
        assert y.shape[1] == 64 * 14 and y.shape[2] > 0


def test_two_stage_padded_4096x16_strided_equals_gather(gpu):
    """4096 x 16 critical cascade, random 12 * 4096 + 1-tap stage 1, one pol, two calls of about
    1.5 M samples: strided equals the corner-turn / gather path bit for bit (stage 1 through
    the pair kernel's 16-byte channel-major stores, stage 2 through the fused kernel's
    112-byte runs over 4096 series)."""
    import torch
    pfb = _pfb()
    taps1 = np.random.default_rng(512).standard_normal(12 * 4096 + 1) / 64.0
    taps2 = pfb.design_PFB_FIR_filter(16, "8/7", 10)
    a = _cascade(taps1, 4096, taps2, 16, 1, 0, True)
    b = _cascade(taps1, 4096, taps2, 16, 1, 0, False)
    rng = np.random.default_rng(513)
    for n in (1_500_000, 1_400_003):
        x = torch.from_numpy(_noise(rng, (1, 1, n))).to(gpu)
        _, ya = a.execute(x)
        _, yb = b.execute(x)
        assert ya.shape == yb.shape and ya.shape[1] == 4096 * 14 and ya.shape[2] > 0
        assert torch.equal(ya.contiguous(), yb.contiguous()), n


# ----------------------------------------------------------------------------- rejections
def test_padded_strided_rejections(gpu):
    """A padded N = 16 plan: the three bad layouts of the Bunton rejection test are
    PFB_ERR_INVALID_ARG, a capacity one element short of the furthest write is
    PFB_ERR_BUFFER_TOO_SMALL with the sentinel buffer untouched, a LowCBF plan is
    PFB_ERR_UNSUPPORTED; the carry is unchanged each time."""
    import torch
    pfb, lib = _pfb(), _lib()
    taps = pfb.design_PFB_FIR_filter(16, "8/7", 10)
    plan = pfb.AnalysisPlan(taps, 16, "8/7", PADDED, 2, 0)
    rng = np.random.default_rng(520)
    x0 = torch.from_numpy(_noise(rng, (2, 1000))).to(gpu)
    plan.execute(x0, stateful=True)          # leave a carry behind
    B = plan.buffered_samples
    assert B > 0
    x = torch.from_numpy(_noise(rng, (2, 3000))).to(gpu)
    T = plan.stream_rows(3000)
    assert T > 0
    Tc = (T + 15) // 16 * 16
    total = 2 * 16 * Tc
    for rs, cs, sel in ((0, 1, (0, 0, 0)), (1, Tc, (12, 6, 10)), (1, Tc, (0, 0, 17))):
        buf = _sentinel(gpu, total)
        st, _ = _exec_strided(lib, plan, x, buf, 0, 16 * Tc, rs, cs, sel, total, gpu)
        torch.cuda.synchronize(gpu)
        assert st == INVALID_ARG and plan.buffered_samples == B, (rs, cs, sel)
        assert bool((buf == SENT64).all())
    # furthest write of the channel-major layout: (n_pol-1) ps + (T-1) rs + (C-1) cs
    last = 16 * Tc + (T - 1) + 15 * Tc
    buf = _sentinel(gpu, total)
    st, n = _exec_strided(lib, plan, x, buf, 0, 16 * Tc, 1, Tc, (0, 0, 0), last, gpu)
    torch.cuda.synchronize(gpu)
    assert st == TOO_SMALL and plan.buffered_samples == B
    assert bool((buf == SENT64).all())
    # ... and with exactly that element available the call goes through
    st, n = _exec_strided(lib, plan, x, buf, 0, 16 * Tc, 1, Tc, (0, 0, 0), last + 1, gpu)
    torch.cuda.synchronize(gpu)
    assert st == OK and n == T and plan.buffered_samples != B
    assert int((buf != SENT64).sum()) == 2 * 16 * T
    # LowCBF
    pst = pfb.read_fir_filter_coeff(__import__("os").path.join(pfb.config.config_dir, "PST_filtertaps.txt"))
    low = pfb.AnalysisPlan(pst, 256, "4/3", "polyphase_analysis_lowcbf", 1, 0)
    xl = torch.from_numpy(_noise(rng, (1, 20_000))).to(gpu)
    low.execute(xl, stateful=True)
    Bl = low.buffered_samples
    bufl = _sentinel(gpu, 216 * 256)
    st, _ = _exec_strided(lib, low, xl, bufl, 0, 216 * 256, 1, 256, (0, 0, 0), 216 * 256, gpu)
    torch.cuda.synchronize(gpu)
    assert st == UNSUPPORTED and low.buffered_samples == Bl
    assert bool((bufl == SENT64).all())
