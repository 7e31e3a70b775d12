"""GPU tests of the verification kernels (csrc/pfb_verify.hip) and of the device path of the
purity sweep built on them (verify.device_vectors, verify.score_vectors_device,
verify.purity_sweep(scoring="device")).  The reference of every comparison is the existing
NumPy function of verify.py, run on the same data copied to the host.

Tolerances: the scores accumulate in double, so a maximum, a single power and an index agree
with NumPy to a few ulp (asserted: relative 1e-12, indices equal); a sum of n <= 2^23 positive
terms taken in another order differs by at most n 2^-53 relative (asserted: 1e-9).  The spectral
scores of a real round trip compare two complex128 FFT implementations of the same input
(relative 1e-6) above the 1e-13 floor the reference's own dB() adds."""
import functools
from ctypes import POINTER, c_double, c_int32, c_void_p

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_MAX = 1e-12
REL_SUM = 1e-9
SIZES = (40, 5003, 70001)


def _torch():
    import torch
    return torch


def _close(got, ref, rel, what=""):
    assert abs(got - ref) <= rel * abs(ref), f"{what}: {got!r} vs {ref!r} (relative {rel})"


@functools.lru_cache(maxsize=None)
def _noise(n_vec, n, seed=5):
    """Complex Gaussian noise of rms 1e-4, float32 (read-only: shared among the tests)."""
    rng = np.random.default_rng(seed)
    z = (1e-4 / np.sqrt(2)) * (rng.standard_normal((n_vec, n)) + 1j * rng.standard_normal((n_vec, n)))
    z = z.astype(np.complex64)
    z.setflags(write=False)
    return z


def _strided(host, pad, offset, dtype=None):
    """``host`` (n_vec, n) on the device as rows ``n + pad`` elements apart, the first one
    ``offset`` elements into its buffer -> (view, whole buffer)."""
    torch = _torch()
    n_vec, n = host.shape
    t = torch.from_numpy(np.array(host)).to("cuda:0")
    buf = torch.zeros(offset + n_vec * (n + pad), dtype=dtype or t.dtype, device="cuda:0")
    view = buf[offset:].view(n_vec, n + pad)[:, :n]
    view.copy_(t)
    return view, buf


# ------------------------------------------------------------------ generators
def _generate(kinds, params, n, stride, offset=0, sentinel=complex(7.0, -3.0)):
    """pfb_testvec_generate into a sentinel-filled buffer -> the whole buffer on the host,
    shaped (n_vec, stride) from element ``offset`` on."""
    torch = _torch()
    from ska_pst_dsp_model_amd import _lib
    n_vec = len(kinds)
    buf = torch.full((offset + n_vec * stride,), sentinel, dtype=torch.complex64, device="cuda:0")
    kind = np.asarray(kinds, np.int32)
    param = np.zeros((n_vec, 4), np.float64)
    for i, p in enumerate(params):
        param[i, :len(p)] = p
    _lib.check(_lib.load().pfb_testvec_generate(
        kind.ctypes.data_as(POINTER(c_int32)), param.ctypes.data_as(POINTER(c_double)), n_vec, n,
        c_void_p(buf.data_ptr() + 8 * offset), stride, c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:offset] == np.complex64(sentinel))
    return host[offset:].reshape(n_vec, stride)


@pytest.mark.parametrize("offset", [0, 1])
def test_generator_impulse(gpu, offset):
    """Four impulses in one call, rows n + 5 apart: bit-identical to time_domain_impulse,
    the clip at the end included, and the gaps between the rows untouched."""
    from ska_pst_dsp_model_amd import verify
    n = 5003
    cases = [(1, 1), (n, 1), (n - 1, 3), (n + 7, 1)]
    got = _generate([0] * 4, cases, n, n + 5, offset)
    for row, (off, width) in zip(got, cases):
        ref = verify.time_domain_impulse(n, off, width)
        assert ref.shape == (n,)
        assert np.array_equal(row[:n].view(np.uint32), ref.view(np.uint32)), (off, width)
        assert np.all(row[n:] == np.complex64(complex(7.0, -3.0))), (off, width)
    assert got[2][:n].real.sum() == 2.0 and got[3][:n].real.sum() == 0.0


def _check_tone(row, ref):
    # both are float32 roundings (<= 2^-25 below 1, 2^-24 at 1) of doubles whose phases differ by < 1e-8 rad
    err = max(np.abs(row.real.astype(np.float64) - ref.real).max(), np.abs(row.imag.astype(np.float64) - ref.imag).max())
    mod = np.abs(row.real.astype(np.float64) ** 2 + row.imag.astype(np.float64) ** 2 - 1.0).max()
    print(f"tone: max component error {err:.3e} (bound {2.0 ** -23:.3e}), max | |x|^2 - 1 | {mod:.3e}")
    assert err <= 2.0 ** -23
    assert mod <= 3 * 2.0 ** -23


def test_generator_sinusoid_small(gpu):
    from ska_pst_dsp_model_amd import verify
    n = 5003
    got = _generate([1, 1], [(3, np.pi / 4, 0.0), (n - 3, np.pi / 4, 0.0)], n, n + 5)
    for row, f in zip(got, (3, n - 3)):
        _check_tone(row[:n], verify.complex_sinusoid(n, f))
        assert np.all(row[n:] == np.complex64(complex(7.0, -3.0)))


def test_generator_sinusoid_largest_phase(gpu):
    """The largest tone of the 'mid' sweep: phases up to 3.4e7 rad, where only a double
    argument reduction keeps the float32 result."""
    from ska_pst_dsp_model_amd import verify
    n, f = 5505024, 5486952
    got = _generate([1], [(f, np.pi / 4, 0.0)], n, n)
    _check_tone(got[0], verify.complex_sinusoid(n, f))


# ------------------------------------------------------------------ spurious score
def _peaks(n):
    return [0, 17, n // 2, n - 1]


def _impulse_noise(n_vec, n, first=0):
    """Noise plus one sample of amplitude 1 per vector, at _peaks(n)[(first + v) % 4]."""
    a = _noise(n_vec, n).copy()
    pk = [_peaks(n)[(first + v) % 4] for v in range(n_vec)]
    for v, k in enumerate(pk):
        a[v, k] = 1.0
    return a, pk


def _expected_cases(n, peak, v):
    return [-1, 0, n - 1, peak, (peak + 5) % n][v % 5]


def _ref_spurious(p, domain, e):
    """The six results from the power series ``p`` with verify.py's functions."""
    from ska_pst_dsp_model_amd import verify
    k = int(np.argmax(p))
    out = [k, float(p[k]), verify.max_spurious_power(p, domain), verify.total_spurious_power(p, domain), -1.0, -1.0]
    if e is not None and 0 <= e < len(p):
        m = np.ones(len(p), bool)
        m[max(e - 1, 0):e + 2] = False
        out[4], out[5] = float(p[e]), float(p[m].max())
    return out


def _assert_spurious(got, ref, what):
    assert int(got[0]) == ref[0] and got[0] == int(got[0]), (what, got, ref)
    for j, rel in ((1, REL_MAX), (2, REL_MAX), (3, REL_SUM), (4, REL_MAX), (5, REL_MAX)):
        _close(got[j], ref[j], rel, f"{what} [{j}]")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("n_vec", [1, 3, 16])
@pytest.mark.parametrize("domain", [0, 30])
@pytest.mark.parametrize("n", SIZES)
def test_spurious_score(gpu, n, domain, n_vec, dtype):
    torch = _torch()
    from ska_pst_dsp_model_amd import verify
    firsts = range(4) if n_vec == 1 else [0]  # a single vector takes every peak position in turn
    for first in firsts:
        a, pk = _impulse_noise(n_vec, n, first)
        if dtype == 0:
            dev, _ = _strided(a, 3, first & 1)
            scale = 1.0
            power = [np.abs(r.astype(np.complex128)) ** 2 for r in a]
        else:
            spec = np.fft.fft(a.astype(np.complex128), axis=1)
            dev, _ = _strided(spec, 3, first & 1, torch.complex128)
            scale = 1.0 / (float(n) * float(n))
            power = [np.abs(r / n) ** 2 for r in spec]
            pk = [int(np.argmax(p)) for p in power]
        for use_expected in (True, False):
            exp = [_expected_cases(n, pk[v], v + first) for v in range(n_vec)] if use_expected else None
            got = verify._score_spurious(dev, n, scale, domain, exp)
            for v in range(n_vec):
                ref = _ref_spurious(power[v], domain, exp[v] if exp else None)
                _assert_spurious(got[v], ref, f"n {n} domain {domain} vec {v}/{n_vec} dtype {dtype} exp {exp}")
            if dtype == 0:  # the functions the sweep's host path calls, on the series itself
                for v in range(n_vec):
                    mx, tot = verify.temporal_performance(a[v], domain)
                    _close(got[v][2], mx, REL_MAX)
                    _close(got[v][3], tot, REL_SUM)


def test_spurious_window_covers_everything(gpu):
    """n = 40, domain 30, the peak in the middle: every index is zeroed, max = sum = 0."""
    from ska_pst_dsp_model_amd import verify
    a, _ = _impulse_noise(1, 40, 2)
    dev, _ = _strided(a, 3, 1)
    got = verify._score_spurious(dev, 40, 1.0, 30, [20])[0]
    assert (got[0], got[2], got[3]) == (20.0, 0.0, 0.0)
    assert got[1] == 1.0 and got[4] == 1.0 and got[5] > 0


def test_spurious_cf64_series_off_the_16_byte_boundary(gpu):
    """A complex128 series that starts 8 bytes into its buffer (no torch complex tensor does):
    the kernel reads it with 8-byte loads and returns the aligned copy's bits."""
    torch = _torch()
    from ctypes import c_int64
    from ska_pst_dsp_model_amd import _lib, verify
    n = 5003
    a, pk = _impulse_noise(3, n)
    spec = np.fft.fft(a.astype(np.complex128), axis=1)
    flat = torch.zeros(1 + 2 * 3 * (n + 3), dtype=torch.float64, device="cuda:0")
    flat[1:].view(3, 2 * (n + 3))[:, :2 * n].copy_(torch.from_numpy(spec.view(np.float64)).to("cuda:0"))
    aligned, _ = _strided(spec, 3, 0, torch.complex128)
    ref = verify._score_spurious(aligned, n, 1.0 / n ** 2, 30, pk)
    got = np.zeros((3, 6))
    exp = np.asarray(pk, np.int64)
    _lib.check(_lib.load().pfb_purity_score_spurious(
        c_void_p(flat.data_ptr() + 8), 1, n + 3, n, 3, 1.0 / n ** 2, 30, exp.ctypes.data_as(POINTER(c_int64)),
        got.ctypes.data_as(POINTER(c_double)), c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert got.tobytes() == ref.tobytes()


def test_spurious_tie_takes_the_first(gpu):
    from ska_pst_dsp_model_amd import verify
    a = _noise(1, 5003).copy()
    a[0, 100] = a[0, 4000] = np.complex64(0.6 + 0.8j)
    assert a[0, 100].tobytes() == a[0, 4000].tobytes()
    dev, _ = _strided(a, 3, 0)
    got = verify._score_spurious(dev, 5003, 1.0, 0)[0]
    assert got[0] == 100.0 == float(np.argmax(np.abs(a[0].astype(np.complex128)) ** 2))
    _close(got[2], float(np.abs(a[0, 4000].astype(np.complex128)) ** 2), REL_MAX)  # the second one stays


@pytest.mark.parametrize("dtype", [0, 1])
def test_scores_are_deterministic(gpu, dtype):
    torch = _torch()
    from ska_pst_dsp_model_amd import verify
    a, pk = _impulse_noise(3, 70001)
    host = a if dtype == 0 else np.fft.fft(a.astype(np.complex128), axis=1)
    dev, _ = _strided(host, 3, 1, torch.complex128 if dtype else None)
    r1 = verify._score_spurious(dev, 70001, 1.0, 30, pk)
    r2 = verify._score_spurious(dev, 70001, 1.0, 30, pk)
    assert r1.tobytes() == r2.tobytes()
    if dtype == 0:
        b, _ = _strided(_noise(3, 70001, 9), 3, 0)
        d1 = verify._score_difference(dev, b, 70001)
        d2 = verify._score_difference(dev, b, 70001)
        assert d1.tobytes() == d2.tobytes()


# ------------------------------------------------------------------ difference score
@pytest.mark.parametrize("n_vec", [1, 3, 16])
@pytest.mark.parametrize("n", SIZES)
def test_difference_score(gpu, n, n_vec):
    from ska_pst_dsp_model_amd import verify
    a, _ = _impulse_noise(n_vec, n)
    b = (a + _noise(n_vec, n, 11)).astype(np.complex64)
    same = n_vec // 2
    b[same] = a[same]
    for off_a, off_b in ((0, 0), (1, 0), (1, 1)):  # rows meeting and missing each other's 16-byte boundary
        da, _ = _strided(a, 3, off_a)
        db, _ = _strided(b, 3, off_b)
        got = verify._score_difference(da, db, n)
        for v in range(n_vec):
            ref = verify.temporal_difference(a[v], b[v])
            _close(got[v][0], ref[0], REL_MAX, f"max n {n} vec {v}")
            _close(got[v][1], ref[1], REL_SUM, f"sum n {n} vec {v}")
        assert tuple(got[same]) == (0.0, 0.0)


# ------------------------------------------------------------------ a real round trip
BANKS = [
    # channels, Nf, Ov, blocks, vectors, nbins, fft_length, output_nbins
    (16, 128, 16, 3, 18, 5376, 3584, 4032),   # the spectrum truncates the chopped series
    # The spectrum zero-pads it.  (8 channels with Nf 64, Ov 8 would give 1344 / 896 / 672, but
    # the synthesis has no Nf = 64 kernel and refuses the plan; Nf 128, the smallest it has, with
    # the same Ov / Nf and two input blocks leaves one synthesis block of 672 samples for a
    # 1792-point spectrum.)
    (8, 128, 16, 2, 10, 1792, 1792, 672),
]
INT_FIELDS = ("param", "n_chopped", "expected_index", "peak_index")
MAX_FIELDS = ("max_spurious_power", "peak_amplitude", "max_diff_power")
SUM_FIELDS = ("total_spurious_power", "total_diff_power", "mean_diff_power")
DB_OF = {"max_spurious_dB": "max_spurious_power", "total_spurious_dB": "total_spurious_power",
         "max_diff_dB": "max_diff_power"}


@pytest.mark.parametrize("channels, nf, ov, blocks, n_items, nbins, fft_length, output_nbins", BANKS)
def test_scoring_a_real_round_trip(gpu, channels, nf, ov, blocks, n_items, nbins, fft_length, output_nbins):
    import ska_pst_dsp_model_amd as pfb
    from ska_pst_dsp_model_amd import verify
    taps = pfb.design_PFB_FIR_filter(channels, "8/7", 10)
    al = verify.performance_alignment(channels, "8/7", nf, ov, len(taps), blocks, 0, 0)
    assert (al["nbins"], al["fft_length"], al["output_nbins"]) == (nbins, fft_length, output_nbins)
    items = verify.sweep_vectors(al, 4, blocks)
    assert len(items) == n_items
    x = verify.device_vectors(items, nbins)
    assert tuple(x.shape) == (n_items, nbins) and x.is_cuda
    ana = pfb.AnalysisPlan(taps, channels, "8/7", "polyphase_analysis_padded", n_items, 0)
    win = pfb.PFBWindow().lookup["tukey"](nf, ov)
    syn = pfb.SynthesisPlan(channels, "8/7", nf, ov, True, 1, True, taps, win, None, n_items, 0)
    _, y = pfb.roundtrip(ana, syn, x)
    got = verify.score_vectors_device(items, x, y, al)
    assert (got[0]["n_chopped"] < fft_length) == (blocks == 2)  # truncated, or zero-padded
    xh, yh = x.cpu().numpy(), y.cpu().numpy()
    assert len(got) == n_items
    n_expected = 0
    for (domain, param), g, xin, yy in zip(items, got, xh, yh):
        ref = verify.score_vector(domain, param, xin, yy, al)
        assert list(g) == list(ref), (g, ref)   # the same keys in the same order
        assert g["domain"] == ref["domain"] == domain
        n_expected += "expected_index" in ref
        for k in ref:
            what = f"{domain} {param} {k}: {g[k]!r} vs {ref[k]!r}"
            if k in INT_FIELDS:
                assert g[k] == ref[k] and isinstance(g[k], int), what
            elif domain == "freq" and k in ("max_spurious_power", "total_spurious_power"):
                assert abs(g[k] - ref[k]) <= 1e-6 * abs(ref[k]) + 1e-13, what
            elif k in MAX_FIELDS:
                _close(g[k], ref[k], REL_MAX, what)
            elif k in SUM_FIELDS:
                _close(g[k], ref[k], REL_SUM, what)
            elif k == "max_outside_pm1_dB":  # the tolerance applies to the power
                _close(10.0 ** (g[k] / 10.0), 10.0 ** (ref[k] / 10.0), REL_MAX, what)
            elif k in DB_OF:  # formed on the host from the returned power with the existing dB
                assert g[k] == float(verify.dB(g[DB_OF[k]])), what
            else:
                assert k == "domain", k
    assert 0 < n_expected < sum(d == "time" for d, _ in items)  # impulses inside and outside the output


# ------------------------------------------------------------------ the sweep itself
def test_purity_sweep_on_the_device(gpu):
    """verify.purity_sweep(scoring="device") at the 'mid' defaults, asserted as
    test_purity_sweep_ska_mid asserts the host path."""
    from ska_pst_dsp_model_amd import verify
    recs = verify.purity_sweep(npoints=4, batch=8, scoring="device")
    al = verify.performance_alignment(4096, "8/7", 512, 128, 100353, 3, 0, 0)
    items = verify.sweep_vectors(al, 4, 3) + [("comb", 32), ("square_wave", 3981)]
    assert [(r["domain"], r["param"]) for r in recs] == [(d, int(p)) for d, p in items]
    assert all(r["rank"] == 0 for r in recs)
    imp = [r for r in recs if r["domain"] == "time" and "expected_index" in r]
    ton = [r for r in recs if r["domain"] == "freq"]
    assert len(imp) >= 6 and len(ton) == 4
    for r in imp:
        assert r["peak_index"] == r["expected_index"], r
        assert abs(r["peak_amplitude"] - 1.0) < 1e-3, r
        assert r["max_outside_pm1_dB"] <= -60.0, r
    for r in ton:
        assert r["max_spurious_dB"] <= -60.0, r
        assert r["max_diff_dB"] <= -50.0, r
    comb = [r for r in recs if r["domain"] == "comb"]
    sq = [r for r in recs if r["domain"] == "square_wave"]
    assert len(comb) == 1 and len(sq) == 1
    assert set(comb[0]) == {"domain", "param", "n_chopped", "power_ratio", "comb_test", "rank"}
    assert set(sq[0]) == {"domain", "param", "n_chopped", "power_ratio", "on_power", "off_power", "rank"}
    assert comb[0]["comb_test"] == 0, comb
    assert 0.9 < sq[0]["on_power"] < 1.1 and sq[0]["off_power"] < 1e-3, sq
