"""The 4096-channel (SKA-Mid) analysis writing its product straight into a DADA data section:
on these plans the FIR fills the plan's scratch rows and the row FFT
(row_fft4096_pair_dadaout_kernel) converts and stores the NBIT 8 / 16 / 32 samples itself, so
no complex float32 product crosses HBM and no pack launch follows.

The contract is tests/test_gpu_dada_output.py's: bit-identity with the pair (the cf32-output
call, both components times float32(scale), pfb_dada_pack), np.array_equal on bytes, under a
scale at which the pair's own output saturates, rounds both ways and meets an exact .5 tie, in
a framed buffer whose pattern must survive.

Shape: N = 4096, os 8/7 (M = 3584), 4096 * 12 + 1 random taps (13 phases), and the input of
test_analysis_4096_odd_row_count: K = 9 rows (Bunton) and 23 (padded), both odd, so the last
row pair has no row B; the padded shift sds = 7 is odd, so its wrap falls inside a pair of
consecutive output rows; a stream call on a fresh plan returns T_out = 8 / 16 < K, so there are
nu-trimmed rows that must not appear.
"""
import numpy as np
import pytest

import test_gpu_dada_output as base
from test_gpu_dada_output import profiling  # noqa: F401  (the fixture)
from conftest import PARITY_TOL, assert_pfb_close
from oracle import pfb_oracle as orc

pytestmark = pytest.mark.gpu

N, OS, M = 4096, "8/7", 3584
BUNTON, PADDED = "polyphase_analysis", "polyphase_analysis_padded"
VARIANTS = [BUNTON, PADDED]
N_DAT = 13 * 4096 + 9 * 3584 + 100
K_OF = {BUNTON: 9, PADDED: 23}
T_OUT_OF = {BUNTON: 8, PADDED: 16}
PAT = base.PAT

_CACHE = {}


def _taps():
    if "taps" not in _CACHE:
        t = np.random.default_rng(41).standard_normal(4096 * 12 + 1) / 64.0
        t.setflags(write=False)
        _CACHE["taps"] = t
    return _CACHE["taps"]


def _plan(variant, n_pol):
    return base._pfb().AnalysisPlan(_taps(), N, OS, variant, n_pol)


def _vid(v):
    return "bunton" if v == BUNTON else "padded"


def _kernel_names():
    return [base._kernel_name(w) for w in range(6)]


def _one_row(variant):
    """Samples of a stateless call with exactly one output row."""
    return 13 * N + M + 5 if variant == BUNTON else M + 5


# ------------------------------------------------------------------ 1. fused == the pair
@pytest.mark.parametrize("n_pol", [1, 2, 3], ids=["1pol", "2pol", "3pol"])
@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["nbit8", "nbit16", "nbit32"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_fused_matches_the_pair(gpu, profiling, variant, nbit, n_pol):  # noqa: F811
    """On the parent commit this fails: it reports "staged" and launches the pack kernel."""
    rows = K_OF[variant]
    _, rawd = base._section(gpu, 4100 + 16 * n_pol + nbit + len(variant), 16, N_DAT, n_pol)
    x = base._unpacked(rawd, 16, n_pol)
    ref = _plan(variant, n_pol).execute(x)
    assert tuple(ref.shape) == (n_pol, rows, N)
    refh = ref.cpu().numpy()
    scale = base._tie_scale(refh, nbit)
    pair = base._pack_pair(ref, nbit, scale)
    rb = N * n_pol * 2 * (nbit // 8)
    assert pair.size == rows * rb
    base._assert_pair_is_demanding(refh, pair, nbit, scale)
    twin_in = _plan(variant, n_pol)
    assert np.array_equal(twin_in.execute_dada(rawd, 16).cpu().numpy(), refh)
    dada_in_path = twin_in.last_dada_input()
    assert dada_in_path in ("fused", "staged")
    for label, kw in (("cf32", dict(x=x)), ("dada", dict(rawd=rawd, in_nbit=16))):
        plan = _plan(variant, n_pol)
        assert profiling.pfb_profile_reset() == 0
        st, n_out, h, off, _ = base._call(plan, gpu, nbit, scale, **kw)
        assert (st, n_out) == (0, rows), (label, st, n_out)
        assert np.array_equal(base._written(h, off, rows * rb, f"{_vid(variant)} {label}"), pair), label
        assert plan.last_dada_output() == "fused", label
        assert plan.last_dada_input() == (dada_in_path if label == "dada" else "none")
        names = _kernel_names()
        print(f"{_vid(variant)} {label} nbit {nbit} {n_pol} pol: {names}")
        assert any("row_fft4096_pair_dadaout_kernel<" in k and f"OutDada{nbit}" in k for k in names), names
        assert not any("dada_pack" in k for k in names), names
        # the stream call from a fresh plan: T_out < K, the nu-trimmed rows must not appear
        plan, twin = _plan(variant, n_pol), _plan(variant, n_pol)
        ref_s = twin.execute(x, stateful=True)
        t_out = int(ref_s.shape[1])
        assert 0 < t_out < rows and t_out == T_OUT_OF[variant]
        st, n_out, h, off, _ = base._call(plan, gpu, nbit, scale, stateful=True, **kw)
        assert (st, n_out) == (0, t_out), (label, st, n_out)
        assert np.array_equal(base._written(h, off, t_out * rb, f"{_vid(variant)} {label} stream"),
                              base._pack_pair(ref_s, nbit, scale)), label
        assert plan.last_dada_output() == "fused"
        assert plan.buffered_samples == twin.buffered_samples > 0


# ------------------------------------------------------------------ 2. edge row counts
@pytest.mark.parametrize("n_pol", [1, 2], ids=["1pol", "2pol"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_one_row_and_no_row(gpu, variant, n_pol):
    nbit = 16
    n = _one_row(variant)
    _, rawd = base._section(gpu, 4200 + n_pol, 16, n, n_pol)
    x = base._unpacked(rawd, 16, n_pol)
    plan = _plan(variant, n_pol)
    ref = plan.execute(x)
    assert ref.shape[1] == 1
    if variant == BUNTON:
        scale = base._tie_scale(ref.cpu().numpy(), nbit)
    else:
        # (the padded variant's only row lies wholly in its leading zero padding: the row must
        # still be written, as zeros over the frame's pattern)
        assert float(ref.abs().max()) == 0
        scale = 0.37
    pair = base._pack_pair(ref, nbit, scale)
    for kw in (dict(x=x), dict(rawd=rawd, in_nbit=16)):
        st, n_out, h, off, _ = base._call(plan, gpu, nbit, scale, **kw)
        assert (st, n_out) == (0, 1)
        assert plan.last_dada_output() == "fused"
        assert np.array_equal(base._written(h, off, pair.size, "one row"), pair)
    # an input shorter than the taps (Bunton) / than one step (padded): OK, 0 rows, nothing written
    short = 13 * N - 1 if variant == BUNTON else M - 1
    for kw in (dict(x=x[:, :short].contiguous()), dict(rawd=rawd[:short * n_pol * 4].contiguous(), in_nbit=16)):
        plan = _plan(variant, n_pol)
        st, n_out, h, off, _ = base._call(plan, gpu, nbit, 0.37, **kw)
        assert (st, n_out) == (0, 0)
        assert base._written(h, off, 0, "short").size == 0
        assert plan.last_dada_output() == "fused"


# ------------------------------------------------------------------ 3. stream sequence
SIZES = (3000, 131072, 50000, 7777)
# (section in, cf32 out), (cf32 in, section out), (section in, section out), (cf32 in, cf32 out):
# the inputs alternate, both calls that return rows write a section, one from each input kind
MODES = ("dada_in", "to_dada", "dada_to_dada", "cf32")


def test_stream_sequence(gpu):
    nbit, n_pol, scale = 16, 2, 0.0123
    plan, twin = _plan(PADDED, n_pol), _plan(PADDED, n_pol)
    rb = N * n_pol * 2 * (nbit // 8)
    rows_seen = []
    for i, (n, mode) in enumerate(zip(SIZES, MODES)):
        _, rawd = base._section(gpu, 4300 + i, nbit, n, n_pol)
        x = base._unpacked(rawd, nbit, n_pol)
        buffered_before = plan.buffered_samples
        ref = twin.execute(x, stateful=True)
        t_out = int(ref.shape[1])
        rows_seen.append(t_out)
        ref_b = base._pack_pair(ref, nbit, scale)
        assert plan.stream_rows(n) == t_out, i
        if mode == "cf32":
            got_b = base._pack_pair(plan.execute(x, stateful=True), nbit, scale)
            assert plan.last_dada_output() == "none"
        elif mode == "dada_in":
            got_b = base._pack_pair(plan.execute_dada(rawd, nbit, stateful=True), nbit, scale)
            assert plan.last_dada_output() == "none"
        else:
            kw = dict(x=x) if mode == "to_dada" else dict(rawd=rawd, in_nbit=nbit)
            st, n_out, h, off, _ = base._call(plan, gpu, nbit, scale, stateful=True, **kw)
            assert (st, n_out) == (0, t_out), (i, mode, st, n_out)
            got_b = base._written(h, off, t_out * rb, f"call {i}")
            assert plan.last_dada_output() == "fused", (i, mode)
            if mode == "dada_to_dada":
                # samples were buffered: the section is unpacked behind them, the output stays fused
                assert buffered_before > 0 and plan.last_dada_input() == "staged"
        assert np.array_equal(got_b, ref_b), (i, mode)
        assert plan.buffered_samples == twin.buffered_samples, (i, mode)
    assert rows_seen[0] == 0 and rows_seen[1] > 0 and rows_seen[2] > 0, rows_seen


# ------------------------------------------------------------------ 4. what stays staged
@pytest.mark.parametrize("case", [("nbit64", 64, 0), ("out-offset-one-value", 16, 2)], ids=lambda c: c[0])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_staged_remainders(gpu, variant, case):
    name, out_nbit, offset = case
    n_pol, rows = 2, K_OF[variant]
    _, rawd = base._section(gpu, 4400 + len(name), 16, N_DAT, n_pol)
    x = base._unpacked(rawd, 16, n_pol)
    plan, twin = _plan(variant, n_pol), _plan(variant, n_pol)
    ref = twin.execute(x)
    scale = base._tie_scale(ref.cpu().numpy(), out_nbit if out_nbit != 64 else 32)
    pair = base._pack_pair(ref, out_nbit, scale)
    for kw in (dict(x=x), dict(rawd=rawd, in_nbit=16)):
        st, n_out, h, off, _ = base._call(plan, gpu, out_nbit, scale, offset=offset, **kw)
        assert (st, n_out) == (0, rows)
        assert plan.last_dada_output() == "staged"
        assert np.array_equal(base._written(h, off, pair.size, name), pair)
    ref_s = twin.execute(x, stateful=True)
    st, n_out, h, off, _ = base._call(plan, gpu, out_nbit, scale, x=x, stateful=True, offset=offset)
    assert (st, n_out) == (0, int(ref_s.shape[1]))
    assert plan.last_dada_output() == "staged"
    assert np.array_equal(base._written(h, off, n_out * N * n_pol * 2 * (out_nbit // 8), name),
                          base._pack_pair(ref_s, out_nbit, scale))
    assert plan.buffered_samples == twin.buffered_samples
    plan.execute(x)
    assert plan.last_dada_output() == "none"


# ------------------------------------------------------------------ 5. rejections
@pytest.mark.parametrize("stateful", [False, True], ids=["stateless", "stream"])
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_rejections_leave_output_and_state_alone(gpu, variant, stateful):
    from ska_pst_dsp_model_amd import _lib
    nbit, n_pol = 16, 2
    plan, twin = _plan(variant, n_pol), _plan(variant, n_pol)
    if stateful:
        _, r0 = base._section(gpu, 4500, nbit, 6000, n_pol)
        for p in (plan, twin):
            assert p.execute(base._unpacked(r0, nbit, n_pol), stateful=True).shape[1] == 0
        assert plan.buffered_samples == 6000
    buffered = plan.buffered_samples
    _, rawd = base._section(gpu, 4501, nbit, N_DAT, n_pol)
    x = base._unpacked(rawd, nbit, n_pol)
    rows = plan.stream_rows(N_DAT) if stateful else plan.output_length(N_DAT)
    assert rows >= 8
    need = rows * N * n_pol * 2 * (nbit // 8)
    E, S = _lib.PFB_ERR_INVALID_ARG, _lib.PFB_ERR_BUFFER_TOO_SMALL
    for kw in (dict(x=x), dict(rawd=rawd, in_nbit=nbit)):
        st, n_out, h, off, _ = base._call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need - 1, **kw)
        assert (st, n_out) == (S, rows)
        assert (h == PAT).all(), "a call with too small a capacity wrote output"
        for bad in (dict(out_nbit=12), dict(scale=float("nan")), dict(scale=float("inf")), dict(null_out=True)):
            args = dict(out_nbit=nbit, scale=0.01, stateful=stateful, cap_bytes=need)
            args.update(bad)
            args.update(kw)
            st, n_out, h, off, _ = base._call(plan, gpu, args.pop("out_nbit"), args.pop("scale"), **args)
            assert st == E, bad
            assert (h == PAT).all(), bad
        assert plan.buffered_samples == buffered
    ref = twin.execute(x, stateful=stateful)
    assert ref.shape[1] == rows
    st, n_out, h, off, _ = base._call(plan, gpu, nbit, 0.01, stateful=stateful, cap_bytes=need, x=x)
    assert (st, n_out) == (0, rows)
    assert plan.last_dada_output() == "fused"
    assert np.array_equal(base._written(h, off, need), base._pack_pair(ref, nbit, 0.01))
    assert plan.buffered_samples == twin.buffered_samples


# ------------------------------------------------------------------ 6. the input quantiser
def test_input_quantiser_composes(gpu):
    """A STAGED quantising copy, then the plan's ordinary path, which stores the section itself."""
    import torch
    from ska_pst_dsp_model_amd import layout
    nbit, n_pol, rms = 16, 2, 10.0
    _, rawd = base._section(gpu, 4600, 16, N_DAT, n_pol)
    x = base._unpacked(rawd, 16, n_pol)
    plan, twin = _plan(PADDED, n_pol), _plan(PADDED, n_pol)
    plan.set_input_quantiser(rms)
    scale = 0.0123
    st, n_out, h, off, _ = base._call(plan, gpu, nbit, scale, x=x)
    assert (st, n_out) == (0, K_OF[PADDED])
    assert plan.last_input_quantiser() == "staged" and plan.last_dada_output() == "fused"
    s = np.float32(plan.last_input_scale())
    q = layout.quantize(torch.view_as_complex((torch.view_as_real(x.contiguous()) * float(s)).contiguous()), 0.0)
    assert 5.0 < float(torch.view_as_real(q).std()) < 15.0
    st, n_ref, h_ref, off_ref, _ = base._call(twin, gpu, nbit, scale, x=q)
    assert (st, n_ref) == (0, n_out) and twin.last_dada_output() == "fused"
    nbytes = n_out * N * n_pol * 2 * (nbit // 8)
    got = base._written(h, off, nbytes, "quantiser on")
    assert np.array_equal(got, base._written(h_ref, off_ref, nbytes, "quantiser off")) and got.any()


# ------------------------------------------------------------------ 7. oracle
@pytest.fixture(scope="module")
def oracle_case():
    n_pol = 2
    raw = base._file_samples(np.random.default_rng(4700), 16, N_DAT * n_pol * 2)
    x = orc.reshape_dada_data(raw, 2, n_pol, 1)
    y = orc.polyphase_analysis_padded(x, _taps(), N, OS, round_like_matlab=False)
    assert y.dtype == np.complex128 and y.shape == (n_pol, N, K_OF[PADDED])
    y.setflags(write=False)
    raw.setflags(write=False)
    return raw, y


@pytest.mark.parametrize("nbit", [8, 16, 32], ids=["nbit8", "nbit16", "nbit32"])
def test_fused_matches_oracle(gpu, oracle_case, nbit):
    import torch
    raw, y = oracle_case
    n_pol, rows = 2, K_OF[PADDED]
    rawd = torch.from_numpy(raw.view(np.uint8).copy()).to(gpu)
    rms = float(np.sqrt(np.mean(np.abs(y) ** 2)))
    scale = float(np.float32((np.iinfo(orc._NBIT_NP[nbit]).max if nbit != 32 else 1.11) / 3.0 / rms))
    assert np.frexp(scale)[0] != 0.5
    plan = _plan(PADDED, n_pol)
    got = plan.execute_to_dada(base._unpacked(rawd, 16, n_pol), nbit, scale=scale)
    assert plan.last_dada_output() == "fused" and tuple(got.shape) == (rows, N, n_pol, 2)
    sy = np.float64(np.float32(scale)) * y                                     # (n_pol, chan, K)
    expect = orc.write_dada_data(sy, nbit).reshape(rows, N, n_pol, 2)
    q = got.cpu().numpy().astype(np.float64)
    if nbit == 32:
        e = expect.astype(np.float64)
        assert_pfb_close(q[..., 0] + 1j * q[..., 1], e[..., 0] + 1j * e[..., 1], what="to-DADA mid")
        return
    info = np.iinfo(orc._NBIT_NP[nbit])
    t = sy.transpose(2, 1, 0)                                                  # (K, chan, n_pol)
    delta = PARITY_TOL * (np.sqrt(np.mean(np.abs(sy) ** 2)) + np.abs(t))      # assert_pfb_close's allowance
    for comp, part in ((0, t.real), (1, t.imag)):
        err = np.abs(q[..., comp] - np.clip(part, info.min, info.max))
        print(f"nbit {nbit} comp {comp}: max (|q - clip(scale y)| - delta) = {float((err - delta).max()):.6f}")
        assert (err <= 0.5 + delta).all(), (nbit, comp, float((err - delta).max()))


# ------------------------------------------------------------------ 8. Python surface
def test_filterbank_object_execute_to_dada(gpu):
    pfb = base._pfb()
    cfg = dict(analysis_function=PADDED, filt_coeff=_taps(), channels=N, os_factor=OS)
    fb, ref_fb = pfb.FilterBank(cfg), pfb.FilterBank(cfg)
    total = 0
    for i, n in enumerate((N_DAT, 50000)):
        _, rawd = base._section(gpu, 4800 + i, 16, n, 2)
        x = base._unpacked(rawd, 16, 2)
        _, sec = fb.execute_to_dada(x, 16, scale=0.0123)
        _, view = ref_fb.execute(x)
        buf = view.transpose(1, 2).contiguous()
        assert tuple(sec.shape) == (buf.shape[1], N, 2, 2) and str(sec.dtype) == "torch.int16"
        assert np.array_equal(sec.cpu().numpy().view(np.uint8).ravel(), base._pack_pair(buf, 16, 0.0123)), i
        assert fb.buffered_samples == ref_fb.buffered_samples
        assert fb._plan.last_dada_output() == "fused"
        total += buf.shape[1]
    assert total > 16


def test_harness_channelize_writes_the_section_itself(gpu, tmp_path):
    pfb = base._pfb()
    from ska_pst_dsp_model_amd import layout
    taps = _taps()
    fir = tmp_path / "fir.npy"
    pfb.firio.save_fir_filter_coeff(str(fir), taps)
    rng = np.random.default_rng(4900)
    x = 3000.0 * (rng.standard_normal((2, 1, N_DAT)) + 1j * rng.standard_normal((2, 1, N_DAT)))
    src = tmp_path / "series16.dump"
    pfb.dada.write_dada_file(src, x.astype(np.complex64), {"HDR_SIZE": "4096", "TSAMP": "1.0"}, nbit=16)
    f = pfb.harness.channelize(str(src), N, OS, str(fir), output_file_name="chan.dump", output_dir=str(tmp_path),
                               use_padded=True)
    cached = pfb.core.analysis_plan(pfb.read_fir_filter_coeff(str(fir)), N, OS, PADDED, 2)
    assert cached.last_dada_output() == "fused"
    raw, hdr = pfb.dada.read_dada_raw(src)
    # (execute_dada is execute on the unpacked section bit for bit: test_fused_matches_the_pair)
    plan = pfb.AnalysisPlan(pfb.read_fir_filter_coeff(str(fir)), N, OS, PADDED, 2)
    ref = plan.execute_dada(raw, 16)                                            # (n_pol, K, chan)
    assert cached.last_dada_input() == plan.last_dada_input()
    assert tuple(ref.shape) == (2, K_OF[PADDED], N) and float(ref.abs().max()) > 0
    expect = layout.dada_pack(ref, 32).cpu().numpy().view(np.uint8).ravel()
    with open(f.file_path, "rb") as fh:
        got_hdr = pfb.dada.read_header(fh)
        fh.seek(int(got_hdr["HDR_SIZE"]))
        body = np.frombuffer(fh.read(), dtype=np.uint8)
    assert (got_hdr["NBIT"], got_hdr["NCHAN"], got_hdr["NPOL"]) == ("32", str(N), "2")
    assert np.array_equal(body, expect)
