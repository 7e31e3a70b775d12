"""The stream contract of include/pfb_api.h ("Streams") for the 4096-channel to-DADA call, whose
FIR and section-storing row FFT (row_fft4096_pair_dadaout_kernel) are two launches: both must go
to the caller's stream.  The stateless call runs on a side stream behind the delay kernel
(tests/stream_harness.py) and must equal the default-stream call bit for bit; then it is captured
into a graph after one call of that length and replayed on other samples."""
import numpy as np
import pytest

import stream_harness as sh

pytestmark = pytest.mark.gpu

N, OS = 4096, "8/7"
N_DAT = 13 * 4096 + 9 * 3584 + 100   # 23 rows, an odd count


def _plan(n_pol):
    import ska_pst_dsp_model_amd as pfb
    taps = np.random.default_rng(41).standard_normal(4096 * 12 + 1) / 64.0
    return pfb.AnalysisPlan(taps, N, OS, "polyphase_analysis_padded", n_pol)


def _noise(gpu, shape, seed):
    import torch
    rng = np.random.default_rng(seed)
    x = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)).astype(np.complex64)
    return torch.from_numpy(x).to(gpu)


def test_mid_execute_to_dada_on_a_side_stream_and_from_a_graph(gpu):
    import torch
    n_pol, nbit = 2, 16
    inputs = [_noise(gpu, (n_pol, N_DAT), 12000 + k) for k in range(3)]
    y = _plan(n_pol).execute(inputs[0])
    scale = float(3000.0 / torch.view_as_real(y).float().pow(2).mean().sqrt().item())

    def check(p):
        assert p.last_dada_output() == "fused" and p.last_dada_input() == "none"

    ref, _ = sh.poison_delay("AnalysisPlan.execute_to_dada, 4096 channels", lambda: _plan(n_pol),
                             lambda p, xs, outs: [p.execute_to_dada(xs[0], nbit, scale=scale)], [inputs[0]],
                             check=check)
    assert tuple(ref[0].shape) == (23, N, n_pol, 2) and str(ref[0].dtype) == "torch.int16"
    assert float(ref[0].float().abs().mean()) > 100
    # graph capture after one call of that length (the plan's scratch exists: no allocation)
    plan = _plan(n_pol)
    call = lambda x: plan.execute_to_dada(x, nbit, scale=scale)  # noqa: E731
    eager = [call(x).clone() for x in inputs]
    assert sh.same_bits(eager[0], ref[0])
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
        assert sh.same_bits(out, eager[k]), f"replay {k}"
    del g
    plan.close()
