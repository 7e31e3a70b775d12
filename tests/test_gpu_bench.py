"""GPU test of ``bench.py --dump-outputs``: the files hold what the last timed step computed.

One plain run of the benchmark (a child process, small units) with K = 5 steps over the
default 3 plan pairs: step 4 runs on pair 1, whose unit is drawn from seed 100 + 7919.  The
dumped channelised product and synthesised series must equal, bit for bit, the same two
calls (``roundtrip_analysis`` + ``roundtrip_synthesis``, the halves the captured pipeline is
made of) on that unit in this process, as float32 (re, im) pairs.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_dump_outputs_are_the_last_timed_steps_outputs(gpu, tmp_path):
    import torch
    import ska_pst_dsp_model_amd as pfb
    n_dat, steps = 1 << 19, 5
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps",
                        str(steps), "--warmup", "1", "--n-dat", str(n_dat), "--dump-outputs",
                        str(tmp_path)], env=env, capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert line["full"] is False and line["steps"] == steps and line["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["chan.npy", "out.npy"]

    seed = bench.pair_seeds(bench.rank_units("c2", 0), 3, True)[(steps - 1) % 3]
    assert seed == 100 + 7919
    g = torch.Generator(device=gpu).manual_seed(seed)
    x = torch.stack([torch.complex(torch.randn((n_dat,), device=gpu, generator=g),
                                   torch.randn((n_dat,), device=gpu, generator=g)) / np.sqrt(2.0)])
    x = x.to(torch.complex64).contiguous()
    taps = pfb.design_PFB_FIR_filter(bench.N_CHAN, bench.OS_STR, bench.TAPS_PER_CHAN)
    win = pfb.PFBWindow().lookup["tukey"](bench.NF, bench.OV)
    ana = pfb.AnalysisPlan(taps, bench.N_CHAN, bench.OS_STR, "polyphase_analysis", 1, 0)
    syn = pfb.SynthesisPlan(bench.N_CHAN, bench.OS_STR, bench.NF, bench.OV, True, 1, True, taps,
                            win, None, 1, 0)
    K = ana.output_length(n_dat)
    chan = torch.empty((1, K, bench.N_CHAN), dtype=torch.complex64, device=gpu)
    out = torch.empty((1, syn.output_length(K)), dtype=torch.complex64, device=gpu)
    pfb.roundtrip_analysis(ana, syn, x, chan=chan)
    pfb.roundtrip_synthesis(ana, syn, n_dat, out=out)
    torch.cuda.synchronize()
    for name, t in (("chan", chan), ("out", out)):
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        flat = t.reshape(1, -1)
        # both arrays are shorter than the sample size at this n_dat: dumped whole
        pos = bench.dump_positions(flat.shape[1], bench.DUMP_BYTES // (8 * 2))
        assert len(pos) == flat.shape[1]
        want = torch.view_as_real(flat).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape == (1, flat.shape[1], 2)
        assert np.abs(want).max() > 0
        assert np.array_equal(got, want), name
    ana.close()
    syn.close()
