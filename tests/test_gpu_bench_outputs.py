"""A plain `bench.py --gpus 1` run: one JSON line about the NTT alone, with the number of timed steps it was given; --dump-outputs writes the
same numbers in two runs with the same arguments (whatever the warm-up did), and at --steps 1 they are the CPU oracle's NTT of the seeded input."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def run_bench(out_dir, *argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log-n", "16", "--dump-outputs", str(out_dir), *argv],
                       capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-800:], r.stderr[-800:])
    return json.loads(lines[0]), np.load(os.path.join(out_dir, "ntt_output.npy"))


def test_plain_run_dumps_the_oracle_ntt_of_the_seeded_input(tmp_path, hip_lib, oracle):
    import torch
    from lambdaworks_cairo_prover_amd import api
    line, got = run_bench(tmp_path / "a", "--steps", "1", "--warmup", "2")
    _, again = run_bench(tmp_path / "b", "--steps", "1", "--warmup", "7")
    assert line["steps"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0 and line["config"]["log_n"] == 16
    assert not {"proof", "proof_cfg4", "cpu_baseline", "roofline_merkle"} & set(line) and line["summary"] == {}
    n = 1 << 16
    assert got.dtype == np.float64 and got.shape == (n, 8) and np.array_equal(got, again)
    dev_in = bench.ntt_input(torch, n, 0).numpy().view(np.uint8).reshape(n, 32)
    dev_out = got.astype(np.uint32).view(np.uint8).reshape(n, 32)
    assert np.array_equal(api.fe_from_device(dev_out), oracle.ntt(api.fe_from_device(dev_in)))
