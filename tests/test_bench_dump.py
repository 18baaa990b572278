"""bench.py --dump-outputs: what the last timed step computed, written as .npy so that two builds can be compared output for output."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_writes_float32_or_float64_and_keeps_to_the_limit(tmp_path):
    bench = load_bench()
    bench.dump_outputs(str(tmp_path / "d"), {"a": torch.arange(6, dtype=torch.bfloat16).reshape(2, 3), "m": torch.tensor([True, False]),
                                             "l": torch.tensor([0.1], dtype=torch.float64)})
    a, m, l = (np.load(tmp_path / "d" / (k + ".npy")) for k in ("a", "m", "l"))
    assert a.dtype == np.float32 and a.shape == (2, 3) and np.array_equal(a, np.arange(6).reshape(2, 3))
    assert m.dtype == np.float32 and np.array_equal(m, [1.0, 0.0])
    assert l.dtype == np.float64 and l[0] == 0.1
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": torch.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1)})
    assert not (tmp_path / "big").exists()


def test_bench_rejects_zero_steps():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--selftest-cpu"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "--steps must be at least 1" in out.stderr


@pytest.mark.gpu
def test_dumped_forward_is_the_forward_of_the_seeded_inputs(tmp_path):
    """A short graph-replay bench run at a small shape dumps its last step; an eager forward of the same seeded weights and inputs in this process
    must give the same encoder output and mask."""
    import cfm
    B, T, steps = 2, 200, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "1", "--batch", str(B), "--frames", str(T),
           "--train-steps", "0", "--no-cpu-baseline", "--no-live-traffic", "--no-fp16", "--no-parity", "--ramp-ms", "0",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path)) == ["encoder_mask.npy", "encoder_out.npy"]

    bench = load_bench()
    prev = cfm.get_precision()
    cfm.set_precision("bf16")
    try:
        enc = bench.build_encoder("cuda:0")
        x, lens = bench.forward_inputs(B, T, 0, torch.device("cuda:0"))
        with torch.no_grad():
            y, m = enc(x, lens)
        torch.cuda.synchronize()
    finally:
        cfm.set_precision(prev)
    y_dump, m_dump = np.load(tmp_path / "encoder_out.npy"), np.load(tmp_path / "encoder_mask.npy")
    assert y_dump.dtype == np.float32 and y_dump.shape == tuple(y.shape)
    assert np.array_equal(m_dump, m.float().cpu().numpy())
    y = y.double().cpu().numpy()
    assert float(np.abs(y_dump - y).max() / np.abs(y).max()) < 1e-6
