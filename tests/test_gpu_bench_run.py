"""GPU: a plain bench.py run (no --full) at a small size. The line carries the contract keys and
none of what --full adds, --steps sets the timed steps, and --dump-outputs holds the records of the
last timed step's batch, bit-exact against the C oracle."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dump(tmp_path, oracle_lib):
    import torch

    import bench
    from halo_amd import _lib
    from halo_amd._lib import NetIf

    n, rotate, steps, warmup = 3000, 3, 5, 2
    dump = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--frames", str(n), "--rotate", str(rotate),
                        "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert line["unit"] == "Mpps" and line["higher_is_better"] is True and line["dtype"] == "u8"
    # value and ms_per_step come from the same wall time; ms_per_step is rounded to 4 decimals
    assert line["value"] == pytest.approx(n / line["ms_per_step"] / 1e3, rel=0.00005 / line["ms_per_step"] + 1e-3)
    assert line["full"] is False and line["cpu_baseline"] is None
    for k in ("secondary", "validated", "config4_128M_one_gpu"):
        assert k not in line, k
    assert "peak_measured_read" not in line["roofline"] and "size_matched_probe_ms" not in line["roofline"]
    assert os.listdir(tmp_path) == ["dump"]  # no detail file, nothing else beside the dump

    rec = np.load(dump / "records.npy")
    rows = np.load(dump / "record_rows.npy")
    assert rec.dtype == np.float32 and rec.shape == (n, 32)
    assert rows.dtype == np.float64 and np.array_equal(rows, np.arange(n))
    # the last timed step parsed batch (steps - 1) % rotate of rank 0's shard
    assert torch.cuda.is_available(), "GPU tests need a device"
    _lib.check("halo_rx_init", _lib.lib.halo_rx_init(0))
    batches, _ = bench.shard_batches(torch.device("cuda:0"), NetIf.make(), rank=0, n=n, rotate=rotate)
    b = batches[(steps - 1) % rotate]
    want, _ = oracle_lib.rx_batch(b["bytes"].cpu().numpy(), b["layout"]["lens"], oracle_lib.NetIf.make(), 1,
                                  offsets_dw=b["layout"]["offsets_dw"])
    assert np.array_equal(rec, want.view(np.uint8).reshape(n, 32).astype(np.float32))
