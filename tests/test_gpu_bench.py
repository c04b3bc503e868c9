"""bench.py on the MI355X, N = 1: a plain run prints the line of the timed steps and nothing more; --full adds the legs
that describe or check them (here the CPU baseline, which checks the GPU result against the oracle bit for bit)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent


def _bench_line(*extra):
    proc = subprocess.run([sys.executable, str(REPO / "bench.py"), "--workload", "c2", "--steps", "2", "--warmup", "1", *extra],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, proc.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_is_the_timed_steps_and_full_adds_the_checks():
    rec = _bench_line()
    assert rec["n_gpus"] == 1 and rec["steps"] == 2 and rec["warmup"] == 1 and rec["unit"] == "GFLOP/s"
    assert rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["roofline"]["kernel_ms_per_step"] > 0
    assert "cpu_baseline" not in rec and rec["roofline"]["traffic_live_detail"] is None
    assert not str(rec["roofline"]["traffic_source"] or "").startswith("live")
    # (--no-live-pmc: the rocprofv3 passes are left to the committed record here; they are exercised by
    # tests/test_bench_contract.py on recorded counter files)
    full = _bench_line("--full", "--no-live-pmc")
    assert full["config"]["sha256_rowptr_col_val"] == rec["config"]["sha256_rowptr_col_val"]
    assert full["cpu_baseline"]["gpu_matches_oracle_on_sample"] == "bit-exact"
    assert full["cpu_baseline"]["allclose_vs_torch_cpu_rtol1e-5_atol1e-8"] is True
