"""A plain bench.py run (no --full) does only what its headline needs: the timed steps, --dump-outputs and the line.  The
roofline replay, the baselines and the auxiliary legs are --full's; the headline keys keep their meaning."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_only(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["unit"] == "denoising-steps/sec" and res["higher_is_better"] is True and res["dtype"] == "f16"
    assert res["n_gpus"] == 1 and res["steps"] == 2 and res["warmup"] == 1
    assert res["value"] > 0 and abs(res["value"] - 1e3 / res["ms_per_step"]) < 0.01 * res["value"]
    assert "configs[1]" in res["config"]["workload"]
    assert res["roofline"] is None and res["cpu_baseline"] is None and res["vs_baseline"] is None
    for k in ("kernel_avg_us", "cfg2b", "cfg2c_large_logits", "torch_gpu_baseline", "cfg3", "f3_gmflow", "full_step",
              "latent_delta", "cfg5"):
        assert k not in res, k
    assert sorted(os.listdir(out)) == ["layer%d_%s.npy" % (i, n) for i, n in enumerate(["L2"] * 3 + ["L3"] * 3)]
