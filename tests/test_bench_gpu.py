"""bench.py's plain run and --dump-outputs on an MI355X, at the small audio-only C3 configuration: the result line keeps its
contract and nothing that takes runs of its own (roofline / decode / cpu_baseline are --full only); the dumped arrays are
float32/float64 within 64 MB, the loss file is the loss the line reports, and a second run with the same arguments computes the
same outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "c3", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(tmp_path):
    j, arrays = _bench(tmp_path / "a")
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["metric"] == "training samples/sec" and j["unit"] == "samples/s" and j["higher_is_better"] is True and j["dtype"] == "bf16"
    assert not {"roofline", "decode", "cpu_baseline"} & set(j)
    assert sorted(arrays) == ["grads.npy", "loss.npy", "params.npy"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    assert np.isfinite(arrays["loss.npy"]).all() and abs(float(arrays["loss.npy"][0]) - j["final_loss"]) <= 1e-4
    assert arrays["params.npy"].shape == arrays["grads.npy"].shape
    assert np.isfinite(arrays["params.npy"]).all() and np.isfinite(arrays["grads.npy"]).all()
    assert np.abs(arrays["grads.npy"]).max() > 0

    # Same arguments again: every step starts from the same state, so only the order of the fp32 atomics in the weight-gradient
    # sums of the last step differs between the runs (rounding), and Adam's first update is sign-like (lr * g / |g|).
    _, again = _bench(tmp_path / "b")
    np.testing.assert_allclose(again["loss.npy"], arrays["loss.npy"], rtol=1e-5)
    np.testing.assert_allclose(again["params.npy"], arrays["params.npy"], rtol=0, atol=1e-5)
    g0, g1 = arrays["grads.npy"].astype(np.float64), again["grads.npy"].astype(np.float64)
    assert np.linalg.norm(g1 - g0) / np.linalg.norm(g0) < 1e-4
