"""bench.py's plain run in a fresh process (``-m gpu``, MI355X): the headline only -- the line's contract fields, exactly
``--steps`` timed steps, none of the ``--full`` blocks -- and ``--dump-outputs`` writing what the last timed step produced."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    env = dict(os.environ, L4D_BENCH_DETAIL=str(tmp_path / "bench_detail.json"))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c3-1k", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "rays/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 / 1024 - 1) < 1e-3  # value = rays per step / step time
    assert d["config"]["skipped_steps_in_timed_region"] == 0
    assert d["roofline"] is None and not {"cpu_baseline", "parity", "variants", "hash_encoder", "mfma"} & set(d)
    files = sorted(os.listdir(out))
    assert files == ["grads.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    a = {f[:-4]: np.load(out / f) for f in files}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["loss"].shape == (1,) and a["loss"][0] > 0 and a["params"].shape == a["grads"].shape
    assert np.abs(a["grads"]).max() > 0
