"""bench.py's plain run and ``--dump-outputs`` on a small config-2 shape: the line carries the headline
fields only (what ``--full`` adds is absent), ``--steps`` is the number of timed steps, and the dumped
arrays are the three-phase search's results for the same seeded inputs, computed here through
``enhanced.search3``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, NQ, K = 100_000, 8, 10


def test_plain_run_dumps_the_last_timed_steps_results(tmp_path):
    import torch
    from vectorragquantization_amd import synth
    from vectorragquantization_amd.enhanced import search3

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "c2", "--n", str(N_ROWS), "--nq", str(NQ), "--dump-outputs", str(tmp_path / "out")],
                       env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "queries/s" and rec["higher_is_better"] is True
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - NQ / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    for moved in ("phase_ms", "roofline", "recall_at_10", "cpu_baseline", "roofline_encode", "real_data"):
        assert moved not in rec

    dev = torch.device("cuda", 0)
    shard = synth.make_corpus(N_ROWS, device=dev)
    qf, qb, _ = synth.make_queries(N_ROWS, NQ, device=dev)
    ref = search3(shard["codes"], shard["x8"], shard["norms"], qf, qb, K, 10 * K, 3 * K)
    names = ("count", "rows", "hamming", "binary_score", "cosine_score")
    assert sorted(os.listdir(tmp_path / "out")) == sorted(n + ".npy" for n in names)
    for name, t in zip(names, ref):
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == np.float64
        assert np.array_equal(got, t.cpu().numpy().astype(np.float64)), name
    assert np.all(np.load(tmp_path / "out" / "count.npy") == K)
