"""bench.py --dump-outputs on hardware: the files hold the records of the last timed self_play_parallel call, as the engine
delivers them to any caller (small batch: 16 games, iterations = 6, played to completion)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CALL = r"""
import sys
import numpy as np
import diee_amd
eng = diee_amd.Engine(0)
eng.load_weights(diee_amd.random_weights(0))
cfg = diee_amd.MctsConfig(iterations=6, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)
o = eng.self_play_parallel(16, cfg, 1.25, 0xD1EE0001 + 0x9E37, ref_quirks=True)
np.savez(sys.argv[1], **{k: o[k] for k in ("outcome", "ps", "state", "game")})
eng.close()
"""


def test_dump_outputs_holds_the_last_timed_steps_records(tmp_path):
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--games", "16", "--iterations", "6",
                        "--dump-outputs", out], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 2 and d["stats"]["games"] == 2 * 16 and d["ms_per_step"] > 0
    assert "value_pipelined" not in d and "value_hbm_only" not in d and "cpu_baseline" not in d
    got = {n: np.load(os.path.join(out, n + ".npy")) for n in ("outcome", "ps", "state", "game", "rows")}
    # the same call made by another caller: step 1 of the timed loop (seed + 0x9E37 * 1), in a process of its own like the bench
    q = subprocess.run([sys.executable, "-c", _CALL, str(tmp_path / "ref.npz")], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert q.returncode == 0, q.stderr.decode()[-3000:]
    ref = np.load(tmp_path / "ref.npz")
    n = len(ref["outcome"])
    assert n > 0 and d["outputs_dumped"]["rows_delivered"] == d["outputs_dumped"]["rows_written"] == n
    assert (got["rows"] == np.arange(n)).all()
    for k, kind in (("outcome", np.float32), ("ps", np.float32), ("state", np.float32), ("game", np.float64)):
        assert got[k].dtype == kind and got[k].shape == ref[k].shape, k
        assert (got[k] == ref[k]).all(), k                               # bit-exact: the same seeds, the same kernels
