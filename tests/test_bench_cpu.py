"""bench.py's command line on one rank with the stand-in engine of tests/test_dist_cpu.py (the CPU oracle): a plain run times its
steps and prints the line, --full adds the legs beside the headline figure, --dump-outputs writes the last timed step's records."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.test_dist_cpu import _StubEngine      # noqa: E402

BASE = ["--gpus", "1", "--games", "3", "--iterations", "5"]


def _line(capsys, args):
    import bench
    bench.main(BASE + args, engine_factory=_StubEngine)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_nothing_else(oracle, capsys):
    calls = []

    class Counting(_StubEngine):
        def self_play_parallel(self, *a, **k):
            calls.append(("single", k.get("max_steps", 0), k.get("fetch", True)))
            return super().self_play_parallel(*a, **k)

        def self_play_multi(self, *a, **k):
            calls.append(("multi",))
            return super().self_play_multi(*a, **k)
    import bench
    bench.main(BASE + ["--steps", "3", "--warmup", "2"], engine_factory=Counting)
    d = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    # the primer (one move-step), 2 warm-up steps, 3 timed steps: every call delivers its records, none is a leg of --full
    assert calls == [("single", 1, True)] + [("single", 0, True)] * 5
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 2 and d["stats"]["games"] == 3 * 3
    for key in ("value_hbm_only", "value_pipelined", "pipelined", "cpu_baseline", "learn_loop", "outputs_dumped"):
        assert key not in d, key
    assert d["metric"] == "self-play games/sec" and d["unit"] == "games/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["ms_per_step"] > 0 and abs(d["value"] - d["stats"]["games"] / (d["ms_per_step"] * 3 / 1e3)) < 1e-6 * d["value"]


def test_full_adds_the_other_legs(oracle, capsys):
    d = _line(capsys, ["--steps", "2", "--full", "--pipeline", "2", "--no-cpu-baseline"])
    assert d["full"] is True and d["stats"]["games"] == 2 * 3
    assert d["value_hbm_only"] > 0 and d["output_delivery"]["hbm_only_steps"] == 2
    assert d["value_pipelined"] > 0 and d["pipelined"]["batches"] == 2
    assert "cpu_baseline" not in d                                  # dropped by --no-cpu-baseline


def test_dump_outputs_writes_the_last_timed_step(oracle, capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    d = _line(capsys, ["--steps", "2", "--warmup", "1", "--dump-outputs", a])
    _line(capsys, ["--steps", "2", "--warmup", "1", "--dump-outputs", b])
    names = ["outcome", "ps", "state", "game", "rows"]
    assert sorted(os.listdir(a)) == sorted(n + ".npy" for n in names) == sorted(d["outputs_dumped"]["files"])
    got = {n: np.load(os.path.join(a, n + ".npy")) for n in names}
    for n in names:                                                  # same arguments, same files
        assert got[n].dtype in (np.float32, np.float64)
        assert got[n].tobytes() == np.load(os.path.join(b, n + ".npy")).tobytes(), n
    # ... and they hold what the second (last) timed call returns: seed + 0x9E37 * 1, every row (far below the size cap)
    cfg = oracle.MctsCfg(iterations=5, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)
    ref = oracle.self_play_parallel(1, 3, cfg, 1.25, 0xD1EE0001 + 0x9E37, oracle.hash_eval_fn(), oracle.game(1), ref_quirks=1)
    n = len(ref["outcome"])
    assert n > 0 and d["outputs_dumped"]["rows_delivered"] == d["outputs_dumped"]["rows_written"] == n
    assert (got["rows"] == np.arange(n)).all()
    for k in ("outcome", "ps", "state", "game"):
        assert got[k].shape == np.asarray(ref[k]).shape and (got[k] == np.asarray(ref[k])).all(), k
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) < 64 << 20


def test_dump_outputs_samples_the_same_rows_of_every_array(tmp_path, monkeypatch):
    import bench
    rng = np.random.default_rng(1)
    n = 500
    o = {"outcome": rng.integers(-1, 2, n).astype(np.int8), "ps": rng.random((n, 1352), dtype=np.float32),
         "state": rng.random((n, 16), dtype=np.float32), "game": rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)}
    monkeypatch.setattr(bench, "DUMP_BYTES", 100 * (8 + 4 + 1352 * 4 + 16 * 4 + 8))      # room for 100 rows
    rep = [bench.dump_outputs(str(tmp_path / s), o, 7) for s in ("a", "b")]
    assert rep[0]["rows_delivered"] == n and rep[0]["rows_written"] == 100 and rep[0]["bytes"] <= bench.DUMP_BYTES
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and len(np.unique(rows)) == 100 and (np.diff(rows) > 0).all() and rows.max() < n
    idx = rows.astype(np.int64)
    for k, kind in (("outcome", np.float32), ("ps", np.float32), ("state", np.float32), ("game", np.float64)):
        got = np.load(tmp_path / "a" / (k + ".npy"))
        assert got.dtype == kind and (got == o[k][idx]).all(), k              # exact: int8 / float32 in float32, u32 in float64
        assert got.tobytes() == np.load(tmp_path / "b" / (k + ".npy")).tobytes()
