"""CPU checks of the slot-refill boundary (diee_self_play_refill): declared in include/diee.h, exported by libdiee.so, listed in
the Python mirror's EXPORTS and reachable as Engine.self_play_refill.  No compute calls."""
import os
import re

import diee_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_self_play_refill():
    src = open(os.path.join(ROOT, "include", "diee.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"diee_status\s+diee_self_play_refill\s*\(([^;]*)\)\s*;", src)
    assert m, "include/diee.h does not declare diee_self_play_refill"
    args = [a.strip() for a in m.group(1).split(",")]
    # ctx, batches, n_batches, width, cfg, temperature, flags, max_steps, outs, stats
    assert len(args) == 10 and "width" in args[3] and args[3].startswith("uint32_t")


def test_library_exports_self_play_refill():
    L = diee_amd.load_library()
    assert hasattr(L, "diee_self_play_refill")


def test_python_mirror_lists_and_wraps_it():
    assert "diee_self_play_refill" in diee_amd.EXPORTS
    assert callable(getattr(diee_amd.Engine, "self_play_refill", None))


class _RecordingEngine:
    """stands in for the engine under the learn loop's self-play step: records which entry point was called with what"""

    def __init__(self):
        self.calls = []

    def _outs(self, batches):
        import numpy as np
        return [{"outcome": np.zeros(1, np.int8), "ps": np.zeros((1, 1352), np.float32), "state": np.zeros((1, 144), np.float32),
                 "stats": {"games": n}} for n, _, _ in batches]

    def self_play_multi(self, batches, cfg, temperature=1.25, ref_quirks=True, **kw):
        self.calls.append(("multi", list(batches), ref_quirks))
        return self._outs(batches)

    def self_play_refill(self, batches, width, cfg, temperature=1.25, **kw):
        self.calls.append(("refill", list(batches), width))
        return self._outs(batches)


def _learn_loop(engine):
    import importlib
    az_mod = importlib.import_module("die-e_amd.alphazero")
    az = az_mod.AlphaZero.__new__(az_mod.AlphaZero)
    az.engine, az.rank, az.seed, az.calls, az.quiet, az.game = engine, 0, 11, 0, True, az_mod.BACKGAMMON
    az.config = az_mod.AlphaZeroConfig(temperature=1.25, learn_iterations=1, self_play_iterations=3, num_epochs=1, training_batch_size=4,
                                       num_self_play_batches=6)
    az.mcts_config = diee_amd.MctsConfig.default(4)
    return az


def test_learn_loop_plays_through_one_refill_call_only_when_asked(monkeypatch):
    """DIEE_REFILL_WIDTH=n: the K batches of self_play_iterations_pipelined go through ONE diee_self_play_refill call of that width, with
    the seeds and game ids the default path gives them; without it the loop calls diee_self_play_multi with the quirks as before"""
    monkeypatch.delenv("DIEE_REFILL_WIDTH", raising=False)
    e0 = _RecordingEngine()
    out0 = _learn_loop(e0).self_play_iterations_pipelined()
    assert [c[0] for c in e0.calls] == ["multi"] and e0.calls[0][2] is True and len(out0) == 3
    monkeypatch.setenv("DIEE_REFILL_WIDTH", "4")
    e1 = _RecordingEngine()
    out1 = _learn_loop(e1).self_play_iterations_pipelined()
    assert [c[0] for c in e1.calls] == ["refill"] and e1.calls[0][2] == 4 and len(out1) == 3
    assert e1.calls[0][1] == e0.calls[0][1] and len(e1.calls[0][1]) == 3
