"""The arena on the Python driver against the arena in one engine call, on ONE box, back to back in one process:

    python    die-e_amd/versus.py::play         a Python loop over rounds: two diee_mcts_batch calls, sampling, decode, legality, apply per round
    device    die-e_amd/versus.py::play_device  diee_arena: every round on the device, one small device->host read per round

    python scripts/arena_bench.py [--games 400] [--iterations 100] [--round-limit 400] [--temperature 1.25] [--warmup-games 8]
                                  [--record-turns] [--device-repeats 1]

Two random-init networks (seeds 0 and 1) on two engines of device 0, BASELINE configs[4]'s arena by default.  Each path is warmed up on
a few games (buffers, code objects) and then taken ONCE.  The two results must be equal -- final states, wins, rounds, the retired games in
order -- or the script fails.  Prints one JSON line: wall clock of each path and their ratio, rounds, and per player of the device call its
searches and node expansions per second of the call (diee_stats of diee_arena).  --record-turns: both paths record every turn (the
device through its turn log, diee_arena_ex) and the turns must be equal too.  --device-repeats N: the device path is taken N times,
device_s is the first and device_s_all lists them (the repeat spread of one process)."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0xD1EE0001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=400)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--round-limit", type=int, default=400)
    ap.add_argument("--temperature", type=float, default=1.25)
    ap.add_argument("--warmup-games", type=int, default=8)
    ap.add_argument("--record-turns", action="store_true")
    ap.add_argument("--device-repeats", type=int, default=1)
    args = ap.parse_args()
    import diee_amd
    versus = importlib.import_module("die-e_amd.versus")
    e1 = diee_amd.Engine(0); e1.load_weights(diee_amd.random_weights(0))
    e2 = diee_amd.Engine(0); e2.load_weights(diee_amd.random_weights(1))
    cfg = diee_amd.MctsConfig.default(args.iterations)
    p1, p2 = versus.Player(versus.Agent.MODEL, e1), versus.Player(versus.Agent.MODEL, e2)

    def run(fn, games, **kw):
        if args.record_turns:
            kw["record_turns"] = True
        t0 = time.perf_counter()
        res = fn(p1, p2, cfg, args.temperature, seed=SEED, num_games=games, round_limit=args.round_limit, **kw)
        return res, time.perf_counter() - t0

    if args.warmup_games:
        run(versus.play, args.warmup_games, max_rounds=4)
        run(versus.play_device, args.warmup_games, max_rounds=4)
    ref, t_py = run(versus.play, args.games)
    dev, t_dev = run(versus.play_device, args.games)
    t_all = [t_dev] + [run(versus.play_device, args.games)[1] for _ in range(args.device_repeats - 1)]

    def summary(r):
        return (r.wins_p1, r.wins_p2, r.draws, r.rounds, [(g.initial_state["id"], g.winner) for g in r.games])
    assert dev.final_states.tobytes() == ref.final_states.tobytes(), "final states differ"
    assert summary(dev) == summary(ref), "results differ"
    assert dev.turns == ref.turns, "recorded turns differ"
    st = dev.device["stats"]
    line = {"games": args.games, "iterations": args.iterations, "round_limit": args.round_limit, "rounds": dev.rounds,
            "wins_p1": dev.wins_p1, "wins_p2": dev.wins_p2, "draws": dev.draws, "equal": True,
            "python_s": round(t_py, 3), "device_s": round(t_dev, 3), "device_call_s": round(dev.device["seconds"], 3),
            "python_over_device": round(t_py / t_dev, 3), "record_turns": args.record_turns, "device_s_all": [round(t, 3) for t in t_all],
            "turns": None if dev.turns is None else sum(len(t) for t in dev.turns),
            "players": [{"searches": s["move_steps"], "turns": s["plies"], "skipped_turns": s["plies"] - s["fragments"],
                         "expansions": s["expansions"], "expansions_per_s": round(s["expansions"] / s["seconds"], 1)} for s in st]}
    print(json.dumps(line))
    e1.close(); e2.close()


if __name__ == "__main__":
    main()
