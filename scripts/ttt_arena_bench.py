"""Tic-tac-toe arena: the Python driver versus.play_tictactoe against ONE engine call, versus.play_tictactoe_device (diee_ttt_arena), both over
the same two search = device engines of one GPU.

    python scripts/ttt_arena_bench.py [--out FILE] [--reps 20]

Model against Model (two weight blobs), 50 iterations, at 16 and 400 games.  The searches are the same launches on both sides; what differs is
who runs a round between them -- Python (a copy-out and a synchronise per search, np.power, weighted_select and the rules per game) or
k_ttt_arena_split / k_ttt_arena_move (three words per round).  Temperature 1.0, where both drivers sample from the same rows, so every
timed pair is also checked to have played the same games.  Every call is synchronous on return, so a host clock around it is a call time.
Each row is warmed up on both drivers, the two alternate rep by rep; the table gives the median and the spread, and a difference counts only
if it exceeds that spread.  A second table is diee_ttt_arena alone with flags 0 (the quirks off), option search_fused = 0 against 1 on the
hosting ctx: one launch of k_ttt_search per iteration against one of k_ttt_search_run per search, same games checked.  Prints the markdown
tables and, last, one JSON line.  Its third column is search_fused = 2, the whole call as ONE launch of k_ttt_arena_run."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diee_amd  # noqa: E402
from diee_amd import versus  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    engines = []
    for seed in (0, 1):
        e = diee_amd.Engine(0, diee_amd.GAME_TTT)
        e.load_weights(diee_amd.random_weights(seed, diee_amd.GAME_TTT))
        engines.append(e.set_option("nn", "device").set_option("search", "device"))
    players = [versus.Player(versus.Agent.MODEL, e) for e in engines]
    cfg = diee_amd.MctsConfig(iterations=50, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)
    drivers = {"python": versus.play_tictactoe, "device": versus.play_tictactoe_device}

    rows = []
    for n in (16, 400):
        t = {k: [] for k in drivers}
        for i in range(a.reps + 2):                                         # two warm-up rounds
            played = {}
            for k, play in drivers.items():
                t0 = time.perf_counter()
                res = play(players[0], players[1], cfg, 1.0, seed=100 + i, num_games=n)
                dt = time.perf_counter() - t0
                played[k] = (res.wins_p1, res.wins_p2, res.rounds, res.final_states.tobytes())
                if i >= 2:
                    t[k].append(dt)
            assert played["python"] == played["device"], "the two drivers played different games"
        rows.append((f"Model vs Model, {n} games x 50 iterations", t))
        print(rows[-1][0] + ": done", file=sys.stderr, flush=True)
    fused_rows = []
    for n in (16, 400):
        t = {"0": [], "1": [], "2": []}
        for i in range(a.reps + 2):
            played = {}
            for k in t:
                engines[0].set_option("search_fused", k)
                t0 = time.perf_counter()
                r = diee_amd.ttt_arena(engines[0], diee_amd.AGENT_MODEL, engines[1], diee_amd.AGENT_MODEL, n, cfg, 1.0, seed=100 + i, flags=[0, 0])
                dt = time.perf_counter() - t0
                played[k] = (r["wins_p1"], r["wins_p2"], r["rounds"], r["final_states"].tobytes())
                if i >= 2:
                    t[k].append(dt)
            assert played["0"] == played["1"] == played["2"], "the kernels played different games"
        fused_rows.append((f"diee_ttt_arena flags 0, {n} games x 50 iterations", t))
        print(fused_rows[-1][0] + ": done", file=sys.stderr, flush=True)
    engines[0].set_option("search_fused", "0")
    ms = lambda x: f"{1e3 * np.median(x):.2f} ({1e3 * min(x):.2f} .. {1e3 * max(x):.2f}, {len(x)} calls)"
    lines = ["| arena | play_tictactoe, ms: median (min .. max) | play_tictactoe_device, ms: median (min .. max) | python / device |", "|---|---|---|---|"]
    for what, t in rows:
        lines.append(f"| {what} | {ms(t['python'])} | {ms(t['device'])} | {np.median(t['python']) / np.median(t['device']):.2f} |")
    lines += ["", "| arena | search_fused = 0, ms: median (min .. max) | search_fused = 1, ms: median (min .. max) | search_fused = 2, ms: median (min .. max) | 0 / 1 | 1 / 2 |",
              "|---|---|---|---|---|---|"]
    for what, t in fused_rows:
        lines.append(f"| {what} | {ms(t['0'])} | {ms(t['1'])} | {ms(t['2'])} | {np.median(t['0']) / np.median(t['1']):.2f} | {np.median(t['1']) / np.median(t['2']):.2f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps({what: {"python_ms": 1e3 * float(np.median(t["python"])), "device_ms": 1e3 * float(np.median(t["device"]))} for what, t in rows}
                     | {what: {"per_iteration_ms": 1e3 * float(np.median(t["0"])), "fused_ms": 1e3 * float(np.median(t["1"])), "one_launch_ms": 1e3 * float(np.median(t["2"]))}
                        for what, t in fused_rows}))
    for e in engines:
        e.close()


if __name__ == "__main__":
    main()
