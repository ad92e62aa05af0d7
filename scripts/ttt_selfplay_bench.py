"""Tic-tac-toe self-play: the host loop over one k_ttt_search_run launch per move-step (search_fused = 1) against the whole call as one
search-and-play launch of k_ttt_selfplay_run plus the delivery (search_fused = 2), on one ctx of one GPU (nn = device, search = device).

    python scripts/ttt_selfplay_bench.py [--out FILE] [--reps 20] [--games 16,1024,4096]

diee_self_play with the quirks off, 50 iterations, at 16, 1024 and 4096 games.  The call is synchronous on return, so a host clock around it
is a call time.  Each row is warmed up on both paths; the paths alternate call by call (the option is switched between calls, which costs
nothing: the buffers stay); every pair is checked to have delivered the same records.  The table gives the median and the spread, and a
difference counts only if it lies outside both spreads.  Prints a markdown table and, last, one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diee_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--reps", type=int, default=20); ap.add_argument("--games", default="16,1024,4096")
    a = ap.parse_args()
    eng = diee_amd.Engine(0, diee_amd.GAME_TTT)
    eng.set_option("nn", "device").set_option("search", "device")
    eng.load_weights(diee_amd.random_weights(0, diee_amd.GAME_TTT))
    cfg = diee_amd.MctsConfig.default(50)

    rows = []
    for n in map(int, a.games.split(",")):
        t = {"1": [], "2": []}
        for i in range(a.reps + 2):                                         # two warm-up rounds
            got = {}
            for fused in t:
                eng.set_option("search_fused", fused)
                t0 = time.perf_counter()
                got[fused] = eng.self_play_parallel(n, cfg, 1.25, 7 + i, ref_quirks=False)
                dt = time.perf_counter() - t0
                if i >= 2:
                    t[fused].append(dt)
                assert int(eng.get_option("self_play_last_launches")) == (got[fused]["stats"]["move_steps"] if fused == "1" else 1)
            assert all(got["1"][k].tobytes() == got["2"][k].tobytes() for k in ("outcome", "game", "state", "ps")), f"{n} games: the records differ"
        rows.append((n, t, got["1"]["stats"]["move_steps"], len(got["1"]["outcome"])))
        print(f"{n} games: done", file=sys.stderr, flush=True)
    ms = lambda x: f"{1e3 * np.median(x):.3f} ({1e3 * min(x):.3f} .. {1e3 * max(x):.3f})"
    lines = [f"diee_self_play, 50 iterations, quirks off, {a.reps} calls per path, same records checked per pair; ms: median (min .. max)", "",
             "| games | move-steps | rows | search_fused = 1 | search_fused = 2 | 1 / 2 | outside both spreads |", "|---|---|---|---|---|---|---|"]
    for n, t, steps, nf in rows:
        apart = min(t["1"]) > max(t["2"]) or min(t["2"]) > max(t["1"])
        lines.append(f"| {n} | {steps} | {nf} | {ms(t['1'])} | {ms(t['2'])} | {np.median(t['1']) / np.median(t['2']):.2f} | {'yes' if apart else 'no'} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps({f"{n} games": {"fused1_ms": 1e3 * float(np.median(t["1"])), "fused2_ms": 1e3 * float(np.median(t["2"]))} for n, t, _, _ in rows}))
    eng.close()


if __name__ == "__main__":
    main()
