"""Tic-tac-toe search: the host search (option search = host) against k_ttt_search (search = device) and k_ttt_search_run (search = device,
search_fused = 1: the whole search in one launch), all over the device network (nn = device), on one ctx of one GPU.

    python scripts/ttt_search_bench.py [--out FILE] [--reps 30]

diee_mcts_batch at 1, 64, 1024 and 8192 empty-board roots x 50 iterations with the quirks off, at 1 root with them on, and diee_self_play
of 1024 games x 50 iterations (quirks off).  Every call is
synchronous on return, so a host clock around it is a call time.  Each row is warmed up on every path; the paths alternate rep by rep
(the option is switched between calls, which costs nothing: the buffers stay); the table gives the median and the spread, and a difference
counts only if it exceeds that spread.  Prints a markdown table and, last, one JSON line."""
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
    ap.add_argument("--out"); ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    eng = diee_amd.Engine(0, diee_amd.GAME_TTT)
    eng.set_option("nn", "device"); eng.load_weights(diee_amd.random_weights(0, diee_amd.GAME_TTT))
    cfg = diee_amd.MctsConfig.default(50)

    def timed(where, fn):
        eng.set_option("search", "host" if where == "host" else "device")
        if where != "host":
            eng.set_option("search_fused", "1" if where == "fused" else "0")
        t0 = time.perf_counter(); fn()
        return time.perf_counter() - t0

    def compare(fn, reps):
        t = {"host": [], "device": [], "fused": []}
        for i in range(reps + 2):                                           # two warm-up rounds
            for where in t:
                dt = timed(where, fn)
                if i >= 2:
                    t[where].append(dt)
        return t

    rows = []
    for n, quirks in ((1, False), (64, False), (1024, False), (8192, False), (1, True)):
        roots = diee_amd.ttt_new(n)
        reps = a.reps if n < 8192 else max(3, a.reps // 3)
        rows.append((f"mcts_batch {n} roots x 50 iterations, quirks {'on' if quirks else 'off'}",
                     compare(lambda: eng.alpha_mcts_parallel(roots, cfg, 5, 0, ref_quirks=quirks), reps)))
        print(rows[-1][0] + ": done", file=sys.stderr, flush=True)
    rows.append(("self_play 1024 games x 50 iterations, quirks off",
                 compare(lambda: eng.self_play_parallel(1024, cfg, 1.25, 7, ref_quirks=False), max(3, a.reps // 3))))
    ms = lambda x: f"{1e3 * np.median(x):.3f} ({1e3 * min(x):.3f} .. {1e3 * max(x):.3f}, {len(x)} calls)"
    lines = ["| call | search = host, ms: median (min .. max) | search = device, ms: median (min .. max) | search_fused = 1, ms: median (min .. max) "
             "| host / device | device / fused |", "|---|---|---|---|---|---|"]
    for what, t in rows:
        lines.append(f"| {what} | {ms(t['host'])} | {ms(t['device'])} | {ms(t['fused'])} | {np.median(t['host']) / np.median(t['device']):.2f} "
                     f"| {np.median(t['device']) / np.median(t['fused']):.2f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps({what: {"host_ms": 1e3 * float(np.median(t["host"])), "device_ms": 1e3 * float(np.median(t["device"])),
                             "fused_ms": 1e3 * float(np.median(t["fused"]))} for what, t in rows}))
    eng.close()


if __name__ == "__main__":
    main()
