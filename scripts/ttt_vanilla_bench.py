"""Tic-tac-toe Agent::Mcts: the host search (option search = host) against k_ttt_vanilla (search = device) on one weightless ctx of one GPU.

    python scripts/ttt_vanilla_bench.py [--out FILE] [--reps 30]

diee_ttt_mcts_vanilla_batch at 1, 64 and 1024 empty-board roots x 200 iterations, rollouts played (quirks off), round_limit 400; then ONE
launch at the per-launch bound: 1024 empty-board roots x 4096 iterations on the device alone (what kVanillaItersPerLaunch promises to keep
far below a second).  Every call is synchronous on return, so a host clock around it is a call time.  Each row is warmed up on both paths;
the two paths alternate rep by rep (the option is switched between calls, which costs nothing: the buffers stay); the table gives the
median and the spread, and a difference counts only if it exceeds that spread.  Prints a markdown table and, last, one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diee_amd  # noqa: E402

ITERS_PER_LAUNCH = 4096                                                     # kVanillaItersPerLaunch of csrc/ttt_vanilla_device.h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    eng = diee_amd.Engine(0, diee_amd.GAME_TTT)
    eng.set_option("nn", "device")
    cfg = diee_amd.MctsConfig(iterations=200, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)

    def timed(where, fn):
        eng.set_option("search", where)
        t0 = time.perf_counter(); fn()
        return time.perf_counter() - t0

    rows = []
    for n in (1, 64, 1024):
        roots = diee_amd.ttt_new(n)
        t = {"host": [], "device": []}
        for i in range(a.reps + 2):                                         # two warm-up rounds
            for where in ("host", "device"):
                dt = timed(where, lambda: eng.ttt_mct_search(roots, cfg, 5, ref_quirks=False))
                if i >= 2:
                    t[where].append(dt)
        rows.append((f"ttt_mct_search {n} roots x 200 iterations", t))
        print(rows[-1][0] + ": done", file=sys.stderr, flush=True)
    one = diee_amd.MctsConfig(iterations=ITERS_PER_LAUNCH, c=2.0, round_limit=400, dir_alpha=0.3, dir_eps=0.25)
    roots = diee_amd.ttt_new(1024)
    launch = [timed("device", lambda: eng.ttt_mct_search(roots, one, 5, ref_quirks=False)) for _ in range(2 + max(3, a.reps // 3))][2:]
    ms = lambda x: f"{1e3 * np.median(x):.3f} ({1e3 * min(x):.3f} .. {1e3 * max(x):.3f}, {len(x)} calls)"
    lines = ["| call | search = host, ms: median (min .. max) | search = device, ms: median (min .. max) | host / device |", "|---|---|---|---|"]
    for what, t in rows:
        lines.append(f"| {what} | {ms(t['host'])} | {ms(t['device'])} | {np.median(t['host']) / np.median(t['device']):.2f} |")
    lines.append(f"| one launch: 1024 roots x {ITERS_PER_LAUNCH} iterations (the call, copies included) | -- | {ms(launch)} | -- |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    res = {what: {"host_ms": 1e3 * float(np.median(t["host"])), "device_ms": 1e3 * float(np.median(t["device"]))} for what, t in rows}
    res["one_launch_ms"] = 1e3 * float(np.median(launch))
    print(json.dumps(res))
    eng.close()


if __name__ == "__main__":
    main()
