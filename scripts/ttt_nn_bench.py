"""Tic-tac-toe network: host loops (option nn = host) against k_ttt_net (nn = device) on one GPU.

    python scripts/ttt_nn_bench.py [--out FILE] [--host-budget SECONDS] [--sizes 1,64,1024,8192]

forward at n = 1, 64, 1024, 8192 and diee_mcts_batch at 1024 roots x 50 iterations.  Every call is synchronous on return, so a host clock
around it is a call time (transfers, launch and synchronise included: what a search pays per iteration).  Each size is warmed up on both paths;
the two paths alternate rep by rep; the table gives the median and the spread.  The host path is given --host-budget seconds per size (at
least one call), the device path the same number of calls but no fewer than 20.  Prints a markdown table and, last, one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import diee_amd  # noqa: E402


def states(n, seed=3):
    rng = np.random.default_rng(seed)
    s = diee_amd.ttt_new(n)
    s["board"] = rng.integers(-1, 2, size=(n, 9)); s["player"] = rng.choice([-1, 1], size=n)
    return s


def timed(fn):
    t0 = time.perf_counter(); fn()
    return time.perf_counter() - t0


def compare(host_fn, dev_fn, budget):
    first = timed(host_fn); timed(dev_fn); timed(dev_fn)                 # warm-up of both (the host's doubles as its cost estimate)
    print(f"  host warm-up call {first:.3f} s", file=sys.stderr, flush=True)
    reps = max(1, min(200, int(budget / max(first, 1e-6))))
    h, d = [], []
    for i in range(max(reps, 20)):
        if i < reps:
            h.append(timed(host_fn))
        d.append(timed(dev_fn))
    return h, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--host-budget", type=float, default=20.0)
    ap.add_argument("--sizes", default="1,64,1024,8192", help="batch sizes of the forward rows (a finer list locates the crossover)")
    a = ap.parse_args()
    blob = diee_amd.random_weights(0, diee_amd.GAME_TTT)
    host = diee_amd.Engine(0, diee_amd.GAME_TTT); host.load_weights(blob)
    dev = diee_amd.Engine(0, diee_amd.GAME_TTT); dev.load_weights(blob); dev.set_option("nn", "device")
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        s = states(n)
        h, d = compare(lambda: host.forward_t(s), lambda: dev.forward_t(s), a.host_budget)
        dp = np.abs(host.forward_t(s)[0] - dev.forward_t(s)[0]).max()
        rows.append({"what": f"forward n={n}", "host": h, "device": d, "max_dpolicy": float(dp)})
        print(f"forward n={n}: done", file=sys.stderr, flush=True)
    cfg = diee_amd.MctsConfig.default(50)
    roots = diee_amd.ttt_new(1024)
    h, d = compare(lambda: host.alpha_mcts_parallel(roots, cfg, 5, 0), lambda: dev.alpha_mcts_parallel(roots, cfg, 5, 0), a.host_budget)
    rows.append({"what": "mcts_batch 1024 roots x 50 iterations", "host": h, "device": d, "max_dpolicy": None})
    ms = lambda x: f"{1e3 * np.median(x):.3f} ({1e3 * min(x):.3f} .. {1e3 * max(x):.3f}, {len(x)} calls)"
    lines = ["| call | host, ms: median (min .. max) | device, ms: median (min .. max) | host / device |", "|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['what']} | {ms(r['host'])} | {ms(r['device'])} | {np.median(r['host']) / np.median(r['device']):.2f} |")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    print(json.dumps({r["what"]: {"host_ms": 1e3 * float(np.median(r["host"])), "device_ms": 1e3 * float(np.median(r["device"])),
                                  "max_dpolicy": r["max_dpolicy"]} for r in rows}))


if __name__ == "__main__":
    main()
