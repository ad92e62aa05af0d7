"""Agent::Mcts on the device (diee_mcts_vanilla_batch): searches/s and rollout plies/s of the level-1 call -- 400 roots at the opening
position, iterations = 100, round_limit = 400, rollouts played (quirks off) -- against the stand-alone enumerator rate of
scripts/rules_bench.py measured in the same run: every rollout ply is one legal-play enumeration, so that rate is the ceiling for
plies/s.  Then the wall clock of one diee_arena of 400 games, Mcts vs Random.

    python scripts/vanilla_bench.py [--roots 400] [--iterations 100] [--round-limit 400] [--reps 3] [--no-arena]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import diee_amd
from rules_bench import reachable_states

ap = argparse.ArgumentParser()
ap.add_argument("--roots", type=int, default=400)
ap.add_argument("--iterations", type=int, default=100)
ap.add_argument("--round-limit", type=int, default=400)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--no-arena", action="store_true")
args = ap.parse_args()

e = diee_amd.Engine(0)
cfg = diee_amd.MctsConfig(iterations=args.iterations, c=2.0, round_limit=args.round_limit, dir_alpha=0.3, dir_eps=0.25)
versus = __import__("importlib").import_module("die-e_amd.versus")
roots = versus.new_states(args.roots)
roots["roll"] = (3, 1)
ids = np.arange(args.roots, dtype=np.uint32)

for quirks in (False, True):
    e.mct_search(roots, cfg, 1, ids, ref_quirks=quirks)                       # warm-up: code objects, buffers
    best = None
    for rep in range(args.reps):
        st = e.mct_search(roots, cfg, 2 + rep, ids, ref_quirks=quirks)["stats"]
        if best is None or st["seconds"] < best["seconds"]:
            best = st
        print(f"  quirks {'on ' if quirks else 'off'} rep {rep}: {st['seconds'] * 1e3:8.1f} ms, {st['rollout_plies']} plies, "
              f"{st['rollout_decided']} of {st['rollouts']} rollouts decided, mean depth {st['depth_sum'] / max(st['iterations'], 1):.2f}", flush=True)
    if not quirks:
        played = best
    print(f"quirks {'on ' if quirks else 'off'}: {args.roots / best['seconds']:9.1f} searches/s, {best['iterations'] / best['seconds'] / 1e6:7.3f} M iterations/s, "
          f"{best['rollout_plies'] / best['seconds'] / 1e6:7.3f} M rollout plies/s (best of {args.reps}, wall clock of the call)", flush=True)

e.load_weights(diee_amd.random_weights(0))                                    # (the positions of rules_bench.py come from a self-play)
s = reachable_states(e)
m = min(len(s), 8192)
us, k = e.rules_bench(s[:m], 50)
ceiling = m / us                                                              # M states/s
plies = played["rollout_plies"] / played["seconds"] / 1e6
print(f"enumerator alone: {m} resident states in {us:.1f} us = {ceiling:.1f} M enumerations/s (mean plays {k:.2f})")
print(f"rollout plies/s over that ceiling: {plies:.3f} / {ceiling:.1f} = {plies / ceiling * 100:.2f} %", flush=True)

if not args.no_arena:
    for quirks in (True, False):
        t0 = time.perf_counter()
        r = diee_amd.arena(e, diee_amd.AGENT_MCTS, None, diee_amd.AGENT_RANDOM, 400, cfg, seed=7, round_limit=400, ref_quirks=quirks)
        st = r["stats"][0]
        print(f"diee_arena, 400 games Mcts vs Random, quirks {'on' if quirks else 'off'}: {r['seconds']:.2f} s ({time.perf_counter() - t0:.2f} s with the copies), "
              f"{r['rounds']} rounds, {r['wins_p1']} : {r['wins_p2']} (draws {r['draws']}), {st['move_steps']} searches, {st['selections']} iterations", flush=True)
