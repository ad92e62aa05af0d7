"""Slot refill against the two ways the learn loop can play its K batches today, on ONE box, back to back:

    sequential   K diee_self_play calls, one after the other
    multi        one diee_self_play_multi call (the learn loop's default; the yardstick)
    refill:W     one diee_self_play_refill call with W games in flight

    python scripts/refill_bench.py [--batches 4] [--games 1024] [--iterations 100] [--widths 1024,2048] [--leg-timeout 600]

All legs play the same (seed, game id) games without the quirks (refill has no other mode) and deliver their records to host memory inside
the timed region.  Every leg is a process of its own under its own time limit (`--leg` is the worker): a warm-up call truncated to a few
move-steps sizes the buffers and loads the code objects, then ONE timed call (sequential: K of them).  Per leg: games/s over the host clock
around the calls (each ends in a device synchronise), the share of the leg's move-steps played with >= 929 live games (one pass of the chip
through the dominant kernel; from the engine's own move-step trace, option trace_steps), end to end = expansions x 1.0825 GFLOP / time / the
dense bf16 peak, and the box's tower clock fraction: the sampled one-launch evaluations of 929 ... 1024 boards (full_flops / full_seconds)
over the same peak -- boxes differ by that kernel's power-limited clock, so only legs of one run compare.  Prints one JSON line per leg and
a summary line."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0          # dense bf16 MFMA peak (bench.py)
FLOPS_PER_EVAL = 1_082_450_064     # one evaluated state (bench.py)
SEED = 0xD1EE0001
FULL_FROM = 929


def worker(args):
    import diee_amd
    eng = diee_amd.Engine(0)
    eng.load_weights(diee_amd.random_weights(0))
    cfg = diee_amd.MctsConfig.default(args.iterations)
    K, n = args.batches, args.games
    batches = [(n, 0, SEED + 0x9E37 * i) for i in range(K)]
    kind, _, w = args.leg.partition(":")

    def play(max_steps):
        if kind == "sequential":
            return [eng.self_play_parallel(nb, cfg, 1.25, seed, ref_quirks=False, first_game_id=first, max_steps=max_steps, copy=False)
                    for nb, first, seed in batches]
        if kind == "multi":
            return eng.self_play_multi(batches, cfg, 1.25, ref_quirks=False, max_steps=max_steps, copy=False)
        return eng.self_play_refill(batches, int(w), cfg, 1.25, max_steps=max_steps, copy=False)

    for o in play(3):                       # sizes the arenas, the pinned output blocks and the code objects
        o["free"]()
    eng.set_option("trace_steps", 1)        # one stderr line per move-step with its live games (a few hundred lines per leg)
    sys.stderr.write("[refill_bench] timed\n"); sys.stderr.flush()
    t0 = time.perf_counter()
    outs = play(0)
    dt = time.perf_counter() - t0
    eng.set_option("trace_steps", 0)
    tot = {k: sum(o["stats"][k] for o in outs) for k in ("games", "plies", "fragments", "expansions", "full_seconds", "full_launches", "full_flops")}
    steps = (sum if kind == "sequential" else max)(o["stats"]["move_steps"] for o in outs)
    for o in outs:
        o["free"]()
    print(json.dumps({"leg": args.leg, "games": tot["games"], "seconds": dt, "games_per_s": tot["games"] / dt, "move_steps": steps,
                      "plies": tot["plies"], "fragments": tot["fragments"],
                      "end_to_end_frac": tot["expansions"] * FLOPS_PER_EVAL / dt / 1e12 / PEAK_BF16_TFLOPS,
                      "tower_clock_frac": (tot["full_flops"] / tot["full_seconds"] / 1e12 / PEAK_BF16_TFLOPS) if tot["full_seconds"] else None,
                      "full_launches_sampled": tot["full_launches"]}), flush=True)
    eng.close()


def run_leg(leg, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--batches", str(args.batches), "--games", str(args.games),
           "--iterations", str(args.iterations)]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.leg_timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return {"leg": leg, "error": f"time limit of {args.leg_timeout} s"}
    if p.returncode != 0:
        return {"leg": leg, "error": f"exit status {p.returncode}", "stderr": p.stderr.decode(errors="replace")[-2000:]}
    res = json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])
    trace = p.stderr.decode(errors="replace").split("[refill_bench] timed", 1)[-1]
    live = [int(m) for m in re.findall(r"move-step \d+: (\d+) games alive", trace)]
    res["move_steps_traced"] = len(live)
    res["share_of_move_steps_full"] = sum(1 for x in live if x >= FULL_FROM) / max(len(live), 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--widths", default="1024,2048")
    ap.add_argument("--leg-timeout", type=int, default=600)
    ap.add_argument("--leg", default=None, help="worker: sequential | multi | refill:W")
    args = ap.parse_args()
    if args.leg:
        return worker(args)
    legs = ["sequential", "multi"] + [f"refill:{int(w)}" for w in args.widths.split(",") if w]
    results = []
    for leg in legs:
        r = run_leg(leg, args)
        print(json.dumps(r), flush=True)
        results.append(r)
        if "error" in r:                    # a leg that failed or ran out of time: nothing more goes to the GPU from here
            return 1
    base = next(r for r in results if r["leg"] == "multi")
    print(json.dumps({"summary": {r["leg"]: {"games_per_s": round(r["games_per_s"], 2), "vs_multi": round(r["games_per_s"] / base["games_per_s"], 4),
                                             "share_of_move_steps_full": round(r["share_of_move_steps_full"], 4),
                                             "end_to_end_frac": round(r["end_to_end_frac"], 4)} for r in results},
                      "tower_clock_frac": base["tower_clock_frac"], "batches": args.batches, "games": args.games, "iterations": args.iterations}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
