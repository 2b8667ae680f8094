#!/usr/bin/env python3
"""Random shooting with one env's candidates spread over S workgroups (qs_shooting_plan_split), docking-v0, horizon 20, on one
MI355X: N in {1, 8, 64, 512} envs x paths in {1024, 16384, 65536}, and per cell

  base    qs_shooting_plan: one workgroup per env, the kernel this library had before (= S 1)
  auto    qs_shooting_plan_split with splits = 0: the library's choice (qs_shooting_plan_splits reports it)
  S=..    the sweep S in {2, 8, 32, 128, 512, 1024} where S <= min(paths, 1024)

All configurations of a cell alternate inside every round for --rounds rounds after a warm-up round; every figure is per
round and the summary gives ranges, never means.  A window is --reps calls between qs_timer_start / qs_timer_stop on the
handle's stream: stream time, which for plans of tens of microseconds includes the gap in which the host reads the step
counter back (every plan does) and launches; the wall time per plan is recorded beside it.  The calls go to the C entry
points with preallocated outputs so that the gap is the library's and not the allocator's.

Conditions (profiles/shooting_split/README.md): (1) at N = 1 / 65 536 paths `auto` is faster than `base` in every round;
(2) in no cell is `auto` slower than `base` beyond the cell's round-to-round spread, taken as the larger of the two ranges'
widths: max(auto) <= max(base) + spread.

--host adds the host path: wall time of one DockingEnv.shooting_plan(20, 200) + env.step() iteration, beside the 20 ms
control period of dt = 0.02.  One JSON line per (cell, round) on stdout, everything in --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plan_timing  # noqa: E402  (tools/ is the script's directory)

SWEEP = (2, 8, 32, 128, 512, 1024)


def plan_and_step(env, carry):
    t1 = time.perf_counter()
    plan = env.shooting_plan(20, 200)
    carry["plan_s"] += time.perf_counter() - t1
    env.step(plan["actions"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,8,64,512")
    ap.add_argument("--paths", default="1024,16384,65536")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="calls inside one timed window")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa

    lib = qa._lib.load()
    H = args.horizon
    results, summary = [], []
    for n in [int(x) for x in args.envs.split(",")]:
        env = plan_timing.stepped_env(qa, n)
        act = torch.empty((n, 4), dtype=torch.float32, device=env.device)
        score = torch.empty((n,), dtype=torch.float64, device=env.device)
        index = torch.empty((n,), dtype=torch.int32, device=env.device)
        bufs = [C.c_void_p(t.data_ptr()) for t in (act, score, index)] + [None, None]
        env._use_current_stream()
        for paths in [int(p) for p in args.paths.split(",")]:
            auto = qa.plan_splits(env, paths)
            configs = [("base", None), ("auto", 0)] + [("S=%d" % s, s) for s in SWEEP if s <= min(paths, 1024)]

            def plan(s):
                if s is None:
                    rc = lib.qs_shooting_plan(env._h, H, paths, 0, *bufs)
                else:
                    rc = lib.qs_shooting_plan_split(env._h, H, paths, 0, s, *bufs)
                qa._lib.check(rc, "plan")

            want = None
            for name, s in configs:                           # the results agree before anything is timed
                plan(s)
                torch.cuda.synchronize()
                got = (act.clone(), score.clone(), index.clone())
                want = want or got
                assert all(torch.equal(a, b) for a, b in zip(got, want)), (n, paths, name)
            rows = plan_timing.alternating_rounds(torch, env, configs, plan, args.rounds, args.reps,
                                                  dict(envs=n, paths=paths, horizon=H, auto_splits=auto, candidate_steps=n * paths * H))
            results += rows
            cell = dict(envs=n, paths=paths, horizon=H, auto_splits=auto, rounds=len(rows),
                        **plan_timing.ranges(rows, [k for k in rows[0] if k.endswith("_ms")]))
            spread = max(cell["base_ms"][1] - cell["base_ms"][0], cell["auto_ms"][1] - cell["auto_ms"][0])
            cell["spread_ms"] = spread
            cell["auto_faster_than_base_in_every_round"] = all(r["auto_ms"] < r["base_ms"] for r in rows)
            cell["auto_not_slower_than_base_beyond_spread"] = cell["auto_ms"][1] <= cell["base_ms"][1] + spread
            cell["base_over_auto"] = plan_timing.ratio_range(rows, "base_ms", "auto_ms")
            summary.append(cell)
            print(json.dumps(dict(summary=cell)), flush=True)
        env.close()
    host = plan_timing.host_path(qa, args.rounds, plan_and_step, paths=200, horizon=20) if args.host else None
    if host:
        print(json.dumps(dict(host=host)), flush=True)
    plan_timing.write_out(args.out, torch, cus=torch.cuda.get_device_properties(0).multi_processor_count, reps=args.reps,
                          summary=summary, host=host, rounds=results)

if __name__ == "__main__":
    main()
