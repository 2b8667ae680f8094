#!/usr/bin/env python3
"""MPPI with one env's candidates spread over S workgroups (qs_mppi_plan_split), docking-v0, horizon 20, on one MI355X:
N in {1, 8, 64, 512} envs x paths in {1024, 4096, 16384, 65536} x iterations in {1, 2, 4}, and per cell

  base    qs_mppi_plan: one workgroup per env, the kernel this library had before (paths <= 4096 only)
  S=1     qs_mppi_plan_split with splits = 1: the same kernel through the new entry point (paths <= 4096 only)
  auto    qs_mppi_plan_split with splits = 0: the library's choice (plan_splits reports it, raised to 2 above 4096 paths)
  S=..    the sweep S in {2, 8, 32, 128, 512} where S <= min(paths, 1024)
  floor   `iterations` calls of qs_shooting_plan_split with splits = 0 at the same `paths`: as many roll-outs without the
          update, the comparison of tools/mppi_rate.py's case (b); the only baseline above 4096 paths

All configurations of a cell alternate inside every round for --rounds rounds after a warm-up round; every figure is per
round and the summary gives ranges, never means.  A window is --reps calls between qs_timer_start / qs_timer_stop on the
handle's stream: stream time, which includes the gap in which the host reads the step counter back (every plan does) and
launches; the wall time per plan is recorded beside it.  Cells of more than --big candidate steps per plan take --big-reps
calls per window.  The calls go to the C entry points with preallocated outputs.

Conditions (profiles/mppi_split/README.md): (1) at N = 1 / 4096 paths / 2 iterations `auto` is faster than `base` in every
round; (2) in no cell with paths <= 4096 is `auto` slower than `S=1` beyond the cell's round-to-round spread, taken as the
larger of the two ranges' widths: max(auto) <= max(S=1) + spread.

--host adds the host path: wall time of one DockingEnv.mppi_plan(20, 200, 2) + env.step() iteration with the nominal carried,
beside the 20 ms control period of dt = 0.02.  One JSON line per (cell, round) on stdout, everything in --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plan_timing  # noqa: E402  (tools/ is the script's directory)

SWEEP = (2, 8, 32, 128, 512)
LAM, SIGMA = 0.05, 0.25


def plan_and_step(env, carry):
    nominal = carry.get("nominal")
    t1 = time.perf_counter()
    plan = env.mppi_plan(20, 200, 2, nominal=nominal, shift=nominal is not None)
    carry["plan_s"] += time.perf_counter() - t1
    _, _, done, _ = env.step(plan["actions"])
    carry["nominal"] = None if done else plan["nominal"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,8,64,512")
    ap.add_argument("--paths", default="1024,4096,16384,65536")
    ap.add_argument("--iterations", default="1,2,4")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10, help="calls inside one timed window")
    ap.add_argument("--big", type=float, default=2e8, help="candidate steps per plan above which a window has --big-reps calls")
    ap.add_argument("--big-reps", type=int, default=2)
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
        nom = torch.empty((n, H, 4), dtype=torch.float32, device=env.device)
        score = torch.empty((n,), dtype=torch.float64, device=env.device)
        index = torch.empty((n,), dtype=torch.int32, device=env.device)
        p = lambda t: C.c_void_p(t.data_ptr())                # noqa: E731
        env._use_current_stream()
        for paths in [int(x) for x in args.paths.split(",")]:
            auto = max(qa.plan_splits(env, paths), 2 if paths > 4096 else 1)
            for iters in [int(x) for x in args.iterations.split(",")]:
                one = [("base", None), ("S=1", 1)] if paths <= 4096 else []
                configs = one + [("auto", 0)] + [("S=%d" % s, s) for s in SWEEP if s <= min(paths, 1024)] + [("floor", "floor")]
                steps = n * paths * H * iters
                reps = args.reps if steps <= args.big else args.big_reps

                def plan(s):
                    if s == "floor":
                        for _ in range(iters):
                            qa._lib.check(lib.qs_shooting_plan_split(env._h, H, paths, 0, 0, p(act), p(score), p(index), None, None), "floor")
                    elif s is None:
                        qa._lib.check(lib.qs_mppi_plan(env._h, H, paths, iters, 0, LAM, SIGMA, 0, None, None, p(act), p(nom), p(score),
                                                       None, None, None), "base")
                    else:
                        qa._lib.check(lib.qs_mppi_plan_split(env._h, H, paths, iters, 0, LAM, SIGMA, 0, s, None, None, p(act), p(nom),
                                                             p(score), None, None, None), "split")

                want = None
                for name, s in configs[:-1]:                  # the plans agree to one rounding per update before anything is timed
                    plan(s)
                    torch.cuda.synchronize()
                    want = nom.clone() if want is None else want
                    assert float((nom - want).abs().max()) <= iters * 1e-3, (n, paths, iters, name)
                rows = plan_timing.alternating_rounds(torch, env, configs, plan, args.rounds, reps,
                                                      dict(envs=n, paths=paths, iterations=iters, horizon=H, auto_splits=auto, reps=reps,
                                                           candidate_steps=steps))
                results += rows
                cell = dict(envs=n, paths=paths, iterations=iters, horizon=H, auto_splits=auto, rounds=len(rows), reps=reps,
                            **plan_timing.ranges(rows, [k for k in rows[0] if k.endswith("_ms")]))
                cell["floor_over_auto"] = plan_timing.ratio_range(rows, "floor_ms", "auto_ms")
                if paths <= 4096:
                    spread = max(cell["S=1_ms"][1] - cell["S=1_ms"][0], cell["auto_ms"][1] - cell["auto_ms"][0])
                    cell["spread_ms"] = spread
                    cell["auto_faster_than_base_in_every_round"] = all(r["auto_ms"] < r["base_ms"] for r in rows)
                    cell["auto_not_slower_than_one_part_beyond_spread"] = cell["auto_ms"][1] <= cell["S=1_ms"][1] + spread
                    cell["base_over_auto"] = plan_timing.ratio_range(rows, "base_ms", "auto_ms")
                summary.append(cell)
                print(json.dumps(dict(summary=cell)), flush=True)
        env.close()
    host = plan_timing.host_path(qa, args.rounds, plan_and_step, paths=200, horizon=20, mppi_iterations=2) if args.host else None
    if host:
        print(json.dumps(dict(host=host)), flush=True)
    plan_timing.write_out(args.out, torch, cus=torch.cuda.get_device_properties(0).multi_processor_count, reps=args.reps, big=args.big,
                          big_reps=args.big_reps, summary=summary, host=host, rounds=results)

if __name__ == "__main__":
    main()
