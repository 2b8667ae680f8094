#!/usr/bin/env python3
"""Random-shooting MPC at N docking-v0 envs (default 4096), horizon 20, paths 200 and 1024, on one MI355X:

  a  plan        qs_shooting_plan (one launch: candidates on lanes, the target trajectory shared, (score, index) reduced), both
                 objectives
  b  composed    the same work from the calls that existed before it: a handle of N x paths envs with the replicated state,
                 qs_rollout(T = horizon) over pre-staged actions (every step's obs / reward / done written), torch's masked
                 float64 sum and argmax.  Timed twice: the kernels alone (roll-out + reduction), and with the replication
                 (get_state -> repeat_interleave -> set_state) in front
  c  qs_rollout  the roll-out of (b) alone: N x paths x horizon full two-drone env steps, the ceiling such a step sets

(a) and (b) alternate for --rounds rounds after a warm-up round; every figure is reported per round and as a range.  Timed
with qs_timer_start / qs_timer_stop on the handles' stream (= torch's current stream, so the torch reduction is inside the
window); the replication, which ends in a host synchronisation, by wall clock.  One JSON line per (paths, round) on stdout,
everything in --out.  The merge condition of the planner: (a) no slower than (b)'s kernels alone in every round."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plan_timing  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--paths", default="200,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls inside one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa

    n, H = args.envs, args.horizon
    results = []
    for paths in [int(p) for p in args.paths.split(",")]:
        m = n * paths
        env = plan_timing.stepped_env(qa, n)
        big = qa.VecDockingEnv("docking-v0", num_envs=m, seed=6)    # qs_rollout needs auto_reset; steps after a done are masked
        acts = big.random_actions(H, step0=0)
        out = tuple(torch.empty(s, dtype=d, device=env.device) for s, d in
                    (((H, m, 12), torch.float32), ((H, m), torch.float32), ((H, m), torch.uint8)))

        def replicate():
            st = env.get_state(as_numpy=False)
            big.set_state(**{k: v.repeat_interleave(paths, dim=0) for k, v in st.items()})     # ends in a synchronisation

        def composed():
            _, rew, done, _ = big.rollout(acts, out=out + (None,), want_flags=False)
            d = done.to(torch.int32)
            alive = (torch.cumsum(d, 0) - d) == 0
            score = (rew.double() * alive).sum(0).view(n, paths)
            best = score.argmax(1)
            return acts[0].view(n, paths, 4)[torch.arange(n, device=best.device), best], score

        window = lambda env_, fn: plan_timing.window(env_, fn, args.reps)    # noqa: E731

        steps = m * H
        for rnd in range(args.rounds + 1):                   # round 0 warms every shape up and is not reported
            row = dict(envs=n, paths=paths, horizon=H, round=rnd, candidate_steps=steps)
            for objective in ("reward", "position"):
                row["a_%s_ms" % objective], plan = window(env, lambda: env.shooting_plan(H, paths, objective))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            replicate()
            torch.cuda.synchronize()
            row["b_replicate_ms"] = (time.perf_counter() - t0) * 1e3
            row["b_kernels_ms"], _ = window(big, composed)
            replicate()
            row["c_rollout_ms"], _ = window(big, lambda: big.rollout(acts, out=out + (None,), want_flags=False))
            row["b_total_ms"] = row["b_replicate_ms"] + row["b_kernels_ms"]
            for key in ("a_reward_ms", "a_position_ms", "b_kernels_ms", "c_rollout_ms"):
                row[key.replace("_ms", "_g_steps_per_s")] = steps / row[key] / 1e6
            row["b_kernels_over_a_reward"] = row["b_kernels_ms"] / row["a_reward_ms"]
            row["a_reward_rate_over_c"] = row["c_rollout_ms"] / row["a_reward_ms"]
            if rnd:
                results.append(row)
                print(json.dumps(row), flush=True)
        env.close(); big.close()
        del out, acts
        torch.cuda.empty_cache()
    summary = []
    for paths in sorted({r["paths"] for r in results}):
        rows = [r for r in results if r["paths"] == paths]
        summary.append(dict(paths=paths, rounds=len(rows), **plan_timing.ranges(rows, [k for k in rows[0] if k.endswith(("_ms", "_per_s", "_reward", "_c"))]),
                            a_no_slower_than_b_kernels_in_every_round=all(max(r["a_reward_ms"], r["a_position_ms"]) <= r["b_kernels_ms"] for r in rows)))
        print(json.dumps(dict(summary=summary[-1])), flush=True)
    plan_timing.write_out(args.out, torch, rounds=results, summary=summary)

if __name__ == "__main__":
    main()
