#!/usr/bin/env python3
"""Sampling MPC (random shooting or MPPI) on ONE gym-style env: the loop of model_train (MPC-based_RL.py:213-241), ``a = mpc.choose_action();
env.step(a)``, written against the single-env shim -- numpy in, numpy out -- with the exact simulator as the planner's model.

    python examples/mpc_single.py [--planner shooting|mppi] [--steps 300] [--horizon 20] [--paths 200] [--iterations 2]
                                  [--objective reward|position] [--splits auto]

`DockingEnv.shooting_plan` and `DockingEnv.mppi_plan` spread the env's candidates over several workgroups where that pays
(qs_shooting_plan_split, qs_mppi_plan_split; with few paths the automatic choice is one workgroup).  The MPPI loop carries the
nominal sequence from plan to plan (shift=True) and starts from zeros again when the episode is done.  One episode from a reset, or --steps steps at most; prints the return,
whether the episode docked, and the wall time per plan beside the 20 ms control period of dt = 0.02."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import quadsim_amd as qa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--planner", default="shooting", choices=("shooting", "mppi"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--paths", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=2, help="MPPI refinement rounds per plan")
    ap.add_argument("--objective", default="reward", choices=("reward", "position"))
    ap.add_argument("--splits", default="auto", help='"auto" or the number of workgroups the candidates are spread over')
    args = ap.parse_args()
    splits = args.splits if args.splits == "auto" else int(args.splits)
    env = qa.DockingEnv()
    env.reset()
    nominal = None                                            # MPPI: the warm start, carried from plan to plan

    def plan_once():
        if args.planner == "shooting":
            return env.shooting_plan(args.horizon, args.paths, args.objective, splits)
        return env.mppi_plan(args.horizon, args.paths, args.iterations, args.objective, nominal=nominal, shift=nominal is not None,
                             splits=splits)
    plan_once()                                               # the first call allocates; not timed
    episode_reward, docked, plan_s = 0.0, False, 0.0
    for step in range(args.steps):
        t0 = time.perf_counter()
        plan = plan_once()
        plan_s += time.perf_counter() - t0
        _, reward, done, info = env.step(plan["actions"])
        nominal = None if done else plan.get("nominal")      # a new episode starts from a zero nominal
        episode_reward += reward
        docked = docked or info["flag_docking"]
        if done:
            break
    parts = splits if splits != "auto" else max(qa.plan_splits(env, args.paths), 2 if args.planner == "mppi" and args.paths > 4096 else 1)
    print("docking-v0, %s, horizon %d, %d paths over %d workgroup(s), objective %s: %d steps, episode %s, return %.3f, docked: %s; "
          "%.3f ms per plan (control period 20 ms)"
          % (args.planner if args.planner == "shooting" else "mppi x %d iterations" % args.iterations, args.horizon, args.paths, parts,
             args.objective, step + 1, "done" if done else "cut", episode_reward, docked, plan_s / (step + 1) * 1e3))
    env.close()


if __name__ == "__main__":
    main()
