#!/usr/bin/env python3
"""Random-shooting MPC on ONE gym-style env: the loop of model_train (MPC-based_RL.py:213-241), ``a = mpc.choose_action();
env.step(a)``, written against the single-env shim -- numpy in, numpy out -- with the exact simulator as the planner's model.

    python examples/mpc_single.py [--steps 300] [--horizon 20] [--paths 200] [--objective reward|position] [--splits auto]

`DockingEnv.shooting_plan` spreads the env's candidates over several workgroups where that pays (qs_shooting_plan_split; with
few paths the automatic choice is one workgroup).  One episode from a reset, or --steps steps at most; prints the return,
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
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--paths", type=int, default=200)
    ap.add_argument("--objective", default="reward", choices=("reward", "position"))
    ap.add_argument("--splits", default="auto", help='"auto" or the number of workgroups the candidates are spread over')
    args = ap.parse_args()
    splits = args.splits if args.splits == "auto" else int(args.splits)
    env = qa.DockingEnv()
    env.reset()
    env.shooting_plan(args.horizon, args.paths, args.objective, splits)     # the first call allocates; not timed
    episode_reward, docked, plan_s = 0.0, False, 0.0
    for step in range(args.steps):
        t0 = time.perf_counter()
        plan = env.shooting_plan(args.horizon, args.paths, args.objective, splits)
        plan_s += time.perf_counter() - t0
        _, reward, done, info = env.step(plan["actions"])
        episode_reward += reward
        docked = docked or info["flag_docking"]
        if done:
            break
    print("docking-v0, horizon %d, %d paths over %d workgroup(s), objective %s: %d steps, episode %s, return %.3f, docked: %s; "
          "%.3f ms per plan (control period 20 ms)"
          % (args.horizon, args.paths, qa.plan_splits(env, args.paths) if splits == "auto" else splits, args.objective, step + 1,
             "done" if done else "cut", episode_reward, docked, plan_s / (step + 1) * 1e3))
    env.close()


if __name__ == "__main__":
    main()
