#!/usr/bin/env python3
"""Random-shooting MPC in closed loop: the loop of model_train (MPC-based_RL.py:213-241) without the dynamics net -- the planner
(Mpc_Controller, :170-210: 200 random action sequences of horizon 20, the first action of the best one) rolls its candidates
through the exact simulator, one launch per step for all envs (qs_shooting_plan).

    python examples/mpc_shooting.py [--envs 64] [--steps 600] [--horizon 20] [--paths 200] [--objective reward|position]

Every env runs one episode from a reset (or --steps steps at most); the mean episode return is printed, as the script prints
episode_reward.  Nobody has measured what random shooting achieves on this task: the figure is a baseline, not a target."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--paths", type=int, default=200)
    ap.add_argument("--objective", default="reward", choices=("reward", "position"))
    args = ap.parse_args()
    env = qa.VecDockingEnv("docking-v0", num_envs=args.envs, seed=1)
    mpc = qa.ShootingMPC(env, args.horizon, args.paths, args.objective)
    env.reset()
    ret = torch.zeros(args.envs, dtype=torch.float64, device=env.device)
    running = torch.ones(args.envs, dtype=torch.bool, device=env.device)
    length = torch.zeros(args.envs, dtype=torch.int64, device=env.device)
    t0 = time.perf_counter()
    for step in range(args.steps):
        _, r, d, _ = env.step(mpc.act())
        ret += torch.where(running, r.double(), torch.zeros_like(ret))
        length += running
        running &= ~d                                        # the env resets itself; this script keeps its first episode
        if not bool(running.any()):
            break
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    done = ~running
    print("%d envs, horizon %d, %d paths, objective %s: %d of %d episodes finished within %d steps; mean episode return %.3f, "
          "mean length %.1f; %.1f plans/s (%.2f G candidate-steps/s)"
          % (args.envs, args.horizon, args.paths, args.objective, int(done.sum()), args.envs, step + 1, float(ret.mean()),
             float(length.double().mean()), (step + 1) * args.envs / sec, (step + 1) * args.envs * args.paths * args.horizon / sec / 1e9))
    env.close()


if __name__ == "__main__":
    main()
