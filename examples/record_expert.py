#!/usr/bin/env python3
"""Record the PID expert on N docking-v1 envs (every env its own jittered start) into an SB2 ExpertDataset archive -- the
__main__ of run_expert_record.py for N envs at once -- and evaluate the expert in one launch.

    python examples/record_expert.py [--envs 4096] [--episodes 1] [--out expert_docking.npz]

The archive holds every env's first --episodes complete episodes, env by env (keys actions, obs, rewards, episode_returns,
episode_starts), as run_pretrained_ppo2_docking.py:50-69 and run_docking_gail.py:51 load it."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import quadsim_amd as qa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=1, help="complete episodes per env")
    ap.add_argument("--out", default="expert_docking.npz")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    env = qa.VecDockingEnv("docking-v1", num_envs=args.envs, seed=args.seed)
    env.reset()
    res = qa.PIDExpert(env).evaluate(args.episodes)          # read-only: the recording below starts from the same reset
    print("expert on %d docking-v1 envs x %d episodes: mean return %.4f +- %.4f, mean length %.1f, docked %.3f, over limit %.3f"
          % (args.envs, args.episodes, res.mean_return(), res.std_return(), res.mean_length(), res.docked_fraction(),
             res.overlimit_fraction()))
    t0 = time.perf_counter()
    data = qa.record_expert_dataset(env, n_episodes=args.episodes, save_path=args.out)
    print("recorded %d transitions, %d episodes (mean return %.4f) in %.2f s -> %s"
          % (len(data["rewards"]), len(data["episode_returns"]), float(data["episode_returns"].mean()),
             time.perf_counter() - t0, args.out))
    env.close()


if __name__ == "__main__":
    main()
