#!/usr/bin/env python3
"""Evaluate the two shipped checkpoints over many randomised starts, one launch per (checkpoint, env): the EvalCallback /
evaluate_policy step of run_docking_ppo2.py:75-83 and the deterministic replays of run_trained_docking_ppo2.py (docking-v1)
and run_trained_moving_docking_ppo2.py (docking-v2), for N envs at once.

    python examples/evaluate_policy.py [--envs 65536] [--episodes 1] [--precision f32|bf16x3]

docking-v0 / v2 start from rocRAND-drawn chaser states (the C3 ranges, plus per-episode mass / inertia with --randomise 2);
docking-v1 resets to its stored, construction-time jittered initial states."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CHECKPOINTS = {"best_model_v0 (shared trunk)": os.path.join(GOLDEN, "policy_best_model_v0.npz"),
               "ppo2_docking_621_h_30M (towers)": os.path.join(GOLDEN, "sb2_ppo2_docking_621_h_30M.zip")}


def load(path):
    return qa.MlpPolicy.from_npz(path) if path.endswith(".npz") else qa.MlpPolicy.from_sb2_zip(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--episodes", type=int, default=1, help="episodes per env")
    ap.add_argument("--precision", default="f32", choices=("f32", "bf16x3"))
    ap.add_argument("--randomise", type=int, default=1, choices=(1, 2))
    args = ap.parse_args()
    for name, path in CHECKPOINTS.items():
        pol = load(path)
        for env_id in ("docking-v0", "docking-v1", "docking-v2"):
            rnd = 0 if env_id == "docking-v1" else args.randomise
            kw = dict(num_envs=args.envs, randomise=rnd, seed=1)
            if rnd:
                kw.update(init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2))
            env = qa.VecDockingEnv(env_id, **kw)
            env.reset()
            qa.evaluate_policy_episodes(pol, env, args.episodes, precision=args.precision)      # warm-up (weights, code object)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = qa.evaluate_policy_episodes(pol, env, args.episodes, precision=args.precision)
            torch.cuda.synchronize()
            sec = time.perf_counter() - t0
            steps = int(res.lengths.sum().item())
            print("%-32s %s: %d episodes, return %.3f +- %.3f, length %.1f, docked %.1f %%, over limit %.1f %%, %.2f G env-steps/s"
                  % (name, env_id, res.num_episodes(), res.mean_return(), res.std_return(), res.mean_length(),
                     100 * res.docked_fraction(), 100 * res.overlimit_fraction(), steps / sec / 1e9))
            env.close()


if __name__ == "__main__":
    main()
