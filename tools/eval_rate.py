#!/usr/bin/env python3
"""Deterministic evaluation of one episode per env at 65 536 docking-v0 envs (rocRAND starts) on one MI355X, three ways:

  evaluate   quadsim_amd.evaluate_policy_episodes (qs_policy_evaluate / _fast: one launch, episode records only)
  rollout    fused_policy_rollout(T = 600) + qs_episode_stats (EpisodeTracker): every step's obs / reward / done / flags stored
  loop       policy.predict_hip(env, obs) -> env.step(a) for 600 steps, returns / lengths accumulated with torch ops

for both actor precisions.  Every variant starts from the same freshly reset handle (the evaluation leaves it untouched; the
other two are run on a twin reset the same way) and is timed as host wall clock around a synchronised call, the median of
--reps after one warm-up.  Env-steps counted are those actually run: `evaluate` steps a wave until its slowest lane has
finished, so it runs sum over tiles of 64 x (longest episode of the tile) env-steps (`env_steps_run`), of which
sum(lengths) (`env_steps_useful`) belong to recorded episodes; the other two run 600 x N.  One JSON line per
(variant, precision) on stdout, and all of them in --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precisions", default="f32,bf16x3")
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default="evaluate,rollout,loop", help="comma list of evaluate, rollout, loop")
    args = ap.parse_args()
    only = args.only.split(",")
    import numpy as np
    import torch
    import quadsim_amd as qa
    from quadsim_amd.rollout_buffer import EpisodeTracker

    n, T = args.envs, 600
    pol = qa.MlpPolicy.from_npz(os.path.join(ROOT, "tests", "golden", "policy_best_model_v0.npz"))
    kw = dict(num_envs=n, randomise=1, seed=11, init_range=qa.C3_INIT_RANGE)

    def fresh():
        env = qa.VecDockingEnv("docking-v0", **kw)
        env.reset()
        torch.cuda.synchronize()
        return env

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), ts, out

    lines = []
    for prec in args.precisions.split(","):
        # ---- the evaluation kernel: read-only, so every repetition sees the same starts
        if "evaluate" in only:
            env = fresh()
            sec, ts, res = timed(lambda: qa.evaluate_policy_episodes(pol, env, 1, precision=prec), args.reps)
            h = res.numpy()
            ln = h["lengths"][0].astype(np.int64)
            pad = (-n) % 64
            run = int((np.concatenate([ln, np.zeros(pad, np.int64)]).reshape(-1, 64).max(1) * 64).sum())
            useful = int(ln.sum())
            lines.append(dict(variant="evaluate", precision=prec, envs=n, seconds=sec, all_seconds=ts, env_steps_run=run,
                              env_steps_useful=useful, g_env_steps_per_s=run / sec / 1e9, g_useful_env_steps_per_s=useful / sec / 1e9,
                              mean_return=res.mean_return(), std_return=res.std_return(), mean_length=res.mean_length(),
                              docked_fraction=res.docked_fraction(), overlimit_fraction=res.overlimit_fraction()))
            print(json.dumps(lines[-1]), flush=True)
            env.close()
        # ---- fused roll-out of T steps + device episode accounting (state advances: a fresh handle per repetition)
        if "rollout" in only:
            envs = [fresh() for _ in range(args.reps + 1)]
            it = iter(envs)

            def rollout():
                env = next(it)
                obs, rew, done, flags, _ = qa.fused_policy_rollout(env, pol, T, want_actions=False, precision=prec)
                before = torch.cat([torch.zeros_like(done[:1]), done[:-1]])
                tr = EpisodeTracker(env).update(rew, before, done[-1])
                return tr, flags
            sec, ts, (tr, flags) = timed(rollout, args.reps)
            lines.append(dict(variant="rollout", precision=prec, envs=n, seconds=sec, all_seconds=ts, env_steps_run=T * n,
                              g_env_steps_per_s=T * n / sec / 1e9))
            print(json.dumps(lines[-1]), flush=True)
            for e in envs:
                e.close()
        # ---- per-step loop: two launches per step, episode bookkeeping in torch
        if "loop" in only:
            envs = [fresh() for _ in range(2)]
            it = iter(envs)

            def loop():
                env = next(it)
                obs = env.reset()
                ret = torch.zeros(n, dtype=torch.float64, device=env.device)
                length = torch.zeros(n, dtype=torch.int32, device=env.device)
                live = torch.ones(n, dtype=torch.bool, device=env.device)
                for _ in range(T):
                    a = pol.predict_hip(env, obs, prec)
                    obs, r, d, _ = env.step(a)
                    ret += torch.where(live, r.double(), 0.0)
                    length += live.int()
                    live &= ~d
                return ret, length
            sec, ts, _ = timed(loop, 1)
            lines.append(dict(variant="loop", precision=prec, envs=n, seconds=sec, all_seconds=ts, env_steps_run=T * n,
                              g_env_steps_per_s=T * n / sec / 1e9))
            print(json.dumps(lines[-1]), flush=True)
            for e in envs:
                e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), results=lines), f, indent=1)


if __name__ == "__main__":
    main()
