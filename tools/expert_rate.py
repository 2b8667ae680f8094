#!/usr/bin/env python3
"""The PID expert in the loop at 65 536 docking-v1 envs (every env its own jittered start), T = 600 steps, on one MI355X:

  a  loop            a = expert.act(); env.step(a) on a VecDockingEnv(copy=False): two launches per step, nothing kept
  b  record_loop     record_expert_dataset(n_steps=T, fused=False) end to end: (a) + four clones per step + host loops
  c  rollout         qs_expert_rollout alone (PIDExpert.rollout: one launch, every step's obs / action / reward / done stored)
  d  record_fused    record_expert_dataset(n_steps=T, fused=True) end to end: (c) env-major + device bookkeeping + one copy out
  e  evaluate        qs_expert_evaluate, K = 1 (episode records only)
  r  qs_rollout      the same env code with pre-staged actions at the same T, for orientation

(a) and (b) are what the package did before the fused kernels; the ratios that matter are c : a, d : b and c : r (what the
in-loop controller costs).  Every variant runs on its own freshly reset handle(s), once warm and then --reps times, timed
with HIP events around the call (the end-to-end variants block the host, so the events span the host work too) and by wall
clock; the median is reported.  (e) runs a wave until its slowest lane has finished: `env_steps_run` counts those steps,
`env_steps_useful` the recorded episodes' own.  One JSON line per variant on stdout, all of them in --out."""
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
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-reps", type=int, default=2, help="repetitions of the end-to-end recordings (b), (d) and of the loop (a)")
    ap.add_argument("--only", default="a,b,c,d,e,r")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    only = args.only.split(",")
    import numpy as np
    import torch
    import quadsim_amd as qa

    n, T = args.envs, args.steps

    def fresh(**kw):
        env = qa.VecDockingEnv("docking-v1", num_envs=n, seed=11, **kw)
        env.reset()
        torch.cuda.synchronize()
        return env

    def timed(fn, reps):
        """fn(i) for i = 0 (warm-up), 1..reps -> (median ms by HIP events, median ms by wall clock, all event ms, last result)"""
        ev, wall, out = [], [], None
        for i in range(reps + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            out = fn(i)
            e1.record()
            e1.synchronize()
            if i:
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(e0.elapsed_time(e1))
        return float(np.median(ev)), float(np.median(wall)), ev, out

    lines = []

    def report(variant, what, ms, wall_ms, all_ms, steps=None, **extra):
        steps = T * n if steps is None else steps
        lines.append(dict(variant=variant, what=what, envs=n, T=T, ms=ms, wall_ms=wall_ms, all_ms=all_ms, us_per_step=ms * 1e3 / T,
                          env_steps_run=steps, g_env_steps_per_s=steps / ms / 1e6, **extra))
        print(json.dumps(lines[-1]), flush=True)

    if "a" in only:
        envs = [fresh(copy=False) for _ in range(args.slow_reps + 1)]

        def loop(i):
            env = envs[i]
            ex = qa.PIDExpert(env)
            for _ in range(T):
                env.step(ex.act())
        report("a", "loop", *timed(loop, args.slow_reps)[:3])
        for e in envs:
            e.close()
    if "b" in only:
        envs = [fresh() for _ in range(args.slow_reps + 1)]
        report("b", "record_loop", *timed(lambda i: qa.record_expert_dataset(envs[i], n_steps=T, fused=False), args.slow_reps)[:3])
        for e in envs:
            e.close()
    if "c" in only:
        envs = [fresh() for _ in range(args.reps + 1)]
        exs = [qa.PIDExpert(e) for e in envs]
        ms, wall, all_ms, ro = timed(lambda i: exs[i].rollout(T), args.reps)
        report("c", "rollout", ms, wall, all_ms, resets=int(ro["dones"].sum().item()))
        del ro
        for e in envs:
            e.close()
    if "d" in only:
        envs = [fresh() for _ in range(args.slow_reps + 1)]
        ms, wall, all_ms, data = timed(lambda i: qa.record_expert_dataset(envs[i], n_steps=T, fused=True), args.slow_reps)
        report("d", "record_fused", ms, wall, all_ms, episodes=int(len(data["episode_returns"])))
        del data
        for e in envs:
            e.close()
    if "e" in only:
        env = fresh()                                   # read-only: every repetition sees the same starts
        ex = qa.PIDExpert(env)
        ms, wall, all_ms, res = timed(lambda i: ex.evaluate(1), args.reps)
        ln = res.numpy()["lengths"][0].astype(np.int64)
        run = int((np.concatenate([ln, np.zeros((-n) % 64, np.int64)]).reshape(-1, 64).max(1) * 64).sum())
        report("e", "evaluate", ms, wall, all_ms, steps=run, env_steps_useful=int(ln.sum()), mean_return=res.mean_return(),
               mean_length=res.mean_length(), docked_fraction=res.docked_fraction(), overlimit_fraction=res.overlimit_fraction())
        env.close()
    if "r" in only:
        envs = [fresh() for _ in range(args.reps + 1)]
        acts = envs[0].random_actions(T)
        torch.cuda.synchronize()
        report("r", "qs_rollout", *timed(lambda i: envs[i].rollout(acts, T), args.reps)[:3])
        for e in envs:
            e.close()
    by = {x["variant"]: x["ms"] for x in lines}
    ratios = {k: by[p] / by[q] for k, (p, q) in dict(a_over_c=("a", "c"), b_over_d=("b", "d"), c_over_r=("c", "r")).items()
              if p in by and q in by}
    print(json.dumps(dict(ratios=ratios)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), results=lines, ratios=ratios), f, indent=1)


if __name__ == "__main__":
    main()
