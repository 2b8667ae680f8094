#!/usr/bin/env python3
"""Closed-loop return of MPPI over a small (lam, sigma) grid: N docking-v0 envs (default 4096), horizon 20, 200 paths x 2
iterations, objective "reward", --steps env steps (default 600: one episode), beside ShootingMPC at the same candidate
budget (400 paths).  The source of the defaults in quadsim_amd/mpc.py; one JSON line per cell, everything in --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fly(qa, torch, make_controller, n, steps, seed):
    env = qa.VecDockingEnv("docking-v0", num_envs=n, randomise=1, seed=seed, init_range=qa.C3_INIT_RANGE)
    env.reset()
    t0 = time.perf_counter()
    rew, done = make_controller(env).run(steps)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the return of each env's FIRST episode (up to its first done), as an evaluation would count it
    d = done.to(torch.int32)
    first = (torch.cumsum(d, 0) - d) == 0
    ret = (rew.double() * first).sum(0)
    out = dict(mean_return=float(ret.mean()), mean_step_reward=float(rew.double().mean()), episodes_ended=int(done.sum()),
               wall_s=wall)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--lams", default="0.05,0.2,0.8")
    ap.add_argument("--sigmas", default="0.25,0.5,1.0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa
    rows = []
    base = fly(qa, torch, lambda e: qa.ShootingMPC(e, 20, 400, "reward"), args.envs, args.steps, 5)
    rows.append(dict(controller="shooting", paths=400, **base))
    print(json.dumps(rows[-1]), flush=True)
    for lam in [float(x) for x in args.lams.split(",")]:
        for sigma in [float(x) for x in args.sigmas.split(",")]:
            r = fly(qa, torch, lambda e: qa.MPPI(e, 20, 200, 2, "reward", lam, sigma), args.envs, args.steps, 5)
            rows.append(dict(controller="mppi", paths=200, iterations=2, lam=lam, sigma=sigma, **r))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), date=time.strftime("%Y-%m-%d"), envs=args.envs, steps=args.steps,
                           rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
