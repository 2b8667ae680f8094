#!/usr/bin/env python3
"""MPPI in closed loop beside random shooting at the same candidate budget: N docking-v0 envs fly one episode each with
quadsim_amd.MPPI (`paths` Gaussian candidates x `iterations` refinement rounds per plan, the nominal sequence warm-started from
the previous plan; one launch per plan for all envs, qs_mppi_plan) and with quadsim_amd.ShootingMPC at paths x iterations
uniform candidates (qs_shooting_plan).

    python examples/mpc_mppi.py [--envs 64] [--steps 600] [--horizon 20] [--paths 200] [--iterations 2] [--lam L] [--sigma S]

For each controller: the mean return of every env's first episode and the fraction of envs that reported QS_FLAG_DOCKED in it.
The defaults of lam and sigma are tuned on one setting only (profiles/mppi/README.md); the figures are recorded results, not
targets."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402
from quadsim_amd import mpc  # noqa: E402


def fly(name, env, controller, steps):
    n = env.num_envs
    env.reset()
    ret = torch.zeros(n, dtype=torch.float64, device=env.device)
    running = torch.ones(n, dtype=torch.bool, device=env.device)
    docked = torch.zeros(n, dtype=torch.bool, device=env.device)
    t0 = time.perf_counter()
    for step in range(steps):
        _, r, d, _ = env.step(controller.act())
        ret += torch.where(running, r.double(), torch.zeros_like(ret))
        docked |= running & ((torch.as_tensor(env.last_flags) & qa._lib.FLAG_DOCKED) != 0)
        if isinstance(controller, qa.MPPI):
            controller.nominal.masked_fill_(d.bool().view(-1, 1, 1), 0.0)    # what MPPI.run does after each step
        running &= ~d                                        # the env resets itself; this script keeps its first episode
        if not bool(running.any()):
            break
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    print("%-9s %d envs: %d of %d episodes finished within %d steps; mean episode return %.3f, docked in %.1f %% of the episodes; "
          "%.1f plans/s" % (name, n, int((~running).sum()), n, step + 1, float(ret.mean()), 100.0 * float(docked.double().mean()),
                            (step + 1) * n / sec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--paths", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--lam", type=float, default=mpc.MPPI_DEFAULT_LAMBDA)
    ap.add_argument("--sigma", type=float, default=mpc.MPPI_DEFAULT_SIGMA)
    ap.add_argument("--objective", default="reward", choices=("reward", "position"))
    args = ap.parse_args()
    print("horizon %d, objective %s; MPPI: %d paths x %d iterations, lam %g, sigma %g; shooting: %d paths"
          % (args.horizon, args.objective, args.paths, args.iterations, args.lam, args.sigma, args.paths * args.iterations))
    env = qa.VecDockingEnv("docking-v0", num_envs=args.envs, seed=1)
    fly("MPPI", env, qa.MPPI(env, args.horizon, args.paths, args.iterations, args.objective, args.lam, args.sigma), args.steps)
    fly("shooting", env, qa.ShootingMPC(env, args.horizon, args.paths * args.iterations, args.objective), args.steps)
    env.close()


if __name__ == "__main__":
    main()
