#!/usr/bin/env python3
"""MPC through a LEARNED dynamics net, trained while it controls: the loop of model_train (MPC-based_RL.py:213-259) on N envs.

    python examples/mpc_learned.py [--envs 16] [--episodes 5] [--max-steps 600] [--horizon 20] [--paths 200]
                                   [--planner {shooting,mppi}] [--iterations 2] [--lam L] [--sigma S] [--fit {torch,hip}]

Per step: plan with the learned net (--planner shooting: learned_shooting_plan, every candidate of every env in one launch;
--planner mppi: learned_mppi_plan, `iterations` rounds of `paths` Gaussian candidates around a warm-started nominal, whose
lam / sigma defaults are mpc.mppi_plan's and were not tuned for a learned model), env.step, append
(obs, act, delta) to a device-side buffer.  After each episode (the auto-resetting envs each contribute their first episode):
100 Adam steps of batch 128 at lr 1e-4 on the normalised delta (train_dynamic, :120-128) in plain torch, the normalisers
refreshed from the buffer, the net re-packed for the planner.  Prints the mean episode return after every episode, as the
script prints episode_reward.  The fit is not part of the library: DynamicsNet.predict_delta is the formula, torch trains it.
--fit hip runs the same 100 steps in one launch instead (DynamicsNet.fit, libquadsim_dynfit.so: tf.train.AdamOptimizer's
formula, keyed batch draws, a fixed summation order): two runs with the same arguments print the same lines.  The default
stays torch."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402


def train_dynamic(net, opt, buf_x, buf_d, size, iters=100, batch=128):
    """Dynamic_Net.train_dynamic: `iters` Adam steps on random batches of the buffer -> the last loss"""
    loss = torch.zeros(())
    for _ in range(iters):
        idx = torch.randint(0, size, (batch,), device=buf_x.device)
        x, d = buf_x[idx], buf_d[idx]
        target = (d - net.out_mean) / (net.out_std + 1.0e-6)
        loss = torch.mean((net.predict_delta(x[:, :12], x[:, 12:]) - target) ** 2)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    return float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--max-steps", type=int, default=600)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--paths", type=int, default=200)
    ap.add_argument("--capacity", type=int, default=1 << 18)
    ap.add_argument("--planner", choices=("shooting", "mppi"), default="shooting")
    ap.add_argument("--iterations", type=int, default=2, help="mppi: refinement rounds per plan")
    ap.add_argument("--lam", type=float, default=qa.mpc.MPPI_DEFAULT_LAMBDA, help="mppi: temperature of the weights")
    ap.add_argument("--sigma", type=float, default=qa.mpc.MPPI_DEFAULT_SIGMA, help="mppi: standard deviation of the candidates")
    ap.add_argument("--fit", choices=("torch", "hip"), default="torch", help="the fit after each episode: the torch loop or DynamicsNet.fit")
    args = ap.parse_args()
    n = args.envs
    env = qa.VecDockingEnv("docking-v0", num_envs=n, seed=1)
    dev = env.device
    net = qa.DynamicsNet(200, 100, device=dev)
    if args.fit == "torch":
        for p in net.parameters():
            p.requires_grad_(True)
        opt = torch.optim.Adam(net.parameters(), lr=1.0e-4)
    if args.planner == "mppi":
        mpc = qa.LearnedMPPI(env, net, args.horizon, args.paths, args.iterations, args.lam, args.sigma)
    else:
        mpc = qa.LearnedShootingMPC(env, net, args.horizon, args.paths)
    buf_x = torch.zeros(args.capacity, 16, device=dev)
    buf_d = torch.zeros(args.capacity, 12, device=dev)
    size = head = 0
    for episode in range(args.episodes):
        obs = env.reset()
        if args.planner == "mppi":
            mpc.reset()                                      # a new episode starts from a cold nominal
        ret = torch.zeros(n, dtype=torch.float64, device=dev)
        running = torch.ones(n, dtype=torch.bool, device=dev)
        for step in range(args.max_steps):
            act = mpc.act()
            nxt, r, d, _ = env.step(act)
            if args.planner == "mppi":
                mpc.nominal.masked_fill_(d.view(-1, 1, 1), 0.0)
            # the observation after a done step is the reset one: that transition is not a sample of the dynamics
            rows = torch.nonzero(running & ~d).view(-1)
            m = min(int(rows.numel()), args.capacity - head)
            buf_x[head:head + m] = torch.cat([obs, act], dim=1)[rows[:m]]
            buf_d[head:head + m] = (nxt - obs)[rows[:m]]
            head = (head + m) % args.capacity
            size = min(size + m, args.capacity)
            ret += torch.where(running, r.double(), torch.zeros_like(ret))
            running &= ~d
            obs = nxt
            if not bool(running.any()):
                break
        net.set_normalisers(in_mean=buf_x[:size].mean(0), in_std=buf_x[:size].std(0), out_mean=buf_d[:size].mean(0),
                            out_std=buf_d[:size].std(0))
        if args.fit == "hip":
            loss = float(net.fit(buf_x, buf_d, size, iters=100, batch=128, lr=1.0e-4, seed=1)["loss"][-1])
        else:
            loss = train_dynamic(net, opt, buf_x, buf_d, size)
        net.pack()                                           # the optimiser updated the weights in place: the image follows
        print("episode %d: %d steps, mean episode return %.3f, %d transitions, model loss %.4g"
              % (episode, step + 1, float(ret.mean()), size, loss), flush=True)
    env.close()


if __name__ == "__main__":
    main()
