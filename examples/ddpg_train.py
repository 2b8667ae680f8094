#!/usr/bin/env python3
"""DDPG on the device: run_docking_ddpg.py of the reference for N docking-v0 envs, with its hyper-parameters.

    python examples/ddpg_train.py [--envs 16] [--timesteps 1000000] [--update hip|torch] [--save out.npz]

The policy is SB2's CustomDDPGPolicy (layers [128, 128], ReLU, tanh actor) with SB2's initialisation; collection is a per-step
loop over env.step with Ornstein-Uhlenbeck noise (sigma 0.5) and a uniform action with probability 0.3 per env; after every
nb_rollout_steps = 1500 env.step calls ONE call of nb_train_steps = 100 updates of batch_size = 10 from the replay of 50 000
transitions (ddpg_update, libquadsim_ddpg.so).  --update torch runs the same loop through the torch autograd path
(torch_ddpg_update): the comparison.  The evaluation before and after is a plain per-step loop of the deterministic tanh actor:
the fused evaluation kernels run the CLIPPED actor of the PPO2 policies, not a tanh one, and a tanh variant of them is not built.
Whether the result docks is reported, not asserted."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402
from quadsim_amd._lib import FLAG_DOCKED  # noqa: E402
from quadsim_amd.ddpg import DDPG_STAT_NAMES  # noqa: E402


def evaluate(policy, env, max_steps=1000):
    """one episode per env of the deterministic actor, step by step -> (mean return, mean length, docked fraction)"""
    n = env.num_envs
    obs = env.reset().clone()
    ret = torch.zeros(n, dtype=torch.float64, device=env.device)
    length = torch.zeros(n, dtype=torch.int64, device=env.device)
    live = torch.ones(n, dtype=torch.bool, device=env.device)
    docked = torch.zeros(n, dtype=torch.bool, device=env.device)
    for _ in range(max_steps):
        with torch.no_grad():
            a = policy.predict(obs).contiguous()
        obs, rew, done, info = env.step(a)
        obs = obs.clone()
        ret += torch.where(live, rew.double(), torch.zeros_like(ret))
        length += live.long()
        docked |= live & done & ((info._dev[1].long() & FLAG_DOCKED) != 0)          # this step's flags, on the device
        live &= ~done
        if not bool(live.any()):
            break
    return float(ret.mean()), float(length.double().mean()), float(docked.double().mean())


def report(name, res):
    print("%-14s return %9.3f, length %6.1f, docked %5.1f %%" % (name, res[0], res[1], 100 * res[2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=1000000)
    ap.add_argument("--rollout-steps", type=int, default=1500)
    ap.add_argument("--train-steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--buffer", type=int, default=50000)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--tau", type=float, default=1.0e-3)
    ap.add_argument("--actor-lr", type=float, default=1.0e-4)
    ap.add_argument("--critic-lr", type=float, default=1.0e-3)
    ap.add_argument("--sigma", type=float, default=0.5, help="of the Ornstein-Uhlenbeck action noise")
    ap.add_argument("--random-exploration", type=float, default=0.3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--update", default="hip", choices=("hip", "torch"))
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--save", default=None, help="write the four nets and the optimiser state as an .npz DDPGPolicy.from_npz reads")
    args = ap.parse_args()

    env = qa.VecDockingEnv("docking-v0", num_envs=args.envs, seed=args.seed)
    eval_env = qa.VecDockingEnv("docking-v0", num_envs=max(args.envs, 256), seed=args.seed + 1)
    policy = qa.DDPGPolicy(seed=args.seed, device=env.device)
    report("policy before", evaluate(policy, eval_env))
    model = qa.DDPG(policy, env, gamma=args.gamma, tau=args.tau, actor_lr=args.actor_lr, critic_lr=args.critic_lr,
                    nb_rollout_steps=args.rollout_steps, nb_train_steps=args.train_steps, batch_size=args.batch, buffer_size=args.buffer,
                    random_exploration=args.random_exploration,
                    action_noise=qa.OUNoise(args.envs, sigma=args.sigma, device=env.device, seed=args.seed), update=args.update, seed=args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logs = model.learn(args.timesteps)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    for log in logs:
        if log["cycle"] == 1 or log["cycle"] % args.log_every == 0:
            print("cycle %5d  steps %9d  reward %8.4f  %s" % (log["cycle"], log["total_timesteps"], log["reward_mean"],
                                                                "  ".join("%s %.4f" % (k, log[k]) for k in DDPG_STAT_NAMES)))
    print("--update %s: %d cycles of %d x %d env steps and %d updates in %.2f s wall (%.0f env steps / s, host included)"
          % (args.update, len(logs), args.rollout_steps, args.envs, args.train_steps, sec, model.num_timesteps / max(sec, 1e-9)))
    res = evaluate(policy, eval_env)
    report("policy after", res)
    print("the trained policy %s" % ("docks in %.1f %% of its episodes" % (100 * res[2]) if res[2] > 0 else "does not dock"))
    if args.save:
        policy.save_npz(args.save)
        print("saved", args.save)
    env.close()
    eval_env.close()


if __name__ == "__main__":
    main()
