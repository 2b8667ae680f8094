#!/usr/bin/env python3
"""SAC on the device for N docking-v0 envs: the off-policy trainer whose actor learns its own state-dependent exploration.

    python examples/sac_train.py [--envs 16] [--timesteps 1000000] [--rhythm ddpg|sb2] [--update hip|torch] [--save out.npz]

The policy is SB2's SAC MlpPolicy (layers [128, 128], ReLU; the actor's head emits a mean and a log standard deviation, two critics on
[obs ; act], a value net and its target) with SB2's initialisation; collection is the per-step loop over env.step that
examples/ddpg_train.py runs, with uniform actions for the first `learning_starts` transitions and samples of the actor after them:
there is no action noise.  --rhythm ddpg is run_docking_ddpg.py's: after every 1500 env.step calls ONE call of 100 updates of batch
10; --rhythm sb2 is SB2 SAC's default: after every call one update of batch 64 (sac_update, libquadsim_sac.so: one launch of four
workgroups per update).  Single flags override either.  --update torch runs the same loop through the torch autograd path
(torch_sac_update): the comparison.  The evaluation before and after is examples/ddpg_train.py's per-step loop of the deterministic
action tanh(mu).  Whether the result docks is reported, not asserted."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402
from ddpg_train import evaluate, report  # noqa: E402  (the evaluation loop is the same)
from quadsim_amd.sac import SAC_STAT_NAMES  # noqa: E402

RHYTHMS = {"ddpg": dict(train_freq=1500, gradient_steps=100, batch=10), "sb2": dict(train_freq=1, gradient_steps=1, batch=64)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--timesteps", type=int, default=1000000)
    ap.add_argument("--rhythm", default="ddpg", choices=sorted(RHYTHMS), help="run_docking_ddpg.py's 1500 / 100 / 10 or SB2 SAC's 1 / 1 / 64")
    ap.add_argument("--train-freq", type=int, default=None)
    ap.add_argument("--gradient-steps", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--buffer", type=int, default=50000)
    ap.add_argument("--learning-starts", type=int, default=100)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--tau", type=float, default=5.0e-3)
    ap.add_argument("--learning-rate", type=float, default=3.0e-4)
    ap.add_argument("--ent-coef", default="auto", help="'auto', 'auto_<initial value>' or a fixed number")
    ap.add_argument("--target-entropy", default="auto", help="'auto' (-4) or a number")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--update", default="hip", choices=("hip", "torch"))
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--save", default=None, help="write the five nets, the temperature and the optimiser state as an .npz SACPolicy.from_npz reads")
    args = ap.parse_args()
    rhythm = RHYTHMS[args.rhythm]
    train_freq = args.train_freq or rhythm["train_freq"]
    gradient_steps = args.gradient_steps or rhythm["gradient_steps"]
    batch = args.batch or rhythm["batch"]
    ent_coef = args.ent_coef if args.ent_coef.startswith("auto") else float(args.ent_coef)
    target_entropy = args.target_entropy if args.target_entropy == "auto" else float(args.target_entropy)

    env = qa.VecDockingEnv("docking-v0", num_envs=args.envs, seed=args.seed)
    eval_env = qa.VecDockingEnv("docking-v0", num_envs=max(args.envs, 256), seed=args.seed + 1)
    policy = qa.SACPolicy(seed=args.seed, device=env.device)
    report("policy before", evaluate(policy, eval_env))
    model = qa.SAC(policy, env, gamma=args.gamma, learning_rate=args.learning_rate, buffer_size=args.buffer, learning_starts=args.learning_starts,
                   train_freq=train_freq, gradient_steps=gradient_steps, batch_size=batch, tau=args.tau, ent_coef=ent_coef,
                   target_entropy=target_entropy, update=args.update, seed=args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logs = model.learn(args.timesteps)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    for log in logs:
        if log["cycle"] == 1 or log["cycle"] % args.log_every == 0:
            print("cycle %5d  steps %9d  reward %8.4f  %s" % (log["cycle"], log["total_timesteps"], log["reward_mean"],
                                                                "  ".join("%s %.4f" % (k, log[k]) for k in SAC_STAT_NAMES)))
    print("--update %s: %d cycles of %d x %d env steps and %d updates of batch %d in %.2f s wall (%.0f env steps / s, host included)"
          % (args.update, len(logs), train_freq, args.envs, gradient_steps, batch, sec, model.num_timesteps / max(sec, 1e-9)))
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
