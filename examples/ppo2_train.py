#!/usr/bin/env python3
"""Train a docking policy with PPO2, roll-out and update on the device: run_docking_ppo2.py:88-109 on N device envs.

    python examples/ppo2_train.py [--envs 10] [--updates 20] [--update hip|torch] [--eval-every 5] [--save out.npz] [--seed 0]

The defaults are the script's hyper-parameters: n_steps 600, nminibatches 10, noptepochs 10, lr 3e-4, cliprange 0.2, vf_coef 0.5,
max_grad_norm 0.5, ent_coef 0, gamma 0.99, lam 0.95, and a fresh SB2-initialised shared-trunk policy (net_arch [128, dict(pi=[128],
vf=[128])], ReLU: orthogonal with gain sqrt(2), 0.01 for the policy head, 1 for the value head, zero biases, logstd 0).  Per update
one Runner.run() (quadsim_amd.Runner, one launch plus post-processing) and one ppo2_update (qsp_update: noptepochs x nminibatches
Adam steps); the logged fields are printed per update.  --update torch runs the same update as a torch autograd loop
(torch_ppo2_update): the comparison.  Every --eval-every updates evaluate_policy_episodes runs the deterministic policy for one
episode per env."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402

SHAPES = {"w0": (12, 128), "b0": (128,), "w1": (128, 128), "b1": (128,), "w2": (128, 4), "b2": (4,), "wv1": (128, 128), "bv1": (128,),
          "wv2": (128, 1), "bv2": (1,)}


def sb2_actor_critic_weights(seed=0):
    """a fresh SB2 MlpPolicy of the shared-trunk layout as the dict ActorCriticPolicy takes"""
    g = torch.Generator().manual_seed(seed)
    out = {"logstd": np.zeros(4, np.float32)}
    for key, shape in SHAPES.items():
        if len(shape) == 1:
            out[key] = np.zeros(shape, np.float32)
        else:
            w = torch.empty(shape)
            torch.nn.init.orthogonal_(w, gain={"w2": 0.01, "wv2": 1.0}.get(key, 2.0 ** 0.5), generator=g)
            out[key] = w.numpy()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=10)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--n-steps", type=int, default=600)
    ap.add_argument("--nminibatches", type=int, default=10)
    ap.add_argument("--noptepochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--cliprange", type=float, default=0.2)
    ap.add_argument("--ent-coef", type=float, default=0.0)
    ap.add_argument("--update", choices=("hip", "torch"), default="hip")
    ap.add_argument("--eval-every", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None)
    args = ap.parse_args()

    policy = qa.ActorCriticPolicy(sb2_actor_critic_weights(args.seed))
    env = qa.VecDockingEnv("docking-v0", num_envs=args.envs, seed=args.seed)
    eval_env = qa.VecDockingEnv("docking-v0", num_envs=max(args.envs, 256), seed=args.seed + 1)
    model = qa.PPO2(policy, env, n_steps=args.n_steps, nminibatches=args.nminibatches, noptepochs=args.noptepochs, gamma=0.99, lam=0.95,
                    ent_coef=args.ent_coef, vf_coef=0.5, learning_rate=args.lr, max_grad_norm=0.5, cliprange=args.cliprange, seed=args.seed,
                    update=args.update)

    def evaluate(tag):
        eval_env.reset()
        res = qa.evaluate_policy_episodes(policy, eval_env, 1)
        print("eval %s: mean return %.3f +- %.3f, mean length %.1f, docked %.1f %%, over limit %.1f %% (%d episodes)" % (
            tag, res.mean_return(), res.std_return(), res.mean_length(), 100 * res.docked_fraction(), 100 * res.overlimit_fraction(),
            res.num_episodes()), flush=True)

    def callback(loc, glob):
        log = loc["logs"][-1] if loc["logs"] and loc["logs"][-1]["n_updates"] == loc["update"] else None
        if log is not None:
            print("update %(n_updates)d: timesteps %(total_timesteps)d fps %(fps)d explained_variance %(explained_variance).3f" % log
                  + " ep_reward_mean %.3f ep_len_mean %.1f" % (log.get("ep_reward_mean", float("nan")), log.get("ep_len_mean", float("nan")))
                  + " | policy_loss %(policy_loss).5f value_loss %(value_loss).5f entropy %(policy_entropy).4f approxkl %(approxkl).5f"
                    " clipfrac %(clipfrac).4f grad_norm %(grad_norm).4f" % log, flush=True)
        if args.eval_every and loc["update"] % args.eval_every == 0:
            evaluate("after update %d" % loc["update"])
        return True

    evaluate("before")
    t0 = time.perf_counter()
    model.learn(args.updates * model.n_batch, callback=callback)
    torch.cuda.synchronize()
    print("%d updates of %d samples (%d Adam steps each, --update %s) in %.2f s" % (
        args.updates, model.n_batch, args.nminibatches * args.noptepochs, args.update, time.perf_counter() - t0))
    evaluate("at the end")
    if args.save:
        policy.save_npz(args.save)
        print("saved", args.save)
    env.close()
    eval_env.close()


if __name__ == "__main__":
    main()
