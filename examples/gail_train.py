#!/usr/bin/env python3
"""GAIL from the PID expert, all on the device: run_docking_gail.py of the reference for N docking-v1 envs.

    python examples/gail_train.py [--envs 256] [--episodes 1] [--expert expert.npz] [--timesteps 1000000] [--n-steps 128]
                                  [--d-steps 3] [--d-batch 256] [--fit hip|torch] [--generator ppo2|trpo] [--save out.npz]

The expert is recorded (record_expert_dataset, K complete episodes per env) or loaded from an .npz with its keys; the policy is a
fresh SB2 actor-critic of the tower layout (pi = vf = [128, 128], ReLU); ``GAIL.learn`` runs roll-out (scored by the current
discriminator), PPO2 update and discriminator steps per update and prints PPO2's fields, the five discriminator statistics and
the mean TRUE episode return; evaluate_policy_episodes runs before and after, beside the expert's own PIDExpert.evaluate.
--fit torch runs the same loop through the two torch autograd paths (torch_ppo2_update, torch_discriminator_fit): the
comparison.  --generator ppo2 (the default) is this package's PPO2 under ``GAIL``; --generator trpo is SB2's own choice: ``TRPO`` with
the expert (max_kl 0.01, 10 CG iterations, lam 0.98, 3 value passes of batch 128, g_step 3, d_step 1; --d-steps, --d-batch and --d-lr
still apply, the PPO2 options do not).  Whether the result docks is reported, not asserted."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402
from quadsim_amd.gail import DISC_STAT_NAMES  # noqa: E402
from quadsim_amd.ppo2 import SLOT_KEYS, SLOT_SHAPES  # noqa: E402


def sb2_tower_weights(seed=0):
    """a fresh SB2 actor-critic with separate towers as the dict ActorCriticPolicy takes: ortho_init(sqrt(2)) hidden layers,
    ortho_init(0.01) policy head, ortho_init(1) value head, zero biases and logstd"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key, shape in zip(SLOT_KEYS, SLOT_SHAPES):
        if len(shape) == 1:
            out[key] = np.zeros(shape, np.float32)
        else:
            w = torch.empty(shape)
            torch.nn.init.orthogonal_(w, gain={"w2": 0.01, "wv2": 1.0}.get(key, 2.0 ** 0.5), generator=g)
            out[key] = w.numpy()
    return out


def report(name, res):
    print("%-22s %6d episodes, return %9.3f +- %8.3f, length %6.1f, docked %5.1f %%, over limit %5.1f %%"
          % (name, res.num_episodes(), res.mean_return(), res.std_return(), res.mean_length(), 100 * res.docked_fraction(),
             100 * res.overlimit_fraction()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=1, help="expert episodes recorded per env")
    ap.add_argument("--expert", default=None, help="an .npz of record_expert_dataset instead of recording")
    ap.add_argument("--timesteps", type=int, default=1000000)
    ap.add_argument("--n-steps", type=int, default=128)
    ap.add_argument("--nminibatches", type=int, default=4)
    ap.add_argument("--noptepochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=2.5e-4)
    ap.add_argument("--ent-coef", type=float, default=0.0)
    ap.add_argument("--d-steps", type=int, default=3)
    ap.add_argument("--d-batch", type=int, default=256)
    ap.add_argument("--d-lr", type=float, default=3.0e-4)
    ap.add_argument("--hidden", type=int, default=100, help="SB2's hidden_size_adversary")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fit", default="hip", choices=("hip", "torch"))
    ap.add_argument("--generator", default="ppo2", choices=("ppo2", "trpo"), help="what trains the policy: GAIL's PPO2, or TRPO as in SB2")
    ap.add_argument("--g-step", type=int, default=3, help="--generator trpo: roll-outs and policy steps per discriminator fit")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--save", default=None, help="write the trained policy as an .npz ActorCriticPolicy.from_npz reads")
    args = ap.parse_args()

    env = qa.VecDockingEnv("docking-v1", num_envs=args.envs, seed=args.seed)
    eval_env = qa.VecDockingEnv("docking-v1", num_envs=max(args.envs, 256), seed=args.seed + 1)
    if args.expert:
        data = qa.ExpertData(args.expert, seed=args.seed)
        print("loaded %d expert rows from %s" % (data.n, args.expert))
    else:
        t0 = time.perf_counter()
        rec = qa.record_expert_dataset(env, n_episodes=args.episodes, expert=qa.PIDExpert(env))
        print("recorded %d rows (%d episodes, mean return %.3f) in %.2f s"
              % (len(rec["obs"]), len(rec["episode_returns"]), float(np.mean(rec["episode_returns"])), time.perf_counter() - t0))
        data = qa.ExpertData(rec, seed=args.seed)
    policy = qa.ActorCriticPolicy(sb2_tower_weights(args.seed))
    disc = qa.Discriminator(hidden=args.hidden, seed=args.seed, device=env.device)
    eval_env.reset()
    report("expert (PID)", qa.PIDExpert(eval_env).evaluate(1))
    eval_env.reset()
    report("policy before", qa.evaluate_policy_episodes(policy, eval_env, 1))

    if args.generator == "trpo":
        model = qa.TRPO(policy, env, n_steps=args.n_steps, expert_data=data, discriminator=disc, g_step=args.g_step, d_step=args.d_steps,
                        d_batch=args.d_batch, d_stepsize=args.d_lr, update=args.fit, entcoeff=args.ent_coef, seed=args.seed)
    else:
        model = qa.GAIL(policy, env, data, discriminator=disc, d_steps=args.d_steps, d_batch=args.d_batch, d_learning_rate=args.d_lr,
                        update=args.fit, n_steps=args.n_steps, nminibatches=args.nminibatches, noptepochs=args.noptepochs,
                        ent_coef=args.ent_coef, learning_rate=args.lr, seed=args.seed)

    def callback(loc, glob):
        log = loc["logs"][-1] if loc["logs"] and loc["logs"][-1]["n_updates"] == loc["update"] else None
        if log is not None and (log["n_updates"] == 1 or log["n_updates"] % args.log_every == 0):
            print("update %5d  steps %9d  true return %9.3f  paid %7.4f  %s" % (
                log["n_updates"], log["total_timesteps"], log.get("true_ep_reward_mean", float("nan")), log["disc_reward_mean"],
                "  ".join("%s %.4f" % (k, log.get("disc_" + k, log[k])) for k in DISC_STAT_NAMES)))      # (TRPO's log: disc_entropy)
        return True

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logs = model.learn(args.timesteps, callback=callback)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    per = args.g_step if args.generator == "trpo" else 1
    if args.generator == "trpo" and logs:
        print("--generator trpo: last policy step accepted candidate %d after %d CG iterations, kl %.5f" % (
            logs[-1]["accepted"], logs[-1]["cg_iters_run"], logs[-1]["kl_after"]))
    print("--fit %s: %d updates of %d x %d steps in %.2f s wall (%.0f env steps / s, host included)"
          % (args.fit, len(logs), per * args.envs, args.n_steps, sec, len(logs) * per * args.envs * args.n_steps / max(sec, 1e-9)))
    eval_env.reset()
    res = qa.evaluate_policy_episodes(policy, eval_env, 1)
    report("policy after", res)
    print("the trained policy %s" % ("docks in %.1f %% of its episodes" % (100 * res.docked_fraction()) if res.docked_fraction() > 0
                                     else "does not dock"))
    if args.save:
        policy.save_npz(args.save)
        print("saved", args.save)
    env.close()
    eval_env.close()


if __name__ == "__main__":
    main()
