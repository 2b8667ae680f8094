#!/usr/bin/env python3
"""Behaviour-clone a fresh actor from the PID expert, all on the device: the three steps of the reference's imitation path
(run_expert_record.py, then ``model.pretrain(dataset, n_epochs)`` of run_pretrained_ppo2_docking.py:50-69, then evaluation) for N
docking-v1 envs.

    python examples/pretrain_policy.py [--envs 256] [--episodes 1] [--epochs 10] [--batch 64] [--lr 1e-4] [--fit hip|torch]
                                       [--save out.npz]

record_expert_dataset records K complete episodes per env; a fresh actor gets SB2's initialiser (orthogonal, gain sqrt(2) for the
hidden layers and 0.01 for the head, zero biases); ``pretrain`` (qsbc_fit: up to 4096 Adam steps a launch) prints the train and
validation loss per epoch; evaluate_policy_episodes runs before and after, beside the expert's own PIDExpert.evaluate.
--fit torch runs the same schedule through a torch autograd loop with torch.optim.Adam (which puts eps elsewhere than
tf.train.AdamOptimizer: the two are not bit-comparable): the comparison, not part of the library."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import quadsim_amd as qa  # noqa: E402
from quadsim_amd.bc import ACTOR_KEYS, ACTOR_SHAPES, bc_loss, epoch_schedule  # noqa: E402


def sb2_actor_weights(seed=0):
    """a fresh SB2 actor as the dict MlpPolicy takes: ortho_init(sqrt(2)) hidden layers, ortho_init(0.01) head, zero biases"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key, shape in zip(ACTOR_KEYS, ACTOR_SHAPES):
        if len(shape) == 1:
            out[key] = np.zeros(shape, np.float32)
        else:
            w = torch.empty(shape)
            torch.nn.init.orthogonal_(w, gain=0.01 if key == "w2" else 2.0 ** 0.5, generator=g)
            out[key] = w.numpy()
    return out


def torch_steps(params, opt, obs, act, indices, counts):
    """the comparison: the steps of one schedule (indices [steps,batch] on the device, counts a host list) as a torch autograd
    loop -- gather, three linear + ReLU, the mean squared error, backward, Adam.step -> the losses (device tensors)"""
    w0, b0, w1, b1, w2, b2 = params
    losses = []
    for s, c in enumerate(counts):
        rows = indices[s, :c].long()
        h = torch.relu(torch.addmm(b0, obs[rows], w0))
        h = torch.relu(torch.addmm(b1, h, w1))
        loss = ((torch.addmm(b2, h, w2) - act[rows]) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return losses


def torch_pretrain(policy, data, n_epochs, lr, eps, val_interval, seed):
    """qa.pretrain's schedule and return value through torch_steps; the policy's tensors are trained in place"""
    params = [getattr(policy, k).requires_grad_(True) for k in ACTOR_KEYS]
    opt = torch.optim.Adam(params, lr=lr, eps=eps)
    gen = torch.Generator().manual_seed(seed)
    train, val, total = [], {}, 0
    for epoch in range(1, n_epochs + 1):
        pos, counts = epoch_schedule(data.n_train, data.batch_size, 1, gen)
        indices = data.train_rows[pos.long()].to(data.device)
        losses = torch_steps(params, opt, data.obs, data.actions, indices, counts.tolist())
        train.append(float(torch.stack(losses).double().mean()))
        total += len(losses)
        if epoch % val_interval == 0 and data.n_val:
            for p in params:
                p.requires_grad_(False)
            val[epoch] = float(bc_loss(policy, data.obs, data.actions, data.val_rows_device()))
            for p in params:
                p.requires_grad_(True)
    for p in params:
        p.requires_grad_(False)
    qa.bc.drop_cached_images(policy)
    return {"train_loss": train, "val_loss": val, "steps": total}


def report(name, res):
    print("%-22s %6d episodes, return %9.3f +- %8.3f, length %6.1f, docked %5.1f %%, over limit %5.1f %%"
          % (name, res.num_episodes(), res.mean_return(), res.std_return(), res.mean_length(), 100 * res.docked_fraction(),
             100 * res.overlimit_fraction()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=1, help="expert episodes recorded per env")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1.0e-4)
    ap.add_argument("--eps", type=float, default=1.0e-8)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--fit", default="hip", choices=("hip", "torch"))
    ap.add_argument("--save", default=None, help="write the trained actor as an .npz MlpPolicy.from_npz reads")
    args = ap.parse_args()

    env = qa.VecDockingEnv("docking-v1", num_envs=args.envs, seed=args.seed)
    expert = qa.PIDExpert(env)
    t0 = time.perf_counter()
    rec = qa.record_expert_dataset(env, n_episodes=args.episodes, expert=expert)
    print("recorded %d rows (%d episodes, mean return %.3f) in %.2f s"
          % (len(rec["obs"]), len(rec["episode_returns"]), float(np.mean(rec["episode_returns"])), time.perf_counter() - t0))
    data = qa.ExpertData(rec, batch_size=args.batch, seed=args.seed)
    policy = qa.MlpPolicy(sb2_actor_weights(args.seed))
    env.reset()
    report("expert (PID)", qa.PIDExpert(env).evaluate(1))
    report("actor before", qa.evaluate_policy_episodes(policy, env, 1))

    val_interval = max(1, args.epochs // 10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if args.fit == "hip":
        res = policy.pretrain(data, n_epochs=args.epochs, learning_rate=args.lr, adam_epsilon=args.eps, val_interval=val_interval,
                              seed=args.seed)
    else:
        res = torch_pretrain(policy, data, args.epochs, args.lr, args.eps, val_interval, args.seed)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    for e, tr in enumerate(res["train_loss"], 1):
        print("epoch %3d  train loss %.6f%s" % (e, tr, "  validation loss %.6f" % res["val_loss"][e] if e in res["val_loss"] else ""))
    print("--fit %s: %d steps of batch %d on %d train rows in %.2f s wall (%.1f us a step, host included)"
          % (args.fit, res["steps"], args.batch, data.n_train, sec, sec / res["steps"] * 1e6))
    env.reset()
    report("actor after", qa.evaluate_policy_episodes(policy, env, 1))
    if args.save:
        np.savez(args.save, **{k: getattr(policy, k).cpu().numpy() for k in ACTOR_KEYS})
        print("saved", args.save)
    env.close()


if __name__ == "__main__":
    main()
