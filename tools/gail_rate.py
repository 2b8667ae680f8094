#!/usr/bin/env python3
"""GAIL's discriminator on one MI355X: stream time of

  fit      d  device  Discriminator.fit (qsg_fit: every Adam step of the call in one launch of one workgroup)
           t  torch   torch_discriminator_fit: per step two gathers, three library GEMMs with tanh, autograd, tf.train.AdamOptimizer
           per step at 10 / 64 / 256 rows per class (64 steps a call), and a 4096-step call at 64 rows
  reward   d  device  Discriminator.reward (qsg_reward: exact-f32 MFMA, rows on the columns)
           t  torch   normalise, clamp, concat, three linear with tanh, -log(1 - sigmoid + 1e-8)
           a  actor   MlpPolicy.predict_hip (qs_policy_forward) on the same number of rows: the same-shaped net on the same pipe
           at 6 000 rows (the reference's 10 x 600), 65 536 x 32 and 65 536 x 600 rows, with the fraction of the f32-MFMA peak
  update   one GAIL update end to end at 65 536 docking-v0 envs x 32 steps: roll-out, reward, GAE, PPO2 update, discriminator fit, each on the
           device paths (d) and, for the two updates, on the torch paths (t)

on the same device, data and schedules.  The sides alternate for --rounds rounds after a warm-up round, in this order in odd rounds
and reversed in even ones; every figure is stream time between two events, reported per round and as a [min, max] range, never a
mean.  One JSON line per (cell, round) on stdout, everything in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import plan_timing  # noqa: E402  (tools/ is the script's directory)

FIT_CELLS = ((10, 64), (64, 64), (256, 64), (64, 4096))           # (rows per class, steps of a call)
REWARD_ROWS = (6000, 65536 * 32, 65536 * 600)
PEAK_F32_MFMA = 157.3e12                                           # FLOP/s, the part's specification
HIDDEN = 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--max-reward-rows", type=int, default=1 << 62)
    ap.add_argument("--skip-update", action="store_true")
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa
    from gail_train import sb2_tower_weights
    from quadsim_amd.policy import _actor_of

    dev = torch.device("cuda", 0)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    def rounds_of(cell, sides):
        rows = []
        for rnd in range(args.rounds + 1):                       # round 0 warms every cell up and is not reported
            row = dict(cell, round=rnd)
            for name, fn in (sides if rnd % 2 else sides[::-1]):
                torch.cuda.synchronize()
                row[name + "_ms"] = window(fn)
            if rnd:
                rows.append(row)
                print(json.dumps(row), flush=True)
        return rows

    def summarise(cell, rows, fast, slow):
        keys = [k for k in rows[0] if k.endswith("_ms")]
        rg = plan_timing.ranges(rows, keys)
        s = dict(cell, rounds=len(rows), **rg)
        for other in slow:
            spread = max(rg[k][1] - rg[k][0] for k in (fast, other))
            s[other[:-3] + "_over_" + fast[:-3]] = plan_timing.ratio_range(rows, other, fast)
            s[fast[:-3] + "_faster_than_" + other[:-3] + "_in_every_round_by_more_than_the_spread"] = all(r[other] - r[fast] > spread for r in rows)
        return s

    def data(n, seed):
        g = torch.Generator().manual_seed(seed)
        return ((torch.rand(n, 12, generator=g) - 0.5) * 4.0).to(dev), (torch.randn(n, 4, generator=g) * 0.7).to(dev)

    class Expert:
        pass
    expert = Expert()
    expert.obs, expert.actions = data(60000, 7)
    expert.actions.clamp_(-1.0, 1.0)

    results, summary = [], []
    # ------------------------------------------------------------------------------------------------ the fit
    gen_obs, gen_act = data(65536, 8)
    for batch, steps in FIT_CELLS:
        g = torch.Generator().manual_seed(3)
        gi, ei = qa.discriminator_schedule(65536, torch.arange(60000, dtype=torch.int32), batch, steps, g)
        discs = {k: qa.Discriminator(hidden=HIDDEN, seed=1, device=dev) for k in "dt"}
        for d in discs.values():
            d.update_stats(torch.cat([gen_obs[:4096], expert.obs[:4096]]).cpu().numpy())
            d.norm_tensors()
        sides = (("d_device", lambda: discs["d"].fit(gen_obs, gen_act, expert, gi, ei, update_stats=False)),
                 ("t_torch", lambda: qa.torch_discriminator_fit(discs["t"], gen_obs, gen_act, expert, gi, ei, update_stats=False)))
        cell = dict(kind="fit", batch=batch, steps=steps)
        rows = rounds_of(cell, sides)
        results += rows
        s = summarise(cell, rows, "d_device_ms", ("t_torch_ms",))
        s.update(d_us_per_step=[x * 1e3 / steps for x in s["d_device_ms"]], t_us_per_step=[x * 1e3 / steps for x in s["t_torch_ms"]])
        summary.append(s)
        print(json.dumps(dict(summary=s)), flush=True)
    # ------------------------------------------------------------------------------------------------ the reward
    env = qa.VecDockingEnv("docking-v1", num_envs=64, seed=1)
    pol = qa.ActorCriticPolicy(sb2_tower_weights(1))
    actor = _actor_of(pol)
    disc = qa.Discriminator(hidden=HIDDEN, seed=1, device=dev)
    disc.update_stats(expert.obs[:4096].cpu().numpy())
    mean, rscale = disc.norm_tensors()
    w = disc.tensors()

    def torch_reward(obs, act):
        x = torch.cat([(obs - mean) * rscale, act.clamp(-1.0, 1.0)], 1)
        logit = torch.addmm(w[5], torch.tanh(torch.addmm(w[3], torch.tanh(torch.addmm(w[1], x, w[0])), w[2])), w[4])[:, 0]
        return -torch.log(1.0 - torch.sigmoid(logit) + 1e-8)

    for n in REWARD_ROWS:
        if n > args.max_reward_rows:
            continue
        obs, act = data(n, 9)
        out_a = torch.empty((n, 4), dtype=torch.float32, device=dev)
        sides = (("d_device", lambda: disc.reward(obs, act)), ("a_actor", lambda: actor.predict_hip(env, obs, out=out_a)),
                 ("t_torch", lambda: torch_reward(obs, act)))
        cell = dict(kind="reward", rows=n)
        rows = rounds_of(cell, sides)
        results += rows
        s = summarise(cell, rows, "d_device_ms", ("t_torch_ms", "a_actor_ms"))
        flop_d, flop_a = 2.0 * (16 * HIDDEN + HIDDEN * HIDDEN + HIDDEN) * n, 2.0 * (12 * 128 + 128 * 128 + 128 * 4) * n
        s.update(d_fraction_of_f32_mfma_peak=[flop_d / (x * 1e-3) / PEAK_F32_MFMA for x in s["d_device_ms"][::-1]],
                 a_fraction_of_f32_mfma_peak=[flop_a / (x * 1e-3) / PEAK_F32_MFMA for x in s["a_actor_ms"][::-1]])
        summary.append(s)
        print(json.dumps(dict(summary=s)), flush=True)
        del obs, act, out_a
    env.close()
    # ------------------------------------------------------------------------------------------------ one update, end to end
    if not args.skip_update:
        n_envs, n_steps, d_steps, d_batch = 65536, 32, 3, 256
        hp = dict(learning_rate=3e-4, cliprange=0.2, cliprange_vf=None, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
        env = qa.VecDockingEnv("docking-v0", num_envs=n_envs, seed=2)      # the fused roll-out (docking-v1 takes the spelt-out loop)
        pols = {k: qa.ActorCriticPolicy(sb2_tower_weights(1)) for k in "dt"}
        discs = {k: qa.Discriminator(hidden=HIDDEN, seed=1, device=dev) for k in "dt"}
        gen = torch.Generator().manual_seed(4)
        env.reset()
        rows = []
        for rnd in range(args.rounds + 1):
            row = dict(kind="update", envs=n_envs, n_steps=n_steps, d_steps=d_steps, d_batch=d_batch, round=rnd)
            ro = {}
            zeros = torch.zeros(n_envs, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            row["rollout_ms"] = window(lambda: ro.update(qa.fused_runner_rollout(env, pols["d"], n_steps, dones_in=zeros, env_major=True)))
            obs, act = ro["obs"].view(-1, 12), ro["actions"].view(-1, 4)
            paid = {}
            row["reward_ms"] = window(lambda: paid.update(r=discs["d"].reward(obs, act, n_envs=n_envs, n_steps=n_steps)))
            gf = {}
            row["gae_ms"] = window(lambda: gf.update(qa.gae_and_flatten(env, paid["r"], ro["values"], ro["neglogp"], ro["dones"], ro["last_values"],
                                                                         ro["last_dones"], 0.99, 0.95)))
            batch = dict(obs=obs, actions=act, returns=gf["returns"], values=gf["values"], neglogp=gf["neglogp"])
            idx = qa.minibatch_schedule(n_envs * n_steps, 4, 4, gen, dev)
            gi, ei = qa.discriminator_schedule(n_envs * n_steps, torch.arange(60000, dtype=torch.int32), d_batch, d_steps, gen)
            order = (("d", qa.ppo2_update, lambda d, *a: d.fit(*a)), ("t", qa.torch_ppo2_update, qa.torch_discriminator_fit))
            for k, upd, fit in (order if rnd % 2 else order[::-1]):
                torch.cuda.synchronize()
                row[k + "_ppo2_update_ms"] = window(lambda: upd(pols[k], batch, idx, check_indices=False, **hp))
                row[k + "_disc_fit_ms"] = window(lambda: fit(discs[k], obs, act, expert, gi, ei))
            row["d_total_ms"] = sum(row[k] for k in ("rollout_ms", "reward_ms", "gae_ms", "d_ppo2_update_ms", "d_disc_fit_ms"))
            row["t_total_ms"] = sum(row[k] for k in ("rollout_ms", "reward_ms", "gae_ms", "t_ppo2_update_ms", "t_disc_fit_ms"))
            if rnd:
                rows.append(row)
                print(json.dumps(row), flush=True)
        results += rows
        s = summarise(dict(kind="update", envs=n_envs, n_steps=n_steps), rows, "d_total_ms", ("t_total_ms",))
        summary.append(s)
        print(json.dumps(dict(summary=s)), flush=True)
        env.close()
    plan_timing.write_out(args.out, torch, rounds=results, summary=summary)


if __name__ == "__main__":
    main()
