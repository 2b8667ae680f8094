"""The training loops on the device, every row of tests/loop_cases.py, by the record-and-replay recipe of tests/loop_replay.py: a loop run
is recorded through the hooks the public API offers (nothing in quadsim_amd is replaced), and every update is replayed from the record
as a chain of single calls that must end in the loop's own bits, every link of it held to the trainer's float64 reference within that
reference's existing bounds.  What each loop is held to on top of that:

  PPO2      the rates of update u are the row's callables at 1 - (u - 1) / n_updates; its schedule is the u-th draw of one carried
            generator; the second roll-out is the first one's continuation (a twin env and a twin Runner, handed a fresh policy built from
            the snapshot before and after update 1, give the recorded second 9-tuple bit for bit: no stale weight image, no reset, the
            done flags carried); values and observations lie in one row order; the log is the float64 mean of the steps' statistics,
            the counters are the reference's, explained_variance is the float64 formula
  GAIL      as PPO2 (its loop is a copy), docking-v1 on the spelt-out roll-out and docking-v0 on the fused one; the draws interleave on
            the one generator, minibatches first; the discriminator fit as a chain against gail_ref, the expert's shuffles carried and
            renewed inside update 2; element 8 of the tuple is the env's reward and the returns are GAE over the paid one, for both
            roll-outs; the running statistics take one merge per fit
  TRPO      per generator step the policy step and the value fit on the carried generator, both roll-outs of an update recorded; the
            discriminator fit on the LAST roll-out's rows; vf_loss, the counters
  DDPG      the ring after every cycle; the c-th draw over the ring's size then; the behaviour action with a twin OU noise; reward_mean
  TD3       as DDPG, the delay phase and the keyed noise carried over the learn calls, the noise once keyed and once the caller's
  pretrain  every epoch a fresh shuffle of one generator, the partial minibatch, train_loss, val_loss, the second call
The conditions of the records (an episode ends inside a roll-out or cycle and ON its last step, another env is in mid-episode there) are
asserted, not assumed.  The worst error / bound of every row is printed; profiles/loops/README.md has a copy and the table of mutants."""
import numpy as np
import pytest

import bcfit_ref as br
import loop_cases as lc
import loop_replay as lp
import postproc_ref as pp
import ppo2_ref as pr
import trpo_ref as tr
from side_cases import same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def make_env(row):
    import quadsim_amd as qa
    return qa.VecDockingEnv(row.get("env_id", "docking-v0"), num_envs=row["n_envs"], seed=row["env_seed"])


def place(row):
    """after_reset of a Recorded: the envs named in the row's `ends` are moved near their time limit"""
    return lambda env: env.set_state(t=lc.start_times(row["n_envs"], row["ends"]))


def report(row_id, worst):
    top = max(worst, key=worst.get)
    print("loops ratio %s: worst error / bound %.3g (%s)" % (row_id, worst[top], top))


# ---------------------------------------------------------------------------------------------------- DDPG and TD3
@pytest.mark.parametrize("row_id", ["ddpg", "td3-keyed", "td3-caller"])
def test_off_policy_learn_is_a_replay_of_its_ring(torch, row_id):
    import quadsim_amd as qa
    row = lc.BY_ID[row_id]
    env = lp.Recorded(make_env(row), after_reset=place(row))
    rec = lp.run_off_policy(qa, row, env, "hip", DEV)
    env.env.close()
    report(row_id, lp.check_off_policy(qa, row, rec, "hip", DEV))
    lp.check_behaviour_actions(qa, row, rec, DEV)


def test_uniform_exploration_replaces_every_action(torch):
    import quadsim_amd as qa
    row = lc.BY_ID["ddpg-explore"]
    env = lp.Recorded(make_env(row), after_reset=place(row))
    rec = lp.run_off_policy(qa, row, env, "hip", DEV)
    env.env.close()
    lp.check_behaviour_actions(qa, row, rec, DEV)
    assert rec["snaps"][1]["steps"] == row["kwargs"]["nb_train_steps"]


# ---------------------------------------------------------------------------------------------------- pretrain
def test_pretrain_is_a_replay_of_its_epochs(torch):
    import quadsim_amd as qa
    row = lc.BY_ID["pretrain"]
    obs, act = lc.pretrain_data(row)
    data = qa.ExpertData({"obs": obs, "actions": act}, train_fraction=row["train_fraction"], batch_size=row["batch_size"], seed=row["split_seed"],
                         device=DEV)
    train, val = lp.split_rows(row["n"], row["train_fraction"], row["split_seed"])
    W0 = pr.weight_set("he", "shared")
    pol = qa.ActorCriticPolicy(W0, device=DEV)
    snap, worst, bs = lp.bc_snapshot(pol), {}, row["batch_size"]
    for call in row["calls"]:
        out = qa.pretrain(pol, data, **call)
        after = lp.bc_snapshot(pol)
        gen = torch.Generator().manual_seed(call["seed"])
        lr, eps = call["learning_rate"], call["adam_epsilon"]
        cur, seen = snap, []
        for e in range(1, call["n_epochs"] + 1):
            steps = lp.epoch_rows(train, bs, gen)                              # a fresh shuffle of the ONE generator of this call
            assert [len(s) for s in steps] == [64, 41] and not any(np.array_equal(np.concatenate(steps), s) for s in seen)
            seen.append(np.concatenate(steps))
            cur, losses, links = lp.bc_chain(qa, W0, cur, obs, act, steps, bs, lr, eps, DEV)
            for link in links:
                for k, r in lp.bc_check_link(link, obs, act, lr, eps).items():
                    worst[k] = max(worst.get(k, 0.0), r)
            lp.check_mean(out["train_loss"][e - 1], losses, DEV, "epoch %d" % e)
            if e % call["val_interval"] == 0:                                  # the weights as they were at that epoch: the chain's
                F = br.forward64(cur["w"], obs[val], act[val])
                r = abs(out["val_loss"][e] - F["loss"]) / br.loss_bound(cur["w"], obs[val], act[val])
                worst["val_loss"] = max(worst.get("val_loss", 0.0), r)
                assert r <= 1.0, (e, out["val_loss"][e], F["loss"])
        assert sorted(out["val_loss"]) == [e for e in range(1, call["n_epochs"] + 1) if e % call["val_interval"] == 0]
        bad = lp.bc_same_bits(cur, after)
        assert not bad, "the chain does not end in pretrain's bits: %s" % bad
        assert out["steps"] == 2 * call["n_epochs"] and after["steps"] == snap["steps"] + out["steps"]
        snap = after
    assert snap["steps"] == 8 and all(np.abs(snap["m"][k]).max() > 0.0 for k in br.KEYS)
    for k in ("wv1", "bv1", "wv2", "bv2", "logstd"):                            # only the actor moved
        assert same_bits(lp.host(getattr(pol, k)), np.asarray(W0[k], np.float32)), k
    report("pretrain", worst)


# ---------------------------------------------------------------------------------------------------- PPO2
def masks_of(rollout, n, T):
    return rollout[lp.TUPLE["masks"]].reshape(n, T).astype(bool)


def check_episode_ends(first, second, n, T, what):
    """on the record: an episode ends strictly inside either roll-out, one ends ON the first one's last step (the flag carried over
    the boundary) and another env is in mid-episode there"""
    m1, m2 = masks_of(first, n, T), masks_of(second, n, T)
    assert not m1[:, 0].any() and m1[:, 1:].any() and m2[:, 1:].any(), "%s: no episode ends inside a roll-out" % what
    assert m2[:, 0].any() and not m2[:, 0].all(), "%s: the boundary lacks a carried done flag or an env in mid-episode" % what


@pytest.mark.parametrize("row_id", lc.ids_of("ppo2"))
def test_ppo2_learn_is_a_replay_of_its_rollouts(torch, row_id):
    import quadsim_amd as qa
    row = lc.BY_ID[row_id]
    n, T, K = row["n_envs"], row["n_steps"], row["kwargs"]
    n_batch = n * T
    env = make_env(row)
    pol = qa.ActorCriticPolicy(pr.weight_set("sb2", row["layout"]), device=DEV)
    model = qa.PPO2(pol, env, n_steps=T, seed=row["seed"], **K)
    assert model.runner.fused and model.runner.precision == "f32"
    env.set_state(t=lc.start_times(n, row["ends"]))
    before = lp.ppo2_snapshot(pol)
    rec = lp.Recorder(lp.LOOP_KEYS, lambda: lp.ppo2_snapshot(pol))
    logs = model.learn(2 * n_batch + 5, callback=rec)
    env.close()
    assert len(logs) == len(rec.updates) == 2 and model.num_timesteps == 2 * n_batch and rec.updates[1]["after"]["steps"] == 16
    first, second = rec.updates[0]["rollout"], rec.updates[1]["rollout"]
    check_episode_ends(first, second, n, T, row_id)
    # every update from the record
    gen, pre, worst = torch.Generator().manual_seed(row["seed"]), before, np.zeros(3)
    for u in (1, 2):
        r = rec.updates[u - 1]
        idx = lp.draw_minibatches(n_batch, K["nminibatches"], K["noptepochs"], gen)
        worst = np.maximum(worst, lp.check_ppo2_update(qa, row, u, 2, pre, r, idx, lc.EV_TOL, "hip", DEV))
        lp.check_values_of_obs(pre, r["rollout"], "%s roll-out %d" % (row_id, u))
        pre = r["after"]
    print("loops ratio %s: gradients worst error / bound %.3g, statistics %.3g, update %.3g" % (row_id, *worst))
    # the second roll-out continues the first
    twin = make_env(row)
    runner = qa.Runner(env=twin, model=lp.ppo2_restore(qa, before, DEV), n_steps=T, gamma=K["gamma"], lam=K["lam"], collect_ep_infos=False)
    twin.set_state(t=lc.start_times(n, row["ends"]))
    assert not lp.tuples_same_bits(lp.Recorder._copy(runner.run()), first)
    runner.model = lp.ppo2_restore(qa, rec.updates[0]["after"], DEV)
    bad = lp.tuples_same_bits(lp.Recorder._copy(runner.run()), second)
    twin.close()
    assert not bad, "the second roll-out is not the first one's continuation under the updated policy: %s" % bad


# ---------------------------------------------------------------------------------------------------- GAIL
def make_expert(torch, spec):
    import quadsim_amd as qa
    expert = qa.ExpertData(lc.expert_data(spec), train_fraction=spec["train_fraction"], seed=spec["seed"], device=DEV)
    train, _ = lp.split_rows(spec["n"], spec["train_fraction"], spec["seed"])
    assert np.array_equal(train, expert.train_rows.numpy())
    return expert, train


def step_major(flat, n, T):
    return np.ascontiguousarray(flat.reshape(n, T).T)


def check_gae_of(rollout, paid, last_values, last_dones, n, T, gamma, lam, what):
    """the returns of a recorded 9-tuple are GAE over `paid` [T, n], within the bound tests/test_gpu_postproc.py holds the kernel to"""
    ref = pp.gae64(paid, step_major(rollout[lp.TUPLE["values"]], n, T), step_major(rollout[lp.TUPLE["masks"]], n, T), last_values, last_dones, gamma, lam)
    return pp.check_gae(None, step_major(rollout[lp.TUPLE["returns"]], n, T), ref, what)


@pytest.mark.parametrize("row_id", lc.ids_of("gail"))
def test_gail_learn_is_a_replay_of_its_rollouts(torch, row_id):
    import quadsim_amd as qa
    from quadsim_amd.gail import DISC_STAT_NAMES
    row = lc.BY_ID[row_id]
    n, T, K = row["n_envs"], row["n_steps"], row["kwargs"]
    n_batch, fused = n * T, bool(row["fused"])
    expert, train = make_expert(torch, row["expert"])
    env = lp.Recorded(make_env(row), after_reset=place(row))
    pol = qa.ActorCriticPolicy(pr.weight_set("sb2", row["layout"]), device=DEV)
    disc = qa.Discriminator(seed=row["disc_seed"], device=DEV)
    model = qa.GAIL(pol, env, expert, discriminator=disc, fused=row["fused"], seed=row["seed"], **K)
    assert model.runner.fused == fused
    snapshot = lambda: {"policy": lp.ppo2_snapshot(pol), "disc": lp.disc_snapshot(disc)}       # noqa: E731
    before = snapshot()
    rec = lp.Recorder(lp.LOOP_KEYS, snapshot)
    torch.manual_seed(row["seed"])                                             # the spelt-out roll-out samples from torch's generator
    logs = model.learn(2 * n_batch + 5, callback=rec)
    env.env.close()
    assert len(logs) == len(rec.updates) == 2 and (len(env.log) == 2 * T) == (not fused)
    first, second = rec.updates[0]["rollout"], rec.updates[1]["rollout"]
    check_episode_ends(first, second, n, T, row_id)
    # every update from the record: the PPO2 steps, then the discriminator's, the draws interleaved on the one generator in that order
    gen, cursor, pre, worst, worst_d = torch.Generator().manual_seed(row["seed"]), lp.CursorRef(train), before, np.zeros(3), 0.0
    for u in (1, 2):
        r = rec.updates[u - 1]
        idx = lp.draw_minibatches(n_batch, K["nminibatches"], K["noptepochs"], gen)
        gi, ei = lp.disc_schedule_ref(n_batch, cursor, K["d_batch"], K["d_steps"], gen)
        assert same_bits(r["gen_idx"], gi) and same_bits(r["exp_idx"], ei), "update %d: the discriminator's schedule" % u
        worst = np.maximum(worst, lp.check_ppo2_update(qa, row, u, 2, pre["policy"], r, idx, lc.EV_TOL, "hip", DEV))
        lp.check_values_of_obs(pre["policy"], r["rollout"], "%s roll-out %d" % (row_id, u))
        end, dstats, links = lp.disc_chain(qa, pre["disc"], r["rollout"][0], r["rollout"][3], expert, gi, ei, K["d_learning_rate"], "hip", DEV)
        bad = lp.disc_same_bits(end, r["after"]["disc"])
        assert not bad, "update %d: the discriminator's chain does not end in the loop's bits: %s" % (u, bad)
        assert same_bits(dstats, r["d_out"]["stats"])
        worst_d = max([worst_d] + [lp.disc_check_link(link, K["d_learning_rate"]) for link in links])
        lp.check_mean([r["log"][k] for k in DISC_STAT_NAMES], dstats, DEV, "update %d, the discriminator" % u)
        assert r["after"]["disc"]["rms"][2] == 1e-2 + u * 2 * K["d_steps"] * K["d_batch"] and r["after"]["disc"]["steps"] == u * K["d_steps"]
        pre = r["after"]
    assert cursor.shuffles == 2, "the expert's train rows did not run out inside the second update"
    print("loops ratio %s: gradients worst error / bound %.3g, statistics %.3g, update %.3g, discriminator %.3g" % (row_id, *worst, worst_d))
    # the second roll-out continues the first, is paid by the updated discriminator and reports the env's own reward
    twin = make_env(row)
    runner = qa.GailRunner(discriminator=lp.disc_restore(qa, before["disc"], DEV), env=twin, model=lp.ppo2_restore(qa, before["policy"], DEV),
                           n_steps=T, gamma=K["gamma"], lam=K["lam"], collect_ep_infos=False, fused=row["fused"])
    twin.set_state(t=lc.start_times(n, row["ends"]))
    torch.manual_seed(row["seed"])
    worst_gae = 0.0
    for k, (got, state) in enumerate(((first, before), (second, rec.updates[0]["after"]))):
        if k == 1:
            runner.model, runner.discriminator = lp.ppo2_restore(qa, state["policy"], DEV), lp.disc_restore(qa, state["disc"], DEV)
        bad = lp.tuples_same_bits(lp.Recorder._copy(runner.run()), got)
        assert not bad, "roll-out %d is not the twin's under the snapshot's policy and discriminator: %s" % (k + 1, bad)
        paid = lp.host(lp.disc_restore(qa, state["disc"], DEV).reward(lp.to_dev(got[0], DEV), lp.to_dev(got[3], DEV), n_envs=n, n_steps=T))
        assert same_bits(paid, lp.host(runner.last_reward)) and not same_bits(paid, step_major(got[8], n, T))
        assert rec.updates[k]["log"]["disc_reward_mean"] == float(lp.to_dev(paid, DEV).double().mean())
        assert abs(rec.updates[k]["log"]["disc_reward_mean"] - np.asarray(paid, np.float64).mean()) <= paid.size * lp.F64_EPS * np.abs(paid).mean()
        if not fused:                                                         # the env's own rewards, as its step() returned them
            true = np.stack([lp.host(e[2]) for e in env.log[k * T:(k + 1) * T]])
            assert same_bits(step_major(got[8], n, T), true), "roll-out %d: element 8 is not the env's reward" % (k + 1)
            with torch.no_grad():
                last_values = lp.host(runner.model.value(runner.obs, runner.states, runner.dones.bool()))
            worst_gae = max(worst_gae, check_gae_of(got, paid, last_values, lp.host(runner.dones), n, T, K["gamma"], K["lam"], "%s roll-out %d" % (row_id, k + 1)))
    twin.close()
    if fused:                                                                 # the fused roll-outs once more from a third handle, for their [T, N] arrays
        third = make_env(row)
        third.reset()
        third.set_state(t=lc.start_times(n, row["ends"]))
        dones = torch.zeros(n, dtype=torch.uint8, device=DEV)
        for k, (got, state) in enumerate(((first, before), (second, rec.updates[0]["after"]))):
            ro = qa.fused_runner_rollout(third, lp.ppo2_restore(qa, state["policy"], DEV), T, dones_in=dones, env_major=True)
            assert same_bits(lp.host(ro["obs"]).reshape(n * T, 12), got[0])
            assert same_bits(lp.host(ro["rewards"]), step_major(got[8], n, T)), "roll-out %d: element 8 is not the env's reward" % (k + 1)
            paid = lp.host(lp.disc_restore(qa, state["disc"], DEV).reward(lp.to_dev(got[0], DEV), lp.to_dev(got[3], DEV), n_envs=n, n_steps=T))
            worst_gae = max(worst_gae, check_gae_of(got, paid, lp.host(ro["last_values"]), lp.host(ro["last_dones"]), n, T, K["gamma"], K["lam"],
                                                    "%s roll-out %d" % (row_id, k + 1)))
            dones = ro["last_dones"]
        third.close()
    print("loops ratio %s: returns against GAE over the paid reward, worst error / (2^-24 scale) %.3g (kappa %.3g)" % (row_id, worst_gae, pp.KAPPA_GAE))


# ---------------------------------------------------------------------------------------------------- TRPO
@pytest.mark.parametrize("row_id", lc.ids_of("trpo"))
def test_trpo_learn_is_a_replay_of_its_rollouts(torch, row_id):
    import quadsim_amd as qa
    from quadsim_amd import trpo
    from quadsim_amd.gail import DISC_STAT_NAMES
    row = lc.BY_ID[row_id]
    K, n = row["kwargs"], row["n_envs"]
    T, n_batch = K["n_steps"], row["n_envs"] * K["n_steps"]
    expert, train, disc = None, None, None
    if row["expert"] is not None:
        expert, train = make_expert(torch, row["expert"])
        disc = qa.Discriminator(seed=row["disc_seed"], device=DEV)
    g_step = K.get("g_step", 1)
    env = make_env(row)
    pol = qa.ActorCriticPolicy(tr.weights(0.3), device=DEV)
    model = qa.TRPO(pol, env, seed=row["seed"], expert_data=expert, discriminator=disc, **K)
    runs = lp.record_runs(model.runner)
    snapshot = lambda: {"policy": lp.trpo_snapshot(pol), "disc": None if disc is None else lp.disc_snapshot(disc)}       # noqa: E731
    before = snapshot()
    rec = lp.Recorder(("update", "n_updates", "out", "vf", "log", "gen_idx", "exp_idx", "d_stats"), snapshot)
    logs = model.learn(row["updates"] * g_step * n_batch + 5, callback=rec)
    env.close()
    assert len(logs) == len(rec.updates) == row["updates"] and len(runs) == row["updates"] * g_step
    hp = {k: K[k] for k in ("max_kl", "cg_iters", "cg_damping", "entcoeff", "backtracks", "fvp_stride")}
    per = n_batch // K["vf_batch"]
    gen, cursor, pre, worst = torch.Generator().manual_seed(row["seed"]), None if train is None else lp.CursorRef(train), before, {}

    def merge(w):
        for k, r in w.items():
            worst[k] = max(worst.get(k, 0.0), r)
    for u in range(1, row["updates"] + 1):
        r = rec.updates[u - 1]
        chain = lp.trpo_restore(qa, pre["policy"], DEV)
        for j in range(g_step):
            ro = runs[(u - 1) * g_step + j]
            vf_idx = torch.stack([torch.randperm(n_batch, generator=gen)[:per * K["vf_batch"]].to(torch.int32) for _ in range(K["vf_iters"])])
            plink, vlinks = lp.trpo_generator_step(qa, chain, ro, vf_idx.view(K["vf_iters"] * per, K["vf_batch"]), hp, K["vf_stepsize"], DEV)
            merge(lp.trpo_check_policy_link(plink, hp, trpo.TRPO_RESIDUAL_TOL))
            for link in vlinks:
                merge(lp.trpo_check_vf_link(link, K["vf_stepsize"]))
        bad = lp.trpo_same_bits(lp.trpo_snapshot(chain), r["after"]["policy"])
        assert not bad, "update %d: the chain does not end in the loop's bits: %s" % (u, bad[:6])
        losses = np.array([link["loss"] for link in vlinks], np.float32)
        assert same_bits(plink["stats"], r["out"]["stats"]) and same_bits(losses, r["vf"]["stats"])       # the LAST generator step's
        log = r["log"]
        assert [log[k] for k in trpo.STAT_NAMES] == plink["stats"].astype(np.float64).tolist()
        lp.check_mean(log["vf_loss"], losses, DEV, "update %d, vf_loss" % u)
        assert (log["n_updates"], log["total_timesteps"]) == (u, u * g_step * n_batch)
        assert r["after"]["policy"]["steps"] == u * g_step * K["vf_iters"] * per                    # _trpo_steps goes on over the updates
        ev = lp.explained_variance64(ro[4], ro[1])
        assert abs(log["explained_variance"] - ev) <= lc.EV_TOL and lc.EV_TOL < 0.1 * abs(ev - lp.explained_variance64(ro[1], ro[4]))
        if expert is not None:
            gi, ei = lp.disc_schedule_ref(n_batch, cursor, K["d_batch"], K["d_step"], gen)
            assert same_bits(r["gen_idx"], gi) and same_bits(r["exp_idx"], ei), "update %d: the discriminator's schedule" % u
            end, dstats, links = lp.disc_chain(qa, pre["disc"], ro[0], ro[3], expert, gi, ei, K["d_stepsize"], "hip", DEV)     # the LAST roll-out's rows
            bad = lp.disc_same_bits(end, r["after"]["disc"])
            assert not bad, "update %d: the discriminator's chain does not end in the loop's bits: %s" % (u, bad)
            assert same_bits(dstats, r["d_stats"]) and log["entropy"] == float(plink["stats"][3])     # the policy's: the discriminator's has a key of its own
            lp.check_mean([log["disc_entropy" if k == "entropy" else k] for k in DISC_STAT_NAMES], dstats, DEV, "update %d, the discriminator" % u)
            merge({"discriminator": max(lp.disc_check_link(link, K["d_stepsize"]) for link in links)})
        pre = r["after"]
    assert cursor is None or cursor.shuffles == 2
    report(row_id, worst)
