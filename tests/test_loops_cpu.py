"""-m "not gpu": the record-and-replay recipe of the training loops (tests/loop_replay.py, tests/loop_cases.py) on the host paths, before
the device is held to it (tests/test_gpu_loops.py).

  accepted     every row of the table is accepted by its trainer's check_*_args, and names seams and known mutants
  DDPG, TD3    the rows run END TO END with update="torch" on CPU tensors against a small deterministic vec-env written here in torch:
               the ring, the c-th draw of the carried generator over the ring's size, the chain of single calls ending in the loop's
               bits, every link within the bounds of step64 (the torch paths are held to the same bounds by tests/test_gpu_ddpg.py and
               tests/test_gpu_td3.py), the logs, the behaviour actions with the twin noise, the delay phase and the keyed noise over
               the learn calls
  PPO2         PPO2.learn with update="torch" over a stub runner: the rates at frac, the schedule as the u-th draw, the chain ending in
               the loop's bits, the logs as the float64 means, explained_variance.  (The links' bounds belong to the device kernels.)
  pretrain     has no host path (quadsim_amd.bc): the reconstruction of the split and of every epoch's shuffle against
               ExpertData / epoch_schedule, and the float64 twins
  twins        the float64 references tell each row from its twin -- the rate of the next update, time-major rows, a schedule over
               the capacity, a restarted actor count, restarted noise keys, a dropped partial minibatch, a reused shuffle -- by at
               least 10 of their own bounds, the convention of tests/test_hyper_cases_cpu.py
  explained_variance   the float32 torch formula against float64 on fixtures of the recorded shapes: the figure in loop_cases
The separations and the measured figure are printed; profiles/loops/README.md has a copy."""
import numpy as np
import pytest
import torch

import bcfit_ref as br
import ddpg_ref as dd
import loop_cases as lc
import loop_replay as lp
import ppo2_ref as pr
import td3_ref as td

SEPARATION = 10.0


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("row", lc.ROWS, ids=[r["id"] for r in lc.ROWS])
def test_the_rows_are_accepted_by_the_trainers_checks(row):
    import quadsim_amd as qa
    from quadsim_amd import trpo
    assert row["seams"] or row["id"] == "ddpg-explore"
    assert all(m in lc.MUTANTS for m in row["mutants"])
    K = row.get("kwargs", {})
    if row["loop"] in ("ppo2", "gail"):
        n_batch = row["n_envs"] * row["n_steps"]
        assert n_batch % K["nminibatches"] == 0
        for frac in (1.0, 0.5):
            crv = -1.0 if K["cliprange_vf"] is None else K["cliprange_vf"](frac)
            qa.check_ppo2_args(n_batch, K["nminibatches"] * K["noptepochs"], n_batch // K["nminibatches"], 0, K["learning_rate"](frac),
                               K["cliprange"](frac), crv, K["ent_coef"], K["vf_coef"], K["max_grad_norm"])
        if row["loop"] == "gail":
            n_train = int(row["expert"]["train_fraction"] * row["expert"]["n"])
            qa.check_gail_args(n_batch, row["expert"]["n"], K["d_steps"], K["d_batch"], lr=K["d_learning_rate"])
            # the expert's train rows run out inside the second update
            assert K["d_batch"] <= n_train and K["d_steps"] * K["d_batch"] <= n_train < 2 * K["d_steps"] * K["d_batch"]
    elif row["loop"] == "trpo":
        n_batch = row["n_envs"] * K["n_steps"]
        qa.check_trpo_args(n_batch, 0, K["max_kl"], K["cg_iters"], K["cg_damping"], K["entcoeff"], K["backtracks"], K["fvp_stride"])
        trpo.check_vf_args(n_batch, K["vf_iters"] * (n_batch // K["vf_batch"]), K["vf_batch"], K["vf_stepsize"])
        if row["expert"] is not None:
            qa.check_gail_args(n_batch, row["expert"]["n"], K["d_step"], K["d_batch"], lr=K["d_stepsize"])
    elif row["loop"] == "ddpg":
        roll, steps, batch, cap = lp.off_shape(row)
        qa.check_ddpg_args(cap, steps, batch, **lp.off_hyper(row))
        assert row["cycles"] == 1 or row["n_envs"] * roll < cap < 2 * row["n_envs"] * roll      # the ring wraps, and not in the first cycle
    elif row["loop"] == "td3":
        roll, steps, batch, cap = lp.off_shape(row)
        qa.check_td3_args(cap, steps, batch, **lp.off_hyper(row))
        assert steps % K["policy_delay"] == 1                                                  # the delay phase straddles every learn call
    else:
        n_train = int(row["train_fraction"] * row["n"])
        per = -(-n_train // row["batch_size"])
        assert n_train % row["batch_size"] == 41
        t0 = 0
        for call in row["calls"]:
            qa.check_bc_args(row["n"], call["n_epochs"] * per, row["batch_size"], call["learning_rate"], eps=call["adam_epsilon"], t0=t0)
            t0 += call["n_epochs"] * per


def test_every_mutant_has_a_row():
    named = {m for r in lc.ROWS for m in r["mutants"]}
    assert named == set(lc.MUTANTS) and len(lc.MUTANTS) == 13


# ---------------------------------------------------------------------------------------------------- the stub env
class StubVecEnv:
    """a deterministic vec-env in torch on the host: x' = 0.9 x + 0.1 (a B) + c per env, the observation is the state, the reward a
    smooth function of both; the first episode of env i ends at step ends[i] (the others', and every later one, after `period`
    steps) and the env returns to its own initial state, as the device envs' auto-reset does"""

    def __init__(self, n, ends, seed=0, period=50):
        g = torch.Generator().manual_seed(seed)
        self.num_envs, self.device = n, torch.device("cpu")
        self.x0 = torch.randn((n, 12), generator=g) * 0.5
        self.B = torch.randn((4, 12), generator=g)
        self.c = torch.randn((12,), generator=g) * 0.05
        self.first = torch.full((n,), period, dtype=torch.int64)
        self.first[:len(ends)] = torch.as_tensor(ends)
        self.period = period

    def reset(self):
        self.x, self.left = self.x0.clone(), self.first.clone()
        return self.x.clone()

    def step(self, a):
        self.x = 0.9 * self.x + 0.1 * (a @ self.B) + self.c
        rew = -(self.x ** 2).mean(1) + 0.1 * a.sum(1)
        self.left = self.left - 1
        done = self.left <= 0
        self.x = torch.where(done[:, None], self.x0, self.x)
        self.left = torch.where(done, torch.full_like(self.left, self.period), self.left)
        return self.x.clone(), rew, done, {}

    def close(self):
        pass


_records = {}


def off_record(row_id):
    """the host run of an off-policy row, made once and left unchanged"""
    import quadsim_amd as qa
    if row_id not in _records:
        row = lc.BY_ID[row_id]
        env = lp.Recorded(StubVecEnv(row["n_envs"], row["ends"], seed=row["env_seed"]))
        _records[row_id] = lp.run_off_policy(qa, row, env, "torch", "cpu")
    return _records[row_id]


# ---------------------------------------------------------------------------------------------------- DDPG and TD3 end to end
@pytest.mark.parametrize("row_id", ["ddpg", "td3-keyed", "td3-caller"])
def test_off_policy_rows_replay_on_the_host(row_id):
    import quadsim_amd as qa
    row, rec = lc.BY_ID[row_id], off_record(row_id)
    worst = lp.check_off_policy(qa, row, rec, "torch", "cpu")
    lp.check_behaviour_actions(qa, row, rec, "cpu")
    top = max(worst, key=worst.get)
    print("loops cpu %s: worst error / bound %.3g (%s)" % (row_id, worst[top], top))


def test_uniform_exploration_replaces_every_action_on_the_host():
    import quadsim_amd as qa
    row, rec = lc.BY_ID["ddpg-explore"], off_record("ddpg-explore")
    lp.check_behaviour_actions(qa, row, rec, "cpu")
    assert rec["snaps"][1]["steps"] == row["kwargs"]["nb_train_steps"]


def test_a_wrong_record_fails_the_replay():
    """the checks are not vacuous: a ring whose obs0 is obs1 (mutant 8), a schedule drawn over the capacity (10), a restarted actor
    count (11) and a dropped noise reset (9), put into copies of the host records, are each refused"""
    import quadsim_amd as qa
    row, rec = lc.BY_ID["ddpg"], off_record("ddpg")
    bad = dict(rec, rings=[dict(r, data=(r["data"][3],) + r["data"][1:]) for r in rec["rings"]])
    with pytest.raises(AssertionError, match="the ring is not"):
        lp.check_off_policy(qa, row, bad, "torch", "cpu")
    roll, steps, batch, cap = lp.off_shape(row)
    gen = torch.Generator().manual_seed(row["seed"])
    idx = torch.randint(0, cap, (steps, batch), generator=gen, dtype=torch.int32)
    end, _, _ = lp.off_chain(qa, "ddpg", rec["snaps"][0], rec["rings"][0], idx.clamp(max=rec["rings"][0]["size"] - 1), lp.off_hyper(row), "torch", "cpu")
    assert lp.off_same_bits(end, rec["snaps"][1], "ddpg")
    trow, trec = lc.BY_ID["td3-keyed"], off_record("td3-keyed")
    _, tsteps, tbatch, _ = lp.off_shape(trow)
    gen = torch.Generator().manual_seed(trow["seed"])
    torch.randint(0, trec["rings"][0]["size"], (tsteps, tbatch), generator=gen, dtype=torch.int32)
    idx = torch.randint(0, trec["rings"][1]["size"], (tsteps, tbatch), generator=gen, dtype=torch.int32)
    for start, same in ((trec["snaps"][1], True), (dict(trec["snaps"][1], actor_steps=0), False)):
        end, _, _ = lp.off_chain(qa, "td3", start, trec["rings"][1], idx, lp.off_hyper(trow), "torch", "cpu", seed=trow["seed"])
        bad = lp.off_same_bits(end, trec["snaps"][2], "td3")
        assert (not bad) == same and (same or ("w", "actor", "w1") in bad)

    class NoReset(qa.OUNoise):
        def reset(self, done=None):
            pass
    other = type("QA", (), dict(DDPGPolicy=qa.DDPGPolicy, TD3Policy=qa.TD3Policy, OUNoise=NoReset))
    with pytest.raises(AssertionError, match="twin noise"):
        lp.check_behaviour_actions(other, row, rec, "cpu")


# ---------------------------------------------------------------------------------------------------- PPO2 over a stub runner
class StubRunner:
    """run() -> the 9-tuple of Runner.run() on the host, drawn from a generator of its own: a fresh policy's scale of values and
    returns, actions sampled around the policy's own mean so that the ratios start at 1"""

    def __init__(self, policy, n_envs, n_steps, seed):
        self.policy, self.n, self.g, self.runs = policy, n_envs * n_steps, torch.Generator().manual_seed(seed), []

    def run(self):
        obs = torch.randn((self.n, 12), generator=self.g) * 0.5
        with torch.no_grad():
            u, values, _, nl = self.policy.step(obs, noise=torch.randn((self.n, 4), generator=self.g))
        rew = torch.randn((self.n,), generator=self.g) * 0.3
        out = (obs, values + rew - 0.5, torch.zeros(self.n), u, values, nl, None, [], rew)
        self.runs.append(out)
        return out


class StubEnv:
    device = torch.device("cpu")

    def __init__(self, n):
        self.num_envs = n


@pytest.mark.parametrize("row_id", lc.ids_of("ppo2"))
def test_ppo2_learn_replays_on_the_host(row_id):
    import quadsim_amd as qa
    row = lc.BY_ID[row_id]
    n_batch = row["n_envs"] * row["n_steps"]
    pol = qa.ActorCriticPolicy({k: np.array(v) for k, v in pr.weight_set("sb2", row["layout"]).items()}, device="cpu")     # (a host tensor aliases its array: the fixture stays as it is)
    model = qa.PPO2(pol, StubEnv(row["n_envs"]), n_steps=row["n_steps"], seed=row["seed"], update="torch",
                    runner=StubRunner(pol, row["n_envs"], row["n_steps"], row["env_seed"]), **row["kwargs"])
    before = lp.ppo2_snapshot(pol)
    rec = lp.Recorder(lp.LOOP_KEYS, lambda: lp.ppo2_snapshot(pol))
    logs = model.learn(2 * n_batch + 5, callback=rec)
    assert len(logs) == len(rec.updates) == 2 and model.num_timesteps == 2 * n_batch
    gen = torch.Generator().manual_seed(row["seed"])
    for u in (1, 2):
        idx = lp.draw_minibatches(n_batch, row["kwargs"]["nminibatches"], row["kwargs"]["noptepochs"], gen)
        lp.check_ppo2_update(qa, row, u, 2, before, rec.updates[u - 1], idx, lc.EV_TOL, "torch", "cpu", bounds=False)
        before = rec.updates[u - 1]["after"]
    assert logs[1]["learning_rate"] == lc.lr_of(0.5) and logs[0]["learning_rate"] == lc.lr_of(1.0)


# ---------------------------------------------------------------------------------------------------- pretrain: the reconstruction
def test_the_pretrain_schedule_is_reconstructed():
    """split_rows is ExpertData's split; epoch_rows over ONE generator is pretrain's sequence of epoch_schedule calls, the partial
    minibatch of 41 rows kept; two epochs' shuffles differ"""
    import quadsim_amd as qa
    row = lc.BY_ID["pretrain"]
    obs, act = lc.pretrain_data(row)
    data = qa.ExpertData({"obs": obs, "actions": act}, train_fraction=row["train_fraction"], batch_size=row["batch_size"], seed=row["split_seed"],
                         device="cpu")
    train, val = lp.split_rows(row["n"], row["train_fraction"], row["split_seed"])
    assert np.array_equal(train, data.train_rows.numpy()) and np.array_equal(val, data.val_rows.numpy()) and len(train) == 105 and len(val) == 45
    call = row["calls"][0]
    theirs, mine = torch.Generator().manual_seed(call["seed"]), torch.Generator().manual_seed(call["seed"])
    epochs = []
    for _ in range(call["n_epochs"]):
        pos, counts = qa.epoch_schedule(data.n_train, data.batch_size, 1, theirs)
        rows = data.train_rows[pos.long()].numpy()
        steps = lp.epoch_rows(train, row["batch_size"], mine)
        assert [len(s) for s in steps] == counts.tolist() == [64, 41]
        assert all(np.array_equal(s, rows[i, :len(s)]) for i, s in enumerate(steps))
        epochs.append(np.concatenate(steps))
    assert all(sorted(e) == sorted(train) for e in epochs) and not np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[1], epochs[2])


# ---------------------------------------------------------------------------------------------------- the twins
def _median_sep(a, b, bound):
    return float(np.median(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / bound))


def test_the_ppo2_reference_tells_the_rate_and_the_row_order_from_their_twins():
    row = lc.BY_ID["ppo2-shared-t10-novclip"]
    W, data = pr.weight_set("sb2", "shared"), {k: v[:60] for k, v in pr.rollout("sb2", "shared").items()}
    M, V = pr.moments(W)
    kw, twin = lp.ppo2_kw(row, 2, 2), lp.ppo2_kw(row, 3, 2)             # update 2, and what update 2 gets where frac is one update late
    assert kw["learning_rate"] == lc.lr_of(0.5) and twin["learning_rate"] == lc.lr_of(0.0)
    rows = np.arange(15, 30)
    mb = pr.minibatch(data, rows)
    hp, hp_twin = lp.ppo2_hp(kw), lp.ppo2_hp(twin)
    _, G = pr.backward64(W, mb, hp)
    G32 = {k: g.astype(np.float32) for k, g in G.items()}
    Wn, UB, Wt = pr.update64(W, M, V, G32, hp, 9)[0], pr.update_bound(W, M, V, G32, hp, 9), pr.update64(W, M, V, G32, hp_twin, 9)[0]
    sep = min(_median_sep(Wn[k], Wt[k], UB[k][0]) for k in G)
    print("loops separation ppo2 rate of update 2 against update 3's: %.3g bounds" % sep)
    assert sep >= SEPARATION
    # env-major rows against the same flat array read time-major: the observations of another (env, step) under the same index
    n_envs, T = row["n_envs"], row["n_steps"]
    tm = dict(data, obs=np.ascontiguousarray(data["obs"].reshape(n_envs, T, 12).swapaxes(0, 1)).reshape(n_envs * T, 12))
    st, _, SB, _ = pr.backward64(W, mb, hp, with_bound=True)
    st_twin = pr.backward64(W, pr.minibatch(tm, rows), hp)[0]
    sep = float(np.max(np.abs(st - st_twin)[:4] / SB[:4]))
    print("loops separation ppo2 env-major against time-major observations: %.3g bounds" % sep)
    assert sep >= SEPARATION


def test_the_off_policy_references_tell_the_schedule_the_count_and_the_keys_from_their_twins():
    row, rec = lc.BY_ID["ddpg"], off_record("ddpg")
    roll, steps, batch, cap = lp.off_shape(row)
    hyper, ring, P = lp.off_hyper(row), rec["rings"][0], rec["snaps"][0]["w"]
    assert ring["size"] < cap
    right = torch.randint(0, ring["size"], (steps, batch), generator=torch.Generator().manual_seed(row["seed"]), dtype=torch.int32).numpy()
    wrong = torch.randint(0, cap, (steps, batch), generator=torch.Generator().manual_seed(row["seed"]), dtype=torch.int32).numpy()
    assert (wrong[0] >= ring["size"]).any() or not np.array_equal(right[0], wrong[0])
    st, _, _, Es, _ = dd.step64(P, tuple(a[right[0]] for a in ring["data"]), gam=hyper["gamma"], clip=hyper["obs_clip"], with_bound=True)
    st_twin = dd.step64(P, tuple(a[wrong[0]] for a in ring["data"]), gam=hyper["gamma"], clip=hyper["obs_clip"])[0]
    sep = float(np.max(np.abs(st - st_twin) / Es))
    print("loops separation ddpg schedule over the size against over the capacity: %.3g bounds" % sep)
    assert sep >= SEPARATION
    # TD3, the first update of the second learn call (u = 3 is critic-only; u = 4 steps the actor at its count 2 + 1)
    trow, trec = lc.BY_ID["td3-keyed"], off_record("td3-keyed")
    th = lp.off_hyper(trow)
    _, tsteps, tbatch, _ = lp.off_shape(trow)
    gen = torch.Generator().manual_seed(trow["seed"])
    torch.randint(0, trec["rings"][0]["size"], (tsteps, tbatch), generator=gen, dtype=torch.int32)
    idx = torch.randint(0, trec["rings"][1]["size"], (tsteps, tbatch), generator=gen, dtype=torch.int32)
    _, _, links = lp.off_chain(__import__("quadsim_amd"), "td3", trec["snaps"][1], trec["rings"][1], idx, th, "torch", "cpu", seed=trow["seed"])
    link = links[1]
    assert link["pre"]["steps"] == 4 and link["pre"]["actor_steps"] == 2
    seps = []
    for k in td.KEYS:
        a = (link["pre"]["w"]["actor"][k], link["pre"]["m"]["actor"][k], link["pre"]["v"]["actor"][k], link["grads"]["actor"][k])
        seps.append(_median_sep(td.adam64(*a, 3, th["actor_lr"])[0], td.adam64(*a, 1, th["actor_lr"])[0], td.adam_bound(*a, 3, th["actor_lr"])[0]))
    print("loops separation td3 actor's Adam step 3 against a restarted count's step 1: %.3g bounds" % min(seps))
    assert min(seps) >= SEPARATION
    # the keys: what a link holds is the normals themselves, within NORMAL_ABS of those of (seed, the carried update index, the slot)
    z, z_twin = td.normals64(trow["seed"], 3, 1, tbatch)[0], td.normals64(trow["seed"], 0, 1, tbatch)[0]
    sep = _median_sep(z, z_twin, lp.NORMAL_ABS)
    print("loops separation td3 noise keys of update 3 against a restarted call's update 0: %.3g bounds" % sep)
    assert sep >= SEPARATION and links[0]["pre"]["steps"] == 3


def test_the_pretrain_reference_tells_the_partial_minibatch_and_the_shuffle_from_their_twins():
    row = lc.BY_ID["pretrain"]
    obs, act = lc.pretrain_data(row)
    call = row["calls"][0]
    train, _ = lp.split_rows(row["n"], row["train_fraction"], row["split_seed"])
    gen = torch.Generator().manual_seed(call["seed"])
    e1, e2 = lp.epoch_rows(train, row["batch_size"], gen), lp.epoch_rows(train, row["batch_size"], gen)
    W, Z = br.weight_set("sb2"), br.zero_state()
    lr, eps = call["learning_rate"], call["adam_epsilon"]

    def fit(steps, W=W, M=Z, V=Z, t0=0):
        idx = np.zeros((len(steps), row["batch_size"]), np.int64)
        for i, s in enumerate(steps):
            idx[i, :len(s)] = s
        return br.fit64(W, M, V, obs, act, idx, counts=[len(s) for s in steps], t0=t0, lr=lr, eps=eps)
    W1, M1, V1, _ = fit(e1[:1])
    # the partial minibatch: the second step of the epoch against none
    rows = e1[1]
    _, G = br.backward64(W1, obs[rows], act[rows])
    seps = [_median_sep(br.adam64(W1[k], M1[k], V1[k], G[k], 2, lr, br.BETA1, br.BETA2, eps)[0], W1[k],
                        br.adam_bound(W1[k], M1[k], V1[k], G[k], 2, lr, br.BETA1, br.BETA2, eps)[0]) for k in br.KEYS]
    print("loops separation pretrain with the partial minibatch against without: %.3g bounds" % min(seps))
    assert min(seps) >= SEPARATION
    # a fresh shuffle against the first epoch's once more: the loss of epoch 2's first step
    W2 = fit(e1)[0]
    loss, _, lb, _ = br.backward64(W2, obs[e2[0]], act[e2[0]], with_bound=True)
    loss_twin = br.backward64(W2, obs[e1[0]], act[e1[0]])[0]
    print("loops separation pretrain epoch 2 on its own shuffle against epoch 1's: %.3g bounds" % (abs(loss - loss_twin) / lb))
    assert abs(loss - loss_twin) / lb >= SEPARATION


# ---------------------------------------------------------------------------------------------------- explained_variance
def test_explained_variance_in_float32_against_float64():
    """the figure loop_cases.EV_MEASURED: the largest error of the float32 torch formula over the fixtures, and what eight times it is
    worth against the swapped-argument twin"""
    from quadsim_amd.ppo2 import explained_variance
    worst, nearest = 0.0, np.inf
    for n in lc.EV_SHAPES:
        for seed in lc.EV_SEEDS:
            values, returns = lc.ev_fixture(n, seed)
            got = float(explained_variance(torch.as_tensor(values), torch.as_tensor(returns)))
            want = lp.explained_variance64(values, returns)
            worst = max(worst, abs(got - want))
            nearest = min(nearest, abs(want - lp.explained_variance64(returns, values)))
    print("loops explained_variance: float32 against float64 worst %.3g (recorded %.3g), tolerance %.3g, nearest swapped twin %.3g" % (
        worst, lc.EV_MEASURED, lc.EV_TOL, nearest))
    assert 0.5 * lc.EV_MEASURED <= worst <= lc.EV_MEASURED and lc.EV_TOL < 0.1 * nearest
    assert np.isnan(float(explained_variance(torch.zeros(4), torch.ones(4))))
