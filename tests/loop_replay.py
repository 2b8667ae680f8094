"""Record and replay: what the tests of the training loops (tests/test_gpu_loops.py, tests/test_loops_cpu.py) have in common.  A
helper module, not a conftest and not a test: imported where it is needed.

A loop run is recorded with hooks the public API offers -- the ``callback(locals_, globals_)`` of PPO2, GAIL and TRPO (Recorder), an
env wrapper (Recorded), a wrapped ``runner.run`` (record_runs), one ``learn`` call per cycle with snapshots in between -- and every
update is then replayed from the record in two ways:

  the chain    a FRESH policy built from the snapshot taken before the update (weights, Adam's moments, step counts) is given the
               recorded roll-out or ring and a schedule that the test draws itself from its own ``torch.Generator(seed)``, and runs
               the update ONE step per call.  The chain must end in the loop's own bits
  the links    every single step of the chain starts from device weights the test holds, so the trainer's one-step float64 recipe
               and its derived bounds apply as they stand: ppo2_ref.backward64 / update64 / update_bound, ddpg_ref.step64,
               td3_ref.step64 with E_z = NORMAL_ABS, bcfit_ref.backward64 / adam_bound, gail_ref, trpo_ref.  No tolerance is
               introduced here

A recorded minibatch is not a chosen fixture: among its few thousand hidden pre-activations one now and then lies within its forward
bound of zero, where float32 may take the other side of the ReLU.  The references cover that themselves: at such an element the bound
of the back-propagated dz is |dz without the mask| + its bound, either side (ddpg_ref._masked, and the same in ppo2_ref, bcfit_ref and
trpo_ref; at every other element the bounds are what the one-step fixtures, which have no such element, are held to).  The decisions
The value head's clip is covered in the same way (ppo2_ref.head64: a value step within its bound of the clip range, two losses within
their bounds of each other -- a value net that moves 0.06 a step crosses a clip range of 0.2 with every row, and lands within a
forward bound of 1e-4 of it with one row in a few hundred).  The decisions of PPO2's policy head (the ratio at 1 +- eps, an advantage
at zero) have no such cover: a link asserts that its minibatch has no row within its bound of one (ppo2_ref.edge_counts), and a row
of the table at which that fails, fails.
"""
import numpy as np
import torch

import actor_numerics as an
import bcfit_ref as br
import ddpg_ref as dd
import gail_ref as gr
import ppo2_ref as pr
import td3_ref as td
import trpo_ref as tr
from side_cases import same_bits

KEYS = dd.KEYS
NORMAL_ABS = 6.8e-6          # |device normal - float64 Box-Muller on the same words|: the bound tests/test_gpu_mppi.py asserts for normals_from_words
F64_EPS = 2.0 ** -52


def host(t):
    return t.detach().cpu().numpy().copy()


def to_dev(a, device):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device)


def mean64(stats):
    """the float64 mean over the steps of a call's statistics [steps, ...], numpy's"""
    return np.asarray(stats, np.float64).sum(0) / np.asarray(stats).shape[0]


def check_mean(got, stats, device, what=""):
    """`got` (a float, or a list of them) is the loop's ``stats.double().mean(0)`` of the float32 statistics [steps, ...]: EXACTLY what
    that reduction gives for the chain's statistics on the same device (its order of additions is the device's, not numpy's, and an
    approxkl of 1e-14 beside one of 1e-3 makes the order show in the last bit), and within the bound of any float64 summation of n
    terms, n 2^-52 mean|x|, of numpy's mean"""
    x = np.asarray(stats, np.float32)
    same = to_dev(x, device).double()
    same = float(same.mean()) if x.ndim == 1 else same.mean(0).tolist()
    assert got == same, (what, got, same)
    err = np.abs(np.asarray(got, np.float64) - mean64(x))
    assert np.all(err <= x.shape[0] * F64_EPS * np.abs(x.astype(np.float64)).mean(0)), (what, got, mean64(x))


# ---------------------------------------------------------------------------------------------------- the hooks
class Recorded:
    """an env that keeps a copy of everything its step() was given and returned; `after_reset(env)` runs after every reset (the place
    to move envs near a limit with set_state)"""

    def __init__(self, env, after_reset=None):
        self.env, self.log, self.first, self.after_reset = env, [], None, after_reset

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self):
        obs = self.env.reset()
        if self.after_reset is not None:
            self.after_reset(self.env)
        self.first = obs.clone()
        return self.first

    def step(self, a):
        obs, rew, done, info = self.env.step(a)
        self.log.append((a.clone(), obs.clone(), rew.clone(), done.clone()))
        return obs, rew, done, info


class Recorder:
    """the ``callback(locals_, globals_)`` of PPO2, GAIL and TRPO: per update a copy of the loop's locals named in `keys` (tensors as
    host arrays, tuples and dicts of tensors likewise) and `snapshot()`, the policy's training state after the update"""

    def __init__(self, keys, snapshot):
        self.keys, self.snapshot, self.updates = tuple(keys), snapshot, []

    @staticmethod
    def _copy(x):
        if isinstance(x, torch.Tensor):
            return host(x)
        if isinstance(x, (tuple, list)):
            return type(x)(Recorder._copy(v) for v in x)
        if isinstance(x, dict):
            return {k: Recorder._copy(v) for k, v in x.items()}
        return x

    def __call__(self, locals_, globals_):
        rec = {k: self._copy(locals_[k]) for k in self.keys if k in locals_}
        rec["after"] = self.snapshot()
        self.updates.append(rec)
        return True


def record_runs(runner):
    """wrap ``runner.run`` (an instance attribute: the class is left alone) -> the list that every run's result is appended to, as
    host arrays"""
    runs, run = [], runner.run

    def recorded(*a, **kw):
        out = run(*a, **kw)
        runs.append(Recorder._copy(out))
        return out
    runner.run = recorded
    return runs


# ---------------------------------------------------------------------------------------------------- DDPG and TD3
OFF = {"ddpg": dict(nets=dd.NETS, online=("actor", "critic"), counters=("steps",)),
       "td3": dict(nets=td.NETS, online=td.ONLINE, counters=("steps", "actor_steps"))}


def off_snapshot(pol, kind):
    """the training state of a DDPGPolicy / TD3Policy as host arrays: every net, Adam's moments, the step counts"""
    S = OFF[kind]
    snap = {"w": {n: {k: host(w) for k, w in zip(KEYS, getattr(pol, n))} for n in S["nets"]},
            "m": {n: {k: host(t) for k, t in zip(KEYS, pol.m[n])} for n in S["online"]},
            "v": {n: {k: host(t) for k, t in zip(KEYS, pol.v[n])} for n in S["online"]}}
    snap.update({c: int(getattr(pol, c)) for c in S["counters"]})
    return snap


def off_restore(qa, kind, snap, device):
    """a fresh policy with the snapshot's state"""
    S = OFF[kind]
    pol = (qa.DDPGPolicy if kind == "ddpg" else qa.TD3Policy)(device=device, weights=snap["w"])
    for n in S["online"]:
        pol.m[n] = [to_dev(snap["m"][n][k].copy(), pol.device) for k in KEYS]
        pol.v[n] = [to_dev(snap["v"][n][k].copy(), pol.device) for k in KEYS]
    for c in S["counters"]:
        setattr(pol, c, snap[c])
    return pol


def off_same_bits(a, b, kind):
    S = OFF[kind]
    bad = [(p, n, k) for p in ("w", "m", "v") for n in a[p] for k in KEYS if not same_bits(a[p][n][k], b[p][n][k])]
    bad += [c for c in S["counters"] if a[c] != b[c]]
    return bad


def ring_snapshot(rb):
    return {"data": tuple(host(t) for t in rb.tensors()), "size": int(rb.size), "pos": int(rb.pos)}


def expected_ring(env, capacity, steps=None):
    """what the ring must hold after the first `steps` steps that `env` (a Recorded) has logged (None: all): the five arrays of those
    transitions in order, and for the last `capacity` of them the row each lies in -> (arrays, transition numbers, rows)"""
    n = int(env.first.shape[0])
    log = env.log if steps is None else env.log[:steps]
    obs0 = torch.cat([env.first] + [e[1] for e in log[:-1]])
    act, obs1 = torch.cat([e[0] for e in log]), torch.cat([e[1] for e in log])
    rew, done = torch.cat([e[2] for e in log]), torch.cat([e[3] for e in log]).float()
    total = n * len(log)
    which = np.arange(max(0, total - capacity), total)
    return tuple(host(t) for t in (obs0, act, rew, obs1, done)), which, which % capacity


def off_chain(qa, kind, snap, ring, indices, hyper, update, device, seed=0, noise=None):
    """the update of one cycle as a chain of single calls on a fresh policy: `indices` [steps, batch] int32 (host) over the ring's
    snapshot; TD3: `seed` keys the target noise (the policy's carried step count is the key's update index), or `noise` [steps,
    batch, 4] is the caller's -> (the snapshot at the chain's end, statistics [steps, k] float32, the links)"""
    S = OFF[kind]
    pol = off_restore(qa, kind, snap, device)
    data = tuple(to_dev(a, pol.device) for a in ring["data"])
    fn = {("ddpg", "hip"): qa.ddpg_update, ("ddpg", "torch"): qa.torch_ddpg_update, ("td3", "hip"): qa.td3_update,
          ("td3", "torch"): qa.torch_td3_update}[(kind, update)]
    links = []
    for s in range(int(indices.shape[0])):
        pre = off_snapshot(pol, kind)
        kw = {}
        if kind == "td3":
            kw = dict(seed=seed, noise=None if noise is None else noise[s:s + 1].contiguous(), return_noise=True)
        out = fn(pol, data, indices[s:s + 1], return_grads=True, **hyper, **kw)
        grads = {n: None if out["grads"][n] is None else {k: host(g) for k, g in zip(KEYS, out["grads"][n])} for n in S["online"]}
        rows = indices[s].numpy().astype(np.int64)
        links.append(dict(pre=pre, post=off_snapshot(pol, kind), rows=tuple(a[rows] for a in ring["data"]), grads=grads,
                          stats=host(out["stats"])[0].astype(np.float32), noise=host(out["noise"])[0] if kind == "td3" else None))
    return off_snapshot(pol, kind), np.stack([l["stats"] for l in links]), links


def _adam_ratios(ref, link, n, k, t, lr, names, worst):
    P, M, V, g = link["pre"]["w"][n][k], link["pre"]["m"][n][k], link["pre"]["v"][n][k], link["grads"][n][k]
    want, bounds = ref.adam64(P, M, V, g, t, lr), ref.adam_bound(P, M, V, g, t, lr)
    for name, x64, b in zip("wmv", want, bounds):
        if name in names:
            key = "adam %s %s" % (name, n)
            worst[key] = max(worst.get(key, 0.0), float((np.abs(link["post"][name][n][k].astype(np.float64) - x64) / b).max()))


def ddpg_check_link(link, hyper, update="hip"):
    """one DDPG step of a chain against ddpg_ref: the statistics and the twelve gradients within the bounds of step64 on the
    link's rows, w, m, v (the torch path: w, as tests/test_gpu_ddpg.py holds it) within adam_bound of adam64 on the link's OWN
    gradient, the targets the header's formula bit for bit (the device path) -> {quantity: worst error / bound}"""
    P, t = link["pre"]["w"], link["pre"]["steps"] + 1
    stats, G, _, Es, E = dd.step64(P, link["rows"], gam=hyper["gamma"], clip=hyper["obs_clip"], with_bound=True)
    worst = {name: float(e / b) for name, e, b in zip(dd.STAT_NAMES, np.abs(link["stats"].astype(np.float64) - stats), Es)}
    for n, lr in (("actor", hyper["actor_lr"]), ("critic", hyper["critic_lr"])):
        for k in KEYS:
            worst["grad %s %s" % (n, k)] = float((np.abs(link["grads"][n][k].astype(np.float64) - G[n][k]) / E[n][k]).max())
            _adam_ratios(dd, link, n, k, t, lr, "wmv" if update == "hip" else "w", worst)
            if update == "hip":
                assert same_bits(link["post"]["w"][n + "_target"][k], dd.polyak32(P[n + "_target"][k], link["post"]["w"][n][k], hyper["tau"])), (n, k)
    assert link["post"]["steps"] == t
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r < 1.0}
    return worst


def td3_check_link(link, hyper, seed, update="hip"):
    """one TD3 step of a chain against td3_ref: the normals that were used are those of (seed, the carried update index, the slot)
    within NORMAL_ABS of float64 Box-Muller; the statistics and the gradients within the bounds of step64 with E_z = NORMAL_ABS; w,
    m, v within adam_bound on the link's own gradient, the critics at Adam step u + 1 and the actor at its own count; a critic-only
    update leaves the actor, its moments and the three targets bit for bit -> {quantity: worst error / bound}"""
    P, u, ta = link["pre"]["w"], link["pre"]["steps"], link["pre"]["actor_steps"]
    act = bool(td.actor_step(u, hyper["policy_delay"]))
    batch = link["rows"][0].shape[0]
    z = td.normals64(seed, u, 1, batch)[0]
    worst = {"normals": float(np.abs(link["noise"].astype(np.float64) - z).max() / NORMAL_ABS)}
    stats, G, _, Es, E = td.step64(P, link["rows"], z, gam=hyper["gamma"], sigma=hyper["target_policy_noise"], clip=hyper["target_noise_clip"],
                                   actor=act, with_bound=True, E_z=NORMAL_ABS)
    err = np.abs(link["stats"].astype(np.float64) - stats)
    for i, name in enumerate(td.STAT_NAMES):
        if act or i < 5:
            worst[name] = float(err[i] / Es[i])
    for n in (td.ONLINE if act else ("q1", "q2")):
        t, lr = (ta + 1, hyper["actor_lr"]) if n == "actor" else (u + 1, hyper["critic_lr"])
        for k in KEYS:
            worst["grad %s %s" % (n, k)] = float((np.abs(link["grads"][n][k].astype(np.float64) - G[n][k]) / E[n][k]).max())
            _adam_ratios(td, link, n, k, t, lr, "wmv" if update == "hip" else "w", worst)
            if act and update == "hip":
                assert same_bits(link["post"]["w"][n + "_target"][k], td.polyak32(P[n + "_target"][k], link["post"]["w"][n][k], hyper["tau"])), (n, k)
    if not act:
        assert link["grads"]["actor"] is None and float(link["stats"][5]) == 0.0
        for n in ("actor", "actor_target", "q1_target", "q2_target"):
            assert all(same_bits(link["post"]["w"][n][k], P[n][k]) for k in KEYS), n
        assert all(same_bits(link["post"][p]["actor"][k], link["pre"][p]["actor"][k]) for p in "mv" for k in KEYS)
    assert link["post"]["steps"] == u + 1 and link["post"]["actor_steps"] == ta + int(act)
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r < 1.0}
    return worst


def episode_conditions(dones, roll):
    """dones [steps, n] of a record cut into cycles of `roll` steps -> (an episode ends strictly inside a cycle, an env is in
    mid-episode at a cycle's last step while another cycle follows)"""
    d = np.asarray(dones).astype(bool)
    cycles = d.shape[0] // roll
    inside = any(d[c * roll:(c + 1) * roll - 1].any() for c in range(cycles))
    mid = any((~d[(c + 1) * roll - 1]).any() for c in range(cycles - 1))
    return inside, mid


# ---------------------------------------------------------------------------------------------------- behaviour cloning
def bc_snapshot(pol):
    """the actor's six tensors, the moments of the pretrain optimiser (zeros before its first step) and its step count"""
    w = {k: host(getattr(pol, k)) for k in br.KEYS}
    has = getattr(pol, "_bc_m", None) is not None
    m = {k: host(t) if has else np.zeros_like(w[k]) for k, t in zip(br.KEYS, pol._bc_m if has else br.KEYS)}
    v = {k: host(t) if has else np.zeros_like(w[k]) for k, t in zip(br.KEYS, pol._bc_v if has else br.KEYS)}
    return {"w": w, "m": m, "v": v, "steps": int(getattr(pol, "_bc_steps", 0) or 0)}


def bc_restore(qa, W, snap, device):
    """a fresh ActorCriticPolicy: the weights `W` with the snapshot's actor, moments and step count"""
    pol = qa.ActorCriticPolicy({k: np.array(v) for k, v in dict(W, **snap["w"]).items()}, device=device)      # (copies: a host tensor aliases its array)
    pol._bc_m = [to_dev(snap["m"][k].copy(), device) for k in br.KEYS]
    pol._bc_v = [to_dev(snap["v"][k].copy(), device) for k in br.KEYS]
    pol._bc_steps = snap["steps"]
    return pol


def bc_same_bits(a, b):
    return [(p, k) for p in ("w", "m", "v") for k in br.KEYS if not same_bits(a[p][k], b[p][k])] + (["steps"] if a["steps"] != b["steps"] else [])


def split_rows(n, train_fraction, seed):
    """ExpertData's split restated: one permutation from `seed`, its first int(train_fraction n) entries train -> (train, val)"""
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).numpy()
    k = max(1, int(train_fraction * n))
    return perm[:k], perm[k:]


def epoch_rows(train_rows, batch_size, generator):
    """one epoch of pretrain restated: a fresh shuffle of the train positions from `generator`, cut into consecutive minibatches,
    the partial last one kept -> a list of arrays of dataset rows"""
    pos = torch.randperm(len(train_rows), generator=generator).numpy()
    return [train_rows[pos[s:s + batch_size]] for s in range(0, len(pos), batch_size)]


def bc_chain(qa, W, snap, obs, act, steps, batch_size, lr, eps, device):
    """`steps`: a list of arrays of dataset rows; one bc_fit call per step (the rows padded to `batch_size`, with their count) on a
    fresh policy -> (the snapshot at the end, the steps' losses, the links)"""
    pol = bc_restore(qa, W, snap, device)
    o, a = to_dev(obs, device), to_dev(act, device)
    links = []
    for rows in steps:
        idx = np.zeros((1, batch_size), np.int32)
        idx[0, :len(rows)] = rows
        pre = bc_snapshot(pol)
        out = qa.bc_fit(pol, o, a, torch.as_tensor(idx), torch.as_tensor(np.array([len(rows)], np.int32)), lr=lr, eps=eps, return_grads=True)
        links.append(dict(pre=pre, post=bc_snapshot(pol), rows=np.asarray(rows), loss=float(host(out["loss"])[0]),
                          grads={k: host(g) for k, g in zip(br.KEYS, out["grads"])}))
    return bc_snapshot(pol), np.array([l["loss"] for l in links]), links


def bc_check_link(link, obs, act, lr, eps):
    """one step of behaviour cloning against bcfit_ref, as tests/test_gpu_bcfit.py holds the one-step case: the loss and the six
    gradients within the bounds of backward64, w, m, v within adam_bound on the link's own gradient -> {quantity: worst ratio}"""
    W, M, V, t = link["pre"]["w"], link["pre"]["m"], link["pre"]["v"], link["pre"]["steps"] + 1
    x, a = obs[link["rows"]], act[link["rows"]]
    loss64, G, lb, E = br.backward64(W, x, a, with_bound=True)
    worst = {"loss": abs(link["loss"] - loss64) / lb}
    for k in br.KEYS:
        g = link["grads"][k]
        worst["grad " + k] = float((np.abs(g.astype(np.float64) - G[k]) / E[k]).max())
        want = br.adam64(W[k], M[k], V[k], g, t, lr, br.BETA1, br.BETA2, eps)
        for name, x64, b in zip("wmv", want, br.adam_bound(W[k], M[k], V[k], g, t, lr, br.BETA1, br.BETA2, eps)):
            key = "adam " + name
            worst[key] = max(worst.get(key, 0.0), float((np.abs(link["post"][name][k].astype(np.float64) - x64) / b).max()))
    assert link["post"]["steps"] == t
    assert all(np.isfinite(r) and r <= 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r <= 1.0}
    return worst


# ---------------------------------------------------------------------------------------------------- PPO2
TUPLE = {"obs": 0, "returns": 1, "masks": 2, "actions": 3, "values": 4, "neglogp": 5, "true_reward": 8}
DATA_KEYS = ("obs", "actions", "returns", "values", "neglogp")


def ppo2_snapshot(pol):
    """the slots of an ActorCriticPolicy of either layout, the moments of the PPO2 optimiser (zeros before its first step), its
    step count and the host copy of logstd that the Runner samples with"""
    keys = pr.KEYS_TOWERS if pol.towers else pr.KEYS_SHARED
    w = {k: host(getattr(pol, k)) for k in keys}
    has = getattr(pol, "_ppo_m", None) is not None
    slot = {k: i for i, k in enumerate(pr.SLOT_KEYS)}
    m = {k: host(pol._ppo_m[slot[k]]) if has else np.zeros_like(w[k]) for k in keys}
    v = {k: host(pol._ppo_v[slot[k]]) if has else np.zeros_like(w[k]) for k in keys}
    return {"w": w, "m": m, "v": v, "steps": int(getattr(pol, "_ppo_steps", 0) or 0), "logstd_host": np.asarray(pol.logstd_host).copy()}


def ppo2_restore(qa, snap, device):
    pol = qa.ActorCriticPolicy({k: np.array(v) for k, v in snap["w"].items()}, device=device)      # (copies: a host tensor aliases its array)
    pol._ppo_m = [to_dev(snap["m"][k].copy(), device) if k in snap["m"] else None for k in pr.SLOT_KEYS]
    pol._ppo_v = [to_dev(snap["v"][k].copy(), device) if k in snap["v"] else None for k in pr.SLOT_KEYS]
    pol._ppo_steps, pol._ppo_ws = snap["steps"], None
    return pol


def ppo2_same_bits(a, b):
    bad = [(p, k) for p in ("w", "m", "v") for k in a[p] if not same_bits(a[p][k], b[p][k])]
    return bad + (["steps"] if a["steps"] != b["steps"] else []) + ([] if same_bits(a["logstd_host"], b["logstd_host"]) else ["logstd_host"])


def rollout_data(rollout):
    """the five arrays of the update out of a recorded 9-tuple"""
    return {k: rollout[TUPLE[k]] for k in DATA_KEYS}


def ppo2_chain(qa, snap, rollout, indices, kw, update, device):
    """the PPO2 update of one roll-out as a chain of single calls on a fresh policy: `indices` [steps, batch] int32 (host) over the
    recorded 9-tuple, `kw` the keywords of ppo2_update -> (the snapshot at the end, statistics [steps, 6] float32, the links)"""
    pol = ppo2_restore(qa, snap, device)
    data = rollout_data(rollout)
    ro = {k: to_dev(v, device) for k, v in data.items()}
    fn = qa.ppo2_update if update == "hip" else qa.torch_ppo2_update
    keys = list(snap["w"])
    links = []
    for s in range(int(indices.shape[0])):
        pre = ppo2_snapshot(pol)
        out = fn(pol, ro, indices[s:s + 1].contiguous().to(device), return_grads=True, **kw)
        grads = {k: host(g) for k, g in zip(pr.SLOT_KEYS, out["grads"]) if g is not None}
        assert list(grads) == [k for k in pr.SLOT_KEYS if k in keys]
        links.append(dict(pre=pre, post=ppo2_snapshot(pol), mb=pr.minibatch(data, indices[s].numpy().astype(np.int64)), grads=grads,
                          stats=host(out["stats"])[0].astype(np.float32)))
    return ppo2_snapshot(pol), np.stack([l["stats"] for l in links]), links


def ppo2_hp(kw):
    """ppo2_update's keywords as the reference's hyper-parameter dict (cliprange_vf None: the policy's cliprange)"""
    crv = kw["cliprange"] if kw["cliprange_vf"] is None else kw["cliprange_vf"]
    return dict(lr=kw["learning_rate"], cliprange=kw["cliprange"], cliprange_vf=crv, ent_coef=kw["ent_coef"], vf_coef=kw["vf_coef"],
                max_grad_norm=0.0 if kw["max_grad_norm"] is None else kw["max_grad_norm"])


def ppo2_check_link(link, kw):
    """one PPO2 step of a chain against ppo2_ref, as tests/test_gpu_ppo2.py::check_step holds the one-step case (without the two
    conditions it asserts of its own fixtures: that the clip is active and that the step is many bounds long): every gradient and
    the six statistics within the bounds of backward64, the norm, and w, m, v within update_bound of update64 on the link's own
    gradient -> (worst gradient ratio, worst statistics ratio, worst update ratio)"""
    hp = ppo2_hp(kw)
    W, M, V, t = link["pre"]["w"], link["pre"]["m"], link["pre"]["v"], link["pre"]["steps"] + 1
    edges, _ = pr.edge_counts(W, link["mb"], hp)
    edges = {k: edges[k] for k in ("ratio at 1 +- eps", "advantage at zero")}   # (the ReLU masks and the value clip are covered by the bounds themselves)
    assert not any(edges.values()), "rows of this minibatch lie within their bound of a decision of the policy head: %s" % (edges,)
    st64, G, SB, E = pr.backward64(W, link["mb"], hp, with_bound=True)
    worst_g = 0.0
    for k in G:
        err = np.abs(link["grads"][k].astype(np.float64) - G[k])
        worst_g = max(worst_g, float((err / E[k]).max()))
        assert (err <= E[k]).all(), "%d of %d elements of the %s gradient out of bound, worst err / bound %.3g" % (
            int((err > E[k]).sum()), err.size, k, float((err / E[k]).max()))
    rs = np.abs(link["stats"].astype(np.float64) - st64) / SB
    assert (rs <= 1.0).all(), "statistics %s against %s, err / bound %s" % (link["stats"], st64, rs)
    Gd = {k: link["grads"][k] for k in G}
    Wn, Mn, Vn, _, norm = pr.update64(W, M, V, Gd, hp, t)
    assert abs(float(link["stats"][5]) - norm) <= 4 * pr.U32 * norm, (link["stats"][5], norm)
    UB = pr.update_bound(W, M, V, Gd, hp, t)
    worst_a = 0.0
    for k in G:
        for s, x64, b in zip("wmv", (Wn[k], Mn[k], Vn[k]), UB[k]):
            e = np.abs(link["post"][s][k].astype(np.float64) - x64)
            worst_a = max(worst_a, float((e / b).max()))
            assert (e <= b).all(), "%s of %s out of the update bound, worst err / bound %.3g" % (s, k, float((e / b).max()))
    assert link["post"]["steps"] == t
    return worst_g, float(rs.max()), worst_a


def explained_variance64(values, returns):
    """1 - Var[returns - values] / Var[returns] in float64"""
    v, r = np.asarray(values, np.float64), np.asarray(returns, np.float64)
    return 1.0 - (r - v).var() / r.var()


def check_values_of_obs(snap, rollout, what=""):
    """the recorded values are the snapshot's value head on the recorded observations, row for row, within the bound
    tests/actor_numerics.py holds every device evaluation of the net to: observations and values lie in ONE row order"""
    _, v64 = an.net64(snap["w"], rollout[TUPLE["obs"]])
    _, Ev = an.err_scale(snap["w"], rollout[TUPLE["obs"]])
    return an.check_unclipped(rollout[TUPLE["values"]], v64, Ev, "f32", what)


def tuples_same_bits(a, b):
    """the tensors of two 9-tuples of Runner.run()"""
    return [k for k, i in TUPLE.items() if not same_bits(a[i], b[i])]


# ---------------------------------------------------------------------------------------------------- the discriminator
def disc_snapshot(d):
    """a Discriminator's six tensors, Adam's moments, its step count and the running observation statistics"""
    return {"w": {k: host(getattr(d, k)) for k in gr.KEYS}, "m": {k: host(t) for k, t in zip(gr.KEYS, d.m)},
            "v": {k: host(t) for k, t in zip(gr.KEYS, d.v)}, "steps": int(d.steps),
            "rms": (d.stats.sum.copy(), d.stats.sumsq.copy(), float(d.stats.count)), "hidden": d.hidden, "entcoeff": d.entcoeff}


def disc_restore(qa, snap, device):
    d = qa.Discriminator(snap["hidden"], snap["entcoeff"], device=device, weights=snap["w"])
    d.m = [to_dev(snap["m"][k].copy(), device) for k in gr.KEYS]
    d.v = [to_dev(snap["v"][k].copy(), device) for k in gr.KEYS]
    d.steps = snap["steps"]
    d.stats.sum, d.stats.sumsq, d.stats.count = snap["rms"][0].copy(), snap["rms"][1].copy(), snap["rms"][2]
    d._norm = None
    return d


def disc_same_bits(a, b):
    bad = [(p, k) for p in ("w", "m", "v") for k in gr.KEYS if not same_bits(a[p][k], b[p][k])]
    bad += ["steps"] if a["steps"] != b["steps"] else []
    return bad + (["rms"] if not (same_bits(a["rms"][0], b["rms"][0]) and same_bits(a["rms"][1], b["rms"][1]) and a["rms"][2] == b["rms"][2]) else [])


def rms_merge(rms, rows):
    """SB2's RunningMeanStd restated: one merge of the float32 rows [n,12] into (sum, sumsq, count) in float64"""
    x = np.asarray(rows, np.float64)
    return rms[0] + x.sum(0), rms[1] + np.square(x).sum(0), rms[2] + float(x.shape[0])


def rms_norm(rms):
    """(mean, rscale) float32 as the discriminator's kernels receive them"""
    mean = rms[0] / rms[2]
    std = np.sqrt(np.maximum(rms[1] / rms[2] - np.square(mean), 1.0e-2))
    return mean.astype(np.float32), (1.0 / std).astype(np.float32)


class CursorRef:
    """the walk through successive shuffles of the expert's train rows, restated"""

    def __init__(self, rows):
        self.rows, self.order, self.pos, self.shuffles = np.asarray(rows), None, 0, 0


def disc_schedule_ref(n_gen, cur, batch, steps, generator):
    """the discriminator's schedule restated (batch <= the expert's rows): per step the generator rows -- the next piece of a
    permutation of the roll-out, a fresh one where the rest cannot fill the step -- and then the expert rows -- the next piece of the
    current shuffle of the train rows, a fresh one where the rest cannot fill the step, the position carried from call to call"""
    n_exp = len(cur.rows)
    assert batch <= n_exp and batch <= n_gen
    gen, exp = np.empty((steps, batch), np.int32), np.empty((steps, batch), np.int32)
    perm, pos = None, 0
    for s in range(steps):
        if perm is None or pos + batch > n_gen:
            perm, pos = torch.randperm(n_gen, generator=generator).numpy(), 0
        gen[s] = perm[pos:pos + batch]
        pos += batch
        if cur.order is None or cur.pos + batch > n_exp:
            cur.order, cur.pos, cur.shuffles = torch.randperm(n_exp, generator=generator).numpy(), 0, cur.shuffles + 1
        exp[s] = cur.rows[cur.order[cur.pos:cur.pos + batch]]
        cur.pos += batch
    return gen, exp


def disc_chain(qa, snap, gen_obs, gen_act, expert, gen_idx, exp_idx, lr, update, device):
    """one discriminator fit as a chain of single steps on a fresh discriminator.  The loop merges the running statistics ONCE per
    fit, over every row the schedule touches, before the steps: the chain makes that merge itself (rms_merge, checked against the
    snapshot afterwards) and runs its single steps without one -> (the snapshot at the end, statistics [steps, 5], the links)"""
    d = disc_restore(qa, snap, device)
    exp_obs = host(expert.obs)
    rms = rms_merge(snap["rms"], np.concatenate([gen_obs[gen_idx.reshape(-1)], exp_obs[exp_idx.reshape(-1)]]))
    d.stats.sum, d.stats.sumsq, d.stats.count = rms[0].copy(), rms[1].copy(), rms[2]
    d._norm = None
    go, ga = to_dev(gen_obs, device), to_dev(gen_act, device)
    fit = d.fit if update == "hip" else (lambda *a, **kw: qa.torch_discriminator_fit(d, *a, **kw))
    links = []
    for s in range(gen_idx.shape[0]):
        pre = disc_snapshot(d)
        out = fit(go, ga, expert, torch.as_tensor(gen_idx[s:s + 1].copy()), torch.as_tensor(exp_idx[s:s + 1].copy()), lr=lr, return_grads=True,
                  update_stats=False)
        links.append(dict(pre=pre, post=disc_snapshot(d), gen=(gen_obs[gen_idx[s]], gen_act[gen_idx[s]]),
                          exp=(exp_obs[exp_idx[s]], host(expert.actions)[exp_idx[s]]), stats=host(out["stats"])[0].astype(np.float32),
                          grads={k: host(g) for k, g in zip(gr.KEYS, out["grads"])}))
    return disc_snapshot(d), np.stack([l["stats"] for l in links]), links


def disc_check_link(link, lr):
    """one discriminator step against gail_ref, as tests/test_gpu_gail.py::check_step holds the one-step case -> worst error / bound"""
    W, M, V, t = link["pre"]["w"], link["pre"]["m"], link["pre"]["v"], link["pre"]["steps"] + 1
    mean, rscale = rms_norm(link["pre"]["rms"])
    stats, G, Es, E = gr.backward64(W, link["gen"], link["exp"], mean, rscale, link["pre"]["entcoeff"], with_bound=True)
    worst = 0.0
    for k in gr.KEYS:
        err = np.abs(link["grads"][k].astype(np.float64) - G[k])
        assert np.all(err <= E[k]), "discriminator gradient %s off by %.3g of its bound" % (k, (err / E[k]).max())
        worst = max(worst, float((err / E[k]).max()))
    err = np.abs(link["stats"].astype(np.float64) - stats)
    assert np.all(err <= Es), "discriminator statistics %s against %s, bounds %s" % (link["stats"], stats, Es)
    worst = max(worst, float((err / Es).max()))
    for k in gr.KEYS:
        g = link["grads"][k]
        want, bounds = gr.adam64(W[k], M[k], V[k], g, t, lr), gr.adam_bound(W[k], M[k], V[k], g, t, lr)
        for name, x64, b in zip("wmv", want, bounds):
            err = np.abs(link["post"][name][k].astype(np.float64) - x64)
            assert np.all(err <= b), "discriminator %s of %s off by %.3g of its bound" % (name, k, (err / b).max())
            worst = max(worst, float((err / b).max()))
    assert link["post"]["steps"] == t
    return worst


# ---------------------------------------------------------------------------------------------------- TRPO
def trpo_snapshot(pol):
    """the thirteen tensors of a towers policy, the value fit's moments (zeros before its first step), its step count and the host
    copy of logstd"""
    w = {k: host(getattr(pol, k)) for k in pr.KEYS_TOWERS}
    has = getattr(pol, "_trpo_m", None) is not None
    slot = {k: i for i, k in enumerate(pr.SLOT_KEYS)}
    m = {k: host(pol._trpo_m[slot[k]]) if has else np.zeros_like(w[k]) for k in tr.VALUE_KEYS}
    v = {k: host(pol._trpo_v[slot[k]]) if has else np.zeros_like(w[k]) for k in tr.VALUE_KEYS}
    return {"w": w, "m": m, "v": v, "steps": int(getattr(pol, "_trpo_steps", 0) or 0), "logstd_host": np.asarray(pol.logstd_host).copy()}


def trpo_restore(qa, snap, device):
    pol = qa.ActorCriticPolicy({k: np.array(v) for k, v in snap["w"].items()}, device=device)
    pol._trpo_m = [to_dev(snap["m"][k].copy(), device) if k in snap["m"] else None for k in pr.SLOT_KEYS]
    pol._trpo_v = [to_dev(snap["v"][k].copy(), device) if k in snap["v"] else None for k in pr.SLOT_KEYS]
    pol._trpo_steps, pol._trpo_ws = snap["steps"], None
    return pol


def trpo_generator_step(qa, pol, rollout, vf_idx, hp, vf_stepsize, device):
    """one generator step of TRPO on `pol` as the chain has it: trpo_policy_step over the recorded roll-out (with the gradient and
    the trace), then the value fit one step per call over `vf_idx` [steps, batch] -> (the policy step's link, the value links)"""
    data = {k: rollout[TUPLE[k]] for k in ("obs", "actions", "returns", "values")}
    ro = {k: to_dev(v, device) for k, v in data.items()}
    pre = trpo_snapshot(pol)
    out = qa.trpo_policy_step(pol, ro, return_grad=True, trace=True, **hp)
    plink = dict(pre=pre, post=trpo_snapshot(pol), data=data, stats=host(out["stats"]), grad=host(out["grad"]),
                 trace={k: host(v) for k, v in out["trace"].items()})
    vlinks = []
    for s in range(int(vf_idx.shape[0])):
        pre = trpo_snapshot(pol)
        o = qa.trpo_vf_fit(pol, ro, vf_idx[s:s + 1].contiguous().to(device), vf_stepsize=vf_stepsize, return_grads=True)
        rows = vf_idx[s].numpy().astype(np.int64)
        vlinks.append(dict(pre=pre, post=trpo_snapshot(pol), obs=data["obs"][rows], ret=data["returns"][rows], loss=float(host(o["stats"])[0]),
                           grads={k: host(g) for k, g in zip(tr.VALUE_KEYS, o["grads"])}))
    return plink, vlinks


def _within(got, ref, bound, what, worst):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    r = float(np.max(np.abs(got - ref) / bound))
    assert np.all(np.isfinite(got)) and r <= 1.0, "%s: worst |device - float64| / bound = %.3g" % (what, r)
    worst[what] = max(worst.get(what, 0.0), r)


def trpo_check_policy_link(link, hp, residual_tol):
    """one TRPO policy step against trpo_ref, by the recipes of tests/test_gpu_trpo.py: the gradient and the statistics within
    grad64's bounds; every traced product within the bound of the float64 product of the device's own vector, the solver's algebra
    bit for bit the replay from the traced products; surr_k and kl_k of every evaluated candidate within bounds at the device's own
    theta_k, the float64 decision at each that of the device, the policy bit for bit float32(theta_old + fullstep 2^-k); the value
    tower and its moments untouched -> {quantity: worst ratio}"""
    W, data, st, T = link["pre"]["w"], link["data"], link["stats"], link["trace"]
    worst = {}
    G = tr.grad64(W, data, hp["entcoeff"], with_bound=True)
    _within(link["grad"], G["g"], G["E_g"], "g", worst)
    _within(st[0], G["surr_before"], G["E_surr"], "surr_before", worst)
    _within(st[4], G["norm"], G["E_norm"], "|g|", worst)
    iters, want = int(st[9]), int(st[8])
    assert want >= -1 and iters >= 1, "the step was skipped (accepted %d)" % want
    R = tr.replay_cg(link["grad"], T["fvp_out"][:hp["cg_iters"]], T["fvp_out"][hp["cg_iters"]], iters, hp["max_kl"], residual_tol)
    assert R["iters"] == iters
    for k in range(iters):
        assert same_bits(T["fvp_in"][k], R["p"][k]), "p_%d" % k
        ref, E = tr.fvp64(W, data["obs"], hp["fvp_stride"], T["fvp_in"][k], hp["cg_damping"], with_bound=True)
        _within(T["fvp_out"][k], ref, E, "z_k", worst)
    assert same_bits(T["cg"][:iters], R["cg"])
    assert same_bits(T["fvp_in"][hp["cg_iters"]], R["x"]) and same_bits(T["x"], R["x"])
    ref, E = tr.fvp64(W, data["obs"], hp["fvp_stride"], T["x"], hp["cg_damping"], with_bound=True)
    _within(T["fvp_out"][hp["cg_iters"]], ref, E, "(F + damping) x", worst)
    assert same_bits(T["fullstep"], R["fullstep"])
    assert same_bits(st[5:8], np.array([R["shs"], R["lm"], R["expected_improve"]]).astype(np.float32))
    assert same_bits(st[4], np.float32(np.sqrt(R["rdotr0"])))
    th0 = tr.flatten(W, np.float32)
    evaluated = (want + 1) if want >= 0 else hp["backtracks"]
    for k in range(evaluated):
        thk = tr.candidate32(th0, T["fullstep"], k)
        surr, kl, E_s, E_k = tr.ls_eval64(W, thk, data, hp["entcoeff"], with_bound=True)
        _within(T["ls"][k, 0], surr, E_s, "surr_k", worst)
        _within(T["ls"][k, 1], kl, E_k, "kl_k", worst)
        ok = kl <= 1.5 * hp["max_kl"] and surr - G["surr_before"] >= 0.0
        assert ok == (k == want), "the float64 decision at the device's candidate %d" % k
    new = tr.flatten(link["post"]["w"], np.float32)
    assert same_bits(new, tr.candidate32(th0, T["fullstep"], want) if want >= 0 else th0)
    if want >= 0:
        assert same_bits(st[1:3], T["ls"][want])
    for k in tr.VALUE_KEYS:
        assert same_bits(link["post"]["w"][k], W[k]) and same_bits(link["post"]["m"][k], link["pre"]["m"][k]), k
    assert link["post"]["steps"] == link["pre"]["steps"]
    return worst


def trpo_check_vf_link(link, lr):
    """one step of the value fit against trpo_ref, as tests/test_gpu_trpo.py::test_value_fit_one_step_against_float64 holds it"""
    W, M, V, t = link["pre"]["w"], link["pre"]["m"], link["pre"]["v"], link["pre"]["steps"] + 1
    worst = {}
    loss, G, E_loss, E_G = tr.vf_backward64(W, link["obs"], link["ret"], with_bound=True)
    _within(link["loss"], loss, E_loss, "value loss", worst)
    for k in tr.VALUE_KEYS:
        _within(link["grads"][k], G[k], E_G[k], "value gradient", worst)
    B = tr.vf_update_bound(W, M, V, G, E_G, t, lr)
    for k in tr.VALUE_KEYS:
        w, m, v = pr.adam64(W[k], M[k], V[k], G[k], t, lr, tr.VF_BETA1, tr.VF_BETA2, tr.VF_EPS)
        _within(link["post"]["w"][k], w, B[k][0], "value w", worst)
        _within(link["post"]["m"][k], m, B[k][1], "value m", worst)
        _within(link["post"]["v"][k], v, B[k][2], "value v", worst)
    for k in tr.POLICY_KEYS:
        assert same_bits(link["post"]["w"][k], W[k]), k
    assert link["post"]["steps"] == t
    return worst


def trpo_same_bits(a, b):
    bad = [(p, k) for p in ("w", "m", "v") for k in a[p] if not same_bits(a[p][k], b[p][k])]
    return bad + (["steps"] if a["steps"] != b["steps"] else []) + ([] if same_bits(a["logstd_host"], b["logstd_host"]) else ["logstd_host"])


# ---------------------------------------------------------------------------------------------------- the off-policy rows
def off_hyper(row):
    """the keywords of ddpg_update / td3_update from the row's constructor arguments"""
    kw = row["kwargs"]
    if row["loop"] == "ddpg":
        return {k: kw[k] for k in ("gamma", "tau", "actor_lr", "critic_lr", "obs_clip")}
    return dict(gamma=kw["gamma"], tau=kw["tau"], actor_lr=kw["learning_rate"], critic_lr=kw["learning_rate"], policy_delay=kw["policy_delay"],
                target_policy_noise=kw["target_policy_noise"], target_noise_clip=kw["target_noise_clip"])


def off_shape(row):
    """(env steps per cycle, updates per cycle, batch, capacity)"""
    kw = row["kwargs"]
    if row["loop"] == "ddpg":
        return kw["nb_rollout_steps"], kw["nb_train_steps"], kw["batch_size"], kw["buffer_size"]
    return kw["train_freq"], kw["gradient_steps"], kw["batch_size"], kw["buffer_size"]


def run_off_policy(qa, row, env, update, device):
    """DDPG.learn / TD3.learn on `env` (a Recorded), ONE learn call per cycle, with a snapshot of the policy and of the ring after
    each -> the record"""
    kind, n = row["loop"], row["n_envs"]
    pol = (qa.DDPGPolicy if kind == "ddpg" else qa.TD3Policy)(seed=row["policy_seed"], device=device)
    noise = qa.OUNoise(n, device=device, seed=row["noise_seed"])
    model = (qa.DDPG if kind == "ddpg" else qa.TD3)(pol, env, update=update, action_noise=noise, seed=row["seed"], **row["kwargs"])
    roll = off_shape(row)[0]
    rec = dict(model=model, env=env, snaps=[off_snapshot(pol, kind)], rings=[], logs=[])
    for _ in range(row["cycles"]):
        logs = model.learn(roll * n)
        assert len(logs) == 1, logs
        rec["logs"] += logs
        rec["snaps"].append(off_snapshot(pol, kind))
        rec["rings"].append(ring_snapshot(model.replay))
    return rec


def td3_caller_noise(qa, row, t0, steps, batch, ring, update, device):
    """the normals of updates t0 .. t0 + steps - 1 as a caller would hand them over: on the device what a keyed call of a scratch
    policy at that update index reports as its noise (tests/test_gpu_td3.py pins that a call fed them equals the keyed call, and that
    they depend on the seed, the update index and the slot alone), on the host float64 Box-Muller rounded to float32"""
    if update != "hip":
        return to_dev(td.normals64(row["seed"], t0, steps, batch).astype(np.float32), device)
    scratch = qa.TD3Policy(seed=12345, device=device)
    scratch.steps = t0
    data = tuple(to_dev(a, scratch.device) for a in ring["data"])
    out = qa.td3_update(scratch, data, torch.zeros((steps, batch), dtype=torch.int32), seed=row["seed"], return_noise=True, **off_hyper(row))
    return out["noise"]


def check_off_policy(qa, row, rec, update, device):
    """every cycle of a DDPG / TD3 record replayed (module docstring) -> {quantity: worst error / bound over all links}"""
    kind, n, env, hyper = row["loop"], row["n_envs"], rec["env"], off_hyper(row)
    roll, steps, batch, cap = off_shape(row)
    names = dd.STAT_NAMES if kind == "ddpg" else td.STAT_NAMES
    dones = np.stack([host(e[3]) for e in env.log]).astype(bool)
    assert dones.shape == (row["cycles"] * roll, n)
    inside, mid = episode_conditions(dones, roll)
    assert inside and mid and dones[roll - 1].any() and not dones[roll - 1].all(), "the record lacks an episode end inside a cycle, on its last step, or an env in mid-episode there"
    gen = torch.Generator().manual_seed(row["seed"])
    worst = {}
    for c in range(row["cycles"]):
        done_steps = (c + 1) * roll
        size = min(done_steps * n, cap)
        ring = rec["rings"][c]
        assert (ring["size"], ring["pos"]) == (size, (done_steps * n) % cap)
        arrays, which, where = expected_ring(env, cap, done_steps)
        for got, want in zip(ring["data"], arrays):
            assert same_bits(got[where], want[which]), "cycle %d: the ring is not the last transitions the env returned" % (c + 1)
        idx = torch.randint(0, size, (steps, batch), generator=gen, dtype=torch.int32)        # the c-th draw, over the ring's size now
        noise = None
        if kind == "td3" and row["noise"] == "caller":
            noise = td3_caller_noise(qa, row, steps * c, steps, batch, ring, update, device)
        end, stats, links = off_chain(qa, kind, rec["snaps"][c], ring, idx, hyper, update, device, seed=row["seed"], noise=noise)
        bad = off_same_bits(end, rec["snaps"][c + 1], kind)
        assert not bad, "cycle %d: the chain does not end in the loop's bits: %s" % (c + 1, bad[:6])
        log = rec["logs"][c]
        check_mean([log[name] for name in names], stats, device, "cycle %d" % (c + 1))
        assert log["cycle"] == 1 and log["total_timesteps"] == done_steps * n
        rew = np.stack([host(e[2]) for e in env.log[c * roll:done_steps]]).astype(np.float64)
        assert abs(log["reward_mean"] - rew.mean()) <= rew.size * F64_EPS * np.abs(rew).mean(), (c, log["reward_mean"], rew.mean())
        for link in links:
            w = ddpg_check_link(link, hyper, update) if kind == "ddpg" else td3_check_link(link, hyper, row["seed"], update)
            for k, r in w.items():
                worst[k] = max(worst.get(k, 0.0), r)
        if kind == "td3":
            u0, delay = steps * c, hyper["policy_delay"]
            assert rec["snaps"][c + 1]["actor_steps"] == sum(1 for u in range(u0 + steps) if u % delay == 0)
            assert [float(s[5]) != 0.0 for s in stats] == [(u0 + s) % delay == 0 for s in range(steps)]
    return worst


def check_behaviour_actions(qa, row, rec, device):
    """random_exploration = 0: every action the env received is clamp(predict(obs) + noise) of a FRESH policy built from the snapshot
    before that cycle and a twin OUNoise of the same seed, advanced once per step and reset where the recorded done says so, bit for
    bit; the observation is the one the env returned last, over the learn boundary too.  random_exploration = 1: every action lies in
    [-1, 1) and differs from that one in every env"""
    kind, n, env = row["loop"], row["n_envs"], rec["env"]
    roll = off_shape(row)[0]
    uniform = row["kwargs"].get("random_exploration", 0.0) == 1.0
    noise = qa.OUNoise(n, device=device, seed=row["noise_seed"])
    obs = env.first
    for c in range(row["cycles"]):
        pol = off_restore(qa, kind, rec["snaps"][c], device)
        for k in range(roll):
            a_rec, obs1, _, done = env.log[c * roll + k]
            with torch.no_grad():
                a = pol.predict(obs, row["kwargs"]["obs_clip"]) if kind == "ddpg" else pol.predict(obs).to(torch.float32)
                a = (a + noise()).clamp(-1.0, 1.0)
            if uniform:
                assert bool((a_rec >= -1.0).all()) and bool((a_rec < 1.0).all()) and bool((a_rec != a).any(1).all()), (c, k)
            else:
                assert torch.equal(a, a_rec), "cycle %d step %d: the action is not the snapshot's actor plus the twin noise" % (c + 1, k)
            noise.reset(done)
            obs = obs1


# ---------------------------------------------------------------------------------------------------- the on-policy rows
LOOP_KEYS = ("update", "frac", "n_updates", "lr_now", "cliprange_now", "crv_now", "rollout", "indices", "out", "log", "gen_idx", "exp_idx", "d_out")


def ppo2_kw(row, update, n_updates):
    """the keywords of ppo2_update at update `update` (from 1): the row's callables at 1 - (update - 1) / n_updates"""
    K = row["kwargs"]
    frac = 1.0 - (update - 1.0) / n_updates
    return dict(learning_rate=float(K["learning_rate"](frac)), cliprange=float(K["cliprange"](frac)),
                cliprange_vf=None if K["cliprange_vf"] is None else float(K["cliprange_vf"](frac)), ent_coef=K["ent_coef"], vf_coef=K["vf_coef"],
                max_grad_norm=K["max_grad_norm"])


def draw_minibatches(n_batch, nminibatches, noptepochs, generator):
    """the minibatch schedule of one update restated: per epoch one permutation of the roll-out's rows, cut into consecutive pieces"""
    idx = torch.stack([torch.randperm(n_batch, generator=generator).to(torch.int32) for _ in range(noptepochs)])
    return idx.view(noptepochs * nminibatches, n_batch // nminibatches)


def check_ppo2_update(qa, row, u, n_updates, pre, rec, idx, ev_tol, update, device, bounds=True):
    """update `u` of a PPO2 / GAIL record replayed from the snapshot `pre`: the rates, the chain over the test's own schedule `idx`
    ending in the loop's bits and statistics, every link against float64 (`bounds`), the log -> the worst (gradient, statistics,
    update) ratios"""
    K, n_batch = row["kwargs"], row["n_envs"] * row["n_steps"]
    kw = ppo2_kw(row, u, n_updates)
    assert rec["update"] == u and rec["n_updates"] == n_updates
    assert (rec["lr_now"], rec["cliprange_now"], rec["crv_now"]) == (kw["learning_rate"], kw["cliprange"], kw["cliprange_vf"]), "the rates of update %d" % u
    assert same_bits(rec["indices"], idx.numpy()), "the schedule of update %d is not the %d-th draw of one carried generator" % (u, u)
    after = rec["after"]["policy"] if "policy" in rec["after"] else rec["after"]
    end, stats, links = ppo2_chain(qa, pre, rec["rollout"], idx, kw, update, device)
    bad = ppo2_same_bits(end, after)
    assert not bad, "update %d: the chain does not end in the loop's bits: %s" % (u, bad[:6])
    assert same_bits(stats, rec["out"]["stats"]), "update %d: the chain's statistics are not the loop's" % u
    worst = np.zeros(3)
    if bounds:
        for link in links:
            worst = np.maximum(worst, ppo2_check_link(link, kw))
    log = rec["log"]
    check_mean([log[k] for k in pr.STAT_NAMES], stats, device, "update %d" % u)
    assert (log["n_updates"], log["serial_timesteps"], log["total_timesteps"]) == (u, u * row["n_steps"], u * n_batch)
    assert (log["learning_rate"], log["cliprange"]) == (kw["learning_rate"], kw["cliprange"])
    values, returns = rec["rollout"][TUPLE["values"]], rec["rollout"][TUPLE["returns"]]
    ev, swapped = explained_variance64(values, returns), explained_variance64(returns, values)
    print("loops %s update %d: explained_variance %.9g, float64 %.9g, |difference| %.3g (tolerance %.3g), swapped twin %.6g" % (
        row["id"], u, log["explained_variance"], ev, abs(log["explained_variance"] - ev), ev_tol, swapped))
    assert abs(log["explained_variance"] - ev) <= ev_tol and ev_tol < 0.1 * abs(ev - swapped)
    return worst
