"""The poison cases of the trainers on the device: one table per library, built from the fixtures of the float64 references, and the
references' own run of a case.  A helper module, not a test; numpy only.

A case puts ONE non-finite value (NaN, +inf or -inf) into one element of one tensor a training step is given: an input array, a
weight or a moment (for TD3 also the caller's noise).  The contract (the NON-FINITE VALUES paragraph of include/quadsim_ppo.h,
include/quadsim_ddpg.h, include/quadsim_dyn_fit.h, include/quadsim_bc.h, include/quadsim_gail.h, include/quadsim_td3.h and
include/quadsim_trpo.h) says what must follow; tests/test_nonfinite_cpu.py
anchors the references to float64 torch autograd at every case and holds the conditions of the tables,
tests/test_gpu_nonfinite.py runs every case on the device.

The shapes are the smallest at which this can go wrong: a batch of 17 rows (one full 16-row chunk and a one-row tail), the
poisoned row once in the chunk (position 3) and once as the tail (position 16); two steps where the second step alone reads the
poison, or where a poisoned moment reaches a statistic only through the weight it spoils.

How a row is poisoned: the data set gets one row more, a copy of the fixture row at the poisoned position of the step's index
row, and the index row points there instead.  The case's TWIN is the same set-up without the poison (for an infinity that the
header's clamp bounds: with the clamped value), so the twin of a row case is the fixture's own minibatch.

TRPO's policy step takes the rows 0 .. n-1 and no indices: its cases (TRPO_STEP_CASES, outside LIBRARIES like the reward's) poison
a row of the roll-out itself, and a poisoned case there is a REJECTED step, not a diverged net.

  case["clean"] is None   the step reads the poison: at least one statistic of the call is non-finite
  case["clean"] = reason  the contract says the poison changes nothing: bit for bit the twin's result
"""
import numpy as np

import bcfit_ref as br
import ddpg_ref as dd
import dynfit_ref as fr
import dynplan_ref as dr
import gail_ref as gr
import ppo2_ref as pr
import td3_ref as td
import trpo_ref as tr

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
BATCH = 17


def nonfinite(a):
    return ~np.isfinite(np.asarray(a, np.float64))


def has_nonfinite(tensors):
    """any non-finite element in a dict of arrays"""
    return bool(any(nonfinite(v).any() for v in tensors.values()))


def _case(cid, target, elem, value, pos=3, steps=1, step=0, clean=None, **kw):
    """target: ("row", array name) the appended row of a data array, ("w" | "m" | "v", ...) a tensor of the state; elem: the flat
    element (of the row, or of the tensor); step: the step whose index row reads the poisoned row (-1: none); pos: where"""
    return dict(id=cid, target=target, elem=elem, value=value, pos=pos, steps=steps, step=step, clean=clean, **kw)


def _poison(arr, elem, value):
    arr.reshape(-1)[elem] = value


# ---------------------------------------------------------------------------------------------------- DDPG
DDPG_HYPER = dict(gamma=dd.GAMMA, tau=dd.TAU, actor_lr=1e-2, critic_lr=1e-2, obs_clip=dd.OBS_CLIP)
DDPG_ONLINE = ("actor", "critic")
DDPG_DATA = ("obs0", "act", "rew", "obs1", "done")
_TERMINAL = "a terminal row takes y = rew: the target value is never selected"
_CLAMPED = "an infinite observation is its clamped copy"

DDPG_CASES = (
    # ---- every input array the step reads
    _case("obs0-nan-row3", ("row", "obs0"), 5, NAN),
    _case("obs0-nan-row16", ("row", "obs0"), 0, NAN, pos=16),
    _case("act-nan", ("row", "act"), 2, NAN),
    _case("rew-nan", ("row", "rew"), 0, NAN, pos=16),
    _case("obs1-nan", ("row", "obs1"), 11, NAN, rowdone=0.0),
    _case("done-nan", ("row", "done"), 0, NAN),
    _case("rew-pinf", ("row", "rew"), 0, PINF),
    _case("act-ninf", ("row", "act"), 0, NINF, pos=16),
    _case("obs0-nan-step2", ("row", "obs0"), 7, NAN, steps=2, step=1),
    # ---- weights: layer 0, the last layer; a first and a second moment (they reach a statistic through the weight, in step 2)
    _case("actor-w0-nan", ("w", "actor", "w0"), 5 * 128 + 17, NAN),
    _case("critic-w2-nan", ("w", "critic", "w2"), 40, NAN),
    _case("critic-w0-pinf", ("w", "critic", "w0"), 3 * 128 + 2, PINF),
    _case("actor-m-w1-nan", ("m", "actor", "w1"), 1000, NAN, steps=2),
    _case("critic-v-w0-nan", ("v", "critic", "w0"), 300, NAN, steps=2),
    # ---- a target net's weight, every row live
    _case("critic-target-w2-nan-live", ("w", "critic_target", "w2"), 3, NAN, done=0.0),
    _case("actor-target-w0-nan-live", ("w", "actor_target", "w0"), 9, NAN, done=0.0),
    # ---- clean by contract
    _case("critic-target-w2-nan-terminal", ("w", "critic_target", "w2"), 3, NAN, done=1.0, clean=_TERMINAL),
    _case("actor-target-w0-nan-terminal", ("w", "actor_target", "w0"), 9, NAN, done=1.0, clean=_TERMINAL),
    _case("obs1-nan-terminal-row", ("row", "obs1"), 11, NAN, rowdone=1.0, clean=_TERMINAL),
    _case("obs0-pinf-clamped", ("row", "obs0"), 5, PINF, clean=_CLAMPED),
    _case("obs0-ninf-clamped-row16", ("row", "obs0"), 0, NINF, pos=16, clean=_CLAMPED),
    _case("obs1-pinf-clamped", ("row", "obs1"), 4, PINF, rowdone=0.0, clean=_CLAMPED),
    _case("obs0-ninf-step2-clamped", ("row", "obs0"), 7, NINF, steps=2, step=1, clean=_CLAMPED),
    _case("unread-row-nan", ("row", "obs0"), 5, NAN, step=-1, clean="no index row names the row"),
    _case("beyond-count-nan", ("row", "rew"), 0, NAN, pos=12, counts=(10,), clean="the entry lies at or beyond counts[s]"),
    _case("beyond-count-step2-nan", ("row", "act"), 1, NAN, pos=16, steps=2, step=1, counts=(17, 16), clean="the entry lies at or beyond counts[s]"),
)


def ddpg_setup(case, twin=False):
    """-> dict(P, M, V: {net: {key: float32 array}}, rp: the five arrays with one row more, idx [steps,17] int32, counts or None)"""
    P = {n: {k: np.array(dd.nets()[n][k]) for k in dd.KEYS} for n in dd.NETS}
    M0, V0 = dd.moments()
    M = {n: {k: np.array(M0[n][k]) for k in dd.KEYS} for n in DDPG_ONLINE}
    V = {n: {k: np.array(V0[n][k]) for k in dd.KEYS} for n in DDPG_ONLINE}
    rp = [np.concatenate([a, a[:1]]) for a in dd.replay()]
    idx = dd.step_indices(BATCH, steps=case["steps"]).copy()
    new = dd.N_ROWS
    kind = case["target"][0]
    if kind == "row":
        src = idx[max(case["step"], 0), case["pos"]]
        for a in rp:
            a[new] = a[src]
        if "rowdone" in case:
            rp[4][new] = case["rowdone"]
        if case["step"] >= 0:
            idx[case["step"], case["pos"]] = new
    if "done" in case:
        rp[4][:] = case["done"]
    value = case["value"]
    if twin:
        value = np.sign(value) * DDPG_HYPER["obs_clip"] if case["clean"] == _CLAMPED else None
    if value is not None:
        if kind == "row":
            _poison(rp[DDPG_DATA.index(case["target"][1])][new:new + 1], case["elem"], value)
        else:
            _poison({"w": P, "m": M, "v": V}[kind][case["target"][1]][case["target"][2]], case["elem"], value)
    counts = None if case.get("counts") is None else np.asarray(case["counts"], np.int32)
    return dict(P=P, M=M, V=V, rp=tuple(rp), idx=idx, counts=counts)


def ddpg_reference(S, with_bound=False):
    """ddpg_ref's loop (fit64's, kept step by step) over a set-up -> dict(stats [steps,4] float64, gflag [steps,2]: a non-finite
    gradient element per online net, nets [steps,4]: a non-finite weight per net after the step; with_bound: first = step 1's
    (stats, G, Es, E) of step64)"""
    f, hp = np.float64, DDPG_HYPER
    P = {n: {k: np.asarray(S["P"][n][k], f).copy() for k in dd.KEYS} for n in dd.NETS}
    M = {n: {k: np.asarray(S["M"][n][k], f).copy() for k in dd.KEYS} for n in DDPG_ONLINE}
    V = {n: {k: np.asarray(S["V"][n][k], f).copy() for k in dd.KEYS} for n in DDPG_ONLINE}
    out = dict(stats=[], gflag=[], nets=[])
    with np.errstate(all="ignore"):
        for s, rows in enumerate(S["idx"]):
            rows = rows if S["counts"] is None else rows[:S["counts"][s]]
            mb = tuple(a[rows] for a in S["rp"])
            if s == 0 and with_bound:
                st, G, _, Es, E = dd.step64(P, mb, hp["gamma"], hp["obs_clip"], with_bound=True)
                out["first"] = (st, G, Es, E)
            else:
                st, G, _ = dd.step64(P, mb, hp["gamma"], hp["obs_clip"])
            out["stats"].append(st)
            out["gflag"].append([has_nonfinite(G[n]) for n in DDPG_ONLINE])
            for n in DDPG_ONLINE:
                for k in dd.KEYS:
                    P[n][k], M[n][k], V[n][k] = dd.adam64(P[n][k], M[n][k], V[n][k], G[n][k], s + 1, hp[n + "_lr"])
                    P[n + "_target"][k] = (1.0 - hp["tau"]) * P[n + "_target"][k] + hp["tau"] * P[n][k]
            out["nets"].append([has_nonfinite(P[n]) for n in dd.NETS])
    return {k: (v if k == "first" else np.asarray(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- PPO2
PPO2_WEIGHTS = "he"
PPO2_HP = pr.HP_VCLIP                              # the norm clip active, value clipping on: every select of the head is reached
PPO2_DATA = ("obs", "actions", "returns", "values", "neglogp")
_PPO2_FULL = (("shared", 1), ("towers", 3))        # every target
_PPO2_SOME = (("shared", 3), ("towers", 1))        # the rest of the layout x slices matrix: one target of each kind


def _ppo2_cases():
    every = (
        _case("obs-nan-row3", ("row", "obs"), 5, NAN),
        _case("obs-nan-row16", ("row", "obs"), 0, NAN, pos=16),
        _case("actions-nan", ("row", "actions"), 2, NAN, pos=16),
        _case("returns-nan", ("row", "returns"), 0, NAN),
        _case("values-nan", ("row", "values"), 0, NAN),
        _case("neglogp-nan", ("row", "neglogp"), 0, NAN),
        _case("neglogp-pinf", ("row", "neglogp"), 0, PINF, pos=16),
        _case("returns-ninf", ("row", "returns"), 0, NINF),
        _case("obs-nan-step2", ("row", "obs"), 7, NAN, steps=2, step=1),
        _case("w0-nan", ("w", "w0"), 5 * 128 + 17, NAN),
        _case("w2-nan", ("w", "w2"), 40 * 4 + 1, NAN),
        _case("wv2-pinf", ("w", "wv2"), 77, PINF),
        _case("logstd-nan", ("w", "logstd"), 2, NAN),
        _case("m-w1-nan", ("m", "w1"), 1000, NAN, steps=2),
        _case("v-wv1-nan", ("v", "wv1"), 300, NAN, steps=2),
        _case("unread-row-nan", ("row", "obs"), 5, NAN, step=-1, clean="no index row names the row"),
        _case("unread-row-step2-nan", ("row", "neglogp"), 0, NAN, steps=2, step=-1, clean="no index row names the row"),
    )
    some = [c for c in every if c["id"] in ("obs-nan-row16", "values-nan", "neglogp-nan", "w0-nan", "m-w1-nan", "unread-row-nan")]
    out = []
    for combos, cases in ((_PPO2_FULL, every), (_PPO2_SOME, some)):
        for layout, slices in combos:
            out += [dict(c, id="%s-s%d-%s" % (layout, slices, c["id"]), layout=layout, slices=slices) for c in cases]
    return tuple(out)


PPO2_CASES = _ppo2_cases()


def ppo2_setup(case, twin=False):
    """-> dict(W, M, V: {key: float32 array}, data: the five arrays with one row more, idx [steps,17] int32, hp, slices).  Step 1
    is the fixture's minibatch step_rows(.., 17), step 2 the same rows in another order"""
    W0 = pr.weight_set(PPO2_WEIGHTS, case["layout"])
    W = {k: np.array(W0[k]) for k in pr.keys_of(W0)}
    M, V = ({k: np.array(a[k]) for k in a} for a in pr.moments(W0))
    data = {k: np.concatenate([v, v[:1]]) for k, v in pr.rollout(PPO2_WEIGHTS, case["layout"]).items()}
    rows = pr.step_rows(PPO2_WEIGHTS, case["layout"], BATCH)
    idx = np.stack([np.roll(rows, 5 * s) for s in range(case["steps"])]).astype(np.int32)
    new = pr.N_ROWS
    kind = case["target"][0]
    if kind == "row":
        src = idx[max(case["step"], 0), case["pos"]]
        for a in data.values():
            a[new] = a[src]
        if case["step"] >= 0:
            idx[case["step"], case["pos"]] = new
    if not twin:
        if kind == "row":
            _poison(data[case["target"][1]][new:new + 1], case["elem"], case["value"])
        else:
            _poison({"w": W, "m": M, "v": V}[kind][case["target"][1]], case["elem"], case["value"])
    return dict(W=W, M=M, V=V, data=data, idx=idx, hp=PPO2_HP, slices=case["slices"])


def ppo2_reference(S, with_bound=False):
    """ppo2_ref's backward64 and update64, step by step -> dict(stats [steps,6] float64, gflag [steps]: a non-finite gradient
    element, nets [steps]: a non-finite weight after the step; with_bound: first = step 1's (stats, G, SB, E) of backward64)"""
    f = np.float64
    W, M, V = ({k: np.asarray(a[k], f).copy() for k in a} for a in (S["W"], S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    with np.errstate(all="ignore"):
        for s, rows in enumerate(S["idx"]):
            mb = pr.minibatch(S["data"], rows)
            if s == 0 and with_bound:
                st, G, SB, E = pr.backward64(W, mb, S["hp"], with_bound=True)
                out["first"] = (st, G, SB, E)
            else:
                st, G = pr.backward64(W, mb, S["hp"])
            out["stats"].append(st)
            out["gflag"].append(has_nonfinite(G))
            W, M, V, _, _ = pr.update64(W, M, V, G, S["hp"], s + 1)
            out["nets"].append(has_nonfinite(W))
    return {k: (v if k == "first" else np.asarray(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- the dynamics fit
DYNFIT_SET = dr.edge_name(64, 64)                  # a dense (64, 64) net: the 64-wide instantiation, whose 17-row fixture is edge-free
DYNFIT_LR, DYNFIT_ROW = 1e-2, 200                  # the buffer's row that takes the copy (its 300 rows stay 300: the tail is NaN already)
_UNREAD = "no index row names the row"

DYNFIT_CASES = (
    _case("x-nan-row3", ("row", "x"), 5, NAN),
    _case("x-nan-row16", ("row", "x"), 15, NAN, pos=16),
    _case("d-nan", ("row", "d"), 2, NAN),
    _case("d-pinf-row16", ("row", "d"), 0, PINF, pos=16),
    _case("x-ninf", ("row", "x"), 0, NINF),
    _case("x-nan-step2", ("row", "x"), 7, NAN, steps=2, step=1),
    _case("w1-nan", ("w", "w1"), 17 * 16 + 5, NAN),
    _case("w3-nan", ("w", "w3"), 3 * 64 + 40, NAN),
    _case("b2-pinf", ("w", "b2"), 9, PINF),
    _case("m-w2-nan", ("m", "w2"), 1000, NAN, steps=2),
    _case("v-w1-nan", ("v", "w1"), 300, NAN, steps=2),
    _case("unread-row-nan", ("row", "x"), 5, NAN, step=-1, clean=_UNREAD),
    _case("unread-row-step2-pinf", ("row", "d"), 0, PINF, steps=2, step=-1, clean=_UNREAD),
)


def dynfit_setup(case, twin=False):
    """-> dict(W: the weight set with its normalisers, M, V: {key: float32 array}, x [300,16], d [300,12], idx [steps,17] int32)"""
    W0 = dr.weight_set(DYNFIT_SET)
    W = {k: np.array(v) for k, v in W0.items()}
    M, V = ({k: np.array(a[k]) for k in a} for a in fr.moments(W0))
    x, d = (np.array(a) for a in fr.buffer())
    idx = fr.step_indices(BATCH, iters=case["steps"]).copy()
    idx[idx == DYNFIT_ROW] = DYNFIT_ROW + 1
    kind = case["target"][0]
    if kind == "row":
        src = idx[max(case["step"], 0), case["pos"]]
        x[DYNFIT_ROW], d[DYNFIT_ROW] = x[src], d[src]
        if case["step"] >= 0:
            idx[case["step"], case["pos"]] = DYNFIT_ROW
    if not twin:
        if kind == "row":
            _poison({"x": x, "d": d}[case["target"][1]][DYNFIT_ROW:DYNFIT_ROW + 1], case["elem"], case["value"])
        else:
            _poison({"w": W, "m": M, "v": V}[kind][case["target"][1]], case["elem"], case["value"])
    return dict(W=W, M=M, V=V, x=x, d=d, idx=idx)


def dynfit_reference(S, with_bound=False):
    """dynfit_ref's fit64, kept step by step -> dict(stats [steps,1] float64: the loss, gflag [steps], nets [steps]; with_bound:
    first = step 1's (loss, G, loss bound, E) of backward64)"""
    f = np.float64
    W = dict(S["W"])
    for k in fr.GRAD_KEYS:
        W[k] = np.asarray(W[k], f).copy()
    M, V = ({k: np.asarray(a[k], f).copy() for k in fr.GRAD_KEYS} for a in (S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    with np.errstate(all="ignore"):
        for s, rows in enumerate(S["idx"]):
            if s == 0 and with_bound:
                loss, G, lb, E = fr.backward64(W, S["x"][rows], S["d"][rows], with_bound=True)
                out["first"] = (np.array([loss]), G, np.array([lb]), E)
            else:
                loss, G = fr.backward64(W, S["x"][rows], S["d"][rows])
            out["stats"].append([loss])
            out["gflag"].append(has_nonfinite(G))
            for k in fr.GRAD_KEYS:
                W[k], M[k], V[k] = fr.adam64(W[k], M[k], V[k], G[k], s + 1, DYNFIT_LR)
            out["nets"].append(has_nonfinite({k: W[k] for k in fr.GRAD_KEYS}))
    return {k: (v if k == "first" else np.asarray(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- behaviour cloning
BC_SET, BC_LR = "he", 1e-2
BC_DATA = ("obs", "act")
_BEYOND = "the entry lies at or beyond counts[s]"

BC_CASES = (
    _case("obs-nan-row3", ("row", "obs"), 5, NAN),
    _case("obs-nan-row16", ("row", "obs"), 0, NAN, pos=16),
    _case("act-nan", ("row", "act"), 2, NAN),
    _case("act-pinf-row16", ("row", "act"), 0, PINF, pos=16),
    _case("obs-ninf", ("row", "obs"), 11, NINF),
    _case("obs-nan-step2", ("row", "obs"), 7, NAN, steps=2, step=1),
    _case("w0-nan", ("w", "w0"), 5 * 128 + 17, NAN),
    _case("w2-nan", ("w", "w2"), 40 * 4 + 1, NAN),
    _case("b1-pinf", ("w", "b1"), 9, PINF),
    _case("m-w1-nan", ("m", "w1"), 1000, NAN, steps=2),
    _case("v-w0-nan", ("v", "w0"), 300, NAN, steps=2),
    _case("unread-row-nan", ("row", "obs"), 5, NAN, step=-1, clean=_UNREAD),
    _case("beyond-count-nan", ("row", "act"), 0, NAN, pos=12, counts=(10,), clean=_BEYOND),
    _case("beyond-count-step2-nan", ("row", "obs"), 1, NAN, pos=16, steps=2, step=1, counts=(17, 16), clean=_BEYOND),
)


def bc_setup(case, twin=False):
    """-> dict(W, M, V: {key: float32 array}, data: (obs, act) with one row more, idx [steps,17] int32, counts or None)"""
    W = {k: np.array(v) for k, v in br.weight_set(BC_SET).items()}
    M, V = ({k: np.array(a[k]) for k in a} for a in br.moments())
    data = [np.concatenate([a, a[:1]]) for a in br.dataset()]
    idx = br.step_indices(BATCH, steps=case["steps"]).copy()
    new = br.N_ROWS
    kind = case["target"][0]
    if kind == "row":
        src = idx[max(case["step"], 0), case["pos"]]
        for a in data:
            a[new] = a[src]
        if case["step"] >= 0:
            idx[case["step"], case["pos"]] = new
    if not twin:
        if kind == "row":
            _poison(data[BC_DATA.index(case["target"][1])][new:new + 1], case["elem"], case["value"])
        else:
            _poison({"w": W, "m": M, "v": V}[kind][case["target"][1]], case["elem"], case["value"])
    counts = None if case.get("counts") is None else np.asarray(case["counts"], np.int32)
    return dict(W=W, M=M, V=V, data=tuple(data), idx=idx, counts=counts)


def bc_reference(S, with_bound=False):
    """bcfit_ref's fit64, kept step by step -> dict(stats [steps,1] float64: the loss, gflag [steps], nets [steps]; with_bound:
    first = step 1's (loss, G, loss bound, E) of backward64)"""
    f = np.float64
    W, M, V = ({k: np.asarray(a[k], f).copy() for k in br.KEYS} for a in (S["W"], S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    with np.errstate(all="ignore"):
        for s, rows in enumerate(S["idx"]):
            rows = rows if S["counts"] is None else rows[:S["counts"][s]]
            if s == 0 and with_bound:
                loss, G, lb, E = br.backward64(W, S["data"][0][rows], S["data"][1][rows], with_bound=True)
                out["first"] = (np.array([loss]), G, np.array([lb]), E)
            else:
                loss, G = br.backward64(W, S["data"][0][rows], S["data"][1][rows])
            out["stats"].append([loss])
            out["gflag"].append(has_nonfinite(G))
            for k in br.KEYS:
                W[k], M[k], V[k] = br.adam64(W[k], M[k], V[k], G[k], s + 1, BC_LR)
            out["nets"].append(has_nonfinite(W))
    return {k: (v if k == "first" else np.asarray(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- GAIL's discriminator
GAIL_HIDDEN, GAIL_LR = 64, 1e-2                    # the 64-wide instantiation
GAIL_DATA = ("gen_obs", "gen_act", "exp_obs", "exp_act")
_CLAMPED_ACT = "an infinite action is its clamped copy"

# (an infinite OBSERVATION, mean or rscale is no case: tanh saturates, every statistic stays finite in the arbiter too, and only
# the gradient of w0 turns NaN through 0 * inf -- neither of the two lists.  An infinite LOGIT (an infinite weight of the last
# layer) is left out as well: torch's binary_cross_entropy_with_logits evaluates (1 - y) l + max(-l, 0) + log1p(exp(-|l|)) and
# returns NaN for the class whose loss is 0 there (0 * inf, -inf + inf), where gail_ref's and the device's softplus give 0)
GAIL_CASES = (
    _case("gen-obs-nan-row3", ("row", "gen_obs"), 5, NAN),
    _case("exp-obs-nan-row16", ("row", "exp_obs"), 0, NAN, pos=16),
    _case("gen-act-nan-row16", ("row", "gen_act"), 2, NAN, pos=16),
    _case("exp-act-nan", ("row", "exp_act"), 1, NAN),
    _case("gen-obs-nan-step2", ("row", "gen_obs"), 7, NAN, steps=2, step=1),
    _case("mean-nan", ("norm", "mean"), 4, NAN),
    _case("rscale-nan", ("norm", "rscale"), 11, NAN),
    _case("w0-nan", ("w", "w0"), 5 * 64 + 17, NAN),
    _case("w2-nan", ("w", "w2"), 40, NAN),
    _case("m-w1-nan", ("m", "w1"), 1000, NAN, steps=2),
    _case("v-w0-nan", ("v", "w0"), 300, NAN, steps=2),
    _case("gen-act-pinf-clamped", ("row", "gen_act"), 2, PINF, clean=_CLAMPED_ACT),
    _case("gen-act-ninf-clamped-row16", ("row", "gen_act"), 0, NINF, pos=16, clean=_CLAMPED_ACT),
    _case("unread-gen-row-nan", ("row", "gen_obs"), 5, NAN, step=-1, clean=_UNREAD),
    _case("unread-exp-row-nan", ("row", "exp_act"), 0, NAN, step=-1, clean=_UNREAD),
    _case("beyond-count-nan", ("row", "exp_obs"), 0, NAN, pos=12, counts=(10,), clean=_BEYOND),
    _case("beyond-count-step2-nan", ("row", "gen_act"), 1, NAN, pos=16, steps=2, step=1, counts=(17, 16), clean=_BEYOND),
)


def gail_setup(case, twin=False):
    """-> dict(W, M, V: {key: float32 array}, gen, exp: (obs, act) with one row more, mean, rscale [12], gi, ei [steps,17] int32,
    counts or None)"""
    W0 = gr.weights(GAIL_HIDDEN)
    W = {k: np.array(W0[k]) for k in gr.KEYS}
    M, V = ({k: np.array(a[k]) for k in gr.KEYS} for a in gr.moments(W0))
    gen, exp, mean, rscale = gr.dataset()
    data = {n: np.concatenate([a, a[:1]]) for n, a in zip(GAIL_DATA, gen + exp)}
    norm = {"mean": np.array(mean), "rscale": np.array(rscale)}
    gi, ei = (a.copy() for a in gr.step_indices(BATCH, steps=case["steps"]))
    kind = case["target"][0]
    if kind == "row":
        cls = case["target"][1][:3]
        idx, new = (gi, gr.N_GEN) if cls == "gen" else (ei, gr.N_EXP)
        src = idx[max(case["step"], 0), case["pos"]]
        for n in (cls + "_obs", cls + "_act"):
            data[n][new] = data[n][src]
        if case["step"] >= 0:
            idx[case["step"], case["pos"]] = new
    value = case["value"]
    if twin:
        value = np.sign(value) if case["clean"] == _CLAMPED_ACT else None
    if value is not None:
        if kind == "row":
            _poison(data[case["target"][1]][-1:], case["elem"], value)
        elif kind == "norm":
            _poison(norm[case["target"][1]], case["elem"], value)
        else:
            _poison({"w": W, "m": M, "v": V}[kind][case["target"][1]], case["elem"], value)
    counts = None if case.get("counts") is None else np.asarray(case["counts"], np.int32)
    return dict(W=W, M=M, V=V, gen=(data["gen_obs"], data["gen_act"]), exp=(data["exp_obs"], data["exp_act"]), mean=norm["mean"],
                rscale=norm["rscale"], gi=gi, ei=ei, counts=counts)


def gail_reference(S, with_bound=False):
    """gail_ref's fit64, kept step by step -> dict(stats [steps,5] float64, gflag [steps], nets [steps]; with_bound: first = step
    1's (stats, G, Es, E) of backward64)"""
    f = np.float64
    W, M, V = ({k: np.asarray(a[k], f).copy() for k in gr.KEYS} for a in (S["W"], S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    with np.errstate(all="ignore"):
        for s in range(S["gi"].shape[0]):
            c = BATCH if S["counts"] is None else int(S["counts"][s])
            g, e = S["gi"][s][:c], S["ei"][s][:c]
            rows = ((S["gen"][0][g], S["gen"][1][g]), (S["exp"][0][e], S["exp"][1][e]), S["mean"], S["rscale"])
            if s == 0 and with_bound:
                st, G, Es, E = gr.backward64(W, *rows, with_bound=True)
                out["first"] = (st, G, Es, E)
            else:
                st, G = gr.backward64(W, *rows)
            out["stats"].append(st)
            out["gflag"].append(has_nonfinite(G))
            for k in gr.KEYS:
                W[k], M[k], V[k] = gr.adam64(W[k], M[k], V[k], G[k], s + 1, GAIL_LR)
            out["nets"].append(has_nonfinite(W))
    return {k: (v if k == "first" else np.asarray(v)) for k, v in out.items()}


# ---- qsg_reward: `rows` rows of the generator's data, one of them (or a weight) poisoned.  1 row, 17 (one 16-row tile and a
# one-row tail), 65 (four tiles and a tail: more than one wave)
def _rcase(cid, rows, row, target, elem, value, clean=None):
    return dict(id=cid, rows=rows, row=row, target=target, elem=elem, value=value, clean=clean)


GAIL_REWARD_CASES = (
    _rcase("r1-obs-nan", 1, 0, "obs", 3, NAN),
    _rcase("r17-act-nan-tail", 17, 16, "act", 1, NAN),
    _rcase("r17-obs-nan-row3", 17, 3, "obs", 0, NAN),
    _rcase("r65-obs-nan-tail", 65, 64, "obs", 11, NAN),
    _rcase("r65-act-nan-row0", 65, 0, "act", 3, NAN),
    _rcase("r65-w1-nan", 65, -1, "w1", 64 * 7 + 9, NAN),
    _rcase("r17-mean-nan", 17, -1, "mean", 2, NAN),
    _rcase("r65-act-pinf-clamped", 65, 33, "act", 0, PINF, clean=_CLAMPED_ACT),
    _rcase("r17-act-ninf-clamped-tail", 17, 16, "act", 2, NINF, clean=_CLAMPED_ACT),
)


def gail_reward_setup(case, twin=False):
    """-> dict(W, obs [rows,12], act [rows,4], mean, rscale)"""
    W = {k: np.array(v) for k, v in gr.weights(GAIL_HIDDEN).items()}
    gen, _, mean, rscale = gr.dataset()
    S = dict(W=W, obs=np.array(gen[0][:case["rows"]]), act=np.array(gen[1][:case["rows"]]), mean=np.array(mean), rscale=np.array(rscale))
    value = case["value"]
    if twin:
        value = np.sign(value) if case["clean"] else None
    if value is not None:
        if case["target"] in ("obs", "act"):
            _poison(S[case["target"]][case["row"]:case["row"] + 1], case["elem"], value)
        elif case["target"] in ("mean", "rscale"):
            _poison(S[case["target"]], case["elem"], value)
        else:
            _poison(W[case["target"]], case["elem"], value)
    return S


def gail_reward_reference(S):
    """-> (reward [rows], logit [rows], bound of the reward, bound of the logit) in float64"""
    with np.errstate(all="ignore"):
        F = gr.forward64(S["W"], S["obs"], S["act"], S["mean"], S["rscale"])
        return gr.reward64(F["l"]), F["l"], gr.reward_bound(F["l"], F["E_l"]), F["E_l"]


# ---------------------------------------------------------------------------------------------------- TD3
TD3_HYPER = dict(gamma=td.GAMMA, tau=td.TAU, actor_lr=1e-2, critic_lr=1e-2, policy_delay=td.DELAY, target_policy_noise=td.SIGMA,
                 target_noise_clip=td.CLIP)
TD3_DATA = ("obs0", "act", "rew", "obs1", "done")
BIG = 1.0e30                                       # a finite value that every clamp and the twin minimum treat as they treat an infinity
_NOISE_CLAMPED = "an infinite normal is clamped to +-CL, as the large finite normal of the twin is"
_MIN_TAKES_Q2 = "qb < qa takes q2's value in every row, as for the twin's large finite q1"
_NOT_READ = "a critic-only update does not read the actor"

# A call starts at update t0 (0: step 1 is an actor update, step 2 a critic-only one; the actor steps taken before are
# ceil(t0 / policy_delay)).  ("noise",): the caller's normal, component `elem` of row slot `pos` of step `step`; the slot's row is a
# copy of its own with done = rowdone.  twin_value: what the twin holds in the poisoned element; hyper: hyper-parameters of the case;
# nets: the nets that hold a non-finite weight after the last step
TD3_CASES = (
    # ---- every input array the step reads
    _case("obs0-nan-row3", ("row", "obs0"), 5, NAN),
    _case("obs0-nan-row16", ("row", "obs0"), 0, NAN, pos=16),
    _case("act-nan", ("row", "act"), 2, NAN),
    _case("rew-nan", ("row", "rew"), 0, NAN, pos=16),
    _case("obs1-nan", ("row", "obs1"), 11, NAN, rowdone=0.0),
    _case("done-nan", ("row", "done"), 0, NAN),
    _case("rew-pinf", ("row", "rew"), 0, PINF),
    _case("act-ninf", ("row", "act"), 0, NINF, pos=16),
    _case("obs0-nan-step2", ("row", "obs0"), 7, NAN, steps=2, step=1),
    # ---- the caller's noise
    _case("noise-nan-live", ("noise",), 2, NAN, rowdone=0.0),
    _case("noise-nan-live-row16", ("noise",), 0, NAN, pos=16, rowdone=0.0),
    _case("noise-pinf-sigma0", ("noise",), 1, PINF, rowdone=0.0, hyper=dict(target_policy_noise=0.0)),
    _case("noise-nan-terminal", ("noise",), 2, NAN, rowdone=1.0, clean=_TERMINAL),
    _case("noise-pinf-clamped", ("noise",), 3, PINF, rowdone=0.0, twin_value=BIG, clean=_NOISE_CLAMPED),
    _case("noise-ninf-clamped-row16", ("noise",), 0, NINF, pos=16, rowdone=0.0, twin_value=-BIG, clean=_NOISE_CLAMPED),
    # ---- weights: layer 0, the last layer; a first and a second moment (they reach a statistic through the weight, in step 2: the
    # critics', since step 2 is a critic-only update)
    _case("actor-w0-nan", ("w", "actor", "w0"), 5 * 128 + 17, NAN),
    _case("q1-w2-nan", ("w", "q1", "w2"), 40, NAN),
    _case("q2-w0-nan", ("w", "q2", "w0"), 13 * 128 + 2, NAN),
    _case("q1-w0-pinf", ("w", "q1", "w0"), 3 * 128 + 2, PINF),
    _case("q1-m-w1-nan", ("m", "q1", "w1"), 1000, NAN, steps=2),
    _case("q2-v-w0-nan", ("v", "q2", "w0"), 300, NAN, steps=2),
    # ---- a target net's weight, every row live
    _case("q1-target-w2-nan-live", ("w", "q1_target", "w2"), 3, NAN, done=0.0),
    _case("q2-target-w1-nan-live", ("w", "q2_target", "w1"), 5 * 128 + 9, NAN, done=0.0),
    _case("actor-target-w0-nan-live", ("w", "actor_target", "w0"), 9, NAN, done=0.0),
    _case("q1-target-b2-ninf-live", ("w", "q1_target", "b2"), 0, NINF, done=0.0),
    # ---- the schedule, policy_delay = 2
    _case("actor-w0-nan-critic-then-actor", ("w", "actor", "w0"), 2 * 128 + 40, NAN, steps=2, t0=1,
          nets=("actor", "actor_target")),
    _case("q1-w1-nan-actor-update", ("w", "q1", "w1"), 7 * 128 + 3, NAN, nets=("actor", "q1", "actor_target", "q1_target")),
    _case("q2-w1-nan-actor-update", ("w", "q2", "w1"), 7 * 128 + 3, NAN, nets=("q2", "q2_target")),
    # (a NaN activation of q1 with finite weights behind it: dq/da's masks hand the term on, the actor's gradient is finite and
    # NOT zero, as autograd's; the actor and its target stay finite)
    _case("q1-b0-nan-actor-update", ("w", "q1", "b0"), 2, NAN, nets=("q1", "q1_target")),
    _case("q1-w0-nan-obs-row-actor-update", ("w", "q1", "w0"), 3 * 128 + 77, NAN, nets=("q1", "q1_target")),
    # ---- clean by contract
    _case("actor-w0-nan-critic-only", ("w", "actor", "w0"), 2 * 128 + 40, NAN, t0=1, nets=("actor",), clean=_NOT_READ),
    _case("q1-target-w2-nan-terminal", ("w", "q1_target", "w2"), 3, NAN, done=1.0, clean=_TERMINAL),
    _case("q2-target-w1-nan-terminal", ("w", "q2_target", "w1"), 5 * 128 + 9, NAN, done=1.0, clean=_TERMINAL),
    _case("actor-target-w0-nan-terminal", ("w", "actor_target", "w0"), 9, NAN, done=1.0, clean=_TERMINAL),
    _case("q1-target-b2-pinf-live", ("w", "q1_target", "b2"), 0, PINF, done=0.0, twin_value=BIG, clean=_MIN_TAKES_Q2),
    _case("obs1-nan-terminal-row", ("row", "obs1"), 11, NAN, rowdone=1.0, clean=_TERMINAL),
    _case("unread-row-nan", ("row", "obs0"), 5, NAN, step=-1, clean=_UNREAD),
    _case("beyond-count-nan", ("row", "rew"), 0, NAN, pos=12, counts=(10,), clean=_BEYOND),
    _case("beyond-count-step2-nan", ("row", "act"), 1, NAN, pos=16, steps=2, step=1, counts=(17, 16), clean=_BEYOND),
)


def td3_setup(case, twin=False):
    """-> dict(P, M, V: {net: {key: float32 array}}, rp: the five arrays with one row more, idx [steps,17] int32, counts or None,
    z [steps,17,4] the caller's normals, t0, actor_t0, hp)"""
    P = {n: {k: np.array(td.nets()[n][k]) for k in td.KEYS} for n in td.NETS}
    M0, V0 = td.moments()
    M = {n: {k: np.array(M0[n][k]) for k in td.KEYS} for n in td.ONLINE}
    V = {n: {k: np.array(V0[n][k]) for k in td.KEYS} for n in td.ONLINE}
    rp = [np.concatenate([a, a[:1]]) for a in td.replay()]
    idx = td.step_indices(BATCH, steps=case["steps"]).copy()
    z = td.noise(case["steps"], BATCH).copy()
    hp = dict(TD3_HYPER, **case.get("hyper", {}))
    new = td.N_ROWS
    kind = case["target"][0]
    if kind in ("row", "noise"):
        src = idx[max(case["step"], 0), case["pos"]]
        for a in rp:
            a[new] = a[src]
        if "rowdone" in case:
            rp[4][new] = case["rowdone"]
        if case["step"] >= 0:
            idx[case["step"], case["pos"]] = new
    if "done" in case:
        rp[4][:] = case["done"]
    value = case.get("twin_value") if twin else case["value"]
    if value is not None:
        if kind == "row":
            _poison(rp[TD3_DATA.index(case["target"][1])][new:new + 1], case["elem"], value)
        elif kind == "noise":
            _poison(z[case["step"], case["pos"]], case["elem"], value)
        else:
            _poison({"w": P, "m": M, "v": V}[kind][case["target"][1]][case["target"][2]], case["elem"], value)
    counts = None if case.get("counts") is None else np.asarray(case["counts"], np.int32)
    t0 = case.get("t0", 0)
    return dict(P=P, M=M, V=V, rp=tuple(rp), idx=idx, counts=counts, z=z, t0=t0, actor_t0=-(-t0 // hp["policy_delay"]), hp=hp)


def td3_reference(S, with_bound=False):
    """td3_ref's loop (fit64's, kept step by step) over a set-up -> dict(stats [steps,6] float64, gflag [steps,3]: a non-finite
    gradient element per online net (False where the step takes no actor gradient), nets [steps,6]: a non-finite weight per net
    after the step; with_bound: first = step 1's (stats, G, Es, E) of step64)"""
    f, hp = np.float64, S["hp"]
    P = {n: {k: np.asarray(S["P"][n][k], f).copy() for k in td.KEYS} for n in td.NETS}
    M = {n: {k: np.asarray(S["M"][n][k], f).copy() for k in td.KEYS} for n in td.ONLINE}
    V = {n: {k: np.asarray(S["V"][n][k], f).copy() for k in td.KEYS} for n in td.ONLINE}
    out, taken = dict(stats=[], gflag=[], nets=[]), 0
    with np.errstate(all="ignore"):
        for s, rows in enumerate(S["idx"]):
            rows = rows if S["counts"] is None else rows[:S["counts"][s]]
            mb, z = tuple(a[rows] for a in S["rp"]), S["z"][s, :len(rows)]
            act = td.actor_step(S["t0"] + s, hp["policy_delay"])
            args = (P, mb, z, hp["gamma"], hp["target_policy_noise"], hp["target_noise_clip"])
            if s == 0 and with_bound:
                st, G, _, Es, E = td.step64(*args, actor=act, with_bound=True)
                out["first"] = (st, G, Es, E)
            else:
                st, G, _ = td.step64(*args, actor=act)
            out["stats"].append(st)
            out["gflag"].append([n in G and has_nonfinite(G[n]) for n in td.ONLINE])
            for n in (td.ONLINE if act else ("q1", "q2")):
                t, lr = (S["actor_t0"] + taken + 1, hp["actor_lr"]) if n == "actor" else (S["t0"] + s + 1, hp["critic_lr"])
                for k in td.KEYS:
                    P[n][k], M[n][k], V[n][k] = td.adam64(P[n][k], M[n][k], V[n][k], G[n][k], t, lr)
                    if act:
                        P[n + "_target"][k] = (1.0 - hp["tau"]) * P[n + "_target"][k] + hp["tau"] * P[n][k]
            taken += int(act)
            out["nets"].append([has_nonfinite(P[n]) for n in td.NETS])
    return {k: (v if k == "first" else np.asarray(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- TRPO's value fit
TRPO_VF_LR = 1e-2
TRPO_KEYS = pr.KEYS_TOWERS                          # the thirteen slots; the fit owns tr.VALUE_KEYS and their moments
_POLICY_SLOT = "the value fit does not read the policy's slots or their moments"

TRPO_VF_CASES = (
    _case("obs-nan-row3", ("row", "obs"), 5, NAN),
    _case("obs-nan-row16", ("row", "obs"), 0, NAN, pos=16),
    _case("returns-nan", ("row", "returns"), 0, NAN),
    _case("returns-pinf-row16", ("row", "returns"), 0, PINF, pos=16),
    _case("obs-ninf", ("row", "obs"), 11, NINF),
    _case("obs-nan-step2", ("row", "obs"), 7, NAN, steps=2, step=1),
    _case("wv0-nan", ("w", "wv0"), 5 * 128 + 17, NAN),
    _case("wv2-nan", ("w", "wv2"), 40, NAN),
    _case("bv1-pinf", ("w", "bv1"), 9, PINF),
    _case("m-wv1-nan", ("m", "wv1"), 1000, NAN, steps=2),
    _case("v-wv0-nan", ("v", "wv0"), 300, NAN, steps=2),
    _case("unread-row-nan", ("row", "obs"), 5, NAN, step=-1, clean=_UNREAD),
    _case("policy-w0-nan", ("w", "w0"), 5 * 128 + 17, NAN, clean=_POLICY_SLOT),
    _case("policy-logstd-nan", ("w", "logstd"), 2, NAN, steps=2, clean=_POLICY_SLOT),
    _case("policy-m-w1-nan", ("m", "w1"), 1000, NAN, steps=2, clean=_POLICY_SLOT),
)


def trpo_vf_indices(steps):
    """[steps,17] int32 rows of the roll-out's 301, every step a draw of its own"""
    return np.stack([np.random.default_rng(500 + s).permutation(tr.N_ROWS)[:BATCH] for s in range(steps)]).astype(np.int32)


def trpo_vf_setup(case, twin=False):
    """-> dict(W, M, V: {the thirteen keys: float32 array} (the moments of the policy's slots are zeros), data: the roll-out's four
    arrays with one row more, idx [steps,17] int32)"""
    W = {k: np.array(tr.weights()[k]) for k in TRPO_KEYS}
    M0, V0 = tr.moments()
    M, V = ({k: np.array(a[k]) if k in a else np.zeros(pr.SHAPES[k], np.float32) for k in TRPO_KEYS} for a in (M0, V0))
    data = {k: np.concatenate([v, v[:1]]) for k, v in tr.rollout().items()}
    idx = trpo_vf_indices(case["steps"])
    new = tr.N_ROWS
    kind = case["target"][0]
    if kind == "row":
        src = idx[max(case["step"], 0), case["pos"]]
        for a in data.values():
            a[new] = a[src]
        if case["step"] >= 0:
            idx[case["step"], case["pos"]] = new
    if not twin:
        if kind == "row":
            _poison(data[case["target"][1]][new:new + 1], case["elem"], case["value"])
        else:
            _poison({"w": W, "m": M, "v": V}[kind][case["target"][1]], case["elem"], case["value"])
    return dict(W=W, M=M, V=V, data=data, idx=idx)


def trpo_vf_reference(S, with_bound=False):
    """trpo_ref's vf_backward64 and Adam, step by step -> dict(stats [steps,1] float64: the loss, gflag [steps], nets [steps]: a
    non-finite weight of the VALUE tower after the step; with_bound: first = step 1's (loss, G, loss bound, E) of vf_backward64)"""
    f = np.float64
    W = dict(S["W"])
    for k in tr.VALUE_KEYS:
        W[k] = np.asarray(W[k], f).copy()
    M, V = ({k: np.asarray(a[k], f).copy() for k in tr.VALUE_KEYS} for a in (S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    with np.errstate(all="ignore"):
        for s, rows in enumerate(S["idx"]):
            obs, ret = S["data"]["obs"][rows], S["data"]["returns"][rows]
            if s == 0 and with_bound:
                loss, G, lb, E = tr.vf_backward64(W, obs, ret, with_bound=True)
                out["first"] = (np.array([loss]), G, np.array([lb]), E)
            else:
                loss, G = tr.vf_backward64(W, obs, ret)
            out["stats"].append([loss])
            out["gflag"].append(has_nonfinite(G))
            for k in tr.VALUE_KEYS:
                W[k], M[k], V[k] = pr.adam64(W[k], M[k], V[k], G[k], s + 1, TRPO_VF_LR, tr.VF_BETA1, tr.VF_BETA2, tr.VF_EPS)
            out["nets"].append(has_nonfinite({k: W[k] for k in tr.VALUE_KEYS}))
    return {k: (v if k == "first" else np.asarray(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- TRPO's policy step
# qst_policy_step takes rows 0 .. n-1, no indices: `row` is the roll-out's own row.  n = 17 (one chunk and a one-row tail);
# fvp_stride 5 takes the Fisher rows 0, 5, 10, 15 (row 16 outside), 4 the rows 0, 4, .. 16 (row 16 inside); three CG iterations and
# three candidates; every case runs at 1 and at 3 slices (tests/test_gpu_nonfinite.py).  entcoeff > 0: surr_before carries the entropy
TRPO_STEP_N, TRPO_STEP_SLICES = 17, (1, 3)
TRPO_STEP_SEED = 211
TRPO_STEP_HP = dict(max_kl=0.01, cg_iters=3, cg_damping=1e-2, entcoeff=0.01, backtracks=3, fvp_stride=5)
TRPO_STEP_DATA = ("obs", "actions", "returns", "values")
_VALUE_SLOT = "the policy step does not read the value tower"
_MOMENT = "the policy step reads no moment"
_BEYOND_N = "the row lies at or beyond n"


def _scase(cid, target, row, elem, value, stride=5, rows=TRPO_STEP_N, clean=None):
    return dict(id=cid, target=target, row=row, elem=elem, value=value, stride=stride, rows=rows, clean=clean)


TRPO_STEP_CASES = (
    _scase("obs-nan-row3", ("row", "obs"), 3, 5, NAN),
    _scase("obs-nan-row16-stride5", ("row", "obs"), 16, 0, NAN),
    _scase("obs-nan-row16-stride4", ("row", "obs"), 16, 0, NAN, stride=4),
    _scase("actions-nan", ("row", "actions"), 3, 2, NAN, stride=4),
    _scase("actions-pinf-row16", ("row", "actions"), 16, 1, PINF),
    _scase("returns-nan", ("row", "returns"), 16, 0, NAN),
    _scase("values-ninf", ("row", "values"), 3, 0, NINF, stride=4),
    _scase("w0-nan", ("w", "w0"), -1, 5 * 128 + 17, NAN),
    _scase("w2-nan", ("w", "w2"), -1, 40 * 4 + 1, NAN, stride=4),
    _scase("logstd-nan", ("w", "logstd"), -1, 2, NAN),
    _scase("b1-pinf", ("w", "b1"), -1, 9, PINF, stride=4),
    _scase("wv0-nan", ("w", "wv0"), -1, 5 * 128 + 17, NAN, clean=_VALUE_SLOT),
    _scase("m-w1-nan", ("m", "w1"), -1, 1000, NAN, stride=4, clean=_MOMENT),
    _scase("v-logstd-nan", ("v", "logstd"), -1, 1, NAN, clean=_MOMENT),
    _scase("m-wv2-nan", ("m", "wv2"), -1, 3, NAN, clean=_MOMENT),
    _scase("row17-of-18-nan", ("row", "obs"), 17, 4, NAN, stride=4, rows=18, clean=_BEYOND_N),
)


def trpo_step_setup(case, twin=False):
    """-> dict(W, M, V: {the thirteen keys: float32 array}, data: the four arrays of case["rows"] rows, n = 17, hp)"""
    W = {k: np.array(tr.weights()[k]) for k in TRPO_KEYS}
    M0, V0 = tr.moments()
    M, V = ({k: np.array(a[k]) if k in a else np.zeros(pr.SHAPES[k], np.float32) for k in TRPO_KEYS} for a in (M0, V0))
    data = {k: np.array(v) for k, v in tr.head(tr.rollout(seed=TRPO_STEP_SEED), case["rows"]).items()}
    if not twin:
        kind = case["target"][0]
        if kind == "row":
            _poison(data[case["target"][1]][case["row"]:case["row"] + 1], case["elem"], case["value"])
        else:
            _poison({"w": W, "m": M, "v": V}[kind][case["target"][1]], case["elem"], case["value"])
    return dict(W=W, M=M, V=V, data=data, n=TRPO_STEP_N, hp=dict(TRPO_STEP_HP, fvp_stride=case["stride"]))


def trpo_step_reference(S):
    """trpo_ref.step64 over the first n rows -> its dict (stats [10], accepted, iters, theta after, G: grad64's dict with bounds) and
    gflag: a non-finite element of g, nets: a non-finite element of theta after the step"""
    with np.errstate(all="ignore"):
        out = tr.step64(S["W"], tr.head(S["data"], S["n"]), **S["hp"])
    out["gflag"], out["nets"] = bool(nonfinite(out["G"]["g"]).any()), bool(nonfinite(out["theta"]).any())
    return out


LIBRARIES = {"ddpg": (DDPG_CASES, ddpg_setup, ddpg_reference), "ppo2": (PPO2_CASES, ppo2_setup, ppo2_reference),
             "dynfit": (DYNFIT_CASES, dynfit_setup, dynfit_reference), "bc": (BC_CASES, bc_setup, bc_reference),
             "gail": (GAIL_CASES, gail_setup, gail_reference), "td3": (TD3_CASES, td3_setup, td3_reference),
             "trpo_vf": (TRPO_VF_CASES, trpo_vf_setup, trpo_vf_reference)}
