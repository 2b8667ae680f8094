"""-m "not gpu": the float64 references at NaN and inf inputs, before the device is held to them (tests/test_gpu_nonfinite.py).

For every case of tests/nonfinite_cases.py the numpy reference's run is compared with a float64 torch autograd restatement of the
same steps -- the ARBITER of the headers' NON-FINITE VALUES paragraph: torch.relu, torch.clamp, torch.maximum / where, MpiAdam's
(tf.train.AdamOptimizer's) formula -- in what the contract speaks of: which statistics are non-finite, whether a net's gradient
holds a non-finite element, whether a net holds a non-finite weight after the step, and element by element what adam64 / update64
make of a non-finite gradient, weight or moment.  For DDPG the restatement is tests/test_ddpg_cpu.py's (its actor and critic, with
the target value selected by torch.where as quadsim_amd.ddpg.torch_ddpg_update selects it), for PPO2 quadsim_amd.ppo2.ppo2_loss,
which tests/test_ppo2_cpu.py holds the reference to on finite data, for GAIL tests/test_gail_cpu.py's (its loss, with the input
row built by torch.clamp), for TD3 quadsim_amd.torch_td3_update on a float64 CPU TD3Policy, one call per step; the dynamics fit and
behaviour cloning have no torch path in the package, and TRPO's torch paths take float32 only, so their restatements (for the
policy step: the header's steps 1 to 7, the Fisher-vector product as double backprop of the mean KL) are written here the same way.
The one place where the arbiter and the contract part on purpose is held explicitly: surr_before and surr_after of a TRPO policy
step are the header's formula sum A / n + entcoeff entropy, finite where autograd's mean(A exp(nlp_old - neglogp)) is NaN.

The tables' conditions are held here and not on the device: a poisoned case makes at least one statistic non-finite in the
arbiter, a clean-by-contract case none, every case is in exactly one of the two lists and no list is empty.  The package's own
update="torch" paths, float32 on the host, give the arbiter's masks."""
import math
import os
import re

import numpy as np
import pytest

import bcfit_ref as br
import ddpg_ref as dd
import dynfit_ref as fr
import dynplan_ref as dr
import gail_ref as gr
import nonfinite_cases as nc
import ppo2_ref as pr
import td3_ref as td
import trpo_ref as tr

ids = lambda cases: [c["id"] for c in cases]     # noqa: E731


def _mask(t):
    return ~np.isfinite(np.asarray(t.detach().numpy() if hasattr(t, "detach") else t, np.float64))


def _any(ts):
    return bool(any(_mask(t).any() for t in ts))


def _adam_t(torch, w, m, v, g, t, lr, beta1, beta2, eps):
    """MpiAdam's / tf.train.AdamOptimizer's step on float64 tensors -> (w', m', v')"""
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return w - lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t) * m / (torch.sqrt(v) + eps), m, v


# ---------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("lib", sorted(nc.LIBRARIES))
def test_every_case_is_in_exactly_one_list_and_no_list_is_empty(lib):
    cases = nc.LIBRARIES[lib][0]
    names = ids(cases)
    assert len(names) == len(set(names))
    poisoned = [c["id"] for c in cases if c["clean"] is None]
    clean = [c["id"] for c in cases if isinstance(c["clean"], str) and c["clean"]]
    assert poisoned and clean and sorted(poisoned + clean) == sorted(names) and not set(poisoned) & set(clean)
    assert {c["value"] != c["value"] or abs(c["value"]) == float("inf") for c in cases} == {True}
    # the shapes the issue names: both row positions, a second-step case, every kind of target
    assert {3, 16} <= {c["pos"] for c in cases if c["target"][0] == "row" and c["step"] >= 0}
    assert any(c["steps"] == 2 and c["step"] == 1 and c["clean"] is None for c in cases)
    assert {"row", "w", "m", "v"} <= {c["target"][0] for c in cases}
    assert all(c["steps"] <= 2 for c in cases)
    print("%s: %d poisoned, %d clean by contract" % (lib, len(poisoned), len(clean)))


def test_the_tables_cover_the_matrix_the_issue_names():
    got = {(c["layout"], c["slices"]) for c in nc.PPO2_CASES}
    assert got == {("shared", 1), ("shared", 3), ("towers", 1), ("towers", 3)}
    for combo in got:
        sub = [c for c in nc.PPO2_CASES if (c["layout"], c["slices"]) == combo]
        assert any(c["clean"] for c in sub) and any(c["clean"] is None for c in sub)
    full = [c for c in nc.PPO2_CASES if (c["layout"], c["slices"]) == ("shared", 1)]
    assert {c["target"][1] for c in full if c["target"][0] == "row"} == set(nc.PPO2_DATA)
    assert {"w0", "w2", "logstd"} <= {c["target"][1] for c in full if c["target"][0] == "w"}
    assert {c["target"][1] for c in nc.DDPG_CASES if c["target"][0] == "row"} == set(nc.DDPG_DATA)
    tw = [c for c in nc.DDPG_CASES if c["target"][0] == "w" and c["target"][1].endswith("_target")]
    assert {(c["done"], c["clean"] is None) for c in tw} == {(0.0, True), (1.0, False)}


# ---------------------------------------------------------------------------------------------------- DDPG
def ddpg_arbiter(S):
    """the steps of a set-up in float64 torch autograd -> what nonfinite_cases.ddpg_reference returns"""
    import torch
    from test_ddpg_cpu import _t_actor, _t_critic
    hp = nc.DDPG_HYPER
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    P = {n: [t64(S["P"][n][k]) for k in dd.KEYS] for n in dd.NETS}
    M = {n: [t64(S["M"][n][k]) for k in dd.KEYS] for n in nc.DDPG_ONLINE}
    V = {n: [t64(S["V"][n][k]) for k in dd.KEYS] for n in nc.DDPG_ONLINE}
    out = dict(stats=[], gflag=[], nets=[])
    for s, rows in enumerate(S["idx"]):
        rows = rows if S["counts"] is None else rows[:S["counts"][s]]
        o0, act, rew, o1, done = (t64(a[rows]) for a in S["rp"])
        o0c, o1c = o0.clamp(-hp["obs_clip"], hp["obs_clip"]), o1.clamp(-hp["obs_clip"], hp["obs_clip"])
        with torch.no_grad():
            q1 = _t_critic(torch, P["critic_target"], o1c, _t_actor(torch, P["actor_target"], o1c))
            y = torch.where(done >= 1.0, rew, rew + (1.0 - done) * hp["gamma"] * q1)
        A = [w.clone().requires_grad_(True) for w in P["actor"]]
        Cr = [w.clone().requires_grad_(True) for w in P["critic"]]
        q = _t_critic(torch, Cr, o0c, act)
        closs = ((q - y) ** 2).mean()
        g_c = torch.autograd.grad(closs, Cr)
        aloss = -_t_critic(torch, [w.detach() for w in Cr], o0c, _t_actor(torch, A, o0c)).mean()
        g_a = torch.autograd.grad(aloss, A)
        out["stats"].append([float(x.detach()) for x in (closs, aloss, q.mean(), y.mean())])
        out["gflag"].append([_any(g_a), _any(g_c)])
        for n, G in (("actor", g_a), ("critic", g_c)):
            for i in range(6):
                P[n][i], M[n][i], V[n][i] = _adam_t(torch, P[n][i], M[n][i], V[n][i], G[i], s + 1, hp[n + "_lr"], dd.BETA1, dd.BETA2, dd.EPS)
                P[n + "_target"][i] = (1.0 - hp["tau"]) * P[n + "_target"][i] + hp["tau"] * P[n][i]
        out["nets"].append([_any(P[n]) for n in dd.NETS])
    return {k: np.asarray(v) for k, v in out.items()}


def _same_masks(ref, arb, what):
    assert np.array_equal(nc.nonfinite(ref["stats"]), nc.nonfinite(arb["stats"])), (what, "statistics", ref["stats"], arb["stats"])
    assert np.array_equal(ref["gflag"], arb["gflag"]), (what, "gradient flags", ref["gflag"], arb["gflag"])
    assert np.array_equal(ref["nets"], arb["nets"]), (what, "net flags", ref["nets"], arb["nets"])
    # where both are finite they are the same numbers (the existing CPU tests hold that on the fixtures; here on the poisoned steps)
    both = ~nc.nonfinite(ref["stats"])
    assert np.allclose(ref["stats"][both], arb["stats"][both], rtol=1e-9, atol=1e-12), (what, ref["stats"], arb["stats"])


def _conditions(case, ref, arb, bound_ok):
    for r in (ref, arb):
        bad = nc.nonfinite(r["stats"])
        if case["clean"] is None:
            assert bad.any(), (case["id"], "a poisoned case with finite statistics", r["stats"])
            if case["steps"] == 2:
                assert not bad[0].any(), (case["id"], "step 1 of a case that poisons step 2", r["stats"])
        else:
            assert not bad.any() and not r["gflag"].any(), (case["id"], case["clean"], r["stats"])
    assert bound_ok, (case["id"], "a finite statistic of step 1 without a finite bound")


@pytest.mark.parametrize("case", nc.DDPG_CASES, ids=ids(nc.DDPG_CASES))
def test_ddpg_reference_against_torch_float64_autograd(case):
    S = nc.ddpg_setup(case)
    ref, arb = nc.ddpg_reference(S, with_bound=True), ddpg_arbiter(S)
    _same_masks(ref, arb, case["id"])
    st, _, Es, _ = ref["first"]
    _conditions(case, ref, arb, bool(np.isfinite(Es[np.isfinite(st)]).all()))
    if case["clean"]:
        # the twin differs in nothing the step reads: the reference gives the same numbers, every one
        tw = nc.ddpg_reference(nc.ddpg_setup(case, twin=True))
        assert np.array_equal(tw["stats"], ref["stats"])
        nets_clean = [n.endswith("_target") and case["target"][:2] == ("w", n) for n in dd.NETS]
        assert np.array_equal(ref["nets"][-1], nets_clean), (case["id"], ref["nets"])


@pytest.mark.parametrize("case", nc.DDPG_CASES, ids=ids(nc.DDPG_CASES))
def test_adam64_keeps_the_non_finite_elements_torch_keeps(case):
    """adam64 on step 1's reference gradient and the case's weights and moments, element by element against MpiAdam's formula in
    torch: the same elements of w, m and v are non-finite"""
    import torch
    S = nc.ddpg_setup(case)
    G = nc.ddpg_reference(S, with_bound=True)["first"][1]
    with np.errstate(all="ignore"):
        for n in nc.DDPG_ONLINE:
            for k in dd.KEYS:
                w, m, v = S["P"][n][k], S["M"][n][k], S["V"][n][k]
                want = _adam_t(torch, *(torch.tensor(np.asarray(a, np.float64)) for a in (w, m, v, G[n][k])), 1, 1e-2, dd.BETA1, dd.BETA2, dd.EPS)
                for got, t in zip(dd.adam64(w, m, v, G[n][k], 1, 1e-2, dd.BETA1, dd.BETA2, dd.EPS), want):
                    assert np.array_equal(nc.nonfinite(got), _mask(t)), (case["id"], n, k)
                    ok = np.isfinite(got)
                    assert np.allclose(got[ok], t.numpy()[ok], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("case", nc.DDPG_CASES, ids=ids(nc.DDPG_CASES))
def test_torch_ddpg_update_on_the_host_gives_the_arbiters_masks(case):
    import torch
    import quadsim_amd as qa
    S = nc.ddpg_setup(case)
    ref = nc.ddpg_reference(S)
    pol = qa.DDPGPolicy(device="cpu", weights={n: {k: S["P"][n][k].copy() for k in dd.KEYS} for n in dd.NETS})
    for n in nc.DDPG_ONLINE:
        pol.m[n] = [torch.as_tensor(S["M"][n][k].copy()) for k in dd.KEYS]
        pol.v[n] = [torch.as_tensor(S["V"][n][k].copy()) for k in dd.KEYS]
    counts = None if S["counts"] is None else torch.as_tensor(S["counts"])
    out = qa.torch_ddpg_update(pol, tuple(torch.as_tensor(a) for a in S["rp"]), torch.as_tensor(S["idx"]), counts, **nc.DDPG_HYPER)
    assert np.array_equal(_mask(out["stats"]), nc.nonfinite(ref["stats"])), (case["id"], out["stats"], ref["stats"])
    assert [_any(getattr(pol, n)) for n in dd.NETS] == list(ref["nets"][-1]), case["id"]


# ---------------------------------------------------------------------------------------------------- PPO2
def _ppo2_clip_adam_t(torch, W, M, V, G, hp, t):
    """tf.clip_by_global_norm and one Adam step on float64 tensors (the arbiter's update) -> (W', M', V')"""
    norm = torch.sqrt(sum((g ** 2).sum() for g in G.values()))
    scale = hp["max_grad_norm"] / torch.clamp(norm, min=hp["max_grad_norm"]) if hp["max_grad_norm"] > 0 else 1.0
    Wn, Mn, Vn = {}, {}, {}
    for k in G:
        Wn[k], Mn[k], Vn[k] = _adam_t(torch, W[k], M[k], V[k], G[k] * scale, t, hp["lr"], pr.BETA1, pr.BETA2, pr.EPS)
    return Wn, Mn, Vn, norm


def ppo2_arbiter(S):
    """the steps of a set-up in float64 torch autograd of quadsim_amd.ppo2.ppo2_loss -> what nonfinite_cases.ppo2_reference returns"""
    import torch
    from quadsim_amd.ppo2 import ppo2_loss
    hp = S["hp"]
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    W, M, V = ({k: t64(a[k]) for k in a} for a in (S["W"], S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    for s, rows in enumerate(S["idx"]):
        d = {k: t64(v[rows]) for k, v in S["data"].items()}
        T = {k: w.clone().requires_grad_(True) for k, w in W.items()}
        loss, parts = ppo2_loss(torch, T, d["obs"], d["actions"], d["returns"], d["values"], d["neglogp"], hp["cliprange"], hp["cliprange_vf"],
                                hp["ent_coef"], hp["vf_coef"])
        G = dict(zip(T, torch.autograd.grad(loss, list(T.values()))))
        W, M, V, norm = _ppo2_clip_adam_t(torch, W, M, V, G, hp, s + 1)
        out["stats"].append([float(p.detach()) for p in parts] + [float(norm)])
        out["gflag"].append(_any(G.values()))
        out["nets"].append(_any(W.values()))
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.mark.parametrize("case", nc.PPO2_CASES, ids=ids(nc.PPO2_CASES))
def test_ppo2_reference_against_torch_float64_autograd(case):
    S = nc.ppo2_setup(case)
    ref, arb = nc.ppo2_reference(S, with_bound=True), ppo2_arbiter(S)
    # (the reference clips the ratio at float32(1 +- eps), torch at the doubles: 1e-8 of a clipped row's term)
    both = ~nc.nonfinite(ref["stats"]) & ~nc.nonfinite(arb["stats"])
    assert np.allclose(ref["stats"][both], arb["stats"][both], rtol=1e-6, atol=1e-9), (case["id"], ref["stats"], arb["stats"])
    arb["stats"] = np.where(both, ref["stats"], arb["stats"])
    _same_masks(ref, arb, case["id"])
    st, _, SB, _ = ref["first"]
    _conditions(case, ref, arb, bool(np.isfinite(SB[np.isfinite(st)]).all()))
    if case["clean"]:
        tw = nc.ppo2_reference(nc.ppo2_setup(case, twin=True))
        assert np.array_equal(tw["stats"], ref["stats"]) and not ref["nets"].any()


@pytest.mark.parametrize("case", [c for c in nc.PPO2_CASES if (c["layout"], c["slices"]) in (("shared", 1), ("towers", 3))],
                         ids=lambda c: c["id"])
def test_update64_keeps_the_non_finite_elements_torch_keeps(case):
    """update64 (the global-norm clip and adam64) on step 1's reference gradient, element by element against the arbiter's
    update: a non-finite norm spoils every element, as tf.clip_by_global_norm does"""
    import torch
    S = nc.ppo2_setup(case)
    G = nc.ppo2_reference(S, with_bound=True)["first"][1]
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    with np.errstate(all="ignore"):
        got = pr.update64(S["W"], S["M"], S["V"], G, S["hp"], 1)
    want = _ppo2_clip_adam_t(torch, *({k: t64(a[k]) for k in G} for a in (S["W"], S["M"], S["V"], G)), S["hp"], 1)
    assert bool(np.isfinite(got[4])) == bool(np.isfinite(float(want[3])))
    for g, t in zip(got[:3], want[:3]):
        for k in G:
            assert np.array_equal(nc.nonfinite(g[k]), _mask(t[k])), (case["id"], k)
            ok = np.isfinite(g[k])
            assert np.allclose(g[k][ok], t[k].numpy()[ok], rtol=1e-12, atol=0.0)
    if case["clean"] is None and case["steps"] == 1:
        assert all(nc.nonfinite(got[0][k]).all() for k in G), "a poisoned step with the clip on leaves no element finite"


@pytest.mark.parametrize("case", nc.PPO2_CASES, ids=ids(nc.PPO2_CASES))
def test_torch_ppo2_update_on_the_host_gives_the_arbiters_masks(case):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import ppo2
    S = nc.ppo2_setup(case)
    ref, hp = nc.ppo2_reference(S), S["hp"]
    pol = qa.ActorCriticPolicy({k: v.copy() for k, v in S["W"].items()}, device="cpu")
    ws = ppo2.policy_tensors(pol)
    ppo2.reset_ppo2_optimizer(pol)
    pol._ppo_m = [None if w is None else torch.as_tensor(S["M"][k].copy()) for k, w in zip(ppo2.SLOT_KEYS, ws)]
    pol._ppo_v = [None if w is None else torch.as_tensor(S["V"][k].copy()) for k, w in zip(ppo2.SLOT_KEYS, ws)]
    out = ppo2.torch_ppo2_update(pol, {k: torch.as_tensor(v) for k, v in S["data"].items()}, torch.as_tensor(S["idx"]), learning_rate=hp["lr"],
                                 cliprange=hp["cliprange"], cliprange_vf=hp["cliprange_vf"], ent_coef=hp["ent_coef"], vf_coef=hp["vf_coef"],
                                 max_grad_norm=hp["max_grad_norm"])
    assert np.array_equal(_mask(out["stats"]), nc.nonfinite(ref["stats"])), (case["id"], out["stats"], ref["stats"])
    assert _any(w for w in ppo2.policy_tensors(pol) if w is not None) == bool(ref["nets"][-1]), case["id"]


# ---------------------------------------------------------------------------------------------------- the dynamics fit
def dynfit_arbiter(S):
    """the steps of a set-up in float64 torch autograd -> what nonfinite_cases.dynfit_reference returns"""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    W = S["W"]
    P, M, V = ({k: t64(a[k]) for k in fr.GRAD_KEYS} for a in (W, S["M"], S["V"]))
    in_mean, in_rs, out_mean, out_rs = t64(W["in_mean"]), t64(dr.rscale(W)), t64(W["out_mean"]), t64(fr.out_rscale(W))
    out = dict(stats=[], gflag=[], nets=[])
    for s, rows in enumerate(S["idx"]):
        T = {k: w.clone().requires_grad_(True) for k, w in P.items()}
        h = (t64(S["x"][rows]) - in_mean) * in_rs
        h = torch.relu(h @ T["w1"].T + T["b1"])
        h = torch.relu(h @ T["w2"].T + T["b2"])
        loss = ((h @ T["w3"].T + T["b3"] - (t64(S["d"][rows]) - out_mean) * out_rs) ** 2).mean()
        G = dict(zip(T, torch.autograd.grad(loss, list(T.values()))))
        for k in fr.GRAD_KEYS:
            P[k], M[k], V[k] = _adam_t(torch, P[k], M[k], V[k], G[k], s + 1, nc.DYNFIT_LR, fr.BETA1, fr.BETA2, fr.EPS)
        out["stats"].append([float(loss.detach())])
        out["gflag"].append(_any(G.values()))
        out["nets"].append(_any(P.values()))
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.mark.parametrize("case", nc.DYNFIT_CASES, ids=ids(nc.DYNFIT_CASES))
def test_dynfit_reference_against_torch_float64_autograd(case):
    import torch
    S = nc.dynfit_setup(case)
    assert S["W"]["w1"].shape == (64, 16) and S["W"]["w2"].shape == (64, 64)          # the (64, 64) instantiation
    ref, arb = nc.dynfit_reference(S, with_bound=True), dynfit_arbiter(S)
    _same_masks(ref, arb, case["id"])
    st, G, lb, _ = ref["first"]
    _conditions(case, ref, arb, bool(np.isfinite(lb[np.isfinite(st)]).all()))
    if case["clean"]:
        tw = nc.dynfit_reference(nc.dynfit_setup(case, twin=True))
        assert np.array_equal(tw["stats"], ref["stats"]) and not ref["nets"].any()
    # adam64 on step 1's gradient, element by element against the formula in torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    with np.errstate(all="ignore"):
        for k in fr.GRAD_KEYS:
            want = _adam_t(torch, *(t64(a) for a in (S["W"][k], S["M"][k], S["V"][k], G[k])), 1, nc.DYNFIT_LR, fr.BETA1, fr.BETA2, fr.EPS)
            for got, t in zip(fr.adam64(S["W"][k], S["M"][k], S["V"][k], G[k], 1, nc.DYNFIT_LR), want):
                assert np.array_equal(nc.nonfinite(got), _mask(t)), (case["id"], k)
                ok = np.isfinite(got)
                assert np.allclose(got[ok], t.numpy()[ok], rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------------------------------------------- behaviour cloning
def bc_arbiter(S):
    """the steps of a set-up in float64 torch autograd -> what nonfinite_cases.bc_reference returns"""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    P, M, V = ({k: t64(a[k]) for k in br.KEYS} for a in (S["W"], S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    for s, rows in enumerate(S["idx"]):
        rows = rows if S["counts"] is None else rows[:S["counts"][s]]
        T = {k: w.clone().requires_grad_(True) for k, w in P.items()}
        h = torch.relu(t64(S["data"][0][rows]) @ T["w0"] + T["b0"])
        h = torch.relu(h @ T["w1"] + T["b1"])
        loss = ((h @ T["w2"] + T["b2"] - t64(S["data"][1][rows])) ** 2).mean()
        G = dict(zip(T, torch.autograd.grad(loss, list(T.values()))))
        for k in br.KEYS:
            P[k], M[k], V[k] = _adam_t(torch, P[k], M[k], V[k], G[k], s + 1, nc.BC_LR, br.BETA1, br.BETA2, br.EPS)
        out["stats"].append([float(loss.detach())])
        out["gflag"].append(_any(G.values()))
        out["nets"].append(_any(P.values()))
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.mark.parametrize("case", nc.BC_CASES, ids=ids(nc.BC_CASES))
def test_bc_reference_against_torch_float64_autograd(case):
    import torch
    S = nc.bc_setup(case)
    ref, arb = nc.bc_reference(S, with_bound=True), bc_arbiter(S)
    _same_masks(ref, arb, case["id"])
    st, G, lb, _ = ref["first"]
    _conditions(case, ref, arb, bool(np.isfinite(lb[np.isfinite(st)]).all()))
    if case["clean"]:
        tw = nc.bc_reference(nc.bc_setup(case, twin=True))
        assert np.array_equal(tw["stats"], ref["stats"]) and not ref["nets"].any()
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    with np.errstate(all="ignore"):
        for k in br.KEYS:
            want = _adam_t(torch, *(t64(a) for a in (S["W"][k], S["M"][k], S["V"][k], G[k])), 1, nc.BC_LR, br.BETA1, br.BETA2, br.EPS)
            for got, t in zip(br.adam64(S["W"][k], S["M"][k], S["V"][k], G[k], 1, nc.BC_LR), want):
                assert np.array_equal(nc.nonfinite(got), _mask(t)), (case["id"], k)
                ok = np.isfinite(got)
                assert np.allclose(got[ok], t.numpy()[ok], rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------------------------------------------- the recorded instruction diff
def test_the_libraries_that_include_no_touched_kernel_are_instruction_identical():
    """profiles/nonfinite/isa_diff.txt is the output of tools/isa_diff.py, the parent commit's build against this one, for all
    eight libraries: the main library and both planners (whose kernels inline none of the changed functions) say `same` for
    every kernel; no kernel of any library appeared or went, and none gained scratch, a spill or LDS"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "nonfinite", "isa_diff.txt")).read()
    parts = dict(zip(re.findall(r"^## (\S+)$", text, flags=re.M), re.split(r"^## \S+$", text, flags=re.M)[1:]))
    assert list(parts) == ["libquadsim_%s.so" % n for n in ("hip", "dyn", "dynmppi", "dynfit", "bc", "ppo", "gail", "ddpg")]
    for lib, body in parts.items():
        (a, b), = re.findall(r"^identical in fields and disassembly: (\d+) of (\d+)$", body, flags=re.M)
        assert "only in parent [], only in branch []" in body, lib
        assert not re.search(r"(spill_count|private_segment_fixed_size|group_segment_fixed_size) \d+ ->", body), lib
        if lib in ("libquadsim_hip.so", "libquadsim_dyn.so", "libquadsim_dynmppi.so"):
            assert a == b and int(a) > 0, lib
        else:
            assert int(a) < int(b), lib


# ---------------------------------------------------------------------------------------------------- GAIL's discriminator
def _gail_x(torch, obs, act, mean, rscale):
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    return torch.cat([(t64(obs) - t64(mean)) * t64(rscale), t64(act).clamp(-1.0, 1.0)], 1)


def gail_arbiter(S):
    """the steps of a set-up in float64 torch autograd of tests/test_gail_cpu.py's loss -> what nonfinite_cases.gail_reference
    returns (the two accuracies are counted as the device counts them)"""
    import torch
    from test_gail_cpu import _torch_total
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    P, M, V = ({k: t64(a[k]) for k in gr.KEYS} for a in (S["W"], S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    for s in range(S["gi"].shape[0]):
        c = nc.BATCH if S["counts"] is None else int(S["counts"][s])
        g, e = S["gi"][s][:c], S["ei"][s][:c]
        x = torch.cat([_gail_x(torch, S["gen"][0][g], S["gen"][1][g], S["mean"], S["rscale"]),
                       _gail_x(torch, S["exp"][0][e], S["exp"][1][e], S["mean"], S["rscale"])])
        T = {k: w.clone().requires_grad_(True) for k, w in P.items()}
        total, parts = _torch_total(torch, T, x, c, gr.ENTCOEFF)
        G = dict(zip(T, torch.autograd.grad(total, list(T.values()))))
        with torch.no_grad():
            l = (torch.tanh(torch.tanh(x @ P["w0"] + P["b0"]) @ P["w1"] + P["b1"]) @ P["w2"] + P["b2"])[:, 0]
            acc = [float((l[:c] < 0).double().mean()), float((l[c:] > 0).double().mean())]
        for k in gr.KEYS:
            P[k], M[k], V[k] = _adam_t(torch, P[k], M[k], V[k], G[k], s + 1, nc.GAIL_LR, gr.BETA1, gr.BETA2, gr.EPS)
        out["stats"].append([float(p.detach()) for p in parts] + acc)
        out["gflag"].append(_any(G.values()))
        out["nets"].append(_any(P.values()))
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.mark.parametrize("case", nc.GAIL_CASES, ids=ids(nc.GAIL_CASES))
def test_gail_reference_against_torch_float64_autograd(case):
    import torch
    S = nc.gail_setup(case)
    assert gr.hidden_of(S["W"]) == 64
    ref, arb = nc.gail_reference(S, with_bound=True), gail_arbiter(S)
    _same_masks(ref, arb, case["id"])
    st, G, Es, _ = ref["first"]
    _conditions(case, ref, arb, bool(np.isfinite(Es[np.isfinite(st)]).all()))
    if case["clean"]:
        tw = nc.gail_reference(nc.gail_setup(case, twin=True))
        assert np.array_equal(tw["stats"], ref["stats"]) and not ref["nets"].any()
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    with np.errstate(all="ignore"):
        for k in gr.KEYS:
            want = _adam_t(torch, *(t64(a) for a in (S["W"][k], S["M"][k], S["V"][k], G[k])), 1, nc.GAIL_LR, gr.BETA1, gr.BETA2, gr.EPS)
            for got, t in zip(gr.adam64(S["W"][k], S["M"][k], S["V"][k], G[k], 1, nc.GAIL_LR), want):
                assert np.array_equal(nc.nonfinite(got), _mask(t)), (case["id"], k)
                ok = np.isfinite(got)
                assert np.allclose(got[ok], t.numpy()[ok], rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("case", nc.GAIL_REWARD_CASES, ids=ids(nc.GAIL_REWARD_CASES))
def test_gail_reward_reference_against_torch_float64(case):
    """the reward and the logit row by row: non-finite in the rows torch makes non-finite -- the poisoned row alone, or every row
    for a weight or a statistic -- and the other rows the twin's numbers"""
    import torch
    S = nc.gail_reward_setup(case)
    rew, l, _, _ = nc.gail_reward_reference(S)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    x = _gail_x(torch, S["obs"], S["act"], S["mean"], S["rscale"])
    W = {k: t64(S["W"][k]) for k in gr.KEYS}
    tl = (torch.tanh(torch.tanh(x @ W["w0"] + W["b0"]) @ W["w1"] + W["b1"]) @ W["w2"] + W["b2"])[:, 0]
    tr = -torch.log(1.0 - torch.sigmoid(tl) + 1.0e-8)
    assert np.array_equal(nc.nonfinite(l), _mask(tl)) and np.array_equal(nc.nonfinite(rew), _mask(tr)), case["id"]
    ok = np.isfinite(rew)
    assert np.allclose(rew[ok], tr.numpy()[ok], rtol=1e-9, atol=1e-12) and np.allclose(l[ok], tl.numpy()[ok], rtol=1e-9, atol=1e-12)
    want = np.zeros(case["rows"], bool)
    if case["clean"] is None:
        want[case["row"] if case["row"] >= 0 else slice(None)] = True
    assert np.array_equal(nc.nonfinite(rew), want) and np.array_equal(nc.nonfinite(l), want), (case["id"], rew)
    tw = nc.gail_reward_reference(nc.gail_reward_setup(case, twin=True))
    assert np.array_equal(tw[0][~want], rew[~want]) and np.isfinite(tw[0]).all()


def test_the_reward_table_has_both_lists_and_the_three_row_counts():
    cases = nc.GAIL_REWARD_CASES
    assert len({c["id"] for c in cases}) == len(cases) and {c["rows"] for c in cases} == {1, 17, 65}
    assert any(c["clean"] for c in cases) and any(c["clean"] is None for c in cases)
    assert {"obs", "act", "mean"} <= {c["target"] for c in cases} and any(c["target"].startswith("w") for c in cases)


@pytest.mark.parametrize("case", [c for c in nc.GAIL_CASES if c["target"][0] != "norm"], ids=lambda c: c["id"])
def test_torch_discriminator_fit_on_the_host_gives_the_arbiters_masks(case):
    """(the wrapper takes mean and rscale from the discriminator's own running statistics, left as they are here: the reference
    runs with those; the two cases that poison the statistics themselves have no wrapper form)"""
    import torch
    import quadsim_amd as qa
    S = nc.gail_setup(case)
    d = qa.Discriminator(hidden=nc.GAIL_HIDDEN, device="cpu", weights={k: v.copy() for k, v in S["W"].items()})
    d.m = [torch.as_tensor(S["M"][k].copy()) for k in gr.KEYS]
    d.v = [torch.as_tensor(S["V"][k].copy()) for k in gr.KEYS]

    class E:
        obs, actions = torch.as_tensor(S["exp"][0]), torch.as_tensor(S["exp"][1])
    counts = None if S["counts"] is None else torch.as_tensor(S["counts"])
    out = qa.torch_discriminator_fit(d, torch.as_tensor(S["gen"][0]), torch.as_tensor(S["gen"][1]), E, torch.as_tensor(S["gi"]),
                                     torch.as_tensor(S["ei"]), counts, lr=nc.GAIL_LR, update_stats=False)
    mt, rt = d.norm_tensors()
    ref = nc.gail_reference(dict(S, mean=mt.numpy(), rscale=rt.numpy()))
    assert np.array_equal(_mask(out["stats"]), nc.nonfinite(ref["stats"])), (case["id"], out["stats"], ref["stats"])
    assert _any(d.tensors()) == bool(ref["nets"][-1]), case["id"]
    assert nc.nonfinite(ref["stats"]).any() == (case["clean"] is None)


# ---------------------------------------------------------------------------------------------------- TD3
def td3_arbiter(S):
    """the steps of a set-up in quadsim_amd.torch_td3_update on a float64 CPU TD3Policy, one call per step with the step counts the
    policy carries -> what nonfinite_cases.td3_reference returns"""
    import torch
    import quadsim_amd as qa
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    pol = qa.TD3Policy(device="cpu", weights={n: {k: np.asarray(S["P"][n][k], np.float64) for k in td.KEYS} for n in td.NETS}, dtype="float64")
    for n in td.ONLINE:
        pol.m[n], pol.v[n] = [t64(S["M"][n][k]) for k in td.KEYS], [t64(S["V"][n][k]) for k in td.KEYS]
    pol.steps, pol.actor_steps = S["t0"], S["actor_t0"]
    rp = tuple(torch.as_tensor(a) for a in S["rp"])
    out = dict(stats=[], gflag=[], nets=[])
    for s in range(S["idx"].shape[0]):
        counts = None if S["counts"] is None else torch.as_tensor(S["counts"][s:s + 1])
        o = qa.torch_td3_update(pol, rp, torch.as_tensor(S["idx"][s:s + 1]), counts, noise=torch.as_tensor(S["z"][s:s + 1]), return_grads=True,
                                **S["hp"])
        out["stats"].append(o["stats"][0].numpy())
        if s == 0:
            first = {n: [g.numpy().copy() for g in o["grads"][n]] for n in td.ONLINE if o["grads"][n] is not None}
        out["gflag"].append([o["grads"][n] is not None and _any(o["grads"][n]) for n in td.ONLINE])
        out["nets"].append([_any(getattr(pol, n)) for n in td.NETS])
    assert pol.steps == S["t0"] + S["idx"].shape[0]
    return dict({k: np.asarray(v) for k, v in out.items()}, first=first)


def _twin_rows_are_off_every_relu_edge(edges):
    assert not np.asarray(edges).any(), "a twin's row lies on a ReLU edge: the fixtures' census does not hold for it"


@pytest.mark.parametrize("case", nc.TD3_CASES, ids=ids(nc.TD3_CASES))
def test_td3_reference_against_torch_float64_autograd(case):
    S = nc.td3_setup(case)
    ref, arb = nc.td3_reference(S, with_bound=True), td3_arbiter(S)
    _same_masks(ref, arb, case["id"])
    st, G, Es, _ = ref["first"]
    _conditions(case, ref, arb, bool(np.isfinite(Es[np.isfinite(st)]).all()))
    # step 1's gradients: the elements finite in both are the same numbers (a NaN activation of q1 hands dq/da's term on in both)
    assert set(G) == set(arb["first"])
    for n in G:
        for k, g in zip(td.KEYS, arb["first"][n]):
            both = np.isfinite(G[n][k]) & np.isfinite(g.reshape(G[n][k].shape))
            assert np.allclose(G[n][k][both], g.reshape(G[n][k].shape)[both], rtol=1e-7, atol=1e-12), (case["id"], n, k)
    if "nets" in case:
        assert [n for n, bad in zip(td.NETS, ref["nets"][-1]) if bad] == [n for n in td.NETS if n in case["nets"]], (case["id"], ref["nets"])
    T = nc.td3_setup(case, twin=True)
    for s, rows in enumerate(T["idx"]):
        rows = rows if T["counts"] is None else rows[:T["counts"][s]]
        _twin_rows_are_off_every_relu_edge(td.relu_edges(T["P"], tuple(a[rows] for a in T["rp"])))
    if case["clean"]:
        # the twin differs in nothing that reaches a result: the reference gives the same numbers, every one
        tw = nc.td3_reference(T)
        assert np.array_equal(tw["stats"], ref["stats"]) and not tw["nets"].any()
        own = [case["target"][:2] == ("w", n) for n in td.NETS]          # a poisoned weight stays what it was given, and nothing else
        assert np.array_equal(ref["nets"][-1], own), (case["id"], ref["nets"])
        if case["clean"] == nc._NOT_READ:
            assert ref["stats"][0, 5] == 0.0 and arb["stats"][0, 5] == 0.0 and not np.signbit(ref["stats"][0, 5])


@pytest.mark.parametrize("case", nc.TD3_CASES, ids=ids(nc.TD3_CASES))
def test_td3_adam64_keeps_the_non_finite_elements_torch_keeps(case):
    """adam64 on step 1's reference gradient and the case's weights and moments, element by element against the formula in torch"""
    import torch
    S = nc.td3_setup(case)
    G = nc.td3_reference(S, with_bound=True)["first"][1]
    with np.errstate(all="ignore"):
        for n in G:
            t = (S["actor_t0"] if n == "actor" else S["t0"]) + 1
            for k in td.KEYS:
                w, m, v = S["P"][n][k], S["M"][n][k], S["V"][n][k]
                want = _adam_t(torch, *(torch.tensor(np.asarray(a, np.float64)) for a in (w, m, v, G[n][k])), t, 1e-2, td.BETA1, td.BETA2, td.EPS)
                for got, tt in zip(td.adam64(w, m, v, G[n][k], t, 1e-2, td.BETA1, td.BETA2, td.EPS), want):
                    assert np.array_equal(nc.nonfinite(got), _mask(tt)), (case["id"], n, k)
                    ok = np.isfinite(got)
                    assert np.allclose(got[ok], tt.numpy()[ok], rtol=1e-12, atol=0.0)


def test_the_td3_table_covers_what_the_issue_names():
    cases = nc.TD3_CASES
    by = {c["id"]: c for c in cases}
    assert {c["target"][1] for c in cases if c["target"][0] == "row" and c["clean"] is None} == set(nc.TD3_DATA)
    noise = [c for c in cases if c["target"][0] == "noise"]
    assert {(c["rowdone"], c["clean"] is None) for c in noise if c["value"] != c["value"]} == {(0.0, True), (1.0, False)}
    assert {c["value"] for c in noise if c["clean"] == nc._NOISE_CLAMPED} == {nc.PINF, nc.NINF}
    assert by["noise-pinf-sigma0"]["hyper"] == dict(target_policy_noise=0.0) and by["noise-pinf-sigma0"]["clean"] is None
    tw = [c for c in cases if c["target"][0] == "w" and c["target"][1].endswith("_target") and c["value"] != c["value"]]
    assert {(c["target"][1], c["done"], c["clean"] is None) for c in tw} == {(n, d, d == 0.0) for n in ("actor_target", "q1_target", "q2_target")
                                                                             for d in (0.0, 1.0)}
    assert by["q1-target-b2-pinf-live"]["clean"] and by["q1-target-b2-ninf-live"]["clean"] is None
    assert by["actor-w0-nan-critic-only"]["t0"] == 1 and by["actor-w0-nan-critic-then-actor"]["t0"] == 1
    assert {c["target"][:2] for c in cases if c["target"][0] in ("m", "v")} == {("m", "q1"), ("v", "q2")}
    assert {"unread-row-nan", "beyond-count-nan", "beyond-count-step2-nan"} <= set(by)


# ---------------------------------------------------------------------------------------------------- TRPO's value fit
def trpo_vf_arbiter(S):
    """the steps of a set-up in float64 torch autograd -> what nonfinite_cases.trpo_vf_reference returns"""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    P, M, V = ({k: t64(a[k]) for k in tr.VALUE_KEYS} for a in (S["W"], S["M"], S["V"]))
    out = dict(stats=[], gflag=[], nets=[])
    for s, rows in enumerate(S["idx"]):
        T = {k: w.clone().requires_grad_(True) for k, w in P.items()}
        h = torch.relu(t64(S["data"]["obs"][rows]) @ T["wv0"] + T["bv0"])
        h = torch.relu(h @ T["wv1"] + T["bv1"])
        loss = (((h @ T["wv2"] + T["bv2"])[:, 0] - t64(S["data"]["returns"][rows])) ** 2).mean()
        G = dict(zip(T, torch.autograd.grad(loss, list(T.values()))))
        for k in tr.VALUE_KEYS:
            P[k], M[k], V[k] = _adam_t(torch, P[k], M[k], V[k], G[k], s + 1, nc.TRPO_VF_LR, tr.VF_BETA1, tr.VF_BETA2, tr.VF_EPS)
        out["stats"].append([float(loss.detach())])
        out["gflag"].append(_any(G.values()))
        out["nets"].append(_any(P.values()))
    return {k: np.asarray(v) for k, v in out.items()}


@pytest.mark.parametrize("case", nc.TRPO_VF_CASES, ids=ids(nc.TRPO_VF_CASES))
def test_trpo_vf_reference_against_torch_float64_autograd(case):
    import torch
    S = nc.trpo_vf_setup(case)
    ref, arb = nc.trpo_vf_reference(S, with_bound=True), trpo_vf_arbiter(S)
    _same_masks(ref, arb, case["id"])
    st, G, lb, _ = ref["first"]
    _conditions(case, ref, arb, bool(np.isfinite(lb[np.isfinite(st)]).all()))
    T = nc.trpo_vf_setup(case, twin=True)
    for rows in T["idx"]:
        _twin_rows_are_off_every_relu_edge(tr.relu_edges(T["W"], T["data"]["obs"][rows]))
    if case["clean"]:
        tw = nc.trpo_vf_reference(T)
        assert np.array_equal(tw["stats"], ref["stats"]) and not ref["nets"].any()
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    with np.errstate(all="ignore"):
        for k in tr.VALUE_KEYS:
            want = _adam_t(torch, *(t64(a) for a in (S["W"][k], S["M"][k], S["V"][k], G[k])), 1, nc.TRPO_VF_LR, tr.VF_BETA1, tr.VF_BETA2, tr.VF_EPS)
            for got, t in zip(pr.adam64(S["W"][k], S["M"][k], S["V"][k], G[k], 1, nc.TRPO_VF_LR, tr.VF_BETA1, tr.VF_BETA2, tr.VF_EPS), want):
                assert np.array_equal(nc.nonfinite(got), _mask(t)), (case["id"], k)
                ok = np.isfinite(got)
                assert np.allclose(got[ok], t.numpy()[ok], rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------------------------------------------- TRPO's policy step
def trpo_step_arbiter(S):
    """the header's steps 1 to 7 in float64 torch autograd: the surrogate mean(A exp(nlp_old - neglogp)) + entcoeff entropy and its
    gradient, the Fisher-vector product as double backprop of the mean KL over every fvp_stride-th row, SB2's cg and line search
    (quadsim_amd.trpo.torch_trpo_policy_step's loop, whose head, neglogp and KL it takes, in float64 throughout) -> dict(stats [10],
    gflag, nets: a non-finite element of theta after the step, accepted, iters)"""
    import torch
    from quadsim_amd.trpo import _mean_kl, _neglogp, _policy_head
    hp, n = S["hp"], S["n"]
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    obs, actions, returns, values = (t64(S["data"][k][:n]) for k in nc.TRPO_STEP_DATA)
    theta = torch.cat([t64(S["W"][k]).reshape(-1) for k in tr.POLICY_KEYS])
    unflat = lambda vec: {k: p.view(tr.SHAPES[k]) for k, p in zip(tr.POLICY_KEYS, torch.split(vec, tr.SIZES))}      # noqa: E731
    adv = returns - values
    adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    with torch.no_grad():
        P0 = unflat(theta)
        mean_old, ls_old = _policy_head(torch, P0, obs), P0["logstd"].clone()
        nlp_old = _neglogp(torch, mean_old, ls_old, actions)

    def losses(vec):
        P = unflat(vec)
        mean = _policy_head(torch, P, obs)
        ent = (P["logstd"] + 0.5 * math.log(2.0 * math.pi * math.e)).sum()
        surr = (adv * torch.exp(nlp_old - _neglogp(torch, mean, P["logstd"], actions))).mean() + hp["entcoeff"] * ent
        return surr, _mean_kl(torch, mean_old, ls_old, mean, P["logstd"]), ent

    def fvp(vec):
        th = theta.clone().requires_grad_(True)
        P = unflat(th)
        kl = _mean_kl(torch, mean_old[::hp["fvp_stride"]], ls_old, _policy_head(torch, P, obs[::hp["fvp_stride"]]), P["logstd"])
        (gk,) = torch.autograd.grad(kl, th, create_graph=True)
        (hv,) = torch.autograd.grad((gk * vec).sum(), th)
        return hv + hp["cg_damping"] * vec

    th = theta.clone().requires_grad_(True)
    surr_before, _, ent0 = losses(th)
    (g,) = torch.autograd.grad(surr_before, th)
    surr_before = float(surr_before)
    stats = [surr_before, surr_before, 0.0, float(ent0), float(g.norm()), 0.0, 0.0, 0.0, -2.0, 0.0]
    new_theta = theta
    if float((g ** 2).sum()) != 0.0:
        x, r, p = torch.zeros_like(g), g.clone(), g.clone()
        rdotr, iters = float(r.dot(r)), 0
        for _ in range(hp["cg_iters"]):
            z = fvp(p)
            a = rdotr / float(p.dot(z))
            x, r = x + a * p, r - a * z
            new = float(r.dot(r))
            p, rdotr, iters = r + (new / rdotr) * p, new, iters + 1
            if rdotr < 1e-10:
                break
        shs = 0.5 * float(x.dot(fvp(x)))
        lm = math.sqrt(shs / hp["max_kl"]) if shs >= 0.0 else float("nan")
        fullstep = x / lm
        stats[5:10] = [shs, lm, float(g.dot(fullstep)), -1.0, float(iters)]
        with torch.no_grad():
            for k in range(hp["backtracks"]):
                cand = theta + fullstep * 0.5 ** k
                surr, kl, ent = (float(v) for v in losses(cand))
                if math.isfinite(surr) and math.isfinite(kl) and kl <= 1.5 * hp["max_kl"] and surr - surr_before >= 0.0:
                    new_theta = cand
                    stats[1], stats[2], stats[3], stats[8] = surr, kl, ent, float(k)
                    break
    return dict(stats=np.asarray(stats), gflag=_any([g]), nets=_any([new_theta]), accepted=int(stats[8]), iters=int(stats[9]))


@pytest.mark.parametrize("case", nc.TRPO_STEP_CASES, ids=ids(nc.TRPO_STEP_CASES))
def test_trpo_step_reference_against_torch_float64_autograd(case):
    S = nc.trpo_step_setup(case)
    ref, arb = nc.trpo_step_reference(S), trpo_step_arbiter(S)
    rs, as_ = ref["stats"], arb["stats"]
    # (theta is never written by a poisoned step: it holds a non-finite element exactly when the case put one there)
    own = case["target"][0] == "w" and case["target"][1] in tr.POLICY_KEYS
    assert ref["gflag"] == arb["gflag"] and ref["nets"] == arb["nets"] == own, (case["id"], "gradient and theta flags")
    assert ref["accepted"] == arb["accepted"] and ref["iters"] == arb["iters"], (case["id"], rs, as_)
    assert np.array_equal(nc.nonfinite(rs[2:]), nc.nonfinite(as_[2:])), (case["id"], rs, as_)
    both = ~nc.nonfinite(rs) & ~nc.nonfinite(as_)
    assert np.allclose(rs[both], as_[both], rtol=1e-6, atol=1e-9), (case["id"], rs, as_)
    _twin_rows_are_off_every_relu_edge(tr.relu_edges(nc.trpo_step_setup(case, twin=True)["W"], S["data"]["obs"][:S["n"]][np.isfinite(S["data"]["obs"][:S["n"]]).all(1)]))
    if case["clean"]:
        tw = nc.trpo_step_reference(nc.trpo_step_setup(case, twin=True))
        assert np.isfinite(rs).all() and np.isfinite(as_).all() and not ref["gflag"], (case["id"], case["clean"], rs, as_)
        assert np.array_equal(tw["stats"], rs) and np.array_equal(tw["theta"], ref["theta"]) and ref["accepted"] >= 0, (case["id"], rs)
        return
    # a poisoned step: g is non-finite, CG runs every product, every candidate is rejected, theta stays
    assert ref["gflag"] and ref["accepted"] == -1 and ref["iters"] == S["hp"]["cg_iters"] and len(ref["cands"]) == S["hp"]["backtracks"], case["id"]
    assert nc.nonfinite(rs[4:8]).all() and rs[2] == 0.0 and as_[2] == 0.0, (case["id"], rs)
    assert np.array_equal(ref["theta"], tr.flatten(S["W"], np.float64), equal_nan=True)
    # statistics 0 and 1, the documented deviation: the header's sum A / n + entcoeff entropy is finite whenever the advantages and
    # logstd are, autograd's mean(A exp(nlp_old - neglogp)) is NaN with one row's neglogp
    A, logstd = ref["G"]["A"], S["W"]["logstd"]
    header_finite = bool(np.isfinite(A).all() and np.isfinite(logstd).all())
    assert rs[0] == rs[1] or (rs[0] != rs[0] and rs[1] != rs[1])
    assert bool(np.isfinite(rs[0])) == header_finite, (case["id"], rs[0])
    assert as_[0] != as_[0] and as_[1] != as_[1], (case["id"], "autograd's surrogate of a poisoned step is NaN", as_)
    if header_finite:
        tw = nc.trpo_step_reference(nc.trpo_step_setup(case, twin=True))
        if case["target"][0] == "w" or case["target"][1] in ("obs", "actions"):
            assert rs[0] == tw["stats"][0], "the advantages and logstd are the twin's: so is surr_before"


def test_the_trpo_step_table_has_both_lists_and_the_shapes_the_issue_names():
    cases = nc.TRPO_STEP_CASES
    assert len({c["id"] for c in cases}) == len(cases) and nc.TRPO_STEP_N == 17 and nc.TRPO_STEP_SLICES == (1, 3)
    assert nc.TRPO_STEP_HP["cg_iters"] == 3 and nc.TRPO_STEP_HP["backtracks"] == 3
    poisoned, clean = [c for c in cases if c["clean"] is None], [c for c in cases if c["clean"]]
    assert poisoned and clean and len(poisoned) + len(clean) == len(cases)
    assert {(c["row"], c["stride"]) for c in poisoned if c["target"] == ("row", "obs")} == {(3, 5), (16, 5), (16, 4)}
    assert {c["target"][1] for c in poisoned if c["target"][0] == "row"} == set(nc.TRPO_STEP_DATA)
    assert {c["target"][1] for c in poisoned if c["target"][0] == "w"} == {"w0", "w2", "logstd", "b1"}
    assert {c["target"][0] for c in clean} == {"w", "m", "v", "row"} and any(c["rows"] == 18 and c["row"] == 17 for c in clean)
    assert {c["stride"] for c in poisoned} == {4, 5} == {c["stride"] for c in clean}
