"""The acting paths at NaN and inf inputs, without a GPU: the tables of tests/acting_nonfinite_cases.py and the float64
references they are held to.

  anchors      at every actor case the reference (actor_numerics.net64, acting_nonfinite_cases.sample64) gives the same kind of
               value -- finite, NaN, +inf, -inf -- in every element as float64 torch (torch.relu, torch.clamp, torch.tanh;
               MlpPolicy.predict and ActorCriticPolicy.step on float64 CPU tensors), and the same finite values; at every
               planner case one model step of dynplan_ref against DynamicsNet.predict in float64
  sign-decided for every infinite weight, on every one of the 67 rows, the value whose sign decides between an infinity and a
               NaN is larger in magnitude than the error bound of either precision: the kind cannot hang on a rounding
  emulation    the split-bf16 numpy emulation of actor_numerics.py, run on the packed image of every case, is non-finite
               wherever the reference is, and the images carry both NaN patterns (pack_fast_weights, pack_fast_actor_critic)
  planners     which scores dynplan_ref, dynmppi_ref and mppi_ref make NaN, case by case
"""
import numpy as np
import pytest

import acting_nonfinite_cases as ac
import actor_numerics as an
import dynplan_ref as dr
import mppi_ref
import shooting_ref

LAYOUTS = tuple(ac.LAYOUTS)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _eps(n=ac.N):
    return np.random.default_rng(5).standard_normal((n, 4)) * 1.5


def _bits1(v):
    return int(ac.bits(v).reshape(-1)[0])


def _same_kind_and_value(got, ref, what, rtol=1e-9):
    """the same kind in every element, and two float64 evaluations of the same sums in different orders where both are finite
    (the 'cancel' set's outputs are differences of near-equal sums: 1e-11 relative between numpy's and torch's matmul)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    assert np.array_equal(ac.kind(got), ac.kind(ref)), what
    f = np.isfinite(ref)
    np.testing.assert_allclose(got[f], ref[f], rtol=rtol, atol=1e-12, err_msg=str(what))


# ---------------------------------------------------------------------------------------------------- the actor table
@pytest.mark.parametrize("layout", LAYOUTS)
def test_actor_table(layout):
    cases = ac.ACTOR_CASES[layout]
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids)
    sites = 12 + 2 + 3 + (1 if layout == "towers" else 0)
    assert len(cases) == 4 * sites + 4 * len(ac.OBS_ROWS)
    assert ac.bits(np.array([ac.poison_value("nan"), ac.poison_value("nan-signed")])).tolist() == [0x7FC00000, 0xFFC00000]
    W, obs = ac.weights(layout), ac.observations()
    assert ("wv0" in W) == (layout == "towers") and obs.shape == (ac.N, 12)
    assert np.all(np.abs(obs) <= 0.5 * an.BOX_WIDTH)
    clean_m, clean_v = ac.reference(W, obs)
    assert np.isfinite(clean_m).all() and np.isfinite(clean_v).all()
    for c in cases:
        Wp, x = ac.poisoned_weights(c, W), ac.poisoned_obs(c, obs)
        hit = (Wp[c["target"][1]][c["elem"]] if c["target"][0] == "w" else x[c["elem"]])
        assert _bits1(hit) == ac.POISONS[c["poison"]], c["id"]                  # the pattern survives the copy
        m, v = ac.reference(Wp, x)
        finite = bool(np.isfinite(m).all() and np.isfinite(v).all())
        assert finite == (c["clean"] is not None), c["id"]
        key = c["target"][1]
        rm, rv = ac.reached(c)                                               # what the wiring cannot reach is the clean result
        assert np.array_equal(m[~rm], clean_m[~rm]) and np.array_equal(v[~rv], clean_v[~rv]), c["id"]
        assert np.isfinite(m[~rm]).all() and np.isfinite(v[~rv]).all(), c["id"]
        if c["target"][0] == "obs":                                          # the poisoned row alone, all of it
            bad = np.zeros(ac.N, bool); bad[c["elem"][0]] = True
            assert np.array_equal(~np.isfinite(m).all(axis=1), bad) and np.array_equal(~np.isfinite(v), bad), c["id"]
            assert np.array_equal(m[~bad], clean_m[~bad]) and np.array_equal(v[~bad], clean_v[~bad]), c["id"]
        elif key in ("w2", "b2"):                                            # component 3 alone; the value branch untouched
            assert np.isfinite(m[:, :3]).all() and not np.isfinite(m[:, 3]).any(), c["id"]
            assert np.array_equal(m[:, :3], clean_m[:, :3]) and np.array_equal(v, clean_v), c["id"]
        elif key in ac.VALUE_KEYS:                                           # the policy branch untouched
            assert np.array_equal(m, clean_m), c["id"]
        elif layout == "towers":                                             # a policy tower's poison leaves the value alone
            assert np.array_equal(v, clean_v), c["id"]
        if c["poison"].startswith("nan") and c["target"][0] == "w" and key not in ("w2", "b2") + ac.VALUE_KEYS:
            assert np.isnan(m).all(), c["id"]                                # a NaN weight that reaches the mean: every row


# ---------------------------------------------------------------------------------------------------- torch float64 anchors
def _torch_heads(torch, W, x):
    t = lambda k: torch.as_tensor(np.asarray(W[k], np.float64))              # noqa: E731
    x = torch.as_tensor(np.asarray(x, np.float64))
    h = torch.relu(x @ t("w0") + t("b0"))
    mean = torch.relu(h @ t("w1") + t("b1")) @ t("w2") + t("b2")
    hv = torch.relu(x @ t("wv0") + t("bv0")) if "wv0" in W else h
    return mean, (torch.relu(hv @ t("wv1") + t("bv1")) @ t("wv2") + t("bv2"))[:, 0]


def _double(policy, keys):
    for k in keys:
        setattr(policy, k, getattr(policy, k).double())
    return policy


@pytest.mark.parametrize("layout", LAYOUTS)
def test_reference_matches_torch_float64_at_every_case(torch, layout):
    import quadsim_amd as qa
    W, obs, eps = ac.weights(layout), ac.observations(), _eps()
    keys = [k for k in ac.ACTOR_KEYS + ac.VALUE_KEYS if k in W]
    for c in ac.ACTOR_CASES[layout]:
        Wp, x = ac.poisoned_weights(c, W), ac.poisoned_obs(c, obs)
        m, v = ac.reference(Wp, x)
        tm, tv = _torch_heads(torch, Wp, x)
        _same_kind_and_value(tm.numpy(), m, c["id"])
        _same_kind_and_value(tv.numpy(), v, c["id"])
        x64 = torch.as_tensor(x.astype(np.float64))
        mlp = _double(qa.MlpPolicy(Wp, device="cpu"), ac.ACTOR_KEYS)
        with np.errstate(invalid="ignore"):
            _same_kind_and_value(mlp.predict(x64).numpy(), np.clip(m, -1.0, 1.0), c["id"])
        for squash in (False, True):
            u, nl, a = ac.sample64(Wp, m, eps, squash)
            pol = _double(qa.ActorCriticPolicy(Wp, device="cpu", squash=squash), keys + ["logstd"])
            tu, tval, _, tnl = pol.step(x64, noise=torch.as_tensor(eps))
            _same_kind_and_value(tu.numpy(), u, (c["id"], squash))
            _same_kind_and_value(tval.numpy(), v, (c["id"], squash))
            _same_kind_and_value(tnl.numpy(), nl, (c["id"], squash), rtol=1e-7)      # sech^2 against 1 - tanh^2 next to 1e-6
            _same_kind_and_value(pol.env_action(tu).numpy(), a, (c["id"], squash))
            ta = torch.tanh(torch.as_tensor(u)) if squash else torch.clamp(torch.as_tensor(u), -1.0, 1.0)
            _same_kind_and_value(ta.numpy(), a, (c["id"], squash))
            assert np.array_equal(np.isnan(a), np.isnan(u)) and np.isfinite(a[~np.isnan(u)]).all(), c["id"]   # clip(NaN) = NaN, clip(inf) = 1
            assert np.isnan(nl[np.isnan(u).any(axis=1)]).all(), c["id"]


# ---------------------------------------------------------------------------------------------------- the sign decides
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kind_of_an_infinite_weights_result_is_decided_on_every_row(layout):
    W, obs = ac.weights(layout), ac.observations()
    deciding = 0
    for c in ac.weight_cases(layout):
        if c["poison"] not in ("pinf", "ninf"):
            continue
        ok = ac.decided(c, W, obs)
        assert ok.shape == (ac.N,) and ok.all(), (c["id"], np.flatnonzero(~ok))
        d = ac.decider(c, W, obs)
        if d is not None:
            deciding += 1
            assert (d[0] > 0).any() and (d[0] < 0).any(), c["id"]            # both kinds occur among the 67 rows
        # where the reference stays finite behind an infinite weight, the receiving unit is dead: the dead twin's outputs
        Wp = ac.poisoned_weights(c, W)
        m, v = ac.reference(Wp, obs)
        dm, dv = ac.reference(ac.dead_twin(c, W), obs)
        fm, fv = np.isfinite(m), np.isfinite(v)
        np.testing.assert_allclose(m[fm], dm[fm], rtol=1e-13, err_msg=c["id"])
        np.testing.assert_allclose(v[fv], dv[fv], rtol=1e-13, err_msg=c["id"])
        Em, Ev = ac.scales(c, W, Wp, obs)
        assert np.isfinite(Em[fm]).all() and np.isfinite(Ev[fv]).all(), c["id"]
    assert deciding >= 2 * (3 + 1 + 1 + 1 + 3)                               # w0, w1 x 3 units, w2, wv1, wv2 (, wv0), both signs


# ---------------------------------------------------------------------------------------------------- the packed images
def _image_values(c, actor, heads):
    """the elements of the two decoded images that hold the case's weight: [(value as the image stores it, stored as bf16?)]"""
    key, idx = c["target"][1], c["elem"]
    out = []
    if key in ac.ACTOR_KEYS:
        l = int(key[1])
        out.append((actor["hi"][l][idx[::-1]], True) if key[0] == "w" else (actor["b"][l][idx], False))
    where = {"w0": ("w1", False), "b0": ("b1", False), "wv0": ("wv1", False), "bv0": ("bv1", False)}
    if key in where:
        name, _ = where[key]
        out.append((heads[name][idx[::-1]] if key[0] == "w" else heads[name][idx], False))
    elif key in ("w1", "w2", "wv1", "wv2"):
        br = heads["pi" if key[1] != "v" else "vf"]
        out.append((br["hi"][int(key[-1]) - 1][idx[::-1]], True))
    elif key in ("b1", "b2", "bv1"):
        br = heads["pi" if key[1] != "v" else "vf"]
        out.append((br["b"][int(key[-1]) - 1][idx], False))
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_split_bf16_emulation_is_non_finite_wherever_the_reference_is(layout):
    import quadsim_amd as qa
    from quadsim_amd.policy import pack_fast_weights
    from quadsim_amd.runner import pack_fast_actor_critic
    W, obs = ac.weights(layout), ac.observations()
    towers = layout == "towers"
    for c in ac.ACTOR_CASES[layout]:
        Wp, x = ac.poisoned_weights(c, W), ac.poisoned_obs(c, obs)
        m, v = ac.reference(Wp, x)
        blob_a = pack_fast_weights(qa.MlpPolicy(Wp, device="cpu")).copy()
        blob_h = pack_fast_actor_critic(qa.ActorCriticPolicy(Wp, device="cpu")).copy()
        with np.errstate(all="ignore"):
            ea = an.emulate_actor_blob(blob_a, x)
            em, ev = an.emulate_actor_critic_blob(blob_h, x, towers=towers)
        assert not np.isfinite(ea[~np.isfinite(m)]).any(), c["id"]
        assert not np.isfinite(em[~np.isfinite(m)]).any() and not np.isfinite(ev[~np.isfinite(v)]).any(), c["id"]
        if c["target"][0] == "w":
            stored = _image_values(c, an.decode_actor_blob(blob_a), an.decode_actor_critic_blob(blob_h, towers))
            assert len(stored) == (2 if c["target"][1] in ac.ACTOR_KEYS else 1), c["id"]
            for value, as_bf16 in stored:
                want = ac.POISONS[c["poison"]]
                assert _bits1(value) == ((want >> 16) << 16 if as_bf16 else want), (c["id"], hex(_bits1(value)))
        # value-only poisons leave the emulated means' bits alone, policy-only poisons (towers, or behind the trunk) the value's
        cm, cv = an.emulate_actor_critic_blob(pack_fast_actor_critic(qa.ActorCriticPolicy(W, device="cpu")).copy(), obs, towers=towers)
        if c["target"][1] in ac.VALUE_KEYS:
            assert np.array_equal(em, cm), c["id"]
        elif c["target"][0] == "w" and (towers or c["target"][1] not in ("w0", "b0")):
            assert np.array_equal(ev, cv), c["id"]


# ---------------------------------------------------------------------------------------------------- planners
def _plan_acts():
    return np.stack([shooting_ref.actions_fast(dr.EDGE_SEED, dr.EDGE_GID0 + i, dr.EDGE_K, ac.PLAN_PATHS, ac.PLAN_HORIZON)
                     for i in range(ac.PLAN_N)])


def test_dynamics_net_cases_say_which_scores_are_nan(torch):
    W, obs, acts = ac.dyn_weights(), ac.plan_obs(), _plan_acts()
    assert (W["w1"].shape[0], W["w2"].shape[0]) == (64, 64) and dr.EDGE_WIDTHS[(64, 64)] == (64, 64)
    nominal, noise = ac.mppi_inputs()
    assert len(ac.DYN_CASES) == 4 * 8 and len({c["id"] for c in ac.DYN_CASES}) == 32
    clean = ac.shooting_reference(W, obs, acts)
    assert np.isfinite(clean).all()
    for c in ac.DYN_CASES:
        Wp = ac.dyn_poisoned(c, W)
        S = ac.shooting_reference(Wp, obs, acts)
        M = ac.learned_mppi_reference(Wp, obs, nominal, noise)
        assert S.shape == (ac.PLAN_N, ac.PLAN_PATHS) and M["scores"].shape == (ac.PLAN_N, ac.PLAN_ITERATIONS, ac.PLAN_PATHS)
        assert not np.isinf(S).any() and not np.isinf(M["scores"]).any(), c["id"]     # a non-finite score is a NaN score
        if c["poison"].startswith("nan"):
            assert np.isnan(S).all() and np.isnan(M["scores"]).all(), c["id"]         # every env, every candidate
        assert (c["clean"] is not None) == bool(np.isfinite(S).all() and np.isfinite(M["scores"]).all()), c["id"]
        assert ac.dyn_decided(c, W, obs, acts), c["id"]
        all_nan = np.isnan(M["scores"]).all(axis=(1, 2))
        U0 = nominal                                                                   # shift 0: what MPPI keeps
        assert np.array_equal(M["nominal"][all_nan], U0[all_nan]) and (M["best_score"][all_nan] == -np.inf).all(), c["id"]
        # where a score stays finite behind an infinite weight, the receiving unit is dead on that candidate
        D = ac.shooting_reference(ac.dyn_dead_twin(c, W), obs, acts)
        np.testing.assert_allclose(S[np.isfinite(S)], D[np.isfinite(S)], rtol=1e-12, err_msg=c["id"])
        # one model step against DynamicsNet.predict in float64
        net = dr.to_net(Wp, "cpu")
        got = net.predict(torch.as_tensor(obs.astype(np.float64)), torch.as_tensor(acts[:, 0, 0].astype(np.float64))).numpy()
        with np.errstate(all="ignore"):
            _same_kind_and_value(got, dr.step64(Wp, obs, acts[:, 0, 0]), c["id"])
    kinds = {c["id"]: int(np.isnan(ac.shooting_reference(ac.dyn_poisoned(c, W), obs, acts)).sum()) for c in ac.DYN_CASES}
    assert 0 < kinds["dyn-w1[5, 12]-pinf"] < 99 and 0 < kinds["dyn-w2[7, 5]-ninf"] < 99      # live and dead candidates both occur


def test_nominal_and_noise_cases_say_which_candidates_are_nan():
    assert len(ac.MPPI_CASES) == 8 and ac.NOMINAL_ELEM == (1, 0, 2) and ac.NOISE_ELEM == (0, 5, 0) and ac.PLAN_ITERATIONS == 2
    W, obs = ac.dyn_weights(), ac.plan_obs()
    n0, z0 = ac.mppi_inputs()
    assert np.abs(n0).max() < 1.0
    base = ac.learned_mppi_reference(W, obs, n0, z0)
    for c in ac.MPPI_CASES:
        nominal, noise = ac.mppi_poisoned(c)
        tn, tz = ac.mppi_poisoned(c, twin=True)
        nan0 = ac.mppi_nan_candidates(nominal, noise, 0)
        got = ac.learned_mppi_reference(W, obs, nominal, noise)
        twin = ac.learned_mppi_reference(W, obs, tn, tz)
        assert np.array_equal(np.isnan(got["scores"][:, 0]), nan0), c["id"]            # horizon step 0: no candidate ends before it
        if c["clean"] is not None:                                                     # an infinity: the clamp's +-1, as +-1e30
            assert not nan0.any() and np.isfinite(got["scores"]).all(), c["id"]
            with np.errstate(invalid="ignore"):
                assert np.array_equal(mppi_ref.candidates32(nominal, ac.PLAN_SIGMA, noise[0]), mppi_ref.candidates32(tn, ac.PLAN_SIGMA, tz[0]))
            assert np.array_equal(got["scores"], twin["scores"]) and np.array_equal(got["nominal"], twin["nominal"]), c["id"]
            continue
        assert np.array_equal(twin["scores"], base["scores"]), c["id"]
        if c["target"][0] == "nominal":                                                # env 1: every candidate, both iterations
            want = np.zeros((ac.PLAN_N, ac.PLAN_PATHS), bool); want[1] = True
            assert np.array_equal(nan0, want) and np.isnan(got["scores"][1]).all(), c["id"]
            assert got["best_score"][1] == -np.inf and ac.bits(got["nominal"][1]).tolist() == ac.bits(nominal[1]).tolist(), c["id"]
            others = [0, 2]
            assert np.array_equal(got["scores"][others], base["scores"][others]), c["id"]
            assert np.array_equal(got["nominal"][others], base["nominal"][others]), c["id"]
        else:                                                                          # candidate 5 of every env, iteration 0
            want = np.zeros((ac.PLAN_N, ac.PLAN_PATHS), bool); want[:, 5] = True
            assert np.array_equal(nan0, want), c["id"]
            keep = np.arange(ac.PLAN_PATHS) != 5
            assert np.array_equal(got["scores"][:, 0, keep], base["scores"][:, 0, keep]), c["id"]
            # weight 0: the update is the update without candidate 5 -- but for the step the NaN sits in, where update64
            # adds 0 * NaN = NaN.  From there on every candidate of every env is NaN at step 0, and U stays
            want_U = mppi_ref.update64(base["scores"][:, 0][:, keep], mppi_ref.candidates32(n0, ac.PLAN_SIGMA, z0[0])[:, keep],
                                       ac.PLAN_LAM, n0).astype(np.float32)
            hit = np.zeros(want_U.shape, bool); hit[:, ac.NOISE_ELEM[2]] = True        # all four components of noise[0][5][0]
            assert np.isnan(got["trace"][:, 1][hit]).all() and np.array_equal(got["trace"][:, 1][~hit], want_U[~hit]), c["id"]
            assert np.isnan(got["scores"][:, 1]).all() and (got["best_score"] == -np.inf).all(), c["id"]
            assert np.array_equal(ac.bits(got["nominal"]), ac.bits(got["trace"][:, 1])), c["id"]
