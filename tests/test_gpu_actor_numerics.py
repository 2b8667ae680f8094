"""-m gpu: every device actor / critic path against the float64 network of tests/actor_numerics.py, elementwise, with the
scale-aware bound |err| <= kappa * unit * E (E: the first-order forward-error magnitude of each output) -- exact-f32 and
split-bf16 ("bf16x3") -- on weight sets whose action means are mostly unclipped (the trained v0 net and the tower checkpoint
rescaled, dead ReLUs, cancellation), on box / edge / env-distributed observations and ragged row counts.  Plus, bit for bit:
a row's action does not depend on its position in the MFMA wave, on non-finite observations in other rows of the wave, or on
what lies past row n of the input buffer; the K-episode evaluation with a random net equals the per-step loop.

Set ACTOR_NUMERICS_REPORT to a file name to have the worst measured ratio per path, precision and weight set (and the unclipped
fraction each relied on) written there as JSON."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import actor_numerics as an
from actor_numerics import _neglogp64, _neglogp_bound

pytestmark = pytest.mark.gpu

PRECS = ("f32", "bf16x3")
NS = (1, 63, 64, 65, 1000, 4097)
REPORT = {}


def _note(key, worst, free=None):
    r = REPORT.setdefault(key, {"worst_ratio": 0.0})
    r["worst_ratio"] = max(r["worst_ratio"], float(worst))
    if free is not None:
        r["unclipped_min"] = min(r.get("unclipped_min", 1.0), float(free))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ACTOR_NUMERICS_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def sets():
    return {k: an.weight_set(k) for k in an.WEIGHT_SETS}


@pytest.fixture(scope="module")
def obs_sets(qa):
    """box, edge (v0 and v1 ranges) and env-distributed observations: randomise = 1 resets over C3_INIT_RANGE"""
    env = qa.VecDockingEnv("docking-v0", num_envs=4097, randomise=1, seed=3, init_range=qa.C3_INIT_RANGE)
    o = env.reset().cpu().numpy().copy()
    env.close()
    return {"box": an.box_obs(4097, 1), "edge_v0": an.edge_obs(4097, 2, an.RMAX["docking-v0"]),
            "edge_v1": an.edge_obs(4097, 3, an.RMAX["docking-v1"]), "env": o}


def _mlp(qa, W):
    return qa.MlpPolicy({k: W[k] for k in ("w0", "b0", "w1", "b1", "w2", "b2")})


def _check_actions(key, act, W, obs, precision, min_free):
    m64 = an.net64(W, obs)[0]
    Em = an.err_scale(W, obs)[0]
    worst, free = an.check_clipped(act, m64, Em, precision, key)
    assert free >= min_free, (key, free)                   # the comparison is not a check of +-1
    _note(key, worst, free if min_free > 0 else None)


# ---------------------------------------------------------------------------------------------------- actor-only paths
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", an.WEIGHT_SETS)
def test_predict_hip_within_bound(qa, torch, sets, obs_sets, name, precision):
    """qs_policy_forward(_fast) on every observation set at every ragged row count"""
    W = sets[name]
    pol = _mlp(qa, W)
    env = qa.VecDockingEnv("docking-v0", num_envs=64)
    for oname, obs in obs_sets.items():
        for n in NS:
            x = obs[:n]
            a = pol.predict_hip(env, torch.as_tensor(x, device="cuda"), precision).cpu().numpy()
            _check_actions("predict_hip/%s/%s" % (precision, name), a, W, x, precision,
                           0.9 if oname == "box" and n >= 1000 else 0.0)
        a = pol.predict_hip(env, torch.as_tensor(obs, device="cuda"), precision).cpu().numpy()
        _check_actions("predict_hip/%s/%s" % (precision, name), a, W, obs, precision, 0.5)
    env.close()


def _mid_episode_env(qa, env_id, rnd, n):
    from test_gpu_policy_evaluate import _make
    return _make(qa, env_id, rnd, n)


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", an.WEIGHT_SETS)
def test_fused_policy_rollout_and_step_policy_within_bound(qa, torch, sets, name, precision):
    """qs_policy_rollout(_fast) with T = 1 and step_policy act on the observation of the envs' current state: the one the last
    step returned (env-distributed, mid-episode, ragged N)"""
    W = sets[name]
    pol = _mlp(qa, W)
    for env_id, rnd, n in (("docking-v0", 1, 4097), ("docking-v2", 1, 1000), ("docking-v0", 0, 65)):
        env, obs = _mid_episode_env(qa, env_id, rnd, n)
        o = obs.cpu().numpy().copy()
        A = qa.fused_policy_rollout(env, pol, 1, precision=precision)[4][0].cpu().numpy()
        _check_actions("fused_policy_rollout/%s/%s" % (precision, name), A, W, o, precision, 0.5)
        env.close()
        env, obs = _mid_episode_env(qa, env_id, rnd, n)
        assert np.array_equal(obs.cpu().numpy(), o)
        a = env.step_policy(pol, precision=precision)[3].cpu().numpy()
        _check_actions("step_policy/%s/%s" % (precision, name), a, W, o, precision, 0.5)
        assert np.array_equal(a, A)                        # the same mlp_actor on the same values
        env.close()


# ---------------------------------------------------------------------------------------------------- fused Runner
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("name", an.WEIGHT_SETS)
def test_fused_runner_within_bound(qa, torch, sets, name, precision):
    """qs_runner_rollout(_net)(_fast), T = 1, for both runner kernels (role-split and one wave per tile), plain and squashed:
    the un-clipped means (zero noise) and values on the observations the kernel reports, last_values on last_obs; with noise,
    the samples and neglogp against the float64 formula"""
    W = sets[name]
    lib = qa._lib.load()
    lib.qs_debug_set_runner_serial.argtypes = [C.c_int]
    n = 4097
    try:
        for serial in (0, 1):
            lib.qs_debug_set_runner_serial(serial)
            for squash in (False, True):
                ac = qa.ActorCriticPolicy(W, squash=squash)
                tag = "%s/%s/%s%s" % (precision, name, ("split", "serial")[serial], "/squash" if squash else "")
                for noisy in (False, True):
                    env = qa.VecDockingEnv("docking-v0", num_envs=n, randomise=1, seed=7, init_range=qa.C3_INIT_RANGE)
                    env.reset()
                    t0 = np.zeros(n, np.float32); t0[::9] = 599.0                 # some envs reset inside the step
                    env.set_state(t=t0)
                    eps = (torch.randn((1, n, 4), generator=torch.Generator().manual_seed(3)) * 2.0 if noisy
                           else torch.zeros((1, n, 4)))
                    ro = qa.fused_runner_rollout(env, ac, 1, noise=eps, precision=precision)
                    R = {k: v.cpu().numpy() for k, v in ro.items() if v is not None}
                    env.close()
                    obs = R["obs"][0]
                    m64, v64 = an.net64(W, obs)
                    Em, Ev = an.err_scale(W, obs)
                    mb = an.bound(Em, precision)
                    if not noisy:
                        _note("runner_mean/" + tag, an.check_unclipped(R["actions"][0], m64, Em, precision, "runner mean " + tag))
                        assert np.mean(np.abs(m64) < 0.95) >= 0.5
                        _note("runner_value/" + tag, an.check_unclipped(R["values"][0], v64, Ev, precision, "runner value " + tag))
                        lo = R["last_obs"]
                        _, lv64 = an.net64(W, lo)
                        _note("runner_last_value/" + tag, an.check_unclipped(R["last_values"], lv64, an.err_scale(W, lo)[1],
                                                                           precision, "runner last value " + tag))
                        continue
                    e = eps[0].numpy().astype(np.float64)
                    std = np.exp(np.asarray(W["logstd"], np.float32).astype(np.float64)).reshape(1, 4)
                    u64 = m64 + std * e
                    ub = mb + an.KAPPA["f32"] * an.UNIT["f32"] * (np.abs(u64) + std * np.abs(e))
                    du = np.abs(R["actions"][0] - u64)
                    assert (du <= ub).all(), ("runner sample " + tag, float((du / ub).max()))
                    nl64 = _neglogp64(W, u64, e, squash)
                    nb = _neglogp_bound(W, u64, m64, e, mb, squash)
                    dn = np.abs(R["neglogp"][0] - nl64)
                    assert (dn <= nb).all(), ("runner neglogp " + tag, float((dn / nb).max()))
                    _note("runner_neglogp_over_bound/" + tag, float((dn / nb).max()))
    finally:
        lib.qs_debug_set_runner_serial(0)


# ---------------------------------------------------------------------------------------------------- bit-for-bit properties
def _row_out(pol, env, torch, x, precision):
    return pol.predict_hip(env, torch.as_tensor(x, device="cuda"), precision).cpu().numpy()


@pytest.mark.parametrize("precision", PRECS)
def test_action_independent_of_position_in_wave(qa, torch, sets, obs_sets, precision):
    """a row's action is the same at lane 0, lane 37, in the one-row tail wave of n = 65 and in the tail of n = 4097, whatever
    the other rows hold"""
    W = sets["dead"]
    pol = _mlp(qa, W)
    env = qa.VecDockingEnv("docking-v0", num_envs=64)
    probes = np.concatenate([obs_sets["box"][:3], obs_sets["edge_v1"][:3], obs_sets["env"][:2]])
    filler = obs_sets["edge_v0"]
    for p in probes:
        outs = []
        for n, pos in ((1, 0), (64, 0), (64, 37), (65, 64), (4097, 4096), (4097, 64 * 20 + 37), (1000, 999)):
            x = filler[:n].copy()
            x[pos] = p
            outs.append(_row_out(pol, env, torch, x, precision)[pos])
        for o in outs[1:]:
            assert np.array_equal(o, outs[0]), (precision, outs)
    env.close()


@pytest.mark.parametrize("precision", PRECS)
def test_non_finite_rows_do_not_leak_into_other_rows(qa, torch, sets, obs_sets, precision):
    """NaN, +-Inf or 1e30 in other rows of the same wave (whole rows or one element) leave a row's action bit for bit"""
    for name in ("v0", "dead"):
        W = sets[name]
        pol = _mlp(qa, W)
        env = qa.VecDockingEnv("docking-v0", num_envs=64)
        x = obs_sets["box"][:130].copy()
        clean = _row_out(pol, env, torch, x, precision)
        keep = np.array([5, 70, 129])
        rng = np.random.default_rng(4)
        for poison in (np.nan, np.inf, -np.inf, 1e30):
            for whole in (True, False):
                y = x.copy()
                rows = np.setdiff1d(np.arange(130), keep)
                if whole:
                    y[rows] = poison
                else:
                    y[rows, rng.integers(0, 12, rows.size)] = poison
                out = _row_out(pol, env, torch, y, precision)
                assert np.array_equal(out[keep], clean[keep]), (name, precision, poison, whole)
        env.close()


@pytest.mark.parametrize("precision", PRECS)
def test_prefix_view_reads_and_writes_only_n_rows(qa, torch, sets, obs_sets, precision):
    """predict_hip on the first n rows of a larger buffer whose rows past n hold NaN: the same actions as on a buffer of its
    own, and an `out` sentinel past row n untouched"""
    W = sets["v0"]
    pol = _mlp(qa, W)
    env = qa.VecDockingEnv("docking-v0", num_envs=64)
    for n in (1, 63, 64, 65, 1000):
        x = obs_sets["env"][:n]
        ref = _row_out(pol, env, torch, x, precision)
        buf = torch.full((n + 67, 12), float("nan"), device="cuda")
        buf[:n] = torch.as_tensor(x, device="cuda")
        out = torch.full((n + 67, 4), -7.25, device="cuda")
        a = pol.predict_hip(env, buf[:n], precision, out=out[:n])
        torch.cuda.synchronize()
        assert a.data_ptr() == out.data_ptr()
        o = out.cpu().numpy()
        assert np.array_equal(o[:n], ref), (n, precision)
        assert (o[n:] == -7.25).all(), (n, precision)
    env.close()


# ---------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("precision", PRECS)
def test_evaluate_with_random_net_equals_per_step_loop(qa, torch, sets, precision):
    """qs_policy_evaluate(_fast) with the dead-ReLU random net (c) against predict_hip + env.step, bit for bit"""
    from test_gpu_policy_evaluate import _assert_equal_episodes, _episodes, _loop, _make
    pol = _mlp(qa, sets["dead"])
    K = 2
    env, obs = _make(qa, "docking-v0", 1, 1000)
    res = qa.evaluate_policy_episodes(pol, env, K, precision=precision)
    ref = _episodes(*_loop(torch, env, pol, obs, precision, K * 600), K)
    _assert_equal_episodes(res, ref)
    assert (ref[4] == K).all()
    env.close()
