"""-m gpu: the tower actor-critic of the reference's ppo2_docking*.zip archives (net_arch [dict(pi=[128, 128],
vf=[128, 128])], loaded by quadsim_amd.load_sb2_model) on the device: the actor kernels, the reference episode of fixture
g13, the fused Runner kernels (both flavours, both precisions) against a float64 restatement, and Runner.run()."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from helpers import OBS_TOL, reward_atol, set_env_from_rec, state_to_rec, tile_par
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu

TOWERS_ZIP = os.path.join(GOLDEN, "sb2_ppo2_docking_621_h_30M.zip")


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


def _weights(qa):
    return qa.read_sb2_weights(TOWERS_ZIP)[1]


def value_scale(W, obs):
    """|bv2| + sum |hv_i wv2_i|: the magnitude of the terms the value sums.  This checkpoint's values reach 1e3 on random
    starts with heavy cancellation, so a float32 evaluation is held to a bound relative to this, not to |value|."""
    f = lambda k: np.asarray(W[k], np.float64)                    # noqa: E731
    hv = np.maximum(np.maximum(np.asarray(obs, np.float64) @ f("wv0") + f("bv0"), 0.0) @ f("wv1") + f("bv1"), 0.0)
    return np.abs(f("bv2"))[0] + hv @ np.abs(f("wv2"))[:, 0]


def tower_step64(W, obs, noise, squash=False):
    """float64 model.step of the tower MlpPolicy (rl_baselines/common/policies.py:35-92 with an empty shared part, :583-588;
    distributions.py:406-415,:426-430) -> (u, value, neglogp, mean).  value / neglogp: parity-unpinned by TensorFlow."""
    f = lambda k: np.asarray(W[k], np.float64)                    # noqa: E731
    x = np.asarray(obs, np.float64)
    hp = np.maximum(np.maximum(x @ f("w0") + f("b0"), 0.0) @ f("w1") + f("b1"), 0.0)
    hv = np.maximum(np.maximum(x @ f("wv0") + f("bv0"), 0.0) @ f("wv1") + f("bv1"), 0.0)
    mean = hp @ f("w2") + f("b2")
    value = (hv @ f("wv2") + f("bv2"))[:, 0]
    logstd = f("logstd").reshape(1, -1)
    u = mean + np.exp(logstd) * np.asarray(noise, np.float64)
    nl = 0.5 * np.sum(np.square((u - mean) / np.exp(logstd)), 1) + 0.5 * np.log(2 * np.pi) * 4 + np.sum(logstd)
    if squash:
        nl = nl + np.sum(np.log(1.0 - np.tanh(u) ** 2 + 1e-6), 1)
    return u, value, nl, mean


# ---------------------------------------------------------------- actor paths: no kernel change, the weights mapped
def test_tower_actor_paths_match_float64(qa):
    import torch
    W = _weights(qa)
    pol = qa.MlpPolicy.from_sb2_zip(TOWERS_ZIP)
    env = qa.VecDockingEnv("docking-v0", num_envs=64)
    g = torch.Generator(device="cuda").manual_seed(3)
    for n in (1, 63, 65, 1000, 4097):
        obs = (torch.rand((n, 12), device="cuda", generator=g) - 0.5) * torch.tensor([6, 6, 6, 2, 2, 2, 3, 3, 3, 2, 2, 2], device="cuda")
        ref = np.clip(tower_step64(W, obs.cpu().numpy(), np.zeros((n, 4)))[3], -1, 1)
        assert np.abs(pol.predict(obs).cpu().numpy() - ref).max() < 5e-6
        assert np.abs(pol.predict_hip(env, obs).cpu().numpy() - ref).max() < 5e-6
        err = np.abs(pol.predict_hip(env, obs, precision="bf16x3").cpu().numpy() - ref).max()
        assert err < 2e-4, err
    env.close()
    kw = dict(num_envs=1000, randomise=1, seed=5, init_range=qa.C3_INIT_RANGE)
    for prec, tol in (("f32", 5e-6), ("bf16x3", 2e-4)):
        e1 = qa.VecDockingEnv("docking-v0", **kw); e2 = qa.VecDockingEnv("docking-v0", **kw)
        o1 = e1.reset().cpu().numpy(); e2.reset()
        O, R, D, F, A = qa.fused_policy_rollout(e1, pol, 1, precision=prec)          # qs_policy_rollout(_fast)
        ref = np.clip(tower_step64(W, o1, np.zeros((1000, 4)))[3], -1, 1)
        assert np.abs(A[0].cpu().numpy() - ref).max() < tol
        _, _, _, a2 = e2.step_policy(pol, precision=prec)
        assert np.abs(a2.cpu().numpy() - ref).max() < tol
        e1.close(); e2.close()


# ---------------------------------------------------------------- fixture g13: the reference env driven by the tower actor
def test_g13_tower_episode_replayed_per_step(qa):
    """every step of the reference episode from its recorded state: the device actor's actions, the fused env step's outputs,
    the fused Runner's values (T = 1, zero noise) against the fixture's float64 vf tower; the overlimit end at step 323"""
    import torch
    g = load_golden("g13_towers_episode")
    n = len(g["actions"])
    assert n == 323
    pol = qa.MlpPolicy.from_sb2_zip(TOWERS_ZIP)
    ac = qa.load_sb2_model(TOWERS_ZIP)
    W = _weights(qa)
    env = qa.VecDockingEnv("docking-v0", num_envs=n, auto_reset=False)
    set_env_from_rec(env, g["rec_before"])
    obs_in = torch.as_tensor(g["obs_in"].astype(np.float32), device="cuda")
    for prec, tol in (("f32", 1e-5), ("bf16x3", 2e-4)):
        np.testing.assert_allclose(pol.predict_hip(env, obs_in, precision=prec).cpu().numpy(), g["actions"], atol=tol)
    env.close()
    from test_gpu_parity import _golden_single_steps
    _golden_single_steps(qa, g, "docking-v0", 0)                        # env outputs within OBS_TOL / STATE_TOL / reward_atol
    env = qa.VecDockingEnv("docking-v0", num_envs=n, auto_reset=False)
    set_env_from_rec(env, g["rec_before"])
    _, _, done, infos = env.step(g["actions"])
    done, flags = done.cpu().numpy(), infos.flags
    assert np.array_equal(done, g["done"].astype(bool)) and np.array_equal(flags & 7, g["flags"])
    assert done[-1] and not done[:-1].any() and flags[-1] & 2          # the overlimit end at step 323
    env.close()
    for prec, tol in (("f32", 1e-4), ("bf16x3", 2e-4)):                # obs from the float32-rounded recorded states
        env = qa.VecDockingEnv("docking-v0", num_envs=n)
        set_env_from_rec(env, g["rec_before"])
        ro = qa.fused_runner_rollout(env, ac, 1, noise=torch.zeros((1, n, 4)), precision=prec, want_flags=True)
        R = {k: v.cpu().numpy() for k, v in ro.items() if v is not None}
        np.testing.assert_allclose(R["obs"][0], g["obs_in"], **OBS_TOL)
        np.testing.assert_allclose(np.clip(R["actions"][0], -1, 1), g["actions"], atol=tol)
        assert np.all(np.abs(R["values"][0] - g["values"]) <= tol * (1.0 + value_scale(W, g["obs_in"])))
        assert np.array_equal(R["last_dones"].astype(bool), g["done"].astype(bool)) and np.array_equal(R["flags"][0] & 7, g["flags"])
        env.close()


# ---------------------------------------------------------------- fused Runner, tower layout
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("squash", [False, True])
def test_tower_runner_one_step_vs_float64(qa, precision, squash):
    """qs_runner_rollout_net(_fast), T = 1, ragged N: samples, values, neglogp against the float64 restatement on the observations
    the kernel reports; the env side against the oracle's env.step fed with the kernel's own env actions"""
    import torch
    W = _weights(qa)
    pol = qa.load_sb2_model(TOWERS_ZIP, squash=squash)
    n, seed = 1000, 7
    env = qa.VecDockingEnv("docking-v0", num_envs=n, randomise=1, seed=seed, init_range=qa.C3_INIT_RANGE)
    obs0 = env.reset().cpu().numpy()
    t_boost = np.zeros(n, np.float32); t_boost[::5] = 599.0
    env.set_state(t=t_boost)
    rec = state_to_rec(env.get_state()); par = tile_par(n)
    noise = torch.randn((1, n, 4), generator=torch.Generator().manual_seed(3)) * 3.0
    k0 = env.step_counter
    ro = qa.fused_runner_rollout(env, pol, 1, noise=noise, want_flags=True, precision=precision)
    R = {k: (v.cpu().numpy() if v is not None else None) for k, v in ro.items()}
    np.testing.assert_allclose(R["obs"][0], obs0, rtol=1e-6, atol=1e-6)
    u, value, nl, _ = tower_step64(W, R["obs"][0], noise[0].numpy(), squash)
    tol = 1e-5 if precision == "f32" else 1e-4
    np.testing.assert_allclose(R["actions"][0], u, rtol=tol, atol=tol)
    assert np.all(np.abs(R["values"][0] - value) <= tol * (1.0 + value_scale(W, R["obs"][0])))
    np.testing.assert_allclose(R["neglogp"][0], nl, rtol=2e-5 if precision == "f32" else 1e-4, atol=2e-4 if precision == "f32" else 2e-3)
    a_gpu = np.tanh(R["actions"][0].astype(np.float64)) if squash else np.clip(R["actions"][0], -1.0, 1.0)
    o, r, d, f, term = Oracle("f64").vec_step(rec, par, a_gpu.astype(np.float32), kind=0, randomise=1, seed=seed, step_idx=k0,
                                              rr=tuple(qa.C3_INIT_RANGE) + (1, 1, 1, 1), want_term=True)
    assert d[::5].all() and np.array_equal(R["last_dones"], d)
    np.testing.assert_allclose(R["last_obs"], o, **OBS_TOL)
    assert np.all(np.abs(R["rewards"][0] - r) <= reward_atol(rec[:, 38]) + reward_atol(r))
    assert np.array_equal(R["flags"][0] & 7, f & 7)
    _, v2, _, _ = tower_step64(W, R["last_obs"], np.zeros((n, 4)))
    assert np.all(np.abs(R["last_values"] - v2) <= tol * (1.0 + value_scale(W, R["last_obs"])))
    assert env.step_counter == k0 + 1
    env.close()


def test_tower_runner_split_kernel_is_bit_identical_to_one_wave_per_tile(qa):
    """k_runner_split<..., towers> against k_runner_rollout<..., towers> on the same envs, every output and the final env
    state bit for bit, over the case matrix of the shared-trunk test"""
    import torch
    lib = qa._lib.load()
    lib.qs_debug_set_runner_serial.argtypes = [C.c_int]
    cases = [dict(n=3000, T=20, prec="f32", squash=False, rand=1, noise=False, env_major=False),
             dict(n=3000, T=20, prec="bf16x3", squash=False, rand=1, noise=True, env_major=False),
             dict(n=64 * 7 + 5, T=33, prec="f32", squash=True, rand=2, noise=False, env_major=True),
             dict(n=64 * 7 + 5, T=33, prec="bf16x3", squash=True, rand=2, noise=False, env_major=True),
             dict(n=1, T=9, prec="f32", squash=False, rand=0, noise=True, env_major=False),
             dict(n=8192, T=12, prec="bf16x3", squash=False, rand=0, noise=False, env_major=False)]
    try:
        for cs in cases:
            pol = qa.load_sb2_model(TOWERS_ZIP, squash=cs["squash"])
            res = []
            for serial in (1, 0):
                lib.qs_debug_set_runner_serial(serial)
                env = qa.VecDockingEnv("docking-v0", num_envs=cs["n"], randomise=cs["rand"], seed=11, init_range=qa.C3_INIT_RANGE)
                env.reset()
                env.set_state(t=np.full(cs["n"], 592.0, np.float32))
                g = torch.Generator().manual_seed(4)
                noise = torch.randn((cs["T"], cs["n"], 4), generator=g) if cs["noise"] else None
                dones_in = (torch.rand(cs["n"], generator=g) < 0.3)
                out = qa.fused_runner_rollout(env, pol, cs["T"], noise=noise, dones_in=dones_in, want_flags=True,
                                              precision=cs["prec"], env_major=cs["env_major"])
                rec = {k: v.cpu().numpy() for k, v in out.items()}
                rec.update({"state_" + k: v for k, v in env.get_state().items()})
                if cs["rand"] == 2:
                    m, inertia = env.get_params()
                    rec["mass"], rec["inertia"] = np.asarray(m), np.asarray(inertia)
                rec["counter"] = np.int64(env.step_counter)
                res.append(rec)
                env.close()
            a, b = res
            assert a["dones"].any() and a["counter"] == b["counter"]
            assert np.isfinite(a["values"]).all() and np.abs(a["values"]).max() > 0
            for k in a:
                assert np.array_equal(a[k], b[k]), (cs, k, np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
    finally:
        lib.qs_debug_set_runner_serial(0)


def test_tower_runner_run_fused_equals_stepwise(qa):
    """Runner.run() with load_sb2_model(<tower archive>): the fused launch against the spelt-out loop (torch model.step +
    env.step, fused=False) with identical noise; GAE equals compute_gae on the run's own outputs"""
    import torch
    pol = qa.load_sb2_model(TOWERS_ZIP)
    n, T = 777, 40
    kw = dict(num_envs=n, randomise=1, seed=5, init_range=qa.C3_INIT_RANGE)
    e1 = qa.VecDockingEnv("docking-v0", **kw); e2 = qa.VecDockingEnv("docking-v0", **kw)
    r1 = qa.Runner(env=e1, model=pol, n_steps=T, gamma=0.99, lam=0.95, fused=True)
    r2 = qa.Runner(env=e2, model=pol, n_steps=T, gamma=0.99, lam=0.95, fused=False)
    assert r1.fused and not r2.fused
    for e in (e1, e2):
        e.set_state(t=np.full(n, 575.0, np.float32))                  # time-outs at step 25
    noise = torch.randn((T, n, 4), generator=torch.Generator().manual_seed(1)).to(e1.device)
    a = [x for x in r1.run(noise=noise)]
    b = [x for x in r2.run(noise=noise)]
    names = ("obs", "returns", "masks", "actions", "values", "neglogp")
    for i, k in enumerate(names):
        x, y = a[i].cpu().numpy(), b[i].cpu().numpy()
        if k == "masks":
            assert np.array_equal(x, y) and x.any()
        else:
            np.testing.assert_allclose(x, y, rtol=2e-3, atol=2e-2 if k == "neglogp" else 2e-3, err_msg=k)
    np.testing.assert_allclose(a[8].cpu().numpy(), b[8].cpu().numpy(), atol=5e-3)
    assert np.array_equal(r1.dones.cpu().numpy(), r2.dones.cpu().numpy())
    # GAE of the fused run against compute_gae on its own rewards / values / dones
    f = lambda x: x.reshape(n, T).t().contiguous()                    # noqa: E731  undo swap_and_flatten
    last_v = pol.value(r1.obs)
    _, ret = qa.compute_gae(e1, f(a[8]), f(a[4]), f(a[2]).to(torch.uint8), last_v, r1.dones, 0.99, 0.95)
    np.testing.assert_allclose(f(a[1]).cpu().numpy(), ret.cpu().numpy(), rtol=1e-4, atol=1e-4)
    e1.close(); e2.close()
