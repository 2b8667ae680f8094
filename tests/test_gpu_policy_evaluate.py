"""-m gpu: qs_policy_evaluate / _fast (quadsim_amd.evaluate_policy_episodes) == the per-step loop
``obs -> policy.predict_hip(env, obs, precision) -> env.step`` on the same handle, bit for bit: float64 returns, lengths, OR-ed
flags, docked-step counts and finished counts of every env's first K episodes.  The evaluation leaves the handle untouched,
so the loop starts from the very state, parameters and step counter the kernel started from."""
import ctypes as C
import os

import numpy as np
import pytest

from step_matrix import NEW_EVAL_ROWS

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CKPT = {"shared": "sb2_best_model_v0.zip", "towers": "sb2_ppo2_docking_621_h_30M.zip"}


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def policies(qa):
    return {k: qa.MlpPolicy.from_sb2_zip(os.path.join(GOLDEN, v)) for k, v in CKPT.items()}


def _make(qa, env_id, rnd, n, params=False, seed=5, warm=17, integrator="frozen"):
    """a handle mid-episode: some envs close to the time-out, `warm` random steps taken -> (env, the last observation)"""
    kw = dict(num_envs=n, randomise=rnd, seed=seed, integrator=integrator)
    if rnd:
        kw.update(init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2))
    env = qa.VecDockingEnv(env_id, **kw)
    obs = env.reset()
    if params:
        rng = np.random.default_rng(seed)
        env.set_params(mass=rng.uniform(0.15, 0.21, n).astype(np.float32),
                       inertia=(np.array([0.00025, 0.000232, 0.0003738]) * rng.uniform(0.8, 1.2, (n, 3))).astype(np.float32))
    t0 = np.zeros(n, np.float32)
    t0[::7] = 590.0
    env.set_state(t=t0)
    acts = env.random_actions(warm)
    for t in range(warm):
        obs, _, _, _ = env.step(acts[t])
    return env, obs


def _loop(torch, env, pol, obs, precision, steps):
    """the per-step loop -> (reward [T,N] float32, done [T,N] bool, flags [T,N] uint8) on the host"""
    R, D, F = [], [], []
    for _ in range(steps):
        a = pol.predict_hip(env, obs, precision)
        obs, r, d, _ = env.step(a)
        R.append(r); D.append(d); F.append(env.last_flags)
    return torch.stack(R).cpu().numpy(), torch.stack(D).cpu().numpy(), torch.stack(F).cpu().numpy()


def _episodes(R, D, F, K):
    """each env's first K episodes of a loop record: float64 sequential return, length, OR of flags, docked steps, finished"""
    T, N = R.shape
    ret = np.full((K, N), np.nan)
    length = np.zeros((K, N), np.int32)
    flags = np.zeros((K, N), np.uint8)
    docked = np.zeros((K, N), np.int32)
    ep = np.zeros(N, np.int64)
    acc, ln, fl, dk = np.zeros(N), np.zeros(N, np.int32), np.zeros(N, np.uint8), np.zeros(N, np.int32)
    cols = np.arange(N)
    for t in range(T):
        live = ep < K
        acc = np.where(live, acc + R[t].astype(np.float64), acc)
        ln = ln + live
        fl = np.where(live, fl | F[t], fl)
        dk = dk + (live & ((F[t] & 1) != 0))
        end = live & D[t]
        e = cols[end]
        ret[ep[e], e], length[ep[e], e], flags[ep[e], e], docked[ep[e], e] = acc[e], ln[e], fl[e], dk[e]
        acc[end], ln[end], fl[end], dk[end] = 0.0, 0, 0, 0
        ep = ep + end
    return ret, length, flags, docked, ep.astype(np.int32)


def _assert_equal_episodes(res, ref):
    h = res.numpy()
    ret, length, flags, docked, fin = ref
    np.testing.assert_array_equal(h["finished"], fin)
    valid = np.arange(ret.shape[0])[:, None] < fin[None, :]
    # equal, not close (NaN where the loop's rewards are NaN too: a chaser driven into the attitude singularity)
    assert np.array_equal(h["returns"][valid], ret[valid], equal_nan=True)
    np.testing.assert_array_equal(h["lengths"][valid], length[valid])
    np.testing.assert_array_equal(h["flags"][valid], flags[valid])
    np.testing.assert_array_equal(h["docked_steps"][valid], docked[valid])


ENVS = [("docking-v0", 0, False), ("docking-v0", 1, False), ("docking-v0", 2, False), ("docking-v2", 0, False),
        ("docking-v2", 1, False), ("docking-v2", 2, False), ("docking-v1", 0, False), ("docking-v0", 1, True)]
CASES = [(env_id, rnd, params, prec, ck, (1000, 4096)[(i + j) % 2])
         for i, (env_id, rnd, params) in enumerate(ENVS) for prec in ("f32", "bf16x3") for j, ck in enumerate(CKPT)]


@pytest.mark.parametrize("env_id,rnd,params,precision,ckpt,n", CASES)
def test_evaluate_equals_per_step_loop(qa, torch, policies, env_id, rnd, params, precision, ckpt, n):
    K = 2
    env, obs = _make(qa, env_id, rnd, n, params)
    pol = policies[ckpt]
    res = qa.evaluate_policy_episodes(pol, env, K, precision=precision)
    ref = _episodes(*_loop(torch, env, pol, obs, precision, K * 600), K)
    _assert_equal_episodes(res, ref)
    assert (ref[4] == K).all()                        # every episode ends by the env's time-out within K x 600 steps
    env.close()


@pytest.mark.parametrize("row", NEW_EVAL_ROWS, ids=[r["id"] for r in NEW_EVAL_ROWS])
def test_evaluate_matrix_equals_per_step_loop(qa, torch, policies, row):
    """the (INTEG, PARAMS, RMODE) instantiations of both evaluation kernels the cases above do not reach (every rk4 one; per-env
    params with RMODE 0 and 3), K = 1, against the per-step loop through the step kernels (which tests/test_gpu_step_matrix.py
    pins to the oracle)"""
    K = 1
    env, obs = _make(qa, row["env_id"], row["randomise"], row["n"], row["set_params"], integrator=row["integ"])
    lib = env._lib
    lib.qs_debug_step_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    v = (C.c_int32 * 5)()
    assert lib.qs_debug_step_variant(env._h, v) == 0
    assert tuple(v)[1:4] == row["combo"]                   # the evaluation kernel takes the step kernel's (INTEG, PARAMS, RMODE)
    pol = policies[row["ckpt"]]
    res = qa.evaluate_policy_episodes(pol, env, K, precision=row["precision"])
    ref = _episodes(*_loop(torch, env, pol, obs, row["precision"], K * 600), K)
    _assert_equal_episodes(res, ref)
    assert (ref[4] == K).all()
    env.close()


def test_evaluate_is_read_only_and_repeatable(qa, torch, policies):
    """state, per-env parameters and the step counter are unchanged; a second call gives the same episodes"""
    env, _ = _make(qa, "docking-v2", 2, 1000)
    st0, par0, k0 = env.get_state(), env.get_params(), env.step_counter
    a = qa.evaluate_policy_episodes(policies["towers"], env, 2).numpy()
    st1, par1, k1 = env.get_state(), env.get_params(), env.step_counter
    b = qa.evaluate_policy_episodes(policies["towers"], env, 2).numpy()
    assert k0 == k1 == env.step_counter == 17
    for k in st0:
        np.testing.assert_array_equal(st0[k], st1[k])
    for x, y in zip(par0, par1):
        np.testing.assert_array_equal(x, y)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    env.close()


def test_truncation_leaves_unfinished_slots_untouched(qa, torch, policies):
    """max_steps = 250, K = 2 through the C ABI: `finished` as derived from 250 loop steps; slots of episodes that did not
    end keep a sentinel"""
    K, n, T = 2, 1000, 250
    env, obs = _make(qa, "docking-v0", 1, n)
    pol = policies["shared"]
    kw = dict(device=env.device)
    ret = torch.full((K, n), -123.5, dtype=torch.float64, **kw)
    length = torch.full((K, n), -7, dtype=torch.int32, **kw)
    flags = torch.full((K, n), 0xAB, dtype=torch.uint8, **kw)
    docked = torch.full((K, n), -9, dtype=torch.int32, **kw)
    fin = torch.full((n,), -1, dtype=torch.int32, **kw)
    p = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
    assert env._lib.qs_policy_evaluate(env._h, K, T, *[p(w) for w in pol.transposed_weights()], p(ret), p(length), p(flags), p(docked), p(fin)) == 0
    torch.cuda.synchronize()
    r, le, fl, dk, f = _episodes(*_loop(torch, env, pol, obs, "f32", T), K)
    np.testing.assert_array_equal(fin.cpu().numpy(), f)
    assert 0 < (f == 0).sum() and 0 < (f == 1).sum()                 # some envs end an episode inside the window, some do not
    valid = np.arange(K)[:, None] < f[None, :]
    h = [x.cpu().numpy() for x in (ret, length, flags, docked)]
    assert np.array_equal(h[0][valid], r[valid], equal_nan=True) and np.array_equal(h[1][valid], le[valid])
    assert np.array_equal(h[2][valid], fl[valid]) and np.array_equal(h[3][valid], dk[valid])
    assert (h[0][~valid] == -123.5).all() and (h[1][~valid] == -7).all() and (h[2][~valid] == 0xAB).all() and (h[3][~valid] == -9).all()
    env.close()


def test_reference_episode_g5(qa, torch):
    """the shipped actor on docking-v0 from the nominal start: one episode of 600 steps ending by time-out, 183 +- 3 docked
    steps, return within 5e-3 of the reference's (fixture g5; the tolerances of the closed-loop test in test_gpu_parity.py)"""
    g = np.load(os.path.join(GOLDEN, "g5_policy_episode.npz"), allow_pickle=False)
    pol = qa.MlpPolicy.from_npz(os.path.join(GOLDEN, "policy_best_model_v0.npz"))
    env = qa.VecDockingEnv("docking-v0", num_envs=8)
    env.reset()
    h = qa.evaluate_policy_episodes(pol, env, 1).numpy()
    assert (h["finished"] == 1).all() and (h["lengths"] == 600).all()
    assert (h["flags"] & qa._lib.FLAG_OVERTIME).all()
    assert (np.abs(h["docked_steps"] - 183) <= 3).all()
    assert (np.abs(h["returns"] - float(g["reward"].sum())) < 5e-3).all()
    env.close()


def test_private_queue_handle_evaluates_like_hip_stream_twin(qa, torch, policies):
    """a host-ordered private-queue handle (resident step kernel holds its latest state) is drained first: same episodes as a
    HIP-stream twin stepped identically, and both step on identically afterwards"""
    n = 4096
    kw = dict(num_envs=n, randomise=1, seed=9, init_range=qa.C3_INIT_RANGE)
    a, b = qa.VecDockingEnv("docking-v0", **kw), qa.VecDockingEnv("docking-v0", **kw)
    try:
        b.set_queue_mode(True, 2, ordering="host")
    except qa.QuadsimError as exc:
        a.close(); b.close()
        pytest.skip("private queues unavailable: %s" % exc)
    a.reset(); b.reset()
    acts = a.random_actions(12)
    for t in range(12):
        a.step(acts[t]); b.step(acts[t])
    ea = qa.evaluate_policy_episodes(policies["shared"], a, 2, precision="bf16x3").numpy()
    eb = qa.evaluate_policy_episodes(policies["shared"], b, 2, precision="bf16x3").numpy()
    for k in ea:
        np.testing.assert_array_equal(ea[k], eb[k])
    for t in range(5):
        oa, ra, _, _ = a.step(acts[t])
        ob, rb, _, _ = b.step(acts[t])
        assert torch.equal(oa, ob) and torch.equal(ra, rb)
    assert a.step_counter == b.step_counter == 17
    a.close(); b.close()


def test_guards_and_sb2_surface(qa, torch, policies):
    """hovering-v0, episodes = 0 and max_steps = 0 are refused; evaluate_policy = NumPy mean / std over the episode tensors;
    an ActorCriticPolicy evaluates as its actor; the summary helpers"""
    hv = qa.VecDockingEnv("hovering-v0", num_envs=64)
    with pytest.raises(qa.QuadsimError):
        qa.evaluate_policy_episodes(policies["shared"], hv, 1)
    hv.close()
    n = 1000
    env, _ = _make(qa, "docking-v2", 1, n)
    with pytest.raises(qa.QuadsimError):
        qa.evaluate_policy_episodes(policies["shared"], env, 0)
    with pytest.raises(qa.QuadsimError):
        qa.evaluate_policy_episodes(policies["shared"], env, 1, max_steps=0)
    res = qa.evaluate_policy_episodes(policies["towers"], env, 2)
    h = res.numpy()
    mean, std = qa.evaluate_policy(policies["towers"], env, 2 * n)
    flat = h["returns"].reshape(-1).tolist()                          # (k, env) order
    assert np.array_equal([mean, std], [np.mean(flat), np.std(flat)], equal_nan=True)
    rews, lens = qa.evaluate_policy(policies["towers"], env, 2 * n, return_episode_rewards=True)
    assert np.array_equal(rews, flat, equal_nan=True) and lens == h["lengths"].reshape(-1).tolist()
    with pytest.raises(ValueError):
        qa.evaluate_policy(policies["towers"], env, n + 1)
    ac = qa.load_sb2_model(os.path.join(GOLDEN, CKPT["towers"]))
    g = qa.evaluate_policy_episodes(ac, env, 2).numpy()
    for k in h:
        np.testing.assert_array_equal(g[k], h[k])
    assert res.num_episodes() == 2 * n
    assert res.mean_return() == pytest.approx(np.mean(h["returns"]), rel=1e-12, nan_ok=True)
    assert res.std_return() == pytest.approx(np.std(h["returns"]), rel=1e-9, nan_ok=True)
    assert res.mean_length() == pytest.approx(np.mean(h["lengths"]), rel=1e-12, nan_ok=True)
    assert res.docked_fraction() == pytest.approx(np.mean(h["docked_steps"] > 0), rel=1e-12, nan_ok=True)
    assert res.overlimit_fraction() == pytest.approx(np.mean((h["flags"] & 2) != 0), rel=1e-12, nan_ok=True)
    env.close()
