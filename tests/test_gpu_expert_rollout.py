"""-m gpu: qs_expert_rollout / qs_expert_evaluate (PIDExpert.rollout / .evaluate, record_expert_dataset(fused=True)) against
the per-step loop ``a = expert.act(); env.step(a)`` on a twin handle, bit for bit, in every (INTEG, PARAMS, RMODE) combination
of the step API; against the reference's recorded expert episode (fixture g11); and through the handle's other launch paths."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAR_NOM = np.array([0.18, 0.00025, 0.000232, 0.0003738])


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---------------------------------------------------------------- handles
# (env id, mode): nominal resets, rocRAND initial states, + per-episode parameters, stored per-env initial states
MODES = {"nominal": 0, "init": 1, "init_params": 2, "stored": 0}
HANDLES = [(e, m) for e in ("docking-v0", "docking-v2") for m in MODES] + [("docking-v1", "stored")]   # v1 always stores its starts
CASES = []
for _i, (_e, _m) in enumerate(HANDLES):
    for _p in ((False,) if _m == "init_params" else (False, True)):       # per-episode parameters imply per-env parameters
        for _g in ("frozen", "rk4"):
            CASES.append((_e, _m, _p, _g, (200, 40, 257)[len(CASES) % 3]))   # ragged: a last tile that is not full, and N < 64


def _make(qa, env_id, mode, params, integ, n, seed=11, provoke=True):
    """the case's handle after a reset; with `provoke` a fifth of the envs is put at t = 590..599 and another fifth just inside
    the over-limit radius, flying outwards.  Identical for every call with the same arguments."""
    kw = dict(num_envs=n, randomise=MODES[mode], seed=seed, integrator=integ, copy=False)
    if MODES[mode]:
        kw.update(init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2))
    env = qa.VecDockingEnv(env_id, **kw)
    rng = np.random.default_rng(seed)
    if mode == "stored" and env_id != "docking-v1":
        c = np.tile(np.array([8, -50, 5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32), (n, 1))
        c[:, 0:3] += rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
        env.set_init_state(c)
    if params:
        env.set_params(mass=(0.18 * rng.uniform(0.85, 1.15, n)).astype(np.float32),
                       inertia=(PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))
    env.reset()
    if provoke:
        st = env.get_state()
        idx = np.arange(n)
        t0 = st["t"].copy()
        timed = idx % 5 == 0
        t0[timed] = 590.0 + (idx[timed] // 5) % 10                       # time-outs at steps 1..10 (599: on the very next step)
        far = idx % 5 == 1
        rmax = 10.0 if env_id == "docking-v2" else 3.0
        c = st["chaser"].copy()
        gap = 0.03 + 0.04 * ((idx[far] // 5) % 6)                        # port-to-port distance rmax - gap, 2 m/s outwards
        c[far, 0] = st["target"][far, 0] - 0.2 - rmax + gap
        c[far, 1:3] = st["target"][far, 1:3]
        c[far, 3:6] = np.array([-2.0, 0.0, 0.0], np.float32)
        c[far, 6:10] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
        c[far, 10:13] = 0.0
        env.set_state(chaser=c, t=t0)
    return env


def _loop(torch, env, ex, obs, T):
    """T times qs_expert_action; qs_step -> dict like PIDExpert.rollout(T, flags=True) returns, time-major"""
    O, A, R, D, F = [], [], [], [], []
    for _ in range(T):
        a = ex.act()
        O.append(obs.clone()); A.append(a.clone())
        obs, r, d, _ = env.step(a)
        R.append(r.clone()); D.append(d.clone()); F.append(env.last_flags.clone())
    return {"obs": torch.stack(O), "actions": torch.stack(A), "rewards": torch.stack(R), "dones": torch.stack(D),
            "flags": torch.stack(F), "last_obs": obs.clone()}


def _warm(torch, env):
    """one step with zero actions: its observation is what the roll-out's row 0 has to reproduce (the envs put at t = 599 end
    their episode here, so row 0 of those is a reset's observation)"""
    obs, _, d, _ = env.step(torch.zeros((env.num_envs, 4), device=env.device))
    return obs.clone(), d.clone()


def _assert_same_handle(torch, a, b, exa, exb):
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), k
    for x, y in zip(a.get_params(), b.get_params()):
        assert np.array_equal(x, y)
    assert a.step_counter == b.step_counter
    assert torch.equal(exa.state_des, exb.state_des)


def _assert_same_rollout(torch, ref, got, env_major=False):
    wide = (lambda x: x.transpose(0, 1)) if env_major else (lambda x: x)
    assert torch.equal(ref["obs"][0], wide(got["obs"])[0])                # row 0: the observation the previous step returned
    for k in ("obs", "actions"):
        assert torch.equal(ref[k], wide(got[k])), k
    for k in ("rewards", "dones", "flags", "last_obs"):
        assert torch.equal(ref[k], got[k]), k


# ---------------------------------------------------------------- 5. bit identity with the per-step loop
@pytest.mark.parametrize("env_id,mode,params,integ,n", CASES,
                         ids=["%s-%s-%s-%s-%d" % (e, m, "par" if p else "nopar", g, n) for e, m, p, g, n in CASES])
def test_rollout_equals_per_step_loop(qa, torch, env_id, mode, params, integ, n):
    T, T2 = 16, 9
    a, b = _make(qa, env_id, mode, params, integ, n), _make(qa, env_id, mode, params, integ, n)
    exa, exb = qa.PIDExpert(a), qa.PIDExpert(b)
    obs_a, d_a = _warm(torch, a)
    obs_b, d_b = _warm(torch, b)
    assert torch.equal(obs_a, obs_b) and bool(d_a.any())
    ref = _loop(torch, a, exa, obs_a, T)
    got = exb.rollout(T, flags=True)
    _assert_same_rollout(torch, ref, got)
    _assert_same_handle(torch, a, b, exa, exb)
    # conditions of the test: at least a tenth of the envs reset inside T, and some env takes the first step of an episode
    # (the t == 0 rule of the expert) at a step other than 0
    dn = ref["dones"].cpu().numpy()
    assert dn.any(axis=0).sum() * 10 >= n, dn.any(axis=0).sum()
    assert dn[:-1].any()
    fl = ref["flags"].cpu().numpy()
    assert ((fl & 2) != 0).any() and ((fl & 4) != 0).any()                # both the over-limit and the time-out reset ran
    # a second roll-out continues where the loop continues; env-major layout
    ref2 = _loop(torch, a, exa, ref["last_obs"], T2)
    got2 = exb.rollout(T2, flags=True, env_major=True)
    assert tuple(got2["obs"].shape) == (n, T2, 12) and tuple(got2["actions"].shape) == (n, T2, 4)
    _assert_same_rollout(torch, ref2, got2, env_major=True)
    _assert_same_handle(torch, a, b, exa, exb)
    assert b.step_counter == 1 + T + T2
    a.close(); b.close()


def test_rollout_right_after_reset_and_without_optional_outputs(qa, torch):
    """row 0 after qs_reset (nominal: the device-computed nominal observation; stored: docking-v1's jittered starts), flags
    and last_obs left out through the C ABI"""
    for env_id in ("docking-v0", "docking-v1"):
        n, T = 130, 5
        a, b = qa.VecDockingEnv(env_id, num_envs=n, seed=3), qa.VecDockingEnv(env_id, num_envs=n, seed=3)
        exa, exb = qa.PIDExpert(a), qa.PIDExpert(b)
        obs = a.reset(); b.reset()
        ref = _loop(torch, a, exa, obs, T)
        kw = dict(device=b.device)
        O, A = torch.empty((T, n, 12), **kw), torch.empty((T, n, 4), **kw)
        R, D = torch.empty((T, n), **kw), torch.empty((T, n), dtype=torch.uint8, **kw)
        p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
        b._use_current_stream()
        assert b._lib.qs_set_rollout_layout(b._h, 0) == 0
        assert b._lib.qs_expert_rollout(b._h, T, p(exb.state_des), exb.kp, exb.kd, p(O), p(A), p(R), p(D), None, None) == 0
        assert torch.equal(O, ref["obs"]) and torch.equal(A, ref["actions"]) and torch.equal(R, ref["rewards"])
        assert torch.equal(D.bool(), ref["dones"])
        _assert_same_handle(torch, a, b, exa, exb)
        a.close(); b.close()


# ---------------------------------------------------------------- 6. reference parity (fixture g11)
def test_rollout_reproduces_reference_expert_episode_g11(qa, torch):
    """docking-v0 from the nominal start, as fixture g11 was recorded: the tolerances of test_g11_pid_expert_and_dataset's
    per-step closed loop (tests/test_gpu_parity.py)"""
    g = np.load(os.path.join(GOLDEN, "g11_expert_episode.npz"), allow_pickle=False)
    T = len(g["actions"])
    env = qa.VecDockingEnv("docking-v0", num_envs=4, auto_reset=True)
    ex = qa.PIDExpert(env, *g["kp_kd"])
    env.reset()
    ro = ex.rollout(T, flags=True)
    obs, rew = ro["obs"].cpu().numpy(), ro["rewards"].cpu().numpy()
    done, flags = ro["dones"].cpu().numpy(), ro["flags"].cpu().numpy()
    for t in range(T):
        np.testing.assert_allclose(obs[t, 0], g["obs"][t], rtol=5e-3, atol=5e-3)
        assert bool(done[t, 0]) == bool(g["done"][t])
    ret = 0.0
    for t in range(T):
        ret += float(rew[t, 0])
    docked = int((flags[:, 0] & 1).sum())
    print("g11: return %.6f (reference %.6f), docked steps %d (reference 156)" % (ret, float(g["rewards"].sum()), docked))
    assert abs(ret - float(g["rewards"].sum())) < 2e-2 and abs(docked - 156) <= 4
    # ... and the evaluation kernel's record of the same episode
    env.reset()
    ex2 = qa.PIDExpert(env, *g["kp_kd"])
    h = ex2.evaluate(1).numpy()
    assert (h["finished"] == 1).all() and (h["lengths"] == T).all()
    assert (np.abs(h["returns"] - float(g["rewards"].sum())) < 2e-2).all() and (np.abs(h["docked_steps"] - 156) <= 4).all()
    env.close()


# ---------------------------------------------------------------- 7. evaluation
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


EVAL_CASES = [("docking-v0", "init", False, "frozen", 200), ("docking-v2", "init_params", False, "frozen", 257),
              ("docking-v1", "stored", True, "rk4", 40), ("docking-v0", "nominal", True, "rk4", 130)]


@pytest.mark.parametrize("env_id,mode,params,integ,n", EVAL_CASES)
def test_evaluate_equals_per_step_loop_and_is_read_only(qa, torch, env_id, mode, params, integ, n):
    K = 2
    a, b = _make(qa, env_id, mode, params, integ, n), _make(qa, env_id, mode, params, integ, n)
    exa, exb = qa.PIDExpert(a), qa.PIDExpert(b)
    obs_a, _ = _warm(torch, a)
    _warm(torch, b)
    st0, par0, k0, sd0 = b.get_state(), b.get_params(), b.step_counter, exb.state_des.clone()
    res = exb.evaluate(K).numpy()
    res2 = exb.evaluate(K).numpy()
    # nothing written back: state, parameters, step counter, the caller's state_des; a second call gives the same records
    st1, par1 = b.get_state(), b.get_params()
    for k in st0:
        assert np.array_equal(st0[k], st1[k], equal_nan=True), k
    for x, y in zip(par0, par1):
        assert np.array_equal(x, y)
    assert b.step_counter == k0 == 1 and torch.equal(exb.state_des, sd0)
    for k in res:
        assert np.array_equal(res[k], res2[k], equal_nan=True), k
    # the twin's per-step loop: the records
    ref = _loop(torch, a, exa, obs_a, K * 600)
    R, D, F = (ref[k].cpu().numpy() for k in ("rewards", "dones", "flags"))
    ret, length, flags, docked, fin = _episodes(R, D, F, K)
    assert (fin == K).all()
    assert np.array_equal(res["finished"], fin)
    assert np.array_equal(res["returns"], ret, equal_nan=True)                      # bit-equal float64 sums
    assert np.array_equal(res["lengths"], length) and np.array_equal(res["flags"], flags)
    assert np.array_equal(res["docked_steps"], docked)
    assert (length[0] < 600).sum() * 10 >= n                                        # the provoked early ends are among them
    # stepping on gives what the twin that never evaluated gave
    got = _loop(torch, b, exb, obs_a, 20)
    for k in ("obs", "actions", "rewards", "dones", "flags"):
        assert torch.equal(got[k], ref[k][:20]), k
    a.close(); b.close()


def test_evaluate_truncation_leaves_unfinished_slots_untouched(qa, torch):
    """max_steps = 250, K = 2 through the C ABI: `finished` as derived from 250 loop steps; slots of episodes that did not end
    keep a sentinel"""
    K, n, T = 2, 200, 250
    # nominal starts: the expert flies the full 600 steps from them, so only the provoked envs end an episode within 250
    a, b = _make(qa, "docking-v0", "nominal", True, "frozen", n), _make(qa, "docking-v0", "nominal", True, "frozen", n)
    exa, exb = qa.PIDExpert(a), qa.PIDExpert(b)
    obs_a, _ = _warm(torch, a)
    _warm(torch, b)
    kw = dict(device=b.device)
    ret = torch.full((K, n), -123.5, dtype=torch.float64, **kw)
    length = torch.full((K, n), -7, dtype=torch.int32, **kw)
    flags = torch.full((K, n), 0xAB, dtype=torch.uint8, **kw)
    docked = torch.full((K, n), -9, dtype=torch.int32, **kw)
    fin = torch.full((n,), -1, dtype=torch.int32, **kw)
    p = lambda t: C.c_void_p(t.data_ptr())            # noqa: E731
    b._use_current_stream()
    assert b._lib.qs_expert_evaluate(b._h, K, T, p(exb.state_des), exb.kp, exb.kd, p(ret), p(length), p(flags), p(docked), p(fin)) == 0
    torch.cuda.synchronize()
    ref = _loop(torch, a, exa, obs_a, T)
    r, le, fl, dk, f = _episodes(*(ref[k].cpu().numpy() for k in ("rewards", "dones", "flags")), K)
    assert np.array_equal(fin.cpu().numpy(), f)
    assert 0 < (f == 0).sum() and 0 < (f >= 1).sum()                 # some envs end an episode inside the window, some do not
    valid = np.arange(K)[:, None] < f[None, :]
    h = [x.cpu().numpy() for x in (ret, length, flags, docked)]
    assert np.array_equal(h[0][valid], r[valid], equal_nan=True) and np.array_equal(h[1][valid], le[valid])
    assert np.array_equal(h[2][valid], fl[valid]) and np.array_equal(h[3][valid], dk[valid])
    assert (h[0][~valid] == -123.5).all() and (h[1][~valid] == -7).all() and (h[2][~valid] == 0xAB).all() and (h[3][~valid] == -9).all()
    a.close(); b.close()


# ---------------------------------------------------------------- 8. dataset
def _episode_bounds(starts, rewards):
    """per episode of an env-major recording: (first row, float64 sum, L, sum |r|) from episode_starts"""
    first = np.nonzero(starts)[0]
    r64 = rewards.astype(np.float64)
    return first, np.add.reduceat(r64, first), np.diff(np.append(first, len(starts))), np.add.reduceat(np.abs(r64), first)


def test_dataset_fused_equals_per_step_recording(qa, torch, tmp_path):
    n, T = 257, 700
    a, b = qa.VecDockingEnv("docking-v1", num_envs=n, seed=21), qa.VecDockingEnv("docking-v1", num_envs=n, seed=21)
    fused = qa.record_expert_dataset(a, n_steps=T, fused=True)
    loop = qa.record_expert_dataset(b, n_steps=T, fused=False)
    for k in ("actions", "obs", "rewards", "episode_starts"):
        assert fused[k].dtype == loop[k].dtype and np.array_equal(fused[k], loop[k]), k
    assert fused["obs"].shape == (n * T, 12) and fused["actions"].shape == (n * T, 4)
    assert fused["episode_returns"].dtype == np.float64 and fused["episode_returns"].shape == loop["episode_returns"].shape
    # which episodes are complete: the done flags of a third twin's roll-out (an env's last episode may end on the last row)
    c = qa.VecDockingEnv("docking-v1", num_envs=n, seed=21)
    c.reset()
    ro = qa.PIDExpert(c).rollout(T)
    done = ro["dones"].cpu().numpy().T.reshape(-1)
    assert np.array_equal(ro["rewards"].cpu().numpy().T.reshape(-1), fused["rewards"])
    first, s, L, sabs = _episode_bounds(fused["episode_starts"], fused["rewards"])
    complete = np.zeros(len(first), bool)
    complete[(np.cumsum(fused["episode_starts"]) - 1)[done]] = True
    assert complete.sum() == len(fused["episode_returns"]) >= n and (~complete).sum() > 0
    bound = 2.0 * L[complete] * 2.0 ** -53 * sabs[complete]
    assert (np.abs(fused["episode_returns"] - loop["episode_returns"]) <= bound).all()
    assert (np.abs(fused["episode_returns"] - s[complete]) <= bound).all()
    c.close()
    a.close(); b.close()


def test_dataset_n_episodes_records_complete_episodes_only(qa, torch, tmp_path):
    n, K = 257, 2
    a, b = qa.VecDockingEnv("docking-v1", num_envs=n, seed=21), qa.VecDockingEnv("docking-v1", num_envs=n, seed=21)
    path = str(tmp_path / "expert_episodes.npz")
    data = qa.record_expert_dataset(a, n_episodes=K, save_path=path)
    long = qa.record_expert_dataset(b, n_steps=K * 600)
    rows = len(data["rewards"])
    assert data["obs"].shape == (rows, 12) and data["actions"].shape == (rows, 4) and data["episode_starts"].shape == (rows,)
    assert data["episode_starts"].sum() == K * n and len(data["episode_returns"]) == K * n and data["episode_starts"][0]
    first, s, L, sabs = _episode_bounds(data["episode_starts"], data["rewards"])
    assert (np.abs(data["episode_returns"] - s) <= 2.0 * L * 2.0 ** -53 * sabs).all()
    # the rows are every env's leading rows of a long recording of a twin: its first K episodes
    ls = long["episode_starts"].reshape(n, K * 600)
    lead = (np.cumsum(ls, axis=1) <= K).reshape(-1)
    assert lead.sum() == rows
    for k in ("obs", "actions", "rewards", "episode_starts"):
        assert np.array_equal(data[k], long[k][lead]), k
    # every env's rows end with the end of its K-th episode: the row after them starts an episode (or the recording ends)
    assert (L <= 600).all()
    z = np.load(path, allow_pickle=False)
    assert sorted(z.files) == ["actions", "episode_returns", "episode_starts", "obs", "rewards"]
    for k in z.files:
        assert np.array_equal(z[k], data[k])
    a.close(); b.close()


# ---------------------------------------------------------------- 9. launch paths
def _twins_stepped(qa, torch, n, steps, prepare):
    kw = dict(num_envs=n, randomise=1, seed=9, init_range=qa.C3_INIT_RANGE)
    a, b = qa.VecDockingEnv("docking-v0", **kw), qa.VecDockingEnv("docking-v0", **kw)
    prepare(b)
    a.reset(); b.reset()
    acts = a.random_actions(steps)
    return a, b, acts


def _rollout_all(torch, ex, T):
    ro = ex.rollout(T, flags=True)
    torch.cuda.synchronize()
    return ro


def test_private_queue_handle_rolls_out_like_hip_stream_twin(qa, torch):
    """host-ordered private-queue handle with qs_step calls still in flight (the resident step kernel holds the latest state):
    drained first, then the same roll-out as a HIP-stream twin that took the same steps"""
    n, T = 4096, 12
    state = {}

    def prepare(b):
        try:
            b.set_queue_mode(True, 2, ordering="host")
        except qa.QuadsimError as exc:
            state["skip"] = str(exc)
    a, b, acts = _twins_stepped(qa, torch, n, 12, prepare)
    if "skip" in state:
        a.close(); b.close()
        pytest.skip("private queues unavailable: %s" % state["skip"])
    torch.cuda.synchronize()
    for t in range(12):
        a.step(acts[t])
        b.step_async(acts[t])                               # not waited for: in flight when the roll-out is called
    exa, exb = qa.PIDExpert(a), qa.PIDExpert(b)
    ra, rb = _rollout_all(torch, exa, T), _rollout_all(torch, exb, T)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    _assert_same_handle(torch, a, b, exa, exb)
    assert a.step_counter == 12 + T
    oa, ra_, _, _ = a.step(acts[0])
    ob, rb_, _, _ = b.step(acts[0])
    assert torch.equal(oa, ob) and torch.equal(ra_, rb_)
    a.close(); b.close()


def test_grouped_handle_rolls_out_like_plain_twin(qa, torch):
    n, T = 4096, 12
    a, b, acts = _twins_stepped(qa, torch, n, 6, lambda b: b.set_groups(4))
    for t in range(6):
        a.step(acts[t])
        b.step_groups(acts[t])                              # group streams hold the work: the roll-out joins them first
    exa, exb = qa.PIDExpert(a), qa.PIDExpert(b)
    ra, rb = _rollout_all(torch, exa, T), _rollout_all(torch, exb, T)
    for k in ra:
        assert torch.equal(ra[k], rb[k]), k
    _assert_same_handle(torch, a, b, exa, exb)
    a.close(); b.close()


def test_rollout_is_graph_capturable_and_replay_advances(qa, torch):
    """one capture of qs_expert_rollout(T = 8) on the HIP stream, replayed twice == two eager calls (the step counter lives in
    device memory, so a replay draws the next steps' reset randomness)"""
    n, T = 2048, 8
    kw = dict(num_envs=n, randomise=1, seed=8, init_range=qa.C3_INIT_RANGE)
    eager, cap = qa.VecDockingEnv("docking-v0", **kw), qa.VecDockingEnv("docking-v0", **kw)
    t0 = np.zeros(n, np.float32); t0[::2] = 590.0                   # half the envs time out inside the 16 steps
    for e in (eager, cap):
        e.reset(); e.set_state(t=t0)
    exe, exc = qa.PIDExpert(eager), qa.PIDExpert(cap)
    ref = [exe.rollout(T, flags=True) for _ in range(2)]
    torch.cuda.synchronize()
    dkw = dict(device=cap.device)
    O, A = torch.empty((T, n, 12), **dkw), torch.empty((T, n, 4), **dkw)
    R, D, F = torch.empty((T, n), **dkw), torch.empty((T, n), dtype=torch.uint8, **dkw), torch.empty((T, n), dtype=torch.uint8, **dkw)
    L = torch.empty((n, 12), **dkw)
    p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
    assert cap._lib.qs_set_rollout_layout(cap._h, 0) == 0
    torch.cuda.synchronize()
    k_before = cap.step_counter
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap._use_current_stream()
        rc = cap._lib.qs_expert_rollout(cap._h, T, p(exc.state_des), exc.kp, exc.kd, p(O), p(A), p(R), p(D), p(F), p(L))
    assert rc == 0
    cap._use_current_stream()
    assert cap.step_counter == k_before                              # capture launches nothing
    n_done = 0
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        r = ref[rep]
        assert torch.equal(O, r["obs"]) and torch.equal(A, r["actions"]) and torch.equal(R, r["rewards"])
        assert torch.equal(D.bool(), r["dones"]) and torch.equal(F, r["flags"]) and torch.equal(L, r["last_obs"])
        n_done += int(D.sum())
    assert n_done >= n // 2 and cap.step_counter == k_before + 2 * T
    _assert_same_handle(torch, eager, cap, exe, exc)
    eager.close(); cap.close()


# ---------------------------------------------------------------- 10. refusals
def test_refusals_leave_the_handle_usable(qa, torch):
    INVALID = -1
    lib = qa._lib.load()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731

    def calls(env, T=4, K=1, sd="ok", obs="ok"):
        """(rc of qs_expert_rollout, rc of qs_expert_evaluate, their messages) with fresh buffers"""
        n, kw = env.num_envs, dict(device="cuda")
        tt = max(T, 1)
        S = torch.zeros((n, 13), **kw) if sd == "ok" else None
        O = torch.empty((tt, n, 12), **kw) if obs == "ok" else None
        A, R, D = torch.empty((tt, n, 4), **kw), torch.empty((tt, n), **kw), torch.empty((tt, n), dtype=torch.uint8, **kw)
        ret = torch.empty((max(K, 1), n), dtype=torch.float64, **kw)
        le, fin = torch.empty((max(K, 1), n), dtype=torch.int32, **kw), torch.empty((n,), dtype=torch.int32, **kw)
        r1 = lib.qs_expert_rollout(env._h, T, p(S), 0.35, 0.0, p(O), p(A), p(R), p(D), None, None)
        m1 = lib.qs_last_error().decode()
        r2 = lib.qs_expert_evaluate(env._h, K, 600, p(S), 0.35, 0.0, p(ret) if obs == "ok" else None, p(le), None, None, p(fin))
        m2 = lib.qs_last_error().decode()
        torch.cuda.synchronize()
        return r1, r2, m1, m2

    hv = qa.VecDockingEnv("hovering-v0", num_envs=64)
    hv.reset()
    r1, r2, m1, m2 = calls(hv)
    assert r1 == r2 == INVALID and "qs_expert_rollout" in m1 and "qs_expert_evaluate" in m2 and "docking" in m1
    hv.step(torch.rand((64, 4), device="cuda"))                                                            # still usable
    hv.close()

    na = qa.VecDockingEnv("docking-v0", num_envs=64, auto_reset=False)
    na.reset()
    r1, r2, m1, m2 = calls(na)
    assert r1 == r2 == INVALID and "auto_reset" in m1 and "auto_reset" in m2
    na.step(torch.zeros((64, 4), device="cuda"))
    na.close()

    env = qa.VecDockingEnv("docking-v0", num_envs=64)
    env.reset()
    r1, r2, m1, m2 = calls(env, sd=None)
    assert r1 == r2 == INVALID and "state_des" in m1 and "state_des" in m2
    r1, r2, m1, m2 = calls(env, obs=None)
    assert r1 == r2 == INVALID and "required" in m1 and "required" in m2
    r1, _, m1, _ = calls(env, T=0)
    assert r1 == INVALID and "T must be" in m1
    r1, _, m1, _ = calls(env, T=-3)
    assert r1 == INVALID
    _, r2, _, m2 = calls(env, K=0)
    assert r2 == INVALID and "episodes" in m2
    ex = qa.PIDExpert(env)
    with pytest.raises(qa.QuadsimError):
        ex.rollout(0)
    with pytest.raises(qa.QuadsimError):
        ex.evaluate(0)
    with pytest.raises(qa.QuadsimError):
        ex.evaluate(1, max_steps=0)
    r1, r2, _, _ = calls(env)                                               # and a good call still works
    assert r1 == 0 and r2 == 0
    assert env.step_counter == 8                                            # this roll-out and the one beside the refused K = 0
    ro = ex.rollout(3)
    assert bool(torch.isfinite(ro["obs"]).all()) and env.step_counter == 11
    env.close()

    # host I/O: a handle created for host buffers through the C ABI
    cfg = qa._lib.default_config()
    cfg.kind, cfg.num_envs, cfg.io_space, cfg.auto_reset = qa._lib.KIND_V0, 8, qa._lib.IO_HOST, 1
    h = C.c_void_p()
    assert lib.qs_create(C.byref(cfg), C.byref(h)) == 0
    sd = np.zeros((8, 13), np.float32)
    O, A = np.empty((2, 8, 12), np.float32), np.empty((2, 8, 4), np.float32)
    R, D = np.empty((2, 8), np.float32), np.empty((2, 8), np.uint8)
    ret, le, fin = np.empty((1, 8)), np.empty((1, 8), np.int32), np.empty(8, np.int32)
    q = lambda x: x.ctypes.data_as(C.c_void_p)       # noqa: E731
    assert lib.qs_expert_rollout(h, 2, q(sd), 0.35, 0.0, q(O), q(A), q(R), q(D), None, None) == INVALID
    assert "device buffers" in lib.qs_last_error().decode()
    assert lib.qs_expert_evaluate(h, 1, 600, q(sd), 0.35, 0.0, q(ret), q(le), None, None, q(fin)) == INVALID
    assert "device buffers" in lib.qs_last_error().decode()
    obs = np.empty((8, 12), np.float32)
    assert lib.qs_reset(h, None, q(obs)) == 0 and np.isfinite(obs).all()    # still usable
    lib.qs_destroy(h)
