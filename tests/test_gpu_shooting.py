"""-m gpu: qs_shooting_plan (VecDockingEnv.shooting_plan, ShootingMPC).

1. The definition, bit for bit: every candidate's REWARD score equals the float64 sum of the float32 rewards that a second
   handle of N x paths envs, given the replicated state and the candidates' actions, returns from `horizon` qs_step calls,
   masked after its first done; winner, score, first action and sequence follow from those sums.
2. Against the float64 reference (tests/shooting_ref.py), both objectives, with the bounds the step API already asserts.
3. Read-only and reproducible.  4. Prefix property.  5. Independence of the mapping (N, launch path).  6. The closed loop.
7. Errors."""
import ctypes as C

import numpy as np
import pytest

import shooting_ref
from plan_cases import DT, HANDLES, HORIZONS, N, PATHS, SEED, in_flight_pair, make_handle, make_twin, slice_handle, twin_scores
from plan_cases import bits as _bits, rec_par as _rec_par, same as _same, snapshot as _snapshot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---------------------------------------------------------------- candidates and plans
_ACTS = {}


def _actions(k, n, paths, horizon, offset=0):
    """[n, paths, horizon, 4] candidate actions of envs gid = offset .. offset + n - 1 planned before step k; generated once
    for the largest (paths, horizon) and sliced (the prefix property of the keying, pinned in test_shooting_cpu.py)"""
    key = (k, n, offset)
    if key not in _ACTS:
        _ACTS[key] = np.stack([shooting_ref.actions_fast(SEED, offset + g, k, max(PATHS), max(HORIZONS)) for g in range(n)])
    return _ACTS[key][:, :paths, :horizon]


def _plan(env, horizon, paths, objective="reward"):
    out = env.shooting_plan(horizon, paths, objective, return_scores=True, return_sequence=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("env_id,integ,params", HANDLES)
def test_definition_bit_for_bit(qa, torch, env_id, integ, params):
    env = make_handle(qa, env_id, integ, params)
    k = env.step_counter
    st, _, _ = _rec_par(env)
    stopped_inside = 0
    for paths in PATHS:
        twin = make_twin(qa, env, env_id, integ, params, paths)
        for horizon in HORIZONS:
            acts = _actions(k, N, paths, horizon)
            want, stopped = twin_scores(torch, twin, st, acts, paths)
            stopped_inside += stopped
            got = _plan(env, horizon, paths)
            assert np.array_equal(_bits(got["scores"]), _bits(want)), (paths, horizon)
            win = shooting_ref.first_argmax(want)
            assert np.array_equal(got["best_index"], win.astype(np.int32)), (paths, horizon)
            assert np.array_equal(_bits(got["best_score"]), _bits(want[np.arange(N), win])), (paths, horizon)
            assert np.array_equal(_bits(got["sequence"]), _bits(acts[np.arange(N), win])), (paths, horizon)
            assert np.array_equal(_bits(got["actions"]), _bits(acts[np.arange(N), win, 0])), (paths, horizon)
        twin.close()
    assert stopped_inside > 0                                 # candidates did terminate inside a horizon
    assert env.step_counter == k
    env.close()


# ---------------------------------------------------------------- 2. against float64
# bounds, from what the project already asserts per step in __graft_entry__.smoke(): |reward - oracle| <= 1e-5 and
# |obs - oracle| <= 2e-5.  A REWARD score sums `horizon` rewards: <= horizon * 1e-5 per candidate, twice that between the
# chosen candidate and the best one.  A POSITION term is -(o0^2 + o1^2 + o2^2): an observation error e changes it by
# <= 2 r e + e^2 with r = |rel_pos|, so <= horizon * 2 r * 2e-5 per candidate.  Not tightened from what the kernel gives.
F64_CASES = [("docking-v0", "frozen", False, p, h) for p in PATHS for h in HORIZONS]
F64_CASES += [(k, g, q, 200, 20) for (k, g, q) in HANDLES if (k, g, q) != ("docking-v0", "frozen", False)]
F64_CASES += [("docking-v0", "rk4", False, 1000, 20), ("docking-v1", "rk4", True, 1000, 3), ("docking-v2", "rk4", True, 64, 1),
              ("docking-v2", "frozen", True, 1, 20), ("docking-v1", "frozen", True, 64, 3), ("docking-v0", "rk4", True, 1, 1)]
_worst = {"reward": 0.0, "position": 0.0, "reward_pick": 0.0, "position_pick": 0.0}


@pytest.mark.parametrize("env_id,integ,params,paths,horizon", F64_CASES)
def test_against_float64_reference(qa, torch, env_id, integ, params, paths, horizon):
    """the paths x horizon cross product on docking-v0 / frozen / nominal, every other (kind, integrator, params) handle at the
    reference's 200 x 20, and the other path counts and horizons spread over RK4 and per-env-parameter handles; every env
    counts.  The states are plan_cases.make_handle's "decisive" ones (see there); the definition test takes the knife-edge ones."""
    env = make_handle(qa, env_id, integ, params, provoke="decisive")
    k = env.step_counter
    _, rec, par = _rec_par(env)
    acts = _actions(k, N, paths, horizon)
    s_rew, s_pos, r = shooting_ref.plan_scores_both(rec, par, acts, kind=1 if env_id == "docking-v2" else 0, dt=DT,
                                                    integ=1 if integ == "rk4" else 0)
    assert r < 20.0
    rows = np.arange(N)
    for objective, ref, tol in (("reward", s_rew, 2 * horizon * 1e-5), ("position", s_pos, 2 * horizon * 2 * r * 2e-5)):
        got = _plan(env, horizon, paths, objective)
        dev = float(np.max(np.abs(got["scores"] - ref)))
        pick = float(np.max(ref.max(axis=1) - ref[rows, got["best_index"]]))
        _worst[objective] = max(_worst[objective], dev / (tol / 2))
        _worst[objective + "_pick"] = max(_worst[objective + "_pick"], pick / tol)
        print("%s %s params=%d paths=%d horizon=%d %s: max |score - f64| = %.3g (bound %.3g), f64 regret of the pick = %.3g "
              "(bound %.3g), r = %.3g; worst so far as fractions of the bounds: %s"
              % (env_id, integ, params, paths, horizon, objective, dev, tol / 2, pick, tol, r, _worst))
        assert np.all(ref[rows, got["best_index"]] >= ref.max(axis=1) - tol), objective
        assert dev <= tol / 2, objective
        assert np.array_equal(got["best_score"], got["scores"][rows, got["best_index"]])
    env.close()


# ---------------------------------------------------------------- 3. read-only, reproducible
@pytest.mark.parametrize("env_id,params,auto_reset", [("docking-v0", False, True), ("docking-v2", True, False), ("docking-v1", False, True)])
def test_read_only_and_reproducible(qa, torch, env_id, params, auto_reset):
    env = make_handle(qa, env_id, "frozen", params, auto_reset=auto_reset)
    twin = make_handle(qa, env_id, "frozen", params, auto_reset=auto_reset)
    before = _snapshot(env)
    assert _same(before, _snapshot(twin))
    p1 = _plan(env, 20, 200)
    q1 = _plan(env, 20, 200, "position")
    assert _same(before, _snapshot(env))                      # state, params, step counter
    p2 = _plan(env, 20, 200)
    q2 = _plan(env, 20, 200, "position")
    for key in p1:
        assert np.array_equal(_bits(p1[key]), _bits(p2[key])) and np.array_equal(_bits(q1[key]), _bits(q2[key])), key
    acts = env.random_actions(10, step0=100)
    for t in range(10):                                       # the twin never planned: the same next 10 steps
        oa, ra, da, _ = env.step(acts[t])
        ob, rb, db, _ = twin.step(acts[t])
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
        if t == 0:
            p3 = _plan(env, 20, 200)                          # k changed: other candidates
            assert not np.array_equal(p3["sequence"], p1["sequence"])
            assert np.array_equal(_bits(p3["sequence"][:, 0]), _bits(p3["actions"]))
    assert _same(_snapshot(env), _snapshot(twin))
    env.close(); twin.close()


# ---------------------------------------------------------------- 4. prefix property
@pytest.mark.parametrize("objective", ["reward", "position"])
def test_prefix_property_on_the_device(qa, torch, objective):
    env = make_handle(qa, "docking-v0", "rk4", True)
    p64, p200, p1000 = (_plan(env, 20, p, objective) for p in (64, 200, 1000))
    assert np.all(p1000["best_score"] >= p200["best_score"]) and np.all(p200["best_score"] >= p64["best_score"])
    assert np.array_equal(_bits(p1000["scores"][:, :200]), _bits(p200["scores"]))
    assert np.array_equal(_bits(p200["scores"][:, :64]), _bits(p64["scores"]))
    assert np.array_equal(p200["best_index"], shooting_ref.first_argmax(p200["scores"]).astype(np.int32))
    env.close()


# ---------------------------------------------------------------- 5. mapping independence
def test_one_env_handle_plans_like_the_same_env_of_a_large_handle(qa, torch):
    """N = 1 against N = 4096: env 1234 of the large handle and the single env of a handle with env_id_offset = 1234, the same
    state, parameters and step counter -- 1, 64, 200 and 1000 paths (blocks of 64, 64, 256 and 256 threads)"""
    g = 1234
    big = make_handle(qa, "docking-v0", "frozen", True, n=4096)
    one = slice_handle(qa, big, g, 1)
    for paths in PATHS:
        for objective in ("reward", "position"):
            a, b = _plan(big, 20, paths, objective), _plan(one, 20, paths, objective)
            for key in a:
                assert np.array_equal(_bits(a[key][g:g + 1]), _bits(b[key])), (paths, objective, key)
    # and equal-gid envs of two handles of different size: envs 0..95 of both
    small = slice_handle(qa, big, 0, N)
    a, b = _plan(big, 3, 1000), _plan(small, 3, 1000)
    for key in a:
        assert np.array_equal(_bits(a[key][:N]), _bits(b[key])), key
    big.close(); one.close(); small.close()


def test_private_queue_handle_plans_like_hip_stream_twin(qa, torch):
    """a private-queue handle with steps still in flight: drained first, then the same plan as a HIP-stream twin, and both step
    on alike"""
    a, b, last = in_flight_pair(qa, torch)
    pa, pb = _plan(a, 20, 200), _plan(b, 20, 200)
    for key in pa:
        assert np.array_equal(_bits(pa[key]), _bits(pb[key])), key
    assert a.step_counter == b.step_counter == 7
    oa, ra, _, _ = a.step(last)
    ob, rb, _, _ = b.step(last)
    assert torch.equal(oa, ob) and torch.equal(ra, rb)
    a.close(); b.close()


# ---------------------------------------------------------------- 6. closed loop
def test_closed_loop_is_plan_then_step(qa, torch):
    a = make_handle(qa, "docking-v0", "frozen", False, provoke=None)
    b = make_handle(qa, "docking-v0", "frozen", False, provoke=None)
    mpc = qa.ShootingMPC(a, horizon=10, paths=64)
    rew, done = mpc.run(5)
    assert rew.shape == (5, N) and done.shape == (5, N) and done.dtype == torch.bool
    for t in range(5):
        plan = b.shooting_plan(10, 64)
        _, r, d, _ = b.step(plan["actions"])
        assert torch.equal(r, rew[t]) and torch.equal(d, done[t]), t
    assert torch.equal(mpc.act(), b.shooting_plan(10, 64)["actions"])
    a.close(); b.close()


# ---------------------------------------------------------------- 7. errors
def test_errors(qa, torch):
    lib = qa._lib.load()
    INVALID = -1
    env = qa.VecDockingEnv("docking-v0", num_envs=8)
    env.reset()
    act = torch.empty((8, 4), device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr())                    # noqa: E731

    def call(h, horizon=20, paths=200, objective=0, actions=act):
        rc = lib.qs_shooting_plan(h, horizon, paths, objective, p(actions) if actions is not None else None, None, None, None, None)
        return rc, lib.qs_last_error().decode()

    for kw, word in ((dict(paths=0), "paths"), (dict(paths=65537), "paths"), (dict(horizon=0), "horizon"),
                     (dict(horizon=257), "horizon"), (dict(objective=2), "objective"), (dict(objective=-1), "objective"),
                     (dict(actions=None), "actions")):
        rc, msg = call(env._h, **kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
        with pytest.raises(qa.QuadsimError):
            qa._lib.check(rc, "qs_shooting_plan")
    rc, msg = call(env._h, paths=65536, horizon=1)            # the limits themselves are fine
    assert rc == 0, msg
    rc, msg = call(env._h, paths=1, horizon=256)
    assert rc == 0, msg
    misaligned = torch.empty(8 * 4 + 1, device=env.device)[1:].view(8, 4)
    rc, msg = call(env._h, actions=misaligned)
    assert rc == INVALID and "aligned" in msg
    env.step_counter = 1 << 36
    rc, msg = call(env._h)
    assert rc == INVALID and "step counter" in msg
    env.step_counter = (1 << 36) - 1
    rc, msg = call(env._h)
    assert rc == 0, msg
    env.close()

    hov = qa.VecDockingEnv("hovering-v0", num_envs=8)
    hov.reset()
    with pytest.raises(qa.QuadsimError, match="docking envs only"):
        hov.shooting_plan()
    hov.close()

    cfg = qa._lib.default_config()
    cfg.kind, cfg.num_envs, cfg.io_space, cfg.auto_reset = qa._lib.KIND_V0, 8, qa._lib.IO_HOST, 1
    h = C.c_void_p()
    assert lib.qs_create(C.byref(cfg), C.byref(h)) == 0
    host = np.empty((8, 4), np.float32)
    assert lib.qs_shooting_plan(h, 20, 200, 0, host.ctypes.data_as(C.c_void_p), None, None, None, None) == INVALID
    assert "device buffers" in lib.qs_last_error().decode()
    with pytest.raises(qa.QuadsimError):
        qa._lib.check(INVALID, "qs_shooting_plan")
    obs = np.empty((8, 12), np.float32)
    assert lib.qs_reset(h, None, obs.ctypes.data_as(C.c_void_p)) == 0 and np.isfinite(obs).all()
    lib.qs_destroy(h)


def test_global_env_ids_have_48_bits(qa, torch):
    """the planner's Philox subsequence is (5 << 48) | gid: a handle whose last env has the id 2^48 - 1 is accepted and plans
    what the reference draws for it; one env more is refused by qs_create and by VecDockingEnv"""
    lib = qa._lib.load()
    n, top = 8, 1 << 48
    env = qa.VecDockingEnv("docking-v0", num_envs=n, seed=SEED, env_id_offset=top - n)
    env.reset()
    got = _plan(env, 3, 64)
    acts = np.stack([shooting_ref.actions_fast(SEED, top - n + g, env.step_counter, 64, 3) for g in range(n)])
    assert np.array_equal(_bits(got["sequence"]), _bits(acts[np.arange(n), got["best_index"]]))
    env.close()
    with pytest.raises(ValueError, match="48 bits"):
        qa.VecDockingEnv("docking-v0", num_envs=n, env_id_offset=top - n + 1)
    cfg = qa._lib.default_config()
    cfg.kind, cfg.num_envs = qa._lib.KIND_V0, n
    for offset, rc_want in ((top - n + 1, -1), (top, -1), ((1 << 64) - 1, -1), (top - n, 0)):
        cfg.env_id_offset = offset
        h = C.c_void_p()
        assert lib.qs_create(C.byref(cfg), C.byref(h)) == rc_want, offset
        if rc_want:
            assert "48 bits" in lib.qs_last_error().decode() and not h.value
            with pytest.raises(qa.QuadsimError):
                qa._lib.check(rc_want, "qs_create")
    lib.qs_destroy(h)
