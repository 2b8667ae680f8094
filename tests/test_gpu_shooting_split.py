"""-m gpu: qs_shooting_plan_split (shooting_plan(..., splits=S), ShootingMPC(..., splits=S), DockingEnv.shooting_plan).

test_gpu_shooting.py pins qs_shooting_plan to the step API bit for bit; the winner of a plan is defined by a total order, so
every partition of the candidates must give qs_shooting_plan's bits, and that is all this file compares against.
1. Bit identity over handles x paths x horizon x objective x splits.  2. Ties.  3. Every score NaN.  4. One env, 65 536 paths.
5. Independence of the mapping.  6. The workspace.  7. Host handles (the single-env shims).  8. Errors.  9. The closed loop."""
import ctypes as C

import numpy as np
import pytest

from plan_cases import HANDLES, HORIZONS, N, PATHS, in_flight_pair, make_handle, same, same_bits, slice_handle, snapshot

pytestmark = pytest.mark.gpu

SPLITS = (1, 2, 3, 7, 64, 256, "auto")
KEYS = ("actions", "best_score", "best_index", "sequence", "scores")


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _plan(env, horizon, paths, objective="reward", splits=None):
    out = env.shooting_plan(horizon, paths, objective, return_scores=True, return_sequence=True, splits=splits)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same_plan(got, want, what):
    assert sorted(got) == sorted(want) == sorted(KEYS), what
    for key in KEYS:
        assert got[key].dtype == want[key].dtype and same_bits(got[key], want[key]), (what, key)


# ---------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("env_id,integ,params", HANDLES)
def test_bit_identity_with_the_unsplit_plan(qa, torch, env_id, integ, params):
    """paths 1 and 64: one part with work; 200 at S = 64 and 1000 at S = 256: empty trailing parts; S = 3 and 7: ragged chunks;
    1000 at S = 2: a lane loop inside a part.  provoke="all": time-outs, the floor and docked envs inside the horizon"""
    env = make_handle(qa, env_id, integ, params)
    before = snapshot(env)
    cases = 0
    for paths in PATHS:
        for horizon in HORIZONS:
            for objective in ("reward", "position"):
                want = _plan(env, horizon, paths, objective)
                for s in SPLITS:
                    if s != "auto" and s > paths:
                        continue
                    _assert_same_plan(_plan(env, horizon, paths, objective, s), want, (paths, horizon, objective, s))
                    cases += 1
    assert cases == 3 * 2 * (2 + 6 + 6 + 7)                  # S <= paths: 1 | 1..64 | 1..64 | all, each with "auto"
    assert same(before, snapshot(env))                        # state, parameters, step counter
    env.close()


# ---------------------------------------------------------------- 2. ties
@pytest.mark.parametrize("horizon", [1, 2])
def test_ties_go_to_the_lowest_index(qa, torch, horizon):
    """objective "position" with horizon < 3: an action acts with one step's delay, so every candidate of an env scores the
    same and candidate 0 wins in every partition"""
    env = make_handle(qa, "docking-v0", "frozen", False)
    want = _plan(env, horizon, 1000, "position")
    assert np.all(want["scores"] == want["scores"][:, :1])
    for s in SPLITS:
        got = _plan(env, horizon, 1000, "position", s)
        assert np.all(got["best_index"] == 0), s
        _assert_same_plan(got, want, s)
    assert same_bits(want["actions"], _plan(env, horizon, 1, "position")["actions"])      # candidate 0's
    env.close()


# ---------------------------------------------------------------- 3. every score NaN
def test_all_nan_scores_give_index_zero_and_minus_infinity(qa, torch):
    env = make_handle(qa, "docking-v0", "frozen", False)
    c = env.get_state()["chaser"]
    bad = np.arange(N) % 5 == 0
    c[bad, 0:3] = np.nan
    env.set_state(chaser=c)
    want = _plan(env, 3, 200)
    assert np.isnan(want["scores"][bad]).all() and np.isfinite(want["scores"][~bad]).all()
    for s in (1, 7, 64):
        got = _plan(env, 3, 200, "reward", s)
        assert np.all(got["best_index"][bad] == 0) and np.all(got["best_score"][bad] == -np.inf), s
        _assert_same_plan(got, want, s)
    env.close()


# ---------------------------------------------------------------- 4. one env, many paths
def test_one_env_with_65536_paths(qa, torch):
    env = make_handle(qa, "docking-v0", "rk4", True, n=1)
    auto = qa.plan_splits(env, 65536)
    assert 1 < auto <= 1024
    want = _plan(env, 3, 65536)
    for s in ("auto", 256, 1024):
        _assert_same_plan(_plan(env, 3, 65536, "reward", s), want, s)
    env.close()
    big = qa.VecDockingEnv("docking-v0", num_envs=4096)
    assert qa.plan_splits(big, 65536) == 1 and qa.plan_splits(big, 1) == 1
    big.close()


# ---------------------------------------------------------------- 5. mapping independence
def test_env_of_a_handle_plans_like_a_one_env_handle(qa, torch):
    big = make_handle(qa, "docking-v0", "frozen", True)
    one = slice_handle(qa, big, 37, 1)
    a, b = _plan(big, 20, 200, "reward", 7), _plan(one, 20, 200, "reward", 7)
    for key in KEYS:
        assert same_bits(a[key][37:38], b[key]), key
    big.close(); one.close()


def test_private_queue_handle_is_drained_and_agrees_with_its_twin(qa, torch):
    a, b, last = in_flight_pair(qa, torch)
    _assert_same_plan(_plan(b, 20, 200, "reward", 7), _plan(a, 20, 200, "reward", 7), "queues")
    assert a.step_counter == b.step_counter == 7
    oa, ra, _, _ = a.step(last)
    ob, rb, _, _ = b.step(last)
    assert torch.equal(oa, ob) and torch.equal(ra, rb)
    a.close(); b.close()


# ---------------------------------------------------------------- 6. the workspace
def test_workspace_grows_is_reused_and_belongs_to_its_handle(qa, torch):
    a = make_handle(qa, "docking-v0", "frozen", False)
    b = make_handle(qa, "docking-v2", "rk4", True)
    want_a, want_b = _plan(a, 3, 1000), _plan(b, 3, 1000)
    for s in (2, 256, 2):
        got_a = a.shooting_plan(3, 1000, return_scores=True, return_sequence=True, splits=s)      # both in flight together
        got_b = b.shooting_plan(3, 1000, return_scores=True, return_sequence=True, splits=s)
        _assert_same_plan({k: v.cpu().numpy() for k, v in got_a.items()}, want_a, ("a", s))
        _assert_same_plan({k: v.cpu().numpy() for k, v in got_b.items()}, want_b, ("b", s))
    a.close()
    _assert_same_plan(_plan(b, 3, 1000, "reward", 256), want_b, "after the other handle is gone")
    b.close()


# ---------------------------------------------------------------- 7. host handles
def _shim_state(shim):
    """the whole state and the step counter of a single-env shim, through its host handle"""
    lib = shim._lib
    st = dict(chaser=np.zeros((1, 13), np.float32), target=np.zeros((1, 13), np.float32), u_prev=np.zeros((1, 8), np.float32),
              qdes=np.zeros((1, 4), np.float32), last_shaping=np.zeros(1, np.float32), t=np.zeros(1, np.float32))
    assert lib.qs_get_state(shim._h, *[v.ctypes.data_as(C.c_void_p) for v in st.values()]) == 0
    k = C.c_uint64(0)
    assert lib.qs_get_step_counter(shim._h, C.byref(k)) == 0
    return st, int(k.value)


@pytest.mark.parametrize("cls,env_id", [("DockingEnv", "docking-v0"), ("MovingDockingEnv", "docking-v2")])
def test_single_env_shim_plans_through_the_host_path(qa, torch, cls, env_id):
    shim = getattr(qa, cls)()
    shim.reset()
    rng = np.random.default_rng(3)
    for _ in range(3):
        shim.step(rng.uniform(-1, 1, 4))
    st, k = _shim_state(shim)
    assert k == 3
    dev = qa.VecDockingEnv(env_id, num_envs=1, seed=0, auto_reset=False)          # the shim's seed and env id
    dev.set_state(**st)
    dev.step_counter = k
    want = _plan(dev, 3, 200)
    for s in (1, 7):
        got = shim.shooting_plan(horizon=3, paths=200, splits=s, return_scores=True, return_sequence=True)
        assert isinstance(got["actions"], np.ndarray) and got["actions"].shape == (4,) and got["actions"].dtype == np.float32
        assert got["sequence"].shape == (3, 4) and got["scores"].shape == (200,) and got["scores"].dtype == np.float64
        assert same_bits(got["actions"], want["actions"][0]) and same_bits(got["sequence"], want["sequence"][0]), s
        assert same_bits(got["scores"], want["scores"][0]), s
        assert same_bits(np.array([got["best_score"]]), want["best_score"]) and got["best_index"] == int(want["best_index"][0]), s
    plain = shim.shooting_plan(horizon=3, paths=200)          # splits="auto", nothing optional
    assert sorted(plain) == ["actions", "best_index", "best_score"] and same_bits(plain["actions"], want["actions"][0])
    st2, k2 = _shim_state(shim)
    assert k2 == k and all(np.array_equal(st[key], st2[key]) for key in st)
    obs, rew, done, _ = shim.step(got["actions"])
    o2, r2, d2, _ = dev.step(torch.from_numpy(want["actions"]).to(dev.device))
    assert np.array_equal(obs.astype(np.float32), o2[0].cpu().numpy()) and np.float32(rew) == r2[0].item() and done == bool(d2[0])
    shim.close(); dev.close()


# ---------------------------------------------------------------- 8. errors
def test_errors_leave_the_handle_usable(qa, torch):
    lib = qa._lib.load()
    INVALID = -1
    env = make_handle(qa, "docking-v0", "frozen", False, n=8)
    act = torch.empty((8, 4), device=env.device)

    def call(h, splits, paths=200, actions=act):
        rc = lib.qs_shooting_plan_split(h, 20, paths, 0, splits, C.c_void_p(actions.data_ptr()) if actions is not None else None,
                                        None, None, None, None)
        return rc, lib.qs_last_error().decode()

    for kw, word in ((dict(splits=-1), "splits must be"), (dict(splits=201), "[1, 200]"), (dict(splits=65, paths=64), "[1, 64]"),
                     (dict(splits=1025, paths=4096), "[1, 1024]"), (dict(splits=2, actions=None), "actions is required"),
                     (dict(splits=2, paths=0), "paths must be"), (dict(splits=2, paths=65537), "paths must be")):
        rc, msg = call(env._h, **kw)
        assert rc == INVALID and word in msg and "qs_shooting_plan_split" in msg, (kw, rc, msg)
        rc, msg = call(env._h, 7)                             # the next legal call on the same handle succeeds
        assert rc == 0, msg
    _assert_same_plan(_plan(env, 20, 200, "reward", 7), _plan(env, 20, 200), "after the errors")
    s = C.c_int32(-5)
    assert lib.qs_shooting_plan_splits(env._h, 0, C.byref(s)) == INVALID and "paths must be" in lib.qs_last_error().decode()
    assert lib.qs_shooting_plan_splits(env._h, 200, None) == INVALID and s.value == -5
    env.close()

    hov = qa.VecDockingEnv("hovering-v0", num_envs=8)
    hov.reset()
    rc, msg = call(hov._h, 2)
    assert rc == INVALID and "docking envs only" in msg
    with pytest.raises(qa.QuadsimError, match="docking envs only"):
        hov.shooting_plan(splits=2)
    hov.close()


# ---------------------------------------------------------------- 9. closed loop
def test_closed_loop_with_splits_is_the_closed_loop_without(qa, torch):
    a = make_handle(qa, "docking-v0", "frozen", False, provoke=None)
    b = make_handle(qa, "docking-v0", "frozen", False, provoke=None)
    ra, da = qa.ShootingMPC(a, 20, 200, splits=7).run(5)
    rb, db = qa.ShootingMPC(b, 20, 200).run(5)
    assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and torch.equal(da, db)
    assert same(snapshot(a), snapshot(b))
    a.close(); b.close()
