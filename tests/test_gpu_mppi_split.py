"""-m gpu: qs_mppi_plan_split (mppi_plan(..., splits=S), MPPI(..., splits=S), DockingEnv.mppi_plan).

test_gpu_mppi.py pins qs_mppi_plan; here a partition of one env's candidates over S workgroups is pinned to it and to the
step API.  1. S = 1 is qs_mppi_plan.  2. What a partition cannot change.  3. Every iteration's scores bit for bit on a twin
handle.  4. The update against float64.  5. More than 4096 paths.  6. NaN.  7. Independence of the mapping.  8. The
workspace.  9. Host handles.  10. The closed loop.  11. Errors."""
import ctypes as C

import numpy as np
import pytest

import mppi_ref
from plan_cases import HANDLES, HORIZONS, N, PATHS, in_flight_pair, make_handle, make_twin, slice_handle, twin_scores
from plan_cases import rec_par, same, same_bits, snapshot

pytestmark = pytest.mark.gpu

SUBSET = [("docking-v0", "frozen", False), ("docking-v1", "rk4", True), ("docking-v2", "frozen", True), ("docking-v0", "rk4", False)]
LAM, SIGMA = 0.5, 0.4
# Both planners round one float64 quotient to float32 once.  The quotients differ by the order of two float64 sums of at most
# 65 536 terms with weights in [0, 1] and values in [-1, 1] (relative ~65536 * 2^-53 ~ 1e-11), so the two float32 results, in
# [-1, 1], are at most one rounding step apart: 2^-24.
ORDER_TOL = 2.0 ** -24
# test_gpu_mppi.py's UPDATE_TOL and its derivation, which holds for any summation order
UPDATE_TOL = 2.0 * 2.0 ** -24


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _plan(env, horizon, paths, iterations=1, objective="reward", lam=LAM, sigma=SIGMA, **kw):
    kw.setdefault("return_scores", True)
    kw.setdefault("return_trace", True)
    kw.setdefault("return_candidates", True)
    out = env.mppi_plan(horizon, paths, iterations, objective, lam, sigma, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same_plan(got, want, what):
    assert sorted(got) == sorted(want), what
    for key in want:
        assert got[key].dtype == want[key].dtype and same_bits(got[key], want[key]), (what, key)


# ---------------------------------------------------------------- 1. S = 1 is qs_mppi_plan
@pytest.mark.parametrize("env_id,integ,params", SUBSET)
def test_one_part_is_the_unsplit_plan(qa, torch, env_id, integ, params):
    env = make_handle(qa, env_id, integ, params)
    gen = torch.Generator(device="cpu").manual_seed(5)
    for paths in PATHS:
        for horizon in HORIZONS:
            for iters in (1, 3):
                noise = torch.randn((iters, paths, horizon, 4), generator=gen).to(env.device)
                nominal = (torch.rand((N, horizon, 4), generator=gen) * 2.4 - 1.2).to(env.device)
                for kw in (dict(), dict(noise=noise, nominal=nominal, shift=True), dict(nominal=nominal)):
                    want = _plan(env, horizon, paths, iters, **kw)
                    _assert_same_plan(_plan(env, horizon, paths, iters, splits=1, **kw), want, (paths, horizon, iters, sorted(kw)))
    env.close()


# ---------------------------------------------------------------- 2. what a partition cannot change
@pytest.mark.parametrize("env_id,integ,params", SUBSET)
def test_partition_keeps_first_scores_candidates_and_the_update_to_one_rounding(qa, torch, env_id, integ, params):
    """paths 1: one part with work; 3 and 7: ragged chunks; 200 at S = 64: chunk 4, 50 parts with work and 14 empty; 1000 at
    S = 2 or 3: a lane loop inside a part"""
    env = make_handle(qa, env_id, integ, params)
    gen = torch.Generator(device="cpu").manual_seed(9)
    cases, worst = 0, 0.0
    for paths in PATHS:
        for horizon in HORIZONS:
            nominal = (torch.rand((N, horizon, 4), generator=gen) - 0.5).to(env.device)
            want = _plan(env, horizon, paths, 1, nominal=nominal, shift=True)
            want3 = _plan(env, horizon, paths, 3, nominal=nominal, shift=True, return_candidates=False) if horizon == 20 else None
            for s in (2, 3, 7, 64, "auto"):
                if s != "auto" and s > paths:
                    continue
                key = (paths, horizon, s)
                got = _plan(env, horizon, paths, 1, nominal=nominal, shift=True, splits=s)
                assert same_bits(got["trace"][:, 0], want["trace"][:, 0]), key
                assert same_bits(got["scores"][:, 0], want["scores"][:, 0]), key
                assert same_bits(got["candidates"], want["candidates"]), key
                assert same_bits(got["best_score"], want["best_score"]), key
                err = float(np.max(np.abs(got["trace"][:, 1].astype(np.float64) - want["trace"][:, 1].astype(np.float64))))
                worst = max(worst, err)
                assert err <= ORDER_TOL, (key, err)
                if want3 is not None:
                    got3 = _plan(env, horizon, paths, 3, nominal=nominal, shift=True, splits=s, return_candidates=False)
                    assert same_bits(got3["trace"][:, 0], want3["trace"][:, 0]) and same_bits(got3["scores"][:, 0], want3["scores"][:, 0]), key
                    assert same_bits(got3["trace"][:, 1], got["trace"][:, 1]), key
                cases += 1
    assert cases == 3 * (1 + 5 + 5 + 5)                       # S <= paths: auto alone | all five | all five | all five
    print("%s %s params=%d: worst |split - unsplit| after one update = %.3g (bound %.3g)" % (env_id, integ, params, worst, ORDER_TOL))
    env.close()


# ---------------------------------------------------------------- 3. every iteration's scores, bit for bit
SCORE_CASES = ((64, 1, 7), (200, 20, 3), (1000, 3, 7), (1000, 20, 3))      # paths, horizon, S


def _scores_on_twin(qa, torch, env, env_id, integ, params, cases, iters):
    """test_gpu_mppi.py's recipe with `splits`: the device's own candidates of iteration j, stepped by qs_step on the twin, give
    scores[:, j - 1]; fewer iterations are a prefix -> the number of candidates that stopped inside a horizon"""
    st, _, _ = rec_par(env)
    n = env.num_envs
    stopped_inside = 0
    for paths, horizon, s in cases:
        twin = make_twin(qa, env, env_id, integ, params, paths)
        full = None
        for j in range(iters, 0, -1):
            got = _plan(env, horizon, paths, j, splits=s)
            if full is None:
                full = got
            key = (paths, horizon, s, j)
            assert same_bits(got["scores"], full["scores"][:, :j]), key                  # iteration prefix
            assert same_bits(got["trace"], full["trace"][:, :j + 1]), key
            acts = got["candidates"]
            assert acts.shape == (n, paths, horizon, 4) and np.all(np.abs(acts) <= 1.0)
            want, stopped = twin_scores(torch, twin, st, acts, paths)
            stopped_inside += stopped
            assert same_bits(got["scores"][:, j - 1], want), key
            assert same_bits(got["best_score"], want.max(axis=1)), key
            assert same_bits(got["best_score"], got["scores"][:, -1].max(axis=1)), key
        twin.close()
    return stopped_inside


@pytest.mark.parametrize("env_id,integ,params", HANDLES)
def test_scores_bit_for_bit_and_iteration_prefix(qa, torch, env_id, integ, params):
    env = make_handle(qa, env_id, integ, params)
    k = env.step_counter
    cases = SCORE_CASES + (((1000, 20, "auto"),) if (env_id, integ, params) == HANDLES[0] else ())
    assert _scores_on_twin(qa, torch, env, env_id, integ, params, cases, 3) > 0      # candidates did terminate inside a horizon
    assert env.step_counter == k
    env.close()


# ---------------------------------------------------------------- 4. the update, closed on the device's own outputs
def _assert_update(got, it, lam, key):
    want = mppi_ref.update64(got["scores"][:, it], got["candidates"], lam, got["trace"][:, it])
    err = float(np.max(np.abs(got["trace"][:, it + 1].astype(np.float64) - want)))
    assert err <= UPDATE_TOL, (key, it, err)
    assert same_bits(got["nominal"], got["trace"][:, -1]) and same_bits(got["actions"], got["nominal"][:, 0]), key
    return err


@pytest.mark.parametrize("env_id,integ,params", SUBSET)
def test_update_against_float64_on_device_outputs(qa, torch, env_id, integ, params):
    env = make_handle(qa, env_id, integ, params)
    gen = torch.Generator(device="cpu").manual_seed(11)
    worst = 0.0
    for objective, lam in (("reward", 0.05), ("position", 2.0)):
        for paths, horizon in ((200, 3), (200, 20), (1000, 20)):
            noise = torch.randn((3, paths, horizon, 4), generator=gen).to(env.device) if paths == 200 else None
            for s in (2, 7, 64):
                for it in range(3):
                    got = _plan(env, horizon, paths, it + 1, objective, lam=lam, splits=s,
                                noise=None if noise is None else noise[:it + 1].contiguous())
                    worst = max(worst, _assert_update(got, it, lam, (objective, paths, horizon, s)))
    print("%s %s params=%d: worst |update - f64| = %.3g (bound %.3g)" % (env_id, integ, params, worst, UPDATE_TOL))
    env.close()


# ---------------------------------------------------------------- 5. more than 4096 paths
@pytest.mark.parametrize("paths,splits", [(16384, 16), (16384, "auto"), (65536, 1024), (65536, "auto")])
def test_one_env_with_more_paths_than_one_workgroup_holds(qa, torch, paths, splits):
    """16 384 at S = 16: chunk 1024, a lane loop; the twin has `paths` envs"""
    env = make_handle(qa, "docking-v0", "rk4", True, n=1)
    assert qa.plan_splits(env, paths) >= 2
    _scores_on_twin(qa, torch, env, "docking-v0", "rk4", True, ((paths, 3, splits),), 2)
    for it in range(2):
        _assert_update(_plan(env, 3, paths, it + 1, lam=0.05, splits=splits), it, 0.05, (paths, splits))
    with pytest.raises(ValueError):
        env.mppi_plan(3, paths, 2, splits=1)
    act, nom = torch.empty((1, 4), device=env.device), torch.empty((1, 3, 4), device=env.device)
    rc = env._lib.qs_mppi_plan_split(env._h, 3, paths, 2, 0, LAM, SIGMA, 0, 1, None, None, C.c_void_p(act.data_ptr()),
                                     C.c_void_p(nom.data_ptr()), None, None, None, None)
    assert rc == -1 and "4096" in env._lib.qs_last_error().decode()
    env.close()


# ---------------------------------------------------------------- 6. NaN
def test_nan_env_keeps_its_nominal_and_leaves_the_others_alone(qa, torch):
    bad, good = make_handle(qa, "docking-v0", "frozen", False), make_handle(qa, "docking-v0", "frozen", False)
    c = bad.get_state()["chaser"]
    c[5, 0:3] = np.nan
    bad.set_state(chaser=c)
    gen = torch.Generator(device="cpu").manual_seed(21)
    nominal = (torch.rand((N, 20, 4), generator=gen) - 0.5).to(bad.device)
    shifted = nominal.cpu().numpy()[:, np.minimum(np.arange(20) + 1, 19)]
    others = np.arange(N) != 5
    for s in (1, 3):
        got = _plan(bad, 20, 200, 3, nominal=nominal, shift=True, splits=s)
        want = _plan(good, 20, 200, 3, nominal=nominal, shift=True, splits=s)
        assert np.isnan(got["scores"][5]).all() and np.isfinite(got["scores"][others]).all(), s
        assert same_bits(got["nominal"][5], shifted[5]) and got["best_score"][5] == -np.inf, s
        for key in want:
            assert same_bits(got[key][others], want[key][others]), (s, key)
    bad.close(); good.close()


# ---------------------------------------------------------------- 7. mapping independence at a fixed S
MAPPING_CASES = ((7, 1000), (64, 200))                         # S, paths


def test_env_of_a_large_handle_plans_like_a_one_env_handle_and_aliased_nominal(qa, torch):
    g = 1234
    big = make_handle(qa, "docking-v0", "frozen", True, n=4096)
    one = slice_handle(qa, big, g, 1)
    gen = torch.Generator(device="cpu").manual_seed(17)
    for s, paths in MAPPING_CASES:
        nominal = (torch.rand((4096, 20, 4), generator=gen) - 0.5).to(big.device)
        a = _plan(big, 20, paths, 3, nominal=nominal, shift=True, splits=s, return_candidates=False)
        b = _plan(one, 20, paths, 3, nominal=nominal[g:g + 1].contiguous(), shift=True, splits=s, return_candidates=False)
        for key in a:
            assert same_bits(a[key][g:g + 1], b[key]), (s, paths, key)
        # aliased through the raw entry point: nominal_in is nominal_out
        buf, act = nominal.clone(), torch.empty((4096, 4), device=big.device)
        big._use_current_stream()
        big._inputs_ready()
        qa._lib.check(big._lib.qs_mppi_plan_split(big._h, 20, paths, 3, 0, LAM, SIGMA, 1, s, C.c_void_p(buf.data_ptr()), None,
                                                  C.c_void_p(act.data_ptr()), C.c_void_p(buf.data_ptr()), None, None, None, None),
                      "qs_mppi_plan_split")
        big._outputs_ready()
        torch.cuda.synchronize()
        assert same_bits(buf.cpu().numpy(), a["nominal"]) and same_bits(act.cpu().numpy(), a["actions"]), (s, paths)
    big.close(); one.close()


def test_private_queue_handle_plans_like_hip_stream_twin(qa, torch):
    a, b, last = in_flight_pair(qa, torch)
    for s, paths in MAPPING_CASES:
        _assert_same_plan(_plan(b, 20, paths, 3, splits=s, return_candidates=False),
                          _plan(a, 20, paths, 3, splits=s, return_candidates=False), (s, paths))
    assert a.step_counter == b.step_counter == 7
    oa, ra, _, _ = a.step(last)
    ob, rb, _, _ = b.step(last)
    assert torch.equal(oa, ob) and torch.equal(ra, rb)
    a.close(); b.close()


def test_read_only_and_reproducible(qa, torch):
    env = make_handle(qa, "docking-v2", "rk4", True)
    before = snapshot(env)
    for s, paths in MAPPING_CASES:
        p1 = _plan(env, 20, paths, 3, splits=s)
        assert same(before, snapshot(env))
        _assert_same_plan(_plan(env, 20, paths, 3, splits=s), p1, (s, paths))
    env.close()


# ---------------------------------------------------------------- 8. the workspace
def test_workspace_grows_is_reused_and_belongs_to_its_handle(qa, torch):
    a = make_handle(qa, "docking-v0", "frozen", False)
    b = make_handle(qa, "docking-v2", "rk4", True)
    want = {(h, s): _plan(env, 3, 1000, 2, splits=s) for h, env in (("a", a), ("b", b)) for s in (2, 256)}
    for s in (2, 256, 2, 256):                                # grow, then reuse with fewer parts and with more again
        kw = dict(return_scores=True, return_trace=True, return_candidates=True, splits=s)
        got_a = a.mppi_plan(3, 1000, 2, "reward", LAM, SIGMA, **kw)      # both in flight together
        got_b = b.mppi_plan(3, 1000, 2, "reward", LAM, SIGMA, **kw)
        _assert_same_plan({k: v.cpu().numpy() for k, v in got_a.items()}, want["a", s], ("a", s))
        _assert_same_plan({k: v.cpu().numpy() for k, v in got_b.items()}, want["b", s], ("b", s))
    fresh = make_handle(qa, "docking-v0", "frozen", False)   # its first split call is the large one
    _assert_same_plan(_plan(fresh, 3, 1000, 2, splits=256), want["a", 256], "fresh")
    _assert_same_plan(_plan(fresh, 3, 1000, 2, splits=2), want["a", 2], "fresh")
    a.close(); fresh.close()
    _assert_same_plan(_plan(b, 3, 1000, 2, splits=256), want["b", 256], "after the other handles are gone")
    b.close()


def test_one_workspace_serves_both_planners_on_one_handle(qa, torch):
    """Shooting and MPPI split plans share the handle's one workspace: issued back to back on one handle with nothing read back
    in between -- shooting S = 2, MPPI S = 256 (grows the buffer behind shooting's kernels), shooting S = 256, MPPI S = 2,
    shooting S = 2 -- every output of every call has the bits a fresh twin handle gives for that call alone.  1000 paths:
    ragged and empty parts at S = 256, a lane loop at S = 2."""
    every = dict(shooting=dict(return_scores=True, return_sequence=True),
                 mppi=dict(return_scores=True, return_trace=True, return_candidates=True))

    def issue(env, family, s):
        if family == "shooting":
            return env.shooting_plan(3, 1000, "reward", splits=s, **every[family])
        return env.mppi_plan(3, 1000, 2, "reward", LAM, SIGMA, splits=s, **every[family])

    host = lambda out: {k: v.cpu().numpy() for k, v in out.items()}      # noqa: E731
    twin = make_handle(qa, "docking-v2", "rk4", True)
    want = {(f, s): host(issue(twin, f, s)) for f in ("shooting", "mppi") for s in (2, 256)}
    twin.close()
    env = make_handle(qa, "docking-v2", "rk4", True)
    sequence = [("shooting", 2), ("mppi", 256), ("shooting", 256), ("mppi", 2), ("shooting", 2)]
    got = [issue(env, f, s) for f, s in sequence]             # nothing is read back before the last call is issued
    for i, (key, out) in enumerate(zip(sequence, got)):
        _assert_same_plan(host(out), want[key], (i,) + key)
    env.close()


# ---------------------------------------------------------------- 9. host handles
def _shim_state(shim):
    """the whole state and the step counter of a single-env shim, through its host handle"""
    lib = shim._lib
    st = dict(chaser=np.zeros((1, 13), np.float32), target=np.zeros((1, 13), np.float32), u_prev=np.zeros((1, 8), np.float32),
              qdes=np.zeros((1, 4), np.float32), last_shaping=np.zeros(1, np.float32), t=np.zeros(1, np.float32))
    assert lib.qs_get_state(shim._h, *[v.ctypes.data_as(C.c_void_p) for v in st.values()]) == 0
    k = C.c_uint64(0)
    assert lib.qs_get_step_counter(shim._h, C.byref(k)) == 0
    return st, int(k.value)


@pytest.mark.parametrize("cls,env_id", [("DockingEnv", "docking-v0"), ("MovingDockingEnv", "docking-v2"),
                                        ("ImitatingDockingEnv", "docking-v1")])
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
    carried = rng.uniform(-0.5, 0.5, (3, 4)).astype(np.float32)
    dev_nominal = torch.from_numpy(carried[None]).to(dev.device)
    for s in (1, 4, "auto"):
        want = _plan(dev, 3, 200, 2, nominal=dev_nominal, shift=True, splits=s)
        got = shim.mppi_plan(horizon=3, paths=200, iterations=2, lam=LAM, sigma=SIGMA, nominal=carried, shift=True, splits=s,
                             return_scores=True, return_trace=True, return_candidates=True)
        assert isinstance(got["actions"], np.ndarray) and got["actions"].shape == (4,) and got["actions"].dtype == np.float32
        assert got["nominal"].shape == (3, 4) and got["scores"].shape == (2, 200) and got["scores"].dtype == np.float64
        assert got["trace"].shape == (3, 3, 4) and got["candidates"].shape == (200, 3, 4)
        for key in ("actions", "nominal", "scores", "trace", "candidates"):
            assert same_bits(got[key], want[key][0]), (s, key)
        assert same_bits(np.array([got["best_score"]]), want["best_score"]), s
    plain = shim.mppi_plan(horizon=3, paths=200, lam=LAM, sigma=SIGMA, nominal=carried, shift=True)      # "auto", nothing optional
    assert sorted(plain) == ["actions", "best_score", "nominal"] and same_bits(plain["actions"], want["actions"][0])
    st2, k2 = _shim_state(shim)
    assert k2 == k and all(np.array_equal(st[key], st2[key]) for key in st)
    # the closed loop: plan; step, the nominal carried with shift=True, on both
    nom_h, nom_d = None, None
    for t in range(5):
        ph = shim.mppi_plan(horizon=3, paths=200, iterations=2, lam=LAM, sigma=SIGMA, nominal=nom_h, shift=nom_h is not None, splits=4)
        pd = dev.mppi_plan(3, 200, 2, "reward", LAM, SIGMA, nominal=nom_d, shift=nom_d is not None, splits=4)
        assert same_bits(ph["nominal"], pd["nominal"][0].cpu().numpy()), t
        obs, rew, done, _ = shim.step(ph["actions"])
        o2, r2, d2, _ = dev.step(pd["actions"])
        assert np.array_equal(obs.astype(np.float32), o2[0].cpu().numpy()) and np.float32(rew) == r2[0].item() and done == bool(d2[0]), t
        nom_h, nom_d = ph["nominal"], pd["nominal"]
    shim.close(); dev.close()


# ---------------------------------------------------------------- 10. closed loop
def test_closed_loop_is_plan_step_and_masked_zeroing(qa, torch):
    def make():
        env = make_handle(qa, "docking-v0", "frozen", False, provoke=None)
        t0 = env.get_state()["t"].copy()
        t0[5] = 595.0                                         # times out inside the 8 steps
        env.set_state(t=t0)
        return env
    a, b = make(), make()
    ctl = qa.MPPI(a, horizon=10, paths=64, iterations=2, lam=LAM, sigma=SIGMA, splits=3)
    rew, done = ctl.run(8)
    assert rew.shape == (8, N) and done.shape == (8, N) and done.dtype == torch.bool
    assert bool(done[:, 5].any()) and not bool(done.all())
    nominal = None
    for t in range(8):
        plan = b.mppi_plan(10, 64, 2, "reward", LAM, SIGMA, nominal=nominal, shift=nominal is not None, splits=3)
        _, r, d, _ = b.step(plan["actions"])
        assert torch.equal(r, rew[t]) and torch.equal(d, done[t]), t
        nominal = plan["nominal"]
        nominal[d] = 0.0
        if bool(d[5]):
            assert not bool(nominal[5].any()) and bool(nominal[6].any())
    assert torch.equal(ctl.nominal, nominal)
    assert torch.equal(ctl.act(), b.mppi_plan(10, 64, 2, "reward", LAM, SIGMA, nominal=nominal, shift=True, splits=3)["actions"])
    a.close(); b.close()


# ---------------------------------------------------------------- 11. errors
def test_errors_leave_the_handle_usable(qa, torch):
    lib = qa._lib.load()
    INVALID = -1
    env = qa.VecDockingEnv("docking-v0", num_envs=8)
    env.reset()
    act = torch.empty((8, 4), device=env.device)
    nom = torch.empty((8, 128, 4), device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731

    def call(h, horizon=20, paths=200, iterations=2, objective=0, lam=1.0, sigma=0.5, shift=0, splits=2, actions=act, nominal_out=nom):
        rc = lib.qs_mppi_plan_split(h, horizon, paths, iterations, objective, lam, sigma, shift, splits, None, None, p(actions),
                                    p(nominal_out), None, None, None, None)
        return rc, lib.qs_last_error().decode()

    for kw, word in ((dict(splits=-1), "splits"), (dict(splits=201), "splits"), (dict(splits=65, paths=64), "splits"),
                     (dict(splits=1025, paths=4096), "splits"), (dict(paths=0), "paths"), (dict(paths=65537), "paths"),
                     (dict(horizon=0), "horizon"), (dict(horizon=129), "horizon"), (dict(iterations=0), "iterations"),
                     (dict(iterations=17), "iterations"), (dict(objective=2), "objective"), (dict(lam=0.0), "lambda"),
                     (dict(lam=float("nan")), "lambda"), (dict(lam=float("inf")), "lambda"), (dict(sigma=-1.0), "sigma"),
                     (dict(sigma=float("inf")), "sigma"), (dict(shift=2), "shift"), (dict(shift=-1), "shift"),
                     (dict(actions=None), "actions"), (dict(nominal_out=None), "nominal_out")):
        rc, msg = call(env._h, **kw)
        assert rc == INVALID and word in msg and "qs_mppi_plan_split" in msg, (kw, rc, msg)
    for kw in (dict(paths=65536, horizon=1, iterations=1, splits=1024), dict(paths=1, horizon=128, iterations=16, splits=1),
               dict(paths=4096, horizon=128, iterations=1, splits=1), dict(paths=4096, horizon=128, iterations=1, splits=1024),
               dict(paths=65536, horizon=2, iterations=1, splits=0), dict(paths=200, splits=200), dict(sigma=0.0)):
        rc, msg = call(env._h, **kw)                          # the limits themselves are fine
        assert rc == 0, (kw, msg)
    torch.cuda.synchronize()
    misaligned = torch.empty(8 * 4 + 1, device=env.device)[1:].view(8, 4)
    rc, msg = call(env._h, actions=misaligned)
    assert rc == INVALID and "aligned" in msg
    env.step_counter = 1 << 33
    rc, msg = call(env._h)
    assert rc == INVALID and "step counter" in msg
    env.step_counter = (1 << 33) - 1
    rc, msg = call(env._h)
    assert rc == 0, msg
    env.step_counter = 0
    obs, r, d, _ = env.step(torch.zeros((8, 4), device=env.device))       # the handle still steps
    assert bool(torch.isfinite(obs).all())
    env.close()

    hov = qa.VecDockingEnv("hovering-v0", num_envs=8)
    hov.reset()
    rc, msg = call(hov._h)
    assert rc == INVALID and "docking envs only" in msg
    with pytest.raises(qa.QuadsimError, match="docking envs only"):
        hov.mppi_plan(splits=2)
    hov.close()
