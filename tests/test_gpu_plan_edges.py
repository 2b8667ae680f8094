"""-m gpu: the four planners on the exact simulator (qs_shooting_plan, qs_shooting_plan_split, qs_mppi_plan, qs_mppi_plan_split) at
the edges of their keys, their strided loops and their buffers.  The cases are tests/plan_cases.py's, tests/plan_matrix.py names
one per compiled instantiation, tests/test_plan_edges_cpu.py shows on the references alone that each case can see its fault.

a. Shooting keys: at every step counter where a field of (k << 26) | (c << 10) | h crosses a 32-bit word, with a 64-bit seed and
   global ids on both sides of 2^32 and at the top of the 48-bit id space, all 200 scores bit for bit against the step API fed
   with shooting_ref.actions_fast; one env with 65 536 paths at k = 2^36 - 1.
b. MPPI keys: the in-kernel normals of iterations 0, 1, 2 and 15 against float64 Box-Muller of mppi_ref.normals at every step
   counter where k << 30 crosses a word; one env with 65 536 paths through the split entry point at k = 2^33 - 1.
c. Horizons past one trip of the loops strided over h: 65, and the admitted maxima 256 / 128, against the float64 oracle.
d. k_mppi at 4096 paths x horizon 128: its four LDS regions at their largest together.
e. Every output of the four entry points between sentinel bytes, each nullable output passed as NULL in turn.
Every case runs through the unsplit entry point and through the split one with 3 (ragged) and 7 parts (one part where there is
one path).  No element is left out of a comparison; the bounds are the ones test_gpu_shooting.py and test_gpu_mppi.py derive,
plus sigma NORMAL_TOL + 2^-24 for a candidate built from an in-kernel normal (one float32 rounding of a value in [-1, 1]).
Worst error / bound ratios measured on an MI355X, and two trials with deliberately wrong builds, are in
profiles/plan_edges/README.md."""
import ctypes as C

import numpy as np
import pytest

import mppi_ref
import shooting_ref
from plan_cases import (DT, EDGE_HORIZON, EDGE_N, EDGE_OFFSETS, EDGE_PATHS, EDGE_SEED, EDGE_SPLITS, LONG_HANDLES, LONG_K, LONG_MPPI,
                        LONG_SHOOT, LONG_SIGMA, MPPI_K, SHOOT_K, edge_handle, key_cases, long_handle, long_mppi_inputs, make_twin,
                        rec_par, same_bits, twin_scores)
from test_gpu_mppi import NORMAL_TOL, UPDATE_TOL
from test_gpu_mppi_split import ORDER_TOL
from test_gpu_postproc import Guards

pytestmark = pytest.mark.gpu

KEY_SIGMA, KEY_LAM = 0.25, 1e6          # sigma z is exact in float32; lam so large that the nominal stays near 0: nothing clamps
DRAW_TOL = KEY_SIGMA * NORMAL_TOL + 2.0 ** -24
_worst = {"normal": 0.0, "draw": 0.0, "shoot_reward": 0.0, "shoot_position": 0.0, "shoot_reward_pick": 0.0, "shoot_position_pick": 0.0,
          "mppi_reward": 0.0, "mppi_position": 0.0, "mppi_score_reward": 0.0, "mppi_score_position": 0.0, "update": 0.0, "order": 0.0}


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _shoot(env, horizon, paths, objective="reward", splits=None):
    return _host(env.shooting_plan(horizon, paths, objective, return_scores=True, return_sequence=True, splits=splits))


def _mppi(env, horizon, paths, iterations, objective="reward", lam=KEY_LAM, sigma=KEY_SIGMA, **kw):
    return _host(env.mppi_plan(horizon, paths, iterations, objective, lam, sigma, return_scores=True, return_trace=True,
                               return_candidates=True, **kw))


def _splits(paths):
    return EDGE_SPLITS if paths >= max(EDGE_SPLITS) else (1,)


def _assert_same_plan(got, want, what):
    assert sorted(got) == sorted(want), what
    for key in want:
        assert got[key].dtype == want[key].dtype and same_bits(got[key], want[key]), (what, key)


def _keyed_actions(offset, k, n, paths, horizon):
    return np.stack([shooting_ref.actions_fast(EDGE_SEED, offset + g, k, paths, horizon) for g in range(n)])


# ---------------------------------------------------------------- a. shooting keys
def _assert_definition(got, want, acts, what):
    """test_gpu_shooting.py's test_definition_bit_for_bit: the scores are the twin's, and winner, score, sequence and first
    action follow from them"""
    rows = np.arange(want.shape[0])
    assert same_bits(got["scores"], want), what
    win = shooting_ref.first_argmax(want)
    assert np.array_equal(got["best_index"], win.astype(np.int32)), what
    assert same_bits(got["best_score"], want[rows, win]), what
    assert same_bits(got["sequence"], acts[rows, win]), what
    assert same_bits(got["actions"], acts[rows, win, 0]), what


def _shooting_on_twin(qa, torch, env, env_id, integ, params, offset, k, paths, horizon):
    n = env.num_envs
    assert env.step_counter == k
    st, _, _ = rec_par(env)
    acts = _keyed_actions(offset, k, n, paths, horizon)
    twin = make_twin(qa, env, env_id, integ, params, paths)
    want, stopped = twin_scores(torch, twin, st, acts, paths)
    twin.close()
    got = _shoot(env, horizon, paths)
    _assert_definition(got, want, acts, "unsplit")
    for s in _splits(paths):
        _assert_same_plan(_shoot(env, horizon, paths, splits=s), got, s)
    assert env.step_counter == k
    return stopped


@pytest.mark.parametrize("case", key_cases(SHOOT_K), ids=lambda c: c[0])
def test_shooting_keys(qa, torch, case):
    _, env_id, integ, params, offset, k = case
    env = edge_handle(qa, env_id, integ, params, offset, k)
    assert _shooting_on_twin(qa, torch, env, env_id, integ, params, offset, k, EDGE_PATHS, EDGE_HORIZON) > 0
    env.close()


def test_shooting_one_env_with_65536_paths_is_the_step_api(qa, torch):
    """c up to 65 535 in the key and 256 candidates per lane, at the largest k and the global id of env 11 of the edge handle
    (2^32 + 5): the unsplit kernel, which is the reference of test_gpu_shooting_split.py's test_one_env_with_65536_paths"""
    k, gid = SHOOT_K[-1], EDGE_OFFSETS[0] + 11
    env = edge_handle(qa, "docking-v0", "rk4", True, gid, k, n=1)
    _shooting_on_twin(qa, torch, env, "docking-v0", "rk4", True, gid, k, 65536, EDGE_HORIZON)
    env.close()


# ---------------------------------------------------------------- b. MPPI keys
def _assert_draws(got, z64, it, what):
    """the candidates of iteration `it` (the last of `got`) are clamp(fma(sigma, z, U)), U = trace[:, it]: every unclamped element
    within DRAW_TOL of U + sigma z64, every clamped one with a reference at or beyond the clamp, candidate 0 clamp(U) exactly"""
    U, cand = got["trace"][:, it], got["candidates"]
    assert cand.shape == z64.shape and np.all(np.abs(cand) <= 1.0), what
    assert same_bits(cand[:, 0], np.clip(U, np.float32(-1), np.float32(1))), what
    ref = U.astype(np.float64)[:, None] + KEY_SIGMA * z64
    free = np.abs(cand) < 1.0
    free[:, 0] = False
    clamped = ~free
    clamped[:, 0] = False
    if cand.shape[1] > 1:
        assert free[:, 1:].mean() > 0.99, what
        err = float(np.max(np.abs(cand.astype(np.float64) - ref)[free]))
        znorm = float(np.max(np.abs((cand.astype(np.float64) - U.astype(np.float64)[:, None]) / KEY_SIGMA - z64)[free]))
        _worst["draw"], _worst["normal"] = max(_worst["draw"], err / DRAW_TOL), max(_worst["normal"], znorm)
        if err > DRAW_TOL:
            i = np.unravel_index(np.argmax(np.where(free, np.abs(cand.astype(np.float64) - ref), 0.0)), cand.shape)
            print("worst draw at (env, candidate, step, component) = %s: device %.9g, reference %.17g" % (i, cand[i], ref[i]))
        assert np.all(np.abs(ref[clamped]) >= 1.0 - DRAW_TOL), what
        assert err <= DRAW_TOL, (what, err)


def _assert_split_of(split, whole, what):
    """what a partition cannot change in an iteration that starts from the same nominal: test_gpu_mppi_split.py's identities"""
    for key in ("scores", "candidates", "best_score"):
        assert same_bits(split[key], whole[key]), (what, key)
    assert same_bits(split["trace"][:, 0], whole["trace"][:, 0]), what
    err = float(np.max(np.abs(split["trace"][:, 1].astype(np.float64) - whole["trace"][:, 1].astype(np.float64))))
    _worst["order"] = max(_worst["order"], err / ORDER_TOL)
    assert err <= ORDER_TOL, (what, err)


def _mppi_keys(qa, torch, env, env_id, integ, params, offset, k, paths, horizon, its, every=True):
    """iteration `it` of the key through a plan of it + 1 iterations (a prefix of a longer one), for the unsplit entry point and
    the split one: the draws against float64, the scores against the step API on the device's own candidates"""
    n = env.num_envs
    assert env.step_counter == k
    st, _, _ = rec_par(env)
    twin = make_twin(qa, env, env_id, integ, params, paths)
    stopped = 0
    for splits in ((None,) if every else ()) + _splits(paths):
        kw = {} if splits is None else dict(splits=splits)
        full = None
        for it in sorted(its, reverse=True):
            z64 = np.stack([mppi_ref.normals(EDGE_SEED, offset + g, k, it, paths, horizon) for g in range(n)])
            got = _mppi(env, horizon, paths, it + 1, **kw)
            what = (splits, it)
            if full is None:
                full = got
            assert same_bits(got["scores"], full["scores"][:, :it + 1]) and same_bits(got["trace"], full["trace"][:, :it + 2]), what
            _assert_draws(got, z64, it, what)
            want, s = twin_scores(torch, twin, st, got["candidates"], paths)
            stopped += s
            assert same_bits(got["scores"][:, it], want) and same_bits(got["best_score"], want.max(axis=1)), what
            assert same_bits(got["nominal"], got["trace"][:, -1]) and same_bits(got["actions"], got["nominal"][:, 0]), what
            if it == 0 and splits is None:
                first = got
            elif it == 0 and every:
                _assert_split_of(got, first, what)
    twin.close()
    assert env.step_counter == k
    print("worst so far: |z_dev - z_64| = %.4g (NORMAL_TOL %.4g), |candidate - f64| / bound = %.3g"
          % (_worst["normal"], NORMAL_TOL, _worst["draw"]))
    return stopped


@pytest.mark.parametrize("case", key_cases(MPPI_K), ids=lambda c: c[0])
def test_mppi_keys(qa, torch, case):
    _, env_id, integ, params, offset, k = case
    env = edge_handle(qa, env_id, integ, params, offset, k)
    assert _mppi_keys(qa, torch, env, env_id, integ, params, offset, k, EDGE_PATHS, EDGE_HORIZON, (0, 1, 2)) > 0
    env.close()


def test_mppi_keys_at_the_last_iteration(qa, torch):
    """iterations = 16, the maximum: it = 15 in the key"""
    _, env_id, integ, params, offset, k = key_cases(MPPI_K)[-1]
    assert k == (1 << 33) - 1 and offset == EDGE_OFFSETS[1]
    env = edge_handle(qa, env_id, integ, params, offset, k)
    _mppi_keys(qa, torch, env, env_id, integ, params, offset, k, EDGE_PATHS, EDGE_HORIZON, (15,))
    env.close()


def test_mppi_split_one_env_with_65536_paths(qa, torch):
    """c up to 65 535 in MPPI's key, at the largest k and the global id 2^32 + 5: the split entry point alone (one workgroup
    holds 4096 paths)"""
    k, gid = MPPI_K[-1], EDGE_OFFSETS[0] + 11
    env = edge_handle(qa, "docking-v0", "rk4", True, gid, k, n=1)
    _mppi_keys(qa, torch, env, "docking-v0", "rk4", True, gid, k, 65536, 1, (0,), every=False)
    env.close()


# ---------------------------------------------------------------- c. long horizons
@pytest.mark.parametrize("paths,horizon", LONG_SHOOT)
@pytest.mark.parametrize("env_id,integ,params", LONG_HANDLES)
def test_long_horizon_shooting(qa, torch, env_id, integ, params, paths, horizon):
    """test_gpu_shooting.py's test_against_float64_reference and its bounds where the loops strided over h take two and four
    trips (blocks of 64 threads at paths 1 and 64) -- and the winner's sequence and first action bit for bit"""
    env, rec_cpu, par_cpu = long_handle(qa, env_id, integ, params)
    _, rec, par = rec_par(env)
    assert np.array_equal(rec, rec_cpu) and np.array_equal(par, par_cpu)      # the states test_plan_edges_cpu.py judged
    n, rows = EDGE_N, np.arange(EDGE_N)
    acts = _keyed_actions(EDGE_OFFSETS[0], LONG_K, n, paths, horizon)
    s_rew, s_pos, r = shooting_ref.plan_scores_both(rec, par, acts, kind=1 if env_id == "docking-v2" else 0, dt=DT,
                                                    integ=1 if integ == "rk4" else 0)
    assert r < 20.0
    for objective, ref, tol in (("reward", s_rew, 2 * horizon * 1e-5), ("position", s_pos, 2 * horizon * 2 * r * 2e-5)):
        got = _shoot(env, horizon, paths, objective)
        dev = float(np.max(np.abs(got["scores"] - ref)))
        pick = float(np.max(ref.max(axis=1) - ref[rows, got["best_index"]]))
        _worst["shoot_" + objective] = max(_worst["shoot_" + objective], dev / (tol / 2))
        _worst["shoot_" + objective + "_pick"] = max(_worst["shoot_" + objective + "_pick"], pick / tol)
        print("%s %s params=%d paths=%d horizon=%d %s: max |score - f64| = %.3g (bound %.3g), f64 regret of the pick = %.3g "
              "(bound %.3g), r = %.3g; worst so far as fractions of the bounds: %s"
              % (env_id, integ, params, paths, horizon, objective, dev, tol / 2, pick, tol, r, _worst))
        assert np.all(ref[rows, got["best_index"]] >= ref.max(axis=1) - tol), objective
        assert dev <= tol / 2, objective
        assert np.array_equal(got["best_score"], got["scores"][rows, got["best_index"]])
        assert same_bits(got["sequence"], acts[rows, got["best_index"]]), objective
        assert same_bits(got["actions"], acts[rows, got["best_index"], 0]), objective
        for s in _splits(paths):
            _assert_same_plan(_shoot(env, horizon, paths, objective, s), got, (objective, s))
    env.close()


@pytest.mark.parametrize("paths,horizon,shift", LONG_MPPI)
def test_long_horizon_mppi(qa, torch, paths, horizon, shift):
    """one iteration with caller noise: the candidates exactly, the update closed on the device's own outputs, and end to end
    against the float64 oracle with test_gpu_mppi.py's bounds (lam doubled from that test's value until its tol <= 0.05 holds)"""
    env_id, integ, params = LONG_HANDLES[0]
    env, rec_cpu, par_cpu = long_handle(qa, env_id, integ, params)
    _, rec, par = rec_par(env)
    assert np.array_equal(rec, rec_cpu) and np.array_equal(par, par_cpu)
    nominal, z = long_mppi_inputs()
    nominal, z = np.ascontiguousarray(nominal[:, :horizon]), np.ascontiguousarray(z[:paths, :horizon])
    U = nominal[:, np.minimum(np.arange(horizon) + shift, horizon - 1)]
    cands = mppi_ref.candidates32(U, LONG_SIGMA, z)
    s_rew, s_pos, r = shooting_ref.plan_scores_both(rec, par, cands, kind=0, dt=DT, integ=0)
    assert r < 20.0
    kw = dict(sigma=LONG_SIGMA, noise=torch.from_numpy(z[None]).to(env.device), nominal=torch.from_numpy(nominal).to(env.device),
              shift=bool(shift))

    def closed_update(got, lam, what):
        want = mppi_ref.update64(got["scores"][:, 0], got["candidates"], lam, got["trace"][:, 0])
        err = float(np.max(np.abs(got["trace"][:, 1].astype(np.float64) - want)))
        _worst["update"] = max(_worst["update"], err / UPDATE_TOL)
        assert err <= UPDATE_TOL, (what, err)
        assert same_bits(got["nominal"], got["trace"][:, -1]) and same_bits(got["actions"], got["nominal"][:, 0]), what
        assert same_bits(got["best_score"], got["scores"][:, -1].max(axis=1)), what

    for objective, S, ds, lam in (("reward", s_rew, horizon * 1e-5, 0.02), ("position", s_pos, horizon * 2 * r * 2e-5, 1.5)):
        while 4 * ds / lam + 2.0 ** -23 > 0.05:
            lam *= 2.0
        tol = 4 * ds / lam + 2.0 ** -23
        assert tol <= 0.05
        want = mppi_ref.update64(S, cands, lam, U)
        got = _mppi(env, horizon, paths, 1, objective, lam=lam, **kw)
        assert same_bits(got["trace"][:, 0], U), objective                       # min(h + shift, horizon - 1)
        assert same_bits(got["candidates"], cands), objective
        closed_update(got, lam, objective)
        dev_s = float(np.max(np.abs(got["scores"][:, 0] - S)))
        err = float(np.max(np.abs(got["nominal"].astype(np.float64) - want)))
        _worst["mppi_" + objective] = max(_worst["mppi_" + objective], err / tol)
        _worst["mppi_score_" + objective] = max(_worst["mppi_score_" + objective], dev_s / ds)
        print("paths=%d horizon=%d shift=%d %s lam=%g: max |score - f64| = %.3g (bound %.3g), max |nominal - f64| = %.3g (bound %.3g), "
              "r = %.3g; worst so far as fractions of the bounds: %s" % (paths, horizon, shift, objective, lam, dev_s, ds, err, tol, r, _worst))
        assert dev_s <= ds and err <= tol, objective
        for s in _splits(paths):
            split = _mppi(env, horizon, paths, 1, objective, lam=lam, splits=s, **kw)
            _assert_split_of(split, got, (objective, s))
            closed_update(split, lam, (objective, s))
            assert float(np.max(np.abs(split["nominal"].astype(np.float64) - want))) <= tol, (objective, s)
    env.close()


# ---------------------------------------------------------------- d. the LDS corner
def test_mppi_at_4096_paths_and_horizon_128(qa, torch):
    """58 432 B of dynamic LDS: partial sums [4][128][4] f64, the nominal [128] float4, the scores [4096] f64 and the target rows
    [128][14], each at its largest.  Two envs in free flight (global ids 2^32 - 1 and 2^32) around a nominal near hover, so that
    the roll-outs read the rows of all 128 steps; the scores bit for bit against the step API on an 8192-env twin"""
    env_id, integ, params = "docking-v2", "rk4", True
    n, paths, horizon, lam, offset, k = 2, 4096, 128, 0.5, EDGE_OFFSETS[0] + 5, MPPI_K[-1]
    env = edge_handle(qa, env_id, integ, params, offset, k, provoke=None, n=n)
    st, _, _ = rec_par(env)
    rng = np.random.default_rng(31)
    nominal = (-0.5 + 0.1 * (rng.random((n, horizon, 4)) - 0.5)).astype(np.float32)
    z = rng.standard_normal((paths, horizon, 4)).astype(np.float32)
    kw = dict(lam=lam, sigma=LONG_SIGMA, noise=torch.from_numpy(z[None]).to(env.device), nominal=torch.from_numpy(nominal).to(env.device))
    got = _mppi(env, horizon, paths, 1, **kw)
    assert same_bits(got["trace"][:, 0], nominal)
    assert same_bits(got["candidates"], mppi_ref.candidates32(nominal, LONG_SIGMA, z))
    twin = make_twin(qa, env, env_id, integ, params, paths)
    want, stopped = twin_scores(torch, twin, st, got["candidates"], paths)
    twin.close()
    assert stopped < n * paths                                 # candidates did fly the whole horizon
    assert same_bits(got["scores"][:, 0], want) and same_bits(got["best_score"], want.max(axis=1))
    upd = mppi_ref.update64(got["scores"][:, 0], got["candidates"], lam, nominal)
    err = float(np.max(np.abs(got["nominal"].astype(np.float64) - upd)))
    print("4096 x 128: %d of %d candidates stopped inside the horizon; |update - f64| = %.3g (bound %.3g)" % (stopped, n * paths, err, UPDATE_TOL))
    assert err <= UPDATE_TOL
    assert same_bits(got["nominal"], got["trace"][:, 1]) and same_bits(got["actions"], got["nominal"][:, 0])
    for s in EDGE_SPLITS:
        split = _mppi(env, horizon, paths, 1, splits=s, **kw)
        _assert_split_of(split, got, s)
        assert float(np.max(np.abs(split["nominal"].astype(np.float64) - upd))) <= UPDATE_TOL, s
    env.close()


# ---------------------------------------------------------------- e. sentinels
SENTINEL_SHAPES = ((65, 200, 3), (3, 64, 65))                 # n, paths, horizon: a tail tile of one env; the strided loops over h
F4, F8, I4 = np.float32, np.float64, np.int32


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _raw(torch, env, fn, *args):
    env._use_current_stream()
    env._inputs_ready()
    rc = fn(env._h, *args)
    assert rc == 0, env._lib.qs_last_error().decode()
    env._outputs_ready()
    torch.cuda.synchronize()


def _sentinel_handle(qa, n, k):
    return edge_handle(qa, "docking-v2", "rk4", True, EDGE_OFFSETS[0], k, n=n)


@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split7"])
@pytest.mark.parametrize("n,paths,horizon", SENTINEL_SHAPES)
def test_shooting_outputs_between_sentinels(qa, torch, n, paths, horizon, split):
    env = _sentinel_handle(qa, n, SHOOT_K[-1])
    lib = qa._lib.load()
    want = _shoot(env, horizon, paths, splits=7 if split else None)
    shapes = dict(actions=((n, 4), F4), best_score=((n,), F8), best_index=((n,), I4), sequence=((n, horizon, 4), F4),
                  scores=((n, paths), F8))
    for drop in (None, "best_score", "best_index", "sequence", "scores"):
        G = Guards(torch, env.device)
        out = {key: G.out(*shapes[key]) for key in shapes if key != drop}
        bufs = [_ptr(out.get(key)) for key in shapes]
        if split:
            _raw(torch, env, lib.qs_shooting_plan_split, horizon, paths, 0, 7, *bufs)
        else:
            _raw(torch, env, lib.qs_shooting_plan, horizon, paths, 0, *bufs)
        G.check()
        for key, t in out.items():
            assert same_bits(t.cpu().numpy(), want[key]), (drop, key)
    env.close()


@pytest.mark.parametrize("split", [False, True], ids=["unsplit", "split7"])
@pytest.mark.parametrize("n,paths,horizon", SENTINEL_SHAPES)
def test_mppi_outputs_between_sentinels(qa, torch, n, paths, horizon, split):
    env = _sentinel_handle(qa, n, MPPI_K[-1])
    lib = qa._lib.load()
    iters, lam, sigma = 2, 0.5, 0.4
    rng = np.random.default_rng(37)
    nominal = (rng.random((n, horizon, 4)) * 2.4 - 1.2).astype(np.float32)      # beyond the clamp too
    noise = rng.standard_normal((iters, paths, horizon, 4)).astype(np.float32)
    want = _mppi(env, horizon, paths, iters, lam=lam, sigma=sigma, nominal=torch.from_numpy(nominal).to(env.device),
                 noise=torch.from_numpy(noise).to(env.device), shift=True, **(dict(splits=7) if split else {}))
    shapes = dict(actions=((n, 4), F4), nominal=((n, horizon, 4), F4), best_score=((n,), F8), scores=((n, iters, paths), F8),
                  trace=((n, iters + 1, horizon, 4), F4), candidates=((n, paths, horizon, 4), F4))
    for drop in (None, "best_score", "scores", "trace", "candidates"):
        G = Guards(torch, env.device)
        ins = [_ptr(G.put(nominal)), _ptr(G.put(noise))]      # read-only: check() holds them to their bytes
        out = {key: G.out(*shapes[key]) for key in shapes if key != drop}
        bufs = ins + [_ptr(out.get(key)) for key in shapes]
        if split:
            _raw(torch, env, lib.qs_mppi_plan_split, horizon, paths, iters, 0, lam, sigma, 1, 7, *bufs)
        else:
            _raw(torch, env, lib.qs_mppi_plan, horizon, paths, iters, 0, lam, sigma, 1, *bufs)
        G.check()
        for key, t in out.items():
            assert same_bits(t.cpu().numpy(), want[key]), (drop, key)
    env.close()
