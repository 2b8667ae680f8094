"""-m gpu: qs_mppi_plan (VecDockingEnv.mppi_plan, MPPI).

1. Scores, bit for bit: the device's own candidates, staged on a second handle of N x paths envs with the replicated state and
   stepped `horizon` times with qs_step, give the scores of every iteration; iterations are a prefix.
2. Candidates, exactly, with caller noise; the shift; the zero nominal.
3. The update, closed on the device's own scores and candidates, against float64 with a derived bound.
4. The in-kernel normals against float64.  5. End to end against the float64 oracle, one iteration.
6. Read-only and reproducible.  7. Independence of the mapping.  8. The closed loop.  9. Errors."""
import ctypes as C

import numpy as np
import pytest

import mppi_ref
from plan_cases import DT, HANDLES, HORIZONS, N, PATHS, SEED, in_flight_pair, make_handle, make_twin, slice_handle, twin_scores
from plan_cases import rec_par as _rec_par, same as _same, same_bits as _same_bits, snapshot as _snapshot

pytestmark = pytest.mark.gpu

ITERATIONS = (1, 3)
SUBSET = [("docking-v0", "frozen", False), ("docking-v1", "rk4", True), ("docking-v2", "frozen", True), ("docking-v0", "rk4", False)]
LAM, SIGMA = 0.5, 0.4


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---------------------------------------------------------------- plans
def _plan(env, horizon, paths, iterations=1, objective="reward", lam=LAM, sigma=SIGMA, **kw):
    kw.setdefault("return_scores", True)
    kw.setdefault("return_trace", True)
    kw.setdefault("return_candidates", True)
    out = env.mppi_plan(horizon, paths, iterations, objective, lam, sigma, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------- 1. scores, bit for bit
@pytest.mark.parametrize("env_id,integ,params", HANDLES)
def test_scores_bit_for_bit_and_iteration_prefix(qa, torch, env_id, integ, params):
    env = make_handle(qa, env_id, integ, params)
    k = env.step_counter
    st, _, _ = _rec_par(env)
    stopped_inside = 0
    iters = max(ITERATIONS)
    for paths in PATHS:
        twin = make_twin(qa, env, env_id, integ, params, paths)
        for horizon in HORIZONS:
            full = None
            for j in range(iters, 0, -1):
                got = _plan(env, horizon, paths, j)
                if full is None:
                    full = got
                assert _same_bits(got["scores"], full["scores"][:, :j]), (paths, horizon, j)      # iteration prefix
                assert _same_bits(got["trace"], full["trace"][:, :j + 1]), (paths, horizon, j)
                acts = got["candidates"]
                assert acts.shape == (N, paths, horizon, 4) and np.all(np.abs(acts) <= 1.0)
                want, stopped = twin_scores(torch, twin, st, acts, paths)
                stopped_inside += stopped
                assert _same_bits(got["scores"][:, j - 1], want), (paths, horizon, j)
                assert _same_bits(got["best_score"], want.max(axis=1)), (paths, horizon, j)
        twin.close()
    assert stopped_inside > 0                                 # candidates did terminate inside a horizon
    assert env.step_counter == k
    env.close()


# ---------------------------------------------------------------- 2. candidates with caller noise, shift, zero nominal
@pytest.mark.parametrize("env_id,integ,params", SUBSET)
def test_candidates_exact_with_caller_noise(qa, torch, env_id, integ, params):
    env = make_handle(qa, env_id, integ, params)
    gen = torch.Generator(device="cpu").manual_seed(7)
    for paths in PATHS:
        for horizon in HORIZONS:
            for iters in ITERATIONS:
                noise = torch.randn((iters, paths, horizon, 4), generator=gen).to(env.device)
                nominal = (torch.rand((N, horizon, 4), generator=gen) * 2.4 - 1.2).to(env.device)     # beyond the clamp too
                nominal[0, 0, 0] = -0.0
                zn = noise.cpu().numpy()
                for shift, nom in ((False, None), (True, nominal), (False, nominal)):
                    got = _plan(env, horizon, paths, iters, noise=noise, nominal=nom, shift=shift)
                    if nom is None:
                        first = np.zeros((N, horizon, 4), np.float32)
                    else:
                        src = nom.cpu().numpy()
                        first = src[:, np.minimum(np.arange(horizon) + int(shift), horizon - 1)]
                    key = (paths, horizon, iters, shift, nom is None)
                    assert _same_bits(got["trace"][:, 0], first), key
                    U = got["trace"][:, iters - 1]
                    want = mppi_ref.candidates32(U, SIGMA, zn[iters - 1])
                    assert _same_bits(got["candidates"], want), key
                    assert _same_bits(got["candidates"][:, 0], np.clip(U, np.float32(-1), np.float32(1))), key
    env.close()


# ---------------------------------------------------------------- 3. the update, closed on the device's own outputs
# Both sums and the exponential are float64 on the device, so the quotient agrees with numpy's to ~1e-13 before it is rounded
# to float32 once: values in [-1, 1] differ by at most one rounding (2^-24) plus the reference's own; 2 * 2^-24.
UPDATE_TOL = 2.0 * 2.0 ** -24


@pytest.mark.parametrize("env_id,integ,params", SUBSET)
def test_update_against_float64_on_device_outputs(qa, torch, env_id, integ, params):
    env = make_handle(qa, env_id, integ, params)
    gen = torch.Generator(device="cpu").manual_seed(11)
    worst = 0.0
    for objective, lam in (("reward", 0.05), ("position", 2.0)):
        for paths in PATHS:
            for horizon in HORIZONS:
                noise = torch.randn((max(ITERATIONS), paths, horizon, 4), generator=gen).to(env.device) if paths == 200 else None
                for it in range(max(ITERATIONS)):
                    got = _plan(env, horizon, paths, it + 1, objective, lam=lam, noise=None if noise is None else noise[:it + 1].contiguous())
                    want = mppi_ref.update64(got["scores"][:, it], got["candidates"], lam, got["trace"][:, it])
                    err = float(np.max(np.abs(got["trace"][:, it + 1].astype(np.float64) - want)))
                    worst = max(worst, err)
                    assert err <= UPDATE_TOL, (objective, paths, horizon, it, err)
                    assert _same_bits(got["nominal"], got["trace"][:, -1]) and _same_bits(got["actions"], got["nominal"][:, 0])
                    assert _same_bits(got["best_score"], got["scores"][:, -1].max(axis=1))
    print("%s %s params=%d: worst |update - f64| = %.3g (bound %.3g)" % (env_id, integ, params, worst, UPDATE_TOL))
    env.close()


# ---------------------------------------------------------------- 4. the in-kernel normals
# q_ln, q_sqrt and q_sincos are approximations, so this bound is measured, not derived: max |z_dev - z_64| over this test's
# 7.67e6 draws on an MI355X was NORMAL_ERR_MEASURED (profiles/mppi/README.md); the assertion allows four times that, because
# the tail of the error at u -> 0 is thinly sampled by ~10^7 draws.
NORMAL_ERR_MEASURED = 1.7e-6          # 1.69990e-6 over 7 671 814 draws, MI355X, 2026-10-17
NORMAL_TOL = 4.0 * NORMAL_ERR_MEASURED


def test_in_kernel_normals_against_float64(qa, torch):
    env = make_handle(qa, "docking-v0", "frozen", False, provoke=None)
    k = env.step_counter
    sigma, paths, horizon = 0.25, 1000, 20
    got = _plan(env, horizon, paths, 1, sigma=sigma)
    cand = got["candidates"]
    assert np.all(cand[:, 0] == 0.0)
    z64 = np.stack([mppi_ref.normals(SEED, g, k, 0, paths, horizon) for g in range(N)])
    free = np.abs(cand) < 1.0                                 # no clamping reached: 0.25 z is exact, so cand / 0.25 is z
    free[:, 0] = False
    assert free[:, 1:].mean() > 0.999
    err = float(np.max(np.abs(cand.astype(np.float64)[free] / sigma - z64[free])))
    print("max |z_dev - z_64| over %d draws = %.4g (asserted at %.4g)" % (int(free.sum()), err, NORMAL_TOL))
    clamped = ~free
    clamped[:, 0] = False
    assert np.all(np.abs(z64[clamped]) >= 4.0 - 1e-3)         # what was clamped was a draw beyond 4 sigma
    assert err <= NORMAL_TOL
    # with no tolerance: the draws differ between envs, between iterations, and between k and k + 1
    assert not np.array_equal(cand[0], cand[1])
    three = _plan(env, horizon, paths, 3, sigma=sigma, lam=1e6)     # lam large: the nominal stays near 0, candidates ~ sigma z
    z0 = cand[:, 1:].astype(np.float64)
    z2 = (three["candidates"][:, 1:].astype(np.float64) - three["trace"][:, 2][:, None])
    assert float(np.mean(np.abs(z2 - z0))) > 0.1 * sigma
    env.step(torch.zeros((N, 4), device=env.device))
    nxt = _plan(env, horizon, paths, 1, sigma=sigma)
    assert float(np.mean(np.abs(nxt["candidates"][:, 1:] - cand[:, 1:]))) > 0.1 * sigma
    env.close()


# ---------------------------------------------------------------- 5. end to end against float64, one iteration
# Per step the project asserts |reward - oracle| <= 1e-5 and |obs - oracle| <= 2e-5.  |dS| <= horizon * 1e-5 (REWARD) or
# horizon * 2 r * 2e-5 (POSITION, r = the largest |rel_pos|).  A weight ratio exp((S_c - S_max) / lam) is then off by a
# factor within exp(+-2 |dS| / lam), and a weighted mean of values in [-1, 1] by at most 4 |dS| / lam, plus the float32
# rounding of the result (2^-23 with the reference's).  lam is chosen per objective so that the bound is <= 0.05.
# Cases: the whole paths x horizon grid on each of the four handles of SUBSET (48 cases, every env counts); one iteration and
# caller noise throughout, as the comparison needs identical candidates.
E2E_CASES = [(k, g, q, p, h) for (k, g, q) in SUBSET for p in PATHS for h in HORIZONS]
_worst = {"reward": 0.0, "position": 0.0}


@pytest.mark.parametrize("env_id,integ,params,paths,horizon", E2E_CASES)
def test_end_to_end_against_float64_oracle(qa, torch, env_id, integ, params, paths, horizon):
    env = make_handle(qa, env_id, integ, params, provoke="decisive")
    _, rec, par = _rec_par(env)
    gen = torch.Generator(device="cpu").manual_seed(13)
    noise = torch.randn((1, paths, horizon, 4), generator=gen).to(env.device)
    nominal = (torch.rand((N, horizon, 4), generator=gen) - 0.5).to(env.device)
    U, z = nominal.cpu().numpy(), noise.cpu().numpy()[0]
    cands = mppi_ref.candidates32(U, SIGMA, z)
    s_rew, s_pos, r = mppi_ref.shooting_ref.plan_scores_both(rec, par, cands, kind=1 if env_id == "docking-v2" else 0, dt=DT,
                                                            integ=1 if integ == "rk4" else 0)
    assert r < 20.0
    for objective, S, ds, lam in (("reward", s_rew, horizon * 1e-5, 0.02), ("position", s_pos, horizon * 2 * r * 2e-5, 1.5)):
        tol = 4 * ds / lam + 2.0 ** -23
        assert tol <= 0.05
        want = mppi_ref.update64(S, cands, lam, U)
        got = _plan(env, horizon, paths, 1, objective, lam=lam, noise=noise, nominal=nominal)
        assert _same_bits(got["candidates"], cands)
        dev_s = float(np.max(np.abs(got["scores"][:, 0] - S)))
        err = float(np.max(np.abs(got["nominal"].astype(np.float64) - want)))
        _worst[objective] = max(_worst[objective], err / tol)
        print("%s %s params=%d paths=%d horizon=%d %s lam=%g: max |score - f64| = %.3g (bound %.3g), max |nominal - f64| = %.3g "
              "(bound %.3g); worst so far as fractions of the bound: %s"
              % (env_id, integ, params, paths, horizon, objective, lam, dev_s, ds, err, tol, _worst))
        assert dev_s <= ds and err <= tol, objective
    env.close()


# ---------------------------------------------------------------- 6. read-only, reproducible
@pytest.mark.parametrize("env_id,params,auto_reset", [("docking-v0", False, True), ("docking-v2", True, False), ("docking-v1", False, True)])
def test_read_only_and_reproducible(qa, torch, env_id, params, auto_reset):
    env = make_handle(qa, env_id, "frozen", params, auto_reset=auto_reset)
    twin = make_handle(qa, env_id, "frozen", params, auto_reset=auto_reset)
    before = _snapshot(env)
    assert _same(before, _snapshot(twin))
    init_before = env.get_init_state() if env_id == "docking-v1" else None      # the only kind with stored initial states
    p1 = _plan(env, 20, 200, 3)
    q1 = _plan(env, 20, 200, 3, "position", lam=2.0)
    assert _same(before, _snapshot(env))                      # state, params, step counter (the rollout layout: below)
    if init_before is not None:
        after = env.get_init_state()
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(init_before, after))
    p2 = _plan(env, 20, 200, 3)
    q2 = _plan(env, 20, 200, 3, "position", lam=2.0)
    for key in p1:
        assert _same_bits(p1[key], p2[key]) and _same_bits(q1[key], q2[key]), key
    # the rollout layout: there is no getter, so it is observed.  Both handles are set env-major, `env` plans, and both then run
    # the same expert roll-out WITHOUT the layout being set again: a plan that had reset it would write obs [T,N,12], not [N,T,12]
    if auto_reset:                                            # (qs_expert_rollout, the observer, needs an auto_reset handle)
        lib, T = qa._lib.load(), 3
        ptr = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
        outs = []
        for h in (env, twin):
            qa._lib.check(lib.qs_set_rollout_layout(h._h, 1), "qs_set_rollout_layout")
        _plan(env, 20, 200, 3)
        for h in (env, twin):
            ex = qa.PIDExpert(h)
            o = {k: torch.zeros(sh, dtype=dt, device=h.device) for k, sh, dt in
                 (("obs", (N, T, 12), torch.float32), ("act", (N, T, 4), torch.float32), ("rew", (T, N), torch.float32),
                  ("done", (T, N), torch.uint8), ("last", (N, 12), torch.float32))}
            h._use_current_stream()
            h._inputs_ready()
            qa._lib.check(lib.qs_expert_rollout(h._h, T, ptr(ex.state_des), ex.kp, ex.kd, ptr(o["obs"]), ptr(o["act"]), ptr(o["rew"]),
                                                ptr(o["done"]), None, ptr(o["last"])), "qs_expert_rollout")
            h._outputs_ready()
            h._nstep += T
            outs.append(o)
        for key in outs[0]:
            assert torch.equal(outs[0][key], outs[1][key]), key
        time_major = outs[1]["obs"].reshape(T, N, 12).transpose(0, 1)
        assert not torch.equal(time_major, outs[1]["obs"])        # the two layouts are distinguishable on this data
        for h in (env, twin):
            qa._lib.check(lib.qs_set_rollout_layout(h._h, 0), "qs_set_rollout_layout")
    assert _same(_snapshot(env), _snapshot(twin))
    acts = env.random_actions(10, step0=100)
    for t in range(10):                                       # the twin never planned: the same next 10 steps
        oa, ra, da, _ = env.step(acts[t])
        ob, rb, db, _ = twin.step(acts[t])
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db), t
        if t == 0:
            p3 = _plan(env, 20, 200, 3)                       # k changed: other candidates
            assert not np.array_equal(p3["candidates"], p1["candidates"]) and not np.array_equal(p3["nominal"], p1["nominal"])
    assert _same(_snapshot(env), _snapshot(twin))
    env.close(); twin.close()


# ---------------------------------------------------------------- 7. mapping independence
def _raw(qa, torch, env, horizon, paths, iterations, nominal_in, nominal_out, lam=LAM, sigma=SIGMA, shift=0):
    """the C entry point with the caller's own nominal buffers (the Python wrapper always allocates the output)"""
    act = torch.empty((env.num_envs, 4), device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    env._use_current_stream()
    env._inputs_ready()
    qa._lib.check(env._lib.qs_mppi_plan(env._h, horizon, paths, iterations, 0, lam, sigma, shift, p(nominal_in), None, p(act),
                                        p(nominal_out), None, None, None, None), "qs_mppi_plan")
    env._outputs_ready()
    torch.cuda.synchronize()
    return act.cpu().numpy(), nominal_out.cpu().numpy()


def test_one_env_handle_plans_like_the_same_env_of_a_large_handle(qa, torch):
    """N = 1 against N = 4096: env 1234 of the large handle and the single env of a handle with env_id_offset = 1234, the same
    state, parameters and step counter -- 1, 64, 200 and 1000 paths (blocks of 64, 64, 256 and 256 threads); and a nominal
    buffer that is both input and output"""
    g = 1234
    big = make_handle(qa, "docking-v0", "frozen", True, n=4096)
    one = slice_handle(qa, big, g, 1)
    gen = torch.Generator(device="cpu").manual_seed(17)
    for paths in PATHS:
        nominal = (torch.rand((4096, 20, 4), generator=gen) - 0.5).to(big.device)
        for objective, lam in (("reward", LAM), ("position", 2.0)):
            a = _plan(big, 20, paths, 3, objective, lam=lam, nominal=nominal, shift=True, return_candidates=False)
            b = _plan(one, 20, paths, 3, objective, lam=lam, nominal=nominal[g:g + 1].contiguous(), shift=True)
            for key in a:                                     # (the large handle's candidates alone would be 1.3 GB)
                assert _same_bits(a[key][g:g + 1], b[key]), (paths, objective, key)
        # aliased: nominal_in is nominal_out
        want = _plan(big, 20, paths, 3, nominal=nominal, shift=True, return_candidates=False, return_scores=False)
        buf = nominal.clone()
        act, nom = _raw(qa, torch, big, 20, paths, 3, buf, buf, shift=1)
        assert _same_bits(nom, want["nominal"]) and _same_bits(act, want["actions"]), paths
    big.close(); one.close()


def test_private_queue_handle_plans_like_hip_stream_twin(qa, torch):
    """a private-queue handle with steps still in flight: drained first, then the same plan as a HIP-stream twin, and both step
    on alike"""
    a, b, last = in_flight_pair(qa, torch)
    pa, pb = _plan(a, 20, 200, 3, return_candidates=False), _plan(b, 20, 200, 3, return_candidates=False)
    for key in pa:
        assert _same_bits(pa[key], pb[key]), key
    assert a.step_counter == b.step_counter == 7
    oa, ra, _, _ = a.step(last)
    ob, rb, _, _ = b.step(last)
    assert torch.equal(oa, ob) and torch.equal(ra, rb)
    a.close(); b.close()


# ---------------------------------------------------------------- 8. closed loop
def test_closed_loop_is_plan_step_and_masked_zeroing(qa, torch):
    def make():
        env = make_handle(qa, "docking-v0", "frozen", False, provoke=None)
        st = env.get_state()
        t0 = st["t"].copy()
        t0[5] = 595.0                                         # times out inside the 8 steps
        env.set_state(t=t0)
        return env
    a, b = make(), make()
    ctl = qa.MPPI(a, horizon=10, paths=64, iterations=2, lam=LAM, sigma=SIGMA)
    rew, done = ctl.run(8)
    assert rew.shape == (8, N) and done.shape == (8, N) and done.dtype == torch.bool
    assert bool(done[:, 5].any()) and not bool(done.all())
    nominal = None
    for t in range(8):
        plan = b.mppi_plan(10, 64, 2, "reward", LAM, SIGMA, nominal=nominal, shift=nominal is not None)
        _, r, d, _ = b.step(plan["actions"])
        assert torch.equal(r, rew[t]) and torch.equal(d, done[t]), t
        nominal = plan["nominal"]
        nominal[d] = 0.0
        if bool(d[5]):
            assert not bool(nominal[5].any()) and bool(nominal[6].any())
    assert torch.equal(ctl.nominal, nominal)
    assert torch.equal(ctl.act(), b.mppi_plan(10, 64, 2, "reward", LAM, SIGMA, nominal=nominal, shift=True)["actions"])
    ctl.reset()
    assert ctl.nominal is None
    a.close(); b.close()


# ---------------------------------------------------------------- 9. errors
def test_errors(qa, torch):
    lib = qa._lib.load()
    INVALID = -1
    env = qa.VecDockingEnv("docking-v0", num_envs=8)
    env.reset()
    act = torch.empty((8, 4), device=env.device)
    nom = torch.empty((8, 128, 4), device=env.device)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731

    def call(h, horizon=20, paths=200, iterations=2, objective=0, lam=1.0, sigma=0.5, shift=0, actions=act, nominal_out=nom):
        rc = lib.qs_mppi_plan(h, horizon, paths, iterations, objective, lam, sigma, shift, None, None, p(actions), p(nominal_out),
                              None, None, None, None)
        return rc, lib.qs_last_error().decode()

    for kw, word in ((dict(paths=0), "paths"), (dict(paths=4097), "paths"), (dict(horizon=0), "horizon"),
                     (dict(horizon=129), "horizon"), (dict(iterations=0), "iterations"), (dict(iterations=17), "iterations"),
                     (dict(objective=2), "objective"), (dict(lam=0.0), "lambda"), (dict(lam=float("nan")), "lambda"),
                     (dict(lam=float("inf")), "lambda"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("inf")), "sigma"),
                     (dict(shift=2), "shift"), (dict(shift=-1), "shift"),
                     (dict(actions=None), "actions"), (dict(nominal_out=None), "nominal_out")):
        rc, msg = call(env._h, **kw)
        assert rc == INVALID and word in msg, (kw, rc, msg)
        with pytest.raises(qa.QuadsimError):
            qa._lib.check(rc, "qs_mppi_plan")
    for kw in (dict(paths=4096, horizon=1, iterations=1), dict(paths=1, horizon=128, iterations=16), dict(paths=4096, horizon=128, iterations=1),
               dict(sigma=0.0)):
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
    with pytest.raises(qa.QuadsimError, match="docking envs only"):
        hov.mppi_plan()
    hov.close()

    cfg = qa._lib.default_config()
    cfg.kind, cfg.num_envs, cfg.io_space, cfg.auto_reset = qa._lib.KIND_V0, 8, qa._lib.IO_HOST, 1
    h = C.c_void_p()
    assert lib.qs_create(C.byref(cfg), C.byref(h)) == 0
    host, hnom = np.empty((8, 4), np.float32), np.empty((8, 20, 4), np.float32)
    assert lib.qs_mppi_plan(h, 20, 200, 2, 0, 1.0, 0.5, 0, None, None, host.ctypes.data_as(C.c_void_p),
                            hnom.ctypes.data_as(C.c_void_p), None, None, None, None) == INVALID
    assert "device buffers" in lib.qs_last_error().decode()
    obs = np.empty((8, 12), np.float32)
    assert lib.qs_reset(h, None, obs.ctypes.data_as(C.c_void_p)) == 0 and np.isfinite(obs).all()
    lib.qs_destroy(h)
