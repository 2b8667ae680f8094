"""-m gpu: every instantiation of the Runner kernels (k_runner_rollout, k_runner_split) and of the policy roll-out kernels
(k_policy_rollout, k_policy_rollout_fast), one row of tests/rollout_matrix.py each, run through the production dispatch.

Per row: two handles with identical arguments, `a` for the kernel under test and the twin `b`; per-env parameters where the row
says so; a fifth of the envs at t = 590..599 (time-outs on distinct steps inside T) and a fifth just inside the over-limit radius
flying outwards; one warm step with zero actions, whose observation is the one the roll-out acts on first.  The row is checked to
reach its own instantiation (qs_debug_rollout_variant), then

  env side   the twin is stepped T times with exactly what the kernel's env received (the Runner: clip(actions[t], -1, 1), rows
             are not squashed; the policy roll-out: the reported actions) and every next observation, reward, done flag and flag
             byte of the roll-out equals the twin's BIT FOR BIT, as do the final state, parameters and step counter.  The
             roll-outs' step is step_and_maybe_reset / env_step_target + env_step_chaser + maybe_reset, the functions the step
             kernels instantiate, and qs_step is tied to float64 for the same (INTEG, PARAMS, RMODE) by tests/step_matrix.py
             (tests/test_rollout_matrix_cpu.py asserts that such a row exists).  No row needed the per-step tolerances.
  network    at EVERY step, on the observations the kernel itself acted on, against the float64 network with the derived bounds
             of tests/actor_numerics.py: the Runner's samples against mean64 + std eps (the sample bound of
             test_fused_runner_within_bound), values / last_values within the value bound, neglogp within _neglogp_bound; a
             policy roll-out's clipped actions with check_clipped.  Tower rows use the tower weight set.
  noise      rows with in-kernel normals take eps from the oracle's float64 restatement of the draw,
             normal4(seed, env_id_offset + env, k0 + t), for every (t, env): the indexing of the noise stream for t > 0 and across
             in-loop resets.  The kernel evaluates the same Box-Muller formula in float32; the samples stay inside the
             same bound all the same (worst 0.29 of it, against 0.30 with caller noise).

The conditions on the inputs are checked on the twin's outputs: a tenth of the envs end an episode inside T, one before the last
step, and (rows with n >= 30, T > 1: at least one in every (INTEG, RMODE) group) both the over-limit and the time-out reset ran."""
import ctypes as C

import numpy as np
import pytest

import actor_numerics as an
from actor_numerics import _neglogp64, _neglogp_bound
from rollout_matrix import NETS, POLICY_ROWS, PRECISIONS, RUNNER_ROWS

pytestmark = pytest.mark.gpu

PAR_NOM = np.array([0.18, 0.00025, 0.000232, 0.0003738])
GID0 = 977                       # env_id_offset of every handle: the noise stream is keyed by GID0 + env


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def nets(qa):
    """{net: (float64-able weight dict, ActorCriticPolicy)} of the shipped checkpoints, and the v0 actor of the policy rows"""
    Wv0, Wtow = an.weights_v0(), an.weights_towers()
    out = {"shared": (Wv0, qa.ActorCriticPolicy(Wv0)), "towers": (Wtow, qa.load_sb2_model(an.TOWERS_ZIP))}
    assert not out["shared"][1].towers and out["towers"][1].towers
    out["actor"] = (Wv0, qa.MlpPolicy({k: Wv0[k] for k in ("w0", "b0", "w1", "b1", "w2", "b2")}))
    return out


def _variant(env, family, fast, layout):
    lib = env._lib
    lib.qs_debug_rollout_variant.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 6)()
    assert lib.qs_debug_rollout_variant(env._h, family, fast, layout, out) == 0, lib.qs_last_error()
    return tuple(out)


def _make(qa, torch, row, seed):
    """the row's handle, identical for every call with the same arguments -> (env, the observation of its current state)"""
    n = row["n"]
    kw = dict(num_envs=n, integrator=row["integ"], dt=row["dt"], randomise=row["randomise"], seed=seed, env_id_offset=GID0)
    if row["randomise"]:
        kw.update(init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2))
    env = qa.VecDockingEnv(row["env_id"], **kw)
    rng = np.random.default_rng(seed)
    env.reset()
    if row["set_params"]:
        env.set_params(mass=(0.18 * rng.uniform(0.85, 1.15, n)).astype(np.float32),
                       inertia=(PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))
    st = env.get_state()
    idx = np.arange(n)
    t0 = st["t"].copy()
    timed = idx % 5 == 0
    t0[timed] = 590.0 + (idx[timed] // 5) % 10                           # time-outs on distinct steps (599: in the warm step)
    far = idx % 5 == 1
    rmax = 10.0 if row["env_id"] == "docking-v2" else 3.0
    c = st["chaser"].copy()
    gap = 0.03 + 0.04 * ((idx[far] // 5) % 6)                            # port-to-port distance rmax - gap, 2 m/s outwards
    c[far, 0] = st["target"][far, 0] - 0.2 - rmax + gap
    c[far, 1:3] = st["target"][far, 1:3]
    c[far, 3:6] = np.array([-2.0, 0.0, 0.0], np.float32)
    c[far, 6:10] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    c[far, 10:13] = 0.0
    env.set_state(chaser=c, t=t0)
    obs, _, _, _ = env.step(torch.zeros((n, 4), device=env.device))      # the warm step: step counter 1 afterwards
    return env, obs.clone()


def _same(torch, got, ref, what):
    if not torch.equal(got, ref):
        g, r = got.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
        bad = g != r
        raise AssertionError("%s: %d of %d elements differ from the per-step loop, worst |diff| %.3g, first at %s" % (
            what, int(bad.sum()), bad.size, float(np.abs(g - r)[bad].max()), tuple(np.argwhere(bad)[0])))


def _same_handle(a, b):
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), "final state: " + k
    for x, y, k in zip(a.get_params(), b.get_params(), ("mass", "inertia")):
        assert np.array_equal(x, y), "final parameters: " + k
    assert a.step_counter == b.step_counter


def _input_conditions(row, done, flags):
    """on the twin's records done [T,n] bool / flags [T,n] u8"""
    n, T = row["n"], row["T"]
    if T > 1 and n >= 10:
        assert done.any(axis=0).sum() * 10 >= n, done.any(axis=0).sum()
        assert done[:-1].any()
    if T > 1 and n >= 30:
        assert ((flags & 2) != 0).any() and ((flags & 4) != 0).any()      # both the over-limit and the time-out reset ran
        assert np.all(done[(flags & 6) != 0])


def _params_before(env):
    m, inertia = env.get_params()
    return np.asarray(m).copy(), np.asarray(inertia).copy()


@pytest.mark.parametrize("row", RUNNER_ROWS, ids=[r["id"] for r in RUNNER_ROWS])
def test_runner_row(qa, torch, oracle64, nets, row):
    seed = 2000 + RUNNER_ROWS.index(row)
    n, T, prec = row["n"], row["T"], row["precision"]
    W, pol = nets[row["net"]]
    fast, layout = PRECISIONS.index(prec), NETS.index(row["net"])
    a, obs0 = _make(qa, torch, row, seed)
    b, obs0b = _make(qa, torch, row, seed)
    assert torch.equal(obs0, obs0b)
    par0 = _params_before(a)
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn((T, n, 4), generator=g) if row["noise"] == "caller" else None
    dones_in = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    k0 = a.step_counter
    assert k0 == 1
    lib = a._lib
    lib.qs_debug_set_runner_serial.argtypes = [C.c_int]
    before = lib.qs_debug_set_runner_serial(row["serial"])
    try:
        assert _variant(a, 0, fast, layout) == tuple(row["variant"]), (_variant(a, 0, fast, layout), row["variant"])
        ro = qa.fused_runner_rollout(a, pol, T, noise=noise, dones_in=dones_in, want_flags=True, precision=prec)
        torch.cuda.synchronize()
    finally:
        lib.qs_debug_set_runner_serial(before)

    # ---- env side: the twin's per-step loop on what the kernel's env received, bit for bit
    _same(torch, ro["obs"][0], obs0, "obs[0]")
    assert torch.equal(ro["dones"][0], dones_in.to(a.device))
    D, F = [], []
    for t in range(T):
        o, r, d, _ = b.step(torch.clamp(ro["actions"][t], -1.0, 1.0))
        last = t + 1 == T
        _same(torch, ro["last_obs"] if last else ro["obs"][t + 1], o, "observation after step %d" % t)
        _same(torch, ro["rewards"][t], r, "rewards[%d]" % t)
        _same(torch, ro["last_dones"] if last else ro["dones"][t + 1], d.to(torch.uint8), "done flag after step %d" % t)
        _same(torch, ro["flags"][t], b.last_flags, "flags[%d]" % t)
        D.append(d.cpu().numpy().copy()); F.append(b.last_flags.cpu().numpy().copy())
    _same_handle(a, b)
    assert a.step_counter == k0 + T
    D, F = np.stack(D), np.stack(F)
    _input_conditions(row, D, F)
    if row["randomise"] == 2 and D.any():
        ended = D.any(axis=0)
        assert np.all(a.get_params()[0][ended] != par0[0][ended])        # per-episode parameters were redrawn and stored

    # ---- network side: float64 at every step on the observations the kernel acted on
    R = {k: v.cpu().numpy() for k, v in ro.items() if v is not None}
    obs = R["obs"].reshape(T * n, 12)
    m64, v64 = an.net64(W, obs)
    Em, Ev = an.err_scale(W, obs)
    mb = an.bound(Em, prec)
    std = np.exp(np.asarray(W["logstd"], np.float32).astype(np.float64)).reshape(1, 4)
    u32 = an.KAPPA["f32"] * an.UNIT["f32"]
    if noise is not None:
        e = noise.numpy().astype(np.float64).reshape(T * n, 4)
    else:
        e = np.stack([oracle64.normal4(seed, GID0 + i, k0 + t) for t in range(T) for i in range(n)]).astype(np.float64)
    u64 = m64 + std * e
    ub = mb + u32 * (np.abs(u64) + std * np.abs(e))
    du = np.abs(R["actions"].reshape(T * n, 4) - u64)
    tag = "%s %s" % (row["id"], row["noise"])
    worst_v = an.check_unclipped(R["values"].reshape(-1), v64, Ev, prec, "runner value " + tag)
    nl64 = _neglogp64(W, u64, e, False)
    nb = _neglogp_bound(W, u64, m64, e, mb, False)
    dn = np.abs(R["neglogp"].reshape(-1) - nl64)
    print("%s: sample err / bound %.3f, value ratio %.3f of kappa %.3g, neglogp err / bound %.3f" % (
        tag, (du / ub).max(), worst_v, an.KAPPA[prec], (dn / nb).max()))
    assert (du <= ub).all(), ("runner sample " + tag, float((du / ub).max()))
    assert (dn <= nb).all(), ("runner neglogp " + tag, float((dn / nb).max()))
    lo = R["last_obs"]
    an.check_unclipped(R["last_values"], an.net64(W, lo)[1], an.err_scale(W, lo)[1], prec, "runner last value " + tag)
    a.close(); b.close()


@pytest.mark.parametrize("row", POLICY_ROWS, ids=[r["id"] for r in POLICY_ROWS])
def test_policy_rollout_row(qa, torch, nets, row):
    seed = 3000 + POLICY_ROWS.index(row)
    n, T, prec = row["n"], row["T"], row["precision"]
    W, pol = nets["actor"]
    a, obs0 = _make(qa, torch, row, seed)
    b, obs0b = _make(qa, torch, row, seed)
    assert torch.equal(obs0, obs0b)
    k0 = a.step_counter
    assert _variant(a, 1, PRECISIONS.index(prec), 0) == tuple(row["variant"]), (_variant(a, 1, PRECISIONS.index(prec), 0), row["variant"])
    O, Rw, Dn, Fl, A = qa.fused_policy_rollout(a, pol, T, precision=prec)
    torch.cuda.synchronize()
    # ---- env side
    D, F = [], []
    for t in range(T):
        o, r, d, _ = b.step(A[t])
        _same(torch, O[t], o, "obs[%d]" % t)
        _same(torch, Rw[t], r, "rewards[%d]" % t)
        _same(torch, Dn[t], d.to(torch.uint8), "dones[%d]" % t)
        _same(torch, Fl[t], b.last_flags, "flags[%d]" % t)
        D.append(d.cpu().numpy().copy()); F.append(b.last_flags.cpu().numpy().copy())
    _same_handle(a, b)
    assert a.step_counter == k0 + T
    _input_conditions(row, np.stack(D), np.stack(F))
    # ---- network side: the actor on the observation of the current state, then on each step's own output
    acted = torch.cat([obs0[None], O[:-1]]).cpu().numpy().reshape(T * n, 12)
    worst, free = an.check_clipped(A.cpu().numpy().reshape(T * n, 4), an.net64(W, acted)[0], an.err_scale(W, acted)[0], prec,
                                   "policy roll-out " + row["id"])
    print("%s: action ratio %.3f of kappa %.3g, unclipped fraction %.2f" % (row["id"], worst, an.KAPPA[prec], free))
    a.close(); b.close()


def test_step_policy_is_the_policy_rollout_with_one_step(qa, torch, nets):
    """VecDockingEnv.step_policy against qs_policy_rollout with T = 1 on a twin, bit for bit, on an rk4 rocRAND row"""
    row = [r for r in POLICY_ROWS if r["combo"] == (1, 0, 1) and r["precision"] == "f32"][0]
    W, pol = nets["actor"]
    a, _ = _make(qa, torch, row, 5)
    b, _ = _make(qa, torch, row, 5)
    for _ in range(3):
        o, r, d, act = a.step_policy(pol)
        O, Rw, Dn, Fl, A = qa.fused_policy_rollout(b, pol, 1)
        for x, y, k in ((o, O[0], "obs"), (r, Rw[0], "reward"), (d.to(torch.uint8), Dn[0], "done"), (a.last_flags, Fl[0], "flags"),
                        (act, A[0], "actions")):
            _same(torch, x, y, k)
    _same_handle(a, b)
    a.close(); b.close()


def test_runner_still_refuses_stored_initial_states(qa, torch, nets):
    """docking-v1 (stored initial states, RMODE 3) has no Runner kernel: the launch and qs_debug_rollout_variant refuse it with
    the same message and leave the handle usable"""
    env = qa.VecDockingEnv("docking-v1", num_envs=70, seed=1)
    env.reset()
    with pytest.raises(qa._lib.QuadsimError, match="no stored initial states"):
        qa.fused_runner_rollout(env, nets["shared"][1], 2)
    out = (C.c_int32 * 6)(*([7] * 6))
    env._lib.qs_debug_rollout_variant.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    assert env._lib.qs_debug_rollout_variant(env._h, 0, 0, 0, out) != 0 and list(out) == [7] * 6
    assert b"no stored initial states" in env._lib.qs_last_error()
    k = env.step_counter
    obs, _, _, _ = env.step(torch.zeros((70, 4), device=env.device))
    assert bool(torch.isfinite(obs).all()) and env.step_counter == k + 1
    env.close()
