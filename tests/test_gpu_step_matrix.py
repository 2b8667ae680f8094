"""-m gpu: every instantiation of the env-step kernels (one row of tests/step_matrix.py each) against the float64 oracle.

Per row: a handle at the row's edges (ragged env count; on the rocRAND rows env ids and step counters that cross 32 bits
inside the window; per-env parameters drawn per env; distinct per-env stored initial states; a fifth of the envs timing out on
even and odd steps), checked to launch the row's instantiation (qs_debug_step_variant), then
  1. T single steps, each against the oracle started from the kernel's own pre-step state and parameters: outputs, flags,
     post-step state, parameters, step counter, and the terminal rows against an oracle step without the reset;
  2. a twin handle runs the same actions through the multi-step path -- the fused roll-out (the kernel's T-loop, state in
     registers), or for the resident rows T undrained private-queue steps of one resident dispatch -- and must equal 1. bit
     for bit, final state included.
Tolerances and knife-edge exclusions are those of tests/helpers.py and test_vec_step_vs_oracle_random_resets."""
import ctypes as C

import numpy as np
import pytest

from helpers import OBS_TOL, STATE_TOL, reward_atol, state_to_rec, threshold_margin
from oracle.pyoracle import RR_NONE, Oracle
from step_matrix import HOVER, RESIDENT, ROCRAND_GID0, ROCRAND_K0, STEP_ROWS

pytestmark = pytest.mark.gpu

T = 8
TAIL = 2048                     # large handles: the oracle runs on the first and the last TAIL envs
RR = (0.5, 0.1, 0.2, 0.1, 0.8, 1.2, 0.8, 1.2)     # init_range (C3_INIT_RANGE), mass_scale, inertia_scale
PAR_NOM = np.array([0.18, 0.00025, 0.000232, 0.0003738])


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def orc():
    return Oracle("f64")


def step_variant(env):
    lib = env._lib
    lib.qs_debug_step_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 5)()
    assert lib.qs_debug_step_variant(env._h, out) == 0, lib.qs_last_error()
    return tuple(out)


def _dispatches(env):
    env._lib.qs_debug_chain_resident.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    d = C.c_uint64(0)
    assert env._lib.qs_debug_chain_resident(env._h, C.byref(d)) == 0
    return int(d.value)


class Outs:
    """distinct output buffers for each of T steps; terminal rows seeded with a pattern that rows of envs that do not finish keep"""
    def __init__(self, torch, n, od, hover):
        kw = dict(device="cuda")
        self.obs = torch.empty((T, n, od), dtype=torch.float32, **kw)
        self.rew = torch.empty((T, n), dtype=torch.float32, **kw)
        self.done = torch.empty((T, n), dtype=torch.uint8, **kw)
        self.flags = torch.empty((T, n), dtype=torch.uint8, **kw)
        self.term = torch.full((T, n, od), -7.0, dtype=torch.float32, **kw)
        self.tstate = None if hover else torch.full((T, n, 26), -9.0, dtype=torch.float32, **kw)

    def args(self, k):
        p = lambda t: None if t is None else C.c_void_p(t[k].data_ptr())     # noqa: E731
        return tuple(p(t) for t in (self.obs, self.rew, self.done, self.flags, self.term, self.tstate))

    def all(self):
        return [t for t in (self.obs, self.rew, self.done, self.flags, self.term, self.tstate) if t is not None]


def _init_states(rng, orc, n):
    """distinct per-env initial states around the nominal start: chaser | target [n,13] each"""
    rec = orc.env_init(n)
    out = []
    for lo, hi in ((0, 13), (13, 26)):
        s = rec[:, lo:hi].copy()
        s[:, 0:3] += rng.uniform(-0.5, 0.5, (n, 3))
        s[:, 3:6] += rng.uniform(-0.1, 0.1, (n, 3))
        q = s[:, 6:10] + rng.uniform(-0.05, 0.05, (n, 4))
        s[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
        s[:, 10:13] += rng.uniform(-0.1, 0.1, (n, 3))
        out.append(s.astype(np.float32))
    return out


def _make(qa, orc, row, seed):
    """the row's handle, set up identically for every call with the same seed"""
    n = row["n"]
    kw = dict(num_envs=n, integrator=row["integ"], dt=row["dt"], randomise=row["randomise"], seed=seed, copy=False,
              env_id_offset=ROCRAND_GID0 if row["rocrand"] else 977)
    if row["randomise"]:
        kw.update(init_range=RR[:4], mass_scale=RR[4:6], inertia_scale=RR[6:8])
    env = qa.VecDockingEnv(row["env_id"], **kw)
    rng = np.random.default_rng(seed)
    if row["set_init"]:
        env.set_init_state(*_init_states(rng, orc, n))
    env.reset()
    if row["set_params"]:
        env.set_params(mass=(0.18 * rng.uniform(0.85, 1.15, n)).astype(np.float32),
                       inertia=(PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))
    idx = np.arange(0, n, 5)
    if row["env_id"] == "hovering-v0":
        c = env.get_state()["chaser"]
        c[idx, 0:3] += 99.0                                  # a fifth start near the |pos| > 100 limit
        env.set_state(chaser=c)
    else:
        t0 = np.zeros(n, np.float32)
        t0[idx] = 593.0 + (idx // 5) % 7                     # a fifth time out within the window, on even and odd steps
        env.set_state(t=t0)
    if row["rocrand"]:
        env.step_counter = ROCRAND_K0
    if row["queues"]:
        env.set_queue_mode(True, row["queues"], ordering=row["ordering"])
        assert env.queue_ordering == row["ordering"]
    assert step_variant(env) == tuple(row["variant"]), (step_variant(env), row["variant"])
    return env


def _actions(torch, row, seed):
    rng = np.random.default_rng(seed + 1)
    lo = 0.0 if row["env_id"] == "hovering-v0" else -1.0
    a = rng.uniform(lo, 1.0, (T, row["n"], 4)).astype(np.float32)
    return a, torch.from_numpy(a).cuda()


def _blocks(n):
    return [(0, n)] if n <= 4 * TAIL else [(0, TAIL), (n - TAIL, n)]


def _full_state(env):
    st = env.get_state()
    return np.concatenate([st[k].reshape(len(st["t"]), -1) for k in sorted(st)], 1)


def _check_docking(orc, row, seed, k, rec, par, init, kk, a, o_k, st2, par2):
    """step k of the handle (device outputs o_k, post-step state st2 / params par2) against the oracle"""
    kind = 1 if row["env_id"] == "docking-v2" else 0
    integ = 1 if row["integ"] == "rk4" else 0
    dt = float(np.float32(row["dt"]))
    rnd = row["randomise"]
    gid0 = ROCRAND_GID0 if row["rocrand"] else 977
    rmax = 3.0 if kind == 0 else 10.0
    obs, rew, done, flags, term, tstate = o_k
    rec2 = state_to_rec(st2)
    for lo, hi in _blocks(len(rec)):
        r, p = rec[lo:hi].copy(), par[lo:hi].copy()
        rn, pn = rec[lo:hi].copy(), par[lo:hi].copy()
        if row["variant"][3] == 3:
            o, rw, d, f, tm = orc.vec_step_stored_init(r, p, a[lo:hi], init[lo:hi], kind=kind, dt=dt, integ=integ, want_term=True)
            o2, _, d2, _, _ = orc.vec_step_stored_init(rn, pn, a[lo:hi], init[lo:hi], kind=kind, dt=dt, integ=integ,
                                                       auto_reset=False)
        else:
            kw = dict(kind=kind, dt=dt, integ=integ, randomise=rnd, seed=seed, step_idx=kk, gid0=gid0 + lo,
                      rr=RR if rnd else RR_NONE)
            o, rw, d, f, tm = orc.vec_step(r, p, a[lo:hi], want_term=True, **kw)
            o2, _, d2, _, _ = orc.vec_step(rn, pn, a[lo:hi], auto_reset=False, **kw)
        db = d.astype(bool)
        assert np.array_equal(db, d2.astype(bool))
        pre = rec[lo:hi]
        t_obs = np.where(db[:, None], tm, o)
        safe = threshold_margin(t_obs, np.where(db, 1.0, pre[:, 2]), pre[:, 39], rmax) > 1e-4
        safe &= np.abs(pre[:, 2] - 0.1) > 5e-2          # chaser z crossing 0.1 is decided on the post-step z
        assert safe.mean() > 0.97, (k, lo, safe.mean())
        dn = done[lo:hi].astype(bool)
        assert np.array_equal(dn[safe], db[safe]), (k, lo)
        same = safe & (dn == db)
        np.testing.assert_allclose(obs[lo:hi][same], o[same], **OBS_TOL)
        shp = reward_atol(pre[same, 38]) + reward_atol(rw[same])
        assert np.all(np.abs(rew[lo:hi][same] - rw[same]) <= shp), k
        assert np.array_equal(flags[lo:hi][same] & 7, f[same] & 7), k
        assert np.array_equal(flags[lo:hi][same] & 24, f[same] & 24), k          # attitude limiter bits
        post = rec2[lo:hi]
        np.testing.assert_allclose(post[same][:, :38], r[same][:, :38], **STATE_TOL)
        assert np.all(np.abs(post[same, 38] - r[same, 38]) <= shp), k            # last_shaping: the reward's bound
        assert np.array_equal(post[same, 39], r[same, 39]), k
        # parameters: untouched where no episode ended; RMODE 2 redraws them exactly where one did
        pm = par2[lo:hi]
        assert np.array_equal(pm[~dn], par[lo:hi][~dn]), k
        np.testing.assert_allclose(pm[same], p[same], rtol=1e-6)
        if rnd == 2 and (same & db).any():
            assert np.all(np.any(pm[same & db] != par[lo:hi][same & db], axis=1)), k
        # terminal rows: the oracle's terminal quantities and an oracle step without the reset; other rows keep the pattern
        fin = same & db
        np.testing.assert_allclose(term[lo:hi][fin], tm[fin], **OBS_TOL)
        np.testing.assert_allclose(term[lo:hi][fin], o2[fin], **OBS_TOL)
        np.testing.assert_allclose(tstate[lo:hi][fin], rn[fin][:, :26], **STATE_TOL)
        assert np.all(term[lo:hi][~dn] == -7.0) and np.all(tstate[lo:hi][~dn] == -9.0), k
    return int(done.sum())


def _check_hover(orc, row, k, s17, par, init, a, o_k, st2, par2):
    integ = 1 if row["integ"] == "rk4" else 0
    dt = float(np.float32(row["dt"]))
    obs, rew, done, flags, term, _ = o_k
    for lo, hi in _blocks(len(s17)):
        s, sn = s17[lo:hi].copy(), s17[lo:hi].copy()
        o, rw, d, f, tm = orc.hover_vec_step(s, par[lo:hi], a[lo:hi], init[lo:hi], dt=dt, integ=integ, want_term=True)
        o2, _, d2, _, _ = orc.hover_vec_step(sn, par[lo:hi], a[lo:hi], init[lo:hi], dt=dt, integ=integ, auto_reset=False)
        db = d.astype(bool)
        pre_pos = np.linalg.norm(np.where(db[:, None], tm[:, 0:3], o[:, 0:3]), axis=1)
        safe = np.abs(pre_pos - 100.0) > 1e-3
        assert safe.mean() > 0.97, (k, safe.mean())
        dn = done[lo:hi].astype(bool)
        assert np.array_equal(dn[safe], db[safe]), k
        same = safe & (dn == db)
        np.testing.assert_allclose(obs[lo:hi][same], o[same], **STATE_TOL)
        np.testing.assert_allclose(rew[lo:hi][same], rw[same], rtol=0, atol=2e-5)
        assert np.array_equal(flags[lo:hi][same], f[same]), k
        np.testing.assert_allclose(st2["chaser"][lo:hi][same], s[same][:, :13], **STATE_TOL)
        np.testing.assert_allclose(st2["u_prev"][lo:hi][same][:, :4], s[same][:, 13:17], **STATE_TOL)
        assert np.array_equal(par2[lo:hi], par[lo:hi])
        fin = same & db
        np.testing.assert_allclose(term[lo:hi][fin], tm[fin], **STATE_TOL)
        np.testing.assert_allclose(term[lo:hi][fin], o2[fin], **STATE_TOL)
        assert np.all(term[lo:hi][~dn] == -7.0), k
    return int(done.sum())


def _params(env):
    m, I = env.get_params()
    return np.concatenate([m[:, None], I], axis=1).astype(np.float64)


@pytest.mark.parametrize("row", STEP_ROWS, ids=[r["id"] for r in STEP_ROWS])
def test_step_kernel_row(qa, torch, orc, row):
    seed = 1000 + STEP_ROWS.index(row)
    hover = row["variant"][0] == HOVER
    resident = row["variant"][0] == RESIDENT
    n = row["n"]
    a_np, acts = _actions(torch, row, seed)
    env = _make(qa, orc, row, seed)
    lib, h = env._lib, env._h
    od = env.obs_dim
    init = None
    if hover:
        init = env.get_init_state()[0].astype(np.float64)
    elif row["variant"][3] == 3:
        c, t = env.get_init_state()
        init = np.concatenate([c, t], axis=1).astype(np.float64)
        assert len(np.unique(init[:, 0:3], axis=0)) == n          # distinct per-env initial states
    outs = Outs(torch, n, od, hover)
    d0 = _dispatches(env)
    n_done = 0
    # 1. single steps against the oracle
    for k in range(T):
        st, par, kk = env.get_state(), _params(env), env.step_counter
        torch.cuda.synchronize()
        assert lib.qs_step_ex(h, C.c_void_p(acts[k].data_ptr()), *outs.args(k)) == 0, lib.qs_last_error()
        env.sync()
        torch.cuda.synchronize()
        st2, par2 = env.get_state(), _params(env)
        assert env.step_counter == kk + 1
        o_k = [t[k].cpu().numpy() for t in (outs.obs, outs.rew, outs.done, outs.flags, outs.term)]
        o_k.append(None if hover else outs.tstate[k].cpu().numpy())
        if hover:
            s17 = np.concatenate([st["chaser"], st["u_prev"][:, :4]], axis=1).astype(np.float64)
            n_done += _check_hover(orc, row, k, s17, par, init, a_np[k], o_k, st2, par2)
        else:
            n_done += _check_docking(orc, row, seed, k, state_to_rec(st), par, init, kk, a_np[k], o_k, st2, par2)
    assert n_done >= n // 10, n_done                          # the reset path ran
    if row["rocrand"]:
        assert env.step_counter == ROCRAND_K0 + T and env.step_counter >= 2 ** 32
    if resident:
        assert _dispatches(env) > d0, "the resident step kernel was not used"
    # 2. the multi-step path of a twin, bit for bit against the single steps
    twin = _make(qa, orc, row, seed)
    if resident:
        ob = Outs(torch, n, od, hover)
        d1 = _dispatches(twin)
        torch.cuda.synchronize()                              # host-ordered: the inputs are complete at the call
        for k in range(T):
            assert twin._lib.qs_step_ex(twin._h, C.c_void_p(acts[k].data_ptr()), *ob.args(k)) == 0, twin._lib.qs_last_error()
        twin.sync()
        torch.cuda.synchronize()
        assert _dispatches(twin) > d1, "the resident step kernel was not used"
        for x, y in zip(outs.all(), ob.all()):
            assert torch.equal(x, y)
    else:
        O, R, D, F = twin.rollout(acts)
        torch.cuda.synchronize()
        for x, y in zip((outs.obs, outs.rew, outs.done, outs.flags), (O, R, D, F)):
            assert torch.equal(x, y)
    np.testing.assert_array_equal(_full_state(env), _full_state(twin))
    np.testing.assert_array_equal(_params(env), _params(twin))
    assert env.step_counter == twin.step_counter
    env.close()
    twin.close()
