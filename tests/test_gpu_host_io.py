"""-m gpu: every entry point that serves a QS_IO_HOST handle, against a QS_IO_DEVICE handle of the same configuration.

Both handles run the same kernels on the same values; only the way the caller's buffers reach the kernels differs (UserIO,
csrc/host_util.hpp).  So every comparison is bit for bit.  Each case runs at n = 8 (the kernels work in the mapped mirror in
place), n = 65 (one lane into a second tile), n = 8192 (every call moves more than kDirectBytes = 64 KiB -- the smallest one,
qs_set_params / qs_get_params, 128 KiB -- and the calls up to kMirrorBytes = 1 MiB take one DMA each way through the mirror) and
n = 131072 (every call moves more than that -- qs_get_params 2 MiB -- and copies between the caller's arrays and the device)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (8, 65, 8192, 131072)
SEED, OFFSET = 11, 5
SENTINEL = np.float32(-7777.0)


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


class Pair:
    """a raw QS_IO_HOST handle and a VecDockingEnv (device I/O) of the same configuration, seed and env_id_offset"""

    def __init__(self, qa, n):
        self.qa, self.n = qa, n
        self.lib = qa._lib.load()
        self.env = qa.VecDockingEnv("docking-v0", num_envs=n, auto_reset=True, randomise=1, seed=SEED, env_id_offset=OFFSET,
                                    init_range=qa.C3_INIT_RANGE)
        cfg = qa._lib.default_config()
        cfg.kind, cfg.num_envs, cfg.io_space, cfg.auto_reset = qa._lib.KIND_V0, n, qa._lib.IO_HOST, 1
        cfg.randomise, cfg.seed, cfg.env_id_offset = 1, SEED, OFFSET
        cfg.init_range = (C.c_float * 4)(*qa.C3_INIT_RANGE)
        self.h = C.c_void_p()
        qa._lib.check(self.lib.qs_create(C.byref(cfg), C.byref(self.h)), "qs_create")

    def close(self):
        self.lib.qs_destroy(self.h)
        self.env.close()

    def call(self, name, *args):
        return call_both(self.qa, self.h, self.env._h, name, *args)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def call_both(qa, h_host, h_dev, name, *args):
    """lib.<name>(handle, *args) on the host handle with the numpy arrays among args, and on the device handle with device
    copies of them.  Asserts that every array -- inputs, outputs, in-outs -- is the same bit for bit afterwards and returns
    the host handle's arguments."""
    import torch
    fn = getattr(qa._lib.load(), name)
    host = [np.ascontiguousarray(a).copy() if isinstance(a, np.ndarray) else a for a in args]
    dev = [torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a for a in host]
    qa._lib.check(fn(h_host, *[a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a for a in host]), name + " (host)")
    torch.cuda.current_stream().synchronize()            # the device copies of the inputs are complete
    qa._lib.check(fn(h_dev, *[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in dev]), name + " (device)")
    qa._lib.check(qa._lib.load().qs_sync(h_dev), "qs_sync")
    for i, (a, d) in enumerate(zip(host, dev)):
        if isinstance(a, np.ndarray):
            assert bits_equal(a, d.cpu().numpy()), "%s: argument %d differs between the host and the device handle" % (name, i)
    return host


def f32(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


@pytest.fixture(params=SIZES)
def pair(qa, request):
    p = Pair(qa, request.param)
    yield p
    p.close()


def reset_both(p):
    obs = p.call("qs_reset", None, np.full((p.n, 12), SENTINEL))[1]
    assert not (obs == SENTINEL).any()
    return obs


@pytest.mark.parametrize("staged", [True, False])
def test_rollout(pair, staged):
    p, n, T = pair, pair.n, 3
    reset_both(p)
    t = np.zeros(n, np.float32)
    t[::3] = 598.0                                       # a third of the envs run out of time inside the window: auto-reset
    p.call("qs_set_state", None, None, None, None, None, t)
    acts = p.call("qs_fill_random_actions", T, 0, np.zeros((T, n, 4), np.float32))[2] if staged else None
    out = p.call("qs_rollout", T, acts, np.full((T, n, 12), SENTINEL), np.full((T, n), SENTINEL),
                 np.full((T, n), 0xAB, np.uint8), np.full((T, n), 0xAB, np.uint8))
    obs, rew, done, flags = out[2:]
    assert not (obs == SENTINEL).any() and not (rew == SENTINEL).any()
    assert set(np.unique(done)) == {0, 1} and done[:, ::3].any(axis=0).all() and not done.all(axis=0).any()
    assert ((flags[:, ::3] & 4) != 0).any(axis=0).all()


def test_fill_random_actions(pair):
    T = 3
    a = pair.call("qs_fill_random_actions", T, 5, np.full((T, pair.n, 4), SENTINEL))[2]
    assert (np.abs(a) <= 1.0).all() and len(np.unique(a)) > pair.n


def test_params_round_trip(pair):
    p, n = pair, pair.n
    rng = np.random.RandomState(n)

    def get():
        out = p.call("qs_get_params", np.full(n, SENTINEL), np.full((n, 3), SENTINEL))
        return out[0], out[1]

    m0, i0 = get()
    assert (m0 == np.float32(0.18)).all() and not (i0 == SENTINEL).any()
    m1 = (0.18 + 0.05 * f32(rng, n)).astype(np.float32)
    p.call("qs_set_params", m1, None)
    m, i = get()
    assert bits_equal(m, m1) and bits_equal(i, i0)       # a null inertia leaves the inertia as it was
    i1 = (2.5e-4 + 1e-4 * f32(rng, n, 3)).astype(np.float32)
    p.call("qs_set_params", None, i1)
    m, i = get()
    assert bits_equal(m, m1) and bits_equal(i, i1)       # ... and a null mass the mass
    m2, i2 = (m1 * np.float32(1.25)).astype(np.float32), (i1 * np.float32(0.75)).astype(np.float32)
    p.call("qs_set_params", m2, i2)
    m, i = get()
    assert bits_equal(m, m2) and bits_equal(i, i2)
    m_only = p.call("qs_get_params", np.full(n, SENTINEL), None)[0]
    assert bits_equal(m_only, m2)


STATE_WORDS = (13, 13, 8, 4, 1, 1)


def get_state(p):
    return p.call("qs_get_state", *[np.full((p.n, w) if w > 1 else (p.n,), SENTINEL) for w in STATE_WORDS])


def test_state_round_trip(pair):
    p, n = pair, pair.n
    rng = np.random.RandomState(n)
    reset_both(p)
    s0 = get_state(p)
    assert not any((a == SENTINEL).any() for a in s0)
    chaser, t = f32(rng, n, 13), (100.0 * np.abs(f32(rng, n))).astype(np.float32)
    p.call("qs_set_state", chaser, None, None, None, None, t)
    s1 = get_state(p)
    assert bits_equal(s1[0], chaser) and bits_equal(s1[5], t)
    for k in (1, 2, 3, 4):                               # the fields that were not given are unchanged
        assert bits_equal(s1[k], s0[k])
    u_prev, qdes = f32(rng, n, 8), f32(rng, n, 4)
    p.call("qs_set_state", None, None, u_prev, qdes, None, None)
    part = p.call("qs_get_state", None, np.full((n, 13), SENTINEL), np.full((n, 8), SENTINEL), None, None, np.full(n, SENTINEL))
    assert bits_equal(part[1], s0[1]) and bits_equal(part[2], u_prev) and bits_equal(part[5], t)
    s2 = get_state(p)
    assert bits_equal(s2[0], chaser) and bits_equal(s2[3], qdes) and bits_equal(s2[4], s0[4])


def test_step_ex_keeps_terminal_rows_of_unfinished_envs(pair):
    p, n = pair, pair.n
    reset_both(p)
    chaser = get_state(p)[0]
    chaser[1::2, 0] += 10.0                              # every second env is out of bounds: it finishes at the next step
    p.call("qs_set_state", chaser, None, None, None, None, None)
    out = p.call("qs_step_ex", np.zeros((n, 4), np.float32), np.full((n, 12), SENTINEL), np.full(n, SENTINEL),
                 np.full(n, 0xAB, np.uint8), np.full(n, 0xAB, np.uint8), np.full((n, 12), SENTINEL), np.full((n, 26), SENTINEL))
    obs, rew, done, flags, term, tstate = out[1:]
    assert done[1::2].all() and not done[0::2].any() and ((flags[1::2] & 2) != 0).all()
    assert not (obs == SENTINEL).any() and not (rew == SENTINEL).any()
    assert (term[0::2] == SENTINEL).all() and (tstate[0::2] == SENTINEL).all()       # unfinished rows: the caller's values
    assert not (term[1::2] == SENTINEL).any() and not (tstate[1::2] == SENTINEL).any()
    assert (tstate[1::2, 0] > 5.0).all()                 # finished rows carry the terminal state, not the reset one
    # without the optional outputs: the same obs / reward / done
    p.call("qs_set_state", chaser, None, None, None, None, None)
    p.call("qs_step_ex", np.zeros((n, 4), np.float32), np.zeros((n, 12), np.float32), np.zeros(n, np.float32),
           np.zeros(n, np.uint8), None, None, None)


def test_masked_reset_keeps_rows_of_other_envs(pair):
    p, n = pair, pair.n
    reset_both(p)
    p.call("qs_step_ex", np.full((n, 4), 0.5, np.float32), np.zeros((n, 12), np.float32), np.zeros(n, np.float32),
           np.zeros(n, np.uint8), None, None, None)
    mask = np.zeros(n, np.uint8)
    mask[::3] = 1
    obs = p.call("qs_reset", mask, np.full((n, 12), SENTINEL))[1]
    assert not (obs[::3] == SENTINEL).any()
    assert (np.delete(obs, np.s_[::3], axis=0) == SENTINEL).all()
    assert p.lib.qs_reset(p.h, mask.ctypes.data_as(C.c_void_p), None) == 0            # no output at all


# ---------------------------------------------------------------- layer 1: the host context of quadsim_amd.drone
@pytest.fixture(scope="module")
def layer1(qa):
    env = qa.VecDockingEnv("docking-v0", num_envs=1)
    yield lambda name, *args: call_both(qa, qa.drone._context(), env._h, name, *args)
    env.close()


def states(rng, n):
    s = f32(rng, n, 13)
    s[:, 6:10] /= np.linalg.norm(s[:, 6:10], axis=1, keepdims=True)
    return s


@pytest.mark.parametrize("n", SIZES)
def test_layer1_drone_step_and_ctrl(layer1, n):
    rng = np.random.RandomState(n)
    s, up, u = states(rng, n), f32(rng, n, 4), f32(rng, n, 4)
    par = np.tile(np.array([0.2, 2.6e-4, 2.4e-4, 3.8e-4], np.float32), (n, 1))
    out = layer1("qs_drone_step", n, s, up, u, None, np.full(n, 0xAB, np.uint8))
    assert not bits_equal(out[1], s) and set(np.unique(out[5])) <= {0, 1}
    out_par = layer1("qs_drone_step", n, s, up, u, par, None)
    assert not bits_equal(out_par[1], out[1])
    sd, last = states(rng, n), states(rng, n)
    for mode, sl in ((0, None), (0, last), (1, last)):
        o = layer1("qs_ctrl", n, mode, sd, s, sl, 0.18, np.full((n, 4), SENTINEL))
        assert not (o[6] == SENTINEL).any() and (o[2][:, 10:12] == 0).all() and bits_equal(o[2][:, :6], sd[:, :6])


@pytest.mark.parametrize("n", SIZES)
def test_layer1_transforms_and_rel_obs(layer1, n):
    rng = np.random.RandomState(n)
    q = states(rng, n)[:, 6:10].copy()
    for op, x, wo in ((0, q, 3), (1, f32(rng, n, 3), 4), (2, q, 9), (3, f32(rng, n, 9), 3)):
        o = layer1("qs_transform", op, n, x, np.full((n, wo), SENTINEL))
        assert not (o[3] == SENTINEL).any()
    o = layer1("qs_rel_obs", n, states(rng, n), states(rng, n), np.full((n, 12), SENTINEL))
    assert not (o[3] == SENTINEL).any()
