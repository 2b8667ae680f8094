"""-m gpu: host-ordered private-queue steps through the resident step kernel (k_env_resident: one dispatch per queue, a
descriptor ring the host writes per step) == the HIP-stream chain, bit for bit: every output of every step, terminal rows and
states, the final state and the step counter.  Every step writes its own output buffers, so each step is shown to write
exactly where its descriptor said."""
import ctypes as C
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _full_state(env):
    st = env.get_state()
    return np.concatenate([st["chaser"], st["target"], st["u_prev"], st["qdes"], st["last_shaping"][:, None], st["t"][:, None]], 1)


def _dispatches(lib, env):
    lib.qs_debug_chain_resident.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    d = C.c_uint64(0)
    assert lib.qs_debug_chain_resident(env._h, C.byref(d)) == 0
    return int(d.value)


class Outs:
    """distinct output buffers for each of T steps; term_obs / term_state seeded with a pattern (rows of envs that do not
    finish keep it)"""
    def __init__(self, torch, T, n, od):
        kw = dict(device="cuda")
        self.obs = torch.empty((T, n, od), dtype=torch.float32, **kw)
        self.rew = torch.empty((T, n), dtype=torch.float32, **kw)
        self.done = torch.empty((T, n), dtype=torch.uint8, **kw)
        self.flags = torch.empty((T, n), dtype=torch.uint8, **kw)
        self.term = torch.full((T, n, od), -7.0, dtype=torch.float32, **kw)
        self.tstate = torch.full((T, n, 26), -9.0, dtype=torch.float32, **kw)

    def args(self, k):
        p = lambda t: C.c_void_p(t.data_ptr())              # noqa: E731
        return (p(self.obs[k]), p(self.rew[k]), p(self.done[k]), p(self.flags[k]), p(self.term[k]), p(self.tstate[k]))

    def equal(self, torch, other):
        return all(torch.equal(x, y) for x, y in zip((self.obs, self.rew, self.done, self.flags, self.term, self.tstate),
                                                      (other.obs, other.rew, other.done, other.flags, other.term, other.tstate)))


def _pair(qa, n, env_id, rnd, queues, seed=21):
    kw = dict(num_envs=n, randomise=rnd, seed=seed, init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2),
              copy=False)
    a, b = qa.VecDockingEnv(env_id, **kw), qa.VecDockingEnv(env_id, **kw)
    b.set_queue_mode(True, queues, ordering="host")
    assert b.queue_ordering == "host"
    a.reset(); b.reset()
    t0 = np.zeros(n, np.float32); t0[::5] = 585.0            # a fifth of the envs time out inside the window: resets
    a.set_state(t=t0); b.set_state(t=t0)
    return a, b


def _steps(torch, env, acts, outs, ks, P):
    lib, h = env._lib, env._h
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    torch.cuda.synchronize()                                 # host-ordered: the inputs are complete at the call
    for k in ks:
        assert lib.qs_step_ex(h, p(acts[k % P]), *outs.args(k)) == 0, lib.qs_last_error()


@pytest.mark.parametrize("n,env_id,rnd,queues", [
    (1000, "docking-v2", 2, 1), (1000, "docking-v0", 1, 3), (4096, "docking-v0", 0, 2), (4096, "docking-v2", 2, 3),
    (65536, "docking-v0", 1, 1), (65536, "docking-v0", 1, 2), (65536, "docking-v0", 1, 3), (65536, "docking-v2", 2, 2)])
def test_resident_bit_identical_to_hip_stream(qa, torch, n, env_id, rnd, queues):
    """a roll-out with a draining call (get_state, sync) in the middle, then continued"""
    T, P = 24, 8
    a, b = _pair(qa, n, env_id, rnd, queues)
    lib = b._lib
    od = a.obs_dim
    acts = a.random_actions(P, step0=0)
    oa, ob = Outs(torch, T, n, od), Outs(torch, T, n, od)
    d0 = _dispatches(lib, b)
    _steps(torch, a, acts, oa, range(12), P)
    _steps(torch, b, acts, ob, range(12), P)
    np.testing.assert_array_equal(_full_state(a), _full_state(b))          # drains the resident roll-out mid-way
    assert a.step_counter == b.step_counter == 12
    assert _dispatches(lib, b) > d0, "the resident step kernel was not used"
    _steps(torch, a, acts, oa, range(12, T), P)
    _steps(torch, b, acts, ob, range(12, T), P)
    b.sync(); torch.cuda.synchronize()
    assert oa.equal(torch, ob)
    assert int(oa.done.sum()) > n // 10
    np.testing.assert_array_equal(_full_state(a), _full_state(b))
    assert a.step_counter == b.step_counter == T
    a.close(); b.close()


def test_resident_ring_wraps(qa, torch):
    """600 steps (the ring has 256 slots: more than two laps) without a synchronisation, every step its own buffers"""
    n, T, P = 4096, 600, 16
    a, b = _pair(qa, n, "docking-v0", 1, 2, seed=3)
    od = a.obs_dim
    acts = a.random_actions(P, step0=0)
    oa, ob = Outs(torch, T, n, od), Outs(torch, T, n, od)
    _steps(torch, a, acts, oa, range(T), P)
    _steps(torch, b, acts, ob, range(T), P)
    b.sync(); torch.cuda.synchronize()
    assert oa.equal(torch, ob)
    np.testing.assert_array_equal(_full_state(a), _full_state(b))
    assert a.step_counter == b.step_counter == T
    a.close(); b.close()


def test_resident_host_pause_beyond_idle_limit(qa, torch):
    """a host pause far longer than the idle limit between two steps: the tiles store their state and end, the next qs_step
    dispatches them again and they resume where they stopped"""
    n, T, P = 65536, 40, 8
    a, b = _pair(qa, n, "docking-v0", 1, 2, seed=8)
    lib = b._lib
    od = a.obs_dim
    acts = a.random_actions(P, step0=0)
    oa, ob = Outs(torch, T, n, od), Outs(torch, T, n, od)
    _steps(torch, a, acts, oa, range(T), P)
    d0 = _dispatches(lib, b)
    _steps(torch, b, acts, ob, range(20), P)
    time.sleep(0.05)                                         # 50 ms: a thousand idle limits
    d1 = _dispatches(lib, b)
    _steps(torch, b, acts, ob, range(20, T), P)
    assert _dispatches(lib, b) > d1 > d0, "no dispatch after the pause"
    b.sync(); torch.cuda.synchronize()
    assert oa.equal(torch, ob)
    np.testing.assert_array_equal(_full_state(a), _full_state(b))
    assert a.step_counter == b.step_counter == T
    a.close(); b.close()


def test_resident_vec_env_steps_and_raw_loop(qa, torch):
    """VecDockingEnv.step in host-ordered mode (every step drained: a roll-out of one step) and the bench's raw qs_step loop
    into the same buffers, against the HIP stream"""
    n, P = 65536, 64
    a, b = _pair(qa, n, "docking-v0", 1, 2, seed=5)
    acts = a.random_actions(P, step0=0)
    for k in range(6):
        ra = a.step(acts[k]); rb = b.step(acts[k])
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(ra[:3], rb[:3])), k
    p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    for env in (a, b):
        args = (p(env._obs), p(env._rew), p(env._done), p(env._flags), p(env._term))
        torch.cuda.synchronize()
        for k in range(3000):
            assert env._lib.qs_step(env._h, p(acts[k % P]), *args) == 0, (k, env._lib.qs_last_error())
        env.sync()
    torch.cuda.synchronize()
    assert torch.equal(a._obs, b._obs) and torch.equal(a._rew, b._rew) and torch.equal(a._done, b._done)
    np.testing.assert_array_equal(_full_state(a), _full_state(b))
    assert a.step_counter == b.step_counter == 3006
    a.close(); b.close()


def test_resident_off_switch_same_results(qa, torch):
    """QS_RESIDENT=0 at qs_set_queue_mode keeps the packet chain: no resident dispatch, the same results"""
    n, T, P = 4096, 30, 8
    a, b = _pair(qa, n, "docking-v2", 2, 2, seed=13)
    old = os.environ.get("QS_RESIDENT")
    os.environ["QS_RESIDENT"] = "0"
    try:
        c = qa.VecDockingEnv("docking-v2", num_envs=n, randomise=2, seed=13, init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2),
                             inertia_scale=(0.8, 1.2), copy=False)
        c.set_queue_mode(True, 2, ordering="host")
    finally:
        if old is None:
            del os.environ["QS_RESIDENT"]
        else:
            os.environ["QS_RESIDENT"] = old
    c.reset()
    t0 = np.zeros(n, np.float32); t0[::5] = 585.0
    c.set_state(t=t0)
    od = a.obs_dim
    acts = a.random_actions(P, step0=0)
    outs = [Outs(torch, T, n, od) for _ in range(3)]
    for env, o in zip((a, b, c), outs):
        _steps(torch, env, acts, o, range(T), P)
        env.sync()
    torch.cuda.synchronize()
    assert _dispatches(b._lib, c) == 0 and _dispatches(b._lib, b) > 0
    assert outs[0].equal(torch, outs[1]) and outs[0].equal(torch, outs[2])
    np.testing.assert_array_equal(_full_state(a), _full_state(c))
    np.testing.assert_array_equal(_full_state(b), _full_state(c))
    for env in (a, b, c):
        env.close()
