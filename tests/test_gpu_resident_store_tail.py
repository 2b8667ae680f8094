"""-m gpu: the resident step loop keeps a step's output and terminal stores in flight across the next step (its chaser wave
waits for memory once per step, in FRONT of the step's stores, and the reset branch stores nothing before that wait).  What that
could break is a store that is lost, lands late, or lands in another step's buffer.  So the resident path (host-ordered private
queue, k_env_resident) is compared bit for bit with the HIP-stream path of the same handle arguments while

  * the steps ROTATE over three distinct sets of output buffers: after a drain, set j must hold the last step k with k % 3 == j,
    and its terminal rows the last terminal row each env wrote into that set -- an older step's store that landed behind a newer
    one, or not at all, leaves a stale row;
  * the roll-outs are drained after 1, 2, 31, 32, 33 and 34 steps: a fresh roll-out counts its progress windows (kResWin = 32
    descriptors, staggered by tile % 32) from its first descriptor, so these lengths end on both sides of a tile's window report,
    whose result is what the chaser wave's one wait is for;
  * every env resets many times, on full and on ragged tiles: all of them by time-out at step 1, all of them by a push out of
    range at the start of the 31-step roll-out, and in the last three roll-outs env i is set to time out at step i % length
    (unless it leaves the range before that, which is a reset too) -- ragged sets of lanes take the reset branch all through a
    roll-out, up to its last steps before the drain.

Sizes 1, 63, 65, 257: one lane, a ragged tile below and above one tile, five workgroups.  Each case once with flags, terminal obs
and terminal state requested and once with the three null.  One run of 300 steps at 65 envs wraps the 256-slot descriptor ring:
slot reuse needs the progress word that the chaser wave writes next to its wait.  The HIP-stream reference of a (case, size) is
computed once, into one buffer per step, and shared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROLLOUTS = (1, 2, 31, 32, 33, 34)
T = sum(ROLLOUTS)
SETS, P = 3, 6
SIZES = (1, 63, 65, 257)
RESIDENT = 2                                                     # StepFamily of qs_debug_step_variant
PAR_NOM = np.array([0.18, 0.00025, 0.000232, 0.0003738])
# (env id, integrator, randomise, per-env params set, reset preparation: 0 two waves per tile, 2 three)
CASES = [
    ("docking-v0", "frozen", 1, False, 0),
    ("docking-v0", "frozen", 1, False, 2),
    ("docking-v2", "rk4", 2, True, 0),
    ("docking-v2", "rk4", 2, True, 2),
]
PATTERN = {"obs": -5.0, "rew": -5.0, "done": 0xEE, "flags": 0xEE, "term": -7.0, "tstate": -9.0}
SHAPE = {"obs": (12,), "rew": (), "done": (), "flags": (), "term": (12,), "tstate": (26,)}
DTYPE = {"obs": np.float32, "rew": np.float32, "done": np.uint8, "flags": np.uint8, "term": np.float32, "tstate": np.float32}


def _case_id(case):
    env_id, integ, rnd, par, prep = case
    return "%s-%s-rnd%d-prep%d-%s" % (env_id[-2:], integ, rnd, prep, "par" if par else "nopar")


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
    return np.concatenate([st[k].reshape(len(st["t"]), -1) for k in sorted(st)], 1)


def _params(env):
    m, inertia = env.get_params()
    return np.concatenate([m[:, None], inertia], axis=1)


def _dispatches(env):
    env._lib.qs_debug_chain_resident.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    d = C.c_uint64(0)
    assert env._lib.qs_debug_chain_resident(env._h, C.byref(d)) == 0
    return int(d.value)


def _family(env):
    env._lib.qs_debug_step_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 5)()
    assert env._lib.qs_debug_step_variant(env._h, out) == 0, env._lib.qs_last_error()
    return int(out[0])


def _buffers(torch, rows, n, keys):
    tdt = {np.float32: torch.float32, np.uint8: torch.uint8}
    return {k: torch.full((rows, n) + SHAPE[k], PATTERN[k], dtype=tdt[DTYPE[k]], device="cuda") for k in keys}


def _run(qa, torch, case, n, resident, keys, rollouts, before, check):
    """the case's roll-outs on the resident path (step k into buffer set k % SETS) or on the HIP stream (step k into row k);
    before(env, r) prepares roll-out r, check(r, k_end, buffers, env) runs after the drain behind it"""
    env_id, integ, rnd, set_par, prep = case
    seed = 70 + CASES.index(case)
    lib = qa._lib.load()
    lib.qs_debug_set_reset_prep.argtypes = [C.c_int]
    lib.qs_debug_set_reset_prep(prep)
    try:
        env = qa.VecDockingEnv(env_id, num_envs=n, integrator=integ, randomise=rnd, seed=seed, copy=False, env_id_offset=977,
                               init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2))
        rng = np.random.default_rng(seed)
        env.reset()
        if set_par:
            env.set_params(mass=(0.18 * rng.uniform(0.85, 1.15, n)).astype(np.float32),
                           inertia=(PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))
        if resident:
            env.set_queue_mode(True, 1, ordering="host")
            assert env.queue_ordering == "host"
            assert _family(env) == RESIDENT, _family(env)
        steps = sum(rollouts)
        acts = torch.from_numpy(rng.uniform(-1.0, 1.0, (P, n, 4)).astype(np.float32)).cuda()
        buf = _buffers(torch, SETS if resident else steps, n, keys)
        p = lambda key, row: C.c_void_p(buf[key][row].data_ptr()) if key in buf else None   # noqa: E731
        d0 = _dispatches(env)
        k = 0
        for r, length in enumerate(rollouts):
            before(env, r)
            torch.cuda.synchronize()                             # host-ordered: the inputs are complete at the call
            for _ in range(length):
                row = k % SETS if resident else k
                rc = env._lib.qs_step_ex(env._h, C.c_void_p(acts[k % P].data_ptr()), p("obs", row), p("rew", row), p("done", row),
                                         p("flags", row), p("term", row), p("tstate", row))
                assert rc == 0, env._lib.qs_last_error()
                k += 1
            env.sync()
            torch.cuda.synchronize()
            check(r, k, {key: v.cpu().numpy() for key, v in buf.items()}, env)
        assert (_dispatches(env) > d0) if resident else (_dispatches(env) == 0)
        env.close()
    finally:
        lib.qs_debug_set_reset_prep(-1)


def _before(case, n, rollouts):
    """the forced resets (module docstring), the same on both paths"""
    def before(env, r):
        if r == 0:
            env.set_state(t=np.full(n, 598.0, np.float32))       # two steps before the time-out: every env resets at step 1
        elif r == 2:
            st = env.get_state()
            c = st["chaser"].copy()
            c[:, 0:3] = st["target"][:, 0:3]
            c[:, 1] += np.float32((10.0 if case[0] == "docking-v2" else 3.0) * 1.05)   # just outside the range limit
            env.set_state(chaser=c)
        elif r >= 3:
            env.set_state(t=(599.0 - np.arange(n) % rollouts[r]).astype(np.float32))   # env i times out at step i % length
    return before


_REF = {}


def _reference(qa, torch, case, n):
    """HIP stream, one buffer row per step: {key: [T, n, ...]}, and the state, params and step counter at every drain"""
    if (case, n) not in _REF:
        ref = {"drain": []}

        def check(r, k_end, b, env):
            ref["drain"].append((_full_state(env), _params(env), env.step_counter))
            ref.update(b)
        _run(qa, torch, case, n, False, tuple(PATTERN), ROLLOUTS, _before(case, n, ROLLOUTS), check)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        resets = ref["done"].astype(np.int64).sum(axis=0)
        assert resets.min() >= 2, resets.min()                   # every env: the time-out at step 1 and the push
        assert ref["done"][1].all() and ref["done"][sum(ROLLOUTS[:2])].all()
        for r in (3, 4, 5):                                      # ragged resets in the first step and in a third of the others
            k0, L = sum(ROLLOUTS[:r]), ROLLOUTS[r]
            assert ref["done"][k0].any() and ref["done"][k0:k0 + L].any(axis=1).sum() >= max(1, min(n, L) // 3), (r, n)
        _REF[(case, n)] = ref
    return _REF[(case, n)]


def _rotated(ref, keys, n, k_end):
    """what the SETS buffer sets hold after steps 0 .. k_end - 1 wrote set k % SETS in order"""
    exp = {key: np.full((SETS, n) + SHAPE[key], PATTERN[key], DTYPE[key]) for key in keys}
    for k in range(k_end):
        dn = ref["done"][k].astype(bool)
        for key in keys:
            if key in ("term", "tstate"):
                exp[key][k % SETS][dn] = ref[key][k][dn]         # rows of envs that did not finish keep what they held
            else:
                exp[key][k % SETS] = ref[key][k]
    return exp


@pytest.mark.parametrize("full", (True, False), ids=("term", "null"))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_rotating_buffers_hold_their_own_steps_at_every_drain(qa, torch, case, n, full):
    ref = _reference(qa, torch, case, n)
    keys = tuple(PATTERN) if full else ("obs", "rew", "done")
    drains = []

    def check(r, k_end, b, env):
        exp = _rotated(ref, keys, n, k_end)
        for key in keys:
            assert np.array_equal(b[key].view(np.uint8), exp[key].view(np.uint8)), (r, k_end, key)
        state, par, counter = ref["drain"][r]
        assert np.array_equal(_full_state(env).view(np.uint8), state.view(np.uint8)), (r, "state")
        assert np.array_equal(_params(env).view(np.uint8), par.view(np.uint8)), (r, "params")
        assert env.step_counter == counter == k_end
        drains.append(k_end)
    _run(qa, torch, case, n, True, keys, ROLLOUTS, _before(case, n, ROLLOUTS), check)
    assert drains == list(np.cumsum(ROLLOUTS))


def test_ring_wraps_with_stores_in_flight(qa, torch):
    """300 steps in one roll-out at 65 envs: the host reuses ring slots by the progress word, env i times out at step 4 i"""
    case, n, steps = CASES[0], 65, (300,)
    keys = tuple(PATTERN)

    def before(env, r):
        env.set_state(t=(599.0 - 4.0 * np.arange(n)).astype(np.float32))
    ref = {}

    def keep(r, k_end, b, env):
        ref.update(b, state=_full_state(env), counter=env.step_counter)
    _run(qa, torch, case, n, False, keys, steps, before, keep)
    assert ref["done"].astype(np.int64).sum(axis=0).min() >= 1 and ref["done"].any(axis=1).sum() >= n

    def check(r, k_end, b, env):
        exp = _rotated(ref, keys, n, k_end)
        for key in keys:
            assert np.array_equal(b[key].view(np.uint8), exp[key].view(np.uint8)), key
        assert np.array_equal(_full_state(env).view(np.uint8), ref["state"].view(np.uint8))
        assert env.step_counter == ref["counter"] == steps[0]
    _run(qa, torch, case, n, True, keys, steps, before, check)
