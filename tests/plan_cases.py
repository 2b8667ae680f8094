"""What the GPU tests of the two sampling planners share (test_gpu_shooting.py, test_gpu_mppi.py): the shapes, the handles with
their provoked states, bit comparisons, and the definition of a candidate's score on a twin handle.  A helper module."""
import numpy as np

N = 96                               # one full tile and a tail tile
PATHS = (1, 64, 200, 1000)           # one lane, one wave, a ragged last wave, a lane loop (4 candidates per lane, ragged)
HORIZONS = (1, 3, 20)
KINDS = ("docking-v0", "docking-v1", "docking-v2")
SEED = 23
PAR_NOM = np.array([0.18, 0.00025, 0.000232, 0.0003738])
DT = float(np.float32(0.02))
HANDLES = [(k, g, p) for k in KINDS for g in ("frozen", "rk4") for p in (False, True)]


def handle_params(n, seed=SEED):
    """the per-env (mass [n], inertia [n,3]) float32 that make_handle(params=True) sets: numpy alone, so a CPU test has them too"""
    rng = np.random.default_rng(seed)
    return ((0.18 * rng.uniform(0.85, 1.15, n)).astype(np.float32),
            (PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))


def make_handle(qa, env_id, integ, params, n=N, provoke="all", offset=0, auto_reset=True, seed=SEED):
    """a handle with rocRAND initial states (docking-v1: its own stored jittered starts, the only reset it has) after a reset
    and two random steps (stored controls and last_shaping are live, k = 2), then -- by env index modulo 6 --
      0  t = 595: times out at horizon step 5;          1  t = 599: times out at the first step;
      2  chaser at z = 0.13 m falling at 2 m/s: under the 0.1 m floor after the first step (0.09 m), whatever the action;
      3  ("all" only) chaser 0.17 m up falling at 2 m/s: crosses the floor around the second step, action-dependent;
      4  ("all" only) chaser's port 5 cm from the target's with zero relative velocity: inside the docked thresholds;
      5  untouched.
    provoke="decisive" leaves 3 and 4 out: there a threshold is crossed within float32 rounding of some candidate, where a
    float32 and a float64 simulator may decide differently; the definition test takes them, the float64 comparison does not."""
    kw = dict(num_envs=n, seed=seed, integrator=integ, env_id_offset=offset, auto_reset=auto_reset)
    if env_id != "docking-v1":
        kw.update(randomise=1, init_range=qa.C3_INIT_RANGE)
    env = qa.VecDockingEnv(env_id, **kw)
    if params:
        mass, inertia = handle_params(n, seed)
        env.set_params(mass=mass, inertia=inertia)
    env.reset()
    for a in env.random_actions(2, step0=0):
        env.step(a)
    if provoke:
        st = env.get_state()
        idx = np.arange(n)
        t0, c = st["t"].copy(), st["chaser"].copy()
        t0[idx % 6 == 0] = 595.0
        t0[idx % 6 == 1] = 599.0
        for m, z in ((2, 0.13), (3, 0.17)):
            sel = idx % 6 == m
            if m == 3 and provoke != "all":
                continue
            c[sel, 2] = z
            c[sel, 3:6] = np.array([0.0, 0.0, -2.0], np.float32)
        if provoke == "all":
            sel = idx % 6 == 4
            c[sel] = st["target"][sel]
            c[sel, 0] -= 0.25                                # ports at +0.1 / -0.1: 5 cm apart
        env.set_state(chaser=c, t=t0)
    return env


def rec_par(env):
    st = env.get_state()
    rec = np.zeros((env.num_envs, 40), np.float64)
    rec[:, 0:13], rec[:, 13:26], rec[:, 26:34], rec[:, 34:38] = st["chaser"], st["target"], st["u_prev"], st["qdes"]
    rec[:, 38], rec[:, 39] = st["last_shaping"], st["t"]
    m, i = env.get_params()
    return st, rec, np.concatenate([m[:, None], i], axis=1).astype(np.float64)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def snapshot(env):
    st = env.get_state()
    m, i = env.get_params()
    return [st[k].copy() for k in sorted(st)] + [m, i, env.step_counter]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def make_twin(qa, env, env_id, integ, params, paths):
    """a handle of env.num_envs x paths envs without auto-reset: `paths` copies of each env of `env`, its parameters included"""
    twin = qa.VecDockingEnv(env_id, num_envs=env.num_envs * paths, integrator=integ, auto_reset=False, seed=SEED + 1)
    if params:
        mass, inertia = env.get_params()
        twin.set_params(mass=np.repeat(mass, paths, axis=0), inertia=np.repeat(inertia, paths, axis=0))
    return twin


def twin_scores(torch, twin, st, acts, paths):
    """The definition of the REWARD score: the state `st` replicated `paths` times on `twin` (make_twin), the candidates' actions
    acts [n, paths, horizon, 4] staged, `horizon` qs_step calls, and the float64 sum of the float32 rewards masked after the
    first done -> (want [n, paths] float64, the number of candidates that stopped inside the horizon)"""
    n, _, horizon, _ = acts.shape
    rep = lambda x: np.repeat(x, paths, axis=0)               # noqa: E731
    twin.set_state(chaser=rep(st["chaser"]), target=rep(st["target"]), u_prev=rep(st["u_prev"]), qdes=rep(st["qdes"]),
                   last_shaping=rep(st["last_shaping"]), t=rep(st["t"]))
    staged = torch.from_numpy(np.ascontiguousarray(acts.reshape(n * paths, horizon, 4).transpose(1, 0, 2))).to(twin.device)
    total = torch.zeros(n * paths, dtype=torch.float64, device=twin.device)
    alive = torch.ones(n * paths, dtype=torch.bool, device=twin.device)
    for h in range(horizon):
        _, r, d, _ = twin.step(staged[h])
        total += torch.where(alive, r.double(), torch.zeros_like(total))
        alive &= ~d
    return total.cpu().numpy().reshape(n, paths), int((~alive).sum())


def slice_handle(qa, big, lo, n):
    """a docking-v0 handle of n envs that are envs lo .. lo + n - 1 of `big`: global ids, state, parameters and step counter"""
    env = qa.VecDockingEnv("docking-v0", num_envs=n, seed=SEED, env_id_offset=lo)
    m, i = big.get_params()
    env.set_params(mass=m[lo:lo + n], inertia=i[lo:lo + n])
    env.set_state(**{k: v[lo:lo + n] for k, v in big.get_state().items()})
    env.step_counter = big.step_counter
    return env


def in_flight_pair(qa, torch):
    """two equal 4096-env handles after the same five steps, b on private queues with its steps not waited for
    -> (a, b, the actions of a sixth step)"""
    a = make_handle(qa, "docking-v0", "frozen", False, n=4096)
    b = make_handle(qa, "docking-v0", "frozen", False, n=4096)
    b.set_queue_mode(True, 2, ordering="host")
    acts = a.random_actions(6, step0=50)
    torch.cuda.synchronize()
    for t in range(5):
        a.step(acts[t])
        b.step_async(acts[t])                                 # not waited for
    return a, b, acts[5]


# ---------------------------------------------------------------- the key, loop and buffer edges
# tests/test_gpu_plan_edges.py runs them on the device, tests/test_plan_edges_cpu.py shows on the references alone that each
# case can see the fault it is there for, tests/plan_matrix.py names the cases by the ids made here.
EDGE_N = 12                                        # two envs of each provoked state
EDGE_SEED = 0x5EED0123456789AB                     # both key words of Philox are in use
EDGE_OFFSETS = ((1 << 32) - 6, (1 << 48) - 12)     # the global ids cross 32 bits inside the handle; the top of the id space
# the step counters at which a field of a candidate's key crosses a 32-bit word
SHOOT_K = (15, 16,                                 # rocRAND's offset 4 * ((k << 26) | ...) crosses 2^32
           63, 64,                                 # the block index (k << 26) | ... crosses 2^32
           (1 << 32) - 1, 1 << 32,                 # k itself crosses 32 bits
           (1 << 36) - 1)                          # the largest k the key holds
MPPI_K = (3, 4,                                    # k << 30 crosses into the upper counter word
          (1 << 32) - 1, 1 << 32, (1 << 33) - 1)
EDGE_SPLITS = (3, 7)                               # 200 paths: chunks of 67 (ragged, two waves) and of 29 (one wave)
EDGE_PATHS, EDGE_HORIZON = 200, 3
# one handle per (INTEG, PARAMS) instantiation of the templated kernels
EDGE_COMBOS = (("docking-v0", "frozen", False), ("docking-v2", "rk4", True), ("docking-v1", "frozen", True),
               ("docking-v0", "rk4", False))
LONG_HANDLES = (("docking-v0", "frozen", False), ("docking-v2", "rk4", True))
LONG_SHOOT = ((1, 65), (64, 256), (200, 256))      # paths, horizon: blocks of 64, 64 and 256 threads
LONG_MPPI = ((1, 65, 0), (64, 128, 1), (200, 128, 0))      # paths, horizon, shift
LONG_K = (1 << 32) - 1
LONG_SIGMA = 0.1                                   # around a nominal near hover (-0.5): the candidates fly all 128 steps
OBS_BOUND = 2e-5                                   # what the project asserts per step: |obs - oracle| (smoke())


def key_cases(ks):
    """[(id, env_id, integ, params, offset, k)]: every k at both offsets, the four handles of EDGE_COMBOS in turn"""
    out = []
    for i, k in enumerate(ks):
        for j, offset in enumerate(EDGE_OFFSETS):
            env_id, integ, params = EDGE_COMBOS[(i + 2 * j) % 4]
            out.append(("k%d-gid%s-%s-%s-%d" % (k, ("32", "48")[j], env_id[-2:], integ, params), env_id, integ, params, offset, k))
    return out


def edge_handle(qa, env_id, integ, params, offset, k, provoke="all", n=EDGE_N):
    """make_handle's handle of EDGE_N envs at global ids offset .., with the 64-bit seed, and the step counter set to k"""
    env = make_handle(qa, env_id, integ, params, n=n, provoke=provoke, offset=offset, seed=EDGE_SEED)
    env.step_counter = k
    return env


# The states of the long horizons are made on the CPU and set on the handle, so that test_plan_edges_cpu.py judges exactly
# what the device runs: over 65 .. 256 steps nearly every shooting candidate leaves the rmax ball (3 m / 10 m), and a state
# qualifies only if no candidate passes a done threshold within the per-step bound (knife_edges).  The seeds are the first
# from 0 on that qualify, for the shooting candidates of (200, 256) and, on the first handle, the MPPI candidates of LONG_MPPI.
# (docking-v2 / rk4 / per-env parameters at seed 0: one candidate within the margin of rmax.)
LONG_STATE_SEEDS = {LONG_HANDLES[0]: 0, LONG_HANDLES[1]: 1}


def long_par(params, n=EDGE_N):
    """[n,4] float64 of the float32 parameters the long-horizon handle holds"""
    if not params:
        return np.tile(PAR_NOM.astype(np.float32).astype(np.float64), (n, 1))
    mass, inertia = handle_params(n, EDGE_SEED)
    return np.concatenate([mass[:, None], inertia], axis=1).astype(np.float64)


def long_states(env_id, integ, params, seed=None, n=EDGE_N):
    """-> (set_state's arguments in float32, the same as records [n,40] float64, parameters [n,4] float64): the nominal start
    with the chaser 0.6 m from the target in a random direction at up to 0.1 m/s, two random steps on the float64 oracle (stored
    controls and last_shaping live), rounded to float32, then make_handle's "decisive" states by env index modulo 6"""
    from oracle.pyoracle import Oracle
    orc = Oracle("f64")
    rng = np.random.default_rng(LONG_STATE_SEEDS[(env_id, integ, params)] if seed is None else seed)
    par = long_par(params, n)
    rec = orc.env_init(n)
    d = rng.standard_normal((n, 3))
    rec[:, 0:3] = rec[:, 13:16] + 0.6 * d / np.linalg.norm(d, axis=1, keepdims=True)
    rec[:, 3:6] = rng.uniform(-0.1, 0.1, (n, 3))
    for _ in range(2):
        orc.vec_step(rec, par, rng.uniform(-1.0, 1.0, (n, 4)), kind=1 if env_id == "docking-v2" else 0, dt=DT,
                     integ=1 if integ == "rk4" else 0, auto_reset=False)
    rec = rec.astype(np.float32)
    idx = np.arange(n)
    rec[idx % 6 == 0, 39] = 595.0
    rec[idx % 6 == 1, 39] = 599.0
    rec[idx % 6 == 2, 2] = 0.13
    rec[idx % 6 == 2, 3:6] = np.array([0.0, 0.0, -2.0], np.float32)
    state = dict(chaser=rec[:, 0:13].copy(), target=rec[:, 13:26].copy(), u_prev=rec[:, 26:34].copy(), qdes=rec[:, 34:38].copy(),
                 last_shaping=rec[:, 38].copy(), t=rec[:, 39].copy())
    return state, rec.astype(np.float64), par


def long_handle(qa, env_id, integ, params):
    """the edge handle at the first offset and LONG_K holding long_states -> (env, rec, par)"""
    state, rec, par = long_states(env_id, integ, params)
    env = edge_handle(qa, env_id, integ, params, EDGE_OFFSETS[0], LONG_K, provoke=None)
    env.set_state(**state)
    return env, rec, par


def long_mppi_inputs(n=EDGE_N):
    """-> (nominal [n,128,4] float32 near hover, noise [200,128,4] float32): the largest long MPPI case; the others slice it"""
    rng = np.random.default_rng(29)
    nominal = (-0.5 + 0.1 * (rng.random((n, 128, 4)) - 0.5)).astype(np.float32)
    return nominal, rng.standard_normal((200, 128, 4)).astype(np.float32)


def knife_edges(rec, par, acts, kind, integ):
    """The number of (candidate, step) pairs, over the steps a candidate takes up to its first done on the float64 oracle, at
    which an error of OBS_BOUND per observation component could flip a decision: |rel_pos| within sqrt(3) OBS_BOUND of rmax, the
    chaser's height within OBS_BOUND of the 0.1 m floor, or the docked predicate (which adds 1 to the reward) true with every
    threshold loosened by its margin and false with every threshold tightened.  The time-out compares integers."""
    from oracle.pyoracle import Oracle
    orc = Oracle("f64")
    n, paths, horizon = acts.shape[:3]
    r = np.ascontiguousarray(np.repeat(np.asarray(rec, np.float64), paths, axis=0))
    p = np.ascontiguousarray(np.repeat(np.asarray(par, np.float64), paths, axis=0))
    a = np.asarray(acts, np.float64).reshape(n * paths, horizon, 4)
    alive = np.ones(n * paths, bool)
    m3, rmax, l10 = np.sqrt(3.0) * OBS_BOUND, (10.0 if kind else 3.0), np.deg2rad(10.0)
    margins = np.array([m3, m3, OBS_BOUND, OBS_BOUND, OBS_BOUND])
    bad = 0
    for h in range(horizon):
        if not alive.any():
            break
        obs, _, _, flags, _ = orc.vec_step(r, p, np.ascontiguousarray(a[:, h]), kind=kind, dt=DT, integ=integ, auto_reset=False)
        dist, speed = np.linalg.norm(obs[:, 0:3], axis=1), np.linalg.norm(obs[:, 3:6], axis=1)
        over = (np.abs(dist - rmax) <= m3) | (np.abs(r[:, 2] - 0.1) <= OBS_BOUND)
        q = np.stack([dist - 0.1, speed - 0.1, np.abs(obs[:, 6]) - l10, np.abs(obs[:, 7]) - l10, np.abs(obs[:, 8]) - l10], axis=1)
        docked = np.all(q < margins, axis=1) != np.all(q < -margins, axis=1)
        bad += int((alive & (over | docked)).sum())
        alive &= (flags & (2 | 4)) == 0
    return bad
