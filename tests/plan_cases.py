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


def make_handle(qa, env_id, integ, params, n=N, provoke="all", offset=0, auto_reset=True):
    """a handle with rocRAND initial states (docking-v1: its own stored jittered starts, the only reset it has) after a reset
    and two random steps (stored controls and last_shaping are live, k = 2), then -- by env index modulo 6 --
      0  t = 595: times out at horizon step 5;          1  t = 599: times out at the first step;
      2  chaser at z = 0.13 m falling at 2 m/s: under the 0.1 m floor after the first step (0.09 m), whatever the action;
      3  ("all" only) chaser 0.17 m up falling at 2 m/s: crosses the floor around the second step, action-dependent;
      4  ("all" only) chaser's port 5 cm from the target's with zero relative velocity: inside the docked thresholds;
      5  untouched.
    provoke="decisive" leaves 3 and 4 out: there a threshold is crossed within float32 rounding of some candidate, where a
    float32 and a float64 simulator may decide differently; the definition test takes them, the float64 comparison does not."""
    kw = dict(num_envs=n, seed=SEED, integrator=integ, env_id_offset=offset, auto_reset=auto_reset)
    if env_id != "docking-v1":
        kw.update(randomise=1, init_range=qa.C3_INIT_RANGE)
    env = qa.VecDockingEnv(env_id, **kw)
    rng = np.random.default_rng(SEED)
    if params:
        env.set_params(mass=(0.18 * rng.uniform(0.85, 1.15, n)).astype(np.float32),
                       inertia=(PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))
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
