"""-m gpu: the lifecycle kernels at the end of csrc/step_kernels.hpp -- the resets, the construction-time fills, the action
stream and the conversions behind get / set -- against the float64 references of tests/lifecycle_ref.py, on every element, at
env counts of one lane, the 64-lane tile edges, the 256-thread block edges and sixteen tiles with a ragged last one.  Every call
goes through the C ABI on a handle made by qs_create, with each user buffer a view into a larger device tensor, 256 sentinel
bytes on each side (the Guards of test_gpu_postproc.py): a store outside a buffer shows as a changed sentinel byte, never as a
fault, and an output the kernel skips keeps its sentinel payload.  One row per instantiation: tests/lifecycle_matrix.py.

Every test prints `lifecycle ratio <kernel> <x>`: the worst error as a fraction of its bound (0 where everything is bit-exact)."""
import ctypes as C

import numpy as np
import pytest

import lifecycle_ref as lr
import step_matrix
from helpers import OBS_TOL, STATE_TOL, reward_atol
from oracle.pyoracle import REC_LS, REC_QD, REC_T, REC_UC, Oracle
from test_gpu_postproc import Guards

pytestmark = pytest.mark.gpu

f32 = np.float32
GID0, K0 = step_matrix.ROCRAND_GID0, step_matrix.ROCRAND_K0
KIND = {"docking-v0": 0, "docking-v2": 1, "docking-v1": 2, "hovering-v0": 3}


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def o64():
    return Oracle("f64")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _untouched(t):
    """an output buffer that was not passed still holds its sentinel payload"""
    return bool((t.cpu().numpy().reshape(-1).view(np.uint8) == 0xA5).all())


def _report(kernel, worst):
    print("lifecycle ratio %s %.4f" % (kernel, worst))


class Handle:
    """one qs_create handle and its C ABI calls, each ordered against torch by a device-wide synchronisation before and a
    qs_sync after; every buffer of every call sits between sentinel bands and is checked when the call has returned"""

    def __init__(self, qa, torch, env_id, n, randomise=0, gid0=0, auto_reset=0, rr=lr.RR):
        self.qa, self.torch, self.lib, self.n = qa, torch, qa._lib.load(), n
        self.hover = env_id == "hovering-v0"
        self.obs_dim = 13 if self.hover else 12
        self.device = torch.device("cuda", torch.cuda.current_device())
        cfg = qa._lib.default_config()
        cfg.kind, cfg.num_envs, cfg.device = KIND[env_id], n, torch.cuda.current_device()
        cfg.auto_reset, cfg.randomise, cfg.seed, cfg.env_id_offset = auto_reset, randomise, lr.SEED, gid0
        cfg.init_range = (C.c_float * 4)(*rr[0:4])
        cfg.mass_scale = (C.c_float * 2)(*rr[4:6])
        cfg.inertia_scale = (C.c_float * 2)(*rr[6:8])
        cfg.mass = lr.PAR_NOM[0]
        cfg.inertia = (C.c_float * 3)(*lr.PAR_NOM[1:4])
        self.h = C.c_void_p()
        qa._lib.check(self.lib.qs_create(C.byref(cfg), C.byref(self.h)), "qs_create")

    def close(self):
        if self.h:
            self.lib.qs_destroy(self.h)
            self.h = None

    def call(self, name, *args, want=0):
        self.torch.cuda.synchronize()
        rc = getattr(self.lib, name)(self.h, *args)
        assert rc == want, "%s returned %d: %s" % (name, rc, self.lib.qs_last_error().decode("utf-8", "replace"))
        assert self.lib.qs_sync(self.h) == 0
        self.torch.cuda.synchronize()

    def guards(self):
        return Guards(self.torch, self.device)

    # ---- state ----
    def set_fields(self, fields):
        """qs_set_state with the given {field: array}; absent fields are NULL"""
        G = self.guards()
        t = {k: G.put(np.ascontiguousarray(v, f32)) for k, v in fields.items()}
        self.call("qs_set_state", *[_p(t.get(name)) for name, _, _ in lr.REC_FIELDS])
        G.check()

    def get_fields(self, names):
        """qs_get_state with the named fields passed and the others NULL -> {field: array}; the buffers of the others are
        allocated all the same and must keep their sentinel payload"""
        G = self.guards()
        t = {name: G.out((self.n, w) if w > 1 else (self.n,)) for name, _, w in lr.REC_FIELDS}
        self.call("qs_get_state", *[_p(t[name]) if name in names else None for name, _, _ in lr.REC_FIELDS])
        G.check()
        for name in t:
            if name not in names:
                assert _untouched(t[name]), "qs_get_state wrote %s, which was not passed" % name
        return {name: t[name].cpu().numpy() for name in names}

    def set_rec(self, rec):
        self.set_fields({name: rec[:, o:o + w] if w > 1 else rec[:, o] for name, o, w in lr.REC_FIELDS})

    def get_rec(self):
        got = self.get_fields([f[0] for f in lr.REC_FIELDS])
        rec = np.zeros((self.n, 40), f32)
        for name, o, w in lr.REC_FIELDS:
            rec[:, o:o + w] = got[name].reshape(self.n, w)
        return rec

    # ---- parameters ----
    def set_par(self, mass=None, inertia=None, want=0):
        G = self.guards()
        m = G.put(np.ascontiguousarray(mass, f32)) if mass is not None else None
        i = G.put(np.ascontiguousarray(inertia, f32)) if inertia is not None else None
        self.call("qs_set_params", _p(m), _p(i), want=want)
        G.check()

    def get_par(self, mass=True, inertia=True):
        """-> [n, 4] with the sentinel bit pattern where a part was not asked for (and was verified untouched)"""
        G = self.guards()
        m, i = G.out((self.n,)), G.out((self.n, 3))
        self.call("qs_get_params", _p(m) if mass else None, _p(i) if inertia else None)
        G.check()
        assert mass or _untouched(m)
        assert inertia or _untouched(i)
        return np.ascontiguousarray(np.c_[m.cpu().numpy(), i.cpu().numpy()], f32)

    # ---- counter, step, reset ----
    @property
    def counter(self):
        k = C.c_uint64(0)
        self.call("qs_get_step_counter", C.byref(k))
        return k.value

    @counter.setter
    def counter(self, k):
        self.call("qs_set_step_counter", C.c_uint64(k))

    def step(self, actions):
        """qs_step -> (obs, reward, done)"""
        G = self.guards()
        a = G.put(np.ascontiguousarray(actions, f32))
        obs, rew, done = G.out((self.n, self.obs_dim)), G.out((self.n,)), G.out((self.n,), np.uint8)
        self.call("qs_step", _p(a), _p(obs), _p(rew), _p(done), None, None)
        G.check()
        return obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()

    def reset(self, mask, want_obs):
        """qs_reset -> obs_out (its payload started as sentinel bytes) or None"""
        G = self.guards()
        m = G.put(mask) if mask is not None else None
        obs = G.out((self.n, self.obs_dim)) if want_obs else None
        self.call("qs_reset", _p(m), _p(obs))
        G.check()
        return obs.cpu().numpy() if want_obs else None

    # ---- stored initial states ----
    def get_init(self, chaser=True, target=True):
        G = self.guards()
        c, t = G.out((self.n, 13)), G.out((self.n, 13))
        self.call("qs_get_init_state", _p(c) if chaser else None, _p(t) if target else None)
        G.check()
        assert chaser or _untouched(c)
        assert (target and not self.hover) or _untouched(t), "target_init written although not passed / on a hovering handle"
        return c.cpu().numpy(), t.cpu().numpy()

    def set_init(self, chaser, target=None):
        G = self.guards()
        c = G.put(np.ascontiguousarray(chaser, f32))
        t = G.put(np.ascontiguousarray(target, f32)) if target is not None else None
        self.call("qs_set_init_state", _p(c), _p(t))
        G.check()


@pytest.fixture
def make(qa, torch):
    made = []

    def _make(*args, **kw):
        made.append(Handle(qa, torch, *args, **kw))
        return made[-1]
    yield _make
    for h in made:
        h.close()


def _actions(n, seed, hover=False):
    a = np.random.RandomState(seed).uniform(-1, 1, (2, n, 4)).astype(f32)
    return 0.5 * a + 0.5 if hover else a


# ==================================================================================================== state and parameter I/O
@pytest.mark.parametrize("n", lr.N_ENVS)
@pytest.mark.parametrize("env_id", ["docking-v0", "hovering-v0"])
def test_state_io(make, env_id, n):
    """k_state_io<false> / <true>: for every pointer subset (none, each field, all but each field, all) raw 32-bit patterns --
    NaN payloads, -0.0, denormals, infinities among them -- set into the subset come back bit for bit, the fields not passed
    keep the bits they had, get buffers not passed are never touched and inputs are never written"""
    h = make(env_id, n)
    names = [f[0] for f in lr.REC_FIELDS]
    for j, subset in enumerate(lr.field_subsets()):
        A, B = lr.raw_words((n, 40), 1000 * j + n), lr.raw_words((n, 40), 1000 * j + n + 500)
        h.set_rec(A)
        assert lr.same_bits(h.get_rec(), A), "all fields, round trip"
        h.set_fields({name: (B[:, o:o + w] if w > 1 else B[:, o]) for name, o, w in lr.REC_FIELDS if name in subset})
        want = A.copy()
        for name, o, w in lr.REC_FIELDS:
            if name in subset:
                want[:, o:o + w] = B[:, o:o + w]
        assert lr.same_bits(h.get_rec(), want), "set subset %s" % (subset,)
        got = h.get_fields(subset)                                   # the get side with the same subset
        for name, o, w in lr.REC_FIELDS:
            if name in subset:
                assert lr.same_bits(got[name].reshape(n, w), want[:, o:o + w]), "get subset %s: %s" % (subset, name)
    assert set(names) == set(lr.field_subsets()[-1])
    _report("k_state_io", 0.0)


@pytest.mark.parametrize("n", lr.N_ENVS)
def test_par_io(make, n):
    """k_par_io<false> / <true>: mass only, inertia only, both -- bit for bit, the part not passed untouched on either side;
    a fresh handle holds the configured nominals at every env (k_fill_par)"""
    h = make("docking-v0", n)
    nominal = np.tile(np.asarray(lr.PAR_NOM, f32), (n, 1))
    assert lr.same_bits(h.get_par(), nominal)
    A, B = lr.raw_words((n, 4), n), lr.raw_words((n, 4), n + 77)
    h.set_par(A[:, 0], A[:, 1:])
    assert lr.same_bits(h.get_par(), A)
    h.set_par(mass=B[:, 0])
    assert lr.same_bits(h.get_par(), np.c_[B[:, 0], A[:, 1:]])
    h.set_par(A[:, 0], A[:, 1:])
    h.set_par(inertia=B[:, 1:])
    want = np.ascontiguousarray(np.c_[A[:, 0], B[:, 1:]], f32)
    assert lr.same_bits(h.get_par(), want)
    assert lr.same_bits(h.get_par(inertia=False)[:, 0], want[:, 0])
    assert lr.same_bits(h.get_par(mass=False)[:, 1:], want[:, 1:])
    h.set_par(want=-1)                                               # QS_ERR_INVALID: nothing to set
    assert lr.same_bits(h.get_par(), want)
    _report("k_par_io", 0.0)


def test_one_step_from_a_set_state_matches_the_oracle(make, o64):
    """no round trip: a state and parameters with a different finite value in every word of every env go in through
    qs_set_state / qs_set_params, one qs_step (auto_reset off) is compared with Oracle("f64").vec_step from the same values.  A
    permutation that k_state_io or k_par_io applies in both directions alike cancels in a round trip and fails here."""
    n = 257
    h = make("docking-v0", n)
    rec, par = lr.distinct_rec(n, 11), lr.distinct_par(n)
    a = _actions(n, 5)[0]
    h.set_rec(rec)
    h.set_par(par[:, 0], par[:, 1:])
    obs, rew, done = h.step(a)
    after = h.get_rec()
    rec64, par64 = rec.astype(np.float64), par.astype(np.float64)
    o_ref, r_ref, d_ref, _, _ = o64.vec_step(rec64, par64, a, kind=0, auto_reset=False)
    assert np.array_equal(done, d_ref)
    eo = np.abs(obs - o_ref) / (OBS_TOL["atol"] + OBS_TOL["rtol"] * np.abs(o_ref))
    es = np.abs(after[:, :REC_LS] - rec64[:, :REC_LS]) / (STATE_TOL["atol"] + STATE_TOL["rtol"] * np.abs(rec64[:, :REC_LS]))
    el = np.abs(after[:, REC_LS] - rec64[:, REC_LS]) / reward_atol(rec64[:, REC_LS])
    _report("k_state_io+k_par_io (one step) obs", float(eo.max()))
    _report("k_state_io+k_par_io (one step) state", float(max(es.max(), el.max())))
    assert eo.max() <= 1 and es.max() <= 1 and el.max() <= 1
    assert np.array_equal(after[:, REC_T], rec64[:, REC_T].astype(f32))
    assert lr.same_bits(h.get_par(), par)


# ==================================================================================================== resets
# source -> (env id, randomise, reset_ref source)
RESETS = {
    "nominal_v0": ("docking-v0", 0, "nominal"), "nominal_v2": ("docking-v2", 0, "nominal"),
    "rocrand1": ("docking-v0", 1, "rocrand1"), "rocrand2": ("docking-v0", 2, "rocrand2"),
    "docking_v1": ("docking-v1", 0, "stored"), "stored_nominal_target": ("docking-v0", 2, "stored"),
    "hover": ("hovering-v0", 0, "hover"),
}
RESET_KERNEL = {"hover": "k_hover_reset"}


def _reset_handle(make, o64, source, n):
    """-> (handle, reset_ref source, its keyword arguments but the counter)"""
    env_id, randomise, src = RESETS[source]
    h = make(env_id, n, randomise=randomise, gid0=GID0)
    kw = {}
    if src.startswith("rocrand"):
        kw = dict(seed=lr.SEED, gid0=GID0, rr=lr.RR, par_nom=lr.PAR_NOM)
    elif source == "docking_v1":
        kw = dict(init=lr.ctor_table(o64, lr.SEED, GID0, n, False)[0].astype(f32))      # all 26 words are bit-exact
    elif source == "stored_nominal_target":
        chaser = lr.stored_init(n, 21)[0]
        h.set_init(chaser)                                              # target_init NULL: k_fill_init_nominal's target
        kw = dict(init=np.ascontiguousarray(np.c_[chaser, lr.fresh_rec(n)[:, 13:26]], f32))
    elif source == "hover":
        kw = dict(init=h.get_init()[0])                                 # held to the oracle by test_ctor_jitter
    return h, src, kw


def _prepare(h, source, n):
    """no default word anywhere, a non-identity q_des, two steps, then the counter of the rocRAND rows"""
    h.set_rec(lr.busy_rec(n, 100 + n, hover=h.hover))
    if source == "rocrand2":
        par = lr.distinct_par(n)
        h.set_par(par[:, 0], par[:, 1:])
    for a in _actions(n, n, h.hover):
        h.step(a)
    h.counter = K0


@pytest.mark.parametrize("n", lr.N_ENVS)
@pytest.mark.parametrize("source", sorted(RESETS))
def test_reset(make, o64, source, n):
    """k_reset / k_hover_reset: every reset source x every mask x obs_out present / NULL, check_reset on every element of every
    env.  The run with obs_out NULL repeats the run with obs_out from the same state and counter: the same bits."""
    h, src, kw = _reset_handle(make, o64, source, n)
    worst = {"quat": 0.0, "obs": 0.0, "ls": 0.0}
    try:
        for mask_kind in lr.MASKS:
            mask = lr.make_mask(mask_kind, n)
            first = None
            for want_obs in (True, False):
                _prepare(h, source, n)
                before = dict(rec=h.get_rec(), par=h.get_par(), ctr=h.counter)
                assert before["ctr"] == K0
                b = before["rec"]                                     # what a reset has to clear is not clear already
                assert (b[:, REC_UC:REC_UC + 4] != 0).any(1).all() and (h.hover or (b[:, REC_UC + 4:REC_UC + 8] != 0).any(1).all())
                assert (b[:, REC_LS] != 0).all() and (b[:, REC_T] != 0).all() and (b[:, REC_QD + 1:REC_QD + 4] != 0).all()
                obs = h.reset(mask, want_obs)
                after = dict(rec=h.get_rec(), par=h.get_par(), ctr=h.counter)
                ref = lr.reset_ref(before["rec"], before["par"], mask, src, ctr=K0, **kw)
                r = lr.check_reset(before, after, obs, mask, ref)
                worst = {k: max(worst[k], r[k]) for k in worst}
                if first is None:
                    first = after
                else:
                    assert lr.same_bits(first["rec"], after["rec"]) and lr.same_bits(first["par"], after["par"]), "a repeated reset"
    finally:
        for k, v in worst.items():
            _report("%s %s %s" % (RESET_KERNEL.get(source, "k_reset"), source, k), v)


def test_reset_quaternion_over_the_whole_half_angle_domain(make):
    """init_range[2] = pi/2, the widest qs_create admits: half-angles over all of |x| <= pi/4, the domain of the reduction-free
    q_sincos_small.  State, parameters and the QUAT_TOL of the narrow rows at every env; obs_out is NULL: at roll near pi/2 the
    relative Euler angles of the observation are singular and no float32 evaluation meets OBS_TOL there (the float32 oracle does
    not either: tests/test_lifecycle_cpu.py)."""
    n = 1000
    h = make("docking-v2", n, randomise=1, gid0=GID0, rr=lr.RR_WIDE)
    worst = 0.0
    for mask_kind in ("null", "bytes_2_255"):
        mask = lr.make_mask(mask_kind, n)
        _prepare(h, "rocrand1", n)
        before = dict(rec=h.get_rec(), par=h.get_par(), ctr=h.counter)
        assert h.reset(mask, False) is None
        after = dict(rec=h.get_rec(), par=h.get_par(), ctr=h.counter)
        ref = lr.reset_ref(before["rec"], before["par"], mask, "rocrand1", seed=lr.SEED, ctr=K0, gid0=GID0, rr=lr.RR_WIDE, par_nom=lr.PAR_NOM)
        err = np.abs(after["rec"][ref["masked"]][:, 6:10] - ref["rec"][ref["masked"]][:, 6:10]).max() / lr.QUAT_TOL
        _report("k_reset rocrand1 Euler half-range pi/2 quat (mask %s)" % mask_kind, float(err))       # printed before it is asserted
        worst = max(worst, lr.check_reset(before, after, None, mask, ref)["quat"])
    assert worst <= 1.0 and np.abs(ref["rec"][:, 7]).max() > 0.6                                  # the angles are wide


def test_step_counter_reaches_every_tile(make):
    """k_fill_ctr: qs_get_step_counter reads tile 0 only; a full rocRAND reset after qs_set_step_counter(k) is keyed by k in all
    sixteen tiles, for two values of k in turn (a tile that kept the previous value shows too)"""
    n = 1000
    h = make("docking-v0", n, randomise=1, gid0=GID0)
    worst = 0.0
    for k in (K0, 12345):
        h.counter = k
        assert h.counter == k
        before = dict(rec=h.get_rec(), par=h.get_par(), ctr=k)
        obs = h.reset(None, True)
        after = dict(rec=h.get_rec(), par=h.get_par(), ctr=h.counter)
        ref = lr.reset_ref(before["rec"], before["par"], None, "rocrand1", seed=lr.SEED, ctr=k, gid0=GID0, rr=lr.RR, par_nom=lr.PAR_NOM)
        worst = max(worst, max(lr.check_reset(before, after, obs, None, ref).values()))
    _report("k_fill_ctr (through k_reset)", worst)


def test_reset_keys_every_env_by_its_own_tiles_counter(make):
    """two groups of one handle that have stepped 3 times and once: the rocRAND reset keys each env by its own tile's step
    counter (include/quadsim.h, qs_reset)"""
    n = 1000
    h = make("docking-v0", n, randomise=2, gid0=GID0)
    h.counter = K0
    h.call("qs_set_groups", 2, 0)
    ranges = []
    for g in range(2):
        lo, hi = C.c_int64(0), C.c_int64(0)
        h.call("qs_group_range", g, C.byref(lo), C.byref(hi))
        ranges.append((lo.value, hi.value))
    assert ranges[0][0] == 0 and ranges[0][1] == ranges[1][0] and ranges[1][1] == n and ranges[0][1] % 64 == 0
    acts = np.random.RandomState(3).uniform(-1, 1, (3, n, 4)).astype(f32)
    for g, steps in ((0, 3), (1, 1)):
        lo, hi = ranges[g]
        for t in range(steps):
            G = h.guards()
            a = G.put(acts[t, lo:hi])
            obs, rew, done = G.out((hi - lo, 12)), G.out((hi - lo,)), G.out((hi - lo,), np.uint8)
            h.call("qs_step_group", g, _p(a), _p(obs), _p(rew), _p(done), None, None, None)
            G.check()
    ctr = np.where(np.arange(n) < ranges[0][1], K0 + 3, K0 + 1).astype(np.uint64)
    before = dict(rec=h.get_rec(), par=h.get_par(), ctr=h.counter)
    assert before["ctr"] == K0 + 3                                     # tile 0 belongs to the group that stepped 3 times
    mask = lr.make_mask("alternating", n)
    obs = h.reset(mask, True)
    after = dict(rec=h.get_rec(), par=h.get_par(), ctr=h.counter)
    ref = lr.reset_ref(before["rec"], before["par"], mask, "rocrand2", seed=lr.SEED, ctr=ctr, gid0=GID0, rr=lr.RR, par_nom=lr.PAR_NOM)
    _report("k_reset uneven group steps", max(lr.check_reset(before, after, obs, mask, ref).values()))


FRESH = [("docking-v0", 0), ("docking-v0", 1), ("docking-v2", 2), ("docking-v1", 0), ("hovering-v0", 0)]


@pytest.mark.parametrize("n", lr.N_ENVS)
@pytest.mark.parametrize("env_id,randomise", FRESH)
def test_fresh_handle(make, o64, env_id, randomise, n):
    """the init_all path of qs_create: the nominal or stored initial state at every env, q_des the identity, u_prev, last_shaping
    and t zero, the configured nominal parameters (k_fill_par; never randomised, QS_RANDOMISE_PARAMS included), counter 0"""
    h = make(env_id, n, randomise=randomise, gid0=GID0)
    init = None
    if env_id == "docking-v1":
        init = lr.ctor_table(o64, lr.SEED, GID0, n, False)[0].astype(f32)
    elif h.hover:
        init = h.get_init()[0]
    assert lr.same_bits(h.get_rec(), lr.fresh_rec(n, init, h.hover))
    assert lr.same_bits(h.get_par(), np.tile(np.asarray(lr.PAR_NOM, f32), (n, 1)))
    assert h.counter == 0
    _report("k_fill_par+init_all %s" % env_id, 0.0)


@pytest.mark.parametrize("n", [1, 257])
def test_nominal_obs_is_the_nominal_reset_observation(make, n):
    """k_nominal_obs: QsEnv::nominal_obs is what a step returns as the observation of an env it has just reset (RMODE 0,
    auto_reset).  Bit for bit the obs_out of a nominal qs_reset."""
    h = make("docking-v0", n, auto_reset=1)
    obs_reset = h.reset(None, True)
    h.set_rec(lr.busy_rec(n, 9))
    h.set_fields({"t": np.full(n, 599.0, f32)})                        # the next step is the 600th: overtime, done, auto-reset
    obs, rew, done = h.step(np.zeros((n, 4), f32))
    assert done.all()
    assert lr.same_bits(obs, obs_reset)
    np.testing.assert_allclose(obs_reset, np.tile([1.8] + [0.0] * 11, (n, 1)), **OBS_TOL)
    _report("k_nominal_obs", 0.0)


# ==================================================================================================== construction jitter, init_io
@pytest.mark.parametrize("n", lr.N_ENVS)
@pytest.mark.parametrize("env_id", ["docking-v1", "hovering-v0"])
def test_ctor_jitter(make, o64, env_id, n):
    """k_ctor_init through qs_get_init_state against Oracle.ctor_init at every env: docking all 26 words bit-exact; hovering the
    position words (and every zero) bit-exact, the quaternion within QUAT_TOL of the float64 one and of unit norm"""
    h = make(env_id, n, gid0=GID0)
    chaser, target = h.get_init()
    got = chaser if h.hover else np.ascontiguousarray(np.c_[chaser, target], f32)
    ref, exact = lr.ctor_table(o64, lr.SEED, GID0, n, h.hover)
    bad = exact & (lr.bits(got) != lr.bits(ref.astype(f32)))
    assert not bad.any(), np.argwhere(bad)[:8].tolist()
    worst = 0.0
    if h.hover:
        worst = float(np.abs(got[:, 6:10] - ref[:, 6:10]).max() / lr.QUAT_TOL)
        norm = np.abs(np.linalg.norm(got[:, 6:10].astype(np.float64), axis=1) - 1).max()
    _report("k_ctor_init %s" % env_id, worst)
    assert worst <= 1.0 and (not h.hover or norm <= 4 * lr.QUAT_TOL)


@pytest.mark.parametrize("env_id", ["docking-v1", "hovering-v0"])
def test_ctor_jitter_depends_on_the_global_id_alone(make, env_id):
    """a 65-env handle at an offset holds the same initial states as those envs of a 1000-env handle"""
    big, small = make(env_id, 1000, gid0=GID0), make(env_id, 65, gid0=GID0 + 7)
    for a, b in zip(big.get_init(), small.get_init()):
        assert lr.same_bits(a[7:72], b)


@pytest.mark.parametrize("n", lr.N_ENVS)
@pytest.mark.parametrize("env_id", ["docking-v0", "hovering-v0"])
def test_init_io(make, env_id, n):
    """init_io's strided 2-D copies with distinct values per env and per word: chaser only (the target NULL = nominal, from
    k_fill_init_nominal on a docking-v0 handle), both, and on the get side chaser only and target only.  Hovering ignores
    target_init on both sides."""
    h = make(env_id, n)
    c1, t1 = lr.stored_init(n, 31, h.hover)
    c2, t2 = lr.stored_init(n, 32, h.hover)
    h.set_init(c1)
    gc, gt = h.get_init()
    assert lr.same_bits(gc, c1)
    if not h.hover:
        assert lr.same_bits(gt, lr.fresh_rec(n)[:, 13:26])
    h.set_init(c2, t2)
    gc, gt = h.get_init()
    assert lr.same_bits(gc, c2) and (h.hover or lr.same_bits(gt, t2))
    assert lr.same_bits(h.get_init(target=False)[0], c2)
    gt = h.get_init(chaser=False)[1]
    assert h.hover or lr.same_bits(gt, t2)
    h.set_init(c1)                                                     # target NULL now leaves the stored target alone
    gc, gt = h.get_init()
    assert lr.same_bits(gc, c1) and (h.hover or lr.same_bits(gt, t2))
    _report("k_fill_init_nominal+init_io %s" % env_id, 0.0)


# ==================================================================================================== the action stream
@pytest.mark.parametrize("T,n", [(1, 1), (3, 85), (4, 64), (1, 257), (3, 1000)])
def test_fill_random_actions(make, o64, T, n):
    """k_fill_actions: every element equals Oracle.random_action bit for bit; the global env id and the step index both cross
    (or, for a single env / step, lie beyond) 32 bits"""
    gid0 = 2 ** 32 - n // 2 if n > 1 else 2 ** 32 + 3
    step0 = 2 ** 32 - T // 2 if T > 1 else 2 ** 32 + 5
    h = make("docking-v0", n, gid0=gid0)
    G = h.guards()
    out = G.out((T, n, 4))
    h.call("qs_fill_random_actions", C.c_int64(T), C.c_uint64(step0), _p(out))
    G.check()
    assert lr.same_bits(out.cpu().numpy(), lr.action_table(o64, lr.SEED, gid0, n, step0, T))
    assert h.counter == 0
    _report("k_fill_actions", 0.0)
