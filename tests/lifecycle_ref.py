"""Float64 references and checking functions of the lifecycle kernels at the end of csrc/step_kernels.hpp (k_reset,
k_hover_reset, k_ctor_init, k_fill_init_nominal, k_fill_ctr, k_nominal_obs, k_fill_par, k_fill_actions, k_state_io, k_par_io),
shared by tests/test_lifecycle_cpu.py and tests/test_gpu_lifecycle.py.  numpy and oracle/pyoracle.py only: no torch here.

Records are [n, 40] float32 in the layout of oracle.pyoracle (chaser 13 | target 13 | u_prev 8 | qdes 4 | last_shaping | t),
parameters [n, 4] float32 (mass, Ixx, Iyy, Izz).  A hovering handle has one drone: its env is the chaser words and the first
four words of u_prev; the remaining words of its record belong to no env and a reset must leave them alone.

What is compared how (reset_ref marks every element "bit-exact" or "bounded"):
  bit-exact  everything drawn on a lattice with pinned fused multiply-adds (positions, velocities, body rates, mass, inertia of
             random_init; the position words of ctor_init), every copied word (stored initial states, the target, q_des) and
             every zero (u_prev, last_shaping, t);
  bounded    the reset quaternion, against the float64 euler2quat of the exact float32 Euler angles (QUAT_TOL); the
             observation, against Oracle("f64") rel_obs of the float64 record (helpers.OBS_TOL); last_shaping
             (helpers.reward_atol).
The oracle's own reset quaternion is float32 cosf / sinf arithmetic and is NOT the reference.

QUAT_TOL = 2e-7 is the bound the suite already asserted at a handful of envs; it holds at every env, also at the widest Euler
half-range qs_create admits (RR_WIDE), on the MI355X and for libm float32 (profiles/lifecycle/README.md).  The ceiling it may
ever be raised to is QUAT_CEILING = 8.5 * 2^-23 ~ 1.0e-6: a quaternion word is the sum of two terms, each a product of three
factors, each factor a float32 sin / cos of |x| <= pi/4 good to 1 ulp (relative 2^-23).  Per term: three factor errors and two
product roundings of 2^-24, 4 * 2^-23 of a term of magnitude <= 1; two terms and the rounding of the add (2^-24): 8.5 * 2^-23.
"""
import ctypes as C

import numpy as np

from helpers import OBS_TOL, reward_atol
from oracle.pyoracle import PAR_NOMINAL, REC_LEN, REC_LS, REC_QD, REC_SC, REC_ST, REC_T, REC_UC, RR_NONE, Oracle

f32, f64 = np.float32, np.float64

QUAT_TOL = 2e-7
QUAT_CEILING = 8.5 * 2.0 ** -23
STREAM_AUTORESET, STREAM_RESET, STREAM_CTOR = 0, 1, 3
SOURCES = ("nominal", "rocrand1", "rocrand2", "stored", "hover")
TILE = 64
N_ENVS = (1, 63, 64, 65, 255, 256, 257, 1000)     # one lane, the 64-lane tile edges, the 256-thread block edges, 16 ragged tiles

# the rocRAND ranges of the reset rows: init_range (BASELINE config 3), mass scale, inertia scale
RR = (0.5, 0.1, 0.2, 0.1, 0.8, 1.2, 0.7, 1.3)
# ... and with the widest Euler half-range qs_create admits (init_range[2] <= pi/2: half-angles up to pi/4, the whole domain of the
# reduction-free q_sincos_small)
RR_WIDE = (0.5, 0.1, 1.5707963, 0.1, 0.8, 1.2, 0.7, 1.3)
PAR_NOM = (0.21, 0.00027, 0.000251, 0.00039)      # not the defaults: a kernel that ignores the configured nominals shows
SEED = 0xC0FFEE12345

MASKS = ("null", "all", "none", "alternating", "last", "first_of_last_tile", "bytes_2_255")


def make_mask(kind, n):
    """the uint8 mask of a reset case (None = a NULL pointer)"""
    if kind == "null":
        return None
    m = np.zeros(n, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "last":
        m[n - 1] = 1
    elif kind == "first_of_last_tile":
        m[(n - 1) // TILE * TILE] = 1
    elif kind == "bytes_2_255":
        m[1::3] = 2
        m[2::3] = 255
    else:
        assert kind == "none", kind
    return m


def bits(a):
    """the 32-bit patterns of a float32 array"""
    a = np.ascontiguousarray(a)
    assert a.dtype == f32, a.dtype
    return a.view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- inputs
def raw_words(shape, seed):
    """raw random 32-bit patterns as float32, with NaN payloads (quiet and signalling), -0.0, denormals and both infinities
    planted at fixed places -- what k_state_io / k_par_io must pass through bit for bit"""
    rs = np.random.RandomState(seed)
    w = rs.randint(0, 2 ** 32, size=int(np.prod(shape)), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFBFFFFF, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000,
                        0x00000000], np.uint32)
    k = min(len(w), len(special))
    idx = (np.arange(k) * 7919 + seed) % len(w) if len(w) >= k else np.arange(k)
    w[idx[:k]] = special[:k]
    return w.view(f32).reshape(shape)


def busy_rec(n, seed, hover=False):
    """[n, 40] float32 records in flight: no word at its default, a non-identity q_des, plausible enough to be stepped"""
    rs = np.random.RandomState(seed)
    rec = np.zeros((n, REC_LEN), f32)

    def quat(scale):
        q = np.c_[np.ones(n), rs.uniform(-scale, scale, (n, 3))]
        return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)

    base_c = (0.0, 0.0, 5.0) if hover else (8.3, -50.2, 5.1)
    rec[:, 0:3] = np.array(base_c) + rs.uniform(-0.4, 0.4, (n, 3))
    rec[:, 3:6] = rs.uniform(-0.2, 0.2, (n, 3))
    rec[:, 6:10] = quat(0.05)
    rec[:, 10:13] = rs.uniform(-0.1, 0.1, (n, 3))
    rec[:, 13:16] = np.array((10.1, -49.9, 5.05)) + rs.uniform(-0.2, 0.2, (n, 3))
    rec[:, 16:19] = rs.uniform(-0.1, 0.1, (n, 3))
    rec[:, 19:23] = quat(0.03)
    rec[:, 23:26] = rs.uniform(-0.05, 0.05, (n, 3))
    for o in (REC_UC, REC_UC + 4):
        rec[:, o] = rs.uniform(1.6, 2.0, n)
        rec[:, o + 1:o + 4] = rs.uniform(-1e-3, 1e-3, (n, 3)) + 2e-3
    rec[:, REC_QD:REC_QD + 4] = quat(0.1)
    rec[:, REC_LS] = rs.uniform(-7.0, -3.0, n)
    rec[:, REC_T] = 7.0 + (np.arange(n) % 5)
    assert not (rec == 0).any()
    return rec


def _all_distinct(out):
    """the few chance collisions among random float32 words move up by one float32 each -> the array, every word different"""
    flat = out.reshape(-1)
    for _ in range(8):
        _, first = np.unique(flat, return_index=True)
        dup = np.setdiff1d(np.arange(flat.size), first)
        if not dup.size:
            break
        flat[dup] = np.nextafter(flat[dup], f32(np.inf))
    assert len(np.unique(out)) == out.size
    return out


def distinct_rec(n, seed):
    """busy_rec with a different value in every word of every field of every env (for the check that is no round trip)"""
    rec = busy_rec(n, seed)
    step = (np.arange(n * REC_LEN, dtype=np.float64).reshape(n, REC_LEN) + 1.0) * 2.0 ** -17       # < 0.08 at n = 257
    scale = np.ones(REC_LEN)
    for o in (6, 19, REC_QD):
        scale[o:o + 4] = 0.05                                      # quaternions stay unit to 0.4 %
    scale[REC_UC + 1:REC_UC + 4] = scale[REC_UC + 5:REC_UC + 8] = 0.01    # moments stay small
    rec64 = rec.astype(f64) + step * scale
    rec64[:, REC_T] = 3.0 + np.arange(n)                           # integers below the 600-step limit
    return _all_distinct(rec64.astype(f32))


def distinct_par(n):
    """[n, 4] float32 parameters, every word different"""
    k = np.arange(n, dtype=np.float64)[:, None]
    par = np.array(PAR_NOMINAL) * (0.85 + 0.3 * (k * 4 + np.arange(4)) / (4.0 * n))
    out = par.astype(f32)
    assert len(np.unique(out)) == out.size
    return out


def stored_init(n, seed, hover=False):
    """distinct per env and per word: [n, 13] chaser and [n, 13] target initial states (quaternions unit to 1e-3)"""
    rs = np.random.RandomState(seed)
    out = []
    for base in (((0.0, 0.0, 5.0) if hover else (8.0, -50.0, 5.0)), (10.0, -50.0, 5.0)):
        s = np.zeros((n, 13))
        s[:, 0:3] = np.array(base) + rs.uniform(-0.3, 0.3, (n, 3))
        s[:, 3:6] = rs.uniform(-0.1, 0.1, (n, 3))
        q = np.c_[np.ones(n), rs.uniform(-0.08, 0.08, (n, 3))]
        s[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
        s[:, 10:13] = rs.uniform(-0.1, 0.1, (n, 3))
        s += (np.arange(n * 13).reshape(n, 13) + 1) * 2.0 ** -20
        out.append(s.astype(f32))
    both = _all_distinct(np.concatenate(out, 1))
    return np.ascontiguousarray(both[:, :13]), np.ascontiguousarray(both[:, 13:])


# ---------------------------------------------------------------------------------------------------- float64 pieces
def euler2quat64(e):
    """utils/transform.py:123-136 in float64; e [..., 3] roll, pitch, yaw -> [..., 4]"""
    h = np.asarray(e, f64) * 0.5
    sr, cr, sp, cp, sy, cy = np.sin(h[..., 0]), np.cos(h[..., 0]), np.sin(h[..., 1]), np.cos(h[..., 1]), np.sin(h[..., 2]), np.cos(h[..., 2])
    return np.stack([cr * cp * cy - sr * sp * sy, sr * cp * cy - cr * sp * sy, sr * cp * sy + cr * sp * cy, cr * cp * sy + sr * sp * cy], -1)


def _sym(u):
    """2u - 1 of a lattice uniform: exact in float32"""
    return (2.0 * np.asarray(u, f64) - 1.0).astype(f32)


def random_draw(orc, seed, stream, gid, ctr, rr, par_nom):
    """one env's random_init: (chaser [13] float64 with the float64 quaternion, target [13], par [4] float32, exact mask [13])"""
    sc, st, par, u = orc.random_init(seed, stream, gid, ctr, rr, par_nom)
    e = _sym(u[6:9]) * f32(rr[2])                                  # the exact float32 Euler angles (one float32 product)
    c = sc.astype(f64)
    c[6:10] = euler2quat64(e)
    return c, st.astype(f64), par, e


def ctor_ref(orc, seed, gid, hover):
    """construction-time jitter of env gid: (init [26] or [13] float64 with the float64 quaternion, exact mask)"""
    o = orc.ctor_init(seed, gid, 3 if hover else 2)
    ref, exact = o.astype(f64), np.ones(o.shape, bool)
    if hover:
        w = orc.philox(seed, (STREAM_CTOR << 48) | gid, 0)
        h = np.array([w[1] >> 16, w[2] & 0xFFFF, w[2] >> 16], f64)
        e = _sym((h + 0.5) / 65536.0) * f32(0.2)
        ref[6:10] = euler2quat64(e)
        exact[6:10] = False
    return ref, exact


def ctor_table(orc, seed, gid0, n, hover):
    rows = [ctor_ref(orc, seed, gid0 + i, hover) for i in range(n)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def _env_reset(orc, rec_row, ic, it):
    """qso_env_reset on one record in the oracle's precision -> obs [12]"""
    obs = np.zeros(12, orc.dtype)
    ic, it = np.ascontiguousarray(ic, orc.dtype), np.ascontiguousarray(it, orc.dtype)
    orc._f("qso_env_reset")(rec_row.ctypes.data_as(C.c_void_p), ic.ctypes.data_as(C.c_void_p), it.ctypes.data_as(C.c_void_p),
                            obs.ctypes.data_as(C.c_void_p))
    return obs


def per_env(x, n, dtype=np.uint64):
    """a scalar or a per-env array -> per-env array"""
    a = np.asarray(x, dtype)
    return np.full(n, a, dtype) if a.ndim == 0 else a


def tile_counters(ctr_tiles, n):
    """the step counter each env is keyed by: its own tile's"""
    return np.repeat(np.asarray(ctr_tiles, np.uint64), TILE)[:n]


# ---------------------------------------------------------------------------------------------------- the reference
def reset_ref(rec, par, mask, source, seed=0, ctr=0, gid0=0, rr=RR_NONE, par_nom=PAR_NOMINAL, init=None, stream=STREAM_RESET,
              quat="f64"):
    """What qs_reset(mask) must leave behind.  rec [n, 40] / par [n, 4] float32 as they stand before the call (hovering: the
    chaser words are the drone); mask uint8 [n] or None; source one of SOURCES; ctr a scalar or the per-env counter
    (tile_counters); init [n, 26] (stored) / [n, 13] (hover).  quat "f64": the float64 quaternion of the exact float32 Euler
    angles; "f32": Oracle("f32") throughout (what libm float32 gives: the CPU tests hold it to the same bounds).
    -> dict(rec [n, 40] float64, par [n, 4] float32, obs [n, 12 or 13] float64, exact_rec / exact_obs bool, masked bool [n],
    source)"""
    assert source in SOURCES, source
    rec = np.ascontiguousarray(rec, f32); par = np.ascontiguousarray(par, f32)
    n = rec.shape[0]
    assert rec.shape == (n, REC_LEN) and par.shape == (n, 4)
    masked = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    orc = Oracle("f64" if quat == "f64" else "f32")
    ctr = per_env(ctr, n)
    hover = source == "hover"
    out = rec.astype(orc.dtype)
    out_par = par.copy()
    obs = np.zeros((n, 13 if hover else 12), orc.dtype)
    exact_rec = np.ones((n, REC_LEN), bool)
    exact_obs = np.zeros(obs.shape, bool)
    if source in ("stored", "hover"):
        init = np.ascontiguousarray(init, f32)
        assert init.shape == (n, 13 if hover else 26)
    for i in np.nonzero(masked)[0]:
        if hover:
            out[i, 0:13] = init[i]
            out[i, REC_UC:REC_UC + 4] = 0
            obs[i] = init[i]
            exact_obs[i] = True
            continue
        if source == "nominal":
            ic = np.zeros(13); it = np.zeros(13)
            ic[[0, 1, 2, 6]] = (8, -50, 5, 1); it[[0, 1, 2, 6]] = (10, -50, 5, 1)
        elif source == "stored":
            ic, it = init[i, :13], init[i, 13:]
        else:
            if quat == "f64":
                ic, it, p, _ = random_draw(orc, seed, stream, int(gid0) + int(i), int(ctr[i]), rr, par_nom)
            else:
                ic, it, p, _ = orc.random_init(seed, stream, int(gid0) + int(i), int(ctr[i]), rr, par_nom)
            exact_rec[i, REC_SC + 6:REC_SC + 10] = False
            if source == "rocrand2":
                out_par[i] = p
        obs[i] = _env_reset(orc, out[i], ic, it)
        exact_rec[i, REC_LS] = False
    return dict(rec=out, par=out_par, obs=obs, exact_rec=exact_rec, exact_obs=exact_obs, masked=masked, source=source, hover=hover)


def as_device(ref, obs_before=None):
    """the reference cast to what a device would hand back: (rec float32, par float32, obs float32); unmasked obs rows keep
    obs_before (or the 0xA5 sentinel bytes an output buffer starts with)"""
    obs = ref["obs"].astype(f32)
    if obs_before is None:
        obs_before = np.full(obs.shape, 0xA5A5A5A5, np.uint32).view(f32)
    obs[~ref["masked"]] = obs_before[~ref["masked"]]
    return ref["rec"].astype(f32), ref["par"].copy(), obs


def check_reset(before, after, obs, mask, ref, quat_tol=QUAT_TOL):
    """The whole contract of qs_reset in include/quadsim.h.  before / after: dict(rec [n, 40] float32, par [n, 4] float32,
    ctr = the step counter(s)); before may hold obs = the bytes of obs_out before the call (default: 0xA5 sentinel).  obs: obs_out
    after the call, or None when it was NULL.  -> {"quat", "obs", "ls"}: the worst error as a fraction of its bound (asserted
    <= 1 after everything exact has been asserted)."""
    rb, ra = np.ascontiguousarray(before["rec"], f32), np.ascontiguousarray(after["rec"], f32)
    pb, pa = np.ascontiguousarray(before["par"], f32), np.ascontiguousarray(after["par"], f32)
    n = rb.shape[0]
    masked = np.ones(n, bool) if mask is None else np.asarray(mask) != 0
    assert np.array_equal(masked, ref["masked"])
    keep = ~masked
    hover = ref["hover"]
    # the step counter is not a reset's to change
    assert np.array_equal(np.asarray(before["ctr"], np.uint64), np.asarray(after["ctr"], np.uint64)), "the step counter changed"
    # unmasked rows: state, parameters and obs_out bit for bit
    assert same_bits(rb[keep], ra[keep]), "state of an unmasked env changed"
    assert same_bits(pb[keep], pa[keep]), "parameters of an unmasked env changed"
    # q_des is never reset (docking_env.py:233-244), masked or not
    assert same_bits(rb[:, REC_QD:REC_QD + 4], ra[:, REC_QD:REC_QD + 4]), "qdes changed"
    # parameters change only in masked rows (above), and only with per-episode parameters
    if ref["source"] != "rocrand2":
        assert same_bits(pb, pa), "parameters changed without QS_RANDOMISE_PARAMS"
    assert same_bits(pa, ref["par"]), "parameters of a masked env"
    # stored controls and t
    if hover:
        assert not bits(ra[masked][:, REC_UC:REC_UC + 4]).any(), "u_prev not zero after a reset"
        assert same_bits(rb[:, 13:26], ra[:, 13:26]) and same_bits(rb[:, REC_UC + 4:], ra[:, REC_UC + 4:]), \
            "a hovering reset wrote words that belong to no env"
    else:
        assert not bits(ra[masked][:, REC_UC:REC_UC + 8]).any(), "u_prev (8 words) not zero after a reset"
        assert not bits(ra[masked][:, REC_T]).any(), "t not zero after a reset"
    # every element of the masked rows against the reference
    want = ref["rec"]
    ex = ref["exact_rec"]
    got_bits, want_bits = bits(ra), bits(want.astype(f32))
    bad = ex & (got_bits != want_bits)
    assert not bad.any(), "bit-exact words differ at (env, word) %s" % np.argwhere(bad)[:8].tolist()
    err = np.abs(ra.astype(f64) - want.astype(f64))
    assert np.isfinite(ra[masked]).all()
    qsl = slice(REC_SC + 6, REC_SC + 10)
    ratios = {"quat": 0.0, "obs": 0.0, "ls": 0.0}
    if masked.any() and not hover:
        ratios["quat"] = float((err[masked][:, qsl] / quat_tol).max())
        ratios["ls"] = float((err[masked][:, REC_LS] / reward_atol(want[masked][:, REC_LS].astype(f64))).max())
        drawn = masked & ~ex[:, REC_SC + 6]                          # a quaternion the reset computed, not one it copied
        nq = np.abs(np.linalg.norm(ra[drawn][:, qsl].astype(f64), axis=1) - 1.0) if drawn.any() else np.zeros(1)
        assert (nq <= 4 * quat_tol).all(), "reset quaternion not of unit norm: %g" % nq.max()
    # obs_out
    if obs is not None:
        obs = np.ascontiguousarray(obs, f32)
        ob = before.get("obs")
        if ob is None:
            ob = np.full(obs.shape, 0xA5A5A5A5, np.uint32).view(f32)
        assert same_bits(obs[keep], np.ascontiguousarray(ob, f32)[keep]), "an unmasked row of obs_out was written"
        oe = ref["exact_obs"]
        assert not (oe & (bits(obs) != bits(ref["obs"].astype(f32))))[masked].any(), "bit-exact observation words differ"
        if masked.any() and not hover:
            assert np.isfinite(obs[masked]).all()
            w = ref["obs"][masked].astype(f64)
            ratios["obs"] = float((np.abs(obs[masked].astype(f64) - w) / (OBS_TOL["atol"] + OBS_TOL["rtol"] * np.abs(w))).max())
    for k, v in ratios.items():
        assert v <= 1.0, "%s: error / bound = %.3f" % (k, v)
    return ratios


# ---------------------------------------------------------------------------------------------------- other references
def action_table(orc, seed, gid0, n, step0, T):
    """qs_fill_random_actions: [T, n, 4] float32"""
    out = np.zeros((T, n, 4), f32)
    for t in range(T):
        for i in range(n):
            out[t, i] = orc.random_action(seed, gid0 + i, step0 + t)
    return out


def fresh_rec(n, init=None, hover=False):
    """the record of a fresh handle: the nominal or stored initial state, q_des = identity, everything else zero"""
    rec = np.zeros((n, REC_LEN), f32)
    if hover:
        rec[:, 0:13] = init
        return rec                                    # one drone: the other words of the record stay as allocated (zero)
    if init is None:
        rec[:, [0, 1, 2, 6]] = (8, -50, 5, 1)
        rec[:, [13, 14, 15, 19]] = (10, -50, 5, 1)
    else:
        rec[:, 0:26] = init
    rec[:, REC_QD] = 1
    return rec


REC_FIELDS = (("chaser", REC_SC, 13), ("target", REC_ST, 13), ("u_prev", REC_UC, 8), ("qdes", REC_QD, 4), ("last_shaping", REC_LS, 1),
              ("t", REC_T, 1))


def field_subsets():
    """the pointer subsets of qs_set_state / qs_get_state: none, each single field, each all-but-one, all"""
    names = [f[0] for f in REC_FIELDS]
    subs = [()] + [(k,) for k in names] + [tuple(x for x in names if x != k) for k in names] + [tuple(names)]
    return subs
