"""Float64 reference of qs_shooting_plan, built only from what oracle/pyoracle.py exposes: qso_philox4x32_10 + qso_u01 for the
candidates' actions, qso_env_step (through Oracle.vec_step, which calls it per env, auto_reset off) for the steps.  A helper
module, not a test.

The keying is the contract of include/quadsim.h: a[c][h] = 2 u01(w) - 1 in float32, w the four words of Philox block
(k << 26) | (c << 10) | h of subsequence (5 << 48) | gid.  `actions` loops over the oracle's Philox (the definition);
`actions_fast` is the same generator written with numpy integers for the hundreds of thousands of blocks a GPU comparison
stages -- test_shooting_cpu.py holds it to `actions` bit for bit."""
import ctypes as C

import numpy as np

from oracle.pyoracle import REC_LEN, Oracle, lib

STREAM_PLAN = 5
REWARD, POSITION = 0, 1
DONE_FLAGS = 2 | 4            # over limit, over time: what the step API reports as done


def block_index(k, c, h):
    assert 0 <= k < 1 << 36 and 0 <= c < 1 << 16 and 0 <= h < 1 << 10
    return (k << 26) | (c << 10) | h


def actions(seed, gid, k, paths, horizon):
    """[paths, horizon, 4] float32 through qso_philox4x32_10 / qso_u01"""
    L = lib()
    u01 = L.qso_u01_f64
    u01.restype, u01.argtypes = C.c_float, [C.c_uint32]
    w = np.zeros(4, np.uint32)
    out = np.zeros((paths, horizon, 4), np.float32)
    for c in range(paths):
        for h in range(horizon):
            L.qso_philox4x32_10_f64(C.c_uint64(seed), C.c_uint64((STREAM_PLAN << 48) | gid), C.c_uint64(block_index(k, c, h)),
                                    w.ctypes.data_as(C.c_void_p))
            for j in range(4):
                # sym = fma(2, u, -1): 2u is exact in binary32, so the subtraction is the one rounding the fma makes
                out[c, h, j] = np.float32(2.0) * np.float32(u01(int(w[j]))) - np.float32(1.0)
    return out


def philox_np(seed, subsequence, block):
    """Philox4x32-10 for an array of 64-bit block indices -> [..., 4] uint32"""
    block = np.asarray(block, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = block & m32, block >> np.uint64(32)
    c2 = np.full_like(block, subsequence & 0xFFFFFFFF)
    c3 = np.full_like(block, subsequence >> 32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def actions_fast(seed, gid, k, paths, horizon):
    """= actions(...), vectorised.  u01 = fma((float)v, 2^-32, 2^-32): v is rounded to binary32 first, then ((float)v + 1) 2^-32
    is exact in float64 and rounded to binary32 once; 2u - 1 is exact in float64 and rounded once: the device's two fmas."""
    c = np.arange(paths, dtype=np.uint64)[:, None]
    h = np.arange(horizon, dtype=np.uint64)[None, :]
    assert 0 <= k < 1 << 36 and paths <= 1 << 16 and horizon <= 1 << 10
    w = philox_np(seed, (STREAM_PLAN << 48) | gid, (np.uint64(k) << np.uint64(26)) | (c << np.uint64(10)) | h)
    u = ((w.astype(np.float32).astype(np.float64) + 1.0) * 2.0 ** -32).astype(np.float32)
    return (2.0 * u.astype(np.float64) - 1.0).astype(np.float32)


def first_argmax(scores):
    """highest score, ties to the lowest index (np.argmax returns the first maximum)"""
    return np.argmax(scores, axis=-1)


def plan_scores_both(rec, par, acts, kind=0, dt=0.02, integ=0, prec="f64"):
    """Scores of every candidate under both objectives in one pass.  rec [N,40] / par [N,4]: the envs' records and
    parameters; acts [N,paths,horizon,4].  -> (reward [N,paths], position [N,paths], r): float64 sums -- REWARD of the step
    rewards, POSITION of -(o0^2 + o1^2 + o2^2) of the observation before each step; a candidate stops after its first done
    step -- and r, the largest |rel_pos| among the observations that entered a POSITION score."""
    orc = Oracle(prec)
    n, paths, horizon = acts.shape[:3]
    rec = np.asarray(rec, orc.dtype)
    r = np.ascontiguousarray(np.repeat(rec, paths, axis=0))
    p = np.ascontiguousarray(np.repeat(np.asarray(par, orc.dtype), paths, axis=0))
    assert r.shape == (n * paths, REC_LEN)
    obs = np.repeat(np.stack([orc.rel_obs(rec[i, 0:13], rec[i, 13:26]) for i in range(n)]), paths, axis=0)
    a = np.asarray(acts, orc.dtype).reshape(n * paths, horizon, 4)
    alive = np.ones(n * paths, bool)
    s_rew = np.zeros(n * paths, np.float64)
    s_pos = np.zeros(n * paths, np.float64)
    rmax = 0.0
    for h in range(horizon):
        d2 = np.sum(obs[alive, 0:3].astype(np.float64) ** 2, axis=1)
        s_pos[alive] -= d2
        rmax = max(rmax, float(np.sqrt(d2.max())) if d2.size else 0.0)
        obs, rew, _, flags, _ = orc.vec_step(r, p, np.ascontiguousarray(a[:, h]), kind=kind, dt=dt, integ=integ, auto_reset=False)
        s_rew[alive] += rew[alive].astype(np.float64)
        alive &= (flags & DONE_FLAGS) == 0
    return s_rew.reshape(n, paths), s_pos.reshape(n, paths), rmax


def plan_scores(rec, par, acts, kind=0, dt=0.02, integ=0, objective=REWARD, prec="f64"):
    """one objective's [N,paths] of plan_scores_both"""
    return plan_scores_both(rec, par, acts, kind, dt, integ, prec)[1 if objective == POSITION else 0]
