"""Float64 reference of qs_mppi_plan, built only from what oracle/pyoracle.py exposes and from tests/shooting_ref.py
(philox_np for the words, plan_scores_both for the roll-outs).  A helper module, not a test.

The contract is that of include/quadsim.h: in iteration `it` candidate c >= 1 is clamp(fma(sigma, z[c][h], U[h]), -1, 1) in
float32, candidate 0 is clamp(U[h]); z is the caller's noise or Box-Muller on the four words of Philox block
(1 << 63) | (k << 30) | (it << 26) | (c << 10) | h of subsequence (5 << 48) | gid; the new nominal is the mean of the candidates
weighted by exp((S - Smax) / lam), float64 throughout, a NaN score weighing nothing."""
import numpy as np

import shooting_ref
from shooting_ref import POSITION, REWARD, STREAM_PLAN  # noqa: F401

K_BITS, IT_BITS, C_BITS, H_BITS = 33, 4, 16, 10


def block_index(k, it, c, h):
    assert 0 <= k < 1 << K_BITS and 0 <= it < 1 << IT_BITS and 0 <= c < 1 << C_BITS and 0 <= h < 1 << H_BITS
    return (1 << 63) | (k << 30) | (it << 26) | (c << 10) | h


def words(seed, gid, k, it, paths, horizon):
    """[paths, horizon, 4] uint32: the Philox words behind candidate c, step h of iteration `it` (row 0 is never drawn on the
    device; it is generated here all the same so that row c is candidate c)"""
    assert 0 <= k < 1 << K_BITS and 0 <= it < 1 << IT_BITS and paths <= 1 << C_BITS and horizon <= 1 << H_BITS
    c = np.arange(paths, dtype=np.uint64)[:, None]
    h = np.arange(horizon, dtype=np.uint64)[None, :]
    base = np.uint64((1 << 63) | (k << 30) | (it << 26))
    return shooting_ref.philox_np(seed, (STREAM_PLAN << 48) | gid, base | (c << np.uint64(10)) | h)


def normals(seed, gid, k, it, paths, horizon):
    """[paths, horizon, 4] float64 Box-Muller on the same words: u = the device's float32 (0,1] uniform (rounded as in
    shooting_ref.actions_fast), then everything in float64; (w0, w1) -> z0 = r cos, z1 = r sin, (w2, w3) -> z2, z3"""
    w = words(seed, gid, k, it, paths, horizon)
    u = ((w.astype(np.float32).astype(np.float64) + 1.0) * 2.0 ** -32).astype(np.float32).astype(np.float64)
    z = np.empty(u.shape, np.float64)
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(-2.0 * np.log(u[..., a]))
        th = 2.0 * np.pi * u[..., b]
        z[..., a], z[..., b] = r * np.cos(th), r * np.sin(th)
    return z


def fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays: the product is exact in float64; the sum is taken with its rounding error
    (two-sum), and where the float64 sum sits exactly on a float32 tie the error decides the direction -- one rounding of the
    exact value, as the device's v_fma_f32 makes"""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    out = s.astype(np.float32)
    bits = np.ascontiguousarray(s).view(np.uint64)
    tie = ((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) & (err != 0.0) & np.isfinite(s)
    if tie.any():
        lo = (bits & ~np.uint64(0x1FFFFFFF)).view(np.float64).astype(np.float32)          # towards zero: exact in float32
        hi = np.nextafter(lo, np.where(s > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        away = np.sign(err) == np.sign(s)
        out = np.where(tie, np.where(away, hi, lo), out)
    return out.astype(np.float32)


def candidates32(U, sigma, z):
    """U [N,horizon,4] float32 nominal, z [paths,horizon,4] float32 noise shared by the envs -> [N,paths,horizon,4] float32:
    row 0 clamp(U), row c clamp(fma(sigma, z[c], U))"""
    U = np.asarray(U, np.float32)
    z = np.asarray(z, np.float32)
    out = fma32(np.float32(sigma), z[None], U[:, None])
    out = np.clip(out, np.float32(-1.0), np.float32(1.0))
    out[:, 0] = np.clip(U, np.float32(-1.0), np.float32(1.0))
    return out


def update64(scores, cands, lam, U=None):
    """scores [N,paths] float64, cands [N,paths,horizon,4] -> the new nominal [N,horizon,4] in float64 (not rounded).  Rows
    whose scores are all NaN keep U (zeros if U is None)."""
    S = np.asarray(scores, np.float64)
    a = np.asarray(cands, np.float64)
    lam = np.float64(np.float32(lam))
    valid = ~np.isnan(S)
    smax = np.max(np.where(valid, S, -np.inf), axis=1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((S - smax) / lam)
    w = np.where(np.isnan(w), 0.0, w)
    sw = w.sum(axis=1)
    keep = np.zeros(a.shape[:1] + a.shape[2:]) if U is None else np.asarray(U, np.float64)
    num = np.einsum("np,nphi->nhi", w, a)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = num / sw[:, None, None]
    return np.where((sw > 0)[:, None, None], mean, keep)


def plan64(rec, par, U, sigma, z, lam, objective=REWARD, kind=0, dt=0.02, integ=0):
    """one full iteration on the float64 oracle from records rec [N,40] and parameters par [N,4]: the float32 candidates of
    candidates32, their float64 scores, the float64 update -> (new nominal [N,horizon,4] float64, scores [N,paths], r)"""
    cands = candidates32(U, sigma, z)
    s_rew, s_pos, r = shooting_ref.plan_scores_both(rec, par, cands, kind=kind, dt=dt, integ=integ)
    S = s_pos if objective == POSITION else s_rew
    return update64(S, cands, lam, U), S, r
