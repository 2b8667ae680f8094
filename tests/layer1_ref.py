"""Float64 references, input builders, bounds and checking functions of the layer-0 / layer-1 batch kernels of
csrc/layer1_kernels.hpp (k_drone_step, k_ctrl, k_transform, k_rel_obs) and of the hand-rolled device math beneath them (q_asin,
q_atan2, q_sincos of csrc/quadsim_device.hpp), shared by tests/test_layer1_cpu.py and tests/test_gpu_layer1.py.  numpy and
oracle/pyoracle.py only: no torch here.

References.  Oracle("f64") row by row on the exact float32 inputs (drone_step, ctrl_pid, ctrl_vel, rel_obs, quat2euler, euler2quat,
quat2rot, rot2euler); numpy float64 for asin / atan2 / sin / cos.  Nothing is left out of a comparison: what float32 cannot decide
(a limiter threshold, the saturation of r12, gimbal lock) is kept out of the INPUTS by construction, and the builders assert with
the float64 reference that every row is where it was meant to be.

Notation.  u = 2^-24 is half an ulp of a float32 in [1, 2): the relative error of one rounding.  N = |q|^2.  For a quaternion the
entries the Euler angles are taken from satisfy r10^2 + r11^2 = r02^2 + r22^2 = N^2 - r12^2 =: h^2, so N / h (= 1 / cos roll for a unit
quaternion) is the condition number of yaw and pitch, and 1 / sqrt(1 - r12^2) that of roll.

----------------------------------------------------------------------------------------------------------------------------------
Bounds of the device math (absolute error against float64 on the exact float32 argument).  tools/fit_polys.py reports, for each
polynomial evaluated in emulated float32 on its primary interval, the worst error of fit + evaluation (RES_*, its printed three
digits rounded up).  Every step outside the primary interval adds half an ulp of the scale it rounds at, and every float32
constant its representation error:

  q_sincos   RES_COS (the larger of the two polynomials: the quadrant fix-up may hand either one out as sin or as cos)
             + 2^-25, half an ulp of a result <= 1, for what the tool's sampling of roundings may have missed
             + 2^-25 when k != 0: the rounding of the reduced argument |r| < 1 (the first fma of the Cody-Waite reduction is exact:
               k * hi and x are multiples of ulp(x) and the difference is below 1; the second rounds once)
             + |k| * KF_ERR: what hi - lo misses of pi/2 (half an ulp of lo, 2^-49, plus float64's own pi/2)
             => 1.04e-7 on the primary interval, 1.34e-7 after a reduction, + 1.2e-11 at |x| = 1e4.
  q_asin     |x| <= 1/2: RES_ASIN_LO + 2^-25 (half an ulp of a result <= pi/6 < 1) = 6.9e-8; and for |x| <= 2^-6, where the result is
             x (1 + z P(z)) with z P(z) < 5e-5, one final rounding and next to nothing else: 2^-23 |asin x|.
             |x| >  1/2: RES_ASIN_HI (the tool rounds the square root correctly and the rest once)
             + |float32(pi/2) - pi/2| = 4.4e-8 (the tool subtracts from float64's pi/2)
             + 2^-24 s * 2 / sqrt(1 - s^2), s = sqrt((1 - |x|) / 2) <= 1/2: the hardware square root is good to 1 ulp, not 1/2
             + 2^-24: the rounding of r = asin(s) <= pi/6 before it is doubled
             => at most 2.7e-7.
  q_atan2    t = mn * rcp(mx): 1 ulp of rcp and half an ulp of the product, 1.5 * 2^-23 relative, through d atan / dt * t <= 1/2:
             0.75 * 2^-23 absolute (or 1.5 * 2^-23 relative to the result, t / ((1 + t^2) atan t) <= 1)
             + RES_ATAN_ABS (relative: RES_ATAN_REL)
             + 2^-24 + |float32(pi/2) - pi/2| when |y| > |x|: kHalfPi - r rounds at a result in [pi/4, pi/2]
             + 2^-23 + |float32(pi) - pi| when x < 0: kPi - r rounds at a result in [pi/2, pi]
             + 2^-126 where t is denormal
             => 1.9e-7 / 3.0e-7 / 5.1e-7 in the first / second / outer octants.
The hardware rcp, rsq and sqrt are good to 1 ulp (the instruction set's documented accuracy, and what the comment above q_rcp says).

Bounds of the transforms.  op 3 hands the functions out bit for bit: its bounds are the three above.  op 0 adds the float32
evaluation of the entries from the quaternion: |d r12|, |d r10|, |d r02| <= 2 u N (two products, one sum, doubled; |xy| + |wz| <= N / 2),
|d r11|, |d r22| <= 4 u N (four products, three sums of partial sums <= N); an error (dy, dx) of the arguments moves atan2 by at most
(|dy| + |dx|) / h: yaw, pitch <= atan2 bound + 6 u N / h, roll <= asin bound + 2 u N / sqrt(1 - r12^2).  The inputs keep N / h <= 8 and
|roll| <= 1.2, which puts these under the figures tests/test_gpu_parity.py asserts (4e-6; 2e-6 + 3e-7 / sqrt(1 - r12^2)).
op 1: a word is the sum of two terms, each a product of three factors with error e_r, e_p, e_y (the sincos bound of that half
angle); the weights of one angle's factors add up to at most 1 over the two terms (|cp cy| + |sp sy| <= 1, ...), as do the two terms
themselves, so: e_r + e_p + e_y + 3 u (two product roundings per term, one for the sum).  That is 5.8e-7 after reductions, LOOSER
than the 5e-7 test_gpu_parity.py asserts on its fixture: the sum of three worst cases is not attained, and the old figure was
measured.  check_transform asserts both.
op 2: inv = rsq(N): half of the 4 u of N (four products, three sums) plus 1 ulp of rsq: 4 u; n_i: 5 u; 2 n_i^2: 11 u; 2 w n_i: 6 u; the
sum: u.  |d entry| <= u (22 n_i^2 + 12 |w n_i| + |entry|), under 2e-6 + 2e-6 |entry| on the inputs; the diagonal is the constant 1.

Bounds of k_ctrl, stage by stage (each stage against float64 on that stage's exact float32 inputs):
  thrust     F = fma(m, az, m g); mode 0 az = 50 dz + 8 dvz: |d az| <= u (150 |dz| + 16 |dvz|); mode 1 az = dvz + 0.1 dv: u (2 |dvz| + 0.3 |dv|
             + |az|).  |dF| <= m |d az| + 2 u m g + u |F|.
  new qdes   quat_yaw_trig: sin / cos of yaw from (r10, r11) / h: E_yaw = 6 u N / h + 4 u (entries; rsq 1 ulp, h^2, the product); the half
             angles: E_half = 1.1 E_yaw + 6 u (sqrt and rcp 1 ulp each, on the branch that does not cancel).  phi_des, theta_des:
             ((|ax| + |ay|) (E_yaw + 3 u) + |d ax| + |d ay|) / g + 2 u |angle|, halved, plus the primary-interval sincos bound.  A word
             of the quaternion: e_r + e_p + E_half + 3 u as in op 1.  About 1.7e-6, under helpers.STATE_TOL, which is asserted too.
  moments    against the float64 attitude controller on the DEVICE's new qdes (exact float32): 10 x (roll of qdes - roll of the
             state), each roll good to its op 0 bound, plus the three roundings of each term.  End to end (against the float64
             controller throughout) the figure of test_gpu_parity.py stays: atol 2e-5 with rtol 1e-5.

State output of k_drone_step keeps helpers.STATE_TOL, observations keep helpers.OBS_TOL and the 2e-5 (1 + 5 |tan phi|) (1 + |ref|) form
of the relative rates: the project's own figures.

The limiter band.  The device decides on matrix entries, the reference on angles.  A float32 pre-clamp quaternion is within 1.5 u
per component of the float64 one (one rounding of the last fma; the stage errors of RK4 are scaled by dt), which moves r12 by at most
2 sum|q_i| 1.5 u <= 6 u, and its own evaluation by 2 u N, the constant sin 85deg by u / 2: 8.5 u on r12, through 1 / cos 85deg:
DELTA0["roll"] = 5.9e-6 rad.  Pitch and yaw: 8 u on r02 / r10, 10 u on r22 / r11, 0.2 u for the product with tan 5deg, through
N / h = 1 / cos roll <= 1 / cos 0.5 on the band rows: DELTA0["pitch"] = DELTA0["yaw"] = 1.3e-6 rad.  Outside +-DELTA0 the device and the float64
reference must take the same decision; inside they may differ and nothing is asserted.
"""
import numpy as np

from helpers import OBS_TOL, STATE_TOL
from lifecycle_ref import PAR_NOM, _all_distinct, bits, same_bits
from oracle.pyoracle import Oracle

f32, f64 = np.float32, np.float64

N_ENVS = (1, 63, 64, 65, 255, 256, 257, 1000)     # as lifecycle_ref.N_ENVS: one lane, the wave edges, the 256-thread block edges
DT = 0.02
MASS = PAR_NOM[0]                                 # 0.21, not the default 0.18
U = 2.0 ** -24
L85, L175 = np.deg2rad(85.0), np.deg2rad(175.0)
MARGIN = 1e-3                                     # rad: the distance of every matrix row from every limiter threshold
COND_MAX = 20.0                                   # N / h of every k_drone_step row (its state keeps helpers.STATE_TOL)
COND_OP0 = 8.0                                    # ... and of every op 0 row: 5.1e-7 + 6 u N / h stays under the old 4e-6
SENTINEL = np.full(1, 0xA5A5A5A5, np.uint32).view(f32)[0]

# what tools/fit_polys.py prints for the polynomials in use (atan deg 8, asin deg 4, the refitted sincos deg 2), rounded up
RES_ATAN_ABS, RES_ATAN_REL = 1.03e-7, 1.36e-7
RES_ASIN_LO, RES_ASIN_HI = 3.85e-8, 9.22e-8
RES_SIN, RES_COS = 4.37e-8, 7.39e-8
PIO2_ERR = abs(float(f32(np.pi / 2)) - np.pi / 2)             # 4.37e-8
PI_ERR = abs(float(f32(np.pi)) - np.pi)                       # 8.74e-8
KF_ERR = 2.0 ** -49 + 2.0 ** -53

# the argument domain of q_atan2 that include/quadsim.h states: max(|y|, |x|) in [2^ATAN2_LO, 2^(ATAN2_HI + 1)), or both zero.  Found on the
# MI355X by the binade sweep of tests/test_gpu_layer1.py (the largest run of binades without a failure, less one on each side).
ATAN2_LO, ATAN2_HI = -125, 124
# ... and of the quaternion of op 0 / op 2: |q| in [2^QUAT_LO, 2^(QUAT_HI + 1)) (the entries are quadratic in q), found the same way
QUAT_LO, QUAT_HI = -61, 61


# ---------------------------------------------------------------------------------------------------- bounds of the math
def sincos_bound(x):
    """q_sincos(x) against float64 sin / cos, per element"""
    x = np.asarray(x, f64)
    k = np.abs(np.rint(x * (2.0 / np.pi)))
    return RES_COS + 2.0 ** -25 + (k != 0) * 2.0 ** -25 + k * KF_ERR


def asin_bound(x):
    """q_asin(clamp(x)) against float64 asin, per element"""
    a = np.minimum(np.abs(np.asarray(x, f64)), 1.0)
    ref = np.arcsin(a)
    s = np.sqrt((1.0 - a) / 2.0)
    hi = RES_ASIN_HI + PIO2_ERR + 2.0 ** -24 * s * 2.0 / np.sqrt(1.0 - np.minimum(s * s, 0.25)) + 2.0 ** -24
    lo = np.where(a <= 2.0 ** -6, 2.0 ** -23 * ref + 2.0 ** -149, RES_ASIN_LO + 2.0 ** -25)
    return np.where(a > 0.5, hi, lo)


def atan2_bound(y, x):
    """q_atan2(y, x) against float64 atan2 for max(|y|, |x|) inside the stated domain, per element"""
    y, x = np.asarray(y, f64), np.asarray(x, f64)
    ay, ax = np.abs(y), np.abs(x)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    t = np.where(mx > 0, mn / np.where(mx > 0, mx, 1.0), 0.0)
    base = np.minimum(RES_ATAN_ABS + 0.75 * 2.0 ** -23, (RES_ATAN_REL + 1.5 * 2.0 ** -23) * np.arctan(t)) + 2.0 ** -126
    return base + (ay > ax) * (2.0 ** -24 + PIO2_ERR) + (x < 0) * (2.0 ** -23 + PI_ERR)


def angle_err(a, b):
    """|a - b| on the circle (an angle at +-pi may come out on either side)"""
    d = np.abs(np.asarray(a, f64) - np.asarray(b, f64))
    return np.minimum(d, np.abs(d - 2.0 * np.pi))


# ---------------------------------------------------------------------------------------------------- quaternion pieces
def _qmul(a, b):
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0); w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], -1)


def _axis(i, a):
    a = np.asarray(a, f64)
    q = np.zeros(a.shape + (4,))
    q[..., 0] = np.cos(a / 2); q[..., i] = np.sin(a / 2)
    return q


def quat_of(phi, theta, psi):
    """the unit quaternion quat2euler (utils/transform.py:94-120) maps to (phi, theta, psi): qz(psi) qx(phi) qy(theta), float64"""
    return _qmul(_axis(3, psi), _qmul(_axis(1, phi), _axis(2, theta)))


def entries(q):
    """the five matrix entries quat2euler reads, N and h, float64: dict of arrays"""
    q = np.asarray(q, f64)
    w, x, y, z = np.moveaxis(q, -1, 0)
    N = w * w + x * x + y * y + z * z
    r12 = 2 * (w * x + y * z)
    return dict(r10=2 * (x * y - w * z), r11=w * w - x * x + y * y - z * z, r12=r12, r02=2 * (x * z - w * y),
                r22=w * w - x * x - y * y + z * z, N=N, h=np.sqrt(np.maximum(N * N - r12 * r12, 0.0)))


def euler_bounds(q):
    """op 0 on the float32 quaternions q [n, 4]: (bound [n, 3], saturated [n]) in the order roll, pitch, yaw"""
    e = entries(q)
    sat = (e["r12"] >= 1.0) | (e["r12"] < -1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = e["N"] / e["h"]
        d12 = np.minimum(2 * U * e["N"], 1.0)
        # asin moves by at most d / sqrt(1 - r12^2), and never by more than its modulus of continuity acos(1 - d) (attained at +-1)
        roll = asin_bound(e["r12"]) + np.where(sat, 0.0, np.minimum(d12 / np.sqrt(np.maximum(1.0 - e["r12"] ** 2, 1e-300)), np.where(d12 > 1e-9, np.arccos(1.0 - d12), 1.01 * np.sqrt(2.0 * d12))))
    pitch = np.where(sat, 0.0, atan2_bound(-e["r02"], e["r22"]) + 6 * U * cond)
    yaw = atan2_bound(-e["r10"], e["r11"]) + 6 * U * cond
    return np.stack([roll, pitch, yaw], -1), sat


# ---------------------------------------------------------------------------------------------------- k_drone_step: inputs
def _rows64(fn, *arrays):
    return [fn(*[a[i] for a in arrays]) for i in range(arrays[0].shape[0])]


def integrate64(o64, s, up, par, dt, integ):
    """the state BEFORE Drone.attitude_limit, float64, from Oracle("f64").drone_df (quadrotor.py:126-134)"""
    s = np.asarray(s, f64); up = np.asarray(up, f64); par = np.asarray(par, f64)
    k1 = o64.drone_df(s, up, par)
    if integ == 0:
        return s + dt * k1
    k2 = o64.drone_df(s + 0.5 * dt * k1, up, par)
    k3 = o64.drone_df(s + 0.5 * dt * k2, up, par)
    k4 = o64.drone_df(s + dt * k3, up, par)
    return s + (dt / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def pre_clamp(o64, x, integ, dt=DT):
    """per row of the inputs x: the float64 Euler angles [n, 3] before the limiter, r12, N / h, and the distance [n] from the nearest
    decision the float32 path could take the other way: the three thresholds and the saturation of r12"""
    n = x["state"].shape[0]
    par = x["par"] if x["par"] is not None else np.tile(np.asarray(PAR_NOM, f32), (n, 1))
    ang, r12, cond = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    for i in range(n):
        s = integrate64(o64, x["state"][i], x["u_prev"][i], par[i], dt, integ)
        ang[i] = o64.quat2euler(s[6:10])
        e = entries(s[6:10])
        r12[i] = e["r12"]
        cond[i] = e["N"] / max(e["h"], 1e-300)
    sat = (r12 >= 1.0) | (r12 < -1.0)
    m = np.minimum(np.abs(np.abs(ang[:, 0]) - L85), np.abs(np.abs(ang[:, 2]) - L175))
    m = np.minimum(m, np.where(sat, np.inf, np.abs(np.abs(ang[:, 1]) - L85)))
    m = np.minimum(m, np.abs(np.abs(r12) - 1.0))
    return dict(angles=ang, r12=r12, cond=cond, sat=sat, margin=m)


def violated(pre):
    """[n, 3] bool: which of roll, pitch, yaw the float64 reference finds beyond its limit"""
    a = np.abs(pre["angles"])
    return np.stack([a[:, 0] >= L85, a[:, 1] >= L85, a[:, 2] >= L175], -1)


def _body(rs, m, rate=1.0):
    """everything of a drone_step input but the attitude: [m, 13] state with a zero quaternion, u_prev, u, par -- every word drawn
    from a continuous range"""
    s = np.zeros((m, 13))
    s[:, 0:3] = np.array((8.0, -50.0, 5.0)) + rs.uniform(-2, 2, (m, 3))
    s[:, 3:6] = rs.uniform(-2, 2, (m, 3))
    s[:, 10:13] = rs.uniform(-rate, rate, (m, 3))
    up = np.c_[rs.uniform(0.5, 3.5, m), rs.uniform(-5, 5, (m, 3)) * rate]
    u = np.c_[rs.uniform(-1.0, 10.0, m), rs.uniform(-0.1, 0.1, (m, 2)), rs.uniform(-0.1, 0.1, m)]      # per-rotor clamp [0, m g ~ 2]: some clamped
    par = np.asarray(PAR_NOM) * rs.uniform(0.85, 1.15, (m, 4))
    return s, up, u, par


def _pack(s, up, u, par, par_given):
    """float32, every word of the four arrays different"""
    every = _all_distinct(np.concatenate([s, up, u, par], 1).astype(f32))
    return dict(state=np.ascontiguousarray(every[:, 0:13]), u_prev=np.ascontiguousarray(every[:, 13:17]),
                u=np.ascontiguousarray(every[:, 17:21]), par=np.ascontiguousarray(every[:, 21:25]) if par_given else None)


def _take(x, keep, n):
    idx = np.nonzero(keep)[0]
    assert len(idx) >= n, "only %d of %d candidate rows are usable" % (len(idx), n)
    idx = idx[:n]
    return {k: (None if v is None else np.ascontiguousarray(v[idx])) for k, v in x.items()}


def drone_inputs(n, integ, par_given, seed=0):
    """n rows for a k_drone_step matrix case: attitudes over the whole range (so a part of the rows is limited), norms in [0.5, 2]
    on a quarter of them, the rotor clamp active on a part; every row >= MARGIN from every limiter threshold and from the
    saturation of r12, with N / h <= COND_MAX -- by construction: candidates are drawn in order and the first n that qualify are
    the input, none is left out afterwards"""
    o64 = Oracle("f64")
    rs = np.random.RandomState(1000 * seed + 10 * n + 2 * integ + int(par_given))
    m = 3 * n + 48
    s, up, u, par = _body(rs, m)
    q = quat_of(rs.uniform(-1.52, 1.52, m), rs.uniform(-1.9, 1.9, m), rs.uniform(-np.pi, np.pi, m))
    scale = np.where(rs.uniform(size=m) < 0.25, rs.uniform(0.5, 2.0, m), rs.uniform(0.97, 1.03, m))
    s[:, 6:10] = q * scale[:, None]
    x = _pack(s, up, u, par, par_given)
    pre = pre_clamp(o64, x, integ)
    return _take(x, (pre["margin"] >= 1.1 * MARGIN) & (pre["cond"] <= COND_MAX), n)


SUBSETS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]
PER_SUBSET = 36
EXACT_MINUS_ONE = np.array((0.5, -0.5, 0.5, -0.5), f32)      # N = 1, r12 = -1.0f exactly, all rates zero: survives both integrators


def limiter_inputs(integ, seed=0):
    """states whose integrated attitude violates each non-empty subset of {roll, pitch, yaw}: PER_SUBSET rows per subset, both signs of
    every violated angle; in the subsets with roll and without pitch, eight rows each reach roll = +-pi/2 on the saturated
    branches (r12 >= 1, r12 < -1) with un-normalised quaternions; one more row has r12 == -1.0f exactly, which is NOT saturated.
    -> (inputs, subset index per row or -1 for the last row)"""
    o64 = Oracle("f64")
    rs = np.random.RandomState(77 + 13 * seed + integ)
    parts, which = [], []
    for k, sub in enumerate(SUBSETS):
        m = 12 * PER_SUBSET
        sign = lambda: np.where(rs.uniform(size=m) < 0.5, -1.0, 1.0)                 # noqa: E731
        roll = sign() * (rs.uniform(L85 + 0.02, 1.518, m) if sub[0] else rs.uniform(0, 1.2, m))
        pitch = sign() * (rs.uniform(L85 + 0.02, 3.0, m) if sub[1] else rs.uniform(0, 1.3, m))
        yaw = sign() * (rs.uniform(L175 + 0.02, 3.13, m) if sub[2] else rs.uniform(0, 2.9, m))
        s, up, u, par = _body(rs, m, rate=0.05)
        s[:, 6:10] = quat_of(roll, pitch, yaw)
        saturate = np.zeros(m, bool)
        if sub[0] and not sub[1]:
            saturate[::3] = True
            s[saturate, 6:10] *= np.sqrt(rs.uniform(1.03, 1.08, saturate.sum()))[:, None]       # r12 = N sin(roll) > 1
        x = _pack(s, up, u, par, True)
        pre = pre_clamp(o64, x, integ)
        ok = (violated(pre) == np.array(sub, bool)).all(1) & (pre["margin"] >= 1.1 * MARGIN) & (pre["cond"] <= COND_MAX)
        pos = pre["angles"][:, int(np.argmax(sub))] > 0
        for is_sat, cnt in ((True, 8 if saturate.any() else 0), (False, PER_SUBSET - (8 if saturate.any() else 0))):
            for sg in (True, False):
                parts.append(_take(x, ok & (pre["sat"] == is_sat) & (saturate == is_sat) & (pos == sg), cnt // 2))
                which += [k] * (cnt // 2)
    body = _body(np.random.RandomState(5), 1)
    body[0][:, 6:10] = quat_of(0.1, 0.2, 0.3)
    last = _pack(*body, True)
    last["state"][0, 6:10] = EXACT_MINUS_ONE
    last["state"][0, 10:13] = 0
    last["u_prev"][0, 1:4] = 0
    parts.append(last); which.append(-1)
    x = {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in parts[0]}
    return x, np.array(which)


DELTA0 = {"roll": 8.5 * U / np.cos(L85), "pitch": 18.2 * U / np.cos(0.5), "yaw": 18.2 * U / np.cos(0.5)}
LADDER = (1e-6, 2e-6, 5e-6, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3)
BAND_ROWS = 64
AXES = ("roll", "pitch", "yaw")


def band_inputs(integ, seed=0):
    """states at rest (zero rates, no moments: the attitude survives the integration) whose roll / pitch / yaw sits at its threshold
    + delta, delta = +-LADDER, BAND_ROWS rows per rung and sign of delta, half of them at the negative threshold.
    -> (inputs, axis index [m], intended delta [m], actual delta [m]: |pre-clamp angle| - threshold in float64 on the float32 row)"""
    o64 = Oracle("f64")
    rs = np.random.RandomState(4242 + 7 * seed + integ)
    parts, axis, want = [], [], []
    for a in range(3):
        for d in [s * r for r in LADDER for s in (-1.0, 1.0)]:
            m = BAND_ROWS
            sg = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
            ang = [rs.uniform(-0.5, 0.5, m), rs.uniform(-1.0, 1.0, m), rs.uniform(-2.5, 2.5, m)]
            ang[a] = sg * ((L175 if a == 2 else L85) + d)
            s, up, u, par = _body(rs, m)                          # the rates and moments drawn here are zeroed below
            s[:, 6:10] = quat_of(*ang)
            parts.append(_pack(s, up, u, par, True))
            for p in (parts[-1]["state"][:, 10:13], parts[-1]["u_prev"][:, 1:4]):
                p[:] = 0                                           # _all_distinct must not have nudged a zero
            axis += [a] * m; want += [d] * m
    x = {k: np.ascontiguousarray(np.concatenate([p[k] for p in parts])) for k in parts[0]}
    pre = pre_clamp(o64, x, integ)
    axis = np.array(axis)
    thr = np.where(axis == 2, L175, L85)
    actual = np.abs(pre["angles"][np.arange(len(axis)), axis]) - thr
    return x, axis, np.array(want), actual


def outside_band(axis, actual):
    """rows whose decision float32 must share with float64"""
    d0 = np.array([DELTA0[AXES[a]] for a in axis])
    return np.abs(actual) >= d0


# ---------------------------------------------------------------------------------------------------- k_drone_step: reference, checker
def drone_ref(x, integ, dt=DT, par_nom=PAR_NOM, prec="f64"):
    """Oracle(prec).drone_step row by row on the exact float32 inputs -> dict(state [n, 13], u_prev [n, 4], limited uint8 [n])"""
    orc = Oracle(prec)
    n = x["state"].shape[0]
    par = x["par"] if x["par"] is not None else np.tile(np.asarray(par_nom, f32), (n, 1))
    out = dict(state=np.zeros((n, 13), orc.dtype), u_prev=np.zeros((n, 4), orc.dtype), limited=np.zeros(n, np.uint8))
    for i in range(n):
        out["state"][i], out["u_prev"][i], out["limited"][i] = orc.drone_step(x["state"][i], x["u_prev"][i], x["u"][i], par[i], dt, integ)
    return out


def as_device(ref, limited_given=True):
    """a reference cast to what a device would hand back (limited: the sentinel bytes when the pointer was NULL)"""
    return dict(state=ref["state"].astype(f32), u_prev=ref["u_prev"].astype(f32),
                limited=ref["limited"].copy() if limited_given else np.full(len(ref["limited"]), 0xA5, np.uint8))


def _ratio(got, want, rtol, atol):
    want = np.asarray(want, f64)
    return np.abs(np.asarray(got, f64) - want) / (atol + rtol * np.abs(want))


def check_drone_step(before, after, ref, limited_given=True):
    """The whole contract of qs_drone_step.  before: the inputs (state, u_prev, u, par or None) and limited = the bytes of the
    limited buffer before the call; after: state, u_prev, limited (the buffer, also when NULL was passed) and, if present, u / par
    as they stand after the call; ref: drone_ref.  Every element of every row.  -> {"state", "u_prev"}: worst error / bound"""
    n = before["state"].shape[0]
    st, up, lim = (np.ascontiguousarray(after[k]) for k in ("state", "u_prev", "limited"))
    assert st.shape == (n, 13) and up.shape == (n, 4) and lim.shape == (n,) and st.dtype == f32 and up.dtype == f32
    for k in ("u", "par"):
        if after.get(k) is not None:
            assert same_bits(after[k], before[k]), "the input %s was written" % k
    if limited_given:
        assert np.array_equal(lim, ref["limited"]), "limited differs in rows %s" % np.nonzero(lim != ref["limited"])[0][:8].tolist()
    else:
        assert np.array_equal(lim, np.asarray(before["limited"], np.uint8)), "limited was written although NULL was passed"
    assert np.isfinite(st).all() and np.isfinite(up).all()
    hit = ref["limited"] != 0
    assert not bits(st[hit][:, 10:13]).any(), "body rates not +0.0 after the attitude limiter fired"
    ratios = {"state": float(_ratio(st, ref["state"], **STATE_TOL).max()), "u_prev": float(_ratio(up, ref["u_prev"], 1e-5, 1e-5).max())}
    for k, v in ratios.items():
        assert v <= 1.0, "%s: error / bound = %.3f at %s" % (k, v, np.argwhere(_ratio(after[k], ref[k], 1e-5, 1e-5) > 1.0)[:4].tolist())
    return ratios


def first_axis_wins(x, ref, integ, dt=DT, par_nom=PAR_NOM):
    """a WRONG limiter for the CPU tests: the quaternion of every limited row rebuilt with the first violated axis clamped, not the last"""
    from lifecycle_ref import euler2quat64
    o64 = Oracle("f64")
    pre = pre_clamp(o64, x, integ, dt)
    out = {k: v.copy() for k, v in ref.items()}
    v = violated(pre)
    for i in np.nonzero(ref["limited"])[0]:
        a = int(np.argmax(v[i]))
        e = pre["angles"][i].copy()
        e[a] = np.copysign(L175 if a == 2 else L85, e[a])
        out["state"][i, 6:10] = euler2quat64(e)
    return out


# ---------------------------------------------------------------------------------------------------- k_ctrl
def ctrl_inputs(n, seed=0):
    """state_des, state, state_last [n, 13] float32, every word different: desired attitudes within 0.3 rad of level at any yaw up to
    3 rad, states within 0.6 rad, norms within 2 % of 1, nonzero desired rates (words 10, 11 must come back zero, word 12 untouched)"""
    rs = np.random.RandomState(300 + 17 * seed + n)
    sd, s = np.zeros((n, 13)), np.zeros((n, 13))
    sd[:, 0:3] = np.array((10.0, -50.0, 5.0)) + rs.uniform(-0.3, 0.3, (n, 3))
    sd[:, 3:6] = rs.uniform(-0.3, 0.3, (n, 3))
    sd[:, 6:10] = quat_of(rs.uniform(-0.3, 0.3, n), rs.uniform(-0.3, 0.3, n), rs.uniform(-3, 3, n)) * rs.uniform(0.98, 1.02, (n, 1))
    sd[:, 10:13] = rs.uniform(0.1, 0.5, (n, 3)) * np.where(rs.uniform(size=(n, 3)) < 0.5, -1, 1)
    s[:, 0:3] = sd[:, 0:3] + rs.uniform(-0.5, 0.5, (n, 3))
    s[:, 3:6] = rs.uniform(-0.5, 0.5, (n, 3))
    s[:, 6:10] = quat_of(rs.uniform(-0.6, 0.6, n), rs.uniform(-0.6, 0.6, n), rs.uniform(-3, 3, n)) * rs.uniform(0.98, 1.02, (n, 1))
    s[:, 10:13] = rs.uniform(-1, 1, (n, 3))
    sl = s + rs.uniform(-0.1, 0.1, (n, 13))
    every = _all_distinct(np.concatenate([sd, s, sl], 1).astype(f32))
    return dict(state_des=np.ascontiguousarray(every[:, :13]), state=np.ascontiguousarray(every[:, 13:26]),
                state_last=np.ascontiguousarray(every[:, 26:]))


def ctrl_ref(x, mode, mass=MASS, use_last=None, prec="f64"):
    """Oracle(prec).ctrl_pid / ctrl_vel row by row -> dict(u [n, 4], state_des [n, 13]).  use_last: the state_last the controller
    sees (default: the input's in mode 1; mode 0 has none)"""
    orc = Oracle(prec)
    n = x["state"].shape[0]
    m = float(f32(mass))
    out = dict(u=np.zeros((n, 4), orc.dtype), state_des=np.zeros((n, 13), orc.dtype))
    last = x["state_last"] if use_last is None else use_last
    for i in range(n):
        if mode == 0:
            out["u"][i], out["state_des"][i] = orc.ctrl_pid(x["state_des"][i], x["state"][i], m)
        else:
            out["u"][i], out["state_des"][i] = orc.ctrl_vel(x["state_des"][i], x["state"][i], last[i], m)
    return out


def moments64(state_des_after, state):
    """attitude_controller (PIDController.py:52-74) in float64 on a given mutated state_des and state -> [n, 3]"""
    o64 = Oracle("f64")
    sd, s = np.asarray(state_des_after, f64), np.asarray(state, f64)
    ed = np.array([o64.quat2euler(q) for q in sd[:, 6:10]]); en = np.array([o64.quat2euler(q) for q in s[:, 6:10]])
    w = sd[:, 10:13] - s[:, 10:13]
    return np.stack([-10.0 * (ed[:, 0] - en[:, 0]) + 5.1 * w[:, 0], -10.0 * (ed[:, 1] - en[:, 1]) + 5.1 * w[:, 1],
                     -9.5 * (ed[:, 2] - en[:, 2]) + 4.0 * w[:, 2]], -1), ed, en


def ctrl_bounds(x, mode, ref, state_des_after, mass=MASS):
    """the derived bounds of the module docstring, per element -> dict(thrust [n], quat [n], moments [n, 3])"""
    sd, s, sl = (np.asarray(x[k], f64) for k in ("state_des", "state", "state_last"))
    m, g = float(f32(mass)), 9.81
    dp, dv = sd[:, 0:3] - s[:, 0:3], sd[:, 3:6] - s[:, 3:6]
    if mode == 0:
        a = np.stack([-dp[:, 0] - 1.65 * dv[:, 0], -dp[:, 1] - 1.65 * dv[:, 1], 50 * dp[:, 2] + 8 * dv[:, 2]], -1)
        da_xy = U * (2 * np.abs(dp[:, :2]) + 3 * 1.65 * np.abs(dv[:, :2]) + np.abs(a[:, :2]))
        da_z = U * (150 * np.abs(dp[:, 2]) + 16 * np.abs(dv[:, 2]))
    else:
        d2 = s[:, 5] - sl[:, 5]
        a = np.stack([-0.7 * dv[:, 0], -0.7 * dv[:, 1], dv[:, 2] + 0.1 * d2], -1)
        da_xy = U * 3 * 0.7 * np.abs(dv[:, :2])
        da_z = U * (2 * np.abs(dv[:, 2]) + 0.3 * np.abs(d2) + np.abs(a[:, 2]))
    F = m * g + m * a[:, 2]
    thrust = m * da_z + 2 * U * m * g + U * np.abs(F)
    e = entries(sd[:, 6:10])
    e_yaw = 6 * U * e["N"] / e["h"] + 4 * U
    e_half = 1.1 * e_yaw + 6 * U
    axy = np.abs(a[:, 0]) + np.abs(a[:, 1])
    psi = np.arctan2(-e["r10"], e["r11"])
    des = np.stack([(a[:, 0] * np.sin(psi) - a[:, 1] * np.cos(psi)) / g, (a[:, 0] * np.cos(psi) + a[:, 1] * np.sin(psi)) / g], -1)
    d_des = ((axy * (e_yaw + 3 * U) + da_xy.sum(1)) / g)[:, None] + 2 * U * np.abs(des)
    e_rp = 0.5 * d_des + sincos_bound(0.5 * des)
    quat = e_rp.sum(1) + e_half + 3 * U
    # moments: on the device's own new state_des
    M, ed, en = moments64(state_des_after, x["state"])
    bd, _ = euler_bounds(np.asarray(state_des_after, f64)[:, 6:10])
    bn, _ = euler_bounds(s[:, 6:10])
    gain, rate_gain = np.array((10.0, 10.0, 9.5)), np.array((5.1, 5.1, 4.0))
    w = np.asarray(state_des_after, f64)[:, 10:13] - s[:, 10:13]
    moments = gain * (bd + bn) + U * (3 * gain * np.abs(ed - en) + 3 * rate_gain * np.abs(w) + np.abs(M))
    return dict(thrust=thrust, quat=quat, moments=moments, moments_ref=M)


def check_ctrl(before, after, ref, mode, mass=MASS):
    """The whole contract of qs_ctrl.  before: ctrl_inputs; after: dict(state_des [n, 13], u [n, 4]) and, if present, state /
    state_last as they stand after the call; ref: ctrl_ref.  -> worst error / bound per quantity"""
    sd0, sd1, u = before["state_des"], np.ascontiguousarray(after["state_des"]), np.ascontiguousarray(after["u"])
    n = sd0.shape[0]
    assert sd1.shape == (n, 13) and u.shape == (n, 4) and sd1.dtype == f32 and u.dtype == f32
    for k in ("state", "state_last"):
        if after.get(k) is not None:
            assert same_bits(after[k], before[k]), "the input %s was written" % k
    assert same_bits(sd1[:, 0:6], sd0[:, 0:6]), "state_des[:, 0:6] changed"
    assert same_bits(sd1[:, 12], sd0[:, 12]), "state_des[:, 12] changed"
    assert not bits(sd1[:, 10:12]).any(), "state_des[:, 10:12] is not +0.0"
    assert np.isfinite(sd1).all() and np.isfinite(u).all()
    b = ctrl_bounds(before, mode, ref, sd1, mass)
    want_q = ref["state_des"][:, 6:10].astype(f64)
    ratios = {
        "thrust": float((np.abs(u[:, 0].astype(f64) - ref["u"][:, 0]) / b["thrust"]).max()),
        "quat": float((np.abs(sd1[:, 6:10].astype(f64) - want_q) / b["quat"][:, None]).max()),
        "moments": float((np.abs(u[:, 1:4].astype(f64) - b["moments_ref"]) / b["moments"]).max()),
        # the figures tests/test_gpu_parity.py asserts, end to end
        "u_end_to_end": float(_ratio(u, ref["u"], 1e-5, 2e-5).max()),
        "state_des": float(_ratio(sd1, ref["state_des"], **STATE_TOL).max()),
    }
    assert (b["quat"] <= STATE_TOL["atol"]).all() and (b["thrust"] <= 2e-5).all(), "a derived bound is looser than the old figure"
    for k, v in ratios.items():
        assert v <= 1.0, "%s: error / bound = %.3f" % (k, v)
    return ratios


# ---------------------------------------------------------------------------------------------------- k_transform
WIDTH = {0: (4, 3), 1: (3, 4), 2: (4, 9), 3: (9, 3)}
Q_MINUS_ONE = np.array((1.0, -0.5, 0.5, 0.0), f32)            # r12 = -1.0f exactly with a pitch of atan2(1, 0.5): NOT saturated


def transform_inputs(op, n, seed=0):
    """[n, 4 | 3 | 4 | 9] float32, every word different (but for the planted special rows)"""
    rs = np.random.RandomState(900 + 31 * seed + 4 * n + op)
    if op == 0:
        m = 4 * n + 32
        q = quat_of(rs.uniform(-1.2, 1.2, m), rs.uniform(-3.1, 3.1, m), rs.uniform(-3.1, 3.1, m))
        scale = np.where(rs.uniform(size=m) < 0.5, 1.0, rs.uniform(0.7, 1.4, m))          # un-normalised: both saturated branches occur
        q = _all_distinct((q * scale[:, None]).astype(f32))
        e = entries(q)
        keep = (np.abs(np.abs(e["r12"]) - 1.0) >= MARGIN) & (e["N"] <= COND_OP0 * e["h"])
        x = q[keep][:n]
        assert len(x) == n
        if n >= 8:
            x[3] = Q_MINUS_ONE
        return np.ascontiguousarray(x)
    if op == 1:
        x = rs.uniform(-np.pi, np.pi, (n, 3))
        x[::5] = rs.uniform(-12.0, 12.0, (len(x[::5]), 3))                                 # a few reductions by more than one quadrant
        return _all_distinct(x.astype(f32))
    if op == 2:
        q = rs.normal(size=(n, 4))
        q *= (rs.uniform(0.5, 2.0, n) / np.linalg.norm(q, axis=1))[:, None]
        return _all_distinct(q.astype(f32))
    x = _all_distinct(rs.uniform(-1.5, 1.5, (n, 9)).astype(f32))
    kind = np.arange(n) % 4                                                                # R[5]: inside, >= 1, < -1, inside
    x[kind == 1, 5] = (1.0 + np.abs(x[kind == 1, 5])).astype(f32)
    x[kind == 2, 5] = (-1.0 - np.abs(x[kind == 2, 5]) - f32(1e-3)).astype(f32)
    inside = ((kind == 0) | (kind == 3)) & (np.abs(x[:, 5]) > 0.999)
    x[inside, 5] *= f32(0.6)
    if n >= 8:
        x[1, 5] = 1.0                                                                      # saturated
        x[2, 5] = -1.0                                                                     # not saturated
    return np.ascontiguousarray(x)


def transform_ref(op, x, prec="f64"):
    orc = Oracle(prec)
    fn = (orc.quat2euler, orc.euler2quat, lambda q: orc.quat2rot(q).reshape(9), orc.rot2euler)[op]
    return np.array([fn(r) for r in np.asarray(x, orc.dtype)])


ROT_OFF = (1, 2, 3, 5, 6, 7)                                  # the off-diagonal entries of quat2rot
_ROT_N = (2, 1, 2, 0, 1, 0)                                   # ... and the index of the n_i each is built from


def rot_bounds(q64, ref):
    """op 2 on the quaternions q64 [n, 4]: the bound of the six off-diagonal entries [n, 6] (module docstring)"""
    N = (q64 ** 2).sum(1)
    nv = q64[:, 1:4] / np.sqrt(N)[:, None]
    w = np.abs(q64[:, 0])
    return np.stack([U * (22 * nv[:, c] ** 2 + 12 * w * np.abs(nv[:, c]) + np.abs(ref[:, j])) for j, c in zip(ROT_OFF, _ROT_N)], -1)


def check_transform(op, before, after, ref):
    """before: the input [n, wi]; after: dict(out [n, wo], and x = the input after the call if present); ref: transform_ref"""
    x = np.ascontiguousarray(before, f32)
    out = np.ascontiguousarray(after["out"])
    n = x.shape[0]
    assert out.shape == (n, WIDTH[op][1]) and out.dtype == f32
    if after.get("x") is not None:
        assert same_bits(after["x"], x), "the input was written"
    assert np.isfinite(out).all()
    ref = np.asarray(ref, f64)
    x64 = x.astype(f64)
    if op in (0, 3):
        if op == 0:
            bound, sat = euler_bounds(x64)
            r12 = entries(x64)["r12"]
        else:
            r12 = x64[:, 5]
            sat = (r12 >= 1.0) | (r12 < -1.0)
            bound = np.stack([asin_bound(r12), np.where(sat, 0.0, atan2_bound(-x64[:, 2], x64[:, 8])), atan2_bound(-x64[:, 3], x64[:, 4])], -1)
        assert not bits(out[sat][:, 1]).any(), "pitch is not +0.0 on a saturated branch"
        assert same_bits(np.abs(out[sat][:, 0]), np.full(int(sat.sum()), np.pi / 2, f32)), "roll is not +-float32(pi/2) on a saturated branch"
        assert (ref[sat][:, 1] == 0).all() and ((np.abs(r12) > 1) <= sat).all()
        err = np.stack([np.abs(out[:, 0] - ref[:, 0]), angle_err(out[:, 1], ref[:, 1]), angle_err(out[:, 2], ref[:, 2])], -1)
        old = np.stack([2e-6 + 3e-7 / np.sqrt(np.maximum(1 - np.minimum(r12 ** 2, 1), 1e-7)), np.full(n, 4e-6), np.full(n, 4e-6)], -1)
        assert (bound <= old).all(), "a derived bound is looser than the old figure"
        ratios = {"roll": float((err[:, 0] / bound[:, 0]).max()), "pitch": float((err[~sat][:, 1] / bound[~sat][:, 1]).max()) if (~sat).any() else 0.0,
                  "yaw": float((err[:, 2] / bound[:, 2]).max())}
    elif op == 1:
        bound = sincos_bound(0.5 * x64).sum(1) + 3 * U
        err = np.abs(out.astype(f64) - ref).max(1)
        ratios = {"quat": float((err / bound).max()), "quat_old_5e-7": float(err.max() / 5e-7)}
    else:
        assert same_bits(out[:, [0, 4, 8]], np.ones((n, 3), f32)), "the diagonal is not the constant 1"
        bound = rot_bounds(x64, ref)
        err = np.abs(out[:, ROT_OFF].astype(f64) - ref[:, ROT_OFF])
        assert (bound <= 2e-6 + 2e-6 * np.abs(ref[:, ROT_OFF])).all(), "a derived bound is looser than the old figure"
        ratios = {"rot": float((err / bound).max())}
    for k, v in ratios.items():
        assert v <= 1.0, "op %d %s: error / bound = %.3f" % (op, k, v)
    return ratios


# ---------------------------------------------------------------------------------------------------- k_rel_obs
def rel_obs_inputs(n, seed=0):
    """chaser, target [n, 13] float32, every word different; relative roll |phi| <= 1.2 rad, never saturated, both atan2 pairs of the
    relative "rotation" with a hypotenuse >= 0.2 -- by construction, checked with the float64 reference"""
    o64 = Oracle("f64")
    rs = np.random.RandomState(500 + 3 * seed + n)
    m = 4 * n + 32

    def drone(base):
        s = np.zeros((m, 13))
        s[:, 0:3] = np.array(base) + rs.uniform(-1, 1, (m, 3))
        s[:, 3:6] = rs.uniform(-1, 1, (m, 3))
        s[:, 6:10] = quat_of(rs.uniform(-0.45, 0.45, m), rs.uniform(-0.45, 0.45, m), rs.uniform(-3, 3, m)) * rs.uniform(0.98, 1.02, (m, 1))
        s[:, 10:13] = rs.uniform(-1, 1, (m, 3))
        return s
    every = _all_distinct(np.concatenate([drone((8.0, -50.0, 5.0)), drone((10.0, -50.0, 5.0))], 1).astype(f32))
    sc, st = every[:, :13], every[:, 13:]
    keep = np.zeros(m, bool)
    for i in range(m):
        A, B = o64.quat2rot(sc[i, 6:10]), o64.quat2rot(st[i, 6:10])
        R = B @ A.T
        keep[i] = abs(R[1, 2]) <= np.sin(1.2) and np.hypot(R[1, 0], R[1, 1]) >= 0.2 and np.hypot(R[0, 2], R[2, 2]) >= 0.2
    idx = np.nonzero(keep)[0][:n]
    assert len(idx) == n
    return dict(chaser=np.ascontiguousarray(sc[idx]), target=np.ascontiguousarray(st[idx]))


def rel_obs_ref(x, prec="f64"):
    orc = Oracle(prec)
    return np.array([orc.rel_obs(x["chaser"][i], x["target"][i]) for i in range(x["chaser"].shape[0])])


def check_rel_obs(before, after, ref):
    """before: rel_obs_inputs; after: dict(obs [n, 12], and chaser / target after the call if present); ref: rel_obs_ref"""
    obs = np.ascontiguousarray(after["obs"])
    n = before["chaser"].shape[0]
    assert obs.shape == (n, 12) and obs.dtype == f32
    for k in ("chaser", "target"):
        if after.get(k) is not None:
            assert same_bits(after[k], before[k]), "the input %s was written" % k
    assert np.isfinite(obs).all()
    ref = np.asarray(ref, f64)
    assert (np.abs(ref[:, 6]) <= 1.2).all()
    rate_bound = 2e-5 * (1.0 + 5.0 * np.abs(np.tan(ref[:, 6])))[:, None] * (1.0 + np.abs(ref[:, 9:]))
    ratios = {"obs": float(_ratio(obs[:, :9], ref[:, :9], **OBS_TOL).max()),
              "rates": float((np.abs(obs[:, 9:].astype(f64) - ref[:, 9:]) / rate_bound).max())}
    for k, v in ratios.items():
        assert v <= 1.0, "%s: error / bound = %.3f" % (k, v)
    return ratios


# ---------------------------------------------------------------------------------------------------- the math sweeps
def _ulps_around(v, k):
    """every float32 within k ulps of v (v > 0), and their negatives"""
    b = int(np.asarray(v, f32).view(np.uint32))
    a = (b + np.arange(-k, k + 1, dtype=np.int64)).astype(np.uint32).view(f32)
    return np.concatenate([a, -a])


def _rot_rows(m):
    """[m, 9] rot2euler inputs with fixed, harmless entries: pitch = atan2(-0.5, 0.75) and yaw = atan2(0.25, 0.5) unless overwritten"""
    R = np.zeros((m, 9), f32)
    R[:, [0, 4, 8]] = (1.0, 0.5, 0.75)
    R[:, 2], R[:, 3] = 0.5, -0.25
    return R


def asin_sweep():
    """op 3 rows whose R[5] covers: a uniform grid over [-1, 1], every float32 within 2^12 ulps of +-1/2 (the branch switch) and within
    2^16 ulps of +-1 (on both sides: the clamp and the saturation test), +-0, nextafter(+-1) both ways -> (R [m, 9], x [m])"""
    one = f32(1.0)
    x = np.concatenate([np.linspace(-1.0, 1.0, 2 ** 20 + 1).astype(f32), _ulps_around(0.5, 2 ** 12), _ulps_around(1.0, 2 ** 16),
                        np.array([0.0, -0.0, np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), -np.nextafter(one, f32(2)),
                                  -np.nextafter(one, f32(0)), 1.0, -1.0], f32)])
    R = _rot_rows(len(x))
    R[:, 5] = x
    return R, x


def check_asin_sweep(R, out):
    """-> worst error / bound of q_asin; the saturation test and the clamp are exact"""
    x = R[:, 5].astype(f64)
    sat = (x >= 1.0) | (x < -1.0)
    assert np.isfinite(out).all()
    assert not bits(np.ascontiguousarray(out[sat][:, 1])).any(), "pitch not +0.0 where r12 >= 1 or r12 < -1"
    assert same_bits(out[~sat][:, 1], np.full(int((~sat).sum()), out[0, 1], f32)) and out[0, 1] != 0, "pitch differs among unsaturated rows"
    assert same_bits(np.abs(out[np.abs(x) >= 1][:, 0]), np.full(int((np.abs(x) >= 1).sum()), np.pi / 2, f32)), "asin(clamp) is not float32(pi/2)"
    zero = x == 0
    assert same_bits(out[zero][:, 0], R[zero][:, 5]), "asin(+-0) is not +-0"
    assert (np.signbit(out[:, 0]) == np.signbit(R[:, 5])).all(), "asin lost the sign"
    return float((np.abs(out[:, 0].astype(f64) - np.arcsin(np.clip(x, -1, 1))) / asin_bound(x)).max())


def _on_square(a):
    """(sin a, cos a) scaled so that the larger magnitude is 1"""
    s, c = np.sin(a), np.cos(a)
    m = np.maximum(np.abs(s), np.abs(c))
    return s / m, c / m


def atan2_sweep(lo=None, hi=None, m=2 ** 20, seed=3):
    """op 3 rows: the pitch pair (-R[2], R[8]) and the yaw pair (-R[3], R[4]) each carry (y, x) with angles uniform on the circle and
    max(|y|, |x|) log-uniform over the stated domain; then the special rows: the four axes with both signs of zero, (0, 0) in all four
    sign combinations, |y| == |x|, and ratios min / max = 2^-k down to where the quotient underflows -> R [m', 9]"""
    lo = ATAN2_LO if lo is None else lo
    hi = ATAN2_HI + 1 if hi is None else hi
    rs = np.random.RandomState(seed)
    R = _rot_rows(m)
    for cy, cx in ((2, 8), (3, 4)):
        s, c = _on_square(rs.uniform(-np.pi, np.pi, m))
        mag = 2.0 ** rs.uniform(lo, hi - 1e-6, m)
        R[:, cy], R[:, cx] = (-s * mag).astype(f32), (c * mag).astype(f32)
    z = [0.0, -0.0]
    pairs = [(y, x) for y in z for x in z]                                               # (0, 0) x 4
    pairs += [(y, x) for y in z for x in (1.0, -1.0, 3.0e20, -2.0e-20)] + [(y, x) for x in z for y in (1.0, -1.0, 3.0e20, -2.0e-20)]
    pairs += [(sy * v, sx * v) for v in (1.0, 0.3, 2.0 ** ATAN2_LO, 2.0 ** ATAN2_HI, 7.0e-12) for sy in (1, -1) for sx in (1, -1)]
    for k in range(0, 151):
        for big in (1.0, 2.0 ** 60, 2.0 ** ATAN2_HI):
            small = big * 2.0 ** -k
            if small >= 2.0 ** -149:
                pairs += [(small, big), (-big, small), (small, -big), (big, -small)]
    S = _rot_rows(len(pairs))
    y, x = np.array(pairs, f64).T
    S[:, 2], S[:, 8] = (-y).astype(f32), x.astype(f32)
    S[:, 3], S[:, 4] = (-x).astype(f32), y.astype(f32)                                   # the yaw pair: the same with y and x exchanged
    return np.concatenate([R, S])


def check_atan2_sweep(R, out, tag=""):
    """-> worst error / bound of q_atan2 over both pairs; zeros bit for bit against numpy.arctan2"""
    assert np.isfinite(out).all()
    worst = 0.0
    for (cy, cx), col in (((2, 8), 1), ((3, 4), 2)):
        y, x = -R[:, cy].astype(f64), R[:, cx].astype(f64)
        ref = np.arctan2(y, x)
        got = out[:, col].astype(f64)
        both0 = (y == 0) & (x == 0)
        assert same_bits(out[both0][:, col], ref[both0].astype(f32)), "atan2(+-0, +-0) differs from numpy.arctan2: %s -> %s, numpy %s" % (
            np.c_[y[both0], x[both0]][:4].tolist(), got[both0][:4].tolist(), ref[both0][:4].tolist())
        ok = ~both0
        assert (np.signbit(got[ok]) == np.signbit(y[ok])).all(), "atan2 lost the sign of y"
        worst = max(worst, float((np.abs(got[ok] - ref[ok]) / atan2_bound(y[ok], x[ok])).max()))
    return worst


def domain_sweep(per_binade=256, seed=11):
    """op 3 rows for the measurement of the domain of q_atan2: for every binade e of float32 (denormals included, -149 .. 127),
    per_binade (y, x) on each pair with max(|y|, |x|) in [2^e, 2^(e + 1)) -> (R, binade per row)"""
    rs = np.random.RandomState(seed)
    es = np.repeat(np.arange(-149, 128), per_binade)
    m = len(es)
    R = _rot_rows(m)
    for cy, cx in ((2, 8), (3, 4)):
        s, c = _on_square(rs.uniform(-np.pi, np.pi, m))
        mag = 2.0 ** es * rs.uniform(1.0, 1.999, m)
        R[:, cy], R[:, cx] = (-s * mag).astype(f32), (c * mag).astype(f32)
    return R, es


def clean_binades(R, es, out):
    """the largest run of binades in which every result is finite and inside atan2_bound -> (first, last)"""
    bad = np.zeros(len(es), bool)
    for (cy, cx), col in (((2, 8), 1), ((3, 4), 2)):
        y, x = -R[:, cy].astype(f64), R[:, cx].astype(f64)
        got = out[:, col].astype(f64)
        with np.errstate(invalid="ignore"):
            bad |= ~(np.abs(got - np.arctan2(y, x)) <= atan2_bound(y, x))
    dirty = np.unique(es[bad])
    best, start = (0, -1), -149
    for e in list(dirty) + [128]:
        if e - 1 - start > best[1] - best[0]:
            best = (start, e - 1)
        start = e + 1
    return int(best[0]), int(best[1])


def quat_domain_sweep(per_binade=64, seed=12):
    """op 0 rows for the measurement of the quaternion domain: attitudes with |roll| <= 1.2 at |q| = 2^e (1 .. 2), e = -75 .. 63
    -> (q [m, 4], e per row)"""
    rs = np.random.RandomState(seed)
    es = np.repeat(np.arange(-75, 64), per_binade)
    m = len(es)
    q = quat_of(rs.uniform(-1.2, 1.2, m), rs.uniform(-3.1, 3.1, m), rs.uniform(-3.1, 3.1, m)) * (2.0 ** es * rs.uniform(1.0, 1.999, m))[:, None]
    return q.astype(f32), es


def clean_quat_binades(q, es, out, rot):
    """the largest run of binades of |q| in which op 0 (out) is finite and inside euler_bounds (rows within MARGIN of the saturation
    of r12 do not count either way) and op 2 (rot) is finite, inside rot_bounds and has its unit diagonal -> (first, last)"""
    q64 = q.astype(f64)
    ref = transform_ref(0, q64)
    with np.errstate(all="ignore"):
        ref2 = transform_ref(2, q64)
        bad2 = ~(np.abs(rot[:, ROT_OFF].astype(f64) - ref2[:, ROT_OFF]) <= rot_bounds(q64, ref2)).all(1) | (rot[:, [0, 4, 8]] != 1).any(1)
        bound, sat = euler_bounds(q64)
        r12 = entries(q64)["r12"]
        err = np.stack([np.abs(out[:, 0] - ref[:, 0]), angle_err(out[:, 1], ref[:, 1]), angle_err(out[:, 2], ref[:, 2])], -1)
        bad = ~(err <= bound).all(1) & (np.abs(np.abs(r12) - 1.0) >= MARGIN) | bad2
    dirty = np.unique(es[bad])
    best, start = (0, -1), int(es.min())
    for e in list(dirty) + [int(es.max()) + 1]:
        if e - 1 - start > best[1] - best[0]:
            best = (start, e - 1)
        start = e + 1
    return int(best[0]), int(best[1])


SINCOS_RANGES = (np.pi / 4, np.pi, 12.0, 1e3, 1e4)


def sincos_sweep(per_range=2 ** 18):
    """op 1 rows (2 a, 0, 0), which give (cos a, sin a, 0, 0) exactly: a uniform on +-pi/4, +-pi, +-12, +-1e3 and +-1e4, and every
    float32 within 2^10 ulps of the first 64 odd multiples of pi/4 (the quadrant switches) -> (x [m, 3], a [m] float32)"""
    a = [np.linspace(-r, r, per_range).astype(f32) for r in SINCOS_RANGES]
    a += [_ulps_around((2 * j + 1) * np.pi / 4, 2 ** 10) for j in range(64)]
    a = np.concatenate(a)
    x = np.zeros((len(a), 3), f32)
    x[:, 0] = a * f32(2.0)                                      # exact; the kernel halves it again, exactly
    return x, a


def check_sincos_sweep(a, out):
    """-> (worst error / bound of sin, of cos)"""
    assert np.isfinite(out).all()
    assert not out[:, 2:].any(), "euler2quat(x, 0, 0) has a y or z component"
    a64 = a.astype(f64)
    b = sincos_bound(a64)
    return float((np.abs(out[:, 1] - np.sin(a64)) / b).max()), float((np.abs(out[:, 0] - np.cos(a64)) / b).max())
