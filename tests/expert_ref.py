"""Float64 reference, error scale and shared inputs of the PID-expert kernels of csrc/expert_rollout.hpp (test helper; CPU only,
numpy only): k_expert_action and the expert inside k_expert_rollout / k_expert_evaluate.

expert64() restates oracle/quadsim_oracle.c:qso_expert_action, vectorised over envs: the des-vel rule
(run_expert_policy.py:57-59), vel_controller with state_last = state (PIDController.py:106-141), desired_attitude rewriting
state_des[6:12] (:116-134), attitude_controller (:52-74), the inverse rotor map and (f - mean) / mean, not clipped.  In the same
pass it builds a first-order error scale E per action: the sum of the magnitudes of everything that is summed into it, every
stage handing its scale on through the next stage's coefficients (all E are in units of 2^-24):

    des_vel       E_vd  = kp (|p_t| + 0.2 + |p_c|) + kd |v_c|                      (0 on a first step: the word is kept)
    acceleration  E_acc = c (E_vd + |v_d| + |v_c|),  c = 0.7, 0.7, 1.0;  thrust  E_F = m (g + |a_z| + E_acc,z)
    desired yaw   E_psi = ANGLE(q_des)              ANGLE(q) = 3 cond(q) + 2,  cond(q) = 1 / sqrt(1 - r12(q)^2)
    phi_des       E_phi = (E_acc,x |sin psi| + E_acc,y |cos psi| + |a_x sin psi| + |a_y cos psi|
                           + (|a_x cos psi| + |a_y sin psi|) E_psi) / g + |phi_des|,          theta_des alike
    desired Euler angles, read back from the rewritten quaternion:  |J| (E_phi, E_theta, E_psi) + ANGLE(q_new)
                  J = d quat2euler(euler2quat(phi, theta, psi)) / d (phi, theta, psi), central differences in float64
    chaser Euler angles  ANGLE(q_chaser)
    moments       E_M   = 10 (E_d + E_n + |d| + |n|) + 5.1 |w|  (roll, pitch);  9.5 (...) + 4 (|w_des,z| + |w_z|)  (yaw)
    rotor forces  E_f   = (E_F + |F|) / 4 + (E_M + |M|) / (2 L) + (E_Mz + |M_z|) / (4 lambda)
    action        E     = (E_f + |f|) / mean + 1 + |a|,   mean = m g / 2

ANGLE(q): the five r_ij of quat2euler are two products and a sum of magnitudes <= 1 (3 roundings); asin and both atan2 have
the same condition number 1 / sqrt(1 - r12^2) on a unit quaternion (hypot(r02, r22) = hypot(r10, r11) = sqrt(1 - r12^2)); + 2
for the kernel's own asin / atan2 (9.3e-8 and 1.1e-7 absolute, csrc/quadsim_device.hpp: 1.6 and 1.9 x 2^-24).  The new
state_des gets a scale built the same way: [3:6] E_vd, [6:10] (E_phi + E_theta + E_psi) / 2 + QUAT (three products and a sum of
half-angle sines and cosines), [10:12] 0 -- those two words are exact zeros.

A float32 result must satisfy |err| <= KAPPA_EXPERT * 2^-24 * E on EVERY element: the expert has no threshold, nothing is
excluded.  Worst ratios err / (2^-24 E) over inputs() below (three regimes x three gain pairs x 1000 envs = 9000 draws on the
CPU; on the GPU the draws of tests/test_gpu_expert_matrix.py), actions | state_des:

    float32 oracle (libm), nominal / mid / hard             0.018 | 0.198    0.290 | 0.617    0.546 | 1.979    CPU
    numpy float32 expert (expert32), nominal / mid / hard   0.018 | 0.198    0.343 | 0.617    0.546 | 1.979    CPU
    k_expert_action<0>, nominal / mid / hard                0.014 | 0.189    0.196 | 0.421    0.332 | 1.673    MI355X
    k_expert_action<1>, nominal / mid / hard                0.017 | 0.189    0.261 | 0.421    0.471 | 1.673    MI355X
    the expert of the 14 roll-out rows, every step judged (worst row)                         0.220 | 1.579    MI355X
    wrong float32 experts (MUTANTS), each at its worst element: standoff_dropped 6.6e3 | 3.5e5, kd_dropped 6.8e4 | 6.2e6,
    yaw_rate_zero 1.5e5 | 2.0, first_step_ignored 4.1e5 | inf, nominal_mass 4.7e5 | 2.0, sin_cos_swapped 5.7e5 | 9.5e5,
    rates_not_zeroed 1.0e6 | inf, sin_sign 2.0e6 | 7.7e5 (inf: an error on a word whose scale is zero); on the least
    favourable (regime, gains) input that can show it at all, the least visible one (nominal_mass) is at 1.2e4      CPU

The worst correct ratios are those of des_vel x and z (state_des[3], [5]) in the hard regime: four roundings (the stand-off,
the difference, kp, the kd term) of partial results that E_vd counts once.  KAPPA_EXPERT = 5 is 2.5 times the worst correct
ratio (1.979), CPU or MI355X, and more than three orders of magnitude below the least visible mutant (6.6e3 on the actions
alone, 1.2e4 on its least favourable input).  The kernel uses q_rcp, q_sincos, its own asin / atan2 and contracted
multiply-adds where the oracle uses libm: its ratios stay below the float32 oracle's.  sin_sign, the sin psi term of phi_des
with the wrong sign, is inside the bound in the nominal regime (ratio 1.18: the desired yaw is zero there, as in fixture g11)
and 2.9e5 outside it in the others; swapping sin psi and cos psi in phi_des is visible at zero yaw too (a_x / g for -a_y / g).
The MI355X figures are from one run of tests/test_gpu_expert_matrix.py (2026-10-18); profiles/expert/README.md has the table.
"""
import numpy as np

U32 = 2.0 ** -24

KAPPA_EXPERT = 5.0

G = 9.81                       # quadrotor.py:15
ARM = 0.086                    # :20
LAMBDA = 1.5e-9 / 6.11e-8      # k_M / k_F, :43-44
MASS_NOM = 0.18
STANDOFF = 0.2                 # the expert flies to 0.2 m behind the target (run_expert_policy.py:57)
QUAT = 4.0

GAINS = ((0.35, 0.0), (0.35, 0.2), (1.0, 0.5))
# regime: (tilt [rad], yaw [rad], relative position [m], velocities and rates, state_des[12])
REGIMES = {"nominal": (0.05, 0.0, 0.5, 0.1, 0.0), "mid": (0.5, 1.0, 3.0, 2.0, 0.5), "hard": (1.0, 3.0, 10.0, 5.0, 0.5)}
CPU_N = 1000
CPU_CASES = [(regime, g) for regime in REGIMES for g in range(len(GAINS))]

MUTANTS = ("kd_dropped", "nominal_mass", "standoff_dropped", "first_step_ignored", "sin_cos_swapped", "sin_sign",
           "rates_not_zeroed", "yaw_rate_zero")


# ---------------------------------------------------------------------------------------------------- inputs
def _quat_yaw_tilt(yaw, tilt, axis):
    """q_yaw (x) q_tilt: a rotation by `tilt` about the horizontal axis (cos axis, sin axis, 0), then `yaw` about z"""
    cy, sy, ct, st = np.cos(0.5 * yaw), np.sin(0.5 * yaw), np.cos(0.5 * tilt), np.sin(0.5 * tilt)
    tx, ty = st * np.cos(axis), st * np.sin(axis)
    return np.stack([cy * ct, cy * tx - sy * ty, cy * ty + sy * tx, sy * ct], axis=1)


def inputs(regime, n, gains=0, seed=0):
    """n envs of one regime -> dict of float32 arrays chaser [n,13], target [n,13], state_des [n,13], mass [n], bool first [n]
    (one env in seven) and the floats kp, kd.  The chaser's attitude is a tilt of at most the regime's angle about a
    horizontal axis, then a yaw; state_des holds arbitrary position words (never read), an earlier des_vel, a desired attitude
    of the regime's yaw and a fifth of its tilt (only its yaw is read), arbitrary rates in [10:12] (overwritten with zeros) and
    the regime's desired yaw rate."""
    tilt, yaw, rel, vel, wz = REGIMES[regime]
    rs = np.random.RandomState(7919 * list(REGIMES).index(regime) + 104729 * gains + 15485863 * seed + n)
    u = lambda lim, *shape: rs.uniform(-1.0, 1.0, shape) * lim       # noqa: E731
    target = np.zeros((n, 13))
    target[:, 0:3] = np.array([10.0, -50.0, 5.0]) + u(0.5, n, 3)
    target[:, 3:6] = u(0.1, n, 3)
    target[:, 6] = 1.0
    chaser = np.zeros((n, 13))
    chaser[:, 0:3] = target[:, 0:3] - np.array([STANDOFF, 0.0, 0.0]) - u(rel, n, 3)
    chaser[:, 3:6] = u(vel, n, 3)
    chaser[:, 6:10] = _quat_yaw_tilt(u(yaw, n), rs.uniform(0.0, tilt, n), rs.uniform(0.0, 2.0 * np.pi, n))
    chaser[:, 10:13] = u(vel, n, 3)
    sd = np.zeros((n, 13))
    sd[:, 0:3] = u(50.0, n, 3)
    sd[:, 3:6] = u(vel, n, 3)
    sd[:, 6:10] = _quat_yaw_tilt(u(yaw, n), rs.uniform(0.0, 0.2 * tilt, n), rs.uniform(0.0, 2.0 * np.pi, n))
    sd[:, 10:12] = u(vel, n, 2)
    sd[:, 12] = u(wz, n)
    mass = MASS_NOM * rs.uniform(0.8, 1.2, n)
    first = (np.arange(n) + 3 * gains + seed) % 7 == 3
    kp, kd = GAINS[gains]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)              # noqa: E731
    return dict(regime=regime, chaser=f32(chaser), target=f32(target), state_des=f32(sd), mass=f32(mass), first=first,
                kp=float(np.float32(kp)), kd=float(np.float32(kd)))


# ---------------------------------------------------------------------------------------------------- the expert
def _quat2euler(q):
    """utils/transform.py:94-120 on [n,4] -> phi, theta, psi, r12 (any float dtype; the branches as np.where)"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    two, one = q.dtype.type(2.0), q.dtype.type(1.0)
    r10 = two * (x * y - w * z)
    r11 = w * w - x * x + y * y - z * z
    r12 = two * (w * x + y * z)
    r02 = two * (x * z - w * y)
    r22 = w * w - x * x - y * y + z * z
    sat = (r12 >= one) | (r12 < -one)
    half_pi = q.dtype.type(np.pi / 2.0)
    phi = np.where(r12 >= one, half_pi, np.where(r12 < -one, -half_pi, np.arcsin(np.clip(r12, -one, one))))
    theta = np.where(sat, q.dtype.type(0.0), np.arctan2(-r02, r22))
    return phi, theta, np.arctan2(-r10, r11), r12


def _euler2quat(phi, theta, psi):
    """utils/transform.py:123-136 -> [n,4]"""
    h = phi.dtype.type(0.5)
    cy, sy, cp, sp, cr, sr = np.cos(psi * h), np.sin(psi * h), np.cos(theta * h), np.sin(theta * h), np.cos(phi * h), np.sin(phi * h)
    return np.stack([cr * cp * cy - sr * sp * sy, sr * cp * cy - cr * sp * sy, sr * cp * sy + cr * sp * cy,
                     cr * cp * sy + sr * sp * cy], axis=1)


def _expert(dtype, sd, sc, st, first, kp, kd, mass, mutant=None):
    """qso_expert_action in `dtype` arithmetic -> dict of every intermediate the error scale needs.  `mutant`: one of MUTANTS,
    a deliberately wrong expert for tests/test_expert_matrix_cpu.py."""
    assert mutant is None or mutant in MUTANTS, mutant
    r = dtype
    sd, sc, st = np.array(sd, r), np.asarray(sc, r), np.asarray(st, r)
    n = len(sd)
    first = np.broadcast_to(np.asarray(first, bool), (n,))
    mass = np.broadcast_to(np.asarray(mass, r), (n,))
    kp, kd = np.asarray(kp, r), np.asarray(kd, r)
    if mutant == "kd_dropped":
        kd = np.asarray(0.0, r)
    if mutant == "nominal_mass":
        mass = np.full(n, MASS_NOM, r)
    if mutant == "first_step_ignored":
        first = np.zeros(n, bool)
    off = np.array([0.0 if mutant == "standoff_dropped" else -STANDOFF, 0.0, 0.0], r)
    g = r(G)
    # des_vel, run_expert_policy.py:57-59
    vd = np.where(first[:, None], sd[:, 3:6], kp * (st[:, 0:3] + off - sc[:, 0:3]) + kd * (-sc[:, 3:6]))
    # vel_controller, PIDController.py:112-114 (state_last = state: the derivative terms are zero)
    e = vd - sc[:, 3:6]
    ax, ay, az = r(-0.7) * e[:, 0], r(-0.7) * e[:, 1], r(1.0) * e[:, 2]
    F = mass * g + mass * az                                              # :116
    psi = _quat2euler(sd[:, 6:10])[2]                                     # :119
    s, c = np.sin(psi), np.cos(psi)
    if mutant == "sin_cos_swapped":
        phi_des = (ax * c - ay * s) / g
    elif mutant == "sin_sign":
        phi_des = (-ax * s - ay * c) / g
    else:
        phi_des = (ax * s - ay * c) / g                                   # :122
    theta_des = (ax * c + ay * s) / g                                     # :123
    q_new = _euler2quat(phi_des, theta_des, psi)                          # :132
    w_des = np.zeros((n, 3), r)                                           # :133-134
    if mutant == "rates_not_zeroed":
        w_des[:, 0:2] = sd[:, 10:12]
    w_des[:, 2] = r(0.0) if mutant == "yaw_rate_zero" else sd[:, 12]
    # attitude_controller, :61-71
    d = _quat2euler(q_new)
    now = _quat2euler(sc[:, 6:10])
    w = w_des - sc[:, 10:13]
    M = np.stack([r(-10.0) * (d[0] - now[0]) + r(5.1) * w[:, 0], r(-10.0) * (d[1] - now[1]) + r(5.1) * w[:, 1],
                  r(-9.5) * (d[2] - now[2]) + r(4.0) * w[:, 2]], axis=1)
    # inverse of rotor2control (quadrotor.py:56-59), action normalisation (run_expert_policy.py:63)
    a, b = r(1.0) / (r(2.0) * r(ARM)), r(1.0) / (r(4.0) * r(LAMBDA))
    f4 = F / r(4.0)
    f = np.stack([f4 - a * M[:, 1] + b * M[:, 2], f4 + a * M[:, 0] - b * M[:, 2], f4 + a * M[:, 1] + b * M[:, 2],
                  f4 - a * M[:, 0] - b * M[:, 2]], axis=1)
    mean = mass * g / r(2.0)
    act = (f - mean[:, None]) / mean[:, None]
    sd_new = sd.copy()
    sd_new[:, 3:6] = vd
    sd_new[:, 6:10] = q_new
    sd_new[:, 10:12] = w_des[:, 0:2]
    return dict(act=act, sd=sd_new, vd=vd, acc=(ax, ay, az), F=F, psi=psi, s=s, c=c, phi_des=phi_des, theta_des=theta_des,
                q_new=q_new, d=d, now=now, w_des=w_des, M=M, f=f, mean=mean, mass=mass, first=first, kp=kp, kd=kd)


def expert32(sd, sc, st, first, kp, kd, mass, mutant=None):
    """the expert in numpy float32 arithmetic (libm trigonometry, no contraction) -> (actions [n,4], new state_des [n,13])"""
    x = _expert(np.float32, sd, sc, st, first, kp, kd, mass, mutant)
    assert x["act"].dtype == np.float32 and x["sd"].dtype == np.float32
    return x["act"], x["sd"]


def _cond(r12):
    return 1.0 / np.sqrt(np.maximum(1.0 - r12 * r12, 1e-300))


def _angle_term(q):
    return 3.0 * _cond(_quat2euler(q)[3]) + 2.0


def expert64(sd, sc, st, first, kp, kd, mass):
    """-> (actions [n,4], new state_des [n,13], E [n,4], E_sd [n,9] for state_des[3:12]) in float64; the module docstring has
    the scale.  sd, sc [n,13], st [n,>=3], first [n] bool, mass [n] or a scalar.  kp and kd are taken as they are: to judge a
    kernel, pass them rounded to float32 (what the C ABI receives), as inputs() returns them."""
    kp, kd = float(kp), float(kd)
    x = _expert(np.float64, sd, sc, st, first, kp, kd, mass)
    sd, sc, st = np.asarray(sd, np.float64), np.asarray(sc, np.float64), np.asarray(st, np.float64)
    n = len(sd)
    first, m = x["first"], x["mass"]
    ax, ay, az = x["acc"]
    s, c = np.abs(x["s"]), np.abs(x["c"])
    # des_vel
    off = np.array([STANDOFF, 0.0, 0.0])
    E_vd = np.where(first[:, None], 0.0, kp * (np.abs(st[:, 0:3]) + off + np.abs(sc[:, 0:3])) + kd * np.abs(sc[:, 3:6]))
    E_acc = np.array([0.7, 0.7, 1.0]) * (E_vd + np.abs(x["vd"]) + np.abs(sc[:, 3:6]))
    E_F = m * (G + np.abs(az) + E_acc[:, 2])
    # desired angles
    E_psi = _angle_term(sd[:, 6:10])
    E_phi = (E_acc[:, 0] * s + E_acc[:, 1] * c + np.abs(ax) * s + np.abs(ay) * c + (np.abs(ax) * c + np.abs(ay) * s) * E_psi) / G \
        + np.abs(x["phi_des"])
    E_theta = (E_acc[:, 0] * c + E_acc[:, 1] * s + np.abs(ax) * c + np.abs(ay) * s + (np.abs(ax) * s + np.abs(ay) * c) * E_psi) / G \
        + np.abs(x["theta_des"])
    E_in = np.stack([E_phi, E_theta, E_psi], axis=1)
    # ... read back from the rewritten quaternion: |J| E_in + the extraction itself
    ang = np.stack([x["phi_des"], x["theta_des"], x["psi"]], axis=1)
    h = 1e-6
    E_d = np.zeros((n, 3))
    for j in range(3):
        lo, hi = ang.copy(), ang.copy()
        lo[:, j] -= h
        hi[:, j] += h
        dlo, dhi = _quat2euler(_euler2quat(*lo.T)), _quat2euler(_euler2quat(*hi.T))
        for i in range(3):
            diff = dhi[i] - dlo[i]
            diff = (diff + np.pi) % (2.0 * np.pi) - np.pi                 # a yaw next to +-pi
            E_d[:, i] += np.abs(diff / (2.0 * h)) * E_in[:, j]
    E_d += _angle_term(x["q_new"])[:, None]
    E_n = _angle_term(sc[:, 6:10])[:, None]
    d, now = np.stack(x["d"][:3], axis=1), np.stack(x["now"][:3], axis=1)
    # moments, rotor forces, action
    gain_a, gain_w = np.array([10.0, 10.0, 9.5]), np.array([5.1, 5.1, 4.0])
    E_M = gain_a * (E_d + E_n + np.abs(d) + np.abs(now)) + gain_w * (np.abs(x["w_des"]) + np.abs(sc[:, 10:13]))
    T = E_M + np.abs(x["M"])
    a, b = 1.0 / (2.0 * ARM), 1.0 / (4.0 * LAMBDA)
    E_f4 = (E_F + np.abs(x["F"])) / 4.0
    E_f = np.stack([E_f4 + a * T[:, 1] + b * T[:, 2], E_f4 + a * T[:, 0] + b * T[:, 2], E_f4 + a * T[:, 1] + b * T[:, 2],
                    E_f4 + a * T[:, 0] + b * T[:, 2]], axis=1)
    mean = x["mean"][:, None]
    E = (E_f + np.abs(x["f"])) / mean + 1.0 + np.abs(x["act"])
    E_sd = np.zeros((n, 9))
    E_sd[:, 0:3] = E_vd
    E_sd[:, 3:7] = (0.5 * E_in.sum(axis=1) + QUAT)[:, None]
    return x["act"], x["sd"], E, E_sd


def reference(inp):
    """expert64 on a dict of inputs() -> (actions, new state_des, E, E_sd)"""
    return expert64(inp["state_des"], inp["chaser"], inp["target"], inp["first"], inp["kp"], inp["kd"], inp["mass"])


# ---------------------------------------------------------------------------------------------------- the bound
def ratios(act, sd_new, ref):
    """worst err / (2^-24 * scale) of float32 actions [n,4] and a new state_des [n,13] (either may be None) against ref =
    expert64(...) -> (ratio of the actions, ratio of state_des[3:12]); an error on a scale of zero is infinite"""
    a64, sd64, E, E_sd = ref
    out = []
    for got, want, scale in ((act, a64, E), (None if sd_new is None else np.asarray(sd_new)[:, 3:12], sd64[:, 3:12], E_sd)):
        if got is None:
            out.append(0.0)
            continue
        err = np.abs(np.asarray(got, np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / (U32 * scale))
        out.append(float(np.max(np.where(np.isnan(q), np.inf, q))) if q.size else 0.0)
    return tuple(out)


def check(act, sd_new, ref, what=""):
    """EVERY element of the float32 actions and of the new state_des[3:12] within KAPPA_EXPERT * 2^-24 * scale of ref =
    expert64(...) -> the two worst ratios.  Nothing is excluded; a NaN is out of bound; where the scale is zero (state_des[3:6]
    on a first step, [10:12]) the value must be exact."""
    a64, sd64, E, E_sd = ref
    for name, got, want, scale in (("actions", act, a64, E), ("state_des[3:12]", np.asarray(sd_new)[:, 3:12], sd64[:, 3:12], E_sd)):
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == want.shape, "%s %s: %s %s" % (what, name, got.dtype, got.shape)
        err = np.abs(got.astype(np.float64) - want)
        bad = ~(err <= KAPPA_EXPERT * U32 * scale)
        if bad.any():
            i = np.argwhere(bad)[0]
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = float(np.nanmax(np.where(err == 0.0, 0.0, err / (U32 * scale))))
            raise AssertionError("%s %s: %d of %d elements out of bound, worst ratio %.3g (kappa %.3g), first at %s: got %r, want %r"
                                 % (what, name, int(bad.sum()), bad.size, worst, KAPPA_EXPERT, i.tolist(), got[tuple(i)], want[tuple(i)]))
    return ratios(act, sd_new, ref)
