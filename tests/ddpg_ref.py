"""Float64 restatement of the DDPG update on the device (quadsim_amd.ddpg, include/quadsim_ddpg.h) and the derived error bounds of
its float32 statistics and gradients.  A helper module, not a test; numpy only.  Modelled on tests/gail_ref.py; Adam (adam64,
adam_bound, lr_t64: the same formula, as the header says) is tests/dynfit_ref.py's as it is.

What is restated: the clamped observation; the actor 12 -> 128 -> 128 -> 4 with tanh and the critic 12 -> 128, [128 + 4] -> 128 -> 1
(actor64, critic64); the target value, the critic's loss and six gradients, the actor's loss and six gradients through the
critic's layers 1 and 2 (step64); Adam and the Polyak average over a schedule with a count per step (fit64); the header's target
formula in float32 (polyak32).

The bounds.  u = 2^-24, gamma_k = k u / (1 - k u); E_x bounds |computed x - x|.  The device's tanh enters as gail_ref.TANH_ABS, four
times the error gail_ref.MEASURED records for q_tanh over |z| <= 12 (tests/test_gpu_gail.py::test_device_math_sweep asserts it).
  input      min(max(obs, -c), c) is exact; actions, rewards and flags are used as stored
  forward    E_z = E_h |W| + gamma_{K+2} ((|h| + E_h) |W| + |b|), K = 16, 128 or 132 terms; relu is 1-Lipschitz: E_h = E_z
  tanh       a = tanh z is 1-Lipschitz with |a''| <= 0.77: E_a = (1 - a^2) E_z + E_z^2 + TANH_ABS; the derivative is taken as
             fma(-a, a, 1) from the COMPUTED a: |(1 - a_c^2) - (1 - a^2)| <= 2 |a| E_a + E_a^2, plus u of the result
  y          G = float32(gamma), (1 - done) G, the fma: E_y = k (E_q1 + gamma_3 (|q1| + E_q1)) + u |y|, k = (1 - done) gamma; a
             terminal row is exact
  d, dq      d = q - y: E_q + E_y and one rounding; dq = d float32(2 / rows): two roundings
  statistics a sum of `rows` terms and one division: the sum of the rows' bounds over rows plus gamma_{rows+2} of the sum of the
             magnitudes; the squared error adds 2 |d| E_d + E_d^2 per row and gamma_{rows+3}
  masks      the bounds assume the device takes the same side of every ReLU.  Where a float64 pre-activation lies within its
             forward bound of zero it may not: there the bound of dz is |dz without the mask| + its bound, which covers both
             sides.  No element is excluded.
  back-prop  dz1 = fl(w2 dq): one rounding on a computed factor; dz0: four interleaved fma chains of 32 terms and two additions,
             gamma_36; the actor's dz1 a chain of 4; da a chain of 128 on the critic's action rows
  gradients  an fma chain over the rows of the step on two computed factors (the padding rows add exact zeros):
             E_gW = E_h^T |dz| + |h|^T E_dz + E_h^T E_dz + gamma_{rows+2} (|h| + E_h)^T (|dz| + E_dz);  gb: h = 1, E_h = 0
plus TINY per result for the subnormal range.  Nothing is fitted.
"""
import numpy as np

import dynfit_ref as fr
import dynplan_ref as dr
import gail_ref as gr

U32, TINY, gamma = dr.U32, dr.TINY, dr.gamma
adam64, adam_bound, lr_t64 = fr.adam64, fr.adam_bound, fr.lr_t64
TANH_ABS = gr.TANH_ABS
BETA1, BETA2, EPS = 0.9, 0.999, 1.0e-8
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
NETS = ("actor", "critic", "actor_target", "critic_target")
ACTOR_SHAPES = {"w0": (12, 128), "b0": (128,), "w1": (128, 128), "b1": (128,), "w2": (128, 4), "b2": (4,)}
CRITIC_SHAPES = {"w0": (12, 128), "b0": (128,), "w1": (132, 128), "b1": (128,), "w2": (128, 1), "b2": (1,)}
STAT_NAMES = ("critic_loss", "actor_loss", "q_mean", "y_mean")
GAMMA, TAU, OBS_CLIP = 0.99, 1.0e-3, 5.0
f = np.float64


def shapes_of(name):
    return ACTOR_SHAPES if name.startswith("actor") else CRITIC_SHAPES


# ---------------------------------------------------------------------------------------------------- the forward passes
def _layer(h, E, w, b, K):
    w, b = np.asarray(w, f), np.asarray(b, f)
    aw = np.abs(w)
    return h @ w + b, E @ aw + gamma(K + 2) * ((np.abs(h) + E) @ aw + np.abs(b)) + TINY


def clamp(obs, clip=OBS_CLIP):
    return np.clip(np.asarray(obs, f), -clip, clip)


def actor64(W, x):
    """x [B,12] clamped rows -> dict(z0, h0, z1, h1, z2, a) and E_* of each"""
    F = {"x": x}
    F["z0"], F["E_z0"] = _layer(x, np.zeros_like(x), W["w0"], W["b0"], 16)
    F["h0"] = np.maximum(F["z0"], 0.0)
    F["z1"], F["E_z1"] = _layer(F["h0"], F["E_z0"], W["w1"], W["b1"], 128)
    F["h1"] = np.maximum(F["z1"], 0.0)
    F["z2"], F["E_z2"] = _layer(F["h1"], F["E_z1"], W["w2"], W["b2"], 128)
    F["a"] = np.tanh(F["z2"])
    F["E_a"] = (1.0 - F["a"] ** 2) * F["E_z2"] + F["E_z2"] ** 2 + TANH_ABS
    return F


def critic64(W, x, act, E_act=None):
    """x [B,12] clamped rows, act [B,4] (with its bound, None: exact) -> dict(z0, h0, in1, z1, h1, q) and E_* of each"""
    act = np.asarray(act, f)
    F = {"x": x}
    F["z0"], F["E_z0"] = _layer(x, np.zeros_like(x), W["w0"], W["b0"], 16)
    F["h0"] = np.maximum(F["z0"], 0.0)
    F["in1"] = np.concatenate([F["h0"], act], 1)
    F["E_in1"] = np.concatenate([F["E_z0"], np.zeros_like(act) if E_act is None else E_act], 1)
    F["z1"], F["E_z1"] = _layer(F["in1"], F["E_in1"], W["w1"], W["b1"], 132)
    F["h1"] = np.maximum(F["z1"], 0.0)
    q, E_q = _layer(F["h1"], F["E_z1"], W["w2"], W["b2"], 128)
    F["q"], F["E_q"] = q[:, 0], E_q[:, 0]
    return F


def _masked(acc, E_acc, z, E_z):
    """dz = acc under the mask z > 0, and its bound; where |z| <= E_z the device may take either side"""
    m = z > 0.0
    edge = np.abs(z) <= E_z
    return acc * m, np.where(edge, np.abs(acc) + E_acc, E_acc * m)


def _grads(layers, B, G, E):
    for l, dz, E_dz, h, E_h in layers:
        adz, ah = np.abs(dz), np.abs(h)
        G["w%d" % l], G["b%d" % l] = h.T @ dz, dz.sum(0)
        E["w%d" % l] = E_h.T @ adz + ah.T @ E_dz + E_h.T @ E_dz + gamma(B + 2) * ((ah + E_h).T @ (adz + E_dz)) + TINY
        E["b%d" % l] = E_dz.sum(0) + gamma(B + 2) * (adz + E_dz).sum(0) + TINY


def _mean_bound(v, E_v):
    k = v.shape[0]
    return E_v.sum() / k + gamma(k + 2) * (np.abs(v) + E_v).sum() / k + TINY


def relu_edges(P, rows, clip=OBS_CLIP):
    """the number of pre-activations of the three differentiated passes that lie within their forward bound of zero"""
    obs0, act = rows[0], rows[1]
    x0 = clamp(obs0, clip)
    A = actor64(P["actor"], x0)
    C1 = critic64(P["critic"], x0, act)
    C2 = critic64(P["critic"], x0, A["a"], A["E_a"])
    return int(sum(np.count_nonzero(np.abs(F["z%d" % l]) <= F["E_z%d" % l]) for F in (A, C1, C2) for l in (0, 1)))


def step64(P, rows, gam=GAMMA, clip=OBS_CLIP, with_bound=False):
    """P: {net name: {key: array}}, rows = (obs0 [B,12], act [B,4], rew [B], obs1 [B,12], done [B]) float32 -> (stats [4],
    {"actor": {key: gradient}, "critic": {..}}, y [B]) in float64; with_bound: (stats, grads, y, stats bound [4], {..: {key: bound}})"""
    obs0, act, rew, obs1, done = rows
    B = obs0.shape[0]
    x0, x1 = clamp(obs0, clip), clamp(obs1, clip)
    rew, done = np.asarray(rew, f), np.asarray(done, f)
    # 1. the target value
    T = actor64(P["actor_target"], x1)
    Q1 = critic64(P["critic_target"], x1, T["a"], T["E_a"])
    k = np.where(done >= 1.0, 0.0, (1.0 - done) * gam)
    y = np.where(done >= 1.0, rew, rew + k * Q1["q"])                           # (a select: a terminal row is rew whatever q1 is, NaN included)
    E_y = np.where(k == 0.0, 0.0, k * (Q1["E_q"] + gamma(3) * (np.abs(Q1["q"]) + Q1["E_q"])) + U32 * np.abs(y) + TINY)
    # 2. the critic
    Cr = critic64(P["critic"], x0, act)
    d = Cr["q"] - y
    E_d = Cr["E_q"] + E_y
    E_d = E_d + U32 * (np.abs(d) + E_d) + TINY
    c = 2.0 / B
    dq, E_dq = (d * c)[:, None], (c * E_d + gamma(2) * c * (np.abs(d) + E_d) + TINY)[:, None]
    wc = {k_: np.asarray(P["critic"][k_], f) for k_ in KEYS}
    w2 = wc["w2"][:, 0][None, :]
    acc = w2 * dq
    dz1, E_dz1 = _masked(acc, np.abs(w2) * E_dq + U32 * np.abs(w2) * (np.abs(dq) + E_dq) + TINY, Cr["z1"], Cr["E_z1"])
    w1h = wc["w1"][:128]
    acc = dz1 @ w1h.T
    E_acc = E_dz1 @ np.abs(w1h).T + gamma(36) * ((np.abs(dz1) + E_dz1) @ np.abs(w1h).T) + TINY
    dz0, E_dz0 = _masked(acc, E_acc, Cr["z0"], Cr["E_z0"])
    G, E = {"actor": {}, "critic": {}}, {"actor": {}, "critic": {}}
    _grads(((0, dz0, E_dz0, x0, np.zeros_like(x0)), (1, dz1, E_dz1, Cr["in1"], Cr["E_in1"]), (2, dq, E_dq, Cr["h1"], Cr["E_z1"])),
           B, G["critic"], E["critic"])
    # 3. the actor, through the critic's layers 1 and 2
    A = actor64(P["actor"], x0)
    Cp = critic64(P["critic"], x0, A["a"], A["E_a"])
    n = -1.0 / B
    acc = np.broadcast_to(w2 * n, (B, 128))
    dzc, E_dzc = _masked(acc, gamma(2) * np.abs(acc) + TINY, Cp["z1"], Cp["E_z1"])
    w1a = wc["w1"][128:]                                                         # [4,128]
    da = dzc @ w1a.T
    E_da = E_dzc @ np.abs(w1a).T + gamma(129) * ((np.abs(dzc) + E_dzc) @ np.abs(w1a).T) + TINY
    dt = 1.0 - A["a"] ** 2
    E_dt = 2.0 * np.abs(A["a"]) * A["E_a"] + A["E_a"] ** 2
    E_dt = E_dt + U32 * (dt + E_dt) + TINY
    dz2 = da * dt
    E_dz2 = E_da * dt + np.abs(da) * E_dt + E_da * E_dt
    E_dz2 = E_dz2 + U32 * (np.abs(dz2) + E_dz2) + TINY
    wa = {k_: np.asarray(P["actor"][k_], f) for k_ in KEYS}
    acc = dz2 @ wa["w2"].T
    E_acc = E_dz2 @ np.abs(wa["w2"]).T + gamma(6) * ((np.abs(dz2) + E_dz2) @ np.abs(wa["w2"]).T) + TINY
    dz1a, E_dz1a = _masked(acc, E_acc, A["z1"], A["E_z1"])
    acc = dz1a @ wa["w1"].T
    E_acc = E_dz1a @ np.abs(wa["w1"]).T + gamma(36) * ((np.abs(dz1a) + E_dz1a) @ np.abs(wa["w1"]).T) + TINY
    dz0a, E_dz0a = _masked(acc, E_acc, A["z0"], A["E_z0"])
    _grads(((0, dz0a, E_dz0a, x0, np.zeros_like(x0)), (1, dz1a, E_dz1a, A["h0"], A["E_z0"]), (2, dz2, E_dz2, A["h1"], A["E_z1"])),
           B, G["actor"], E["actor"])
    stats = np.array([np.mean(d * d), -np.mean(Cp["q"]), np.mean(Cr["q"]), np.mean(y)])
    if not with_bound:
        return stats, G, y
    sq = np.sum(2.0 * np.abs(d) * E_d + E_d ** 2) / B
    Es = np.array([sq + gamma(B + 3) * (stats[0] + sq) + TINY, _mean_bound(Cp["q"], Cp["E_q"]), _mean_bound(Cr["q"], Cr["E_q"]),
                   _mean_bound(y, E_y)])
    return stats, G, y, Es, E


def polyak32(target, online, tau=TAU):
    """the header's target formula in float32: fma(T, w', U t) with T = float32(tau), U = float32(1 - tau); the product U t is
    rounded to float32, the fma is evaluated in float64 (exact for float32 operands: 48 + 1 bits) and rounded once"""
    T, U = np.float32(tau), np.float32(1.0 - tau)
    p = (U * np.asarray(target, np.float32)).astype(np.float32)
    return (np.asarray(online, np.float32).astype(f) * f(T) + p.astype(f)).astype(np.float32)


def fit64(P, M, V, replay, idx, counts=None, t0=0, gam=GAMMA, tau=TAU, actor_lr=1.0e-4, critic_lr=1.0e-3, clip=OBS_CLIP):
    """the loop: step s takes rows idx[s][:counts[s]] of the replay -> (nets, m, v as dicts of float64 arrays, stats [steps,4])"""
    P = {n: {k: np.asarray(P[n][k], f).copy() for k in KEYS} for n in NETS}
    M = {n: {k: np.asarray(M[n][k], f).copy() for k in KEYS} for n in ("actor", "critic")}
    V = {n: {k: np.asarray(V[n][k], f).copy() for k in KEYS} for n in ("actor", "critic")}
    stats = []
    for s, rows in enumerate(np.asarray(idx)):
        rows = rows if counts is None else rows[:counts[s]]
        st, G, _ = step64(P, tuple(a[rows] for a in replay), gam, clip)
        stats.append(st)
        for n, lr in (("actor", actor_lr), ("critic", critic_lr)):
            for k in KEYS:
                P[n][k], M[n][k], V[n][k] = adam64(P[n][k], M[n][k], V[n][k], G[n][k], t0 + s + 1, lr)
                P[n + "_target"][k] = (1.0 - tau) * P[n + "_target"][k] + tau * P[n][k]
    return P, M, V, np.asarray(stats)


# ---------------------------------------------------------------------------------------------------- the shared fixtures
N_ROWS = 512
STEP_COUNTS = (1, 10, 15, 16, 17, 33, 256)   # the reference's batch, either side of the kernel's chunk of 16, the maximum
_cache = {}


def _net(rng, shapes, gain, bias):
    W = {}
    for k in KEYS:
        shape = shapes[k]
        if len(shape) == 2:
            lim = gain * np.sqrt(6.0 / (shape[0] + shape[1]))
            W[k] = rng.uniform(-lim, lim, shape).astype(np.float32)
        else:
            W[k] = (bias * rng.standard_normal(shape)).astype(np.float32)
    return W


def nets(seed=211, gain=1.0, bias=0.1):
    """four different nets, Glorot-uniform scaled by `gain` with small random biases (both ReLU masks are mixed); the targets are
    nets of their own, so that a mix-up of online and target weights shows"""
    key = ("nets", seed, gain, bias)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        _cache[key] = {n: _net(rng, shapes_of(n), gain, bias) for n in NETS}
    return _cache[key]


def nets_shifted(shift):
    """nets() with `shift` added to b2 of the target critic: target values of O(shift), so that gamma shows in y and in the critic's
    loss (the standard fixtures' target values are small).  The online nets are nets()'s"""
    key = ("shifted", float(shift))
    if key not in _cache:
        P = dict(nets())
        P["critic_target"] = dict(P["critic_target"], b2=(P["critic_target"]["b2"] + np.float32(shift)).astype(np.float32))
        _cache[key] = P
    return _cache[key]


def replay(seed=221, n=N_ROWS):
    """(obs0 [n,12]: docking observations with one entry in fifty moved beyond +-5, so that the clamp acts; act [n,4] in [-1, 1];
    rew [n]; obs1 [n,12] likewise; done [n] mixed 0 / 1) float32"""
    if ("replay", seed, n) not in _cache:
        rng = np.random.default_rng(seed)
        obs0 = dr.sample_obs(n, seed=seed + 1)
        obs1 = (obs0 + 0.1 * rng.standard_normal((n, 12))).astype(np.float32)
        for o in (obs0, obs1):
            far = rng.random((n, 12)) < 0.02
            o[far] = (np.where(o[far] < 0.0, -1.0, 1.0) * rng.uniform(5.0, 9.0, int(far.sum()))).astype(np.float32)
        obs0[0, 0], obs0[n - 1, 11], obs1[0, 3] = 7.5, -9.0, 6.25
        act = rng.uniform(-1.0, 1.0, (n, 4)).astype(np.float32)
        rew = rng.standard_normal(n).astype(np.float32)
        done = (rng.random(n) < 0.3).astype(np.float32)
        done[0], done[n - 1] = 0.0, 1.0
        _cache[("replay", seed, n)] = (obs0, act, rew, obs1, done)
    return _cache[("replay", seed, n)]


def step_indices(count, steps=1, seed=231, n=N_ROWS):
    """explicit rows [steps,count] that contain row 0, the last row and a repeated row wherever the count has room for them"""
    rng = np.random.default_rng(seed + count)
    idx = rng.integers(0, n, (steps, count)).astype(np.int32)
    idx[:, 0] = 0
    if count >= 4:
        idx[:, 1] = n - 1
        idx[:, 2] = idx[:, count - 1]
    return idx


def zero_state():
    return {n: {k: np.zeros(shapes_of(n)[k], np.float32) for k in KEYS} for n in ("actor", "critic")}


def moments(seed=241):
    """non-zero starting moments: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {n: {k: (1e-3 * rng.standard_normal(shapes_of(n)[k])).astype(np.float32) for k in KEYS} for n in ("actor", "critic")}
    V = {n: {k: (1e-6 * rng.random(shapes_of(n)[k])).astype(np.float32) for k in KEYS} for n in ("actor", "critic")}
    return M, V


LEARN_STEPS, LEARN_BATCH, LEARN_CRITIC_LR, LEARN_ACTOR_LR = 200, 16, 1.0e-3, 1.0e-4


def learn_case(seed=251, n=N_ROWS):
    """"it learns": every row terminal, so y = rew and the critic regresses q on rew = a smooth function of (obs0, act) ->
    (nets, replay, idx [200,16])"""
    if ("learn", seed, n) not in _cache:
        rng = np.random.default_rng(seed)
        obs0 = dr.sample_obs(n, seed=seed + 1)
        act = rng.uniform(-1.0, 1.0, (n, 4)).astype(np.float32)
        u, v = rng.standard_normal(12) / 4.0, rng.standard_normal(4)
        rew = np.tanh(obs0.astype(f) @ u + act.astype(f) @ v).astype(np.float32)
        rp = (obs0, act, rew, dr.sample_obs(n, seed=seed + 2), np.ones(n, np.float32))
        idx = rng.integers(0, n, (LEARN_STEPS, LEARN_BATCH)).astype(np.int32)
        _cache[("learn", seed, n)] = (nets(seed + 3, gain=1.0, bias=0.0), rp, idx)
    return _cache[("learn", seed, n)]
