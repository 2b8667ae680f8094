"""Float64 restatement of GAIL's discriminator on the device (quadsim_amd.gail, include/quadsim_gail.h) and the derived error
bounds of its float32 logit, statistics, gradient, Adam update and reward.  A helper module, not a test; numpy only.  Modelled on
tests/bcfit_ref.py; Adam (adam64, adam_bound, lr_t64: the same formula, as the header says) is tests/dynfit_ref.py's as it is.

What is restated: the input row (normalised observation, clamped action), D = 16 -> H -> H -> 1 with tanh, weights in the policy's
(in, out) layout (forward64); SB2's TransitionClassifier loss, its five statistics and its six gradients (backward64);
tf.train.AdamOptimizer over a schedule with a count per step (fit64); the reward, evaluated literally as
-log(1 - sigmoid(l) + 1e-8) (reward64); SB2's RunningMeanStd (running_stats).

The bounds.  u = 2^-24, gamma_k = k u / (1 - k u); E_x bounds |computed x - x|.  The device's tanh, 1 - tanh^2, exp, log and log1p
enter as the constants below: FOUR TIMES the largest error measured against float64 on the device over the swept ranges
(tests/test_gpu_gail.py::test_device_math_sweep asserts them, profiles/gail/README.md records the measurement).
  input        x = fl(fl(o - mean) rscale): gamma_2 |x|; the clamped action is exact
  forward      E_z = E_h |W| + gamma_{K+2} ((|h| + E_h) |W| + |b|), K = 16, H4, H4 (H rounded up to 4; the padding adds exact zeros)
  tanh         a = tanh z is 1-Lipschitz with |a''| <= 0.77: E_a = d E_z + E_z^2 + TANH_ABS; d = 1 - a^2 has |d'| = 2 |a| d, |d''| <= 2:
               E_d = 2 |a| d E_z + 2 E_z^2 + SECH2_REL d
  row terms    every term is a smooth function of the logit, the same formula on both sides of l = 0, so its error is (Lipschitz
               constant) E_l plus the arithmetic error at an exact l: sigmoid 1/4, softplus 1, h'(l) = -s n l,
               (s n l)' <= (1 + |l|) / 4.  Arithmetic: e = exp(-|l|) carries EXP_REL e, p = log1p(e) LOG1P_REL p, every further
               operation u of its result (written out in row_terms)
  statistics   c (or 2 c) additions and one division: the sum of the rows' bounds over c plus gamma_{c+1} of the sum; an accuracy
               is exact unless a logit lies within E_l of zero: each such row may add 1 / c
  back-prop    dz1 = fl(d1 fl(w2 dl)): two roundings on two computed factors; dz0 = fl(d0 acc), acc an fma chain of H terms
  gradients    an fma chain over the 2 c rows of the step on two computed factors (the padding rows add exact zeros):
               E_gW = E_a^T |dz| + |a|^T E_dz + E_a^T E_dz + gamma_{2c+2} (|a| + E_a)^T (|dz| + E_dz);  gb: a = 1, E_a = 0
  reward       the MFMA forward adds the four products of a group in an order of its own: any order of K + 1 terms is within
               gamma_{K+2}, the same E_l.  q = 1 / (1 + exp l), r = -log(q + 1e-8): r'(l) = s q / (q + 1e-8) <= 1, so
               E_r = E_l + the arithmetic error at an exact l (written out in reward_bound)
plus TINY per result for the subnormal range.  Nothing is fitted.
"""
import numpy as np

import dynfit_ref as fr
import dynplan_ref as dr

U32, TINY, gamma = dr.U32, dr.TINY, dr.gamma
adam64, adam_bound, lr_t64 = fr.adam64, fr.adam_bound, fr.lr_t64
BETA1, BETA2, EPS = 0.9, 0.999, 1.0e-8
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
STAT_NAMES = ("gen_loss", "exp_loss", "entropy", "gen_acc", "exp_acc")
ENTCOEFF = 1.0e-3

# ---- the device's math functions: 4 x the measured maximum over the swept range (MEASURED below), see the module docstring
MEASURED = {"tanh_abs": 1.31e-7, "sech2_rel": 1.794e-6, "exp_rel": 8.121e-8, "log_rel": 1.554e-7, "log1p_rel": 6.193e-8}
TANH_ABS, SECH2_REL, EXP_REL, LOG_REL, LOG1P_REL = (4.0 * MEASURED[k] for k in ("tanh_abs", "sech2_rel", "exp_rel", "log_rel", "log1p_rel"))
# the swept ranges: what the tests' nets can reach, with room (pre-activations |z| <= 12, logits |l| <= 40)
SWEEPS = {"tanh_abs": (0, -12.0, 12.0), "sech2_rel": (1, -12.0, 12.0), "exp_rel": (2, -40.0, 40.0), "log_rel": (3, 1.0e-8, 2.0),
          "log1p_rel": (4, 0.0, 1.0)}
MATH64 = {0: np.tanh, 1: lambda x: 1.0 / np.cosh(x) ** 2, 2: np.exp, 3: np.log, 4: np.log1p}


def sweep_points(name, n=1 << 18, seed=5):
    """float32 inputs of a sweep: a uniform grid over the range, random points, and for the ranges that touch zero a
    logarithmic ladder towards it (relative error is decided there)"""
    _, lo, hi = SWEEPS[name]
    rng = np.random.default_rng(seed)
    parts = [np.linspace(lo, hi, n), rng.uniform(lo, hi, n)]
    ladder = 10.0 ** rng.uniform(-30.0, 0.0, n // 4)
    if lo <= 0.0 <= hi:
        parts += [ladder * min(hi, 1.0)] + ([-ladder * min(-lo, 1.0)] if lo < 0.0 else [])
    if name == "log_rel":
        parts += [1.0 + rng.uniform(-1.0, 1.0, n // 4) * 10.0 ** rng.uniform(-7.0, 0.0, n // 4)]      # around log's zero
    x = np.concatenate(parts).astype(np.float32)
    return x[(x >= np.float32(lo)) & (x <= np.float32(hi))]


def sweep_error(name, x, y):
    """the largest error of the device's y = f(x) against float64 on the same float32 x: absolute for tanh, else relative"""
    want = MATH64[SWEEPS[name][0]](x.astype(np.float64))
    err = np.abs(y.astype(np.float64) - want)
    if name.endswith("_rel"):
        err = np.where(want == 0.0, np.where(err == 0.0, 0.0, np.inf), err / np.where(want == 0.0, 1.0, np.abs(want)))
    return float(err.max())


# ---------------------------------------------------------------------------------------------------- the functions
def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def hidden_of(W):
    return int(np.asarray(W["b0"]).shape[0])


def inputs64(obs, act, mean, rscale):
    """-> (x [B,16] float64, E_x)"""
    f = np.float64
    xo = (np.asarray(obs, f) - np.asarray(mean, f)) * np.asarray(rscale, f)
    x = np.concatenate([xo, np.clip(np.asarray(act, f), -1.0, 1.0)], 1)
    E = np.concatenate([gamma(2) * np.abs(xo) + TINY, np.zeros((x.shape[0], 4))], 1)
    return x, E


def forward64(W, obs, act, mean, rscale):
    """rows -> dict(x, z0, a0, d0, z1, a1, d1, l) in float64 and E_* of each"""
    f = np.float64
    x, E = inputs64(obs, act, mean, rscale)
    H = hidden_of(W)
    chain = (16, (H + 3) & ~3, (H + 3) & ~3)
    F = {"x": x, "E_x": E}
    h = x
    for l in range(3):
        w, b = np.asarray(W["w%d" % l], f), np.asarray(W["b%d" % l], f)
        aw = np.abs(w)
        E = E @ aw + gamma(chain[l] + 2) * ((np.abs(h) + E) @ aw + np.abs(b)) + TINY
        z = h @ w + b
        if l < 2:
            a = np.tanh(z)
            d = 1.0 / np.cosh(z) ** 2
            F["z%d" % l], F["E_z%d" % l], F["a%d" % l], F["d%d" % l] = z, E, a, d
            F["E_d%d" % l] = 2.0 * np.abs(a) * d * E + 2.0 * E * E + SECH2_REL * d + TINY
            E = d * E + E * E + TANH_ABS
            F["E_a%d" % l] = E
            h = a
        else:
            F["l"], F["E_l"] = z[:, 0], E[:, 0]
    return F


def row_terms(l, E_l, gen, c, entcoeff):
    """per row: softplus of the row's class, the entropy term h, dl and their bounds.  gen: bool [B] (generator rows)"""
    u = U32
    e = np.exp(-np.abs(l))
    p = np.log1p(e)
    D = 1.0 + e
    s, n = sigmoid(l), sigmoid(-l)
    A_e = EXP_REL * e                                                        # e at an exact l
    A_p = A_e / D + LOG1P_REL * (p + A_e) + TINY
    A_s = A_e / (D * D) * 1.001 + 3.0 * u * s + TINY                         # D = fl(1 + e), then one division: either branch
    A_n = A_e / (D * D) * 1.001 + 3.0 * u * n + TINY
    sp_g, sp_e = softplus(l), softplus(-l)
    A_spg, A_spe = A_p + u * (sp_g + A_p) + TINY, A_p + u * (sp_e + A_p) + TINY
    sp = np.where(gen, sp_g, sp_e)
    E_sp = E_l + np.where(gen, A_spg, A_spe)
    h = n * l + sp_e
    al = np.abs(l)
    E_h = 0.25 * (al + E_l) * E_l + A_n * al + A_spe + u * (np.abs(h) + A_n * al + A_spe) + TINY
    inv, K = 1.0 / c, entcoeff / (2.0 * c)
    base = np.where(gen, s * inv, -n * inv)
    A_base = np.where(gen, A_s, A_n) * inv + 2.0 * u * (np.abs(base) + np.where(gen, A_s, A_n) * inv)      # I rounded, the product
    t1 = s * n * l
    A_t1 = (A_s * n + A_n * s + A_s * A_n) * al + gamma(2) * (np.abs(t1) + (A_s * n + A_n * s + A_s * A_n) * al)
    dl = K * t1 + base
    A_dl = abs(K) * A_t1 + u * abs(K) * (np.abs(t1) + A_t1) + A_base
    A_dl = A_dl + u * (np.abs(dl) + A_dl) + TINY                             # K rounded, the fma
    E_dl = (0.25 * inv + abs(K) * 0.25 * (1.0 + al + E_l)) * E_l + A_dl
    return {"sp": sp, "E_sp": E_sp, "h": h, "E_h": E_h, "dl": dl, "E_dl": E_dl}


def backward64(W, gen, exp, mean, rscale, entcoeff=ENTCOEFF, with_bound=False):
    """gen, exp: (obs [c,12], act [c,4]) float32 rows of the two classes -> (stats [5], {key: gradient}) in float64;
    with_bound: (stats, grads, stats bound [5], {key: bound})"""
    f = np.float64
    c = gen[0].shape[0]
    assert exp[0].shape[0] == c
    obs, act = np.concatenate([gen[0], exp[0]]), np.concatenate([gen[1], exp[1]])
    F = forward64(W, obs, act, mean, rscale)
    isg = np.arange(2 * c) < c
    l, E_l = F["l"], F["E_l"]
    T = row_terms(l, E_l, isg, c, entcoeff)
    stats = np.array([T["sp"][:c].mean(), T["sp"][c:].mean(), T["h"].mean(), (l[:c] < 0).mean(), (l[c:] > 0).mean()])
    w1, w2 = np.asarray(W["w1"], f), np.asarray(W["w2"], f)[:, 0]
    dl, E_dl = T["dl"][:, None], T["E_dl"][:, None]
    aw2 = np.abs(w2)[None, :]
    dz1 = F["d1"] * (w2[None, :] * dl)
    E_dz1 = aw2 * (F["E_d1"] * (np.abs(dl) + E_dl) + F["d1"] * E_dl) + gamma(2) * (F["d1"] + F["E_d1"]) * aw2 * (np.abs(dl) + E_dl) + TINY
    H = hidden_of(W)
    acc = dz1 @ w1.T
    E_acc = E_dz1 @ np.abs(w1).T + gamma(H + 1) * ((np.abs(dz1) + E_dz1) @ np.abs(w1).T) + TINY
    dz0 = F["d0"] * acc
    E_dz0 = F["E_d0"] * (np.abs(acc) + E_acc) + F["d0"] * E_acc + U32 * (F["d0"] + F["E_d0"]) * (np.abs(acc) + E_acc) + TINY
    G, E = {}, {}
    B = 2 * c
    for k, dz, E_dz, a, E_a in ((0, dz0, E_dz0, F["x"], F["E_x"]), (1, dz1, E_dz1, F["a0"], F["E_a0"]), (2, dl, E_dl, F["a1"], F["E_a1"])):
        G["w%d" % k], G["b%d" % k] = a.T @ dz, dz.sum(0)
        adz, aa = np.abs(dz), np.abs(a)
        E["w%d" % k] = E_a.T @ adz + aa.T @ E_dz + E_a.T @ E_dz + gamma(B + 2) * ((aa + E_a).T @ (adz + E_dz)) + TINY
        E["b%d" % k] = E_dz.sum(0) + gamma(B + 2) * (adz + E_dz).sum(0) + TINY
    if not with_bound:
        return stats, G
    def mean_bound(v, E_v):
        k = v.shape[0]
        return E_v.sum() / k + gamma(k + 1) * (np.abs(v) + E_v).sum() / k + TINY
    edge = np.abs(l) <= E_l
    Es = np.array([mean_bound(T["sp"][:c], T["E_sp"][:c]), mean_bound(T["sp"][c:], T["E_sp"][c:]), mean_bound(T["h"], T["E_h"]),
                   edge[:c].sum() / c + U32, edge[c:].sum() / c + U32])
    return stats, G, Es, E


def fit64(W, M, V, gen, exp, gen_idx, exp_idx, mean, rscale, counts=None, t0=0, lr=3.0e-4, entcoeff=ENTCOEFF, beta1=BETA1, beta2=BETA2,
          eps=EPS):
    """the loop: step s takes rows gen_idx[s][:counts[s]] of gen = (obs, act) and exp_idx[s][:counts[s]] of exp -> (weights, m, v
    as dicts of float64 arrays, stats [steps,5])"""
    f = np.float64
    W = {k: np.asarray(W[k], f).copy() for k in KEYS}
    M = {k: np.asarray(M[k], f).copy() for k in KEYS}
    V = {k: np.asarray(V[k], f).copy() for k in KEYS}
    stats = []
    for s in range(len(gen_idx)):
        c = gen_idx.shape[1] if counts is None else int(counts[s])
        gr, er = gen_idx[s][:c], exp_idx[s][:c]
        st, G = backward64(W, (gen[0][gr], gen[1][gr]), (exp[0][er], exp[1][er]), mean, rscale, entcoeff)
        stats.append(st)
        for k in KEYS:
            W[k], M[k], V[k] = adam64(W[k], M[k], V[k], G[k], t0 + s + 1, lr, beta1, beta2, eps)
    return W, M, V, np.asarray(stats)


def reward64(l):
    """the reference's formula, literally, in float64"""
    l = np.asarray(l, np.float64)
    return -np.log(1.0 - 1.0 / (1.0 + np.exp(-l)) + 1.0e-8)


def reward_bound(l, E_l):
    """the bound of the device's reward against reward64 of the float64 logit: r is 1-Lipschitz in l; at an exact l, q = 1 / (1 +
    exp l) carries EXP_REL and two roundings, q + 1e-8f one rounding and the rounding of the constant, the logarithm LOG_REL of
    its result and 1 / (q + 1e-8) of its argument's error.  reward64 itself loses 1e-16 / (q + 1e-8) to the cancellation it
    spells out."""
    l = np.asarray(l, np.float64)
    with np.errstate(over="ignore"):
        q = 1.0 / (1.0 + np.exp(l))
    A_q = (EXP_REL * (1.0 - q) + 3.0 * U32) * q + TINY
    arg = q + 1.0e-8
    A_arg = A_q + U32 * 1.0e-8 + U32 * (arg + A_q)
    r = -np.log(arg)
    A_r = A_arg / (arg - A_arg) + LOG_REL * (np.abs(r) + A_arg / (arg - A_arg)) + TINY
    return E_l + A_r + 2.3e-16 / arg


def running_stats(batches):
    """SB2's RunningMeanStd over a list of [n,12] batches -> (mean, std) float64"""
    s, ss, n = np.zeros(12), np.full(12, 1.0e-2), 1.0e-2
    for b in batches:
        b = np.asarray(b, np.float64)
        s, ss, n = s + b.sum(0), ss + (b * b).sum(0), n + b.shape[0]
    mean = s / n
    return mean, np.sqrt(np.maximum(ss / n - mean * mean, 1.0e-2))


# ---------------------------------------------------------------------------------------------------- the shared fixtures
N_GEN, N_EXP = 300, 200
HIDDENS = (64, 128, 100)                     # both compiled widths full, and SB2's default on the 128 instantiation
STEP_COUNTS = (1, 15, 16, 17, 33, 256)       # rows per class: either side of the kernel's chunk of 16, the maximum
_cache = {}


def weights(hidden, seed=131, gain=1.0, bias=0.1):
    """Xavier-uniform weights scaled by `gain`, small random biases"""
    key = ("w", hidden, seed, gain, bias)
    if key not in _cache:
        rng = np.random.default_rng(seed + hidden)
        W = {}
        for k, shape in zip(KEYS, ((16, hidden), (hidden,), (hidden, hidden), (hidden,), (hidden, 1), (1,))):
            if len(shape) == 2:
                lim = gain * np.sqrt(6.0 / (shape[0] + shape[1]))
                W[k] = rng.uniform(-lim, lim, shape).astype(np.float32)
            else:
                W[k] = (bias * rng.standard_normal(shape)).astype(np.float32)
        _cache[key] = W
    return _cache[key]


def dataset(seed=151):
    """gen = (obs [300,12], act [300,4] with |u| up to 3: unclipped samples), exp = (obs [200,12], act [200,4] in [-1, 1]), and the
    statistics (mean, rscale) float32 of SB2's running statistics after one merge of all 500 observations"""
    if ("data", seed) not in _cache:
        rng = np.random.default_rng(seed)
        gen = (dr.sample_obs(N_GEN, seed=seed + 1), rng.uniform(-3.0, 3.0, (N_GEN, 4)).astype(np.float32))
        exp = (dr.sample_obs(N_EXP, seed=seed + 2), rng.uniform(-1.0, 1.0, (N_EXP, 4)).astype(np.float32))
        mean, std = running_stats([gen[0], exp[0]])
        _cache[("data", seed)] = (gen, exp, mean.astype(np.float32), (1.0 / std).astype(np.float32))
    return _cache[("data", seed)]


def step_indices(count, steps=1, seed=171):
    """explicit rows ([steps,count] generator, [steps,count] expert) that contain row 0, the last row and a repeated row
    wherever the count has room for them"""
    rng = np.random.default_rng(seed + count)
    out = []
    for n in (N_GEN, N_EXP):
        idx = rng.integers(0, n, (steps, count)).astype(np.int32)
        idx[:, 0] = 0
        if count >= 4:
            idx[:, 1] = n - 1
            idx[:, 2] = idx[:, count - 1]
        out.append(idx)
    return out


def zero_state(W):
    return {k: np.zeros_like(W[k]) for k in KEYS}


def moments(W, seed=181):
    """non-zero starting moments: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {k: (1e-3 * rng.standard_normal(W[k].shape)).astype(np.float32) for k in KEYS}
    V = {k: (1e-6 * rng.random(W[k].shape)).astype(np.float32) for k in KEYS}
    return M, V


LEARN_STEPS, LEARN_BATCH, LEARN_LR, LEARN_HIDDEN = 150, 64, 3.0e-3, 100


def separable_case(n=512, seed=191):
    """"it learns": generator actions near +0.5, expert actions near -0.5 (sd 0.1), the same observation distribution ->
    (gen, exp, mean, rscale, gen_idx [150,64], exp_idx [150,64])"""
    if ("sep", n, seed) not in _cache:
        rng = np.random.default_rng(seed)
        gen = (dr.sample_obs(n, seed=seed + 1), (0.5 + 0.1 * rng.standard_normal((n, 4))).astype(np.float32))
        exp = (dr.sample_obs(n, seed=seed + 2), (-0.5 + 0.1 * rng.standard_normal((n, 4))).astype(np.float32))
        mean, std = running_stats([gen[0], exp[0]])
        gi = np.stack([rng.permutation(n)[:LEARN_BATCH] for _ in range(LEARN_STEPS)]).astype(np.int32)
        ei = np.stack([rng.permutation(n)[:LEARN_BATCH] for _ in range(LEARN_STEPS)]).astype(np.int32)
        _cache[("sep", n, seed)] = (gen, exp, mean.astype(np.float32), (1.0 / std).astype(np.float32), gi, ei)
    return _cache[("sep", n, seed)]
