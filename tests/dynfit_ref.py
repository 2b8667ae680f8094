"""Float64 restatement of the device fit of the learned dynamics net (DynamicsNet.fit, include/quadsim_dyn_fit.h) and the derived
error bounds of its float32 gradient and Adam update.  A helper module, not a test; numpy only.

What is restated (MPC-based_RL.py of the reference):
  forward64 / backward64   Dynamic_Net's loss tf.reduce_mean(tf.square(predict - delta)) (:107-110) on a batch of rows, the net of
                           dynplan_ref.step64 without the de-normalisation, and its six gradients
  adam64                   tf.train.AdamOptimizer (:111): lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); m, v; w -= lr_t m / (sqrt(v) + eps)
  fit64                    train_dynamic's loop (:120-128) over given batch indices
  indices                  the keyed batch draw of the contract: mulhi32(Philox word, size), with replacement

The bounds.  u = 2^-24, gamma_k = k u / (1 - k u) (dynplan_ref.gamma); E_x is a bound of |computed x - x|.
  forward      dynplan_ref.step_bound's recurrence: E_0 = gamma_2 |xh|, E_l = E_{l-1} |W_l|^T + gamma_{K_l+2} ((|a_{l-1}| + E_{l-1}) |W_l|^T + |b_l|)
  target       th = fl(fl(d - mu) r): E_th = gamma_2 |th|
  error        e = fl(y - th): E_e = (E_y + E_th) + u (|e| + E_y + E_th)
  dy           fl(e c^), c^ = float32(c): E_dy = |c| E_e + gamma_2 |c| (|e| + E_e)
  back-prop    dz = mask * (W^T d), an fma chain of K terms on computed d: E_dz = mask * (E_d |W| + gamma_{K+2} (|d| + E_d) |W|),
               GIVEN the same mask -- which holds when every pre-activation is further from zero than its forward bound (relu_edge)
  gradients    gW = sum over the batch rows of dz a, an fma chain of B terms on two computed factors:
               E_gW = |dz|^T E_a + E_dz^T |a| + E_dz^T E_a + gamma_{B+2} (|dz| + E_dz)^T (|a| + E_a);  gb: the same with a = 1, E_a = 0
  loss         S = sum e^2 / (12 B): 12 fmas, B adds, a division: E = sum (2 |e| E_e + E_e^2) / (12 B), plus gamma_{B+15} of the sum
plus TINY per result for the subnormal range.  Nothing is fitted.
The Adam update given the SAME float32 gradient (adam_bound) counts the roundings of the header's operation order: the float32
constants B1, C1, B2, C2, E, lr_t (one rounding each), C1 g, g g, C2 (g g), the two fmas, lr_t m', sqrt, + E, the division and
the final subtraction.
"""
import numpy as np

import dynplan_ref as dr
from shooting_ref import philox_np

U32, TINY, gamma = dr.U32, dr.TINY, dr.gamma
STREAM_FIT = 6
BETA1, BETA2, EPS = 0.9, 0.999, 1.0e-8
GRAD_KEYS = dr.WEIGHT_KEYS


def indices(seed, k, t, batch, size):
    """the rows of Adam step t (= t0 + i) of the fit keyed (seed, k): [batch] int32 in [0, size)"""
    j = np.arange(batch, dtype=np.uint64)
    w = philox_np(seed, (STREAM_FIT << 48) | k, (np.uint64(t) << np.uint64(32)) | j)[:, 0].astype(np.uint64)
    return ((w * np.uint64(size)) >> np.uint64(32)).astype(np.int32)


def out_rscale(W):
    """1 / (out_std + 1e-6) in float64, rounded once to float32"""
    return (1.0 / (np.asarray(W["out_std"], np.float64) + dr.STD_EPS)).astype(np.float32)


def forward64(W, x, d, with_bound=False):
    """x [B,16], d [B,12] float32 rows -> dict(loss, xh, z1, a1, z2, a2, y, th, e) in float64 (and E_* with_bound)"""
    f = np.float64
    x, d = np.asarray(x, f), np.asarray(d, f)
    F = {}
    F["xh"] = (x - np.asarray(W["in_mean"], f)) * dr.rscale(W).astype(f)
    a, E = F["xh"], gamma(2) * np.abs(F["xh"])
    F["E_xh"] = E
    for l in (1, 2, 3):
        w, b = np.asarray(W["w%d" % l], f), np.asarray(W["b%d" % l], f)
        aw = np.abs(w).T
        E = E @ aw + gamma(w.shape[1] + 2) * ((np.abs(a) + E) @ aw + np.abs(b)) + TINY
        z = a @ w.T + b
        if l < 3:
            F["z%d" % l], F["E_z%d" % l] = z, E
            a = np.maximum(z, 0.0)
            F["a%d" % l] = a
        else:
            F["y"], F["E_y"] = z, E
    F["th"] = (d - np.asarray(W["out_mean"], f)) * out_rscale(W).astype(f)
    F["E_th"] = gamma(2) * np.abs(F["th"])
    F["e"] = F["y"] - F["th"]
    F["E_e"] = F["E_y"] + F["E_th"] + U32 * (np.abs(F["e"]) + F["E_y"] + F["E_th"]) + TINY
    F["loss"] = np.mean(F["e"] ** 2)
    return F


def backward64(W, x, d, with_bound=False):
    """-> (loss, {w1, b1, w2, b2, w3, b3: gradient}) in float64; with_bound: (loss, grads, loss bound, {key: bound})"""
    f = np.float64
    F = forward64(W, x, d)
    B = F["e"].shape[0]
    c = 2.0 / (12.0 * B)
    dy = F["e"] * c
    E_dy = c * F["E_e"] + gamma(2) * c * (np.abs(F["e"]) + F["E_e"]) + TINY
    w2, w3 = np.asarray(W["w2"], f), np.asarray(W["w3"], f)
    m2, m1 = F["z2"] > 0.0, F["z1"] > 0.0
    dz2 = (dy @ w3) * m2
    E_dz2 = (E_dy @ np.abs(w3) + gamma(12 + 2) * ((np.abs(dy) + E_dy) @ np.abs(w3)) + TINY) * m2
    dz1 = (dz2 @ w2) * m1
    E_dz1 = (E_dz2 @ np.abs(w2) + gamma(w2.shape[0] + 2) * ((np.abs(dz2) + E_dz2) @ np.abs(w2)) + TINY) * m1
    G, E = {}, {}
    for l, dz, E_dz, a, E_a in ((1, dz1, E_dz1, F["xh"], F["E_xh"]), (2, dz2, E_dz2, F["a1"], F["E_z1"]), (3, dy, E_dy, F["a2"], F["E_z2"])):
        G["w%d" % l], G["b%d" % l] = dz.T @ a, dz.sum(0)
        adz, aa = np.abs(dz), np.abs(a)
        E["w%d" % l] = adz.T @ E_a + E_dz.T @ aa + E_dz.T @ E_a + gamma(B + 2) * ((adz + E_dz).T @ (aa + E_a)) + TINY
        E["b%d" % l] = E_dz.sum(0) + gamma(B + 2) * (adz + E_dz).sum(0) + TINY
    if not with_bound:
        return F["loss"], G
    sq = np.sum(2.0 * np.abs(F["e"]) * F["E_e"] + F["E_e"] ** 2) / (12.0 * B)
    return F["loss"], G, sq + gamma(B + 15) * (F["loss"] + sq) + TINY, E


def grad_bound(W, x, d):
    """-> (bound of the float32 loss, {key: bound of the float32 gradient}), element for element"""
    _, _, lb, E = backward64(W, x, d, with_bound=True)
    return lb, E


def relu_edge(W, x, d):
    """the number of hidden pre-activations whose float64 value lies within its forward bound of zero: there a float32
    evaluation may legitimately take the other side of the ReLU, and grad_bound (which assumes the same mask) does not hold"""
    F = forward64(W, x, d)
    return int(sum(np.count_nonzero(np.abs(F["z%d" % l]) <= F["E_z%d" % l]) for l in (1, 2)))


def lr_t64(t, lr, beta1=BETA1, beta2=BETA2):
    return lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def adam64(w, m, v, g, t, lr, beta1=BETA1, beta2=BETA2, eps=EPS):
    """one tf.train.AdamOptimizer step, t counted from 1 -> (w', m', v') in float64"""
    f = np.float64
    w, m, v, g = (np.asarray(a, f) for a in (w, m, v, g))
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    return w - lr_t64(t, lr, beta1, beta2) * m / (np.sqrt(v) + eps), m, v


def adam_bound(w, m, v, g, t, lr, beta1=BETA1, beta2=BETA2, eps=EPS):
    """-> (E_w, E_m, E_v): bounds of |float32 update - adam64| from the same float32 (w, m, v, g), v >= 0, eps > 0"""
    f = np.float64
    w, m, v, g = (np.asarray(a, f) for a in (w, m, v, g))
    wn, mn, vn = adam64(w, m, v, g, t, lr, beta1, beta2, eps)
    u = U32
    a = u * np.abs(beta1 * m) + gamma(2) * np.abs((1.0 - beta1) * g)            # B1 m;  C1 rounded, C1 g rounded
    E_m = a + u * (np.abs(mn) + a) + TINY                                       # the fma
    a = u * np.abs(beta2 * v) + gamma(3) * (1.0 - beta2) * g * g                # B2 v;  g g, C2, C2 (g g)
    E_v = a + u * (vn + a) + TINY
    s = np.sqrt(vn)
    E_s = np.minimum(E_v / np.maximum(s, 1e-300), np.sqrt(E_v))                 # |sqrt a - sqrt b| <= |a - b| / sqrt a and <= sqrt |a - b|
    E_s = E_s + u * (s + E_s) + TINY                                            # the rounding of sqrt
    den = s + eps
    E_den = E_s + u * eps + u * (den + E_s + u * eps) + TINY                    # E rounded, the sum rounded
    lrt = abs(lr_t64(t, lr, beta1, beta2))
    num = lrt * np.abs(mn)
    E_num = lrt * E_m + gamma(2) * (num + lrt * E_m) + 4.0 * dr.U64 * num + TINY  # lr_t rounded (and its float64 pow), the product
    lo = den - E_den
    assert np.all(lo > 0.0), "the denominator's bound reaches zero: eps too small for this bound"
    q = num / den
    E_q = E_num / lo + num * E_den / (lo * den)
    E_q = E_q + u * (q + E_q) + TINY                                            # the division
    E_w = E_q + u * (np.abs(wn) + E_q) + TINY                                   # the subtraction
    return E_w, E_m, E_v


def fit64(W, M, V, buf_x, buf_d, idx, t0=0, lr=1.0e-4, beta1=BETA1, beta2=BETA2, eps=EPS, dtype=np.float64):
    """the loop: idx [iters,batch] rows per step -> (weights, m, v as dicts of `dtype` arrays, losses [iters]).  dtype float32
    runs numpy's own float32 products (not the device's summation order): a measure of float32's effect, not a restatement."""
    W = dict(W)
    for k in GRAD_KEYS:
        W[k] = np.asarray(W[k], dtype).copy()
    M = {k: np.asarray(M[k], dtype).copy() for k in GRAD_KEYS}
    V = {k: np.asarray(V[k], dtype).copy() for k in GRAD_KEYS}
    losses = []
    for i, rows in enumerate(np.asarray(idx)):
        if dtype == np.float64:
            loss, G = backward64(W, buf_x[rows], buf_d[rows])
        else:
            loss, G = _backward_as(W, buf_x[rows], buf_d[rows], dtype)
        losses.append(loss)
        for k in GRAD_KEYS:
            w, m, v = adam64(W[k], M[k], V[k], G[k], t0 + i + 1, lr, beta1, beta2, eps)
            if dtype != np.float64:
                lrt = dtype(lr_t64(t0 + i + 1, lr, beta1, beta2))
                m = dtype(beta1) * M[k] + dtype(1.0 - beta1) * G[k]
                v = dtype(beta2) * V[k] + dtype(1.0 - beta2) * (G[k] * G[k])
                w = W[k] - lrt * m / (np.sqrt(v) + dtype(eps))
            W[k], M[k], V[k] = w.astype(dtype), m.astype(dtype), v.astype(dtype)
    return W, M, V, np.asarray(losses, np.float64)


def _backward_as(W, x, d, dtype):
    f = dtype
    xh = (np.asarray(x, f) - np.asarray(W["in_mean"], f)) * dr.rscale(W).astype(f)
    z1 = xh @ W["w1"].T + W["b1"]; a1 = np.maximum(z1, f(0))
    z2 = a1 @ W["w2"].T + W["b2"]; a2 = np.maximum(z2, f(0))
    y = a2 @ W["w3"].T + W["b3"]
    e = y - (np.asarray(d, f) - np.asarray(W["out_mean"], f)) * out_rscale(W).astype(f)
    dy = e * f(2.0 / (12.0 * e.shape[0]))
    dz2 = (dy @ W["w3"]) * (z2 > 0)
    dz1 = (dz2 @ W["w2"]) * (z1 > 0)
    G = {"w1": dz1.T @ xh, "b1": dz1.sum(0), "w2": dz2.T @ a1, "b2": dz2.sum(0), "w3": dy.T @ a2, "b3": dy.sum(0)}
    return float(np.mean(e.astype(np.float64) ** 2)), G


# ---------------------------------------------------------------------------------------------------- the shared fixtures
CAPACITY, SIZE = 300, 257
STEP_SETS = ("he_20_10", "he_128_128", "ref_200_100", "dead")
STEP_BATCHES = (1, 17, 128, 256)
# the width edges (dynplan_ref.EDGE_WIDTHS): one row, a ragged second chunk of 16 rows, eight full chunks -- every path the
# kernel takes along the batch; the sixteen chunks of 256 rows take no other and stay with STEP_SETS.  step_indices seed 71
# meets the ReLU-edge condition and the mutant conditions of tests/test_dynfit_cpu.py for every (edge set, batch): the sets
# have no entry in STEP_SEEDS.
EDGE_SETS = dr.EDGE_SETS
EDGE_BATCHES = (1, 17, 128)
_cache = {}


def step_batches(name):
    return EDGE_BATCHES if name in EDGE_SETS else STEP_BATCHES


def last_unit_slices(W):
    """the gradient elements only the last unit of a hidden layer reaches: {label: (key, index)}"""
    h1, h2 = W["w1"].shape[0], W["w2"].shape[0]
    return {"row h1-1 of w1": ("w1", np.s_[h1 - 1]), "row h2-1 of w2": ("w2", np.s_[h2 - 1]),
            "column h1-1 of w2": ("w2", np.s_[:, h1 - 1]), "column h2-1 of w3": ("w3", np.s_[:, h2 - 1])}


def buffer(seed=61):
    """buf_x [300,16] (dynplan_ref.sample_obs-like observations, uniform actions), buf_d [300,12] (small deltas); the rows from
    SIZE on are NaN: no valid draw reads them"""
    if seed not in _cache:
        rng = np.random.default_rng(seed)
        x = np.concatenate([dr.sample_obs(CAPACITY, seed=seed + 1), rng.uniform(-1.0, 1.0, (CAPACITY, 4)).astype(np.float32)], axis=1)
        d = (0.05 * rng.standard_normal((CAPACITY, 12))).astype(np.float32)
        x[SIZE:], d[SIZE:] = np.nan, np.nan
        _cache[seed] = (x, d)
    return _cache[seed]


# the seed of step_indices per (weight set, batch): the first seed from 71 on for which the float64 reference alone finds no
# pre-activation within its forward bound of zero (relu_edge == 0; tests/test_dynfit_cpu.py holds it).  A batch of 128 rows of a
# 200 / 100 net has 38 400 pre-activations and the worst-case bound is some hundred times the typical error, so a batch drawn
# blindly holds a few; 71 where the first try had none.
STEP_SEEDS = {("he_128_128", 128): 82, ("he_128_128", 256): 99, ("ref_200_100", 128): 76, ("ref_200_100", 256): 74, ("dead", 128): 72,
              ("dead", 256): 75}


def step_rows(name, batch):
    """the explicit rows [1,batch] of the one-step GPU tests for a weight set"""
    return step_indices(batch, seed=STEP_SEEDS.get((name, batch), 71))


def step_indices(batch, iters=1, seed=71, size=SIZE):
    """explicit rows [iters,batch] that contain row 0, row size - 1 and a repeated row wherever the batch has room for them"""
    rng = np.random.default_rng(seed + batch)
    idx = rng.integers(0, size, (iters, batch)).astype(np.int32)
    idx[:, 0] = 0
    if batch >= 4:
        idx[:, 1] = size - 1
        idx[:, 2] = idx[:, batch - 1]
    return idx


def zero_state(W):
    return {k: np.zeros_like(W[k]) for k in GRAD_KEYS}


def moments(W, seed=81):
    """non-zero starting moments: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {k: (1e-2 * rng.standard_normal(W[k].shape)).astype(np.float32) for k in GRAD_KEYS}
    V = {k: (1e-4 * rng.random(W[k].shape)).astype(np.float32) for k in GRAD_KEYS}
    return M, V
