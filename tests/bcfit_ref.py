"""Float64 restatement of behaviour cloning on the device (quadsim_amd.bc, include/quadsim_bc.h) and the derived error bounds of
its float32 loss, gradient and Adam update.  A helper module, not a test; numpy only.  Modelled on tests/dynfit_ref.py, whose
Adam (adam64, adam_bound, lr_t64: the same formula, as the header says) it uses as it is.

What is restated: SB2's continuous-action pretrain loss mean((a_expert - mean_action)^2) of the actor 12 -> 128 -> 128 -> 4 with
ReLU, weights in the policy's (in, out) layout (forward64), its six gradients (backward64) and tf.train.AdamOptimizer over a
schedule of minibatches with a count per step (fit64).

The bounds.  u = 2^-24, gamma_k = k u / (1 - k u); E_x bounds |computed x - x|.  The observation and the expert's action enter
exactly (E = 0: nothing normalises them).
  forward      E_l = E_{l-1} |W_l| + gamma_{K_l+2} ((|a_{l-1}| + E_{l-1}) |W_l| + |b_l|), K = 16 (the padded row), 128, 128
  error        e = fl(y - a): E_e = E_y + u (|e| + E_y)
  dy           fl(e c^), c^ = float32(2 / (4 B)): E_dy = |c| E_e + gamma_2 |c| (|e| + E_e)
  back-prop    dz1: one fma chain of 4 terms, gamma_{4+2}.  dz0: four interleaved chains of 32 fmas and a tree of two additions,
               34 roundings on the longest path: gamma_{34+2}.  Both GIVEN the same mask; at a pre-activation within its
               forward bound of zero (relu_edge) the bound covers either side of the ReLU (_masked)
  gradients    an fma chain over the B rows of the step on two computed factors (the padding rows add exact zeros):
               E_gW = E_a^T |dz| + |a|^T E_dz + E_a^T E_dz + gamma_{B+2} (|a| + E_a)^T (|dz| + E_dz);  gb: a = 1, E_a = 0
  loss         4 fmas a row, B additions, one division by the exact float32 4 B: sum (2 |e| E_e + E_e^2) / (4 B), plus
               gamma_{B+7} of the sum
plus TINY per result for the subnormal range.  Nothing is fitted.
"""
import os

import numpy as np

import dynfit_ref as fr
import dynplan_ref as dr

U32, TINY, gamma = dr.U32, dr.TINY, dr.gamma
adam64, adam_bound, lr_t64 = fr.adam64, fr.adam_bound, fr.lr_t64
BETA1, BETA2, EPS = 0.9, 0.999, 1.0e-8
KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
SHAPES = {"w0": (12, 128), "b0": (128,), "w1": (128, 128), "b1": (128,), "w2": (128, 4), "b2": (4,)}
CHAIN = (16, 128, 128)                       # the terms of a forward chain per layer
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_best_model_v0.npz")


def forward64(W, x, a, with_bound=False):
    """x [B,12], a [B,4] float32 rows -> dict(loss, z0, a0, z1, a1, y, e) in float64, and E_z0, E_z1, E_y, E_e"""
    f = np.float64
    x, a = np.asarray(x, f), np.asarray(a, f)
    F = {"x": x}
    h, E = x, np.zeros_like(x)
    for l in range(3):
        w, b = np.asarray(W["w%d" % l], f), np.asarray(W["b%d" % l], f)
        aw = np.abs(w)
        E = E @ aw + gamma(CHAIN[l] + 2) * ((np.abs(h) + E) @ aw + np.abs(b)) + TINY
        z = h @ w + b
        if l < 2:
            F["z%d" % l], F["E_z%d" % l] = z, E
            h = np.maximum(z, 0.0)
            F["a%d" % l] = h
        else:
            F["y"], F["E_y"] = z, E
    F["e"] = F["y"] - a
    F["E_e"] = F["E_y"] + U32 * (np.abs(F["e"]) + F["E_y"]) + TINY
    F["loss"] = np.mean(F["e"] ** 2)
    return F


def _masked(acc, E_acc, z, E_z):
    """dz = acc under the mask z > 0, and its bound.  Where the float64 pre-activation lies within its forward bound of zero
    (relu_edge counts these) the device may take either side of the ReLU: there the bound is |acc| + E_acc, which covers both.  At
    every other element this is (acc m, E_acc m), what the one-step fixtures -- chosen so that relu_edge == 0 -- are held to"""
    m = z > 0.0
    edge = np.abs(z) <= E_z
    return acc * m, np.where(edge, np.abs(acc) + E_acc, E_acc * m)


def backward64(W, x, a, with_bound=False):
    """-> (loss, {key: gradient}) in float64; with_bound: (loss, grads, loss bound, {key: bound})"""
    f = np.float64
    F = forward64(W, x, a)
    B = F["e"].shape[0]
    c = 2.0 / (4.0 * B)
    dy = F["e"] * c
    E_dy = c * F["E_e"] + gamma(2) * c * (np.abs(F["e"]) + F["E_e"]) + TINY
    w1, w2 = np.asarray(W["w1"], f), np.asarray(W["w2"], f)
    acc = dy @ w2.T
    dz1, E_dz1 = _masked(acc, E_dy @ np.abs(w2).T + gamma(4 + 2) * ((np.abs(dy) + E_dy) @ np.abs(w2).T) + TINY, F["z1"], F["E_z1"])
    acc = dz1 @ w1.T
    dz0, E_dz0 = _masked(acc, E_dz1 @ np.abs(w1).T + gamma(34 + 2) * ((np.abs(dz1) + E_dz1) @ np.abs(w1).T) + TINY, F["z0"], F["E_z0"])
    G, E = {}, {}
    for l, dz, E_dz, h, E_h in ((0, dz0, E_dz0, F["x"], np.zeros_like(F["x"])), (1, dz1, E_dz1, F["a0"], F["E_z0"]),
                                (2, dy, E_dy, F["a1"], F["E_z1"])):
        G["w%d" % l], G["b%d" % l] = h.T @ dz, dz.sum(0)
        adz, ah = np.abs(dz), np.abs(h)
        E["w%d" % l] = E_h.T @ adz + ah.T @ E_dz + E_h.T @ E_dz + gamma(B + 2) * ((ah + E_h).T @ (adz + E_dz)) + TINY
        E["b%d" % l] = E_dz.sum(0) + gamma(B + 2) * (adz + E_dz).sum(0) + TINY
    if not with_bound:
        return F["loss"], G
    sq = np.sum(2.0 * np.abs(F["e"]) * F["E_e"] + F["E_e"] ** 2) / (4.0 * B)
    return F["loss"], G, sq + gamma(B + 7) * (F["loss"] + sq) + TINY, E


def grad_bound(W, x, a):
    """-> (bound of the float32 loss, {key: bound of the float32 gradient}), element for element"""
    _, _, lb, E = backward64(W, x, a, with_bound=True)
    return lb, E


def loss_bound(W, x, a):
    """the bound of qsbc_loss: the float32 s_row of every row as in grad_bound; the float64 sums add nothing visible"""
    F = forward64(W, x, a)
    n = F["e"].shape[0]
    sq = np.sum(2.0 * np.abs(F["e"]) * F["E_e"] + F["E_e"] ** 2) / (4.0 * n)
    return sq + gamma(4 + 1) * (F["loss"] + sq) + 1e-15 * F["loss"] + TINY


def relu_edge(W, x, a):
    """the number of hidden pre-activations whose float64 value lies within its forward bound of zero: there a float32
    evaluation may legitimately take the other side of the ReLU, and grad_bound widens to cover both sides (_masked)"""
    F = forward64(W, x, a)
    return int(sum(np.count_nonzero(np.abs(F["z%d" % l]) <= F["E_z%d" % l]) for l in (0, 1)))


def fit64(W, M, V, obs, act, idx, counts=None, t0=0, lr=1.0e-4, beta1=BETA1, beta2=BETA2, eps=EPS, dtype=np.float64):
    """the loop: step s takes rows idx[s][:counts[s]] -> (weights, m, v as dicts of `dtype` arrays, losses [steps]).  dtype float32
    runs numpy's own float32 products (not the device's summation order): a measure of float32's effect, not a restatement."""
    W = {k: np.asarray(W[k], dtype).copy() for k in KEYS}
    M = {k: np.asarray(M[k], dtype).copy() for k in KEYS}
    V = {k: np.asarray(V[k], dtype).copy() for k in KEYS}
    losses = []
    for s, rows in enumerate(np.asarray(idx)):
        rows = rows if counts is None else rows[:counts[s]]
        t = t0 + s + 1
        if dtype == np.float64:
            loss, G = backward64(W, obs[rows], act[rows])
        else:
            loss, G = _backward_as(W, obs[rows], act[rows], dtype)
        losses.append(loss)
        for k in KEYS:
            if dtype == np.float64:
                W[k], M[k], V[k] = adam64(W[k], M[k], V[k], G[k], t, lr, beta1, beta2, eps)
            else:
                m = dtype(beta1) * M[k] + dtype(1.0 - beta1) * G[k]
                v = dtype(beta2) * V[k] + dtype(1.0 - beta2) * (G[k] * G[k])
                w = W[k] - dtype(lr_t64(t, lr, beta1, beta2)) * m / (np.sqrt(v) + dtype(eps))
                W[k], M[k], V[k] = w.astype(dtype), m.astype(dtype), v.astype(dtype)
    return W, M, V, np.asarray(losses, np.float64)


def _backward_as(W, x, a, dtype):
    f = dtype
    x = np.asarray(x, f)
    z0 = x @ W["w0"] + W["b0"]; a0 = np.maximum(z0, f(0))
    z1 = a0 @ W["w1"] + W["b1"]; a1 = np.maximum(z1, f(0))
    e = a1 @ W["w2"] + W["b2"] - np.asarray(a, f)
    dy = e * f(2.0 / (4.0 * e.shape[0]))
    dz1 = (dy @ W["w2"].T) * (z1 > 0)
    dz0 = (dz1 @ W["w1"].T) * (z0 > 0)
    G = {"w0": x.T @ dz0, "b0": dz0.sum(0), "w1": a0.T @ dz1, "b1": dz1.sum(0), "w2": a1.T @ dy, "b2": dy.sum(0)}
    return float(np.mean(e.astype(np.float64) ** 2)), G


# ---------------------------------------------------------------------------------------------------- the shared fixtures
N_ROWS = 300
STEP_SETS = ("he", "sb2", "v0", "dead")
STEP_BATCHES = (1, 15, 16, 17, 64, 256)      # either side of the kernel's chunk of 16 rows, SB2's default, the maximum
_cache = {}


def _he(rng, fan_in, fan_out):
    return (rng.standard_normal((fan_in, fan_out)) * np.sqrt(2.0 / fan_in)).astype(np.float32)


def _orthogonal(rng, fan_in, fan_out, gain):
    """SB2's ortho_init: the orthogonal factor of a Gaussian matrix, scaled"""
    a = rng.standard_normal((fan_in, fan_out))
    u, _, vt = np.linalg.svd(a, full_matrices=False)
    q = u if u.shape == (fan_in, fan_out) else vt
    return (gain * q).astype(np.float32)


def weights_he(seed=31):
    rng = np.random.default_rng(seed)
    return {"w0": _he(rng, 12, 128), "b0": (0.1 * rng.standard_normal(128)).astype(np.float32), "w1": _he(rng, 128, 128),
            "b1": (0.1 * rng.standard_normal(128)).astype(np.float32), "w2": _he(rng, 128, 4),
            "b2": (0.1 * rng.standard_normal(4)).astype(np.float32)}


def weights_sb2(seed=32):
    """a fresh SB2 actor: orthogonal with gain sqrt(2) for the hidden layers and 0.01 for the head, zero biases"""
    rng = np.random.default_rng(seed)
    g = np.sqrt(2.0)
    return {"w0": _orthogonal(rng, 12, 128, g), "b0": np.zeros(128, np.float32), "w1": _orthogonal(rng, 128, 128, g),
            "b1": np.zeros(128, np.float32), "w2": _orthogonal(rng, 128, 4, 0.01), "b2": np.zeros(4, np.float32)}


def weights_v0():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: np.ascontiguousarray(z[k], np.float32) for k in KEYS}


def weights_dead(seed=33):
    """He-initialised, with biases that keep about half of the units of either hidden layer inactive on every row"""
    W = weights_he(seed)
    rng = np.random.default_rng(seed + 100)
    for k, scale in (("b0", 12.0), ("b1", 12.0)):
        W[k] = W[k].copy()
        W[k][rng.permutation(128)[:64]] -= np.float32(scale)
    return W


WEIGHT_SETS = {"he": weights_he, "sb2": weights_sb2, "v0": weights_v0, "dead": weights_dead}


def weight_set(name):
    if name not in _cache:
        _cache[name] = WEIGHT_SETS[name]()
    return _cache[name]


def dataset(seed=51):
    """obs [300,12] (dynplan_ref.sample_obs: docking observations), act [300,4] uniform in [-1, 1]"""
    key = ("data", seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        _cache[key] = (dr.sample_obs(N_ROWS, seed=seed + 1), rng.uniform(-1.0, 1.0, (N_ROWS, 4)).astype(np.float32))
    return _cache[key]


# the seed of step_indices per (weight set, batch): the first seed from 71 on for which the float64 reference alone finds no
# pre-activation within its forward bound of zero (relu_edge == 0; tests/test_bcfit_cpu.py holds it for every pair)
STEP_SEEDS = {("he", 64): 72, ("he", 256): 99, ("dead", 15): 72, ("dead", 64): 72, ("dead", 256): 73}


def step_indices(batch, steps=1, seed=71, n=N_ROWS):
    """explicit rows [steps,batch] that contain row 0, row n - 1 and a repeated row wherever the batch has room for them"""
    rng = np.random.default_rng(seed + batch)
    idx = rng.integers(0, n, (steps, batch)).astype(np.int32)
    idx[:, 0] = 0
    if batch >= 4:
        idx[:, 1] = n - 1
        idx[:, 2] = idx[:, batch - 1]
    elif batch == 1:
        idx[1::2, 0] = n - 1
    return idx


def step_rows(name, batch):
    """the rows [1,batch] of the one-step GPU tests for a weight set"""
    return step_indices(batch, seed=STEP_SEEDS.get((name, batch), 71))


def zero_state():
    return {k: np.zeros(SHAPES[k], np.float32) for k in KEYS}


def moments(seed=81):
    """non-zero starting moments: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {k: (1e-2 * rng.standard_normal(SHAPES[k])).astype(np.float32) for k in KEYS}
    V = {k: (1e-4 * rng.random(SHAPES[k])).astype(np.float32) for k in KEYS}
    return M, V


def learn_student():
    """another He-initialised net, from zero moments: the sb2 set's head of gain 0.01 makes Adam's first steps sign steps of noise-
    sized gradients, and float32 then leaves float64 by 3e-4 of the loss -- no case for a margin"""
    return weights_he(35)


LEARN_STEPS, LEARN_BATCH, LEARN_LR = 200, 64, 1.0e-3
# "it learns": |mean of the last epoch's eight losses, float32 numpy - float64| of fit64 measured on the CPU for this very case,
# the largest of eight runs whose hidden units are permuted (the same function, another float32 summation order): 4.2e-9 ..
# 6.52e-9 (the losses fall from 0.622 to 0.01106); four times that for the device's summation order, as tests/test_gpu_dynfit.py
# derives its LEARN_MARGIN
LEARN_MARGIN = 4.0 * 6.52e-9


def teacher_case(n=512, seed=91):
    """"it learns": the targets are a quarter of the mean action of a fixed teacher (the he set) on random observations, the
    student is learn_student(); 25 epochs of 8 minibatches of 64 rows -> (obs [n,12], act [n,4], indices [200,64] int32)"""
    key = ("teacher", n, seed)
    if key not in _cache:
        import torch
        from quadsim_amd.bc import epoch_schedule
        x = dr.sample_obs(n, seed=seed)
        y = forward64(weight_set("he"), x, np.zeros((n, 4)))["y"]
        idx, cnt = epoch_schedule(n, LEARN_BATCH, LEARN_STEPS * LEARN_BATCH // n, torch.Generator().manual_seed(seed))
        assert tuple(idx.shape) == (LEARN_STEPS, LEARN_BATCH) and bool(cnt.eq(LEARN_BATCH).all())
        _cache[key] = (x, (0.25 * y).astype(np.float32), idx.numpy())
    return _cache[key]
