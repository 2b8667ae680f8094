"""Float64 restatement of the learned-dynamics planner (quadsim_amd/dynplan.py, include/quadsim_dyn.h) and the running error
bound of one float32 model step.  A helper module, not a test; numpy only.

What is restated (MPC-based_RL.py of the reference):
  step64         Dynamic_Net.prediction (:130-136): norm = (s_a - mean) / (std + 1e-6); delta = net(norm);
                 out = delta * delta_std + delta_mean + s_a[:, 0:12], the net of :95-105 (16 -> h1 -> h2 -> 12, ReLU, ReLU, linear).
                 The contract keeps the input scale as in_rscale = float32(1 / (std + 1e-6)); step64 multiplies by that number.
  rollout64      the loop of Mpc_Controller.choose_action (:185-197) over given action sequences
  cost64         compute_cost (:203-210): -sum over the horizon of ob_as[j][i, 0:3]^2 -- the observation BEFORE each step
  choose64       choose_action: np.argmax of the costs (:199), the first maximum

A net is a dict of numpy arrays: w1 [h1,16], b1 [h1], w2 [h2,h1], b2 [h2], w3 [12,h2], b3 [12] (torch's Linear layout), in_mean
[16], in_std [16], out_mean [12], out_std [12]; everything float32-representable except in_std, whose float32 reciprocal
`rscale(W)` is what the device sees.

The bound (step_bound).  u = 2^-24, gamma_k = k u / (1 - k u).  Every float32 operation of the contract rounds once:
  normalisation  xh = fl(fl(x - m) r): two roundings, |xh^ - xh| <= gamma_2 |xh|                                        = e_0
  layer l        acc = b; acc = fma(w_k, x_k, acc), k ascending: K_l roundings on the COMPUTED inputs x~ (|x~| <= |x| + e_{l-1}),
                 e_l = |W_l| e_{l-1} + gamma_{K_l + 2} (|W_l| (|x_{l-1}| + e_{l-1}) + |b_l|);  ReLU is 1-Lipschitz.
                 (gamma_{K_l} suffices for a chain of K_l fused steps; the subscript K_l + 2 is deliberate slack.  K_l is the
                 true width: the zero padding adds fma(0, 0, acc) = acc, no rounding.)
  output         v = fma(d, sigma, mu): e_v = |sigma| e_3 + u (|d sigma + mu| + |sigma| e_3);  s' = fl(v + s): e = e_v + u (|s'| + e_v)
plus TINY for results in the subnormal range, where a rounding is absolute (<= 2^-150 each).  Derived, not fitted: no constant
here comes from a measurement.
"""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -130
STD_EPS = 1.0e-6
WEIGHT_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


def gamma(k, u=U32):
    return k * u / (1.0 - k * u)


def rscale(W):
    """in_rscale of the contract: 1 / (std + 1e-6) in float64, rounded once to float32"""
    return (1.0 / (np.asarray(W["in_std"], np.float64) + STD_EPS)).astype(np.float32)


def _layers(W):
    return [(np.asarray(W["w%d" % l], np.float64), np.asarray(W["b%d" % l], np.float64)) for l in (1, 2, 3)]


def step64(W, s, a, with_bound=False):
    """one model step in float64 for s [...,12], a [...,4] -> s' [...,12] (and the bound of a float32 evaluation at this input)"""
    s = np.asarray(s, np.float64)
    x = np.concatenate([s, np.asarray(a, np.float64)], axis=-1)
    h = (x - np.asarray(W["in_mean"], np.float64)) * rscale(W).astype(np.float64)
    e = gamma(2) * np.abs(h)
    for i, (w, b) in enumerate(_layers(W)):
        aw = np.abs(w).T
        if with_bound:
            e = e @ aw + gamma(w.shape[1] + 2) * ((np.abs(h) + e) @ aw + np.abs(b)) + TINY
        z = h @ w.T + b
        h = np.maximum(z, 0.0) if i < 2 else z
    sig, mu = np.asarray(W["out_std"], np.float64), np.asarray(W["out_mean"], np.float64)
    v = h * sig + mu
    out = v + s
    if not with_bound:
        return out
    ev = np.abs(sig) * e + U32 * (np.abs(v) + np.abs(sig) * e) + TINY
    return out, ev + U32 * (np.abs(out) + ev) + TINY


def step_bound(W, s, a):
    return step64(W, s, a, with_bound=True)[1]


def rollout64(W, obs, acts):
    """obs [N,12], acts [N,paths,horizon,4] -> the observations BEFORE each step [N,paths,horizon,12] (ob_as[j][:, 0:12])"""
    n, paths, horizon = acts.shape[:3]
    s = np.repeat(np.asarray(obs, np.float64)[:, None, :], paths, axis=1)
    before = np.zeros((n, paths, horizon, 12))
    for h in range(horizon):
        before[:, :, h] = s
        if h + 1 < horizon:
            s = step64(W, s, acts[:, :, h])
    return before


def cost64(before):
    return -np.sum(np.asarray(before, np.float64)[..., 0:3] ** 2, axis=(-1, -2))


def choose64(W, obs, acts):
    """-> (first action of the first arg-max [N,4], its index [N], the costs [N,paths])"""
    costs = cost64(rollout64(W, obs, acts))
    j = np.argmax(costs, axis=1)
    return acts[np.arange(len(j)), j, 0], j, costs


# ---------------------------------------------------------------------------------------------------- float32 emulation
def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32
    (a double rounding that differs from the fused one only when the float64 sum lands on a float32 tie: far inside the bound)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def step32(W, s, a):
    """the contract in float32, the chain k-ordered: what one lane of the kernel computes"""
    f = np.float32
    s = np.asarray(s, f)
    x = np.concatenate([s, np.asarray(a, f)], axis=-1)
    h = ((x - np.asarray(W["in_mean"], f)).astype(f) * rscale(W)).astype(f)
    for i in (1, 2, 3):
        w, b = np.asarray(W["w%d" % i], f), np.asarray(W["b%d" % i], f)
        acc = np.broadcast_to(b, h.shape[:-1] + b.shape).astype(f)
        for k in range(w.shape[1]):
            acc = _fma32(w[:, k], h[..., k:k + 1], acc)
        h = np.maximum(acc, f(0)) if i < 3 else acc
    v = _fma32(h, np.asarray(W["out_std"], f), np.asarray(W["out_mean"], f))
    return (v + s).astype(f)


# ---------------------------------------------------------------------------------------------------- the score
def score_terms64(before):
    """|rel_pos|^2 of each observation that enters a score, float64 [..., horizon]"""
    return np.sum(np.asarray(before, np.float64)[..., 0:3] ** 2, axis=-1)


def score_bound(before):
    """bound of |device score - cost64| given the SAME float32 observations: each term is -fma(p2, p2, fma(p1, p1, fl(p0 p0))),
    three roundings of a sum of non-negative numbers (gamma_3 t); the H terms are added in float64 (gamma_H at 2^-53)"""
    t = score_terms64(before)
    return gamma(3) * t.sum(-1) + gamma(t.shape[-1] + 1, U64) * (1.0 + gamma(3)) * t.sum(-1) + t.shape[-1] * TINY


# ---------------------------------------------------------------------------------------------------- weight sets
def _he(rng, fan_out, fan_in):
    return (rng.standard_normal((fan_out, fan_in)) * np.sqrt(2.0 / fan_in)).astype(np.float32)


def _normalisers(rng, trivial=False):
    if trivial:
        return dict(in_mean=np.zeros(16, np.float32), in_std=np.ones(16), out_mean=np.zeros(12, np.float32), out_std=np.ones(12, np.float32))
    return dict(in_mean=(0.5 * rng.standard_normal(16)).astype(np.float32), in_std=rng.uniform(0.5, 2.0, 16),
                out_mean=(0.01 * rng.standard_normal(12)).astype(np.float32), out_std=rng.uniform(0.02, 0.1, 12).astype(np.float32))


def weights_he(h1, h2, seed):
    rng = np.random.default_rng(seed)
    W = {"w1": _he(rng, h1, 16), "b1": (0.1 * rng.standard_normal(h1)).astype(np.float32),
         "w2": _he(rng, h2, h1), "b2": (0.1 * rng.standard_normal(h2)).astype(np.float32),
         "w3": _he(rng, 12, h2), "b3": (0.1 * rng.standard_normal(12)).astype(np.float32)}
    W.update(_normalisers(rng))
    return W


def weights_dead_relu(seed=21, h1=200, h2=100):
    """as actor_numerics.weights_dead_relu: half of the first-layer biases are negative by more than the typical pre-activation"""
    rng = np.random.default_rng(seed)
    W = weights_he(h1, h2, seed + 1000)
    b1 = rng.uniform(0.0, 0.5, h1)
    neg = rng.permutation(h1)[:h1 // 2]
    b1[neg] = -rng.uniform(1.0, 4.0, h1 // 2)
    W["b1"] = b1.astype(np.float32)
    return W


def weights_cancel(seed=22, h1=200, h2=100):
    """as actor_numerics.weights_cancel: the second half of layer 2 repeats the first with a 2e-2 perturbation and the output
    weights are A | -A', so every delta is a difference of two near-equal sums: |delta| << the bound's magnitude"""
    rng = np.random.default_rng(seed)
    W = weights_he(h1, h2, seed + 1000)
    half = _he(rng, h2 // 2, h1)
    W["w2"] = np.concatenate([half, half * (1.0 + 2e-2 * rng.standard_normal(half.shape))]).astype(np.float32)
    bh = 0.1 * rng.standard_normal(h2 // 2)
    W["b2"] = np.concatenate([bh, bh * (1.0 + 2e-2 * rng.standard_normal(h2 // 2))]).astype(np.float32)
    A = 4.0 * rng.standard_normal((12, h2 // 2))
    W["w3"] = np.concatenate([A, -A * (1.0 + 2e-2 * rng.standard_normal(A.shape))], axis=1).astype(np.float32)
    return W


def weights_zero(h1=20, h2=10):
    """every candidate predicts a zero delta: all scores tie"""
    W = {"w1": np.zeros((h1, 16), np.float32), "b1": np.zeros(h1, np.float32), "w2": np.zeros((h2, h1), np.float32),
         "b2": np.zeros(h2, np.float32), "w3": np.zeros((12, h2), np.float32), "b3": np.zeros(12, np.float32)}
    W.update(_normalisers(None, trivial=True))
    return W


def weights_wiring():
    """a net whose delta is the action, through relu(x) - relu(-x) pairs: delta[j] = a[j] for j < 3, 0 otherwise; out_std = 0.1,
    in_std = 1 - 1e-6 so that the float32 input scale is exactly 1.  No shared code with step64: the trajectory is closed-form."""
    W = weights_zero(6, 6)
    for j in range(3):
        W["w1"][2 * j, 12 + j], W["w1"][2 * j + 1, 12 + j] = 1.0, -1.0
        W["w2"][2 * j, 2 * j] = W["w2"][2 * j + 1, 2 * j + 1] = 1.0
        W["w3"][j, 2 * j], W["w3"][j, 2 * j + 1] = 1.0, -1.0
    W["in_std"] = np.full(16, 1.0 - STD_EPS)
    W["out_std"] = np.full(12, 0.1, np.float32)
    assert np.all(rscale(W) == np.float32(1.0))
    return W


def pad_net(W, h1, h2):
    """the same function with zero units appended up to (h1, h2)"""
    P = {k: np.asarray(v).copy() for k, v in W.items()}
    a1, a2 = W["w1"].shape[0], W["w2"].shape[0]
    P["w1"] = np.zeros((h1, 16), np.float32); P["w1"][:a1] = W["w1"]
    P["b1"] = np.zeros(h1, np.float32); P["b1"][:a1] = W["b1"]
    P["w2"] = np.zeros((h2, h1), np.float32); P["w2"][:a2, :a1] = W["w2"]
    P["b2"] = np.zeros(h2, np.float32); P["b2"][:a2] = W["b2"]
    P["w3"] = np.zeros((12, h2), np.float32); P["w3"][:, :a2] = W["w3"]
    return P


def weights_edge(h1, h2, seed):
    """weights_he, dense, with the bias of the LAST unit of each hidden layer at +2: that unit is the one a mishandled, partly
    filled last group of units would drop, so it has to be alive on the rows a test uses"""
    W = weights_he(h1, h2, seed)
    W["b1"][h1 - 1] = 2.0
    W["b2"][h2 - 1] = 2.0
    return W


# the width edges: hidden widths -> the compiled pair they run on.  (1, 1): one unit, three of every four k-lanes padding;
# (21, 11): h1 % 4 = 1, h2 % 4 = 3, a partly filled second tile; (64, 64): exact fill; (65, 3) / (3, 65): routed up by one width
# alone, one unit in a new tile; (128, 113): h2 > 112 is legal on (128, 128) only; (129, 1): routed up by h1 alone; (207, 111):
# one below both maxima, both % 4 = 3; (208, 112): the maxima, a full image.
EDGE_WIDTHS = {(1, 1): (64, 64), (21, 11): (64, 64), (64, 64): (64, 64), (65, 3): (128, 128), (3, 65): (128, 128),
               (128, 113): (128, 128), (129, 1): (208, 112), (207, 111): (208, 112), (208, 112): (208, 112)}
# the weight seed of entry i: the first seed from 400 + i on for which the float64 reference alone finds every condition of
# tests/test_dynplan_cpu.py::test_edge_fixture_detects_a_dropped_last_unit and of tests/test_dynfit_cpu.py's edge tests to hold
# (with a dynfit_ref.step_indices seed in 71..199 for each batch of EDGE_BATCHES; 71 does for all).  400 + i does for all but
# three.  (1, 1): at 400 the last unit of layer 1 is dead on the one row of batch 1, at 401 the last unit of layer 2 is dead on
# every plan row.  (65, 3): at 403 the last unit of layer 1 is dead on the one row of batch 1.  (3, 65): at 404 the last unit of
# layer 2 is dead on every plan row.  The bias of +2 makes a dead last unit rare, not impossible.
EDGE_WEIGHT_SEEDS = {(1, 1): 402, (21, 11): 401, (64, 64): 402, (65, 3): 404, (3, 65): 405, (128, 113): 405, (129, 1): 406,
                     (207, 111): 407, (208, 112): 408}


def edge_name(h1, h2):
    return "edge_%d_%d" % (h1, h2)


EDGE_SETS = tuple(edge_name(*w) for w in EDGE_WIDTHS)
# the shape of the edge tests of the planners: the smallest that fills one tile of 16 candidates twice and leaves a ragged
# third, two envs (the second far out: large activations), a few steps along the model's own trajectory
EDGE_N, EDGE_PATHS, EDGE_HORIZON = 2, 33, 5
EDGE_SEED, EDGE_GID0, EDGE_K = 0x5EED0123456789AB, (1 << 32) - 2, (1 << 32) + 5       # tests/test_gpu_dynplan.py's SEED, GID0, K0


def edge_obs():
    obs = sample_obs(EDGE_N)
    obs[1] *= 6.0
    return obs


def edge_plan_rows(W):
    """-> (obs [2,12], acts [2,33,5,4], before [2,33,5,12]): the inputs of every model step of the planners' edge test, along
    the float64 trajectory (the device steps from its own float32 trajectory, within step_bound of these)"""
    import shooting_ref
    obs = edge_obs()
    acts = np.stack([shooting_ref.actions_fast(EDGE_SEED, EDGE_GID0 + i, EDGE_K, EDGE_PATHS, EDGE_HORIZON) for i in range(EDGE_N)])
    s = np.repeat(obs.astype(np.float64)[:, None, :], EDGE_PATHS, axis=1)
    before = np.zeros((EDGE_N, EDGE_PATHS, EDGE_HORIZON, 12))
    for h in range(EDGE_HORIZON):                          # the last step too: the planner computes it when traj is asked for
        before[:, :, h] = s
        s = step64(W, s, acts[:, :, h])
    return obs, acts, before


WEIGHT_SETS = {
    "ref_200_100": lambda: weights_he(200, 100, 31),
    "he_128_128": lambda: weights_he(128, 128, 32),
    "he_64_64": lambda: weights_he(64, 64, 33),
    "he_20_10": lambda: weights_he(20, 10, 34),
    "he_100_50": lambda: weights_he(100, 50, 35),
    "dead": weights_dead_relu,
    "cancel": weights_cancel,
}
WEIGHT_SETS.update({edge_name(*w): (lambda w=w: weights_edge(w[0], w[1], EDGE_WEIGHT_SEEDS[w])) for w in EDGE_WIDTHS})
_cache = {}


def weight_set(name):
    if name not in _cache:
        _cache[name] = WEIGHT_SETS[name]()
    return _cache[name]


def sample_obs(n, seed=41):
    """docking observations: relative position a few metres, moderate velocity, small angles and rates"""
    rng = np.random.default_rng(seed)
    width = np.array([6, 6, 6, 2, 2, 2, 0.6, 0.6, 0.6, 2, 2, 2], np.float64)
    return ((rng.random((n, 12)) - 0.5) * width).astype(np.float32)


def to_net(W, device):
    """the quadsim_amd.DynamicsNet of a weight dict"""
    from quadsim_amd.dynplan import DynamicsNet
    net = DynamicsNet.from_arrays(*[W[k] for k in WEIGHT_KEYS], device=device)
    return net.set_normalisers(W["in_mean"], W["in_std"], W["out_mean"], W["out_std"])
