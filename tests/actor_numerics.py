"""Float64 reference of the device actor / critic heads and a first-order forward-error bound for them (test helper; CPU only,
no GPU, no torch needed except by the packers).

Every network evaluation on the device runs one of two MFMA paths: exact float32 (mlp_actor / mlp_heads<false>) or split bf16
("bf16x3": mlp_actor_fast / mlp_heads<true>, csrc/mlp.hpp).  Neither is held to a fixed tolerance here.
err_scale() propagates the magnitudes of the summed terms layer by layer,

    E_0 = 0,   E_l = |W_l|^T E_{l-1} + (|h_{l-1}| |W_l| + |b_l|),

with h the float64 activations after ReLU, and an evaluation in precision p must satisfy |err| <= KAPPA[p] * UNIT[p] * E
elementwise, for the action means and the value alike.  Worst ratios err / (unit * E): numpy float32 0.29-0.55, the split-bf16
emulation of tests/test_actor_numerics_cpu.py 0.029; on the MI355X the f32 kernels 0.71 and the split-bf16 kernels 0.031 (the
tower checkpoint).  The mutants of the packed images reach 0.09-0.18 (the lo image of W2 tile 3, k-step 2 zeroed; 0.05 for the
least visible fragment of the value branch) to 2.5 (a dropped cross term), so KAPPA16 = 0.08: 2.6 times the worst measured
correct kernel, below every mutant of tests/test_actor_numerics_cpu.py.

Also here: the weight sets and observation sets the numerics tests share (all generated from fixed seeds), the decoders of the
packed split-bf16 weight images (pack_fast_weights, pack_fast_actor_critic) and a numpy emulation of the split-bf16 network
that reads those bytes.
"""
import os

import numpy as np

UNIT = {"f32": 2.0 ** -24, "bf16x3": 2.0 ** -16}
KAPPA = {"f32": 4.0, "bf16x3": 0.08}

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V0_NPZ = os.path.join(GOLDEN, "policy_best_model_v0.npz")
TOWERS_ZIP = os.path.join(GOLDEN, "sb2_ppo2_docking_621_h_30M.zip")

# the uniform box of the existing actor tests: obs = (U(0,1) - 0.5) * BOX_WIDTH
BOX_WIDTH = np.array([6, 6, 6, 2, 2, 2, 3, 3, 3, 2, 2, 2], np.float64)
RMAX = {"docking-v0": 3.0, "docking-v1": 10.0}     # the out-of-range distance of each env (done threshold)


# ---------------------------------------------------------------------------------------------------- reference and bound
def _f(W, k):
    return np.asarray(W[k], np.float64)


def branches(W):
    """the actor and critic as chains of (weight [in,out], bias [out]): shared trunk w0 / b0 under both heads, or towers
    (a 'wv0' key: the value tower has its own first layer)"""
    pi = [(_f(W, "w0"), _f(W, "b0")), (_f(W, "w1"), _f(W, "b1")), (_f(W, "w2"), _f(W, "b2"))]
    if "wv1" not in W:
        return pi, None
    first = (_f(W, "wv0"), _f(W, "bv0")) if "wv0" in W else pi[0]
    return pi, [first, (_f(W, "wv1"), _f(W, "bv1")), (_f(W, "wv2"), _f(W, "bv2"))]


def _chain(layers, x):
    h, E = x, np.zeros_like(x)
    for i, (w, b) in enumerate(layers):
        aw = np.abs(w)
        z = h @ w + b
        E = E @ aw + np.abs(h) @ aw + np.abs(b)
        h = np.maximum(z, 0.0) if i + 1 < len(layers) else z
    return h, E


def net64(W, obs):
    """float64 forward of either layout -> (mean [N,4], value [N] or None without a value head)"""
    x = np.asarray(obs, np.float64)
    pi, vf = branches(W)
    mean = _chain(pi, x)[0]
    return mean, (_chain(vf, x)[0][:, 0] if vf is not None else None)


def err_scale(W, obs):
    """first-order forward-error magnitude E of each output -> (E_mean [N,4], E_value [N] or None)"""
    x = np.asarray(obs, np.float64)
    pi, vf = branches(W)
    Em = _chain(pi, x)[1]
    return Em, (_chain(vf, x)[1][:, 0] if vf is not None else None)


def bound(E, precision):
    return KAPPA[precision] * UNIT[precision] * E


def ratio(err, E, precision):
    """err / (UNIT * E): the measured multiple of the unit bound (what KAPPA caps)"""
    return np.abs(err) / (UNIT[precision] * np.maximum(E, 1e-300))


def check_clipped(act, mean64, E, precision, what=""):
    """actions clipped to [-1, 1] against the float64 mean: within the bound of clip(mean64) everywhere (clip is 1-Lipschitz),
    exactly +-1 where |mean64| exceeds 1 by more than the bound.  -> (worst ratio over the unclipped elements, unclipped
    fraction)"""
    act = np.asarray(act, np.float64)
    b = bound(E, precision)
    err = np.abs(act - np.clip(mean64, -1.0, 1.0))
    bad = ~(err <= b)
    assert not bad.any(), "%s %s: %d elements out of bound, worst err %.3g (bound %.3g)" % (
        what, precision, int(bad.sum()), float(err[bad].max()), float(b[bad][np.argmax(err[bad])]))
    sat = np.abs(mean64) > 1.0 + b
    assert np.array_equal(act[sat], np.sign(mean64[sat])), "%s %s: saturated elements not exactly +-1" % (what, precision)
    free = np.abs(mean64) < 1.0
    worst = float(ratio(act - mean64, E, precision)[free].max()) if free.any() else 0.0
    return worst, float(free.mean())


def check_unclipped(y, ref64, E, precision, what=""):
    """an unclipped output (mean, value) elementwise within the bound -> worst ratio"""
    y = np.asarray(y, np.float64)
    err = np.abs(y - ref64)
    b = bound(E, precision)
    bad = ~(err <= b)
    assert not bad.any(), "%s %s: %d elements out of bound, worst ratio %.3g (kappa %.3g)" % (
        what, precision, int(bad.sum()), float(ratio(err, E, precision)[bad].max()), KAPPA[precision])
    return float(ratio(err, E, precision).max()) if err.size else 0.0


# ---------------------------------------------------------------------------------------------------- the Runner's neglogp
def _neglogp64(W, u64, eps, squash):
    logstd = np.asarray(W["logstd"], np.float32).astype(np.float64).reshape(1, 4)
    nl = 0.5 * np.sum(np.square(eps), 1) + 0.5 * np.log(2 * np.pi) * 4 + np.sum(logstd)
    if squash:
        nl = nl + np.sum(np.log(1.0 - np.tanh(u64) ** 2 + 1e-6), 1)
    return nl


def _neglogp_bound(W, u64, m64, eps, mean_bound, squash):
    """the kernel: u = fma(std, eps, mean) (one rounding), d = (u - mean) * inv_std on ITS mean, nl = nl_const + sum 0.5 d^2
    (fma).  The mean's own error cancels in d, so d differs from eps by the roundings of u, of u - mean and of std / inv_std;
    the squashed term log(sech^2 u + 1e-6) (slope <= 2 in u) also sees the error of u, i.e. the mean's bound plus u's rounding,
    and the hardware exp2 / log2 (1 ulp, arguments up to 2|u| log2 e)."""
    u32 = UNIT["f32"] * KAPPA["f32"]
    std = np.exp(np.asarray(W["logstd"], np.float32).astype(np.float64)).reshape(1, 4)
    dd = u32 * ((np.abs(u64) + np.abs(u64 - m64)) / std + 3.0 * np.abs(eps))
    nl_const = abs(0.5 * np.log(2 * np.pi) * 4 + float(np.sum(np.asarray(W["logstd"], np.float64))))
    b = np.sum(np.abs(eps) * dd + 0.5 * dd * dd, 1) + u32 * (2.0 * np.sum(eps * eps, 1) + 2.0 * nl_const)
    if squash:
        du = mean_bound + u32 * np.abs(u64)
        L = np.log(1.0 - np.tanh(u64) ** 2 + 1e-6)
        b = b + np.sum(2.0 * du + u32 * (4.0 * np.abs(u64) + 8.0 + np.abs(L)), 1)
    return b


# ---------------------------------------------------------------------------------------------------- observations
def box_obs(n, seed):
    """the existing actor tests' uniform box"""
    rng = np.random.default_rng(seed)
    return ((rng.random((n, 12)) - 0.5) * BOX_WIDTH).astype(np.float32)


def edge_obs(n, seed, rmax):
    """observations at the edge of what an env produces: relative position of norm 0.8..1 x rmax, large relative velocity,
    attitude angles up to +-pi (the attitude limit ends far below), large body rates"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d *= (rmax * rng.uniform(0.8, 1.0, (n, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
    vel = rng.uniform(-4.0, 4.0, (n, 3))
    ang = rng.uniform(-np.pi, np.pi, (n, 3))
    rates = rng.uniform(-8.0, 8.0, (n, 3))
    return np.concatenate([d, vel, ang, rates], axis=1).astype(np.float32)


def calibration_obs():
    return np.concatenate([box_obs(4096, 101), edge_obs(2048, 102, RMAX["docking-v0"])])


# ---------------------------------------------------------------------------------------------------- weight sets
def _fit_output(W, obs, frac=0.95, target=0.9):
    """rescale each action mean (w2, b2) so the `frac` quantile of |mean| on `obs` is `target`: the actions are mostly
    unclipped, so an error in the mean reaches the clipped action"""
    W = dict(W)
    mean = net64(W, obs)[0]
    s = target / np.quantile(np.abs(mean), frac, axis=0)
    W["w2"] = (np.asarray(W["w2"], np.float64) * s[None, :]).astype(np.float32)
    W["b2"] = (np.asarray(W["b2"], np.float64) * s).astype(np.float32)
    return W


def _he(rng, fan_in, fan_out):
    return (rng.standard_normal((fan_in, fan_out)) * np.sqrt(2.0 / fan_in)).astype(np.float32)


def weights_v0():
    with np.load(V0_NPZ, allow_pickle=False) as z:
        return {k: np.asarray(z[k]) for k in z.files}


def weights_towers():
    from quadsim_amd.sb2 import read_sb2_weights
    return read_sb2_weights(TOWERS_ZIP)[1]


def weights_dead_relu(seed=11):
    """(c) He-initialised shared-trunk net; half of the first-layer biases are negative by more than the typical pre-activation,
    so many first-layer ReLUs are dead on most observations"""
    rng = np.random.default_rng(seed)
    W = {"w0": _he(rng, 12, 128), "w1": _he(rng, 128, 128), "w2": _he(rng, 128, 4), "wv1": _he(rng, 128, 128),
         "wv2": _he(rng, 128, 1)}
    b0 = rng.uniform(0.0, 0.5, 128)
    neg = rng.permutation(128)[:64]
    b0[neg] = -rng.uniform(1.0, 4.0, 64)
    W["b0"] = b0.astype(np.float32)
    for k, n in (("b1", 128), ("b2", 4), ("bv1", 128), ("bv2", 1)):
        W[k] = (0.1 * rng.standard_normal(n)).astype(np.float32)
    W["logstd"] = np.array([-0.5, -1.0, 0.0, 0.3], np.float32)
    return W


def weights_cancel(seed=12):
    """(d) shared-trunk net built for cancellation: hidden units 64..127 of both second layers repeat 0..63 with a 2e-2
    perturbation, and the output weights are w = A - A' over the two halves (A' = A(1 + 2e-2 noise)), so every mean / value
    is a difference of two near-equal sums: |output| << E"""
    rng = np.random.default_rng(seed)
    W = {"w0": _he(rng, 12, 128), "b0": (0.1 * rng.standard_normal(128)).astype(np.float32)}
    for w, b, o, bo, n_out in (("w1", "b1", "w2", "b2", 4), ("wv1", "bv1", "wv2", "bv2", 1)):
        half = _he(rng, 128, 64)
        pert = 1.0 + 2e-2 * rng.standard_normal((128, 64))
        W[w] = np.concatenate([half, half * pert], axis=1).astype(np.float32)
        bh = 0.1 * rng.standard_normal(64)
        W[b] = np.concatenate([bh, bh * (1.0 + 2e-2 * rng.standard_normal(64))]).astype(np.float32)
        A = 4.0 * rng.standard_normal((64, n_out))
        W[o] = np.concatenate([A, -A * (1.0 + 2e-2 * rng.standard_normal((64, n_out)))]).astype(np.float32)
        W[bo] = (0.01 * rng.standard_normal(n_out)).astype(np.float32)
    W["logstd"] = np.array([-0.7, -0.2, 0.1, -1.2], np.float32)
    return W


def weight_set(name):
    """(a) 'v0': the trained v0 net, (b) 'towers': the tower checkpoint, (c) 'dead': dead ReLUs, (d) 'cancel': cancellation --
    each with its action means rescaled onto mostly-unclipped values over calibration_obs()"""
    make = {"v0": weights_v0, "towers": weights_towers, "dead": weights_dead_relu, "cancel": weights_cancel}[name]
    return _fit_output(make(), calibration_obs())


WEIGHT_SETS = ("v0", "towers", "dead", "cancel")


# ---------------------------------------------------------------------------------------------------- bf16 helpers
def bf16_round(x):
    """float32 -> nearest-even bfloat16, as float32 (v_cvt_pk_bf16_f32)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + (((u >> 16) & 1) + 0x7FFF)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def split(x):
    x = np.asarray(x, np.float32)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def _bf(raw):
    return (np.asarray(raw, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---------------------------------------------------------------------------------------------------- packed-image decoders
# Fragment layout (csrc/mlp.hpp, 'Fast actor'): element j of lane l (g = l >> 4, c = l & 15) of k-step p of row tile
# t holds W^T[16 t + c][hid(p, g, j)], hid(p, g, j) = 16 (2p + (j >> 2)) + 4g + (j & 3); the first layer of the actor-only image
# holds input k = 8g + j (zero for k >= 12); the output layer lives in rows c < 4 (zero elsewhere).
_LANE = np.arange(64)
_G, _C = _LANE >> 4, _LANE & 15
_J = np.arange(8)


def _hid(p, g):
    return 16 * (2 * p + (_J[None, :] >> 2)) + 4 * np.asarray(g)[:, None] + (_J[None, :] & 3)


def _scatter_128(frag):
    """[8 tile][4 k-step][64 lane][8] -> W^T [128 out][128 in], every slot read exactly once"""
    out = np.full((128, 128), np.nan, np.float32)
    seen = np.zeros((128, 128), np.int32)
    for t in range(8):
        for p in range(4):
            rows = np.broadcast_to((16 * t + _C)[:, None], (64, 8))
            cols = _hid(p, _G)
            out[rows, cols] = frag[t, p]
            np.add.at(seen, (rows, cols), 1)
    assert (seen == 1).all(), "the A2 fragments do not cover every weight exactly once"
    return out


def decode_actor_blob(blob):
    """the bytes of pack_fast_weights -> {'hi': [W1^T, W2^T, W3^T], 'lo': [...], 'b': [b1, b2, b3 (16 padded slots)]} as the
    kernel reads them; asserts that every padding slot is zero"""
    raw = np.frombuffer(np.asarray(blob, np.uint8).tobytes(), np.uint8)
    a2 = [_bf(raw[o:o + 32768].view(np.uint16)).reshape(8, 4, 64, 8) for o in (0, 32768)]
    a1 = [_bf(raw[o:o + 8192].view(np.uint16)).reshape(8, 64, 8) for o in (65536, 65536 + 8192)]
    a3 = [_bf(raw[o:o + 4096].view(np.uint16)).reshape(4, 64, 8) for o in (81920, 81920 + 4096)]
    fb = raw[90112:].view(np.float32)
    assert fb.size == 128 + 128 + 16
    d = {"hi": [], "lo": [], "b": [fb[:128].copy(), fb[128:256].copy(), fb[256:272].copy()]}
    k1 = 8 * _G[:, None] + _J[None, :]
    for i in range(2):
        w1 = np.zeros((128, 12), np.float32)
        for rt in range(8):
            live = np.broadcast_to(k1 < 12, (64, 8))
            assert (a1[i][rt][~live] == 0).all(), "A1 padding k-slots are not zero"
            rows = np.broadcast_to((16 * rt + _C)[:, None], (64, 8))
            w1[rows[live], k1[live]] = a1[i][rt][live]
        w3 = np.full((4, 128), np.nan, np.float32)
        for q in range(4):
            assert (a3[i][q][_C >= 4] == 0).all(), "A3 rows >= 4 are not zero"
            rows = np.broadcast_to(_C[:, None], (64, 8))[_C < 4]
            w3[rows, _hid(q, _G)[_C < 4]] = a3[i][q][_C < 4]
        d["hi" if i == 0 else "lo"] = [w1, _scatter_128(a2[i]), w3]
    return d


def decode_actor_critic_blob(blob, towers=False):
    """the bytes of pack_fast_actor_critic -> {'w1': W1^T f32 [128][12], 'b1', 'pi': {'hi': [W2^T, W3^T], 'lo': ...,
    'b': [b2, b3]}, 'vf': {...}, 'wv1' / 'bv1' (towers only)}; asserts the padding zero"""
    raw = np.frombuffer(np.asarray(blob, np.uint8).tobytes(), np.uint8)
    a2 = [[_bf(raw[br * 65536 + o:br * 65536 + o + 32768].view(np.uint16)).reshape(8, 4, 64, 8) for o in (0, 32768)]
          for br in range(2)]
    o3p, o3v, ow1 = 4 * 32768, 4 * 32768 + 2048, 4 * 32768 + 2048 + 512
    a3p = [_bf(raw[o3p + o:o3p + o + 1024].view(np.uint16)).reshape(4, 4, 4, 8) for o in (0, 1024)]     # [q][row][g][j]
    a3v = [_bf(raw[o3v + o:o3v + o + 256].view(np.uint16)).reshape(4, 4, 8) for o in (0, 256)]          # [q][g][j]
    g4 = np.arange(4)
    w1 = raw[ow1:ow1 + 128 * 13 * 4].view(np.float32).reshape(128, 13)
    fb = raw[ow1 + 128 * 13 * 4:].view(np.float32)
    assert (w1[:, 12] == 0).all()
    d = {"w1": w1[:, :12].copy(), "b1": fb[:128].copy(), "pi": {"b": [fb[128:256].copy(), fb[384:388].copy()]},
         "vf": {"b": [fb[256:384].copy(), fb[388:389].copy()]}, "b3pad": fb[384:400].copy()}
    for i, part in enumerate(("hi", "lo")):
        w3p = np.full((4, 128), np.nan, np.float32)
        w3v = np.full((1, 128), np.nan, np.float32)
        for q in range(4):
            for r in range(4):
                w3p[r, _hid(q, g4)] = a3p[i][q, r]
            w3v[0, _hid(q, g4)] = a3v[i][q]
        d["pi"][part] = [_scatter_128(a2[0][i]), w3p]
        d["vf"][part] = [_scatter_128(a2[1][i]), w3v]
    rest = fb[400:]
    if towers:
        assert rest.size == 128 * 13 + 128
        wv1 = rest[:128 * 13].reshape(128, 13)
        assert (wv1[:, 12] == 0).all()
        d["wv1"], d["bv1"] = wv1[:, :12].copy(), rest[128 * 13:].copy()
    else:
        assert rest.size == 0
    return d


# ---------------------------------------------------------------------------------------------------- split-bf16 emulation
TERMS = ("wlo_xhi", "whi_xlo", "whi_xhi")      # the kernels' term order in each k-step


def split_layer(x, wt_hi, wt_lo, b, drop=None):
    """one split-bf16 layer as the kernel runs it: x [N,K] float32, W^T hi / lo [out][K] (bf16 values), bias float32.  x is
    split into RNE hi + lo, each 32-wide k-step adds the three terms, one f32 rounding per MFMA (the products are exact; the
    32-term sum is taken in float64).  drop: a term name to leave out (a mutant)."""
    x = np.asarray(x, np.float32)
    xh, xl = split(x)
    acc = np.broadcast_to(np.asarray(b, np.float32), (x.shape[0], wt_hi.shape[0])).astype(np.float32)
    wh, wl = np.asarray(wt_hi, np.float64).T, np.asarray(wt_lo, np.float64).T
    for k0 in range(0, x.shape[1], 32):
        s = slice(k0, k0 + 32)
        for term, (xa, wa) in zip(TERMS, ((xh, wl), (xl, wh), (xh, wh))):
            if term == drop:
                continue
            acc = (acc.astype(np.float64) + xa[:, s].astype(np.float64) @ wa[s]).astype(np.float32)
    return acc


def emulate_actor_blob(blob, obs, drop=None):
    """mlp_actor_fast from the bytes of pack_fast_weights -> unclipped mean [N,4].  drop = (layer 0..2, term) mutant."""
    d = decode_actor_blob(blob)
    x = np.asarray(obs, np.float32)
    for l in range(3):
        x = split_layer(x, d["hi"][l], d["lo"][l], d["b"][l][:4] if l == 2 else d["b"][l],
                        drop[1] if drop is not None and drop[0] == l else None)
        if l < 2:
            x = np.maximum(x, 0.0)
    return x


def emulate_actor_critic_blob(blob, obs, towers=False, drop=None):
    """mlp_heads<true> (either layout) from the bytes of pack_fast_actor_critic -> (mean [N,4], value [N]).  The first
    layer is exact float32; drop = (branch 'pi' | 'vf', layer 1..2, term) mutant."""
    d = decode_actor_critic_blob(blob, towers)
    x = np.asarray(obs, np.float32)
    f1 = lambda w, b: np.maximum((x.astype(np.float64) @ w.T.astype(np.float64) + b).astype(np.float32), 0.0)   # noqa: E731
    h = {"pi": f1(d["w1"], d["b1"])}
    h["vf"] = f1(d["wv1"], d["bv1"]) if towers else h["pi"]
    out = {}
    for br in ("pi", "vf"):
        y = h[br]
        for l in (1, 2):
            dr = drop[2] if drop is not None and drop[0] == br and drop[1] == l else None
            y = split_layer(y, d[br]["hi"][l - 1], d[br]["lo"][l - 1], d[br]["b"][l - 1], dr)
            if l == 1:
                y = np.maximum(y, 0.0)
        out[br] = y
    return out["pi"], out["vf"][:, 0]


def emulate_f32(W, obs):
    """plain numpy float32 evaluation of both heads -> (mean, value or None)"""
    x = np.asarray(obs, np.float32)
    pi, vf = branches(W)

    def run(layers):
        h = x
        for i, (w, b) in enumerate(layers):
            h = h @ w.astype(np.float32) + b.astype(np.float32)
            if i + 1 < len(layers):
                h = np.maximum(h, 0.0)
        return h
    return run(pi), (run(vf)[:, 0] if vf is not None else None)
