"""Float64 restatement of the TD3 update on the device (quadsim_amd.td3, include/quadsim_td3.h) and the derived error bounds of its
float32 statistics and gradients.  A helper module, not a test; numpy only.  Built on tests/ddpg_ref.py: the layer and its bound
(_layer), the actor (actor64), the masked back-propagation (_masked), the gradient sums (_grads), the mean's bound, Adam (adam64,
adam_bound, lr_t64) and polyak32 are that module's as they are; the Philox words are tests/shooting_ref.py's.

What is restated here: the critic [12 obs + 4 actions] -> 128 -> 128 -> 1 (critic64); the smoothed target action, the twin minimum and
the target value; either critic's loss and six gradients; the actor's loss and six gradients through all three layers of q1 (step64);
Adam, the delayed actor and the delayed Polyak average over a schedule with a count per step (fit64); the keyed normals (normals64).

The bounds, beyond those of ddpg_ref (u = 2^-24, gamma_k = k u / (1 - k u); E_x bounds |computed x - x|):
  e          e = clampsel(SIGMA z, -CL, CL): one rounding of the product, the clamp is 1-Lipschitz (and exact where it acts): E_e = u |SIGMA z|
             (0 for an infinite z: the clamp acts, whatever the rounding)
  a'         a' = clampsel(a1 + e, -1, 1): E_a1 + E_e and one rounding of the sum; the clamp is 1-Lipschitz
  m          min is 1-Lipschitz in the pair: E_m = max(E_qa, E_qb) (where one of the pair is infinite, the other's bound)
  y          as ddpg_ref: E_y = k (E_m + gamma_3 (|m| + E_m)) + u |y|, k = (1 - done) gamma; a terminal row is exact
  critic     the action is an exact input of layer 0 (16 terms); dz0 through w1 [128,128] as ddpg_ref's
  dq/da      dc1 = fl(w2 N) under h1's mask; dc0 a chain of 128 under h0's mask (gamma_130); da a chain of 128 on w0's action rows
             (gamma_130); then ddpg_ref's tanh derivative and the actor's own backward pass
  masks      dq/da's two masks hand a NaN activation's term on (_handed_on), the header's h <= 0 ? 0 : acc.  Otherwise as ddpg_ref: where a float64 pre-activation lies within its forward bound of zero the bound covers both sides.  The
             fixtures are chosen so that this happens nowhere (relu_edges == 0, held by tests/test_td3_cpu.py): no element is excluded.
Nothing is fitted.
"""
import numpy as np

import ddpg_ref as dd
import shooting_ref

U32, TINY, gamma = dd.U32, dd.TINY, dd.gamma
adam64, adam_bound, lr_t64, polyak32 = dd.adam64, dd.adam_bound, dd.lr_t64, dd.polyak32
_layer, _masked, _grads, _mean_bound, actor64 = dd._layer, dd._masked, dd._grads, dd._mean_bound, dd.actor64
BETA1, BETA2, EPS = 0.9, 0.999, 1.0e-8
KEYS = dd.KEYS
ONLINE = ("actor", "q1", "q2")
NETS = ONLINE + ("actor_target", "q1_target", "q2_target")
ACTOR_SHAPES = dd.ACTOR_SHAPES
CRITIC_SHAPES = {"w0": (16, 128), "b0": (128,), "w1": (128, 128), "b1": (128,), "w2": (128, 1), "b2": (1,)}
STAT_NAMES = ("q1_loss", "q2_loss", "q1_mean", "q2_mean", "y_mean", "actor_loss")
GAMMA, TAU, SIGMA, CLIP, DELAY = 0.99, 5.0e-3, 0.2, 0.5, 2
NOISE_STREAM = 6
f = np.float64


def shapes_of(name):
    return ACTOR_SHAPES if name.startswith("actor") else CRITIC_SHAPES


def actor_step(u, delay):
    return u % delay == 0


def schedule(t0, steps, delay):
    """[steps] bool: which updates t0 .. t0 + steps - 1 step the actor and the targets"""
    return np.array([actor_step(t0 + s, delay) for s in range(steps)], bool)


def normals64(seed, t0, steps, batch):
    """[steps, batch, 4] float64 Box-Muller on the words of Philox block t0 + s of subsequence (6 << 48) | slot (tests/mppi_ref.py's
    arithmetic: the device's float32 (0,1] uniform, then float64)"""
    z = np.empty((steps, batch, 4), f)
    for j in range(batch):
        w = shooting_ref.philox_np(seed, (NOISE_STREAM << 48) | j, np.arange(t0, t0 + steps, dtype=np.uint64))
        u = ((w.astype(np.float32).astype(f) + 1.0) * 2.0 ** -32).astype(np.float32).astype(f)
        for a, b in ((0, 1), (2, 3)):
            r, th = np.sqrt(-2.0 * np.log(u[..., a])), 2.0 * np.pi * u[..., b]
            z[:, j, a], z[:, j, b] = r * np.cos(th), r * np.sin(th)
    return z


# ---------------------------------------------------------------------------------------------------- the forward passes
def critic64(W, x, act, E_act=None):
    """x [B,12], act [B,4] (with its bound, None: exact) -> dict(in0, z0, h0, z1, h1, q) and E_* of each"""
    act = np.asarray(act, f)
    F = {"in0": np.concatenate([np.asarray(x, f), act], 1)}
    F["E_in0"] = np.concatenate([np.zeros(x.shape, f), np.zeros_like(act) if E_act is None else E_act], 1)
    F["z0"], F["E_z0"] = _layer(F["in0"], F["E_in0"], W["w0"], W["b0"], 16)
    F["h0"] = np.maximum(F["z0"], 0.0)
    F["z1"], F["E_z1"] = _layer(F["h0"], F["E_z0"], W["w1"], W["b1"], 128)
    F["h1"] = np.maximum(F["z1"], 0.0)
    q, E_q = _layer(F["h1"], F["E_z1"], W["w2"], W["b2"], 128)
    F["q"], F["E_q"] = q[:, 0], E_q[:, 0]
    return F


def clampsel(v, lo, hi):
    """the header's select: a NaN stays"""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def target64(P, rows, z, gam=GAMMA, sigma=SIGMA, clip=CLIP, E_z=0.0):
    """-> dict(a1, e, ap, qa, qb, m, y, E_y): the smoothed target action and the target value of every row.  E_z: what the normals
    the device used may differ from `z` by (0: the device was fed z itself)"""
    _, _, rew, obs1, done = rows
    rew, done, x1, z = np.asarray(rew, f), np.asarray(done, f), np.asarray(obs1, f), np.asarray(z, f)
    sg, cl = f(np.float32(sigma)), f(np.float32(clip))
    T = actor64(P["actor_target"], x1)
    raw = sg * z
    e = clampsel(raw, -cl, cl)
    with np.errstate(invalid="ignore"):
        # (an infinite product is clamped to +-CL exactly: its rounding bound, itself infinite, does not pass the clamp)
        E_e = np.where(np.isinf(raw), 0.0, sg * E_z + U32 * (np.abs(raw) + sg * E_z) + TINY)
    s = T["a"] + e
    ap = clampsel(s, -1.0, 1.0)
    E_ap = T["E_a"] + E_e
    E_ap = E_ap + U32 * (np.abs(s) + E_ap) + TINY
    Qa, Qb = critic64(P["q1_target"], x1, ap, E_ap), critic64(P["q2_target"], x1, ap, E_ap)
    qa, qb = Qa["q"], Qb["q"]
    m = np.where(np.isnan(qa), qa, np.where(np.isnan(qb), qb, np.where(qb < qa, qb, qa)))
    # (an infinite target value is exact in float32 as in float64: the minimum is the other critic's value, with that one's bound)
    E_m = np.where(np.isinf(qa), Qb["E_q"], np.where(np.isinf(qb), Qa["E_q"], np.maximum(Qa["E_q"], Qb["E_q"])))
    k = np.where(done >= 1.0, 0.0, (1.0 - done) * f(np.float32(gam)))
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(done >= 1.0, rew, rew + k * m)
        E_y = np.where(k == 0.0, 0.0, k * (E_m + gamma(3) * (np.abs(m) + E_m)) + U32 * np.abs(y) + TINY)
    return dict(a1=T["a"], raw=raw, e=e, s=s, ap=ap, qa=qa, qb=qb, m=m, y=y, E_y=E_y)


def edge_census(P, rows, z, sigma=SIGMA, clip=CLIP):
    """the number of rows (components) on every edge of the target value: the noise clipped at +CL and at -CL, a1 + e clipped at +1
    and at -1, qa < qb, qb < qa, terminal and non-terminal rows"""
    T = target64(P, rows, z, sigma=sigma, clip=clip)
    cl = f(np.float32(clip))
    done = np.asarray(rows[4])
    return {"noise+": int((T["raw"] > cl).sum()), "noise-": int((T["raw"] < -cl).sum()), "act+": int((T["s"] > 1.0).sum()),
            "act-": int((T["s"] < -1.0).sum()), "qa<qb": int((T["qa"] < T["qb"]).sum()), "qb<qa": int((T["qb"] < T["qa"]).sum()),
            "terminal": int((done >= 1.0).sum()), "live": int((done < 1.0).sum())}


def relu_edges(P, rows):
    """per row: a hidden pre-activation of one of the four differentiated passes (the actor, q1 and q2 on the stored action, q1 on
    the actor's action) within its forward bound of zero"""
    obs0, act = np.asarray(rows[0], f), rows[1]
    A = actor64(P["actor"], obs0)
    passes = (A, critic64(P["q1"], obs0, act), critic64(P["q2"], obs0, act), critic64(P["q1"], obs0, A["a"], A["E_a"]))
    out = np.zeros(obs0.shape[0], bool)
    for F in passes:
        for l in (0, 1):
            out |= (np.abs(F["z%d" % l]) <= F["E_z%d" % l]).any(-1)
    return out


def _handed_on(acc, E_acc, z, E_z):
    """dq/da's masks, z <= 0 ? 0 : acc: _masked for every finite z; a NaN pre-activation hands its term on, as float64 autograd's
    ReLU does (and the header's item 4), where _masked -- the trainers' h > 0 ? acc : 0 -- turns it into 0"""
    with np.errstate(invalid="ignore"):
        m = ~(z <= 0.0)
        edge = np.abs(z) <= E_z
    return acc * m, np.where(edge, np.abs(acc) + E_acc, E_acc * m)


def _critic_step(W, x0, act, y, E_y, B, G, E):
    """one critic's loss, mean and six gradients -> (loss, mean q, loss bound, mean bound)"""
    Cr = critic64(W, x0, act)
    d = Cr["q"] - y
    E_d = Cr["E_q"] + E_y
    E_d = E_d + U32 * (np.abs(d) + E_d) + TINY
    c = 2.0 / B
    dq, E_dq = (d * c)[:, None], (c * E_d + gamma(2) * c * (np.abs(d) + E_d) + TINY)[:, None]
    wc = {k_: np.asarray(W[k_], f) for k_ in KEYS}
    w2 = wc["w2"][:, 0][None, :]
    acc = w2 * dq
    dz1, E_dz1 = _masked(acc, np.abs(w2) * E_dq + U32 * np.abs(w2) * (np.abs(dq) + E_dq) + TINY, Cr["z1"], Cr["E_z1"])
    acc = dz1 @ wc["w1"].T
    E_acc = E_dz1 @ np.abs(wc["w1"]).T + gamma(36) * ((np.abs(dz1) + E_dz1) @ np.abs(wc["w1"]).T) + TINY
    dz0, E_dz0 = _masked(acc, E_acc, Cr["z0"], Cr["E_z0"])
    _grads(((0, dz0, E_dz0, Cr["in0"], Cr["E_in0"]), (1, dz1, E_dz1, Cr["h0"], Cr["E_z0"]), (2, dq, E_dq, Cr["h1"], Cr["E_z1"])), B, G, E)
    loss = np.mean(d * d)
    sq = np.sum(2.0 * np.abs(d) * E_d + E_d ** 2) / B
    return loss, np.mean(Cr["q"]), sq + gamma(B + 3) * (loss + sq) + TINY, _mean_bound(Cr["q"], Cr["E_q"])


def step64(P, rows, z, gam=GAMMA, sigma=SIGMA, clip=CLIP, actor=True, with_bound=False, E_z=0.0):
    """P: {net name: {key: array}}, rows = (obs0 [B,12], act [B,4], rew [B], obs1 [B,12], done [B]) float32, z [B,4] the normals ->
    (stats [6], {"actor": {key: gradient} (actor updates only), "q1": {..}, "q2": {..}}, y [B]) in float64; with_bound: (stats, grads,
    y, stats bound [6], {..: {key: bound}})"""
    obs0, act = rows[0], rows[1]
    B = obs0.shape[0]
    x0 = np.asarray(obs0, f)
    T = target64(P, rows, z, gam, sigma, clip, E_z)
    y, E_y = T["y"], T["E_y"]
    G, E = {"q1": {}, "q2": {}}, {"q1": {}, "q2": {}}
    l1, m1, El1, Em1 = _critic_step(P["q1"], x0, act, y, E_y, B, G["q1"], E["q1"])
    l2, m2, El2, Em2 = _critic_step(P["q2"], x0, act, y, E_y, B, G["q2"], E["q2"])
    aloss, E_aloss = 0.0, 0.0
    if actor:
        G["actor"], E["actor"] = {}, {}
        A = actor64(P["actor"], x0)
        Cp = critic64(P["q1"], x0, A["a"], A["E_a"])
        wc = {k_: np.asarray(P["q1"][k_], f) for k_ in KEYS}
        n = -1.0 / B
        acc = np.broadcast_to(wc["w2"][:, 0][None, :] * n, (B, 128))
        dc1, E_dc1 = _handed_on(acc, gamma(2) * np.abs(acc) + TINY, Cp["z1"], Cp["E_z1"])
        acc = dc1 @ wc["w1"].T
        E_acc = E_dc1 @ np.abs(wc["w1"]).T + gamma(130) * ((np.abs(dc1) + E_dc1) @ np.abs(wc["w1"]).T) + TINY
        dc0, E_dc0 = _handed_on(acc, E_acc, Cp["z0"], Cp["E_z0"])
        w0a = wc["w0"][12:]                                                      # [4,128]
        da = dc0 @ w0a.T
        E_da = E_dc0 @ np.abs(w0a).T + gamma(130) * ((np.abs(dc0) + E_dc0) @ np.abs(w0a).T) + TINY
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
        aloss, E_aloss = -np.mean(Cp["q"]), _mean_bound(Cp["q"], Cp["E_q"])
    stats = np.array([l1, l2, m1, m2, np.mean(y), aloss])
    if not with_bound:
        return stats, G, y
    return stats, G, y, np.array([El1, El2, Em1, Em2, _mean_bound(y, E_y), E_aloss]), E


def fit64(P, M, V, replay, idx, z, counts=None, t0=0, actor_t0=0, delay=DELAY, gam=GAMMA, tau=TAU, sigma=SIGMA, clip=CLIP, actor_lr=3.0e-4,
          critic_lr=3.0e-4):
    """the loop: update u = t0 + s takes rows idx[s][:counts[s]] of the replay and the normals z[s][:counts[s]]; the actor and the
    three targets move where u % delay == 0 -> (nets, m, v as dicts of float64 arrays, stats [steps,6], actor steps taken)"""
    P = {n: {k: np.asarray(P[n][k], f).copy() for k in KEYS} for n in NETS}
    M = {n: {k: np.asarray(M[n][k], f).copy() for k in KEYS} for n in ONLINE}
    V = {n: {k: np.asarray(V[n][k], f).copy() for k in KEYS} for n in ONLINE}
    stats, taken = [], 0
    for s, rows in enumerate(np.asarray(idx)):
        c = len(rows) if counts is None else counts[s]
        act = actor_step(t0 + s, delay)
        st, G, _ = step64(P, tuple(a[rows[:c]] for a in replay), np.asarray(z)[s, :c], gam, sigma, clip, actor=act)
        stats.append(st)
        for n in (ONLINE if act else ("q1", "q2")):
            t, lr = (actor_t0 + taken + 1, actor_lr) if n == "actor" else (t0 + s + 1, critic_lr)
            for k in KEYS:
                P[n][k], M[n][k], V[n][k] = adam64(P[n][k], M[n][k], V[n][k], G[n][k], t, lr)
                if act:
                    P[n + "_target"][k] = (1.0 - tau) * P[n + "_target"][k] + tau * P[n][k]
        taken += int(act)
    return P, M, V, np.asarray(stats), taken


# ---------------------------------------------------------------------------------------------------- the shared fixtures
N_ROWS = 512
STEP_COUNTS = dd.STEP_COUNTS                 # 1, 10, 15, 16, 17, 33, 256: either side of the kernel's chunk of 16, the maximum
_cache = {}


def nets(seed=311, gain=1.0, bias=0.1):
    """six different nets, Glorot-uniform scaled by `gain` with small random biases (both ReLU masks are mixed); the targets are nets
    of their own, so that a mix-up of online and target weights shows; the target actor's head is biased by +-1.5 in two components,
    so that its tanh comes near +-1 there and the smoothed action is clipped on either side"""
    key = ("nets", seed, gain, bias)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        P = {n: dd._net(rng, shapes_of(n), gain, bias) for n in NETS}
        P["actor_target"]["b2"] = (P["actor_target"]["b2"] + np.array([1.5, -1.5, 0.0, 0.0])).astype(np.float32)
        _cache[key] = P
    return _cache[key]


def nets_shifted(shift):
    """nets() with `shift` added to b2 of both target critics: target values of O(shift), so that gamma shows in y and in the critics'
    losses (the standard fixtures' target values are about 0.01).  The online nets, and with them relu_edges, are nets()'s"""
    key = ("shifted", float(shift))
    if key not in _cache:
        P = dict(nets())
        for n in ("q1_target", "q2_target"):
            P[n] = dict(P[n], b2=(P[n]["b2"] + np.float32(shift)).astype(np.float32))
        _cache[key] = P
    return _cache[key]


def replay(seed=321, n=N_ROWS):
    """(obs0 [n,12] docking observations, act [n,4] in [-1, 1], rew [n], obs1 [n,12], done [n] mixed 0 / 1) float32: of 3 n drawn rows
    the first n at which no hidden pre-activation of a differentiated pass of nets() lies within its bound of zero"""
    if ("replay", seed, n) not in _cache:
        rng = np.random.default_rng(seed)
        m = 3 * n
        obs0 = dd.dr.sample_obs(m, seed=seed + 1)
        act = rng.uniform(-1.0, 1.0, (m, 4)).astype(np.float32)
        keep = np.flatnonzero(~relu_edges(nets(), (obs0, act)))[:n]
        assert keep.size == n
        obs0, act = np.ascontiguousarray(obs0[keep]), np.ascontiguousarray(act[keep])
        obs1 = (obs0 + 0.1 * rng.standard_normal((n, 12))).astype(np.float32)
        rew = rng.standard_normal(n).astype(np.float32)
        done = (rng.random(n) < 0.3).astype(np.float32)
        done[0], done[n - 1] = 0.0, 1.0
        _cache[("replay", seed, n)] = (obs0, act, rew, obs1, done)
    return _cache[("replay", seed, n)]


step_indices = dd.step_indices


def noise(steps, batch, seed=331):
    """[steps, batch, 4] float32 standard normals; slot 0 of every step is far out on either side, so that the noise clip acts at +CL
    and at -CL wherever there is a row"""
    rng = np.random.default_rng(seed + 1000 * steps + batch)
    z = rng.standard_normal((steps, batch, 4)).astype(np.float32)
    z[:, 0, 0], z[:, 0, 1] = 3.5, -3.25
    return z


def zero_state():
    return {n: {k: np.zeros(shapes_of(n)[k], np.float32) for k in KEYS} for n in ONLINE}


def moments(seed=341):
    """non-zero starting moments: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {n: {k: (1e-3 * rng.standard_normal(shapes_of(n)[k])).astype(np.float32) for k in KEYS} for n in ONLINE}
    V = {n: {k: (1e-6 * rng.random(shapes_of(n)[k])).astype(np.float32) for k in KEYS} for n in ONLINE}
    return M, V


LEARN_STEPS, LEARN_BATCH, LEARN_LR = 200, 16, 1.0e-3


def learn_case(seed=351, n=N_ROWS):
    """"it learns": every row terminal, so y = rew and both critics regress q on rew = a smooth function of (obs0, act) -> (nets,
    replay, idx [200,16], noise [200,16,4])"""
    if ("learn", seed, n) not in _cache:
        rng = np.random.default_rng(seed)
        obs0 = dd.dr.sample_obs(n, seed=seed + 1)
        act = rng.uniform(-1.0, 1.0, (n, 4)).astype(np.float32)
        u, v = rng.standard_normal(12) / 4.0, rng.standard_normal(4)
        rew = np.tanh(obs0.astype(f) @ u + act.astype(f) @ v).astype(np.float32)
        rp = (obs0, act, rew, dd.dr.sample_obs(n, seed=seed + 2), np.ones(n, np.float32))
        idx = rng.integers(0, n, (LEARN_STEPS, LEARN_BATCH)).astype(np.int32)
        z = rng.standard_normal((LEARN_STEPS, LEARN_BATCH, 4)).astype(np.float32)
        _cache[("learn", seed, n)] = (nets(seed + 3, gain=1.0, bias=0.0), rp, idx, z)
    return _cache[("learn", seed, n)]
