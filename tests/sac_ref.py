"""Float64 restatement of the SAC update on the device (quadsim_amd.sac, include/quadsim_sac.h) and the derived error bounds of its
float32 statistics and gradients.  A helper module, not a test; numpy only.  Built on tests/ddpg_ref.py and tests/td3_ref.py: the layer
and its bound (_layer), the masked back-propagation (_masked, _handed_on), the gradient sums (_grads), the mean's bound, Adam (adam64,
adam_bound, lr_t64) and polyak32 are those modules' as they are; the Philox words are tests/shooting_ref.py's.

What is restated here: a net of any of the three shapes (mlp64); the sample and its log-probability (sample64); the target value; the
regression of a critic or of the value net (_regress); the actor's loss and six gradients through all three layers of q1, the
Jacobian and the Gaussian terms (step64); the temperature's gradient; Adam, the Polyak average and the temperature's step over a
schedule with a count per step (fit64); the keyed normals on stream 7 (normals64); the header's float32 formulas of y and vb (y32,
vb32).  The constants E6 and L2PI are the header's float32 values, taken exactly.

The bounds, beyond those of ddpg_ref and td3_ref (u = 2^-24, gamma_k = k u / (1 - k u); E_x bounds |computed x - x|):
  products   fl(a b), fl(a / b), fma(a, b, c) on computed factors: the first-order terms, the product of the bounds, and u of the
             result (_mul, _div, _fma); a quotient's bound divides by the least the computed divisor can be
  exp        expf carries EXP_REL of tests/gail_ref.py (the same instruction sequence, swept over [-40, 40] there; the qss_math sweep of
             tests/test_gpu_sac.py holds it over [-20, 2]): E = x expm1(E_in) + EXP_REL x exp(E_in)
  ln         q_ln (the hardware log2 times ln 2) has no constant in an earlier reference: LN_REL is twice the worst relative error the
             qss_math sweep over (1e-6, 2] measured on an MI355X against float64 (profiles/sac/README.md); E = E_in / (the least the
             computed or the true argument can be) + LN_REL (|ln in| + that)
  clamp, min 1-Lipschitz.  Where ls_raw lies within its bound of -20 or 2 the device may take either side of the clamp's gradient:
             there the bound of dls_raw is |dls| + its bound.  The fixtures are chosen so that this happens nowhere (clamp_edges == 0)
  Jacobian   s2 = fma(-a, a, 1) from the COMPUTED a: 2 |a| E_a + E_a^2 and one rounding; ln(s2 + E6): the error of s2 + E6 divided by
             the smaller of the computed and the true s2 + E6, propagated, not capped.  Both are at least E6 (ARG_FLOOR below says
             why), so the quotient is finite everywhere: with |u| <= 3 on the fixtures' rows s2 >= 0.0098 and it is small; at
             |u| ~ 12, where s2 is 0 in float32, it is 2 |a| E_a / E6 >= 2 TANH_ABS / E6 = 1.05 per component -- large, derived, finite.
             The quotient of the Jacobian term's derivative jd divides by the same lower limit
  masks      as td3_ref: the fixtures have no pre-activation of a differentiated pass within its forward bound of zero
             (relu_edges == 0, held by tests/test_sac_cpu.py): no element is excluded.
Nothing is fitted.
"""
import numpy as np

import ddpg_ref as dd
import gail_ref as gr
import shooting_ref
import td3_ref as td

U32, TINY, gamma = dd.U32, dd.TINY, dd.gamma
adam64, adam_bound, lr_t64, polyak32 = dd.adam64, dd.adam_bound, dd.lr_t64, dd.polyak32
_layer, _mean_bound = dd._layer, dd._mean_bound
clampsel = td.clampsel
TANH_ABS, EXP_REL = gr.TANH_ABS, gr.EXP_REL
# q_ln: twice the worst relative error of the qss_math sweep on an MI355X, 2026-10-21: 1.626e-07 over 67 536 points of (1e-6, 2],
# 2001 of them within 1e-3 of 1 (profiles/sac/README.md has the measurement)
LN_MEASURED = 1.626e-7
LN_REL = 2.0 * LN_MEASURED
BETA1, BETA2, EPS = 0.9, 0.999, 1.0e-8
KEYS = dd.KEYS
ONLINE = ("actor", "q1", "q2", "v")
NETS = ONLINE + ("v_target",)
ACTOR_SHAPES = {"w0": (12, 128), "b0": (128,), "w1": (128, 128), "b1": (128,), "w2": (128, 8), "b2": (8,)}
CRITIC_SHAPES = td.CRITIC_SHAPES
VALUE_SHAPES = {"w0": (12, 128), "b0": (128,), "w1": (128, 128), "b1": (128,), "w2": (128, 1), "b2": (1,)}
STAT_NAMES = ("q1_loss", "q2_loss", "value_loss", "actor_loss", "alpha_loss", "alpha", "logp_mean", "y_mean")
GAMMA, TAU, TARGET_ENTROPY, LOG_ALPHA = 0.99, 5.0e-3, -4.0, -0.75
NOISE_STREAM = 7
LS_LO, LS_HI = -20.0, 2.0
f = np.float64
E6, L2PI = f(np.float32(1.0e-6)), f(np.float32(np.log(2.0 * np.pi)))
# A lower limit of s2 + E6 that holds for the computed AND for the true value, whatever the error of a: q_tanh returns
# copysign(1 - 2 r, x) with r > 0 and tanh_keep_nan hands that on, so |a_c| <= 1 and, x -> fma(-x, x, 1) being monotone under one
# rounding, the computed s2 = fma(-a_c, a_c, 1) >= fma(-1, 1, 1) = 0; the computed sum is then >= fl(0 + E6) = E6.  The true s2 is
# positive.  The same limit holds for den = sigma + E6, sigma = exp(..) >= 0.  One u is left off for good measure
ARG_FLOOR = E6 * (1.0 - U32)


def shapes_of(name):
    return ACTOR_SHAPES if name == "actor" else CRITIC_SHAPES if name.startswith("q") else VALUE_SHAPES


def normals64(seed, t0, steps, batch):
    """td3_ref.normals64 on Philox stream 7"""
    z = np.empty((steps, batch, 4), f)
    for j in range(batch):
        w = shooting_ref.philox_np(seed, (NOISE_STREAM << 48) | j, np.arange(t0, t0 + steps, dtype=np.uint64))
        u = ((w.astype(np.float32).astype(f) + 1.0) * 2.0 ** -32).astype(np.float32).astype(f)
        for a, b in ((0, 1), (2, 3)):
            r, th = np.sqrt(-2.0 * np.log(u[..., a])), 2.0 * np.pi * u[..., b]
            z[:, j, a], z[:, j, b] = r * np.cos(th), r * np.sin(th)
    return z


# ---------------------------------------------------------------------------------------------------- masks and gradient sums
# ddpg_ref's and td3_ref's, with one difference: should a bound be infinite (none of the fixtures' is), an infinite bound under a
# mask that is surely closed is 0, not inf * 0
def _masked(acc, E_acc, z, E_z):
    """dz = acc under the mask z > 0, and its bound; where |z| <= E_z the device may take either side"""
    m = z > 0.0
    edge = np.abs(z) <= E_z
    return acc * m, np.where(edge, np.abs(acc) + E_acc, np.where(m, E_acc, 0.0))


def _handed_on(acc, E_acc, z, E_z):
    """dq/da's masks, z <= 0 ? 0 : acc: a NaN pre-activation hands its term on (td3_ref._handed_on)"""
    with np.errstate(invalid="ignore"):
        m = ~(z <= 0.0)
        edge = np.abs(z) <= E_z
    return acc * m, np.where(edge, np.abs(acc) + E_acc, np.where(m, E_acc, 0.0))


def _grads(layers, B, G, E):
    """ddpg_ref._grads; an element whose bound is not finite has no bound (inf), whatever inf * 0 made of it"""
    with np.errstate(invalid="ignore"):
        dd._grads(layers, B, G, E)
    for l, *_ in layers:
        for k in ("w%d" % l, "b%d" % l):
            E[k] = np.where(np.isnan(E[k]), np.inf, E[k])


# ---------------------------------------------------------------------------------------------------- rounded operations
def _rnd(v, E):
    return E + U32 * (np.abs(v) + E) + TINY


def _mul(a, Ea, b, Eb):
    v = a * b
    return v, _rnd(v, Ea * np.abs(b) + np.abs(a) * Eb + Ea * Eb)


def _div(a, Ea, b, Eb, floor=0.0):
    """fl(a / b) on computed factors: |a_c / b_c - a / b| = |a_c b - a b_c| / (|b| |b_c|) <= (E_a + |a / b| E_b) / |b_c|, and the
    computed divisor is at least |b| - E_b and at least `floor`, a lower limit that holds for it whatever its error (0: none known);
    inf where neither is positive"""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = a / b
        lo = np.maximum(np.abs(b) - Eb, floor)
        E = np.where(lo > 0.0, (Ea + np.abs(v) * Eb) / np.where(lo > 0.0, lo, 1.0), np.inf)
    return v, _rnd(v, E)


def _fma(a, Ea, b, Eb, c, Ec):
    v = a * b + c
    return v, _rnd(v, Ea * np.abs(b) + np.abs(a) * Eb + Ea * Eb + Ec)


def _exp(x, Ex):
    v = np.exp(x)
    return v, v * np.expm1(Ex) + EXP_REL * v * np.exp(Ex) + TINY


def _ln(x, Ex, floor=0.0):
    """q_ln on a computed argument: |ln x_c - ln x| <= |x_c - x| / min(x_c, x) (the mean value theorem), and the smaller of the two is
    at least x - E_x and at least `floor`, a lower limit that holds for both whatever the error (0: none known); inf where neither is
    positive.  Then LN_REL of the result"""
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.log(x)
        lo = np.maximum(x - Ex, floor)
        a = np.where(lo > 0.0, Ex / np.where(lo > 0.0, lo, 1.0), np.inf)
    return v, a + LN_REL * (np.abs(v) + a) + TINY


# ---------------------------------------------------------------------------------------------------- the forward passes
def mlp64(W, x, E_x=None):
    """x [B,K0] (with its bound, None: exact) -> dict(in0, z0, h0, z1, h1, z2) and E_* of each; K0 = 12 or 16"""
    x = np.asarray(x, f)
    F = {"in0": x, "E_in0": np.zeros_like(x) if E_x is None else E_x}
    F["z0"], F["E_z0"] = _layer(x, F["E_in0"], W["w0"], W["b0"], 16)
    F["h0"] = np.maximum(F["z0"], 0.0)
    F["z1"], F["E_z1"] = _layer(F["h0"], F["E_z0"], W["w1"], W["b1"], 128)
    F["h1"] = np.maximum(F["z1"], 0.0)
    F["z2"], F["E_z2"] = _layer(F["h1"], F["E_z1"], W["w2"], W["b2"], 128)
    return F


def critic64(W, x, act, E_act=None):
    act = np.asarray(act, f)
    x = np.asarray(x, f)
    F = mlp64(W, np.concatenate([x, act], 1), np.concatenate([np.zeros_like(x), np.zeros_like(act) if E_act is None else E_act], 1))
    F["q"], F["E_q"] = F["z2"][:, 0], F["E_z2"][:, 0]
    return F


def sample64(A, z, E_zn=0.0):
    """A = mlp64(actor, obs0), z [B,4] -> dict of every intermediate of the header's item 2 and E_* of each"""
    z = np.asarray(z, f)
    E_zn = np.broadcast_to(np.asarray(E_zn, f), z.shape)
    S = {"z": z, "mu": A["z2"][:, :4], "E_mu": A["E_z2"][:, :4], "lsr": A["z2"][:, 4:], "E_lsr": A["E_z2"][:, 4:]}
    S["ls"] = clampsel(S["lsr"], LS_LO, LS_HI)
    sure = (S["lsr"] < LS_LO - S["E_lsr"]) | (S["lsr"] > LS_HI + S["E_lsr"])          # the clamp acts whatever the rounding: exact
    S["E_ls"] = np.where(sure, 0.0, S["E_lsr"])
    S["sigma"], S["E_sigma"] = _exp(S["ls"], S["E_ls"])
    S["p"], S["E_p"] = _mul(S["sigma"], S["E_sigma"], z, E_zn)
    S["u"], S["E_u"] = _fma(S["sigma"], S["E_sigma"], z, E_zn, S["mu"], S["E_mu"])
    S["a"] = np.tanh(S["u"])
    S["E_a"] = (1.0 - S["a"] ** 2) * S["E_u"] + S["E_u"] ** 2 + TANH_ABS
    S["den"] = S["sigma"] + E6
    S["E_den"] = _rnd(S["den"], S["E_sigma"])
    S["t"], S["E_t"] = _div(S["p"], S["E_p"], S["den"], S["E_den"], ARG_FLOOR)                 # (sigma >= 0: den_c >= fl(E6))
    inner = 2.0 * S["ls"] + L2PI
    S["g"], S["E_g"] = _fma(S["t"], S["E_t"], S["t"], S["E_t"], inner, _rnd(inner, 2.0 * S["E_ls"]))
    S["s2"] = 1.0 - S["a"] ** 2
    S["E_s2"] = _rnd(S["s2"], 2.0 * np.abs(S["a"]) * S["E_a"] + S["E_a"] ** 2)
    S["arg"] = S["s2"] + E6
    S["E_arg"] = _rnd(S["arg"], S["E_s2"])
    S["J"], S["E_J"] = _ln(S["arg"], S["E_arg"], ARG_FLOOR)
    S["term"] = -0.5 * S["g"] - S["J"]
    S["E_term"] = _rnd(S["term"], 0.5 * S["E_g"] + S["E_J"])
    S["logp"] = S["term"].sum(1)
    S["E_logp"] = S["E_term"].sum(1) + gamma(4) * (np.abs(S["term"]) + S["E_term"]).sum(1) + TINY
    return S


def _alpha(la):
    a = np.exp(f(la))
    return a, EXP_REL * a + TINY


def target64(P, rows, gam=GAMMA):
    """-> dict(vt, y, E_y)"""
    _, _, rew, obs1, done = rows
    rew, done = np.asarray(rew, f), np.asarray(done, f)
    T = mlp64(P["v_target"], obs1)
    vt, E_vt = T["z2"][:, 0], T["E_z2"][:, 0]
    k = np.where(done >= 1.0, 0.0, (1.0 - done) * f(np.float32(gam)))
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.where(done >= 1.0, rew, rew + k * vt)
        E_y = np.where(k == 0.0, 0.0, k * (E_vt + gamma(3) * (np.abs(vt) + E_vt)) + U32 * np.abs(y) + TINY)
    return dict(vt=vt, y=y, E_y=E_y)


def value_target64(P, rows, z, la, E_zn=0.0):
    """-> dict(S: the sample, qa, qb, mn, vb, E_vb)"""
    x0 = np.asarray(rows[0], f)
    S = sample64(mlp64(P["actor"], x0), z, E_zn)
    Qa, Qb = critic64(P["q1"], x0, S["a"], S["E_a"]), critic64(P["q2"], x0, S["a"], S["E_a"])
    qa, qb = Qa["q"], Qb["q"]
    mn = np.where(np.isnan(qa), qa, np.where(np.isnan(qb), qb, np.where(qb < qa, qb, qa)))
    E_m = np.where(np.isinf(qa), Qb["E_q"], np.where(np.isinf(qb), Qa["E_q"], np.maximum(Qa["E_q"], Qb["E_q"])))
    alpha, E_alpha = _alpha(la)
    al, E_al = _mul(alpha, E_alpha, S["logp"], S["E_logp"])
    vb = mn - al
    return dict(S=S, qa=qa, qb=qb, mn=mn, vb=vb, E_vb=_rnd(vb, E_m + E_al))


def relu_edges(P, rows, z):
    """per row: a hidden pre-activation of one of the five differentiated passes (the actor, q1 and q2 on the stored action, the value
    net, q1 on the sampled action) within its forward bound of zero"""
    x0, act = np.asarray(rows[0], f), rows[1]
    A = mlp64(P["actor"], x0)
    S = sample64(A, z)
    passes = (A, critic64(P["q1"], x0, act), critic64(P["q2"], x0, act), mlp64(P["v"], x0), critic64(P["q1"], x0, S["a"], S["E_a"]))
    out = np.zeros(x0.shape[0], bool)
    for F in passes:
        for l in (0, 1):
            out |= (np.abs(F["z%d" % l]) <= F["E_z%d" % l]).any(-1)
    return out


def clamp_edges(P, rows, z):
    """per row: a raw log-std within its forward bound of -20 or of 2"""
    S = sample64(mlp64(P["actor"], np.asarray(rows[0], f)), z)
    return ((np.abs(S["lsr"] - LS_LO) <= S["E_lsr"]) | (np.abs(S["lsr"] - LS_HI) <= S["E_lsr"])).any(-1)


def u_max(P, rows, z):
    return float(np.abs(sample64(mlp64(P["actor"], np.asarray(rows[0], f)), z)["u"]).max())


def _regress(W, F, pred, E_pred, tgt, E_tgt, B, G, E):
    """0.5 mean((pred - tgt)^2) of a net with one output whose forward pass is F -> (loss, its bound); the six gradients into G, E"""
    d = pred - tgt
    E_d = _rnd(d, E_pred + E_tgt)
    c = 1.0 / B
    dq, E_dq = (d * c)[:, None], (c * E_d + gamma(2) * c * (np.abs(d) + E_d) + TINY)[:, None]
    wc = {k_: np.asarray(W[k_], f) for k_ in KEYS}
    w2 = wc["w2"][:, 0][None, :]
    acc = w2 * dq
    dz1, E_dz1 = _masked(acc, np.abs(w2) * E_dq + U32 * np.abs(w2) * (np.abs(dq) + E_dq) + TINY, F["z1"], F["E_z1"])
    acc = dz1 @ wc["w1"].T
    with np.errstate(invalid="ignore"):
        E_acc = E_dz1 @ np.abs(wc["w1"]).T + gamma(36) * ((np.abs(dz1) + E_dz1) @ np.abs(wc["w1"]).T) + TINY
    E_acc = np.where(np.isnan(E_acc), np.inf, E_acc)
    dz0, E_dz0 = _masked(acc, E_acc, F["z0"], F["E_z0"])
    _grads(((0, dz0, E_dz0, F["in0"], F["E_in0"]), (1, dz1, E_dz1, F["h0"], F["E_z0"]), (2, dq, E_dq, F["h1"], F["E_z1"])), B, G, E)
    loss = 0.5 * np.mean(d * d)
    sq = 0.5 * np.sum(2.0 * np.abs(d) * E_d + E_d ** 2) / B
    return loss, _rnd(loss, sq + gamma(B + 3) * (loss + sq))


def step64(P, rows, z, la=LOG_ALPHA, gam=GAMMA, te=TARGET_ENTROPY, with_bound=False, E_zn=0.0):
    """P: {net name: {key: array}}, rows = (obs0 [B,12], act [B,4], rew [B], obs1 [B,12], done [B]) float32, z [B,4] the normals, la
    log_alpha -> (stats [8], {"actor": {key: gradient}, "q1", "q2", "v", "log_alpha": scalar}, aux) in float64, aux = dict(y, vb, logp,
    a and the sample S); with_bound: (stats, grads, aux, stats bound [8], {..: {key: bound}, "log_alpha": bound})"""
    obs0, act = rows[0], rows[1]
    B = obs0.shape[0]
    x0 = np.asarray(obs0, f)
    te = f(np.float32(te))
    T = target64(P, rows, gam)
    G, E = {n: {} for n in ONLINE}, {n: {} for n in ONLINE}
    st, Es = np.zeros(8), np.zeros(8)
    for i, n in enumerate(("q1", "q2")):
        Cr = critic64(P[n], x0, act)
        st[i], Es[i] = _regress(P[n], Cr, Cr["q"], Cr["E_q"], T["y"], T["E_y"], B, G[n], E[n])
    VT = value_target64(P, rows, z, la, E_zn)
    Vf = mlp64(P["v"], x0)
    st[2], Es[2] = _regress(P["v"], Vf, Vf["z2"][:, 0], Vf["E_z2"][:, 0], VT["vb"], VT["E_vb"], B, G["v"], E["v"])
    # ---- the actor
    A = mlp64(P["actor"], x0)
    S = VT["S"]
    Cp = critic64(P["q1"], x0, S["a"], S["E_a"])
    wc = {k_: np.asarray(P["q1"][k_], f) for k_ in KEYS}
    R = 1.0 / B
    acc = np.broadcast_to(wc["w2"][:, 0][None, :] * -R, (B, 128))
    dc1, E_dc1 = _handed_on(acc, gamma(2) * np.abs(acc) + TINY, Cp["z1"], Cp["E_z1"])
    acc = dc1 @ wc["w1"].T
    E_acc = E_dc1 @ np.abs(wc["w1"]).T + gamma(130) * ((np.abs(dc1) + E_dc1) @ np.abs(wc["w1"]).T) + TINY
    dc0, E_dc0 = _handed_on(acc, E_acc, Cp["z0"], Cp["E_z0"])
    w0a = wc["w0"][12:]                                                      # [4,128]
    da = dc0 @ w0a.T
    E_da = E_dc0 @ np.abs(w0a).T + gamma(130) * ((np.abs(dc0) + E_dc0) @ np.abs(w0a).T) + TINY
    alpha, E_alpha = _alpha(la)
    AR = alpha * R
    E_AR = R * E_alpha + gamma(2) * (AR + R * E_alpha) + TINY
    num, E_num = _mul(2.0 * S["a"], 2.0 * S["E_a"], S["s2"], S["E_s2"])
    jd, E_jd = _div(num, E_num, S["arg"], S["E_arg"], ARG_FLOOR)
    das2, E_das2 = _mul(da, E_da, S["s2"], S["E_s2"])
    du, E_du = _fma(AR, E_AR, jd, E_jd, das2, E_das2)
    pe, E_pe = _mul(S["p"], S["E_p"], E6, 0.0)
    dd2, E_dd2 = _mul(S["den"], S["E_den"], S["den"], S["E_den"])
    dtl, E_dtl = _div(pe, E_pe, dd2, E_dd2)
    gl, E_gl = _fma(S["t"], S["E_t"], dtl, E_dtl, 1.0, 0.0)
    m2, E_m2 = _mul(-AR, E_AR, gl, E_gl)
    dls, E_dls = _fma(du, E_du, S["p"], S["E_p"], m2, E_m2)
    with np.errstate(invalid="ignore"):
        inside = ~((S["lsr"] < LS_LO) | (S["lsr"] > LS_HI))
        edge = (np.abs(S["lsr"] - LS_LO) <= S["E_lsr"]) | (np.abs(S["lsr"] - LS_HI) <= S["E_lsr"])
    dlsr, E_dlsr = dls * inside, np.where(edge, np.abs(dls) + E_dls, np.where(inside, E_dls, 0.0))
    dz2, E_dz2 = np.concatenate([du, dlsr], 1), np.concatenate([E_du, E_dlsr], 1)
    wa = {k_: np.asarray(P["actor"][k_], f) for k_ in KEYS}
    acc = dz2 @ wa["w2"].T
    with np.errstate(invalid="ignore"):
        E_acc = E_dz2 @ np.abs(wa["w2"]).T + gamma(10) * ((np.abs(dz2) + E_dz2) @ np.abs(wa["w2"]).T) + TINY
    E_acc = np.where(np.isnan(E_acc), np.inf, E_acc)
    dz1a, E_dz1a = _masked(acc, E_acc, A["z1"], A["E_z1"])
    acc = dz1a @ wa["w1"].T
    with np.errstate(invalid="ignore"):
        E_acc = E_dz1a @ np.abs(wa["w1"]).T + gamma(36) * ((np.abs(dz1a) + E_dz1a) @ np.abs(wa["w1"]).T) + TINY
    E_acc = np.where(np.isnan(E_acc), np.inf, E_acc)
    dz0a, E_dz0a = _masked(acc, E_acc, A["z0"], A["E_z0"])
    _grads(((0, dz0a, E_dz0a, x0, np.zeros_like(x0)), (1, dz1a, E_dz1a, A["h0"], A["E_z0"]), (2, dz2, E_dz2, A["h1"], A["E_z1"])),
           B, G["actor"], E["actor"])
    al, E_al = _mul(alpha, E_alpha, S["logp"], S["E_logp"])
    e = al - Cp["q"]
    st[3], Es[3] = np.mean(e), _mean_bound(e, _rnd(e, E_al + Cp["E_q"]))
    w = S["logp"] + te
    mean_w, E_mean_w = np.mean(w), _mean_bound(w, _rnd(w, S["E_logp"]))
    st[4], Es[4] = -(f(la) * mean_w), _rnd(f(la) * mean_w, abs(f(la)) * E_mean_w)
    st[5], Es[5] = alpha, E_alpha
    st[6], Es[6] = np.mean(S["logp"]), _mean_bound(S["logp"], S["E_logp"])
    st[7], Es[7] = np.mean(T["y"]), _mean_bound(T["y"], T["E_y"])
    G["log_alpha"], E["log_alpha"] = -mean_w, E_mean_w
    aux = dict(y=T["y"], vt=T["vt"], vb=VT["vb"], qa=VT["qa"], qb=VT["qb"], logp=S["logp"], a=S["a"], S=S, E_logp=S["E_logp"], E_a=S["E_a"],
               dlsr=dlsr)
    if not with_bound:
        return st, G, aux
    return st, G, aux, np.where(np.isnan(Es), np.inf, Es), E


def fit64(P, M, V, A, replay, idx, z, counts=None, t0=0, gam=GAMMA, tau=TAU, lr=3.0e-4, te=TARGET_ENTROPY, auto_alpha=True):
    """the loop: update u = t0 + s takes rows idx[s][:counts[s]] of the replay and the normals z[s][:counts[s]]; A = [log_alpha, m, v]
    -> (nets, m, v as dicts of float64 arrays, alpha_state [3], stats [steps,8])"""
    P = {n: {k: np.asarray(P[n][k], f).copy() for k in KEYS} for n in NETS}
    M = {n: {k: np.asarray(M[n][k], f).copy() for k in KEYS} for n in ONLINE}
    V = {n: {k: np.asarray(V[n][k], f).copy() for k in KEYS} for n in ONLINE}
    A = np.asarray(A, f).copy()
    stats = []
    for s, rows in enumerate(np.asarray(idx)):
        c = len(rows) if counts is None else counts[s]
        st, G, _ = step64(P, tuple(a[rows[:c]] for a in replay), np.asarray(z)[s, :c], A[0], gam, te)
        stats.append(st)
        for n in ONLINE:
            for k in KEYS:
                P[n][k], M[n][k], V[n][k] = adam64(P[n][k], M[n][k], V[n][k], G[n][k], t0 + s + 1, lr)
        for k in KEYS:
            P["v_target"][k] = (1.0 - tau) * P["v_target"][k] + tau * P["v"][k]
        if auto_alpha:
            A[0], A[1], A[2] = adam64(A[0], A[1], A[2], G["log_alpha"], t0 + s + 1, lr)
    return P, M, V, A, np.asarray(stats)


# ---------------------------------------------------------------------------------------------------- the header's float32 formulas
def fma32(a, b, c):
    """fma on float32 operands, evaluated in float64 (exact: 48 + 1 bits) and rounded once"""
    return (np.asarray(a, np.float32).astype(f) * np.asarray(b, np.float32).astype(f) + np.asarray(c, np.float32).astype(f)).astype(np.float32)


def y32(rew, done, vt, gam=GAMMA):
    """y of the header's item 3 from the device's own v_target(obs1)"""
    rew, done, vt = (np.asarray(a, np.float32) for a in (rew, done, vt))
    k = ((np.float32(1.0) - done) * np.float32(gam)).astype(np.float32)
    return np.where(done >= 1.0, rew, fma32(k, vt, rew))


def vb32(qa, qb, alpha, logp):
    """vb of the header's item 4 from the device's own qa, qb, alpha and logp"""
    qa, qb, logp = (np.asarray(a, np.float32) for a in (qa, qb, logp))
    mn = np.where(np.isnan(qa), qa, np.where(np.isnan(qb), qb, np.where(qb < qa, qb, qa)))
    return (mn - (np.float32(alpha) * logp).astype(np.float32)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the shared fixtures
N_ROWS = 512
STEP_COUNTS = dd.STEP_COUNTS                 # 1, 10, 15, 16, 17, 33, 256: either side of the kernel's chunk of 16, the maximum
_cache = {}


def nets(seed=411, gain=1.0, bias=0.1):
    """five different nets, Glorot-uniform scaled by `gain` with small random biases (both ReLU masks are mixed); the target is a net
    of its own, so that a mix-up of online and target weights shows; the actor's log-std head is biased to about -1, so that
    |u| = |mu + sigma z| stays below 3 on every row of the fixtures"""
    key = ("nets", seed, gain, bias)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        P = {n: dd._net(rng, shapes_of(n), gain, bias) for n in NETS}
        P["actor"]["b2"] = (P["actor"]["b2"] + np.array([0.0, 0.0, 0.0, 0.0, -1.0, -0.5, -1.5, -0.8])).astype(np.float32)
        _cache[key] = P
    return _cache[key]


def _rows(seed=421, n=N_ROWS):
    """replay() and row_noise() together: of 8 n drawn (row, normals) pairs the first n at which no hidden pre-activation of a
    differentiated pass of nets() lies within its bound of zero, no raw log-std within its bound of -20 or 2 and |u| <= 3 -- chosen by the
    float64 reference alone.  The sampled action moves q1's pre-activations, so a row keeps its normals wherever it is used"""
    if ("rows", seed, n) not in _cache:
        rng = np.random.default_rng(seed)
        m = 8 * n
        obs0 = dd.dr.sample_obs(m, seed=seed + 1)
        act = rng.uniform(-1.0, 1.0, (m, 4)).astype(np.float32)
        z = rng.standard_normal((m, 4)).astype(np.float32)
        S = sample64(mlp64(nets()["actor"], np.asarray(obs0, f)), z)
        bad = relu_edges(nets(), (obs0, act), z) | clamp_edges(nets(), (obs0, act), z) | (np.abs(S["u"]) > 3.0).any(-1)
        keep = np.flatnonzero(~bad)[:n]
        assert keep.size == n
        obs0, act, z = np.ascontiguousarray(obs0[keep]), np.ascontiguousarray(act[keep]), np.ascontiguousarray(z[keep])
        obs1 = (obs0 + 0.1 * rng.standard_normal((n, 12))).astype(np.float32)
        rew = rng.standard_normal(n).astype(np.float32)
        done = (rng.random(n) < 0.3).astype(np.float32)
        done[0], done[n - 1] = 0.0, 1.0
        _cache[("rows", seed, n)] = ((obs0, act, rew, obs1, done), z)
    return _cache[("rows", seed, n)]


def replay():
    """(obs0 [n,12] docking observations, act [n,4] in [-1, 1], rew [n], obs1 [n,12], done [n] mixed 0 / 1) float32, n = 512"""
    return _rows()[0]


def row_noise():
    """[n,4] float32 standard normals, row i's wherever row i of replay() is sampled in a fixture"""
    return _rows()[1]


def noise_for(idx):
    """[steps, batch, 4]: the normals of the rows idx [steps, batch]"""
    return np.ascontiguousarray(row_noise()[np.asarray(idx)])


def noise(steps, batch):
    """the normals of the rows step_indices(batch, steps)"""
    key = ("noise", steps, batch)
    if key not in _cache:
        _cache[key] = noise_for(step_indices(batch, steps))
    return _cache[key]


step_indices = dd.step_indices


def zero_state():
    return {n: {k: np.zeros(shapes_of(n)[k], np.float32) for k in KEYS} for n in ONLINE}


def moments(seed=441):
    """non-zero starting moments: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {n: {k: (1e-3 * rng.standard_normal(shapes_of(n)[k])).astype(np.float32) for k in KEYS} for n in ONLINE}
    V = {n: {k: (1e-6 * rng.random(shapes_of(n)[k])).astype(np.float32) for k in KEYS} for n in ONLINE}
    return M, V


ALPHA_STATE = np.array([LOG_ALPHA, 0.05, 0.01], np.float32)      # log_alpha and non-zero moments of it


def noise_log_std(z, hi=(2,), scale=0.05):
    """`z` with the components `hi` scaled down: sigma is e^2 there, and |u| stays below 3 with normals of a twentieth"""
    z = np.array(z, np.float32)
    z[..., list(hi)] *= np.float32(scale)
    return z


def nets_log_std(lo=(0,), hi=(2,), shift=30.0):
    """nets() with the raw log-std of components `lo` forced below -20 and of `hi` above 2 on every row (b2 shifted by -+`shift`);
    use with noise_log_std"""
    key = ("lsclamp", tuple(lo), tuple(hi), shift)
    if key not in _cache:
        P = dict(nets())
        b2 = P["actor"]["b2"].copy()
        for c in lo:
            b2[4 + c] -= shift
        for c in hi:
            b2[4 + c] += shift
        P["actor"] = dict(P["actor"], b2=b2.astype(np.float32))
        _cache[key] = P
    return _cache[key]


def nets_saturated(shift=12.0):
    """nets() with the mean of components 0 and 1 moved to about +-`shift`: |u| ~ 12, where 1 - a^2 is 0 in float32"""
    key = ("saturated", shift)
    if key not in _cache:
        P = dict(nets())
        b2 = P["actor"]["b2"].copy()
        b2[0] += shift
        b2[1] -= shift
        P["actor"] = dict(P["actor"], b2=b2.astype(np.float32))
        _cache[key] = P
    return _cache[key]


LEARN_STEPS, LEARN_BATCH, LEARN_LR = 200, 16, 1.0e-3


def learn_case(seed=451, n=N_ROWS):
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
