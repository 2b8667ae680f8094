"""Float64 restatement of the PPO2 update on the device (quadsim_amd.ppo2, include/quadsim_ppo.h) and the derived error bounds of
its float32 advantages, statistics, gradients, clip and Adam update.  A helper module, not a test; numpy only.  Modelled on
tests/bcfit_ref.py, whose forward64 (the forward chain and its bound) and Adam (adam64, adam_bound) it uses as they are.

What is restated: the loss of rl_baselines/ppo2/ppo2.py:147-188 on the actor-critic 12 -> 128 -> 128 -> {4 | 1} of either layout,
hand-derived PER BRANCH as the kernel computes it (backward64), the six statistics (loss64), the advantage normalisation
(adv_norm64) and tf.clip_by_global_norm + tf.train.AdamOptimizer (update64).

The bounds.  u = 2^-24, gamma_k = k u / (1 - k u); E_x bounds |computed x - x|; every product of two bounds is kept.  Inputs
(obs, actions, returns, values, old neglogp, the weights) enter exactly.
  advantage    d^ = fl(R - V): E_d = u |d|;  mean^ = fl(mean of d^): E_mean = mean E_d + u |mean|;  |std^ - std| <= sqrt(mean E_d^2)
               (the norm of the centred perturbation), R^ = fl(1 / (std^ + 1e-8)): E_R = E_std / ((std - E_std + 1e-8) (std + 1e-8))
               + u R;  A^ = fl(fl(d^ - mean^) R^): E_c = E_d + E_mean, then u;  E_A = E_c R + |d - mean| E_R + E_c E_R, then u; the
               float64 sums to 1e-12 relative.  A batch of one row: d^ - mean^ = 0 exactly, A = 0 on both sides, E_A = 0
  exp          ocml expf, 1 ulp: relative 2u =: e_x, on top of the argument's error
  z            t = fl(a - mean^): E_t = E_mean + u (|t| + E_mean);  z = fl(t / sigma^): E_z = (E_t / sigma + |z| (e_x + u)) (1 + 8u)
  neglogp      q: sum (2 |z| E_z + E_z^2) + gamma_4 sum (|z| + E_z)^2;  nl = fma(.5, q, fl(C)): E_nl = .5 E_q + u |C|, then u of the sum
  ratio        dn = fl(nl - old), r = expf(-dn): E_r = r (exp(E_dn) - 1) + e_x r exp(E_dn)
  A r, dn      two products and the rounded 1 / B: E_Ar = |A| E_r + r E_A + E_A E_r, then u; E_dn = (E_Ar + 3u |A r|) / B (1 + 8u)
  dmean        -(dn z) / sigma^: ((E_dn |z| + |dn| E_z + E_dn E_z) / sigma + |dn z / sigma| (2u + e_x)) (1 + 8u)
  dlogstd row  dn - fl(z z) dn, one rounding: E_zz = 2 |z| E_z + E_z^2 + u (z^2 + ..);  E_dn (1 + z^2 + E_zz) + |dn| E_zz, then u
  value head   e1 = fl(v^ - R): E_v + u (|e1| + E_v);  dv = fl(e1 fl(c / B)): (c / B) (E_e1 + 2u (|e1| + E_e1)).  Where the value step lies
               within its bound of the clip range, or the two losses within their bounds of each other, the device may decide
               otherwise than float64: there the gradient's bound covers e1 c / B and 0, vc either candidate, and the larger loss
               the larger bound (head64).  The fixtures have no such row; a recorded minibatch (tests/loop_replay.py) now and then has
  back-prop    tests/bcfit_ref.py's: dz1 gamma_{4+2}, dz0 gamma_{34+2}, GIVEN the same head decisions, which tests/test_ppo2_cpu.py
               holds for every fixture.  The ReLU masks: the fixtures have no pre-activation within its forward bound of zero; where a
               recorded minibatch has one (tests/loop_replay.py), the device may take either side and the bound of that dz covers both
               (_masked, as tests/ddpg_ref.py has it)
  gradients    fma chains over the rows of a slice, the slices' partials added in float64 and rounded once: gamma_{B+4} covers any
               cut of the B rows into slices; the shared trunk adds both branches' bounds and u |G|
  statistics   the rows' float32 terms are added in float64: the rows' bounds add up, divided by B, then u of the result
plus TINY per result for the subnormal range.  Nothing is fitted.
"""
import os

import numpy as np

import bcfit_ref as br
import dynplan_ref as dr

U32, TINY, gamma = br.U32, br.TINY, br.gamma
adam64, adam_bound, lr_t64 = br.adam64, br.adam_bound, br.lr_t64
BETA1, BETA2, EPS = 0.9, 0.999, 1.0e-5
E_X = 2.0 * U32                                  # expf: 1 ulp
KEYS_SHARED = ("w0", "b0", "w1", "b1", "w2", "b2", "wv1", "bv1", "wv2", "bv2", "logstd")
KEYS_TOWERS = ("w0", "b0", "w1", "b1", "w2", "b2", "wv0", "bv0", "wv1", "bv1", "wv2", "bv2", "logstd")
SLOT_KEYS = KEYS_TOWERS
SHAPES = {"w0": (12, 128), "b0": (128,), "w1": (128, 128), "b1": (128,), "w2": (128, 4), "b2": (4,), "wv0": (12, 128), "bv0": (128,),
          "wv1": (128, 128), "bv1": (128,), "wv2": (128, 1), "bv2": (1,), "logstd": (4,)}
STAT_NAMES = ("policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac", "grad_norm")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOG2PI = np.log(2.0 * np.pi)


def keys_of(W):
    return KEYS_TOWERS if "wv0" in W else KEYS_SHARED


def branches(W):
    """the two 12 -> 128 -> 128 -> out nets of the kernel's workgroups, in bcfit_ref's keys, and the slot keys behind them"""
    t = "wv0" in W
    pol = {k: W[k] for k in br.KEYS}
    vk = (("wv0", "bv0") if t else ("w0", "b0")) + ("wv1", "bv1", "wv2", "bv2")
    val = dict(zip(br.KEYS, (W[k] for k in vk)))
    return (pol, br.KEYS), (val, vk)


def adv_norm64(returns, values, with_bound=False):
    """float32 rows -> A in float64 (ppo2.py:264-265, population std), and its bound"""
    d = np.asarray(returns, np.float64) - np.asarray(values, np.float64)
    mean, std = d.mean(), d.std()
    R = 1.0 / (std + 1e-8)
    A = (d - mean) * R
    if not with_bound:
        return A
    if d.size == 1:
        return A, np.zeros_like(A)
    E_d = U32 * np.abs(d)
    E_mean = E_d.mean() + U32 * (abs(mean) + E_d.mean()) + 1e-12 * np.abs(d).mean()
    E_std = np.sqrt((E_d ** 2).mean()) + 1e-12 * std
    E_R = E_std / ((std - E_std + 1e-8) * (std + 1e-8)) + U32 * R * (1 + 4 * U32)
    E_c = E_d + E_mean
    E_c = E_c + U32 * (np.abs(d - mean) + E_c)
    E = E_c * R + np.abs(d - mean) * E_R + E_c * E_R
    return A, E + U32 * (np.abs(A) + E) + TINY


def forward64(W, batch):
    """batch: dict(obs, actions, returns, values, neglogp) of the minibatch's float32 rows -> everything of the forward pass"""
    f = np.float64
    x = np.asarray(batch["obs"], f)
    (pol, _), (val, _) = branches(W)
    Fp = br.forward64(pol, x, np.zeros((x.shape[0], 4)))
    Fv = br.forward64(val, x, np.zeros((x.shape[0], 1)))
    return Fp, Fv


def head64(W, batch, hp, Fp, Fv):
    """the two heads, per row, with bounds -> dict"""
    f = np.float64
    B = Fp["y"].shape[0]
    a, ret, vold, nlo = (np.asarray(batch[k], f) for k in ("actions", "returns", "values", "neglogp"))
    ls = np.asarray(W["logstd"], f)
    sig = np.exp(ls)
    A, E_A = adv_norm64(batch["returns"], batch["values"], with_bound=True)
    H = {"A": A, "E_A": E_A}
    mean, E_mean = Fp["y"], Fp["E_y"]
    t = a - mean
    E_t = E_mean + U32 * (np.abs(t) + E_mean) + TINY
    z = t / sig
    E_z = (E_t / sig + np.abs(z) * (E_X + U32)) * (1 + 8 * U32) + TINY
    q = (z ** 2).sum(-1)
    E_q = (2 * np.abs(z) * E_z + E_z ** 2).sum(-1) + gamma(4) * ((np.abs(z) + E_z) ** 2).sum(-1) + TINY
    Cn = 2.0 * LOG2PI + ls.sum()
    nl = 0.5 * q + Cn
    E_nl = 0.5 * E_q + U32 * abs(Cn)
    E_nl = E_nl + U32 * (np.abs(nl) + E_nl) + TINY
    dn = nl - nlo
    E_dn = E_nl + U32 * (np.abs(dn) + E_nl) + TINY
    r = np.exp(-dn)
    E_r = r * np.expm1(E_dn) + E_X * r * np.exp(E_dn) + TINY
    cr = hp["cliprange"]
    lo, hi = f(np.float32(1.0 - cr)), f(np.float32(1.0 + cr))
    rc = np.clip(r, lo, hi)
    p1, p2 = -A * r, -A * rc
    active = ~(p1 < p2)                                                   # p1 >= p2, and every NaN row: autograd hands it its NaN
    Ar = A * r
    E_Ar = np.abs(A) * E_r + r * E_A + E_A * E_r
    E_Ar = E_Ar + U32 * (np.abs(Ar) + E_Ar) + TINY
    g = np.where(active, Ar / B, 0.0 * r)                                 # dL / dneglogp (0 r: a clipped-off infinite ratio is autograd's NaN)
    E_g = np.where(active, (E_Ar + 3 * U32 * np.abs(Ar)) / B * (1 + 8 * U32) + TINY, 0.0)
    gz = g[:, None] * z
    dmean = -gz / sig
    E_dmean = ((E_g[:, None] * np.abs(z) + np.abs(g)[:, None] * E_z + E_g[:, None] * E_z) / sig + np.abs(dmean) * (2 * U32 + E_X)) * (1 + 8 * U32) + TINY
    zz = z ** 2
    E_zz = 2 * np.abs(z) * E_z + E_z ** 2
    E_zz = E_zz + U32 * (zz + E_zz) + TINY
    dls = g[:, None] * (1.0 - zz)
    E_dls = E_g[:, None] * (1.0 + zz + E_zz) + np.abs(g)[:, None] * E_zz
    E_dls = E_dls + U32 * (np.abs(dls) + E_dls) + TINY
    # the chosen surrogate term: p1, or -A times a clip constant
    rs = np.where(active, r, rc)
    E_rs = np.where(active | (rc == r), E_r, U32 * rc)
    E_p = np.abs(A) * E_rs + rs * E_A + E_A * E_rs
    E_p = E_p + U32 * (np.abs(A) * rs + E_p) + TINY
    kl = 0.5 * dn ** 2
    E_kl = np.abs(dn) * E_dn + 0.5 * E_dn ** 2 + 2 * U32 * (kl + np.abs(dn) * E_dn) + TINY
    H.update(z=z, E_z=E_z, nl=nl, E_nl=E_nl, r=r, E_r=E_r, lo=lo, hi=hi, p1=p1, p2=p2, pol_active=active, dmean=dmean, E_dmean=E_dmean,
             dls=dls, E_dls=E_dls, pg=np.maximum(p1, p2), E_pg=E_p, kl=kl, E_kl=E_kl, clipped=np.abs(r - 1.0) > f(np.float32(cr)))
    # ---- the value head
    v, E_v = Fv["y"][:, 0], Fv["E_y"][:, 0]
    crv = hp["cliprange_vf"]
    c = f(np.float32(max(crv, 0.0)))
    dv = v - vold
    vc = v if crv < 0 else np.where(dv > c, vold + c, np.where(dv < -c, vold - c, np.where(np.isnan(dv), dv, v)))
    e1, e2 = v - ret, vc - ret
    E_e1 = E_v + U32 * (np.abs(e1) + E_v) + TINY
    # a value step within its bound of the clip range: the device may clip where float64 does not, or the other way round.  The
    # two candidates for vc, v and vold +- c, lie within E_dvdiff of each other there, so the device's vc is within its own error
    # of one of them and within E_dvdiff more of float64's
    E_dvdiff = E_v + U32 * (np.abs(dv) + E_v) + TINY
    with np.errstate(invalid="ignore"):
        step_edge = (np.abs(np.abs(dv) - c) <= E_dvdiff) if crv >= 0 else np.zeros(B, bool)
    E_vc = np.where(vc == v, E_v, U32 * (np.abs(vc) + c))
    E_vc = np.where(step_edge, np.maximum(E_v, U32 * (np.abs(vc) + c)) + E_dvdiff, E_vc)
    E_e2 = np.where((vc == v) & ~step_edge, E_e1, E_vc + U32 * (np.abs(e2) + E_vc) + TINY)
    l1, l2 = e1 ** 2, e2 ** 2
    E_l1 = 2 * np.abs(e1) * E_e1 + E_e1 ** 2
    E_l1 = E_l1 + U32 * (l1 + E_l1) + TINY
    E_l2 = 2 * np.abs(e2) * E_e2 + E_e2 ** 2
    E_l2 = E_l2 + U32 * (l2 + E_l2) + TINY
    vact = ~(l1 < l2)                                                     # l1 >= l2, and every NaN row
    cB = hp["vf_coef"] / B
    dvv = np.where(vact, e1 * cB, 0.0)
    E_act = abs(cB) * (E_e1 + 2 * U32 * (np.abs(e1) + E_e1)) * (1 + 4 * U32) + TINY
    # where the two losses lie within their bounds of each other (or the step is at the clip range: float64 has l1 == l2 there, the
    # device need not) the device may take either side of l1 < l2: the gradient's bound covers e1 c / B and 0, and the larger loss
    # is within the larger bound of float64's (a maximum moves by no more than its arguments do).  Everywhere else the bounds are
    # (E_act or 0, E_l1 or E_l2) by float64's own decision, what the one-step fixtures -- which have no such row -- are held to
    with np.errstate(invalid="ignore"):
        close = (step_edge | ((l1 != l2) & (np.abs(l1 - l2) <= E_l1 + E_l2))) if crv >= 0 else np.zeros(B, bool)
    E_dvv = np.where(close, np.abs(e1 * cB) + E_act, np.where(vact, E_act, 0.0))
    vf = 0.5 * np.maximum(l1, l2)
    E_vf = 0.5 * np.where(close, np.maximum(E_l1, E_l2), np.where(vact, E_l1, E_l2))
    E_vf = E_vf + U32 * (vf + E_vf) + TINY
    H.update(v=v, E_v=E_v, dv=dv, E_dvdiff=E_dvdiff, crv=c, vc=vc, l1=l1, l2=l2, E_l1=E_l1, E_l2=E_l2,
             val_active=vact, val_clipped=(vc != v) if crv >= 0 else np.zeros(B, bool), dvv=dvv, E_dvv=E_dvv, vf=vf, E_vf=E_vf)
    return H


def _masked(acc, E_acc, z, E_z):
    """dz = acc under the mask z > 0, and its bound.  Where the float64 pre-activation lies within its forward bound of zero the device
    may take either side of the ReLU: there the bound is |acc| + E_acc, which covers both (tests/ddpg_ref.py's treatment).  At every
    other element this is (acc m, E_acc m), what the fixtures of the one-step tests -- chosen to have no such element -- are held to"""
    m = z > 0.0
    edge = np.abs(z) <= E_z
    return acc * m, np.where(edge, np.abs(acc) + E_acc, E_acc * m)


def _branch_backward(Wb, F, dy, E_dy, B):
    """bcfit_ref.backward64's back-propagation and gradients from a given dy [B,out] and its bound -> ({key: G}, {key: E})"""
    f = np.float64
    w1, w2 = np.asarray(Wb["w1"], f), np.asarray(Wb["w2"], f)
    outs = w2.shape[1]
    acc = dy @ w2.T
    dz1, E_dz1 = _masked(acc, E_dy @ np.abs(w2).T + gamma(outs + 2) * ((np.abs(dy) + E_dy) @ np.abs(w2).T) + TINY, F["z1"], F["E_z1"])
    acc = dz1 @ w1.T
    dz0, E_dz0 = _masked(acc, E_dz1 @ np.abs(w1).T + gamma(34 + 2) * ((np.abs(dz1) + E_dz1) @ np.abs(w1).T) + TINY, F["z0"], F["E_z0"])
    G, E = {}, {}
    for l, dz, E_dz, h, E_h in ((0, dz0, E_dz0, F["x"], np.zeros_like(F["x"])), (1, dz1, E_dz1, F["a0"], F["E_z0"]),
                                (2, dy, E_dy, F["a1"], F["E_z1"])):
        G["w%d" % l], G["b%d" % l] = h.T @ dz, dz.sum(0)
        adz, ah = np.abs(dz), np.abs(h)
        E["w%d" % l] = E_h.T @ adz + ah.T @ E_dz + E_h.T @ E_dz + gamma(B + 4) * ((ah + E_h).T @ (adz + E_dz)) + TINY
        E["b%d" % l] = E_dz.sum(0) + gamma(B + 4) * (adz + E_dz).sum(0) + TINY
    return G, E


def backward64(W, batch, hp, with_bound=False):
    """-> (stats [6] float64, {slot key: gradient}); with_bound: (stats, grads, stat bounds [6], {slot key: bound})"""
    Fp, Fv = forward64(W, batch)
    H = head64(W, batch, hp, Fp, Fv)
    B = Fp["y"].shape[0]
    (pol, pk), (val, vk) = branches(W)
    Gp, Ep = _branch_backward(pol, Fp, H["dmean"], H["E_dmean"], B)
    Gv, Ev = _branch_backward(val, Fv, H["dvv"][:, None], H["E_dvv"][:, None], B)
    G, E = {}, {}
    for Gb, Eb, ks in ((Gp, Ep, pk), (Gv, Ev, vk)):
        for bk, k in zip(br.KEYS, ks):
            if k in G:                                                    # the shared trunk: both branches, one rounding
                G[k] = G[k] + Gb[bk]
                E[k] = E[k] + Eb[bk] + U32 * np.abs(G[k])
            else:
                G[k], E[k] = Gb[bk], Eb[bk]
    ent = -np.float64(np.float32(-hp["ent_coef"]))
    G["logstd"] = H["dls"].sum(0) - hp["ent_coef"]
    E["logstd"] = (abs(ent - hp["ent_coef"]) + H["E_dls"].sum(0) + gamma(B + 5) * (abs(ent) + (np.abs(H["dls"]) + H["E_dls"]).sum(0)) + TINY)
    ls = np.asarray(W["logstd"], np.float64)
    entropy = ls.sum() + 2.0 * (LOG2PI + 1.0)
    norm = np.sqrt(sum((g ** 2).sum() for g in G.values()))
    stats = np.array([H["pg"].mean(), H["vf"].mean(), entropy, H["kl"].mean(), H["clipped"].mean(), norm])
    if not with_bound:
        return stats, G
    E_norm = np.sqrt(sum((e ** 2).sum() for e in E.values()))

    def fin(x, e):
        return e + 2 * U32 * (abs(x) + e) + TINY
    SB = np.array([fin(stats[0], H["E_pg"].mean()), fin(stats[1], H["E_vf"].mean()), fin(entropy, 0.0), fin(stats[3], H["E_kl"].mean()),
                   fin(stats[4], 0.0), fin(norm, E_norm)])
    return stats, G, SB, E


def loss64(W, batch, hp):
    """the six statistics of the minibatch"""
    return backward64(W, batch, hp)[0]


def total_loss64(W, batch, hp):
    s = loss64(W, batch, hp)
    return s[0] - hp["ent_coef"] * s[2] + hp["vf_coef"] * s[1]


def clip_scale64(G, max_grad_norm):
    norm = np.sqrt(sum((np.asarray(g, np.float64) ** 2).sum() for g in G.values()))
    return (max_grad_norm / max(norm, max_grad_norm) if max_grad_norm > 0 else 1.0), norm


def adam_input_bound(m, v, g, dg, t, lr, beta1=BETA1, beta2=BETA2, eps=EPS):
    """how far adam64's (w', m', v') move when the gradient moves by at most dg: first differences, every term kept"""
    f = np.float64
    m, v, g, dg = (np.asarray(a, f) for a in (m, v, g, dg))
    _, mn, vn = adam64(np.zeros_like(g), m, v, g, t, lr, beta1, beta2, eps)
    dm = (1.0 - beta1) * dg
    dv = (1.0 - beta2) * (2.0 * np.abs(g) * dg + dg ** 2)
    s = np.sqrt(vn)
    ds = np.minimum(dv / np.maximum(s, 1e-300), np.sqrt(dv))
    den = s + eps
    lo = np.maximum(den - ds, eps)
    lrt = abs(lr_t64(t, lr, beta1, beta2))
    return lrt * (dm / lo + np.abs(mn) * ds / (lo * den)), dm, dv


def update64(W, M, V, G, hp, t, beta1=BETA1, beta2=BETA2, eps=EPS):
    """tf.clip_by_global_norm + one tf.train.AdamOptimizer step from the gradients G -> (W', M', V', scale, norm)"""
    scale, norm = clip_scale64(G, hp["max_grad_norm"])
    Wn, Mn, Vn = {}, {}, {}
    for k in G:
        Wn[k], Mn[k], Vn[k] = adam64(W[k], M[k], V[k], np.asarray(G[k], np.float64) * scale, t, hp["lr"], beta1, beta2, eps)
    return Wn, Mn, Vn, scale, norm


def update_bound(W, M, V, G, hp, t, beta1=BETA1, beta2=BETA2, eps=EPS):
    """bounds of the device's (w, m, v) against update64 of the SAME float32 gradients G: the scale is rounded to float32 and the
    product rounded (and the norm's float64 sum may be ordered otherwise): dg = 4u |g'|, through adam_input_bound, on top of
    adam_bound at g'"""
    scale, _ = clip_scale64(G, hp["max_grad_norm"])
    out = {}
    for k in G:
        g = np.asarray(G[k], np.float64) * scale
        dg = 4 * U32 * np.abs(g) + TINY if hp["max_grad_norm"] > 0 else np.zeros_like(g)
        Ew, Em, Ev = adam_bound(W[k], M[k], V[k], g, t, hp["lr"], beta1, beta2, eps)
        dw, dm, dv = adam_input_bound(M[k], V[k], g, dg, t, hp["lr"], beta1, beta2, eps)
        out[k] = (Ew + dw * (1 + 4 * U32), Em + dm * (1 + 4 * U32), Ev + dv * (1 + 4 * U32))
    return out


# ---------------------------------------------------------------------------------------------------- the fixture conditions
def head_classes(H):
    """the six head classes of a minibatch -> {name: row mask}"""
    A, r, lo, hi = H["A"], H["r"], H["lo"], H["hi"]
    return {"policy clipped-off A>0": (A > 0) & (r > hi) & ~H["pol_active"], "policy clipped-off A<0": (A < 0) & (r < lo) & ~H["pol_active"],
            "policy active outside A>0": (A > 0) & (r < lo) & H["pol_active"], "policy active outside A<0": (A < 0) & (r > hi) & H["pol_active"],
            "value clipped-off": H["val_clipped"] & ~H["val_active"], "value active": H["val_active"]}


def edge_rows(W, batch, hp):
    """the rows of a minibatch at which float32 may legitimately decide otherwise than float64 -> ({condition: row mask}, H); the
    bounds above hold where no row is marked.  Only "advantage at zero" depends on the other rows of the minibatch"""
    Fp, Fv = forward64(W, batch)
    H = head64(W, batch, hp, Fp, Fv)
    out = {"preactivation": np.any([(np.abs(F["z%d" % l]) <= F["E_z%d" % l]).any(-1) for F in (Fp, Fv) for l in (0, 1)], axis=0)}
    r, E_r = H["r"], H["E_r"] + 2.0 * U32
    out["ratio at 1 +- eps"] = ((np.abs(r - H["lo"]) <= E_r) | (np.abs(r - H["hi"]) <= E_r)
                                | (np.abs(np.abs(r - 1.0) - np.float64(np.float32(hp["cliprange"]))) <= E_r))
    out["advantage at zero"] = (np.abs(H["A"]) <= H["E_A"]) & (H["A"] != 0.0)
    if hp["cliprange_vf"] >= 0:
        out["value step at cliprange_vf"] = np.abs(np.abs(H["dv"]) - H["crv"]) <= H["E_dvdiff"]
        out["value losses close"] = (H["l1"] != H["l2"]) & (np.abs(H["l1"] - H["l2"]) <= H["E_l1"] + H["E_l2"])
    return out, H


def edge_counts(W, batch, hp):
    """edge_rows as counts"""
    out, H = edge_rows(W, batch, hp)
    return {k: int(np.count_nonzero(v)) for k, v in out.items()}, H


# ---------------------------------------------------------------------------------------------------- the shared fixtures
N_ROWS = 300
CLIPRANGE = 0.2
STEP_BATCHES = (1, 15, 16, 17, 64, 300)
CASES = (("he", "shared"), ("he", "towers"), ("sb2", "shared"), ("sb2", "towers"), ("dead", "shared"), ("dead", "towers"), ("v0", "shared"),
         ("zip", "towers"))
CASE_IDS = ["%s-%s" % c for c in CASES]
# the settings of the one-step case: the clip active (the gradient norms of the fixtures are 0.05 .. 50), both value modes
HP_NOVCLIP = dict(lr=1e-2, cliprange=CLIPRANGE, cliprange_vf=-1.0, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.01)
HP_VCLIP = dict(HP_NOVCLIP, cliprange_vf=CLIPRANGE)
HPS = {"novclip": HP_NOVCLIP, "vclip": HP_VCLIP}
_cache = {}


def _value_branch(rng, towers, kind):
    if kind == "sb2":
        g = np.sqrt(2.0)
        W = {"wv1": br._orthogonal(rng, 128, 128, g), "bv1": np.zeros(128, np.float32), "wv2": br._orthogonal(rng, 128, 1, 1.0),
             "bv2": np.zeros(1, np.float32)}
        if towers:
            W.update(wv0=br._orthogonal(rng, 12, 128, g), bv0=np.zeros(128, np.float32))
        return W
    W = {"wv1": br._he(rng, 128, 128), "bv1": (0.1 * rng.standard_normal(128)).astype(np.float32), "wv2": br._he(rng, 128, 1),
         "bv2": (0.1 * rng.standard_normal(1)).astype(np.float32)}
    if towers:
        W.update(wv0=br._he(rng, 12, 128), bv0=(0.1 * rng.standard_normal(128)).astype(np.float32))
    if kind == "dead":
        for k in (("bv0", "bv1") if towers else ("bv1",)):
            W[k] = W[k].copy()
            W[k][rng.permutation(128)[:64]] -= np.float32(12.0)
    return W


def weight_set(name, layout):
    """he / sb2 / dead: bcfit_ref's actor with a value branch of the same kind and a logstd; v0: the golden shared-trunk archive;
    zip: the golden tower archive sb2_ppo2_docking_621_h_30M.zip"""
    key = ("w", name, layout)
    if key not in _cache:
        towers = layout == "towers"
        if name == "v0":
            assert not towers
            with np.load(os.path.join(GOLDEN, "policy_best_model_v0.npz"), allow_pickle=False) as z:
                W = {k: np.ascontiguousarray(z[k], np.float32).reshape(SHAPES[k]) for k in KEYS_SHARED}
        elif name == "zip":
            assert towers
            from quadsim_amd.sb2 import read_sb2_weights
            lay, Z = read_sb2_weights(os.path.join(GOLDEN, "sb2_ppo2_docking_621_h_30M.zip"))
            assert lay == "towers"
            W = {k: np.ascontiguousarray(Z[k], np.float32).reshape(SHAPES[k]) for k in KEYS_TOWERS}
        else:
            rng = np.random.default_rng({"he": 131, "sb2": 132, "dead": 133}[name] + (10 if towers else 0))
            W = dict(br.weight_set(name))
            W.update(_value_branch(rng, towers, name))
            W["logstd"] = np.zeros(4, np.float32) if name == "sb2" else np.array([-0.3, 0.1, -0.5, 0.0], np.float32)
        _cache[key] = W
    return _cache[key]


def perturbed(W, seed=141):
    """the behaviour policy of the roll-out: the heads' weights and logstd moved so that ratios and value differences fall on both
    sides of both clip ranges"""
    rng = np.random.default_rng(seed)
    P = {k: np.asarray(v, np.float32).copy() for k, v in W.items()}
    sig = np.exp(P["logstd"].astype(np.float64))
    P["b2"] = (P["b2"] + 0.45 * sig * rng.standard_normal(4)).astype(np.float32)
    P["logstd"] = (P["logstd"] + 0.12 * rng.standard_normal(4)).astype(np.float32)
    P["bv2"] = (P["bv2"] + 0.05).astype(np.float32)
    return P


DRAWN_ROWS, ROLLOUT_SEED = 800, 151


def _draw_rollout(W, seed, n):
    P = perturbed(W)
    rng = np.random.default_rng(seed)
    obs = dr.sample_obs(n, seed=seed + 1)
    Fp, Fv = forward64(P, {"obs": obs})
    sig = np.exp(P["logstd"].astype(np.float64))
    act = (Fp["y"] + sig * rng.standard_normal((n, 4))).astype(np.float32)
    z = (act.astype(np.float64) - Fp["y"]) / sig
    nl = 0.5 * (z ** 2).sum(-1) + 2.0 * LOG2PI + P["logstd"].astype(np.float64).sum()
    v = Fv["y"][:, 0]
    scale = max(1.0, float(np.abs(v).mean()))
    values = (v + 0.35 * rng.standard_normal(n)).astype(np.float32)
    returns = (values + 0.6 * scale * rng.standard_normal(n)).astype(np.float32)
    return {"obs": obs, "actions": act, "returns": returns, "values": values, "neglogp": nl.astype(np.float32)}


def rollout(name, layout):
    """300 rows of what Runner.run() returns, float32: obs (docking observations), actions sampled from the PERTURBED policy with
    its neglogp, values of the perturbed value branch plus a spread, returns = values + noise.  HOW THE ROWS ARE CHOSEN: 800 rows
    are drawn, and the roll-out is the first 300 of them at which the float64 reference alone finds no row-wise edge (edge_rows:
    a pre-activation, the ratio or the value step within its bound of a decision) in either setting -- with bounds of 1e-3 of
    a ratio, 300 drawn rows hold about five such rows whatever the seed.  Every comparison then uses all rows of its minibatch"""
    key = ("roll", name, layout)
    if key not in _cache:
        W = weight_set(name, layout)
        data = _draw_rollout(W, ROLLOUT_SEED, DRAWN_ROWS)
        bad = np.zeros(DRAWN_ROWS, bool)
        for hp in HPS.values():
            for k, mask in edge_rows(W, data, hp)[0].items():
                if k != "advantage at zero":
                    bad |= mask
        keep = np.flatnonzero(~bad)[:N_ROWS]
        assert keep.size == N_ROWS, "%s %s: %d of %d drawn rows are edge rows" % (name, layout, int(bad.sum()), DRAWN_ROWS)
        _cache[key] = {k: np.ascontiguousarray(v[keep]) for k, v in data.items()}
        _cache[key + ("dropped",)] = int(bad[:keep[-1] + 1].sum())
    return _cache[key]


def minibatch(data, rows):
    return {k: v[rows] for k, v in data.items()}


def _pools(W, data, hp):
    """the rows of each head class judged on the whole roll-out, the advantage's sign with a margin of 0.3 standard deviations"""
    _, H = edge_counts(W, data, hp)
    d = (data["returns"] - data["values"]).astype(np.float64)
    up, dn = d > d.mean() + 0.3 * d.std(), d < d.mean() - 0.3 * d.std()
    r = H["r"]
    pools = [up & (r > H["hi"]), dn & (r < H["lo"]), up & (r < H["lo"]), dn & (r > H["hi"])]
    if hp["cliprange_vf"] >= 0:
        pools.append(H["val_clipped"] & ~H["val_active"])
    return [np.flatnonzero(p) for p in pools]


def step_rows(name, layout, batch, hpname="vclip"):
    """the rows [batch] of the GPU tests' minibatches, without repetition: from 15 rows on three of every head class of the
    setting first (drawn from the classes judged on the whole roll-out), then a drawn rest; the first seed from 171 on at which
    edge_counts finds no edge row IN THIS MINIBATCH (the advantage depends on it) and every head class has at least three rows.
    tests/test_ppo2_cpu.py holds both for every fixture.  batch == N_ROWS: every row once"""
    key = ("rows", name, layout, batch, hpname)
    if key in _cache:
        return _cache[key]
    W, data, hp = weight_set(name, layout), rollout(name, layout), HPS[hpname]
    pools = _pools(W, data, hp) if batch >= 15 else []
    for s in range(171, 571):
        rng = np.random.default_rng(s * 1000 + batch)
        first = []
        for p in pools:
            p = np.setdiff1d(p, first)
            first += list(rng.permutation(p)[:3])
        rest = rng.permutation(np.setdiff1d(np.arange(N_ROWS), first))[:max(batch - len(first), 0)]
        rows = rng.permutation(np.concatenate([np.asarray(first, np.int64), rest])[:batch]).astype(np.int32)
        edges, H = edge_counts(W, minibatch(data, rows), hp)
        if any(edges.values()):
            continue
        if batch >= 15:
            cls = head_classes(H)
            need = [k for k in cls if hp["cliprange_vf"] >= 0 or not k.startswith("value clipped")]
            if min(int(cls[k].sum()) for k in need) < 3:
                continue
        _cache[key] = rows
        return rows
    raise AssertionError("no seed gives an edge-free minibatch with every head class: %s %s batch %d %s" % (name, layout, batch, hpname))


def zero_state(W):
    return {k: np.zeros(SHAPES[k], np.float32) for k in keys_of(W)}


def moments(W, seed=181):
    """non-zero starting moments: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {k: (1e-2 * rng.standard_normal(SHAPES[k])).astype(np.float32) for k in keys_of(W)}
    V = {k: (1e-4 * rng.random(SHAPES[k])).astype(np.float32) for k in keys_of(W)}
    return M, V


LEARN_STEPS, LEARN_LR = 20, 1.0e-3


def learn64(name="he", layout="shared", batch=64):
    """"it learns": LEARN_STEPS steps of update64 on ONE fixed minibatch (step_rows), from zero moments, value clipping on,
    max_grad_norm 0.5 -> the statistics [LEARN_STEPS, 6] of the float64 reference itself"""
    key = ("learn", name, layout, batch)
    if key not in _cache:
        W0, data = weight_set(name, layout), rollout(name, layout)
        mb = minibatch(data, step_rows(name, layout, batch))
        hp = dict(HP_VCLIP, lr=LEARN_LR, max_grad_norm=0.5)
        W = {k: np.asarray(W0[k], np.float64) for k in keys_of(W0)}
        M = {k: np.zeros(SHAPES[k]) for k in W}
        V = {k: np.zeros(SHAPES[k]) for k in W}
        stats = []
        for s in range(LEARN_STEPS):
            st, G = backward64(W, mb, hp)
            stats.append(st)
            W, M, V, _, _ = update64(W, M, V, G, hp, s + 1)
        _cache[key] = np.asarray(stats)
    return _cache[key]
