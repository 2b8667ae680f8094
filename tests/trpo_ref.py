"""Float64 restatement of TRPO on the device (quadsim_amd.trpo, include/quadsim_trpo.h) and the derived error bounds of its
float32 gradient, Fisher-vector product, line-search statistics and value fit, plus a REPLAY of the solver's algebra in the
contract's own arithmetic.  A helper module, not a test; numpy only.  Modelled on tests/ppo2_ref.py, whose advantage normalisation
(adv_norm64), back-propagation bound (_branch_backward) and Adam bounds it uses as they are, and on tests/bcfit_ref.py, whose forward
pass it restates with running error bounds (forward_net).

What is restated: the surrogate mean(A exp(nlp_old - neglogp)) + entcoeff entropy and its gradient (grad64), the Fisher-vector
product as J^T diag(1 / sigma^2) J v / n_f + 2 v on logstd (fvp64; tests/test_trpo_cpu.py holds it to torch's double backprop of
the mean KL), SB2's cg, step and line search (step64), the candidates' statistics at a given float32 theta (ls_eval64) and the
value fit's loss, gradient and Adam step (vf_backward64).  theta is the flat vector of the header: w0 | b0 | w1 | b1 | w2 | b2 |
logstd.

The replay (replay_cg): given the z vectors the device traced, alpha, mu, x, r, p, shs, lm and fullstep are computed as the header
states them -- an exact float32 fma (tests/mppi_ref.py's fma32) and DOT's float64 tree -- so the solver is pinned bit for bit
without a tolerance that would depend on the condition number of F.

The bounds.  u = 2^-24, gamma_k = k u / (1 - k u); E_x bounds |computed x - x|; inputs (rows, weights, v) enter exactly; expf is
1 ulp (e_x = 2u); sigma^ = expf(logstd) has relative error e_x.
  forward      per layer E = E_prev |W| + u sum_k (|s_k| + E_prev |W|) (1 + 2 K u), s_k the partial sums of the fma chain from the bias:
               each step rounds once, |error| <= u |s_k| (a running bound; unit-normal observations through He-scaled layers make
               the a-priori gamma_K sum |w a| ten times wider, which no line-search fixture's margin would survive)
  gradient     A, z, q as tests/ppo2_ref.py.  dn = fl(A fl(1 / n)): E_dn = (E_A + 2u (|A| + E_A)) / n.  dmean = fl(fl(dn z) / sigma^):
               ((E_dn |z| + |dn| E_z + E_dn E_z) / sigma + |dmean| (2u + e_x)) (1 + 8u).  dlogstd row fma(fl(z z), dn, -dn):
               E_dn (1 + z^2 + E_zz) + |dn| E_zz, then u.  Back-propagation and the sums over rows: _branch_backward's (gamma_{n+4}
               covers any cut into slices and the one rounding of the float64 sum).  logstd: the rounding of entcoeff, the rows'
               bounds and gamma_{n+5} of the magnitudes.  surr_before: mean E_A.  |g|: the norm of the bounds.
  tangent      t0: an fma chain of 12 products and the bias on exact inputs: gamma_{14} (|x| |V0| + |vb0|) under the mask.
               t1: a chain of 256: E_h0 |V1| + E_t0 |W1| + gamma_{258} ((|h0| + E_h0) |V1| + (|t0| + E_t0) |W1| + |vb1|).
               tmu likewise from (h1, t1).  dmu = fl(fl(tmu / fl(sigma^ sigma^)) fl(1 / n_f)): the denominator has relative error
               2 e_x + u, then three roundings: (E_tmu + |tmu| (2 e_x + 4u)) / (sigma^2 n_f) (1 + 8u).
  F v          _branch_backward from (dmu, E_dmu) over the n_f rows; logstd elements are 2 v exactly.  z = fma(float32(damping), v,
               Fv): E_Fv + |float32(damping) - damping| |v| + u |z|.  GIVEN the same ReLU masks as float64 (the fixtures' rows are
               drawn so that no pre-activation lies within its bound of zero).
  candidates   theta_k is float32 and enters exactly.  neglogp_k and the OLD neglogp the device kept each carry ppo2_ref's E_nl;
               dn = fl(nlp_old^ - nl^): both, then u; r = expf(dn): r expm1(E_dn) + e_x r exp(E_dn); fl(A r) as ppo2_ref.
               KL row: c = fl(ls_k - ls_old): u |c|;  d = fl(mu_old^ - mu_k^): E_mu_old + E_mu_k, then u;  fl(sigma_old^2):
               sigma_old^2 (2 e_x + u);  num = fma(d, d, .): 2 |d| E_d + E_d^2 + E_so2, then u;  den = fl(2 fl(sigma_k^2)): relative
               rho = 2 e_x + u;  t = fl(num / den): (E_num / den + t rho) / (1 - rho), then u;  fl(fl(c + t) - 0.5): two roundings;
               four terms added: gamma_4.  The means over rows are float64: the rows' bounds averaged, then 2u of the result.
  value fit    e = fl(v^ - R): E_v + u (|e| + E_v); dv = fl(e fl(2 / B)); loss: sum (2 |e| E_e + E_e^2) / B + gamma_{B+3};
               gradients: _branch_backward; Adam: adam_bound at the reference's gradient plus adam_input_bound of the gradient's bound.
plus TINY per result for the subnormal range.  Nothing is fitted to device output.
"""
import numpy as np

import bcfit_ref as br
import mppi_ref as mr
import ppo2_ref as pr

U32, TINY, gamma, E_X = pr.U32, pr.TINY, pr.gamma, pr.E_X
fma32 = mr.fma32
LOG2PI = pr.LOG2PI
POLICY_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2", "logstd")
VALUE_KEYS = ("wv0", "bv0", "wv1", "bv1", "wv2", "bv2")
SHAPES = pr.SHAPES
SIZES = [int(np.prod(SHAPES[k])) for k in POLICY_KEYS]
STARTS = np.concatenate([[0], np.cumsum(SIZES)])
P = int(STARTS[-1])
LS0 = int(STARTS[6])
VF_BETA1, VF_BETA2, VF_EPS = 0.9, 0.999, 1.0e-8
STAT_NAMES = ("surr_before", "surr_after", "kl_after", "entropy", "grad_norm", "shs", "lm", "expected_improve", "accepted", "cg_iters_run")
assert P == 18696


def flatten(W, dtype=None):
    v = np.concatenate([np.asarray(W[k]).reshape(-1) for k in POLICY_KEYS])
    return v if dtype is None else v.astype(dtype)


def unflatten(theta):
    return {k: np.asarray(theta[STARTS[i]:STARTS[i + 1]]).reshape(SHAPES[k]) for i, k in enumerate(POLICY_KEYS)}


def policy_net(W):
    return {k: W[k] for k in br.KEYS}


def value_net(W):
    return dict(zip(br.KEYS, (W[k] for k in VALUE_KEYS)))


def forward_net(net, obs):
    """bcfit_ref.forward64's pass over a 12 -> 128 -> 128 -> out net (its keys) with RUNNING error bounds: a chain
    s_k = fl(s_{k-1} + w_k a_k) from the bias errs by at most u |s_k| per step, so E = E_prev |W| + u sum_k (|s_k| + E_prev |W|) (1 + 2 K u)
    with the float64 partial sums s_k -- the a-priori gamma_K sum |w a| without its factor K on terms of mixed sign"""
    f = np.float64
    x = np.asarray(obs, f)
    F = {"x": x}
    h, E = x, np.zeros_like(x)
    for l in range(3):
        w, b = np.asarray(net["w%d" % l], f), np.asarray(net["b%d" % l], f)
        K = w.shape[0]
        part = np.abs(np.cumsum(h[:, :, None] * w[None], axis=1) + b).sum(1)
        prop = E @ np.abs(w)
        E = prop + U32 * (part + K * prop) * (1 + 2 * K * U32) + TINY
        z = h @ w + b
        if l < 2:
            F["z%d" % l], F["E_z%d" % l] = z, E
            h = np.maximum(z, 0.0)
            F["a%d" % l] = h
        else:
            F["y"], F["E_y"] = z, E
    return F


def forward(W, obs):
    """the policy tower's forward pass (y: the means)"""
    return forward_net(policy_net(W), obs)


def relu_edges(W, obs):
    """per row: a hidden pre-activation of either tower within its forward bound of zero"""
    out = np.zeros(np.asarray(obs).shape[0], bool)
    for net, outs in ((policy_net(W), 4), (value_net(W), 1)):
        F = forward_net(net, obs)
        for l in (0, 1):
            out |= (np.abs(F["z%d" % l]) <= 4.0 * F["E_z%d" % l]).any(-1)
    return out


def _head(W, F, actions):
    """z, neglogp and their bounds from a forward pass (tests/ppo2_ref.py's head64, the part both passes share)"""
    f = np.float64
    a = np.asarray(actions, f)
    ls = np.asarray(W["logstd"], f)
    sig = np.exp(ls)
    mean, E_mean = F["y"], F["E_y"]
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
    return dict(sig=sig, z=z, E_z=E_z, nl=nl, E_nl=E_nl, ent=ls.sum() + 2.0 * (LOG2PI + 1.0))


def grad64(W, data, entcoeff=0.0, with_bound=False):
    """-> dict(g [P], surr_before, entropy, norm, mu_old, nlp_old, A) in float64; with_bound also E_g, E_surr, E_norm, E_A, E_mu, E_nl"""
    f = np.float64
    n = np.asarray(data["obs"]).shape[0]
    F = forward(W, data["obs"])
    H = _head(W, F, data["actions"])
    A, E_A = pr.adv_norm64(data["returns"], data["values"], with_bound=True)
    sig, z, E_z = H["sig"], H["z"], H["E_z"]
    dn = A / n
    E_dn = (E_A + 2 * U32 * (np.abs(A) + E_A)) / n + TINY
    dmean = dn[:, None] * z / sig
    E_dmean = ((E_dn[:, None] * np.abs(z) + np.abs(dn)[:, None] * E_z + E_dn[:, None] * E_z) / sig + np.abs(dmean) * (2 * U32 + E_X)) * (1 + 8 * U32) + TINY
    zz = z ** 2
    E_zz = 2 * np.abs(z) * E_z + E_z ** 2
    E_zz = E_zz + U32 * (zz + E_zz) + TINY
    dls = dn[:, None] * (zz - 1.0)
    E_dls = E_dn[:, None] * (1.0 + zz + E_zz) + np.abs(dn)[:, None] * E_zz
    E_dls = E_dls + U32 * (np.abs(dls) + E_dls) + TINY
    G, E = pr._branch_backward(policy_net(W), F, dmean, E_dmean, n)
    e32 = f(np.float32(entcoeff))
    G["logstd"] = dls.sum(0) + entcoeff
    E["logstd"] = abs(e32 - entcoeff) + E_dls.sum(0) + gamma(n + 5) * (abs(e32) + (np.abs(dls) + E_dls).sum(0)) + TINY
    g, E_g = flatten(G, f), flatten(E, f)
    surr = A.mean() + entcoeff * H["ent"]
    out = dict(g=g, surr_before=surr, entropy=H["ent"], norm=np.sqrt((g ** 2).sum()), mu_old=F["y"], nlp_old=H["nl"], A=A)
    if with_bound:
        E_norm = np.sqrt((E_g ** 2).sum())
        out.update(E_g=E_g, E_surr=E_A.mean() + 2 * U32 * (abs(surr) + E_A.mean()) + TINY,
                   E_norm=E_norm + 2 * U32 * (out["norm"] + E_norm) + TINY, E_A=E_A, E_mu=F["E_y"], E_nl=H["E_nl"])
    return out


def fvp64(W, obs, stride, v, damping=0.0, with_bound=False):
    """(F + damping) v over the rows 0, stride, .. of obs, v [P] (float32 values) -> z [P] float64; with_bound: (z, E_z)"""
    f = np.float64
    x = np.asarray(obs)[::stride]
    nf = x.shape[0]
    F = forward(W, x)
    V = {k: np.asarray(a, f) for k, a in unflatten(np.asarray(v, f)).items()}
    w1, w2 = np.asarray(W["w1"], f), np.asarray(W["w2"], f)
    sig2 = np.exp(2.0 * np.asarray(W["logstd"], f))
    # (the masks: where a pre-activation lies within its forward bound of zero the device may take either side of the ReLU, in the
    # activation, in the tangent and in the back-propagation alike: ppo2_ref._masked's bound covers both.  The fixtures have none)
    m0, m1 = F["z0"] > 0.0, F["z1"] > 0.0
    edge0, edge1 = np.abs(F["z0"]) <= F["E_z0"], np.abs(F["z1"]) <= F["E_z1"]
    h0, h1, E_h0, E_h1 = F["a0"], F["a1"], F["E_z0"] * (m0 | edge0), F["E_z1"] * (m1 | edge1)
    xa = np.abs(F["x"])
    t0, E_t0 = pr._masked(F["x"] @ V["w0"] + V["b0"], gamma(14) * (xa @ np.abs(V["w0"]) + np.abs(V["b0"])) + TINY, F["z0"], F["E_z0"])
    t1, E_t1 = pr._masked(h0 @ V["w1"] + t0 @ w1 + V["b1"],
                          E_h0 @ np.abs(V["w1"]) + E_t0 @ np.abs(w1)
                          + gamma(258) * ((h0 + E_h0) @ np.abs(V["w1"]) + (np.abs(t0) + E_t0) @ np.abs(w1) + np.abs(V["b1"])) + TINY,
                          F["z1"], F["E_z1"])
    tmu = h1 @ V["w2"] + t1 @ w2 + V["b2"]
    E_tmu = (E_h1 @ np.abs(V["w2"]) + E_t1 @ np.abs(w2)
             + gamma(258) * ((h1 + E_h1) @ np.abs(V["w2"]) + (np.abs(t1) + E_t1) @ np.abs(w2) + np.abs(V["b2"])) + TINY)
    dmu = tmu / sig2 / nf
    E_dmu = (E_tmu + np.abs(tmu) * (2 * E_X + 4 * U32)) / (sig2 * nf) * (1 + 8 * U32) + TINY
    G, E = pr._branch_backward(policy_net(W), F, dmu, E_dmu, nf)
    G["logstd"], E["logstd"] = 2.0 * V["logstd"], np.full(4, TINY)
    Fv, E_Fv = flatten(G, f), flatten(E, f)
    vv = np.asarray(v, f)
    z = Fv + damping * vv
    if not with_bound:
        return z
    return z, E_Fv + abs(f(np.float32(damping)) - damping) * np.abs(vv) + U32 * (np.abs(z) + E_Fv) + TINY


def ls_eval64(W_old, theta_k, data, entcoeff=0.0, with_bound=False):
    """the surrogate and the mean KL of the candidate theta_k [P] (float32 values) against the old policy W_old -> (surr, kl) in
    float64; with_bound: (surr, kl, E_surr, E_kl)"""
    f = np.float64
    Wk = unflatten(np.asarray(theta_k, f))
    Fo, Fk = forward(W_old, data["obs"]), forward(Wk, data["obs"])
    Ho, Hk = _head(W_old, Fo, data["actions"]), _head(Wk, Fk, data["actions"])
    A, E_A = pr.adv_norm64(data["returns"], data["values"], with_bound=True)
    dn = Ho["nl"] - Hk["nl"]
    E_dn = Ho["E_nl"] + Hk["E_nl"]
    E_dn = E_dn + U32 * (np.abs(dn) + E_dn) + TINY
    r = np.exp(dn)
    E_r = r * np.expm1(E_dn) + E_X * r * np.exp(E_dn) + TINY
    Ar = A * r
    E_Ar = np.abs(A) * E_r + r * E_A + E_A * E_r
    E_Ar = E_Ar + U32 * (np.abs(Ar) + E_Ar) + TINY
    surr = Ar.mean() + entcoeff * Hk["ent"]
    lso, lsk = np.asarray(W_old["logstd"], f), np.asarray(Wk["logstd"], f)
    c = lsk - lso
    E_c = U32 * np.abs(c)
    d = Fo["y"] - Fk["y"]
    E_d = Fo["E_y"] + Fk["E_y"]
    E_d = E_d + U32 * (np.abs(d) + E_d) + TINY
    so2, sk2 = np.exp(2.0 * lso), np.exp(2.0 * lsk)
    rho = 2 * E_X + U32
    E_so2 = so2 * rho * (1 + 4 * U32)
    num = d * d + so2
    E_num = 2 * np.abs(d) * E_d + E_d ** 2 + E_so2
    E_num = E_num + U32 * (num + E_num) + TINY
    den = 2.0 * sk2
    t = num / den
    E_t = (E_num / den + t * rho) / (1.0 - rho)
    E_t = E_t + U32 * (t + E_t) + TINY
    s1 = c + t
    E_s1 = E_c + E_t
    E_s1 = E_s1 + U32 * (np.abs(s1) + E_s1) + TINY
    term = s1 - 0.5
    E_term = E_s1 + U32 * (np.abs(term) + E_s1) + TINY
    row = term.sum(-1)
    E_row = E_term.sum(-1) + gamma(4) * (np.abs(term) + E_term).sum(-1) + TINY
    kl = row.mean()
    if not with_bound:
        return surr, kl
    return (surr, kl, E_Ar.mean() + 2 * U32 * (abs(surr) + E_Ar.mean()) + TINY, E_row.mean() + 2 * U32 * (abs(kl) + E_row.mean()) + TINY)


def step64(W, data, max_kl=0.01, cg_iters=10, cg_damping=1e-2, entcoeff=0.0, backtracks=10, fvp_stride=5, residual_tol=1e-10):
    """one TRPO policy step in float64 throughout -> dict(accepted, stats [10], theta [P] after, cands: per evaluated candidate
    (surr, kl, E_surr, E_kl), G: grad64's dict with bounds, iters, fullstep)"""
    G = grad64(W, data, entcoeff, with_bound=True)
    g = G["g"]
    th0 = flatten(W, np.float64)
    stats = np.zeros(10)
    stats[[0, 1, 3, 4, 8]] = G["surr_before"], G["surr_before"], G["entropy"], G["norm"], -2.0
    out = dict(accepted=-2, stats=stats, theta=th0, cands=[], G=G, iters=0, fullstep=None)
    rdotr = g @ g
    if rdotr == 0.0:
        return out
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    for it in range(cg_iters):
        z = fvp64(W, data["obs"], fvp_stride, p, cg_damping)
        a = rdotr / (p @ z)
        x, r = x + a * p, r - a * z
        new = r @ r
        p, rdotr = r + (new / rdotr) * p, new
        out["iters"] = it + 1
        if rdotr < residual_tol:
            break
    shs = 0.5 * (x @ fvp64(W, data["obs"], fvp_stride, x, cg_damping))
    lm = np.sqrt(shs / max_kl)
    fs = x / lm
    out["fullstep"] = fs
    stats[5:10] = shs, lm, g @ fs, -1.0, out["iters"]
    out["accepted"] = -1
    for k in range(backtracks):
        th = th0 + fs * 0.5 ** k
        surr, kl, E_s, E_k = ls_eval64(W, th, data, entcoeff, with_bound=True)
        out["cands"].append((surr, kl, E_s, E_k))
        if np.isfinite(surr) and np.isfinite(kl) and kl <= 1.5 * max_kl and surr - G["surr_before"] >= 0.0:
            out["accepted"], out["theta"] = k, th
            stats[1], stats[2], stats[8] = surr, kl, k
            stats[3] = th[LS0:].sum() + 2.0 * (LOG2PI + 1.0)
            break
    return out


# ---------------------------------------------------------------------------------------------------- the replay
def dot_tree(a, b):
    """DOT of the header on float32 arrays [P] -> float64"""
    pr_ = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    blocks = -(-pr_.size // 256)
    t = np.zeros(blocks * 256)
    t[:pr_.size] = pr_
    t = t.reshape(blocks, 256)
    h = 128
    while h > 0:
        t[:, :h] = t[:, :h] + t[:, h:2 * h]
        h >>= 1
    total = 0.0
    for s in t[:, 0]:
        total = total + s
    return total


def replay_cg(g, zs, z_last, cg_iters, max_kl, residual_tol=1e-10):
    """steps 4 and 5 of the header from the traced products: g [P] float32, zs [cg_iters, P] the z of every iteration (rows of
    iterations that did not run are not read), z_last [P] the product on x -> dict(x, fullstep float32; p: the vector handed to
    every product that ran and to the last one; cg [iters, 4] float64 (DOT(p, z), alpha, rdotr', mu); rdotr0, shs, lm,
    expected_improve, iters)"""
    f32 = np.float32
    g = np.asarray(g, f32)
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rdotr = dot_tree(g, g)
    out = dict(rdotr0=rdotr, p=[], cg=[], iters=0)
    for k in range(cg_iters):
        z = np.asarray(zs[k], f32)
        out["p"].append(p.copy())
        pz = dot_tree(p, z)
        with np.errstate(all="ignore"):
            alpha = f32(rdotr / pz)
        x = fma32(alpha, p, x)
        r = fma32(-alpha, z, r)
        new = dot_tree(r, r)
        with np.errstate(all="ignore"):
            mu = f32(new / rdotr)
        p = fma32(mu, p, r)
        out["cg"].append((pz, float(alpha), new, float(mu)))
        rdotr, out["iters"] = new, k + 1
        if rdotr < residual_tol:
            break
    with np.errstate(all="ignore"):
        shs = 0.5 * dot_tree(x, np.asarray(z_last, f32))
        lm = f32(np.sqrt(shs / max_kl))
        fs = (x / lm).astype(f32)
    out.update(x=x, fullstep=fs, shs=shs, lm=lm, expected_improve=dot_tree(g, fs), cg=np.asarray(out["cg"], np.float64).reshape(-1, 4))
    return out


def candidate32(theta_old, fullstep, k):
    """theta_k of the header: float32(theta_old + float32(fullstep 2^-k))"""
    return (np.asarray(theta_old, np.float32) + np.asarray(fullstep, np.float32) * np.float32(0.5 ** k)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the value fit
def vf_backward64(W, obs, ret, with_bound=False):
    """mean((v - R)^2) of the value tower over the rows -> (loss, {VALUE_KEYS: gradient}); with_bound: also the loss's bound and
    {key: bound}"""
    f = np.float64
    net = value_net(W)
    B = np.asarray(obs).shape[0]
    F = forward_net(net, obs)
    v, E_v = F["y"][:, 0], F["E_y"][:, 0]
    e = v - np.asarray(ret, f)
    E_e = E_v + U32 * (np.abs(e) + E_v) + TINY
    c = 2.0 / B
    dv = e * c
    E_dv = c * (E_e + 2 * U32 * (np.abs(e) + E_e)) * (1 + 4 * U32) + TINY
    Gb, Eb = pr._branch_backward(net, F, dv[:, None], E_dv[:, None], B)
    G = {k: Gb[b] for k, b in zip(VALUE_KEYS, br.KEYS)}
    loss = np.mean(e ** 2)
    if not with_bound:
        return loss, G
    sq = np.sum(2 * np.abs(e) * E_e + E_e ** 2) / B
    return loss, G, sq + gamma(B + 3) * (loss + sq) + TINY, {k: Eb[b] for k, b in zip(VALUE_KEYS, br.KEYS)}


def vf_update_bound(W, M, V, G, E_G, t, lr, beta1=VF_BETA1, beta2=VF_BETA2, eps=VF_EPS):
    """bounds of the device's (w, m, v) after one step against adam64 at the reference's gradient G whose device value lies within E_G"""
    out = {}
    for k in VALUE_KEYS:
        Ew, Em, Ev = pr.adam_bound(W[k], M[k], V[k], G[k], t, lr, beta1, beta2, eps)
        dw, dm, dv = pr.adam_input_bound(M[k], V[k], G[k], E_G[k], t, lr, beta1, beta2, eps)
        out[k] = ((Ew + dw) * (1 + 8 * U32), (Em + dm) * (1 + 8 * U32), (Ev + dv) * (1 + 8 * U32))
    return out


# ---------------------------------------------------------------------------------------------------- the shared fixtures
N_ROWS = 301
_cache = {}
# n, fvp_stride, weight scale, max_kl, backtracks, the roll-out's seed, the accepted k of the float64 reference (-1: none).  The seed of
# "small" is the first from 211 on at which the first candidate is rejected for a negative improvement, the next four for their KL
# and every margin of the census (tests/test_trpo_cpu.py) holds.  "stride": every one of 400 seeds gives k = 2 here (KL 0.11, 0.03,
# 0.008): sixty rows underestimate the curvature of 18 696 parameters by more than the factor four of one halving
LS_FIXTURES = {"full": (300, 1, 1.0, 0.01, 10, 211, 0), "stride": (300, 5, 1.0, 0.01, 10, 211, 2), "small": (17, 5, 1.0, 0.01, 10, 263, 5),
               "none": (300, 5, 1.0, 8.0, 1, 211, -1), "scaled": (300, 5, 0.3, 0.01, 10, 211, 0)}
SEED = 211


def weights(scale=1.0):
    """He-scaled towers (tests/ppo2_ref.py's "he" towers set) with every tensor but logstd times `scale`"""
    key = ("w", scale)
    if key not in _cache:
        W = pr.weight_set("he", "towers")
        _cache[key] = {k: (np.asarray(W[k], np.float32) if k == "logstd" else (np.asarray(W[k], np.float64) * scale).astype(np.float32))
                       for k in pr.KEYS_TOWERS}
    return _cache[key]


def rollout(scale=1.0, seed=SEED):
    """N_ROWS rows: unit-normal observations, actions drawn from the policy itself, values of the value tower plus a spread, random
    returns; of 2 N_ROWS drawn rows the first N_ROWS at which no hidden pre-activation of either tower lies within four times its
    bound of zero.  The tests take the first n rows."""
    key = ("r", scale, seed)
    if key not in _cache:
        W = weights(scale)
        rng = np.random.default_rng(seed)
        m = 2 * N_ROWS
        obs = rng.standard_normal((m, 12)).astype(np.float32)
        keep = np.flatnonzero(~relu_edges(W, obs))[:N_ROWS]
        assert keep.size == N_ROWS
        obs = np.ascontiguousarray(obs[keep])
        F = forward(W, obs)
        sig = np.exp(np.asarray(W["logstd"], np.float64))
        act = (F["y"] + sig * rng.standard_normal((N_ROWS, 4))).astype(np.float32)
        v = forward_net(value_net(W), obs)["y"][:, 0]
        values = (v + 0.3 * rng.standard_normal(N_ROWS)).astype(np.float32)
        returns = (values + rng.standard_normal(N_ROWS)).astype(np.float32)
        _cache[key] = {"obs": obs, "actions": act, "returns": returns, "values": values}
    return _cache[key]


def head(data, n):
    return {k: np.ascontiguousarray(v[:n]) for k, v in data.items()}


def ls_fixture(name):
    """-> (W, data, hyper-parameters, the float64 reference's step64) of a line-search fixture"""
    key = ("ls", name)
    if key not in _cache:
        n, stride, scale, max_kl, backtracks, seed, _ = LS_FIXTURES[name]
        W, data = weights(scale), head(rollout(scale, seed), n)
        hp = dict(max_kl=max_kl, cg_iters=10, cg_damping=1e-2, entcoeff=0.0, backtracks=backtracks, fvp_stride=stride)
        _cache[key] = (W, data, hp, step64(W, data, **hp))
    return _cache[key]


def moments(seed=281):
    """non-zero starting moments of the value tower: m of the gradient's typical size, v >= 0"""
    rng = np.random.default_rng(seed)
    M = {k: (1e-2 * rng.standard_normal(SHAPES[k])).astype(np.float32) for k in VALUE_KEYS}
    V = {k: (1e-4 * rng.random(SHAPES[k])).astype(np.float32) for k in VALUE_KEYS}
    return M, V
