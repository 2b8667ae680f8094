"""The hyper-parameter cases of the seven trainers on the device: one table per trainer, the one-step fixtures they run on and the
float64 references' own run of a case.  A helper module, not a test; numpy only.

Every other GPU test of the trainers runs at ONE point of hyper-parameter space: Adam's betas and eps at the module constants,
actor_lr == critic_lr, gamma 0.99, tau the default or 1.  A row here moves one hyper-parameter (or one pair) away from that point:

  row["hyper"]   the overrides of the case on DEFAULTS[trainer]
  row["twin"]    the overrides of the setting the case must be told apart from ({}: the defaults; for a pair of rates: the swap)
  row["about"]   the quantity the case is about: "w" every trained tensor after the step, "w:PREFIX" those whose label starts so,
                 "g" / "g:PREFIX" the gradients, "stat:NAME" one statistic, "target" the target nets after the Polyak step
  row["fix"]     the fixture variant ("": the standard one; "shifted": target critics with b2 + SHIFT, for gamma and the smoothing)

tests/test_hyper_cases_cpu.py holds, without a GPU, that every row is accepted by the trainer's check_*_args, that the float64
reference at the case and at its twin differ in the row's quantity by at least SEPARATION of the reference's OWN bounds (the median
over a tensor's elements, the worst tensor) -- a device that ignored the hyper-parameter would be that far out -- and anchors the
references to the package's float64 torch paths at the cases.  tests/test_gpu_hyper.py runs every row on the device through the
sentinel-guarded runners of the tests/test_gpu_*.py modules.  No tolerance is introduced: every bound is step64's / backward64's,
adam_bound's, update_bound's or vf_update_bound's at the case's own arguments, the rest are bit-for-bit statements.

The fixtures are the one-step fixtures of the references: 17 rows (one full 16-row chunk and a one-row tail), non-zero moments,
Adam step t = T0 + 1 = 7 (TD3: the actor's own step 4).
"""
import numpy as np

import bcfit_ref as br
import ddpg_ref as dd
import dynfit_ref as fr
import dynplan_ref as dr
import gail_ref as gr
import nonfinite_cases as nc
import ppo2_ref as pr
import td3_ref as td
import trpo_ref as tr

f = np.float64
BATCH, T0 = 17, 6
TD3_ACTOR_T0 = 3
SEPARATION = 10.0
# chosen on the CPU (tests/test_hyper_cases_cpu.py::test_the_shift_and_the_tau_are_the_first_that_qualify): the first of 4, 8, 16 at
# which y_mean and the critic losses of DDPG and of TD3 at gamma 1 and at gamma 0.99 lie 10 bounds apart (4: 3.5, 8: 6.9 for TD3); the first two-digit decimal tau at which
# float32(1 - tau) is not float32(1) - float32(tau), so that forming 1 - tau in float32 would show
SHIFT = 16.0
SHIFT_CANDIDATES = (4.0, 8.0, 16.0)
TAU_CANDIDATES = tuple(k / 100.0 for k in range(1, 51))     # 0.01, 0.02, .. 0.5: the first that qualifies is 0.09


def tau_shows_float32_subtraction(tau):
    return np.float32(1.0 - tau) != np.float32(1.0) - np.float32(tau)


TAU_ODD = next(t for t in TAU_CANDIDATES if tau_shows_float32_subtraction(t))
T_EDGE = (10 ** 5, 2 ** 31 - 2)                     # the step counter's cases, as test_step_counter_at_its_upper_edge has them


def _row(cid, about, twin=None, fix="", **hyper):
    return dict(id=cid, hyper=hyper, twin=twin or {}, about=about, fix=fix)


def _adam_rows(lr_keys, more_eps=()):
    """the rows every trainer has: Adam's betas, eps and the rate(s)"""
    lr = lambda v: {k: v for k in lr_keys}           # noqa: E731
    rows = [_row("betas-0-0", "w", beta1=0.0, beta2=0.0), _row("betas-0.5-0.9", "w", beta1=0.5, beta2=0.9),
            _row("betas-0.99-0.9", "w", beta1=0.99, beta2=0.9), _row("beta1-0", "w", beta1=0.0), _row("beta2-0", "w", beta2=0.0),
            _row("eps-1e-3", "w", eps=1.0e-3)]
    rows += [_row("eps-%g" % e, "w", eps=e) for e in more_eps]
    rows += [_row("lr-0", "w", **lr(0.0)), _row("lr-negative", "w", **lr(-1.0e-2))]
    return rows


_SWAP = dict(actor_lr=1.0e-2, critic_lr=3.0e-3)
_RATES = [_row("actor-3e-3-critic-1e-2", "w", twin=_SWAP, actor_lr=3.0e-3, critic_lr=1.0e-2),
          _row("actor-1e-2-critic-3e-3", "w", twin=dict(actor_lr=3.0e-3, critic_lr=1.0e-2), **_SWAP),
          _row("actor-lr-0", "w:actor", actor_lr=0.0, critic_lr=1.0e-2)]
_GAMMAS = [_row("gamma-0", "stat:y_mean", fix="shifted", gamma=0.0), _row("gamma-0.5", "stat:y_mean", fix="shifted", gamma=0.5),
           _row("gamma-1", "stat:y_mean", fix="shifted", gamma=1.0)]
_TAUS = [_row("tau-0.5", "target", tau=0.5), _row("tau-1e-9", "target", tau=1.0e-9), _row("tau-%g" % TAU_ODD, "target", tau=TAU_ODD)]

DEFAULTS = {
    "td3": dict(nc.TD3_HYPER, beta1=td.BETA1, beta2=td.BETA2, eps=td.EPS),
    "ddpg": dict(nc.DDPG_HYPER, beta1=dd.BETA1, beta2=dd.BETA2, eps=dd.EPS),
    "dynfit": dict(lr=nc.DYNFIT_LR, beta1=fr.BETA1, beta2=fr.BETA2, eps=fr.EPS),
    "bc": dict(lr=nc.BC_LR, beta1=br.BETA1, beta2=br.BETA2, eps=br.EPS),
    "gail": dict(lr=nc.GAIL_LR, entcoeff=gr.ENTCOEFF, beta1=gr.BETA1, beta2=gr.BETA2, eps=gr.EPS),
    "ppo2": dict(pr.HP_VCLIP, beta1=pr.BETA1, beta2=pr.BETA2, eps=pr.EPS),
    "trpo_vf": dict(lr=nc.TRPO_VF_LR, beta1=tr.VF_BETA1, beta2=tr.VF_BETA2, eps=tr.VF_EPS),
}

# PPO2: with no clip the scale is float32(1) and m' of betas (0, 0) is the gradient itself, so that row runs unclipped
_PPO2 = [dict(r, hyper=dict(r["hyper"], max_grad_norm=0.0), twin=dict(max_grad_norm=0.0)) if r["id"] == "betas-0-0" else r
         for r in _adam_rows(("lr",), more_eps=(1.0e-8,))]
_PPO2 += [_row("max-grad-norm-0", "w", max_grad_norm=0.0), _row("max-grad-norm-negative", "w", max_grad_norm=-1.0),
          _row("max-grad-norm-1e6", "w", max_grad_norm=1.0e6), _row("vf-coef-0", "g:wv2", vf_coef=0.0), _row("cliprange-0", "stat:policy_loss", cliprange=0.0),
          _row("cliprange-10", "stat:clipfrac", cliprange=10.0), _row("cliprange-vf-0", "stat:value_loss", cliprange_vf=0.0)]

TABLES = {
    "td3": tuple(_adam_rows(("actor_lr", "critic_lr")) + _RATES + _GAMMAS + _TAUS),
    "ddpg": tuple(_adam_rows(("actor_lr", "critic_lr")) + _RATES + _GAMMAS + _TAUS),
    "dynfit": tuple(_adam_rows(("lr",))),
    "bc": tuple(_adam_rows(("lr",))),
    "gail": tuple(_adam_rows(("lr",)) + [_row("entcoeff-0.1", "g:w1", entcoeff=0.1)]),
    "ppo2": tuple(_PPO2),
    "trpo_vf": tuple(_adam_rows(("lr",))),
}
# Rows the float64 references canNOT tell from their twins by 10 of their own bounds (the measured separations are in
# profiles/hyper/README.md): they are no rows of the tables.  The device still runs them within the bounds, which holds that the
# setting itself works; that the setting is READ is held by bit-for-bit statements where there is one (TD3's smoothing)
EXTRA = {
    "td3": (_row("noise-clip-0", "g:q1", fix="shifted", target_noise_clip=0.0), _row("noise-4-clip-0.5", "g:q1", fix="shifted", target_policy_noise=4.0)),
    "gail": (_row("entcoeff-0", "g", entcoeff=0.0),),
    "ppo2": (_row("ent-coef-0", "g:logstd", ent_coef=0.0),),
}
PPO2_LAYOUTS = ("shared", "towers")
TD3_DELAY_EDGE = 1 << 16                            # the documented maximum of policy_delay


def ids(trainer):
    return [r["id"] for r in TABLES[trainer]]


def hyper_of(trainer, row, twin=False):
    return dict(DEFAULTS[trainer], **(row["twin"] if twin else row["hyper"]))


def adam_args(hp):
    return hp["beta1"], hp["beta2"], hp["eps"]


# ---------------------------------------------------------------------------------------------------- the fixtures
_cache = {}


def fixture(trainer, variant=""):
    """the one-step set-up of a trainer (cached, never changed).  ppo2: variant is the layout ("": shared)"""
    key = (trainer, variant)
    if key in _cache:
        return _cache[key]
    if trainer == "td3":
        M, V = td.moments()
        F = dict(P=td.nets_shifted(SHIFT) if variant == "shifted" else td.nets(), M=M, V=V, rp=td.replay(), idx=td.step_indices(BATCH),
                 z=td.noise(1, BATCH), t0=T0, actor_t0=TD3_ACTOR_T0)
    elif trainer == "ddpg":
        M, V = dd.moments()
        F = dict(P=dd.nets_shifted(SHIFT) if variant == "shifted" else dd.nets(), M=M, V=V, rp=dd.replay(), idx=dd.step_indices(BATCH), t0=T0)
    elif trainer == "dynfit":
        W = dr.weight_set(nc.DYNFIT_SET)
        M, V = fr.moments(W)
        x, d = fr.buffer()
        F = dict(W=W, M=M, V=V, x=x, d=d, idx=fr.step_indices(BATCH), t0=T0)
    elif trainer == "bc":
        M, V = br.moments()
        F = dict(W=br.weight_set(nc.BC_SET), M=M, V=V, data=br.dataset(), idx=br.step_rows(nc.BC_SET, BATCH), t0=T0)
    elif trainer == "gail":
        W = gr.weights(int(variant or nc.GAIL_HIDDEN))
        M, V = gr.moments(W)
        gen, exp, mean, rscale = gr.dataset()
        gi, ei = gr.step_indices(BATCH)
        F = dict(W=W, M=M, V=V, gen=gen, exp=exp, mean=mean, rscale=rscale, gi=gi, ei=ei, t0=T0)
    elif trainer == "ppo2":
        layout = variant or "shared"
        W = pr.weight_set(nc.PPO2_WEIGHTS, layout)
        M, V = pr.moments(W)
        F = dict(W=W, M=M, V=V, data=pr.rollout(nc.PPO2_WEIGHTS, layout), rows=pr.step_rows(nc.PPO2_WEIGHTS, layout, BATCH), layout=layout,
                 t0=T0)
    elif trainer == "trpo_vf":
        M, V = tr.moments()
        F = dict(W=tr.weights(), M=M, V=V, data=tr.rollout(), idx=nc.trpo_vf_indices(1), t0=T0)
    else:
        raise KeyError(trainer)
    _cache[key] = F
    return F


def fixture_of(trainer, row, variant=None):
    return fixture(trainer, row["fix"] if variant is None else variant)


def _nested(trainer):
    return trainer in ("td3", "ddpg")


def online(trainer):
    return {"td3": td.ONLINE, "ddpg": nc.DDPG_ONLINE}[trainer]


def tensors(trainer, F):
    """{label: (w, m, v)} float32, the trained tensors of the fixture"""
    if _nested(trainer):
        return {"%s/%s" % (n, k): (F["P"][n][k], F["M"][n][k], F["V"][n][k]) for n in online(trainer) for k in dd.KEYS}
    keys = {"dynfit": fr.GRAD_KEYS, "bc": br.KEYS, "gail": gr.KEYS, "trpo_vf": tr.VALUE_KEYS}.get(trainer) or pr.keys_of(F["W"])
    return {k: (F["W"][k], F["M"][k], F["V"][k]) for k in keys}


STAT_NAMES = {"td3": td.STAT_NAMES, "ddpg": dd.STAT_NAMES, "dynfit": ("loss",), "bc": ("loss",), "gail": gr.STAT_NAMES, "ppo2": pr.STAT_NAMES,
              "trpo_vf": ("loss",)}


def rows_of(F):
    return tuple(a[F["idx"][0]] for a in F["rp"])


def step64(trainer, F, hp, t0=None, actor_t0=None):
    """the float64 reference's step at the hyper-parameters -> dict(stats, Es: [n] float64, G, E: {label: array}, t, lr: {label:
    Adam's step and rate of the tensor})"""
    t0 = F["t0"] if t0 is None else t0
    if trainer == "td3":
        actor_t0 = F["actor_t0"] if actor_t0 is None else actor_t0
        act = td.actor_step(t0, hp["policy_delay"])
        st, G, _, Es, E = td.step64(F["P"], rows_of(F), F["z"][0], hp["gamma"], hp["target_policy_noise"], hp["target_noise_clip"], actor=act,
                                    with_bound=True)
        out = dict(stats=st, Es=Es, G={}, E={}, t={}, lr={})
        for n in G:
            for k in td.KEYS:
                lab = "%s/%s" % (n, k)
                out["G"][lab], out["E"][lab] = G[n][k], E[n][k]
                out["t"][lab], out["lr"][lab] = (actor_t0 + 1, hp["actor_lr"]) if n == "actor" else (t0 + 1, hp["critic_lr"])
        return out
    if trainer == "ddpg":
        st, G, _, Es, E = dd.step64(F["P"], rows_of(F), hp["gamma"], hp["obs_clip"], with_bound=True)
        out = dict(stats=st, Es=Es, G={}, E={}, t={}, lr={})
        for n in G:
            for k in dd.KEYS:
                lab = "%s/%s" % (n, k)
                out["G"][lab], out["E"][lab], out["t"][lab], out["lr"][lab] = G[n][k], E[n][k], t0 + 1, hp[n + "_lr"]
        return out
    if trainer == "dynfit":
        rows = F["idx"][0]
        loss, G, lb, E = fr.backward64(F["W"], F["x"][rows], F["d"][rows], with_bound=True)
        st, Es = np.array([loss]), np.array([lb])
    elif trainer == "bc":
        rows = F["idx"][0]
        loss, G, lb, E = br.backward64(F["W"], F["data"][0][rows], F["data"][1][rows], with_bound=True)
        st, Es = np.array([loss]), np.array([lb])
    elif trainer == "gail":
        g, e = F["gi"][0], F["ei"][0]
        st, G, Es, E = gr.backward64(F["W"], (F["gen"][0][g], F["gen"][1][g]), (F["exp"][0][e], F["exp"][1][e]), F["mean"], F["rscale"],
                                     hp["entcoeff"], with_bound=True)
    elif trainer == "ppo2":
        st, G, Es, E = pr.backward64(F["W"], pr.minibatch(F["data"], F["rows"]), hp, with_bound=True)
    elif trainer == "trpo_vf":
        rows = F["idx"][0]
        loss, G, lb, E = tr.vf_backward64(F["W"], F["data"]["obs"][rows], F["data"]["returns"][rows], with_bound=True)
        st, Es = np.array([loss]), np.array([lb])
    else:
        raise KeyError(trainer)
    labels = list(tensors(trainer, F))
    return dict(stats=np.asarray(st, f), Es=np.asarray(Es, f), G={k: G[k] for k in labels}, E={k: E[k] for k in labels},
                t={k: t0 + 1 for k in labels}, lr={k: hp["lr"] for k in labels})


def after64(trainer, F, hp, G, t, lr):
    """Adam (for PPO2: the norm clip and Adam) in float64 on the gradients G {label: array} from the fixture's weights and moments,
    at the case's betas and eps -> ({label: (w', m', v')}, {label: (E_w, E_m, E_v)}): adam64 / update64 and adam_bound / update_bound
    / vf_update_bound at those very arguments"""
    b1, b2, eps = adam_args(hp)
    T = tensors(trainer, F)
    if trainer == "ppo2":
        W, M, V = ({k: T[k][i] for k in T} for i in range(3))
        (tt,) = set(t.values())
        Wn, Mn, Vn, _, _ = pr.update64(W, M, V, G, hp, tt, b1, b2, eps)
        UB = pr.update_bound(W, M, V, G, hp, tt, b1, b2, eps)
        return {k: (Wn[k], Mn[k], Vn[k]) for k in G}, {k: UB[k] for k in G}
    new, bound = {}, {}
    for lab in G:
        w, m, v = T[lab]
        new[lab] = dd.adam64(w, m, v, G[lab], t[lab], lr[lab], b1, b2, eps)
        bound[lab] = dd.adam_bound(w, m, v, G[lab], t[lab], lr[lab], b1, b2, eps)
    if trainer == "trpo_vf":
        # (vf_update_bound at a gradient known exactly, as tests/test_gpu_nonfinite.py takes it: adam_bound and its (1 + 8u))
        W, M, V = ({k: T[k][i] for k in T} for i in range(3))
        zeros = {k: np.zeros_like(np.asarray(G[k], f)) for k in G}
        (tt,), (ll,) = set(t.values()), set(lr.values())
        bound = tr.vf_update_bound(W, M, V, G, zeros, tt, ll, b1, b2, eps)
    return new, bound


def targets32(trainer, F, online_after, tau):
    """{label: the target tensor after the Polyak step}: the header's formula in float32 (polyak32) on the given online weights"""
    out = {}
    for n in online(trainer):
        for k in dd.KEYS:
            out["%s/%s" % (n, k)] = dd.polyak32(F["P"][n + "_target"][k], online_after["%s/%s" % (n, k)], tau)
    return out


def _select(labels, about):
    prefix = about.partition(":")[2]
    return [k for k in labels if k.startswith(prefix)]


def separation(trainer, row, variant=None):
    """how far the float64 reference at the case lies from the reference at the twin, in the case's quantity and in units of the
    reference's own bound at the case: the median over a tensor's elements, the worst tensor; -> (separation, {label: median})"""
    F = fixture_of(trainer, row, variant)
    hc, ht = hyper_of(trainer, row), hyper_of(trainer, row, twin=True)
    c, t = step64(trainer, F, hc), step64(trainer, F, ht)
    about = row["about"]
    if about.startswith("stat:"):
        i = STAT_NAMES[trainer].index(about[5:])
        s = abs(c["stats"][i] - t["stats"][i]) / c["Es"][i]
        return float(s), {about: float(s)}
    if about.startswith("g"):
        per = {k: float(np.median(np.abs(c["G"][k] - t["G"][k]) / c["E"][k])) for k in _select(c["G"], about)}
    else:
        wc, bc = after64(trainer, F, hc, c["G"], c["t"], c["lr"])
        wt, _ = after64(trainer, F, ht, t["G"], t["t"], t["lr"])
        if about == "target":
            tc = targets32(trainer, F, {k: np.asarray(wc[k][0], np.float32) for k in wc}, hc["tau"])
            tt = targets32(trainer, F, {k: np.asarray(wt[k][0], np.float32) for k in wt}, ht["tau"])
            per = {k: float(np.median(np.abs(tc[k].astype(f) - tt[k].astype(f)) / np.spacing(np.abs(tc[k])).astype(f))) for k in tc}
        else:
            per = {k: float(np.median(np.abs(wc[k][0] - wt[k][0]) / bc[k][0])) for k in _select(wc, about)}
    assert per, (trainer, row["id"], about)
    return min(per.values()), per


def clipped_noise(z, sigma, clip):
    """the normals that, fed at the same sigma, give the device the clipped values themselves: sign(z) (clip / sigma) where
    |sigma z| exceeds the clip.  Exact only where float32(sigma) * float32(clip / sigma) == float32(clip) (the caller holds that)"""
    lim = np.float32(clip / sigma)
    return np.clip(np.asarray(z, np.float32), -lim, lim)


# ---------------------------------------------------------------------------------------------------- TRPO's solver settings
# qst_policy_step on the first 17 rows of the roll-out in 2 slices, compared as tests/test_gpu_trpo.py compares the solver: the CG
# scalars, x, the full step and shs, lm, the expected improvement replayed bit for bit from the device's own products, every product
# and every evaluated candidate within the bounds of fvp64 / ls_eval64.  about: the statistic of trpo_ref.step64 that the setting moves
TRPO_STEP_N, TRPO_STEP_SLICES = 17, 2
TRPO_STEP_DEFAULT = dict(max_kl=0.01, cg_iters=10, cg_damping=1e-2, entcoeff=0.0, backtracks=10, fvp_stride=5)
TRPO_STEP_CASES = (
    _row("max-kl-1e-4", "stat:lm", max_kl=1.0e-4), _row("max-kl-1", "stat:lm", max_kl=1.0),
    _row("cg-damping-0", "stat:shs", cg_damping=0.0), _row("cg-damping-1", "stat:shs", cg_damping=1.0),
    _row("cg-iters-1", "stat:cg_iters_run", cg_iters=1), _row("cg-iters-64", "stat:cg_iters_run", cg_iters=64),
    _row("backtracks-1", "stat:accepted", backtracks=1),
)


def trpo_step_fixture():
    return tr.weights(), tr.head(tr.rollout(), TRPO_STEP_N)
