"""The poison cases of the ACTING paths on the device -- the code that evaluates a network to choose an action: the actor and
actor-critic kernels (predict_hip, the policy roll-outs, the K-episode evaluation, both Runner kernels) and the planners (the
learned-dynamics shooting plan and MPPI, the simulator MPPI in one launch and split).  One table per family and the float64
references' own run of a case.  A helper module, not a test; numpy only.

A case puts ONE non-finite value into one element of one tensor an acting call is given: a weight, a bias, an observation (for
a roll-out: the chaser position of one env, through set_state), a normaliser, a nominal control, a caller's noise sample.  The
contract (the NON-FINITE VALUES paragraph of include/quadsim.h, include/quadsim_dyn.h and include/quadsim_dyn_mppi.h) says what
must follow; tests/test_acting_nonfinite_cpu.py anchors the references to float64 torch at every case and holds the conditions
of the tables, tests/test_gpu_acting_nonfinite.py runs every case on the device.

  case["poison"]          one of POISONS: a NaN with the sign bit clear (0x7fc00000), a NaN with the sign bit set (0xffc00000:
                          what inf - inf and 0 / 0 give on x86), +inf, -inf
  case["clean"] is None   the call reads the poison: at least one output of the reference is non-finite
  case["clean"] = reason  the reference stays finite everywhere (a -inf bias is a dead unit); held to the bound, not to the twin
  case["twin"]            the same call with the poison replaced by the finite value it overwrote: outputs the poison does not
                          reach equal the twin's bit for bit

The shapes are the smallest that reach every lane role: N = 67 envs or rows (one full wave of 64 and three lanes of a ragged
one; for k_runner_split one workgroup with two of its four tiles absent), N = 259 for the one k_runner_split case that reaches a
second workgroup, T = 3 steps, K = 1 episode of at most 4 steps.  Hidden units 0, 77 (= 16*4 + 4*3 + 1: the middle of the MFMA
permutation) and 127; observation rows 3 (tile-0 interior), 16 (first column of the second 16-env tile), 63 (last lane) and 66
(the ragged wave).
"""
import numpy as np

import actor_numerics as an

N, N_TWO_WORKGROUPS, T = 67, 259, 3
EVAL_K, EVAL_MAX_STEPS = 1, 4
POISONS = {"nan": 0x7FC00000, "nan-signed": 0xFFC00000, "pinf": 0x7F800000, "ninf": 0xFF800000}
UNITS = (0, 77, 127)
OBS_ROWS = (3, 16, 63, 66)
# one seeded weight set per layout (actor_numerics.WEIGHT_SETS): 'cancel' has live and dead rows at every unit of UNITS in
# both hidden layers on OBS_SEED's observations, the tower checkpoint is the only tower set
LAYOUTS = {"shared": "cancel", "towers": "towers"}
OBS_SEED = 2
_DEAD = "a -inf bias is a dead unit: every output of the reference is finite"
_W0_INPUT = {0: 0, 77: 5, 127: 11}             # the input k of the poisoned w0[k, j]
_NEXT = {0: 77, 77: 127, 127: 0}               # the output unit j' of the poisoned w1[j, j']


def poison_value(name):
    return np.array([POISONS[name]], np.uint32).view(np.float32)[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kind(a):
    """0 finite, 1 NaN, 2 +inf, 3 -inf, elementwise"""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))


# ---------------------------------------------------------------------------------------------------- actor sites
def _sites(layout):
    """(key, index) of every poisoned weight element of a layout, in the order of the issue's list"""
    s = []
    for j in UNITS:
        s += [("w0", (_W0_INPUT[j], j)), ("b0", (j,)), ("w1", (j, _NEXT[j])), ("b1", (j,))]
    s += [("w2", (77, 3)), ("b2", (3,))]
    s += [("wv1", (77, 127)), ("bv1", (127,)), ("wv2", (77, 0))]
    if layout == "towers":
        s += [("wv0", (5, 77))]
    return s


ACTOR_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")          # what an MlpPolicy holds: the deterministic actor
VALUE_KEYS = ("wv0", "bv0", "wv1", "bv1", "wv2", "bv2")


def _actor_cases(layout):
    cases = []
    for key, idx in _sites(layout):
        for p in POISONS:
            clean = _DEAD if p == "ninf" and key in ("b0", "b1", "bv1") else None
            cases.append(dict(id="%s-%s%s-%s" % (layout, key, list(idx), p), layout=layout, target=("w", key), elem=idx, poison=p,
                              clean=clean, twin="the clean weights"))
    for row in OBS_ROWS:
        for p in POISONS:
            cases.append(dict(id="%s-obs[%d]-%s" % (layout, row, p), layout=layout, target=("obs", None), elem=(row, 0), poison=p,
                              clean=None, twin="the clean observation / chaser position"))
    return cases


ACTOR_CASES = {layout: _actor_cases(layout) for layout in LAYOUTS}


def weight_cases(layout, keys=None):
    return [c for c in ACTOR_CASES[layout] if c["target"][0] == "w" and (keys is None or c["target"][1] in keys)]


def obs_cases(layout, rows=OBS_ROWS):
    return [c for c in ACTOR_CASES[layout] if c["target"][0] == "obs" and c["elem"][0] in rows]


_W = {}


def weights(layout):
    """the clean weight set of a layout (float32 arrays; do not modify)"""
    if layout not in _W:
        _W[layout] = {k: np.asarray(v, np.float32) for k, v in an.weight_set(LAYOUTS[layout]).items()}
    return _W[layout]


def observations(n=N):
    return an.box_obs(n, OBS_SEED)


def poisoned_weights(case, W):
    """a copy of W with the case's weight poisoned (the twin's weights are W itself)"""
    W = {k: np.array(v, np.float32) for k, v in W.items()}
    if case["target"][0] == "w":
        W[case["target"][1]][case["elem"]] = poison_value(case["poison"])
    return W


def poisoned_obs(case, obs):
    obs = np.array(obs, np.float32)
    if case["target"][0] == "obs":
        obs[case["elem"]] = poison_value(case["poison"])
    return obs


def reached(case, n=N):
    """(mean [n,4] bool, value [n] bool): the outputs the poison can reach by the wiring of the net alone.  Every other output
    has the twin's bits (the contract's 'no leak': other rows, other action components, the other branch)."""
    mean, value = np.zeros((n, 4), bool), np.zeros(n, bool)
    if case["target"][0] == "obs":
        mean[case["elem"][0]], value[case["elem"][0]] = True, True
        return mean, value
    key = case["target"][1]
    if key in ("w2", "b2"):
        mean[:, case["elem"][-1]] = True
    elif key in VALUE_KEYS:
        value[:] = True
    else:
        mean[:] = True
        value[:] = case["layout"] == "shared" and key in ("w0", "b0")       # the trunk feeds both branches
    return mean, value


# ---------------------------------------------------------------------------------------------------- the float64 reference
def reference(W, obs):
    """actor_numerics.net64 with the floating-point warnings of a poisoned evaluation off -> (mean [N,4], value [N] or None)"""
    with np.errstate(all="ignore"):
        return an.net64(W, obs)


def sample64(W, mean, eps, squash):
    """the Runner's sample in float64: u = mean + std eps (distributions.py:429), its neglogp under the diagonal Gaussian
    (:407-410) with the squash term of :414, and what the env receives, np.clip(u, -1, 1) or np.tanh(u) -> (u, neglogp, a)"""
    logstd = np.asarray(W["logstd"], np.float32).astype(np.float64).reshape(1, 4)
    std = np.exp(logstd)
    with np.errstate(all="ignore"):
        u = mean + std * eps
        d = (u - mean) / std
        nl = 0.5 * np.sum(d * d, 1) + 0.5 * np.log(2 * np.pi) * 4 + np.sum(logstd)
        if squash:
            a = np.tanh(u)
            nl = nl + np.sum(np.log(1.0 - a ** 2 + 1e-6), 1)
        else:
            a = np.clip(u, -1.0, 1.0)
    return u, nl, a


def _pre(layers, x, depth):
    """pre-activation z of layer `depth` of a chain and its first-order error magnitude (actor_numerics.err_scale's recursion)"""
    h, E = np.asarray(x, np.float64), np.zeros(np.shape(x))
    for i, (w, b) in enumerate(layers):
        aw = np.abs(w)
        z = h @ w + b
        E = E @ aw + np.abs(h) @ aw + np.abs(b)
        if i == depth:
            return z, E
        h = np.maximum(z, 0.0)


def decider(case, W, obs):
    """For an infinite weight the kind of the result (an infinity or NaN) hangs on the sign of one value of the CLEAN net per
    row: inf * h is inf for h > 0 and NaN for h = 0, so for w1[j, j'] / wv1[j, j'] it is the layer-0 pre-activation of unit j, for
    w2[j, 3] / wv2[j] the layer-1 pre-activation of unit j; for w0[k, j] / wv0[k, j] the observation element k itself (exact).
    An infinite bias decides nothing.  -> (values [N], error magnitudes E [N]) or None"""
    if case["target"][0] != "w" or case["poison"] not in ("pinf", "ninf"):
        return None
    key, idx = case["target"][1], case["elem"]
    x = np.asarray(obs, np.float64)
    pi, vf = an.branches(W)
    if key in ("w0", "wv0"):
        return x[:, idx[0]], np.zeros(x.shape[0])
    if key in ("w1", "w2"):
        z, E = _pre(pi, x, 0 if key == "w1" else 1)
    elif key in ("wv1", "wv2"):
        z, E = _pre(vf, x, 0 if key == "wv1" else 1)
    else:
        return None
    return z[:, idx[0]], E[:, idx[0]]


def decided(case, W, obs):
    """[N] bool: the deciding value of each row is larger in magnitude than the error bound of either precision (all True
    where nothing decides)"""
    d = decider(case, W, obs)
    if d is None or case["target"][1] in ("w0", "wv0"):        # an observation element is exact: 0 * inf is NaN on both sides
        return np.ones(np.shape(obs)[0], bool)
    z, E = d
    return np.abs(z) > np.maximum(an.bound(E, "f32"), an.bound(E, "bf16x3"))


def dead_twin(case, W):
    """the clean net with the unit that RECEIVES the poisoned weight or bias silenced (zero incoming weights and bias): in
    float64 the same outputs as the poisoned net on every row where that unit's pre-activation is -inf, with finite error
    magnitudes"""
    key = case["target"][1]
    W = {k: np.array(v, np.float32) for k, v in W.items()}
    if key in ("w0", "b0", "w1", "b1", "wv0", "bv0", "wv1", "bv1"):
        w, b = ("w" + key[1:], "b" + key[1:])
        W[w][:, case["elem"][-1]] = 0.0
        W[b][case["elem"][-1]] = 0.0
    return W


def scales(case, W, Wp, obs):
    """error magnitudes (E_mean [N,4], E_value [N] or None) for the finite outputs of a case: err_scale of the poisoned net, and
    where that is itself non-finite (everything behind an infinite weight) of dead_twin"""
    with np.errstate(all="ignore"):
        Em, Ev = an.err_scale(Wp, obs)
        if case["target"][0] == "w":
            Dm, Dv = an.err_scale(dead_twin(case, W), obs)
            Em = np.where(np.isfinite(Em), Em, Dm)
            Ev = None if Ev is None else np.where(np.isfinite(Ev), Ev, Dv)
    return Em, Ev


# ---------------------------------------------------------------------------------------------------- planner sites
# the smallest compiled width pair (tests/dynplan_matrix.py: (64, 64)), three envs, two tiles of 16 candidates and a ragged one,
# three steps: a non-finite prediction of step 0 reaches the score through the observations before steps 1 and 2
import dynmppi_ref  # noqa: E402
import dynplan_ref as dr  # noqa: E402
import mppi_ref  # noqa: E402

DYN_NET = "he_64_64"
PLAN_N, PLAN_PATHS, PLAN_HORIZON, PLAN_ITERATIONS = 3, 33, 3, 2
PLAN_LAM, PLAN_SIGMA = 0.5, 0.4
NOMINAL_ELEM, NOISE_ELEM = (1, 0, 2), (0, 5, 0)      # nominal_in[env][h][component]; noise[it][c][h]: all four components
_CLAMPED = "an infinity is clamped like any other value: the twin holds +-1e30 in its place"
# w1 is poisoned in the column of action component 0: the sign of its normalised input is the sign of an exact float32
# difference, the same on the device and in the reference, at every step of every candidate
DYN_SITES = (("w", "w1", (5, 12)), ("w", "b1", (5,)), ("w", "w2", (7, 5)), ("w", "b2", (7,)), ("w", "w3", (0, 7)), ("w", "b3", (4,)),
             ("norm", "in_mean", (3,)), ("norm", "out_std", (0,)))


def _dyn_cases():
    cases = []
    for kind_, key, idx in DYN_SITES:
        for p in POISONS:
            clean = _DEAD if p == "ninf" and key in ("b1", "b2") else None
            cases.append(dict(id="dyn-%s%s-%s" % (key, list(idx), p), target=(kind_, key), elem=idx, poison=p, clean=clean,
                              twin="the clean net"))
    return cases


def _mppi_cases():
    cases = []
    for what, idx in (("nominal", NOMINAL_ELEM), ("noise", NOISE_ELEM)):
        for p in POISONS:
            cases.append(dict(id="mppi-%s%s-%s" % (what, list(idx), p), target=(what, None), elem=idx, poison=p,
                              clean=_CLAMPED if p in ("pinf", "ninf") else None,
                              twin="+-1e30 in the element" if p in ("pinf", "ninf") else "the clean nominal / noise"))
    return cases


DYN_CASES = _dyn_cases()              # learned_shooting_plan and learned_mppi_plan
MPPI_CASES = _mppi_cases()            # mppi_plan, its split form and learned_mppi_plan


def dyn_weights():
    return dr.weight_set(DYN_NET)


def dyn_poisoned(case, W):
    W = {k: np.array(v) for k, v in W.items()}
    if case["target"][0] in ("w", "norm"):
        W[case["target"][1]][case["elem"]] = poison_value(case["poison"])
    return W


def dyn_dead_twin(case, W):
    """dead_twin for the dynamics net: the unit that receives the poisoned weight or bias silenced"""
    W = {k: np.array(v) for k, v in W.items()}
    key = case["target"][1]
    if key in ("w1", "b1", "w2", "b2"):
        W["w" + key[1]][case["elem"][0], :] = 0.0
        W["b" + key[1]][case["elem"][0]] = 0.0
    return W


def plan_obs():
    return dr.sample_obs(PLAN_N)


def mppi_inputs():
    """-> (nominal [n,horizon,4] float32 inside the clamp, noise [iterations,paths,horizon,4] float32), both finite"""
    rng = np.random.default_rng(77)
    nominal = rng.uniform(-0.6, 0.6, (PLAN_N, PLAN_HORIZON, 4)).astype(np.float32)
    return nominal, rng.standard_normal((PLAN_ITERATIONS, PLAN_PATHS, PLAN_HORIZON, 4)).astype(np.float32)


def mppi_poisoned(case, twin=False):
    """the case's (nominal, noise); twin: with the finite value the contract equates the poison to"""
    nominal, noise = mppi_inputs()
    if case["target"][0] in ("nominal", "noise"):
        a = nominal if case["target"][0] == "nominal" else noise
        v = poison_value(case["poison"])
        if twin:
            v = np.float32(np.sign(v) * 1e30) if case["clean"] == _CLAMPED else a[case["elem"]]
        a[case["elem"]] = v
    return nominal, noise


def mppi_nan_candidates(nominal, noise, it=0):
    """[n,paths] bool: the candidates of iteration `it` that mppi_ref.candidates32 makes NaN, given that every env keeps its
    nominal or moves to a finite one (a NaN in the nominal stays: every candidate of its env is NaN in every iteration)"""
    with np.errstate(invalid="ignore"):
        c = mppi_ref.candidates32(nominal, PLAN_SIGMA, noise[it])
    return np.isnan(c).any(axis=(2, 3))


def shooting_reference(W, obs, acts):
    """dynplan_ref's scores of the shooting plan, warnings off -> [n,paths] float64"""
    with np.errstate(all="ignore"):
        return dr.cost64(dr.rollout64(W, obs, acts))


def learned_mppi_reference(W, obs, nominal, noise):
    with np.errstate(all="ignore"):
        return dynmppi_ref.plan64(W, obs, PLAN_SIGMA, noise, PLAN_LAM, nominal=nominal, shift=0)


def dyn_decided(case, W, obs, acts, rel=1e-3):
    """For an infinite w2[j', j] / w3[r, j] the result hangs on whether hidden unit j (of layer 1 / layer 2) of the CLEAN net is
    alive, for every candidate at every step along the clean float64 trajectory.  -> True if that unit's pre-activation is, at
    every such input, larger in magnitude than `rel` times the sum of the magnitudes of its terms: the float32 error of a
    three-step trajectory is below 1e-5 of that sum (dynplan_ref.step_bound), so the sign is the same on the device."""
    if case["target"][0] != "w" or case["poison"] not in ("pinf", "ninf") or case["target"][1] not in ("w2", "w3"):
        return True
    j = case["elem"][1]
    before = dr.rollout64(W, obs, acts)
    x = np.concatenate([before, np.asarray(acts, np.float64)], axis=-1)
    h = (x - np.asarray(W["in_mean"], np.float64)) * dr.rscale(W).astype(np.float64)
    w1, b1 = np.asarray(W["w1"], np.float64), np.asarray(W["b1"], np.float64)
    z, m = h @ w1.T + b1, np.abs(h) @ np.abs(w1).T + np.abs(b1)
    if case["target"][1] == "w3":
        h1 = np.maximum(z, 0.0)
        w2, b2 = np.asarray(W["w2"], np.float64), np.asarray(W["b2"], np.float64)
        z, m = h1 @ w2.T + b2, (h1 + rel * m) @ np.abs(w2).T + np.abs(b2)
    return bool(np.all(np.abs(z[..., j]) > rel * m[..., j]))
