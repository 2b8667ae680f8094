"""-m gpu: the acting paths at NaN and inf inputs -- every case of tests/acting_nonfinite_cases.py as one call through the
production wrapper, plus its twin (the same call with the poison replaced by the finite value it overwrote).

What a case holds (the NON-FINITE VALUES paragraphs of include/quadsim.h, quadsim_dyn.h, quadsim_dyn_mppi.h):
  kind      an output of a network evaluation is non-finite exactly where the float64 reference over the same weights and
            observations is; on the exact-f32 paths it is the same kind (NaN, +inf, -inf).  On the split-bf16 paths an infinity
            may come out as NaN, and behind an infinite weight that the image stores split (hi = inf, lo = inf - inf) a finite
            reference may come out as NaN
  bound     the finite elements stay inside actor_numerics.bound / the planner tests' derived bounds: no tolerance of its own
  no leak   what the wiring of the net cannot reach (acting_nonfinite_cases.reached) has the twin's bits: other rows and envs,
            other action components, the other branch of an actor-critic
  hand-over clip(NaN) = NaN, tanh(NaN) = NaN with a NaN neglogp; an infinity is clipped or squashed like any other value
  roll-outs the reward of a step that takes a NaN action is NaN; an evaluation returns NaN for every env whose first action is
  planners  every score the reference makes NaN is NaN; an all-NaN env: winner 0, MPPI keeps U, best_score as documented
  sentinels nothing is written outside the outputs

A test runs all the cases of one entry point and configuration and reports every failing case id together.
What env.step does with a NaN action after the step it is taken in is not held (the headers' out-of-scope line): a
state-poisoned env is held at the step the poison enters, a weight-poisoned policy at every step, on the observations the kernel
reports."""
import ctypes as C

import numpy as np
import pytest

import acting_nonfinite_cases as ac
import actor_numerics as an
import dynmppi_ref
import dynplan_ref as dr
import mppi_ref
import shooting_ref
from actor_numerics import _neglogp_bound

pytestmark = pytest.mark.gpu

PRECS = ("f32", "bf16x3")
LAYOUTS = tuple(ac.LAYOUTS)
ROW = dict(env_id="docking-v0", integ="frozen", dt=0.02, randomise=1, set_params=False, n=ac.N)     # test_gpu_rollout_matrix._make's
SEED = 4100
U32 = an.KAPPA["f32"] * an.UNIT["f32"]
# the weights each packed image stores as split bf16 (hi = inf makes lo = inf - inf); everything else is float32 in the image
SPLIT_STORED = {"actor": ("w0", "w1", "w2"), "heads": ("w1", "w2", "wv1", "wv2")}


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class Problems:
    """the failing cases of one test, reported together"""

    def __init__(self):
        self.found = {}

    def add(self, cid, what):
        self.found.setdefault(cid, []).append(what)

    def check(self, cid, ok, what):
        if not ok:
            self.add(cid, what)

    def done(self, total):
        print("acting non-finite: %d of %d cases fail%s" % (len(self.found), total, (": " + ", ".join(sorted(self.found))) if self.found else ""))
        assert not self.found, "%d of %d cases fail:\n%s" % (len(self.found), total, "\n".join(
            "  %s: %s" % (k, "; ".join(v[:4])) for k, v in sorted(self.found.items())))


def _split_inf(case, image):
    return case["target"][0] == "w" and case["poison"] in ("pinf", "ninf") and case["target"][1] in SPLIT_STORED[image]


def _hold(P, cid, name, got, ref, bound, prec, split_inf, reach=None, twin=None, clipped=False):
    """one output of a network evaluation against the float64 reference `ref` (before the clip, if `clipped`)"""
    got64 = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        target = np.clip(ref, -1.0, 1.0) if clipped else ref
    if prec == "f32":
        P.check(cid, np.array_equal(ac.kind(got64), ac.kind(target)), "%s: kinds differ in %d elements (0 finite 1 NaN 2 +inf 3 -inf: got %s, reference %s)" % (
            name, int((ac.kind(got64) != ac.kind(target)).sum()), np.bincount(ac.kind(got64).ravel(), minlength=4).tolist(),
            np.bincount(ac.kind(target).ravel(), minlength=4).tolist()))
        inf_clipped = clipped & np.isinf(ref)                                 # an infinite mean is clipped to exactly +-1
        P.check(cid, bool(np.all(got64[inf_clipped] == target[inf_clipped])), "%s: a clipped infinity is not +-1" % name)
    else:
        P.check(cid, not np.isfinite(got64[~np.isfinite(target)]).any(), "%s: finite where the reference is not" % name)
        inf_clipped = clipped & np.isinf(ref)                                 # ... or, split, NaN (inf - inf)
        P.check(cid, bool(np.all(np.isnan(got64[inf_clipped]) | (got64[inf_clipped] == target[inf_clipped]))), "%s: a clipped infinity is neither +-1 nor NaN" % name)
        if not split_inf:
            P.check(cid, np.isfinite(got64[np.isfinite(ref)]).all(), "%s: non-finite where the reference is finite" % name)
    f = np.isfinite(ref) & np.isfinite(got64)
    err = np.abs(got64 - target)[f]
    P.check(cid, bool((err <= bound[f]).all()), "%s: %d finite elements out of bound, worst err / bound %.3g" % (
        name, int((~(err <= bound[f])).sum()), float((err / np.maximum(bound[f], 1e-300)).max()) if err.size else 0.0))
    if twin is not None:
        keep = ~reach
        P.check(cid, np.array_equal(_bits(got)[keep], _bits(twin)[keep]), "%s: %d elements the poison cannot reach differ from the twin" % (
            name, int((_bits(got)[keep] != _bits(twin)[keep]).sum())))


def _mlp(qa, W):
    return qa.MlpPolicy({k: W[k] for k in ac.ACTOR_KEYS})


def _actor_cases(layout):
    return ac.weight_cases(layout, ac.ACTOR_KEYS) + ac.obs_cases(layout)


# ---------------------------------------------------------------------------------------------------- predict_hip
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_predict_hip(qa, torch, layout, precision):
    """qs_policy_forward(_fast): every actor weight site and every observation row, all four poisons"""
    W, obs = ac.weights(layout), ac.observations()
    env = qa.VecDockingEnv("docking-v0", num_envs=64)

    def run(Wc, x):
        out = torch.full((ac.N + 61, 4), -7.25, device="cuda")
        a = _mlp(qa, Wc).predict_hip(env, torch.as_tensor(x, device="cuda"), precision, out=out[:ac.N])
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert a.data_ptr() == out.data_ptr() and (o[ac.N:] == -7.25).all()      # nothing past row N
        return o[:ac.N]
    twin = run(W, obs)
    P, cases = Problems(), _actor_cases(layout)
    for c in cases:
        Wp, x = ac.poisoned_weights(c, W), ac.poisoned_obs(c, obs)
        assert ac.decided(c, W, obs).all()
        m64 = ac.reference(Wp, x)[0]
        Em = ac.scales(c, W, Wp, x)[0]
        _hold(P, c["id"], "actions", run(Wp, x), m64, an.bound(Em, precision), precision, _split_inf(c, "actor"), ac.reached(c)[0], twin, clipped=True)
    env.close()
    P.done(len(cases))


# ---------------------------------------------------------------------------------------------------- policy roll-outs
def _make(qa, torch, n=ac.N, seed=SEED, t0=None):
    from test_gpu_rollout_matrix import _make as make
    env, obs = make(qa, torch, dict(ROW, n=n), seed)
    if t0 is not None:
        env.set_state(t=np.full(n, t0, np.float32))
    return env, obs.cpu().numpy().copy()


def _poison_state(env, case):
    """the case's poison as the chaser's x position of its env: the observation of that env is non-finite from then on"""
    c = env.get_state()["chaser"].copy()
    c[case["elem"][0], 0] = ac.poison_value(case["poison"])
    env.set_state(chaser=c)


def _rollout_outputs(qa, torch, pol, precision, case=None):
    env, obs0 = _make(qa, torch)
    if case is not None and case["target"][0] == "obs":
        _poison_state(env, case)
    O, R, D, F, A = (t.cpu().numpy() for t in qa.fused_policy_rollout(env, pol, ac.T, precision=precision))
    env.close()
    env, _ = _make(qa, torch)
    if case is not None and case["target"][0] == "obs":
        _poison_state(env, case)
    o, r, d, a = (t.cpu().numpy() for t in env.step_policy(pol, precision=precision))
    env.close()
    return dict(obs0=obs0, O=O, R=R, D=D, F=F, A=A, step=(o, r, d.astype(np.uint8), a))


@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_policy_rollout_and_step_policy(qa, torch, layout, precision):
    """qs_policy_rollout(_fast), T = 3, and step_policy: a weight-poisoned actor at every step on the observations the kernel
    reports, a state-poisoned env at step 0; step_policy is the roll-out's first step bit for bit"""
    W = ac.weights(layout)
    twin = _rollout_outputs(qa, torch, _mlp(qa, W), precision)
    P, cases = Problems(), _actor_cases(layout)
    for c in cases:
        cid = c["id"]
        Wp = ac.poisoned_weights(c, W)
        out = _rollout_outputs(qa, torch, _mlp(qa, Wp), precision, c)
        for k, (x, y) in enumerate(zip(out["step"], (out["O"][0], out["R"][0], out["D"][0], out["A"][0]))):
            P.check(cid, _same_bits(x, y), "step_policy output %d is not the roll-out's first step" % k)
        A, R = out["A"], out["R"]
        P.check(cid, bool(np.isnan(R[np.isnan(A).any(axis=2)]).all()), "a finite reward at a step that took a NaN action")
        if c["target"][0] == "obs":
            row = c["elem"][0]
            others = np.arange(ac.N) != row
            for name in ("O", "R", "D", "F", "A"):                            # every other env, every step: the twin's bits
                P.check(cid, _same_bits(out[name][:, others], twin[name][:, others]), "%s of the other envs differs from the twin" % name)
            a0 = A[0, row]
            if c["poison"].startswith("nan"):
                P.check(cid, bool(np.isnan(a0).all() and np.isnan(R[0, row])), "the poisoned env's first action / reward is not NaN: %s %s" % (a0, R[0, row]))
            else:                                                             # a non-finite mean in every component: NaN or a clipped infinity
                P.check(cid, bool(np.all(np.isnan(a0) | (np.abs(a0) == 1.0))), "the poisoned env's first action is neither NaN nor +-1: %s" % a0)
            continue
        acted = np.concatenate([out["obs0"][None], out["O"][:-1]])
        P.check(cid, bool(ac.decided(c, W, acted[0]).all()), "set-up: an undecided row at step 0")
        reach = ac.reached(c)[0]
        for t in range(ac.T):
            m64 = ac.reference(Wp, acted[t])[0]
            Em = ac.scales(c, W, Wp, acted[t])[0]
            _hold(P, cid, "actions[%d]" % t, A[t], m64, an.bound(Em, precision), precision, _split_inf(c, "actor"),
                  reach if t == 0 else None, twin["A"][0] if t == 0 else None, clipped=True)
        same_row = np.all(_bits(A[0]) == _bits(twin["A"][0]), axis=1)          # the env received the twin's action: the twin's step
        for name in ("O", "R", "D", "F"):
            P.check(cid, _same_bits(out[name][0][same_row], twin[name][0][same_row]), "%s[0] differs from the twin where the action does not" % name)
        if c["poison"].startswith("nan") and c["target"][1] not in ("w2", "b2"):
            P.check(cid, bool(np.isnan(A).all() and np.isnan(R).all()), "a NaN weight that reaches the mean: finite actions or rewards")
    P.done(len(cases))


# ---------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("precision", PRECS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_evaluate_policy_episodes(qa, torch, layout, precision):
    """qs_policy_evaluate(_fast), K = 1, max_steps = 4, every env three steps before its time-out: an env whose first action
    is NaN returns NaN; a poisoned value branch changes nothing; the handle is left as it was"""
    W = ac.weights(layout)
    env, obs0 = _make(qa, torch, t0=597.0)
    state = env.get_state()

    def run(Wc):
        return qa.evaluate_policy_episodes(qa.ActorCriticPolicy(Wc), env, ac.EVAL_K, precision=precision, max_steps=ac.EVAL_MAX_STEPS).numpy()
    twin = run(W)
    assert (twin["finished"] == 1).all() and np.isfinite(twin["returns"]).all() and (twin["lengths"] <= 3).all()
    P, cases = Problems(), ac.weight_cases(layout) + ac.obs_cases(layout)
    for c in cases:
        cid = c["id"]
        Wp = ac.poisoned_weights(c, W)
        x = obs0
        if c["target"][0] == "obs":
            _poison_state(env, c)
        got = run(Wp)
        if c["target"][0] == "obs":
            env.set_state(**state)
            row = c["elem"][0]
            others = np.arange(ac.N) != row
            for k in got:
                P.check(cid, _same_bits(got[k][..., others], twin[k][..., others]), "%s of the other envs differs from the twin" % k)
            if c["poison"].startswith("nan"):
                P.check(cid, bool(np.isnan(got["returns"][0, row]) and got["finished"][row] == 1), "the poisoned env's return is not NaN")
            continue
        P.check(cid, bool((got["finished"] == 1).all()), "an env did not finish its episode")
        if c["target"][1] in ac.VALUE_KEYS:                                   # the evaluation runs the actor alone
            for k in got:
                P.check(cid, _same_bits(got[k], twin[k]), "%s differs from the twin for a value-branch poison" % k)
            continue
        P.check(cid, bool(ac.decided(c, W, x).all()), "set-up: an undecided row at step 0")
        with np.errstate(invalid="ignore"):
            nan_first = np.isnan(np.clip(ac.reference(Wp, x)[0], -1.0, 1.0)).any(axis=1)
        P.check(cid, bool(np.isnan(got["returns"][0, nan_first]).all()), "%d envs whose first action is NaN return a number" % int(
            np.isfinite(got["returns"][0, nan_first]).sum()))
        if c["poison"].startswith("nan") and c["target"][1] not in ("w2", "b2"):
            P.check(cid, bool(nan_first.all() and np.isnan(got["returns"]).all()), "a NaN weight that reaches the mean: a finite return")
    after = env.get_state()
    assert all(_same_bits(after[k], state[k]) for k in state)
    env.close()
    P.done(len(cases))


# ---------------------------------------------------------------------------------------------------- the Runner kernels
RUNNER_CONFIGS = [(serial, prec, layout, squash, noise) for serial in (1, 0) for prec in PRECS for layout in LAYOUTS
                  for squash in (False, True) for noise in ("caller", "kernel")]


def _runner_id(cfg):
    serial, prec, layout, squash, noise = cfg
    return "%s-%s-%s-%s-%s" % (("k_runner_split", "k_runner_rollout")[serial], prec, layout, ("clip", "squash")[squash], noise)


def _runner(qa, torch, W, cfg, case=None, n=ac.N):
    serial, prec, _, squash, noise_src = cfg
    env, _ = _make(qa, torch, n=n)
    if case is not None and case["target"][0] == "obs":
        _poison_state(env, case)
    k0 = env.step_counter
    noise = torch.randn((ac.T, n, 4), generator=torch.Generator().manual_seed(SEED)) * 1.5 if noise_src == "caller" else None
    lib = env._lib
    lib.qs_debug_set_runner_serial.argtypes = [C.c_int]
    before = lib.qs_debug_set_runner_serial(serial)
    try:
        ro = qa.fused_runner_rollout(env, qa.ActorCriticPolicy(W, squash=squash), ac.T, noise=noise, precision=prec)
        torch.cuda.synchronize()
    finally:
        lib.qs_debug_set_runner_serial(before)
    out = {k: v.cpu().numpy() for k, v in ro.items() if v is not None}
    env.close()
    out["eps"] = None if noise is None else noise.numpy().astype(np.float64)
    out["k0"] = k0
    return out


def _runner_eps(out, oracle64, n):
    from test_gpu_rollout_matrix import GID0
    if out["eps"] is None:
        out["eps"] = np.stack([[oracle64.normal4(SEED, GID0 + i, out["k0"] + t) for i in range(n)] for t in range(ac.T)]).astype(np.float64)
    return out["eps"]


ROLLOUT_KEYS = ("obs", "actions", "values", "neglogp", "dones", "rewards", "last_obs", "last_values", "last_dones")


def _hold_runner(P, c, W, cfg, out, twin, eps, n=ac.N):
    cid, (_, prec, _, squash, _) = c["id"], cfg
    Wp = ac.poisoned_weights(c, W)
    split_inf = _split_inf(c, "heads")
    U, V, NL, R = out["actions"], out["values"], out["neglogp"], out["rewards"]
    P.check(cid, bool(np.isnan(R[np.isnan(U).any(axis=2)]).all()), "a finite reward at a step that took a NaN action")
    P.check(cid, bool(np.isnan(NL[np.isnan(U).any(axis=2)]).all()), "a finite neglogp for a NaN sample")
    rm, rv = ac.reached(c, n)
    if c["target"][0] == "obs":                                               # every other env, every step, every output
        others = np.arange(n) != c["elem"][0]
        for k in ROLLOUT_KEYS:
            a, b = (out[k][others], twin[k][others]) if k.startswith("last") else (out[k][:, others], twin[k][:, others])
            P.check(cid, _same_bits(a, b), "%s of the other envs differs from the twin" % k)
        P.check(cid, not np.isfinite(out["obs"][0, c["elem"][0]]).all(), "set-up: the poisoned env's observation is finite")
    elif not rm.any():                                                        # a poisoned value branch: only the values move
        for k in ROLLOUT_KEYS:
            if k not in ("values", "last_values"):
                P.check(cid, _same_bits(out[k], twin[k]), "%s differs from the twin for a value-branch poison" % k)
    steps = (0,) if c["target"][0] == "obs" else range(ac.T)
    std = np.exp(np.asarray(W["logstd"], np.float32).astype(np.float64)).reshape(1, 4)
    for t in steps:
        x, e = out["obs"][t], eps[t]
        if c["target"][0] == "w" and t == 0:
            P.check(cid, bool(ac.decided(c, W, x).all()), "set-up: an undecided row at step 0")
        m64, v64 = ac.reference(Wp, x)
        Em, Ev = ac.scales(c, W, Wp, x)
        u64, nl64, a64 = ac.sample64(Wp, m64, e, squash)
        with np.errstate(invalid="ignore"):
            mb = an.bound(Em, prec)
            ub = mb + U32 * (np.abs(u64) + std * np.abs(e))
            nb = _neglogp_bound(Wp, u64, m64, e, mb, squash)
        first = t == 0 and c["target"][0] == "w"                             # the twin acted on the same observations
        _hold(P, cid, "actions[%d]" % t, U[t], u64, ub, prec, split_inf, rm if first else None, twin["actions"][0] if first else None)
        _hold(P, cid, "values[%d]" % t, V[t], v64, an.bound(Ev, prec), prec, split_inf, rv if first else None, twin["values"][0] if first else None)
        nl = NL[t].astype(np.float64)
        if prec == "f32":
            P.check(cid, np.array_equal(np.isnan(nl), np.isnan(nl64)), "neglogp[%d] is NaN in other rows than the reference's" % t)
        f = np.isfinite(nl64) & np.isfinite(nl)
        P.check(cid, bool((np.abs(nl - nl64)[f] <= nb[f]).all()), "neglogp[%d] out of bound" % t)
        if first:
            keep = ~rm.any(axis=1)
            P.check(cid, _same_bits(NL[0][keep], twin["neglogp"][0][keep]), "neglogp[0] differs from the twin where the mean does not")
            same_row = np.all(_bits(U[0]) == _bits(twin["actions"][0]), axis=1)
            P.check(cid, _same_bits(R[0][same_row], twin["rewards"][0][same_row]), "rewards[0] differs from the twin where the sample does not")
        if t == 0:                                                            # where no component is NaN the env got a number
            P.check(cid, bool(np.isfinite(R[0][~np.isnan(U[0]).any(axis=1) & np.isfinite(x).all(axis=1)]).all()), "a NaN reward without a NaN action")
    if c["target"][0] == "w":
        lo = out["last_obs"]
        _hold(P, cid, "last_values", out["last_values"], ac.reference(Wp, lo)[1], an.bound(ac.scales(c, W, Wp, lo)[1], prec), prec, split_inf)


@pytest.mark.parametrize("cfg", RUNNER_CONFIGS, ids=[_runner_id(c) for c in RUNNER_CONFIGS])
def test_fused_runner_rollout(qa, torch, oracle64, cfg):
    """qs_runner_rollout(_net)(_fast) through both kernels: every weight site of the layout and two observation rows (3 and the
    ragged wave's 66); the four poisons go round the sites, shifted by the configuration's index, so that every site meets
    every poison in four configurations"""
    layout = cfg[2]
    W = ac.weights(layout)
    twin = _runner(qa, torch, W, cfg)
    eps = _runner_eps(twin, oracle64, ac.N)
    for k in ROLLOUT_KEYS:
        assert np.isfinite(twin[k].astype(np.float64)).all(), k
    sites = ac.weight_cases(layout)[::4] + ac.obs_cases(layout, (3, 66))[::4]
    shift = RUNNER_CONFIGS.index(cfg)
    by_id = {c["id"]: c for c in ac.ACTOR_CASES[layout]}
    names = list(ac.POISONS)
    P, cases = Problems(), []
    for i, site in enumerate(sites):
        cases.append(by_id[site["id"].rsplit("-nan", 1)[0] + "-" + names[(i + shift) % 4]])
    for c in cases:
        out = _runner(qa, torch, ac.poisoned_weights(c, W), cfg, c)
        _hold_runner(P, c, W, cfg, out, twin, eps)
    P.done(len(cases))


@pytest.mark.parametrize("precision", PRECS)
def test_runner_split_second_workgroup(qa, torch, oracle64, precision):
    """k_runner_split with N = 259: envs 256..258 are the one ragged tile of a second workgroup.  A state poison there, and a
    NaN weight that reaches every env"""
    cfg = (0, precision, "shared", False, "caller")
    n = ac.N_TWO_WORKGROUPS
    W = ac.weights("shared")
    twin = _runner(qa, torch, W, cfg, n=n)
    eps = _runner_eps(twin, oracle64, n)
    P = Problems()
    cases = [dict(ac.obs_cases("shared", (3,))[1], id="shared-obs[258]-nan-signed", elem=(n - 1, 0)),
             [c for c in ac.weight_cases("shared", ("w1",)) if c["poison"] == "nan-signed"][1]]
    for c in cases:
        out = _runner(qa, torch, ac.poisoned_weights(c, W), cfg, c, n=n)
        _hold_runner(P, c, W, cfg, out, twin, eps, n=n)
        if c["target"][0] == "w":
            P.check(c["id"], bool(np.isnan(out["actions"]).all() and np.isnan(out["rewards"]).all()), "an env of the second workgroup acted on a number")
    P.done(len(cases))


# ---------------------------------------------------------------------------------------------------- learned planners
def _plan_acts():
    return np.stack([shooting_ref.actions_fast(dr.EDGE_SEED, dr.EDGE_GID0 + i, dr.EDGE_K, ac.PLAN_PATHS, ac.PLAN_HORIZON)
                     for i in range(ac.PLAN_N)])


def _finite_steps(P, cid, Wb, obs, traj, cands, scores):
    """the planner tests' own bounds on whatever stays finite: every model step from the kernel's own inputs within
    dynplan_ref.step_bound (of the net Wb, whose error magnitudes are finite), every score within score_bound of its trajectory"""
    paths = cands.shape[1]
    before = np.concatenate([np.repeat(np.asarray(obs, np.float32)[:, None, None, :], paths, axis=1), traj[:, :, :-1]], axis=2)
    with np.errstate(all="ignore"):
        ref, bound = dr.step64(Wb, before, cands, with_bound=True)
        f = np.isfinite(traj) & np.isfinite(ref)
        P.check(cid, bool((np.abs(traj - ref)[f] <= bound[f]).all()), "finite trajectory elements out of the step bound")
        cost, sb = dr.cost64(before), dr.score_bound(before)
        g = np.isfinite(scores)
        P.check(cid, bool(np.isfinite(cost[g]).all() and (np.abs(scores - cost)[g] <= sb[g]).all()), "finite scores out of the score bound")
        P.check(cid, np.array_equal(np.isnan(scores), np.isnan(cost)), "a score is NaN where its own trajectory is not, or the reverse")


def test_learned_shooting_plan(qa, torch):
    """qsd_shooting_plan through learned_shooting_plan (and once per case between sentinel bytes): every site of the dynamics
    net and its normalisers, all four poisons"""
    from test_gpu_dynplan import GID0, K0, SEED as PSEED, plan
    W, obs, acts = ac.dyn_weights(), ac.plan_obs(), _plan_acts()
    assert (PSEED, GID0, K0) == (dr.EDGE_SEED, dr.EDGE_GID0, dr.EDGE_K)
    n, paths, horizon = ac.PLAN_N, ac.PLAN_PATHS, ac.PLAN_HORIZON
    twin = plan(torch, dr.to_net(W, "cuda"), obs, horizon, paths)
    P = Problems()
    for c in ac.DYN_CASES:
        cid = c["id"]
        Wp = ac.dyn_poisoned(c, W)
        net = dr.to_net(Wp, "cuda")
        assert net.compiled == (64, 64)
        out = plan(torch, net, obs, horizon, paths)                           # raises if a sentinel byte was overwritten
        pub = qa.learned_shooting_plan(net, torch.as_tensor(obs).cuda(), horizon, paths, seed=PSEED, k=K0, gid0=GID0, return_scores=True,
                                       return_sequence=True, return_traj=True)
        for k, v in pub.items():
            P.check(cid, _same_bits(v.cpu().numpy(), out[k]), "the public call's %s differs from the raw call's" % k)
        S64 = ac.shooting_reference(Wp, obs, acts)
        S = out["scores"]
        P.check(cid, np.array_equal(np.isnan(S), np.isnan(S64)), "scores: %d NaN, the reference %d" % (int(np.isnan(S).sum()), int(np.isnan(S64).sum())))
        P.check(cid, not np.isinf(S).any(), "an infinite score")
        _finite_steps(P, cid, ac.dyn_dead_twin(c, W), obs, out["traj"], acts, S)
        for i in range(n):                                                    # the winner: the header's total order, NaN never wins
            with np.errstate(invalid="ignore"):
                b = 0 if np.isnan(S[i]).all() else int(np.nanargmax(S[i]))
            P.check(cid, int(out["best_index"][i]) == b, "env %d: winner %d, expected %d" % (i, int(out["best_index"][i]), b))
            P.check(cid, _same_bits(out["best_score"][i:i + 1], S[i, b:b + 1]), "env %d: best_score is not the winner's score" % i)
            P.check(cid, _same_bits(out["sequence"][i], acts[i, b]) and _same_bits(out["actions"][i], acts[i, b, 0]), "env %d: not the winner's actions" % i)
        if c["clean"] is None and c["poison"].startswith("nan"):
            P.check(cid, bool(np.isnan(S).all() and (out["best_index"] == 0).all() and np.isnan(out["best_score"]).all()), "all-NaN outcome")
    assert np.isfinite(twin["scores"]).all()
    P.done(len(ac.DYN_CASES))


def _hold_mppi(P, cid, out, nominal, noise, lam, sigma):
    """what every MPPI plan of this file must show on its own outputs: the candidates mppi_ref makes of the trace and the
    noise, a NaN score exactly for a NaN candidate where stated by the caller, weight 0 for a NaN score, U kept by an all-NaN
    env, best_score as documented"""
    n, iters = out["scores"].shape[:2]
    with np.errstate(invalid="ignore"):
        P.check(cid, _same_bits(out["trace"][:, 0], nominal), "trace[0] is not the nominal")
        want = mppi_ref.candidates32(out["trace"][:, iters - 1], sigma, noise[iters - 1])
        P.check(cid, _same_bits(out["candidates"], want), "the last iteration's candidates are not mppi_ref.candidates32's")
        for it in range(iters):
            S = out["scores"][:, it]
            new = mppi_ref.update64(S, mppi_ref.candidates32(out["trace"][:, it], sigma, noise[it]), lam, out["trace"][:, it])
            got = out["trace"][:, it + 1].astype(np.float64)
            P.check(cid, np.array_equal(np.isnan(got), np.isnan(new)), "trace[%d]: NaN in other elements than update64's" % (it + 1))
            f = np.isfinite(new)
            P.check(cid, bool((np.abs(got - new)[f] <= 2.0 * 2.0 ** -24).all()), "trace[%d] off update64 of the device's own scores" % (it + 1))
            dead = np.isnan(S).all(axis=1)
            P.check(cid, _same_bits(out["trace"][dead, it + 1], out["trace"][dead, it]), "an all-NaN env did not keep U in iteration %d" % it)
        last = out["scores"][:, -1]
        best = np.where(np.isnan(last).all(axis=1), -np.inf, np.nanmax(np.where(np.isnan(last), -np.inf, last), axis=1))
    P.check(cid, _same_bits(out["best_score"], best), "best_score is not the largest non-NaN score (-inf without one)")
    P.check(cid, _same_bits(out["nominal"], out["trace"][:, -1]) and _same_bits(out["actions"], out["nominal"][:, 0]), "nominal / actions")


def test_learned_mppi_plan(qa, torch):
    """qsdm_mppi_plan between sentinel bytes and through learned_mppi_plan, two iterations with the caller's noise: the
    dynamics-net sites, then a NaN / inf in nominal_in[1][0][2] and in noise[0][5][0]"""
    from test_gpu_dynmppi import GID0, K0, SEED as PSEED, plan
    W, obs = ac.dyn_weights(), ac.plan_obs()
    paths, horizon, iters, lam, sigma = ac.PLAN_PATHS, ac.PLAN_HORIZON, ac.PLAN_ITERATIONS, ac.PLAN_LAM, ac.PLAN_SIGMA
    nominal, noise = ac.mppi_inputs()
    clean_net = dr.to_net(W, "cuda")
    base = plan(torch, clean_net, obs, horizon, paths, iters, lam=lam, sigma=sigma, nominal=nominal, noise=noise)
    assert np.isfinite(base["scores"]).all()
    P = Problems()
    for c in ac.DYN_CASES:
        cid = c["id"]
        Wp = ac.dyn_poisoned(c, W)
        net = dr.to_net(Wp, "cuda")
        out = plan(torch, net, obs, horizon, paths, iters, lam=lam, sigma=sigma, nominal=nominal, noise=noise)
        pub = qa.learned_mppi_plan(net, torch.as_tensor(obs).cuda(), horizon=horizon, paths=paths, iterations=iters, lam=lam, sigma=sigma,
                                   nominal=torch.as_tensor(nominal).cuda(), noise=torch.as_tensor(noise).cuda(), seed=PSEED, k=K0, gid0=GID0,
                                   return_scores=True, return_trace=True, return_candidates=True, return_traj=True)
        for k, v in pub.items():
            P.check(cid, _same_bits(v.cpu().numpy(), out[k]), "the public call's %s differs from the raw call's" % k)
        ref = ac.learned_mppi_reference(Wp, obs, nominal, noise)
        S = out["scores"]
        P.check(cid, np.array_equal(np.isnan(S[:, 0]), np.isnan(ref["scores"][:, 0])), "iteration 0: %d NaN scores, the reference %d" % (
            int(np.isnan(S[:, 0]).sum()), int(np.isnan(ref["scores"][:, 0]).sum())))
        P.check(cid, not np.isinf(S).any(), "an infinite score")
        _hold_mppi(P, cid, out, nominal, noise, lam, sigma)
        _finite_steps(P, cid, ac.dyn_dead_twin(c, W), obs, out["traj"], out["candidates"], S[:, -1])
        if c["clean"] is None and c["poison"].startswith("nan"):
            P.check(cid, bool(np.isnan(S).all() and (out["best_score"] == -np.inf).all() and _same_bits(out["nominal"], nominal)), "all-NaN outcome: U kept, -inf")
    for c in ac.MPPI_CASES:
        cid = c["id"]
        nom, z = ac.mppi_poisoned(c)
        tn, tz = ac.mppi_poisoned(c, twin=True)
        out = plan(torch, clean_net, obs, horizon, paths, iters, lam=lam, sigma=sigma, nominal=nom, noise=z)
        twin = plan(torch, clean_net, obs, horizon, paths, iters, lam=lam, sigma=sigma, nominal=tn, noise=tz)
        _hold_mppi_case(P, c, out, twin, nom, z, lam, sigma)
    P.done(len(ac.DYN_CASES) + len(ac.MPPI_CASES))


def _hold_mppi_case(P, c, out, twin, nom, z, lam, sigma):
    """a nominal / noise case of any of the MPPI entry points against its twin"""
    cid = c["id"]
    n = out["scores"].shape[0]
    _hold_mppi(P, cid, out, nom, z, lam, sigma)
    nan0 = ac.mppi_nan_candidates(nom, z, 0)
    P.check(cid, np.array_equal(np.isnan(out["scores"][:, 0]), nan0), "iteration 0: the NaN scores are not the NaN candidates")
    if c["clean"] is not None:                                                # an infinity: the clamp's +-1, the twin's +-1e30
        for k in out:
            a, b = out[k], twin[k]
            if k == "trace" and c["target"][0] == "nominal":                  # trace[0] holds the nominal itself
                a, b = a[:, 1:], b[:, 1:]
            P.check(cid, _same_bits(a, b), "%s differs from the twin's" % k)
        P.check(cid, bool(np.isfinite(out["scores"]).all()), "a clamped infinity made a NaN score")
    elif c["target"][0] == "nominal":                                         # env 1 alone, both iterations; U kept with its NaN
        i = c["elem"][0]
        others = np.arange(n) != i
        for k in out:
            P.check(cid, _same_bits(out[k][others], twin[k][others]), "%s of the other envs differs from the twin" % k)
        P.check(cid, bool(np.isnan(out["scores"][i]).all() and out["best_score"][i] == -np.inf), "the poisoned env has a score")
        P.check(cid, _same_bits(out["nominal"][i], nom[i]), "the poisoned env did not keep U")
    else:                                                                     # candidate 5 of every env in iteration 0
        keep = np.arange(out["scores"].shape[2]) != c["elem"][1]
        P.check(cid, _same_bits(out["scores"][:, 0][:, keep], twin["scores"][:, 0][:, keep]), "scores of the other candidates differ from the twin")
        h = c["elem"][2]
        P.check(cid, bool(np.isnan(out["trace"][:, 1, h]).all() and np.isnan(out["scores"][:, 1]).all()), "0 * NaN did not reach the nominal (mppi_ref.update64)")
        rest = np.arange(out["trace"].shape[2]) != h
        P.check(cid, bool(np.isfinite(out["trace"][:, 1][:, rest]).all()), "the NaN spread to other steps of the nominal")


# ---------------------------------------------------------------------------------------------------- simulator MPPI
@pytest.mark.parametrize("splits", [None, 1, 2], ids=["qs_mppi_plan", "split-1", "split-2"])
def test_mppi_plan_nominal_and_noise(qa, torch, splits):
    """qs_mppi_plan and qs_mppi_plan_split (S = 1, 2): NaN / inf in nominal_in[1][0][2] and in the caller's noise[0][5][0]"""
    from plan_cases import make_handle, snapshot, same
    paths, horizon, iters, lam, sigma = ac.PLAN_PATHS, ac.PLAN_HORIZON, ac.PLAN_ITERATIONS, ac.PLAN_LAM, ac.PLAN_SIGMA
    env = make_handle(qa, "docking-v0", "frozen", False, n=ac.PLAN_N, provoke=None)
    before = snapshot(env)

    def run(nominal, noise):
        out = env.mppi_plan(horizon, paths, iters, "reward", lam, sigma, nominal=torch.as_tensor(nominal).to(env.device),
                            noise=torch.as_tensor(noise).to(env.device), return_scores=True, return_trace=True, return_candidates=True,
                            **({} if splits is None else {"splits": splits}))
        return {k: v.cpu().numpy() for k, v in out.items()}
    base = run(*ac.mppi_inputs())
    assert np.isfinite(base["scores"]).all()
    P = Problems()
    for c in ac.MPPI_CASES:
        nom, z = ac.mppi_poisoned(c)
        out, twin = run(nom, z), run(*ac.mppi_poisoned(c, twin=True))
        _hold_mppi_case(P, c, out, twin, nom, z, lam, sigma)
    assert same(snapshot(env), before)                                        # a plan leaves the handle as it was
    env.close()
    P.done(len(ac.MPPI_CASES))
