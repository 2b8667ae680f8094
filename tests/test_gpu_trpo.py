"""TRPO on the device (quadsim_amd.trpo, libquadsim_trpo.so) against tests/trpo_ref.py: the float64 restatement, its derived
bounds and the replay of the solver's algebra.  All tests call the C ABI through ctypes with every array the library writes (the
thirteen tensors, the moments, the statistics, the gradient, the trace, the workspace) between 256 sentinel bytes on both sides.
What is held:
  gradient     every element of g and the statistics of a step within grad64's bounds; n = 1, 15, 16, 17, 300, slices 1, 2, 7 (more
               slices than chunks: trailing slices are empty)
  one product  cg_iters = 1: the traced z against the float64 (F + damping) v of the traced v, n = 1, 6, 17, 301 at stride 5 and 1
  the solver   cg_iters = 10: every traced z_k within the bound of the float64 product of the DEVICE's p_k; p_k, the CG scalars, x,
               shs, lm, fullstep and expected_improve bit for bit the replay from the traced z's; an early residual_tol stop leaves
               the later trace rows untouched
  line search  the five fixtures of trpo_ref.LS_FIXTURES: surr_k and kl_k of every evaluated candidate within bounds at the device's
               own theta_k, the accepted k that of the float64 reference, the policy bit for bit float32(theta_old + fullstep 2^-k),
               the value tower and the moments untouched
  skips        n = 1, equal advantages: accepted = -2, every tensor bit for bit; a NaN observation row: rejected, theta bit for bit.
               The table of single poisons of the policy step and of the value fit is tests/nonfinite_cases.py's TRPO_STEP_CASES and
               TRPO_VF_CASES, run by tests/test_gpu_nonfinite.py through policy_step and vf_fit; for that policy_step takes moments,
               a row count below the arrays', the workspace's bytes at entry (and returns them) and a trace of marked NaNs (filled,
               unwritten: whether an element was written is a question of bits also where a NaN is written)
  invariants   a second stream, with and without the trace, twice from the same state: the same bits
  value fit    one step at batch 1, 15, 16, 17, 128, 256 within bounds; five steps in one launch = five launches; the policy untouched
  Python       trpo_policy_step feeds predict_hip and the Runner; TRPO.learn with and without an expert; the refusals"""
import ctypes as C

import numpy as np
import pytest

import ppo2_ref as pr
import trpo_ref as tr
from side_cases import Guarded, same_bits

pytestmark = pytest.mark.gpu

KEYS = pr.KEYS_TOWERS
HP = dict(max_kl=0.01, cg_iters=10, cg_damping=1e-2, entcoeff=0.0, backtracks=10, fvp_stride=5)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _net(torch, W, M=None, V=None):
    from quadsim_amd import _lib
    g = {k: Guarded(torch, np.asarray(W[k], np.float32)) for k in KEYS}
    zero = {k: np.zeros(pr.SHAPES[k], np.float32) for k in KEYS}
    gm = {k: Guarded(torch, (M or zero).get(k, zero[k])) for k in KEYS}
    gv = {k: Guarded(torch, (V or zero).get(k, zero[k])) for k in KEYS}
    arr = lambda d: (C.c_void_p * 13)(*[d[k].ptr for k in KEYS])  # noqa: E731
    return _lib.QstNet(C.sizeof(_lib.QstNet), 1, arr(g), arr(gm), arr(gv)), g, gm, gv


FILL32, FILL64 = 0x7FC12345, 0x7FF8000012345678      # NaNs with a payload no arithmetic produces: a trace element the call did not write


def filled(shape, dtype):
    """an array of the marked NaN: whether the call wrote an element is a question of bits, also where it writes a NaN"""
    bits, word = (FILL32, np.uint32) if np.dtype(dtype) == np.float32 else (FILL64, np.uint64)
    return np.full(shape, bits, word).view(dtype)


def unwritten(a):
    """the elements of a trace array that still hold the marked NaN of `filled`"""
    bits, word = (FILL32, np.uint32) if a.dtype == np.float32 else (FILL64, np.uint64)
    return np.ascontiguousarray(a).view(word) == bits


def policy_step(torch, W, data, hp, slices=0, trace=True, stream=None, nan_fill=True, M=None, V=None, n=None, ws_init=None, marked=False):
    """one qst_policy_step -> dict of host arrays (sentinels checked): stats, grad, W (the thirteen tensors after), M, V, trace, ws
    (the workspace's bytes after the call).  M, V: the moments (None: zeros); n: the rows the call is told of (None: all the arrays
    hold); ws_init: the bytes the workspace holds at entry (None: zeros); marked: the trace starts as `filled`"""
    from quadsim_amd import _lib, trpo
    lib = trpo.load_trpo()
    n = data["obs"].shape[0] if n is None else n
    assert 1 <= n <= data["obs"].shape[0]
    hp = dict(HP, **hp)
    hp.setdefault("residual_tol", 1e-10)
    net, g, gm, gv = _net(torch, W, M, V)
    d = {k: Guarded(torch, data[k]) for k in ("obs", "actions", "returns", "values")}
    bat = _lib.QstBatch(C.sizeof(_lib.QstBatch), 0, n, *(d[k].ptr for k in ("obs", "actions", "returns", "values")))
    hyp = _lib.QstHyper(C.sizeof(_lib.QstHyper), hp["cg_iters"], hp["backtracks"], hp["fvp_stride"], hp["max_kl"], hp["cg_damping"],
                        hp["entcoeff"], hp["residual_tol"])
    need = C.c_size_t(0)
    assert lib.qst_workspace_bytes(n, slices, C.byref(need)) == 0
    ws = Guarded(torch, np.zeros(need.value, np.uint8) if ws_init is None else np.asarray(ws_init, np.uint8))
    assert ws.n == need.value
    stats, grad = Guarded(torch, np.full(10, np.nan, np.float32)), Guarded(torch, np.full(tr.P, np.nan, np.float32))
    fill = np.nan if nan_fill else 0.0
    new = filled if marked else (lambda shape, dtype: np.full(shape, fill, dtype))
    T = None
    if trace:
        T = {"fvp_in": Guarded(torch, new((hp["cg_iters"] + 1, tr.P), np.float32)), "fvp_out": Guarded(torch, new((hp["cg_iters"] + 1, tr.P), np.float32)),
             "cg": Guarded(torch, new((hp["cg_iters"], 4), np.float64)), "x": Guarded(torch, new(tr.P, np.float32)),
             "fullstep": Guarded(torch, new(tr.P, np.float32)), "ls": Guarded(torch, new((hp["backtracks"], 2), np.float32))}
        trs = _lib.QstTrace(C.sizeof(_lib.QstTrace), 0, *(T[k].ptr for k in ("fvp_in", "fvp_out", "cg", "x", "fullstep", "ls")))
    s = torch.cuda.current_stream() if stream is None else stream
    rc = lib.qst_policy_step(C.byref(net), C.byref(bat), slices, C.byref(hyp), ws.ptr, need.value, stats.ptr, grad.ptr,
                             C.byref(trs) if trace else None, s.cuda_stream)
    assert rc == 0, lib.qst_last_error()
    s.synchronize()
    wsb = ws.get("workspace")
    for k in d:
        assert same_bits(d[k].get(k), data[k])
    out = {"stats": stats.get("stats"), "grad": grad.get("grad"), "W": {k: g[k].get(k) for k in KEYS},
           "M": {k: gm[k].get("m " + k) for k in KEYS}, "V": {k: gv[k].get("v " + k) for k in KEYS}, "ws": wsb}
    if trace:
        out["trace"] = {k: T[k].get("trace " + k) for k in T}
    return out


def within(got, ref, bound, what):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    ratio = np.abs(got - ref) / bound
    worst = float(np.max(ratio))
    print("%s: worst |device - float64| / bound = %.3g" % (what, worst))
    assert np.all(np.isfinite(got)) and worst <= 1.0, what


def untouched(out, W, keys, what):
    for k in keys:
        assert same_bits(out["W"][k], np.asarray(W[k], np.float32)), (what, k)
    for k in KEYS:
        assert not out["M"][k].any() and not out["V"][k].any(), (what, k)


# ---------------------------------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("n,slices", [(1, 1), (15, 2), (16, 1), (17, 7), (300, 7), (300, 2), (300, 0)])
def test_gradient_and_statistics_against_float64(torch, n, slices):
    """(17, 7): two chunks in seven slices, five of them empty; entcoeff 0.01 so that the logstd elements carry both terms"""
    W, data = tr.weights(), tr.head(tr.rollout(), n)
    out = policy_step(torch, W, data, dict(entcoeff=0.01, backtracks=1), slices, trace=False)
    G = tr.grad64(W, data, 0.01, with_bound=True)
    within(out["grad"], G["g"], G["E_g"], "g n=%d slices=%d" % (n, slices))
    st = out["stats"]
    within(st[0], G["surr_before"], G["E_surr"], "surr_before")
    within(st[4], G["norm"], G["E_norm"], "|g|")
    assert same_bits(st[3], np.float32(G["entropy"])) or st[8] == 0.0


# ---------------------------------------------------------------------------------------------------- one product
@pytest.mark.parametrize("n,stride", [(1, 5), (6, 5), (17, 5), (301, 5), (17, 1), (301, 1)])
def test_one_fisher_vector_product_against_float64(torch, n, stride):
    """cg_iters = 1: product 0 is on p = g, product 1 on x = alpha g; both traced pairs are held (n = 1 has g = 0 with entcoeff 0:
    the entropy term makes g the four logstd elements)"""
    W, data = tr.weights(), tr.head(tr.rollout(), n)
    out = policy_step(torch, W, data, dict(cg_iters=1, fvp_stride=stride, entcoeff=0.01, backtracks=1), 2)
    T = out["trace"]
    for k in range(2):
        v, z = T["fvp_in"][k], T["fvp_out"][k]
        assert np.all(np.isfinite(v)) and np.any(v != 0.0)
        ref, E = tr.fvp64(W, data["obs"], stride, v, 1e-2, with_bound=True)
        within(z, ref, E, "F v, product %d, n=%d stride=%d" % (k, n, stride))
    assert same_bits(T["fvp_in"][0], out["grad"])


# ---------------------------------------------------------------------------------------------------- the solver
def _check_solver(W, data, hp, out):
    T = out["trace"]
    hp = dict(HP, **hp)
    iters = int(out["stats"][9])
    R = tr.replay_cg(out["grad"], T["fvp_out"][:hp["cg_iters"]], T["fvp_out"][hp["cg_iters"]], iters, hp["max_kl"], hp.get("residual_tol", 1e-10))
    assert R["iters"] == iters
    for k in range(iters):
        assert same_bits(T["fvp_in"][k], R["p"][k]), "p_%d" % k
        ref, E = tr.fvp64(W, data["obs"], hp["fvp_stride"], T["fvp_in"][k], hp["cg_damping"], with_bound=True)
        within(T["fvp_out"][k], ref, E, "z_%d" % k)
    assert same_bits(T["cg"][:iters], R["cg"])
    assert same_bits(T["fvp_in"][hp["cg_iters"]], R["x"]) and same_bits(T["x"], R["x"])
    ref, E = tr.fvp64(W, data["obs"], hp["fvp_stride"], T["x"], hp["cg_damping"], with_bound=True)
    within(T["fvp_out"][hp["cg_iters"]], ref, E, "(F + damping) x")
    assert same_bits(T["fullstep"], R["fullstep"])
    st = out["stats"]
    assert same_bits(st[5:8], np.array([R["shs"], R["lm"], R["expected_improve"]]).astype(np.float32))
    assert same_bits(st[4], np.float32(np.sqrt(R["rdotr0"])))
    return R, iters


def test_conjugate_gradient_and_step_replay_bit_for_bit(torch):
    W, data = tr.weights(), tr.head(tr.rollout(), 300)
    out = policy_step(torch, W, data, {}, 7)
    _, iters = _check_solver(W, data, {}, out)
    assert iters == 10


def test_residual_tol_stops_the_solver_and_leaves_the_trace_rows(torch):
    """one row: A = 0, so g is entcoeff on the four logstd elements, an eigenvector of F + damping (eigenvalue 2.01): the first
    iteration leaves a residual of rounding size, rdotr < 1e-10, and the launches of the other nine return at once.  (Two rows
    stall at 7.6e-10 in float32 after ten iterations: the float64 tree of the contract on float32 vectors.)"""
    W, data = tr.weights(), tr.head(tr.rollout(), 1)
    hp = dict(entcoeff=0.01)
    out = policy_step(torch, W, data, hp, 1)
    _, iters = _check_solver(W, data, hp, out)
    print("CG iterations run: %d" % iters)
    assert 1 <= iters < 10 and out["trace"]["cg"][iters - 1, 2] < 1e-10
    T = out["trace"]
    assert np.isnan(T["fvp_in"][iters:10]).all() and np.isnan(T["fvp_out"][iters:10]).all() and np.isnan(T["cg"][iters:]).all()
    assert np.isfinite(T["fvp_out"][10]).all()


# ---------------------------------------------------------------------------------------------------- the line search
@pytest.mark.parametrize("name", list(tr.LS_FIXTURES))
def test_line_search(torch, name):
    W, data, hp, S = tr.ls_fixture(name)
    want = tr.LS_FIXTURES[name][-1]
    assert S["accepted"] == want
    out = policy_step(torch, W, data, hp, 7)
    st, T = out["stats"], out["trace"]
    th0 = tr.flatten(W, np.float32)
    evaluated = (want + 1) if want >= 0 else hp["backtracks"]
    sb = S["G"]["surr_before"]
    for k in range(evaluated):
        thk = tr.candidate32(th0, T["fullstep"], k)
        surr, kl, E_s, E_k = tr.ls_eval64(W, thk, data, hp["entcoeff"], with_bound=True)
        within(T["ls"][k, 0], surr, E_s, "%s surr_%d" % (name, k))
        within(T["ls"][k, 1], kl, E_k, "%s kl_%d" % (name, k))
        ok = kl <= 1.5 * hp["max_kl"] and surr - sb >= 0.0
        assert ok == (k == want), "the float64 decision at the device's candidate %d" % k
    assert np.isnan(T["ls"][evaluated:]).all()
    assert st[8] == want and st[9] == S["iters"]
    new = tr.flatten(out["W"], np.float32)
    assert same_bits(new, tr.candidate32(th0, T["fullstep"], want) if want >= 0 else th0)
    untouched(out, W, tr.VALUE_KEYS, name)
    if want >= 0:
        assert same_bits(st[1:3], T["ls"][want]) and st[3] == np.float32(new[tr.LS0:].astype(np.float64).sum() + 2.0 * (tr.LOG2PI + 1.0))
    else:
        assert st[1] == st[0] and st[2] == 0.0


# ---------------------------------------------------------------------------------------------------- skips and non-finite rows
def test_zero_gradient_skips_the_update(torch):
    W = tr.weights()
    one = tr.head(tr.rollout(), 1)
    flat = tr.head(tr.rollout(), 40)
    flat["values"] = (np.round(flat["values"] * 4.0) / 4.0).astype(np.float32)               # quarters: the difference below is exact
    flat["returns"] = (flat["values"] + np.float32(0.5)).astype(np.float32)
    assert np.unique(flat["returns"] - flat["values"]).size == 1
    for data in (one, flat):
        out = policy_step(torch, W, data, {}, 2)
        assert out["stats"][8] == -2.0 and out["stats"][4] == 0.0 and out["stats"][9] == 0.0
        assert not out["grad"].any()
        untouched(out, W, KEYS, "skipped")
        assert np.isnan(out["trace"]["fvp_in"]).all() and np.isnan(out["trace"]["ls"]).all()


def test_a_nan_observation_row_is_a_rejected_step(torch):
    W, data = tr.weights(), tr.head(tr.rollout(), 40)
    data["obs"] = data["obs"].copy()
    data["obs"][23] = np.nan
    out = policy_step(torch, W, data, {}, 2)
    assert out["stats"][8] == -1.0
    untouched(out, W, KEYS, "NaN row")


# ---------------------------------------------------------------------------------------------------- invariants
def test_stream_trace_and_repetition_do_not_change_the_bits(torch):
    W, data, hp, _ = tr.ls_fixture("small")
    a = policy_step(torch, W, data, hp, 2)
    b = policy_step(torch, W, data, hp, 2, stream=torch.cuda.Stream())
    c = policy_step(torch, W, data, hp, 2, trace=False)
    d = policy_step(torch, W, data, hp, 2)
    for o in (b, c, d):
        assert same_bits(o["stats"], a["stats"]) and same_bits(o["grad"], a["grad"])
        for k in KEYS:
            assert same_bits(o["W"][k], a["W"][k])
    for o in (b, d):
        for k in a["trace"]:
            assert same_bits(o["trace"][k], a["trace"][k]), k


# ---------------------------------------------------------------------------------------------------- the value fit
def vf_fit(torch, W, M, V, data, idx, t0=0, lr=1e-3, want_grads=True, beta1=tr.VF_BETA1, beta2=tr.VF_BETA2, eps=tr.VF_EPS):
    from quadsim_amd import trpo
    lib = trpo.load_trpo()
    net, g, gm, gv = _net(torch, W, M, V)
    obs, ret = Guarded(torch, data["obs"]), Guarded(torch, data["returns"])
    gi = Guarded(torch, np.ascontiguousarray(idx, np.int32))
    steps, batch = idx.shape
    stats = Guarded(torch, np.full(steps, np.nan, np.float32))
    grads = [Guarded(torch, np.full(pr.SHAPES[k], np.nan, np.float32)) for k in tr.VALUE_KEYS]
    arr = (C.c_void_p * 6)(*[x.ptr for x in grads])
    rc = lib.qst_vf_fit(C.byref(net), obs.ptr, ret.ptr, data["obs"].shape[0], gi.ptr, steps, batch, lr, beta1, beta2, eps,
                        t0, stats.ptr, C.byref(arr) if want_grads else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.qst_last_error()
    torch.cuda.synchronize()
    return {"stats": stats.get("stats"), "grads": {k: x.get("grad " + k) for k, x in zip(tr.VALUE_KEYS, grads)},
            "W": {k: g[k].get(k) for k in KEYS}, "M": {k: gm[k].get("m " + k) for k in KEYS}, "V": {k: gv[k].get("v " + k) for k in KEYS}}


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 128, 256])
def test_value_fit_one_step_against_float64(torch, batch):
    W, data = tr.weights(), tr.rollout()
    M, V = tr.moments()
    idx = np.random.default_rng(300 + batch).permutation(tr.N_ROWS)[:batch].astype(np.int32)[None]
    out = vf_fit(torch, W, M, V, data, idx, t0=6)
    loss, G, E_loss, E_G = tr.vf_backward64(W, data["obs"][idx[0]], data["returns"][idx[0]], with_bound=True)
    within(out["stats"][0], loss, E_loss, "value loss, batch %d" % batch)
    for k in tr.VALUE_KEYS:
        within(out["grads"][k], G[k], E_G[k], "value gradient %s" % k)
    B = tr.vf_update_bound(W, M, V, G, E_G, 7, 1e-3)
    for k in tr.VALUE_KEYS:
        w, m, v = pr.adam64(W[k], M[k], V[k], G[k], 7, 1e-3, tr.VF_BETA1, tr.VF_BETA2, tr.VF_EPS)
        within(out["W"][k], w, B[k][0], "w " + k)
        within(out["M"][k], m, B[k][1], "m " + k)
        within(out["V"][k], v, B[k][2], "v " + k)
    for k in tr.POLICY_KEYS:
        assert same_bits(out["W"][k], np.asarray(W[k], np.float32)) and not out["M"][k].any() and not out["V"][k].any()


def test_value_fit_five_steps_equal_five_launches(torch):
    W, data = tr.weights(), tr.rollout()
    M, V = tr.moments()
    idx = np.stack([np.random.default_rng(400 + s).permutation(tr.N_ROWS)[:33] for s in range(5)]).astype(np.int32)
    one = vf_fit(torch, W, M, V, data, idx, t0=3)
    w, m, v, losses = W, M, V, []
    for s in range(5):
        o = vf_fit(torch, w, m, v, data, idx[s:s + 1], t0=3 + s)
        w, m, v = o["W"], {k: o["M"][k] for k in tr.VALUE_KEYS}, {k: o["V"][k] for k in tr.VALUE_KEYS}
        losses.append(o["stats"][0])
    assert same_bits(one["stats"], np.asarray(losses, np.float32))
    for k in KEYS:
        assert same_bits(one["W"][k], o["W"][k]) and same_bits(one["M"][k], o["M"][k]) and same_bits(one["V"][k], o["V"][k]), k
    for k in tr.VALUE_KEYS:
        assert same_bits(one["grads"][k], o["grads"][k])


# ---------------------------------------------------------------------------------------------------- the Python layer
def _policy(scale=1.0):
    import quadsim_amd as qa
    return qa.ActorCriticPolicy(tr.weights(scale), device="cuda")


def test_policy_step_reaches_predict_and_the_runner(torch):
    """predict_hip and the fused Runner roll-out after trpo_policy_step agree bit for bit with a FRESH policy built from the updated
    weights: the images cached before the update would give the old network, the host copy of logstd the old standard deviation"""
    import quadsim_amd as qa
    from quadsim_amd.policy import _actor_of
    W, data, hp, S = tr.ls_fixture("scaled")
    pol = _policy(0.3)
    noise = torch.randn((4, 8, 4), generator=torch.Generator().manual_seed(1)).cuda()
    obs = torch.as_tensor(data["obs"][:8]).cuda()

    def paths(p):
        env = qa.VecDockingEnv("docking-v0", num_envs=8, seed=3)
        out = [_actor_of(p).predict_hip(env, obs).clone()]
        r = qa.Runner(env=env, model=p, n_steps=4, gamma=0.99, lam=0.98).run(noise=noise)
        out += [r[3].clone(), r[5].clone()]
        env.close()
        return [x.cpu().numpy() for x in out]
    before = paths(pol)                                          # builds and caches every image of the OLD weights
    out = qa.trpo_policy_step(pol, {k: torch.as_tensor(v).cuda() for k, v in data.items()}, **hp)
    assert out["stats"].cpu().numpy()[8] == S["accepted"] == 0
    ref = policy_step(torch, W, data, hp, 0, trace=False)
    for k in tr.POLICY_KEYS:
        assert same_bits(getattr(pol, k).cpu().numpy(), ref["W"][k]), k
    assert same_bits(pol.logstd_host, ref["W"]["logstd"]) and not same_bits(pol.logstd_host, np.asarray(W["logstd"], np.float32))
    after, fresh = paths(pol), paths(qa.ActorCriticPolicy(ref["W"], device="cuda"))
    for x, y, z in zip(before, after, fresh):
        assert same_bits(y, z) and not same_bits(x, y)


def test_trpo_learn_two_updates(torch):
    import quadsim_amd as qa
    from quadsim_amd import trpo
    env = qa.VecDockingEnv("docking-v0", num_envs=8, seed=5)
    model = qa.TRPO(_policy(0.3), env, n_steps=16, vf_batch=32, vf_iters=2)
    logs = model.learn(2 * 128)
    env.close()
    assert len(logs) == 2
    for log in logs:
        assert set(trpo.STAT_NAMES) | {"vf_loss", "explained_variance", "n_updates", "total_timesteps", "fps", "time_elapsed"} <= set(log)
        assert all(np.isfinite(log[k]) for k in trpo.STAT_NAMES + ("vf_loss",))
    assert logs[-1]["total_timesteps"] == 256 and model.policy._trpo_steps == 2 * 2 * 4


def test_trpo_learn_with_an_expert(torch):
    import quadsim_amd as qa
    from quadsim_amd import gail, trpo
    rng = np.random.default_rng(9)
    expert = type("Expert", (), {})()
    expert.obs = torch.as_tensor(rng.standard_normal((64, 12)).astype(np.float32)).cuda()
    expert.actions = torch.as_tensor(rng.uniform(-1, 1, (64, 4)).astype(np.float32)).cuda()
    expert.train_rows = None
    env = qa.VecDockingEnv("docking-v1", num_envs=8, seed=6)
    disc = qa.Discriminator(seed=4, device="cuda")
    w_before = disc.w0.clone()
    model = qa.TRPO(_policy(0.3), env, n_steps=16, vf_batch=32, vf_iters=1, expert_data=expert, discriminator=disc, g_step=2, d_step=1, d_batch=32)
    logs = model.learn(2 * 128)
    env.close()
    assert len(logs) == 1 and logs[0]["total_timesteps"] == 256
    assert set(trpo.STAT_NAMES) | set(gail.DISC_STAT_NAMES) | {"vf_loss", "disc_reward_mean"} <= set(logs[0])
    assert all(np.isfinite(logs[0][k]) for k in trpo.STAT_NAMES + gail.DISC_STAT_NAMES + ("vf_loss", "disc_reward_mean"))
    assert disc.steps == 1 and not torch.equal(disc.w0, w_before)


def test_refusals_come_before_the_gpu(torch):
    import quadsim_amd as qa

    class Env:
        num_envs, device = 8, "cuda"

    shared = qa.ActorCriticPolicy(pr.weight_set("he", "shared"), device="cuda")
    with pytest.raises(ValueError, match="shared"):
        qa.TRPO(shared, Env(), n_steps=16)
    with pytest.raises(ValueError, match="squash"):
        qa.TRPO(qa.ActorCriticPolicy(tr.weights(), device="cuda", squash=True), Env(), n_steps=16)
    with pytest.raises(qa.QuadsimError, match="HIP device"):
        qa.TRPO(qa.ActorCriticPolicy(tr.weights(), device="cpu"), Env(), n_steps=16)
    with pytest.raises(ValueError, match="value batch"):
        qa.TRPO(_policy(), Env(), n_steps=8, vf_batch=128)
