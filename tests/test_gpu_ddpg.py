"""The DDPG update on the device (qsdd_update of libquadsim_ddpg.so, quadsim_amd.ddpg) against tests/ddpg_ref.py.

Every raw call goes through `run_update`, which puts every tensor the kernels write (24 weights, 24 moments, the statistics, twelve
gradients, the workspace) between 256 sentinel bytes on both sides and checks them afterwards.  What is held:
  one step     every element of the twelve gradients and the four statistics within the derived bounds of step64, and w, m, v of
               both online nets within adam_bound of adam64 applied to the device's OWN gradient, from non-zero moments; 1, 10, 15,
               16, 17, 33 and 256 rows
  targets      the header's formula restated in numpy float32 on the device's own updated online weights, bit for bit, after 1 and
               after 3 steps; tau = 1
  terminal     done = 1 everywhere: target nets of 1e30 change no bit but their own; done = 0: they do
  clamp        rows beyond +-5 act as their clamped copies, bit for bit; obs_clip = inf differs
  ragged       counts inside a call of batch 256 equal one call per step with batch = counts[s], bit for bit
  many steps   5 steps = 2 + 3 = five calls, bit for bit in all 48 tensors and the statistics; another stream
  it learns    the regression case ddpg_ref.learn_case, which test_ddpg_cpu.py holds the float64 reference to first
  wrapper      ddpg_update equals the raw call, bit for bit; torch_ddpg_update within the same bounds
  the loop     DDPG.learn on 16 docking-v0 envs, two cycles, both update paths
Measured worst ratios are in profiles/ddpg/README.md."""
import ctypes as C

import numpy as np
import pytest

import ddpg_ref as dd
from loop_replay import Recorded
from side_cases import Guarded, same_bits

pytestmark = pytest.mark.gpu

KEYS, NETS, ONLINE = dd.KEYS, dd.NETS, ("actor", "critic")
HYPER = dict(gamma=dd.GAMMA, tau=dd.TAU, actor_lr=1e-2, critic_lr=1e-2, obs_clip=dd.OBS_CLIP)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_dev = {}


def dev(torch, a):
    """the device copy of a fixture array (made once; the arrays of ddpg_ref are cached and never change)"""
    if id(a) not in _dev:
        _dev[id(a)] = (a, torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous())
    return _dev[id(a)][1]


def run_update(torch, P, M, V, rp, idx, counts=None, t0=0, want_grads=False, stream=None, beta1=dd.BETA1, beta2=dd.BETA2, eps=dd.EPS, **hyper):
    """qsdd_update on copies of (P, M, V) -> dict(w: {net: {key: array}}, m, v, stats, grads)"""
    from quadsim_amd import ddpg
    lib = ddpg.load_ddpg()
    hp = dict(HYPER, **hyper)
    idx = np.ascontiguousarray(idx, np.int32)
    steps, batch = idx.shape
    gw = {n: [Guarded(torch, np.asarray(P[n][k], np.float32)) for k in KEYS] for n in NETS}
    gm = {n: [Guarded(torch, np.asarray(M[n][k], np.float32)) for k in KEYS] for n in ONLINE}
    gv = {n: [Guarded(torch, np.asarray(V[n][k], np.float32)) for k in KEYS] for n in ONLINE}
    gg = {n: [Guarded(torch, np.full(dd.shapes_of(n)[k], np.nan, np.float32)) for k in KEYS] for n in ONLINE} if want_grads else None
    stats = Guarded(torch, np.full((steps, 4), np.nan, np.float32))
    nbytes = C.c_size_t(0)
    ddpg.check_ddpg(lib.qsdd_workspace_bytes(C.byref(nbytes)), "qsdd_workspace_bytes")
    ws = Guarded(torch, nbytes=nbytes.value)
    assert ws.ptr % 16 == 0
    it = torch.as_tensor(idx).cuda()
    cnt = None if counts is None else torch.as_tensor(np.ascontiguousarray(counts, np.int32)).cuda()
    data = [dev(torch, a) for a in rp]
    ptrs = lambda gs: [g.ptr for g in gs]                                 # noqa: E731
    nets = ddpg.QsddNets(C.sizeof(ddpg.QsddNets), 0, (C.c_void_p * 24)(*[p for n in NETS for p in ptrs(gw[n])]),
                         (C.c_void_p * 12)(*[p for n in ONLINE for p in ptrs(gm[n])]), (C.c_void_p * 12)(*[p for n in ONLINE for p in ptrs(gv[n])]))
    replay = ddpg.QsddReplay(C.sizeof(ddpg.QsddReplay), 0, data[0].shape[0], *[t.data_ptr() for t in data])
    hyp = ddpg.QsddHyper(C.sizeof(ddpg.QsddHyper), 0, hp["gamma"], hp["tau"], hp["actor_lr"], hp["critic_lr"], hp["obs_clip"], beta1, beta2,
                         eps)
    s = stream if stream is not None else torch.cuda.current_stream()
    grads = None if gg is None else (C.c_void_p * 12)(*[p for n in ONLINE for p in ptrs(gg[n])])
    ddpg.check_ddpg(lib.qsdd_update(C.byref(nets), C.byref(replay), it.data_ptr(), None if cnt is None else cnt.data_ptr(), steps, batch,
                                    C.byref(hyp), t0, ws.ptr, nbytes.value, stats.ptr, grads, C.c_void_p(s.cuda_stream)), "qsdd_update")
    s.synchronize()
    ws.get("the workspace")
    out = {"w": {n: {k: g.get("%s %s" % (n, k)) for k, g in zip(KEYS, gw[n])} for n in NETS},
           "m": {n: {k: g.get("m %s %s" % (n, k)) for k, g in zip(KEYS, gm[n])} for n in ONLINE},
           "v": {n: {k: g.get("v %s %s" % (n, k)) for k, g in zip(KEYS, gv[n])} for n in ONLINE}, "stats": stats.get("stats")}
    if want_grads:
        out["grads"] = {n: {k: g.get("grad %s %s" % (n, k)) for k, g in zip(KEYS, gg[n])} for n in ONLINE}
    return out


def tensors_of(out, skip=()):
    return [(p, n, k, out[p][n][k]) for p in ("w", "m", "v") for n in out[p] if n not in skip for k in KEYS]


def state_bits_equal(a, b, skip=()):
    return all(same_bits(x[3], y[3]) for x, y in zip(tensors_of(a, skip), tensors_of(b, skip)))


# ---------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("count", dd.STEP_COUNTS)
def test_one_step_against_float64(torch, count):
    """the twelve gradients, the four statistics and both nets' weights and moments after Adam (t = 7, from non-zero moments): every
    element within its derived bound, none excluded.  Measured worst error / bound on an MI355X, 2026-10-20, over the seven row
    counts: statistics 1.5e-4, gradients 0.028 (actor) / 0.0056 (critic), Adam w / m / v 0.971 / 0.713 / 0.818"""
    P, rp = dd.nets(), dd.replay()
    M, V = dd.moments()
    idx = dd.step_indices(count)
    out = run_update(torch, P, M, V, rp, idx, t0=6, want_grads=True)
    stats, G, _, Es, E = dd.step64(P, tuple(a[idx[0]] for a in rp), with_bound=True)
    worst = {}
    err = np.abs(out["stats"][0].astype(np.float64) - stats)
    for name, e, b in zip(dd.STAT_NAMES, err, Es):
        worst[name] = e / b
    for n in ONLINE:
        for k in KEYS:
            e = np.abs(out["grads"][n][k].astype(np.float64) - G[n][k])
            worst["grad %s %s" % (n, k)] = float((e / E[n][k]).max())
            g = out["grads"][n][k]
            wn, mn, vn = dd.adam64(P[n][k], M[n][k], V[n][k], g, 7, 1e-2)
            for got, want, bound, name in zip((out["w"][n][k], out["m"][n][k], out["v"][n][k]), (wn, mn, vn),
                                              dd.adam_bound(P[n][k], M[n][k], V[n][k], g, 7, 1e-2), "wmv"):
                key = "adam %s %s" % (name, n)
                worst[key] = max(worst.get(key, 0.0), float((np.abs(got.astype(np.float64) - want) / bound).max()))
    for key, ratio in worst.items():
        print("ddpg step rows %d: %s worst error / bound %.3g" % (count, key, ratio))
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r < 1.0}
    assert all(out["w"][n][k].shape == dd.shapes_of(n)[k] for n in NETS for k in KEYS)


# ---------------------------------------------------------------------------------------------------- the targets
def test_targets_are_the_headers_formula_bit_for_bit(torch):
    P, rp = dd.nets(), dd.replay()
    Z = dd.zero_state()
    idx = dd.step_indices(10, steps=3)
    st, tgt = {"w": P, "m": Z, "v": Z}, {n: {k: np.asarray(P[n + "_target"][k]) for k in KEYS} for n in ONLINE}
    for s in range(3):
        st = run_update(torch, st["w"], st["m"], st["v"], rp, idx[s:s + 1], t0=s)
        tgt = {n: {k: dd.polyak32(tgt[n][k], st["w"][n][k]) for k in KEYS} for n in ONLINE}
        if s == 0:
            for n in ONLINE:
                for k in KEYS:
                    assert same_bits(st["w"][n + "_target"][k], tgt[n][k]), (n, k)
                    assert not same_bits(st["w"][n + "_target"][k], P[n + "_target"][k]), (n, k)
    three = run_update(torch, P, Z, Z, rp, idx)
    for n in ONLINE:
        for k in KEYS:
            assert same_bits(three["w"][n + "_target"][k], tgt[n][k]), (n, k)
    for steps in (1, 2):
        one = run_update(torch, P, Z, Z, rp, idx[:steps], tau=1.0)
        assert all(same_bits(one["w"][n + "_target"][k], one["w"][n][k]) for n in ONLINE for k in KEYS)


def test_terminal_rows_never_read_the_target_value(torch):
    P, rp = dd.nets(), dd.replay()
    M, V = dd.moments()
    idx = dd.step_indices(17, steps=2)
    huge = dict(P, critic_target={k: np.full_like(P["critic_target"][k], 1e30) for k in KEYS},
                actor_target={k: (3.0 * P["actor_target"][k]).astype(np.float32) for k in KEYS})
    term = rp[:4] + (np.ones_like(rp[4]),)
    a, b = run_update(torch, P, M, V, term, idx, want_grads=True), run_update(torch, huge, M, V, term, idx, want_grads=True)
    skip = ("actor_target", "critic_target")
    assert state_bits_equal(a, b, skip) and same_bits(a["stats"], b["stats"]) and np.isfinite(a["stats"]).all()
    assert all(same_bits(a["grads"][n][k], b["grads"][n][k]) for n in ONLINE for k in KEYS)
    live = rp[:4] + (np.zeros_like(rp[4]),)
    a, b = run_update(torch, P, M, V, live, idx), run_update(torch, huge, M, V, live, idx)
    assert not same_bits(a["stats"], b["stats"]) and not state_bits_equal(a, b, skip) and np.isfinite(a["stats"]).all()


def test_observations_are_clamped_as_they_are_loaded(torch):
    P, rp = dd.nets(), dd.replay()
    Z = dd.zero_state()
    idx = dd.step_indices(33, steps=2)
    assert (np.abs(rp[0][idx]) > 5.0).any() and (np.abs(rp[3][idx]) > 5.0).any()
    clamped = (np.clip(rp[0], -5.0, 5.0), rp[1], rp[2], np.clip(rp[3], -5.0, 5.0), rp[4])
    a, b = run_update(torch, P, Z, Z, rp, idx, want_grads=True), run_update(torch, P, Z, Z, clamped, idx, want_grads=True)
    assert state_bits_equal(a, b) and same_bits(a["stats"], b["stats"])
    assert all(same_bits(a["grads"][n][k], b["grads"][n][k]) for n in ONLINE for k in KEYS)
    c = run_update(torch, P, Z, Z, rp, idx, obs_clip=float("inf"))
    assert not same_bits(a["stats"], c["stats"]) and not state_bits_equal(a, c)
    assert same_bits(c["stats"], run_update(torch, P, Z, Z, rp, idx, obs_clip=1e30)["stats"])


# ---------------------------------------------------------------------------------------------------- ragged steps, many steps
def test_ragged_counts_equal_the_call_with_that_batch(torch):
    """counts [1, 10, 17] in a call of batch 256: each step is bit for bit the call with batch = counts[s]; the entries at and
    beyond the count hold rows far outside the replay and are never read"""
    P, rp = dd.nets(), dd.replay()
    M, V = dd.moments()
    counts = np.array([1, 10, 17], np.int32)
    idx = dd.step_indices(256, steps=3).copy()
    for s, c in enumerate(counts):
        idx[s, c:] = (1 << 30) if s % 2 else -(1 << 30)
    whole = run_update(torch, P, M, V, rp, idx, counts=counts)
    st = {"w": P, "m": M, "v": V}
    for s, c in enumerate(counts):
        st = run_update(torch, st["w"], st["m"], st["v"], rp, idx[s:s + 1, :c], t0=s)
        assert same_bits(st["stats"][0], whole["stats"][s]), s
    assert state_bits_equal(st, whole) and np.isfinite(whole["stats"]).all()


def test_split_and_stream_invariance(torch):
    """five steps = two then three (t0 carried) = five single calls, and the same on a second stream: all 48 tensors and the
    statistics bit for bit.  The two-step call ends in the workspace's first half, the others in its second"""
    P, rp = dd.nets(), dd.replay()
    M, V = dd.moments()
    idx = dd.step_indices(33, steps=5)
    five = run_update(torch, P, M, V, rp, idx, want_grads=True)
    a = run_update(torch, P, M, V, rp, idx[:2])
    b = run_update(torch, a["w"], a["m"], a["v"], rp, idx[2:], t0=2, want_grads=True)
    assert state_bits_equal(five, b) and same_bits(five["stats"], np.concatenate([a["stats"], b["stats"]]))
    assert all(same_bits(five["grads"][n][k], b["grads"][n][k]) for n in ONLINE for k in KEYS)
    st, stats = {"w": P, "m": M, "v": V}, []
    for s in range(5):
        st = run_update(torch, st["w"], st["m"], st["v"], rp, idx[s:s + 1], t0=s)
        stats.append(st["stats"])
        if s == 1:
            assert state_bits_equal(st, a)
    assert state_bits_equal(five, st) and same_bits(five["stats"], np.concatenate(stats))
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        again = run_update(torch, P, M, V, rp, idx, stream=other)
    assert state_bits_equal(five, again) and same_bits(five["stats"], again["stats"])
    assert np.isfinite(five["stats"]).all() and not same_bits(five["w"]["actor"]["w1"], a["w"]["actor"]["w1"])
    assert all(not same_bits(five[p][n][k], src[n][k]) for p, src in (("w", P), ("m", M), ("v", V)) for n in five[p] for k in KEYS)


def test_the_regression_case_is_learnt(torch):
    """200 steps of batch 16 with every row terminal: the mean critic loss of the last 20 steps is below half that of the first
    20 (the float64 reference reaches a quarter: tests/test_ddpg_cpu.py)"""
    P, rp, idx = dd.learn_case()
    Z = dd.zero_state()
    out = run_update(torch, P, Z, Z, rp, idx, critic_lr=dd.LEARN_CRITIC_LR, actor_lr=dd.LEARN_ACTOR_LR)
    first, last = out["stats"][:20, 0].astype(np.float64).mean(), out["stats"][-20:, 0].astype(np.float64).mean()
    print("ddpg learn device: critic loss first 20 %.4g, last 20 %.4g" % (first, last))
    assert np.isfinite(out["stats"]).all() and last < 0.5 * first


# ---------------------------------------------------------------------------------------------------- the wrappers
def _policy(torch, P, M=None, V=None):
    import quadsim_amd as qa
    pol = qa.DDPGPolicy(device="cuda", weights=P)
    if M is not None:
        for n in ONLINE:
            pol.m[n] = [torch.as_tensor(M[n][k].copy()).cuda() for k in KEYS]
            pol.v[n] = [torch.as_tensor(V[n][k].copy()).cuda() for k in KEYS]
    return pol


def test_wrapper_equals_the_raw_call(torch):
    import quadsim_amd as qa
    P, rp = dd.nets(), dd.replay()
    M, V = dd.moments()
    idx = dd.step_indices(10, steps=4)
    counts = np.array([10, 3, 10, 7], np.int32)
    raw = run_update(torch, P, M, V, rp, idx, counts=counts, t0=5, want_grads=True)
    pol = _policy(torch, P, M, V)
    pol.steps = 5
    out = qa.ddpg_update(pol, tuple(dev(torch, a) for a in rp), torch.as_tensor(idx), torch.as_tensor(counts), return_grads=True, **HYPER)
    torch.cuda.synchronize()
    assert pol.steps == 9 and same_bits(out["stats"].cpu().numpy(), raw["stats"])
    for n in NETS:
        assert all(same_bits(w.cpu().numpy(), raw["w"][n][k]) for k, w in zip(KEYS, getattr(pol, n))), n
    for n in ONLINE:
        assert all(same_bits(t.cpu().numpy(), raw["m"][n][k]) for k, t in zip(KEYS, pol.m[n]))
        assert all(same_bits(t.cpu().numpy(), raw["v"][n][k]) for k, t in zip(KEYS, pol.v[n]))
        assert all(same_bits(g.cpu().numpy(), raw["grads"][n][k]) for k, g in zip(KEYS, out["grads"][n]))
    # a second call continues from the policy's own state and workspace
    qa.ddpg_update(pol, tuple(dev(torch, a) for a in rp), torch.as_tensor(idx[:1]), **HYPER)
    nxt = run_update(torch, raw["w"], raw["m"], raw["v"], rp, idx[:1], t0=9)
    assert pol.steps == 10 and all(same_bits(w.cpu().numpy(), nxt["w"][n][k]) for n in NETS for k, w in zip(KEYS, getattr(pol, n)))


def test_torch_update_is_within_the_bounds_of_the_reference(torch):
    """torch_ddpg_update on the device from the same start: one step's statistics and gradients within the bounds of step64
    (which hold for any summation order), its update within adam_bound of its own gradient"""
    import quadsim_amd as qa
    P, rp = dd.nets(), dd.replay()
    M, V = dd.moments()
    idx = dd.step_indices(33)
    pol = _policy(torch, P, M, V)
    pol.steps = 6
    out = qa.torch_ddpg_update(pol, tuple(dev(torch, a) for a in rp), torch.as_tensor(idx), return_grads=True, **HYPER)
    stats, G, _, Es, E = dd.step64(P, tuple(a[idx[0]] for a in rp), with_bound=True)
    assert np.all(np.abs(out["stats"][0].double().cpu().numpy() - stats) <= Es)
    for n in ONLINE:
        for i, k in enumerate(KEYS):
            g = out["grads"][n][i].cpu().numpy()
            e = np.abs(g.astype(np.float64) - G[n][k])
            assert np.all(e <= E[n][k]), (n, k, (e / E[n][k]).max())
            # (the loop's update has the header's operations in the header's order, library kernels or not: the same bound)
            wn = dd.adam64(P[n][k], M[n][k], V[n][k], g, 7, 1e-2)[0]
            assert np.all(np.abs(getattr(pol, n)[i].cpu().numpy() - wn) <= dd.adam_bound(P[n][k], M[n][k], V[n][k], g, 7, 1e-2)[0]), (n, k)
    assert pol.steps == 7


# ---------------------------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("update", ["hip", "torch"])
def test_learn_fills_the_ring_and_changes_all_four_nets(torch, update):
    import quadsim_amd as qa
    n_envs, roll, cap = 16, 40, 512
    env = Recorded(qa.VecDockingEnv("docking-v0", num_envs=n_envs, seed=7))
    pol = qa.DDPGPolicy(seed=2, device="cuda")
    before = [[w.clone() for w in ws] for ws in pol.nets()]
    model = qa.DDPG(pol, env, nb_rollout_steps=roll, nb_train_steps=5, batch_size=10, buffer_size=cap, random_exploration=0.3,
                    action_noise=qa.OUNoise(n_envs, device="cuda", seed=3), update=update, critic_lr=1e-3, actor_lr=1e-3, tau=0.05)
    logs = model.learn(2 * roll * n_envs)
    assert len(logs) == 2 and pol.steps == 10 and model.num_timesteps == 2 * roll * n_envs and len(env.log) == 2 * roll
    for log in logs:
        assert all(k in log for k in qa.ddpg.DDPG_STAT_NAMES + ("reward_mean", "fps")) and all(np.isfinite(v) for v in log.values()), log
    for ws, ws0 in zip(pol.nets(), before):
        assert all(not torch.equal(w, w0) for w, w0 in zip(ws, ws0))
    # the ring: the last 512 of the 1280 transitions the env returned, each where the wrap puts it
    obs0 = torch.cat([env.first] + [e[1] for e in env.log[:-1]])
    act, obs1 = torch.cat([e[0] for e in env.log]), torch.cat([e[1] for e in env.log])
    rew, done = torch.cat([e[2] for e in env.log]), torch.cat([e[3] for e in env.log]).float()
    total = 2 * roll * n_envs
    rb = model.replay
    assert (rb.size, rb.pos) == (cap, total % cap) and float(act.abs().max()) <= 1.0
    rows = torch.arange(total - cap, total, device=obs0.device)
    for got, want in zip(rb.tensors(), (obs0, act, rew, obs1, done)):
        assert torch.equal(got[rows % cap], want[rows])
    # predict runs the updated actor
    obs = env.first
    fresh = qa.DDPGPolicy(device="cuda", weights={"actor": pol.actor_weights(), "critic": {k: w.cpu().numpy() for k, w in zip(KEYS, pol.critic)}})
    assert torch.equal(pol.predict(obs), fresh.predict(obs)) and not torch.equal(pol.predict(obs), qa.DDPGPolicy(seed=2, device="cuda").predict(obs))
    env.env.close()
