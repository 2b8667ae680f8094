"""GAIL's discriminator on the device (qsg_fit, qsg_reward and qsg_math of libquadsim_gail.so, quadsim_amd.gail) against
tests/gail_ref.py.

Every raw call goes through `run_fit` / `run_reward`, which put every tensor the kernels write (six weights, twelve moments, the
statistics, six gradients; reward and logits) between 256 sentinel bytes on both sides and check them afterwards.  What is held:
  device math  tanh, 1 - tanh^2, exp, log, log1p against float64 over the ranges of gail_ref.SWEEPS, at the constants of its bounds
  one step     every element of the six gradients and the five statistics within the derived bounds of backward64, and w, m, v
               after the step within adam_bound of adam64 applied to the device's OWN gradient, from non-zero moments; both
               compiled widths and H = 100 on the 128 instantiation; 1, 15, 16, 17, 33 and 256 rows per class
  ragged       counts inside a larger batch equal one launch per step with batch = counts[s], bit for bit, with the unused index
               entries far out of range
  many steps   5 steps = 2 + 3 = five launches, bit for bit; another stream; duplicate rows; unclipped generator actions
  padding      units beyond H with zero weights have exactly zero gradients, stay zero and change no bit of the others
  it learns    a separable set: float64 first, then the device
  reward       rows either side of the wave's tile of 16 and the workgroup's 64, and a few thousand; saturated logits; the
               [n_envs, n_steps] -> [n_steps, n_envs] output; grid and stream; logits = NULL
  the loop     GailRunner and GAIL.learn on 64 docking-v1 envs x 16 steps x 2 updates, both update paths
Measured worst ratios are in profiles/gail/README.md."""
import ctypes as C

import numpy as np
import pytest

import gail_ref as gr
from side_cases import Guarded, same_bits, six

pytestmark = pytest.mark.gpu

KEYS = gr.KEYS


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_dev = {}


def dev(torch, a):
    """the device copy of a fixture array (made once; the arrays of gail_ref are cached and never change)"""
    if id(a) not in _dev:
        _dev[id(a)] = (a, torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous())
    return _dev[id(a)][1]


def run_fit(torch, W, M, V, gen, exp, mean, rscale, gen_idx, exp_idx, counts=None, lr=1e-2, t0=0, entcoeff=gr.ENTCOEFF, want_grads=False,
            stream=None, beta1=gr.BETA1, beta2=gr.BETA2, eps=gr.EPS):
    """qsg_fit on copies of (W, M, V) -> dict(w, m, v: dicts of numpy arrays, stats, grads)"""
    from quadsim_amd import gail
    lib = gail.load_gail()
    gen_idx, exp_idx = np.ascontiguousarray(gen_idx, np.int32), np.ascontiguousarray(exp_idx, np.int32)
    steps, batch = gen_idx.shape
    assert exp_idx.shape == (steps, batch)
    gw = [Guarded(torch, np.asarray(W[k], np.float32)) for k in KEYS]
    gm = [Guarded(torch, np.asarray(M[k], np.float32)) for k in KEYS]
    gv = [Guarded(torch, np.asarray(V[k], np.float32)) for k in KEYS]
    gg = [Guarded(torch, np.full(np.asarray(W[k]).shape, np.nan, np.float32)) for k in KEYS] if want_grads else None
    stats = Guarded(torch, np.full((steps, 5), np.nan, np.float32))
    gi, ei = torch.as_tensor(gen_idx).cuda(), torch.as_tensor(exp_idx).cuda()
    cnt = None if counts is None else torch.as_tensor(np.ascontiguousarray(counts, np.int32)).cuda()
    mt, rt = dev(torch, mean), dev(torch, rscale)
    go, ga, eo, ea = (dev(torch, a) for a in (gen[0], gen[1], exp[0], exp[1]))
    net = gail.QsgNet(C.sizeof(gail.QsgNet), gr.hidden_of(W), six(gw), six(gm), six(gv), mt.data_ptr(), rt.data_ptr())
    s = stream if stream is not None else torch.cuda.current_stream()
    gail.check_gail(lib.qsg_fit(C.byref(net), go.data_ptr(), ga.data_ptr(), go.shape[0], eo.data_ptr(), ea.data_ptr(), eo.shape[0],
                                gi.data_ptr(), ei.data_ptr(), None if cnt is None else cnt.data_ptr(), steps, batch, entcoeff, lr, beta1,
                                beta2, eps, t0, stats.ptr, None if gg is None else six(gg), C.c_void_p(s.cuda_stream)), "qsg_fit")
    s.synchronize()
    out = {"w": {k: g.get(k) for k, g in zip(KEYS, gw)}, "m": {k: g.get("m " + k) for k, g in zip(KEYS, gm)},
           "v": {k: g.get("v " + k) for k, g in zip(KEYS, gv)}, "stats": stats.get("stats")}
    if want_grads:
        out["grads"] = {k: g.get("grad " + k) for k, g in zip(KEYS, gg)}
    return out


def state_bits_equal(a, b):
    return all(same_bits(a[p][k], b[p][k]) for p in ("w", "m", "v") for k in KEYS)


def run_reward(torch, W, obs, act, mean, rscale, n_envs=0, n_steps=0, grid=0, want_logits=True, stream=None):
    """qsg_reward -> (reward, logits or None) as numpy arrays [rows]"""
    from quadsim_amd import gail
    lib = gail.load_gail()
    ws = [dev(torch, W[k]) for k in KEYS]
    rows = obs.shape[0]
    rew = Guarded(torch, np.full(rows, np.nan, np.float32))
    lg = Guarded(torch, np.full(rows, np.nan, np.float32))
    null = (C.c_void_p * 6)()
    net = gail.QsgNet(C.sizeof(gail.QsgNet), gr.hidden_of(W), (C.c_void_p * 6)(*[w.data_ptr() for w in ws]), null, null,
                      dev(torch, mean).data_ptr(), dev(torch, rscale).data_ptr())
    s = stream if stream is not None else torch.cuda.current_stream()
    gail.check_gail(lib.qsg_reward(C.byref(net), dev(torch, obs).data_ptr(), dev(torch, act).data_ptr(), rows, n_envs, n_steps, rew.ptr,
                                   lg.ptr if want_logits else None, grid, C.c_void_p(s.cuda_stream)), "qsg_reward")
    s.synchronize()
    logits = lg.get("logits")
    if not want_logits:
        assert np.isnan(logits).all(), "logits = NULL, and something was written beside reward"
    return rew.get("reward"), logits if want_logits else None


# ---------------------------------------------------------------------------------------------------- the device math
@pytest.mark.parametrize("name", sorted(gr.SWEEPS))
def test_device_math_sweep(torch, name):
    """the constants of gail_ref's bounds: the device function against float64 on the same float32 inputs, asserted at four times
    the maximum measured over this very sweep (gail_ref.MEASURED)"""
    from quadsim_amd import gail
    lib = gail.load_gail()
    x = gr.sweep_points(name)
    xd = torch.as_tensor(x).cuda()
    y = Guarded(torch, np.full(x.shape, np.nan, np.float32))
    s = torch.cuda.current_stream()
    gail.check_gail(lib.qsg_math(gr.SWEEPS[name][0], xd.data_ptr(), y.ptr, x.shape[0], C.c_void_p(s.cuda_stream)), "qsg_math")
    s.synchronize()
    got = gr.sweep_error(name, x, y.get("y"))
    print("gail math %s: measured maximum %.4g over %d points, constant %.4g" % (name, got, x.shape[0], 4.0 * gr.MEASURED[name]))
    assert got <= 4.0 * gr.MEASURED[name]


# ---------------------------------------------------------------------------------------------------- one step
def check_step(out, W, M, V, gen_rows, exp_rows, mean, rscale, t, lr, what):
    """the device's gradients and statistics within the derived bounds; its update within adam_bound of its own gradient -> the
    worst ratio error / bound"""
    stats, G, Es, E = gr.backward64(W, gen_rows, exp_rows, mean, rscale, with_bound=True)
    worst = 0.0
    for k in KEYS:
        err = np.abs(out["grads"][k].astype(np.float64) - G[k])
        assert np.all(err <= E[k]), "%s: gradient %s off by %.3g of its bound" % (what, k, (err / E[k]).max())
        worst = max(worst, float((err / E[k]).max()))
    err = np.abs(out["stats"][0].astype(np.float64) - stats)
    assert np.all(err <= Es), "%s: statistics %s against %s, bounds %s" % (what, out["stats"][0], stats, Es)
    worst = max(worst, float((err / Es).max()))
    for k in KEYS:
        g = out["grads"][k]
        wn, mn, vn = gr.adam64(W[k], M[k], V[k], g, t, lr)
        Ew, Em, Ev = gr.adam_bound(W[k], M[k], V[k], g, t, lr)
        for got, want, bound, name in ((out["w"][k], wn, Ew, "w"), (out["m"][k], mn, Em, "m"), (out["v"][k], vn, Ev, "v")):
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= bound), "%s: %s of %s off by %.3g of its bound" % (what, name, k, (err / bound).max())
    return worst


@pytest.mark.parametrize("count", gr.STEP_COUNTS)
@pytest.mark.parametrize("hidden", gr.HIDDENS)
def test_gradients_statistics_and_adam_of_one_step(torch, hidden, count):
    W = gr.weights(hidden)
    M, V = gr.moments(W)
    gen, exp, mean, rscale = gr.dataset()
    gi, ei = gr.step_indices(count)
    out = run_fit(torch, W, M, V, gen, exp, mean, rscale, gi, ei, t0=6, want_grads=True)
    worst = check_step(out, W, M, V, (gen[0][gi[0]], gen[1][gi[0]]), (exp[0][ei[0]], exp[1][ei[0]]), mean, rscale, 7, 1e-2,
                       "H %d, %d rows" % (hidden, count))
    assert all(out["w"][k].shape == np.asarray(W[k]).shape for k in KEYS)
    print("gail step H %d rows %d: worst error / bound %.3g" % (hidden, count, worst))


def test_ragged_counts_equal_the_launch_with_that_batch(torch):
    """counts [1, 39, 40, 17] in a launch of batch 40: each step is bit for bit the launch with batch = counts[s]; the entries at
    and beyond the count hold rows far outside both arrays and are never read"""
    W = gr.weights(100)
    M, V = gr.moments(W)
    gen, exp, mean, rscale = gr.dataset()
    counts = np.array([1, 39, 40, 17], np.int32)
    gi, ei = gr.step_indices(40, steps=4)
    gi, ei = gi.copy(), ei.copy()
    for s, c in enumerate(counts):
        gi[s, c:] = 1 << 30
        ei[s, c:] = -(1 << 30)
    whole = run_fit(torch, W, M, V, gen, exp, mean, rscale, gi, ei, counts=counts)
    st = {"w": W, "m": M, "v": V}
    for s, c in enumerate(counts):
        st = run_fit(torch, st["w"], st["m"], st["v"], gen, exp, mean, rscale, gi[s:s + 1, :c], ei[s:s + 1, :c], t0=s)
        assert same_bits(st["stats"][0], whole["stats"][s]), s
    assert state_bits_equal(whole, st)


def test_five_steps_are_two_and_three_and_five_launches_on_any_stream(torch):
    """duplicate rows inside every step (step_indices repeats one); the second stream computes at other addresses"""
    W = gr.weights(100)
    Z = gr.zero_state(W)
    gen, exp, mean, rscale = gr.dataset()
    gi, ei = gr.step_indices(33, steps=5)
    assert all(len(set(r.tolist())) < 33 for r in gi)
    whole = run_fit(torch, W, Z, Z, gen, exp, mean, rscale, gi, ei, want_grads=True)
    a = run_fit(torch, W, Z, Z, gen, exp, mean, rscale, gi[:2], ei[:2])
    b = run_fit(torch, a["w"], a["m"], a["v"], gen, exp, mean, rscale, gi[2:], ei[2:], t0=2, want_grads=True)
    assert state_bits_equal(whole, b) and same_bits(whole["stats"], np.concatenate([a["stats"], b["stats"]]))
    assert all(same_bits(whole["grads"][k], b["grads"][k]) for k in KEYS)
    st, stats = {"w": W, "m": Z, "v": Z}, []
    for s in range(5):
        st = run_fit(torch, st["w"], st["m"], st["v"], gen, exp, mean, rscale, gi[s:s + 1], ei[s:s + 1], t0=s)
        stats.append(st["stats"])
    assert state_bits_equal(whole, st) and same_bits(whole["stats"], np.concatenate(stats))
    other = run_fit(torch, W, Z, Z, gen, exp, mean, rscale, gi, ei, stream=torch.cuda.Stream())
    assert state_bits_equal(whole, other) and same_bits(whole["stats"], other["stats"])
    assert np.isfinite(whole["stats"]).all() and not same_bits(whole["w"]["w1"], np.asarray(W["w1"]))


def test_unclipped_generator_actions_act_as_their_clamped_copies(torch):
    W = gr.weights(64)
    Z = gr.zero_state(W)
    gen, exp, mean, rscale = gr.dataset()
    assert np.abs(gen[1]).max() > 2.5 and (np.abs(gen[1]) > 1.0).mean() > 0.5
    clamped = (gen[0], np.clip(gen[1], -1.0, 1.0))
    gi, ei = gr.step_indices(17, steps=3)
    a = run_fit(torch, W, Z, Z, gen, exp, mean, rscale, gi, ei, want_grads=True)
    b = run_fit(torch, W, Z, Z, clamped, exp, mean, rscale, gi, ei, want_grads=True)
    assert state_bits_equal(a, b) and same_bits(a["stats"], b["stats"]) and all(same_bits(a["grads"][k], b["grads"][k]) for k in KEYS)
    ra = run_reward(torch, W, gen[0], gen[1], mean, rscale)
    rb = run_reward(torch, W, clamped[0], clamped[1], mean, rscale)
    assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1])


def test_zero_padded_units_get_zero_gradients_and_stay_zero(torch):
    """H = 100 widened to H = 128 with zero weights and biases on units 100 .. 127, three steps from zero moments: the padded
    units' gradients, moments and weights are exactly zero after every launch (tanh(0) = 0 forwards nothing and dz = d (w2 dl) = 0
    comes back), and the first hundred units carry the bits of the H = 100 run -- the extra terms of every chain are fma(0, a, s)"""
    W = gr.weights(100)
    P = {k: np.zeros(s, np.float32) for k, s in zip(KEYS, ((16, 128), (128,), (128, 128), (128,), (128, 1), (1,)))}
    cut = {"w0": np.s_[:, :100], "b0": np.s_[:100], "w1": np.s_[:100, :100], "b1": np.s_[:100], "w2": np.s_[:100], "b2": np.s_[:]}
    for k in KEYS:
        P[k][cut[k]] = W[k]
    gen, exp, mean, rscale = gr.dataset()
    gi, ei = gr.step_indices(33, steps=3)
    a = run_fit(torch, W, gr.zero_state(W), gr.zero_state(W), gen, exp, mean, rscale, gi, ei, want_grads=True)
    b = run_fit(torch, P, gr.zero_state(P), gr.zero_state(P), gen, exp, mean, rscale, gi, ei, want_grads=True)
    assert same_bits(a["stats"], b["stats"])
    for k in KEYS:
        for part in ("w", "m", "v", "grads"):
            whole = b[part][k]
            assert same_bits(np.ascontiguousarray(whole[cut[k]]), a[part][k]), (part, k)
            pad = np.ones(whole.shape, bool)
            pad[cut[k]] = False
            assert not whole[pad].any(), "%s of %s: a padded unit moved" % (part, k)
    ra, rb = run_reward(torch, a["w"], gen[0], gen[1], mean, rscale), run_reward(torch, b["w"], gen[0], gen[1], mean, rscale)
    assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1])


# ---------------------------------------------------------------------------------------------------- it learns
def test_the_fit_separates_a_separable_set_as_float64_does(torch):
    gen, exp, mean, rscale, gi, ei = gr.separable_case()
    W = gr.weights(gr.LEARN_HIDDEN, bias=0.0)
    Z = gr.zero_state(W)
    ref = gr.fit64(W, Z, Z, gen, exp, gi, ei, mean, rscale, lr=gr.LEARN_LR)[3]
    total = lambda st: st[:, 0] + st[:, 1] - gr.ENTCOEFF * st[:, 2]       # noqa: E731
    assert ref[-1, 3] == 1.0 and ref[-1, 4] == 1.0 and total(ref)[-1] < total(ref)[0], "the float64 reference does not learn this case"
    out = run_fit(torch, W, Z, Z, gen, exp, mean, rscale, gi, ei, lr=gr.LEARN_LR)
    st = out["stats"].astype(np.float64)
    print("gail learn: total %.6g -> %.6g on the device, %.6g -> %.6g in float64; accuracies %s" % (total(st)[0], total(st)[-1], total(ref)[0],
                                                                                                     total(ref)[-1], st[-1, 3:]))
    assert np.isfinite(st).all() and st[-1, 3] == 1.0 and st[-1, 4] == 1.0 and total(st)[-1] < total(st)[0]


# ---------------------------------------------------------------------------------------------------- the reward
def _reward_rows(n, seed=211):
    key = ("rew", n, seed)
    if key not in gr._cache:
        rng = np.random.default_rng(seed + n)
        gr._cache[key] = (gr.dr.sample_obs(n, seed=seed + n), rng.uniform(-3.0, 3.0, (n, 4)).astype(np.float32))
    return gr._cache[key]


def check_reward(W, obs, act, mean, rscale, reward, logits, what):
    F = gr.forward64(W, obs, act, mean, rscale)
    err = np.abs(logits.astype(np.float64) - F["l"])
    assert np.all(err <= F["E_l"]), "%s: a logit off by %.3g of its bound" % (what, (err / F["E_l"]).max())
    worst = float((err / F["E_l"]).max())
    want, bound = gr.reward64(F["l"]), gr.reward_bound(F["l"], F["E_l"])
    err = np.abs(reward.astype(np.float64) - want)
    assert np.all(np.isfinite(reward)) and np.all(err <= bound), "%s: a reward off by %.3g of its bound" % (what, (err / bound).max())
    return max(worst, float((err / bound).max()))


@pytest.mark.parametrize("rows", [1, 15, 16, 17, 63, 64, 65, 4099])
@pytest.mark.parametrize("hidden", gr.HIDDENS)
def test_reward_and_logits(torch, hidden, rows):
    """rows either side of a wave's tile (16) and of a workgroup's four tiles (64), and enough for several workgroups"""
    W = gr.weights(hidden)
    _, _, mean, rscale = gr.dataset()
    obs, act = _reward_rows(rows)
    reward, logits = run_reward(torch, W, obs, act, mean, rscale)
    worst = check_reward(W, obs, act, mean, rscale, reward, logits, "H %d, %d rows" % (hidden, rows))
    print("gail reward H %d rows %d: worst error / bound %.3g" % (hidden, rows, worst))


def test_saturated_logits_give_finite_rewards_at_both_ends(torch):
    """the last layer scaled until |l| reaches about 30: the reward approaches -log(1e-8) at one end and 0 at the other"""
    W = dict(gr.weights(100))
    _, _, mean, rscale = gr.dataset()
    obs, act = _reward_rows(4099)
    l0 = gr.forward64(W, obs, act, mean, rscale)["l"]
    scale = np.float32(30.0 / np.abs(l0 - l0.mean()).max())
    W["w2"] = (W["w2"] * scale).astype(np.float32)
    W["b2"] = np.float32([-(l0.mean() - np.float64(W["b2"][0])) * scale]).astype(np.float32)
    reward, logits = run_reward(torch, W, obs, act, mean, rscale)
    check_reward(W, obs, act, mean, rscale, reward, logits, "saturated")
    assert logits.max() > 25.0 or logits.min() < -25.0
    assert np.isfinite(reward).all() and reward.max() <= -np.log(1e-8) + 1e-4 and reward.min() >= -1e-6
    big = np.array([[40.0], [-40.0], [100.0], [-100.0]], np.float32)
    Z = {k: np.zeros_like(W[k]) for k in KEYS}
    for b in big:
        Z["b2"] = b
        r, l = run_reward(torch, Z, obs[:3], act[:3], mean, rscale)
        assert np.all(l == b[0]) and np.isfinite(r).all()
        assert abs(r[0] - (-np.log(1e-8) if b[0] > 0 else 0.0)) < 1e-5, (b, r)


@pytest.mark.parametrize("shape", [(3, 5), (1, 7), (65, 2)])
def test_reward_is_written_step_major(torch, shape):
    n_envs, n_steps = shape
    W = gr.weights(100)
    _, _, mean, rscale = gr.dataset()
    obs, act = _reward_rows(n_envs * n_steps)
    flat = run_reward(torch, W, obs, act, mean, rscale)
    tr = run_reward(torch, W, obs, act, mean, rscale, n_envs=n_envs, n_steps=n_steps)
    for a, b in zip(flat, tr):
        assert same_bits(a.reshape(n_envs, n_steps).T, b.reshape(n_steps, n_envs))


def test_reward_bits_do_not_depend_on_grid_stream_or_logits(torch):
    W = gr.weights(100)
    _, _, mean, rscale = gr.dataset()
    obs, act = _reward_rows(4099)
    base = run_reward(torch, W, obs, act, mean, rscale)
    for grid in (1, 3, 65535):
        got = run_reward(torch, W, obs, act, mean, rscale, grid=grid)
        assert same_bits(base[0], got[0]) and same_bits(base[1], got[1]), grid
    other = run_reward(torch, W, obs, act, mean, rscale, stream=torch.cuda.Stream())
    assert same_bits(base[0], other[0]) and same_bits(base[1], other[1])
    alone = run_reward(torch, W, obs, act, mean, rscale, want_logits=False)
    assert same_bits(base[0], alone[0]) and alone[1] is None
    # a row's bits do not depend on the rows beside it
    part = run_reward(torch, W, obs[100:171], act[100:171], mean, rscale)
    assert same_bits(base[0][100:171], part[0]) and same_bits(base[1][100:171], part[1])


def test_wrapper_is_the_raw_call(torch):
    import quadsim_amd as qa
    W = gr.weights(100)
    gen, exp, mean, rscale = gr.dataset()
    d = qa.Discriminator(hidden=100, device="cuda", weights=W)
    d._norm = (dev(torch, mean), dev(torch, rscale))

    class E:
        obs, actions = dev(torch, exp[0]), dev(torch, exp[1])
    gi, ei = gr.step_indices(17, steps=3)
    out = d.fit(dev(torch, gen[0]), dev(torch, gen[1]), E, torch.as_tensor(gi), torch.as_tensor(ei), lr=1e-2, update_stats=False, return_grads=True)
    Z = gr.zero_state(W)
    raw = run_fit(torch, W, Z, Z, gen, exp, mean, rscale, gi, ei, want_grads=True)
    assert d.steps == 3 and same_bits(out["stats"].cpu().numpy(), raw["stats"])
    assert all(same_bits(getattr(d, k).cpu().numpy(), raw["w"][k]) for k in KEYS)
    assert all(same_bits(g.cpu().numpy(), raw["grads"][k]) for g, k in zip(out["grads"], KEYS))
    r, l = d.reward(dev(torch, gen[0]), dev(torch, gen[1]), return_logits=True)
    rr = run_reward(torch, raw["w"], gen[0], gen[1], mean, rscale)
    assert same_bits(r.cpu().numpy(), rr[0]) and same_bits(l.cpu().numpy(), rr[1])
    # with the merge: the statistics of SB2's RunningMeanStd over the rows the schedule touches
    d2 = qa.Discriminator(hidden=100, device="cuda", weights=W)
    d2.fit(dev(torch, gen[0]), dev(torch, gen[1]), E, torch.as_tensor(gi), torch.as_tensor(ei))
    m64, s64 = gr.running_stats([gen[0][gi.reshape(-1)], exp[0][ei.reshape(-1)]])
    np.testing.assert_allclose(d2.stats.mean, m64, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d2.stats.std, s64, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------- the loop
N_ENVS, N_STEPS = 64, 16


@pytest.fixture(scope="module")
def expert(torch):
    import quadsim_amd as qa
    env = qa.VecDockingEnv("docking-v1", num_envs=N_ENVS, seed=11)
    data = qa.record_expert_dataset(env, n_steps=32)
    env.close()
    return qa.ExpertData(data, device="cuda")


def _policy():
    import ppo2_ref as pr
    import quadsim_amd as qa
    return qa.ActorCriticPolicy(pr.weight_set("he", "towers"), device="cuda")


@pytest.mark.parametrize("env_id", ["docking-v1", "docking-v0"])
def test_gail_runner_pays_the_discriminator_and_reports_the_env(torch, expert, env_id):
    """docking-v1 (the spelt-out roll-out: the fused kernel refuses its stored initial states) and docking-v0 (the fused one)"""
    import quadsim_amd as qa
    fused = env_id == "docking-v0"
    disc = qa.Discriminator(seed=3, device="cuda")
    noise = torch.randn((N_STEPS, N_ENVS, 4), generator=torch.Generator().manual_seed(2)).cuda()
    env = qa.VecDockingEnv(env_id, num_envs=N_ENVS, seed=5)
    plain = qa.Runner(env=env, model=_policy(), n_steps=N_STEPS, gamma=0.99, lam=0.95, fused=fused)
    ref = [x.clone() if isinstance(x, torch.Tensor) else x for x in plain.run(noise=noise)]
    ref_ret, ref_len = plain.last_ep_returns, plain.last_ep_lengths
    env.close()
    env = qa.VecDockingEnv(env_id, num_envs=N_ENVS, seed=5)
    pol = _policy()
    runner = qa.GailRunner(discriminator=disc, env=env, model=pol, n_steps=N_STEPS, gamma=0.99, lam=0.95)
    assert runner.fused == fused
    out = runner.run(noise=noise)
    for i in (0, 2, 3, 4, 5, 8):                         # obs, masks, actions, values, neglogp and the TRUE rewards: the plain Runner's
        assert torch.equal(out[i], ref[i]), i
    assert out[7] == ref[7]
    if ref_ret is not None:
        assert torch.equal(runner.last_ep_returns, ref_ret) and torch.equal(runner.last_ep_lengths, ref_len)
    paid = disc.reward(out[0], out[3], n_envs=N_ENVS, n_steps=N_STEPS)
    assert tuple(paid.shape) == (N_STEPS, N_ENVS) and torch.equal(paid, runner.last_reward)
    assert torch.equal(paid, disc.reward(out[0], out[3]).view(N_ENVS, N_STEPS).t())
    # the returns are GAE over what the discriminator paid
    if fused:                                            # the same roll-out once more from a third handle, for its [T, N] arrays
        env.close()
        env = qa.VecDockingEnv(env_id, num_envs=N_ENVS, seed=5)
        env.reset()
        ro = qa.fused_runner_rollout(env, _policy(), N_STEPS, noise=noise, dones_in=torch.zeros(N_ENVS, dtype=torch.uint8, device="cuda"),
                                     env_major=True)
        assert torch.equal(ro["obs"].view(-1, 12), out[0]) and torch.equal(ro["rewards"].t().reshape(-1), out[8])
        gf = qa.gae_and_flatten(env, paid, ro["values"], ro["neglogp"], ro["dones"], ro["last_values"], ro["last_dones"], 0.99, 0.95)
    else:                                                # the loop's last value is policy.value of the last observation
        T = lambda x: x.view(N_ENVS, N_STEPS).t().contiguous()          # noqa: E731
        gf = qa.gae_and_flatten(env, paid, T(out[4]), T(out[5]), T(out[2].to(torch.uint8)), pol.value(runner.obs, runner.states, runner.dones.bool()),
                                runner.dones, 0.99, 0.95)
    assert torch.equal(gf["returns"], out[1]) and not torch.equal(out[1], ref[1])
    env.close()


@pytest.mark.parametrize("update", ["hip", "torch"])
def test_gail_learn_changes_both_nets_and_every_path_runs_the_new_policy(torch, expert, update):
    import quadsim_amd as qa
    from quadsim_amd.policy import _actor_of
    env = qa.VecDockingEnv("docking-v1", num_envs=N_ENVS, seed=7)
    pol = _policy()
    disc = qa.Discriminator(seed=4, device="cuda")
    w_before = {k: getattr(disc, k).clone() for k in KEYS}
    p_before = pol.w1.clone()
    model = qa.GAIL(pol, env, expert, discriminator=disc, d_steps=3, d_batch=64, n_steps=N_STEPS, nminibatches=4, noptepochs=2, update=update,
                    learning_rate=1e-3)
    logs = model.learn(2 * N_ENVS * N_STEPS)
    assert len(logs) == 2 and disc.steps == 6 and pol._ppo_steps == 16
    from quadsim_amd.gail import DISC_STAT_NAMES
    from quadsim_amd.ppo2 import STAT_NAMES
    for log in logs:
        assert all(k in log for k in DISC_STAT_NAMES + tuple(STAT_NAMES) + ("disc_reward_mean", "explained_variance"))
        assert all(np.isfinite(v) for v in log.values()), log
    assert all(not torch.equal(getattr(disc, k), w_before[k]) for k in KEYS) and not torch.equal(pol.w1, p_before)
    assert disc.stats.count == pytest.approx(1e-2 + 2 * 2 * 3 * 64)
    env.close()
    # the updated policy on the device paths: a fresh policy built from the updated weights gives the same bits
    fresh = qa.ActorCriticPolicy({k: getattr(pol, k).cpu().numpy() for k in ("w0", "b0", "w1", "b1", "w2", "b2", "wv0", "bv0", "wv1", "bv1",
                                                                            "wv2", "bv2", "logstd")}, device="cuda")
    noise = torch.randn((N_STEPS, N_ENVS, 4), generator=torch.Generator().manual_seed(8)).cuda()
    got = []
    for p in (pol, fresh):
        env = qa.VecDockingEnv("docking-v0", num_envs=N_ENVS, seed=9)           # the fused Runner's kernel
        obs = env.reset().clone()
        got.append([_actor_of(p).predict_hip(env, obs).clone()] + [x.clone() for x in qa.Runner(env=env, model=p, n_steps=N_STEPS, gamma=0.99,
                                                                                               lam=0.95).run(noise=noise)[:6]])
        env.close()
    assert all(torch.equal(x, y) for x, y in zip(*got))
