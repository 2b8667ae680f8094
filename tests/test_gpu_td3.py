"""The TD3 update on the device (qstd_update of libquadsim_td3.so, quadsim_amd.td3) against tests/td3_ref.py.

Every raw call goes through `run_update`, which puts every tensor the kernels write (36 weights, 36 moments, the statistics, eighteen
gradients, the noise that was used, the workspace) between 256 sentinel bytes on both sides and checks them afterwards.  What is held:
  one step     an actor update: every element of the eighteen gradients and the six statistics within the derived bounds of step64,
               and w, m, v of the three online nets within adam_bound of adam64 applied to the device's OWN gradient, from non-zero
               moments; 1, 10, 15, 16, 17, 33 and 256 rows
  targets      the header's formula restated in numpy float32 on the device's own updated online weights, bit for bit, after 1 and
               after 3 updates; tau = 1
  delay        policy_delay 2 and 3: a critic-only update leaves the actor, its moments and the three targets bit for bit and reports
               actor_loss 0.0; 5 updates = 2 + 3 = five calls with actor_t0 carried, all 72 tensors and the statistics; another stream
  smoothing    sigma = 0 equals zero noise; clipped noise acts as the clipped values; a keyed call equals the call fed its noise_out;
               noise_out against float64 Box-Muller on the same Philox words; the keys depend on (seed, update, slot) alone
  twin minimum swapping the target critics changes nothing; q2_target = q1_target gives the one-critic y restated in numpy float32
  terminal     done = 1 everywhere: target nets of 1e30 change no bit but their own
  ragged       counts inside a call of batch 256 equal one call per step with batch = counts[s], bit for bit
  non-finite   a NaN observation row, an inf reward, a NaN in q2_target only, a NaN weight in the actor over three steps: finiteness
               of the statistics and of every net as float64 torch_td3_update has it; unread rows and earlier steps bit for bit.
               The table of single poisons (every input array, the caller's noise, weights, moments, the target nets live and
               terminal, the actor/critic-only schedule) is tests/nonfinite_cases.py's TD3_CASES, run by tests/test_gpu_nonfinite.py
               through run_update, which takes the workspace's bytes at entry and returns them after the call for that
  it learns    the regression case td3_ref.learn_case, which test_td3_cpu.py holds the float64 reference to first
  wrapper      td3_update equals the raw call, bit for bit; torch_td3_update within the same bounds
  the loop     TD3.learn on 16 docking-v0 envs, two cycles, both update paths
Measured worst ratios are in profiles/td3/README.md."""
import ctypes as C

import numpy as np
import pytest

import mppi_ref
import td3_ref as td
from loop_replay import NORMAL_ABS
from side_cases import Guarded, same_bits

pytestmark = pytest.mark.gpu

KEYS, NETS, ONLINE = td.KEYS, td.NETS, td.ONLINE
HYPER = dict(gamma=td.GAMMA, tau=td.TAU, actor_lr=1e-2, critic_lr=1e-2, policy_delay=td.DELAY, target_policy_noise=td.SIGMA,
             target_noise_clip=td.CLIP)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_dev = {}


def dev(torch, a):
    """the device copy of a fixture array (made once; the arrays of td3_ref are cached and never change)"""
    if id(a) not in _dev:
        _dev[id(a)] = (a, torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous())
    return _dev[id(a)][1]


def run_update(torch, P, M, V, rp, idx, counts=None, t0=0, actor_t0=0, noise=None, seed=0, want_grads=False, want_noise=False, stream=None,
               ws_init=None, beta1=td.BETA1, beta2=td.BETA2, eps=td.EPS, **hyper):
    """qstd_update on copies of (P, M, V) -> dict(w: {net: {key: array}}, m, v, stats, grads, noise, ws: the workspace's bytes after
    the call).  ws_init: the bytes the workspace holds at entry (None: zeros)"""
    from quadsim_amd import td3
    lib = td3.load_td3()
    hp = dict(HYPER, **hyper)
    idx = np.ascontiguousarray(idx, np.int32)
    steps, batch = idx.shape
    gw = {n: [Guarded(torch, np.asarray(P[n][k], np.float32)) for k in KEYS] for n in NETS}
    gm = {n: [Guarded(torch, np.asarray(M[n][k], np.float32)) for k in KEYS] for n in ONLINE}
    gv = {n: [Guarded(torch, np.asarray(V[n][k], np.float32)) for k in KEYS] for n in ONLINE}
    gg = {n: [Guarded(torch, np.full(td.shapes_of(n)[k], np.nan, np.float32)) for k in KEYS] for n in ONLINE} if want_grads else None
    stats = Guarded(torch, np.full((steps, 6), np.nan, np.float32))
    nout = Guarded(torch, np.full((steps, batch, 4), np.nan, np.float32)) if want_noise else None
    nbytes = C.c_size_t(0)
    td3.check_td3(lib.qstd_workspace_bytes(C.byref(nbytes)), "qstd_workspace_bytes")
    ws = Guarded(torch, nbytes=nbytes.value) if ws_init is None else Guarded(torch, np.asarray(ws_init, np.uint8))
    assert ws.ptr % 16 == 0 and ws.n == nbytes.value
    it = torch.as_tensor(idx).cuda()
    cnt = None if counts is None else torch.as_tensor(np.ascontiguousarray(counts, np.int32)).cuda()
    nz = None if noise is None else torch.as_tensor(np.ascontiguousarray(noise, np.float32)).cuda()
    assert nz is None or tuple(nz.shape) == (steps, batch, 4)
    data = [dev(torch, a) for a in rp]
    ptrs = lambda gs: [g.ptr for g in gs]                                 # noqa: E731
    nets = td3.QstdNets(C.sizeof(td3.QstdNets), 0, (C.c_void_p * 36)(*[p for n in NETS for p in ptrs(gw[n])]),
                        (C.c_void_p * 18)(*[p for n in ONLINE for p in ptrs(gm[n])]), (C.c_void_p * 18)(*[p for n in ONLINE for p in ptrs(gv[n])]))
    replay = td3.QstdReplay(C.sizeof(td3.QstdReplay), 0, data[0].shape[0], *[t.data_ptr() for t in data])
    hyp = td3.QstdHyper(C.sizeof(td3.QstdHyper), hp["policy_delay"], hp["gamma"], hp["tau"], hp["actor_lr"], hp["critic_lr"],
                        hp["target_policy_noise"], hp["target_noise_clip"], beta1, beta2, eps)
    s = stream if stream is not None else torch.cuda.current_stream()
    grads = None if gg is None else (C.c_void_p * 18)(*[p for n in ONLINE for p in ptrs(gg[n])])
    td3.check_td3(lib.qstd_update(C.byref(nets), C.byref(replay), it.data_ptr(), None if cnt is None else cnt.data_ptr(), steps, batch,
                                  C.byref(hyp), t0, actor_t0, None if nz is None else nz.data_ptr(), seed, None if nout is None else nout.ptr,
                                  ws.ptr, nbytes.value, stats.ptr, grads, C.c_void_p(s.cuda_stream)), "qstd_update")
    s.synchronize()
    out = {"ws": ws.get("the workspace"), "w": {n: {k: g.get("%s %s" % (n, k)) for k, g in zip(KEYS, gw[n])} for n in NETS},
           "m": {n: {k: g.get("m %s %s" % (n, k)) for k, g in zip(KEYS, gm[n])} for n in ONLINE},
           "v": {n: {k: g.get("v %s %s" % (n, k)) for k, g in zip(KEYS, gv[n])} for n in ONLINE}, "stats": stats.get("stats")}
    if want_grads:
        out["grads"] = {n: {k: g.get("grad %s %s" % (n, k)) for k, g in zip(KEYS, gg[n])} for n in ONLINE}
    if want_noise:
        out["noise"] = nout.get("noise_out")
    return out


def tensors_of(out, skip=()):
    return [(p, n, k, out[p][n][k]) for p in ("w", "m", "v") for n in out[p] if n not in skip for k in KEYS]


def state_bits_equal(a, b, skip=()):
    return all(same_bits(x[3], y[3]) for x, y in zip(tensors_of(a, skip), tensors_of(b, skip)))


def rows_of(rp, idx_row):
    return tuple(a[idx_row] for a in rp)


# ---------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("count", td.STEP_COUNTS)
def test_one_step_against_float64(torch, count):
    """an actor update (u = 6, policy_delay 2; the critics' Adam step 7, the actor's 4, from non-zero moments): the eighteen gradients,
    the six statistics and the three nets' weights and moments, every element within its derived bound, none excluded.  Measured
    worst error / bound on an MI355X, 2026-10-21, over the seven row counts: statistics 3.9e-4, gradients 0.0091 (actor) / 0.0060
    (q1) / 0.0094 (q2), Adam w / m / v 0.977 / 0.721 / 0.796"""
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(count), td.noise(1, count)
    out = run_update(torch, P, M, V, rp, idx, t0=6, actor_t0=3, noise=z, want_grads=True)
    stats, G, _, Es, E = td.step64(P, rows_of(rp, idx[0]), z[0], with_bound=True)
    worst = {}
    err = np.abs(out["stats"][0].astype(np.float64) - stats)
    for name, e, b in zip(td.STAT_NAMES, err, Es):
        worst[name] = e / b
    for n in ONLINE:
        t = 4 if n == "actor" else 7
        for k in KEYS:
            e = np.abs(out["grads"][n][k].astype(np.float64) - G[n][k])
            worst["grad %s %s" % (n, k)] = float((e / E[n][k]).max())
            g = out["grads"][n][k]
            wn, mn, vn = td.adam64(P[n][k], M[n][k], V[n][k], g, t, 1e-2)
            for got, want, bound, name in zip((out["w"][n][k], out["m"][n][k], out["v"][n][k]), (wn, mn, vn),
                                              td.adam_bound(P[n][k], M[n][k], V[n][k], g, t, 1e-2), "wmv"):
                key = "adam %s %s" % (name, n)
                worst[key] = max(worst.get(key, 0.0), float((np.abs(got.astype(np.float64) - want) / bound).max()))
    for key, ratio in worst.items():
        print("td3 step rows %d: %s worst error / bound %.3g" % (count, key, ratio))
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r < 1.0}
    assert all(out["w"][n][k].shape == td.shapes_of(n)[k] for n in NETS for k in KEYS)
    assert all(np.abs(out["grads"][n][k]).max() > 0.0 for n in ONLINE for k in KEYS)


# ---------------------------------------------------------------------------------------------------- the targets
def test_targets_are_the_headers_formula_bit_for_bit(torch):
    P, rp = td.nets(), td.replay()
    Z = td.zero_state()
    idx, z = td.step_indices(10, steps=3), td.noise(3, 10)
    st, tgt = {"w": P, "m": Z, "v": Z}, {n: {k: np.asarray(P[n + "_target"][k]) for k in KEYS} for n in ONLINE}
    for s in range(3):
        st = run_update(torch, st["w"], st["m"], st["v"], rp, idx[s:s + 1], t0=s, actor_t0=s, noise=z[s:s + 1], policy_delay=1)
        tgt = {n: {k: td.polyak32(tgt[n][k], st["w"][n][k], td.TAU) for k in KEYS} for n in ONLINE}
        if s == 0:
            for n in ONLINE:
                for k in KEYS:
                    assert same_bits(st["w"][n + "_target"][k], tgt[n][k]), (n, k)
                    assert not same_bits(st["w"][n + "_target"][k], P[n + "_target"][k]), (n, k)
    three = run_update(torch, P, Z, Z, rp, idx, noise=z, policy_delay=1)
    for n in ONLINE:
        for k in KEYS:
            assert same_bits(three["w"][n + "_target"][k], tgt[n][k]), (n, k)
    for steps in (1, 2):
        one = run_update(torch, P, Z, Z, rp, idx[:steps], noise=z[:steps], tau=1.0, policy_delay=1)
        assert all(same_bits(one["w"][n + "_target"][k], one["w"][n][k]) for n in ONLINE for k in KEYS)


# ---------------------------------------------------------------------------------------------------- the delay
@pytest.mark.parametrize("delay", [2, 3])
def test_a_critic_only_update_leaves_the_actor_and_the_targets(torch, delay):
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(17), td.noise(1, 17)
    out = run_update(torch, P, M, V, rp, idx, t0=1, actor_t0=1, noise=z, policy_delay=delay, want_grads=True)
    for n in ("actor", "actor_target", "q1_target", "q2_target"):
        assert all(same_bits(out["w"][n][k], P[n][k]) for k in KEYS), n
    assert all(same_bits(out["m"]["actor"][k], M["actor"][k]) and same_bits(out["v"]["actor"][k], V["actor"][k]) for k in KEYS)
    assert all(np.isnan(out["grads"]["actor"][k]).all() for k in KEYS)          # not written: no actor step, no actor gradient
    assert out["stats"][0, 5] == 0.0 and not np.signbit(out["stats"][0, 5]) and np.isfinite(out["stats"]).all()
    for n in ("q1", "q2"):
        assert all(not same_bits(out["w"][n][k], P[n][k]) and not same_bits(out["m"][n][k], M[n][k]) for k in KEYS), n
    # the critics' half of the update is that of the actor update from the same state
    stats, G, _, Es, E = td.step64(P, rows_of(rp, idx[0]), z[0], actor=False, with_bound=True)
    assert np.all(np.abs(out["stats"][0].astype(np.float64) - stats)[:5] <= Es[:5])
    assert all(np.all(np.abs(out["grads"][n][k].astype(np.float64) - G[n][k]) <= E[n][k]) for n in ("q1", "q2") for k in KEYS)


def test_delay_split_and_stream_invariance(torch):
    """five updates with policy_delay 2 (actor steps at u = 0, 2, 4) = two then three (t0 and actor_t0 carried) = five single calls,
    and the same on a second stream: all 72 tensors and the statistics bit for bit"""
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(33, steps=5), td.noise(5, 33)
    five = run_update(torch, P, M, V, rp, idx, noise=z, want_grads=True)
    a = run_update(torch, P, M, V, rp, idx[:2], noise=z[:2])
    b = run_update(torch, a["w"], a["m"], a["v"], rp, idx[2:], t0=2, actor_t0=1, noise=z[2:], want_grads=True)
    assert state_bits_equal(five, b) and same_bits(five["stats"], np.concatenate([a["stats"], b["stats"]]))
    assert all(same_bits(five["grads"][n][k], b["grads"][n][k]) for n in ONLINE for k in KEYS)
    wrong = run_update(torch, a["w"], a["m"], a["v"], rp, idx[2:], t0=2, actor_t0=0, noise=z[2:])
    assert not state_bits_equal(five, wrong)                                    # actor_t0 is an argument of its own
    st, stats, taken = {"w": P, "m": M, "v": V}, [], 0
    for s in range(5):
        st = run_update(torch, st["w"], st["m"], st["v"], rp, idx[s:s + 1], t0=s, actor_t0=taken, noise=z[s:s + 1])
        taken += int(td.actor_step(s, 2))
        stats.append(st["stats"])
        if s == 1:
            assert state_bits_equal(st, a)
    assert taken == 3 and state_bits_equal(five, st) and same_bits(five["stats"], np.concatenate(stats))
    assert [float(v) != 0.0 for v in five["stats"][:, 5]] == [True, False, True, False, True]
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        again = run_update(torch, P, M, V, rp, idx, noise=z, stream=other)
    assert state_bits_equal(five, again) and same_bits(five["stats"], again["stats"])
    assert np.isfinite(five["stats"]).all()
    assert all(not same_bits(five[p][n][k], src[n][k]) for p, src in (("w", P), ("m", M), ("v", V)) for n in five[p] for k in KEYS)


# ---------------------------------------------------------------------------------------------------- the smoothing
def test_smoothing_noise_sources(torch):
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(33, steps=3), td.noise(3, 33)
    kw = dict(want_grads=True)
    # sigma = 0: the noise plays no part
    a = run_update(torch, P, M, V, rp, idx, noise=z, target_policy_noise=0.0, **kw)
    b = run_update(torch, P, M, V, rp, idx, noise=np.zeros_like(z), **kw)
    assert state_bits_equal(a, b) and same_bits(a["stats"], b["stats"])
    c = run_update(torch, P, M, V, rp, idx, noise=z, **kw)
    assert not same_bits(a["stats"], c["stats"])
    # clipped rows act as rows fed the clipped values: SIGMA * 2.5 rounds to CL itself
    lim = np.float32(td.CLIP / td.SIGMA)
    assert (np.abs(z) > lim).any() and np.float32(td.SIGMA) * lim == np.float32(td.CLIP)
    d = run_update(torch, P, M, V, rp, idx, noise=np.clip(z, -lim, lim), **kw)
    assert state_bits_equal(c, d) and same_bits(c["stats"], d["stats"])
    assert not same_bits(c["stats"], run_update(torch, P, M, V, rp, idx, noise=z, target_noise_clip=float("inf"))["stats"])
    # a keyed call equals the call fed its own noise_out
    k1 = run_update(torch, P, M, V, rp, idx, seed=77, t0=4, actor_t0=2, want_noise=True, **kw)
    k2 = run_update(torch, P, M, V, rp, idx, noise=k1["noise"], t0=4, actor_t0=2, **kw)
    assert state_bits_equal(k1, k2) and same_bits(k1["stats"], k2["stats"])
    assert all(same_bits(k1["grads"][n][k], k2["grads"][n][k]) for n in ONLINE for k in KEYS)
    want = td.normals64(77, 4, 3, 33)
    err = float(np.abs(k1["noise"].astype(np.float64) - want).max())
    print("td3 noise_out: max |device - float64 Box-Muller| %.3g (bound %.3g)" % (err, NORMAL_ABS))
    assert err <= NORMAL_ABS and abs(float(k1["noise"].std()) - 1.0) < 0.15
    assert not same_bits(k1["noise"], run_update(torch, P, M, V, rp, idx, seed=78, t0=4, actor_t0=2, want_noise=True)["noise"])
    # the keys: (seed, update index, row slot) alone -- not the batch, not the split of a call, not the replay index
    small = run_update(torch, P, M, V, rp, idx[:, :10], seed=77, t0=4, actor_t0=2, want_noise=True)
    assert same_bits(small["noise"], k1["noise"][:, :10])
    tail = run_update(torch, P, M, V, rp, idx[1:], seed=77, t0=5, actor_t0=2, want_noise=True)
    assert same_bits(tail["noise"], k1["noise"][1:])
    other = run_update(torch, P, M, V, rp, (idx + 5) % td.N_ROWS, seed=77, t0=4, actor_t0=2, want_noise=True)
    assert same_bits(other["noise"], k1["noise"]) and not same_bits(other["stats"], k1["stats"])
    # slots at and beyond the count are not written
    counts = np.array([33, 5, 16], np.int32)
    rag = run_update(torch, P, M, V, rp, idx, counts=counts, seed=77, t0=4, actor_t0=2, want_noise=True)["noise"]
    for s, cnt in enumerate(counts):
        assert same_bits(rag[s, :cnt], k1["noise"][s, :cnt]) and np.isnan(rag[s, cnt:]).all()


# ---------------------------------------------------------------------------------------------------- the twin minimum
def _net32(W, x):
    """a critic's forward pass in numpy float32 in the header's order: one fma per term, k ascending from the bias"""
    h = x
    for l in range(3):
        w, b = np.asarray(W["w%d" % l], np.float32), np.asarray(W["b%d" % l], np.float32)
        acc = np.broadcast_to(b[None, :], (h.shape[0], w.shape[1])).astype(np.float32)
        for k in range(w.shape[0]):
            acc = mppi_ref.fma32(np.broadcast_to(w[k][None, :], acc.shape), np.broadcast_to(h[:, k:k + 1], acc.shape), acc)
        h = np.where(acc <= 0.0, np.float32(0.0), acc) if l < 2 else acc
    return h[:, 0]


def test_twin_minimum(torch):
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(33), td.noise(1, 33)
    census = td.edge_census(P, rows_of(rp, idx[0]), z[0])
    assert census["qa<qb"] > 0 and census["qb<qa"] > 0, census
    a = run_update(torch, P, M, V, rp, idx, t0=1, noise=z)
    swapped = dict(P, q1_target=P["q2_target"], q2_target=P["q1_target"])
    b = run_update(torch, swapped, M, V, rp, idx, t0=1, noise=z)
    skip = ("q1_target", "q2_target")
    assert state_bits_equal(a, b, skip) and same_bits(a["stats"], b["stats"])      # y in every bit: both critics regress on it
    one = dict(P, q2_target=P["q1_target"])
    assert not same_bits(a["stats"], run_update(torch, one, M, V, rp, idx, t0=1, noise=z)["stats"])
    # one critic, and a target actor whose head is zero (tanh(0) = 0 exactly): a' = clampsel(SIGMA z), everything after it restated
    flat = dict(one, actor_target=dict(P["actor_target"], w2=np.zeros((128, 4), np.float32), b2=np.zeros(4, np.float32)))
    got = run_update(torch, flat, M, V, rp, idx, t0=1, noise=z)["stats"][0, 4]
    rows = rows_of(rp, idx[0])
    e = np.float32(td.SIGMA) * z[0]
    ap = np.clip(np.clip(e, -np.float32(td.CLIP), np.float32(td.CLIP)), -1.0, 1.0).astype(np.float32)
    q = _net32(P["q1_target"], np.concatenate([rows[3], ap], 1))
    k = ((np.float32(1.0) - rows[4]) * np.float32(td.GAMMA)).astype(np.float32)
    y = np.where(rows[4] >= 1.0, rows[2], mppi_ref.fma32(k, q, rows[2]))
    acc = np.float32(0.0)
    for v in y:
        acc = np.float32(acc + v)
    assert same_bits(np.float32(acc / np.float32(33.0)), got)


def test_terminal_rows_never_read_the_target_value(torch):
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(17, steps=2), td.noise(2, 17)
    huge = dict(P, q1_target={k: np.full_like(P["q1_target"][k], 1e30) for k in KEYS},
                q2_target={k: np.full_like(P["q2_target"][k], 1e30) for k in KEYS},
                actor_target={k: (3.0 * P["actor_target"][k]).astype(np.float32) for k in KEYS})
    term = rp[:4] + (np.ones_like(rp[4]),)
    a, b = run_update(torch, P, M, V, term, idx, noise=z, want_grads=True), run_update(torch, huge, M, V, term, idx, noise=z, want_grads=True)
    skip = ("actor_target", "q1_target", "q2_target")
    assert state_bits_equal(a, b, skip) and same_bits(a["stats"], b["stats"]) and np.isfinite(a["stats"]).all()
    assert all(same_bits(a["grads"][n][k], b["grads"][n][k]) for n in ("q1", "q2") for k in KEYS)
    live = rp[:4] + (np.zeros_like(rp[4]),)
    a, b = run_update(torch, P, M, V, live, idx, noise=z), run_update(torch, huge, M, V, live, idx, noise=z)
    assert not same_bits(a["stats"], b["stats"]) and not state_bits_equal(a, b, skip) and np.isfinite(a["stats"]).all()


# ---------------------------------------------------------------------------------------------------- ragged steps
def test_ragged_counts_equal_the_call_with_that_batch(torch):
    """counts [1, 10, 17] in a call of batch 256: each step is bit for bit the call with batch = counts[s]; the entries at and
    beyond the count hold rows far outside the replay and are never read"""
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    counts = np.array([1, 10, 17], np.int32)
    idx, z = td.step_indices(256, steps=3).copy(), td.noise(3, 256).copy()
    for s, c in enumerate(counts):
        idx[s, c:] = (1 << 30) if s % 2 else -(1 << 30)
        z[s, c:] = np.nan
    whole = run_update(torch, P, M, V, rp, idx, counts=counts, noise=z)
    st, taken = {"w": P, "m": M, "v": V}, 0
    for s, c in enumerate(counts):
        st = run_update(torch, st["w"], st["m"], st["v"], rp, idx[s:s + 1, :c], t0=s, actor_t0=taken, noise=z[s:s + 1, :c])
        taken += int(td.actor_step(s, 2))
        assert same_bits(st["stats"][0], whole["stats"][s]), s
    assert state_bits_equal(st, whole) and np.isfinite(whole["stats"]).all()


# ---------------------------------------------------------------------------------------------------- non-finite values
def _arbiter(torch, P, M, V, rp, idx, z, **kw):
    """float64 torch_td3_update on the host from the same start -> (stats [steps,6], {net: any element non-finite})"""
    import quadsim_amd as qa
    pol = qa.TD3Policy(device="cpu", weights={n: {k: np.asarray(P[n][k], np.float64) for k in KEYS} for n in NETS}, dtype="float64")
    for n in ONLINE:
        pol.m[n] = [torch.as_tensor(np.asarray(M[n][k], np.float64)) for k in KEYS]
        pol.v[n] = [torch.as_tensor(np.asarray(V[n][k], np.float64)) for k in KEYS]
    out = qa.torch_td3_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), noise=torch.as_tensor(z), **dict(HYPER, **kw))
    return out["stats"].numpy(), {n: not all(bool(torch.isfinite(w).all()) for w in getattr(pol, n)) for n in NETS}


def _poisoned(name):
    P, rp = td.nets(), td.replay()
    idx = td.step_indices(17, steps=3).copy()
    idx[idx == 100] = 101
    idx[1, 5] = 100                                                             # row 100 is read by step 1 alone
    rp = tuple(a.copy() for a in rp)
    rp[4][100] = 0.0
    if name == "nan-obs":
        rp[0][100, 3] = np.nan
    elif name == "nan-obs1":
        rp[3][100, 7] = np.nan
    elif name == "inf-rew":
        rp[2][100] = np.inf
    elif name == "nan-q2-target":
        P = dict(P, q2_target=dict(P["q2_target"], w1=P["q2_target"]["w1"].copy()))
        P["q2_target"]["w1"][5, 9] = np.nan
    elif name == "nan-actor":
        P = dict(P, actor=dict(P["actor"], w0=P["actor"]["w0"].copy()))
        P["actor"]["w0"][2, 40] = np.nan
    return P, rp, idx


@pytest.mark.parametrize("name", ["nan-obs", "nan-obs1", "inf-rew", "nan-q2-target", "nan-actor"])
def test_non_finite_values_go_where_float64_autograd_puts_them(torch, name):
    P, rp, idx = _poisoned(name)
    M, V = td.moments()
    z = td.noise(3, 17)
    out = run_update(torch, P, M, V, rp, idx, noise=z)
    with np.errstate(all="ignore"):
        stats, bad = _arbiter(torch, P, M, V, rp, idx, z)
    assert np.array_equal(np.isfinite(out["stats"]), np.isfinite(stats)), (out["stats"], stats)
    assert not np.isfinite(stats).all()
    got = {n: not all(np.isfinite(out["w"][n][k]).all() for k in KEYS) for n in NETS}
    assert got == bad, (got, bad)
    clean_P, clean_rp = td.nets(), td.replay()
    if name in ("nan-obs", "nan-obs1", "inf-rew"):
        # the step before the one that reads the row is bit for bit the clean run's, and so is a run whose poisoned row no index names
        clean_rp = tuple(a.copy() for a in clean_rp)
        clean_rp[4][100] = 0.0
        clean = run_update(torch, clean_P, M, V, clean_rp, idx, noise=z)
        assert same_bits(out["stats"][0], clean["stats"][0]) and not same_bits(out["stats"][1], clean["stats"][1])
        idx2 = idx.copy()
        idx2[1, 5] = 101
        a, b = run_update(torch, P, M, V, rp, idx2, noise=z), run_update(torch, clean_P, M, V, clean_rp, idx2, noise=z)
        assert state_bits_equal(a, b) and same_bits(a["stats"], b["stats"]) and np.isfinite(a["stats"]).all()


# ---------------------------------------------------------------------------------------------------- it learns
def test_the_regression_case_is_learnt(torch):
    """200 updates of batch 16 with every row terminal: for either critic the mean loss of the last 20 updates is below half that of
    the first 20 -- the margin tests/test_gpu_ddpg.py::test_the_regression_case_is_learnt uses (the float64 reference reaches a
    quarter: tests/test_td3_cpu.py)"""
    P, rp, idx, z = td.learn_case()
    Z = td.zero_state()
    out = run_update(torch, P, Z, Z, rp, idx, noise=z, critic_lr=td.LEARN_LR, actor_lr=td.LEARN_LR)
    for c in (0, 1):
        first, last = out["stats"][:20, c].astype(np.float64).mean(), out["stats"][-20:, c].astype(np.float64).mean()
        print("td3 learn device: q%d loss first 20 %.4g, last 20 %.4g" % (c + 1, first, last))
        assert last < 0.5 * first
    assert np.isfinite(out["stats"]).all()


# ---------------------------------------------------------------------------------------------------- the wrappers
def _policy(torch, P, M=None, V=None):
    import quadsim_amd as qa
    pol = qa.TD3Policy(device="cuda", weights=P)
    if M is not None:
        for n in ONLINE:
            pol.m[n] = [torch.as_tensor(M[n][k].copy()).cuda() for k in KEYS]
            pol.v[n] = [torch.as_tensor(V[n][k].copy()).cuda() for k in KEYS]
    return pol


def test_wrapper_equals_the_raw_call(torch):
    import quadsim_amd as qa
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx = td.step_indices(10, steps=5)
    counts = np.array([10, 3, 10, 7, 9], np.int32)
    raw = run_update(torch, P, M, V, rp, idx, counts=counts, t0=5, actor_t0=3, seed=11, want_grads=True, want_noise=True)
    pol = _policy(torch, P, M, V)
    pol.steps, pol.actor_steps = 5, 3
    cached = pol.actor_weights()
    out = qa.td3_update(pol, tuple(dev(torch, a) for a in rp), torch.as_tensor(idx), torch.as_tensor(counts), seed=11, return_grads=True,
                        return_noise=True, **HYPER)
    torch.cuda.synchronize()
    assert pol.steps == 10 and pol.actor_steps == 5 and same_bits(out["stats"].cpu().numpy(), raw["stats"])    # actor steps at u = 6, 8
    assert pol.actor_weights() is not cached and same_bits(pol.actor_weights()["w1"], raw["w"]["actor"]["w1"])
    for s, c in enumerate(counts):
        assert same_bits(out["noise"][s, :c].cpu().numpy(), raw["noise"][s, :c])
    for n in NETS:
        assert all(same_bits(w.cpu().numpy(), raw["w"][n][k]) for k, w in zip(KEYS, getattr(pol, n))), n
    assert out["grads"]["actor"] is None                                        # u = 9 is no actor step
    for n in ONLINE:
        assert all(same_bits(t.cpu().numpy(), raw["m"][n][k]) for k, t in zip(KEYS, pol.m[n]))
        assert all(same_bits(t.cpu().numpy(), raw["v"][n][k]) for k, t in zip(KEYS, pol.v[n]))
        assert n == "actor" or all(same_bits(g.cpu().numpy(), raw["grads"][n][k]) for k, g in zip(KEYS, out["grads"][n]))
    # a second call continues from the policy's own state, counts and workspace
    qa.td3_update(pol, tuple(dev(torch, a) for a in rp), torch.as_tensor(idx[:1]), seed=11, **HYPER)
    nxt = run_update(torch, raw["w"], raw["m"], raw["v"], rp, idx[:1], t0=10, actor_t0=5, seed=11)
    assert pol.steps == 11 and pol.actor_steps == 6
    assert all(same_bits(w.cpu().numpy(), nxt["w"][n][k]) for n in NETS for k, w in zip(KEYS, getattr(pol, n)))


def test_torch_update_is_within_the_bounds_of_the_reference(torch):
    """torch_td3_update on the device from the same start: one actor update's statistics and gradients within the bounds of step64
    (which hold for any summation order), its update within adam_bound of its own gradient"""
    import quadsim_amd as qa
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(33), td.noise(1, 33)
    pol = _policy(torch, P, M, V)
    pol.steps, pol.actor_steps = 6, 3
    out = qa.torch_td3_update(pol, tuple(dev(torch, a) for a in rp), torch.as_tensor(idx), noise=torch.as_tensor(z).cuda(), return_grads=True,
                              **HYPER)
    stats, G, _, Es, E = td.step64(P, rows_of(rp, idx[0]), z[0], with_bound=True)
    assert np.all(np.abs(out["stats"][0].double().cpu().numpy() - stats) <= Es)
    for n in ONLINE:
        t = 4 if n == "actor" else 7
        for i, k in enumerate(KEYS):
            g = out["grads"][n][i].cpu().numpy()
            e = np.abs(g.astype(np.float64) - G[n][k])
            assert np.all(e <= E[n][k]), (n, k, (e / E[n][k]).max())
            wn = td.adam64(P[n][k], M[n][k], V[n][k], g, t, 1e-2)[0]
            assert np.all(np.abs(getattr(pol, n)[i].cpu().numpy() - wn) <= td.adam_bound(P[n][k], M[n][k], V[n][k], g, t, 1e-2)[0]), (n, k)
    assert pol.steps == 7 and pol.actor_steps == 4


# ---------------------------------------------------------------------------------------------------- the loop
def test_learn_runs_both_paths_and_they_agree_on_the_first_update(torch):
    """TD3.learn on 16 docking-v0 envs, two cycles of one update each (u = 0 steps the actor, u = 1 does not), both update paths from
    the same seeds: the replay, the schedule and the noise keys are the same, so the first cycle's statistics are one update's and
    either path's lie within the bounds of step64 on those rows -- with the normals allowed to differ from float64 Box-Muller by
    NORMAL_ABS -- and so within twice the bounds of each other"""
    import quadsim_amd as qa
    n_envs, roll, batch = 16, 20, 64
    res = {}
    for update in ("hip", "torch"):
        env = qa.VecDockingEnv("docking-v0", num_envs=n_envs, seed=7)
        pol = qa.TD3Policy(seed=2, device="cuda")
        P0 = {n: {k: w.cpu().numpy().copy() for k, w in zip(KEYS, getattr(pol, n))} for n in NETS}
        model = qa.TD3(pol, env, learning_starts=roll * n_envs // 2, train_freq=roll, gradient_steps=1, batch_size=batch, buffer_size=1024,
                       action_noise=qa.NormalActionNoise(n_envs, sigma=0.1, device="cuda", seed=3), update=update, seed=5, learning_rate=1e-3)
        logs = model.learn(roll * n_envs)
        first_rows = tuple(t[:roll * n_envs].cpu().numpy().copy() for t in model.replay.tensors())
        logs += model.learn(roll * n_envs)
        assert len(logs) == 2 and pol.steps == 2 and pol.actor_steps == 1 and model.num_timesteps == 2 * roll * n_envs
        for log in logs:
            assert all(k in log for k in qa.td3.TD3_STAT_NAMES + ("reward_mean", "fps")) and all(np.isfinite(v) for v in log.values()), log
        assert logs[0]["actor_loss"] != 0.0 and logs[1]["actor_loss"] == 0.0
        for n in NETS:
            assert all(not torch.equal(w, torch.as_tensor(P0[n][k]).cuda()) for k, w in zip(KEYS, getattr(pol, n))), n
        assert float(model.replay.act.abs().max()) <= 1.0 and model.replay.size == 2 * roll * n_envs
        res[update] = (P0, first_rows, np.array([logs[0][k] for k in td.STAT_NAMES]))
        env.close()
    P0, rows, _ = res["hip"]
    assert all(np.array_equal(a, b) for a, b in zip(rows, res["torch"][1]))     # the same transitions on either path
    idx = qa.replay_schedule(roll * n_envs, 1, batch, torch.Generator().manual_seed(5)).numpy()
    z = td.normals64(5, 0, 1, batch)
    stats, _, _, Es, _ = td.step64(P0, rows_of(rows, idx[0]), z[0], gam=0.99, with_bound=True, E_z=NORMAL_ABS)
    for update in ("hip", "torch"):
        err = np.abs(res[update][2] - stats)
        print("td3 loop %s: first update, worst error / bound %.3g" % (update, float((err / Es).max())))
        assert np.all(err <= Es), (update, err, Es)
