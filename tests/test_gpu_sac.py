"""The SAC update on the device (qss_update of libquadsim_sac.so, quadsim_amd.sac) against tests/sac_ref.py.

Every raw call goes through `run_update`, which puts every tensor the kernels write (30 weights, 48 moments, alpha_state, the
statistics, 24 gradients, the noise that was used, the four traces, the workspace) between 256 sentinel bytes on both sides and
checks them afterwards.  What is held:
  one step     every element of the 24 gradients and the eight statistics within the derived bounds of step64, none excluded; w, m, v
               of the four online nets and log_alpha, its m and v within adam_bound of adam64 applied to the device's OWN gradient,
               from non-zero moments; v_target bit for bit polyak32 of the device's own new value net; y and vb bit for bit the header's
               float32 formula replayed from the device's own traced forward values and logp; logp_out == vlogp_out bit for bit;
               1, 10, 15, 16, 17, 33 and 256 rows
  noise        a keyed call equals the call fed its noise_out; noise_out against float64 Box-Muller on the same Philox words of
               stream 7; the keys depend on (seed, update, slot) alone; slots beyond the count are not written
  twin minimum taken both ways in one fixture; swapping the critics changes no bit of the value branch
  terminal     done = 1 everywhere with a NaN-filled v_target: every other output finite
  invariance   ragged counts, an a + b split and a second stream, bit for bit
  temperature  auto_alpha = 0 leaves alpha_state's bits
  clamp        ls_raw forced below -20 and above 2 on chosen components: exactly zero log-std gradient there, the rest within bound
  saturation   |u| ~ 12, 1 - a^2 = 0 in float32: finite, and within the (large, finite) derived bound, no element excluded
  non-finite   six single poisons go where float64 torch autograd puts them
  it learns    the regression case sac_ref.learn_case, which test_sac_cpu.py holds the float64 reference to first
  wrapper      sac_update equals the raw call, bit for bit; torch_sac_update on the device within the same bounds
  the loop     SAC.learn on 4 docking-v0 envs, both update paths, the first update of each within the bounds
  device math  qss_math: exp over [-20, 2], ln over (1e-6, 2], the Jacobian term over [-12, 12] against float64
Measured worst ratios are in profiles/sac/README.md."""
import ctypes as C

import numpy as np
import pytest

from quadsim_amd import sac as _feature  # noqa: F401  (without the feature nothing of this file is collected)

import sac_ref as sr
from loop_replay import NORMAL_ABS
from side_cases import Guarded, same_bits

pytestmark = pytest.mark.gpu

KEYS, NETS, ONLINE = sr.KEYS, sr.NETS, sr.ONLINE
HYPER = dict(gamma=sr.GAMMA, tau=sr.TAU, lr=1e-2, target_entropy=sr.TARGET_ENTROPY, auto_alpha=1)
f64 = np.float64


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_dev = {}


def dev(torch, a):
    """the device copy of a fixture array (made once; the arrays of sac_ref are cached and never change)"""
    if id(a) not in _dev:
        _dev[id(a)] = (a, torch.as_tensor(np.ascontiguousarray(a)).cuda().contiguous())
    return _dev[id(a)][1]


def run_update(torch, P, M, V, A, rp, idx, counts=None, t0=0, noise=None, seed=0, want_grads=False, want_noise=False, want_trace=False,
               stream=None, beta1=sr.BETA1, beta2=sr.BETA2, eps=sr.EPS, **hyper):
    """qss_update on copies of (P, M, V, A) -> dict(w: {net: {key: array}}, m, v, alpha [3], stats, grads, noise, trace)"""
    from quadsim_amd import sac
    lib = sac.load_sac()
    hp = dict(HYPER, **hyper)
    idx = np.ascontiguousarray(idx, np.int32)
    steps, batch = idx.shape
    gw = {n: [Guarded(torch, np.asarray(P[n][k], np.float32)) for k in KEYS] for n in NETS}
    gm = {n: [Guarded(torch, np.asarray(M[n][k], np.float32)) for k in KEYS] for n in ONLINE}
    gv = {n: [Guarded(torch, np.asarray(V[n][k], np.float32)) for k in KEYS] for n in ONLINE}
    ga = Guarded(torch, np.asarray(A, np.float32))
    gg = {n: [Guarded(torch, np.full(sr.shapes_of(n)[k], np.nan, np.float32)) for k in KEYS] for n in ONLINE} if want_grads else None
    stats = Guarded(torch, np.full((steps, 8), np.nan, np.float32))
    nout = Guarded(torch, np.full((steps, batch, 4), np.nan, np.float32)) if want_noise else None
    gt = {k: Guarded(torch, np.full((steps, batch) + tail, np.nan, np.float32))
          for k, tail in (("logp", ()), ("vlogp", ()), ("act", (4,)), ("fwd", (5,)))} if want_trace else None
    nbytes = C.c_size_t(0)
    sac.check_sac(lib.qss_workspace_bytes(C.byref(nbytes)), "qss_workspace_bytes")
    ws = Guarded(torch, nbytes=nbytes.value)
    assert ws.ptr % 16 == 0 and ws.n == nbytes.value
    it = torch.as_tensor(idx).cuda()
    cnt = None if counts is None else torch.as_tensor(np.ascontiguousarray(counts, np.int32)).cuda()
    nz = None if noise is None else torch.as_tensor(np.ascontiguousarray(noise, np.float32)).cuda()
    assert nz is None or tuple(nz.shape) == (steps, batch, 4)
    data = [dev(torch, a) for a in rp]
    ptrs = lambda gs: [g.ptr for g in gs]                                 # noqa: E731
    nets = sac.QssNets(C.sizeof(sac.QssNets), 0, (C.c_void_p * 30)(*[p for n in NETS for p in ptrs(gw[n])]),
                       (C.c_void_p * 24)(*[p for n in ONLINE for p in ptrs(gm[n])]), (C.c_void_p * 24)(*[p for n in ONLINE for p in ptrs(gv[n])]),
                       ga.ptr)
    replay = sac.QssReplay(C.sizeof(sac.QssReplay), 0, data[0].shape[0], *[t.data_ptr() for t in data])
    hyp = sac.QssHyper(C.sizeof(sac.QssHyper), hp["auto_alpha"], hp["gamma"], hp["tau"], hp["lr"], hp["target_entropy"], beta1, beta2, eps)
    trace = None if gt is None else C.byref(sac.QssTrace(C.sizeof(sac.QssTrace), 0, gt["logp"].ptr, gt["vlogp"].ptr, gt["act"].ptr, gt["fwd"].ptr))
    s = stream if stream is not None else torch.cuda.current_stream()
    grads = None if gg is None else (C.c_void_p * 24)(*[p for n in ONLINE for p in ptrs(gg[n])])
    sac.check_sac(lib.qss_update(C.byref(nets), C.byref(replay), it.data_ptr(), None if cnt is None else cnt.data_ptr(), steps, batch,
                                 C.byref(hyp), t0, None if nz is None else nz.data_ptr(), seed, None if nout is None else nout.ptr,
                                 ws.ptr, nbytes.value, stats.ptr, trace, grads, C.c_void_p(s.cuda_stream)), "qss_update")
    s.synchronize()
    ws.get("the workspace")
    out = {"w": {n: {k: g.get("%s %s" % (n, k)) for k, g in zip(KEYS, gw[n])} for n in NETS},
           "m": {n: {k: g.get("m %s %s" % (n, k)) for k, g in zip(KEYS, gm[n])} for n in ONLINE},
           "v": {n: {k: g.get("v %s %s" % (n, k)) for k, g in zip(KEYS, gv[n])} for n in ONLINE}, "alpha": ga.get("alpha_state"),
           "stats": stats.get("stats")}
    if want_grads:
        out["grads"] = {n: {k: g.get("grad %s %s" % (n, k)) for k, g in zip(KEYS, gg[n])} for n in ONLINE}
    if want_noise:
        out["noise"] = nout.get("noise_out")
    if want_trace:
        out["trace"] = {k: g.get("trace " + k) for k, g in gt.items()}
    return out


def tensors_of(out, skip=()):
    return [(p, n, k, out[p][n][k]) for p in ("w", "m", "v") for n in out[p] if n not in skip for k in KEYS]


def state_bits_equal(a, b, skip=()):
    return all(same_bits(x[3], y[3]) for x, y in zip(tensors_of(a, skip), tensors_of(b, skip))) and same_bits(a["alpha"], b["alpha"])


def rows_of(rp, idx_row):
    return tuple(a[idx_row] for a in rp)


def check_step(out, P, M, V, A, rows, z, t, lr, what, te=sr.TARGET_ENTROPY, gam=sr.GAMMA, tau=sr.TAU, E_zn=0.0):
    """the one-step checks of a call with grads and traces -> {name: worst error / bound}"""
    count = rows[0].shape[0]
    stats, G, aux, Es, E = sr.step64(P, rows, z, la=f64(A[0]), gam=gam, te=te, with_bound=True, E_zn=E_zn)
    # no ratio below is zeroed by an infinite bound: every bound is finite, on the saturated fixture too
    assert np.isfinite(Es).all() and np.isfinite(E["log_alpha"]) and all(np.isfinite(E[n][k]).all() for n in ONLINE for k in KEYS), what
    assert np.isfinite(aux["E_logp"]).all() and np.isfinite(aux["E_a"]).all(), what
    worst = {}
    err = np.abs(out["stats"][0].astype(f64) - stats)
    for name, e, b in zip(sr.STAT_NAMES, err, Es):
        worst[name] = e / b
    for n in ONLINE:
        for k in KEYS:
            g = out["grads"][n][k]
            e = np.abs(g.astype(f64) - G[n][k])
            with np.errstate(invalid="ignore", divide="ignore"):
                worst["grad %s %s" % (n, k)] = float(np.where(e == 0.0, 0.0, e / E[n][k]).max())
            wn, mn, vn = sr.adam64(P[n][k], M[n][k], V[n][k], g, t, lr)
            for got, want, bound, name in zip((out["w"][n][k], out["m"][n][k], out["v"][n][k]), (wn, mn, vn),
                                              sr.adam_bound(P[n][k], M[n][k], V[n][k], g, t, lr), "wmv"):
                key = "adam %s %s" % (name, n)
                worst[key] = max(worst.get(key, 0.0), float((np.abs(got.astype(f64) - want) / bound).max()))
    T = out["trace"]
    lp, fwd = T["logp"][0, :count], T["fwd"][0, :count]
    assert same_bits(lp, T["vlogp"][0, :count]), what
    worst["trace logp"] = float((np.abs(lp.astype(f64) - aux["logp"]) / aux["E_logp"]).max())
    worst["trace act"] = float((np.abs(T["act"][0, :count].astype(f64) - aux["a"]) / aux["E_a"]).max())
    # y and vb: the header's float32 formula on the device's own forward values; v_target: on the device's own new value net
    assert same_bits(fwd[:, 1], sr.y32(rows[2], rows[4], fwd[:, 0], gam)), what
    assert same_bits(fwd[:, 4], sr.vb32(fwd[:, 2], fwd[:, 3], out["stats"][0, 5], lp)), what
    for k in KEYS:
        assert same_bits(out["w"]["v_target"][k], sr.polyak32(P["v_target"][k], out["w"]["v"][k], tau)), (what, k)
    # the temperature: its gradient replayed in float32 from the traced logp, then Adam's bound on it
    acc = np.float32(0.0)
    for v in lp:
        acc = np.float32(acc + np.float32(v + np.float32(te)))
    g32 = -np.float32(acc / np.float32(count))
    worst["grad log_alpha"] = abs(f64(g32) - G["log_alpha"]) / E["log_alpha"]
    want = sr.adam64(A[0], A[1], A[2], g32, t, lr)
    for got, w_, b_, name in zip(out["alpha"], want, sr.adam_bound(A[0], A[1], A[2], g32, t, lr), "wmv"):
        worst["adam %s log_alpha" % name] = float(abs(f64(got) - w_) / b_)
    for key, ratio in worst.items():
        print("sac %s: %s worst error / bound %.3g" % (what, key, ratio))
    return worst


# ---------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("count", sr.STEP_COUNTS)
def test_one_step_against_float64(torch, count):
    """update u = 6 (Adam step 7) from non-zero moments: the 24 gradients, the eight statistics, the four nets' weights and moments and
    alpha_state, every element within its derived bound, none excluded; v_target, y and vb bit for bit.  Measured worst error / bound
    on an MI355X are in profiles/sac/README.md"""
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    idx, z = sr.step_indices(count), sr.noise(1, count)
    out = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, t0=6, noise=z, want_grads=True, want_trace=True)
    worst = check_step(out, P, M, V, sr.ALPHA_STATE, rows_of(rp, idx[0]), z[0], 7, 1e-2, "step rows %d" % count)
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r < 1.0}
    assert all(out["w"][n][k].shape == sr.shapes_of(n)[k] for n in NETS for k in KEYS)
    assert all(np.abs(out["grads"][n][k]).max() > 0.0 for n in ONLINE for k in KEYS)
    assert all(not same_bits(out["w"][n][k], P[n][k]) for n in NETS for k in KEYS) and not same_bits(out["alpha"], sr.ALPHA_STATE)
    if count >= 10:
        fwd = out["trace"]["fwd"][0]
        assert (fwd[:, 2] < fwd[:, 3]).sum() > 0 and (fwd[:, 3] < fwd[:, 2]).sum() > 0       # the twin minimum is taken both ways


# ---------------------------------------------------------------------------------------------------- the noise
def test_noise_sources(torch):
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    idx = sr.step_indices(33, steps=3)
    kw = dict(want_grads=True, want_trace=True)
    # a keyed call equals the call fed its own noise_out
    k1 = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, seed=77, t0=4, want_noise=True, **kw)
    k2 = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, noise=k1["noise"], t0=4, **kw)
    assert state_bits_equal(k1, k2) and same_bits(k1["stats"], k2["stats"])
    assert all(same_bits(k1["grads"][n][k], k2["grads"][n][k]) for n in ONLINE for k in KEYS)
    assert all(same_bits(k1["trace"][k], k2["trace"][k]) for k in k1["trace"]) and same_bits(k1["trace"]["logp"], k1["trace"]["vlogp"])
    want = sr.normals64(77, 4, 3, 33)
    err = float(np.abs(k1["noise"].astype(f64) - want).max())
    print("sac noise_out: max |device - float64 Box-Muller| %.3g (bound %.3g)" % (err, NORMAL_ABS))
    assert err <= NORMAL_ABS and abs(float(k1["noise"].std()) - 1.0) < 0.15
    assert not same_bits(k1["noise"], run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, seed=78, t0=4, want_noise=True)["noise"])
    # the keys: (seed, update index, row slot) alone -- not the batch, not the split of a call, not the replay index
    small = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx[:, :10], seed=77, t0=4, want_noise=True)
    assert same_bits(small["noise"], k1["noise"][:, :10])
    tail = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx[1:], seed=77, t0=5, want_noise=True)
    assert same_bits(tail["noise"], k1["noise"][1:])
    other = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, (idx + 5) % sr.N_ROWS, seed=77, t0=4, want_noise=True)
    assert same_bits(other["noise"], k1["noise"]) and not same_bits(other["stats"], k1["stats"])
    # slots at and beyond the count are not written, in the noise and in every trace
    counts = np.array([33, 5, 16], np.int32)
    rag = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, counts=counts, seed=77, t0=4, want_noise=True, want_trace=True)
    for s, cnt in enumerate(counts):
        assert same_bits(rag["noise"][s, :cnt], k1["noise"][s, :cnt]) and np.isnan(rag["noise"][s, cnt:]).all()
        assert all(np.isfinite(rag["trace"][k][s, :cnt]).all() and np.isnan(rag["trace"][k][s, cnt:]).all() for k in rag["trace"])


# ---------------------------------------------------------------------------------------------------- the twin minimum, terminal rows
def test_twin_minimum_is_taken_both_ways_and_is_symmetric(torch):
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    idx, z = sr.step_indices(33), sr.noise(1, 33)
    a = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, t0=1, noise=z, want_trace=True)
    fwd = a["trace"]["fwd"][0]
    assert (fwd[:, 2] < fwd[:, 3]).sum() > 0 and (fwd[:, 3] < fwd[:, 2]).sum() > 0
    mn = np.minimum(fwd[:, 2], fwd[:, 3])
    assert same_bits(fwd[:, 4], sr.vb32(mn, mn, a["stats"][0, 5], a["trace"]["vlogp"][0]))
    swapped = dict(P, q1=P["q2"], q2=P["q1"])
    Ms, Vs = dict(M, q1=M["q2"], q2=M["q1"]), dict(V, q1=V["q2"], q2=V["q1"])
    b = run_update(torch, swapped, Ms, Vs, sr.ALPHA_STATE, rp, idx, t0=1, noise=z, want_trace=True)
    assert same_bits(a["trace"]["fwd"][0, :, 4], b["trace"]["fwd"][0, :, 4]) and same_bits(a["stats"][0, 2], b["stats"][0, 2])
    assert all(same_bits(a["w"][n][k], b["w"][n][k]) for n in ("v", "v_target") for k in KEYS)
    assert all(same_bits(a["w"]["q1"][k], b["w"]["q2"][k]) and same_bits(a["w"]["q2"][k], b["w"]["q1"][k]) for k in KEYS)
    assert not same_bits(a["stats"][0, 3], b["stats"][0, 3])                      # the actor's loss is on q1 alone


def test_terminal_rows_never_read_the_target_value(torch):
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    idx = sr.step_indices(17, steps=2)
    z = sr.noise_for(idx)
    poisoned = dict(P, v_target={k: np.full_like(P["v_target"][k], np.nan) for k in KEYS})
    term = rp[:4] + (np.ones_like(rp[4]),)
    a = run_update(torch, P, M, V, sr.ALPHA_STATE, term, idx, noise=z, want_grads=True, want_trace=True)
    b = run_update(torch, poisoned, M, V, sr.ALPHA_STATE, term, idx, noise=z, want_grads=True, want_trace=True)
    assert state_bits_equal(a, b, ("v_target",)) and same_bits(a["stats"], b["stats"]) and np.isfinite(b["stats"]).all()
    assert all(same_bits(a["grads"][n][k], b["grads"][n][k]) and np.isfinite(b["grads"][n][k]).all() for n in ONLINE for k in KEYS)
    assert all(np.isfinite(b["trace"][k]).all() for k in b["trace"]) and (b["trace"]["fwd"][..., 0] == 0.0).all()
    assert all(np.isfinite(b[p][n][k]).all() for p in ("w", "m", "v") for n in ONLINE for k in KEYS) and np.isfinite(b["alpha"]).all()
    live = rp[:4] + (np.zeros_like(rp[4]),)
    c = run_update(torch, poisoned, M, V, sr.ALPHA_STATE, live, idx, noise=z)
    # (a live row reads it: y and both critics' losses at once, and through the critics the value's and the actor's a step later)
    assert np.isnan(c["stats"][:, [0, 1, 7]]).all() and np.isfinite(c["stats"][0, 2:7]).all() and np.isnan(c["stats"][1, 2:4]).all()


# ---------------------------------------------------------------------------------------------------- the invariants
def test_split_ragged_and_stream_invariance(torch):
    """five updates = two then three (t0 carried) = five single calls, and the same on a second stream: all 78 tensors, alpha_state
    and the statistics bit for bit; counts [1, 10, 17] in a call of batch 256 equal one call per step with batch = counts[s]"""
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    A = sr.ALPHA_STATE
    idx = sr.step_indices(33, steps=5)
    z = sr.noise_for(idx)
    five = run_update(torch, P, M, V, A, rp, idx, noise=z, want_grads=True)
    a = run_update(torch, P, M, V, A, rp, idx[:2], noise=z[:2])
    b = run_update(torch, a["w"], a["m"], a["v"], a["alpha"], rp, idx[2:], t0=2, noise=z[2:], want_grads=True)
    assert state_bits_equal(five, b) and same_bits(five["stats"], np.concatenate([a["stats"], b["stats"]]))
    assert all(same_bits(five["grads"][n][k], b["grads"][n][k]) for n in ONLINE for k in KEYS)
    st, stats = {"w": P, "m": M, "v": V, "alpha": A}, []
    for s in range(5):
        st = run_update(torch, st["w"], st["m"], st["v"], st["alpha"], rp, idx[s:s + 1], t0=s, noise=z[s:s + 1])
        stats.append(st["stats"])
    assert state_bits_equal(five, st) and same_bits(five["stats"], np.concatenate(stats))
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        again = run_update(torch, P, M, V, A, rp, idx, noise=z, stream=other)
    assert state_bits_equal(five, again) and same_bits(five["stats"], again["stats"]) and np.isfinite(five["stats"]).all()
    assert all(not same_bits(five[p][n][k], src[n][k]) for p, src in (("w", P), ("m", M), ("v", V)) for n in five[p] for k in KEYS)
    # ragged
    counts = np.array([1, 10, 17], np.int32)
    wide = np.full((3, 256), 1 << 30, np.int32)
    zw = np.full((3, 256, 4), np.nan, np.float32)
    for s, c in enumerate(counts):
        wide[s, :c], zw[s, :c] = idx[s, :c], z[s, :c]
    rag = run_update(torch, P, M, V, A, rp, wide, counts=counts, noise=zw)
    st = {"w": P, "m": M, "v": V, "alpha": A}
    for s, c in enumerate(counts):
        st = run_update(torch, st["w"], st["m"], st["v"], st["alpha"], rp, idx[s:s + 1, :c], t0=s, noise=z[s:s + 1, :c])
        assert same_bits(st["stats"][0], rag["stats"][s]), s
    assert state_bits_equal(rag, st)


def test_a_fixed_temperature_keeps_its_bits(torch):
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    idx = sr.step_indices(17, steps=3)
    z = sr.noise_for(idx)
    fixed = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, noise=z, auto_alpha=0)
    assert same_bits(fixed["alpha"], sr.ALPHA_STATE) and len(set(fixed["stats"][:, 5].tolist())) == 1
    assert abs(f64(fixed["stats"][0, 5]) - np.exp(f64(sr.ALPHA_STATE[0]))) <= sr.EXP_REL * np.exp(f64(sr.ALPHA_STATE[0])) + sr.TINY
    learned = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, noise=z)
    assert not same_bits(learned["alpha"], sr.ALPHA_STATE) and same_bits(learned["stats"][0], fixed["stats"][0])
    assert not same_bits(learned["stats"][1], fixed["stats"][1]) and len(set(learned["stats"][:, 5].tolist())) == 3


# ---------------------------------------------------------------------------------------------------- the clamp, saturation
def test_the_clamp_passes_no_gradient_outside_its_range(torch):
    P, rp = sr.nets_log_std(), sr.replay()
    M, V = sr.moments()
    idx, z = sr.step_indices(33), sr.noise_log_std(sr.noise(1, 33))
    out = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, t0=6, noise=z, want_grads=True, want_trace=True)
    g = out["grads"]["actor"]
    assert not g["w2"][:, [4, 6]].any() and not g["b2"][[4, 6]].any()          # exactly zero: +0 or -0
    assert g["w2"][:, [5, 7]].any() and g["b2"][[5, 7]].all() and g["w2"][:, :4].any()
    worst = check_step(out, P, M, V, sr.ALPHA_STATE, rows_of(rp, idx[0]), z[0], 7, 1e-2, "log-std clamped")
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r < 1.0}


def test_a_saturated_sample_stays_finite_and_within_its_bound(torch):
    P, rp = sr.nets_saturated(), sr.replay()
    M, V = sr.moments()
    idx, z = sr.step_indices(33), sr.noise(1, 33)
    out = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, t0=6, noise=z, want_grads=True, want_trace=True)
    a = out["trace"]["act"][0]
    assert (np.abs(a[:, :2]) == 1.0).all() and (np.abs(a[:, 2:]) < 1.0).all()
    assert np.isfinite(out["stats"]).all() and all(np.isfinite(out["trace"][k]).all() for k in out["trace"])
    assert all(np.isfinite(out[p][n][k]).all() for p in ("w", "m", "v", "grads") for n in ONLINE for k in KEYS)
    worst = check_step(out, P, M, V, sr.ALPHA_STATE, rows_of(rp, idx[0]), z[0], 7, 1e-2, "saturated")
    # every bound is finite here too (check_step asserts it): the Jacobian term's is of order one per saturated component, and the
    # actor's and the value net's gradients, logp, vb and the four statistics behind it are held by what follows from that
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), {k: r for k, r in worst.items() if not r < 1.0}
    assert all(0.0 < worst[k] for k in ("actor_loss", "value_loss", "logp_mean", "trace logp", "grad actor w2", "grad actor b2", "grad v w2",
                                         "grad log_alpha", "q1_loss", "grad q1 w1"))
    # the saturated components' own elements: du is exactly 0 there (s2 = 0: jd = 0 and da s2 = 0), dls is -AR gl and not 0
    g = out["grads"]["actor"]
    assert not g["b2"][:2].any() and not g["w2"][:, :2].any() and g["b2"][2:].all()


# ---------------------------------------------------------------------------------------------------- non-finite values
def _poison(which, P, rp, idx, z):
    P, rp, z = {n: {k: P[n][k].copy() for k in KEYS} for n in NETS}, [a.copy() for a in rp], z.copy()
    live = int(np.flatnonzero(rp[4][idx[0]] < 1.0)[0])                           # a slot of step 0 whose row is not terminal
    row = int(idx[0, live])
    if which == "nan-obs":
        rp[0][row, 3] = np.nan
    elif which == "nan-obs1":
        rp[3][row, 5] = np.nan
    elif which == "inf-rew":
        rp[2][row] = np.inf
    elif which == "nan-v-target":
        P["v_target"]["w1"][7, 9] = np.nan
    elif which == "nan-actor":
        P["actor"]["b1"][11] = np.nan
    elif which == "nan-noise":
        z[0, live, 2] = np.nan
    return P, tuple(rp), z


@pytest.mark.parametrize("which", ["nan-obs", "nan-obs1", "inf-rew", "nan-v-target", "nan-actor", "nan-noise"])
def test_non_finite_values_go_where_float64_autograd_puts_them(torch, which):
    """two updates from a single poison: the finiteness of every statistic, of every net and its moments (per net) and of
    alpha_state is that of torch_sac_update in float64 on the host (torch.where for the minimum, the clamp and the terminal rows)"""
    import quadsim_amd as qa
    P0, rp0 = sr.nets(), sr.replay()
    Z = sr.zero_state()
    idx = sr.step_indices(17, steps=2)
    P, rp, z = _poison(which, P0, rp0, idx, sr.noise_for(idx))
    out = run_update(torch, P, Z, Z, sr.ALPHA_STATE, rp, idx, noise=z)
    pol = qa.SACPolicy(device="cpu", weights={n: {k: np.asarray(P[n][k], f64) for k in KEYS} for n in NETS}, dtype="float64")
    pol.alpha_state = torch.as_tensor(sr.ALPHA_STATE.astype(f64))
    ref = qa.torch_sac_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), noise=torch.as_tensor(z), lr=1e-2)
    want_stats = np.isfinite(ref["stats"].numpy())
    assert np.array_equal(np.isfinite(out["stats"]), want_stats), (which, out["stats"], ref["stats"])
    assert not want_stats.all()                                                  # the poison reaches something
    # per net, not per element (rule 2 of quadsim_ddpg.h: the backward masks stay h > 0 ? acc : 0, which turn a NaN activation's term
    # into 0 where autograd's ReLU hands it on)
    got = {n: not all(np.isfinite(out["w"][n][k]).all() for k in KEYS) for n in NETS}
    bad = {n: not all(bool(torch.isfinite(w).all()) for w in getattr(pol, n)) for n in NETS}
    assert got == bad, (which, got, bad)
    for p, ref_p in (("m", pol.m), ("v", pol.v_)):
        got = {n: not all(np.isfinite(out[p][n][k]).all() for k in KEYS) for n in ONLINE}
        assert got == {n: not all(bool(torch.isfinite(t).all()) for t in ref_p[n]) for n in ONLINE}, (which, p, got)
    assert np.array_equal(np.isfinite(out["alpha"]), np.isfinite(pol.alpha_state.numpy())), which


# ---------------------------------------------------------------------------------------------------- it learns
def test_the_regression_case_is_learnt(torch):
    """200 updates of batch 16 on terminal rows: for either critic the mean loss of the last 20 updates is below HALF of that of the
    first 20 (the float64 reference reaches a quarter), and every statistic stays finite"""
    P, rp, idx, z = sr.learn_case()
    Z = sr.zero_state()
    out = run_update(torch, P, Z, Z, [0.0, 0.0, 0.0], rp, idx, noise=z, lr=sr.LEARN_LR)
    assert np.isfinite(out["stats"]).all()
    for c in (0, 1):
        first, last = out["stats"][:20, c].mean(), out["stats"][-20:, c].mean()
        print("sac learn device: q%d loss first 20 %.4g, last 20 %.4g" % (c + 1, first, last))
        assert last < 0.5 * first


# ---------------------------------------------------------------------------------------------------- the wrapper and the loop
def _policy(torch, P, M, V, A, steps):
    import quadsim_amd as qa
    pol = qa.SACPolicy(device="cuda", weights=P)
    for n in ONLINE:
        pol.m[n] = [torch.as_tensor(np.asarray(M[n][k], np.float32).copy()).cuda() for k in KEYS]
        pol.v_[n] = [torch.as_tensor(np.asarray(V[n][k], np.float32).copy()).cuda() for k in KEYS]
    pol.alpha_state = torch.as_tensor(np.asarray(A, np.float32).copy()).cuda()
    pol.steps = steps
    return pol


def test_the_wrapper_is_the_raw_call_and_the_torch_path_is_within_the_bounds(torch):
    import quadsim_amd as qa
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    idx = sr.step_indices(33, steps=3)
    z = sr.noise_for(idx)
    counts = np.array([33, 17, 33], np.int32)
    raw = run_update(torch, P, M, V, sr.ALPHA_STATE, rp, idx, counts=counts, t0=6, noise=z, want_grads=True, want_trace=True, want_noise=True)
    pol = _policy(torch, P, M, V, sr.ALPHA_STATE, 6)
    data = tuple(dev(torch, a) for a in rp)
    cached = pol.actor_as_mlp()
    out = qa.sac_update(pol, data, torch.as_tensor(idx), torch.as_tensor(counts), noise=torch.as_tensor(z).cuda(), lr=1e-2, return_grads=True,
                        return_noise=True, return_trace=True)
    torch.cuda.synchronize()
    assert pol.steps == 9 and same_bits(out["stats"].cpu().numpy(), raw["stats"]) and same_bits(pol.alpha_state.cpu().numpy(), raw["alpha"])
    for n in NETS:
        assert all(same_bits(w.cpu().numpy(), raw["w"][n][k]) for k, w in zip(KEYS, getattr(pol, n))), n
    for n in ONLINE:
        assert all(same_bits(t.cpu().numpy(), raw["m"][n][k]) for k, t in zip(KEYS, pol.m[n])), n
        assert all(same_bits(t.cpu().numpy(), raw["v"][n][k]) for k, t in zip(KEYS, pol.v_[n])), n
        assert all(same_bits(g.cpu().numpy(), raw["grads"][n][k]) for k, g in zip(KEYS, out["grads"][n])), n
    for s, c in enumerate(counts):
        assert same_bits(out["noise"].cpu().numpy()[s, :c], raw["noise"][s, :c])
        assert all(same_bits(out["trace"][k].cpu().numpy()[s, :c], raw["trace"][k][s, :c]) for k in raw["trace"])
    assert pol.actor_as_mlp() is not cached and same_bits(pol.actor_as_mlp()["w2"], raw["w"]["actor"]["w2"][:, :4])
    assert abs(pol.alpha - float(np.exp(f64(raw["alpha"][0])))) < 1e-6
    # the torch path on the device: one step within the bounds of the float64 reference
    tp = _policy(torch, P, M, V, sr.ALPHA_STATE, 6)
    ref = qa.torch_sac_update(tp, data, torch.as_tensor(idx[:1]), noise=torch.as_tensor(z[:1]).cuda(), lr=1e-2, return_grads=True)
    stats, G, aux, Es, E = sr.step64(P, rows_of(rp, idx[0]), z[0], la=f64(sr.ALPHA_STATE[0]), with_bound=True)
    assert np.all(np.abs(ref["stats"][0].double().cpu().numpy() - stats) <= Es)
    for n in ONLINE:
        for k, g in zip(KEYS, ref["grads"][n]):
            assert np.all(np.abs(g.double().cpu().numpy() - G[n][k]) <= E[n][k]), (n, k)
    # a keyed wrapper call draws on stream 7
    kp = _policy(torch, P, M, V, sr.ALPHA_STATE, 4)
    keyed = qa.sac_update(kp, data, torch.as_tensor(idx), seed=77, return_noise=True)
    assert float(np.abs(keyed["noise"].cpu().numpy().astype(f64) - sr.normals64(77, 4, 3, 33)).max()) <= NORMAL_ABS


def test_sac_learn_runs_both_update_paths(torch):
    """SAC.learn on 4 docking-v0 envs: uniform actions for two env steps, then ONE update of batch 8 on the 8 transitions, through the
    device path and through the torch path from the same seed: the same replay and schedule, and the logged statistics of that first
    update of either within the bounds of the float64 reference (the keyed normals of the two paths differ by at most NORMAL_ABS)"""
    import quadsim_amd as qa
    logs, models = {}, {}
    for update in ("hip", "torch"):
        env = qa.VecDockingEnv("docking-v0", num_envs=4, seed=5)
        pol = qa.SACPolicy(seed=9, device=env.device)
        model = qa.SAC(pol, env, learning_starts=8, train_freq=2, gradient_steps=1, batch_size=8, update=update, seed=3, buffer_size=64,
                       learning_rate=1e-2)
        logs[update] = model.learn(8)
        models[update] = model
        assert len(logs[update]) == 1 and pol.steps == 1 and model.num_timesteps == 8 and model.replay.size == 8
        more = model.learn(8)                                                       # past learning_starts: the actor's own samples
        assert len(more) == 1 and pol.steps == 2 and all(np.isfinite(more[0][k]) for k in qa.sac.SAC_STAT_NAMES)
        env.close()
    rp = tuple(t[:8].cpu().numpy() for t in models["hip"].replay.tensors())
    assert all(same_bits(a, t[:8].cpu().numpy()) for a, t in zip(rp, models["torch"].replay.tensors()))
    idx = qa.replay_schedule(8, 1, 8, torch.Generator().manual_seed(3)).numpy()
    fresh = qa.SACPolicy(seed=9, device="cpu")
    P = {n: {k: w.numpy() for k, w in zip(KEYS, getattr(fresh, n))} for n in NETS}
    z = sr.normals64(3, 0, 1, 8)
    stats, _, _, Es, _ = sr.step64(P, rows_of(rp, idx[0]), z[0], la=0.0, with_bound=True, E_zn=NORMAL_ABS)
    for update in ("hip", "torch"):
        got = np.array([logs[update][0][k] for k in qa.sac.SAC_STAT_NAMES])
        print("sac learn %s: first update error / bound %s" % (update, np.abs(got - stats) / Es))
        assert np.all(np.abs(got - stats) <= Es), (update, got, stats, Es)


# ---------------------------------------------------------------------------------------------------- the device's math functions
def test_device_math_sweep(torch):
    """qss_math against float64: exp over [-20, 2] within gail_ref's EXP_REL, ln over (1e-6, 2] within LN_REL (twice the measured
    worst, profiles/sac/README.md), the Jacobian term over [-12, 12] within the bound derived from the tanh's and the ln's (finite everywhere: sac_ref.ARG_FLOOR)"""
    from quadsim_amd import sac
    n = 1 << 16
    sweep = {0: np.linspace(-20.0, 2.0, n), 1: np.concatenate([np.geomspace(1.0e-6, 2.0, n)[1:], 1.0 + np.linspace(-1e-3, 1e-3, 2001)]),
             2: np.linspace(-12.0, 12.0, n)}
    got = {}
    for which, x in sweep.items():
        x32 = x.astype(np.float32)
        g = Guarded(torch, np.full(x32.shape, np.nan, np.float32))
        xin = torch.as_tensor(x32).cuda()
        sac.check_sac(sac.load_sac().qss_math(which, xin.data_ptr(), g.ptr, x32.size, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "qss_math")
        torch.cuda.synchronize()
        got[which] = (x32.astype(f64), g.get("qss_math %d" % which).astype(f64))
    x, y = got[0]
    rel = float((np.abs(y - np.exp(x)) / np.exp(x)).max())
    print("sac math exp: worst relative error %.4g (bound %.4g)" % (rel, sr.EXP_REL))
    assert rel <= sr.EXP_REL
    x, y = got[1]
    want = np.log(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = float(np.where(want == 0.0, np.where(y == 0.0, 0.0, np.inf), np.abs(y - want) / np.abs(want)).max())
    print("sac math ln: worst relative error %.4g (LN_REL %.4g = 2 x %.4g)" % (rel, sr.LN_REL, sr.LN_MEASURED))
    assert rel <= sr.LN_REL
    x, y = got[2]
    a = np.tanh(x)
    s2 = 1.0 - a * a
    E_s2 = sr._rnd(s2, 2.0 * np.abs(a) * sr.TANH_ABS + sr.TANH_ABS ** 2)
    arg = s2 + sr.E6
    want, bound = sr._ln(arg, sr._rnd(arg, E_s2), sr.ARG_FLOOR)
    err = np.abs(y - want)
    small = np.abs(x) <= 3.0
    print("sac math jacobian: worst error / bound %.4g over [-12, 12], %.4g over [-3, 3]; worst error %.4g, worst bound %.4g"
          % (float((err / bound).max()), float((err[small] / bound[small]).max()), float(err.max()), float(bound.max())))
    assert np.isfinite(y).all() and np.isfinite(bound).all() and np.all(err <= bound) and bound[small].max() < 1e-3
    assert np.all(y <= 2.0e-6) and np.all(y >= np.log(sr.E6) * (1.0 + sr.LN_REL))
