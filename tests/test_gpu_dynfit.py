"""The fit of the learned dynamics net on the device (qsdf_fit of libquadsim_dynfit.so, DynamicsNet.fit) against
tests/dynfit_ref.py.

Every raw call goes through `run`, which puts every tensor the kernel writes (six weights, twelve moments, loss, indices_out,
six gradients) between 256 sentinel bytes on both sides and checks them afterwards.  The buffer is dynfit_ref.buffer(): 300
rows of which 257 are valid, the tail NaN.  What is held:
  one step     every element of the six gradients within grad_bound of backward64 and the loss within its bound (no element
               excluded: tests/test_dynfit_cpu.py holds that no fixture has a pre-activation within its bound of zero), and
               w, m, v after the step within adam_bound of adam64 applied to the device's OWN gradient, from non-zero moments
  many steps   a launch of 5 steps is bit for bit five launches of one and a launch of 3 then one of 2 -- so every step of a
               multi-step launch is a step held as above, with no drift tolerance
  draws        indices_out bit for bit dynfit_ref.indices; the NaN tail is never read
  invariants   a second run on another stream at other addresses gives the same bits; zero padding of the net is invisible
  the planner  DynamicsNet.fit invalidates the packed image: the next plan runs the updated net
  widths       the one-step, multi-step and padding tests also run dense nets at the width edges of dynplan_ref.EDGE_WIDTHS
               (h1 % 4 != 0, widths of 1, every routing edge, both maxima) with dynfit_ref.EDGE_BATCHES
Measured worst ratios are in profiles/dynfit/README.md and profiles/dyn_edges/README.md."""
import ctypes as C

import numpy as np
import pytest

import dynfit_ref as fr
import dynplan_ref as dr
from side_cases import Guarded, same_bits

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
KEYS = fr.GRAD_KEYS
# "it learns": |mean of the last ten losses, float32 numpy - float64| of fit64 measured on the CPU for this very case is 3.05e-7
# (the losses fall from 3.12 to 1.44; profiles/dynfit/README.md); four times that for the device's different summation order
LEARN_MARGIN = 4.0 * 3.05e-7


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def buf(torch):
    x, d = fr.buffer()
    return torch.as_tensor(x).cuda().contiguous(), torch.as_tensor(d).cuda().contiguous()


def run(torch, W, M, V, buf, iters, batch, lr=1e-2, t0=0, seed=SEED, k=3, size=fr.SIZE, indices=None, want_indices=False, want_grads=False,
        stream=None, beta1=fr.BETA1, beta2=fr.BETA2, eps=fr.EPS):
    """qsdf_fit on copies of (W, M, V) -> dict(w, m, v: dicts of numpy arrays, loss, indices, grads)"""
    from quadsim_amd import dynplan
    lib = dynplan.load_fit()
    gw = [Guarded(torch, np.asarray(W[key], np.float32)) for key in KEYS]
    gm = [Guarded(torch, np.asarray(M[key], np.float32)) for key in KEYS]
    gv = [Guarded(torch, np.asarray(V[key], np.float32)) for key in KEYS]
    gg = [Guarded(torch, np.full(W[key].shape, np.nan, np.float32)) for key in KEYS] if want_grads else None
    loss = Guarded(torch, np.full(iters, np.nan, np.float32))
    iout = Guarded(torch, np.full((iters, batch), -1, np.int32)) if want_indices else None
    norm = [torch.as_tensor(np.asarray(a, np.float32)).cuda() for a in (W["in_mean"], dr.rscale(W), W["out_mean"], fr.out_rscale(W))]
    idx = None if indices is None else torch.as_tensor(np.ascontiguousarray(indices, np.int32)).cuda()
    six = lambda gs: (C.c_void_p * 6)(*[g.ptr for g in gs])     # noqa: E731
    net = dynplan.QsdfNet(C.sizeof(dynplan.QsdfNet), W["w1"].shape[0], W["w2"].shape[0], 0, six(gw), six(gm), six(gv),
                          *[t.data_ptr() for t in norm])
    s = stream if stream is not None else torch.cuda.current_stream()
    dynplan.check_fit(lib.qsdf_fit(C.byref(net), buf[0].data_ptr(), buf[1].data_ptr(), buf[0].shape[0], size, iters, batch, lr, beta1,
                                   beta2, eps, t0, seed, k, None if idx is None else idx.data_ptr(), loss.ptr,
                                   None if iout is None else iout.ptr, None if gg is None else six(gg), C.c_void_p(s.cuda_stream)), "qsdf_fit")
    s.synchronize()
    out = {"w": {key: g.get(key) for key, g in zip(KEYS, gw)}, "m": {key: g.get("m " + key) for key, g in zip(KEYS, gm)},
           "v": {key: g.get("v " + key) for key, g in zip(KEYS, gv)}, "loss": loss.get("loss")}
    if want_indices:
        out["indices"] = iout.get("indices_out")
    if want_grads:
        out["grads"] = {key: g.get("grad " + key) for key, g in zip(KEYS, gg)}
    return out


def state_bits_equal(a, b):
    return all(same_bits(a[s][key], b[s][key]) for s in ("w", "m", "v") for key in KEYS)


# ---------------------------------------------------------------------------------------------------- 1, 2: one step
@pytest.mark.parametrize("name", fr.STEP_SETS + fr.EDGE_SETS)
def test_gradients_loss_and_adam_of_one_step(torch, buf, name):
    """the width edges (dynfit_ref.EDGE_SETS) run EDGE_BATCHES: tests/test_dynfit_cpu.py holds that on these very rows every
    gradient slice that only the last unit of a hidden layer reaches is out of bound if left at zero"""
    W = dr.weight_set(name)
    bx, bd = fr.buffer()
    M, V = fr.moments(W)
    worst_g, worst_l, worst_a = 0.0, 0.0, 0.0
    for batch in fr.step_batches(name):
        idx = fr.step_rows(name, batch)
        loss64, G, lb, E = fr.backward64(W, bx[idx[0]], bd[idx[0]], with_bound=True)
        for t0 in (0, 7):
            out = run(torch, W, M, V, buf, 1, batch, lr=1e-2, t0=t0, indices=idx, want_grads=True, want_indices=True)
            what = "%s batch %d t0 %d" % (name, batch, t0)
            assert np.array_equal(out["indices"], idx), what
            for key in KEYS:
                err = np.abs(out["grads"][key].astype(np.float64) - G[key])
                r = float((err / E[key]).max())
                worst_g = max(worst_g, r)
                assert (err <= E[key]).all(), "%s: %d of %d elements of the %s gradient out of bound, worst err / bound %.3g" % (
                    what, int((err > E[key]).sum()), err.size, key, r)
                g = out["grads"][key]
                ref = fr.adam64(W[key], M[key], V[key], g, t0 + 1, 1e-2)
                bounds = fr.adam_bound(W[key], M[key], V[key], g, t0 + 1, 1e-2)
                for s, x64, b in zip("wmv", ref, bounds):
                    e = np.abs(out[s][key].astype(np.float64) - x64)
                    ra = float((e / b).max())
                    worst_a = max(worst_a, ra)
                    assert (e <= b).all(), "%s: %s of %s out of the update bound, worst err / bound %.3g" % (what, s, key, ra)
                # a wrong update is far outside: the step itself is many bounds long
                assert np.median(np.abs(ref[0] - W[key]) / bounds[0]) > 100.0, (what, key)
            rl = abs(float(out["loss"][0]) - loss64) / lb
            worst_l = max(worst_l, rl)
            assert rl <= 1.0, "%s: loss %.9g against %.9g, err / bound %.3g" % (what, out["loss"][0], loss64, rl)
    print("dynfit ratio %s gradients worst err/bound %.3g, loss %.3g, adam %.3g" % (name, worst_g, worst_l, worst_a))
    assert worst_g <= 1.0 and worst_l <= 1.0 and worst_a <= 1.0, (worst_g, worst_l, worst_a)


# ---------------------------------------------------------------------------------------------------- 3: keyed draws
@pytest.mark.parametrize("seed", [SEED, 7])
def test_keyed_draws(torch, buf, seed):
    W = dr.weight_set("he_20_10")
    Z = fr.zero_state(W)
    assert np.isnan(fr.buffer()[0][fr.SIZE:]).all()
    for size in (fr.SIZE, 1):
        for t0 in (0, 5):
            out = run(torch, W, Z, Z, buf, 3, 37, t0=t0, seed=seed, k=9, size=size, want_indices=True)
            ref = np.stack([fr.indices(seed, 9, t0 + i, 37, size) for i in range(3)])
            assert same_bits(out["indices"], ref), (seed, size, t0)
            assert np.isfinite(out["loss"]).all() and all(np.isfinite(out["w"][key]).all() for key in KEYS)
    # explicit indices equal to the keyed draws give the keyed fit, bit for bit
    a = run(torch, W, Z, Z, buf, 3, 37, t0=5, seed=seed, k=9)
    b = run(torch, W, Z, Z, buf, 3, 37, t0=5, seed=1, k=0, indices=np.stack([fr.indices(seed, 9, 5 + i, 37, fr.SIZE) for i in range(3)]))
    assert state_bits_equal(a, b) and same_bits(a["loss"], b["loss"])


# ---------------------------------------------------------------------------------------------------- 3b: the step counter's edge
def test_step_counter_at_its_upper_edge(torch, buf):
    """t0 = 2^31 - 2 is the last step the contract takes (t0 + iters below 2^31): the counter enters the Philox block's upper
    word and, as t = t0 + 1 = 2^31 - 1, Adam's bias correction, where both powers have long underflowed to 0 and lr_t = lr"""
    from quadsim_amd import dynplan
    W = dr.weight_set("he_20_10")
    M, V = fr.moments(W)
    batch, lr = 37, 1e-2
    for t0 in (10 ** 5, 2 ** 31 - 2):
        assert dynplan.check_fit_args(20, 10, fr.CAPACITY, fr.SIZE, 1, batch, lr, t0=t0, seed=SEED, k=9)[7] == t0
        out = run(torch, W, M, V, buf, 1, batch, lr=lr, t0=t0, seed=SEED, k=9, want_indices=True, want_grads=True)
        ref = fr.indices(SEED, 9, t0, batch, fr.SIZE)
        assert same_bits(out["indices"], ref[None]), t0
        assert not np.array_equal(ref, fr.indices(SEED, 9, t0 - 1, batch, fr.SIZE)) and not np.array_equal(ref, fr.indices(SEED, 9, t0 & 0xFFFF, batch, fr.SIZE))
        worst = 0.0
        for key in KEYS:
            g = out["grads"][key]
            x64 = fr.adam64(W[key], M[key], V[key], g, t0 + 1, lr)
            bounds = fr.adam_bound(W[key], M[key], V[key], g, t0 + 1, lr)
            for s, x, b in zip("wmv", x64, bounds):
                e = np.abs(out[s][key].astype(np.float64) - x)
                worst = max(worst, float((e / b).max()))
                assert (e <= b).all(), "t0 %d: %s of %s out of the update bound, worst err / bound %.3g" % (t0, s, key, (e / b).max())
            assert np.median(np.abs(x64[0] - W[key]) / bounds[0]) > 100.0, (t0, key)
        # the gradient itself does not depend on t0: the rows are the reference's, so it is backward64's within grad_bound
        bx, bd = fr.buffer()
        _, G, lb, E = fr.backward64(W, bx[ref], bd[ref], with_bound=True)
        assert fr.relu_edge(W, bx[ref], bd[ref]) == 0                  # grad_bound's condition, on the reference alone
        assert all((np.abs(out["grads"][key] - G[key]) <= E[key]).all() for key in KEYS), t0
        print("dynfit ratio t0 %d adam worst err/bound %.3g" % (t0, worst))
    assert fr.lr_t64(2 ** 31 - 1, lr) == lr


# ---------------------------------------------------------------------------------------------------- 4: one launch = the sequence
@pytest.mark.parametrize("name,batch", [(name, batch) for name in ("he_20_10", "ref_200_100", "he_128_128") for batch in (17, 128)]
                         + [(name, 17) for name in ("edge_21_11", "edge_207_111", "edge_208_112")],
                         ids=lambda v: str(v))
def test_one_launch_equals_the_sequence(torch, buf, name, batch):
    """(the width edges too: five steps in one launch keep the LDS padding of W2 and W3 for the whole call, five launches
    load it again -- equal bits show that the padding stayed harmless)"""
    W = dr.weight_set(name)
    M, V = fr.moments(W)
    whole = run(torch, W, M, V, buf, 5, batch, t0=2)
    st, losses = {"w": W, "m": M, "v": V}, []
    for i in range(5):
        one = run(torch, dict(W, **st["w"]), st["m"], st["v"], buf, 1, batch, t0=2 + i)
        st, losses = one, losses + [one["loss"]]
    assert state_bits_equal(whole, st) and same_bits(whole["loss"], np.concatenate(losses))
    a = run(torch, W, M, V, buf, 3, batch, t0=2)
    b = run(torch, dict(W, **a["w"]), a["m"], a["v"], buf, 2, batch, t0=5)
    assert state_bits_equal(whole, b) and same_bits(whole["loss"], np.concatenate([a["loss"], b["loss"]]))
    assert not same_bits(whole["w"]["w2"], np.asarray(W["w2"]))


# ---------------------------------------------------------------------------------------------------- 5: run twice
def test_run_twice_same_bits_on_another_stream(torch, buf):
    W = dr.weight_set("ref_200_100")
    M, V = fr.moments(W)
    a = run(torch, W, M, V, buf, 4, 100, want_grads=True, want_indices=True)
    dummy = torch.empty(123457, dtype=torch.uint8, device="cuda")      # moves the addresses of everything allocated after it
    b = run(torch, W, M, V, buf, 4, 100, want_grads=True, want_indices=True, stream=torch.cuda.Stream())
    del dummy
    assert state_bits_equal(a, b) and same_bits(a["loss"], b["loss"]) and same_bits(a["indices"], b["indices"])
    assert all(same_bits(a["grads"][key], b["grads"][key]) for key in KEYS)


# ---------------------------------------------------------------------------------------------------- 6: padding
def padding_is_invisible(torch, buf, name, to):
    """three steps on the net and on the net with zero units appended up to `to`: the same bits on the cut, and every padded
    entry of w, m, v and the gradients exactly zero"""
    W = dr.weight_set(name)
    h1, h2 = W["w1"].shape[0], W["w2"].shape[0]
    P = dr.pad_net(W, *to)
    assert (P["w1"].shape[0], P["w2"].shape[0]) == tuple(to) and to[0] >= h1 and to[1] >= h2
    Z, ZP = fr.zero_state(W), fr.zero_state(P)
    a = run(torch, W, Z, Z, buf, 3, 37, want_grads=True)
    b = run(torch, P, ZP, ZP, buf, 3, 37, want_grads=True)
    assert same_bits(a["loss"], b["loss"]), (name, to)
    cut = {"w1": np.s_[:h1], "b1": np.s_[:h1], "w2": np.s_[:h2, :h1], "b2": np.s_[:h2], "w3": np.s_[:, :h2], "b3": np.s_[:]}
    for key in KEYS:
        for s in ("w", "m", "v", "grads"):
            assert same_bits(a[s][key], b[s][key][cut[key]]), (name, to, s, key)
            rest = b[s][key].copy()
            rest[cut[key]] = 0.0
            assert not rest.any(), "%s to %s, %s of %s: a padded entry is not zero" % (name, to, s, key)


def test_padding_is_invisible(torch, buf):
    padding_is_invisible(torch, buf, "he_20_10", (64, 64))
    # the width edges: to the multiple of 4 the kernel rounds to and to the compiled pair; from one unit of layer 2 to the maxima
    padding_is_invisible(torch, buf, "edge_21_11", (24, 12))
    padding_is_invisible(torch, buf, "edge_21_11", (64, 64))
    padding_is_invisible(torch, buf, "edge_129_1", (208, 112))


# ---------------------------------------------------------------------------------------------------- 7: the planner sees the fit
def test_the_planner_sees_the_fit(torch, buf):
    from quadsim_amd import learned_shooting_plan
    import shooting_ref
    W = dr.weight_set("he_20_10")
    net = dr.to_net(W, "cuda")
    before = net.pack().clone()
    versions = [t._version for t in net.parameters()]
    out = net.fit(buf[0], buf[1], fr.SIZE, iters=3, batch=37, lr=1e-2, seed=SEED, return_indices=True, return_grads=True)
    assert net.fit_steps == 3 and [t._version for t in net.parameters()] == versions
    after = net.pack()
    assert not torch.equal(before, after)
    # DynamicsNet.fit is the raw call: same bits (k defaults to fit_steps before the call = 0)
    raw = run(torch, W, fr.zero_state(W), fr.zero_state(W), buf, 3, 37, lr=1e-2, k=0, want_indices=True, want_grads=True)
    assert all(same_bits(getattr(net, key).cpu().numpy(), raw["w"][key]) for key in KEYS)
    assert all(same_bits(net.adam_m[i].cpu().numpy(), raw["m"][key]) and same_bits(net.adam_v[i].cpu().numpy(), raw["v"][key])
               and same_bits(out["grads"][i].cpu().numpy(), raw["grads"][key]) for i, key in enumerate(KEYS))
    assert same_bits(out["loss"].cpu().numpy(), raw["loss"]) and same_bits(out["indices"].cpu().numpy(), raw["indices"])
    # the plan runs the UPDATED net: its first predictions are one float32 model step of the updated weights
    obs = dr.sample_obs(2)
    paths, horizon = 16, 2
    plan = learned_shooting_plan(net, torch.as_tensor(obs).cuda(), horizon, paths, seed=5, k=1, gid0=0, return_traj=True)
    traj = plan["traj"].cpu().numpy()[:, :, 0]
    acts = np.stack([shooting_ref.actions_fast(5, i, 1, paths, horizon) for i in range(2)])[:, :, 0]
    s = np.repeat(obs[:, None, :], paths, axis=1)
    new = dict(W, **raw["w"])
    ref, bound = dr.step64(new, s, acts, with_bound=True)
    assert (np.abs(traj - ref) <= bound).all()
    assert (np.abs(traj.astype(np.float64) - dr.step32(new, s, acts)) <= bound).all()     # step32's own contract: inside the bound
    old = dr.step64(W, s, acts)
    assert (np.abs(traj - old) > 100.0 * bound).any(), "the plan after the fit is the plan of the old weights"
    net.reset_optimizer()
    assert net.fit_steps == 0 and net.adam_m is None


# ---------------------------------------------------------------------------------------------------- 8: it learns
def learn_case():
    """targets = a fixed random linear map of the inputs; he_20_10 with its normalisers; 200 keyed steps of batch 128"""
    W = dr.weight_set("he_20_10")
    x = fr.buffer()[0][:fr.SIZE]
    A = (0.02 * np.random.default_rng(91).standard_normal((16, 12))).astype(np.float32)
    d = (x.astype(np.float64) @ A.astype(np.float64)).astype(np.float32)
    idx = np.stack([fr.indices(SEED, 0, t, 128, fr.SIZE) for t in range(200)])
    return W, x, d, idx


def test_it_learns(torch):
    W, x, d, idx = learn_case()
    Z = fr.zero_state(W)
    out = run(torch, W, Z, Z, (torch.as_tensor(x).cuda(), torch.as_tensor(d).cuda()), 200, 128, lr=1e-3, k=0, want_indices=True)
    assert np.array_equal(out["indices"], idx)
    ref = fr.fit64(W, Z, Z, x, d, idx, lr=1e-3)[3]
    first, last, last64 = float(out["loss"][:10].mean(dtype=np.float64)), float(out["loss"][-10:].mean(dtype=np.float64)), float(ref[-10:].mean())
    print("dynfit learns: first ten %.9g, last ten %.9g, float64 last ten %.9g, margin %.3g" % (first, last, last64, LEARN_MARGIN))
    assert last < first
    assert abs(last - last64) <= LEARN_MARGIN, (last, last64, abs(last - last64), LEARN_MARGIN)
