"""The PPO2 update on the device (qsp_update of libquadsim_ppo.so, quadsim_amd.ppo2) against tests/ppo2_ref.py.

Every raw call goes through `run`, which puts every tensor the kernels write (the weights, the moments, the statistics, the
gradients and the workspace) between 256 sentinel bytes on both sides and checks them afterwards.  What is held:
  one step     every element of every gradient (logstd's included) and the six statistics within the derived bounds of
               backward64, and w, m, v after the step within update_bound of update64 applied to the device's OWN gradient, from
               non-zero moments, with the clip active; every weight set x layout x batch 1 / 15 / 16 / 17 / 64 / 300 at slices 1,
               without and with value clipping.  No row is left out: tests/test_ppo2_cpu.py holds the fixtures' conditions
  slices       batch 17 / 33 / 64 / 300 x slices 2 / 3 / 7 / 64 / auto within the same bounds; run twice, the second time on
               another stream, the same bits
  many steps   a 5-step call is five 1-step calls bit for bit, statistics included; the wrapper's split at its maximum
  edges        t0 at its upper edge; the same minibatch as rows of a 300-row and of a 100 000-row data set
  the policy   after ppo2_update every device path runs the new network and the new logstd
  it learns    twenty steps on one minibatch lower the value loss as the float64 reference's do
Measured worst ratios are in profiles/ppo2_update/README.md."""
import ctypes as C

import numpy as np
import pytest

import ppo2_ref as pr
from side_cases import Guarded, same_bits

pytestmark = pytest.mark.gpu

DATA_KEYS = ("obs", "actions", "returns", "values", "neglogp")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_dev = {}


def device_data(torch, data):
    """the roll-out's five arrays on the device, uploaded once per roll-out"""
    key = id(data)
    if key not in _dev:
        _dev[key] = (data, [torch.as_tensor(np.ascontiguousarray(data[k], np.float32)).cuda().contiguous() for k in DATA_KEYS])
    return _dev[key][1]


def thirteen(W, gs):
    keys = pr.keys_of(W)
    return (C.c_void_p * 13)(*[gs[keys.index(k)].ptr if k in keys else None for k in pr.SLOT_KEYS])


def run(torch, W, M, V, data, indices, hp, slices=1, t0=0, want_grads=False, stream=None, beta1=pr.BETA1, beta2=pr.BETA2, eps=pr.EPS):
    """qsp_update on copies of (W, M, V) -> dict(w, m, v: dicts of numpy arrays, stats [steps,6], grads)"""
    from quadsim_amd import _lib, ppo2
    lib = ppo2.load_ppo()
    keys = pr.keys_of(W)
    indices = np.ascontiguousarray(indices, np.int32)
    steps, batch = indices.shape
    gw = [Guarded(torch, np.asarray(W[k], np.float32)) for k in keys]
    gm = [Guarded(torch, np.asarray(M[k], np.float32)) for k in keys]
    gv = [Guarded(torch, np.asarray(V[k], np.float32)) for k in keys]
    gg = [Guarded(torch, np.full(pr.SHAPES[k], np.nan, np.float32)) for k in keys] if want_grads else None
    stats = Guarded(torch, np.full((steps, 6), np.nan, np.float32))
    need = C.c_size_t(0)
    ppo2.check_ppo(lib.qsp_workspace_bytes(batch, slices, C.byref(need)), "qsp_workspace_bytes")
    ws = Guarded(torch, np.zeros(need.value // 8 + 1, np.float64))
    assert ws.ptr % 8 == 0
    dev = device_data(torch, data)
    idx = torch.as_tensor(indices).cuda()
    net = _lib.QspNet(C.sizeof(_lib.QspNet), 1 if "wv0" in W else 0, thirteen(W, gw), thirteen(W, gm), thirteen(W, gv))
    bat = _lib.QspBatch(C.sizeof(_lib.QspBatch), 0, dev[0].shape[0], *[t.data_ptr() for t in dev])
    hyp = _lib.QspHyper(C.sizeof(_lib.QspHyper), 0, hp["lr"], hp["cliprange"], hp["cliprange_vf"], hp["ent_coef"], hp["vf_coef"],
                        hp["max_grad_norm"], beta1, beta2, eps)
    s = stream if stream is not None else torch.cuda.current_stream()
    ppo2.check_ppo(lib.qsp_update(C.byref(net), C.byref(bat), idx.data_ptr(), steps, batch, slices, C.byref(hyp), t0, ws.ptr, need.value,
                                  stats.ptr, None if gg is None else C.byref(thirteen(W, gg)), C.c_void_p(s.cuda_stream)), "qsp_update")
    s.synchronize()
    ws.get("the workspace")
    out = {"w": {k: g.get(k) for k, g in zip(keys, gw)}, "m": {k: g.get("m " + k) for k, g in zip(keys, gm)},
           "v": {k: g.get("v " + k) for k, g in zip(keys, gv)}, "stats": stats.get("stats")}
    if want_grads:
        out["grads"] = {k: g.get("grad " + k) for k, g in zip(keys, gg)}
    return out


def state_bits_equal(a, b):
    return all(same_bits(a[s][k], b[s][k]) for s in ("w", "m", "v") for k in a["w"])


def check_step(out, W, M, V, mb, hp, t, what):
    """one step's gradients, statistics and update against the reference -> the worst err / bound of the three"""
    st64, G, SB, E = pr.backward64(W, mb, hp, with_bound=True)
    worst_g = 0.0
    for k in G:
        err = np.abs(out["grads"][k].astype(np.float64) - G[k])
        worst_g = max(worst_g, float((err / E[k]).max()))
        assert (err <= E[k]).all(), "%s: %d of %d elements of the %s gradient out of bound, worst err / bound %.3g" % (
            what, int((err > E[k]).sum()), err.size, k, float((err / E[k]).max()))
    rs = np.abs(out["stats"][-1].astype(np.float64) - st64) / SB
    assert (rs <= 1.0).all(), "%s: statistics %s against %s, err / bound %s" % (what, out["stats"][-1], st64, rs)
    Gd = {k: out["grads"][k] for k in G}
    Wn, Mn, Vn, scale, norm = pr.update64(W, M, V, Gd, hp, t)
    assert hp["max_grad_norm"] <= 0 or scale < 1.0, "%s: the clip is not active (norm %.3g)" % (what, norm)
    assert abs(float(out["stats"][-1][5]) - norm) <= 4 * pr.U32 * norm, (what, out["stats"][-1][5], norm)
    UB = pr.update_bound(W, M, V, Gd, hp, t)
    worst_a = 0.0
    for k in G:
        for s, x64, b in zip("wmv", (Wn[k], Mn[k], Vn[k]), UB[k]):
            e = np.abs(out[s][k].astype(np.float64) - x64)
            worst_a = max(worst_a, float((e / b).max()))
            assert (e <= b).all(), "%s: %s of %s out of the update bound, worst err / bound %.3g" % (what, s, k, float((e / b).max()))
        # a wrong update is far outside: the step itself is many bounds long
        assert np.median(np.abs(Wn[k] - W[k]) / UB[k][0]) > 100.0, (what, k)
    return worst_g, float(rs.max()), worst_a


# ---------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("case", pr.CASES, ids=pr.CASE_IDS)
def test_gradients_statistics_clip_and_adam_of_one_step(torch, case):
    name, layout = case
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    M, V = pr.moments(W)
    worst = np.zeros(3)
    for hpname, hp in pr.HPS.items():
        for batch in pr.STEP_BATCHES:
            rows = pr.step_rows(name, layout, batch, hpname)
            t0 = 7 if batch == 17 else 0
            out = run(torch, W, M, V, data, rows[None, :], hp, slices=1, t0=t0, want_grads=True)
            worst = np.maximum(worst, check_step(out, W, M, V, pr.minibatch(data, rows), hp, t0 + 1, "%s %s %s batch %d" % (name, layout, hpname, batch)))
    print("ppo2 ratio %s-%s gradients worst err/bound %.3g, statistics %.3g, update %.3g" % (name, layout, *worst))
    assert (worst <= 1.0).all()


# ---------------------------------------------------------------------------------------------------- slices
@pytest.mark.parametrize("batch", [17, 33, 64, 300])
def test_slices_within_the_same_bounds_and_the_same_bits_on_another_stream(torch, batch):
    """one slice with work, ragged slices, empty trailing slices and more slices than chunks"""
    from quadsim_amd import ppo2
    name, layout, hp = "he", "shared" if batch in (17, 64) else "towers", pr.HP_VCLIP
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    M, V = pr.moments(W)
    rows = pr.step_rows(name, layout, batch)
    mb = pr.minibatch(data, rows)
    other = torch.cuda.Stream()
    worst, seen = np.zeros(3), []
    for slices in (2, 3, 7, 64, 0):
        out = run(torch, W, M, V, data, rows[None, :], hp, slices=slices, want_grads=True)
        worst = np.maximum(worst, check_step(out, W, M, V, mb, hp, 1, "batch %d slices %d" % (batch, slices)))
        again = run(torch, W, M, V, data, rows[None, :], hp, slices=slices, want_grads=True, stream=other)
        assert state_bits_equal(out, again) and same_bits(out["stats"], again["stats"]) and all(
            same_bits(out["grads"][k], again["grads"][k]) for k in out["grads"]), (batch, slices)
        seen.append(out)
    # auto is min(chunks, 128): for these batches one chunk a slice, which 64 slices give too wherever the chunks are fewer
    assert ppo2.auto_slices(batch) == -(-batch // 16)
    assert state_bits_equal(seen[-1], seen[-2]) and same_bits(seen[-1]["stats"], seen[-2]["stats"])
    print("ppo2 ratio slices batch %d gradients worst err/bound %.3g, statistics %.3g, update %.3g" % (batch, *worst))


# ---------------------------------------------------------------------------------------------------- many steps
def test_five_steps_are_five_calls_bit_for_bit(torch):
    name, layout, hp = "he", "shared", dict(pr.HP_VCLIP, max_grad_norm=0.5, lr=1e-3)
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    M, V = pr.moments(W)
    idx = np.stack([np.random.default_rng(200 + s).permutation(pr.N_ROWS)[:40] for s in range(5)]).astype(np.int32)
    whole = run(torch, W, M, V, data, idx, hp, slices=2, t0=2)
    st, stats = {"w": W, "m": M, "v": V}, []
    for i in range(5):
        one = run(torch, st["w"], st["m"], st["v"], data, idx[i:i + 1], hp, slices=2, t0=2 + i)
        st, stats = one, stats + [one["stats"]]
    assert np.isfinite(whole["stats"]).all()
    assert state_bits_equal(whole, st) and same_bits(whole["stats"], np.concatenate(stats))
    assert not same_bits(whole["w"]["w1"], np.asarray(W["w1"])) and not same_bits(whole["w"]["logstd"], np.asarray(W["logstd"]))


def _policy(torch, name, layout):
    import quadsim_amd as qa
    return qa.ActorCriticPolicy(pr.weight_set(name, layout), device="cuda")


def _tensors(torch, data):
    d = device_data(torch, data)
    return dict(zip(DATA_KEYS, d))


HP_KW = dict(learning_rate=1e-3, cliprange=0.2, cliprange_vf=None, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)


def test_wrapper_split_at_its_maximum_equals_one_call(torch, monkeypatch):
    """steps 3 with a maximum of 2: two qsp_update calls that continue each other, the bits of the one call"""
    from quadsim_amd import ppo2
    data = pr.rollout("he", "towers")
    idx = torch.as_tensor(np.stack([np.random.default_rng(300 + s).permutation(pr.N_ROWS)[:33] for s in range(3)]).astype(np.int32)).cuda()
    a, b = _policy(torch, "he", "towers"), _policy(torch, "he", "towers")
    one = ppo2.ppo2_update(a, _tensors(torch, data), idx, **HP_KW)
    monkeypatch.setattr(ppo2, "PPO_MAX_STEPS", 2)
    two = ppo2.ppo2_update(b, _tensors(torch, data), idx, **HP_KW, return_grads=True)
    assert a._ppo_steps == b._ppo_steps == 3 and torch.equal(one["stats"], two["stats"])
    for k in pr.KEYS_TOWERS:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert all(torch.equal(x, y) for x, y in zip(a._ppo_m + a._ppo_v, b._ppo_m + b._ppo_v))
    assert all(torch.isfinite(g).all() for g in two["grads"])


# ---------------------------------------------------------------------------------------------------- edges
def test_step_counter_at_its_upper_edge(torch):
    """t0 + steps = 2^31 - 1 is accepted and gives float64's Adam factors (both powers have underflowed: lr_t = lr);
    t0 + steps = 2^31 is refused"""
    from quadsim_amd import QuadsimError
    name, layout, hp = "sb2", "shared", pr.HP_NOVCLIP
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    M, V = pr.moments(W)
    rows = pr.step_rows(name, layout, 17, "novclip")
    t0 = (1 << 31) - 2
    out = run(torch, W, M, V, data, rows[None, :], hp, t0=t0, want_grads=True)
    check_step(out, W, M, V, pr.minibatch(data, rows), hp, t0 + 1, "t0 = 2^31 - 2")
    with pytest.raises(QuadsimError, match="t0"):
        run(torch, W, M, V, data, rows[None, :], hp, t0=t0 + 1)


def test_the_same_minibatch_in_a_large_data_set_gives_the_same_bits(torch):
    """the rows of a minibatch placed among 100 000 rows (the last one included): the bits depend on the rows, not on n"""
    name, layout, hp = "he", "shared", pr.HP_VCLIP
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    M, V = pr.moments(W)
    rows = pr.step_rows(name, layout, 64)
    n = 100000
    where = np.random.default_rng(400).permutation(n)[:64].astype(np.int32)
    where[0], where[1] = n - 1, 0
    big = {k: np.zeros((n,) + data[k].shape[1:], np.float32) for k in DATA_KEYS}
    for k in DATA_KEYS:
        big[k][where] = data[k][rows]
    a = run(torch, W, M, V, data, rows[None, :], hp, slices=3, want_grads=True)
    b = run(torch, W, M, V, big, where[None, :], hp, slices=3, want_grads=True)
    _dev.pop(id(big))
    assert state_bits_equal(a, b) and same_bits(a["stats"], b["stats"]) and all(same_bits(a["grads"][k], b["grads"][k]) for k in a["grads"])


# ---------------------------------------------------------------------------------------------------- the policy afterwards
@pytest.mark.parametrize("layout", ["shared", "towers"])
def test_every_device_path_runs_the_updated_policy(torch, layout):
    """policy.step, the fused Runner roll-out in both precisions, predict_hip and evaluate_policy_episodes after ppo2_update agree with a
    FRESH policy built from the updated weights; the images cached before the update would give the old network, and the host
    copy of logstd the old standard deviation"""
    import quadsim_amd as qa
    from quadsim_amd import ppo2
    from quadsim_amd.policy import _actor_of
    data = pr.rollout("he", layout)
    pol = _policy(torch, "he", layout)
    noise = torch.randn((4, 64, 4), generator=torch.Generator().manual_seed(1)).cuda()

    def paths(p):
        env = qa.VecDockingEnv("docking-v0", num_envs=64, seed=3)      # a fresh env: the same resets every time
        out = []
        for precision in ("f32", "bf16x3"):
            env.reset()
            ro = qa.fused_runner_rollout(env, p, 4, noise=noise, precision=precision)
            out += [ro["actions"].clone(), ro["values"].clone(), ro["neglogp"].clone()]
        obs = _tensors(torch, data)["obs"][:64].contiguous()
        out += [x.clone() for x in p.step(obs, noise=noise[0])[:2]]
        out += [_actor_of(p).predict_hip(env, obs).clone()]
        env.reset()
        res = qa.evaluate_policy_episodes(p, env, 1, max_steps=8)
        out += [res.returns.clone(), res.lengths.clone()]
        env.close()
        return out
    before = paths(pol)                                          # builds and caches every image of the OLD weights
    old_logstd = pol.logstd_host.copy()
    idx = qa.minibatch_schedule(pr.N_ROWS, 3, 2, torch.Generator().manual_seed(5), "cuda")
    ppo2.ppo2_update(pol, _tensors(torch, data), idx, **dict(HP_KW, learning_rate=1e-2))
    assert pol._ppo_steps == 6 and not np.array_equal(pol.logstd_host, old_logstd)
    assert np.array_equal(pol.logstd_host, pol.logstd.cpu().numpy())
    fresh = qa.ActorCriticPolicy({k: getattr(pol, k).cpu().numpy() for k in pr.keys_of(pr.weight_set("he", layout))}, device="cuda")
    after, ref = paths(pol), paths(fresh)
    for i, (x, y, z) in enumerate(zip(after, ref, before)):
        assert torch.equal(x, y) or torch.allclose(x.double(), y.double(), equal_nan=True, rtol=0, atol=0), i
        if i < 9:
            assert not torch.equal(x, z), i


# ---------------------------------------------------------------------------------------------------- it learns
def test_twenty_steps_lower_the_value_loss_as_the_reference_does(torch):
    from quadsim_amd import ppo2
    name, layout = "he", "shared"
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    rows = pr.step_rows(name, layout, 64)
    hp = dict(pr.HP_VCLIP, lr=pr.LEARN_LR, max_grad_norm=0.5)
    idx = np.repeat(rows[None, :], pr.LEARN_STEPS, 0)
    out = run(torch, W, pr.zero_state(W), pr.zero_state(W), data, idx, hp, slices=0)
    ref = pr.learn64()
    vl = out["stats"][:, 1].astype(np.float64)
    print("ppo2 learn: value loss %.6g -> %.6g on the device, %.6g -> %.6g in float64, margin %.3g" % (vl[0], vl[-1], ref[0, 1], ref[-1, 1], ref[0, 1] - ref[-1, 1]))
    assert np.isfinite(out["stats"]).all() and vl[-1] < vl[0]
    # the device's descent is the reference's to a tenth of the reference's own descent
    assert abs(vl[-1] - ref[-1, 1]) <= 0.1 * (ref[0, 1] - ref[-1, 1]), (vl[-1], ref[-1, 1])
    pol = _policy(torch, name, layout)
    res = ppo2.ppo2_update(pol, _tensors(torch, data), torch.as_tensor(idx).cuda(), learning_rate=hp["lr"], cliprange=0.2, ent_coef=0.01,
                           vf_coef=0.5, max_grad_norm=0.5, slices="auto")
    assert same_bits(res["stats"].cpu().numpy(), out["stats"])     # the wrapper is the raw call
    with pytest.raises(ValueError, match="indices"):
        ppo2.ppo2_update(pol, _tensors(torch, data), torch.full((1, 4), pr.N_ROWS, dtype=torch.int32, device="cuda"), **HP_KW)
