"""Behaviour cloning on the device (qsbc_fit and qsbc_loss of libquadsim_bc.so, quadsim_amd.bc) against tests/bcfit_ref.py.

Every raw call goes through `run` / `run_loss`, which put every tensor the kernels write (six weights, twelve moments, loss, six
gradients; partials and the result) between 256 sentinel bytes on both sides and check them afterwards.  What is held:
  one step     every element of the six gradients within grad_bound of backward64 and the loss within its bound (no element
               excluded: tests/test_bcfit_cpu.py holds that no fixture has a pre-activation within its bound of zero), and w, m, v
               after the step within adam_bound of adam64 applied to the device's OWN gradient, from non-zero moments; batches
               either side of the chunk of 16 rows, SB2's 64 and the maximum, rows 0 and n - 1 among them
  ragged       counts of 1, batch - 1 and batch in one launch equal one launch per step with batch = counts[s], bit for bit, with
               the unused index entries far out of range
  many steps   a launch of a + b steps is bit for bit the launch of a then the launch of b; five steps are five launches
  invariants   a second run on another stream at other addresses gives the same bits; t0 at its upper edge
  qsbc_loss    against the float64 loss at counts around the block of 256 rows, a row list against the all-rows form, two grids
  the policy   after pretrain every device path of MlpPolicy and ActorCriticPolicy runs the UPDATED actor
  it learns    200 steps towards a teacher; end to end from record_expert_dataset
Measured worst ratios are in profiles/bcfit/README.md."""
import ctypes as C
import copy

import numpy as np
import pytest

import actor_numerics as an
import bcfit_ref as br
from side_cases import Guarded, same_bits, six

pytestmark = pytest.mark.gpu

KEYS = br.KEYS


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def data(torch):
    x, a = br.dataset()
    return torch.as_tensor(x).cuda().contiguous(), torch.as_tensor(a).cuda().contiguous()


def run(torch, W, M, V, data, indices, counts=None, lr=1e-2, t0=0, want_grads=False, stream=None, beta1=br.BETA1, beta2=br.BETA2, eps=br.EPS):
    """qsbc_fit on copies of (W, M, V) -> dict(w, m, v: dicts of numpy arrays, loss, grads)"""
    from quadsim_amd import bc
    lib = bc.load_bc()
    indices = np.ascontiguousarray(indices, np.int32)
    steps, batch = indices.shape
    gw = [Guarded(torch, np.asarray(W[key], np.float32)) for key in KEYS]
    gm = [Guarded(torch, np.asarray(M[key], np.float32)) for key in KEYS]
    gv = [Guarded(torch, np.asarray(V[key], np.float32)) for key in KEYS]
    gg = [Guarded(torch, np.full(br.SHAPES[key], np.nan, np.float32)) for key in KEYS] if want_grads else None
    loss = Guarded(torch, np.full(steps, np.nan, np.float32))
    idx = torch.as_tensor(indices).cuda()
    cnt = None if counts is None else torch.as_tensor(np.ascontiguousarray(counts, np.int32)).cuda()
    net = bc.QsbcNet(C.sizeof(bc.QsbcNet), 0, six(gw), six(gm), six(gv))
    s = stream if stream is not None else torch.cuda.current_stream()
    bc.check_bc(lib.qsbc_fit(C.byref(net), data[0].data_ptr(), data[1].data_ptr(), data[0].shape[0], idx.data_ptr(),
                             None if cnt is None else cnt.data_ptr(), steps, batch, lr, beta1, beta2, eps, t0, loss.ptr,
                             None if gg is None else six(gg), C.c_void_p(s.cuda_stream)), "qsbc_fit")
    s.synchronize()
    out = {"w": {key: g.get(key) for key, g in zip(KEYS, gw)}, "m": {key: g.get("m " + key) for key, g in zip(KEYS, gm)},
           "v": {key: g.get("v " + key) for key, g in zip(KEYS, gv)}, "loss": loss.get("loss")}
    if want_grads:
        out["grads"] = {key: g.get("grad " + key) for key, g in zip(KEYS, gg)}
    return out


def run_loss(torch, W, obs, act, rows=None, count=None, grid=0):
    """qsbc_loss -> (the float64 result, the partials)"""
    from quadsim_amd import bc
    lib = bc.load_bc()
    ws = [torch.as_tensor(np.asarray(W[key], np.float32)).cuda().contiguous() for key in KEYS]
    count = (len(rows) if rows is not None else obs.shape[0]) if count is None else count
    r = None if rows is None else torch.as_tensor(np.ascontiguousarray(rows, np.int32)).cuda()
    part = Guarded(torch, np.full(lib.qsbc_loss_blocks(count), np.nan, np.float64))
    out = Guarded(torch, np.full(1, np.nan, np.float64))
    s = torch.cuda.current_stream()
    bc.check_bc(lib.qsbc_loss((C.c_void_p * 6)(*[w.data_ptr() for w in ws]), obs.data_ptr(), act.data_ptr(), obs.shape[0],
                              None if r is None else r.data_ptr(), count, part.ptr, out.ptr, grid, C.c_void_p(s.cuda_stream)), "qsbc_loss")
    s.synchronize()
    return float(out.get("out")[0]), part.get("partials")


def state_bits_equal(a, b):
    return all(same_bits(a[s][key], b[s][key]) for s in ("w", "m", "v") for key in KEYS)


# ---------------------------------------------------------------------------------------------------- one step
@pytest.mark.parametrize("name", br.STEP_SETS)
def test_gradients_loss_and_adam_of_one_step(torch, data, name):
    W = br.weight_set(name)
    obs, act = br.dataset()
    M, V = br.moments()
    worst_g, worst_l, worst_a = 0.0, 0.0, 0.0
    for batch in br.STEP_BATCHES:
        idx = br.step_rows(name, batch)
        assert idx[0, 0] == 0 and (batch < 4 or idx[0, 1] == br.N_ROWS - 1)
        loss64, G, lb, E = br.backward64(W, obs[idx[0]], act[idx[0]], with_bound=True)
        for t0 in (0, 7):
            out = run(torch, W, M, V, data, idx, lr=1e-2, t0=t0, want_grads=True)
            what = "%s batch %d t0 %d" % (name, batch, t0)
            for key in KEYS:
                err = np.abs(out["grads"][key].astype(np.float64) - G[key])
                r = float((err / E[key]).max())
                worst_g = max(worst_g, r)
                assert (err <= E[key]).all(), "%s: %d of %d elements of the %s gradient out of bound, worst err / bound %.3g" % (
                    what, int((err > E[key]).sum()), err.size, key, r)
                g = out["grads"][key]
                ref = br.adam64(W[key], M[key], V[key], g, t0 + 1, 1e-2)
                bounds = br.adam_bound(W[key], M[key], V[key], g, t0 + 1, 1e-2)
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
    print("bcfit ratio %s gradients worst err/bound %.3g, loss %.3g, adam %.3g" % (name, worst_g, worst_l, worst_a))
    assert worst_g <= 1.0 and worst_l <= 1.0 and worst_a <= 1.0, (worst_g, worst_l, worst_a)


# ---------------------------------------------------------------------------------------------------- ragged steps
@pytest.mark.parametrize("batch", [17, 64])
def test_ragged_steps_equal_their_own_launches(torch, data, batch):
    """counts 1, batch - 1 and batch (and a count inside a chunk) in ONE launch: each step's loss and the final state equal the
    run in which every step is its own launch with batch = counts[s]; the index entries at or beyond counts[s] are far outside
    [0, n) -- a kernel that read them would fetch from unmapped addresses or change the result"""
    W = br.weight_set("he")
    M, V = br.moments()
    counts = np.array([1, batch - 1, batch, 5, batch], np.int32)
    idx = br.step_indices(batch, steps=len(counts), seed=75)
    junk = np.array([1 << 30, -(1 << 30), br.N_ROWS, -1], np.int32)
    for s, c in enumerate(counts):
        idx[s, c:] = junk[np.arange(batch - c) % 4]
    whole = run(torch, W, M, V, data, idx, counts, t0=3)
    st, losses = {"w": W, "m": M, "v": V}, []
    for s, c in enumerate(counts):
        one = run(torch, st["w"], st["m"], st["v"], data, idx[s:s + 1, :c], None, t0=3 + s)
        st, losses = one, losses + [one["loss"]]
    assert np.isfinite(whole["loss"]).all() and all(np.isfinite(whole["w"][key]).all() for key in KEYS)
    assert same_bits(whole["loss"], np.concatenate(losses)), (whole["loss"], np.concatenate(losses))
    assert state_bits_equal(whole, st)
    # and with counts given for a full schedule: the same bits as without
    full = br.step_indices(batch, steps=2, seed=76)
    assert state_bits_equal(run(torch, W, M, V, data, full, np.full(2, batch, np.int32)), run(torch, W, M, V, data, full))


# ---------------------------------------------------------------------------------------------------- one launch = the sequence
@pytest.mark.parametrize("batch", [10, 64])
def test_one_launch_equals_the_sequence(torch, data, batch):
    W = br.weight_set("he")
    M, V = br.moments()
    idx = br.step_indices(batch, steps=5, seed=77)
    whole = run(torch, W, M, V, data, idx, t0=2)
    st, losses = {"w": W, "m": M, "v": V}, []
    for i in range(5):
        one = run(torch, st["w"], st["m"], st["v"], data, idx[i:i + 1], t0=2 + i)
        st, losses = one, losses + [one["loss"]]
    assert state_bits_equal(whole, st) and same_bits(whole["loss"], np.concatenate(losses))
    a = run(torch, W, M, V, data, idx[:3], t0=2)
    b = run(torch, a["w"], a["m"], a["v"], data, idx[3:], t0=5)
    assert state_bits_equal(whole, b) and same_bits(whole["loss"], np.concatenate([a["loss"], b["loss"]]))
    assert not same_bits(whole["w"]["w1"], np.asarray(W["w1"]))


# ---------------------------------------------------------------------------------------------------- run twice
def test_run_twice_same_bits_on_another_stream(torch, data):
    W = br.weight_set("v0")
    M, V = br.moments()
    idx = br.step_indices(100, steps=4, seed=78)
    counts = np.array([100, 37, 100, 64], np.int32)
    a = run(torch, W, M, V, data, idx, counts, want_grads=True)
    dummy = torch.empty(123457, dtype=torch.uint8, device="cuda")      # moves the addresses of everything allocated after it
    b = run(torch, W, M, V, data, idx, counts, want_grads=True, stream=torch.cuda.Stream())
    del dummy
    assert state_bits_equal(a, b) and same_bits(a["loss"], b["loss"])
    assert all(same_bits(a["grads"][key], b["grads"][key]) for key in KEYS)


# ---------------------------------------------------------------------------------------------------- the step counter's edge
def test_step_counter_at_its_upper_edge(torch, data):
    """t0 = 2^31 - 2 is the last step the contract takes (t0 + steps below 2^31): as t = 2^31 - 1 it enters Adam's bias
    correction, where both powers have long underflowed to 0 and lr_t = lr"""
    from quadsim_amd import bc
    W = br.weight_set("he")
    M, V = br.moments()
    obs, act = br.dataset()
    idx = br.step_rows("he", 17)
    _, G, lb, E = br.backward64(W, obs[idx[0]], act[idx[0]], with_bound=True)
    lr = 1e-2
    for t0 in (10 ** 5, 2 ** 31 - 2):
        assert bc.check_bc_args(br.N_ROWS, 1, 17, lr, t0=t0)[7] == t0
        out = run(torch, W, M, V, data, idx, lr=lr, t0=t0, want_grads=True)
        worst = 0.0
        for key in KEYS:
            g = out["grads"][key]
            assert (np.abs(g - G[key]) <= E[key]).all(), (t0, key)                 # the gradient does not depend on t0
            x64 = br.adam64(W[key], M[key], V[key], g, t0 + 1, lr)
            bounds = br.adam_bound(W[key], M[key], V[key], g, t0 + 1, lr)
            for s, x, b in zip("wmv", x64, bounds):
                e = np.abs(out[s][key].astype(np.float64) - x)
                worst = max(worst, float((e / b).max()))
                assert (e <= b).all(), "t0 %d: %s of %s out of the update bound, worst err / bound %.3g" % (t0, s, key, (e / b).max())
            assert np.median(np.abs(x64[0] - W[key]) / bounds[0]) > 100.0, (t0, key)
        print("bcfit ratio t0 %d adam worst err/bound %.3g" % (t0, worst))
    assert br.lr_t64(2 ** 31 - 1, lr) == lr
    with pytest.raises(ValueError):
        bc.check_bc_args(br.N_ROWS, 1, 17, lr, t0=2 ** 31 - 1)


# ---------------------------------------------------------------------------------------------------- qsbc_loss
@pytest.fixture(scope="module")
def big(torch):
    """1024 rows: four blocks of the validation pass"""
    import dynplan_ref as dr
    x = dr.sample_obs(1024, seed=93)
    a = np.random.default_rng(94).uniform(-1.0, 1.0, (1024, 4)).astype(np.float32)
    return x, a, torch.as_tensor(x).cuda(), torch.as_tensor(a).cuda()


@pytest.mark.parametrize("count", [1, 255, 256, 257, 1024])
def test_validation_loss(torch, big, count):
    x, a, xd, ad = big
    worst = 0.0
    for name in br.STEP_SETS:
        W = br.weight_set(name)
        ref = br.forward64(W, x[:count], a[:count])["loss"]
        bound = br.loss_bound(W, x[:count], a[:count])
        got, part = run_loss(torch, W, xd, ad, count=count)                        # the all-rows form: rows 0 .. count-1
        assert part.shape == (-(-count // 256),) and np.isfinite(part).all()
        asc = 0.0
        for p in part:                                                             # the contract's order: ascending, in float64
            asc += float(p)
        assert got == asc / (4.0 * count)
        worst = max(worst, abs(got - ref) / bound)
        assert abs(got - ref) <= bound, "%s count %d: %.17g against %.17g, err / bound %.3g" % (name, count, got, ref, abs(got - ref) / bound)
        listed, part_l = run_loss(torch, W, xd, ad, rows=np.arange(count))
        assert listed == got and same_bits(part, part_l)
        for grid in (1, 3):
            g, p = run_loss(torch, W, xd, ad, count=count, grid=grid)
            assert g == got and same_bits(p, part), (name, count, grid)
        # a row list in another order with repeats, reaching the last row: against the reference on those rows
        rows = np.random.default_rng(count).integers(0, 1024, count).astype(np.int32)
        rows[0] = 1023
        got_r, _ = run_loss(torch, W, xd, ad, rows=rows)
        assert abs(got_r - br.forward64(W, x[rows], a[rows])["loss"]) <= br.loss_bound(W, x[rows], a[rows]), (name, count)
        # the first partial in ascending order: a float64 sum of float32 row sums
        assert abs(part[0] / (4.0 * min(count, 256)) - br.forward64(W, x[:min(count, 256)], a[:min(count, 256)])["loss"]) <= br.loss_bound(
            W, x[:min(count, 256)], a[:min(count, 256)])
    print("bcfit ratio qsbc_loss count %d worst err/bound %.3g" % (count, worst))


# ---------------------------------------------------------------------------------------------------- the stale-image test
def _outputs(torch, qa, policy, kind):
    """every device path that runs the policy's actor, from fresh envs of one seed -> {path: numpy array}"""
    from quadsim_amd.policy import _actor_of
    out = {}
    env = qa.VecDockingEnv("docking-v0", num_envs=64, randomise=1, seed=5, init_range=qa.C3_INIT_RANGE)
    obs = env.reset().clone()
    actor = _actor_of(policy)
    out["predict"] = actor.predict(obs).cpu().numpy()
    for precision in ("f32", "bf16x3"):
        out["predict_hip/" + precision] = actor.predict_hip(env, obs, precision).cpu().numpy()
        if kind == "mlp":
            env.reset()
            out["policy_rollout/" + precision] = qa.fused_policy_rollout(env, policy, 4, precision=precision)[4].cpu().numpy()
        else:
            env.reset()
            ro = qa.fused_runner_rollout(env, policy, 4, noise=torch.zeros((4, 64, 4), device="cuda"), precision=precision)
            out["runner_rollout/" + precision] = ro["actions"].cpu().numpy()
            out["runner_values/" + precision] = ro["values"].cpu().numpy()
    if kind != "mlp":
        out["step"] = policy.step(obs, deterministic=True)[0].cpu().numpy()
    env.close()
    return out, obs.cpu().numpy()


@pytest.mark.parametrize("kind", ["mlp", "shared", "towers"])
def test_every_device_path_runs_the_updated_actor(torch, data, kind):
    """pretrain writes the weights behind the policy's back; every cached device image of them (transposed copies, packed
    split-bf16 blobs, the evaluation actor) must go, or the kernels keep running the old network -- silently"""
    import quadsim_amd as qa
    if kind == "mlp":
        W = an.weight_set("v0")                                                    # rescaled: its actions are mostly unclipped
        policy = qa.MlpPolicy({k: W[k] for k in KEYS})
    else:
        W = an.weight_set("v0" if kind == "shared" else "towers")
        policy = qa.ActorCriticPolicy(W)
        assert policy.towers == (kind == "towers")
    critic = {k: getattr(policy, k).clone() for k in ("wv0", "bv0", "wv1", "bv1", "wv2", "bv2") if hasattr(policy, k)}
    before, obs = _outputs(torch, qa, policy, kind)                               # builds every cached image
    idx = torch.as_tensor(br.step_indices(64, seed=79))
    res = qa.bc_fit(policy, data[0], data[1], idx, lr=1e-2)
    assert np.isfinite(res["loss"].cpu().numpy()).all() and policy._bc_steps == 1
    after, _ = _outputs(torch, qa, policy, kind)
    new = {k: getattr(policy, k).cpu().numpy() for k in KEYS}
    assert all(not same_bits(new[k], np.asarray(W[k], np.float32)) for k in KEYS)
    assert all(torch.equal(getattr(policy, k), v) for k, v in critic.items())      # only the actor moved
    for path in before:
        if path.startswith("runner_values") and kind == "towers":
            # the value tower has nothing of the actor's: the same value of the first observation (the later ones differ with
            # the actions taken)
            assert same_bits(before[path][0], after[path][0]) and not same_bits(before[path][1:], after[path][1:]), path
        else:
            assert not same_bits(before[path], after[path]), "%s still runs the old weights" % path
    # and they run the NEW weights: the float64 net of the updated tensors, within the bound tests/test_gpu_actor_numerics.py holds
    m64, Em = an.net64(new, obs)[0], an.err_scale(new, obs)[0]
    for path, precision in (("predict", "f32"), ("predict_hip/f32", "f32"), ("predict_hip/bf16x3", "bf16x3")):
        an.check_clipped(after[path], m64, Em, precision, "%s after pretrain (%s)" % (path, kind))
    old64 = an.net64({k: np.asarray(W[k], np.float32) for k in KEYS}, obs)[0]
    assert (np.abs(np.clip(m64, -1, 1) - np.clip(old64, -1, 1)) > 100.0 * an.bound(Em, "bf16x3")).any()
    # a second call continues from the moments kept on the policy; reset_pretrain_optimizer forgets them
    m_before = policy._bc_m[2].clone()
    policy.pretrain(qa.ExpertData({"obs": br.dataset()[0], "actions": br.dataset()[1]}, batch_size=64, train_fraction=0.5), n_epochs=1)
    assert policy._bc_steps == 1 + 3 and not torch.equal(policy._bc_m[2], m_before)
    policy.reset_pretrain_optimizer()
    assert policy._bc_steps == 0 and policy._bc_m is None


# ---------------------------------------------------------------------------------------------------- it learns
def test_it_learns(torch):
    x, a, idx = br.teacher_case()
    W, Z = br.learn_student(), br.zero_state()
    xd, ad = torch.as_tensor(x).cuda(), torch.as_tensor(a).cuda()
    out = run(torch, W, Z, Z, (xd, ad), idx, lr=br.LEARN_LR)
    ref = br.fit64(W, Z, Z, x, a, idx, lr=br.LEARN_LR)[3]
    first, last, last64 = float(out["loss"][:8].mean(dtype=np.float64)), float(out["loss"][-8:].mean(dtype=np.float64)), float(ref[-8:].mean())
    print("bcfit learns: first epoch %.9g, last epoch %.9g, float64 last epoch %.9g, diff %.3g, margin %.3g" % (
        first, last, last64, abs(last - last64), br.LEARN_MARGIN))
    assert last < first
    assert abs(last - last64) <= br.LEARN_MARGIN, (last, last64, abs(last - last64), br.LEARN_MARGIN)
    # the validation pass on the final weights agrees with the reference's loss of those weights
    val, _ = run_loss(torch, out["w"], xd, ad)
    ref_val, bound = br.forward64(out["w"], x, a)["loss"], br.loss_bound(out["w"], x, a)
    print("bcfit learns: validation loss %.17g against %.17g, err / bound %.3g" % (val, ref_val, abs(val - ref_val) / bound))
    assert abs(val - ref_val) <= bound and val < first


# ---------------------------------------------------------------------------------------------------- end to end, small
def test_end_to_end_from_a_recorded_dataset(torch):
    import quadsim_amd as qa
    env = qa.VecDockingEnv("docking-v1", num_envs=8, seed=11)
    rec = qa.record_expert_dataset(env, n_episodes=1)
    env.close()
    data = qa.ExpertData(rec, batch_size=64, seed=3)
    assert data.n == len(rec["obs"]) and data.n_train == int(0.7 * data.n) and data.obs.device.type == "cuda"
    results = []
    for _ in range(2):
        policy = qa.MlpPolicy(copy.deepcopy(br.weight_set("sb2")))
        res = policy.pretrain(data, n_epochs=2, seed=4)
        assert sorted(res) == ["steps", "train_loss", "val_loss"]
        assert len(res["train_loss"]) == 2 and all(np.isfinite(v) for v in res["train_loss"])
        assert sorted(res["val_loss"]) == [1, 2] and all(np.isfinite(v) for v in res["val_loss"].values())
        assert res["steps"] == 2 * -(-data.n_train // 64) == policy._bc_steps
        results.append((res, {k: getattr(policy, k).cpu().numpy() for k in KEYS}, [m.cpu().numpy() for m in policy._bc_m]))
    (ra, wa, ma), (rb, wb, mb) = results
    assert ra == rb and all(same_bits(wa[k], wb[k]) for k in KEYS) and all(same_bits(x, y) for x, y in zip(ma, mb))
    assert all(not same_bits(wa[k], br.weight_set("sb2")[k]) for k in KEYS)
    print("bcfit end to end: %d rows, %d steps, train %s, val %s" % (data.n, ra["steps"], ra["train_loss"], ra["val_loss"]))
