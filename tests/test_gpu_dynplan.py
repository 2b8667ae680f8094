"""The learned-dynamics planner on the device (qsd_shooting_plan of libquadsim_dyn.so) against tests/dynplan_ref.py.

Every call goes through `plan`, which puts each output buffer between 256 sentinel bytes on both sides and checks them
afterwards.  What is held, on every element of every output:
  draws      sequence / actions = shooting_ref.actions(seed, gid, k, paths, horizon)[best_index], bit for bit
  steps      |traj[env, c, h] - step64(traj[env, c, h - 1], a[c][h])| <= the derived bound at that input (traj[.., -1] = obs): one
             float32 model step at a time from the kernel's OWN inputs, so the bound never compounds
  scores     against the float64 sum over the kernel's own trajectory, within the bound of the squared terms; best_index = the
             first arg-max of the kernel's own scores; best_score = scores[best_index] bit for bit
The mapping has edges at 16 candidates (a wave's tile), 64 (a workgroup's four tiles; work items are numbered across envs, so
with n = 3 an env's tiles start inside a workgroup) and at cus x 4 tiles, where the persistent grid starts to loop.  The net has
edges of its own, the hidden widths at which the packer masks a partly filled block of 16 units and the router changes the
instantiation: test_edge_widths runs a dense net at each (dynplan_ref.EDGE_WIDTHS), both maxima included.
Worst error / bound ratios measured on an MI355X are in profiles/dynplan/README.md.
"""
import ctypes as C

import numpy as np
import pytest

import dynplan_ref as dr
import shooting_ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
GID0 = (1 << 32) - 2                 # env ids on both sides of 2^32 with n = 3
K0 = (1 << 32) + 5                   # k << 26 needs all 64 bits of the block index
GUARD = 256


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_nets = {}


def net_of(name):
    if name not in _nets:
        W = {"zero": dr.weights_zero, "wiring": dr.weights_wiring}[name]() if name in ("zero", "wiring") else dr.weight_set(name)
        _nets[name] = (W, dr.to_net(W, "cuda"))
    return _nets[name]


def plan(torch, net, obs, horizon, paths, seed=SEED, gid0=GID0, k=K0, want=("best_score", "best_index", "sequence", "scores", "traj")):
    """qsd_shooting_plan with every output between sentinel bytes -> dict of numpy arrays"""
    from quadsim_amd import dynplan
    lib = dynplan.load()
    obs_t = torch.as_tensor(np.ascontiguousarray(obs, np.float32)).cuda()
    n = obs_t.shape[0]
    shapes = {"actions": ((n, 4), torch.float32), "best_score": ((n,), torch.float64), "best_index": ((n,), torch.int32),
              "sequence": ((n, horizon, 4), torch.float32), "scores": ((n, paths), torch.float64),
              "traj": ((n, paths, horizon, 12), torch.float32)}
    raw, view = {}, {}
    for name in ("actions",) + tuple(want):
        shape, dtype = shapes[name]
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        raw[name] = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        view[name] = raw[name][GUARD:GUARD + nbytes].view(dtype).view(shape)
    wb = C.c_size_t(0)
    dynplan.check(lib.qsd_plan_workspace_bytes(n, paths, C.byref(wb)), "qsd_plan_workspace_bytes")
    raw["workspace"] = torch.full((GUARD + wb.value + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    p = lambda name: C.c_void_p(view[name].data_ptr()) if name in view else None     # noqa: E731
    image = net.pack()
    dynplan.check(lib.qsd_shooting_plan(C.c_void_p(image.data_ptr()), n, C.c_void_p(obs_t.data_ptr()), seed, gid0, k, horizon, paths,
                                        C.c_void_p(raw["workspace"].data_ptr() + GUARD), p("actions"), p("best_score"), p("best_index"),
                                        p("sequence"), p("scores"), p("traj"),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "qsd_shooting_plan")
    torch.cuda.synchronize()
    for name, r in raw.items():
        g = torch.cat([r[:GUARD], r[-GUARD:]])
        assert bool((g == 0xA5).all()), "sentinel bytes around %s were overwritten" % name
    return {name: v.cpu().numpy() for name, v in view.items()}


_acts = {}


def draws(n, paths, horizon, gid0=GID0, k=K0, seed=SEED):
    key = (n, paths, horizon, gid0, k, seed)
    if key not in _acts:
        _acts[key] = np.stack([shooting_ref.actions_fast(seed, gid0 + i, k, paths, horizon) for i in range(n)])
    return _acts[key]


def check_plan(W, obs, out, acts, what):
    """every check of the module's docstring on one plan -> (worst step err / bound, worst score err / bound)"""
    n, paths, horizon = acts.shape[:3]
    traj, scores = out["traj"], out["scores"]
    assert traj.shape == (n, paths, horizon, 12) and scores.shape == (n, paths)
    before = np.concatenate([np.repeat(np.asarray(obs, np.float32)[:, None, None, :], paths, axis=1), traj[:, :, :-1]], axis=2)
    ref, bound = dr.step64(W, before, acts, with_bound=True)
    err = np.abs(traj.astype(np.float64) - ref)
    ok = err <= bound                                    # NaN inputs: handled by the caller, never excluded here
    r_step = float((err / bound).max())
    print("dynplan ratio %s steps worst err/bound %.3g over %d elements" % (what, r_step, err.size))
    assert ok.all(), "%s: %d of %d trajectory elements out of bound, worst err / bound %.3g" % (what, int((~ok).sum()), ok.size, r_step)
    cost = dr.cost64(before)
    sb = dr.score_bound(before)
    serr = np.abs(scores - cost)
    r_score = float((serr / np.maximum(sb, 1e-300)).max())
    print("dynplan ratio %s scores worst err/bound %.3g" % (what, r_score))
    assert (serr <= sb).all(), "%s: scores out of bound, worst ratio %.3g" % (what, r_score)
    check_winner(out, acts, what)
    return r_step, r_score


def check_winner(out, acts, what):
    n = acts.shape[0]
    best = out["best_index"]
    assert np.array_equal(best, np.argmax(out["scores"], axis=1).astype(np.int32)), what
    assert np.array_equal(out["best_score"].view(np.uint64), out["scores"][np.arange(n), best].view(np.uint64)), what
    assert np.array_equal(out["sequence"].view(np.uint32), acts[np.arange(n), best].view(np.uint32)), what
    assert np.array_equal(out["actions"].view(np.uint32), acts[np.arange(n), best, 0].view(np.uint32)), what


# ---------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize("n", [1, 3])
def test_draws(torch, n):
    """sequence and actions against the oracle's own Philox (shooting_ref.actions, the definition), gid0 and k across 2^32"""
    W, net = net_of("he_20_10")
    paths, horizon = 17, 5
    assert GID0 < 1 << 32 <= GID0 + 2 and K0 > 1 << 32
    out = plan(torch, net, dr.sample_obs(n), horizon, paths)
    for i in range(n):
        ref = shooting_ref.actions(SEED, GID0 + i, K0, paths, horizon)
        assert np.array_equal(ref.view(np.uint32), draws(n, paths, horizon)[i].view(np.uint32))
        b = int(out["best_index"][i])
        assert 0 <= b < paths
        assert np.array_equal(out["sequence"][i].view(np.uint32), ref[b].view(np.uint32))
        assert np.array_equal(out["actions"][i].view(np.uint32), ref[b, 0].view(np.uint32))
    # the first steps and candidates of the stream do not depend on the plan's size
    small = plan(torch, net, dr.sample_obs(n), 1, 1)
    assert np.array_equal(small["actions"].view(np.uint32), draws(n, paths, horizon)[:, 0, 0].view(np.uint32))


# ---------------------------------------------------------------------------------------------------- every shape edge
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("horizon", [1, 2, 20])
@pytest.mark.parametrize("paths", [1, 15, 16, 17, 63, 64, 65, 200, 257])
def test_shapes(torch, paths, horizon, n):
    W, net = net_of("ref_200_100")
    obs = dr.sample_obs(n)
    out = plan(torch, net, obs, horizon, paths)
    check_plan(W, obs, out, draws(n, paths, horizon), "shape %dx%dx%d" % (n, paths, horizon))


def test_persistent_grid_loops(torch):
    """more tiles than the grid has waves (4 per compute unit for the 118 KB image): a wave takes a second tile"""
    W, net = net_of("ref_200_100")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, horizon = 3, 2
    paths = 16 * ((4 * cus) // n + 2) + 1                 # n * ceil(paths / 16) = 4 cus + 9 tiles at least
    assert n * ((paths + 15) // 16) > 4 * cus and paths <= 65536
    obs = dr.sample_obs(n)
    out = plan(torch, net, obs, horizon, paths)
    check_plan(W, obs, out, draws(n, paths, horizon), "grid loop %dx%d" % (n, paths))


# ---------------------------------------------------------------------------------------------------- every net
@pytest.mark.parametrize("name", ["ref_200_100", "he_128_128", "he_64_64", "he_20_10", "he_100_50", "dead", "cancel"])
def test_steps_scores_and_winner(torch, name):
    W, net = net_of(name)
    n, paths, horizon = 3, 65, 20
    obs = dr.sample_obs(n)
    obs[1] *= 6.0                                         # one env far out: large activations
    out = plan(torch, net, obs, horizon, paths)
    r_step, _ = check_plan(W, obs, out, draws(n, paths, horizon), name)
    if name.startswith(("he_", "ref_")):
        assert r_step > 1e-3                              # on the generic nets the bound is within a small factor of what float32 does
    if name == "dead":
        x = np.concatenate([obs, draws(n, paths, horizon)[:, 0, 0]], axis=1).astype(np.float64)
        z = ((x - W["in_mean"]) * dr.rscale(W)) @ W["w1"].astype(np.float64).T + W["b1"]
        assert 0.3 < (z <= 0).mean() < 0.9


# ---------------------------------------------------------------------------------------------------- every width edge
@pytest.mark.parametrize("name", dr.EDGE_SETS)
def test_edge_widths(torch, name):
    """dense nets at the widths where the packer masks a partly filled block of 16, where the router changes the instantiation
    and at both maxima (dynplan_ref.EDGE_WIDTHS); tests/test_dynplan_cpu.py holds that on these very steps a dropped last unit
    of either hidden layer is out of bound.  Two tiles of 16 candidates and a ragged third, the second env far out."""
    W, net = net_of(name)
    assert (SEED, GID0, K0) == (dr.EDGE_SEED, dr.EDGE_GID0, dr.EDGE_K)
    assert net.compiled == dr.EDGE_WIDTHS[(net.h1, net.h2)] and dr.edge_name(net.h1, net.h2) == name
    n, paths, horizon = dr.EDGE_N, dr.EDGE_PATHS, dr.EDGE_HORIZON
    obs = dr.edge_obs()
    out = plan(torch, net, obs, horizon, paths)
    check_plan(W, obs, out, draws(n, paths, horizon), name)


def test_without_optional_outputs(torch):
    """every nullable output NULL: the scores go through the workspace, the last prediction is not computed, same winner"""
    W, net = net_of("ref_200_100")
    obs = dr.sample_obs(3)
    full = plan(torch, net, obs, 20, 65)
    bare = plan(torch, net, obs, 20, 65, want=())
    assert set(bare) == {"actions"} and np.array_equal(bare["actions"].view(np.uint32), full["actions"].view(np.uint32))
    some = plan(torch, net, obs, 20, 65, want=("best_score", "scores"))
    assert np.array_equal(some["scores"].view(np.uint64), full["scores"].view(np.uint64))
    assert np.array_equal(some["best_score"].view(np.uint64), full["best_score"].view(np.uint64))


# ---------------------------------------------------------------------------------------------------- ties and NaN
def test_all_ties_index_zero_wins(torch):
    W, net = net_of("zero")
    n, paths, horizon = 3, 200, 20
    obs = dr.sample_obs(n)
    out = plan(torch, net, obs, horizon, paths)
    assert np.array_equal(out["traj"], np.broadcast_to(obs[:, None, None, :], out["traj"].shape))
    assert (out["scores"] == out["scores"][:, :1]).all() and (out["best_index"] == 0).all()
    check_plan(W, obs, out, draws(n, paths, horizon), "zero")


def test_nan_observation_gives_index_zero_and_leaves_the_others(torch):
    W, net = net_of("ref_200_100")
    n, paths, horizon = 3, 65, 20
    obs = dr.sample_obs(n)
    clean = plan(torch, net, obs, horizon, paths)
    bad = obs.copy()
    bad[1, 0] = np.nan
    out = plan(torch, net, bad, horizon, paths)
    acts = draws(n, paths, horizon)
    assert np.isnan(out["scores"][1]).all() and out["best_index"][1] == 0 and np.isnan(out["best_score"][1])
    assert np.array_equal(out["best_score"].view(np.uint64)[1], out["scores"].view(np.uint64)[1, 0])
    assert np.array_equal(out["actions"][1].view(np.uint32), acts[1, 0, 0].view(np.uint32))
    assert np.array_equal(out["sequence"][1].view(np.uint32), acts[1, 0].view(np.uint32))
    for name in out:
        for i in (0, 2):
            a, b = out[name][i:i + 1], clean[name][i:i + 1]
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, i)


# ---------------------------------------------------------------------------------------------------- mapping-independence
def test_scores_do_not_depend_on_paths_or_n(torch):
    W, net = net_of("ref_200_100")
    obs = dr.sample_obs(3)
    wide = plan(torch, net, obs, 20, 1024, want=("scores", "best_index", "best_score"))
    narrow = plan(torch, net, obs, 20, 200, want=("scores", "traj"))
    assert np.array_equal(narrow["scores"].view(np.uint64), wide["scores"][:, :200].view(np.uint64))
    for i in range(3):
        alone = plan(torch, net, obs[i:i + 1], 20, 200, gid0=GID0 + i, want=("scores", "traj"))
        assert np.array_equal(alone["scores"].view(np.uint64), narrow["scores"][i:i + 1].view(np.uint64))
        assert np.array_equal(alone["traj"].view(np.uint32), narrow["traj"][i:i + 1].view(np.uint32))
        assert np.array_equal(alone["actions"].shape, (1, 4))


def test_padding_is_invisible(torch):
    """a (100, 50) net and the same net hand-padded with zero units to (128, 128): the same bits (k_dyn_pack pads the first);
    likewise three of the width edges and their paddings"""
    W, net = net_of("he_100_50")
    P = dr.pad_net(W, 128, 128)
    padded = dr.to_net(P, "cuda")
    assert net.compiled == padded.compiled == (128, 128)
    obs = dr.sample_obs(3)
    a, b = plan(torch, net, obs, 20, 65), plan(torch, padded, obs, 20, 65)
    for name in a:
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
    assert np.array_equal(net.pack().cpu().numpy(), padded.pack().cpu().numpy())
    check_plan(W, obs, a, draws(3, 65, 20), "he_100_50")
    # the width edges: padded to the next multiple of 4 (what the fit rounds to) and to the compiled pair, across a tile
    # boundary by one unit, and from one unit of layer 2 to a full image
    n, paths, horizon = dr.EDGE_N, dr.EDGE_PATHS, dr.EDGE_HORIZON
    obs = dr.edge_obs()
    for name, to in (("edge_21_11", (24, 12)), ("edge_21_11", (64, 64)), ("edge_65_3", (128, 128)), ("edge_129_1", (208, 112))):
        W, net = net_of(name)
        padded = dr.to_net(dr.pad_net(W, *to), "cuda")
        assert (padded.h1, padded.h2) == to and net.compiled == padded.compiled == dr.EDGE_WIDTHS[(net.h1, net.h2)]
        a, b = plan(torch, net, obs, horizon, paths), plan(torch, padded, obs, horizon, paths)
        assert set(a) == {"actions", "best_score", "best_index", "sequence", "scores", "traj"}
        for out in a:
            assert np.array_equal(a[out].view(np.uint8), b[out].view(np.uint8)), (name, to, out)
        assert np.array_equal(net.pack().cpu().numpy(), padded.pack().cpu().numpy()), (name, to)


# ---------------------------------------------------------------------------------------------------- independent wiring check
def test_wiring_closed_form(torch):
    """delta[0:3] = 0.1 a[0:3], the rest 0: the trajectory is obs + 0.1 cumsum(a) in float64 from the draws -- no code shared with
    step64.  Bound of |device score - closed form| per candidate: per step the position takes two roundings, fl(a * 0.1f) and the
    addition, and 0.1f differs from 0.1 by at most u 0.1, so e_{h+1} = e_h + u (|0.1 a| + |p_{h+1}| + e_h) + u |0.1 a|; a score term
    moves by at most sum_j (2 |p_j| e + e^2), plus score_bound's roundings of the terms themselves.  The kernel's winner W and
    the closed-form best B: cf(W) >= dev(W) - b >= dev(B) - b >= cf(B) - 2 b."""
    W, net = net_of("wiring")
    n, paths, horizon = 3, 200, 20
    obs = dr.sample_obs(n)
    out = plan(torch, net, obs, horizon, paths)
    acts = draws(n, paths, horizon).astype(np.float64)
    step = 0.1 * acts[..., :3]
    pos = obs[:, None, None, :3].astype(np.float64) + np.concatenate([np.zeros((n, paths, 1, 3)), np.cumsum(step, axis=2)[:, :, :-1]], axis=2)
    closed = -np.sum(pos ** 2, axis=(2, 3))
    e = np.zeros((n, paths, 3))
    b = np.zeros((n, paths))
    for h in range(horizon):
        b += np.sum(2 * np.abs(pos[:, :, h]) * e + e * e, axis=-1)
        nxt = np.abs(pos[:, :, h]) + np.abs(step[:, :, h])
        e = e + dr.U32 * (np.abs(step[:, :, h]) + nxt + e) + dr.U32 * np.abs(step[:, :, h])
    full = np.zeros((n, paths, horizon, 12)); full[..., :3] = np.abs(pos) + 1e-3
    b += dr.score_bound(full)
    assert (np.abs(out["scores"] - closed) <= b).all(), float((np.abs(out["scores"] - closed) / b).max())
    win = out["best_index"]
    assert (closed[np.arange(n), win] >= closed.max(axis=1) - 2 * b.max(axis=1)).all()
    # the other nine observation words never move
    assert np.array_equal(out["traj"][..., 3:], np.broadcast_to(obs[:, None, None, 3:], out["traj"][..., 3:].shape))
    check_winner(out, draws(n, paths, horizon), "wiring")
    print("dynplan ratio wiring closed-form worst err/bound %.3g" % float((np.abs(out["scores"] - closed) / b).max()))


# ---------------------------------------------------------------------------------------------------- the public path
def test_stream_order(torch):
    """plan, change obs in place on the same stream, plan again, no host synchronisation in between = the two plans apart"""
    import quadsim_amd as qa
    W, net = net_of("ref_200_100")
    o1, o2 = dr.sample_obs(3, seed=51), dr.sample_obs(3, seed=52)
    kw = dict(horizon=20, paths=200, seed=SEED, k=K0, gid0=GID0, return_scores=True, return_sequence=True)
    t1, t2 = torch.as_tensor(o1).cuda(), torch.as_tensor(o2).cuda()
    sep1 = {k: v.cpu().numpy() for k, v in qa.learned_shooting_plan(net, t1, **kw).items()}
    sep2 = {k: v.cpu().numpy() for k, v in qa.learned_shooting_plan(net, t2, **kw).items()}
    torch.cuda.synchronize()
    buf = t1.clone()
    a = qa.learned_shooting_plan(net, buf, **kw)
    buf.copy_(t2)
    b = qa.learned_shooting_plan(net, buf, **kw)
    torch.cuda.synchronize()
    for k in sep1:
        assert np.array_equal(a[k].cpu().numpy().view(np.uint8), sep1[k].view(np.uint8)), k
        assert np.array_equal(b[k].cpu().numpy().view(np.uint8), sep2[k].view(np.uint8)), k
    raw = plan(torch, net, o1, 20, 200)
    assert np.array_equal(raw["scores"].view(np.uint64), sep1["scores"].view(np.uint64))
    assert np.array_equal(raw["actions"].view(np.uint32), sep1["actions"].view(np.uint32))


def test_repack_follows_the_weights(torch):
    """pack() is cached, and rebuilt after an in-place update of a weight: the plan then agrees with the new weights"""
    import quadsim_amd as qa
    W = {k: np.array(v, copy=True) for k, v in dr.weight_set("he_64_64").items()}
    net = dr.to_net(W, "cuda")
    img = net.pack()
    assert net.pack() is img
    obs = dr.sample_obs(2)
    before = plan(torch, net, obs, 3, 17)
    net.w3.mul_(0.5)
    W["w3"] = W["w3"] * np.float32(0.5)
    after = plan(torch, net, obs, 3, 17)
    assert not np.array_equal(before["traj"], after["traj"])
    check_plan(W, obs, after, draws(2, 17, 3), "repacked")
    t = qa.learned_shooting_plan(net, torch.as_tensor(obs).cuda(), 3, 17, seed=SEED, k=K0, gid0=GID0, return_traj=True)
    assert np.array_equal(t["traj"].cpu().numpy().view(np.uint32), after["traj"].view(np.uint32))


def test_learned_mpc_closed_loop(torch):
    """LearnedShootingMPC on a VecDockingEnv and on the single-env shim: obs, k, seed and gid0 come from the env"""
    import quadsim_amd as qa
    W, net = net_of("he_20_10")
    env = qa.VecDockingEnv("docking-v0", num_envs=3, seed=11, env_id_offset=5)
    obs = env.reset()
    env.step(env.random_actions(1)[0])
    mpc = qa.LearnedShootingMPC(env, net, horizon=5, paths=17)
    a = mpc.act()
    ref = plan(torch, net, env._obs.cpu().numpy(), 5, 17, seed=11, gid0=5, k=env.step_counter)
    assert np.array_equal(a.cpu().numpy().view(np.uint32), ref["actions"].view(np.uint32))
    rew, done = mpc.run(2)
    assert tuple(rew.shape) == (2, 3) and tuple(done.shape) == (2, 3) and env.step_counter == 3
    env.close()
    one = qa.DockingEnv()
    o = one.reset()
    m1 = qa.LearnedShootingMPC(one, net, horizon=5, paths=17)
    a1 = m1.act()
    ref1 = plan(torch, net, np.asarray(o, np.float32)[None], 5, 17, seed=int(one.cfg.seed), gid0=int(one.cfg.env_id_offset), k=0)
    assert a1.shape == (4,) and a1.dtype == np.float32 and np.array_equal(a1.view(np.uint32), ref1["actions"][0].view(np.uint32))
    r1, d1 = m1.run(2)
    assert tuple(r1.shape) == (2, 1)
    one.close()
    del obs
