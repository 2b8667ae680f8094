"""MPPI over the learned dynamics net on the device (qsdm_mppi_plan of libquadsim_dynmppi.so) against tests/dynmppi_ref.py's
parts: tests/mppi_ref.py for the candidates and the update, tests/dynplan_ref.py for the model step and the score.

Every call goes through `plan`, which puts each output buffer and the workspace between 256 sentinel bytes on both sides and
checks them afterwards.  What is held, on every element of every output:
  candidates  with caller noise and the kernel's own trace[it], candidates = mppi_ref.candidates32, bit for bit; with keyed
              draws the normals recovered from the unclamped candidates against mppi_ref.normals within NORMAL_TOL
  steps       |traj[env, c, h] - step64(traj[env, c, h - 1], candidates[env, c, h])| <= the derived bound at that input, one
              float32 model step at a time from the kernel's OWN inputs
  scores      against cost64 of the kernel's own trajectory, within score_bound
  update      trace[it + 1] against mppi_ref.update64 of the kernel's own scores and candidates within UPDATE_TOL; actions =
              nominal[:, 0] = trace[:, -1, 0] and best_score = nanmax(scores[:, -1]) bit for bit
  earlier iterations through the prefix property: scores[:, :j] and trace[:, :j + 1] of a 3-iteration call are those of the
              j-iteration call bit for bit, whose candidates and traj are iteration j - 1's
The mapping has edges at 16 candidates (a wave's tile), 64 (a roll-out workgroup's four tiles), 128 (the update workgroup's
rows), 1024 (its threads), 8 horizon steps (a row's lanes) and at cus x 4 tiles, where the persistent grid starts to loop.  The
tests over the nets also run a dense net at every width edge of dynplan_ref.EDGE_WIDTHS.  Measured worst ratios are in
profiles/dynmppi/README.md and profiles/dyn_edges/README.md."""
import ctypes as C

import numpy as np
import pytest

import dynmppi_ref
import dynplan_ref as dr
import mppi_ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
GID0 = (1 << 32) - 2                 # env ids on both sides of 2^32 with n = 3 (tests/test_gpu_dynplan.py)
K0 = (1 << 32) + 5                   # k << 30 needs the upper word of the block index; below 2^33
GUARD = 256
LAM, SIGMA = 0.5, 0.4
# tests/test_gpu_mppi.py's: the update is float64 on the device and rounded to float32 once (values in [-1, 1]): one rounding
# plus the reference's own; the normals' tolerance is four times the error measured there over 7.67e6 draws
UPDATE_TOL = 2.0 * 2.0 ** -24
NORMAL_TOL = 4.0 * 1.7e-6
NETS = ["he_20_10", "he_128_128", "ref_200_100"]       # one per instantiation: (64, 64), (128, 128), (208, 112)
EDGES = list(dr.EDGE_SETS)                              # every width edge: tests/dynplan_ref.py's EDGE_WIDTHS
OUTPUTS = ("actions", "nominal", "best_score", "scores", "trace", "candidates", "traj")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_nets = {}


def net_of(name):
    if name not in _nets:
        W = dr.weight_set(name)
        _nets[name] = (W, dr.to_net(W, "cuda"))
    return _nets[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def plan(torch, net, obs, horizon, paths, iterations=1, lam=LAM, sigma=SIGMA, shift=0, nominal=None, noise=None, seed=SEED, gid0=GID0,
         k=K0, want=OUTPUTS[2:], widths=None, alias=False, filled=False):
    """qsdm_mppi_plan with every output between sentinel bytes -> dict of numpy arrays (`alias`: nominal_in IS nominal_out;
    `filled`: the raw bytes of the outputs instead, for a call that must write nothing)"""
    from quadsim_amd import dynplan
    lib = dynplan.load_mppi()
    obs_t = torch.as_tensor(np.ascontiguousarray(obs, np.float32)).cuda()
    n = obs_t.shape[0]
    shapes = {"actions": ((n, 4), torch.float32), "nominal": ((n, horizon, 4), torch.float32), "best_score": ((n,), torch.float64),
              "scores": ((n, iterations, paths), torch.float64), "trace": ((n, iterations + 1, horizon, 4), torch.float32),
              "candidates": ((n, paths, horizon, 4), torch.float32), "traj": ((n, paths, horizon, 12), torch.float32)}
    raw, view = {}, {}
    for name in ("actions", "nominal") + tuple(want):
        shape, dtype = shapes[name]
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        raw[name] = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        view[name] = raw[name][GUARD:GUARD + nbytes].view(dtype).view(shape)
    wb = C.c_size_t(0)
    dynplan.check_mppi(lib.qsdm_workspace_bytes(n, horizon, paths, C.byref(wb)), "qsdm_workspace_bytes")
    assert wb.value == n * horizon * 16 + n * paths * 8
    raw["workspace"] = torch.full((GUARD + wb.value + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    p = lambda name: C.c_void_p(view[name].data_ptr()) if name in view else None     # noqa: E731
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()     # noqa: E731
    nominal_t, noise_t = t(nominal), t(noise)
    if alias:
        view["nominal"].copy_(nominal_t)
        nominal_t = view["nominal"]
    q = lambda a: None if a is None else C.c_void_p(a.data_ptr())     # noqa: E731
    h1, h2 = widths or (net.h1, net.h2)
    image = net.pack()
    dynplan.check_mppi(lib.qsdm_mppi_plan(C.c_void_p(image.data_ptr()), h1, h2, n, C.c_void_p(obs_t.data_ptr()), seed, gid0, k, horizon,
                                          paths, iterations, lam, sigma, shift, q(nominal_t), q(noise_t),
                                          C.c_void_p(raw["workspace"].data_ptr() + GUARD), p("actions"), p("nominal"), p("best_score"),
                                          p("scores"), p("trace"), p("candidates"), p("traj"),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "qsdm_mppi_plan")
    torch.cuda.synchronize()
    for name, r in raw.items():
        g = torch.cat([r[:GUARD], r[-GUARD:]])
        assert bool((g == 0xA5).all()), "sentinel bytes around %s were overwritten" % name
    if filled:
        return {name: r.cpu().numpy() for name, r in raw.items()}
    return {name: v.cpu().numpy() for name, v in view.items()}


def check_last_iteration(W, obs, out, lam, what):
    """steps, scores, update and the identities of the module's docstring on the LAST iteration of one plan -> the worst
    (step err / bound, score err / bound, update err)"""
    cands, traj, scores, trace = out["candidates"], out["traj"], out["scores"], out["trace"]
    n, paths, horizon = cands.shape[:3]
    assert traj.shape == (n, paths, horizon, 12) and scores.shape[0::2] == (n, paths) and trace.shape[1] == scores.shape[1] + 1
    assert np.all(np.abs(cands) <= 1.0)
    before = np.concatenate([np.repeat(np.asarray(obs, np.float32)[:, None, None, :], paths, axis=1), traj[:, :, :-1]], axis=2)
    ref, bound = dr.step64(W, before, cands, with_bound=True)
    err = np.abs(traj.astype(np.float64) - ref)
    ok = err <= bound                                    # NaN inputs: handled by the caller, never excluded here
    r_step = float((err / bound).max())
    print("dynmppi ratio %s steps worst err/bound %.3g over %d elements" % (what, r_step, err.size))
    assert ok.all(), "%s: %d of %d trajectory elements out of bound, worst err / bound %.3g" % (what, int((~ok).sum()), ok.size, r_step)
    S = scores[:, -1]
    sb = dr.score_bound(before)
    serr = np.abs(S - dr.cost64(before))
    r_score = float((serr / np.maximum(sb, 1e-300)).max())
    print("dynmppi ratio %s scores worst err/bound %.3g" % (what, r_score))
    assert (serr <= sb).all(), "%s: scores out of bound, worst ratio %.3g" % (what, r_score)
    want = mppi_ref.update64(S, cands, lam, trace[:, -2])
    uerr = float(np.max(np.abs(trace[:, -1].astype(np.float64) - want)))
    print("dynmppi update %s worst |update - f64| %.3g (bound %.3g)" % (what, uerr, UPDATE_TOL))
    assert uerr <= UPDATE_TOL, (what, uerr)
    assert same_bits(cands[:, 0], np.clip(trace[:, -2], np.float32(-1), np.float32(1))), what
    assert same_bits(out["nominal"], trace[:, -1]) and same_bits(out["actions"], out["nominal"][:, 0]), what
    assert same_bits(out["best_score"], np.nanmax(S, axis=1)), what
    return r_step, r_score, uerr


def check_prefix(full, part, j, what):
    assert same_bits(part["scores"], full["scores"][:, :j]), (what, j)
    assert same_bits(part["trace"], full["trace"][:, :j + 1]), (what, j)


# ---------------------------------------------------------------------------------------------------- every shape edge
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("horizon", [1, 2, 5])
@pytest.mark.parametrize("paths", [1, 15, 16, 17, 63, 64, 65, 257])
def test_shapes_keyed_draws_every_iteration(torch, paths, horizon, n):
    """keyed draws, warm start through the shift: iterations 1, 2 and 3, each checked on its own last iteration, and the prefix"""
    W, net = net_of("ref_200_100")
    obs = dr.sample_obs(n)
    nominal = np.random.default_rng(5).uniform(-0.6, 0.6, (n, horizon, 4)).astype(np.float32)
    full = None
    for j in (3, 2, 1):
        out = plan(torch, net, obs, horizon, paths, j, nominal=nominal, shift=1)
        full = full or out
        check_prefix(full, out, j, (n, paths, horizon))
        check_last_iteration(W, obs, out, LAM, "shape %dx%dx%d it %d" % (n, paths, horizon, j))
    assert same_bits(full["trace"][:, 0], dynmppi_ref.shifted(nominal, horizon, 1))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("horizon", [1, 2, 5])
@pytest.mark.parametrize("paths", [1, 15, 16, 17, 63, 64, 65, 257])
@pytest.mark.parametrize("iterations", [1, 3])
def test_candidates_exact_with_caller_noise(torch, iterations, paths, horizon, n):
    """caller noise; a nominal beyond the clamp and a -0; no nominal, shift 0 and shift 1"""
    W, net = net_of("he_20_10")
    obs = dr.sample_obs(n)
    rng = np.random.default_rng(7)
    noise = rng.standard_normal((iterations, paths, horizon, 4)).astype(np.float32)
    nominal = rng.uniform(-1.2, 1.2, (n, horizon, 4)).astype(np.float32)
    nominal[0, 0, 0] = -0.0
    for shift, nom in ((0, None), (1, nominal), (0, nominal)):
        out = plan(torch, net, obs, horizon, paths, iterations, noise=noise, nominal=nom, shift=shift)
        key = (paths, horizon, iterations, shift, nom is None)
        assert same_bits(out["trace"][:, 0], dynmppi_ref.shifted(nom, horizon, shift, n)), key
        assert same_bits(out["candidates"], mppi_ref.candidates32(out["trace"][:, iterations - 1], SIGMA, noise[iterations - 1])), key
        check_last_iteration(W, obs, out, LAM, "noise %s" % (key,))


@pytest.mark.parametrize("paths,horizon", [(127, 7), (128, 8), (129, 9), (1023, 2), (1024, 16), (1025, 17)])
def test_update_workgroup_edges(torch, paths, horizon):
    """the update workgroup has 1024 threads in 128 rows of 8 lanes: a row takes a second candidate at 129 paths, a thread a
    second score at 1025, and a row's lanes a second chunk of horizon steps at 9 (a third at 17)"""
    W, net = net_of("he_20_10")
    obs = dr.sample_obs(2)
    nominal = np.random.default_rng(31).uniform(-0.6, 0.6, (2, horizon, 4)).astype(np.float32)
    out = plan(torch, net, obs, horizon, paths, 2, nominal=nominal, shift=1)
    check_last_iteration(W, obs, out, LAM, "update edge 2x%dx%d" % (paths, horizon))


def test_persistent_grid_loops(torch):
    """one tile more than the grid has waves (4 per compute unit for the 118 KB image): a wave takes a second tile"""
    W, net = net_of("ref_200_100")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    paths = cus * 4 * 16 + 1
    assert paths <= 65536
    obs = dr.sample_obs(1)
    out = plan(torch, net, obs, 2, paths, 2)
    check_last_iteration(W, obs, out, LAM, "grid loop 1x%d" % paths)


# ---------------------------------------------------------------------------------------------------- every net
def case_of(name, net, far):
    """-> (n, paths, horizon, obs, iterations) of a test over NETS + EDGES: the width edges run tests/dynplan_ref.py's small
    shape (two tiles of 16 candidates and a ragged third, the second env far out) with two iterations"""
    if name in EDGES:
        assert net.compiled == dr.EDGE_WIDTHS[(net.h1, net.h2)] and dr.edge_name(net.h1, net.h2) == name
        return dr.EDGE_N, dr.EDGE_PATHS, dr.EDGE_HORIZON, dr.edge_obs(), 2
    obs = dr.sample_obs(3)
    if far:
        obs[1] *= 6.0                                     # one env far out: large activations
    return 3, 65, 5, obs, 3


@pytest.mark.parametrize("name", NETS + EDGES)
def test_steps_scores_and_update(torch, name):
    W, net = net_of(name)
    n, paths, horizon, obs, iterations = case_of(name, net, far=True)
    full = None
    for lam in (0.05, 2.0):                               # a peaked and a flat weighting
        for j in (iterations, 1):
            out = plan(torch, net, obs, horizon, paths, j, lam=lam)
            r_step, _, _ = check_last_iteration(W, obs, out, lam, "%s lam %g it %d" % (name, lam, j))
            assert r_step > 1e-3 or name in EDGES         # on the generic nets the bound is within a small factor of what float32 does
            if j == iterations:
                full = out
            check_prefix(full, out, j, (name, lam))
        assert not same_bits(full["trace"][:, 1], full["trace"][:, 0])


# ---------------------------------------------------------------------------------------------------- keyed draws
def test_in_kernel_normals_against_float64(torch):
    """tests/test_gpu_mppi.py's recipe: zero nominal, sigma = 0.25 (0.25 z is exact, so an unclamped candidate / 0.25 is z)"""
    W, net = net_of("he_20_10")
    sigma, paths, horizon, n = 0.25, 1000, 5, 3
    obs = dr.sample_obs(n)
    assert GID0 < 1 << 32 <= GID0 + 2 and 1 << 32 < K0 < 1 << 33
    out = plan(torch, net, obs, horizon, paths, 1, sigma=sigma, want=("candidates",))
    cand = out["candidates"]
    assert np.all(cand[:, 0] == 0.0)
    z64 = np.stack([mppi_ref.normals(SEED, GID0 + i, K0, 0, paths, horizon) for i in range(n)])
    free = np.abs(cand) < 1.0
    free[:, 0] = False
    assert free[:, 1:].mean() > 0.999
    err = float(np.max(np.abs(cand.astype(np.float64)[free] / sigma - z64[free])))
    print("dynmppi max |z_dev - z_64| over %d draws = %.4g (asserted at %.4g)" % (int(free.sum()), err, NORMAL_TOL))
    clamped = ~free
    clamped[:, 0] = False
    assert np.all(np.abs(z64[clamped]) >= 4.0 - 1e-3)
    assert err <= NORMAL_TOL
    assert not np.array_equal(cand[0], cand[1])
    # iteration 2's draws are iteration 2's blocks: cand = fl(sigma z + U) with |cand| <= 1, one more rounding of at most 2^-24
    three = plan(torch, net, obs, horizon, paths, 3, sigma=sigma, lam=1e6, want=("candidates", "trace"))
    z2 = np.stack([mppi_ref.normals(SEED, GID0 + i, K0, 2, paths, horizon) for i in range(n)])
    got = (three["candidates"].astype(np.float64) - three["trace"][:, 2][:, None].astype(np.float64)) / sigma
    free = np.abs(three["candidates"]) < 1.0
    free[:, 0] = False
    assert float(np.max(np.abs(got[free] - z2[free]))) <= NORMAL_TOL + 2.0 ** -24 / sigma
    nxt = plan(torch, net, obs, horizon, paths, 1, sigma=sigma, k=K0 + 1, want=("candidates",))
    assert float(np.mean(np.abs(nxt["candidates"][:, 1:] - cand[:, 1:]))) > 0.1 * sigma


# ---------------------------------------------------------------------------------------------------- one model step
@pytest.mark.parametrize("name", NETS + EDGES)
def test_model_step_is_the_shooting_planner_s(torch, name):
    """paths = 1, iterations = 1, shift 0 and the nominal = the winner's sequence of qsd_shooting_plan for the same (net, obs):
    candidate 0 is clamp(U) = U, and its trajectory is that plan's traj[:, best] bit for bit"""
    import quadsim_amd as qa
    W, net = net_of(name)
    n, paths, horizon, obs, _ = case_of(name, net, far=False)
    shot = qa.learned_shooting_plan(net, torch.as_tensor(obs).cuda(), horizon, paths, seed=SEED, k=K0, gid0=GID0, return_sequence=True,
                                    return_traj=True)
    seq = shot["sequence"].cpu().numpy()
    best = shot["best_index"].cpu().numpy()
    out = plan(torch, net, obs, horizon, 1, 1, nominal=seq)
    assert same_bits(out["candidates"][:, 0], seq)
    assert same_bits(out["traj"][:, 0], shot["traj"].cpu().numpy()[np.arange(n), best])


# ---------------------------------------------------------------------------------------------------- mapping-independence
def test_an_env_planned_alone_and_fewer_paths(torch):
    W, net = net_of("ref_200_100")
    obs = dr.sample_obs(3)
    nominal = np.random.default_rng(17).uniform(-0.5, 0.5, (3, 5, 4)).astype(np.float32)
    batch = plan(torch, net, obs, 5, 65, 3, nominal=nominal, shift=1)
    alone = plan(torch, net, obs[1:2], 5, 65, 3, nominal=nominal[1:2], shift=1, gid0=GID0 + 1)
    for name in batch:
        assert same_bits(batch[name][1:2], alone[name]), name
    narrow = plan(torch, net, obs, 5, 17, 1, want=("scores", "candidates", "traj"))
    wide = plan(torch, net, obs, 5, 257, 1, want=("scores", "candidates", "traj"))
    for name in ("scores", "candidates", "traj"):
        a, b = (narrow[name], wide[name][:, :, :17]) if name == "scores" else (narrow[name], wide[name][:, :17])
        assert same_bits(a, np.ascontiguousarray(b)), name


@pytest.mark.parametrize("iterations", [1, 3])
def test_aliased_nominal_and_shift(torch, iterations):
    W, net = net_of("he_20_10")
    obs = dr.sample_obs(3)
    nominal = np.random.default_rng(19).uniform(-0.5, 0.5, (3, 5, 4)).astype(np.float32)
    for shift in (0, 1):
        apart = plan(torch, net, obs, 5, 65, iterations, nominal=nominal, shift=shift)
        same = plan(torch, net, obs, 5, 65, iterations, nominal=nominal, shift=shift, alias=True)
        for name in apart:
            assert same_bits(apart[name], same[name]), (name, shift)
        assert same_bits(apart["trace"][:, 0], nominal[:, [1, 2, 3, 4, 4]] if shift else nominal)
        assert not same_bits(apart["nominal"], apart["trace"][:, 0])


def test_without_optional_outputs(torch):
    W, net = net_of("ref_200_100")
    obs = dr.sample_obs(3)
    full = plan(torch, net, obs, 5, 65, 3)
    bare = plan(torch, net, obs, 5, 65, 3, want=())
    assert set(bare) == {"actions", "nominal"}
    some = plan(torch, net, obs, 5, 65, 3, want=("best_score", "scores"))
    for part in (bare, some):
        for name in part:
            assert same_bits(part[name], full[name]), name


# ---------------------------------------------------------------------------------------------------- NaN, the image check
def test_nan_observation_leaves_the_nominal_and_the_other_envs(torch):
    W, net = net_of("ref_200_100")
    n, paths, horizon = 3, 65, 5
    obs = dr.sample_obs(n)
    nominal = np.random.default_rng(23).uniform(-0.5, 0.5, (n, horizon, 4)).astype(np.float32)
    clean = plan(torch, net, obs, horizon, paths, 3, nominal=nominal, shift=1)
    bad = obs.copy()
    bad[1, 0] = np.nan
    out = plan(torch, net, bad, horizon, paths, 3, nominal=nominal, shift=1)
    assert np.isnan(out["scores"][1]).all() and out["best_score"][1] == -np.inf
    U0 = dynmppi_ref.shifted(nominal, horizon, 1)
    assert same_bits(out["nominal"][1], U0[1]) and same_bits(out["actions"][1], U0[1, 0])
    assert all(same_bits(out["trace"][1, j], U0[1]) for j in range(4))
    for name in out:
        for i in (0, 2):
            assert same_bits(out[name][i:i + 1], clean[name][i:i + 1]), (name, i)


def test_an_image_of_another_instantiation_writes_nothing(torch):
    W, net = net_of("he_20_10")
    assert net.compiled == (64, 64)
    obs = dr.sample_obs(3)
    for widths in ((128, 128), (200, 100)):
        raw = plan(torch, net, obs, 5, 65, 3, widths=widths, want=OUTPUTS[2:], filled=True)
        assert set(raw) == set(OUTPUTS) | {"workspace"}
        for name, r in raw.items():
            assert (r == 0xA5).all(), (widths, name)
    ok = plan(torch, net, obs, 5, 65, 3, widths=(64, 10))      # any widths of the same compiled pair are the same image
    assert same_bits(ok["nominal"], plan(torch, net, obs, 5, 65, 3)["nominal"])


# ---------------------------------------------------------------------------------------------------- the public path
def test_public_plan_and_stream_order(torch):
    """learned_mppi_plan is the raw call; plan, change obs in place on the same stream, plan again = the two plans apart"""
    import quadsim_amd as qa
    W, net = net_of("ref_200_100")
    o1, o2 = dr.sample_obs(3, seed=51), dr.sample_obs(3, seed=52)
    nominal = np.random.default_rng(29).uniform(-0.5, 0.5, (3, 5, 4)).astype(np.float32)
    kw = dict(horizon=5, paths=65, iterations=3, lam=LAM, sigma=SIGMA, nominal=torch.as_tensor(nominal).cuda(), shift=True, seed=SEED, k=K0,
              gid0=GID0, return_scores=True, return_trace=True, return_candidates=True, return_traj=True)
    raw1 = plan(torch, net, o1, 5, 65, 3, nominal=nominal, shift=1)
    raw2 = plan(torch, net, o2, 5, 65, 3, nominal=nominal, shift=1)
    buf = torch.as_tensor(o1).cuda()
    a = qa.learned_mppi_plan(net, buf, **kw)
    buf.copy_(torch.as_tensor(o2).cuda())
    b = qa.learned_mppi_plan(net, buf, **kw)
    torch.cuda.synchronize()
    assert set(a) == set(raw1)
    for name in raw1:
        assert same_bits(a[name].cpu().numpy(), raw1[name]), name
        assert same_bits(b[name].cpu().numpy(), raw2[name]), name


def test_learned_mppi_closed_loop(torch):
    """LearnedMPPI on a VecDockingEnv and on the single-env shim: obs, k, seed and gid0 come from the env; the nominal is carried
    with shift 1 and zeroed where an episode ended"""
    import quadsim_amd as qa
    W, net = net_of("he_20_10")

    def make():
        env = qa.VecDockingEnv("docking-v0", num_envs=3, seed=11, env_id_offset=5)
        env.reset()
        t0 = env.get_state()["t"].copy()
        t0[1] = 597.0                                     # env 1 times out inside the run
        env.set_state(t=t0)
        env.step(env.random_actions(1)[0])
        return env
    a, b = make(), make()
    ctl = qa.LearnedMPPI(a, net, horizon=5, paths=17, iterations=2, lam=LAM, sigma=SIGMA)
    rew, done = ctl.run(6)
    assert tuple(rew.shape) == (6, 3) and done.dtype == torch.bool and bool(done[:, 1].any()) and not bool(done.all())
    nominal = None
    for t in range(6):
        ref = plan(torch, net, b._obs.cpu().numpy(), 5, 17, 2, seed=11, gid0=5, k=b.step_counter, shift=int(nominal is not None),
                   nominal=nominal, want=())
        _, r, d, _ = b.step(torch.as_tensor(ref["actions"]).cuda())
        assert torch.equal(r, rew[t]) and torch.equal(d, done[t]), t
        nominal = ref["nominal"]
        nominal[d.cpu().numpy().astype(bool)] = 0.0
    assert same_bits(ctl.nominal.cpu().numpy(), nominal)
    ctl.reset()
    assert ctl.nominal is None
    a.close(); b.close()
    one = qa.DockingEnv()
    o = one.reset()
    m1 = qa.LearnedMPPI(one, net, horizon=5, paths=17, iterations=2, lam=LAM, sigma=SIGMA)
    a1 = m1.act()
    ref1 = plan(torch, net, np.asarray(o, np.float32)[None], 5, 17, 2, seed=int(one.cfg.seed), gid0=int(one.cfg.env_id_offset), k=0, want=())
    assert a1.shape == (4,) and a1.dtype == np.float32 and same_bits(a1, ref1["actions"][0])
    r1, d1 = m1.run(2)
    assert tuple(r1.shape) == (2, 1) and tuple(m1.nominal.shape) == (1, 5, 4)
    one.close()
