"""-m gpu: every instantiation of the PID-expert kernels (k_expert_action, k_expert_rollout, k_expert_evaluate), one row of
tests/expert_matrix.py each, run through the production dispatch and held to the float64 expert of tests/expert_ref.py.

Every buffer a kernel is handed (state_des, actions, the roll-out's and the evaluation's outputs) is a view into a larger device
tensor with 256 sentinel bytes on each side, checked after every call: a store outside a buffer shows as a changed sentinel byte,
never as a fault.  Every handle is checked to have the (INTEG, PARAMS, RMODE) of its row (qs_debug_step_variant: the fused entry
points dispatch on the same step_combo, qs_expert_action on PARAMS).

  action rows    the three regimes of expert_ref.inputs() x the three gain pairs at n = 1, 63, 65, 257, written with set_state
                 (t = 0 on the `first` envs) and, on the PARAMS row, set_params: every action and every word of
                 state_des[3:12] within KAPPA_EXPERT * 2^-24 * E of expert64, NO element excluded; state_des[0:3] and [12]
                 bit-unchanged, [3:6] bit-unchanged on a first step.
  roll-out rows  T = 12.  Handle `a` runs the loop qs_expert_action; qs_step, and before every qs_expert_action its state,
                 parameters and state_des are read back: that step's actions and state_des are held to expert64 of exactly what
                 the kernel read.  The env step is tied to float64 by tests/step_matrix.py and is not judged again.  The twin
                 `b` runs qs_expert_rollout in the row's layout and equals the loop bit for bit (outputs, final state,
                 parameters, step counter, state_des), as does a second call with T = 1.
  evaluation     K = 2 from t = 560..599: the first episode ends through the row's own reset, the second starts from it.  The
  rows           records equal those of the twin's 640-step loop (returns bit-equal float64 sums), the handle and state_des are
                 untouched.  One more case stops after 100 steps: the unfinished slots keep their sentinel bytes.
"""
import ctypes as C

import numpy as np
import pytest

import expert_ref as er
from expert_matrix import ACTION_ROWS, EVAL_ROWS, K, ROLLOUT_ROWS, T
from test_gpu_expert_rollout import _episodes
from test_gpu_postproc import Guards

pytestmark = pytest.mark.gpu

PAR_NOM = np.array([0.18, 0.00025, 0.000232, 0.0003738])
MASS_NOM32 = np.float32(0.18)


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class ExpertGuards(Guards):
    def inout(self, data):
        """a guarded buffer the kernel reads and writes: the bands are checked, the payload is not"""
        data = np.asarray(data)
        t = self._make(data.shape, data.dtype, data)
        self.items[-1] = self.items[-1][:3] + (False,)
        return t


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _variant(env):
    lib = env._lib
    lib.qs_debug_step_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 5)()
    assert lib.qs_debug_step_variant(env._h, out) == 0, lib.qs_last_error()
    return tuple(out)


def _handle(qa, row, n, seed):
    """the row's handle after a reset; identical for every call with the same arguments"""
    kw = dict(num_envs=n, randomise=row["randomise"], seed=seed, integrator=row["integ"], copy=False)
    if row["randomise"]:
        kw.update(init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2))
    env = qa.VecDockingEnv(row["env_id"], **kw)
    rng = np.random.default_rng(seed)
    if row["set_init"]:
        c = np.tile(np.array([8, -50, 5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32), (n, 1))
        c[:, 0:3] += rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
        env.set_init_state(c)
    env.reset()
    if row["set_params"]:
        env.set_params(mass=(0.18 * rng.uniform(0.8, 1.2, n)).astype(np.float32),
                       inertia=(PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))
    assert _variant(env)[1:4] == tuple(row["combo"]), (row["id"], _variant(env))
    return env


def _expert(qa, env, row, guards, seed, gains=None):
    """a PIDExpert on guarded buffers; a fifth of the envs (env % 5 == 2) wants a yaw of up to 1 rad and a yaw rate"""
    kp, kd = gains or row["gains"]
    ex = qa.PIDExpert(env, kp, kd)
    n = env.num_envs
    sd = ex.state_des.cpu().numpy().copy()
    rs = np.random.RandomState(seed)
    sel = np.arange(n) % 5 == 2
    yaw = rs.uniform(-1.0, 1.0, n)
    sd[sel, 6:10] = er._quat_yaw_tilt(yaw, np.zeros(n), np.zeros(n))[sel].astype(np.float32)
    sd[sel, 12] = rs.uniform(-0.5, 0.5, n)[sel].astype(np.float32)
    ex.state_des = guards.inout(sd)
    ex._actions = guards.out((n, 4))
    return ex


def _mass(env, row):
    return env.get_params()[0].copy() if row["combo"][1] else MASS_NOM32


def _act_checked(torch, env, ex, row, guards, what):
    """one qs_expert_action held to expert64 of the state, parameters and state_des it read -> (actions tensor, pre-step t, the
    two worst ratios)"""
    st = env.get_state()
    sd0 = ex.state_des.cpu().numpy().copy()
    first = st["t"] == 0
    a = ex.act()
    torch.cuda.synchronize()
    guards.check()
    got_a, got_sd = a.cpu().numpy(), ex.state_des.cpu().numpy()
    ref = er.expert64(sd0, st["chaser"], st["target"], first, np.float32(ex.kp), np.float32(ex.kd), _mass(env, row))
    ra, rs = er.check(got_a, got_sd, ref, what)
    assert _bits(got_sd[:, 0:3], sd0[:, 0:3]) and _bits(got_sd[:, 12], sd0[:, 12]), what + ": state_des[0:3] / [12] written"
    assert _bits(got_sd[first, 3:6], sd0[first, 3:6]), what + ": des_vel rewritten on a first step"
    assert (got_sd[:, 10:12] == 0).all(), what
    return a, st["t"], ra, rs


# ---------------------------------------------------------------------------------------------------- k_expert_action
@pytest.mark.parametrize("row", ACTION_ROWS, ids=[r["id"] for r in ACTION_ROWS])
def test_action_row(qa, torch, row):
    worst = {}
    for n in row["n"]:
        env = _handle(qa, row, n, seed=40 + n)
        for regime in er.REGIMES:
            for g, (kp, kd) in enumerate(row["gains"]):
                inp = er.inputs(regime, n, g, seed=1)
                if row["set_params"]:
                    env.set_params(mass=inp["mass"], inertia=np.tile(PAR_NOM[1:].astype(np.float32), (n, 1)))
                    assert _bits(env.get_params()[0], inp["mass"])
                t = np.where(inp["first"], 0.0, 1.0 + (np.arange(n) * 37) % 599).astype(np.float32)
                env.set_state(chaser=inp["chaser"], target=inp["target"], t=t)
                assert _variant(env)[1:4] == tuple(row["combo"])
                guards = ExpertGuards(torch, env.device)
                ex = qa.PIDExpert(env, kp, kd)
                ex.state_des, ex._actions = guards.inout(inp["state_des"]), guards.out((n, 4))
                what = "%s n %d %s gains %d" % (row["id"], n, regime, g)
                _, t_read, ra, rs = _act_checked(torch, env, ex, row, guards, what)
                assert _bits(t_read, t) and (np.asarray(t_read == 0) == inp["first"]).all()
                st = env.get_state()                                   # the env itself is only read
                assert _bits(st["chaser"], inp["chaser"]) and _bits(st["target"], inp["target"]) and _bits(st["t"], t)
                w = worst.setdefault(regime, [0.0, 0.0])
                w[0], w[1] = max(w[0], ra), max(w[1], rs)
        env.close()
    for regime, (ra, rs) in worst.items():
        print("expert ratio %s %-8s actions %.3f state_des %.3f" % (row["id"], regime, ra, rs))


# ---------------------------------------------------------------------------------------------------- k_expert_rollout
def _provoked(qa, row, seed, eval_start=False):
    """the row's handle with a fifth of the envs at t = 590..599, a fifth just inside the over-limit radius flying outwards
    (both as test_gpu_expert_rollout._make(provoke=True)) and a fifth tilted by up to 0.5 rad, yawed and turning; with
    `eval_start` every env at t = 560..599 instead of the first fifth"""
    n = row["n"]
    env = _handle(qa, row, n, seed)
    rs = np.random.RandomState(seed + 1)
    st = env.get_state()
    idx = np.arange(n)
    t0 = st["t"].copy()
    if eval_start:
        t0[:] = 560.0 + (idx * 7) % 40
    else:
        timed = idx % 5 == 0
        t0[timed] = 590.0 + (idx[timed] // 5) % 10
    far = idx % 5 == 1
    rmax = 10.0 if row["env_id"] == "docking-v2" else 3.0
    c = st["chaser"].copy()
    gap = 0.03 + 0.04 * ((idx[far] // 5) % 6)                            # port-to-port distance rmax - gap, 2 m/s outwards
    c[far, 0] = st["target"][far, 0] - 0.2 - rmax + gap
    c[far, 1:3] = st["target"][far, 1:3]
    c[far, 3:6] = np.array([-2.0, 0.0, 0.0], np.float32)
    c[far, 6:10] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    c[far, 10:13] = 0.0
    tilted = idx % 5 == 2
    q = er._quat_yaw_tilt(rs.uniform(-1.0, 1.0, n), rs.uniform(0.0, 0.5, n), rs.uniform(0.0, 2.0 * np.pi, n))
    c[tilted, 6:10] = q[tilted].astype(np.float32)
    c[tilted, 10:13] = rs.uniform(-0.5, 0.5, (n, 3))[tilted].astype(np.float32)
    env.set_state(chaser=c, t=t0)
    return env


def _loop(torch, env, ex, row, guards, steps, what, judge=True):
    """`steps` times qs_expert_action; qs_step -> dict of stacked device tensors, time-major, + the pre-step t of every step and
    the worst ratios"""
    O, A, R, D, F, Tpre = [], [], [], [], [], []
    worst = [0.0, 0.0]
    obs = None
    for k in range(steps):
        if judge:
            a, t_pre, ra, rs = _act_checked(torch, env, ex, row, guards, "%s step %d" % (what, k))
            worst = [max(worst[0], ra), max(worst[1], rs)]
            Tpre.append(t_pre.copy())
        else:
            a = ex.act()
        A.append(a.clone())
        obs, r, d, _ = env.step(a)
        O.append(obs.clone()); R.append(r.clone()); D.append(d.clone()); F.append(env.last_flags.clone())
    return dict(next_obs=torch.stack(O), actions=torch.stack(A), rewards=torch.stack(R), dones=torch.stack(D).to(torch.uint8),
                flags=torch.stack(F), t_pre=np.stack(Tpre) if Tpre else None, worst=worst)


def _fused_rollout(torch, env, ex, guards, steps, env_major):
    n = env.num_envs
    wide = (n, steps) if env_major else (steps, n)
    out = dict(obs=guards.out(wide + (12,)), actions=guards.out(wide + (4,)), rewards=guards.out((steps, n)),
               dones=guards.out((steps, n), np.uint8), flags=guards.out((steps, n), np.uint8), last_obs=guards.out((n, 12)))
    env._use_current_stream()
    torch.cuda.synchronize()
    assert env._lib.qs_set_rollout_layout(env._h, 1 if env_major else 0) == 0
    rc = env._lib.qs_expert_rollout(env._h, steps, _p(ex.state_des), ex.kp, ex.kd, _p(out["obs"]), _p(out["actions"]),
                                    _p(out["rewards"]), _p(out["dones"]), _p(out["flags"]), _p(out["last_obs"]))
    torch.cuda.synchronize()
    assert rc == 0, env._lib.qs_last_error()
    guards.check()
    if env_major:
        out["obs"], out["actions"] = out["obs"].transpose(0, 1), out["actions"].transpose(0, 1)
    return out


def _same(torch, got, ref, what):
    if not torch.equal(got, ref):
        g, r = got.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64)
        bad = g != r
        raise AssertionError("%s: %d of %d elements differ from the per-step loop, worst |diff| %.3g, first at %s" % (
            what, int(bad.sum()), bad.size, float(np.abs(g - r)[bad].max()), tuple(np.argwhere(bad)[0])))


def _same_rollout(torch, obs0, loop, fused, what):
    steps = loop["actions"].shape[0]
    _same(torch, fused["obs"][0], obs0, what + " obs[0]")
    if steps > 1:
        _same(torch, fused["obs"][1:], loop["next_obs"][:-1], what + " obs")
    _same(torch, fused["last_obs"], loop["next_obs"][-1], what + " last_obs")
    for k in ("actions", "rewards", "dones", "flags"):
        _same(torch, fused[k], loop[k], what + " " + k)


def _same_handle(torch, a, b, exa, exb, what):
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k], equal_nan=True), "%s final state: %s" % (what, k)
    for x, y, k in zip(a.get_params(), b.get_params(), ("mass", "inertia")):
        assert np.array_equal(x, y), "%s final parameters: %s" % (what, k)
    assert a.step_counter == b.step_counter, what
    assert torch.equal(exa.state_des, exb.state_des), what + " state_des"


@pytest.mark.parametrize("row", ROLLOUT_ROWS, ids=[r["id"] for r in ROLLOUT_ROWS])
def test_rollout_row(qa, torch, row):
    seed = 500 + ROLLOUT_ROWS.index(row)
    n = row["n"]
    a, b = _provoked(qa, row, seed), _provoked(qa, row, seed)
    ga, gb = ExpertGuards(torch, a.device), ExpertGuards(torch, b.device)
    exa, exb = _expert(qa, a, row, ga, seed), _expert(qa, b, row, gb, seed)
    assert torch.equal(exa.state_des, exb.state_des)
    # one warm step with zero actions: its observation is what the roll-out's row 0 has to reproduce
    zero = torch.zeros((n, 4), device=a.device)
    obs0 = a.step(zero)[0].clone()
    assert torch.equal(b.step(zero)[0], obs0)
    par0 = a.get_params()[0].copy()
    assert _variant(a)[1:4] == _variant(b)[1:4] == tuple(row["combo"])
    loop = _loop(torch, a, exa, row, ga, T, row["id"])
    fused = _fused_rollout(torch, b, exb, gb, T, row["layout"] == "env_major")
    _same_rollout(torch, obs0, loop, fused, row["id"])
    _same_handle(torch, a, b, exa, exb, row["id"])
    assert b.step_counter == 1 + T
    # conditions of the test
    dn, fl, t_pre = loop["dones"].cpu().numpy() != 0, loop["flags"].cpu().numpy(), loop["t_pre"]
    assert dn.any(axis=0).sum() * 10 >= n, dn.any(axis=0).sum()              # a tenth of the envs reset inside T
    assert (t_pre[1:] == 0).any()                                            # a first step (t == 0) at a step other than 0
    assert ((fl & 2) != 0).any() and ((fl & 4) != 0).any()                   # both the over-limit and the time-out reset ran
    if row["combo"][2] == 2:
        assert (a.get_params()[0] != par0).any()                             # per-episode parameters were redrawn and stored
    # a second call with T = 1 continues the same way
    loop1 = _loop(torch, a, exa, row, ga, 1, row["id"] + " second call")
    fused1 = _fused_rollout(torch, b, exb, gb, 1, row["layout"] == "env_major")
    _same_rollout(torch, loop["next_obs"][-1], loop1, fused1, row["id"] + " second call")
    _same_handle(torch, a, b, exa, exb, row["id"] + " second call")
    assert b.step_counter == 2 + T
    print("expert ratio %s loop actions %.3f state_des %.3f (gains %s, %s, n %d)" % (
        row["id"], max(loop["worst"][0], loop1["worst"][0]), max(loop["worst"][1], loop1["worst"][1]), row["gains"], row["layout"], n))
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------- k_expert_evaluate
def _evaluate(torch, env, ex, guards, episodes, max_steps):
    """qs_expert_evaluate into guarded buffers whose payload starts as sentinel bytes -> dict of host arrays"""
    n = env.num_envs
    sd = guards.put(ex.state_des.cpu().numpy())                              # an input: check() wants it unchanged
    out = dict(returns=guards.out((episodes, n), np.float64), lengths=guards.out((episodes, n), np.int32),
               flags=guards.out((episodes, n), np.uint8), docked_steps=guards.out((episodes, n), np.int32),
               finished=guards.out((n,), np.int32))
    env._use_current_stream()
    torch.cuda.synchronize()
    rc = env._lib.qs_expert_evaluate(env._h, episodes, max_steps, _p(sd), ex.kp, ex.kd, _p(out["returns"]), _p(out["lengths"]),
                                     _p(out["flags"]), _p(out["docked_steps"]), _p(out["finished"]))
    torch.cuda.synchronize()
    assert rc == 0, env._lib.qs_last_error()
    guards.check()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _eval_twins(qa, torch, row, seed):
    a, b = _provoked(qa, row, seed, eval_start=True), _provoked(qa, row, seed, eval_start=True)
    ga, gb = ExpertGuards(torch, a.device), ExpertGuards(torch, b.device)
    exa, exb = _expert(qa, a, row, ga, seed), _expert(qa, b, row, gb, seed)
    assert _variant(a)[1:4] == _variant(b)[1:4] == tuple(row["combo"])
    return a, b, ga, gb, exa, exb


def _untouched(torch, env, ex, before):
    st0, par0, k0, sd0 = before
    st1, par1 = env.get_state(), env.get_params()
    for k in st0:
        assert _bits(st0[k], st1[k]), "evaluation changed the state: " + k
    for x, y in zip(par0, par1):
        assert _bits(x, y), "evaluation changed the parameters"
    assert env.step_counter == k0 and torch.equal(ex.state_des, sd0)


@pytest.mark.parametrize("row", EVAL_ROWS, ids=[r["id"] for r in EVAL_ROWS])
def test_evaluate_row(qa, torch, row):
    seed = 700 + EVAL_ROWS.index(row)
    n = row["n"]
    a, b, ga, gb, exa, exb = _eval_twins(qa, torch, row, seed)
    before = (b.get_state(), b.get_params(), b.step_counter, exb.state_des.clone())
    res = _evaluate(torch, b, exb, gb, K, K * 600)
    _untouched(torch, b, exb, before)
    # the twin's per-step loop of 640 steps: the records
    loop = _loop(torch, a, exa, row, ga, 640, row["id"], judge=False)
    ga.check()
    R, D, F = (loop[k].cpu().numpy() for k in ("rewards", "dones", "flags"))
    ret, length, flags, docked, fin = _episodes(R, D != 0, F, K)
    assert (fin == K).all() and np.array_equal(res["finished"], fin)
    assert _bits(res["returns"], ret) or np.array_equal(res["returns"], ret, equal_nan=True)      # bit-equal float64 sums
    assert np.array_equal(res["lengths"], length) and np.array_equal(res["flags"], flags)
    assert np.array_equal(res["docked_steps"], docked)
    assert (length[0] <= 40).all() and (length[1] > 40).any()                 # the first episode ended through the row's reset
    a.close(); b.close()


def test_evaluate_truncation_keeps_the_sentinel_bytes(qa, torch):
    """max_steps = 100, K = 2: every env ends its first episode (t = 560..599 at the start), the slots of episodes that did
    not end keep the bytes they held before the call"""
    row = EVAL_ROWS[4]
    steps = 100
    a, b, ga, gb, exa, exb = _eval_twins(qa, torch, row, 31)
    before = (b.get_state(), b.get_params(), b.step_counter, exb.state_des.clone())
    res = _evaluate(torch, b, exb, gb, K, steps)
    _untouched(torch, b, exb, before)
    loop = _loop(torch, a, exa, row, ga, steps, row["id"], judge=False)
    R, D, F = (loop[k].cpu().numpy() for k in ("rewards", "dones", "flags"))
    ret, length, flags, docked, fin = _episodes(R, D != 0, F, K)
    assert np.array_equal(res["finished"], fin) and (fin >= 1).all() and (fin == 1).any()
    valid = np.arange(K)[:, None] < fin[None, :]
    assert np.array_equal(res["returns"][valid], ret[valid], equal_nan=True) and np.array_equal(res["lengths"][valid], length[valid])
    assert np.array_equal(res["flags"][valid], flags[valid]) and np.array_equal(res["docked_steps"][valid], docked[valid])
    for k in ("returns", "lengths", "flags", "docked_steps"):
        assert (res[k][~valid].view(np.uint8) == 0xA5).all(), k
    a.close(); b.close()
