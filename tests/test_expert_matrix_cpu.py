"""-m "not gpu": the float64 reference of the PID expert (tests/expert_ref.py) against the oracle and fixture g11, the float32
oracle and a numpy float32 expert inside the error bound on every shared input, eight wrong experts outside it, and
tests/expert_matrix.py with exactly one row per instantiation of k_expert_action / k_expert_rollout / k_expert_evaluate as the built
code object holds them, every row naming a GPU test case that exists."""
import os
import subprocess
import sys

import numpy as np
import pytest

import expert_matrix as em
import expert_ref as er
import kernel_notes
import step_matrix
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(o, inp):
    """Oracle.expert_action env by env -> (actions [n,4], new state_des [n,13]) in the oracle's dtype"""
    n = len(inp["mass"])
    A, S = np.zeros((n, 4), o.dtype), np.zeros((n, 13), o.dtype)
    for i in range(n):
        A[i], _, S[i] = o.expert_action(inp["state_des"][i], inp["chaser"][i], inp["target"][i], inp["first"][i], inp["kp"], inp["kd"],
                                        inp["mass"][i])
    return A, S


def _args(inp):
    return inp["state_des"], inp["chaser"], inp["target"], inp["first"], inp["kp"], inp["kd"], inp["mass"]


@pytest.fixture(scope="module")
def cases():
    """{(regime, gains): (inputs, expert64 of them)}: computed once, left unchanged"""
    out = {}
    for regime, g in er.CPU_CASES:
        inp = er.inputs(regime, er.CPU_N, g)
        out[(regime, g)] = (inp, er.reference(inp))
    return out


# ---------------------------------------------------------------------------------------------------- the reference
def test_inputs_are_what_the_regimes_say(cases):
    for (regime, g), (inp, ref) in cases.items():
        tilt, yaw, rel, vel, wz = er.REGIMES[regime]
        sc, st, sd = (inp[k].astype(np.float64) for k in ("chaser", "target", "state_des"))
        eps = 1e-5
        assert np.abs(st[:, 0:3] - [er.STANDOFF, 0, 0] - sc[:, 0:3]).max() <= rel + eps
        assert np.abs(sc[:, 3:6]).max() <= vel and np.abs(sc[:, 10:13]).max() <= vel and np.abs(sd[:, 12]).max() <= wz
        w, x, y, z = sc[:, 6:10].T
        # the angle between the body and the world z axis, and the yaw of quat2euler
        assert np.arccos(np.clip(1.0 - 2.0 * (x * x + y * y), -1, 1)).max() <= tilt + eps
        phi, theta, psi, r12 = er._quat2euler(sc[:, 6:10])
        assert np.abs(r12).max() <= np.sin(tilt) + eps < 1.0                 # far from quat2euler's |r12| >= 1 branches
        assert np.abs(er._quat2euler(sd[:, 6:10])[2]).max() <= yaw + 0.05 * tilt + eps
        assert 0.1 < inp["first"].mean() < 0.2 and inp["first"].any()
        assert inp["mass"].min() >= np.float32(0.8 * 0.18) and inp["mass"].max() <= np.float32(1.2 * 0.18) and np.ptp(inp["mass"]) > 0.05
        assert (inp["kp"], inp["kd"]) == tuple(float(np.float32(v)) for v in er.GAINS[g])
        for k in ("chaser", "target", "state_des", "mass"):
            assert inp[k].dtype == np.float32
        assert np.isfinite(ref[2]).all() and (ref[2] > 0).all() and np.isfinite(ref[3]).all() and (ref[3] >= 0).all()
    assert {r for r, _ in cases} == set(er.REGIMES) and {g for _, g in cases} == set(range(len(er.GAINS)))
    hard = np.concatenate([np.abs(er._quat2euler(cases[("hard", g)][0]["state_des"][:, 6:10].astype(np.float64))[2]) for g in range(3)])
    assert hard.max() > 2.5                                                  # a desired yaw well beyond pi / 2


def test_expert64_is_the_float64_oracle(cases, oracle64):
    for key, (inp, ref) in cases.items():
        A, S = _oracle(oracle64, inp)
        np.testing.assert_allclose(ref[0], A, rtol=1e-12, atol=1e-14, err_msg=str(key))
        np.testing.assert_allclose(ref[1], S, rtol=1e-12, atol=1e-14, err_msg=str(key))
        assert np.array_equal(ref[1][:, [0, 1, 2, 12]], inp["state_des"][:, [0, 1, 2, 12]].astype(np.float64))


def test_expert64_reproduces_fixture_g11():
    """all 600 steps of the recorded episode at once: step t starts from the state_des step t - 1 left"""
    g = load_golden("g11_expert_episode")
    T = len(g["actions"])
    sd = np.concatenate([np.array([[8, -50, 5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]], float), g["state_des_after"][:-1]])
    first = np.arange(T) == 0
    act, sd_new, E, E_sd = er.expert64(sd, g["chaser"], g["target"], first, g["kp_kd"][0], g["kp_kd"][1], 0.18)
    np.testing.assert_allclose(act, g["actions"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(sd_new, g["state_des_after"], rtol=1e-12, atol=1e-12)
    # ... and what the fixture cannot see: no kd, a level desired attitude, no desired yaw rate, one first step
    assert g["kp_kd"][1] == 0 and np.abs(er._quat2euler(sd[:, 6:10])[2]).max() < 1e-12 and (sd[:, 12] == 0).all() and first.sum() == 1


# ---------------------------------------------------------------------------------------------------- the bound
def test_float32_experts_are_within_the_bound(cases, oracle32):
    """the float32 oracle (libm) and the numpy float32 expert, every element of every input"""
    worst = {}
    for (regime, g), (inp, ref) in cases.items():
        for name, got in (("oracle f32", _oracle(oracle32, inp)), ("numpy f32", er.expert32(*_args(inp)))):
            ra, rs = er.check(got[0], got[1], ref, "%s %s gains %d" % (name, regime, g))
            w = worst.setdefault((name, regime), [0.0, 0.0])
            w[0], w[1] = max(w[0], ra), max(w[1], rs)
            first = inp["first"]
            assert np.array_equal(got[1][first, 3:6], inp["state_des"][first, 3:6]) and (got[1][:, 10:12] == 0).all()
    for (name, regime), (ra, rs) in sorted(worst.items()):
        print("expert ratio %-10s %-8s actions %.3f state_des %.3f" % (name, regime, ra, rs))
    top = max(max(v) for v in worst.values())
    assert er.KAPPA_EXPERT >= 2.0 * top, (er.KAPPA_EXPERT, top)


# which inputs can show a mutant at all: kd = 0 hides the dropped kd term, the nominal regime has state_des[12] = 0
_VISIBLE = {"kd_dropped": lambda regime, g: er.GAINS[g][1] > 0, "yaw_rate_zero": lambda regime, g: regime != "nominal",
            "sin_sign": lambda regime, g: regime != "nominal"}


def test_mutants_are_out_of_bound(cases):
    """Eight wrong float32 experts, each at least 100 x KAPPA_EXPERT out on EVERY (regime, gains) input that can show it.
    sin_sign (the sin psi term of phi_des with the wrong sign) is the one that needs a desired yaw: out of bound in the mid and
    hard regimes, INSIDE the bound in the nominal one, where sin psi is zero as in fixture g11 -- which therefore could not see
    it.  sin_cos_swapped (phi_des = (a_x cos psi - a_y sin psi) / g) is NOT of that kind: at psi = 0 it gives a_x / g for
    -a_y / g, so it is out of bound in all three regimes."""
    worst = {}
    for (regime, g), (inp, ref) in cases.items():
        for m in er.MUTANTS:
            ra, rs = er.ratios(*er.expert32(*_args(inp), mutant=m), ref)
            r = max(ra, rs)
            if _VISIBLE.get(m, lambda *_: True)(regime, g):
                assert r >= 100.0 * er.KAPPA_EXPERT, (m, regime, g, r)
                w = worst.setdefault(m, [np.inf, 0.0, 0.0])
                w[0], w[1], w[2] = min(w[0], r), max(w[1], ra), max(w[2], rs)
            elif m == "sin_sign":
                assert r <= er.KAPPA_EXPERT, (m, regime, g, r)              # passes where the desired yaw is zero
                print("mutant sin_sign on the nominal regime, gains %d: ratio %.3f (inside the bound)" % (g, r))
            else:
                # the mutant changes nothing there: the correct expert's own ratios
                assert (ra, rs) == er.ratios(*er.expert32(*_args(inp)), ref), (m, regime, g)
    assert set(worst) == set(er.MUTANTS)
    for m in er.MUTANTS:
        print("mutant %-20s least visible input %.3g, worst ratio actions %.3g state_des %.3g" % ((m,) + tuple(worst[m])))
    assert min(max(w[1:]) for w in worst.values()) >= 100.0 * er.KAPPA_EXPERT


# ---------------------------------------------------------------------------------------------------- the rows
@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return kernel_notes.kernel_notes(kernel_notes.code_object(tmp_path_factory.mktemp("isa_expert_matrix")))


def test_rows_are_exactly_the_instantiations(notes):
    keys = [r["key"] for r in em.ROWS]
    assert len(keys) == len(set(keys)), "duplicate rows"
    got = kernel_notes.instantiations(notes, em.KERNELS)
    assert {k[0] for k in got} == set(em.KERNELS)
    assert set(keys) == got, "rows without an instantiation: %s; instantiations without a row: %s" % (
        sorted(set(keys) - got), sorted(got - set(keys)))
    assert (len(em.ACTION_ROWS), len(em.ROLLOUT_ROWS), len(em.EVAL_ROWS)) == (2, 14, 14) and len(got) == 30
    print("%d rows matched to %d instantiations" % (len(em.ROWS), len(got)))


def test_rows_are_consistent():
    assert len({r["id"] for r in em.ROWS}) == len(em.ROWS)
    for r in em.ROLLOUT_ROWS + em.EVAL_ROWS:
        integ, params, rmode = r["combo"]
        assert r["key"] == (r["kernel"], integ, params, rmode) and (params, rmode) in step_matrix.PAIRS, r["id"]
        assert r["integ"] == step_matrix.INTEGS[integ] and r["randomise"] == (rmode if rmode in (1, 2) else 0), r["id"]
        assert (params == 1) == (r["set_params"] or rmode == 2), r["id"]         # per-episode params imply per-env params
        assert (rmode == 3) == (r["set_init"] or r["env_id"] == "docking-v1"), r["id"]
        assert not (r["set_init"] and r["env_id"] == "docking-v1"), r["id"]
        assert r["n"] % 64 != 0 and r["gains"] in er.GAINS and r["layout"] in em.LAYOUTS, r["id"]
    assert all(r["n"] <= 300 for r in em.ROLLOUT_ROWS) and all(r["n"] <= 130 for r in em.EVAL_ROWS)
    assert any(r["n"] > 256 for r in em.ROLLOUT_ROWS) and any(r["n"] < 64 for r in em.ROLLOUT_ROWS)
    assert all(r["layout"] == em.LAYOUTS[0] for r in em.EVAL_ROWS)
    for rows in (em.ROLLOUT_ROWS, em.EVAL_ROWS):
        # stored initial states both ways, every gain pair with both integrators, RMODE 2 with and without set_params
        assert {(r["env_id"] == "docking-v1", r["set_init"]) for r in rows if r["combo"][2] == 3} == {(True, False), (False, True)}
        assert len({(r["gains"], r["integ"]) for r in rows}) == 6
        assert {r["set_params"] for r in rows if r["combo"][2] == 2} == {True, False}
        assert {r["env_id"] for r in rows} == {"docking-v0", "docking-v1", "docking-v2"}
    for a in ("integ", "gains", "env_id"):
        assert len({(r["layout"], r[a]) for r in em.ROLLOUT_ROWS}) == 2 * len({r[a] for r in em.ROLLOUT_ROWS}), a
    assert len({(r["layout"], r["combo"][2]) for r in em.ROLLOUT_ROWS}) >= 7     # every RMODE bar one in both layouts
    for r in em.ACTION_ROWS:
        assert r["key"] == ("k_expert_action", int(r["set_params"])) and r["n"] == (1, 63, 65, 257) and r["gains"] == er.GAINS, r["id"]


def test_rows_lean_on_step_rows_tied_to_float64():
    """the GPU test holds a fused kernel to the per-step loop bit for bit and judges the loop's expert at every step; the loop's
    env step is tied to the float64 oracle by a row of tests/step_matrix.py with the same (INTEG, PARAMS, RMODE)"""
    tied = {r["variant"][1:4] for r in step_matrix.STEP_ROWS if r["variant"][0] in (step_matrix.SERIAL, step_matrix.SPLIT)}
    for r in em.ROLLOUT_ROWS + em.EVAL_ROWS:
        assert tuple(r["combo"]) in tied, r["id"]


def test_rows_name_existing_gpu_tests():
    files = sorted({r["test"].split("::")[0] for r in em.ROWS})
    assert files == ["tests/test_gpu_expert_matrix.py"]
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ids = set(out.stdout.split())
    missing = [r["test"] for r in em.ROWS if r["test"] not in ids]
    assert not missing, missing
    ours = {i for i in ids if i.split("[")[0] in {t.split("[")[0] for t in (em.ACTION_TEST, em.ROLLOUT_TEST, em.EVAL_TEST)}}
    assert ours == {r["test"] for r in em.ROWS}                       # one case per row, no case without a row
