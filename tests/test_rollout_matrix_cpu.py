"""-m "not gpu": tests/rollout_matrix.py has exactly one row per instantiation of the Runner kernels (k_runner_rollout,
k_runner_split) and of the policy roll-out kernels (k_policy_rollout, k_policy_rollout_fast) as the built code object holds them;
every row is self-consistent, leans on a step-kernel row of the same (INTEG, PARAMS, RMODE) that tests/step_matrix.py ties to the
float64 oracle, and names a GPU test case that exists -- a new instantiation without a test row fails here."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import kernel_notes
import rollout_matrix as rm
import step_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return kernel_notes.kernel_notes(kernel_notes.code_object(tmp_path_factory.mktemp("isa_rollouts")))


def test_rows_are_exactly_the_instantiations(notes):
    keys = [r["key"] for r in rm.ROWS]
    assert len(keys) == len(set(keys)), "duplicate rows"
    got = kernel_notes.instantiations(notes, rm.KERNELS)
    assert {k[0] for k in got} == set(rm.KERNELS)
    assert set(keys) == got, "rows without an instantiation: %s; instantiations without a row: %s" % (
        sorted(set(keys) - got), sorted(got - set(keys)))
    assert len(rm.RUNNER_ROWS) == 80 and len(rm.POLICY_ROWS) == 8
    print("%d + %d rows matched to %d instantiations" % (len(rm.RUNNER_ROWS), len(rm.POLICY_ROWS), len(got)))


def test_rows_are_consistent():
    """each row's key is its kernel's template arguments in declaration order and what qs_debug_rollout_variant reports; a ragged
    last tile everywhere; the one-wave-per-tile flavour exactly on the k_runner_rollout rows"""
    assert len({r["id"] for r in rm.ROWS}) == len(rm.ROWS)
    for r in rm.RUNNER_ROWS:
        integ, params, rmode = r["combo"]
        fast, net = rm.PRECISIONS.index(r["precision"]), rm.NETS.index(r["net"])
        assert r["key"] == (r["kernel"], integ, rmode, params, fast, net), r["id"]
        assert r["variant"] == (rm.RUNNER_KERNELS.index(r["kernel"]),) + r["key"][1:], r["id"]
        assert (r["serial"] == 1) == (r["kernel"] == "k_runner_rollout") and r["serial"] in (0, 1), r["id"]
        assert r["noise"] in ("caller", "kernel"), r["id"]
        assert (params == 1) == (r["set_params"] or rmode == 2), r["id"]       # per-episode params imply per-env params
    for r in rm.POLICY_ROWS:
        integ, params, rmode = r["combo"]
        assert r["key"] == (r["kernel"], integ, rmode) and params == 0 and not r["set_params"], r["id"]
        assert r["variant"] == (2 + rm.POLICY_KERNELS.index(r["kernel"]), integ, rmode, -1, -1, -1), r["id"]
        assert rm.PRECISIONS[rm.POLICY_KERNELS.index(r["kernel"])] == r["precision"], r["id"]
    for r in rm.ROWS:
        assert r["n"] % 64 != 0 and r["n"] < 400, r["id"]
        assert r["integ"] == step_matrix.INTEGS[r["combo"][0]] and r["randomise"] == r["combo"][2], r["id"]
        assert r["env_id"] in ("docking-v0", "docking-v2") and r["dt"] in (0.02, 0.01), r["id"]
        assert r["T"] in (1, rm.T), r["id"]
    assert sum(r["T"] == 1 for r in rm.ROWS) == 2
    assert sum(r["n"] < 64 for r in rm.RUNNER_ROWS) >= 2 and sum(r["n"] < 64 for r in rm.POLICY_ROWS) >= 1
    assert any(r["n"] == 1 for r in rm.ROWS)
    # rows on which the GPU test requires both kinds of episode end (n >= 30, T > 1) exist in every (INTEG, RMODE) group
    for rows in (rm.RUNNER_ROWS, rm.POLICY_ROWS):
        for group in {(r["combo"][0], r["combo"][2]) for r in rows}:
            assert any(r["n"] >= 30 and r["T"] > 1 for r in rows if (r["combo"][0], r["combo"][2]) == group), group
    # every setting occurs with both values of every other one it could be tied to
    for a, b in (("env_id", "net"), ("env_id", "precision"), ("dt", "precision"), ("dt", "net"), ("noise", "net"),
                 ("noise", "precision"), ("noise", "serial"), ("env_id", "serial"), ("dt", "integ")):
        assert len({(r[a], r[b]) for r in rm.RUNNER_ROWS}) == 4, (a, b)


def test_rows_lean_on_step_rows_tied_to_float64():
    """the GPU test holds the env side bit for bit to qs_step: that step is tied to the float64 oracle by a SERIAL or SPLIT row of
    tests/step_matrix.py with the same (INTEG, PARAMS, RMODE)"""
    tied = {r["variant"][1:4] for r in step_matrix.STEP_ROWS if r["variant"][0] in (step_matrix.SERIAL, step_matrix.SPLIT)}
    for r in rm.ROWS:
        assert tuple(r["combo"]) in tied, r["id"]


def test_rows_name_existing_gpu_tests():
    files = sorted({r["test"].split("::")[0] for r in rm.ROWS})
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ids = set(out.stdout.split())
    missing = [r["test"] for r in rm.ROWS if r["test"] not in ids]
    assert not missing, missing
    ours = {i for i in ids if i.startswith("tests/test_gpu_rollout_matrix.py::test_runner_row[")
            or i.startswith("tests/test_gpu_rollout_matrix.py::test_policy_rollout_row[")}
    assert ours == {r["test"] for r in rm.ROWS}                       # one case per row, no case without a row


def test_debug_rollout_variant_rejects_bad_arguments():
    """qs_debug_rollout_variant (which roll-out kernel instantiation a call launches) checks its arguments without a GPU"""
    from quadsim_amd import _lib
    lib = _lib.load()
    lib.qs_debug_rollout_variant.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.qs_last_error.restype = C.c_char_p
    out = (C.c_int32 * 6)(*([7] * 6))
    assert lib.qs_debug_rollout_variant(None, 0, 0, 0, out) != 0
    assert b"qs_debug_rollout_variant" in lib.qs_last_error()
    assert list(out) == [7] * 6
    assert lib.qs_debug_rollout_variant(None, 1, 0, 0, None) != 0
    assert "qs_debug_rollout_variant" not in _lib.EXPORTS                # diagnostic: not part of include/quadsim.h
