"""-m "not gpu": tests/step_matrix.py has exactly one row per instantiation of the step kernels (k_env, k_env_split,
k_env_resident, k_hover) and of the evaluation kernels that share their step, as the built code object holds them, and every
row names a GPU test case that exists -- a new instantiation without a test row fails here."""
import os
import subprocess
import sys

import pytest

import kernel_notes
import step_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_env_resident", "k_env_split", "k_env", "k_hover", "k_policy_evaluate_fast", "k_policy_evaluate")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return kernel_notes.kernel_notes(kernel_notes.code_object(tmp_path_factory.mktemp("isa_steps")))


def test_rows_are_exactly_the_instantiations(notes):
    keys = [r["key"] for r in step_matrix.ROWS]
    assert len(keys) == len(set(keys)), "duplicate rows"
    got = kernel_notes.instantiations(notes, KERNELS)
    assert {k[0] for k in got} == set(KERNELS)
    assert set(keys) == got, "rows without an instantiation: %s; instantiations without a row: %s" % (
        sorted(set(keys) - got), sorted(got - set(keys)))


def test_rows_are_consistent():
    """each step row's variant is its kernel's template arguments; ids are unique; every row is reached in production"""
    assert len({r["id"] for r in step_matrix.ROWS}) == len(step_matrix.ROWS)
    for r in step_matrix.STEP_ROWS:
        fam, integ, params, rmode, prep = r["variant"]
        assert step_matrix.FAMILY_KERNEL[fam] == r["kernel"] == r["key"][0], r["id"]
        args = {"k_env": (integ, params, rmode), "k_hover": (integ, params)}.get(r["kernel"], (integ, params, rmode, prep))
        assert r["key"][1:] == args, r["id"]
        assert r["n"] % 64 != 0, r["id"]                      # a ragged last tile on every row
        assert r["production"] and r["force_prep"] is None, r["id"]
        assert (r["queues"] > 0) == (fam == step_matrix.RESIDENT), r["id"]
    for r in step_matrix.EVAL_ROWS:
        assert r["key"][1:] == r["combo"] and step_matrix.EVAL_PRECISION[r["kernel"]] == r["precision"], r["id"]


def test_rows_name_existing_gpu_tests():
    files = sorted({r["test"].split("::")[0] for r in step_matrix.ROWS})
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ids = set(out.stdout.split())
    missing = [r["test"] for r in step_matrix.ROWS if r["test"] not in ids]
    assert not missing, missing
