"""-m "not gpu": everything of MPPI over the learned dynamics net that needs no device.  include/quadsim_dyn_mppi.h is plain C99
and every symbol it declares is exported by libquadsim_dynmppi.so; every refusal the header promises happens before anything
is launched; tests/dynmppi_matrix.py has exactly one row per kernel and instantiation of the new library's code object, no
kernel uses scratch or spills and each fits the compute unit's LDS; the other two libraries are built without the new
fragment; tests/dynmppi_ref.py composes the two float64 references consistently."""
import os
import re

import numpy as np
import pytest

import dynmppi_matrix
import dynmppi_ref
import dynplan_ref as dr
import side_cases
import mppi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, dynplan
    _lib.build_library()
    return dynplan.load_mppi()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("dynmppi", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    from quadsim_amd import dynplan
    side_cases.check_exports("dynmppi", lib, ["qsdm_last_error", "qsdm_mppi_plan", "qsdm_version", "qsdm_workspace_bytes"])
    assert sorted(dynplan.MPPI_EXPORTS) == side_cases.declared("dynmppi")
    assert dynplan.EXPORTS == ["qsd_version", "qsd_last_error", "qsd_net_image_bytes", "qsd_net_pack", "qsd_plan_workspace_bytes",
                               "qsd_shooting_plan"]
    assert not set(dynplan.EXPORTS) & set(dynplan.MPPI_EXPORTS)


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_dyn_mppi.h"

static float buf[64 + 4];
static float *x;
static double s[4];

static int refused(int rc, const char *word)
{
    if (rc == QSDM_OK || strstr(qsdm_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qsdm_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int call(const void *image, int h1, int h2, int64_t n, const float *obs, uint64_t k, int horizon, int paths, int iterations,
                float lambda, float sigma, int shift, void *workspace, float *actions, float *nominal_out)
{
    return qsdm_mppi_plan(image, h1, h2, n, obs, 1, 2, k, horizon, paths, iterations, lambda, sigma, shift, NULL, NULL, workspace, actions,
                          nominal_out, s, NULL, NULL, NULL, NULL, NULL);
}

int main(void)
{
    size_t bytes = 0;
    int ok = 1;
    void *fns[] = {(void *)qsdm_version, (void *)qsdm_last_error, (void *)qsdm_workspace_bytes, (void *)qsdm_mppi_plan};
    x = (float *)(((uintptr_t)buf + 15) & ~(uintptr_t)15);
    if (qsdm_version() != QSDM_VERSION) return 2;
    if (qsdm_workspace_bytes(3, 20, 200, &bytes) != QSDM_OK || bytes != 3 * 20 * 4 * sizeof(float) + 3 * 200 * sizeof(double)) return 3;
    if (qsdm_workspace_bytes(1, 1024, 65536, &bytes) != QSDM_OK || bytes != 1024 * 16 + 65536 * 8) return 4;
    ok &= refused(qsdm_workspace_bytes(0, 20, 200, &bytes), "n must");
    ok &= refused(qsdm_workspace_bytes(1, 0, 200, &bytes), "horizon");
    ok &= refused(qsdm_workspace_bytes(1, 20, 65537, &bytes), "paths");
    ok &= refused(qsdm_workspace_bytes(1, 20, 200, NULL), "bytes");
    ok &= refused(qsdm_workspace_bytes((int64_t)1 << 31, 20, 16, &bytes), "2^31");
    ok &= refused(call(x, 200, 100, 1, x, 0, 0, 200, 2, 1.0f, 0.5f, 0, x, x, x), "horizon");
    ok &= refused(call(x, 200, 100, 1, x, 0, 1025, 200, 2, 1.0f, 0.5f, 0, x, x, x), "horizon");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 0, 2, 1.0f, 0.5f, 0, x, x, x), "paths");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 65537, 2, 1.0f, 0.5f, 0, x, x, x), "paths");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 0, 1.0f, 0.5f, 0, x, x, x), "iterations");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 17, 1.0f, 0.5f, 0, x, x, x), "iterations");
    ok &= refused(call(x, 200, 100, 1, x, (uint64_t)1 << 33, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "k must");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 0.0f, 0.5f, 0, x, x, x), "lambda");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, INFINITY, 0.5f, 0, x, x, x), "lambda");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, NAN, 0.5f, 0, x, x, x), "lambda");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, -1.0f, 0.5f, 0, x, x, x), "lambda");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, -0.5f, 0, x, x, x), "sigma");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, INFINITY, 0, x, x, x), "sigma");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, NAN, 0, x, x, x), "sigma");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 2, x, x, x), "shift");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, -1, x, x, x), "shift");
    ok &= refused(call(x, 209, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "hidden widths");
    ok &= refused(call(x, 200, 113, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "hidden widths");
    ok &= refused(call(x, 129, 128, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "hidden widths");
    ok &= refused(call(x, 0, 10, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "hidden widths");
    ok &= refused(call(x, 200, 100, 0, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "n must");
    ok &= refused(call(NULL, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "NULL");
    ok &= refused(call(x, 200, 100, 1, NULL, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, x), "NULL");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, NULL, x, x), "NULL");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, NULL, x), "NULL");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x, NULL), "NULL");
    ok &= refused(call(x, 200, 100, 1, x, 0, 20, 200, 2, 1.0f, 0.5f, 0, x, x + 1, x), "aligned");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before the device is queried or anything is launched,
    here without a device and on a machine with one alike"""
    side_cases.run_c_caller("dynmppi", C_CALLER, tmp_path)


def test_python_checks_refuse_before_the_library_is_touched(monkeypatch):
    import torch
    from quadsim_amd import dynplan

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(dynplan, "load_mppi", touched)
    monkeypatch.setattr(dynplan, "load", touched)
    good = dict(horizon=20, paths=200, iterations=2, lam=0.5, sigma=0.25, shift=False, k=0, n=1)
    assert dynplan.check_mppi_plan_args(**good) == (20, 200, 2, 0.5, 0.25, 0, 0, 1)
    assert dynplan.check_mppi_plan_args(1024, 65536, 16, 1e-3, 0.0, True, (1 << 33) - 1, 1) == (1024, 65536, 16, 1e-3, 0.0, 1, (1 << 33) - 1, 1)
    for kw in (dict(horizon=0), dict(horizon=1025), dict(paths=0), dict(paths=65537), dict(iterations=0), dict(iterations=17),
               dict(k=1 << 33), dict(k=-1), dict(lam=0.0), dict(lam=-1.0), dict(lam=float("inf")), dict(lam=float("nan")),
               dict(sigma=-0.1), dict(sigma=float("inf")), dict(sigma=float("nan")), dict(shift=2), dict(shift=-1), dict(n=0),
               dict(n=1 << 31, paths=16)):
        with pytest.raises(ValueError):
            dynplan.check_mppi_plan_args(**dict(good, **kw))
    net = dr.to_net(dr.weight_set("he_20_10"), "cpu")
    obs = torch.zeros(2, 12)
    for kw in (dict(horizon=0), dict(paths=65537), dict(iterations=17), dict(k=1 << 33), dict(lam=0.0), dict(sigma=-1.0), dict(shift=2),
               dict(gid0=-1), dict(seed=1 << 64), dict(nominal=torch.zeros(2, 19, 4)), dict(nominal=torch.zeros(2, 20, 4, dtype=torch.float64)),
               dict(noise=torch.zeros(2, 200, 20, 3)), dict(noise=np.zeros((2, 200, 20, 4), np.float32))):
        with pytest.raises(ValueError):
            dynplan.learned_mppi_plan(net, obs, **kw)
    for wrong in (torch.zeros(2, 13), torch.zeros(2, 12, dtype=torch.float64), torch.zeros(12), torch.zeros(0, 12)):
        with pytest.raises(ValueError):
            dynplan.learned_mppi_plan(net, wrong)
    with pytest.raises(ValueError):
        dynplan.learned_mppi_plan(object(), obs)
    for kw in (dict(iterations=0), dict(lam=0.0), dict(sigma=-1.0), dict(paths=0)):
        with pytest.raises(ValueError):
            dynplan.LearnedMPPI(object(), net, **kw)
    with pytest.raises(ValueError):
        dynplan.LearnedMPPI(object(), object())
    import quadsim_amd as qa
    assert qa.learned_mppi_plan is dynplan.learned_mppi_plan and qa.LearnedMPPI is dynplan.LearnedMPPI
    assert qa.check_mppi_plan_args is dynplan.check_mppi_plan_args
    assert "untuned" in dynplan.learned_mppi_plan.__doc__


# ---------------------------------------------------------------------------------------------------- the census
def _instantiations(notes):
    got = set()
    for sym in notes:
        m = re.match(r"^_ZN3qsd(\d+)(k_\w+?)(?:I((?:Li\d+E)+)E)?(?:E|Ev)", sym)
        assert m and int(m.group(1)) == len(m.group(2)), "a kernel outside namespace qsd: %s" % sym
        got.add((m.group(2),) + tuple(int(a) for a in re.findall(r"Li(\d+)E", m.group(3) or "")))
    return got


@pytest.fixture(scope="module")
def census(notes):
    return side_cases.check_census(notes, dynmppi_matrix, _instantiations, "dynmppi")


def test_rows_are_exactly_the_kernels_of_the_code_object(census):
    import dynplan_matrix
    keys = [r["key"] for r in dynmppi_matrix.ROWS]
    from quadsim_amd import dynplan
    assert {(16 * k[1], 16 * k[2]) for k in keys if k[0] == "k_dynm_roll"} == set(dynplan.COMPILED_WIDTHS)
    assert {r["widths"] for r in dynmppi_matrix.ROWS if r["widths"]} == set(dynplan.COMPILED_WIDTHS)
    # the inherited kernels are the non-template kernels of the shooting planner's census, each with that census's own test
    theirs = {r["key"]: r["test"] for r in dynplan_matrix.ROWS if len(r["key"]) == 1}
    inherited = {r["key"]: r["test"] for r in dynmppi_matrix.ROWS if r["inherited"]}
    assert inherited == theirs and len(inherited) == 2
    assert all(r["note"] == "inherited, pinned by tests/dynplan_matrix.py" for r in dynmppi_matrix.ROWS if r["inherited"])
    assert not any(r["kernel"].startswith("k_dynm_") for r in dynmppi_matrix.ROWS if r["inherited"])


def test_rows_with_widths_name_a_net_of_exactly_those_widths():
    """a row's `widths` are the hidden widths of the net its test id names (the widest the instantiation takes)"""
    for r in dynmppi_matrix.ROWS:
        if r["widths"]:
            W = dr.weight_set(re.search(r"\[(\w+)\]$", r["test"]).group(1))
            assert (W["w1"].shape[0], W["w2"].shape[0]) == r["widths"] == (16 * r["key"][1], 16 * r["key"][2]), r


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(dynmppi_matrix)


def test_no_kernel_uses_scratch_or_spills_and_each_fits_lds(census):
    assert max(fl["group_segment_fixed_size"] for k, fl in census.items() if k[0] == "k_dynm_roll") == 120656        # the 208 x 112 image, as quadsim_dyn.h says


def test_the_other_libraries_are_built_without_the_new_fragment():
    """dynmppi_kernels.hpp is a dependency of the third library alone, whose translation unit is the only file that includes
    it, and no other library lists it"""
    from quadsim_amd import _lib
    side_cases.check_entry("dynmppi", ["dynmppi_kernels.hpp", "dynplan_host.hpp", "dynplan_image.hpp", "dynplan_kernels.hpp", "quadsim_device.hpp",
                                       "quadsim_dyn_mppi.h", "side_host.hpp"], "dynmppi.hip")
    csrc = os.path.join(ROOT, "quadsim_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp")) and f != "dynmppi_kernels.hpp"
                   and "dynmppi_kernels.hpp\"" in open(os.path.join(csrc, f)).read())
    assert users == ["dynmppi.hip"]
    assert _lib.build_library() == _lib.LIB_PATH and os.path.exists(_lib.SIDE["dyn"]["path"]) and os.path.exists(_lib.SIDE["dynmppi"]["path"])
    side_cases.check_no_foreign_kernels("dynmppi")
    assert b"k_dynm_roll" in open(_lib.SIDE["dynmppi"]["path"], "rb").read()


# ---------------------------------------------------------------------------------------------------- the reference glue
def _case(n=2, paths=40, horizon=6, iterations=2, seed=3):
    rng = np.random.default_rng(seed)
    W = dr.weight_set("he_20_10")
    obs = dr.sample_obs(n, seed=47)
    noise = rng.standard_normal((iterations, paths, horizon, 4)).astype(np.float32)
    nominal = rng.uniform(-1.2, 1.2, (n, horizon, 4)).astype(np.float32)
    return W, obs, noise, nominal


def test_reference_composes_the_two_references():
    W, obs, noise, nominal = _case()
    out = dynmppi_ref.plan64(W, obs, 0.4, noise, 0.5, nominal, shift=1)
    U0 = nominal[:, [1, 2, 3, 4, 5, 5]]
    assert np.array_equal(out["trace"][:, 0], U0) and out["trace"].dtype == np.float32
    cands = mppi_ref.candidates32(U0, 0.4, noise[0])
    S = dr.cost64(dr.rollout64(W, obs, cands))
    assert np.array_equal(out["scores"][:, 0], S)
    U1 = mppi_ref.update64(S, cands, 0.5, U0).astype(np.float32)
    assert np.array_equal(out["trace"][:, 1], U1)
    assert np.array_equal(out["candidates"], mppi_ref.candidates32(U1, 0.4, noise[1]))
    assert np.array_equal(out["nominal"], out["trace"][:, -1]) and np.array_equal(out["actions"], out["nominal"][:, 0])
    assert np.array_equal(out["best_score"], out["scores"][:, -1].max(axis=1))
    # the first iteration of two is the plan with one
    one = dynmppi_ref.plan64(W, obs, 0.4, noise[:1], 0.5, nominal, shift=1)
    assert np.array_equal(one["trace"], out["trace"][:, :2]) and np.array_equal(one["scores"], out["scores"][:, :1])
    assert np.array_equal(dynmppi_ref.shifted(None, 6, 1, 2), np.zeros((2, 6, 4), np.float32))


def test_lam_to_zero_is_the_arg_max_of_choose64():
    """with lam -> 0 every weight but the best candidate's underflows to 0: the update is choose64's winner"""
    W, obs, noise, nominal = _case(iterations=1)
    new, S, cands = dynmppi_ref.iteration64(W, obs, nominal, 0.4, noise[0], 1e-12)
    first, j, costs = dr.choose64(W, obs, cands)
    assert np.array_equal(costs, S)
    assert np.array_equal(new, cands[np.arange(len(j)), j].astype(np.float64))
    assert np.array_equal(new[:, 0], first.astype(np.float64))


def test_one_path_one_iteration_is_the_clamped_nominal():
    W, obs, noise, nominal = _case(paths=1, iterations=1)
    assert np.abs(nominal).max() > 1.0
    out = dynmppi_ref.plan64(W, obs, 0.4, noise, 0.5, nominal)
    assert np.array_equal(out["nominal"], np.clip(nominal, -1, 1)) and np.array_equal(out["candidates"][:, 0], out["nominal"])
    # a NaN observation: every score NaN, the nominal stays as it is, -inf
    bad = obs.copy()
    bad[0, 1] = np.nan
    out = dynmppi_ref.plan64(W, bad, 0.4, noise, 0.5, nominal)
    assert np.array_equal(out["nominal"][0], nominal[0]) and out["best_score"][0] == -np.inf and np.isfinite(out["best_score"][1])
