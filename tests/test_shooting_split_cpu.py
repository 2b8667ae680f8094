"""-m "not gpu": qs_shooting_plan_split / qs_shooting_plan_splits -- the C ABI from plain C99, the instantiations and resources
of the two new kernels in the built library beside the eight planner kernels that stay, and the Python `splits` argument."""
import re
import types

import pytest

from plan_cases_cpu import (ALL_COMBOS, StubLib, code_object, combos, declarations, library_and_header, notes,  # noqa: F401
                            run_c_caller, stub_env)

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "quadsim.h"
typedef int (*split_fn)(QsEnv *, int32_t, int32_t, int32_t, int32_t, float *, double *, int32_t *, float *, double *);
typedef int (*splits_fn)(QsEnv *, int32_t, int32_t *);
int main(void) {
    split_fn pl = &qs_shooting_plan_split;
    splits_fn ps = &qs_shooting_plan_splits;
    static float act[4];
    int32_t s = -7;
    int a = pl(NULL, 20, 200, QS_SHOOT_REWARD, 0, act, NULL, NULL, NULL, NULL);
    const char *ma = strstr(qs_last_error(), "null handle") ? "msg" : "nomsg";
    int b = ps(NULL, 200, &s);
    const char *mb = strstr(qs_last_error(), "null handle") ? "msg" : "nomsg";
    printf("%d %s %d %s %d %d %d\n", a, ma, b, mb, (int)s, QS_ERR_INVALID, qs_version());
    return 0;
}
"""

SPLIT_SIG = ("int qs_shooting_plan_split(QsEnv *env, int32_t horizon, int32_t paths, int32_t objective, int32_t splits, "
             "float *actions, double *best_score, int32_t *best_index, float *sequence, double *scores);")
SPLITS_SIG = "int qs_shooting_plan_splits(QsEnv *env, int32_t paths, int32_t *splits);"


def test_split_abi_symbols_and_plain_c(tmp_path):
    """include/quadsim.h declares both entry points with the agreed signatures and documents the automatic rule, the library
    exports them, QS_VERSION stays 131, and a C99 caller that takes their addresses compiles with -Wall -Werror, links and
    gets QS_ERR_INVALID with a message for a null handle from both, without a device; `splits` is left alone on failure"""
    from quadsim_amd import _lib
    lib, header = library_and_header()
    decl = declarations(header)
    assert SPLIT_SIG in decl and SPLITS_SIG in decl
    assert "multiProcessorCount" in header and "QS_IO_HOST handles are accepted" in header
    for name, nargs in (("qs_shooting_plan_split", 10), ("qs_shooting_plan_splits", 3)):
        assert hasattr(lib, name) and name in _lib.EXPORTS
        assert len(getattr(lib, name).argtypes) == nargs
    assert lib.qs_version() == 131
    assert run_c_caller(tmp_path, C_PROGRAM, "split") == ["-1", "msg", "-1", "msg", "-7", "-1", "131"]


# ---------------------------------------------------------------- code object
def test_wide_kernel_instantiations_and_resources(notes):
    """exactly four k_wide_candidates (INTEG x PARAMS) and one k_wide_finish (no template parameters), and no other kernel
    with `k_wide` in its name; no private segment, no spills, at most 128 VGPRs; 256 / 64 threads at most; the candidates
    kernel's LDS is dynamic (sized by the horizon) and the finish kernel has none"""
    cand = combos(notes, r"\d+k_wide_candidatesILi(\d)ELb([01])EEEv")
    finish = [s for s in notes if re.search(r"\d+k_wide_finishE", s)]
    other = [s for s in notes if "k_wide" in s and s not in cand.values() and s not in finish]
    assert set(cand) == ALL_COMBOS and len(finish) == 1 and not other, (sorted(cand), finish, other)
    for key, sym in list(cand.items()) + [("finish", finish[0])]:
        n = notes[sym]
        print(key, n)
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
        assert n["vgpr_count"] <= 128, (key, n)
        assert n["group_segment_fixed_size"] == 0, (key, n)
        assert n["max_flat_workgroup_size"] == (64 if key == "finish" else 256), (key, n)


def test_existing_planner_kernels_are_still_there(notes):
    """the four k_shooting_plan and the four k_mppi, with the resources their own tests assert"""
    for pattern in (r"\d+k_shooting_planILi(\d)ELb([01])EEEv", r"\d+k_mppiILi(\d)ELb([01])EEEv"):
        got = combos(notes, pattern)
        assert set(got) == ALL_COMBOS, (pattern, sorted(got))
        for key, sym in got.items():
            n = notes[sym]
            assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
            assert n["group_segment_fixed_size"] == 0 and n["max_flat_workgroup_size"] == 256, (key, n)
            assert n["vgpr_count"] <= 128, (key, n)


# ---------------------------------------------------------------- Python argument checks
def test_splits_argument_checks_raise_before_any_gpu_work():
    """ValueError for a `splits` that is negative, zero, above `paths`, above 1024 or no integer; the env is never touched (it
    is an empty namespace here).  The legal spellings pass the check."""
    import quadsim_amd
    from quadsim_amd import mpc
    env = types.SimpleNamespace()
    for kw in (dict(splits=-1), dict(splits=0), dict(splits=201), dict(paths=64, splits=65), dict(paths=4096, splits=1025),
               dict(splits=2.0), dict(splits="7"), dict(splits="automatic"), dict(splits=True), dict(splits=[2])):
        with pytest.raises(ValueError):
            quadsim_amd.shooting_plan(env, **kw)
        with pytest.raises(ValueError):
            quadsim_amd.VecDockingEnv.shooting_plan(env, **kw)
        with pytest.raises(ValueError):
            quadsim_amd.ShootingMPC(env, **kw)
        with pytest.raises(ValueError):
            quadsim_amd.DockingEnv.shooting_plan(env, **kw)
    assert mpc.check_plan_args(20, 200, "reward") == (20, 200, 0, None)
    assert mpc.check_plan_args(20, 200, "position", "auto") == (20, 200, 1, 0)
    assert mpc.check_plan_args(20, 200, "reward", 200) == (20, 200, 0, 200)
    assert mpc.check_plan_args(3, 65536, "reward", 1024) == (3, 65536, 0, 1024)
    import numpy as np
    assert mpc.check_plan_args(3, 64, "reward", np.int64(7))[3] == 7
    assert quadsim_amd.ShootingMPC(env, splits=7).splits == 7 and quadsim_amd.ShootingMPC(env).splits is None
    with pytest.raises(ValueError):
        quadsim_amd.plan_splits(env, 0)
    with pytest.raises(ValueError):
        quadsim_amd.plan_splits(env, 65537)


def test_splits_none_keeps_the_old_call_path():
    """by symbol name on a stub library: without `splits` the call is qs_shooting_plan with its nine arguments; an int or
    "auto" (= 0) goes to qs_shooting_plan_split with `splits` after the objective"""
    torch = pytest.importorskip("torch")
    from quadsim_amd import mpc
    lib = StubLib()
    env = stub_env(torch, lib)
    out = mpc.shooting_plan(env, 5, 64, "position")
    assert out["actions"].shape == (3, 4) and "scores" not in out
    mpc.ShootingMPC(env, 5, 64).act()
    mpc.shooting_plan(env, 5, 64, "position", splits=7)
    mpc.shooting_plan(env, 5, 64, splits="auto", return_scores=True)
    mpc.ShootingMPC(env, 5, 64, splits=2).act()
    assert lib.calls == [("qs_shooting_plan", (5, 64, 1)), ("qs_shooting_plan", (5, 64, 0)),
                         ("qs_shooting_plan_split", (5, 64, 1, 7)), ("qs_shooting_plan_split", (5, 64, 0, 0)),
                         ("qs_shooting_plan_split", (5, 64, 0, 2))]
