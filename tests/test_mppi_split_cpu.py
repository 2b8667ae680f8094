"""-m "not gpu": qs_mppi_plan_split -- the C ABI from plain C99, the instantiations and resources of the three new kernels in
the built library beside the planner kernels that stay, and the Python `splits` argument of the MPPI entry points."""
import re
import types

import pytest

from plan_cases_cpu import (ALL_COMBOS, StubLib, code_object, combos, declarations, library_and_header, notes,  # noqa: F401
                            run_c_caller, stub_env)

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "quadsim.h"
typedef int (*split_fn)(QsEnv *, int32_t, int32_t, int32_t, int32_t, float, float, int32_t, int32_t, const float *, const float *,
                        float *, float *, double *, double *, float *, float *);
int main(void) {
    split_fn pl = &qs_mppi_plan_split;
    static float act[4], nom[80];
    int a = pl(NULL, 20, 200, 2, QS_SHOOT_REWARD, 1.0f, 0.5f, 0, 0, NULL, NULL, act, nom, NULL, NULL, NULL, NULL);
    const char *ma = strstr(qs_last_error(), "null handle") ? "msg" : "nomsg";
    printf("%d %s %d %d\n", a, ma, QS_ERR_INVALID, qs_version());
    return 0;
}
"""

SPLIT_SIG = ("int qs_mppi_plan_split(QsEnv *env, int32_t horizon, int32_t paths, int32_t iterations, int32_t objective, "
             "float lambda, float sigma, int32_t shift, int32_t splits, const float *nominal_in, const float *noise, "
             "float *actions, float *nominal_out, double *best_score, double *scores, float *trace, float *candidates);")


def test_split_abi_symbol_and_plain_c(tmp_path):
    """include/quadsim.h declares the entry point with the agreed signature and documents the one-part rule (qs_mppi_plan's
    kernel, at most 4096 paths) and the automatic rule, the library exports it, QS_VERSION stays 131, and a C99 caller that
    takes its address compiles with -Wall -Werror, links and gets QS_ERR_INVALID with a message for a null handle, without a
    device"""
    from quadsim_amd import _lib
    lib, header = library_and_header()
    assert SPLIT_SIG in declarations(header)
    doc = re.sub(r"\s+\*?\s*", " ", header[header.index("/* qs_mppi_plan with ONE ENV'S CANDIDATES"):header.index("int qs_mppi_plan_split(")])
    assert "splits = 1 launches qs_mppi_plan's own kernel" in doc and "S = 1 needs paths <= 4096" in doc
    assert "what qs_shooting_plan_splits reports), raised to 2 when paths > 4096" in doc
    assert "QS_IO_HOST handles are accepted" in doc
    assert hasattr(lib, "qs_mppi_plan_split") and "qs_mppi_plan_split" in _lib.EXPORTS
    assert len(lib.qs_mppi_plan_split.argtypes) == 17
    assert lib.qs_version() == 131
    assert run_c_caller(tmp_path, C_PROGRAM, "mppi_split") == ["-1", "msg", "-1", "131"]


# ---------------------------------------------------------------- code object
def test_part_kernel_instantiations_and_resources(notes):
    """exactly four k_pathint_part_roll (INTEG x PARAMS), one k_pathint_part_sums and one k_pathint_part_finish -- the weights and the
    sums need the candidates' keys only, no integrator and no per-env parameters, so those two have no template parameters --
    and no other kernel with `k_pathint` in its name; no private segment, no spills, at most 128 VGPRs; 256 / 256 / 64
    threads at most; all LDS is dynamic (the finish kernel has none)"""
    roll = combos(notes, r"\d+k_pathint_part_rollILi(\d)ELb([01])EEEv")
    sums = [s for s in notes if re.search(r"\d+k_pathint_part_sumsE", s)]
    finish = [s for s in notes if re.search(r"\d+k_pathint_part_finishE", s)]
    other = [s for s in notes if "k_pathint" in s and s not in roll.values() and s not in sums and s not in finish]
    assert set(roll) == ALL_COMBOS and len(sums) == 1 and len(finish) == 1 and not other, \
        (sorted(roll), sums, finish, other)
    for key, sym in list(roll.items()) + [("sums", sums[0]), ("finish", finish[0])]:
        n = notes[sym]
        print(key, n)
        assert "k_wide" not in sym and "mppi" not in sym, sym    # the patterns test_mppi_cpu.py and test_shooting_split_cpu.py own
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
        assert n["vgpr_count"] <= 128, (key, n)
        assert n["group_segment_fixed_size"] == 0, (key, n)
        assert n["max_flat_workgroup_size"] == (64 if key == "finish" else 256), (key, n)


def test_existing_planner_kernels_are_still_there(notes):
    """the four k_mppi, the four k_shooting_plan, the four k_wide_candidates and the one k_wide_finish"""
    for pattern in (r"\d+k_mppiILi(\d)ELb([01])EEEv", r"\d+k_shooting_planILi(\d)ELb([01])EEEv",
                    r"\d+k_wide_candidatesILi(\d)ELb([01])EEEv"):
        got = combos(notes, pattern)
        assert set(got) == ALL_COMBOS, (pattern, sorted(got))
        for key, sym in got.items():
            n = notes[sym]
            assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
            assert n["group_segment_fixed_size"] == 0 and n["max_flat_workgroup_size"] == 256, (key, n)
            assert n["vgpr_count"] <= 128, (key, n)
    assert len([s for s in notes if re.search(r"\d+k_wide_finishE", s)]) == 1
    assert len([s for s in notes if "k_wide" in s]) == 5


# ---------------------------------------------------------------- Python argument checks
def test_splits_argument_checks_raise_before_any_gpu_work():
    """ValueError for a `splits` that is negative, zero, above `paths`, above 1024 or no integer, and for one part with more
    paths than qs_mppi_plan's kernel holds; the env is never touched (it is an empty namespace here)"""
    import quadsim_amd
    from quadsim_amd import mpc
    env = types.SimpleNamespace()
    for kw in (dict(splits=-1), dict(splits=0), dict(splits=201), dict(paths=64, splits=65), dict(paths=4096, splits=1025),
               dict(splits=2.0), dict(splits="7"), dict(splits="automatic"), dict(splits=True), dict(splits=[2]),
               dict(paths=4097, splits=1), dict(paths=65537, splits=2), dict(paths=4097)):
        with pytest.raises(ValueError):
            quadsim_amd.mppi_plan(env, **kw)
        with pytest.raises(ValueError):
            quadsim_amd.VecDockingEnv.mppi_plan(env, **kw)
        with pytest.raises(ValueError):
            quadsim_amd.MPPI(env, **kw)
        if kw != dict(paths=4097):                            # the shim always plans through the split entry point
            with pytest.raises(ValueError):
                quadsim_amd.DockingEnv.mppi_plan(env, **kw)
    # paths = 4097 is legal with `splits`
    assert mpc.check_mppi_split_args(20, 4097, 2, "reward", 0.5, 0.4, False, 2) == (20, 4097, 2, 0, 0.5, 0.4, 0, 2)
    assert mpc.check_mppi_split_args(20, 65536, 2, "position", 0.5, 0.4, True, "auto") == (20, 65536, 2, 1, 0.5, 0.4, 1, 0)
    assert mpc.check_mppi_split_args(20, 200, 2, "reward", 0.5, 0.4, False, None) == (20, 200, 2, 0, 0.5, 0.4, 0, None)
    assert quadsim_amd.MPPI(env, paths=4097, splits="auto").splits == "auto" and quadsim_amd.MPPI(env).splits is None
    # the pinned contract of the unsplit check
    assert mpc.check_mppi_args(128, 4096, 16, "position", 1e-3, 0.0, True) == (128, 4096, 16, 1, 1e-3, 0.0, 1)
    with pytest.raises(ValueError):
        mpc.check_mppi_args(20, 4097, 2, "reward", 0.5, 0.4, False)


def test_splits_none_keeps_the_old_call_path():
    """by symbol name on a stub library: without `splits` the call is qs_mppi_plan with its old scalar arguments; an int or
    "auto" (= 0) goes to qs_mppi_plan_split with `splits` after `shift`"""
    torch = pytest.importorskip("torch")
    from quadsim_amd import mpc
    lib = StubLib((int, float))
    env = stub_env(torch, lib)
    out = mpc.mppi_plan(env, 5, 64, 2, "position", 0.5, 0.25)
    assert out["actions"].shape == (3, 4) and out["nominal"].shape == (3, 5, 4) and "scores" not in out
    mpc.MPPI(env, 5, 64, 2, lam=0.5, sigma=0.25).act()
    mpc.mppi_plan(env, 5, 64, 2, "position", 0.5, 0.25, shift=True, splits=7)
    mpc.mppi_plan(env, 5, 4097, 2, "reward", 0.5, 0.25, splits="auto", return_scores=True)
    ctl = mpc.MPPI(env, 5, 64, 2, lam=0.5, sigma=0.25, splits=2)
    ctl.act()
    ctl.act()                                                 # the second plan shifts the carried nominal
    assert lib.calls == [("qs_mppi_plan", (5, 64, 2, 1, 0.5, 0.25, 0)), ("qs_mppi_plan", (5, 64, 2, 0, 0.5, 0.25, 0)),
                         ("qs_mppi_plan_split", (5, 64, 2, 1, 0.5, 0.25, 1, 7)), ("qs_mppi_plan_split", (5, 4097, 2, 0, 0.5, 0.25, 0, 0)),
                         ("qs_mppi_plan_split", (5, 64, 2, 0, 0.5, 0.25, 0, 2)), ("qs_mppi_plan_split", (5, 64, 2, 0, 0.5, 0.25, 1, 2))]
