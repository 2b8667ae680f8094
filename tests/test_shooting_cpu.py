"""-m "not gpu": qs_shooting_plan -- the C ABI from plain C99, the instantiations and resources of the planning kernel in the
built library, the Python argument checks, and the candidate keying of the float64 reference (tests/shooting_ref.py)."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

import kernel_notes
import shooting_ref
from plan_cases_cpu import ALL_COMBOS, ROOT, code_object, declarations, library_and_header, notes, run_c_caller  # noqa: F401

LLVM = kernel_notes.LLVM

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "quadsim.h"
typedef int (*plan_fn)(QsEnv *, int32_t, int32_t, int32_t, float *, double *, int32_t *, float *, double *);
int main(void) {
    plan_fn pl = &qs_shooting_plan;
    static float act[4];
    int a = pl(NULL, 20, 200, QS_SHOOT_REWARD, act, NULL, NULL, NULL, NULL);
    printf("%d %d %d %d %d %s\n", a, QS_ERR_INVALID, qs_version(), QS_SHOOT_REWARD, QS_SHOOT_POSITION,
           strstr(qs_last_error(), "null handle") ? "msg" : "nomsg");
    return 0;
}
"""

PLAN_SIG = ("int qs_shooting_plan(QsEnv *env, int32_t horizon, int32_t paths, int32_t objective, float *actions, double *best_score, "
            "int32_t *best_index, float *sequence, double *scores);")


def test_shooting_abi_symbol_and_plain_c(tmp_path):
    """include/quadsim.h declares the entry point with the agreed signature and the objective ids, the library exports it,
    QS_VERSION stays 131, and a C99 caller that takes its address compiles, links and gets QS_ERR_INVALID for a null handle"""
    from quadsim_amd import _lib
    lib, header = library_and_header()
    decl = declarations(header)
    assert PLAN_SIG in decl
    assert "enum { QS_SHOOT_REWARD = 0, QS_SHOOT_POSITION = 1 };" in decl
    assert "MPC-based_RL.py:170-210" in header
    assert hasattr(lib, "qs_shooting_plan") and "qs_shooting_plan" in _lib.EXPORTS
    assert lib.qs_shooting_plan.argtypes is not None and len(lib.qs_shooting_plan.argtypes) == 9
    assert lib.qs_version() == 131
    assert run_c_caller(tmp_path, C_PROGRAM, "plan") == ["-1", "-1", "131", "0", "1", "msg"]


def test_plan_stream_id_is_new():
    """STREAM_PLAN = 5 in quadsim_device.hpp, after the five streams the step API and the policies own"""
    text = open(os.path.join(ROOT, "quadsim_amd", "csrc", "quadsim_device.hpp")).read()
    m = re.search(r"enum : uint64_t \{([^}]*)\}", text)
    ids = dict((k.strip(), int(v)) for k, v in (item.split("=") for item in m.group(1).split(",")))
    assert ids["STREAM_PLAN"] == shooting_ref.STREAM_PLAN == 5
    assert sorted(ids.values()) == list(range(6))


# ---------------------------------------------------------------- ISA
def _plan_kernels(notes):
    """{(INTEG, PARAMS): symbol} of the planning kernel; any other kernel with `shooting` or `plan` in its name counts as
    unexpected"""
    got, other = {}, []
    for sym in notes:
        m = re.search(r"\d+k_shooting_planILi(\d)ELb([01])EEEv", sym)
        if m:
            got[(int(m.group(1)), int(m.group(2)))] = sym
        elif "shooting" in sym or "k_plan" in sym:
            other.append(sym)
    return got, other


def test_plan_kernel_instantiations_and_resources(notes):
    """four instantiations (INTEG x PARAMS; the objective is a runtime argument, there is no RMODE); no private segment, no
    spills; LDS is dynamic (sized by the horizon); 256 threads at most; five (frozen) / four (RK4) waves per SIMD"""
    got, other = _plan_kernels(notes)
    assert set(got) == ALL_COMBOS and not other, (sorted(got), other)
    for key, sym in got.items():
        n = notes[sym]
        print(key, n)
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
        assert n["group_segment_fixed_size"] == 0 and n["max_flat_workgroup_size"] == 256, (key, n)
        assert n["vgpr_count"] <= 128, (key, n)               # four waves per SIMD at least


def test_plan_kernel_isa(code_object, notes):
    """no scratch instruction, no buffer store, no matrix instruction; the target rows go through LDS
    and the kernel has its barriers"""
    got, _ = _plan_kernels(notes)
    syms = sorted(got.values())
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(syms),
                          code_object], capture_output=True, text=True, check=True).stdout
    bodies = dict(zip(*[iter(re.split(r"^(?:[0-9a-f]+ )?<(\S+)>:\n", dis, flags=re.M)[1:])] * 2))
    assert sorted(bodies) == syms
    for sym in syms:
        body = bodies[sym]
        assert "scratch_" not in body and "buffer_store" not in body and "v_mfma" not in body, sym
        assert "s_barrier" in body and "ds_write" in body and "ds_read" in body, sym
        # the only global stores are the outputs: scores, best_score, best_index, actions, sequence
        assert len(re.findall(r"\bglobal_store_\w+", body)) <= 6, sym


# ---------------------------------------------------------------- Python argument checks
def test_python_argument_checks_raise_before_any_gpu_work():
    """ValueError for a bad objective, horizon or paths; the env is never touched (it is an empty namespace here)"""
    import quadsim_amd
    env = types.SimpleNamespace()
    for kw in (dict(objective="cost"), dict(objective=0), dict(horizon=0), dict(horizon=257), dict(paths=0), dict(paths=65537)):
        with pytest.raises(ValueError):
            quadsim_amd.shooting_plan(env, **kw)
        with pytest.raises(ValueError):
            quadsim_amd.VecDockingEnv.shooting_plan(env, **kw)
        with pytest.raises(ValueError):
            quadsim_amd.ShootingMPC(env, **kw)
    mpc = quadsim_amd.ShootingMPC(env)
    assert (mpc.horizon, mpc.paths, mpc.objective) == (20, 200, "reward")     # Mpc_Controller.__init__, MPC-based_RL.py:171
    with pytest.raises(ValueError):
        mpc.run(0)


# ---------------------------------------------------------------- the keying
def test_reference_keying_prefix_and_bit_layout():
    """candidate c does not depend on `paths` (prefix property) nor step h on `horizon`; the actions differ between two values of
    k, two envs and two candidates; the block index is (k << 26) | (c << 10) | h with c < 2^16, h < 2^10, k < 2^36"""
    seed, gid, k = 12345, 7, 3
    big = shooting_ref.actions_fast(seed, gid, k, 300, 20)
    small = shooting_ref.actions_fast(seed, gid, k, 64, 5)
    assert big.shape == (300, 20, 4) and big.dtype == np.float32
    assert np.array_equal(small, big[:64, :5])
    assert np.all(big > -1.0 - 1e-7) and np.all(big <= 1.0) and abs(float(big.mean())) < 0.02
    assert not np.array_equal(big, shooting_ref.actions_fast(seed, gid, k + 1, 300, 20))
    assert not np.array_equal(big, shooting_ref.actions_fast(seed, gid + 1, k, 300, 20))
    assert not np.array_equal(big, shooting_ref.actions_fast(seed + 1, gid, k, 300, 20))
    flat = big.reshape(-1, 4)
    assert len(np.unique(flat.view(np.uint32), axis=0)) == len(flat)           # no two (c, h) share a block
    assert shooting_ref.block_index(1, 0, 0) == 1 << 26 and shooting_ref.block_index(0, 1, 0) == 1 << 10
    assert shooting_ref.block_index(0, 0, 1) == 1
    assert shooting_ref.block_index(0, 65535, 1023) == (1 << 26) - 1           # c and h fill the 26 bits below k exactly
    assert shooting_ref.block_index((1 << 36) - 1, 65535, 255) < 1 << 62       # 4 x block fits rocRAND's 64-bit offset
    # neighbouring keys do not alias: (k, c = 0, h = 0) of the next k is not (k, c, h) of any candidate of this k
    nxt = shooting_ref.actions_fast(seed, gid, k + 1, 1, 1)
    assert not (flat.view(np.uint32) == nxt.reshape(1, 4).view(np.uint32)).all(axis=1).any()


def test_vectorised_generator_is_the_oracles():
    """actions_fast (numpy integers) == actions (qso_philox4x32_10 + qso_u01) bit for bit, at small and at extreme keys"""
    for seed, gid, k, paths, horizon in ((7, 3, 5, 70, 4), (2 ** 40 + 9, 2 ** 33 + 1, 2 ** 36 - 1, 9, 3), (0, 0, 0, 3, 20)):
        a = shooting_ref.actions(seed, gid, k, paths, horizon)
        b = shooting_ref.actions_fast(seed, gid, k, paths, horizon)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    from oracle.pyoracle import Oracle
    w = shooting_ref.philox_np(99, (5 << 48) | 11, np.array([(3 << 26) | (2 << 10) | 1], np.uint64))[0]
    assert np.array_equal(w, Oracle("f64").philox(99, (5 << 48) | 11, (3 << 26) | (2 << 10) | 1))


def test_reference_scores_stop_at_done_and_break_ties_low():
    """an env one step from its time-out scores one step only, whatever the horizon; equal scores go to the lowest index"""
    from oracle.pyoracle import PAR_NOMINAL, Oracle
    rec = Oracle("f64").env_init(2)
    rec[1, 39] = 599.0
    par = np.tile(np.array(PAR_NOMINAL), (2, 1))
    acts = np.stack([shooting_ref.actions_fast(1, g, 0, 8, 6) for g in range(2)])
    long_ = shooting_ref.plan_scores(rec, par, acts)
    short = shooting_ref.plan_scores(rec, par, acts[:, :, :1])
    assert np.array_equal(long_[1], short[1]) and not np.array_equal(long_[0], short[0])
    pos = shooting_ref.plan_scores(rec, par, acts, objective=shooting_ref.POSITION)
    o = Oracle("f64").rel_obs(rec[1, 0:13], rec[1, 13:26])
    assert np.allclose(pos[1], -(o[0] ** 2 + o[1] ** 2 + o[2] ** 2), rtol=0, atol=1e-15)   # the current observation only
    assert len(np.unique(pos[0])) > 1
    assert shooting_ref.first_argmax(np.array([[1.0, 3.0, 3.0, 2.0]]))[0] == 1
