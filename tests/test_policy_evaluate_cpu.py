"""-m "not gpu": qs_policy_evaluate / _fast -- the C ABI from plain C99, the ISA of every instantiation of the two evaluation
kernels in the built library, and the host reduction behind quadsim_amd.evaluate_policy on NumPy arrays."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import kernel_notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = kernel_notes.LLVM

# the (INTEG, PARAMS, RMODE) combinations launch_integ dispatches for the step kernels
COMBOS = [(i, p, r) for i in (0, 1) for (p, r) in ((0, 0), (1, 0), (0, 1), (1, 1), (1, 2), (0, 3), (1, 3))]
LDS_LIMIT = {"k_policy_evaluate": 100160, "k_policy_evaluate_fast": 107584}   # k_policy_rollout / k_policy_rollout_fast

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "quadsim.h"
int main(void) {
    static float w[128 * 128];
    double ret[4];
    int32_t len[4], docked[4], fin[4];
    uint8_t fl[4];
    int a = qs_policy_evaluate(NULL, 1, 600, w, w, w, w, w, w, ret, len, fl, docked, fin);
    int b = qs_policy_evaluate_fast(NULL, 1, 600, w, ret, len, NULL, NULL, fin);
    printf("%d %d %d %s\n", a, b, QS_ERR_INVALID, strstr(qs_last_error(), "null handle") ? "msg" : "nomsg");
    return 0;
}
"""


def test_evaluate_abi_symbols_and_plain_c(tmp_path):
    """include/quadsim.h declares both entry points, the library exports them, and a C99 caller compiles, links and gets
    QS_ERR_INVALID for a null handle (no GPU involved)"""
    from quadsim_amd import _lib
    _lib.build_library()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "quadsim.h")).read()
    for name in ("qs_policy_evaluate", "qs_policy_evaluate_fast"):
        assert re.search(r"\bint " + name + r"\(QsEnv \*env, int32_t episodes, int64_t max_steps,", header), name
        assert hasattr(lib, name) and name in _lib.EXPORTS
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "ev.c"
    src.write_text(C_PROGRAM)
    exe = str(tmp_path / "ev")
    libdir = os.path.join(ROOT, "quadsim_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-lquadsim_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["-1", "-1", "-1", "msg"]


# ---------------------------------------------------------------- ISA
@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    return kernel_notes.code_object(tmp_path_factory.mktemp("isa_eval"))


_kernel_notes = kernel_notes.kernel_notes


def _eval_kernels(notes):
    """{(kernel, INTEG, PARAMS, RMODE): symbol} of the evaluation kernels"""
    got = {}
    for sym in notes:
        m = re.search(r"(k_policy_evaluate(?:_fast)?)ILi(\d)ELb([01])ELi(\d)E", sym)
        if m:
            got[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = sym
    return got


def test_evaluate_kernels_instantiations_and_resources(code_object):
    """exactly the launch_integ combinations, for both kernels; no private segment, no spills, LDS within the policy
    roll-out kernels' and one 256-thread block per CU (<= 512 VGPRs incl. AGPRs)"""
    notes = _kernel_notes(code_object)
    got = _eval_kernels(notes)
    want = {(k, i, p, r) for k in LDS_LIMIT for (i, p, r) in COMBOS}
    assert set(got) == want, sorted(set(got) ^ want)
    for key, sym in got.items():
        n = notes[sym]
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
        assert 0 < n["group_segment_fixed_size"] <= LDS_LIMIT[key[0]], (key, n)
        assert n["vgpr_count"] <= 512 and n["max_flat_workgroup_size"] == 256, (key, n)


def test_evaluate_kernels_isa(code_object):
    """no scratch instruction; exact-f32 MFMA in k_policy_evaluate, bf16 MFMA in k_policy_evaluate_fast; the early exit is a
    ballot (wave-uniform branch) and the step loop holds no workgroup barrier beyond the one after the weight staging"""
    got = _eval_kernels(_kernel_notes(code_object))
    syms = sorted(got.values())
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(syms),
                          code_object], capture_output=True, text=True, check=True).stdout
    bodies = dict(zip(*[iter(re.split(r"^(?:[0-9a-f]+ )?<(\S+)>:\n", dis, flags=re.M)[1:])] * 2))
    assert sorted(bodies) == syms
    for (kern, _, _, _), sym in got.items():
        body = bodies[sym]
        assert "scratch_" not in body and "buffer_store" not in body, sym
        fast = kern.endswith("_fast")
        assert ("v_mfma_f32_16x16x32_bf16" in body) == fast, sym
        if not fast:
            assert "v_mfma_f32_16x16x4_f32" in body, sym
        assert body.count("s_barrier") == 1, (sym, body.count("s_barrier"))


# ---------------------------------------------------------------- host reduction of evaluate_policy
def test_summarise_episodes_matches_numpy_in_k_env_order():
    from quadsim_amd.policy import summarise_episodes
    rng = np.random.default_rng(3)
    K, N = 3, 5
    ret = rng.normal(size=(K, N))
    length = rng.integers(1, 600, size=(K, N)).astype(np.int32)
    fin = np.full(N, K, np.int32)
    mean, std = summarise_episodes(ret, length, fin)
    assert mean == float(np.mean(ret)) and std == float(np.std(ret))
    rewards, lengths = summarise_episodes(ret, length, fin, return_episode_rewards=True)
    assert rewards == [float(ret[k, e]) for k in range(K) for e in range(N)]
    assert lengths == [int(length[k, e]) for k in range(K) for e in range(N)]
    assert all(type(x) is float for x in rewards) and all(type(x) is int for x in lengths)
    fin[2] = K - 1
    with pytest.raises(RuntimeError):
        summarise_episodes(ret, length, fin)


def test_evaluate_policy_argument_checks_need_no_gpu():
    """n_eval_episodes must be a positive multiple of num_envs (SB2 runs one env; here every env runs the same number);
    stochastic evaluation is not offered -- both refused before anything touches a device"""
    from quadsim_amd import evaluate_policy
    from quadsim_amd.policy import episodes_for
    env = types.SimpleNamespace(num_envs=4)
    for bad in (6, 0, -4, 2):
        with pytest.raises(ValueError):
            evaluate_policy(object(), env, bad)
    with pytest.raises(NotImplementedError):
        evaluate_policy(object(), env, 8, deterministic=False)
    assert episodes_for(8, 4) == 2 and episodes_for(4, 4) == 1 and episodes_for(65536, 65536) == 1
