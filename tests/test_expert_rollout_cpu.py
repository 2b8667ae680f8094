"""-m "not gpu": qs_expert_rollout / qs_expert_evaluate -- the C ABI from plain C99, the instantiations and resources of the two
kernels in the built library, the dataset bookkeeping behind quadsim_amd.record_expert_dataset on CPU tensors, and its
argument checks."""
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
KERNELS = ("k_expert_rollout", "k_expert_evaluate")

C_PROGRAM = r"""
#include <stdio.h>
#include <string.h>
#include "quadsim.h"
typedef int (*rollout_fn)(QsEnv *, int64_t, float *, float, float, float *, float *, float *, uint8_t *, uint8_t *, float *);
typedef int (*evaluate_fn)(QsEnv *, int32_t, int64_t, const float *, float, float, double *, int32_t *, uint8_t *, int32_t *,
                           int32_t *);
int main(void) {
    rollout_fn ro = &qs_expert_rollout;
    evaluate_fn ev = &qs_expert_evaluate;
    static float sd[13], obs[12], act[4], rew[1];
    uint8_t done[1];
    double ret[1];
    int32_t len[1], fin[1];
    int a = ro(NULL, 1, sd, 0.35f, 0.0f, obs, act, rew, done, NULL, NULL);
    int b = ev(NULL, 1, 600, sd, 0.35f, 0.0f, ret, len, NULL, NULL, fin);
    printf("%d %d %d %d %s\n", a, b, QS_ERR_INVALID, qs_version(), strstr(qs_last_error(), "null handle") ? "msg" : "nomsg");
    return 0;
}
"""

ROLLOUT_SIG = ("int qs_expert_rollout(QsEnv *env, int64_t T, float *state_des, float kp, float kd, float *obs, float *actions, "
               "float *reward, uint8_t *done, uint8_t *flags, float *last_obs);")
EVALUATE_SIG = ("int qs_expert_evaluate(QsEnv *env, int32_t episodes, int64_t max_steps, const float *state_des, float kp, float kd, "
                "double *ep_return, int32_t *ep_length, uint8_t *ep_flags, int32_t *ep_docked, int32_t *finished);")


def _declarations(header):
    """the header without comments, white space normalised"""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    return re.sub(r" ([,)])", r"\1", text)


def test_expert_abi_symbols_and_plain_c(tmp_path):
    """include/quadsim.h declares both entry points with the agreed signatures, the library exports them, QS_VERSION stays
    131, and a C99 caller that takes their addresses compiles, links and gets QS_ERR_INVALID for a null handle"""
    from quadsim_amd import _lib
    _lib.build_library()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "quadsim.h")).read()
    decl = _declarations(header)
    assert ROLLOUT_SIG in decl and EVALUATE_SIG in decl
    for name in ("qs_expert_rollout", "qs_expert_evaluate"):
        assert hasattr(lib, name) and name in _lib.EXPORTS
    assert lib.qs_version() == 131
    assert shutil.which("gcc") is not None
    src = tmp_path / "ex.c"
    src.write_text(C_PROGRAM)
    exe = str(tmp_path / "ex")
    libdir = os.path.join(ROOT, "quadsim_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-lquadsim_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib",
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["-1", "-1", "-1", "131", "msg"]


# ---------------------------------------------------------------- ISA
@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    return kernel_notes.code_object(tmp_path_factory.mktemp("isa_expert"))


def _expert_kernels(notes):
    """{(kernel, INTEG, PARAMS, RMODE): symbol} of the two fused expert kernels"""
    got = {}
    for sym in notes:
        m = re.search(r"\d+(k_expert_rollout|k_expert_evaluate)ILi(\d)ELb([01])ELi(\d)E", sym)
        if m:
            got[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = sym
    return got


def test_expert_kernels_instantiations_and_resources(code_object):
    """14 instantiations of each kernel = the launch_integ combinations; no private segment, no spills, no LDS, 256 threads"""
    notes = kernel_notes.kernel_notes(code_object)
    got = _expert_kernels(notes)
    want = {(k, i, p, r) for k in KERNELS for (i, p, r) in COMBOS}
    assert set(got) == want and len(got) == 28, sorted(set(got) ^ want)
    for key, sym in got.items():
        n = notes[sym]
        assert n["private_segment_fixed_size"] == 0 and n["vgpr_spill_count"] == 0, (key, n)
        assert n["group_segment_fixed_size"] == 0 and n["max_flat_workgroup_size"] == 256, (key, n)
        assert n["vgpr_count"] <= 256, (key, n)               # two waves per SIMD at least: no AGPR spill area either


def test_expert_kernels_isa(code_object):
    """no scratch instruction and no workgroup barrier in either kernel; the evaluation's early exit is a wave-uniform branch"""
    got = _expert_kernels(kernel_notes.kernel_notes(code_object))
    syms = sorted(got.values())
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--disassemble-symbols=" + ",".join(syms),
                          code_object], capture_output=True, text=True, check=True).stdout
    bodies = dict(zip(*[iter(re.split(r"^(?:[0-9a-f]+ )?<(\S+)>:\n", dis, flags=re.M)[1:])] * 2))
    assert sorted(bodies) == syms
    for sym in syms:
        body = bodies[sym]
        assert "scratch_" not in body and "buffer_store" not in body and "s_barrier" not in body, sym
        assert "v_mfma" not in body, sym


# ---------------------------------------------------------------- the dataset bookkeeping on CPU tensors
def _case():
    """4 envs x 8 steps.  env 0: episodes end on the first step, a middle step and the last step; env 1: two middle ends; env 2:
    one episode ending on the last step; env 3: one end in the middle only"""
    import torch
    d = np.zeros((4, 8), bool)
    d[0, [0, 4, 7]] = True
    d[1, [2, 5]] = True
    d[2, 7] = True
    d[3, 3] = True
    r = (np.arange(32, dtype=np.float32).reshape(4, 8) + 1.0) * np.float32(0.1)
    return d, r, torch.as_tensor(d), torch.as_tensor(r)


def _sum64(r, env, lo, hi):
    return float(np.sum(r[env, lo:hi].astype(np.float64)))


def test_assemble_all_rows():
    from quadsim_amd import assemble_expert_dataset
    d, r, td, tr = _case()
    starts, rets, mask = assemble_expert_dataset(td, tr)
    assert mask is None and starts.dtype.is_floating_point is False and rets.dtype.itemsize == 8
    want = np.zeros((4, 8), bool)
    want[:, 0] = True
    want[0, [1, 5]] = True
    want[1, [3, 6]] = True
    want[3, 4] = True
    assert np.array_equal(starts.numpy(), want)
    # complete episodes only, env by env in time order; the tails of envs 1 and 3 are cut episodes and give no entry
    ref = [_sum64(r, 0, 0, 1), _sum64(r, 0, 1, 5), _sum64(r, 0, 5, 8), _sum64(r, 1, 0, 3), _sum64(r, 1, 3, 6), _sum64(r, 2, 0, 8),
           _sum64(r, 3, 0, 4)]
    np.testing.assert_allclose(rets.numpy(), ref, rtol=0, atol=1e-14)


def test_assemble_first_k_complete_episodes():
    from quadsim_amd import IncompleteEpisodes, assemble_expert_dataset
    d, r, td, tr = _case()
    starts, rets, mask = assemble_expert_dataset(td, tr, 1)
    want = np.zeros((4, 8), bool)
    want[0, :1] = True; want[1, :3] = True; want[2, :8] = True; want[3, :4] = True
    assert np.array_equal(mask.numpy(), want)
    np.testing.assert_allclose(rets.numpy(), [_sum64(r, 0, 0, 1), _sum64(r, 1, 0, 3), _sum64(r, 2, 0, 8), _sum64(r, 3, 0, 4)],
                               rtol=0, atol=1e-14)
    assert int(starts[mask].sum()) == 4 and len(rets) == 4
    # envs 2 and 3 never finish two episodes within the 8 steps: refused, no cut episode is emitted
    with pytest.raises(IncompleteEpisodes):
        assemble_expert_dataset(td, tr, 2)
    # ... and with those two envs left out, two episodes each, the one ending on the last step included
    starts, rets, mask = assemble_expert_dataset(td[:2], tr[:2], 2)
    want = np.zeros((2, 8), bool)
    want[0, :5] = True; want[1, :6] = True
    assert np.array_equal(mask.numpy(), want)
    np.testing.assert_allclose(rets.numpy(), [_sum64(r, 0, 0, 1), _sum64(r, 0, 1, 5), _sum64(r, 1, 0, 3), _sum64(r, 1, 3, 6)],
                               rtol=0, atol=1e-14)
    assert int(starts[mask].sum()) == 4
    starts, rets, mask = assemble_expert_dataset(td[:1], tr[:1], 3)
    assert bool(mask.all()) and len(rets) == 3 and rets[2].item() == pytest.approx(_sum64(r, 0, 5, 8), abs=1e-14)
    with pytest.raises(ValueError):
        assemble_expert_dataset(td, tr, 0)


def test_episode_returns_are_segmented_float64_sums():
    """a long recording of large rewards followed by a short episode of tiny ones: the short episode's return keeps its own
    precision (a difference of float32 or running totals would not)"""
    import torch
    from quadsim_amd import assemble_expert_dataset
    T = 4000
    r = np.full((1, T), 1.0e4, np.float32)
    r[0, -3:] = np.float32(1.0e-4)
    d = np.zeros((1, T), bool)
    d[0, T - 4] = True; d[0, T - 1] = True
    _, rets, _ = assemble_expert_dataset(torch.as_tensor(d), torch.as_tensor(r))
    small = 3.0 * float(np.float32(1.0e-4))
    assert abs(rets[1].item() - small) <= 2 * 3 * 2.0 ** -53 * small


def test_record_expert_dataset_needs_exactly_one_of_n_steps_n_episodes():
    """both or neither -> ValueError, before anything touches a device"""
    from quadsim_amd import record_expert_dataset
    env = types.SimpleNamespace(num_envs=4)
    with pytest.raises(ValueError):
        record_expert_dataset(env)
    with pytest.raises(ValueError):
        record_expert_dataset(env, 700, n_episodes=2)
    with pytest.raises(ValueError):
        record_expert_dataset(env, n_steps=700, n_episodes=1, fused=False)
    with pytest.raises(ValueError):
        record_expert_dataset(env, fused=False)
