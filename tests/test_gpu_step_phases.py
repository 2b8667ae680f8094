"""-m gpu: the resident step loop, whichever reset-preparation variant it resolves (its own choice since it picks two waves per
tile for large handles, or a forced one), computes what every other launch path of the same handle computes, bit for bit.

Per case (env, integrator, reset mode, reset-preparation variant, per-env params) and env count (1, 63, 65, 257: one lane, a
ragged tile below and above one tile, five workgroups): 24 steps in which every env resets at least twice -- all of them time out
at step 1 (`t` set two steps before the time-out), and after step 11 every chaser is put just outside the range limit.  Run
  1. on a host-ordered private queue: the resident kernel k_env_resident (qs_debug_chain_resident counts its dispatches);
  2. on the HIP stream: k_env_split;
  3. in a child process with QS_RESIDENT=0: the packet chain of k_env_split on the private queue;
  4. in a child process with QS_SPLIT=0: the serial kernel k_env on the HIP stream.
All four must agree on every step's obs, reward, done, flags, terminal obs and terminal state, on the state and the params at
the drain in the middle and at the end, and on the step counter.  The two children run every case once (module fixture)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

T, HALF, P = 24, 12, 6
SIZES = (1, 63, 65, 257)
PAR_NOM = np.array([0.18, 0.00025, 0.000232, 0.0003738])
FAMILY = {"serial": 0, "hip": 1, "resident": 2, "chain": 3}    # StepFamily of qs_debug_step_variant
# (env id, integrator, randomise, stored init states, per-env params set, reset preparation: 0 two waves per tile, 2 three)
CASES = [
    ("docking-v0", "frozen", 1, False, False, 2),
    ("docking-v0", "frozen", 1, False, False, 0),
    ("docking-v0", "rk4", 1, False, True, 2),
    ("docking-v2", "frozen", 1, False, True, 0),
    ("docking-v2", "frozen", 2, False, False, 2),
    ("docking-v2", "rk4", 2, False, False, 0),
    ("docking-v0", "frozen", 0, False, False, 0),
    ("docking-v2", "rk4", 0, False, True, 0),
    ("docking-v0", "frozen", 0, True, False, 0),
    ("docking-v2", "rk4", 1, True, True, 2),
]
KEYS = ("obs", "rew", "done", "flags", "term", "tstate", "state_mid", "par_mid", "state_end", "par_end", "counter")


def _case_id(case):
    env_id, integ, rnd, init, par, prep = case
    return "%s-%s-%s-prep%d-%s" % (env_id[-2:], integ, "init" if init else "rnd%d" % rnd, prep, "par" if par else "nopar")


def _full_state(env):
    st = env.get_state()
    return np.concatenate([st[k].reshape(len(st["t"]), -1) for k in sorted(st)], 1)


def _params(env):
    m, inertia = env.get_params()
    return np.concatenate([m[:, None], inertia], axis=1)


def _dispatches(env):
    env._lib.qs_debug_chain_resident.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    d = C.c_uint64(0)
    assert env._lib.qs_debug_chain_resident(env._h, C.byref(d)) == 0
    return int(d.value)


def _family(env):
    env._lib.qs_debug_step_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    out = (C.c_int32 * 5)()
    assert env._lib.qs_debug_step_variant(env._h, out) == 0, env._lib.qs_last_error()
    return int(out[0])


def run_case(qa, torch, case, n, path):
    """the case's 24 steps on launch path `path` ('resident', 'hip', 'chain', 'serial') -> {key: numpy array}"""
    env_id, integ, rnd, set_init, set_par, prep = case
    seed = 40 + CASES.index(case)
    lib = qa._lib.load()
    lib.qs_debug_set_reset_prep.argtypes = [C.c_int]
    lib.qs_debug_set_reset_prep(prep)
    try:
        kw = dict(num_envs=n, integrator=integ, randomise=rnd, seed=seed, copy=False, env_id_offset=977)
        if rnd:
            kw.update(init_range=qa.C3_INIT_RANGE, mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2))
        env = qa.VecDockingEnv(env_id, **kw)
        rng = np.random.default_rng(seed)
        if set_init:
            env.reset()
            st = env.get_state()
            ini = []
            for s in (st["chaser"], st["target"]):
                s = s.copy()
                s[:, 0:3] += rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32)
                q = s[:, 6:10] + rng.uniform(-0.05, 0.05, (n, 4)).astype(np.float32)
                s[:, 6:10] = q / np.linalg.norm(q, axis=1, keepdims=True)
                s[:, 10:13] += rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
                ini.append(s.astype(np.float32))
            env.set_init_state(*ini)
        env.reset()
        if set_par:
            env.set_params(mass=(0.18 * rng.uniform(0.85, 1.15, n)).astype(np.float32),
                           inertia=(PAR_NOM[1:] * rng.uniform(0.85, 1.15, (n, 3))).astype(np.float32))
        env.set_state(t=np.full(n, 598.0, np.float32))           # two steps before the time-out: every env resets at step 1
        if path in ("resident", "chain"):
            env.set_queue_mode(True, 1, ordering="host")
            assert env.queue_ordering == "host"
        assert _family(env) == FAMILY[path], (_family(env), path)
        acts = torch.from_numpy(rng.uniform(-1.0, 1.0, (P, n, 4)).astype(np.float32)).cuda()
        kwd = dict(device="cuda")
        obs = torch.empty((T, n, 12), dtype=torch.float32, **kwd)
        rew = torch.empty((T, n), dtype=torch.float32, **kwd)
        done = torch.empty((T, n), dtype=torch.uint8, **kwd)
        flags = torch.empty((T, n), dtype=torch.uint8, **kwd)
        term = torch.full((T, n, 12), -7.0, dtype=torch.float32, **kwd)
        tstate = torch.full((T, n, 26), -9.0, dtype=torch.float32, **kwd)
        p = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
        d0 = _dispatches(env)

        def steps(ks):
            torch.cuda.synchronize()                             # host-ordered: the inputs are complete at the call
            for k in ks:
                r = env._lib.qs_step_ex(env._h, p(acts[k % P]), p(obs[k]), p(rew[k]), p(done[k]), p(flags[k]), p(term[k]), p(tstate[k]))
                assert r == 0, env._lib.qs_last_error()
        steps(range(HALF))
        out = {"state_mid": _full_state(env), "par_mid": _params(env)}   # drains the roll-out
        st = env.get_state()
        c = st["chaser"].copy()
        rmax = 10.0 if env_id == "docking-v2" else 3.0
        c[:, 0:3] = st["target"][:, 0:3]
        c[:, 1] += np.float32(rmax * 1.05)                       # just outside the range limit: every env resets at step 12
        env.set_state(chaser=c)
        steps(range(HALF, T))
        env.sync()
        torch.cuda.synchronize()
        d1 = _dispatches(env)
        assert (d1 > d0) if path == "resident" else (d1 == 0), (path, d0, d1)
        out.update(obs=obs.cpu().numpy(), rew=rew.cpu().numpy(), done=done.cpu().numpy(), flags=flags.cpu().numpy(),
                   term=term.cpu().numpy(), tstate=tstate.cpu().numpy(), state_end=_full_state(env), par_end=_params(env),
                   counter=np.array([env.step_counter], np.int64))
        env.close()
    finally:
        lib.qs_debug_set_reset_prep(-1)
    return out


def _child_main(path, out_file):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import quadsim_amd as qa
    res = {}
    for i, case in enumerate(CASES):
        for n in SIZES:
            for k, v in run_case(qa, torch, case, n, path).items():
                res["%d_%d_%s" % (i, n, k)] = v
    np.savez(out_file, **res)


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """every case on the packet chain (QS_RESIDENT=0) and on the serial kernel (QS_SPLIT=0): both switches are read once per
    process, so one child process each, started together"""
    d = tmp_path_factory.mktemp("step_phases")
    procs = {}
    for path, var in (("chain", "QS_RESIDENT"), ("serial", "QS_SPLIT")):
        f = str(d / (path + ".npz"))
        procs[path] = (f, subprocess.Popen([sys.executable, os.path.abspath(__file__), path, f], env=dict(os.environ, **{var: "0"}),
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for path, (f, pr) in procs.items():
        log = pr.communicate(timeout=600)[0]
        assert pr.returncode == 0, "%s child failed (%d):\n%s" % (path, pr.returncode, log[-3000:])
        out[path] = np.load(f)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_step_paths_agree_bit_for_bit(qa, torch, children, case, n):
    res = run_case(qa, torch, case, n, "resident")
    hip = run_case(qa, torch, case, n, "hip")
    i = CASES.index(case)
    others = {"hip": hip}
    for path in ("chain", "serial"):
        others[path] = {k: children[path]["%d_%d_%s" % (i, n, k)] for k in KEYS}
    resets = res["done"].astype(np.int64).sum(axis=0)
    assert resets.min() >= 2, resets.min()                       # every env: the time-out and the range limit
    assert res["done"][1].all() and res["done"][HALF].all()
    assert int(res["counter"][0]) == T
    for path, o in others.items():
        for k in KEYS:
            assert res[k].dtype == o[k].dtype and np.array_equal(res[k].view(np.uint8), o[k].view(np.uint8)), (path, k)
    # rows of envs that did not finish keep the pattern; finished rows were written
    dn = res["done"].astype(bool)
    assert np.all(res["term"][~dn] == -7.0) and np.all(res["tstate"][~dn] == -9.0)
    assert np.all(res["term"][dn] != -7.0)


@pytest.mark.gpu
def test_resident_path_resolves_its_own_reset_preparation(qa):
    """host-ordered private queue, rocRAND resets: up to 768 tiles the resident kernel takes the packet chain's three-wave variant
    (PREP 2), above it the two-wave one (PREP 0) -- unless a variant is forced"""
    lib = qa._lib.load()
    lib.qs_debug_set_reset_prep.argtypes = [C.c_int]
    lib.qs_debug_step_variant.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]

    def variant(n, rnd):
        env = qa.VecDockingEnv("docking-v0", num_envs=n, randomise=rnd, seed=5, init_range=qa.C3_INIT_RANGE, copy=False)
        env.reset()
        env.set_queue_mode(True, 1, ordering="host")
        out = (C.c_int32 * 5)()
        assert lib.qs_debug_step_variant(env._h, out) == 0, lib.qs_last_error()
        env.close()
        return tuple(out)
    assert variant(768 * 64, 1) == (FAMILY["resident"], 0, 0, 1, 2)
    assert variant(768 * 64 + 1, 1) == (FAMILY["resident"], 0, 0, 1, 0)
    assert variant(65536, 1) == (FAMILY["resident"], 0, 0, 1, 0)
    assert variant(65536, 2) == (FAMILY["resident"], 0, 1, 2, 0)
    assert variant(65536, 0) == (FAMILY["resident"], 0, 0, 0, 0)
    try:
        lib.qs_debug_set_reset_prep(2)
        assert variant(65536, 1) == (FAMILY["resident"], 0, 0, 1, 2)
    finally:
        lib.qs_debug_set_reset_prep(-1)


def test_role_split_kernels_keep_their_resource_limits(tmp_path):
    """CPU: every k_env_resident / k_env_split instantiation of the built code object -- no scratch, no VGPR spill, LDS that
    lets four workgroups share a CU's 160 KiB, at most 168 VGPRs (resident; three waves per SIMD) and at most 128 for the
    three-wave k_env_split<.., 2> (four waves per SIMD)"""
    from kernel_notes import code_object, instantiations, kernel_notes
    notes = kernel_notes(code_object(tmp_path))
    seen = instantiations(notes, ["k_env_resident", "k_env_split"])
    assert len([k for k in seen if k[0] == "k_env_resident"]) == 20 and len([k for k in seen if k[0] == "k_env_split"]) == 20, seen
    checked = 0
    for sym, f in notes.items():
        m = re.search(r"_GLOBAL__N_1\d+(k_env_resident|k_env_split)ILi\d+ELb\d+ELi\d+ELi(\d+)E", sym)
        if not m:
            continue
        checked += 1
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (sym, f)
        assert f["group_segment_fixed_size"] <= 160 * 1024 // 4, (sym, f)
        cap = 168 if m.group(1) == "k_env_resident" else (128 if m.group(2) == "2" else 168)
        assert f["vgpr_count"] <= cap, (sym, f)
    assert checked == 40, checked


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
