"""-m "not gpu": everything of TD3 on the device that needs no device.  include/quadsim_td3.h is plain C99 and every symbol it
declares is exported by libquadsim_td3.so; the entry of _lib.SIDE matches the header's prototypes (tests/side_cases.py has the
checks every side library shares); every refusal the header promises happens before
anything is launched, and check_td3_args mirrors it; tests/td3_matrix.py has exactly one row per kernel of the code object, none uses
scratch and each fits the compute unit's LDS; the schedule of actor steps; tests/td3_ref.py is checked against torch's float64
autograd (quadsim_amd.torch_td3_update, which it shares no code with), its fixtures lie on every edge of the target value and off
every ReLU edge; the float64 reference meets the learning condition the device is held to; and the recorded instruction diff of the
other nine libraries says `same` for every kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import kernel_notes
import side_cases
import td3_matrix
import td3_ref as td
import test_call_path_cpu as call_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS, NETS, ONLINE = td.KEYS, td.NETS, td.ONLINE
EXPECTED = ["qstd_last_error", "qstd_update", "qstd_version", "qstd_workspace_bytes"]


def entry():
    from quadsim_amd import _lib
    return _lib.SIDE["td3"]


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, td3
    _lib.build_library()
    return td3.load_td3()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from quadsim_amd import _lib
    _lib.build_library()
    co = kernel_notes.code_object(tmp_path_factory.mktemp("isa_td3"), so=entry()["path"])
    return kernel_notes.kernel_notes(co, kernel_notes.FIELDS + ("sgpr_spill_count",))


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_header_table_and_exports_are_the_same_names(lib):
    """the header's prototypes are exactly the table's signatures (count and kind of every parameter, kind of the result), the
    library's defined symbols and the expected list; SIDE_POINTERS holds the pointers' positions; version 1"""
    from quadsim_amd import _lib
    e = entry()
    protos = call_path._header_prototypes(e["header"], e["prefix"])
    assert sorted(protos) == sorted(e["signatures"]) == sorted(e["exports"]) == EXPECTED
    for name, sig in e["signatures"].items():
        args, result = sig if isinstance(sig, tuple) else (sig, C.c_int)
        assert (call_path._ctype_kind(result), [call_path._ctype_kind(t) for t in args]) == protos[name], name
        assert _lib.SIDE_POINTERS[name] == tuple(i for i, k in enumerate(protos[name][1]) if k == "ptr"), name
    assert protos["qstd_last_error"] == ("ptr", []) and protos["qstd_version"] == ("int32", []) and len(protos["qstd_update"][1]) == 17
    side_cases.check_exports("td3", lib, EXPECTED)


def test_table_entry_names_its_own_files():
    import quadsim_amd as qa
    from quadsim_amd import _lib, td3
    e = entry()
    assert list(_lib.SIDE) == ["dyn", "dynmppi", "dynfit", "bc", "ppo", "gail", "trpo", "ddpg", "td3", "sac"]         # build order
    assert td3.TD3_EXPORTS is e["exports"]
    assert e["prefix"] == "qstd_" and e["kernels"] == b"k_td3_"
    # (with it: no file of the main library or of another entry carries this library's name, so the main library is not rebuilt for
    # its fragment)
    side_cases.check_entry("td3", ["quadsim_device.hpp", "quadsim_td3.h", "side_host.hpp", "side_offpolicy.hpp", "td3_kernels.hpp",
                                   "train_offpolicy.hpp", "train_pieces.hpp"], "td3.hip")
    for name in ("TD3", "TD3Policy", "NormalActionNoise", "td3_update", "torch_td3_update", "check_td3_args", "reset_td3_optimizer"):
        assert getattr(qa, name) is getattr(td3, name) and name in qa.__all__
    assert td3.TD3_MAX_STEPS == 4096 and td3.TD3_MAX_BATCH == 256 and td3.TD3_MAX_DELAY == 65536
    assert td3.ReplayBuffer is qa.ReplayBuffer and td3.OUNoise is qa.OUNoise and td3.replay_schedule is qa.replay_schedule
    assert td3.collect_and_train is qa.ddpg.collect_and_train                   # one collection loop for both off-policy trainers


def test_no_other_library_holds_its_kernels(lib):
    blob = open(entry()["path"], "rb").read()
    assert b"k_td3_step" in blob and b"k_td3_copy" in blob
    side_cases.check_no_foreign_kernels("td3")


def test_structs_and_workspace_match_the_header(lib):
    from quadsim_amd import _lib
    # the structs: two 32-bit fields, then 72 tensors; n and five tensors; nine doubles
    assert C.sizeof(_lib.QstdNets) == 8 + 72 * 8 and _lib.QstdNets.m.offset == 8 + 36 * 8 and _lib.QstdNets.v.offset == 8 + 54 * 8
    assert C.sizeof(_lib.QstdReplay) == 16 + 5 * 8 and C.sizeof(_lib.QstdHyper) == 8 + 9 * 8 and _lib.QstdHyper.policy_delay.offset == 4
    # the workspace: two buffers of six nets (each padded to four floats), and m, v and the gradients of the three online nets
    actor, critic = 12 * 128 + 128 + 128 * 128 + 128 + 128 * 4 + 4, 16 * 128 + 128 + 128 * 128 + 128 + 128 + 1
    online = ((actor + 3) & ~3) + 2 * ((critic + 3) & ~3)
    nbytes = C.c_size_t(0)
    assert lib.qstd_workspace_bytes(C.byref(nbytes)) == 0 and nbytes.value == 4 * (2 * 2 * online + 3 * online)
    assert lib.qstd_workspace_bytes(None) == 1 and b"bytes" in lib.qstd_last_error()


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_td3.h"

static float x[8192], y[30000], big[1900000];
static float ws_store[400000];
static int32_t idx[64];
static QstdNets nets;
static QstdReplay rp;
static QstdHyper hp;
static float *grads[18];
static size_t ws_bytes;

static int refused(int rc, const char *word)
{
    if (rc == QSTD_OK || strstr(qstd_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qstd_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int upd(int steps, int batch, int64_t t0, int64_t at0)
{
    return qstd_update(&nets, &rp, idx, NULL, steps, batch, &hp, t0, at0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL);
}

static int full(float *noise_out, void *ws, uint64_t bytes, float *stats, float *const *g)
{
    return qstd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, 0, NULL, 0, noise_out, ws, bytes, stats, g, NULL);
}

static void good(void)
{
    /* 72 tensors and 18 gradients that do not overlap: 20000 floats apart in `big` */
    int k, i;
    for (k = 0; k < 6; ++k) for (i = 0; i < 6; ++i) nets.w[k][i] = big + 20000 * (6 * k + i);
    for (k = 0; k < 3; ++k) for (i = 0; i < 6; ++i) { nets.m[k][i] = big + 20000 * (36 + 6 * k + i); nets.v[k][i] = big + 20000 * (54 + 6 * k + i); }
    for (i = 0; i < 18; ++i) grads[i] = big + 20000 * (72 + i);
    nets.struct_size = sizeof nets;
    rp.struct_size = sizeof rp; rp.n = 300; rp.obs0 = rp.act = rp.rew = rp.obs1 = rp.done = x;
    hp.struct_size = sizeof hp; hp.policy_delay = 2; hp.gamma = 0.99; hp.tau = 5e-3; hp.actor_lr = 3e-4; hp.critic_lr = 3e-4;
    hp.target_policy_noise = 0.2; hp.target_noise_clip = 0.5; hp.beta1 = 0.9; hp.beta2 = 0.999; hp.eps = 1e-8;
}

int main(void)
{
    int ok = 1;
    void *fns[] = {(void *)qstd_version, (void *)qstd_last_error, (void *)qstd_workspace_bytes, (void *)qstd_update};
    if (qstd_version() != QSTD_VERSION) return 2;
    if (qstd_workspace_bytes(&ws_bytes) != QSTD_OK || ws_bytes > sizeof ws_store) return 3;
    good();
    ok &= refused(upd(100, 0, 0, 0), "batch");
    ok &= refused(upd(100, 257, 0, 0), "batch");
    ok &= refused(upd(0, 10, 0, 0), "steps");
    ok &= refused(upd(4097, 10, 0, 0), "steps");
    rp.n = 0; ok &= refused(upd(100, 10, 0, 0), "n must"); good();
    rp.n = (int64_t)1 << 31; ok &= refused(upd(100, 10, 0, 0), "n must"); good();
    ok &= refused(upd(100, 10, -1, 0), "t0");
    ok &= refused(upd(100, 10, ((int64_t)1 << 31) - 50, 0), "t0");
    ok &= refused(upd(100, 10, 0, -1), "actor_t0");
    ok &= refused(upd(100, 10, 0, ((int64_t)1 << 31) - 50), "actor_t0");
    hp.policy_delay = 0; ok &= refused(upd(100, 10, 0, 0), "policy_delay"); good();
    hp.policy_delay = 65537; ok &= refused(upd(100, 10, 0, 0), "policy_delay"); good();
    hp.gamma = -0.1; ok &= refused(upd(100, 10, 0, 0), "gamma"); good();
    hp.gamma = 1.5; ok &= refused(upd(100, 10, 0, 0), "gamma"); good();
    hp.gamma = NAN; ok &= refused(upd(100, 10, 0, 0), "gamma"); good();
    hp.tau = 0.0; ok &= refused(upd(100, 10, 0, 0), "tau"); good();
    hp.tau = 1.5; ok &= refused(upd(100, 10, 0, 0), "tau"); good();
    hp.tau = NAN; ok &= refused(upd(100, 10, 0, 0), "tau"); good();
    hp.target_policy_noise = -0.1; ok &= refused(upd(100, 10, 0, 0), "target_policy_noise"); good();
    hp.target_policy_noise = NAN; ok &= refused(upd(100, 10, 0, 0), "target_policy_noise"); good();
    hp.target_policy_noise = INFINITY; ok &= refused(upd(100, 10, 0, 0), "target_policy_noise"); good();
    hp.target_noise_clip = -0.5; ok &= refused(upd(100, 10, 0, 0), "target_noise_clip"); good();
    hp.target_noise_clip = NAN; ok &= refused(upd(100, 10, 0, 0), "target_noise_clip"); good();
    hp.actor_lr = INFINITY; ok &= refused(upd(100, 10, 0, 0), "actor_lr"); good();
    hp.actor_lr = NAN; ok &= refused(upd(100, 10, 0, 0), "actor_lr"); good();
    hp.critic_lr = INFINITY; ok &= refused(upd(100, 10, 0, 0), "critic_lr"); good();
    hp.critic_lr = NAN; ok &= refused(upd(100, 10, 0, 0), "critic_lr"); good();
    hp.beta1 = 1.0; ok &= refused(upd(100, 10, 0, 0), "beta1"); good();
    hp.beta2 = -0.1; ok &= refused(upd(100, 10, 0, 0), "beta2"); good();
    hp.eps = INFINITY; ok &= refused(upd(100, 10, 0, 0), "eps"); good();
    /* two tensors one float short of disjoint, stats inside a moment, a gradient on a target weight, noise_out and the workspace on a net */
    nets.m[1][2] = nets.w[4][2] + 128 * 128 - 1; ok &= refused(upd(100, 10, 0, 0), "overlap"); good();
    ok &= refused(full(NULL, ws_store, ws_bytes, nets.v[0][0] + 8, NULL), "overlap");
    grads[7] = nets.w[3][4]; ok &= refused(full(NULL, ws_store, ws_bytes, y, grads), "overlap"); good();
    ok &= refused(full(nets.w[5][2] + 16, ws_store, ws_bytes, y, NULL), "overlap");
    ok &= refused(full(NULL, big, ws_bytes, y, NULL), "overlap");
    nets.w[5][3] = NULL; ok &= refused(upd(100, 10, 0, 0), "NULL"); good();
    nets.v[2][5] = (float *)((char *)nets.v[2][5] + 2); ok &= refused(upd(100, 10, 0, 0), "aligned"); good();
    rp.done = NULL; ok &= refused(upd(100, 10, 0, 0), "NULL"); good();
    grads[17] = NULL; ok &= refused(full(NULL, ws_store, ws_bytes, y, grads), "NULL"); good();
    nets.struct_size = 8; ok &= refused(upd(100, 10, 0, 0), "QstdNets.struct_size"); good();
    rp.struct_size = 8; ok &= refused(upd(100, 10, 0, 0), "QstdReplay.struct_size"); good();
    hp.struct_size = 8; ok &= refused(upd(100, 10, 0, 0), "QstdHyper.struct_size"); good();
    ok &= refused(full(NULL, ws_store, ws_bytes - 1, y, NULL), "workspace");
    ok &= refused(full(NULL, (char *)ws_store + 4, ws_bytes, y, NULL), "aligned");
    ok &= refused(full((float *)((char *)x + 2), ws_store, ws_bytes, y, NULL), "aligned");
    ok &= refused(qstd_update(NULL, &rp, idx, NULL, 100, 10, &hp, 0, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qstd_update(&nets, NULL, idx, NULL, 100, 10, &hp, 0, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qstd_update(&nets, &rp, NULL, NULL, 100, 10, &hp, 0, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qstd_update(&nets, &rp, idx, NULL, 100, 10, NULL, 0, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(full(NULL, NULL, ws_bytes, y, NULL), "NULL");
    ok &= refused(full(NULL, ws_store, ws_bytes, NULL, NULL), "NULL");
    ok &= refused(full(NULL, ws_store, ws_bytes, (float *)((char *)y + 2), NULL), "aligned");
    ok &= refused(qstd_workspace_bytes(NULL), "bytes");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    e = entry()
    assert shutil.which("gcc") is not None
    src = tmp_path / "td3_caller.c"
    src.write_text(C_CALLER)
    exe = str(tmp_path / "td3_caller")
    libdir = os.path.dirname(e["path"])
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-l" + e["file"][len("lib"):-len(".so")], "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ALL-REFUSED", str(len(EXPECTED))]


GOOD = dict(n=300, steps=100, batch=10, gamma=0.99, tau=5e-3, actor_lr=3e-4, critic_lr=3e-4, policy_delay=2, target_policy_noise=0.2,
            target_noise_clip=0.5, beta1=0.9, beta2=0.999, eps=1e-8, t0=0, actor_t0=0)


@pytest.mark.parametrize("kw", [
    dict(batch=0), dict(batch=257), dict(steps=0), dict(steps=4097), dict(n=0), dict(n=1 << 31), dict(t0=-1), dict(t0=(1 << 31) - 50),
    dict(actor_t0=-1), dict(actor_t0=(1 << 31) - 50), dict(policy_delay=0), dict(policy_delay=65537),
    dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(tau=0.0), dict(tau=1.5), dict(tau=float("nan")),
    dict(target_policy_noise=-0.1), dict(target_policy_noise=float("nan")), dict(target_policy_noise=float("inf")),
    dict(target_noise_clip=-0.5), dict(target_noise_clip=float("nan")), dict(actor_lr=float("inf")), dict(actor_lr=float("nan")),
    dict(critic_lr=float("inf")), dict(critic_lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=float("inf")),
    dict(steps=2, batch=3, counts=np.array([0, 3])), dict(steps=2, batch=3, counts=np.array([4, 3])), dict(steps=2, batch=3, counts=np.array([3])),
    dict(steps=2, batch=3, indices=np.array([[0, 1, 2], [3, 300, 5]])), dict(steps=2, batch=3, indices=np.array([[0, -1, 2], [3, 4, 5]])),
    dict(steps=2, batch=3, indices=np.zeros((2, 4), np.int32))],
    ids=lambda kw: "-".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_check_td3_args_refuses_before_the_library_is_touched(monkeypatch, kw):
    from quadsim_amd import td3

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(td3, "load_td3", touched)
    assert td3.check_td3_args(**GOOD) == (300, 100, 10, 0.99, 5e-3, 3e-4, 3e-4, 2, 0.2, 0.5, 0.9, 0.999, 1e-8, 0, 0)
    assert td3.check_td3_args((1 << 31) - 1, 4096, 256, 0.0, 1.0, 0.0, 0.0, 65536, 0.0, float("inf"), 0.0, 0.0, 0.0, (1 << 31) - 4097,
                              (1 << 31) - 4097)[0] == (1 << 31) - 1
    # entries at or beyond counts[s] are never read: they may hold anything
    assert td3.check_td3_args(300, 2, 3, counts=np.array([3, 1]), indices=np.array([[0, 1, 299], [3, -7, 1 << 30]]))[1] == 2
    with pytest.raises(ValueError):
        td3.check_td3_args(**dict(GOOD, **kw))


def test_host_policies_and_bad_arguments_are_refused(monkeypatch, tmp_path):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import td3
    monkeypatch.setattr(td3, "load_td3", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    p = qa.TD3Policy(seed=3, device="cpu")
    rb = qa.ReplayBuffer(32, device="cpu")
    idx = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(qa.QuadsimError):
        qa.td3_update(p, rb, idx)
    with pytest.raises(ValueError):
        qa.torch_td3_update(p, rb, idx + 32)
    with pytest.raises(ValueError):
        qa.torch_td3_update(p, rb, idx.long())
    with pytest.raises(ValueError):
        qa.torch_td3_update(p, rb, idx, noise=torch.zeros((1, 3, 4)))

    class Env:
        num_envs, device = 4, torch.device("cpu")
    with pytest.raises(ValueError, match="update"):
        qa.TD3(p, Env(), update="jax")
    with pytest.raises(ValueError, match="batch"):
        qa.TD3(p, Env(), batch_size=257)
    with pytest.raises(ValueError, match="policy_delay"):
        qa.TD3(p, Env(), policy_delay=0)
    model = qa.TD3(p, Env())                                           # SB2's defaults
    assert (model.train_freq, model.gradient_steps, model.batch_size, model.learning_starts, model.replay.capacity) == (100, 100, 128, 100, 50000)
    assert model.hyper == dict(gamma=0.99, tau=0.005, actor_lr=3e-4, critic_lr=3e-4, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5)
    # the policy: SB2's initialisation, the cache, save and load
    for name in ONLINE:
        shapes = td.shapes_of(name)
        for k, w, tw in zip(KEYS, getattr(p, name), getattr(p, name + "_target")):
            assert tuple(w.shape) == shapes[k] and w.dtype == torch.float32 and torch.equal(w, tw) and w.data_ptr() != tw.data_ptr()
            lim = 0.0 if len(shapes[k]) == 1 else np.sqrt(6.0 / sum(shapes[k]))
            assert float(w.abs().max()) <= lim and (lim == 0.0 or float(w.abs().max()) > 0.5 * lim)
    assert not torch.equal(p.q1[0], p.q2[0]) and not torch.equal(qa.TD3Policy(seed=4, device="cpu").actor[0], p.actor[0])
    assert sorted(p.actor_weights()) == sorted(KEYS) and p.actor_weights()["w1"].shape == (128, 128) and p.actor_weights() is p.actor_weights()
    a = p.predict(torch.randn((5, 12)) * 4.0)
    assert tuple(a.shape) == (5, 4) and float(a.abs().max()) < 1.0
    cached = p.actor_weights()
    rb.add(torch.randn((32, 12)), torch.rand((32, 4)), torch.randn(32), torch.randn((32, 12)), torch.zeros(32))
    qa.torch_td3_update(p, rb, torch.arange(8, dtype=torch.int32).reshape(2, 4))
    assert p.actor_weights() is not cached and not np.array_equal(p.actor_weights()["w1"], cached["w1"])      # dropped after an update
    assert (p.steps, p.actor_steps) == (2, 1)
    p.m["q2"][0][15, 0] = 0.5
    path = str(tmp_path / "td3.npz")
    p.save_npz(path)
    q = qa.TD3Policy.from_npz(path, device="cpu")
    assert (q.steps, q.actor_steps) == (2, 1) and float(q.m["q2"][0][15, 0]) == 0.5
    assert all(torch.equal(a, b) for x, y in zip(p.nets(), q.nets()) for a, b in zip(x, y))
    qa.reset_td3_optimizer(p)
    assert (p.steps, p.actor_steps) == (0, 0) and not p.m["q2"][0].any()
    noise = qa.NormalActionNoise(4096, sigma=0.1, device="cpu", seed=1)
    x = noise()
    assert tuple(x.shape) == (4096, 4) and abs(float(x.std()) - 0.1) < 0.005 and torch.equal(qa.NormalActionNoise(4096, device="cpu", seed=1)(), x)


# ---------------------------------------------------------------------------------------------------- the census
def test_rows_are_exactly_the_kernels_of_the_code_object_without_scratch(notes):
    side_cases.check_census(notes, td3_matrix, lambda n: kernel_notes.instantiations_with_types(n, td3_matrix.KERNELS, namespace="qstd"), "td3")


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(td3_matrix)


def test_the_other_nine_libraries_are_instruction_identical():
    """profiles/td3/isa_diff.txt is the output of tools/isa_diff.py, the parent commit's build against this one, for each of
    the other nine libraries, libquadsim_ddpg.so (whose streamed-net helpers moved into train_pieces.hpp) among them: every kernel
    line says `same`"""
    text = open(os.path.join(ROOT, "profiles", "td3", "isa_diff.txt")).read()
    libs = re.findall(r"^## (\S+)$", text, flags=re.M)
    assert libs == ["libquadsim_hip.so", "libquadsim_dyn.so", "libquadsim_dynmppi.so", "libquadsim_dynfit.so", "libquadsim_bc.so",
                    "libquadsim_ppo.so", "libquadsim_gail.so", "libquadsim_trpo.so", "libquadsim_ddpg.so"]
    lines = [ln for ln in text.splitlines() if re.match(r"^_Z\S+: ", ln)]
    assert len(lines) > 100 and all(ln.endswith(": same") for ln in lines)
    totals = re.findall(r"^identical in fields and disassembly: (\d+) of (\d+)$", text, flags=re.M)
    assert len(totals) == 9 and all(a == b for a, b in totals)
    assert not re.findall(r"only in (?:parent|branch) \[[^\]]+\]", text)


# ---------------------------------------------------------------------------------------------------- the schedule of actor steps
@pytest.mark.parametrize("delay", [1, 2, 3])
@pytest.mark.parametrize("t0", [0, 1, 5])
def test_schedule_of_actor_steps(delay, t0):
    """update u steps the actor exactly when u % policy_delay == 0, whatever the split of the run into calls: the count that the
    wrapper carries (td3.actor_steps) is the reference's, and the float64 loop moves the actor and the targets on those updates alone"""
    from quadsim_amd import td3
    steps = 5
    want = [(t0 + s) % delay == 0 for s in range(steps)]
    assert td.schedule(t0, steps, delay).tolist() == want
    assert td3.actor_steps(t0, steps, delay) == sum(want)
    assert all(td3.actor_steps(t0, a, delay) + td3.actor_steps(t0 + a, steps - a, delay) == sum(want) for a in range(steps + 1))
    P, rp = td.nets(), td.replay()
    Z = td.zero_state()
    idx, z = td.step_indices(4, steps=steps), td.noise(steps, 4)
    st = {"w": P, "m": Z, "v": Z}
    for s in range(steps):
        before = st
        Pn, Mn, Vn, S, taken = td.fit64(st["w"], st["m"], st["v"], rp, idx[s:s + 1], z[s:s + 1], t0=t0 + s, delay=delay, critic_lr=1e-2, actor_lr=1e-2)
        moved = [not all(np.array_equal(Pn[n][k], np.asarray(before["w"][n][k], np.float64)) for k in KEYS) for n in NETS]
        assert taken == int(want[s]) and moved == [want[s], True, True, want[s], want[s], want[s]], (s, moved)
        assert (S[0, 5] != 0.0) == want[s]
        st = {"w": Pn, "m": Mn, "v": Vn}


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("count", td.STEP_COUNTS)
def test_fixtures_lie_off_every_relu_edge_and_on_every_target_edge(count):
    """no pre-activation of a differentiated pass of the float64 reference lies within its bound of zero, no element excluded; from
    ten rows on the step's rows hold the noise clipped at +CL and at -CL, a1 + e clipped at +1 and at -1, qa < qb and qb < qa, terminal
    and non-terminal rows"""
    P, rp = td.nets(), td.replay()
    assert not td.relu_edges(P, rp[:2]).any()
    idx, z = td.step_indices(count), td.noise(1, count)
    rows = tuple(a[idx[0]] for a in rp)
    assert not td.relu_edges(P, rows[:2]).any()
    census = td.edge_census(P, rows, z[0])
    print("td3 fixture rows %d: %s" % (count, census))
    assert census["noise+"] > 0 and census["noise-"] > 0
    if count >= 10:
        assert all(v > 0 for v in census.values()), census


def _torch64(torch, P, M, V, rp, idx, z, **kw):
    import quadsim_amd as qa
    pol = qa.TD3Policy(device="cpu", weights={n: {k: np.asarray(P[n][k], np.float64) for k in KEYS} for n in NETS}, dtype="float64")
    for n in ONLINE:
        pol.m[n] = [torch.as_tensor(np.asarray(M[n][k], np.float64).copy()) for k in KEYS]
        pol.v[n] = [torch.as_tensor(np.asarray(V[n][k], np.float64).copy()) for k in KEYS]
    out = qa.torch_td3_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), noise=torch.as_tensor(z), return_grads=True, **kw)
    return pol, out


@pytest.mark.parametrize("count", [1, 17, 256])
def test_step64_against_torch_float64_autograd(count):
    """both losses, the three means, the actor's loss and all eighteen gradients to 1e-10 relative against torch_td3_update in float64
    on the host, which the restatement shares no code with -- and so far inside the bounds of step64"""
    import torch
    P, rp = td.nets(), td.replay()
    Z = td.zero_state()
    idx, z = td.step_indices(count), td.noise(1, count)
    stats, G, y, Es, E = td.step64(P, tuple(a[idx[0]] for a in rp), z[0], with_bound=True)
    pol, out = _torch64(torch, P, Z, Z, rp, idx, z)
    got = out["stats"][0].numpy()
    assert got.dtype == np.float64 and np.all(np.abs(got - stats) <= 1e-10 * np.maximum(1.0, np.abs(stats))) and np.all(np.abs(got - stats) <= Es)
    for n in ONLINE:
        for i, k in enumerate(KEYS):
            g = out["grads"][n][i].numpy()
            assert g.shape == td.shapes_of(n)[k] and np.abs(g - G[n][k]).max() <= 1e-10 * max(1.0, np.abs(G[n][k]).max()), (n, k)
            assert np.all(np.abs(g - G[n][k]) <= E[n][k]) and E[n][k].max() <= 0.5 * np.abs(G[n][k]).max(), (n, k)
    # (worst-case chains, six layers deep behind the target actor -- one more than DDPG's, whose action enters after layer 0)
    assert np.all(Es[:5] <= 0.1 * np.maximum(np.abs(stats[:5]), 0.1))
    # wildly different targets change nothing where every row is terminal
    huge = dict(P, q1_target={k: np.full_like(P["q1_target"][k], 1e30) for k in KEYS})
    term = tuple(a[idx[0]] for a in rp[:4]) + (np.ones(count, np.float32),)
    with np.errstate(over="ignore", invalid="ignore"):
        s2, G2, y2 = td.step64(huge, term, z[0])
    s1, G1, y1 = td.step64(P, term, z[0])
    assert np.array_equal(y1, y2) and np.array_equal(s1, s2) and all(np.array_equal(G1[n][k], G2[n][k]) for n in G1 for k in KEYS)


def test_fit64_against_the_torch_loop_with_delay_and_counts():
    """several updates with delay: five updates from t0 = 1 with policy_delay 2 (actor steps at u = 2, 4) and a count per step, the
    float64 loop of td3_ref against torch_td3_update in float64; and the loop is the loop of its parts"""
    import torch
    P, rp = td.nets(), td.replay()
    M, V = td.moments()
    idx, z = td.step_indices(8, steps=5), td.noise(5, 8)
    counts = np.array([8, 1, 7, 8, 3], np.int32)
    kw = dict(critic_lr=1e-2, actor_lr=1e-2)
    P5, M5, V5, S5, taken = td.fit64(P, M, V, rp, idx, z, counts, t0=1, actor_t0=4, **kw)
    assert taken == 2
    Pa, Ma, Va, Sa, ta = td.fit64(P, M, V, rp, idx[:2], z[:2], counts[:2], t0=1, actor_t0=4, **kw)
    Pb, Mb, Vb, Sb, tb = td.fit64(Pa, Ma, Va, rp, idx[2:], z[2:], counts[2:], t0=3, actor_t0=4 + ta, **kw)
    assert (ta, tb) == (1, 1) and all(np.array_equal(P5[n][k], Pb[n][k]) for n in NETS for k in KEYS) and np.array_equal(S5, np.concatenate([Sa, Sb]))
    import quadsim_amd as qa
    pol = qa.TD3Policy(device="cpu", weights={n: {k: np.asarray(P[n][k], np.float64) for k in KEYS} for n in NETS}, dtype="float64")
    for n in ONLINE:
        pol.m[n] = [torch.as_tensor(np.asarray(M[n][k], np.float64).copy()) for k in KEYS]
        pol.v[n] = [torch.as_tensor(np.asarray(V[n][k], np.float64).copy()) for k in KEYS]
    pol.steps, pol.actor_steps = 1, 4
    out = qa.torch_td3_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), torch.as_tensor(counts), noise=torch.as_tensor(z), **kw)
    assert (pol.steps, pol.actor_steps) == (6, 6)
    assert np.abs(out["stats"].numpy() - S5).max() <= 1e-9
    for n in NETS:
        for k, w in zip(KEYS, getattr(pol, n)):
            assert np.abs(w.numpy() - P5[n][k]).max() <= 1e-9 * max(1.0, np.abs(P5[n][k]).max()), (n, k)


def test_bounds_hold_for_torch_float32_in_another_summation_order():
    """torch's own float32 autograd of the same step (library GEMMs, another summation order, another tanh) stays within the derived
    bounds: they are not so tight that only the device's order meets them"""
    import torch
    import quadsim_amd as qa
    P, rp = td.nets(), td.replay()
    idx, z = td.step_indices(33), td.noise(1, 33)
    pol = qa.TD3Policy(device="cpu", weights=P)
    out = qa.torch_td3_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), noise=torch.as_tensor(z), return_grads=True)
    stats, G, y, Es, E = td.step64(P, tuple(a[idx[0]] for a in rp), z[0], with_bound=True)
    err = np.abs(out["stats"][0].double().numpy() - stats)
    assert np.all(err <= Es), (err, Es)
    for n in ONLINE:
        for k, g in zip(KEYS, out["grads"][n]):
            e = np.abs(g.double().numpy() - G[n][k])
            assert np.all(e <= E[n][k]), (n, k, (e / E[n][k]).max())
    assert pol.steps == 1 and pol.actor_steps == 1 and not torch.equal(pol.q2_target[2], torch.as_tensor(P["q2_target"]["w1"]))


def test_keyed_noise_of_the_host_path_is_the_references():
    """the normals that torch_td3_update draws without `noise` are float64 Box-Muller on the Philox words of (seed, update, slot),
    rounded to float32; tests/test_gpu_td3.py holds the device's noise_out to the same float64 values"""
    from quadsim_amd import td3
    z = td3.keyed_noise(77, 4, 3, 33)
    want = td.normals64(77, 4, 3, 33)
    assert z.dtype == np.float32 and z.shape == (3, 33, 4) and np.array_equal(z, want.astype(np.float32))
    assert np.array_equal(td3.keyed_noise(77, 5, 2, 10), z[1:, :10]) and not np.array_equal(td3.keyed_noise(78, 4, 3, 33), z)
    big = td3.keyed_noise(1, 0, 64, 256)
    assert abs(float(big.mean())) < 0.02 and abs(float(big.std()) - 1.0) < 0.02


def test_the_regression_case_is_learnt_in_float64():
    """the condition tests/test_gpu_td3.py holds the device to, met by the float64 reference with room: for either critic the mean
    loss of the last 20 of 200 updates is below a QUARTER of that of the first 20 (the device has to reach half)"""
    P, rp, idx, z = td.learn_case()
    Z = td.zero_state()
    st = td.fit64(P, Z, Z, rp, idx, z, critic_lr=td.LEARN_LR, actor_lr=td.LEARN_LR)[3]
    for c in (0, 1):
        first, last = st[:20, c].mean(), st[-20:, c].mean()
        print("td3 learn float64: q%d loss first 20 %.4g, last 20 %.4g" % (c + 1, first, last))
        assert last < 0.25 * first
