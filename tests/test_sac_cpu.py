"""-m "not gpu": everything of SAC on the device that needs no device.  include/quadsim_sac.h is plain C99 and every symbol it
declares is exported by libquadsim_sac.so; the entry of _lib.SIDE matches the header's prototypes (tests/side_cases.py has the
checks every side library shares); every refusal the header promises happens before anything is launched, and check_sac_args
mirrors it; tests/sac_matrix.py has exactly one row per
kernel of the code object, none uses scratch and each fits the compute unit's LDS; tests/sac_ref.py is checked against torch's float64
autograd (quadsim_amd.torch_sac_update, which it shares no code with), its fixtures lie off every ReLU edge and off the clamp's ends
with |u| <= 3; the float64 reference meets the learning condition the device is held to; and the recorded instruction diff of the
other ten libraries says `same` for every kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from quadsim_amd import sac as _feature  # noqa: F401  (without the feature nothing of this file is collected)

import kernel_notes
import sac_matrix
import sac_ref as sr
import side_cases
import test_call_path_cpu as call_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS, NETS, ONLINE = sr.KEYS, sr.NETS, sr.ONLINE
EXPECTED = ["qss_last_error", "qss_math", "qss_update", "qss_version", "qss_workspace_bytes"]


def entry():
    from quadsim_amd import _lib
    return _lib.SIDE["sac"]


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, sac
    _lib.build_library()
    return sac.load_sac()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from quadsim_amd import _lib
    _lib.build_library()
    co = kernel_notes.code_object(tmp_path_factory.mktemp("isa_sac"), so=entry()["path"])
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
    assert protos["qss_last_error"] == ("ptr", []) and protos["qss_version"] == ("int32", []) and len(protos["qss_update"][1]) == 17
    assert protos["qss_math"] == ("int32", ["int32", "ptr", "ptr", "int64", "ptr"])
    side_cases.check_exports("sac", lib, EXPECTED)


def test_table_entry_names_its_own_files():
    import quadsim_amd as qa
    from quadsim_amd import _lib, sac
    e = entry()
    assert list(_lib.SIDE) == ["dyn", "dynmppi", "dynfit", "bc", "ppo", "gail", "trpo", "ddpg", "td3", "sac"]         # build order
    assert sorted(e) == sorted(_lib.SIDE["td3"])                                # the same shape of entry, derived fields included
    assert sac.SAC_EXPORTS is e["exports"]
    assert e["prefix"] == "qss_" and e["kernels"] == b"k_sac_"
    # (with it: no file of the main library or of another entry carries this library's name, so the main library is not rebuilt for
    # its fragment)
    side_cases.check_entry("sac", ["quadsim_device.hpp", "quadsim_sac.h", "sac_kernels.hpp", "side_host.hpp", "side_offpolicy.hpp",
                                   "train_offpolicy.hpp", "train_pieces.hpp"], "sac.hip")
    for name in ("SAC", "SACPolicy", "sac_update", "torch_sac_update", "check_sac_args", "reset_sac_optimizer"):
        assert getattr(qa, name) is getattr(sac, name) and name in qa.__all__
    assert sac.SAC_MAX_STEPS == 4096 and sac.SAC_MAX_BATCH == 256 and sac.SAC_NOISE_STREAM == sr.NOISE_STREAM == 7
    assert sac.ReplayBuffer is qa.ReplayBuffer and sac.replay_schedule is qa.replay_schedule
    assert sac.collect_and_train is qa.ddpg.collect_and_train                   # one collection loop for the three off-policy trainers
    text = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.SIDE.items()" in text


def test_no_other_library_holds_its_kernels(lib):
    blob = open(entry()["path"], "rb").read()
    assert b"k_sac_step" in blob and b"k_sac_copy" in blob and b"k_sac_math" in blob
    side_cases.check_no_foreign_kernels("sac")


def test_structs_and_workspace_match_the_header(lib):
    from quadsim_amd import _lib
    # the structs: two 32-bit fields, then 78 tensors and alpha_state; n and five tensors; seven doubles; four traces
    assert C.sizeof(_lib.QssNets) == 8 + 79 * 8 and _lib.QssNets.m.offset == 8 + 30 * 8 and _lib.QssNets.v.offset == 8 + 54 * 8
    assert _lib.QssNets.alpha_state.offset == 8 + 78 * 8
    assert C.sizeof(_lib.QssReplay) == 16 + 5 * 8 and C.sizeof(_lib.QssHyper) == 8 + 7 * 8 and _lib.QssHyper.auto_alpha.offset == 4
    assert C.sizeof(_lib.QssTrace) == 8 + 4 * 8
    # the workspace: two buffers of five nets (each padded to four floats), m, v and the gradients of the four online nets, four floats
    actor, critic = 12 * 128 + 128 + 128 * 128 + 128 + 128 * 8 + 8, 16 * 128 + 128 + 128 * 128 + 128 + 128 + 1
    value = 12 * 128 + 128 + 128 * 128 + 128 + 128 + 1
    pad = lambda n: (n + 3) & ~3                                                 # noqa: E731
    online = pad(actor) + 2 * pad(critic) + pad(value)
    nbytes = C.c_size_t(0)
    assert lib.qss_workspace_bytes(C.byref(nbytes)) == 0 and nbytes.value == 4 * (2 * (online + pad(value)) + 3 * online + 4)
    assert lib.qss_workspace_bytes(None) == 1 and b"bytes" in lib.qss_last_error()


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_sac.h"

static float x[8192], y[40000], big[2200000];
static float ws_store[500000];
static int32_t idx[64];
static QssNets nets;
static QssReplay rp;
static QssHyper hp;
static QssTrace tr;
static float *grads[24];
static size_t ws_bytes;

static int refused(int rc, const char *word)
{
    if (rc == QSS_OK || strstr(qss_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qss_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int upd(int steps, int batch, int64_t t0)
{
    return qss_update(&nets, &rp, idx, NULL, steps, batch, &hp, t0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL, NULL);
}

static int full(float *noise_out, void *ws, uint64_t bytes, float *stats, const QssTrace *t, float *const *g)
{
    return qss_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, NULL, 0, noise_out, ws, bytes, stats, t, g, NULL);
}

static void good(void)
{
    /* 78 tensors, alpha_state and 24 gradients that do not overlap: 20000 floats apart in `big` */
    int k, i;
    for (k = 0; k < 5; ++k) for (i = 0; i < 6; ++i) nets.w[k][i] = big + 20000 * (6 * k + i);
    for (k = 0; k < 4; ++k) for (i = 0; i < 6; ++i) { nets.m[k][i] = big + 20000 * (30 + 6 * k + i); nets.v[k][i] = big + 20000 * (54 + 6 * k + i); }
    nets.alpha_state = big + 20000 * 78;
    for (i = 0; i < 24; ++i) grads[i] = big + 20000 * (79 + i);
    nets.struct_size = sizeof nets;
    rp.struct_size = sizeof rp; rp.n = 300; rp.obs0 = rp.act = rp.rew = rp.obs1 = rp.done = x;
    hp.struct_size = sizeof hp; hp.auto_alpha = 1; hp.gamma = 0.99; hp.tau = 5e-3; hp.lr = 3e-4; hp.target_entropy = -4.0;
    hp.beta1 = 0.9; hp.beta2 = 0.999; hp.eps = 1e-8;
    tr.struct_size = sizeof tr; tr.logp_out = tr.vlogp_out = tr.act_out = tr.fwd_out = NULL;
}

int main(void)
{
    int ok = 1;
    void *fns[] = {(void *)qss_version, (void *)qss_last_error, (void *)qss_workspace_bytes, (void *)qss_update, (void *)qss_math};
    if (qss_version() != QSS_VERSION) return 2;
    if (qss_workspace_bytes(&ws_bytes) != QSS_OK || ws_bytes > sizeof ws_store) return 3;
    good();
    ok &= refused(upd(100, 0, 0), "batch");
    ok &= refused(upd(100, 257, 0), "batch");
    ok &= refused(upd(0, 10, 0), "steps");
    ok &= refused(upd(4097, 10, 0), "steps");
    rp.n = 0; ok &= refused(upd(100, 10, 0), "n must"); good();
    rp.n = (int64_t)1 << 31; ok &= refused(upd(100, 10, 0), "n must"); good();
    ok &= refused(upd(100, 10, -1), "t0");
    ok &= refused(upd(100, 10, ((int64_t)1 << 31) - 50), "t0");
    hp.auto_alpha = 2; ok &= refused(upd(100, 10, 0), "auto_alpha"); good();
    hp.auto_alpha = -1; ok &= refused(upd(100, 10, 0), "auto_alpha"); good();
    hp.gamma = -0.1; ok &= refused(upd(100, 10, 0), "gamma"); good();
    hp.gamma = 1.5; ok &= refused(upd(100, 10, 0), "gamma"); good();
    hp.gamma = NAN; ok &= refused(upd(100, 10, 0), "gamma"); good();
    hp.tau = 0.0; ok &= refused(upd(100, 10, 0), "tau"); good();
    hp.tau = 1.5; ok &= refused(upd(100, 10, 0), "tau"); good();
    hp.tau = NAN; ok &= refused(upd(100, 10, 0), "tau"); good();
    hp.target_entropy = NAN; ok &= refused(upd(100, 10, 0), "target_entropy"); good();
    hp.target_entropy = -INFINITY; ok &= refused(upd(100, 10, 0), "target_entropy"); good();
    hp.lr = INFINITY; ok &= refused(upd(100, 10, 0), "lr"); good();
    hp.lr = NAN; ok &= refused(upd(100, 10, 0), "lr"); good();
    hp.beta1 = 1.0; ok &= refused(upd(100, 10, 0), "beta1"); good();
    hp.beta2 = -0.1; ok &= refused(upd(100, 10, 0), "beta2"); good();
    hp.eps = INFINITY; ok &= refused(upd(100, 10, 0), "eps"); good();
    /* two tensors one float short of disjoint, stats inside a moment, a gradient on the target, alpha_state inside a net, noise_out,
       a trace and the workspace on a net */
    nets.m[1][2] = nets.w[4][2] + 128 * 128 - 1; ok &= refused(upd(100, 10, 0), "overlap"); good();
    ok &= refused(full(NULL, ws_store, ws_bytes, nets.v[0][0] + 8, NULL, NULL), "overlap");
    grads[7] = nets.w[4][4]; ok &= refused(full(NULL, ws_store, ws_bytes, y, NULL, grads), "overlap"); good();
    nets.alpha_state = nets.w[0][2] + 5; ok &= refused(upd(100, 10, 0), "overlap"); good();
    ok &= refused(full(nets.w[3][2] + 16, ws_store, ws_bytes, y, NULL, NULL), "overlap");
    tr.fwd_out = nets.m[2][2]; ok &= refused(full(NULL, ws_store, ws_bytes, y, &tr, NULL), "overlap"); good();
    tr.logp_out = y + 8; ok &= refused(full(NULL, ws_store, ws_bytes, y, &tr, NULL), "overlap"); good();
    ok &= refused(full(NULL, big, ws_bytes, y, NULL, NULL), "overlap");
    nets.w[4][3] = NULL; ok &= refused(upd(100, 10, 0), "NULL"); good();
    nets.alpha_state = NULL; ok &= refused(upd(100, 10, 0), "NULL"); good();
    nets.v[3][5] = (float *)((char *)nets.v[3][5] + 2); ok &= refused(upd(100, 10, 0), "aligned"); good();
    rp.done = NULL; ok &= refused(upd(100, 10, 0), "NULL"); good();
    grads[23] = NULL; ok &= refused(full(NULL, ws_store, ws_bytes, y, NULL, grads), "NULL"); good();
    tr.act_out = (float *)((char *)x + 2); ok &= refused(full(NULL, ws_store, ws_bytes, y, &tr, NULL), "aligned"); good();
    nets.struct_size = 8; ok &= refused(upd(100, 10, 0), "QssNets.struct_size"); good();
    rp.struct_size = 8; ok &= refused(upd(100, 10, 0), "QssReplay.struct_size"); good();
    hp.struct_size = 8; ok &= refused(upd(100, 10, 0), "QssHyper.struct_size"); good();
    tr.struct_size = 8; ok &= refused(full(NULL, ws_store, ws_bytes, y, &tr, NULL), "QssTrace.struct_size"); good();
    ok &= refused(full(NULL, ws_store, ws_bytes - 1, y, NULL, NULL), "workspace");
    ok &= refused(full(NULL, (char *)ws_store + 4, ws_bytes, y, NULL, NULL), "aligned");
    ok &= refused(full((float *)((char *)x + 2), ws_store, ws_bytes, y, NULL, NULL), "aligned");
    ok &= refused(qss_update(NULL, &rp, idx, NULL, 100, 10, &hp, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(qss_update(&nets, NULL, idx, NULL, 100, 10, &hp, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(qss_update(&nets, &rp, NULL, NULL, 100, 10, &hp, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(qss_update(&nets, &rp, idx, NULL, 100, 10, NULL, 0, NULL, 0, NULL, ws_store, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(full(NULL, NULL, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(full(NULL, ws_store, ws_bytes, NULL, NULL, NULL), "NULL");
    ok &= refused(full(NULL, ws_store, ws_bytes, (float *)((char *)y + 2), NULL, NULL), "aligned");
    ok &= refused(qss_workspace_bytes(NULL), "bytes");
    ok &= refused(qss_math(3, x, y, 16, NULL), "which");
    ok &= refused(qss_math(-1, x, y, 16, NULL), "which");
    ok &= refused(qss_math(QSS_MATH_LN, NULL, y, 16, NULL), "NULL");
    ok &= refused(qss_math(QSS_MATH_LN, x, (float *)((char *)y + 2), 16, NULL), "aligned");
    ok &= refused(qss_math(QSS_MATH_JAC, x, y, 0, NULL), "n must");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    e = entry()
    assert shutil.which("gcc") is not None
    src = tmp_path / "sac_caller.c"
    src.write_text(C_CALLER)
    exe = str(tmp_path / "sac_caller")
    libdir = os.path.dirname(e["path"])
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + libdir,
                           "-l" + e["file"][len("lib"):-len(".so")], "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == ["ALL-REFUSED", str(len(EXPECTED))]


GOOD = dict(n=300, steps=100, batch=10, gamma=0.99, tau=5e-3, lr=3e-4, target_entropy=-4.0, auto_alpha=True, beta1=0.9, beta2=0.999, eps=1e-8, t0=0)


@pytest.mark.parametrize("kw", [
    dict(batch=0), dict(batch=257), dict(steps=0), dict(steps=4097), dict(n=0), dict(n=1 << 31), dict(t0=-1), dict(t0=(1 << 31) - 50),
    dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(tau=0.0), dict(tau=1.5), dict(tau=float("nan")),
    dict(target_entropy=float("nan")), dict(target_entropy=float("-inf")), dict(auto_alpha=2), dict(lr=float("inf")), dict(lr=float("nan")),
    dict(beta1=1.0), dict(beta2=-0.1), dict(eps=float("inf")),
    dict(steps=2, batch=3, counts=np.array([0, 3])), dict(steps=2, batch=3, counts=np.array([4, 3])), dict(steps=2, batch=3, counts=np.array([3])),
    dict(steps=2, batch=3, indices=np.array([[0, 1, 2], [3, 300, 5]])), dict(steps=2, batch=3, indices=np.array([[0, -1, 2], [3, 4, 5]])),
    dict(steps=2, batch=3, indices=np.zeros((2, 4), np.int32))],
    ids=lambda kw: "-".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_check_sac_args_refuses_before_the_library_is_touched(monkeypatch, kw):
    from quadsim_amd import sac

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(sac, "load_sac", touched)
    assert sac.check_sac_args(**GOOD) == (300, 100, 10, 0.99, 5e-3, 3e-4, -4.0, 1, 0.9, 0.999, 1e-8, 0)
    assert sac.check_sac_args((1 << 31) - 1, 4096, 256, 0.0, 1.0, 0.0, 0.0, False, 0.0, 0.0, 0.0, (1 << 31) - 4097)[0] == (1 << 31) - 1
    # entries at or beyond counts[s] are never read: they may hold anything
    assert sac.check_sac_args(300, 2, 3, counts=np.array([3, 1]), indices=np.array([[0, 1, 299], [3, -7, 1 << 30]]))[1] == 2
    with pytest.raises(ValueError):
        sac.check_sac_args(**dict(GOOD, **kw))


def test_host_policies_and_bad_arguments_are_refused(monkeypatch, tmp_path):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import sac
    monkeypatch.setattr(sac, "load_sac", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    p = qa.SACPolicy(seed=3, device="cpu")
    rb = qa.ReplayBuffer(32, device="cpu")
    idx = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(qa.QuadsimError):
        qa.sac_update(p, rb, idx)
    with pytest.raises(ValueError):
        qa.torch_sac_update(p, rb, idx + 32)
    with pytest.raises(ValueError):
        qa.torch_sac_update(p, rb, idx.long())
    with pytest.raises(ValueError):
        qa.torch_sac_update(p, rb, idx, noise=torch.zeros((1, 3, 4)))

    class Env:
        num_envs, device = 4, torch.device("cpu")
    with pytest.raises(ValueError, match="update"):
        qa.SAC(p, Env(), update="jax")
    with pytest.raises(ValueError, match="batch"):
        qa.SAC(p, Env(), batch_size=257)
    with pytest.raises(ValueError, match="ent_coef"):
        qa.SAC(p, Env(), ent_coef="fixed")
    with pytest.raises(ValueError, match="target_entropy"):
        qa.SAC(p, Env(), target_entropy="low")
    model = qa.SAC(p, Env())                                           # SB2's defaults
    assert (model.train_freq, model.gradient_steps, model.batch_size, model.learning_starts, model.replay.capacity) == (1, 1, 64, 100, 50000)
    assert model.hyper == dict(gamma=0.99, tau=0.005, lr=3e-4, target_entropy=-4.0, auto_alpha=True) and model.action_noise is None
    assert float(p.alpha_state[0]) == 0.0 and p.alpha == 1.0
    fixed = qa.SAC(qa.SACPolicy(seed=3, device="cpu"), Env(), ent_coef=0.2, target_entropy=-2.0)
    assert fixed.hyper["auto_alpha"] is False and fixed.hyper["target_entropy"] == -2.0 and abs(fixed.policy.alpha - 0.2) < 1e-7
    assert abs(qa.SAC(qa.SACPolicy(seed=3, device="cpu"), Env(), ent_coef="auto_0.5").policy.alpha - 0.5) < 1e-7
    # before learning_starts uniform actions, after them samples of the actor
    obs = torch.randn((4, 12))
    a0 = model.act(obs)
    model.num_timesteps = 100
    a1, a2 = model.act(obs), model.act(obs)
    assert tuple(a0.shape) == tuple(a1.shape) == (4, 4) and float(a1.abs().max()) < 1.0 and not torch.equal(a1, a2)
    # the policy: SB2's initialisation, the cache, save and load
    for name in ONLINE:
        shapes = sr.shapes_of(name)
        tw = getattr(p, "v_target") if name == "v" else [None] * 6
        for k, w, t in zip(KEYS, getattr(p, name), tw):
            assert tuple(w.shape) == shapes[k] and w.dtype == torch.float32
            assert t is None or (torch.equal(w, t) and w.data_ptr() != t.data_ptr())
            lim = 0.0 if len(shapes[k]) == 1 else np.sqrt(6.0 / sum(shapes[k]))
            assert float(w.abs().max()) <= lim and (lim == 0.0 or float(w.abs().max()) > 0.5 * lim)
    assert not torch.equal(p.q1[0], p.q2[0]) and not torch.equal(qa.SACPolicy(seed=4, device="cpu").actor[0], p.actor[0])
    mlp = p.actor_as_mlp()
    assert sorted(mlp) == sorted(KEYS) and mlp["w2"].shape == (128, 4) and mlp["b2"].shape == (4,) and p.actor_as_mlp() is mlp
    x = torch.randn((5, 12)) * 4.0
    a = p.predict(x)
    assert tuple(a.shape) == (5, 4) and float(a.abs().max()) < 1.0 and torch.equal(a, p.predict(x, deterministic=True))
    gen = torch.Generator().manual_seed(5)
    s1 = p.sample(x, gen)
    assert tuple(s1.shape) == (5, 4) and not torch.equal(s1, a) and torch.equal(p.predict(x, deterministic=False, generator=torch.Generator().manual_seed(5)), s1)
    rb.add(torch.randn((32, 12)), torch.rand((32, 4)), torch.randn(32), torch.randn((32, 12)), torch.zeros(32))
    qa.torch_sac_update(p, rb, torch.arange(8, dtype=torch.int32).reshape(2, 4))
    assert p.actor_as_mlp() is not mlp and not np.array_equal(p.actor_as_mlp()["w1"], mlp["w1"])      # dropped after an update
    assert p.steps == 2 and float(p.alpha_state[0]) != 0.0 and float(p.alpha_state[2]) > 0.0
    p.m["q2"][0][15, 0] = 0.5
    path = str(tmp_path / "sac.npz")
    p.save_npz(path)
    q = qa.SACPolicy.from_npz(path, device="cpu")
    assert q.steps == 2 and float(q.m["q2"][0][15, 0]) == 0.5 and torch.equal(q.alpha_state, p.alpha_state)
    assert all(torch.equal(a, b) for x, y in zip(p.nets(), q.nets()) for a, b in zip(x, y))
    la = float(p.alpha_state[0])
    qa.reset_sac_optimizer(p)
    assert p.steps == 0 and not p.m["q2"][0].any() and float(p.alpha_state[0]) == la and not p.alpha_state[1:].any()


# ---------------------------------------------------------------------------------------------------- the census
def test_rows_are_exactly_the_kernels_of_the_code_object_without_scratch(notes):
    # (k_sac_step keeps fourteen scalars in lanes of a vector register: that costs no scratch)
    side_cases.check_census(notes, sac_matrix, lambda n: kernel_notes.instantiations_with_types(n, sac_matrix.KERNELS, namespace="qssac"), "sac",
                            sgpr_spills=("k_sac_step",))


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(sac_matrix)


def test_the_other_ten_libraries_are_instruction_identical():
    """profiles/sac/isa_diff.txt is the output of tools/isa_diff.py, the parent commit's build against this one, for each of the
    other ten libraries (backward_chunk of train_pieces.hpp gained a template parameter whose default is what it was): every kernel
    line says `same`"""
    text = open(os.path.join(ROOT, "profiles", "sac", "isa_diff.txt")).read()
    libs = re.findall(r"^## (\S+)$", text, flags=re.M)
    assert libs == ["libquadsim_hip.so", "libquadsim_dyn.so", "libquadsim_dynmppi.so", "libquadsim_dynfit.so", "libquadsim_bc.so",
                    "libquadsim_ppo.so", "libquadsim_gail.so", "libquadsim_trpo.so", "libquadsim_ddpg.so", "libquadsim_td3.so"]
    lines = [ln for ln in text.splitlines() if re.match(r"^_Z\S+: ", ln)]
    assert len(lines) > 100 and all(ln.endswith(": same") for ln in lines)
    totals = re.findall(r"^identical in fields and disassembly: (\d+) of (\d+)$", text, flags=re.M)
    assert len(totals) == 10 and all(a == b for a, b in totals)
    assert not re.findall(r"only in (?:parent|branch) \[[^\]]+\]", text)


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("count", sr.STEP_COUNTS)
def test_fixtures_lie_off_every_edge(count):
    """on the rows of every step count: no pre-activation of a differentiated pass of the float64 reference within its bound of zero,
    no raw log-std within its bound of -20 or 2 (so NO element is excluded), |u| <= 3, the twin minimum taken both ways from ten rows
    on, terminal and non-terminal rows"""
    P, rp = sr.nets(), sr.replay()
    assert not sr.relu_edges(P, rp, sr.row_noise()).any() and not sr.clamp_edges(P, rp, sr.row_noise()).any()
    assert sr.u_max(P, rp, sr.row_noise()) <= 3.0
    idx, z = sr.step_indices(count), sr.noise(1, count)
    rows = tuple(a[idx[0]] for a in rp)
    assert not sr.relu_edges(P, rows, z[0]).any() and not sr.clamp_edges(P, rows, z[0]).any() and sr.u_max(P, rows, z[0]) <= 3.0
    VT = sr.value_target64(P, rows, z[0], sr.LOG_ALPHA)
    census = {"qa<qb": int((VT["qa"] < VT["qb"]).sum()), "qb<qa": int((VT["qb"] < VT["qa"]).sum()), "terminal": int((rows[4] >= 1.0).sum()),
              "live": int((rows[4] < 1.0).sum())}
    print("sac fixture rows %d: %s" % (count, census))
    if count >= 10:
        assert all(v > 0 for v in census.values()), census
    # the clamped and the saturated fixtures are what they say
    zc = sr.noise_log_std(z[0])
    S = sr.sample64(sr.mlp64(sr.nets_log_std()["actor"], np.asarray(rows[0], np.float64)), zc)
    assert (S["lsr"][:, 0] < -20.0 - S["E_lsr"][:, 0]).all() and (S["lsr"][:, 2] > 2.0 + S["E_lsr"][:, 2]).all()
    assert not sr.clamp_edges(sr.nets_log_std(), rows, zc).any() and sr.u_max(sr.nets_log_std(), rows, zc) <= 3.0
    S = sr.sample64(sr.mlp64(sr.nets_saturated()["actor"], np.asarray(rows[0], np.float64)), z[0])
    a32 = np.tanh(S["u"][:, :2]).astype(np.float32)
    assert (np.abs(S["u"][:, :2]) > 9.5).all() and (np.float32(1.0) - a32 * a32 == 0.0).all()


def _torch64(torch, P, M, V, A, rp, idx, z, dtype="float64", **kw):
    import quadsim_amd as qa
    pol = qa.SACPolicy(device="cpu", weights={n: {k: np.asarray(P[n][k], np.float64) for k in KEYS} for n in NETS}, dtype=dtype)
    for n in ONLINE:
        pol.m[n] = [torch.as_tensor(np.asarray(M[n][k], np.float64).copy()).to(pol.dtype) for k in KEYS]
        pol.v_[n] = [torch.as_tensor(np.asarray(V[n][k], np.float64).copy()).to(pol.dtype) for k in KEYS]
    pol.alpha_state = torch.as_tensor(np.asarray(A, np.float64).copy()).to(pol.dtype)
    out = qa.torch_sac_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), noise=torch.as_tensor(z), return_grads=True,
                              return_trace=True, **kw)
    return pol, out


@pytest.mark.parametrize("count", [1, 17, 256])
def test_step64_against_torch_float64_autograd(count):
    """the eight statistics, all 24 gradients and the gradient of log_alpha to 1e-12 relative against torch_sac_update in float64 on the
    host, which the restatement shares no code with -- and so far inside the bounds of step64; y, vb, logp and the sample likewise"""
    import torch
    P, rp = sr.nets(), sr.replay()
    Z = sr.zero_state()
    idx, z = sr.step_indices(count), sr.noise(1, count)
    stats, G, aux, Es, E = sr.step64(P, tuple(a[idx[0]] for a in rp), z[0], with_bound=True)
    pol, out = _torch64(torch, P, Z, Z, [sr.LOG_ALPHA, 0.0, 0.0], rp, idx, z)
    got = out["stats"][0].numpy()
    assert got.dtype == np.float64 and np.all(np.abs(got - stats) <= 1e-12 * np.maximum(1.0, np.abs(stats))) and np.all(np.abs(got - stats) <= Es)
    for n in ONLINE:
        for i, k in enumerate(KEYS):
            g = out["grads"][n][i].numpy()
            assert g.shape == sr.shapes_of(n)[k] and np.abs(g - G[n][k]).max() <= 1e-12 * max(1.0, np.abs(G[n][k]).max()), (n, k)
            # (the value net regresses on vb, whose bound carries alpha times logp's: looser than the others')
            assert np.all(np.abs(g - G[n][k]) <= E[n][k]) and (n == "v" or E[n][k].max() <= 0.5 * np.abs(G[n][k]).max()), (n, k)
    assert abs(float(out["grads"]["log_alpha"]) - G["log_alpha"]) <= 1e-12 * max(1.0, abs(G["log_alpha"]))
    T = out["trace"]
    for got, want in ((T["logp"][0], aux["logp"]), (T["vlogp"][0], aux["logp"]), (T["fwd"][0, :, 1], aux["y"]), (T["fwd"][0, :, 4], aux["vb"]),
                      (T["act"][0], aux["a"])):
        assert np.abs(got.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.all(Es <= 0.1 * np.maximum(np.abs(stats), 0.1))
    # a wildly different target changes nothing where every row is terminal
    huge = dict(P, v_target={k: np.full_like(P["v_target"][k], 1e30) for k in KEYS})
    term = tuple(a[idx[0]] for a in rp[:4]) + (np.ones(count, np.float32),)
    with np.errstate(over="ignore", invalid="ignore"):
        s2, G2, a2 = sr.step64(huge, term, z[0])
    s1, G1, a1 = sr.step64(P, term, z[0])
    assert np.array_equal(a1["y"], a2["y"]) and np.array_equal(s1, s2) and all(np.array_equal(G1[n][k], G2[n][k]) for n in ONLINE for k in KEYS)


def test_fit64_against_the_torch_loop_with_counts_and_both_temperature_modes():
    """five updates from t0 = 1 with a count per step and non-zero moments, the float64 loop of sac_ref against torch_sac_update in
    float64, with the temperature learned and with it fixed; and the loop is the loop of its parts"""
    import torch
    P, rp = sr.nets(), sr.replay()
    M, V = sr.moments()
    idx = sr.step_indices(8, steps=5)
    z = sr.noise_for(idx)
    counts = np.array([8, 1, 7, 8, 3], np.int32)
    for auto in (True, False):
        kw = dict(lr=1e-2, auto_alpha=auto)
        P5, M5, V5, A5, S5 = sr.fit64(P, M, V, sr.ALPHA_STATE, rp, idx, z, counts, t0=1, **kw)
        Pa, Ma, Va, Aa, Sa = sr.fit64(P, M, V, sr.ALPHA_STATE, rp, idx[:2], z[:2], counts[:2], t0=1, **kw)
        Pb, Mb, Vb, Ab, Sb = sr.fit64(Pa, Ma, Va, Aa, rp, idx[2:], z[2:], counts[2:], t0=3, **kw)
        assert all(np.array_equal(P5[n][k], Pb[n][k]) for n in NETS for k in KEYS) and np.array_equal(S5, np.concatenate([Sa, Sb]))
        assert np.array_equal(A5, Ab) and (np.array_equal(A5, sr.ALPHA_STATE.astype(np.float64)) != auto)
        import quadsim_amd as qa
        pol = qa.SACPolicy(device="cpu", weights={n: {k: np.asarray(P[n][k], np.float64) for k in KEYS} for n in NETS}, dtype="float64")
        for n in ONLINE:
            pol.m[n] = [torch.as_tensor(np.asarray(M[n][k], np.float64).copy()) for k in KEYS]
            pol.v_[n] = [torch.as_tensor(np.asarray(V[n][k], np.float64).copy()) for k in KEYS]
        pol.alpha_state = torch.as_tensor(sr.ALPHA_STATE.astype(np.float64))
        pol.steps = 1
        out = qa.torch_sac_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), torch.as_tensor(counts), noise=torch.as_tensor(z), **kw)
        assert pol.steps == 6 and np.abs(out["stats"].numpy() - S5).max() <= 1e-9
        assert np.abs(pol.alpha_state.numpy() - A5).max() <= 1e-9
        for n in NETS:
            for k, w in zip(KEYS, getattr(pol, n)):
                assert np.abs(w.numpy() - P5[n][k]).max() <= 1e-9 * max(1.0, np.abs(P5[n][k]).max()), (n, k)


@pytest.mark.parametrize("which", ["standard", "log_std_clamped", "saturated"])
def test_bounds_hold_for_torch_float32_in_another_summation_order(which):
    """torch's own float32 autograd of the same step (library GEMMs, another summation order, another tanh, exp and log) stays within
    the derived bounds: they are not so tight that only the device's order meets them.  With the log-std clamped on chosen components
    the reference's gradient into those components of the head is exactly zero"""
    import torch
    P = {"standard": sr.nets, "log_std_clamped": sr.nets_log_std, "saturated": sr.nets_saturated}[which]()
    rp = sr.replay()
    Z = sr.zero_state()
    idx, z = sr.step_indices(33), sr.noise(1, 33)
    if which == "log_std_clamped":
        z = sr.noise_log_std(z)
    la32 = float(np.float32(sr.LOG_ALPHA))
    pol, out = _torch64(torch, P, Z, Z, [la32, 0.0, 0.0], rp, idx, z, dtype="float32")
    stats, G, aux, Es, E = sr.step64(P, tuple(a[idx[0]] for a in rp), z[0], la=la32, with_bound=True)
    err = np.abs(out["stats"][0].double().numpy() - stats)
    assert np.all(err <= Es), (err, Es)
    for n in ONLINE:
        for k, g in zip(KEYS, out["grads"][n]):
            e = np.abs(g.double().numpy() - G[n][k])
            assert np.isfinite(e).all() and np.all(e <= E[n][k]), (n, k, (e / E[n][k]).max())
            assert np.isfinite(E[n][k]).all(), (n, k)                           # the saturated sample included: large, never infinite
    assert abs(float(out["grads"]["log_alpha"]) - G["log_alpha"]) <= E["log_alpha"] and np.isfinite(Es).all() and np.isfinite(E["log_alpha"])
    if which == "saturated":
        # the Jacobian term's bound at a = +-1: 2 |a| E_a / E6 per saturated component with E_a = TANH_ABS + E_u^2, of order one
        S = aux["S"]
        assert (S["E_J"][:, :2] > 2.0 * sr.TANH_ABS / sr.E6).all() and (S["E_J"][:, :2] < 4.0).all() and (S["E_J"][:, 2:] < 1e-2).all()
        assert np.isfinite(aux["E_logp"]).all() and aux["E_logp"].max() < 8.0
    if which == "log_std_clamped":
        assert not aux["dlsr"][:, [0, 2]].any() and aux["dlsr"][:, [1, 3]].all()
        assert not G["actor"]["w2"][:, [4, 6]].any() and not G["actor"]["b2"][[4, 6]].any() and not E["actor"]["b2"][[4, 6]].max() > 1e-30
        assert not out["grads"]["actor"][4][:, [4, 6]].any() and out["grads"]["actor"][4][:, [5, 7]].any()
    assert pol.steps == 1 and not torch.equal(pol.v_target[2], torch.as_tensor(P["v_target"]["w1"]))


def test_keyed_noise_of_the_host_path_is_the_references():
    """the normals that torch_sac_update draws without `noise` are float64 Box-Muller on the Philox words of (seed, update, slot) of
    stream 7, rounded to float32; tests/test_gpu_sac.py holds the device's noise_out to the same float64 values"""
    from quadsim_amd import sac, td3
    z = sac.keyed_noise(77, 4, 3, 33)
    want = sr.normals64(77, 4, 3, 33)
    assert z.dtype == np.float32 and z.shape == (3, 33, 4) and np.array_equal(z, want.astype(np.float32))
    assert np.array_equal(sac.keyed_noise(77, 5, 2, 10), z[1:, :10]) and not np.array_equal(td3.keyed_noise(77, 4, 3, 33), z)


def test_the_regression_case_is_learnt_in_float64():
    """the condition tests/test_gpu_sac.py holds the device to, met by the float64 reference with room: for either critic the mean
    loss of the last 20 of 200 updates is below a QUARTER of that of the first 20 (the device has to reach half)"""
    P, rp, idx, z = sr.learn_case()
    Z = sr.zero_state()
    st = sr.fit64(P, Z, Z, [0.0, 0.0, 0.0], rp, idx, z, lr=sr.LEARN_LR)[4]
    for c in (0, 1):
        first, last = st[:20, c].mean(), st[-20:, c].mean()
        print("sac learn float64: q%d loss first 20 %.4g, last 20 %.4g" % (c + 1, first, last))
        assert last < 0.25 * first
