"""-m "not gpu": everything of DDPG on the device that needs no device.  include/quadsim_ddpg.h is plain C99 and every symbol it
declares is exported by libquadsim_ddpg.so; the table entry of _lib.SIDE matches the header's prototypes; every refusal the
header promises happens before anything is launched, and check_ddpg_args mirrors it; tests/ddpg_matrix.py has exactly one row per
kernel of the new code object, none uses scratch and each fits the compute unit's LDS; tests/ddpg_ref.py is checked against torch's
float64 autograd, which it shares no code with; the float64 reference meets the learning condition the device is held to; the
schedule, the noise and the ring hold their properties; and the recorded instruction diff of the other seven libraries says `same`
for every kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddpg_matrix
import ddpg_ref as dd
import kernel_notes
import side_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = dd.KEYS


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, ddpg
    _lib.build_library()
    return ddpg.load_ddpg()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("ddpg", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    side_cases.check_exports("ddpg", lib, ["qsdd_last_error", "qsdd_update", "qsdd_version", "qsdd_workspace_bytes"])


def test_table_entry_names_its_own_files():
    import quadsim_amd as qa
    from quadsim_amd import _lib, ddpg
    assert ddpg.DDPG_EXPORTS is _lib.SIDE["ddpg"]["exports"]
    side_cases.check_entry("ddpg", ["ddpg_kernels.hpp", "quadsim_ddpg.h", "quadsim_device.hpp", "side_host.hpp", "side_offpolicy.hpp",
                                     "train_offpolicy.hpp", "train_pieces.hpp"], "ddpg.hip")
    for name in ("DDPG", "DDPGPolicy", "ReplayBuffer", "OUNoise", "replay_schedule", "ddpg_update", "torch_ddpg_update", "check_ddpg_args"):
        assert getattr(qa, name) is getattr(ddpg, name) and name in qa.__all__
    assert ddpg.DDPG_MAX_STEPS == 4096 and ddpg.DDPG_MAX_BATCH == 256


def test_no_other_library_holds_its_kernels(lib):
    from quadsim_amd import _lib
    side_cases.check_no_foreign_kernels("ddpg")
    assert b"k_ddpg_step" in open(_lib.SIDE["ddpg"]["path"], "rb").read()


def test_table_entry_matches_the_header(lib):
    """the structs and the workspace; the prototypes are held by tests/test_call_path_cpu.py, for every side library"""
    from quadsim_amd import _lib
    # the structs: two 32-bit fields, then 48 tensors; n and five tensors; eight doubles
    assert C.sizeof(_lib.QsddNets) == 8 + 48 * 8 and _lib.QsddNets.m.offset == 8 + 24 * 8 and _lib.QsddNets.v.offset == 8 + 36 * 8
    assert C.sizeof(_lib.QsddReplay) == 16 + 5 * 8 and C.sizeof(_lib.QsddHyper) == 8 + 8 * 8
    # the workspace: two buffers of four nets (each padded to four floats), and m, v and the gradients of the two online nets
    actor, critic = 12 * 128 + 128 + 128 * 128 + 128 + 128 * 4 + 4, 12 * 128 + 128 + 132 * 128 + 128 + 128 + 1
    online = actor + ((critic + 3) & ~3)
    nbytes = C.c_size_t(0)
    assert lib.qsdd_workspace_bytes(C.byref(nbytes)) == 0 and nbytes.value == 4 * (2 * 2 * online + 3 * online)
    assert lib.qsdd_workspace_bytes(None) == 1 and b"bytes" in lib.qsdd_last_error()


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_ddpg.h"

static float x[8192], y[20000], big[1200000];
static float ws_store[300000];
static int32_t idx[64];
static QsddNets nets;
static QsddReplay rp;
static QsddHyper hp;
static float *grads[12];
static size_t ws_bytes;

static int refused(int rc, const char *word)
{
    if (rc == QSDD_OK || strstr(qsdd_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qsdd_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int upd(int steps, int batch, int64_t t0)
{
    return qsdd_update(&nets, &rp, idx, NULL, steps, batch, &hp, t0, ws_store, ws_bytes, y, NULL, NULL);
}

static void good(void)
{
    /* 48 tensors that do not overlap: 20000 floats apart in `big` */
    int k, i;
    for (k = 0; k < 4; ++k) for (i = 0; i < 6; ++i) nets.w[k][i] = big + 20000 * (6 * k + i);
    for (k = 0; k < 2; ++k) for (i = 0; i < 6; ++i) { nets.m[k][i] = big + 20000 * (24 + 6 * k + i); nets.v[k][i] = big + 20000 * (36 + 6 * k + i); }
    for (i = 0; i < 12; ++i) grads[i] = big + 20000 * (48 + i);
    nets.struct_size = sizeof nets;
    rp.struct_size = sizeof rp; rp.n = 300; rp.obs0 = rp.act = rp.rew = rp.obs1 = rp.done = x;
    hp.struct_size = sizeof hp; hp.gamma = 0.99; hp.tau = 1e-3; hp.actor_lr = 1e-4; hp.critic_lr = 1e-3; hp.obs_clip = 5.0;
    hp.beta1 = 0.9; hp.beta2 = 0.999; hp.eps = 1e-8;
}

int main(void)
{
    int ok = 1;
    void *fns[] = {(void *)qsdd_version, (void *)qsdd_last_error, (void *)qsdd_workspace_bytes, (void *)qsdd_update};
    if (qsdd_version() != QSDD_VERSION) return 2;
    if (qsdd_workspace_bytes(&ws_bytes) != QSDD_OK || ws_bytes > sizeof ws_store) return 3;
    good();
    ok &= refused(upd(100, 0, 0), "batch");
    ok &= refused(upd(100, 257, 0), "batch");
    ok &= refused(upd(0, 10, 0), "steps");
    ok &= refused(upd(4097, 10, 0), "steps");
    rp.n = 0; ok &= refused(upd(100, 10, 0), "n must"); good();
    rp.n = (int64_t)1 << 31; ok &= refused(upd(100, 10, 0), "n must"); good();
    ok &= refused(upd(100, 10, -1), "t0");
    ok &= refused(upd(100, 10, ((int64_t)1 << 31) - 50), "t0");
    hp.gamma = -0.1; ok &= refused(upd(100, 10, 0), "gamma"); good();
    hp.gamma = 1.5; ok &= refused(upd(100, 10, 0), "gamma"); good();
    hp.gamma = NAN; ok &= refused(upd(100, 10, 0), "gamma"); good();
    hp.tau = 0.0; ok &= refused(upd(100, 10, 0), "tau"); good();
    hp.tau = 1.5; ok &= refused(upd(100, 10, 0), "tau"); good();
    hp.tau = NAN; ok &= refused(upd(100, 10, 0), "tau"); good();
    hp.obs_clip = 0.0; ok &= refused(upd(100, 10, 0), "obs_clip"); good();
    hp.obs_clip = -5.0; ok &= refused(upd(100, 10, 0), "obs_clip"); good();
    hp.obs_clip = NAN; ok &= refused(upd(100, 10, 0), "obs_clip"); good();
    hp.actor_lr = INFINITY; ok &= refused(upd(100, 10, 0), "actor_lr"); good();
    hp.actor_lr = NAN; ok &= refused(upd(100, 10, 0), "actor_lr"); good();
    hp.critic_lr = INFINITY; ok &= refused(upd(100, 10, 0), "critic_lr"); good();
    hp.critic_lr = NAN; ok &= refused(upd(100, 10, 0), "critic_lr"); good();
    hp.beta1 = 1.0; ok &= refused(upd(100, 10, 0), "beta1"); good();
    hp.beta2 = -0.1; ok &= refused(upd(100, 10, 0), "beta2"); good();
    hp.eps = INFINITY; ok &= refused(upd(100, 10, 0), "eps"); good();
    /* two tensors one float short of disjoint, stats inside a moment, a gradient on a target weight, the workspace on a net */
    nets.m[1][2] = nets.w[3][2] + 132 * 128 - 1; ok &= refused(upd(100, 10, 0), "overlap"); good();
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, nets.v[0][0] + 8, NULL, NULL), "overlap");
    grads[7] = nets.w[2][4]; ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, y, grads, NULL), "overlap"); good();
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, big, ws_bytes, y, NULL, NULL), "overlap");
    nets.w[2][3] = NULL; ok &= refused(upd(100, 10, 0), "NULL"); good();
    nets.v[1][5] = (float *)((char *)nets.v[1][5] + 2); ok &= refused(upd(100, 10, 0), "aligned"); good();
    rp.done = NULL; ok &= refused(upd(100, 10, 0), "NULL"); good();
    grads[11] = NULL; ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, y, grads, NULL), "NULL"); good();
    nets.struct_size = 8; ok &= refused(upd(100, 10, 0), "QsddNets.struct_size"); good();
    rp.struct_size = 8; ok &= refused(upd(100, 10, 0), "QsddReplay.struct_size"); good();
    hp.struct_size = 8; ok &= refused(upd(100, 10, 0), "QsddHyper.struct_size"); good();
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes - 1, y, NULL, NULL), "workspace");
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, (char *)ws_store + 4, ws_bytes, y, NULL, NULL), "aligned");
    ok &= refused(qsdd_update(NULL, &rp, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qsdd_update(&nets, NULL, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qsdd_update(&nets, &rp, NULL, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, NULL, 0, ws_store, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, NULL, ws_bytes, y, NULL, NULL), "NULL");
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, NULL, NULL, NULL), "NULL");
    ok &= refused(qsdd_update(&nets, &rp, idx, NULL, 100, 10, &hp, 0, ws_store, ws_bytes, (float *)((char *)y + 2), NULL, NULL), "aligned");
    ok &= refused(qsdd_workspace_bytes(NULL), "bytes");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    side_cases.run_c_caller("ddpg", C_CALLER, tmp_path)


GOOD = dict(n=300, steps=100, batch=10, gamma=0.99, tau=1e-3, actor_lr=1e-4, critic_lr=1e-3, obs_clip=5.0, beta1=0.9, beta2=0.999, eps=1e-8,
            t0=0)


@pytest.mark.parametrize("kw", [
    dict(batch=0), dict(batch=257), dict(steps=0), dict(steps=4097), dict(n=0), dict(n=1 << 31), dict(t0=-1), dict(t0=(1 << 31) - 50),
    dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(tau=0.0), dict(tau=1.5), dict(tau=float("nan")),
    dict(obs_clip=0.0), dict(obs_clip=-5.0), dict(obs_clip=float("nan")), dict(actor_lr=float("inf")), dict(actor_lr=float("nan")),
    dict(critic_lr=float("inf")), dict(critic_lr=float("nan")), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=float("inf")),
    dict(steps=2, batch=3, counts=np.array([0, 3])), dict(steps=2, batch=3, counts=np.array([4, 3])), dict(steps=2, batch=3, counts=np.array([3])),
    dict(steps=2, batch=3, indices=np.array([[0, 1, 2], [3, 300, 5]])), dict(steps=2, batch=3, indices=np.array([[0, -1, 2], [3, 4, 5]])),
    dict(steps=2, batch=3, indices=np.zeros((2, 4), np.int32))],
    ids=lambda kw: "-".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_check_ddpg_args_refuses_before_the_library_is_touched(monkeypatch, kw):
    from quadsim_amd import ddpg

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(ddpg, "load_ddpg", touched)
    assert ddpg.check_ddpg_args(**GOOD) == (300, 100, 10, 0.99, 1e-3, 1e-4, 1e-3, 5.0, 0.9, 0.999, 1e-8, 0)
    assert ddpg.check_ddpg_args((1 << 31) - 1, 4096, 256, 0.0, 1.0, 0.0, 0.0, float("inf"), 0.0, 0.0, 0.0, (1 << 31) - 4097)[0] == (1 << 31) - 1
    # entries at or beyond counts[s] are never read: they may hold anything
    assert ddpg.check_ddpg_args(300, 2, 3, counts=np.array([3, 1]), indices=np.array([[0, 1, 299], [3, -7, 1 << 30]]))[1] == 2
    with pytest.raises(ValueError):
        ddpg.check_ddpg_args(**dict(GOOD, **kw))


def test_host_policies_and_bad_arguments_are_refused(monkeypatch):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import ddpg
    monkeypatch.setattr(ddpg, "load_ddpg", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    p = qa.DDPGPolicy(device="cpu")
    rb = qa.ReplayBuffer(32, device="cpu")
    idx = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(qa.QuadsimError):
        qa.ddpg_update(p, rb, idx)
    with pytest.raises(ValueError):
        qa.torch_ddpg_update(p, rb, idx + 32)
    with pytest.raises(ValueError):
        qa.torch_ddpg_update(p, rb, idx.long())

    class Env:
        num_envs, device = 4, torch.device("cpu")
    with pytest.raises(ValueError, match="update"):
        qa.DDPG(p, Env(), update="jax")
    with pytest.raises(ValueError, match="batch"):
        qa.DDPG(p, Env(), batch_size=257)
    with pytest.raises(ValueError, match="random_exploration"):
        qa.DDPG(p, Env(), random_exploration=1.5)


# ---------------------------------------------------------------------------------------------------- the census
def test_rows_are_exactly_the_kernels_of_the_code_object_without_scratch(notes):
    side_cases.check_census(notes, ddpg_matrix, lambda n: kernel_notes.instantiations_with_types(n, ddpg_matrix.KERNELS, namespace="qsdd"), "ddpg")


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(ddpg_matrix)


def test_the_other_seven_libraries_are_instruction_identical():
    """profiles/ddpg/isa_diff.txt is the output of tools/isa_diff.py, the parent commit's build against this one, for each of
    the other seven libraries: every kernel line says `same`.  None of them can have moved: no file they are built from belongs to
    this library (held above)"""
    text = open(os.path.join(ROOT, "profiles", "ddpg", "isa_diff.txt")).read()
    libs = re.findall(r"^## (\S+)$", text, flags=re.M)
    assert libs == ["libquadsim_hip.so", "libquadsim_dyn.so", "libquadsim_dynmppi.so", "libquadsim_dynfit.so", "libquadsim_bc.so",
                    "libquadsim_ppo.so", "libquadsim_gail.so"]
    lines = [ln for ln in text.splitlines() if re.match(r"^_Z\S+: ", ln)]
    assert len(lines) > 100 and all(ln.endswith(": same") for ln in lines)
    totals = re.findall(r"^identical in fields and disassembly: (\d+) of (\d+)$", text, flags=re.M)
    assert len(totals) == 7 and all(a == b for a, b in totals)
    assert not re.findall(r"only in (?:parent|branch) \[[^\]]+\]", text)


# ---------------------------------------------------------------------------------------------------- the reference itself
def _torch_nets(torch, P):
    return {n: [torch.tensor(np.asarray(P[n][k], np.float64), requires_grad=True) for k in KEYS] for n in dd.NETS}


def _t_actor(torch, w, o):
    return torch.tanh(torch.relu(torch.relu(o @ w[0] + w[1]) @ w[2] + w[3]) @ w[4] + w[5])


def _t_critic(torch, w, o, a):
    return (torch.relu(torch.cat([torch.relu(o @ w[0] + w[1]), a], 1) @ w[2] + w[3]) @ w[4] + w[5])[:, 0]


@pytest.mark.parametrize("count", [1, 17, 256])
def test_step64_against_torch_float64_autograd(count):
    """y, both losses, the two means and all twelve gradients to 1e-10 relative, against code the restatement does not share.
    The actor term gives the critic no gradient; a terminal row ignores q1"""
    import torch
    P = dd.nets()
    rp = dd.replay()
    rows = tuple(a[dd.step_indices(count)[0]] for a in rp)
    stats, G, y = dd.step64(P, rows)
    T = _torch_nets(torch, P)
    o0, act, rew, o1, done = (torch.tensor(np.asarray(a, np.float64)) for a in rows)
    o0c, o1c = o0.clamp(-5.0, 5.0), o1.clamp(-5.0, 5.0)
    assert not torch.equal(o0, o0c) or count == 1                     # the clamp acts
    q1 = _t_critic(torch, T["critic_target"], o1c, _t_actor(torch, T["actor_target"], o1c)).detach()
    ty = rew + (1.0 - done) * 0.99 * q1
    q = _t_critic(torch, T["critic"], o0c, act)
    closs = ((q - ty) ** 2).mean()
    aloss = -_t_critic(torch, T["critic"], o0c, _t_actor(torch, T["actor"], o0c)).mean()
    g_c = torch.autograd.grad(closs, T["critic"], retain_graph=True)
    g_a = torch.autograd.grad(aloss, T["actor"], retain_graph=True)
    g_ca = torch.autograd.grad(aloss, T["critic"])                     # what the actor term WOULD give the critic
    rel = lambda got, want: np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max())      # noqa: E731
    assert rel(y, ty.numpy())
    assert np.array_equal(y[np.asarray(rows[4]) == 1.0], np.asarray(rows[2], np.float64)[np.asarray(rows[4]) == 1.0])
    for got, want in zip(stats, (closs, aloss, q.mean(), ty.mean())):
        assert abs(got - float(want.detach())) <= 1e-10 * max(1.0, abs(float(want.detach())))
    for i, k in enumerate(KEYS):
        assert G["critic"][k].shape == dd.CRITIC_SHAPES[k] and G["actor"][k].shape == dd.ACTOR_SHAPES[k]
        assert rel(G["critic"][k], g_c[i].numpy()), k
        assert rel(G["actor"][k], g_a[i].numpy()), k
    assert any(float(g.abs().max()) > 1e-6 for g in g_ca[2:]) and not rel(G["critic"]["w2"], (g_c[4] + g_ca[4]).numpy())
    # wildly different targets change nothing where every row is terminal
    huge = dict(P, critic_target={k: np.full_like(P["critic_target"][k], 1e30) for k in KEYS})
    term = rows[:4] + (np.ones_like(rows[4]),)
    with np.errstate(over="ignore", invalid="ignore"):
        s2, G2, y2 = dd.step64(huge, term)
    s1, G1, y1 = dd.step64(P, term)
    assert np.array_equal(y1, y2) and np.array_equal(s1, s2) and all(np.array_equal(G1[n][k], G2[n][k]) for n in G1 for k in KEYS)


def test_fit64_is_the_loop_of_its_parts_with_counts_and_polyak32_is_the_average():
    P, rp = dd.nets(), dd.replay()
    Z = dd.zero_state()
    idx = dd.step_indices(8, steps=3)
    counts = np.array([8, 1, 7])
    P3, M3, V3, S3 = dd.fit64(P, Z, Z, rp, idx, counts, critic_lr=1e-2)
    Pa, Ma, Va, Sa = dd.fit64(P, Z, Z, rp, idx[:2], counts[:2], critic_lr=1e-2)
    Pb, Mb, Vb, Sb = dd.fit64(Pa, Ma, Va, rp, idx[2:], counts[2:], t0=2, critic_lr=1e-2)
    assert all(np.array_equal(P3[n][k], Pb[n][k]) for n in dd.NETS for k in KEYS)
    assert all(np.array_equal(V3[n][k], Vb[n][k]) for n in V3 for k in KEYS)
    assert np.array_equal(S3, np.concatenate([Sa, Sb])) and np.all(np.isfinite(S3))
    assert not np.array_equal(P3["actor_target"]["w1"], P["actor_target"]["w1"])
    t, w = P["critic_target"]["w1"], P["critic"]["w1"]
    got = dd.polyak32(t, w, 1e-3)
    assert got.dtype == np.float32 and np.abs(got.astype(np.float64) - (0.999 * t.astype(np.float64) + 1e-3 * w)).max() < 3e-7
    assert np.array_equal(dd.polyak32(t, w, 1.0), w) and np.array_equal(dd.polyak32(np.full_like(t, 1e30), w, 1.0), w)


def test_the_regression_case_is_learnt_in_float64():
    """the condition tests/test_gpu_ddpg.py holds the device to, met by the float64 reference with room: the mean critic loss of
    the last 20 of 200 steps is below a QUARTER of that of the first 20 (the device has to reach half)"""
    P, rp, idx = dd.learn_case()
    Z = dd.zero_state()
    st = dd.fit64(P, Z, Z, rp, idx, critic_lr=dd.LEARN_CRITIC_LR, actor_lr=dd.LEARN_ACTOR_LR)[3]
    first, last = st[:20, 0].mean(), st[-20:, 0].mean()
    print("ddpg learn float64: critic loss first 20 %.4g, last 20 %.4g" % (first, last))
    assert last < 0.25 * first


def test_bounds_hold_for_torch_float32_in_another_summation_order():
    """torch's own float32 autograd of the same step (library GEMMs, another summation order, another tanh) stays within the
    derived bounds, and the bounds bound something: they are not empty, and not so tight that only the device's order meets them"""
    import torch
    import quadsim_amd as qa
    P, rp = dd.nets(), dd.replay()
    idx = dd.step_indices(33)
    pol = qa.DDPGPolicy(device="cpu", weights=P)
    out = qa.torch_ddpg_update(pol, tuple(torch.as_tensor(a) for a in rp), torch.as_tensor(idx), return_grads=True)
    stats, G, y, Es, E = dd.step64(P, tuple(a[idx[0]] for a in rp), with_bound=True)
    err = np.abs(out["stats"][0].double().numpy() - stats)
    assert np.all(err <= Es), (err, Es)
    assert np.all(Es <= 0.05 * np.maximum(np.abs(stats), 0.1))            # worst-case chains of 128 and 132 terms, three layers deep
    for n in ("actor", "critic"):
        for k, g in zip(KEYS, out["grads"][n]):
            e = np.abs(g.double().numpy() - G[n][k])
            assert np.all(e <= E[n][k]), (n, k, (e / E[n][k]).max())
            assert E[n][k].max() <= 0.5 * np.abs(G[n][k]).max(), (n, k)   # (a ReLU within its forward bound of zero costs its whole term)
    assert pol.steps == 1 and not torch.equal(pol.critic_target[2], torch.as_tensor(P["critic_target"]["w1"]))


# ---------------------------------------------------------------------------------------------------- the schedule, the noise, the ring
def test_replay_schedule():
    import torch
    from quadsim_amd import replay_schedule
    gen = lambda s: torch.Generator().manual_seed(s)     # noqa: E731
    for size, steps, batch in ((50, 100, 10), (1, 3, 4), (50000, 7, 256)):
        idx = replay_schedule(size, steps, batch, gen(3))
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (steps, batch) and idx.device.type == "cpu" and idx.is_contiguous()
        assert int(idx.min()) >= 0 and int(idx.max()) < size
        assert torch.equal(idx, replay_schedule(size, steps, batch, gen(3)))
        assert size == 1 or not torch.equal(idx, replay_schedule(size, steps, batch, gen(4)))
    idx = replay_schedule(50, 100, 10, gen(3))
    assert len(set(idx.reshape(-1).tolist())) == 50                   # uniform over the whole ring ...
    assert any(len(set(r.tolist())) < 10 for r in idx)                # ... with replacement
    with pytest.raises(ValueError):
        replay_schedule(0, 1, 1, gen(0))


def test_ou_noise_reverts_to_the_mean_and_resets_where_done():
    import torch
    from quadsim_amd import OUNoise
    ou = OUNoise(4096, sigma=0.5, theta=0.15, dt=1e-2, device="cpu", seed=1)
    assert tuple(ou.x.shape) == (4096, 4) and not ou.x.any()
    x1 = ou().clone()
    assert abs(float(x1.std()) - 0.05) < 0.003                        # one step from zero: sigma sqrt(dt)
    # mean reversion: with sigma = 0 the state decays by (1 - theta dt) per step
    calm = OUNoise(3, sigma=0.0, theta=0.15, dt=1e-2, device="cpu")
    calm.x = torch.ones((3, 4))
    for _ in range(10):
        calm()
    np.testing.assert_allclose(calm.x.numpy(), (1.0 - 0.15e-2) ** 10, rtol=1e-6)
    for _ in range(50):
        ou()
    before = ou.x.clone()
    done = torch.zeros(4096, dtype=torch.bool)
    done[::3] = True
    ou.reset(done)
    assert not ou.x[::3].any() and torch.equal(ou.x[1::3], before[1::3]) and torch.equal(ou.x[2::3], before[2::3])
    again = OUNoise(4096, device="cpu", seed=1)
    assert torch.equal(again(), x1)
    ou.reset()
    assert not ou.x.any()


def test_replay_buffer_wraps_in_order(tmp_path):
    import torch
    import quadsim_amd as qa
    rb = qa.ReplayBuffer(10, device="cpu")
    mk = lambda lo, n: (torch.arange(lo, lo + n, dtype=torch.float32)[:, None].repeat(1, 12), torch.arange(lo, lo + n, dtype=torch.float32)[:, None].repeat(1, 4),   # noqa: E731,E501
                        torch.arange(lo, lo + n, dtype=torch.float32), -torch.arange(lo, lo + n, dtype=torch.float32)[:, None].repeat(1, 12),
                        torch.arange(lo, lo + n) % 2 == 0)
    rb.add(*mk(0, 4))
    assert (rb.size, rb.pos) == (4, 4) and rb.rew[:4].tolist() == [0, 1, 2, 3] and rb.done[:4].tolist() == [1, 0, 1, 0]
    rb.add(*mk(4, 4))
    rb.add(*mk(8, 4))                                                  # rows 8, 9, then 0, 1 again
    assert (rb.size, rb.pos) == (10, 2) and rb.rew.tolist() == [10, 11, 2, 3, 4, 5, 6, 7, 8, 9]
    assert rb.obs0[:, 5].tolist() == rb.rew.tolist() and rb.obs1[:, 0].tolist() == [-v for v in rb.rew.tolist()] and rb.act[:, 3].tolist() == rb.rew.tolist()
    assert rb.done.dtype == torch.float32 and rb.done.tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    with pytest.raises(ValueError):
        rb.add(*mk(0, 11))
    # the policy: SB2's initialisation, save and load
    p = qa.DDPGPolicy(seed=3, device="cpu")
    for name in ("actor", "critic"):
        shapes = dd.shapes_of(name)
        for k, w, tw in zip(KEYS, getattr(p, name), getattr(p, name + "_target")):
            assert tuple(w.shape) == shapes[k] and w.dtype == torch.float32 and torch.equal(w, tw) and w.data_ptr() != tw.data_ptr()
            lim = 0.0 if len(shapes[k]) == 1 else 3e-3 if k == "w2" else np.sqrt(6.0 / sum(shapes[k]))
            assert float(w.abs().max()) <= lim and (lim == 0.0 or float(w.abs().max()) > 0.5 * lim)
    assert not torch.equal(qa.DDPGPolicy(seed=4, device="cpu").actor[0], p.actor[0])
    assert sorted(p.actor_weights()) == sorted(KEYS) and p.actor_weights()["w1"].shape == (128, 128)
    obs = torch.randn((5, 12)) * 4.0
    a = p.predict(obs)
    assert tuple(a.shape) == (5, 4) and float(a.abs().max()) < 1.0 and torch.equal(a, p.predict(obs.clamp(-5.0, 5.0)))
    p.steps, p.m["critic"][2][131, 0] = 7, 0.5
    path = str(tmp_path / "ddpg.npz")
    p.save_npz(path)
    q = qa.DDPGPolicy.from_npz(path, device="cpu")
    assert q.steps == 7 and float(q.m["critic"][2][131, 0]) == 0.5
    assert all(torch.equal(a, b) for x, y in zip(p.nets(), q.nets()) for a, b in zip(x, y))
    p.reset_optimizer()
    assert p.steps == 0 and not p.m["critic"][2].any()
