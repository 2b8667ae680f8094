"""-m "not gpu": everything of TRPO on the device that needs no device.  include/quadsim_trpo.h is plain C99 and every symbol it
declares is exported by libquadsim_trpo.so; the table entry of _lib.SIDE matches the header's prototypes; every refusal the header
promises happens before anything is launched, and check_trpo_args mirrors it; tests/trpo_matrix.py has exactly one row per kernel
of the new code object, none uses scratch or spills a vector register and each fits the compute unit's LDS; tests/trpo_ref.py is
checked against torch's float64 autograd, which it shares no code with (the Fisher-vector product against double backprop of the
mean KL); the replay's fma rounds float32 ties once; vf_schedule holds its properties; and the census of the line-search fixtures:
every decision of the float64 reference sits more than ten bounds from its threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kernel_notes
import ppo2_ref as pr
import side_cases
import trpo_matrix
import trpo_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, trpo
    _lib.build_library()
    return trpo.load_trpo()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("trpo", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    side_cases.check_exports("trpo", lib, ["qst_auto_slices", "qst_last_error", "qst_policy_step", "qst_version", "qst_vf_fit", "qst_workspace_bytes"])


def test_table_entry_names_its_own_files():
    import quadsim_amd as qa
    from quadsim_amd import _lib, trpo
    assert trpo.TRPO_EXPORTS is _lib.SIDE["trpo"]["exports"]
    side_cases.check_entry("trpo", ["quadsim_device.hpp", "quadsim_trpo.h", "side_host.hpp", "train_pieces.hpp", "trpo_kernels.hpp"], "trpo.hip")
    for name in ("TRPO", "check_trpo_args", "vf_schedule", "trpo_policy_step", "trpo_vf_fit", "reset_trpo_optimizer", "torch_trpo_policy_step",
                 "torch_trpo_vf_fit"):
        assert getattr(qa, name) is getattr(trpo, name) and name in qa.__all__
    assert trpo.TRPO_PARAMS == tr.P == 18696 and trpo.STAT_NAMES == tr.STAT_NAMES


def test_no_other_library_holds_its_kernels(lib):
    from quadsim_amd import _lib
    side_cases.check_no_foreign_kernels("trpo")
    assert b"k_trpo_fvp" in open(_lib.SIDE["trpo"]["path"], "rb").read()


def test_table_entry_matches_the_header(lib):
    """the structs, the workspace and the slices; the prototypes are held by tests/test_call_path_cpu.py, for every side library"""
    from quadsim_amd import _lib
    assert C.sizeof(_lib.QstNet) == 8 + 39 * 8 and C.sizeof(_lib.QstBatch) == 16 + 4 * 8 and C.sizeof(_lib.QstHyper) == 16 + 4 * 8
    assert C.sizeof(_lib.QstTrace) == 8 + 6 * 8
    # the workspace: 4 + 2 slices doubles, 4 ints, 4 floats, seven vectors, the old means and neglogp, the slices' partials
    nbytes = C.c_size_t(0)
    assert lib.qst_workspace_bytes(300, 7, C.byref(nbytes)) == 0 and nbytes.value == 8 * (4 + 14) + 16 + 16 + 4 * (7 * tr.P + 5 * 300 + 7 * tr.P)
    assert lib.qst_workspace_bytes(1024, 0, C.byref(nbytes)) == 0 and nbytes.value == 8 * (4 + 128) + 32 + 4 * (7 * tr.P + 5 * 1024 + 64 * tr.P)
    assert lib.qst_auto_slices(1024) == 64 and lib.qst_auto_slices(65536 * 32) == 128 and lib.qst_auto_slices(1) == 1 and lib.qst_auto_slices(0) == 0
    assert lib.qst_workspace_bytes(300, 7, None) == 1 and b"bytes" in lib.qst_last_error()


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_trpo.h"

static float x[8192], y[64], big[40 * 20000], tr_f[4 * 11 * 18696];
static double ws_store[400000], cg[64];
static int32_t idx[4096];
static QstNet net;
static QstBatch bat;
static QstHyper hp;
static QstTrace trace;
static float *grads[6];
static size_t ws_bytes;

static int refused(int rc, const char *word)
{
    if (rc == QST_OK || strstr(qst_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qst_last_error()); return 0; }
    return 1;
}

static void good(void)
{
    int k;
    for (k = 0; k < 13; ++k) { net.w[k] = big + 20000 * k; net.m[k] = big + 20000 * (13 + k); net.v[k] = big + 20000 * (26 + k); }
    for (k = 0; k < 6; ++k) grads[k] = tr_f + 20000 * k;
    net.struct_size = sizeof net; net.layout = QST_NET_TOWERS;
    bat.struct_size = sizeof bat; bat.n = 300; bat.obs = bat.actions = bat.returns = bat.values = x;
    hp.struct_size = sizeof hp; hp.cg_iters = 10; hp.backtracks = 10; hp.fvp_stride = 5;
    hp.max_kl = 0.01; hp.cg_damping = 0.01; hp.entcoeff = 0.0; hp.residual_tol = 1e-10;
    trace.struct_size = sizeof trace; trace.fvp_in = tr_f; trace.fvp_out = tr_f + 11 * 18696; trace.cg = cg;
    trace.x = tr_f + 22 * 18696; trace.fullstep = tr_f + 23 * 18696; trace.ls = tr_f + 24 * 18696;
}

static int step(void) { return qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, y, NULL, NULL, NULL); }
static int fit(int steps, int batch, int64_t t0) { return qst_vf_fit(&net, x, x, 300, idx, steps, batch, 3e-4, 0.9, 0.999, 1e-8, t0, y, NULL, NULL); }

int main(void)
{
    int ok = 1;
    void *fns[] = {(void *)qst_version, (void *)qst_last_error, (void *)qst_auto_slices, (void *)qst_workspace_bytes, (void *)qst_policy_step,
                   (void *)qst_vf_fit};
    if (qst_version() != QST_VERSION) return 2;
    if (qst_workspace_bytes(300, 7, &ws_bytes) != QST_OK || ws_bytes > sizeof ws_store) return 3;
    good();
    bat.n = 0; ok &= refused(step(), "n must"); good();
    bat.n = (int64_t)1 << 31; ok &= refused(step(), "n must"); good();
    ok &= refused(qst_policy_step(&net, &bat, -1, &hp, ws_store, ws_bytes, y, NULL, NULL, NULL), "slices");
    ok &= refused(qst_policy_step(&net, &bat, 1025, &hp, ws_store, ws_bytes, y, NULL, NULL, NULL), "slices");
    hp.cg_iters = 0; ok &= refused(step(), "cg_iters"); good();
    hp.cg_iters = 65; ok &= refused(step(), "cg_iters"); good();
    hp.backtracks = 0; ok &= refused(step(), "backtracks"); good();
    hp.backtracks = 33; ok &= refused(step(), "backtracks"); good();
    hp.fvp_stride = 0; ok &= refused(step(), "fvp_stride"); good();
    hp.max_kl = 0.0; ok &= refused(step(), "max_kl"); good();
    hp.max_kl = NAN; ok &= refused(step(), "max_kl"); good();
    hp.max_kl = INFINITY; ok &= refused(step(), "max_kl"); good();
    hp.cg_damping = -1.0; ok &= refused(step(), "cg_damping"); good();
    hp.cg_damping = NAN; ok &= refused(step(), "cg_damping"); good();
    hp.entcoeff = INFINITY; ok &= refused(step(), "entcoeff"); good();
    hp.residual_tol = NAN; ok &= refused(step(), "residual_tol"); good();
    net.layout = QST_NET_SHARED_TRUNK; ok &= refused(step(), "shared-trunk"); ok &= refused(fit(10, 10, 0), "shared-trunk"); good();
    net.layout = 2; ok &= refused(step(), "layout"); good();
    net.w[12] = NULL; ok &= refused(step(), "NULL"); good();
    net.w[3] = (float *)((char *)net.w[3] + 2); ok &= refused(step(), "aligned"); good();
    bat.values = NULL; ok &= refused(step(), "NULL"); good();
    net.w[2] = net.w[0] + 1535; ok &= refused(step(), "overlap"); good();
    ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, net.w[2] + 8, NULL, NULL, NULL), "overlap");
    ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, y, net.w[4], NULL, NULL), "overlap");
    ok &= refused(qst_policy_step(&net, &bat, 7, &hp, big, ws_bytes, y, NULL, NULL, NULL), "overlap");
    trace.x = trace.fvp_out + 18696 * 10; ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, y, NULL, &trace, NULL), "overlap"); good();
    trace.ls = NULL; ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, y, NULL, &trace, NULL), "NULL"); good();
    trace.cg = (double *)((char *)cg + 4); ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, y, NULL, &trace, NULL), "aligned"); good();
    trace.struct_size = 8; ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, y, NULL, &trace, NULL), "QstTrace.struct_size"); good();
    net.struct_size = 8; ok &= refused(step(), "QstNet.struct_size"); good();
    bat.struct_size = 8; ok &= refused(step(), "QstBatch.struct_size"); good();
    hp.struct_size = 8; ok &= refused(step(), "QstHyper.struct_size"); good();
    ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes - 1, y, NULL, NULL, NULL), "workspace");
    ok &= refused(qst_policy_step(&net, &bat, 7, &hp, (char *)ws_store + 4, ws_bytes, y, NULL, NULL, NULL), "aligned");
    ok &= refused(qst_policy_step(NULL, &bat, 7, &hp, ws_store, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(qst_policy_step(&net, NULL, 7, &hp, ws_store, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(qst_policy_step(&net, &bat, 7, NULL, ws_store, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(qst_policy_step(&net, &bat, 7, &hp, NULL, ws_bytes, y, NULL, NULL, NULL), "NULL");
    ok &= refused(qst_policy_step(&net, &bat, 7, &hp, ws_store, ws_bytes, NULL, NULL, NULL, NULL), "NULL");
    ok &= refused(qst_workspace_bytes(300, 7, NULL), "bytes");
    ok &= refused(qst_workspace_bytes(0, 7, &ws_bytes), "n must");
    /* the value fit */
    ok &= refused(fit(10, 0, 0), "batch");
    ok &= refused(fit(10, 257, 0), "batch");
    ok &= refused(fit(0, 10, 0), "steps");
    ok &= refused(fit(4097, 10, 0), "steps");
    ok &= refused(fit(10, 10, -1), "t0");
    ok &= refused(fit(10, 10, ((int64_t)1 << 31) - 5), "t0");
    ok &= refused(qst_vf_fit(&net, x, x, 0, idx, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, y, NULL, NULL), "n must");
    ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, NAN, 0.9, 0.999, 1e-8, 0, y, NULL, NULL), "lr");
    ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, 3e-4, 1.0, 0.999, 1e-8, 0, y, NULL, NULL), "beta1");
    ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, 3e-4, 0.9, -0.1, 1e-8, 0, y, NULL, NULL), "beta2");
    ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, 3e-4, 0.9, 0.999, INFINITY, 0, y, NULL, NULL), "eps");
    net.m[8] = NULL; ok &= refused(fit(10, 10, 0), "NULL"); good();
    net.v[11] = (float *)((char *)net.v[11] + 2); ok &= refused(fit(10, 10, 0), "aligned"); good();
    net.m[9] = net.w[8] + 128 * 128 - 1; ok &= refused(fit(10, 10, 0), "overlap"); good();
    grads[5] = NULL; ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, y, grads, NULL), "NULL"); good();
    grads[2] = net.v[8]; ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, y, grads, NULL), "overlap"); good();
    ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, net.m[6] + 4, NULL, NULL), "overlap");
    ok &= refused(qst_vf_fit(NULL, x, x, 300, idx, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, y, NULL, NULL), "NULL");
    ok &= refused(qst_vf_fit(&net, NULL, x, 300, idx, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, y, NULL, NULL), "NULL");
    ok &= refused(qst_vf_fit(&net, x, x, 300, NULL, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, y, NULL, NULL), "NULL");
    ok &= refused(qst_vf_fit(&net, x, x, 300, idx, 10, 10, 3e-4, 0.9, 0.999, 1e-8, 0, NULL, NULL, NULL), "NULL");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    side_cases.run_c_caller("trpo", C_CALLER, tmp_path)


def test_check_args_mirror_the_library():
    from quadsim_amd import trpo
    n, s, hp = trpo.check_trpo_args(1024)
    assert (n, s) == (1024, 0) and hp == dict(max_kl=0.01, cg_damping=0.01, entcoeff=0.0, residual_tol=1e-10, cg_iters=10, backtracks=10, fvp_stride=5)
    bad = [dict(n=0), dict(n=1 << 31), dict(slices=-1), dict(slices=1025), dict(cg_iters=0), dict(cg_iters=65), dict(backtracks=0),
           dict(backtracks=33), dict(fvp_stride=0), dict(max_kl=0.0), dict(max_kl=float("nan")), dict(cg_damping=-1.0),
           dict(entcoeff=float("inf")), dict(residual_tol=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            trpo.check_trpo_args(**dict(dict(n=300), **kw))
    for args in ((0, 1, 1), (300, 0, 10), (300, 4097, 10), (300, 10, 0), (300, 10, 257)):
        with pytest.raises(ValueError):
            trpo.check_vf_args(*args)
    with pytest.raises(ValueError):
        trpo.check_vf_args(300, 10, 10, t0=-1)
    assert trpo.auto_slices(1024) == 64 and trpo.auto_slices(17) == 2 and trpo.auto_slices(0) == 0


# ---------------------------------------------------------------------------------------------------- the code object
def test_matrix_rows_are_the_kernels_of_the_code_object(notes):
    """k_trpo_vf_fit, which keeps Adam's state in registers, spills scalar registers"""
    assert len(notes) == 10
    side_cases.check_census(notes, trpo_matrix, lambda n: kernel_notes.instantiations_with_types(n, trpo_matrix.KERNELS, namespace="qst"), "trpo",
                            sgpr_spills=("k_trpo_vf_fit",))


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(trpo_matrix)


# ---------------------------------------------------------------------------------------------------- the reference against autograd
def _torch_policy(torch, W):
    return {k: torch.tensor(np.asarray(W[k], np.float64), requires_grad=True) for k in tr.POLICY_KEYS}


def _torch_mean(torch, P, obs):
    return torch.relu(torch.relu(obs @ P["w0"] + P["b0"]) @ P["w1"] + P["b1"]) @ P["w2"] + P["b2"]


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300))


def test_gradient_and_losses_equal_float64_autograd():
    import torch
    W, data = tr.weights(), tr.head(tr.rollout(), 300)
    P = _torch_policy(torch, W)
    obs, act = torch.tensor(data["obs"], dtype=torch.float64), torch.tensor(data["actions"], dtype=torch.float64)
    d = torch.tensor(data["returns"].astype(np.float64) - data["values"].astype(np.float64))
    adv = (d - d.mean()) / (d.std(unbiased=False) + 1e-8)
    mean, ls = _torch_mean(torch, P, obs), P["logstd"]
    nl = 0.5 * (((act - mean) / torch.exp(ls)) ** 2).sum(-1) + 2.0 * np.log(2.0 * np.pi) + ls.sum()
    ent = (ls + 0.5 * np.log(2.0 * np.pi * np.e)).sum()
    surr = (adv * torch.exp(nl.detach() - nl)).mean() + 0.01 * ent
    grads = torch.autograd.grad(surr, [P[k] for k in tr.POLICY_KEYS])
    G = tr.grad64(W, data, 0.01)
    assert _rel(G["g"], np.concatenate([g.numpy().reshape(-1) for g in grads])) < 1e-10
    assert abs(G["surr_before"] - float(surr.detach())) < 1e-12 and _rel(G["nlp_old"], nl.detach().numpy()) < 1e-12
    # a candidate: the surrogate and the mean KL at a moved theta
    rng = np.random.default_rng(3)
    th = (tr.flatten(W, np.float64) + 0.01 * rng.standard_normal(tr.P)).astype(np.float32)
    Pk = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in tr.unflatten(th).items()}
    mk, lk = _torch_mean(torch, Pk, obs), Pk["logstd"]
    nlk = 0.5 * (((act - mk) / torch.exp(lk)) ** 2).sum(-1) + 2.0 * np.log(2.0 * np.pi) + lk.sum()
    s_ref = (adv * torch.exp(nl.detach() - nlk)).mean() + 0.01 * (lk + 0.5 * np.log(2.0 * np.pi * np.e)).sum()
    kl_ref = (lk - ls.detach() + (torch.exp(2 * ls.detach()) + (mean.detach() - mk) ** 2) / (2 * torch.exp(2 * lk)) - 0.5).sum(-1).mean()
    s, kl = tr.ls_eval64(W, th, data, 0.01)
    assert abs(s - float(s_ref)) < 1e-10 * max(1.0, abs(float(s_ref))) and abs(kl - float(kl_ref)) < 1e-10 * float(kl_ref)


@pytest.mark.parametrize("n,stride", [(300, 5), (17, 1)])
def test_fisher_vector_product_equals_double_backprop_of_the_mean_kl(n, stride):
    import torch
    W, data = tr.weights(), tr.head(tr.rollout(), n)
    obs = torch.tensor(data["obs"][::stride], dtype=torch.float64)
    P = _torch_policy(torch, W)
    ps = [P[k] for k in tr.POLICY_KEYS]
    mean, ls = _torch_mean(torch, P, obs), P["logstd"]
    kl = (ls - ls.detach() + (torch.exp(2 * ls.detach()) + (mean.detach() - mean) ** 2) / (2 * torch.exp(2 * ls)) - 0.5).sum(-1).mean()
    gk = torch.autograd.grad(kl, ps, create_graph=True)
    flat = torch.cat([g.reshape(-1) for g in gk])
    rng = np.random.default_rng(5)
    basis_ls, basis_b0 = np.zeros(tr.P, np.float32), np.zeros(tr.P, np.float32)
    basis_ls[tr.LS0 + 2] = 1.0
    basis_b0[int(tr.STARTS[1]) + int(np.argmax(tr.forward(W, data["obs"][::stride])["z0"][0]))] = 1.0   # a unit that is active on a row
    for v in (rng.standard_normal(tr.P).astype(np.float32), basis_ls, basis_b0):
        hv = torch.autograd.grad((flat * torch.tensor(v.astype(np.float64))).sum(), ps, retain_graph=True)
        ref = np.concatenate([h.numpy().reshape(-1) for h in hv])
        assert np.abs(ref).max() > 0.0
        assert _rel(tr.fvp64(W, data["obs"], stride, v), ref) < 1e-10
        assert _rel(tr.fvp64(W, data["obs"], stride, v, 0.01), ref + 0.01 * v.astype(np.float64)) < 1e-10


@pytest.mark.parametrize("batch", [1, 17, 128])
def test_value_fit_gradients_equal_float64_autograd(batch):
    import torch
    W, data = tr.weights(), tr.head(tr.rollout(), batch)
    P = [torch.tensor(np.asarray(W[k], np.float64), requires_grad=True) for k in tr.VALUE_KEYS]
    obs, ret = torch.tensor(data["obs"], dtype=torch.float64), torch.tensor(data["returns"], dtype=torch.float64)
    v = (torch.relu(torch.relu(obs @ P[0] + P[1]) @ P[2] + P[3]) @ P[4] + P[5])[:, 0]
    loss = ((v - ret) ** 2).mean()
    grads = torch.autograd.grad(loss, P)
    l, G = tr.vf_backward64(W, data["obs"], data["returns"])
    assert abs(l - float(loss)) < 1e-12 * float(loss)
    for k, g in zip(tr.VALUE_KEYS, grads):
        assert _rel(G[k], g.numpy()) < 1e-10, k


# ---------------------------------------------------------------------------------------------------- the replay
def test_fma32_rounds_once_on_float32_ties():
    f = np.float32
    one = lambda a, b, c: tr.fma32(np.array([f(a)]), np.array([f(b)]), np.array([f(c)]))[0]  # noqa: E731
    assert one(2.0 ** -12, 2.0 ** -12, 1.0) == f(1.0)                                   # 1 + 2^-24, the tie itself: to even
    assert one(1.0 + 2.0 ** -23, 2.0 ** -24, 1.0) == f(1.0 + 2.0 ** -23)                # 1 + 2^-24 + 2^-47: above the tie
    assert one(1.0 - 2.0 ** -24, 2.0 ** -24, 1.0) == f(1.0)                             # 1 + 2^-24 - 2^-48: below it
    # the exact value 2^30 + 2^7 + 2^6 - 2^-40 lies below the tie of an ODD neighbour; a float64 sum lands ON the tie and a second
    # rounding to even would go up to 2^30 + 2^8
    c = 2.0 ** 30 + 2.0 ** 7
    assert f(c) == c and one(8.0 * (1.0 + 2.0 ** -23), 8.0 * (1.0 - 2.0 ** -23), c) == f(c)
    assert np.float64(8.0 * (1.0 + 2.0 ** -23)) * np.float64(8.0 * (1.0 - 2.0 ** -23)) + c == c + 64.0      # what float64 makes of it
    assert one(8.0 * (1.0 + 2.0 ** -23), 8.0 * (1.0 + 2.0 ** -23), c) == f(c + 2.0 ** 7)   # 2^6 (1 + 2^-22 + 2^-46): above the tie
    assert one(-8.0 * (1.0 + 2.0 ** -23), 8.0 * (1.0 - 2.0 ** -23), -c) == f(-c)


def test_dot_tree_and_replay_follow_the_float64_solver():
    rng = np.random.default_rng(11)
    a, b = rng.standard_normal(tr.P).astype(np.float32), rng.standard_normal(tr.P).astype(np.float32)
    assert abs(tr.dot_tree(a, b) - float(a.astype(np.float64) @ b.astype(np.float64))) < 1e-9
    one = np.zeros(tr.P, np.float32)
    one[[0, 255, 256, tr.P - 1]] = 1.0
    assert tr.dot_tree(one, one) == 4.0
    # the replay on a small SPD system embedded in P elements follows SB2's cg in float64
    W, data = tr.weights(), tr.head(tr.rollout(), 17)
    g = tr.grad64(W, data, 0.01)["g"].astype(np.float32)
    x, r, p, zs = np.zeros(tr.P), g.astype(np.float64), g.astype(np.float64), []
    ps = []
    for k in range(4):
        ps.append(p.astype(np.float32))
        z = tr.fvp64(W, data["obs"], 5, ps[-1], 0.01)
        zs.append(z.astype(np.float32))
        al = (r @ r) / (p @ z)
        x, rn = x + al * p, r - al * z
        p, r = rn + (rn @ rn) / (r @ r) * p, rn
    # (each z was computed at the float32 p of the float64 iteration, so the replay sees nearly the same sequence)
    R = tr.replay_cg(g, zs, zs[-1], 4, 0.01)
    assert R["iters"] == 4 and _rel(R["x"], x) < 1e-3 and R["x"].dtype == np.float32 and R["fullstep"].dtype == np.float32
    assert same_sign(R["cg"][:, 1]) and np.all(R["cg"][:, 2] > 0)


def same_sign(a):
    return bool(np.all(a > 0) or np.all(a < 0))


# ---------------------------------------------------------------------------------------------------- the schedule
def test_vf_schedule_properties():
    import torch
    from quadsim_amd import trpo
    g = torch.Generator().manual_seed(3)
    idx = trpo.vf_schedule(300, 128, 3, g)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (6, 128) and idx.is_contiguous()
    for e in range(3):
        rows = idx[2 * e:2 * e + 2].reshape(-1).numpy()
        assert np.unique(rows).size == 256 and rows.min() >= 0 and rows.max() < 300
    assert not torch.equal(idx[:2], idx[2:4])
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    assert torch.equal(trpo.vf_schedule(64, 16, 3, g1), torch.cat([trpo.vf_schedule(64, 16, 1, g2), trpo.vf_schedule(64, 16, 2, g2)]))
    assert tuple(trpo.vf_schedule(128, 128, 1, g).shape) == (1, 128)
    with pytest.raises(ValueError, match="value batch"):
        trpo.vf_schedule(127, 128, 3, g)
    with pytest.raises(ValueError):
        trpo.vf_schedule(300, 0, 3, g)


def test_python_refusals_need_no_device():
    import quadsim_amd as qa

    class Env:
        num_envs, device = 8, "cpu"

    with pytest.raises(ValueError, match="shared"):
        qa.TRPO(qa.ActorCriticPolicy(pr.weight_set("he", "shared"), device="cpu"), Env(), n_steps=16)
    with pytest.raises(ValueError, match="squash"):
        qa.TRPO(qa.ActorCriticPolicy(tr.weights(), device="cpu", squash=True), Env(), n_steps=16)
    with pytest.raises(qa.QuadsimError, match="HIP device"):
        qa.TRPO(qa.ActorCriticPolicy(tr.weights(), device="cpu"), Env(), n_steps=16)
    with pytest.raises(ValueError, match="value batch"):
        qa.TRPO(qa.ActorCriticPolicy(tr.weights(), device="cpu"), Env(), n_steps=8, vf_batch=128, update="torch")
    with pytest.raises(qa.QuadsimError, match="HIP device"):
        qa.trpo_policy_step(qa.ActorCriticPolicy(tr.weights(), device="cpu"), {})


def test_torch_paths_follow_the_float64_reference():
    """the comparison paths on the CPU: the accepted candidate of a fixture and one value step against the reference"""
    import torch
    import quadsim_amd as qa
    W, data, hp, S = tr.ls_fixture("small")
    pol = qa.ActorCriticPolicy({k: np.array(v) for k, v in W.items()}, device="cpu")       # (a CPU tensor would share the fixture's memory)
    ro = {k: torch.as_tensor(v) for k, v in data.items()}
    out = qa.torch_trpo_policy_step(pol, ro, **hp)
    st = out["stats"].numpy()
    assert st[8] == S["accepted"] and abs(st[2] - S["stats"][2]) < 0.05 * S["stats"][2] and st[9] == S["iters"]
    idx = torch.arange(17, dtype=torch.int32)[None]
    vf = qa.torch_trpo_vf_fit(pol, ro, idx, vf_stepsize=1e-3)
    loss, _ = tr.vf_backward64(W, data["obs"], data["returns"])
    assert abs(float(vf["stats"][0]) - loss) < 1e-4 * loss and pol._trpo_steps == 1
    qa.reset_trpo_optimizer(pol)
    assert pol._trpo_steps == 0 and pol._trpo_m is None


# ---------------------------------------------------------------------------------------------------- the census
@pytest.mark.parametrize("name", list(tr.LS_FIXTURES))
def test_line_search_fixture_census(name):
    """for every candidate up to the accepted one, |kl_k - 1.5 max_kl| and |surr_k - surr_before| exceed ten times the derived bound
    of that statistic in the float64 reference; the reference accepts the recorded k; no hidden unit of the fixture's rows lies
    within four bounds of zero"""
    W, data, hp, S = tr.ls_fixture(name)
    n, stride, scale, max_kl, backtracks, seed, want = tr.LS_FIXTURES[name]
    assert S["accepted"] == want and data["obs"].shape[0] == n and not tr.relu_edges(W, data["obs"]).any()
    sb, E_sb = S["G"]["surr_before"], S["G"]["E_surr"]
    assert len(S["cands"]) == (want + 1 if want >= 0 else backtracks)
    for k, (surr, kl, E_s, E_k) in enumerate(S["cands"]):
        print("%s candidate %d: improve %.4g (bound %.3g), kl %.4g (bound %.3g)" % (name, k, surr - sb, E_s + E_sb, kl, E_k))
        assert abs(kl - 1.5 * max_kl) > 10.0 * E_k and abs(surr - sb) > 10.0 * (E_s + E_sb), k
    if name == "small":
        c = S["cands"]
        assert c[0][0] - sb < 0.0 and all(c[k][0] - sb >= 0.0 and c[k][1] > 1.5 * max_kl for k in range(1, 5))
    if name == "none":
        assert np.array_equal(S["theta"], tr.flatten(W, np.float64))


def test_the_other_eight_libraries_are_instruction_identical():
    """profiles/trpo/isa_diff.txt is the output of tools/isa_diff.py, the parent commit's build against this one, for each of the
    other eight libraries: every kernel line says `same`.  None of them can have moved: no file they are built from belongs to
    this library (held above)"""
    text = open(os.path.join(ROOT, "profiles", "trpo", "isa_diff.txt")).read()
    libs = re.findall(r"^## (\S+)$", text, flags=re.M)
    assert libs == ["libquadsim_hip.so", "libquadsim_dyn.so", "libquadsim_dynmppi.so", "libquadsim_dynfit.so", "libquadsim_bc.so",
                    "libquadsim_ppo.so", "libquadsim_gail.so", "libquadsim_ddpg.so"]
    lines = [ln for ln in text.splitlines() if re.match(r"^_Z\S+: ", ln)]
    assert len(lines) == 279 and all(ln.endswith(": same") for ln in lines)
    totals = re.findall(r"^identical in fields and disassembly: (\d+) of (\d+)$", text, flags=re.M)
    assert len(totals) == 8 and all(a == b for a, b in totals)
