"""-m "not gpu": everything of the PPO2 update on the device that needs no device.  include/quadsim_ppo.h is plain C99 and every
symbol it declares is exported by libquadsim_ppo.so; the entry of quadsim_amd._lib.SIDE matches the header; every refusal the
header promises happens before anything is launched, and check_ppo2_args mirrors it; tests/ppo2_matrix.py has exactly one row per
kernel of the new code object, none uses scratch or spills; tests/ppo2_ref.py is checked against torch's float64 autograd of the
loss as the reference writes it and against central differences; every fixture of tests/test_gpu_ppo2.py holds the conditions
under which the derived bounds apply, with no row left out; and the host logic (schedule, arguments, the learn loop's
bookkeeping, save_npz) does what it says."""
import ctypes as C
import os

import numpy as np
import pytest

import kernel_notes
import ppo2_matrix
import ppo2_ref as pr
import side_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, ppo2
    _lib.build_library()
    return ppo2.load_ppo()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("ppo", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    side_cases.check_exports("ppo", lib, ["qsp_auto_slices", "qsp_last_error", "qsp_update", "qsp_version", "qsp_workspace_bytes"])


def test_no_other_library_holds_its_kernels(lib):
    side_cases.check_no_foreign_kernels("ppo")


def test_table_entry_names_its_own_files(lib):
    import quadsim_amd as qa
    from quadsim_amd import _lib, ppo2
    assert ppo2.PPO_EXPORTS is _lib.SIDE["ppo"]["exports"]
    side_cases.check_entry("ppo", ["ppo2_kernels.hpp", "quadsim_device.hpp", "quadsim_ppo.h", "side_host.hpp", "train_pieces.hpp"], "ppo2.hip")
    assert [lib.qsp_auto_slices(b) for b in (-1, 0, 1, 16, 17, 600, 2048, 2049, (1 << 31) - 1)] == [0, 0, 1, 1, 2, 38, 128, 128, 128]
    assert [ppo2.auto_slices(b) for b in (-1, 0, 1, 16, 17, 600, 2048, 2049, (1 << 31) - 1)] == [0, 0, 1, 1, 2, 38, 128, 128, 128]
    for name in ("PPO2", "ppo2_update", "torch_ppo2_update", "minibatch_schedule", "check_ppo2_args", "reset_ppo2_optimizer"):
        assert getattr(qa, name) is getattr(ppo2, name) and name in qa.__all__
    assert ppo2.SLOT_KEYS == pr.SLOT_KEYS and dict(zip(ppo2.SLOT_KEYS, ppo2.SLOT_SHAPES)) == pr.SHAPES


def test_train_signature_table_matches_the_header():
    """the structs have the header's sizes; the prototypes are held by tests/test_call_path_cpu.py, for every side library"""
    from quadsim_amd import _lib
    assert C.sizeof(_lib.QspNet) == 8 + 39 * 8 and C.sizeof(_lib.QspBatch) == 16 + 5 * 8 and C.sizeof(_lib.QspHyper) == 8 + 9 * 8


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_ppo.h"

static float x[40][64];
static double ws[1 << 20];
static int32_t idx[64];
static QspNet net;
static QspBatch data;
static QspHyper hp;
static float *grads[13];

static int refused(int rc, const char *word)
{
    if (rc == QSP_OK || strstr(qsp_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qsp_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int call(int steps, int64_t batch, int slices, int64_t t0)
{
    return qsp_update(&net, &data, idx, steps, batch, slices, &hp, t0, ws, sizeof ws, x[39], NULL, NULL);
}

static int with(double *field, double value, const char *word)
{
    const double keep = *field;
    int ok;
    *field = value;
    ok = refused(call(10, 64, 1, 0), word);
    *field = keep;
    return ok;
}

int main(void)
{
    int ok = 1, i;
    size_t bytes = 0;
    void *fns[] = {(void *)qsp_version, (void *)qsp_last_error, (void *)qsp_auto_slices, (void *)qsp_workspace_bytes, (void *)qsp_update};
    if (qsp_version() != QSP_VERSION) return 2;
    net.struct_size = sizeof net; net.layout = QSP_NET_TOWERS;
    data.struct_size = sizeof data; data.n = 300;
    data.obs = data.actions = data.returns = data.values = data.neglogp = x[38];
    hp.struct_size = sizeof hp;
    hp.lr = 3e-4; hp.cliprange = 0.2; hp.cliprange_vf = -1.0; hp.ent_coef = 0.0; hp.vf_coef = 0.5; hp.max_grad_norm = 0.5;
    hp.beta1 = 0.9; hp.beta2 = 0.999; hp.eps = 1e-5;
    for (i = 0; i < 13; ++i) { net.w[i] = net.m[i] = net.v[i] = x[0]; grads[i] = x[0]; }
    ok &= refused(call(0, 64, 1, 0), "steps");
    ok &= refused(call(4097, 64, 1, 0), "steps");
    ok &= refused(call(10, 0, 1, 0), "batch");
    ok &= refused(call(10, (int64_t)1 << 31, 1, 0), "batch");
    ok &= refused(call(10, 64, -1, 0), "slices");
    ok &= refused(call(10, 64, 1025, 0), "slices");
    ok &= refused(call(10, 64, 1, -1), "t0");
    ok &= refused(call(10, 64, 1, ((int64_t)1 << 31) - 10), "t0");
    ok &= with(&hp.lr, NAN, "lr");
    ok &= with(&hp.lr, INFINITY, "lr");
    ok &= with(&hp.cliprange, NAN, "cliprange");
    ok &= with(&hp.cliprange, -0.1, "cliprange");
    ok &= with(&hp.cliprange_vf, INFINITY, "cliprange_vf");
    ok &= with(&hp.ent_coef, NAN, "ent_coef");
    ok &= with(&hp.vf_coef, INFINITY, "vf_coef");
    ok &= with(&hp.max_grad_norm, NAN, "max_grad_norm");
    ok &= with(&hp.beta1, 1.0, "beta1");
    ok &= with(&hp.beta1, -0.1, "beta1");
    ok &= with(&hp.beta2, 1.0, "beta2");
    ok &= with(&hp.beta2, NAN, "beta2");
    ok &= with(&hp.eps, INFINITY, "eps");
    data.n = 0;
    ok &= refused(call(10, 64, 1, 0), "n must");
    data.n = (int64_t)1 << 31;
    ok &= refused(call(10, 64, 1, 0), "n must");
    data.n = 300;
    /* every tensor of the net is the same array here: the call is otherwise acceptable, and overlapping tensors are refused */
    ok &= refused(call(10, 64, 1, 0), "overlap");
    /* with tensors of their own the workspace that is one byte short is what is wrong */
    for (i = 0; i < 13; ++i) { net.w[i] = x[i]; net.m[i] = x[13 + i]; net.v[i] = x[26 + i]; }
    if (qsp_workspace_bytes(64, 1, &bytes) != QSP_OK || bytes == 0 || bytes > sizeof ws) { printf("workspace_bytes\n"); ok = 0; }
    ok &= refused(qsp_update(&net, &data, idx, 10, 64, 1, &hp, 0, ws, bytes - 1, x[39], NULL, NULL), "workspace");
    ok &= refused(qsp_update(&net, &data, idx, 10, 64, 1, &hp, 0, (char *)ws + 4, sizeof ws - 4, x[39], NULL, NULL), "aligned");
    ok &= refused(qsp_update(&net, &data, idx, 10, 64, 1, &hp, 0, ws, sizeof ws, (float *)ws + 5, NULL, NULL), "overlap");
    net.w[3] = NULL;
    ok &= refused(call(10, 64, 1, 0), "NULL");
    net.w[3] = x[3];
    net.layout = QSP_NET_SHARED_TRUNK;          /* wv0, bv0 given where the layout has none */
    ok &= refused(call(10, 64, 1, 0), "NULL");
    net.layout = 2;
    ok &= refused(call(10, 64, 1, 0), "layout");
    net.layout = QSP_NET_TOWERS;
    net.struct_size = 8;
    ok &= refused(call(10, 64, 1, 0), "QspNet.struct_size");
    net.struct_size = sizeof net;
    data.struct_size = 8;
    ok &= refused(call(10, 64, 1, 0), "QspBatch.struct_size");
    data.struct_size = sizeof data;
    hp.struct_size = 8;
    ok &= refused(call(10, 64, 1, 0), "QspHyper.struct_size");
    hp.struct_size = sizeof hp;
    data.obs = NULL;
    ok &= refused(call(10, 64, 1, 0), "NULL");
    data.obs = (const float *)((const char *)x[38] + 2);
    ok &= refused(call(10, 64, 1, 0), "aligned");
    data.obs = x[38];
    grads[5] = NULL;
    ok &= refused(qsp_update(&net, &data, idx, 10, 64, 1, &hp, 0, ws, sizeof ws, x[39], grads, NULL), "NULL");
    ok &= refused(qsp_update(NULL, &data, idx, 10, 64, 1, &hp, 0, ws, sizeof ws, x[39], NULL, NULL), "NULL");
    ok &= refused(qsp_update(&net, NULL, idx, 10, 64, 1, &hp, 0, ws, sizeof ws, x[39], NULL, NULL), "NULL");
    ok &= refused(qsp_update(&net, &data, NULL, 10, 64, 1, &hp, 0, ws, sizeof ws, x[39], NULL, NULL), "NULL");
    ok &= refused(qsp_update(&net, &data, idx, 10, 64, 1, NULL, 0, ws, sizeof ws, x[39], NULL, NULL), "NULL");
    ok &= refused(qsp_update(&net, &data, idx, 10, 64, 1, &hp, 0, NULL, sizeof ws, x[39], NULL, NULL), "NULL");
    ok &= refused(qsp_update(&net, &data, idx, 10, 64, 1, &hp, 0, ws, sizeof ws, NULL, NULL, NULL), "NULL");
    ok &= refused(qsp_workspace_bytes(0, 1, &bytes), "batch");
    ok &= refused(qsp_workspace_bytes(64, 1025, &bytes), "slices");
    ok &= refused(qsp_workspace_bytes(64, 1, NULL), "NULL");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    side_cases.run_c_caller("ppo", C_CALLER, tmp_path)


GOOD = dict(n=300, steps=100, batch=60, slices=0)


@pytest.mark.parametrize("kw", [
    dict(steps=0), dict(steps=4097), dict(batch=0), dict(batch=1 << 31), dict(slices=-1), dict(slices=1025), dict(n=0), dict(n=1 << 31),
    dict(t0=-1), dict(t0=(1 << 31) - 100), dict(learning_rate=float("nan")), dict(learning_rate=float("inf")), dict(cliprange=-0.1),
    dict(cliprange=float("nan")), dict(cliprange_vf=float("inf")), dict(ent_coef=float("nan")), dict(vf_coef=float("inf")),
    dict(max_grad_norm=float("nan")), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=float("inf"))],
    ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_check_ppo2_args_refuses_before_the_library_is_touched(monkeypatch, kw):
    from quadsim_amd import ppo2
    monkeypatch.setattr(ppo2, "load_ppo", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    n, steps, batch, slices, hp, t0 = ppo2.check_ppo2_args(**GOOD)
    assert (n, steps, batch, slices, t0) == (300, 100, 60, 0, 0) and hp["eps"] == 1e-5 and hp["cliprange_vf"] == -1.0
    assert ppo2.check_ppo2_args((1 << 31) - 1, 4096, (1 << 31) - 1, 1024, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, (1 << 31) - 4097)[1] == 4096
    with pytest.raises(ValueError):
        ppo2.check_ppo2_args(**dict(GOOD, **kw))


def test_update_refuses_squashed_and_host_policies_before_the_library_is_touched(monkeypatch):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import ppo2
    monkeypatch.setattr(ppo2, "load_ppo", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    W = pr.weight_set("he", "shared")
    data = {k: torch.as_tensor(v) for k, v in pr.rollout("he", "shared").items()}
    idx = torch.zeros((2, 10), dtype=torch.int32)
    kw = dict(learning_rate=3e-4, cliprange=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)
    with pytest.raises(ValueError, match="squash"):
        ppo2.ppo2_update(qa.ActorCriticPolicy(W, device="cpu", squash=True), data, idx, **kw)
    with pytest.raises(ValueError, match="squash"):
        ppo2.torch_ppo2_update(qa.ActorCriticPolicy(W, device="cpu", squash=True), data, idx, **kw)
    with pytest.raises(ValueError, match="squash"):
        ppo2.PPO2(qa.ActorCriticPolicy(W, device="cpu", squash=True), None)
    with pytest.raises(qa.QuadsimError, match="HIP device"):
        ppo2.ppo2_update(qa.ActorCriticPolicy(W, device="cpu"), data, idx, **kw)
    with pytest.raises(TypeError):
        ppo2.policy_tensors(qa.MlpPolicy(pr.br.weight_set("he"), device="cpu"))
    pol = qa.ActorCriticPolicy(W, device="cpu")
    pol._ppo_steps, pol._ppo_m = 5, [1]
    pol.reset_ppo2_optimizer()
    assert pol._ppo_steps == 0 and pol._ppo_m is None and pol._ppo_ws is None and not hasattr(pol, "_bc_steps")


# ---------------------------------------------------------------------------------------------------- the census
def test_rows_are_exactly_the_kernels_of_the_code_object_without_scratch(notes):
    got = side_cases.check_census(notes, ppo2_matrix, lambda n: kernel_notes.instantiations_with_types(n, ppo2_matrix.KERNELS, namespace="qsp"), "ppo2")
    assert got[("k_ppo_grad",)]["vgpr_count"] < 230                   # Adam's moments do not live in it, unlike k_bc_fit


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(ppo2_matrix)


# ---------------------------------------------------------------------------------------------------- the reference itself
# clip ranges whose 1 +- eps are float32 numbers: the reference clips at float32(1 +- eps) as the device does, torch at the doubles
HP_EXACT = {"novclip": dict(pr.HP_NOVCLIP, cliprange=0.25), "vclip": dict(pr.HP_VCLIP, cliprange=0.25, cliprange_vf=0.25)}


def _torch_case(W, mb, hp):
    import torch
    from quadsim_amd.ppo2 import ppo2_loss
    T = {k: torch.tensor(np.asarray(W[k], np.float64), requires_grad=True) for k in pr.keys_of(W)}
    d = {k: torch.tensor(v.astype(np.float64)) for k, v in mb.items()}
    loss, parts = ppo2_loss(torch, T, d["obs"], d["actions"], d["returns"], d["values"], d["neglogp"], hp["cliprange"], hp["cliprange_vf"],
                            hp["ent_coef"], hp["vf_coef"])
    loss.backward()
    return float(loss.detach()), np.array([float(p.detach()) for p in parts]), {k: T[k].grad.numpy() for k in T}


@pytest.mark.parametrize("case", pr.CASES, ids=pr.CASE_IDS)
def test_backward64_against_torch_float64_autograd(case):
    """the hand-derived per-branch form against autograd of the loss written as ppo2.py:147-188 writes it (quadsim_amd.ppo2.ppo2_loss,
    which shares no code with it)"""
    name, layout = case
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    for hpname, hp in HP_EXACT.items():
        for batch in (17, 300):
            mb = pr.minibatch(data, pr.step_rows(name, layout, batch, hpname))
            st, G = pr.backward64(W, mb, hp)
            loss, parts, Gt = _torch_case(W, mb, hp)
            assert abs(loss - pr.total_loss64(W, mb, hp)) <= 1e-12 * max(1.0, abs(loss))
            assert np.abs(parts - st[:5]).max() <= 1e-12 * max(1.0, np.abs(parts).max()), (parts, st)
            assert sorted(G) == sorted(Gt)
            for k in G:
                assert G[k].shape == pr.SHAPES[k] and np.abs(G[k] - Gt[k]).max() <= 1e-11 * max(1.0, np.abs(Gt[k]).max()), (k, hpname, batch)
            norm = np.sqrt(sum((g ** 2).sum() for g in Gt.values()))
            assert abs(st[5] - norm) <= 1e-11 * max(1.0, norm)


def test_backward64_against_central_differences():
    name, layout, hp = "he", "towers", HP_EXACT["vclip"]
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    mb = pr.minibatch(data, pr.step_rows(name, layout, 17))
    _, G = pr.backward64(W, mb, hp)
    rng = np.random.default_rng(5)
    h = 1e-6
    for key in pr.keys_of(W):
        for j in rng.permutation(W[key].size)[:12]:
            P, M = dict(W), dict(W)
            P[key] = W[key].astype(np.float64); M[key] = W[key].astype(np.float64)
            P[key].flat[j] += h; M[key].flat[j] -= h
            num = (pr.total_loss64(P, mb, hp) - pr.total_loss64(M, mb, hp)) / (2 * h)
            assert abs(num - G[key].flat[j]) <= 2e-7 * max(1.0, abs(num)), (key, j, num, G[key].flat[j])


def test_tie_goes_to_the_unclipped_term():
    """rows whose old neglogp is the new one: r is exactly 1, both surrogate terms are equal, and the row is active with the
    unclipped term's gradient (tf.maximum's x >= y) -- as is a row whose value has not moved, whose two losses are equal"""
    name, layout, hp = "sb2", "shared", HP_EXACT["vclip"]
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    mb = dict(pr.minibatch(data, pr.step_rows(name, layout, 17)))
    Fp, Fv = pr.forward64(W, mb)
    mb["neglogp"] = pr.head64(W, mb, hp, Fp, Fv)["nl"]               # float64: the reference's own value, exactly
    H = pr.head64(W, mb, hp, Fp, Fv)
    assert (H["r"] == 1.0).all() and (H["p1"] == H["p2"]).all() and H["pol_active"].all() and not H["clipped"].any()
    assert np.array_equal(H["dmean"], -(H["A"] / 17.0)[:, None] * H["z"] / np.exp(W["logstd"].astype(np.float64)))
    assert (np.abs(H["dmean"]).max(-1) > 0).all() and (H["kl"] == 0.0).all()
    one = dict(mb, values=Fv["y"][:, 0])                             # and the value head at v == old_v
    H = pr.head64(W, one, hp, Fp, Fv)
    assert (H["dv"] == 0.0).all() and (H["l1"] == H["l2"]).all() and H["val_active"].all() and not H["val_clipped"].any()
    # the whole gradient at the tie is autograd's (inside the range both terms carry the same gradient, however a tie is split)
    st, G = pr.backward64(W, mb, hp)
    _, parts, Gt = _torch_case(W, mb, hp)
    assert all(np.abs(G[k] - Gt[k]).max() <= 1e-11 * max(1.0, np.abs(Gt[k]).max()) for k in G) and parts[4] == 0.0 == st[4]


# ---------------------------------------------------------------------------------------------------- the fixtures' conditions
@pytest.mark.parametrize("case", pr.CASES, ids=pr.CASE_IDS)
def test_every_gpu_fixture_minibatch_holds_the_conditions_of_the_bounds(case):
    """the bounds assume that the device takes the float64 reference's side of every decision.  For every minibatch that
    tests/test_gpu_ppo2.py compares with them, with NO exclusion: no pre-activation within its bound of zero, no ratio within its
    bound of 1 +- eps, no advantage within its bound of zero (its sign decides which side of the range is clipped off), no value
    step within its bound of cliprange_vf, no two unequal value losses within their bounds of each other; and, from 15 rows on,
    at least three rows in every head class (a minibatch of one row has one row)"""
    name, layout = case
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    assert all(v.shape[0] == pr.N_ROWS for v in data.values())
    assert pr.STEP_BATCHES == (1, 15, 16, 17, 64, 300)
    for hpname, hp in pr.HPS.items():
        for batch in pr.STEP_BATCHES + (33,):
            rows = pr.step_rows(name, layout, batch, hpname)
            assert rows.shape == (batch,) and len(set(rows.tolist())) == batch and 0 <= rows.min() and rows.max() < pr.N_ROWS
            edges, H = pr.edge_counts(W, pr.minibatch(data, rows), hp)
            assert not any(edges.values()), (hpname, batch, edges)
            if batch >= 15:
                cls = {k: int(v.sum()) for k, v in pr.head_classes(H).items()}
                if hp["cliprange_vf"] < 0:
                    assert cls.pop("value clipped-off") == 0
                assert min(cls.values()) >= 3, (hpname, batch, cls)
            else:
                assert (H["A"] == 0.0).all() and (H["E_A"] == 0.0).all()           # one row: a normalised advantage of 0, as numpy gives


def test_the_clip_of_the_one_step_case_is_active():
    for name, layout in pr.CASES:
        W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
        for hpname, hp in pr.HPS.items():
            for batch in pr.STEP_BATCHES:
                st = pr.loss64(W, pr.minibatch(data, pr.step_rows(name, layout, batch, hpname)), hp)
                assert st[5] > 1.5 * hp["max_grad_norm"], (name, layout, hpname, batch, st[5])


def test_adv_norm64_is_numpys():
    data = pr.rollout("he", "shared")
    d = data["returns"] - data["values"]                                       # float32, as numpy subtracts the Runner's arrays
    A, E = pr.adv_norm64(data["returns"], data["values"], with_bound=True)
    assert abs(A.mean()) < 1e-12 and abs(A.std() - 1.0) < 1e-6 and (E < 1e-5).all() and (E > 0).all()
    assert (np.abs(A - (d - d.mean()) / (d.std() + 1e-8)) <= 8.0 * E + 1e-6).all()           # the float32 original (numpy's own sums)
    one, e1 = pr.adv_norm64(data["returns"][:1], data["values"][:1], with_bound=True)
    assert one[0] == 0.0 and e1[0] == 0.0


# ---------------------------------------------------------------------------------------------------- the reference's behaviour
def test_twenty_steps_lower_the_references_own_value_loss():
    st = pr.learn64()
    assert st.shape == (pr.LEARN_STEPS, 6) and np.isfinite(st).all()
    margin = st[0, 1] - st[-1, 1]
    print("ppo2 learn64: value loss %.6g -> %.6g (margin %.3g), approxkl %.3g -> %.3g" % (st[0, 1], st[-1, 1], margin, st[0, 3], st[-1, 3]))
    assert margin > 0.1 * st[0, 1] and np.isfinite(st[:, 3]).all()


def test_torch_update_is_the_references_update():
    """torch_ppo2_update on the host, float32, against update64: the same loss, clip and Adam (to float32's accuracy on library
    GEMMs: a part in a thousand of the step)"""
    import torch
    import quadsim_amd as qa
    from quadsim_amd import ppo2
    name, layout, hp = "he", "towers", dict(pr.HP_VCLIP, max_grad_norm=0.5, lr=1e-3)
    W, data = pr.weight_set(name, layout), pr.rollout(name, layout)
    rows = pr.step_rows(name, layout, 64)
    pol = qa.ActorCriticPolicy({k: v.copy() for k, v in W.items()}, device="cpu")      # on the host a policy shares its arrays' memory
    out = ppo2.torch_ppo2_update(pol, {k: torch.as_tensor(v) for k, v in data.items()}, torch.as_tensor(rows[None, :]), learning_rate=hp["lr"],
                                 cliprange=hp["cliprange"], cliprange_vf=hp["cliprange_vf"], ent_coef=hp["ent_coef"], vf_coef=hp["vf_coef"],
                                 max_grad_norm=hp["max_grad_norm"], return_grads=True)
    st, G = pr.backward64(W, pr.minibatch(data, rows), hp)
    Z = pr.zero_state(W)
    Wn = pr.update64(W, Z, Z, G, hp, 1)[0]
    assert np.abs(out["stats"][0].numpy() - st).max() <= 1e-3 * np.abs(st).max()
    for k, g in zip(ppo2.SLOT_KEYS, out["grads"]):
        assert np.abs(g.numpy() - G[k]).max() <= 1e-3 * np.abs(G[k]).max(), k
        step = np.abs(Wn[k] - W[k]).max()
        assert np.abs(getattr(pol, k).numpy() - Wn[k]).max() <= 5e-2 * step, k
    assert pol._ppo_steps == 1 and np.array_equal(pol.logstd_host, pol.logstd.numpy()) and not np.array_equal(pol.logstd_host, W["logstd"])


# ---------------------------------------------------------------------------------------------------- the host logic
def test_minibatch_schedule():
    import torch
    from quadsim_amd import minibatch_schedule
    gen = lambda s: torch.Generator().manual_seed(s)     # noqa: E731
    for n_batch, nmb, epochs in ((6000, 10, 10), (12, 3, 2), (7, 7, 3), (5, 1, 1)):
        idx = minibatch_schedule(n_batch, nmb, epochs, gen(3))
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (epochs * nmb, n_batch // nmb) and idx.is_contiguous() and idx.device.type == "cpu"
        for e in range(epochs):
            used = idx[e * nmb:(e + 1) * nmb].reshape(-1)
            assert torch.equal(torch.sort(used).values, torch.arange(n_batch, dtype=torch.int32))       # a permutation per epoch
        assert torch.equal(idx, minibatch_schedule(n_batch, nmb, epochs, gen(3)))
        if n_batch > 5:
            assert not torch.equal(idx, minibatch_schedule(n_batch, nmb, epochs, gen(4)))
        g = gen(3)                                               # epoch by epoch from one generator: the same schedule
        assert torch.equal(idx, torch.cat([minibatch_schedule(n_batch, nmb, 1, g) for _ in range(epochs)]))
    idx = minibatch_schedule(6000, 10, 2, gen(3))
    assert not torch.equal(idx[:10], idx[10:])                   # a fresh shuffle every epoch
    for bad in ((10, 3, 1), (0, 1, 1), (10, 0, 1), (10, 2, 0)):
        with pytest.raises(ValueError):
            minibatch_schedule(*bad, gen(0))


class StubRunner:
    """what PPO2.learn may use of a Runner: run() -> the 9-tuple, the device episode tensors"""

    def __init__(self, torch, n_batch):
        self.torch, self.n_batch, self.runs = torch, n_batch, 0
        self.last_ep_returns, self.last_ep_lengths = torch.tensor([1.0, 3.0]), torch.tensor([10, 30], dtype=torch.int32)

    def run(self):
        t = self.torch
        self.runs += 1
        z = t.zeros(self.n_batch)
        return (t.zeros((self.n_batch, 12)), t.arange(self.n_batch, dtype=t.float32), z.bool(), t.zeros((self.n_batch, 4)), z, z, None, [], z)


class StubEnv:
    num_envs = 4


def test_learn_bookkeeping_on_a_stub_runner(monkeypatch):
    """frac falls from 1 by 1 / n_updates, callables of it give the rates of every update, loss_vals is the mean of the steps'
    statistics, the schedule is noptepochs x nminibatches rows of n_batch / nminibatches, and a callback returning False stops"""
    import torch
    import quadsim_amd as qa
    from quadsim_amd import ppo2
    calls = []

    def fake_update(policy, rollout, indices, **kw):
        calls.append((tuple(indices.shape), kw["learning_rate"], kw["cliprange"], kw["cliprange_vf"], kw["check_indices"]))
        stats = torch.arange(indices.shape[0] * 6, dtype=torch.float32).view(-1, 6)
        return {"stats": stats, "grads": None}
    monkeypatch.setattr(ppo2, "ppo2_update", fake_update)
    pol = qa.ActorCriticPolicy(pr.weight_set("he", "shared"), device="cpu")
    runner = StubRunner(torch, 4 * 6)
    model = qa.PPO2(pol, StubEnv(), n_steps=6, nminibatches=3, noptepochs=2, learning_rate=lambda f: 1e-3 * f, cliprange=lambda f: 0.2 * f,
                    runner=runner)
    logs = model.learn(4 * 24 + 5)
    assert runner.runs == 4 and model.num_timesteps == 96 and len(logs) == 4
    assert [c[0] for c in calls] == [(6, 8)] * 4 and not any(c[4] for c in calls) and all(c[3] is None for c in calls)
    np.testing.assert_allclose([c[1] for c in calls], [1e-3, 0.75e-3, 0.5e-3, 0.25e-3], rtol=1e-12)
    np.testing.assert_allclose([c[2] for c in calls], [0.2, 0.15, 0.1, 0.05], rtol=1e-12)
    for i, log in enumerate(logs):
        assert log["n_updates"] == i + 1 and log["total_timesteps"] == 24 * (i + 1) and log["serial_timesteps"] == 6 * (i + 1)
        assert [log[k] for k in ppo2.STAT_NAMES] == [15.0 + j for j in range(6)]         # the mean over six steps of 6 s + j
        assert log["ep_reward_mean"] == 2.0 and log["ep_len_mean"] == 20.0 and log["explained_variance"] == 0.0 and log["fps"] > 0
    # the callback sees the loop's locals and stops it
    seen = []
    model2 = qa.PPO2(pol, StubEnv(), n_steps=6, nminibatches=3, noptepochs=2, learning_rate=1e-3, cliprange=0.2, cliprange_vf=-1.0,
                     runner=StubRunner(torch, 24))
    logs = model2.learn(240, callback=lambda loc, glob: seen.append(loc["update"]) or loc["update"] < 2, log_interval=2)
    assert seen == [1, 2] and [log["n_updates"] for log in logs] == [1, 2] and calls[-1][1:4] == (1e-3, 0.2, -1.0)
    with pytest.raises(ValueError):
        qa.PPO2(pol, StubEnv(), n_steps=6, nminibatches=5, runner=runner)
    with pytest.raises(ValueError):
        qa.PPO2(pol, StubEnv(), n_steps=6, nminibatches=3, update="eager", runner=runner)


@pytest.mark.parametrize("layout", ["shared", "towers"])
def test_save_npz_round_trip(tmp_path, layout):
    import torch
    import quadsim_amd as qa
    W = pr.weight_set("he", layout)
    pol = qa.ActorCriticPolicy(W, device="cpu")
    pol.logstd += 0.25                                           # what a trained policy holds is the device tensor
    path = str(tmp_path / "policy.npz")
    pol.save_npz(path)
    back = qa.ActorCriticPolicy.from_npz(path, device="cpu")
    assert back.towers == (layout == "towers")
    for k in pr.keys_of(W):
        assert torch.equal(getattr(back, k), getattr(pol, k)), k
    assert np.array_equal(back.logstd_host, (W["logstd"] + np.float32(0.25)).astype(np.float32))
    with np.load(path) as z:
        assert sorted(z.files) == sorted(pr.keys_of(W))
