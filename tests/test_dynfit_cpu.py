"""-m "not gpu": everything of the device fit of the learned dynamics net that needs no device.  include/quadsim_dyn_fit.h is
plain C99 and every symbol it declares is exported by libquadsim_dynfit.so; every refusal the header promises happens before
anything is launched; tests/dynfit_matrix.py has exactly one row per kernel instantiation of the new code object, none uses
scratch and each fits the compute unit's LDS; tests/dynfit_ref.py is checked against finite differences and closed forms; and
no fixture of tests/test_gpu_dynfit.py holds a pre-activation within its forward bound of zero; on the width-edge fixtures a
gradient slot of the last unit of either hidden layer that was left at zero would be out of bound."""
import re

import numpy as np
import pytest

import dynfit_matrix
import dynfit_ref as fr
import dynplan_ref as dr
import kernel_notes
import side_cases


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, dynplan
    _lib.build_library()
    return dynplan.load_fit()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("dynfit", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    from quadsim_amd import dynplan
    side_cases.check_exports("dynfit", lib, ["qsdf_fit", "qsdf_last_error", "qsdf_version"])
    assert sorted(dynplan.FIT_EXPORTS) == side_cases.declared("dynfit")
    assert not set(dynplan.FIT_EXPORTS) & (set(dynplan.EXPORTS) | set(dynplan.MPPI_EXPORTS))


def test_table_entry_names_its_own_files():
    side_cases.check_entry("dynfit", ["dynfit_kernels.hpp", "quadsim_device.hpp", "quadsim_dyn_fit.h", "side_host.hpp", "train_pieces.hpp"], "dynfit.hip")


def test_no_other_library_holds_its_kernels(lib):
    side_cases.check_no_foreign_kernels("dynfit")


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_dyn_fit.h"

static float x[64];
static QsdfNet net;

static int refused(int rc, const char *word)
{
    if (rc == QSDF_OK || strstr(qsdf_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qsdf_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int call(int h1, int h2, int64_t capacity, int64_t size, int iters, int batch, double lr, double b1, double b2, double eps,
                int64_t t0, uint64_t k)
{
    net.h1 = h1; net.h2 = h2;
    return qsdf_fit(&net, x, x, capacity, size, iters, batch, lr, b1, b2, eps, t0, 1, k, NULL, x, NULL, NULL, NULL);
}

int main(void)
{
    int ok = 1, i;
    void *fns[] = {(void *)qsdf_version, (void *)qsdf_last_error, (void *)qsdf_fit};
    if (qsdf_version() != QSDF_VERSION) return 2;
    net.struct_size = sizeof net;
    for (i = 0; i < 6; ++i) net.w[i] = net.m[i] = net.v[i] = x;
    net.in_mean = net.in_rscale = net.out_mean = net.out_rscale = x;
    ok &= refused(call(209, 100, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "hidden widths");
    ok &= refused(call(200, 113, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "hidden widths");
    ok &= refused(call(0, 10, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "hidden widths");
    ok &= refused(call(200, 100, 300, 257, 100, 0, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "batch");
    ok &= refused(call(200, 100, 300, 257, 100, 257, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "batch");
    ok &= refused(call(200, 100, 300, 257, 0, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "iters");
    ok &= refused(call(200, 100, 300, 257, 4097, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "iters");
    ok &= refused(call(200, 100, 300, 0, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "size");
    ok &= refused(call(200, 100, 300, 301, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "size");
    ok &= refused(call(200, 100, (int64_t)1 << 31, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "capacity");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, -1, 0), "t0");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, ((int64_t)1 << 31) - 100, 0), "t0");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, (uint64_t)1 << 48), "k must");
    ok &= refused(call(200, 100, 300, 257, 100, 128, NAN, 0.9, 0.999, 1e-8, 0, 0), "lr");
    ok &= refused(call(200, 100, 300, 257, 100, 128, INFINITY, 0.9, 0.999, 1e-8, 0, 0), "lr");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 1.0, 0.999, 1e-8, 0, 0), "beta1");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, -0.1, 0.999, 1e-8, 0, 0), "beta1");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, 1.0, 1e-8, 0, 0), "beta2");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, NAN, 1e-8, 0, 0), "beta2");
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, 0.999, INFINITY, 0, 0), "eps");
    net.w[3] = NULL;
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "NULL");
    net.w[3] = x;
    net.struct_size = 8;
    ok &= refused(call(200, 100, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0), "struct_size");
    net.struct_size = sizeof net;
    ok &= refused(qsdf_fit(NULL, x, x, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 1, 0, NULL, x, NULL, NULL, NULL), "NULL");
    ok &= refused(qsdf_fit(&net, x, x, 300, 257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 1, 0, NULL, NULL, NULL, NULL, NULL), "NULL");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    side_cases.run_c_caller("dynfit", C_CALLER, tmp_path)


GOOD = dict(h1=200, h2=100, capacity=300, size=257, iters=100, batch=128, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, t0=0, seed=0, k=0)


@pytest.mark.parametrize("kw", [
    dict(h1=209), dict(h2=113), dict(h1=129, h2=128), dict(h1=0), dict(batch=0), dict(batch=257), dict(iters=0), dict(iters=4097),
    dict(size=0), dict(size=301), dict(capacity=1 << 31, size=1), dict(capacity=0), dict(t0=-1), dict(t0=(1 << 31) - 100),
    dict(lr=float("nan")), dict(lr=float("inf")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")),
    dict(eps=float("inf")), dict(eps=float("nan")), dict(seed=1 << 64), dict(seed=-1), dict(k=1 << 48), dict(k=-1)],
    ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_check_fit_args_refuses_before_the_library_is_touched(monkeypatch, kw):
    from quadsim_amd import dynplan

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(dynplan, "load_fit", touched)
    assert dynplan.check_fit_args(**GOOD) == (257, 100, 128, 1e-4, 0.9, 0.999, 1e-8, 0, 0, 0)
    assert dynplan.check_fit_args(208, 112, (1 << 31) - 1, (1 << 31) - 1, 4096, 256, 0.0, 0.0, 0.0, 0.0, (1 << 31) - 4097, (1 << 64) - 1,
                                  (1 << 48) - 1)[0] == (1 << 31) - 1
    with pytest.raises(ValueError):
        dynplan.check_fit_args(**dict(GOOD, **kw))


def test_fit_refuses_bad_tensors_and_has_no_cpu_path(monkeypatch):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import dynplan
    monkeypatch.setattr(dynplan, "load_fit", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    net = dr.to_net(dr.weight_set("he_20_10"), "cpu")
    assert net.adam_m is None and net.adam_v is None and net.fit_steps == 0
    assert net.out_rscale.dtype == torch.float32 and np.array_equal(net.out_rscale.numpy(), fr.out_rscale(dr.weight_set("he_20_10")))
    with pytest.raises(qa.QuadsimError):
        net.fit(torch.zeros(300, 16), torch.zeros(300, 12), 257)
    assert qa.check_fit_args is dynplan.check_fit_args
    net.fit_steps = 5
    net.reset_optimizer()
    assert net.fit_steps == 0 and net.adam_m is None


# ---------------------------------------------------------------------------------------------------- the census
def test_rows_are_exactly_the_kernels_of_the_code_object_without_scratch(notes):
    """every kernel is the template in namespace qsf; it keeps Adam's state in registers and spills scalar registers"""
    from quadsim_amd import dynplan
    keys = [r["key"] for r in dynfit_matrix.ROWS]
    side_cases.check_census(notes, dynfit_matrix, lambda n: kernel_notes.instantiations_with_types(n, dynfit_matrix.KERNELS, namespace="qsf"), "dynfit",
                            sgpr_spills=("k_dyn_fit",))
    assert {k[1:] for k in keys} == set(dynplan.COMPILED_WIDTHS) == {r["widths"] for r in dynfit_matrix.ROWS}
    assert {len(k) for k in keys} == {3} and {r["block"] for r in dynfit_matrix.ROWS} == {512}


def test_rows_name_a_net_of_exactly_their_widths():
    """a row's `widths` are the hidden widths of the net its test id names (the widest the instantiation takes)"""
    for r in dynfit_matrix.ROWS:
        W = dr.weight_set(re.search(r"\[(\w+)\]$", r["test"]).group(1))
        assert (W["w1"].shape[0], W["w2"].shape[0]) == r["widths"] == r["key"][1:], r


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(dynfit_matrix)


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_backward64_against_central_differences():
    W = dr.weight_set("he_20_10")
    bx, bd = fr.buffer()
    rows = fr.step_indices(17)[0]
    x, d = bx[rows], bd[rows]
    assert fr.relu_edge(W, x, d) == 0
    loss, G = fr.backward64(W, x, d)
    assert loss == fr.forward64(W, x, d)["loss"]
    rng = np.random.default_rng(5)
    h = 1e-6
    for key in fr.GRAD_KEYS:
        flat = rng.permutation(W[key].size)[:24]
        for j in flat:
            P, M = dict(W), dict(W)
            P[key] = W[key].astype(np.float64); M[key] = W[key].astype(np.float64)
            P[key].flat[j] += h; M[key].flat[j] -= h
            num = (fr.forward64(P, x, d)["loss"] - fr.forward64(M, x, d)["loss"]) / (2 * h)
            # the loss is piecewise quadratic: the central difference is exact up to rounding unless a ReLU flips inside +-h
            assert abs(num - G[key].flat[j]) <= 1e-8 * max(1.0, abs(num)), (key, j, num, G[key].flat[j])


def test_adam64_first_step_is_the_closed_form():
    rng = np.random.default_rng(6)
    g = rng.standard_normal(50) * 10.0 ** rng.integers(-6, 2, 50)
    w = rng.standard_normal(50)
    lr, b2, eps = 1e-2, 0.999, 1e-8
    wn, m, v = fr.adam64(w, np.zeros(50), np.zeros(50), g, 1, lr)
    np.testing.assert_allclose(wn - w, -lr * g / (np.abs(g) + eps / np.sqrt(1.0 - b2)), rtol=1e-12, atol=0)
    np.testing.assert_allclose(m, 0.1 * g, rtol=1e-15)
    np.testing.assert_allclose(v, 0.001 * g * g, rtol=1e-12)
    Ew, Em, Ev = fr.adam_bound(w.astype(np.float32), np.zeros(50), np.zeros(50), g.astype(np.float32), 1, lr)
    assert np.all(Ew > 0) and np.all(Ew < 1e-5 * lr + 2e-7 * np.abs(w) + 1e-30) and np.all(Em <= 4 * fr.U32 * np.abs(m) + 1e-30)


def test_indices_in_range_repeatable_and_prefix():
    for size in (1, 257, (1 << 31) - 1):
        a = fr.indices(3, 2, 5, 256, size)
        assert a.dtype == np.int32 and a.min() >= 0 and a.max() < size
        assert np.array_equal(a, fr.indices(3, 2, 5, 256, size))
        assert np.array_equal(a[:17], fr.indices(3, 2, 5, 17, size))
    a = fr.indices(3, 2, 5, 256, 257)
    assert len(np.unique(a)) > 100 and len(np.unique(a)) < 256          # spread over the buffer, drawn with replacement
    for other in (fr.indices(4, 2, 5, 256, 257), fr.indices(3, 3, 5, 256, 257), fr.indices(3, 2, 6, 256, 257)):
        assert not np.array_equal(a, other)


def test_fit64_is_the_loop_of_its_parts_and_learns():
    W = dr.weight_set("he_20_10")
    bx, bd = fr.buffer()
    idx = np.stack([fr.indices(1, 0, t, 32, fr.SIZE) for t in range(3)])
    Z = fr.zero_state(W)
    W3, M3, V3, L3 = fr.fit64(W, Z, Z, bx, bd, idx, lr=1e-2)
    Wa, Ma, Va, La = fr.fit64(W, Z, Z, bx, bd, idx[:2], lr=1e-2)
    Wb, Mb, Vb, Lb = fr.fit64(Wa, Ma, Va, bx, bd, idx[2:], t0=2, lr=1e-2)
    assert all(np.array_equal(W3[k], Wb[k]) and np.array_equal(V3[k], Vb[k]) for k in fr.GRAD_KEYS)
    assert np.array_equal(L3, np.concatenate([La, Lb])) and np.all(np.isfinite(L3))
    loss, G = fr.backward64(W, bx[idx[0]], bd[idx[0]])
    W1 = fr.fit64(W, Z, Z, bx, bd, idx[:1], lr=1e-2)[0]
    assert L3[0] == loss and all(np.array_equal(W1[k], fr.adam64(W[k], Z[k], Z[k], G[k], 1, 1e-2)[0]) for k in fr.GRAD_KEYS)


# ---------------------------------------------------------------------------------------------------- the ReLU-edge condition
@pytest.mark.parametrize("name", fr.STEP_SETS + fr.EDGE_SETS)
def test_no_gpu_fixture_has_a_preactivation_within_its_bound_of_zero(name):
    """grad_bound assumes the device takes the same side of every ReLU as the float64 reference; that is guaranteed only where
    |z| exceeds the forward bound of z.  The allowed share of such elements is zero: every (weight set, batch) that
    tests/test_gpu_dynfit.py compares with grad_bound is checked here, the width edges with their batches included"""
    W = dr.weight_set(name)
    bx, bd = fr.buffer()
    assert fr.step_batches(name) == (fr.EDGE_BATCHES if name.startswith("edge_") else fr.STEP_BATCHES)
    for batch in fr.step_batches(name):
        rows = fr.step_rows(name, batch)[0]
        assert rows[0] == 0 and (batch < 4 or (rows[1] == fr.SIZE - 1 and rows[2] == rows[batch - 1]))
        assert rows.max() < fr.SIZE
        n = fr.relu_edge(W, bx[rows], bd[rows])
        assert n == 0, "%s, batch %d: %d pre-activations within their bound of zero" % (name, batch, n)


# ---------------------------------------------------------------------------------------------------- the width edges
def test_check_fit_args_accepts_every_edge_width():
    from quadsim_amd import dynplan
    for (h1, h2), compiled in dr.EDGE_WIDTHS.items():
        assert dynplan.check_fit_args(**dict(GOOD, h1=h1, h2=h2, batch=max(fr.EDGE_BATCHES)))[2] == 128
        assert dynplan.check_widths(h1, h2)[2] == compiled
    assert fr.EDGE_BATCHES == (1, 17, 128) and fr.EDGE_SETS == dr.EDGE_SETS and not set(fr.EDGE_SETS) & set(fr.STEP_SETS)


@pytest.mark.parametrize("name", fr.EDGE_SETS)
def test_edge_fixture_detects_an_unowned_gradient_slot(name):
    """for every batch of the edge sets, the float64 gradient exceeds its grad_bound on at least one element of each slice that
    only the last unit of a hidden layer reaches: a kernel that left those slots at zero could not pass.  The float32
    restatement of the whole gradient stays inside the bounds on the same rows."""
    W = dr.weight_set(name)
    bx, bd = fr.buffer()
    for batch in fr.EDGE_BATCHES:
        rows = fr.step_rows(name, batch)[0]
        x, d = bx[rows], bd[rows]
        loss, G, lb, E = fr.backward64(W, x, d, with_bound=True)
        ratios = []
        for label, (key, at) in fr.last_unit_slices(W).items():
            r = np.abs(G[key][at]) / E[key][at]
            ratios.append(float(r.max()))
            assert (r > 1.0).any(), "%s, batch %d: %s is within its bound of zero everywhere (worst %.3g)" % (name, batch, label, r.max())
        loss32, G32 = fr._backward_as(W, x, d, np.float32)
        worst = max(float((np.abs(G32[key].astype(np.float64) - G[key]) / E[key]).max()) for key in fr.GRAD_KEYS)
        print("dynfit edge %s batch %d |gradient| / bound of the last unit's slices %s; float32 restatement err/bound %.3g, loss %.3g" % (
            name, batch, " ".join("%.3g" % r for r in ratios), worst, abs(loss32 - loss) / lb))
        assert worst < 1.0 and abs(loss32 - loss) <= lb
