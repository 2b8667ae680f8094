"""-m "not gpu": everything of behaviour cloning on the device that needs no device.  include/quadsim_bc.h is plain C99 and every
symbol it declares is exported by libquadsim_bc.so; every refusal the header promises happens before anything is launched, and
check_bc_args mirrors it; tests/bcfit_matrix.py has exactly one row per kernel of the new code object, none uses scratch and each
fits the compute unit's LDS; tests/bcfit_ref.py is checked against torch's float64 autograd and central differences; the host
schedule covers every train row once an epoch; and no fixture of tests/test_gpu_bcfit.py holds a pre-activation within its forward
bound of zero."""
import numpy as np
import pytest

import bcfit_matrix
import bcfit_ref as br
import kernel_notes
import side_cases


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, bc
    _lib.build_library()
    return bc.load_bc()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("bc", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    from quadsim_amd import bc
    side_cases.check_exports("bc", lib, ["qsbc_fit", "qsbc_last_error", "qsbc_loss", "qsbc_loss_blocks", "qsbc_version"])
    assert sorted(bc.BC_EXPORTS) == side_cases.declared("bc")


def test_no_other_library_holds_its_kernels(lib):
    side_cases.check_no_foreign_kernels("bc")


def test_table_entry_names_its_own_files(lib):
    import quadsim_amd as qa
    from quadsim_amd import bc, dynplan
    assert not set(bc.BC_EXPORTS) & (set(dynplan.EXPORTS) | set(dynplan.MPPI_EXPORTS) | set(dynplan.FIT_EXPORTS))
    side_cases.check_entry("bc", ["bcfit_kernels.hpp", "quadsim_bc.h", "quadsim_device.hpp", "side_host.hpp", "train_pieces.hpp"], "bcfit.hip")
    assert [lib.qsbc_loss_blocks(c) for c in (-1, 0, 1, 256, 257, (1 << 31) - 1)] == [0, 0, 1, 1, 2, 1 << 23]
    for name in ("ExpertData", "epoch_schedule", "pretrain", "check_bc_args", "bc_fit", "bc_loss"):
        assert getattr(qa, name) is getattr(bc, name) and name in qa.__all__
    assert bc.BC_MAX_STEPS == dynplan.FIT_MAX_ITERS == 4096 and bc.BC_MAX_BATCH == 256


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_bc.h"

static float x[8192];
static double d[64];
static int32_t idx[64];
static QsbcNet net;
static float *grads[6];
static const float *w[6];

static int refused(int rc, const char *word)
{
    if (rc == QSBC_OK || strstr(qsbc_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qsbc_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int call(int64_t n, int steps, int batch, double lr, double b1, double b2, double eps, int64_t t0)
{
    return qsbc_fit(&net, x, x, n, idx, NULL, steps, batch, lr, b1, b2, eps, t0, x, NULL, NULL);
}

int main(void)
{
    int ok = 1, i;
    void *fns[] = {(void *)qsbc_version, (void *)qsbc_last_error, (void *)qsbc_fit, (void *)qsbc_loss_blocks, (void *)qsbc_loss};
    if (qsbc_version() != QSBC_VERSION) return 2;
    net.struct_size = sizeof net;
    for (i = 0; i < 6; ++i) { net.w[i] = net.m[i] = net.v[i] = x; w[i] = x; grads[i] = x; }
    ok &= refused(call(300, 100, 0, 1e-4, 0.9, 0.999, 1e-8, 0), "batch");
    ok &= refused(call(300, 100, 257, 1e-4, 0.9, 0.999, 1e-8, 0), "batch");
    ok &= refused(call(300, 0, 64, 1e-4, 0.9, 0.999, 1e-8, 0), "steps");
    ok &= refused(call(300, 4097, 64, 1e-4, 0.9, 0.999, 1e-8, 0), "steps");
    ok &= refused(call(0, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0), "n must");
    ok &= refused(call((int64_t)1 << 31, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0), "n must");
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, 0.999, 1e-8, -1), "t0");
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, 0.999, 1e-8, ((int64_t)1 << 31) - 100), "t0");
    ok &= refused(call(300, 100, 64, NAN, 0.9, 0.999, 1e-8, 0), "lr");
    ok &= refused(call(300, 100, 64, INFINITY, 0.9, 0.999, 1e-8, 0), "lr");
    ok &= refused(call(300, 100, 64, 1e-4, 1.0, 0.999, 1e-8, 0), "beta1");
    ok &= refused(call(300, 100, 64, 1e-4, -0.1, 0.999, 1e-8, 0), "beta1");
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, 1.0, 1e-8, 0), "beta2");
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, NAN, 1e-8, 0), "beta2");
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, 0.999, INFINITY, 0), "eps");
    /* every tensor of the net is the same array here: the call is otherwise acceptable, and overlapping tensors are refused */
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0), "overlap");
    net.w[3] = NULL;
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0), "NULL");
    net.w[3] = x;
    net.struct_size = 8;
    ok &= refused(call(300, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0), "struct_size");
    net.struct_size = sizeof net;
    ok &= refused(qsbc_fit(NULL, x, x, 300, idx, NULL, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0, x, NULL, NULL), "NULL");
    ok &= refused(qsbc_fit(&net, x, x, 300, NULL, NULL, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0, x, NULL, NULL), "NULL");
    ok &= refused(qsbc_fit(&net, x, x, 300, idx, NULL, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0, NULL, NULL, NULL), "NULL");
    ok &= refused(qsbc_fit(&net, x, x, 300, idx, NULL, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0, (float *)((char *)x + 2), grads, NULL), "aligned");
    ok &= refused(qsbc_loss(w, x, x, 300, NULL, 0, d, d + 8, 0, NULL), "count");
    ok &= refused(qsbc_loss(w, x, x, 300, NULL, 301, d, d + 8, 0, NULL), "count");
    ok &= refused(qsbc_loss(w, x, x, 300, idx, (int64_t)1 << 31, d, d + 8, 0, NULL), "count");
    ok &= refused(qsbc_loss(w, x, x, 0, NULL, 1, d, d + 8, 0, NULL), "n must");
    ok &= refused(qsbc_loss(w, x, x, 300, NULL, 300, d, d + 8, -1, NULL), "grid");
    ok &= refused(qsbc_loss(w, x, x, 300, NULL, 300, d, d + 8, 65536, NULL), "grid");
    ok &= refused(qsbc_loss(w, x, x, 300, NULL, 300, d, d + 1, 0, NULL), "overlap");
    ok &= refused(qsbc_loss(w, x, x, 300, NULL, 300, NULL, d, 0, NULL), "NULL");
    ok &= refused(qsbc_loss(NULL, x, x, 300, NULL, 300, d, d + 8, 0, NULL), "NULL");
    ok &= refused(qsbc_loss(w, x, x, 300, NULL, 300, (double *)((char *)d + 4), d + 8, 0, NULL), "misaligned");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    side_cases.run_c_caller("bc", C_CALLER, tmp_path)


GOOD = dict(n=300, steps=100, batch=64, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, t0=0)


@pytest.mark.parametrize("kw", [
    dict(batch=0), dict(batch=257), dict(steps=0), dict(steps=4097), dict(n=0), dict(n=1 << 31), dict(t0=-1), dict(t0=(1 << 31) - 100),
    dict(lr=float("nan")), dict(lr=float("inf")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")),
    dict(eps=float("inf")), dict(eps=float("nan")),
    dict(steps=2, batch=3, counts=np.array([0, 3])), dict(steps=2, batch=3, counts=np.array([4, 3])), dict(steps=2, batch=3, counts=np.array([3])),
    dict(steps=2, batch=3, indices=np.array([[0, 1, 2], [3, 300, 5]])), dict(steps=2, batch=3, indices=np.array([[0, -1, 2], [3, 4, 5]])),
    dict(steps=2, batch=3, indices=np.zeros((2, 4), np.int32)),
    dict(steps=2, batch=3, counts=np.array([3, 2]), indices=np.array([[0, 1, 2], [3, 300, 5]]))],
    ids=lambda kw: "-".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_check_bc_args_refuses_before_the_library_is_touched(monkeypatch, kw):
    from quadsim_amd import bc

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(bc, "load_bc", touched)
    assert bc.check_bc_args(**GOOD) == (300, 100, 64, 1e-4, 0.9, 0.999, 1e-8, 0)
    assert bc.check_bc_args((1 << 31) - 1, 4096, 256, 0.0, 0.0, 0.0, 0.0, (1 << 31) - 4097)[0] == (1 << 31) - 1
    # entries at or beyond counts[s] are never read: they may hold anything
    assert bc.check_bc_args(300, 2, 3, counts=np.array([3, 1]), indices=np.array([[0, 1, 299], [3, -7, 1 << 30]]))[1] == 2
    with pytest.raises(ValueError):
        bc.check_bc_args(**dict(GOOD, **kw))


def test_pretrain_refuses_a_host_policy_and_has_no_cpu_path(monkeypatch):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import bc
    monkeypatch.setattr(bc, "load_bc", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    obs, act = br.dataset()
    data = qa.ExpertData({"obs": obs, "actions": act}, device="cpu")
    pol = qa.MlpPolicy(br.weight_set("sb2"), device="cpu")
    with pytest.raises(qa.QuadsimError):
        pol.pretrain(data, n_epochs=1)
    ac = qa.ActorCriticPolicy(dict(np.load(br.GOLDEN)), device="cpu")
    with pytest.raises(qa.QuadsimError):
        ac.pretrain(data, n_epochs=1)
    ac._bc_steps = 5
    ac.reset_pretrain_optimizer()
    assert ac._bc_steps == 0 and ac._bc_m is None
    # the cached images of either class are dropped, whatever they hold
    pol._wt, pol._blob, ac._wt, ac._ac_blob, ac._eval_actor = 1, 2, 3, 4, 5
    bc.drop_cached_images(pol)
    bc.drop_cached_images(ac)
    assert not hasattr(pol, "_wt") and not hasattr(pol, "_blob") and ac._wt is None and ac._ac_blob is None and not hasattr(ac, "_eval_actor")
    assert torch.equal(pol.transposed_weights()[0], pol.w0.t())
    with pytest.raises(TypeError):
        bc.actor_tensors(object())


# ---------------------------------------------------------------------------------------------------- the census
def test_rows_are_exactly_the_kernels_of_the_code_object_without_scratch(notes):
    """no kernel is a template; k_bc_fit, which keeps Adam's state in registers, spills scalar registers"""
    assert {(r["kernel"],) for r in bcfit_matrix.ROWS} == {r["key"] for r in bcfit_matrix.ROWS}
    side_cases.check_census(notes, bcfit_matrix, lambda n: kernel_notes.instantiations_with_types(n, bcfit_matrix.KERNELS, namespace="qsb"), "bcfit",
                            sgpr_spills=("k_bc_fit",))


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(bcfit_matrix)


# ---------------------------------------------------------------------------------------------------- the reference itself
def _torch_loss(torch, W, x, a):
    h = torch.relu(x @ W["w0"] + W["b0"])
    h = torch.relu(h @ W["w1"] + W["b1"])
    return ((h @ W["w2"] + W["b2"] - a) ** 2).mean()


@pytest.mark.parametrize("name", br.STEP_SETS)
def test_backward64_against_torch_float64_autograd(name):
    import torch
    W = br.weight_set(name)
    obs, act = br.dataset()
    rows = br.step_rows(name, 17)[0]
    loss, G = br.backward64(W, obs[rows], act[rows])
    T = {k: torch.tensor(np.asarray(W[k], np.float64), requires_grad=True) for k in br.KEYS}
    lt = _torch_loss(torch, T, torch.tensor(obs[rows].astype(np.float64)), torch.tensor(act[rows].astype(np.float64)))
    lt.backward()
    assert abs(float(lt) - loss) <= 1e-13 * max(1.0, loss)
    for k in br.KEYS:
        g = T[k].grad.numpy()
        assert G[k].shape == br.SHAPES[k] and np.abs(G[k] - g).max() <= 1e-12 * max(1.0, np.abs(g).max()), k


def test_backward64_against_central_differences():
    W = br.weight_set("he")
    obs, act = br.dataset()
    rows = br.step_rows("he", 17)[0]
    x, a = obs[rows], act[rows]
    assert br.relu_edge(W, x, a) == 0
    loss, G = br.backward64(W, x, a)
    assert loss == br.forward64(W, x, a)["loss"]
    rng = np.random.default_rng(5)
    h = 1e-6
    for key in br.KEYS:
        for j in rng.permutation(W[key].size)[:24]:
            P, M = dict(W), dict(W)
            P[key] = W[key].astype(np.float64); M[key] = W[key].astype(np.float64)
            P[key].flat[j] += h; M[key].flat[j] -= h
            num = (br.forward64(P, x, a)["loss"] - br.forward64(M, x, a)["loss"]) / (2 * h)
            # the loss is piecewise quadratic: the central difference is exact up to rounding unless a ReLU flips inside +-h
            assert abs(num - G[key].flat[j]) <= 1e-8 * max(1.0, abs(num)), (key, j, num, G[key].flat[j])


def test_fit64_is_the_loop_of_its_parts_with_counts():
    W = br.weight_set("sb2")
    obs, act = br.dataset()
    idx = br.step_indices(8, steps=3)
    counts = np.array([8, 1, 7])
    Z = br.zero_state()
    W3, M3, V3, L3 = br.fit64(W, Z, Z, obs, act, idx, counts, lr=1e-2)
    Wa, Ma, Va, La = br.fit64(W, Z, Z, obs, act, idx[:2], counts[:2], lr=1e-2)
    Wb, Mb, Vb, Lb = br.fit64(Wa, Ma, Va, obs, act, idx[2:], counts[2:], t0=2, lr=1e-2)
    assert all(np.array_equal(W3[k], Wb[k]) and np.array_equal(V3[k], Vb[k]) for k in br.KEYS)
    assert np.array_equal(L3, np.concatenate([La, Lb])) and np.all(np.isfinite(L3))
    W1 = br.fit64(W, Z, Z, obs, act, idx[:1], counts[:1], lr=1e-2)[0]
    assert L3[1] == br.forward64(W1, obs[idx[1, :1]], act[idx[1, :1]])["loss"]           # step 1 reads its first row alone


def test_adam_formula_at_t_near_2_31():
    """t = 2^31 - 1 is the last step the contract takes: both powers have long underflowed to 0 and lr_t = lr exactly; the update
    is m' / (sqrt(v') + eps) scaled by lr, and adam_bound stays a small multiple of the unit"""
    lr = 1e-4
    t = 2 ** 31 - 1
    assert br.lr_t64(t, lr) == lr and br.lr_t64(1, lr) == lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    rng = np.random.default_rng(7)
    w, g = rng.standard_normal(64).astype(np.float32), (1e-2 * rng.standard_normal(64)).astype(np.float32)
    M, V = br.moments()
    m, v = M["b0"][:64], V["b0"][:64]
    wn, mn, vn = br.adam64(w, m, v, g, t, lr)
    np.testing.assert_allclose(wn, w - lr * mn / (np.sqrt(vn) + 1e-8), rtol=1e-15)
    Ew, Em, Ev = br.adam_bound(w, m, v, g, t, lr)
    assert np.all(Ew > 0) and np.all(Ew < 4 * br.U32 * (np.abs(w) + lr)) and np.all(Em <= 4 * br.U32 * (np.abs(mn) + np.abs(m)) + 1e-30)


# ---------------------------------------------------------------------------------------------------- the ReLU-edge condition
@pytest.mark.parametrize("name", br.STEP_SETS)
def test_no_gpu_fixture_has_a_preactivation_within_its_bound_of_zero(name):
    """grad_bound assumes the device takes the same side of every ReLU as the float64 reference; that is guaranteed only where
    |z| exceeds the forward bound of z.  The allowed share of such elements is zero, for every (weight set, batch) that
    tests/test_gpu_bcfit.py compares with grad_bound"""
    W = br.weight_set(name)
    obs, act = br.dataset()
    assert br.STEP_BATCHES == (1, 15, 16, 17, 64, 256)
    for batch in br.STEP_BATCHES:
        rows = br.step_rows(name, batch)[0]
        assert rows[0] == 0 and (batch < 4 or (rows[1] == br.N_ROWS - 1 and rows[2] == rows[batch - 1])) and rows.max() < br.N_ROWS
        n = br.relu_edge(W, obs[rows], act[rows])
        assert n == 0, "%s, batch %d: %d pre-activations within their bound of zero" % (name, batch, n)
    F = br.forward64(br.weight_set("dead"), obs, act)
    assert (F["z0"] > 0).mean() < 0.3 and (F["z1"] > 0).mean() < 0.3           # "dead": most units inactive


def test_weight_sets_are_what_they_say():
    W = br.weight_set("sb2")
    for k, gain in (("w0", np.sqrt(2.0)), ("w1", np.sqrt(2.0)), ("w2", 0.01)):
        w = W[k].astype(np.float64)
        small = w.T @ w if w.shape[0] >= w.shape[1] else w @ w.T
        np.testing.assert_allclose(small, gain ** 2 * np.eye(small.shape[0]), atol=1e-6)
    assert all(br.weight_set(n)[k].shape == br.SHAPES[k] and br.weight_set(n)[k].dtype == np.float32 for n in br.STEP_SETS for k in br.KEYS)


# ---------------------------------------------------------------------------------------------------- the host schedule
def test_epoch_schedule():
    import torch
    from quadsim_amd import epoch_schedule
    gen = lambda s: torch.Generator().manual_seed(s)     # noqa: E731
    for n_train, batch, epochs in ((210, 64, 3), (128, 64, 2), (10, 64, 4), (7, 1, 2), (257, 256, 1)):
        idx, cnt = epoch_schedule(n_train, batch, epochs, gen(3))
        per = -(-n_train // batch)
        assert idx.dtype == torch.int32 and cnt.dtype == torch.int32 and tuple(idx.shape) == (epochs * per, batch) and tuple(cnt.shape) == (epochs * per,)
        assert idx.device.type == "cpu" and idx.is_contiguous()
        for e in range(epochs):
            c = cnt[e * per:(e + 1) * per]
            assert c[:-1].eq(batch).all() and int(c[-1]) == n_train - (per - 1) * batch and 1 <= int(c[-1]) <= batch
            used = torch.cat([idx[e * per + s, :int(c[s])] for s in range(per)])
            assert torch.equal(torch.sort(used).values, torch.arange(n_train, dtype=torch.int32))     # every row exactly once
        if n_train < batch:
            assert per == 1 and cnt.eq(n_train).all()                                                # one partial batch an epoch
        assert int(idx.min()) >= 0 and int(idx.max()) < n_train
        again = epoch_schedule(n_train, batch, epochs, gen(3))
        assert torch.equal(idx, again[0]) and torch.equal(cnt, again[1])
        if n_train > 1:
            assert not torch.equal(idx, epoch_schedule(n_train, batch, epochs, gen(4))[0])
        # epoch by epoch from one generator: the same schedule
        g = gen(3)
        parts = [epoch_schedule(n_train, batch, 1, g)[0] for _ in range(epochs)]
        assert torch.equal(idx, torch.cat(parts))
    idx, _ = epoch_schedule(210, 64, 2, gen(3))
    assert not torch.equal(idx[:4], idx[4:])                                                         # a fresh shuffle every epoch
    with pytest.raises(ValueError):
        epoch_schedule(0, 64, 1, gen(0))


def test_expert_data_reads_a_dict_and_an_npz(tmp_path):
    import torch
    from quadsim_amd import ExpertData
    obs, act = br.dataset()
    full = {"obs": obs, "actions": act, "rewards": np.zeros(len(obs), np.float32), "episode_returns": np.zeros(3), "episode_starts": np.zeros(len(obs), bool)}
    a = ExpertData(full, device="cpu")
    path = str(tmp_path / "expert.npz")
    np.savez(path, **full)
    b = ExpertData(path, device="cpu")
    assert a.n == b.n == br.N_ROWS and a.batch_size == 64 and a.n_train == int(0.7 * br.N_ROWS) and a.n_val == br.N_ROWS - a.n_train
    assert torch.equal(a.obs, b.obs) and torch.equal(a.actions, b.actions) and torch.equal(a.train_rows, b.train_rows)
    assert np.array_equal(a.obs.numpy(), obs) and np.array_equal(a.actions.numpy(), act)
    both = torch.cat([a.train_rows, a.val_rows])
    assert a.train_rows.dtype == torch.int32 and torch.equal(torch.sort(both).values, torch.arange(br.N_ROWS, dtype=torch.int32))
    assert not set(a.train_rows.tolist()) & set(a.val_rows.tolist())
    c = ExpertData(full, seed=1, train_fraction=0.5, batch_size=10, device="cpu")
    assert not torch.equal(c.train_rows[:100], a.train_rows[:100]) and c.n_train == 150 and c.batch_size == 10
    assert ExpertData(full, train_fraction=1.0, device="cpu").n_val == 0
    for bad in (dict(train_fraction=0.0), dict(batch_size=0), dict(batch_size=257)):
        with pytest.raises(ValueError):
            ExpertData(full, device="cpu", **bad)
    with pytest.raises(ValueError):
        ExpertData({"obs": obs[:, :11], "actions": act}, device="cpu")
