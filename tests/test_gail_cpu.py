"""-m "not gpu": everything of GAIL on the device that needs no device.  include/quadsim_gail.h is plain C99 and every symbol it
declares is exported by libquadsim_gail.so; the table entry of _lib.SIDE matches the header's prototypes; every refusal the
header promises happens before anything is launched, and check_gail_args mirrors it; tests/gail_matrix.py has exactly one row per
kernel instantiation of the new code object, none uses scratch and each fits the compute unit's LDS; tests/gail_ref.py is checked
against torch's float64 autograd, which it shares no code with; the schedule and the running statistics hold their properties;
and the recorded instruction diff of the other six libraries says `same` for every kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gail_matrix
import gail_ref as gr
import kernel_notes
import side_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, gail
    _lib.build_library()
    return gail.load_gail()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("gail", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    side_cases.check_exports("gail", lib, ["qsg_fit", "qsg_last_error", "qsg_math", "qsg_reward", "qsg_version"])


def test_table_entry_names_its_own_files():
    import quadsim_amd as qa
    from quadsim_amd import _lib, gail
    assert gail.GAIL_EXPORTS is _lib.SIDE["gail"]["exports"]
    side_cases.check_entry("gail", ["gail_kernels.hpp", "quadsim_device.hpp", "quadsim_gail.h", "side_host.hpp", "train_pieces.hpp"], "gail.hip")
    for name in ("GAIL", "Discriminator", "GailRunner", "discriminator_schedule", "torch_discriminator_fit", "check_gail_args"):
        assert getattr(qa, name) is getattr(gail, name) and name in qa.__all__
    assert gail.GAIL_MAX_STEPS == 4096 and gail.GAIL_MAX_BATCH == 256 and gail.GAIL_MAX_HIDDEN == 128
    assert [gail.compiled_width(h) for h in (1, 64, 65, 100, 128)] == [64, 64, 128, 128, 128]


def test_no_other_library_holds_its_kernels(lib):
    side_cases.check_no_foreign_kernels("gail")


def test_table_entry_matches_the_header():
    """the struct; the prototypes are held by tests/test_call_path_cpu.py, for every side library"""
    from quadsim_amd import _lib
    # the struct: two 32-bit fields, eighteen tensors, mean and rscale
    assert C.sizeof(_lib.QsgNet) == 8 + 20 * 8 and _lib.QsgNet.mean.offset == 8 + 18 * 8


C_CALLER = r"""
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "quadsim_gail.h"

static float x[8192], y[8192], big[200000];
static int32_t idx[64];
static QsgNet net;
static float *grads[6];

static int refused(int rc, const char *word)
{
    if (rc == QSG_OK || strstr(qsg_last_error(), word) == NULL) { printf("NOT-REFUSED:%s (%d: %s)\n", word, rc, qsg_last_error()); return 0; }
    return 1;
}

/* the call with one thing changed; everything else is acceptable, so a refusal names what was changed */
static int fit(int64_t ng, int64_t ne, int steps, int batch, double ent, double lr, double b1, double b2, double eps, int64_t t0)
{
    return qsg_fit(&net, x, x, ng, x, x, ne, idx, idx, NULL, steps, batch, ent, lr, b1, b2, eps, t0, y, NULL, NULL);
}

static void distinct(void)
{
    /* eighteen tensors of a net of H = 100 that do not overlap: 10000 floats apart in `big` */
    int i;
    for (i = 0; i < 6; ++i) { net.w[i] = big + 10000 * i; net.m[i] = big + 10000 * (6 + i); net.v[i] = big + 10000 * (12 + i); }
}

int main(void)
{
    int ok = 1, i;
    void *fns[] = {(void *)qsg_version, (void *)qsg_last_error, (void *)qsg_fit, (void *)qsg_reward, (void *)qsg_math};
    if (qsg_version() != QSG_VERSION) return 2;
    net.struct_size = sizeof net;
    net.hidden = 100;
    net.mean = net.rscale = x;
    distinct();
    for (i = 0; i < 6; ++i) grads[i] = big + 10000 * 18 + 1000 * i;
    ok &= refused(fit(300, 200, 100, 0, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "batch");
    ok &= refused(fit(300, 200, 100, 257, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "batch");
    ok &= refused(fit(300, 200, 0, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "steps");
    ok &= refused(fit(300, 200, 4097, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "steps");
    ok &= refused(fit(0, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "n_gen");
    ok &= refused(fit((int64_t)1 << 31, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "n_gen");
    ok &= refused(fit(300, 0, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "n_exp");
    ok &= refused(fit(300, (int64_t)1 << 31, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "n_exp");
    ok &= refused(fit(300, 200, 100, 64, NAN, 3e-4, 0.9, 0.999, 1e-8, 0), "entcoeff");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, -1), "t0");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, ((int64_t)1 << 31) - 100), "t0");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, NAN, 0.9, 0.999, 1e-8, 0), "lr");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, INFINITY, 0.9, 0.999, 1e-8, 0), "lr");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 1.0, 0.999, 1e-8, 0), "beta1");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, -0.1, 0.999, 1e-8, 0), "beta1");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 1.0, 1e-8, 0), "beta2");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, NAN, 1e-8, 0), "beta2");
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, INFINITY, 0), "eps");
    net.hidden = 0;
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "hidden");
    net.hidden = 129;
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "hidden");
    net.hidden = 100;
    /* two tensors of the net one float short of disjoint, then stats inside a moment, then a gradient on a weight */
    net.m[2] = net.w[2] + 9999;
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "overlap");
    distinct();
    ok &= refused(qsg_fit(&net, x, x, 300, x, x, 200, idx, idx, NULL, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0, net.v[0] + 8, NULL, NULL), "overlap");
    grads[4] = net.w[4];
    ok &= refused(qsg_fit(&net, x, x, 300, x, x, 200, idx, idx, NULL, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0, y, grads, NULL), "overlap");
    grads[4] = big + 10000 * 18 + 4000;
    net.w[3] = NULL;
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "NULL");
    distinct();
    net.v[5] = (float *)((char *)net.v[5] + 2);
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "aligned");
    distinct();
    net.mean = NULL;
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "mean");
    net.mean = x;
    net.struct_size = 8;
    ok &= refused(fit(300, 200, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0), "struct_size");
    net.struct_size = sizeof net;
    ok &= refused(qsg_fit(NULL, x, x, 300, x, x, 200, idx, idx, NULL, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0, y, NULL, NULL), "NULL");
    ok &= refused(qsg_fit(&net, x, x, 300, x, x, 200, NULL, idx, NULL, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0, y, NULL, NULL), "NULL");
    ok &= refused(qsg_fit(&net, x, x, 300, x, x, 200, idx, idx, NULL, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0, NULL, NULL, NULL), "NULL");
    ok &= refused(qsg_fit(&net, x, x, 300, x, x, 200, idx, idx, NULL, 100, 64, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0, (float *)((char *)y + 2), grads, NULL), "aligned");
    /* the reward */
    ok &= refused(qsg_reward(&net, x, x, 0, 0, 0, y, NULL, 0, NULL), "rows");
    ok &= refused(qsg_reward(&net, x, x, (int64_t)1 << 31, 0, 0, y, NULL, 0, NULL), "rows");
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 4, y, NULL, 0, NULL), "n_envs");
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 0, y, NULL, 0, NULL), "n_envs");
    ok &= refused(qsg_reward(&net, x, x, 15, -3, -5, y, NULL, 0, NULL), "n_envs");
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 5, y, NULL, -1, NULL), "grid");
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 5, y, NULL, 65536, NULL), "grid");
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 5, y, y + 14, 0, NULL), "overlap");
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 5, NULL, NULL, 0, NULL), "NULL");
    ok &= refused(qsg_reward(NULL, x, x, 15, 3, 5, y, NULL, 0, NULL), "NULL");
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 5, (float *)((char *)y + 2), NULL, 0, NULL), "aligned");
    net.w[0] = NULL;
    ok &= refused(qsg_reward(&net, x, x, 15, 3, 5, y, NULL, 0, NULL), "NULL");
    distinct();
    ok &= refused(qsg_math(5, x, y, 10, NULL), "kind");
    ok &= refused(qsg_math(0, x, y, 0, NULL), "n must");
    ok &= refused(qsg_math(0, NULL, y, 10, NULL), "NULL");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone.  Every call it makes is one the library
    refuses, with host pointers it would never dereference: each returns before anything is launched"""
    side_cases.run_c_caller("gail", C_CALLER, tmp_path)


GOOD = dict(n_gen=300, n_exp=200, steps=100, batch=64, hidden=100, entcoeff=1e-3, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, t0=0)


@pytest.mark.parametrize("kw", [
    dict(batch=0), dict(batch=257), dict(steps=0), dict(steps=4097), dict(n_gen=0), dict(n_gen=1 << 31), dict(n_exp=0), dict(n_exp=1 << 31),
    dict(hidden=0), dict(hidden=129), dict(entcoeff=float("nan")), dict(entcoeff=float("inf")), dict(t0=-1), dict(t0=(1 << 31) - 100),
    dict(lr=float("nan")), dict(lr=float("inf")), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")),
    dict(eps=float("inf")), dict(eps=float("nan")),
    dict(steps=2, batch=3, counts=np.array([0, 3])), dict(steps=2, batch=3, counts=np.array([4, 3])), dict(steps=2, batch=3, counts=np.array([3])),
    dict(steps=2, batch=3, gen_idx=np.array([[0, 1, 2], [3, 300, 5]])), dict(steps=2, batch=3, exp_idx=np.array([[0, 1, 2], [3, 200, 5]])),
    dict(steps=2, batch=3, gen_idx=np.array([[0, -1, 2], [3, 4, 5]])), dict(steps=2, batch=3, exp_idx=np.zeros((2, 4), np.int32)),
    dict(steps=2, batch=3, counts=np.array([3, 2]), exp_idx=np.array([[0, 1, 2], [3, 200, 5]]))],
    ids=lambda kw: "-".join("%s=%s" % (k, getattr(v, "shape", v)) for k, v in kw.items()))
def test_check_gail_args_refuses_before_the_library_is_touched(monkeypatch, kw):
    from quadsim_amd import gail

    def touched(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(gail, "load_gail", touched)
    assert gail.check_gail_args(**GOOD) == (300, 200, 100, 64, 100, 1e-3, 3e-4, 0.9, 0.999, 1e-8, 0)
    assert gail.check_gail_args((1 << 31) - 1, (1 << 31) - 1, 4096, 256, 128, 0.0, 0.0, 0.0, 0.0, 0.0, (1 << 31) - 4097)[0] == (1 << 31) - 1
    # entries at or beyond counts[s] are never read: they may hold anything
    assert gail.check_gail_args(300, 200, 2, 3, counts=np.array([3, 1]), gen_idx=np.array([[0, 1, 299], [3, -7, 1 << 30]]),
                                exp_idx=np.array([[0, 1, 199], [3, 1 << 30, -1]]))[2] == 2
    with pytest.raises(ValueError):
        gail.check_gail_args(**dict(GOOD, **kw))


@pytest.mark.parametrize("kw", [dict(rows=0), dict(rows=1 << 31), dict(rows=15, n_envs=3), dict(rows=15, n_envs=3, n_steps=4),
                                dict(rows=15, n_envs=0, n_steps=5), dict(rows=15, n_envs=-3, n_steps=-5), dict(rows=15, grid=-1),
                                dict(rows=15, grid=65536)], ids=str)
def test_check_reward_args(kw):
    from quadsim_amd import gail
    assert gail.check_reward_args(15) == gail.check_reward_args(15, 0, 0) == (15, 0, 0, 0) and gail.check_reward_args(15, 3, 5, 7) == (15, 3, 5, 7)
    with pytest.raises(ValueError):
        gail.check_reward_args(**kw)


def test_squashed_policies_and_host_discriminators_are_refused(monkeypatch):
    import torch
    import quadsim_amd as qa
    from quadsim_amd import gail
    monkeypatch.setattr(gail, "load_gail", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))

    class Squashed:
        squash = True

    class Env:
        num_envs, device = 4, torch.device("cpu")

    class Expert:
        obs, actions = torch.zeros((50, 12)), torch.zeros((50, 4))
    with pytest.raises(ValueError, match="squash"):
        qa.GAIL(Squashed(), Env(), Expert(), n_steps=16)
    with pytest.raises(ValueError, match="update"):
        qa.GAIL(object(), Env(), Expert(), n_steps=16, update="jax")
    with pytest.raises(ValueError, match="d_batch"):
        qa.GAIL(object(), Env(), Expert(), n_steps=16, d_batch=65)
    d = qa.Discriminator(hidden=10, device="cpu")
    with pytest.raises(qa.QuadsimError):
        d.reward(torch.zeros((3, 12)), torch.zeros((3, 4)))
    idx = torch.zeros((1, 2), dtype=torch.int32)
    with pytest.raises(qa.QuadsimError):
        d.fit(torch.zeros((3, 12)), torch.zeros((3, 4)), Expert(), idx, idx)
    with pytest.raises(ValueError):
        qa.Discriminator(hidden=129, device="cpu")
    with pytest.raises(ValueError):
        qa.torch_discriminator_fit(d, torch.zeros((3, 12)), torch.zeros((3, 4)), Expert(), idx + 3, idx)


# ---------------------------------------------------------------------------------------------------- the census
def test_rows_are_exactly_the_kernels_of_the_code_object_without_scratch(notes):
    """k_gail_fit, which keeps Adam's state in registers, spills scalar registers"""
    side_cases.check_census(notes, gail_matrix, lambda n: kernel_notes.instantiations_with_types(n, gail_matrix.KERNELS, namespace="qsg"), "gail",
                            sgpr_spills=("k_gail_fit",))


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(gail_matrix)


def test_the_other_six_libraries_are_instruction_identical():
    """profiles/gail/isa_diff.txt is the output of tools/isa_diff.py, the parent commit's build against this one, for each of
    the other six libraries: every kernel line says `same`.  None of them can have moved: no file they are built from belongs to
    this library (held above)"""
    text = open(os.path.join(ROOT, "profiles", "gail", "isa_diff.txt")).read()
    libs = re.findall(r"^## (\S+)$", text, flags=re.M)
    assert libs == ["libquadsim_hip.so", "libquadsim_dyn.so", "libquadsim_dynmppi.so", "libquadsim_dynfit.so", "libquadsim_bc.so",
                    "libquadsim_ppo.so"]
    lines = [ln for ln in text.splitlines() if re.match(r"^_Z\S+: ", ln)]
    assert len(lines) > 100 and all(ln.endswith(": same") for ln in lines)
    totals = re.findall(r"^identical in fields and disassembly: (\d+) of (\d+)$", text, flags=re.M)
    assert len(totals) == 6 and all(a == b for a, b in totals)
    assert not re.findall(r"only in (?:parent|branch) \[[^\]]+\]", text)


# ---------------------------------------------------------------------------------------------------- the reference itself
def _torch_total(torch, P, x, c, entcoeff):
    F = torch.nn.functional
    l = (torch.tanh(torch.tanh(x @ P["w0"] + P["b0"]) @ P["w1"] + P["b1"]) @ P["w2"] + P["b2"])[:, 0]
    gen = F.binary_cross_entropy_with_logits(l[:c], torch.zeros(c, dtype=l.dtype))
    exp = F.binary_cross_entropy_with_logits(l[c:], torch.ones(c, dtype=l.dtype))
    s = torch.sigmoid(l)
    ent = -(s * torch.log(s) + (1 - s) * torch.log(1 - s)).mean()
    return gen + exp - entcoeff * ent, (gen, exp, ent)


@pytest.mark.parametrize("entcoeff", [1e-3, 0.5])
@pytest.mark.parametrize("hidden", gr.HIDDENS)
def test_backward64_against_torch_float64_autograd(hidden, entcoeff):
    """loss and gradient to 1e-12 relative, against code the restatement does not share; the entropy there is the textbook
    -(s log s + (1 - s) log(1 - s)), which logit_bernoulli_entropy must equal"""
    import torch
    W = gr.weights(hidden)
    gen, exp, mean, rscale = gr.dataset()
    gi, ei = gr.step_indices(17)
    g, e = (gen[0][gi[0]], gen[1][gi[0]]), (exp[0][ei[0]], exp[1][ei[0]])
    stats, G = gr.backward64(W, g, e, mean, rscale, entcoeff)
    x = np.concatenate([np.concatenate([(np.float64(o) - np.float64(mean)) * np.float64(rscale), np.clip(np.float64(a), -1, 1)], 1)
                        for o, a in (g, e)])
    P = {k: torch.tensor(np.asarray(W[k], np.float64), requires_grad=True) for k in gr.KEYS}
    total, parts = _torch_total(torch, P, torch.tensor(x), 17, entcoeff)
    total.backward()
    for got, want in zip(stats[:3], parts):
        assert abs(got - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    for k in gr.KEYS:
        t = P[k].grad.numpy()
        assert G[k].shape == np.asarray(W[k]).shape and np.abs(G[k] - t).max() <= 1e-12 * max(1.0, np.abs(t).max()), k


def test_entropy_softplus_and_reward_formulas():
    l = np.concatenate([np.linspace(-30, 30, 601), [0.0, 1e-9, -1e-9]])
    s = 1.0 / (1.0 + np.exp(-l))
    h = gr.sigmoid(-l) * l + gr.softplus(-l)
    with np.errstate(divide="ignore", invalid="ignore"):
        text = -(s * np.log(s) + (1 - s) * np.log1p(-s))
    ok = np.isfinite(text)
    # (both forms cancel at large |l|: 30 (1 - s) against 30 leaves 30 x 2^-53 absolute)
    np.testing.assert_allclose(h[ok], text[ok], rtol=1e-9, atol=2e-14)
    np.testing.assert_allclose(gr.softplus(l), np.log1p(np.exp(l)), rtol=1e-13)
    np.testing.assert_allclose(gr.sigmoid(l) + gr.sigmoid(-l), 1.0, rtol=1e-15)
    # the kernel's form of the reward is the reference's in exact arithmetic
    q = 1.0 / (1.0 + np.exp(l))
    np.testing.assert_allclose(-np.log(q + 1e-8), gr.reward64(l), rtol=0, atol=3e-8)
    assert abs(gr.reward64(100.0) + np.log(1e-8)) < 1e-7 and abs(gr.reward64(-100.0)) < 2e-8


def test_fit64_is_the_loop_of_its_parts_with_counts():
    W = gr.weights(64)
    Z = gr.zero_state(W)
    gen, exp, mean, rscale = gr.dataset()
    gi, ei = gr.step_indices(8, steps=3)
    counts = np.array([8, 1, 7])
    W3, M3, V3, S3 = gr.fit64(W, Z, Z, gen, exp, gi, ei, mean, rscale, counts, lr=1e-2)
    Wa, Ma, Va, Sa = gr.fit64(W, Z, Z, gen, exp, gi[:2], ei[:2], mean, rscale, counts[:2], lr=1e-2)
    Wb, Mb, Vb, Sb = gr.fit64(Wa, Ma, Va, gen, exp, gi[2:], ei[2:], mean, rscale, counts[2:], t0=2, lr=1e-2)
    assert all(np.array_equal(W3[k], Wb[k]) and np.array_equal(V3[k], Vb[k]) for k in gr.KEYS)
    assert np.array_equal(S3, np.concatenate([Sa, Sb])) and np.all(np.isfinite(S3))


def test_the_separable_case_is_learnt_in_float64():
    gen, exp, mean, rscale, gi, ei = gr.separable_case()
    W = gr.weights(gr.LEARN_HIDDEN, bias=0.0)
    Z = gr.zero_state(W)
    st = gr.fit64(W, Z, Z, gen, exp, gi, ei, mean, rscale, lr=gr.LEARN_LR)[3]
    total = st[:, 0] + st[:, 1] - gr.ENTCOEFF * st[:, 2]
    assert st[-1, 3] == 1.0 and st[-1, 4] == 1.0 and total[-1] < 0.1 * total[0]


def test_bounds_hold_for_a_float32_emulation_in_another_summation_order():
    """numpy's own float32 products of the same step (another summation order, numpy's tanh and exp) stay within the derived
    bounds: the bounds are not empty, and not so tight that only the device's order meets them"""
    f = np.float32
    W = gr.weights(100)
    gen, exp, mean, rscale = gr.dataset()
    gi, ei = gr.step_indices(33)
    g, e = (gen[0][gi[0]], gen[1][gi[0]]), (exp[0][ei[0]], exp[1][ei[0]])
    stats, G, Es, E = gr.backward64(W, g, e, mean, rscale, with_bound=True)
    obs, act = np.concatenate([g[0], e[0]]), np.concatenate([g[1], e[1]])
    x = np.concatenate([(obs - mean) * rscale, np.clip(act, f(-1), f(1))], 1).astype(f)
    a0 = np.tanh(x @ W["w0"] + W["b0"]); a1 = np.tanh(a0 @ W["w1"] + W["b1"])
    l = (a1 @ W["w2"] + W["b2"])[:, 0]
    assert l.dtype == f
    F = gr.forward64(W, obs, act, mean, rscale)
    assert np.all(np.abs(l.astype(np.float64) - F["l"]) <= F["E_l"])
    c = 33
    s, n = (f(1) / (f(1) + np.exp(-l))).astype(f), (f(1) / (f(1) + np.exp(l))).astype(f)
    isg = np.arange(2 * c) < c
    dl = (f(gr.ENTCOEFF / (2 * c)) * (s * n * l) + np.where(isg, s * f(1 / c), -n * f(1 / c))).astype(f)[:, None]
    dz1 = ((f(1) - a1 * a1) * (W["w2"][:, 0][None, :] * dl)).astype(f)
    dz0 = ((f(1) - a0 * a0) * (dz1 @ W["w1"].T)).astype(f)
    got = {"w0": x.T @ dz0, "b0": dz0.sum(0), "w1": a0.T @ dz1, "b1": dz1.sum(0), "w2": a1.T @ dl, "b2": dl.sum(0)}
    for k in gr.KEYS:
        assert got[k].dtype == f
        err = np.abs(got[k].astype(np.float64) - G[k])
        assert np.all(err <= E[k]), (k, (err / E[k]).max())
        assert E[k].max() <= 0.1 * np.abs(G[k]).max(), k                                   # and the bounds bound something
    r32 = (-np.log(n + f(1e-8))).astype(f)
    assert np.all(np.abs(r32.astype(np.float64) - gr.reward64(F["l"])) <= gr.reward_bound(F["l"], F["E_l"]))


# ---------------------------------------------------------------------------------------------------- the schedule, the statistics
def test_discriminator_schedule():
    import torch
    from quadsim_amd import discriminator_schedule
    from quadsim_amd.gail import ExpertCursor
    gen = lambda s: torch.Generator().manual_seed(s)     # noqa: E731
    rows = torch.arange(1000, 1035, dtype=torch.int32)   # 35 train rows of an expert with ids of its own
    for n_gen, batch, steps in ((80, 16, 7), (64, 64, 3), (1024, 10, 5), (17, 1, 40)):
        gi, ei = discriminator_schedule(n_gen, rows, batch, steps, gen(3))
        assert gi.dtype == ei.dtype == torch.int32 and tuple(gi.shape) == tuple(ei.shape) == (steps, batch)
        assert gi.device.type == "cpu" and gi.is_contiguous() and ei.is_contiguous()
        assert int(gi.min()) >= 0 and int(gi.max()) < n_gen and int(ei.min()) >= 1000 and int(ei.max()) < 1035
        for s in range(steps):
            assert len(set(gi[s].tolist())) == batch, "a generator row twice inside a step"
            if batch <= 35:
                assert len(set(ei[s].tolist())) == batch, "an expert row twice inside a step"
        again = discriminator_schedule(n_gen, rows, batch, steps, gen(3))
        assert torch.equal(gi, again[0]) and torch.equal(ei, again[1])
        assert not torch.equal(gi, discriminator_schedule(n_gen, rows, batch, steps, gen(4))[0]) or n_gen == batch == 1
        # a prefix of a longer schedule
        longer = discriminator_schedule(n_gen, rows, batch, steps + 3, gen(3))
        assert torch.equal(longer[0][:steps], gi) and torch.equal(longer[1][:steps], ei)
    # the expert's shuffles are carried across calls: two calls on one cursor and one generator are the one longer call
    g, cur = gen(5), ExpertCursor(rows)
    a = discriminator_schedule(80, cur, 10, 2, g)
    b = discriminator_schedule(80, cur, 10, 4, g)
    g2, cur2 = gen(5), ExpertCursor(rows)
    a2 = discriminator_schedule(80, cur2, 10, 2, g2)
    assert torch.equal(a[1], a2[1]) and cur.pos == 30
    # three steps of 10 take 30 of the 35 rows of a shuffle; every shuffle's steps are disjoint
    first = torch.cat([a[1].reshape(-1), b[1][0]])
    assert len(set(first.tolist())) == 30
    assert set(b[1][1].tolist()) & set(first.tolist())           # the fourth step starts the next shuffle
    with pytest.raises(ValueError):
        discriminator_schedule(8, rows, 9, 1, gen(0))
    with pytest.raises(ValueError):
        discriminator_schedule(8, rows, 4, 0, gen(0))
    # fewer expert rows than a step: rows repeat, and the walk still covers every row
    gi, ei = discriminator_schedule(80, torch.arange(5, dtype=torch.int32), 16, 2, gen(1))
    assert set(ei.reshape(-1).tolist()) == set(range(5))


def test_running_statistics_against_numpy_on_concatenated_batches(tmp_path):
    import torch
    import quadsim_amd as qa
    rng = np.random.default_rng(3)
    batches = [rng.standard_normal((n, 12)) * rng.uniform(0.01, 5.0, 12) + rng.uniform(-3, 3, 12) for n in (7, 1, 300)]
    d = qa.Discriminator(hidden=10, device="cpu")
    np.testing.assert_allclose(d.stats.mean, 0.0)
    np.testing.assert_allclose(d.stats.std, 1.0)                 # sqrt(max(1e-2 / 1e-2 - 0, 1e-2))
    for b in batches:
        d.update_stats(b.astype(np.float32))
    cat = np.concatenate([b.astype(np.float32).astype(np.float64) for b in batches])
    n = cat.shape[0] + 1e-2
    mean = cat.sum(0) / n
    std = np.sqrt(np.maximum(((cat ** 2).sum(0) + 1e-2) / n - mean ** 2, 1e-2))
    np.testing.assert_allclose(d.stats.mean, mean, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(d.stats.std, std, rtol=1e-13)
    m64, s64 = gr.running_stats([b.astype(np.float32) for b in batches])
    np.testing.assert_allclose(m64, mean, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(s64, std, rtol=1e-13)
    mt, rt = d.norm_tensors()
    assert mt.dtype == rt.dtype == torch.float32 and np.array_equal(rt.numpy(), (1.0 / std).astype(np.float32))
    assert (std >= 0.1).all() and (std == 0.1).any() is not None
    # Xavier-uniform weights, zero biases; save and load
    for k, shape in zip(gr.KEYS, ((16, 10), (10,), (10, 10), (10,), (10, 1), (1,))):
        w = getattr(d, k).numpy()
        assert w.shape == shape and w.dtype == np.float32
        if len(shape) == 2:
            lim = np.sqrt(6.0 / sum(shape))
            assert np.abs(w).max() <= lim and np.abs(w).max() > 0.5 * lim
        else:
            assert not w.any()
    assert not np.array_equal(qa.Discriminator(hidden=10, seed=1, device="cpu").w1.numpy(), d.w1.numpy())
    d.steps, d.m[0][0, 0] = 7, 0.5
    path = str(tmp_path / "disc.npz")
    d.save_npz(path)
    e = qa.Discriminator.from_npz(path, device="cpu")
    assert e.hidden == 10 and e.steps == 7 and e.entcoeff == d.entcoeff and float(e.m[0][0, 0]) == 0.5
    assert all(torch.equal(a, b) for a, b in zip(d.tensors() + d.m + d.v, e.tensors() + e.m + e.v))
    assert np.array_equal(e.stats.mean, d.stats.mean) and np.array_equal(e.stats.std, d.stats.std)
    d.reset_optimizer()
    assert d.steps == 0 and not d.m[0].any()


def test_torch_fit_is_the_reference_update():
    """torch_discriminator_fit (float32, on the CPU here) against fit64 over three steps with a ragged count: the statistics and
    the weights agree to float32's precision, from the same merge of the statistics"""
    import torch
    import quadsim_amd as qa
    W = gr.weights(100)
    gen, exp, _, _ = gr.dataset()
    gi, ei = gr.step_indices(17, steps=3)
    counts = np.array([17, 5, 16], np.int32)
    d = qa.Discriminator(hidden=100, device="cpu", weights=W)

    class E:
        obs, actions = torch.as_tensor(exp[0]), torch.as_tensor(exp[1])
    out = qa.torch_discriminator_fit(d, torch.as_tensor(gen[0]), torch.as_tensor(gen[1]), E, torch.as_tensor(gi), torch.as_tensor(ei),
                                     torch.as_tensor(counts), lr=1e-2, return_grads=True)
    used = np.arange(17)[None, :] < counts[:, None]
    mean, std = gr.running_stats([np.concatenate([gen[0][gi[used]], exp[0][ei[used]]])])
    mt, rt = d.norm_tensors()
    assert np.array_equal(mt.numpy(), mean.astype(np.float32)) and np.array_equal(rt.numpy(), (1.0 / std).astype(np.float32))
    Z = gr.zero_state(W)
    W64, _, _, S64 = gr.fit64(W, Z, Z, gen, exp, gi, ei, mt.numpy(), rt.numpy(), counts, lr=1e-2)
    np.testing.assert_allclose(out["stats"].numpy(), S64, rtol=2e-5, atol=2e-6)
    assert d.steps == 3 and len(out["grads"]) == 6
    for k in gr.KEYS:
        np.testing.assert_allclose(getattr(d, k).numpy(), W64[k], rtol=0, atol=2e-4)       # Adam's first steps are sign steps of lr
        assert not np.array_equal(getattr(d, k).numpy(), W[k])
