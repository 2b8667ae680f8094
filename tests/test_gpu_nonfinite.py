"""The trainers on the device at NaN and inf inputs: every case of tests/nonfinite_cases.py through the raw entry point, in the
sentinel-guarded runners of tests/test_gpu_ddpg.py, tests/test_gpu_ppo2.py, tests/test_gpu_dynfit.py, tests/test_gpu_bcfit.py and tests/test_gpu_gail.py, against the float64 references that
tests/test_nonfinite_cpu.py anchors to torch autograd at the same cases.  What is held, per case (the NON-FINITE VALUES paragraph
of the headers):
  statistics   a statistic is non-finite exactly where the reference's is; the finite ones within the reference's derived bounds
  state        a net's gradient holds a non-finite element, and a net a non-finite weight after the step, exactly where the
               reference's does; w, m, v are non-finite in exactly the elements adam64 / update64 make non-finite from the device's
               OWN gradient, the finite ones within adam_bound / update_bound; finite gradient elements within their bounds
  no invention a clean-by-contract case (an infinity the clamp bounds, a terminal row's target value) is bit for bit its twin
  unread data  rows no index names, entries at and beyond counts[s], and the step before the poisoned one: bit for bit the twin's
  no faults    every tensor the call writes lies between sentinel bytes, checked by the runners
and per trainer, at the wrappers, update="hip" and update="torch" log the same non-finite statistics.
No case has more than two steps of 17 rows."""
import numpy as np
import pytest

import bcfit_ref as br
import ddpg_ref as dd
import dynfit_ref as fr
import gail_ref as gr
import nonfinite_cases as nc
import ppo2_ref as pr
import test_gpu_bcfit as tgb
import test_gpu_ddpg as tgd
import test_gpu_dynfit as tgf
import test_gpu_gail as tgg
import test_gpu_ppo2 as tgp

pytestmark = pytest.mark.gpu

ids = lambda cases: [c["id"] for c in cases]     # noqa: E731
same_bits, nonfinite, has_nonfinite = tgd.same_bits, nc.nonfinite, nc.has_nonfinite


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _zeroed(a):
    a = np.asarray(a, np.float64)
    return np.where(np.isfinite(a), a, 0.0)


def within(got, want, bound, what):
    """the non-finite elements are the same ones; the finite ones within the bound"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(nonfinite(got), nonfinite(want)), "%s: %d non-finite elements on the device, %d in the reference, %d differ" % (
        what, int(nonfinite(got).sum()), int(nonfinite(want).sum()), int((nonfinite(got) != nonfinite(want)).sum()))
    ok = np.isfinite(want)
    assert np.isfinite(np.asarray(bound)[ok]).all() and (np.abs(got[ok] - want[ok]) <= np.asarray(bound)[ok]).all(), what


def finite_within(got, want, bound, what):
    """where the device, the reference and its bound are all finite: within the bound"""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    ok = np.isfinite(got) & np.isfinite(want) & np.isfinite(bound)
    assert (np.abs(got[ok] - want[ok]) <= bound[ok]).all(), what


# ---------------------------------------------------------------------------------------------------- DDPG
def ddpg_run(torch, S, steps=None, want_grads=False):
    idx = S["idx"] if steps is None else S["idx"][:steps]
    counts = None if S["counts"] is None else S["counts"][:idx.shape[0]]
    return tgd.run_update(torch, S["P"], S["M"], S["V"], S["rp"], idx, counts=counts, want_grads=want_grads, **nc.DDPG_HYPER)


def ddpg_same(a, b, case):
    """every tensor and statistic of two runs bit for bit; a poisoned target weight itself apart (it stays what it was given)"""
    assert same_bits(a["stats"], b["stats"]), (case["id"], a["stats"], b["stats"])
    if "grads" in a:
        assert all(same_bits(a["grads"][n][k], b["grads"][n][k]) for n in nc.DDPG_ONLINE for k in dd.KEYS), case["id"]
    for (p, n, k, x), (_, _, _, y) in zip(tgd.tensors_of(a), tgd.tensors_of(b)):
        if case["target"] == (p, n, k):
            x, y = x.copy(), y.copy()
            assert nonfinite(x.reshape(-1)[case["elem"]]) and np.isfinite(y).all()
            x.reshape(-1)[case["elem"]] = y.reshape(-1)[case["elem"]]
        assert same_bits(x, y), (case["id"], p, n, k)


@pytest.mark.parametrize("case", nc.DDPG_CASES, ids=ids(nc.DDPG_CASES))
def test_ddpg_case(torch, case):
    S = nc.ddpg_setup(case)
    ref = nc.ddpg_reference(S, with_bound=True)
    st, G, Es, E = ref["first"]
    one = ddpg_run(torch, S, steps=1, want_grads=True)
    within(one["stats"][0], st, Es, "%s: the statistics of step 1" % case["id"])
    for i, n in enumerate(nc.DDPG_ONLINE):
        assert has_nonfinite(one["grads"][n]) == bool(ref["gflag"][0][i]), (case["id"], n, "a non-finite gradient element")
        for k in dd.KEYS:
            g = one["grads"][n][k]
            finite_within(g, G[n][k], E[n][k], "%s: the finite elements of the gradient of %s %s" % (case["id"], n, k))
            w0, m0, v0 = S["P"][n][k], S["M"][n][k], S["V"][n][k]
            with np.errstate(all="ignore"):
                want = dd.adam64(w0, m0, v0, g, 1, nc.DDPG_HYPER[n + "_lr"])
            bounds = dd.adam_bound(_zeroed(w0), _zeroed(m0), _zeroed(v0), _zeroed(g), 1, nc.DDPG_HYPER[n + "_lr"])
            for p, wnt, b in zip("wmv", want, bounds):
                within(one[p][n][k], wnt, b, "%s: %s of %s %s after Adam on the device's own gradient" % (case["id"], p, n, k))
    assert [has_nonfinite(one["w"][n]) for n in dd.NETS] == list(ref["nets"][0]), (case["id"], "a non-finite weight per net after step 1")
    last = one
    if case["steps"] == 2:
        last = ddpg_run(torch, S, want_grads=True)
        assert same_bits(last["stats"][0], one["stats"][0])
        assert np.array_equal(nonfinite(last["stats"]), nonfinite(ref["stats"])), (case["id"], last["stats"], ref["stats"])
        assert [has_nonfinite(last["w"][n]) for n in dd.NETS] == list(ref["nets"][1]), (case["id"], "a non-finite weight per net after step 2")
    if case["clean"] or case["step"] == 1:
        twin = ddpg_run(torch, nc.ddpg_setup(case, twin=True), want_grads=True)
        if case["clean"]:
            assert np.isfinite(last["stats"]).all()
            ddpg_same(last, twin, case)
        else:
            assert same_bits(last["stats"][0], twin["stats"][0]) and np.isfinite(twin["stats"]).all(), case["id"]


@pytest.mark.parametrize("cid", ["obs0-nan-row3", "rew-nan", "critic-target-w2-nan-live", "critic-target-w2-nan-terminal"])
def test_ddpg_wrappers_log_the_same_non_finite_statistics(torch, cid):
    import quadsim_amd as qa
    (case,) = [c for c in nc.DDPG_CASES if c["id"] == cid]
    S = nc.ddpg_setup(case)
    ref = nc.ddpg_reference(S)
    masks = []
    for update in (qa.ddpg_update, qa.torch_ddpg_update):
        pol = tgd._policy(torch, S["P"], S["M"], S["V"])
        out = update(pol, tuple(tgd.dev(torch, a) for a in S["rp"]), torch.as_tensor(S["idx"]), **nc.DDPG_HYPER)
        torch.cuda.synchronize()
        masks.append(nonfinite(out["stats"].cpu().numpy()))
        assert [bool(any(not torch.isfinite(w).all() for w in getattr(pol, n))) for n in dd.NETS] == list(ref["nets"][-1]), (cid, update.__name__)
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], nonfinite(ref["stats"])), (cid, masks)
    assert masks[0].any() == (case["clean"] is None)


# ---------------------------------------------------------------------------------------------------- PPO2
def ppo2_run(torch, S, steps=None, want_grads=False):
    idx = S["idx"] if steps is None else S["idx"][:steps]
    return tgp.run(torch, S["W"], S["M"], S["V"], S["data"], idx, S["hp"], slices=S["slices"], want_grads=want_grads)


@pytest.mark.parametrize("case", nc.PPO2_CASES, ids=ids(nc.PPO2_CASES))
def test_ppo2_case(torch, case):
    S = nc.ppo2_setup(case)
    hp = S["hp"]
    ref = nc.ppo2_reference(S, with_bound=True)
    st, G, SB, E = ref["first"]
    one = ppo2_run(torch, S, steps=1, want_grads=True)
    within(one["stats"][0], st, SB, "%s: the statistics of step 1 %s against %s" % (case["id"], one["stats"][0], st))
    assert has_nonfinite(one["grads"]) == bool(ref["gflag"][0]), (case["id"], "a non-finite gradient element")
    for k in G:
        finite_within(one["grads"][k], G[k], E[k], "%s: the finite elements of the gradient of %s" % (case["id"], k))
    Gd = {k: one["grads"][k] for k in G}
    with np.errstate(all="ignore"):
        Wn, Mn, Vn, _, _ = pr.update64(S["W"], S["M"], S["V"], Gd, hp, 1)
    UB = pr.update_bound(*({k: _zeroed(a[k]) for k in G} for a in (S["W"], S["M"], S["V"], Gd)), hp, 1)
    for k in G:
        for p, wnt, b in zip("wmv", (Wn[k], Mn[k], Vn[k]), UB[k]):
            within(one[p][k], wnt, b, "%s: %s of %s after the clip and Adam on the device's own gradient" % (case["id"], p, k))
    assert has_nonfinite(one["w"]) == bool(ref["nets"][0]), (case["id"], "a non-finite weight after step 1")
    last = one
    if case["steps"] == 2:
        last = ppo2_run(torch, S, want_grads=True)
        assert same_bits(last["stats"][0], one["stats"][0])
        assert np.array_equal(nonfinite(last["stats"]), nonfinite(ref["stats"])), (case["id"], last["stats"], ref["stats"])
        assert has_nonfinite(last["w"]) == bool(ref["nets"][1]), (case["id"], "a non-finite weight after step 2")
    if case["clean"] or case["step"] == 1:
        twin = ppo2_run(torch, nc.ppo2_setup(case, twin=True), want_grads=True)
        if case["clean"]:
            assert np.isfinite(last["stats"]).all() and same_bits(last["stats"], twin["stats"]) and tgp.state_bits_equal(last, twin), case["id"]
            assert all(same_bits(last["grads"][k], twin["grads"][k]) for k in G), case["id"]
        else:
            assert same_bits(last["stats"][0], twin["stats"][0]) and np.isfinite(twin["stats"]).all(), case["id"]


@pytest.mark.parametrize("cid", ["shared-s1-values-nan", "towers-s3-neglogp-nan", "towers-s3-obs-nan-row16", "shared-s1-unread-row-nan"])
def test_ppo2_wrappers_log_the_same_non_finite_statistics(torch, cid):
    import quadsim_amd as qa
    from quadsim_amd import ppo2
    (case,) = [c for c in nc.PPO2_CASES if c["id"] == cid]
    S = nc.ppo2_setup(case)
    hp, ref = S["hp"], nc.ppo2_reference(S)
    kw = dict(learning_rate=hp["lr"], cliprange=hp["cliprange"], cliprange_vf=hp["cliprange_vf"], ent_coef=hp["ent_coef"], vf_coef=hp["vf_coef"],
              max_grad_norm=hp["max_grad_norm"])
    data = dict(zip(tgp.DATA_KEYS, tgp.device_data(torch, S["data"])))
    idx = torch.as_tensor(S["idx"]).cuda()
    masks = []
    for update, extra in ((ppo2.ppo2_update, dict(slices=case["slices"])), (ppo2.torch_ppo2_update, {})):
        pol = qa.ActorCriticPolicy({k: v.copy() for k, v in S["W"].items()}, device="cuda")
        out = update(pol, data, idx, **kw, **extra)
        torch.cuda.synchronize()
        masks.append(nonfinite(out["stats"].cpu().numpy()))
        bad = any(not torch.isfinite(w).all() for w in ppo2.policy_tensors(pol) if w is not None)
        assert bool(bad) == bool(ref["nets"][-1]), (cid, update.__name__)
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], nonfinite(ref["stats"])), (cid, masks)
    assert masks[0].any() == (case["clean"] is None)


# ---------------------------------------------------------------------------------------------------- the dynamics fit
def dynfit_run(torch, S, steps=None):
    idx = S["idx"] if steps is None else S["idx"][:steps]
    buf = tuple(torch.as_tensor(a).cuda().contiguous() for a in (S["x"], S["d"]))
    return tgf.run(torch, S["W"], S["M"], S["V"], buf, idx.shape[0], idx.shape[1], lr=nc.DYNFIT_LR, indices=idx, want_grads=True)


@pytest.mark.parametrize("case", nc.DYNFIT_CASES, ids=ids(nc.DYNFIT_CASES))
def test_dynfit_case(torch, case):
    S = nc.dynfit_setup(case)
    ref = nc.dynfit_reference(S, with_bound=True)
    st, G, lb, E = ref["first"]
    one = dynfit_run(torch, S, steps=1)
    within(one["loss"][:1], st, lb, "%s: the loss of step 1 %s against %s" % (case["id"], one["loss"], st))
    assert has_nonfinite(one["grads"]) == bool(ref["gflag"][0]), (case["id"], "a non-finite gradient element")
    for k in fr.GRAD_KEYS:
        g = one["grads"][k]
        finite_within(g, G[k], E[k], "%s: the finite elements of the gradient of %s" % (case["id"], k))
        w0, m0, v0 = S["W"][k], S["M"][k], S["V"][k]
        with np.errstate(all="ignore"):
            want = fr.adam64(w0, m0, v0, g, 1, nc.DYNFIT_LR)
        bounds = fr.adam_bound(_zeroed(w0), _zeroed(m0), _zeroed(v0), _zeroed(g), 1, nc.DYNFIT_LR)
        for p, wnt, b in zip("wmv", want, bounds):
            within(one[p][k], wnt, b, "%s: %s of %s after Adam on the device's own gradient" % (case["id"], p, k))
    assert has_nonfinite(one["w"]) == bool(ref["nets"][0]), (case["id"], "a non-finite weight after step 1")
    last = one
    if case["steps"] == 2:
        last = dynfit_run(torch, S)
        assert same_bits(last["loss"][0], one["loss"][0])
        assert np.array_equal(nonfinite(last["loss"]), nonfinite(ref["stats"][:, 0])), (case["id"], last["loss"], ref["stats"])
        assert has_nonfinite(last["w"]) == bool(ref["nets"][1]), (case["id"], "a non-finite weight after step 2")
    if case["clean"] or case["step"] == 1:
        twin = dynfit_run(torch, nc.dynfit_setup(case, twin=True))
        if case["clean"]:
            assert np.isfinite(last["loss"]).all() and same_bits(last["loss"], twin["loss"]) and tgf.state_bits_equal(last, twin), case["id"]
            assert all(same_bits(last["grads"][k], twin["grads"][k]) for k in fr.GRAD_KEYS), case["id"]
        else:
            assert same_bits(last["loss"][0], twin["loss"][0]) and np.isfinite(twin["loss"]).all(), case["id"]


# ---------------------------------------------------------------------------------------------------- behaviour cloning
def bc_run(torch, S, steps=None):
    idx = S["idx"] if steps is None else S["idx"][:steps]
    counts = None if S["counts"] is None else S["counts"][:idx.shape[0]]
    data = tuple(torch.as_tensor(a).cuda().contiguous() for a in S["data"])
    return tgb.run(torch, S["W"], S["M"], S["V"], data, idx, counts=counts, lr=nc.BC_LR, want_grads=True)


@pytest.mark.parametrize("case", nc.BC_CASES, ids=ids(nc.BC_CASES))
def test_bc_case(torch, case):
    S = nc.bc_setup(case)
    ref = nc.bc_reference(S, with_bound=True)
    st, G, lb, E = ref["first"]
    one = bc_run(torch, S, steps=1)
    within(one["loss"][:1], st, lb, "%s: the loss of step 1 %s against %s" % (case["id"], one["loss"], st))
    assert has_nonfinite(one["grads"]) == bool(ref["gflag"][0]), (case["id"], "a non-finite gradient element")
    for k in br.KEYS:
        g = one["grads"][k]
        finite_within(g, G[k], E[k], "%s: the finite elements of the gradient of %s" % (case["id"], k))
        w0, m0, v0 = S["W"][k], S["M"][k], S["V"][k]
        with np.errstate(all="ignore"):
            want = br.adam64(w0, m0, v0, g, 1, nc.BC_LR)
        bounds = br.adam_bound(_zeroed(w0), _zeroed(m0), _zeroed(v0), _zeroed(g), 1, nc.BC_LR)
        for p, wnt, b in zip("wmv", want, bounds):
            within(one[p][k], wnt, b, "%s: %s of %s after Adam on the device's own gradient" % (case["id"], p, k))
    assert has_nonfinite(one["w"]) == bool(ref["nets"][0]), (case["id"], "a non-finite weight after step 1")
    last = one
    if case["steps"] == 2:
        last = bc_run(torch, S)
        assert same_bits(last["loss"][0], one["loss"][0])
        assert np.array_equal(nonfinite(last["loss"]), nonfinite(ref["stats"][:, 0])), (case["id"], last["loss"], ref["stats"])
        assert has_nonfinite(last["w"]) == bool(ref["nets"][1]), (case["id"], "a non-finite weight after step 2")
    if case["clean"] or case["step"] == 1:
        twin = bc_run(torch, nc.bc_setup(case, twin=True))
        if case["clean"]:
            assert np.isfinite(last["loss"]).all() and same_bits(last["loss"], twin["loss"]) and tgb.state_bits_equal(last, twin), case["id"]
            assert all(same_bits(last["grads"][k], twin["grads"][k]) for k in br.KEYS), case["id"]
        else:
            assert same_bits(last["loss"][0], twin["loss"][0]) and np.isfinite(twin["loss"]).all(), case["id"]


# ---------------------------------------------------------------------------------------------------- GAIL's discriminator
def gail_run(torch, S, steps=None):
    gi, ei = (S[k] if steps is None else S[k][:steps] for k in ("gi", "ei"))
    counts = None if S["counts"] is None else S["counts"][:gi.shape[0]]
    return tgg.run_fit(torch, S["W"], S["M"], S["V"], S["gen"], S["exp"], S["mean"], S["rscale"], gi, ei, counts=counts, lr=nc.GAIL_LR,
                       want_grads=True)


@pytest.mark.parametrize("case", nc.GAIL_CASES, ids=ids(nc.GAIL_CASES))
def test_gail_fit_case(torch, case):
    S = nc.gail_setup(case)
    ref = nc.gail_reference(S, with_bound=True)
    st, G, Es, E = ref["first"]
    one = gail_run(torch, S, steps=1)
    within(one["stats"][0], st, Es, "%s: the statistics of step 1 %s against %s" % (case["id"], one["stats"][0], st))
    assert has_nonfinite(one["grads"]) == bool(ref["gflag"][0]), (case["id"], "a non-finite gradient element")
    for k in gr.KEYS:
        g = one["grads"][k]
        finite_within(g, G[k], E[k], "%s: the finite elements of the gradient of %s" % (case["id"], k))
        w0, m0, v0 = S["W"][k], S["M"][k], S["V"][k]
        with np.errstate(all="ignore"):
            want = gr.adam64(w0, m0, v0, g, 1, nc.GAIL_LR)
        bounds = gr.adam_bound(_zeroed(w0), _zeroed(m0), _zeroed(v0), _zeroed(g), 1, nc.GAIL_LR)
        for p, wnt, b in zip("wmv", want, bounds):
            within(one[p][k], wnt, b, "%s: %s of %s after Adam on the device's own gradient" % (case["id"], p, k))
    assert has_nonfinite(one["w"]) == bool(ref["nets"][0]), (case["id"], "a non-finite weight after step 1")
    last = one
    if case["steps"] == 2:
        last = gail_run(torch, S)
        assert same_bits(last["stats"][0], one["stats"][0])
        assert np.array_equal(nonfinite(last["stats"]), nonfinite(ref["stats"])), (case["id"], last["stats"], ref["stats"])
        assert has_nonfinite(last["w"]) == bool(ref["nets"][1]), (case["id"], "a non-finite weight after step 2")
    if case["clean"] or case["step"] == 1:
        twin = gail_run(torch, nc.gail_setup(case, twin=True))
        if case["clean"]:
            assert np.isfinite(last["stats"]).all() and same_bits(last["stats"], twin["stats"]) and tgg.state_bits_equal(last, twin), case["id"]
            assert all(same_bits(last["grads"][k], twin["grads"][k]) for k in gr.KEYS), case["id"]
        else:
            assert same_bits(last["stats"][0], twin["stats"][0]) and np.isfinite(twin["stats"]).all(), case["id"]


@pytest.mark.parametrize("case", nc.GAIL_REWARD_CASES, ids=ids(nc.GAIL_REWARD_CASES))
def test_gail_reward_case(torch, case):
    """qsg_reward: the reward and the logit are non-finite in exactly the reference's rows and within their bounds elsewhere;
    every other row, and every row of a clean case, is bit for bit the twin's"""
    S, T = nc.gail_reward_setup(case), nc.gail_reward_setup(case, twin=True)
    rew64, l64, Er, El = nc.gail_reward_reference(S)
    rew, lg = tgg.run_reward(torch, S["W"], S["obs"], S["act"], S["mean"], S["rscale"])
    within(lg, l64, El, "%s: the logits" % case["id"])
    within(rew, rew64, Er, "%s: the rewards" % case["id"])
    trew, tlg = tgg.run_reward(torch, T["W"], T["obs"], T["act"], T["mean"], T["rscale"])
    ok = np.isfinite(rew64)
    assert np.isfinite(trew).all() and same_bits(rew[ok], trew[ok]) and same_bits(lg[ok], tlg[ok]), case["id"]
    assert ok.all() == bool(case["clean"])


@pytest.mark.parametrize("cid", ["gen-act-nan-row16", "exp-obs-nan-row16", "gen-act-pinf-clamped"])
def test_gail_wrappers_log_the_same_non_finite_statistics(torch, cid):
    """Discriminator.fit and torch_discriminator_fit from the same start, the running statistics left as they are"""
    import quadsim_amd as qa
    (case,) = [c for c in nc.GAIL_CASES if c["id"] == cid]
    S = nc.gail_setup(case)
    masks = []
    for torch_path in (False, True):
        d = qa.Discriminator(hidden=nc.GAIL_HIDDEN, device="cuda", weights=S["W"])

        class E:
            obs, actions = tgg.dev(torch, S["exp"][0]), tgg.dev(torch, S["exp"][1])
        args = (tgg.dev(torch, S["gen"][0]), tgg.dev(torch, S["gen"][1]), E, torch.as_tensor(S["gi"]), torch.as_tensor(S["ei"]))
        out = (qa.torch_discriminator_fit(d, *args, lr=nc.GAIL_LR, update_stats=False) if torch_path
               else d.fit(*args, lr=nc.GAIL_LR, update_stats=False))
        torch.cuda.synchronize()
        masks.append(nonfinite(out["stats"].cpu().numpy()))
        mt, rt = d.norm_tensors()
        ref = nc.gail_reference(dict(S, mean=mt.cpu().numpy(), rscale=rt.cpu().numpy(), M=gr.zero_state(S["W"]), V=gr.zero_state(S["W"])))
        assert bool(any(not torch.isfinite(w).all() for w in d.tensors())) == bool(ref["nets"][-1]), (cid, torch_path)
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], nonfinite(ref["stats"])), (cid, masks)
    assert masks[0].any() == (case["clean"] is None)
