"""The trainers on the device at NaN and inf inputs: every case of tests/nonfinite_cases.py through the raw entry point, in the
sentinel-guarded runners of tests/test_gpu_ddpg.py, tests/test_gpu_ppo2.py, tests/test_gpu_dynfit.py, tests/test_gpu_bcfit.py,
tests/test_gpu_gail.py, tests/test_gpu_td3.py (run_update) and tests/test_gpu_trpo.py (vf_fit, policy_step), against the float64
references that tests/test_nonfinite_cpu.py anchors to torch autograd at the same cases.  What is held, per case (the NON-FINITE
VALUES paragraph of the headers):
  statistics   a statistic is non-finite exactly where the reference's is; the finite ones within the reference's derived bounds
  state        a net's gradient holds a non-finite element, and a net a non-finite weight after the step, exactly where the
               reference's does; w, m, v are non-finite in exactly the elements adam64 / update64 make non-finite from the device's
               OWN gradient, the finite ones within adam_bound / update_bound; finite gradient elements within their bounds
  no invention a clean-by-contract case (an infinity the clamp bounds, a terminal row's target value, a net or a moment the call
               does not read) is bit for bit its twin
  unread data  rows no index names, entries at and beyond counts[s], and the step before the poisoned one: bit for bit the twin's
  no faults    every tensor the call writes lies between sentinel bytes, checked by the runners
and per trainer, at the wrappers, update="hip" and update="torch" log the same non-finite statistics.
TRPO's policy step has no Adam and no index rows: a poisoned step is a REJECTED step -- every CG product and every candidate run and
are traced, theta, the value tower and the moments keep their bits, at 1 and at 3 slices, with and without the trace -- and its
surr_before / surr_after are the header's formula where autograd's are NaN (the documented deviation).  TD3 and TRPO keep state in a
workspace between launches: the workspace a poisoned, a skipped or an early-stopped call leaves, and one of 0xFF bytes, change no
bit of the next call.
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
import td3_ref as td
import test_gpu_td3 as tgt
import test_gpu_trpo as tgr
import trpo_ref as tr

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


# ---------------------------------------------------------------------------------------------------- TD3
def td3_run(torch, S, steps=None, ws_init=None):
    idx = S["idx"] if steps is None else S["idx"][:steps]
    counts = None if S["counts"] is None else S["counts"][:idx.shape[0]]
    return tgt.run_update(torch, S["P"], S["M"], S["V"], S["rp"], idx, counts=counts, t0=S["t0"], actor_t0=S["actor_t0"],
                          noise=S["z"][:idx.shape[0]], want_grads=True, want_noise=True, ws_init=ws_init, **S["hp"])


def td3_same(a, b, case, last_is_actor_step):
    """every tensor, statistic and gradient of two runs bit for bit; a poisoned weight itself apart (it stays non-finite)"""
    assert same_bits(a["stats"], b["stats"]), (case["id"], a["stats"], b["stats"])
    for n in td.ONLINE if last_is_actor_step else ("q1", "q2"):
        assert all(same_bits(a["grads"][n][k], b["grads"][n][k]) for k in td.KEYS), (case["id"], "gradients", n)
    for (p, n, k, x), (_, _, _, y) in zip(tgt.tensors_of(a), tgt.tensors_of(b)):
        if case is not None and case["target"] == (p, n, k):
            x, y = x.copy(), y.copy()
            assert nonfinite(x.reshape(-1)[case["elem"]]) and np.isfinite(y).all()
            x.reshape(-1)[case["elem"]] = y.reshape(-1)[case["elem"]]
        assert same_bits(x, y), (case["id"], p, n, k)


@pytest.mark.parametrize("case", nc.TD3_CASES, ids=ids(nc.TD3_CASES))
def test_td3_case(torch, case):
    S = nc.td3_setup(case)
    hp = S["hp"]
    ref = nc.td3_reference(S, with_bound=True)
    st, G, Es, E = ref["first"]
    one = td3_run(torch, S, steps=1)
    within(one["stats"][0], st, Es, "%s: the statistics of step 1 %s against %s" % (case["id"], one["stats"][0], st))
    for i, n in enumerate(td.ONLINE):
        if n not in G:
            # a critic-only update: the actor and its moments keep the bits they were given, non-finite ones included
            assert not td.actor_step(S["t0"], hp["policy_delay"]) and one["stats"][0, 5] == 0.0 and not np.signbit(one["stats"][0, 5])
            assert all(same_bits(one[p][n][k], src[n][k]) for p, src in (("w", S["P"]), ("m", S["M"]), ("v", S["V"])) for k in td.KEYS), case["id"]
            continue
        assert has_nonfinite(one["grads"][n]) == bool(ref["gflag"][0][i]), (case["id"], n, "a non-finite gradient element")
        t, lr = (S["actor_t0"] + 1, hp["actor_lr"]) if n == "actor" else (S["t0"] + 1, hp["critic_lr"])
        for k in td.KEYS:
            g = one["grads"][n][k]
            finite_within(g, G[n][k], E[n][k], "%s: the finite elements of the gradient of %s %s" % (case["id"], n, k))
            w0, m0, v0 = S["P"][n][k], S["M"][n][k], S["V"][n][k]
            with np.errstate(all="ignore"):
                want = td.adam64(w0, m0, v0, g, t, lr)
            bounds = td.adam_bound(_zeroed(w0), _zeroed(m0), _zeroed(v0), _zeroed(g), t, lr)
            for p, wnt, b in zip("wmv", want, bounds):
                within(one[p][n][k], wnt, b, "%s: %s of %s %s after Adam on the device's own gradient" % (case["id"], p, n, k))
    assert [has_nonfinite(one["w"][n]) for n in td.NETS] == list(ref["nets"][0]), (case["id"], "a non-finite weight per net after step 1")
    # noise_out carries the normals that were used, a non-finite one included, slot for slot
    c0 = nc.BATCH if S["counts"] is None else int(S["counts"][0])
    assert same_bits(one["noise"][0, :c0], S["z"][0, :c0]) and (case["target"][0] != "noise" or nonfinite(one["noise"]).sum() == 1), case["id"]
    last = one
    if case["steps"] == 2:
        last = td3_run(torch, S)
        assert same_bits(last["stats"][0], one["stats"][0])
        assert np.array_equal(nonfinite(last["stats"]), nonfinite(ref["stats"])), (case["id"], last["stats"], ref["stats"])
        assert [has_nonfinite(last["w"][n]) for n in td.NETS] == list(ref["nets"][1]), (case["id"], "a non-finite weight per net after step 2")
    if "nets" in case:
        assert [n for n in td.NETS if has_nonfinite(last["w"][n])] == [n for n in td.NETS if n in case["nets"]], case["id"]
    first_is_clean = case["steps"] == 2 and not nonfinite(ref["stats"][0]).any()
    if case["clean"] or first_is_clean:
        twin = td3_run(torch, nc.td3_setup(case, twin=True))
        if case["clean"]:
            assert np.isfinite(last["stats"]).all()
            td3_same(last, twin, case, td.actor_step(S["t0"] + case["steps"] - 1, hp["policy_delay"]))
        else:
            assert same_bits(last["stats"][0], twin["stats"][0]) and np.isfinite(twin["stats"]).all(), case["id"]


@pytest.mark.parametrize("cid", ["obs0-nan-row3", "noise-nan-live", "q1-target-b2-pinf-live", "actor-w0-nan-critic-only"])
def test_td3_wrappers_log_the_same_non_finite_statistics(torch, cid):
    import quadsim_amd as qa
    (case,) = [c for c in nc.TD3_CASES if c["id"] == cid]
    S = nc.td3_setup(case)
    ref = nc.td3_reference(S)
    masks = []
    for update in (qa.td3_update, qa.torch_td3_update):
        pol = tgt._policy(torch, S["P"], S["M"], S["V"])
        pol.steps, pol.actor_steps = S["t0"], S["actor_t0"]
        out = update(pol, tuple(tgt.dev(torch, a) for a in S["rp"]), torch.as_tensor(S["idx"]), noise=torch.as_tensor(S["z"]).cuda(), **S["hp"])
        torch.cuda.synchronize()
        masks.append(nonfinite(out["stats"].cpu().numpy()))
        assert [bool(any(not torch.isfinite(w).all() for w in getattr(pol, n))) for n in td.NETS] == list(ref["nets"][-1]), (cid, update.__name__)
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], nonfinite(ref["stats"])), (cid, masks)
    assert masks[0].any() == (case["clean"] is None)


def test_td3_workspace_of_a_poisoned_call_does_not_reach_the_next_call(torch):
    """the workspace holds both places of every net, the moments and the gradients: after a call whose q1 and actor diverged it is
    full of NaNs.  The clean twin run on THAT workspace is bit for bit the twin on a fresh one; so is a run on 0xFF bytes"""
    (case,) = [c for c in nc.TD3_CASES if c["id"] == "q1-w1-nan-actor-update"]
    bad = td3_run(torch, nc.td3_setup(case))
    assert nonfinite(bad["stats"]).any() and nonfinite(bad["ws"].view(np.float32)).any()
    T = nc.td3_setup(case, twin=True)
    fresh = td3_run(torch, T)
    assert np.isfinite(fresh["stats"]).all()
    for ws in (bad["ws"], np.full_like(bad["ws"], 0xFF)):
        again = td3_run(torch, T, ws_init=ws)
        td3_same(again, fresh, dict(case, target=None), True)
        assert same_bits(again["noise"], fresh["noise"])


# ---------------------------------------------------------------------------------------------------- TRPO's value fit
def trpo_vf_run(torch, S, steps=None):
    idx = S["idx"] if steps is None else S["idx"][:steps]
    return tgr.vf_fit(torch, S["W"], S["M"], S["V"], S["data"], idx, t0=0, lr=nc.TRPO_VF_LR)


def trpo_same(a, b, case):
    """the thirteen tensors and their moments of two runs bit for bit; a poisoned element itself apart (it stays what it was given)"""
    for p, key in (("w", "W"), ("m", "M"), ("v", "V")):
        for k in nc.TRPO_KEYS:
            x, y = a[key][k], b[key][k]
            if case["target"] == (p, k):
                x, y = x.copy(), y.copy()
                assert nonfinite(x.reshape(-1)[case["elem"]]) and np.isfinite(y).all()
                x.reshape(-1)[case["elem"]] = y.reshape(-1)[case["elem"]]
            assert same_bits(x, y), (case["id"], p, k)


@pytest.mark.parametrize("case", nc.TRPO_VF_CASES, ids=ids(nc.TRPO_VF_CASES))
def test_trpo_vf_case(torch, case):
    S = nc.trpo_vf_setup(case)
    ref = nc.trpo_vf_reference(S, with_bound=True)
    st, G, lb, E = ref["first"]
    one = trpo_vf_run(torch, S, steps=1)
    within(one["stats"][:1], st, lb, "%s: the loss of step 1 %s against %s" % (case["id"], one["stats"], st))
    assert has_nonfinite(one["grads"]) == bool(ref["gflag"][0]), (case["id"], "a non-finite gradient element")
    value = lambda d: {k: d[k] for k in tr.VALUE_KEYS}       # noqa: E731
    for k in tr.VALUE_KEYS:
        finite_within(one["grads"][k], G[k], E[k], "%s: the finite elements of the gradient of %s" % (case["id"], k))
    Gd = {k: one["grads"][k] for k in tr.VALUE_KEYS}
    zeros = {k: np.zeros_like(np.asarray(G[k], np.float64)) for k in tr.VALUE_KEYS}
    # (vf_update_bound at a gradient known exactly: the device's own)
    UB = tr.vf_update_bound(*({k: _zeroed(a[k]) for k in tr.VALUE_KEYS} for a in (S["W"], S["M"], S["V"], Gd)), zeros, 1, nc.TRPO_VF_LR)
    for k in tr.VALUE_KEYS:
        with np.errstate(all="ignore"):
            want = pr.adam64(S["W"][k], S["M"][k], S["V"][k], Gd[k], 1, nc.TRPO_VF_LR, tr.VF_BETA1, tr.VF_BETA2, tr.VF_EPS)
        for p, key, wnt, b in zip("wmv", ("W", "M", "V"), want, UB[k]):
            within(one[key][k], wnt, b, "%s: %s of %s after Adam on the device's own gradient" % (case["id"], p, k))
    assert has_nonfinite(value(one["W"])) == bool(ref["nets"][0]), (case["id"], "a non-finite weight after step 1")
    last = one
    if case["steps"] == 2:
        last = trpo_vf_run(torch, S)
        assert same_bits(last["stats"][0], one["stats"][0])
        assert np.array_equal(nonfinite(last["stats"]), nonfinite(ref["stats"][:, 0])), (case["id"], last["stats"], ref["stats"])
        assert has_nonfinite(value(last["W"])) == bool(ref["nets"][1]), (case["id"], "a non-finite weight after step 2")
    # the policy's slots and their moments are not the fit's: bit for bit what they were given, a NaN included
    for key in ("W", "M", "V"):
        assert all(same_bits(last[key][k], S[key][k]) for k in tr.POLICY_KEYS), (case["id"], key)
    if case["clean"] or case["step"] == 1:
        twin = trpo_vf_run(torch, nc.trpo_vf_setup(case, twin=True))
        if case["clean"]:
            assert np.isfinite(last["stats"]).all() and same_bits(last["stats"], twin["stats"]), case["id"]
            trpo_same(last, twin, case)
            assert all(same_bits(last["grads"][k], twin["grads"][k]) for k in tr.VALUE_KEYS), case["id"]
        else:
            assert same_bits(last["stats"][0], twin["stats"][0]) and np.isfinite(twin["stats"]).all(), case["id"]


@pytest.mark.parametrize("cid", ["obs-nan-row16", "returns-pinf-row16", "wv2-nan", "policy-logstd-nan"])
def test_trpo_vf_wrappers_log_the_same_non_finite_statistics(torch, cid):
    """trpo_vf_fit and torch_trpo_vf_fit from the same start; the wrappers begin with zero moments, so the reference runs with those"""
    import quadsim_amd as qa
    (case,) = [c for c in nc.TRPO_VF_CASES if c["id"] == cid]
    S = nc.trpo_vf_setup(case)
    zero = {k: np.zeros_like(S["M"][k]) for k in nc.TRPO_KEYS}
    ref = nc.trpo_vf_reference(dict(S, M=zero, V=zero))
    data = {k: torch.as_tensor(v).cuda() for k, v in S["data"].items()}
    idx = torch.as_tensor(S["idx"]).cuda()
    masks = []
    for fit in (qa.trpo_vf_fit, qa.torch_trpo_vf_fit):
        pol = qa.ActorCriticPolicy({k: v.copy() for k, v in S["W"].items()}, device="cuda")
        out = fit(pol, data, idx, vf_stepsize=nc.TRPO_VF_LR)
        torch.cuda.synchronize()
        masks.append(nonfinite(out["stats"].cpu().numpy()))
        bad = any(not torch.isfinite(getattr(pol, k)).all() for k in tr.VALUE_KEYS)
        assert bool(bad) == bool(ref["nets"][-1]), (cid, fit.__name__)
    assert np.array_equal(masks[0], masks[1]) and np.array_equal(masks[0], nonfinite(ref["stats"][:, 0])), (cid, masks)
    assert masks[0].any() == (case["clean"] is None)


# ---------------------------------------------------------------------------------------------------- TRPO's policy step
def trpo_step_run(torch, S, slices, trace=True, ws_init=None, **hp):
    return tgr.policy_step(torch, S["W"], S["data"], dict(S["hp"], **hp), slices, trace=trace, M=S["M"], V=S["V"], n=S["n"], ws_init=ws_init,
                           marked=True)


def trpo_step_same(a, b, case, what):
    assert same_bits(a["stats"], b["stats"]) and same_bits(a["grad"], b["grad"]), (case["id"], what, a["stats"], b["stats"])
    for key in ("W", "M", "V"):
        assert all(same_bits(a[key][k], b[key][k]) for k in nc.TRPO_KEYS), (case["id"], what, key)
    if "trace" in a and "trace" in b:
        assert all(same_bits(a["trace"][k], b["trace"][k]) for k in a["trace"]), (case["id"], what, "the trace")


@pytest.mark.parametrize("case", nc.TRPO_STEP_CASES, ids=ids(nc.TRPO_STEP_CASES))
def test_trpo_step_case(torch, case):
    """a poisoned step is a rejected step.  Across 1 and 3 slices its statistics, theta, the value tower and the moments are the
    same bits (17 rows: one slice adds the rows' advantages in the order in which three slices add their sums) and g is non-finite
    in the same elements; the FINITE elements of g are rounded per slice and depend on the slices by contract.  A clean case is bit
    for bit its twin at either number of slices, the trace included"""
    S = nc.trpo_step_setup(case)
    hp, ref = S["hp"], nc.trpo_step_reference(S)
    G = ref["G"]
    runs = {sl: trpo_step_run(torch, S, sl) for sl in nc.TRPO_STEP_SLICES}
    a = runs[1]
    trpo_step_same(a, trpo_step_run(torch, S, 1, trace=False), case, "with and without the trace")
    for sl, o in runs.items():
        what = "%s, %d slices" % (case["id"], sl)
        st = o["stats"]
        assert np.array_equal(nonfinite(st), nonfinite(ref["stats"])), (what, st, ref["stats"])
        assert has_nonfinite({"g": o["grad"]}) == ref["gflag"], (what, "a non-finite element of g")
        finite_within(o["grad"], G["g"], G["E_g"], "%s: the finite elements of g" % what)
        finite_within(st[[0, 4]], [G["surr_before"], G["norm"]], [G["E_surr"], G["E_norm"]], "%s: surr_before and |g|" % what)
        T = o["trace"]
        if case["clean"]:
            twin = trpo_step_run(torch, nc.trpo_step_setup(case, twin=True), sl)
            assert np.isfinite(st).all() and st[8] >= 0.0 and same_bits(st, twin["stats"]) and same_bits(o["grad"], twin["grad"]), (what, st)
            trpo_same(o, twin, case)
            assert all(same_bits(T[k], twin["trace"][k]) for k in T), what
            assert not same_bits(o["W"]["w0"], S["W"]["w0"]) or case["target"] == ("w", "w0")
            continue
        # the header's statistics of a rejected step
        assert st[8] == -1.0 and st[9] == hp["cg_iters"] and st[2] == 0.0 and not np.signbit(st[2]), (what, st)
        assert same_bits(st[1], st[0]) and (same_bits(st[3], np.float32(G["entropy"])) or st[3] != st[3]), (what, st)
        for key in ("W", "M", "V"):
            assert all(same_bits(o[key][k], S[key][k]) for k in nc.TRPO_KEYS), (what, key, "bit for bit the input's")
        # every product, every CG iteration and every candidate ran: no trace element is left as it was
        for k in ("fvp_in", "fvp_out", "cg", "x", "fullstep", "ls"):
            assert not tgr.unwritten(T[k]).any(), (what, "trace " + k, int(tgr.unwritten(T[k]).sum()))
    if case["clean"] is None:
        b = runs[3]
        assert same_bits(a["stats"], b["stats"]), (case["id"], "1 and 3 slices", a["stats"], b["stats"])
        assert np.array_equal(nonfinite(a["grad"]), nonfinite(b["grad"])), (case["id"], "1 and 3 slices: the non-finite elements of g")


@pytest.mark.parametrize("cid", ["obs-nan-row3", "returns-nan", "w2-nan", "wv0-nan"])
def test_trpo_step_wrappers_log_the_same_non_finite_statistics(torch, cid):
    """trpo_policy_step and torch_trpo_policy_step: the same masks but for statistics 0 and 1 of a poisoned step with finite
    advantages and logstd -- the header's formula on the device, autograd's NaN on the torch path (the documented deviation)"""
    import quadsim_amd as qa
    (case,) = [c for c in nc.TRPO_STEP_CASES if c["id"] == cid]
    S = nc.trpo_step_setup(case)
    ref = nc.trpo_step_reference(S)
    data = {k: torch.as_tensor(v).cuda() for k, v in S["data"].items()}
    masks = []
    for step in (qa.trpo_policy_step, qa.torch_trpo_policy_step):
        pol = qa.ActorCriticPolicy({k: v.copy() for k, v in S["W"].items()}, device="cuda")
        out = step(pol, data, slices=1, **S["hp"])
        torch.cuda.synchronize()
        masks.append(nonfinite(out["stats"].cpu().numpy()))
        moved = any(not same_bits(getattr(pol, k).cpu().numpy(), S["W"][k]) for k in nc.TRPO_KEYS)
        assert moved == bool(case["clean"]), (cid, step.__name__)
    hip, tch = masks
    assert np.array_equal(hip, nonfinite(ref["stats"])) and np.array_equal(hip[2:], tch[2:]), (cid, masks)
    if case["clean"]:
        assert not hip.any() and not tch.any()
    else:
        header_finite = bool(np.isfinite(ref["G"]["A"]).all() and np.isfinite(S["W"]["logstd"]).all())
        assert list(hip[:2]) == [not header_finite] * 2 and list(tch[:2]) == [True, True] and hip[4:8].all(), (cid, masks)


def test_trpo_workspace_of_another_call_does_not_reach_the_next_call(torch):
    """the workspace keeps the skip, CG-converged and accepted flags, the CG scalars and every vector of the solver.  A clean step
    on the workspace a poisoned call left, on that of a skipped call (equal advantages, entcoeff 0), on that of a call whose CG
    residual_tol stopped after one iteration and on 0xFF bytes is bit for bit the step on a zeroed one, trace included"""
    (case,) = [c for c in nc.TRPO_STEP_CASES if c["id"] == "w0-nan"]
    sl = 3
    T = nc.trpo_step_setup(case, twin=True)
    fresh = trpo_step_run(torch, T, sl)
    assert np.isfinite(fresh["stats"]).all() and fresh["stats"][8] >= 0.0 and fresh["stats"][9] == T["hp"]["cg_iters"]
    bad = trpo_step_run(torch, nc.trpo_step_setup(case), sl)
    assert bad["stats"][8] == -1.0 and nonfinite(bad["stats"]).any()
    flat = dict(T, data=dict(T["data"]))
    flat["data"]["values"] = (np.round(T["data"]["values"] * 4.0) / 4.0).astype(np.float32)      # quarters: the difference below is exact
    flat["data"]["returns"] = (flat["data"]["values"] + np.float32(0.5)).astype(np.float32)
    skipped = trpo_step_run(torch, flat, sl, entcoeff=0.0)
    assert skipped["stats"][8] == -2.0 and tgr.unwritten(skipped["trace"]["fvp_in"]).all()
    early = trpo_step_run(torch, T, sl, residual_tol=1e30)
    assert early["stats"][9] == 1.0 and tgr.unwritten(early["trace"]["cg"][1:]).all() and not same_bits(early["stats"], fresh["stats"])
    for name, ws in (("poisoned", bad["ws"]), ("skipped", skipped["ws"]), ("early-stopped", early["ws"]), ("0xFF", np.full_like(bad["ws"], 0xFF))):
        assert ws.shape == fresh["ws"].shape
        trpo_step_same(trpo_step_run(torch, T, sl, ws_init=ws), fresh, case, "on the workspace of a %s call" % name)
