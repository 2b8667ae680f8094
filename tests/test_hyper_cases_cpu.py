"""-m "not gpu": the tables of tests/hyper_cases.py, before the device is held to them (tests/test_gpu_hyper.py).

  accepted     every row is accepted by the trainer's check_*_args; the out-of-range neighbours the GPU tests name (policy_delay
               65537, t0 = 2^31 - 1, actor_t0 = 2^31 - 1) are refused
  separated    for every row the float64 reference at the case and at its twin differ in the row's quantity by at least 10 of the
               reference's own bounds at the case (the median over a tensor's elements, the worst tensor of those the row names):
               a device that ignored the hyper-parameter, or swapped a pair, would be that far out of the bounds the GPU test
               asserts.  The bound helpers' own assertions (adam_bound: the denominator stays positive) hold at every row.  The
               separations are printed; profiles/hyper/README.md has a copy.  The rows of hyper_cases.EXTRA are NOT separated, and
               that is held too: a row that becomes separable belongs in the table
  constants    SHIFT is the first candidate at which gamma 1 and gamma 0.99 lie 10 bounds apart in y_mean and in every critic loss of
               DDPG and TD3; TAU_ODD the first candidate whose float32(1 - tau) differs from the float32 difference
  anchored     Adam: adam64 at every row's betas, eps and rate against tf.train.AdamOptimizer's formula in float64 torch, element by
               element.  TD3: statistics, gradients, w, m, v and targets against quadsim_amd.torch_td3_update on a float64 CPU
               TD3Policy at every row the wrapper takes (it has no betas and eps).  DDPG (DDPGPolicy is float32 only): every row
               against a float64 autograd step at the row's rates, betas, eps and tau, targets included; torch_ddpg_update on the
               host, float32, within step64's bounds.  PPO2: backward64 at every row of both layouts against float64 autograd of
               quadsim_amd.ppo2.ppo2_loss, update64 against the clip and Adam of tests/test_nonfinite_cpu.py at the row's
               max_grad_norm, betas and eps; torch_ppo2_update on the host within the bounds.  GAIL: backward64 at entcoeff 0, the
               default and 0.1, every width, against float64 autograd.  TRPO's value fit: float64 autograd, and
               torch_trpo_vf_fit on the host at every row's betas and eps within the bounds.
               The tolerances are those of tests/test_nonfinite_cpu.py for two float64 evaluations."""
import numpy as np
import pytest

import ddpg_ref as dd
import hyper_cases as hc
import nonfinite_cases as nc
import td3_ref as td

F64_STATS = dict(rtol=1e-9, atol=1e-12)          # tests/test_nonfinite_cpu.py: statistics of two float64 evaluations
F64_TENSORS = dict(rtol=1e-7, atol=1e-12)        # and their gradients (here: what one Adam step makes of them)


def _params(tables):
    out = []
    for trainer, rows in tables.items():
        for variant in (hc.PPO2_LAYOUTS if trainer == "ppo2" else (None,)):
            out += [pytest.param(trainer, row, variant, id="-".join(x for x in (trainer, variant, row["id"]) if x)) for row in rows]
    return out


def check_args(trainer, hp, t0=hc.T0, actor_t0=hc.TD3_ACTOR_T0):
    import quadsim_amd as qa
    from quadsim_amd import bc, ddpg, dynplan, gail, ppo2, td3, trpo
    F = hc.fixture(trainer)
    if trainer == "td3":
        return td3.check_td3_args(td.N_ROWS, 1, hc.BATCH, t0=t0, actor_t0=actor_t0, indices=F["idx"], **hp)
    if trainer == "ddpg":
        return ddpg.check_ddpg_args(dd.N_ROWS, 1, hc.BATCH, t0=t0, indices=F["idx"], **hp)
    if trainer == "dynfit":
        W = F["W"]
        return dynplan.check_fit_args(W["w1"].shape[0], W["w2"].shape[0], F["x"].shape[0], hc.fr.SIZE, 1, hc.BATCH, t0=t0, **hp)
    if trainer == "bc":
        return bc.check_bc_args(F["data"][0].shape[0], 1, hc.BATCH, t0=t0, indices=F["idx"], **hp)
    if trainer == "gail":
        return gail.check_gail_args(hc.gr.N_GEN, hc.gr.N_EXP, 1, hc.BATCH, hidden=nc.GAIL_HIDDEN, t0=t0, gen_idx=F["gi"], exp_idx=F["ei"], **hp)
    if trainer == "ppo2":
        hp = dict(hp, learning_rate=hp["lr"])
        del hp["lr"]
        return ppo2.check_ppo2_args(hc.pr.N_ROWS, 1, hc.BATCH, slices=1, t0=t0, **hp)
    assert trainer == "trpo_vf" and qa is not None
    return trpo.check_vf_args(hc.tr.N_ROWS, 1, hc.BATCH, t0=t0, **hp)


# ---------------------------------------------------------------------------------------------------- the tables
def test_the_tables_hold_what_the_gpu_tests_look_up():
    for trainer, rows in hc.TABLES.items():
        names = [r["id"] for r in rows + hc.EXTRA.get(trainer, ())]
        assert len(names) == len(set(names)), trainer
        assert {"betas-0-0", "betas-0.5-0.9", "betas-0.99-0.9", "eps-1e-3", "lr-0", "lr-negative"} <= set(names), trainer
        for r in rows:
            assert r["hyper"] and set(r["hyper"]) | set(r["twin"]) <= set(hc.DEFAULTS[trainer]), (trainer, r["id"])
            assert hc.hyper_of(trainer, r) != hc.hyper_of(trainer, r, twin=True), (trainer, r["id"])
    assert "eps-1e-08" in hc.ids("ppo2") and hc.DEFAULTS["ppo2"]["eps"] == 1e-5
    for trainer in ("ddpg", "td3"):
        assert {"actor-3e-3-critic-1e-2", "actor-1e-2-critic-3e-3", "actor-lr-0", "gamma-0", "gamma-0.5", "gamma-1", "tau-0.5", "tau-1e-9",
                "tau-%g" % hc.TAU_ODD} <= set(hc.ids(trainer))
    # nothing below 1e-8 and no eps of 0: the first cannot be told from the default, the second is a non-finite question
    assert all(r["hyper"].get("eps", 1.0) >= 1e-8 for rows in hc.TABLES.values() for r in rows)


@pytest.mark.parametrize("trainer, row, variant", _params(dict(hc.TABLES, **{k + "+": v for k, v in hc.EXTRA.items()})))
def test_every_row_is_accepted(trainer, row, variant):
    trainer = trainer.rstrip("+")
    check_args(trainer, hc.hyper_of(trainer, row))
    check_args(trainer, hc.hyper_of(trainer, row, twin=True))


def test_the_out_of_range_neighbours_are_refused():
    from quadsim_amd import td3
    D = hc.DEFAULTS
    for trainer in ("gail", "trpo_vf", "ddpg", "td3", "bc", "dynfit", "ppo2"):
        for t0 in hc.T_EDGE:
            check_args(trainer, D[trainer], t0=t0)
        with pytest.raises(ValueError, match="t0"):
            check_args(trainer, D[trainer], t0=2 ** 31 - 1)
    check_args("td3", D["td3"], t0=10 ** 5, actor_t0=2 ** 31 - 2)
    with pytest.raises(ValueError, match="actor_t0"):
        check_args("td3", D["td3"], t0=0, actor_t0=2 ** 31 - 1)
    delay = hc.TD3_DELAY_EDGE
    assert td3.TD3_MAX_DELAY == delay
    check_args("td3", dict(D["td3"], policy_delay=delay), t0=delay)
    with pytest.raises(ValueError, match="policy_delay"):
        check_args("td3", dict(D["td3"], policy_delay=delay + 1))
    for t0, want in ((delay, 1), (delay - 1, 0), (0, 1), (1, 0)):
        assert td3.actor_steps(t0, 1, delay) == int(td.schedule(t0, 1, delay).sum()) == want
    for name, bad in (("gamma", 1.5), ("tau", 0.0), ("target_noise_clip", -1.0), ("beta1", 1.0), ("beta2", -0.1)):
        with pytest.raises(ValueError, match=name):
            check_args("td3", dict(D["td3"], **{name: bad}))


# ---------------------------------------------------------------------------------------------------- case against twin
@pytest.mark.parametrize("trainer, row, variant", _params(hc.TABLES))
def test_the_reference_tells_the_case_from_its_twin(trainer, row, variant):
    sep, per = hc.separation(trainer, row, variant)
    worst = min(per, key=per.get)
    print("hyper separation %s %s%s (%s): %.3g bounds (worst: %s)" % (trainer, (variant + " ") if variant else "", row["id"], row["about"], sep, worst))
    assert np.isfinite(sep) and sep >= hc.SEPARATION, (trainer, variant, row["id"], per)


@pytest.mark.parametrize("trainer, row, variant", _params(hc.EXTRA))
def test_the_extra_rows_are_not_told_apart_by_the_bounds(trainer, row, variant):
    sep, per = hc.separation(trainer, row, variant)
    print("hyper separation %s %s%s (%s, no row of the table): %.3g bounds" % (trainer, (variant + " ") if variant else "", row["id"], row["about"], sep))
    assert sep < hc.SEPARATION, (trainer, row["id"], "is separable: it belongs in the table", per)


def test_the_shift_and_the_tau_are_the_first_that_qualify():
    """SHIFT: gamma 1 against gamma 0.99 in y_mean and in every critic loss, DDPG and TD3; TAU_ODD: the float32 subtraction"""
    found = None
    for shift in hc.SHIFT_CANDIDATES:
        seps = {}
        for trainer, losses in (("td3", ("q1_loss", "q2_loss")), ("ddpg", ("critic_loss",))):
            P = {"td3": td, "ddpg": dd}[trainer].nets_shifted(shift)
            F = dict(hc.fixture(trainer), P=P)
            D = hc.DEFAULTS[trainer]
            one, twin = hc.step64(trainer, F, dict(D, gamma=1.0)), hc.step64(trainer, F, D)
            for name in ("y_mean",) + losses:
                i = hc.STAT_NAMES[trainer].index(name)
                seps["%s %s" % (trainer, name)] = float(abs(one["stats"][i] - twin["stats"][i]) / one["Es"][i])
        print("hyper shift %g: gamma 1 against 0.99, %s" % (shift, ", ".join("%s %.3g" % kv for kv in seps.items())))
        if found is None and min(seps.values()) >= hc.SEPARATION:
            found = shift
    assert found == hc.SHIFT
    first = next(t for t in hc.TAU_CANDIDATES if hc.tau_shows_float32_subtraction(t))
    assert first == hc.TAU_ODD and 0.0 < first <= 0.5
    assert np.float32(1.0 - 1.0e-9) == np.float32(1.0) and not hc.tau_shows_float32_subtraction(0.5)
    print("hyper tau: %g, float32(1 - tau) = %.9g, float32(1) - float32(tau) = %.9g" % (
        first, np.float32(1.0 - first), np.float32(1.0) - np.float32(first)))
    # sigma 4 with clip 0.5: the clipped normal times sigma is the clip itself
    assert np.float32(4.0) * np.float32(0.125) == np.float32(0.5)
    assert np.array_equal(hc.clipped_noise(np.array([-3.0, -0.1, 0.05, 2.0], np.float32), 4.0, 0.5), np.array([-0.125, -0.1, 0.05, 0.125], np.float32))


# ---------------------------------------------------------------------------------------------------- the anchors
def _adam_settings():
    seen, out = set(), []
    for trainer, rows in hc.TABLES.items():
        for row in rows:
            hp = hc.hyper_of(trainer, row)
            for lr in {hp.get("lr"), hp.get("actor_lr"), hp.get("critic_lr")} - {None}:
                key = hc.adam_args(hp) + (lr,)
                if key not in seen:
                    seen.add(key)
                    out.append(key)
    return out


@pytest.mark.parametrize("beta1, beta2, eps, lr", _adam_settings())
def test_adam64_is_adams_formula_at_every_setting(beta1, beta2, eps, lr):
    import torch
    from test_nonfinite_cpu import _adam_t
    F = hc.fixture("td3")
    G = hc.step64("td3", F, hc.DEFAULTS["td3"])["G"]
    for t in (1, 4, 7, 10 ** 5 + 1, 2 ** 31 - 1):
        for lab in ("actor/w2", "q1/w0", "q2/b1"):
            w, m, v = hc.tensors("td3", F)[lab]
            want = _adam_t(torch, *(torch.tensor(np.asarray(a, np.float64)) for a in (w, m, v, G[lab])), t, lr, beta1, beta2, eps)
            for got, x in zip(dd.adam64(w, m, v, G[lab], t, lr, beta1, beta2, eps), want):
                assert np.allclose(got, x.numpy(), rtol=1e-12, atol=0.0), (lab, t)


def _wrapper_rows(trainer):
    """the rows the torch wrappers take: they have no betas and no eps"""
    return [pytest.param(r, id=r["id"]) for r in hc.TABLES[trainer] + hc.EXTRA.get(trainer, ()) if not set(r["hyper"]) & {"beta1", "beta2", "eps"}]


def _after(trainer, F, hp, t0=None, actor_t0=None):
    ref = hc.step64(trainer, F, hp, t0=t0, actor_t0=actor_t0)
    new, _ = hc.after64(trainer, F, hp, ref["G"], ref["t"], ref["lr"])
    return ref, new


@pytest.mark.parametrize("row", _wrapper_rows("td3"))
def test_td3_reference_against_torch_td3_update_in_float64(row):
    import torch
    import quadsim_amd as qa
    F, hp = hc.fixture_of("td3", row), hc.hyper_of("td3", row)
    ref, new = _after("td3", F, hp)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    pol = qa.TD3Policy(device="cpu", weights={n: {k: np.asarray(F["P"][n][k], np.float64) for k in td.KEYS} for n in td.NETS}, dtype="float64")
    for n in td.ONLINE:
        pol.m[n], pol.v[n] = [t64(F["M"][n][k]) for k in td.KEYS], [t64(F["V"][n][k]) for k in td.KEYS]
    pol.steps, pol.actor_steps = F["t0"], F["actor_t0"]
    out = qa.torch_td3_update(pol, tuple(torch.as_tensor(a) for a in F["rp"]), torch.as_tensor(F["idx"]), noise=torch.as_tensor(F["z"]),
                              return_grads=True, **{k: hp[k] for k in nc.TD3_HYPER})
    assert np.allclose(out["stats"][0].numpy(), ref["stats"], **F64_STATS), (row["id"], out["stats"], ref["stats"])
    for n in td.ONLINE:
        for i, k in enumerate(td.KEYS):
            lab = "%s/%s" % (n, k)
            assert np.allclose(out["grads"][n][i].numpy().reshape(ref["G"][lab].shape), ref["G"][lab], **F64_TENSORS), (row["id"], lab, "gradient")
            for got, want, p in zip((getattr(pol, n)[i], pol.m[n][i], pol.v[n][i]), new[lab], "wmv"):
                assert np.allclose(got.numpy(), want, **F64_TENSORS), (row["id"], lab, p)
            tgt = (1.0 - hp["tau"]) * np.asarray(F["P"][n + "_target"][k], np.float64) + hp["tau"] * new[lab][0]
            assert np.allclose(getattr(pol, n + "_target")[i].numpy(), tgt, **F64_TENSORS), (row["id"], lab, "target")


def _ddpg_autograd64(F, hp):
    """one DDPG step in float64 torch autograd (tests/test_ddpg_cpu.py's actor and critic, the target value selected by torch.where
    as torch_ddpg_update selects it), Adam at the row's betas, eps, rates and the fixture's step count, the Polyak step at the row's
    tau -> (stats [4], {label: gradient}, {label: (w', m', v')}, {label: target'})"""
    import torch
    from test_ddpg_cpu import _t_actor, _t_critic
    from test_nonfinite_cpu import _adam_t
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))      # noqa: E731
    P = {n: [t64(F["P"][n][k]) for k in dd.KEYS] for n in dd.NETS}
    o0, act, rew, o1, done = (t64(a) for a in hc.rows_of(F))
    o0c, o1c = o0.clamp(-hp["obs_clip"], hp["obs_clip"]), o1.clamp(-hp["obs_clip"], hp["obs_clip"])
    with torch.no_grad():
        q1 = _t_critic(torch, P["critic_target"], o1c, _t_actor(torch, P["actor_target"], o1c))
        y = torch.where(done >= 1.0, rew, rew + (1.0 - done) * hp["gamma"] * q1)
    A = [w.clone().requires_grad_(True) for w in P["actor"]]
    Cr = [w.clone().requires_grad_(True) for w in P["critic"]]
    q = _t_critic(torch, Cr, o0c, act)
    closs = ((q - y) ** 2).mean()
    g_c = torch.autograd.grad(closs, Cr)
    aloss = -_t_critic(torch, [w.detach() for w in Cr], o0c, _t_actor(torch, A, o0c)).mean()
    g_a = torch.autograd.grad(aloss, A)
    stats = np.array([float(x.detach()) for x in (closs, aloss, q.mean(), y.mean())])
    G, new, tgt = {}, {}, {}
    for n, gs in (("actor", g_a), ("critic", g_c)):
        for i, k in enumerate(dd.KEYS):
            lab = "%s/%s" % (n, k)
            G[lab] = gs[i].numpy()
            w, m, v = _adam_t(torch, P[n][i], t64(F["M"][n][k]), t64(F["V"][n][k]), gs[i], F["t0"] + 1, hp[n + "_lr"], *hc.adam_args(hp))
            new[lab] = (w.numpy(), m.numpy(), v.numpy())
            tgt[lab] = ((1.0 - hp["tau"]) * P[n + "_target"][i] + hp["tau"] * w).numpy()
    return stats, G, new, tgt


@pytest.mark.parametrize("row", [pytest.param(r, id=r["id"]) for r in hc.TABLES["ddpg"]])
def test_ddpg_reference_against_float64_autograd(row):
    """every row, the betas and eps included: statistics, gradients, w, m, v after Adam and the targets after the Polyak step"""
    F, hp = hc.fixture_of("ddpg", row), hc.hyper_of("ddpg", row)
    ref, new = _after("ddpg", F, hp)
    stats, G, anew, tgt = _ddpg_autograd64(F, hp)
    assert np.allclose(stats, ref["stats"], **F64_STATS), (row["id"], stats, ref["stats"])
    for lab in ref["G"]:
        n, k = lab.split("/")
        assert np.allclose(G[lab].reshape(ref["G"][lab].shape), ref["G"][lab], **F64_TENSORS), (row["id"], lab, "gradient")
        for got, want, p in zip(anew[lab], new[lab], "wmv"):
            assert np.allclose(got.reshape(want.shape), want, **F64_TENSORS), (row["id"], lab, p)
        want = (1.0 - hp["tau"]) * np.asarray(F["P"][n + "_target"][k], np.float64) + hp["tau"] * new[lab][0]
        assert np.allclose(tgt[lab].reshape(want.shape), want, **F64_TENSORS), (row["id"], lab, "target")


@pytest.mark.parametrize("row", _wrapper_rows("ddpg"))
def test_torch_ddpg_update_on_the_host_within_the_references_bounds(row):
    import torch
    import quadsim_amd as qa
    F, hp = hc.fixture_of("ddpg", row), hc.hyper_of("ddpg", row)
    own = {k: hp[k] for k in nc.DDPG_HYPER}
    # float32 on the host: the package's own torch path, within the bounds of step64 at the row's gamma, from the fixture's step count
    ref = hc.step64("ddpg", F, hp)
    pol = qa.DDPGPolicy(device="cpu", weights={n: {k: F["P"][n][k].copy() for k in dd.KEYS} for n in dd.NETS})
    for n in nc.DDPG_ONLINE:
        pol.m[n] = [torch.as_tensor(F["M"][n][k].copy()) for k in dd.KEYS]
        pol.v[n] = [torch.as_tensor(F["V"][n][k].copy()) for k in dd.KEYS]
    pol.steps = F["t0"]
    out = qa.torch_ddpg_update(pol, tuple(torch.as_tensor(a) for a in F["rp"]), torch.as_tensor(F["idx"]), return_grads=True, **own)
    assert np.all(np.abs(out["stats"][0].double().numpy() - ref["stats"]) <= ref["Es"]), (row["id"], out["stats"], ref["stats"])
    for n in nc.DDPG_ONLINE:
        for i, k in enumerate(dd.KEYS):
            lab = "%s/%s" % (n, k)
            g = out["grads"][n][i].numpy().reshape(ref["G"][lab].shape)
            assert np.all(np.abs(g.astype(np.float64) - ref["G"][lab]) <= ref["E"][lab]), (row["id"], lab)
            w, m, v = hc.tensors("ddpg", F)[lab]
            want = dd.adam64(w, m, v, g, ref["t"][lab], ref["lr"][lab])[0]
            bound = dd.adam_bound(w, m, v, g, ref["t"][lab], ref["lr"][lab])[0]
            assert np.all(np.abs(getattr(pol, n)[i].numpy() - want) <= bound), (row["id"], lab, "w")
            # the target at the row's tau, from its own updated weight: three float32 roundings of O(|t| + |w|)
            t0_, w1 = np.asarray(F["P"][n + "_target"][k], np.float64), getattr(pol, n)[i].double().numpy()
            tw = (1.0 - hp["tau"]) * t0_ + hp["tau"] * w1
            assert np.all(np.abs(getattr(pol, n + "_target")[i].double().numpy() - tw) <= dd.gamma(4) * (np.abs(t0_) + np.abs(w1)) + dd.TINY), (row["id"], lab, "target")


# ---------------------------------------------------------------------------------------------------- TRPO's solver settings
@pytest.mark.parametrize("row", hc.TRPO_STEP_CASES, ids=[r["id"] for r in hc.TRPO_STEP_CASES])
def test_trpo_solver_setting_is_accepted_and_moves_its_statistic(row):
    """the solver's results are replayed bit for bit on the device, so there is no bound to count in: the statistic the setting is
    about differs between trpo_ref.step64 at the case and at the defaults (printed), and both are finite"""
    from quadsim_amd import trpo
    hp = dict(hc.TRPO_STEP_DEFAULT, **row["hyper"])
    assert trpo.check_trpo_args(hc.TRPO_STEP_N, hc.TRPO_STEP_SLICES, **hp)[2]["cg_iters"] == hp["cg_iters"]
    W, data = hc.trpo_step_fixture()
    case, twin = hc.tr.step64(W, data, **hp), hc.tr.step64(W, data, **hc.TRPO_STEP_DEFAULT)
    i = hc.tr.STAT_NAMES.index(row["about"][5:])
    print("hyper trpo %s: %s %.6g at the case, %.6g at the defaults; cg iterations %d / %d, accepted %d / %d" % (
        row["id"], row["about"][5:], case["stats"][i], twin["stats"][i], case["iters"], twin["iters"], case["accepted"], twin["accepted"]))
    assert np.isfinite(case["stats"]).all() and case["stats"][i] != twin["stats"][i], (row["id"], case["stats"], twin["stats"])


def test_trpo_out_of_range_neighbours_are_refused():
    from quadsim_amd import trpo
    for name, bad in (("cg_iters", 0), ("cg_iters", trpo.TRPO_MAX_CG_ITERS + 1), ("backtracks", 0), ("max_kl", 0.0), ("cg_damping", -1.0e-3)):
        with pytest.raises(ValueError, match=name):
            trpo.check_trpo_args(hc.TRPO_STEP_N, hc.TRPO_STEP_SLICES, **dict(hc.TRPO_STEP_DEFAULT, **{name: bad}))
    assert trpo.TRPO_MAX_CG_ITERS == 64


# ---------------------------------------------------------------------------------------------------- PPO2, GAIL, TRPO's value fit
def _t64(a):
    import torch
    return torch.tensor(np.asarray(a, np.float64))


def _all_rows(trainer):
    return _params({trainer: hc.TABLES[trainer] + hc.EXTRA.get(trainer, ())})


@pytest.mark.parametrize("trainer, row, variant", _all_rows("ppo2"))
def test_ppo2_reference_against_float64_autograd_of_ppo2_loss(trainer, row, variant, monkeypatch):
    """every PPO2 row of both layouts, hyper_cases.EXTRA included: backward64's statistics and gradients against float64 autograd of
    quadsim_amd.ppo2.ppo2_loss at the row's coefficients (cliprange 0 and 10, cliprange_vf 0, ent_coef 0, vf_coef 0: settings no
    earlier test ran the reference at), and update64 at the row's max_grad_norm, betas and eps against the arbiter's
    tf.clip_by_global_norm + Adam of tests/test_nonfinite_cpu.py on the same gradients"""
    import torch
    import test_nonfinite_cpu as tn
    from quadsim_amd.ppo2 import ppo2_loss
    pr = hc.pr
    F, hp = hc.fixture_of(trainer, row, variant), hc.hyper_of(trainer, row)
    ref = hc.step64(trainer, F, hp)
    d = {k: _t64(v[F["rows"]]) for k, v in F["data"].items()}
    T = {k: _t64(F["W"][k]).requires_grad_(True) for k in pr.keys_of(F["W"])}
    loss, parts = ppo2_loss(torch, T, d["obs"], d["actions"], d["returns"], d["values"], d["neglogp"], hp["cliprange"], hp["cliprange_vf"],
                            hp["ent_coef"], hp["vf_coef"])
    G = dict(zip(T, torch.autograd.grad(loss, list(T.values()))))
    norm = float(torch.sqrt(sum((g ** 2).sum() for g in G.values())))
    stats = np.array([float(p.detach()) for p in parts] + [norm])
    # (the reference clips the ratio at float32(1 +- eps), torch at the doubles: tests/test_nonfinite_cpu.py's tolerance for these)
    assert np.allclose(stats, ref["stats"], rtol=1e-6, atol=1e-9), (row["id"], stats, ref["stats"])
    assert stats[4] == ref["stats"][4], (row["id"], "the clip fraction")
    for k in ref["G"]:
        assert np.allclose(G[k].numpy().reshape(ref["G"][k].shape), ref["G"][k], **F64_TENSORS), (row["id"], k, "gradient")
    b1, b2, eps = hc.adam_args(hp)
    for name, val in (("BETA1", b1), ("BETA2", b2), ("EPS", eps)):
        monkeypatch.setattr(pr, name, val)                         # _ppo2_clip_adam_t reads the module's constants when it is called
    own = {k: hp[k] for k in pr.HP_VCLIP}
    t = F["t0"] + 1
    Wt, Mt, Vt, _ = tn._ppo2_clip_adam_t(torch, *({k: _t64(a[k]) for k in G} for a in (F["W"], F["M"], F["V"])), G, own, t)
    Gn = {k: G[k].numpy() for k in G}
    Wn, Mn, Vn, scale, _ = pr.update64(F["W"], F["M"], F["V"], Gn, own, t, b1, b2, eps)
    assert (scale == 1.0) == (hp["max_grad_norm"] <= 0.0 or norm <= hp["max_grad_norm"]), (row["id"], scale, norm)
    for got, want, start in ((Wn, Wt, F["W"]), (Mn, Mt, F["M"]), (Vn, Vt, F["V"])):
        for k in G:
            # tests/test_nonfinite_cpu.py's 1e-12, relative to the operands of the last subtraction: at beta2 = 0 an element whose
            # gradient is tiny moves by tens, and where w - step cancels the result itself is no measure of two float64 evaluations
            w = want[k].numpy()
            size = np.abs(np.asarray(start[k], np.float64)) + np.abs(w - np.asarray(start[k], np.float64))
            assert np.all(np.abs(got[k] - w) <= 1e-12 * size), (row["id"], k)


@pytest.mark.parametrize("trainer, row, variant", _params({"ppo2": tuple(r for r in hc.TABLES["ppo2"] + hc.EXTRA["ppo2"]
                                                                            if not set(r["hyper"]) & {"beta1", "beta2", "eps"})}))
def test_torch_ppo2_update_on_the_host_within_the_references_bounds(trainer, row, variant):
    """the package's own torch path, float32 on the host, at the rows it takes (it has no betas and no eps): its statistics and
    gradients within backward64's bounds at the row, its update within update_bound of update64 on its own gradient"""
    import torch
    import quadsim_amd as qa
    from quadsim_amd import ppo2
    pr = hc.pr
    F, hp = hc.fixture_of(trainer, row, variant), hc.hyper_of(trainer, row)
    ref = hc.step64(trainer, F, hp)
    pol = qa.ActorCriticPolicy({k: v.copy() for k, v in F["W"].items()}, device="cpu")
    ws = ppo2.policy_tensors(pol)
    ppo2.reset_ppo2_optimizer(pol)
    pol._ppo_m = [None if w is None else torch.as_tensor(F["M"][k].copy()) for k, w in zip(ppo2.SLOT_KEYS, ws)]
    pol._ppo_v = [None if w is None else torch.as_tensor(F["V"][k].copy()) for k, w in zip(ppo2.SLOT_KEYS, ws)]
    pol._ppo_steps = F["t0"]
    out = ppo2.torch_ppo2_update(pol, {k: torch.as_tensor(v) for k, v in F["data"].items()}, torch.as_tensor(F["rows"][None, :].copy()),
                                 learning_rate=hp["lr"], cliprange=hp["cliprange"], cliprange_vf=hp["cliprange_vf"], ent_coef=hp["ent_coef"],
                                 vf_coef=hp["vf_coef"], max_grad_norm=hp["max_grad_norm"], return_grads=True)
    err = np.abs(out["stats"][0].double().numpy() - ref["stats"])
    assert np.all(err <= ref["Es"]), (row["id"], err / ref["Es"])
    Gd = {k: g.numpy().reshape(ref["G"][k].shape) for k, g in zip(ppo2.SLOT_KEYS, out["grads"]) if g is not None}
    for k in ref["G"]:
        assert np.all(np.abs(Gd[k].astype(np.float64) - ref["G"][k]) <= ref["E"][k]), (row["id"], k, "gradient")
    new, bound = hc.after64(trainer, F, hp, Gd, ref["t"], ref["lr"])
    after = {k: w for k, w in zip(ppo2.SLOT_KEYS, ppo2.policy_tensors(pol)) if w is not None}
    for k in ref["G"]:
        assert np.all(np.abs(after[k].detach().double().numpy().reshape(new[k][0].shape) - new[k][0]) <= bound[k][0]), (row["id"], k, "w")


@pytest.mark.parametrize("hidden", hc.gr.HIDDENS)
@pytest.mark.parametrize("entcoeff", [0.0, hc.gr.ENTCOEFF, 0.1])
def test_gail_reference_against_float64_autograd_at_every_entcoeff(hidden, entcoeff):
    """gail_ref.backward64 at entcoeff 0 and 0.1 (and the default), every hidden width: the three losses and every gradient against
    float64 autograd of tests/test_gail_cpu.py's loss on the input row tests/test_nonfinite_cpu.py builds"""
    import torch
    import test_nonfinite_cpu as tn
    from test_gail_cpu import _torch_total
    gr = hc.gr
    F = hc.fixture("gail", str(hidden))
    hp = dict(hc.DEFAULTS["gail"], entcoeff=entcoeff)
    ref = hc.step64("gail", F, hp)
    g, e = F["gi"][0], F["ei"][0]
    x = torch.cat([tn._gail_x(torch, F["gen"][0][g], F["gen"][1][g], F["mean"], F["rscale"]),
                   tn._gail_x(torch, F["exp"][0][e], F["exp"][1][e], F["mean"], F["rscale"])])
    T = {k: _t64(F["W"][k]).requires_grad_(True) for k in gr.KEYS}
    total, parts = _torch_total(torch, T, x, hc.BATCH, entcoeff)
    G = dict(zip(T, torch.autograd.grad(total, list(T.values()))))
    assert np.allclose([float(p.detach()) for p in parts], ref["stats"][:3], **F64_STATS), (hidden, entcoeff, parts, ref["stats"])
    for k in gr.KEYS:
        assert np.allclose(G[k].numpy().reshape(ref["G"][k].shape), ref["G"][k], **F64_TENSORS), (hidden, entcoeff, k)


@pytest.mark.parametrize("trainer, row, variant", _all_rows("trpo_vf"))
def test_torch_trpo_vf_fit_on_the_host_within_the_references_bounds(trainer, row, variant):
    """quadsim_amd.torch_trpo_vf_fit takes betas and eps: float32 on the host at every row, its loss and gradients within
    vf_backward64's bounds, its update within vf_update_bound of adam64 on its own gradient; and the reference's loss and gradients
    against float64 autograd (tests/test_nonfinite_cpu.py's restatement of the value tower)"""
    import torch
    import quadsim_amd as qa
    from quadsim_amd import trpo
    tr = hc.tr
    F, hp = hc.fixture_of(trainer, row, variant), hc.hyper_of(trainer, row)
    ref = hc.step64(trainer, F, hp)
    rows = F["idx"][0]
    T = {k: _t64(F["W"][k]).requires_grad_(True) for k in tr.VALUE_KEYS}
    h = torch.relu(torch.relu(_t64(F["data"]["obs"][rows]) @ T["wv0"] + T["bv0"]) @ T["wv1"] + T["bv1"])
    loss = (((h @ T["wv2"] + T["bv2"])[:, 0] - _t64(F["data"]["returns"][rows])) ** 2).mean()
    G64 = dict(zip(T, torch.autograd.grad(loss, list(T.values()))))
    assert np.allclose(float(loss.detach()), ref["stats"][0], **F64_STATS)
    for k in tr.VALUE_KEYS:
        assert np.allclose(G64[k].numpy().reshape(ref["G"][k].shape), ref["G"][k], **F64_TENSORS), (row["id"], k)
    pol = qa.ActorCriticPolicy({k: v.copy() for k, v in F["W"].items()}, device="cpu")
    ws = trpo.policy_tensors(pol)
    trpo.reset_trpo_optimizer(pol)
    m, v = trpo._state(pol, ws)
    for i, k in zip(trpo.VALUE_SLOTS, tr.VALUE_KEYS):
        m[i].copy_(torch.as_tensor(F["M"][k]).reshape(m[i].shape))
        v[i].copy_(torch.as_tensor(F["V"][k]).reshape(v[i].shape))
    pol._trpo_steps = F["t0"]
    data = {k: torch.as_tensor(a) for k, a in F["data"].items()}
    out = qa.torch_trpo_vf_fit(pol, dict(data, neglogp=data["values"]), torch.as_tensor(F["idx"].copy()), vf_stepsize=hp["lr"], beta1=hp["beta1"],
                               beta2=hp["beta2"], eps=hp["eps"], return_grads=True)
    assert abs(float(out["stats"][0]) - ref["stats"][0]) <= ref["Es"][0], row["id"]
    Gd = {k: g.numpy().reshape(ref["G"][k].shape) for k, g in zip(tr.VALUE_KEYS, out["grads"])}
    for k in tr.VALUE_KEYS:
        assert np.all(np.abs(Gd[k].astype(np.float64) - ref["G"][k]) <= ref["E"][k]), (row["id"], k, "gradient")
    new, bound = hc.after64(trainer, F, hp, Gd, ref["t"], ref["lr"])
    for i, k in zip(trpo.VALUE_SLOTS, tr.VALUE_KEYS):
        got = trpo.policy_tensors(pol)[i].detach().double().numpy().reshape(new[k][0].shape)
        assert np.all(np.abs(got - new[k][0]) <= bound[k][0]), (row["id"], k, "w")
