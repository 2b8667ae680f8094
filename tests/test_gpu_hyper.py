"""The seven trainers on the device across their hyper-parameter ranges: every row of tests/hyper_cases.py through the raw entry
point, in the sentinel-guarded runners of tests/test_gpu_ddpg.py, tests/test_gpu_td3.py (run_update), tests/test_gpu_dynfit.py,
tests/test_gpu_bcfit.py (run), tests/test_gpu_gail.py (run_fit), tests/test_gpu_ppo2.py (run) and tests/test_gpu_trpo.py (vf_fit),
against the float64 references that tests/test_hyper_cases_cpu.py anchors and separates from their twins first.  What is held:
  every row    one step of 17 rows from non-zero moments at the row's hyper-parameters: the statistics and every gradient element
               within the bounds of the reference's step at those hyper-parameters, and w, m, v of every trained tensor within
               adam_bound (update_bound, vf_update_bound) of adam64 (update64) on the device's OWN gradient, both called with the
               row's betas, eps and rate(s).  Every ratio is printed
  betas (0,0)  m' is bit for bit the gradient and v' bit for bit fl(g g)
  rates        lr = 0: the weights keep their bits, the moments move, DDPG's and TD3's targets still take their Polyak step;
               actor_lr = 0: the actor keeps its bits, the critics do not; actor_lr != critic_lr, either way round, through
               ddpg_update and td3_update: bit for bit the raw call
  step counter t0 = 10^5 and 2^31 - 2 for GAIL's fit, TRPO's value fit, DDPG and TD3 (its actor's count the other of the two), as
               test_step_counter_at_its_upper_edge has it for behaviour cloning; t0 = 2^31 - 1 is refused
  gamma        0: bit for bit the run with done = 1 on every row, y_mean the float32 ascending sum of rew; 0.5 and 1: y_mean bit for
               bit from the header's formula restated in numpy float32; 0, 0.5 and 1 within step64(gam=..) on target critics whose
               values are O(1) (hyper_cases.SHIFT)
  tau          the targets bit for bit polyak32(.., tau) at 0.5, at 1e-9 (float32(1 - tau) is 1) and at a tau where 1 - tau formed in
               float32 would differ (hyper_cases.TAU_ODD)
  smoothing    TD3: target_noise_clip = 0 is target_policy_noise = 0; sigma 4 with clip 0.5 acts as the noise clipped at 0.125
  delay        TD3: policy_delay 65536, an actor step at t0 = 65536 and none at 65535; 65537 is refused
  PPO2         max_grad_norm -1, 0 and 1e6 give the same bits; vf_coef = 0 leaves the value tower's gradients exactly 0
  GAIL         entcoeff 0 and 0.1 at every hidden width of gail_ref.HIDDENS
  TRPO         the policy step at max_kl 1e-4 and 1, cg_damping 0 and 1, cg_iters 1 and 64, backtracks 1: the solver replayed bit for
               bit from the device's own products, the products and the candidates within fvp64's and ls_eval64's bounds
The rows of hyper_cases.EXTRA (the float64 reference cannot tell them from their twins by its bounds) run within the bounds as well.
No case has more than two steps of 17 rows.  Measured ratios: profiles/hyper/README.md."""
import numpy as np
import pytest

import ddpg_ref as dd
import gail_ref as gr
import hyper_cases as hc
import mppi_ref
import nonfinite_cases as nc
import ppo2_ref as pr
import td3_ref as td
import test_gpu_bcfit as tgb
import test_gpu_ddpg as tgd
import test_gpu_dynfit as tgf
import test_gpu_gail as tgg
import test_gpu_ppo2 as tgp
import test_gpu_td3 as tgt
import test_gpu_trpo as tgr
import trpo_ref as tr

pytestmark = pytest.mark.gpu

same_bits = tgd.same_bits
f32 = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _cases():
    out = []
    for trainer, rows in hc.TABLES.items():
        rows = rows + hc.EXTRA.get(trainer, ())
        for variant in (hc.PPO2_LAYOUTS if trainer == "ppo2" else (None,)):
            out += [pytest.param(trainer, row, variant, id="-".join(x for x in (trainer, variant, row["id"]) if x)) for row in rows]
    return out


def row_of(trainer, cid):
    (row,) = [r for r in hc.TABLES[trainer] + hc.EXTRA.get(trainer, ()) if r["id"] == cid]
    return row


# ---------------------------------------------------------------------------------------------------- one uniform run
_buffers = {}


def _flat(nested, nets):
    return {"%s/%s" % (n, k): nested[n][k] for n in nets for k in dd.KEYS}


def run(torch, trainer, F, hp, t0=None, actor_t0=None, **kw):
    """one call of the trainer's guarded runner on the fixture at the hyper-parameters -> dict(stats [steps, n], grads, w, m, v:
    {label: float32 array} of the trained tensors, targets: {label of the online tensor: its target} (DDPG, TD3), raw)"""
    t0 = F["t0"] if t0 is None else t0
    adam = dict(beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"])
    if trainer == "td3":
        own = {k: hp[k] for k in nc.TD3_HYPER}
        raw = tgt.run_update(torch, F["P"], F["M"], F["V"], kw.pop("rp", F["rp"]), kw.pop("idx", F["idx"]), t0=t0,
                             actor_t0=F["actor_t0"] if actor_t0 is None else actor_t0, noise=kw.pop("noise", F["z"]), want_grads=True, **adam,
                             **own, **kw)
        nets = td.ONLINE
    elif trainer == "ddpg":
        own = {k: hp[k] for k in nc.DDPG_HYPER}
        raw = tgd.run_update(torch, F["P"], F["M"], F["V"], kw.pop("rp", F["rp"]), kw.pop("idx", F["idx"]), t0=t0, want_grads=True, **adam, **own,
                             **kw)
        nets = nc.DDPG_ONLINE
    if trainer in ("td3", "ddpg"):
        out = dict(stats=raw["stats"], raw=raw, grads=_flat(raw["grads"], nets), targets=_flat({n: raw["w"][n + "_target"] for n in nets}, nets))
        out.update({p: _flat(raw[p], nets) for p in "wmv"})
        return out
    if trainer == "dynfit":
        if "dynfit" not in _buffers:
            _buffers["dynfit"] = tuple(torch.as_tensor(a).cuda().contiguous() for a in (F["x"], F["d"]))
        raw = tgf.run(torch, F["W"], F["M"], F["V"], _buffers["dynfit"], 1, hc.BATCH, lr=hp["lr"], t0=t0, indices=F["idx"], want_grads=True, **adam)
        stats = raw["loss"][:, None]
    elif trainer == "bc":
        if "bc" not in _buffers:
            _buffers["bc"] = tuple(torch.as_tensor(a).cuda().contiguous() for a in F["data"])
        raw = tgb.run(torch, F["W"], F["M"], F["V"], _buffers["bc"], F["idx"], lr=hp["lr"], t0=t0, want_grads=True, **adam)
        stats = raw["loss"][:, None]
    elif trainer == "gail":
        raw = tgg.run_fit(torch, F["W"], F["M"], F["V"], F["gen"], F["exp"], F["mean"], F["rscale"], F["gi"], F["ei"], lr=hp["lr"], t0=t0,
                          entcoeff=hp["entcoeff"], want_grads=True, **adam)
        stats = raw["stats"]
    elif trainer == "ppo2":
        own = {k: hp[k] for k in pr.HP_VCLIP}
        raw = tgp.run(torch, F["W"], F["M"], F["V"], F["data"], F["rows"][None, :], own, slices=kw.pop("slices", 1), t0=t0, want_grads=True, **adam)
        stats = raw["stats"]
    elif trainer == "trpo_vf":
        M, V = ({k: np.array(a[k]) if k in a else np.zeros(pr.SHAPES[k], f32) for k in nc.TRPO_KEYS} for a in (F["M"], F["V"]))
        raw = tgr.vf_fit(torch, F["W"], M, V, F["data"], F["idx"], t0=t0, lr=hp["lr"], **adam)
        raw = dict(raw, w=raw["W"], m=raw["M"], v=raw["V"])
        stats = raw["stats"][:, None]
    else:
        raise KeyError(trainer)
    labels = list(hc.tensors(trainer, F))
    out = dict(stats=stats, raw=raw, grads={k: raw["grads"][k] for k in labels})
    out.update({p: {k: raw[p][k] for k in labels} for p in "wmv"})
    return out


def _ratio(got, want, bound):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / np.asarray(bound, np.float64))
    return float(np.max(r))


def check_step(trainer, F, hp, out, what, t0=None, actor_t0=None):
    """the statistics and gradients of step 1 within the reference's bounds at the hyper-parameters; w, m, v within the update's
    bounds of the float64 update on the device's own gradient, at the hyper-parameters' betas, eps and rates -> the worst ratios"""
    ref = hc.step64(trainer, F, hp, t0=t0, actor_t0=actor_t0)
    worst = {"statistics": _ratio(out["stats"][0], ref["stats"], ref["Es"])}
    labels = list(ref["G"])
    worst["gradients"] = max(_ratio(out["grads"][k], ref["G"][k], ref["E"][k]) for k in labels)
    Gd = {k: out["grads"][k] for k in labels}
    new, bound = hc.after64(trainer, F, hp, Gd, ref["t"], ref["lr"])
    for i, p in enumerate("wmv"):
        worst["adam " + p] = max(_ratio(out[p][k], new[k][i], bound[k][i]) for k in labels)
    print("hyper %s: worst error / bound %s" % (what, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert all(np.isfinite(r) and r < 1.0 for r in worst.values()), (what, worst)
    assert np.isfinite(out["stats"]).all(), what
    return ref, new, bound


# ---------------------------------------------------------------------------------------------------- every row of every table
@pytest.mark.parametrize("trainer, row, variant", _cases())
def test_case_within_the_references_bounds(torch, trainer, row, variant):
    F, hp = hc.fixture_of(trainer, row, variant), hc.hyper_of(trainer, row)
    what = "%s %s%s" % (trainer, (variant + " ") if variant else "", row["id"])
    out = run(torch, trainer, F, hp)
    ref, new, bound = check_step(trainer, F, hp, out, what)
    T = hc.tensors(trainer, F)
    labels = list(ref["G"])
    if hp["beta1"] == 0.0 and (trainer != "ppo2" or hp["max_grad_norm"] <= 0.0):
        # m' = fma(0, m, 1 g): the gradient itself
        assert all(same_bits(out["m"][k], out["grads"][k]) for k in labels), (what, "m' is not the gradient bit for bit")
    if hp["beta2"] == 0.0 and (trainer != "ppo2" or hp["max_grad_norm"] <= 0.0):
        # v' = fma(0, v, 1 (g g)): the rounded square
        assert all(same_bits(out["v"][k], (out["grads"][k] * out["grads"][k]).astype(f32)) for k in labels), (what, "v' is not fl(g g)")
    zero_rate = [k for k in labels if ref["lr"][k] == 0.0]
    for k in labels:
        moved = not same_bits(out["w"][k], T[k][0])
        assert moved == (k not in zero_rate), (what, k, "a rate of 0 keeps the weight's bits, any other rate moves it")
        assert not same_bits(out["m"][k], T[k][1]) and not same_bits(out["v"][k], T[k][2]), (what, k, "the moments move at any rate")
    if row["id"] == "actor-lr-0":
        assert sorted(zero_rate) == sorted(k for k in labels if k.startswith("actor/"))
    if "targets" in out:
        # the Polyak step on the device's own updated weights, the header's formula in float32: also where the rate is 0
        for k in labels:
            n, key = k.split("/")
            assert same_bits(out["targets"][k], dd.polyak32(F["P"][n + "_target"][key], out["w"][k], hp["tau"])), (what, k, "target")
        # (at tau = 1e-9 an element moves only where tau w' reaches half an ulp of the target: some small tensors keep every bit)
        moved = [k for k in labels if not same_bits(out["targets"][k], F["P"][k.split("/")[0] + "_target"][k.split("/")[1]])]
        assert moved if hp["tau"] < 1e-6 else moved == labels, (what, "the targets that moved", moved)
    if trainer == "ppo2" and row["id"] == "vf-coef-0" and variant == "towers":
        assert all(not out["grads"][k].any() for k in tr.VALUE_KEYS), (what, "the value tower's gradients are not exactly 0")
        assert all(not same_bits(out["w"][k], T[k][0]) for k in tr.VALUE_KEYS), (what, "the decaying moments still move the tower")
    if trainer == "ppo2" and row["id"].startswith("cliprange"):
        edges, _ = pr.edge_counts(F["W"], pr.minibatch(F["data"], F["rows"]), {k: hp[k] for k in pr.HP_VCLIP})
        left_out = edges["ratio at 1 +- eps"]
        print("hyper %s: %d of %d rows within their bound of the clip edge" % (what, left_out, hc.BATCH))
        assert left_out <= 2
        # the rows off the edge are counted as the reference counts them: the two counts differ by at most the rows left out
        assert abs(round(float(out["stats"][0, 4]) * hc.BATCH) - round(ref["stats"][4] * hc.BATCH)) <= left_out, (what, out["stats"][0, 4], ref["stats"][4])
        if left_out == 0:
            # the same count of clipped rows: the statistic is that count over float32(rows)
            assert same_bits(out["stats"][0, 4], f32(f32(round(ref["stats"][4] * hc.BATCH)) / f32(hc.BATCH))), (what, "the clip fraction")
        if row["id"] == "cliprange-10":
            assert out["stats"][0, 4] == 0.0


# ---------------------------------------------------------------------------------------------------- the rates through the wrappers
@pytest.mark.parametrize("trainer", ["ddpg", "td3"])
@pytest.mark.parametrize("cid", ["actor-3e-3-critic-1e-2", "actor-1e-2-critic-3e-3"])
def test_unequal_rates_through_the_wrapper_equal_the_raw_call(torch, trainer, cid):
    import quadsim_amd as qa
    row = row_of(trainer, cid)
    F, hp = hc.fixture_of(trainer, row), hc.hyper_of(trainer, row)
    raw = run(torch, trainer, F, hp)["raw"]
    mod = {"ddpg": tgd, "td3": tgt}[trainer]
    pol = mod._policy(torch, F["P"], F["M"], F["V"])
    pol.steps = F["t0"]
    rp = tuple(mod.dev(torch, a) for a in F["rp"])
    if trainer == "td3":
        pol.actor_steps = F["actor_t0"]
        out = qa.td3_update(pol, rp, torch.as_tensor(F["idx"]), noise=torch.as_tensor(F["z"]).cuda(), **{k: hp[k] for k in nc.TD3_HYPER})
        nets, online = td.NETS, td.ONLINE
    else:
        out = qa.ddpg_update(pol, rp, torch.as_tensor(F["idx"]), **{k: hp[k] for k in nc.DDPG_HYPER})
        nets, online = dd.NETS, nc.DDPG_ONLINE
    torch.cuda.synchronize()
    assert same_bits(out["stats"].cpu().numpy(), raw["stats"]), (trainer, cid, out["stats"], raw["stats"])
    for n in nets:
        assert all(same_bits(w.cpu().numpy(), raw["w"][n][k]) for k, w in zip(dd.KEYS, getattr(pol, n))), (trainer, cid, n)
    for n in online:
        assert all(same_bits(t.cpu().numpy(), raw["m"][n][k]) for k, t in zip(dd.KEYS, pol.m[n])), (trainer, cid, "m", n)
        assert all(same_bits(t.cpu().numpy(), raw["v"][n][k]) for k, t in zip(dd.KEYS, pol.v[n])), (trainer, cid, "v", n)
    # and the run is not the swapped one's: the two rates are arguments of their own
    swapped = run(torch, trainer, F, hc.hyper_of(trainer, row, twin=True))["raw"]
    assert all(not same_bits(swapped["w"][n][k], raw["w"][n][k]) for n in online for k in dd.KEYS), (trainer, cid)


# ---------------------------------------------------------------------------------------------------- the step counter
def _counter_step(torch, trainer, t0, actor_t0=None):
    F, hp = hc.fixture(trainer), hc.DEFAULTS[trainer]
    what = "%s t0 %d%s" % (trainer, t0, "" if actor_t0 is None else " actor_t0 %d" % actor_t0)
    out = run(torch, trainer, F, hp, t0=t0, actor_t0=actor_t0)
    ref, new, bound = check_step(trainer, F, hp, out, what, t0=t0, actor_t0=actor_t0)
    T = hc.tensors(trainer, F)
    for k in ref["G"]:
        # a wrong update is far outside: the step itself is many bounds long
        assert np.median(np.abs(new[k][0] - T[k][0]) / bound[k][0]) > 100.0, (what, k)
    return ref


@pytest.mark.parametrize("trainer", ["gail", "trpo_vf", "ddpg"])
def test_step_counter_at_its_upper_edge(torch, trainer):
    """t0 = 2^31 - 2 is the last step the contract takes: as t = 2^31 - 1 it enters Adam's bias correction (GAIL and TRPO's value
    fit: a float64 pow on the device; DDPG: on the host), where both powers have underflowed and lr_t = lr"""
    from quadsim_amd import QuadsimError
    for t0 in hc.T_EDGE:
        _counter_step(torch, trainer, t0)
    assert dd.lr_t64(2 ** 31 - 1, 1e-2) == 1e-2
    with pytest.raises((QuadsimError, AssertionError), match="t0"):
        run(torch, trainer, hc.fixture(trainer), hc.DEFAULTS[trainer], t0=2 ** 31 - 1)


@pytest.mark.parametrize("t0, actor_t0", [(2 ** 31 - 2, 10 ** 5), (10 ** 5, 2 ** 31 - 2)])
def test_td3_step_counters_at_their_upper_edges(torch, t0, actor_t0):
    """both t0 are even: an actor step at delay 2.  The critics' correction is taken at t0 + 1, the actor's at actor_t0 + 1 (in
    float64 both factors are exactly 1 from t = 10^5 on: what is held is that either counter is accepted at the edge, enters the
    host's float64 pow and leaves an update within the bounds)"""
    from quadsim_amd import QuadsimError
    ref = _counter_step(torch, "td3", t0, actor_t0)
    assert ref["t"]["actor/w0"] == actor_t0 + 1 and ref["t"]["q1/w0"] == t0 + 1
    assert dd.lr_t64(10 ** 5 + 1, 1e-2) == dd.lr_t64(2 ** 31 - 1, 1e-2) == 1e-2
    F, hp = hc.fixture("td3"), hc.DEFAULTS["td3"]
    with pytest.raises(QuadsimError, match="t0"):
        run(torch, "td3", F, hp, t0=2 ** 31 - 1, actor_t0=0)
    with pytest.raises(QuadsimError, match="actor_t0"):
        run(torch, "td3", F, hp, t0=0, actor_t0=2 ** 31 - 1)


# ---------------------------------------------------------------------------------------------------- the discount
def _layer32(w, b, h):
    """one layer in numpy float32 in the header's order: one fma per term, k ascending from the bias"""
    w, b = np.asarray(w, f32), np.asarray(b, f32)
    acc = np.broadcast_to(b[None, :], (h.shape[0], w.shape[1])).astype(f32)
    for k in range(w.shape[0]):
        acc = mppi_ref.fma32(np.broadcast_to(w[k][None, :], acc.shape), np.broadcast_to(h[:, k:k + 1], acc.shape), acc)
    return acc


def _relu32(z):
    return np.where(z <= 0.0, f32(0.0), z)


def _mean32(y):
    acc = f32(0.0)
    for v in np.asarray(y, f32):
        acc = f32(acc + v)
    return f32(acc / f32(len(y)))


def _y32(rows, q, gamma):
    """y = done >= 1 ? rew : fma((1 - done) G, q, rew), G = float32(gamma)"""
    rew, done = rows[2], rows[4]
    k = ((f32(1.0) - done) * f32(gamma)).astype(f32)
    return np.where(done >= 1.0, rew, mppi_ref.fma32(k, q, rew)).astype(f32)


def _flat_targets(trainer, P):
    """one target critic, and a target actor whose head is zero (tanh(0) = 0 exactly): the target action is the clipped noise (TD3)
    or zero (DDPG), everything after it can be restated"""
    flat = dict(P, actor_target=dict(P["actor_target"], w2=np.zeros((128, 4), f32), b2=np.zeros(4, f32)))
    return dict(flat, q2_target=P["q1_target"]) if trainer == "td3" else flat


def _target_q32(trainer, P, rows, z, hp):
    if trainer == "td3":
        e = f32(hp["target_policy_noise"]) * z
        cl = f32(hp["target_noise_clip"])
        ap = np.clip(np.clip(e, -cl, cl), -1.0, 1.0).astype(f32)
        return tgt._net32(P["q1_target"], np.concatenate([rows[3], ap], 1))
    W = P["critic_target"]
    x1 = np.clip(rows[3], -f32(hp["obs_clip"]), f32(hp["obs_clip"])).astype(f32)
    h0 = _relu32(_layer32(W["w0"], W["b0"], x1))
    h1 = _relu32(_layer32(W["w1"], W["b1"], np.concatenate([h0, np.zeros((x1.shape[0], 4), f32)], 1)))     # the action last, and zero
    return _layer32(W["w2"], W["b2"], h1)[:, 0]


@pytest.mark.parametrize("trainer", ["ddpg", "td3"])
@pytest.mark.parametrize("count", [17, 1])
def test_y_mean_is_the_headers_formula_at_every_gamma(torch, trainer, count):
    """gamma 0.5 and 1 (and the default 0.99): y_mean bit for bit from the float32 restatement, on target critics of O(1) values;
    gamma 0: the float32 ascending sum of rew over float32(rows).  The four differ"""
    F = hc.fixture(trainer, "shifted")
    flat = dict(F, P=_flat_targets(trainer, F["P"]))
    idx, z = F["idx"][:, :count], (F["z"][:, :count] if trainer == "td3" else None)
    rows = tuple(a[idx[0]] for a in F["rp"])
    at = 4 if trainer == "td3" else 3
    seen = []
    for gam in (0.0, 0.5, 0.99, 1.0):
        hp = dict(hc.DEFAULTS[trainer], gamma=gam)
        kw = dict(idx=idx, noise=z) if trainer == "td3" else dict(idx=idx)
        got = run(torch, trainer, flat, hp, **kw)["stats"][0, at]
        want = _mean32(_y32(rows, _target_q32(trainer, flat["P"], rows, None if z is None else z[0], hp), gam))
        assert same_bits(got, want), (trainer, count, gam, got, want)
        if gam == 0.0:
            assert same_bits(got, _mean32(rows[2])), (trainer, count, "gamma 0: y_mean is the mean of rew")
        seen.append(got)
    assert count == 1 or len({float(v) for v in seen}) == 4, (trainer, seen)


@pytest.mark.parametrize("trainer", ["ddpg", "td3"])
def test_gamma_zero_is_every_row_terminal(torch, trainer):
    """y = fma(0, m, rew) = rew for a finite target value: every tensor (the targets included: the same Polyak step), the
    statistics and the gradients bit for bit those of the run with done = 1 on every row"""
    F = hc.fixture(trainer, "shifted")
    a = run(torch, trainer, F, dict(hc.DEFAULTS[trainer], gamma=0.0))
    term = F["rp"][:4] + (np.ones_like(F["rp"][4]),)
    b = run(torch, trainer, F, hc.DEFAULTS[trainer], rp=term)
    mod = {"ddpg": tgd, "td3": tgt}[trainer]
    assert same_bits(a["stats"], b["stats"]) and mod.state_bits_equal(a["raw"], b["raw"]), (trainer, a["stats"], b["stats"])
    assert all(same_bits(a["grads"][k], b["grads"][k]) for k in a["grads"]), trainer
    live = run(torch, trainer, F, hc.DEFAULTS[trainer])
    assert not same_bits(a["stats"], live["stats"]) and not mod.state_bits_equal(a["raw"], live["raw"])
    assert (F["rp"][4][F["idx"][0]] < 1.0).any()


# ---------------------------------------------------------------------------------------------------- TD3's smoothing and delay
def test_td3_smoothing_at_other_ratios(torch):
    F, D = hc.fixture("td3", "shifted"), hc.DEFAULTS["td3"]
    same = lambda a, b: (tgt.state_bits_equal(a["raw"], b["raw"]) and same_bits(a["stats"], b["stats"])       # noqa: E731
                         and all(same_bits(a["grads"][k], b["grads"][k]) for k in a["grads"]))
    base = run(torch, "td3", F, D)
    # a clip of 0 leaves no noise: sigma = 0
    a, b = run(torch, "td3", F, dict(D, target_noise_clip=0.0)), run(torch, "td3", F, dict(D, target_policy_noise=0.0))
    assert same(a, b) and not same_bits(a["stats"], base["stats"])
    # sigma 4, clip 0.5: clipped rows act as rows fed the clipped values, sign(z) 0.125; 4 * 0.125 is 0.5 itself
    hp = dict(D, target_policy_noise=4.0)
    lim = f32(hp["target_noise_clip"] / hp["target_policy_noise"])
    assert f32(4.0) * f32(0.125) == f32(0.5) and lim == f32(0.125)
    z = F["z"]
    print("hyper td3 noise-4-clip-0.5: %d of %d normals beyond 0.125" % (int((np.abs(z) > lim).sum()), z.size))
    assert (np.abs(z) > lim).sum() > z.size // 2
    c, d = run(torch, "td3", F, hp), run(torch, "td3", F, hp, noise=hc.clipped_noise(z, 4.0, 0.5))
    assert same(c, d) and not same_bits(c["stats"], base["stats"])
    assert not same_bits(c["stats"], run(torch, "td3", F, dict(hp, target_noise_clip=float("inf")))["stats"])


def test_td3_policy_delay_at_its_maximum(torch):
    from quadsim_amd import QuadsimError, td3
    F, P = hc.fixture("td3"), hc.fixture("td3")["P"]
    delay = hc.TD3_DELAY_EDGE
    hp = dict(hc.DEFAULTS["td3"], policy_delay=delay)
    assert td3.TD3_MAX_DELAY == delay
    for t0, steps in ((delay, 1), (delay - 1, 0)):
        assert td3.actor_steps(t0, 1, delay) == int(td.schedule(t0, 1, delay).sum()) == steps
        assert td3.check_td3_args(td.N_ROWS, 1, hc.BATCH, policy_delay=delay, t0=t0, actor_t0=1)[7] == delay
    # u = 65536: an actor step
    out = run(torch, "td3", F, hp, t0=delay, actor_t0=1)
    check_step("td3", F, hp, out, "td3 policy_delay 65536 at t0 65536", t0=delay, actor_t0=1)
    assert out["stats"][0, 5] != 0.0 and all(np.isfinite(out["grads"]["actor/" + k]).all() for k in td.KEYS)
    assert all(not same_bits(out["raw"]["w"][n][k], P[n][k]) for n in td.NETS for k in td.KEYS)
    # u = 65535: none.  The actor, its moments and the three targets keep their bits, actor_loss is +0.0
    out = run(torch, "td3", F, hp, t0=delay - 1, actor_t0=1)["raw"]
    for n in ("actor", "actor_target", "q1_target", "q2_target"):
        assert all(same_bits(out["w"][n][k], P[n][k]) for k in td.KEYS), n
    assert all(same_bits(out["m"]["actor"][k], F["M"]["actor"][k]) and same_bits(out["v"]["actor"][k], F["V"]["actor"][k]) for k in td.KEYS)
    assert all(np.isnan(out["grads"]["actor"][k]).all() for k in td.KEYS)
    assert out["stats"][0, 5] == 0.0 and not np.signbit(out["stats"][0, 5]) and np.isfinite(out["stats"]).all()
    assert all(not same_bits(out["w"][n][k], P[n][k]) for n in ("q1", "q2") for k in td.KEYS)
    # the critics' half is that of the reference's critic-only step
    stats, G, _, Es, E = td.step64(P, hc.rows_of(F), F["z"][0], actor=False, with_bound=True)
    assert np.all(np.abs(out["stats"][0].astype(np.float64) - stats)[:5] <= Es[:5])
    assert all(np.all(np.abs(out["grads"][n][k].astype(np.float64) - G[n][k]) <= E[n][k]) for n in ("q1", "q2") for k in td.KEYS)
    # 65537 is refused before anything is launched
    with pytest.raises(ValueError, match="policy_delay"):
        td3.check_td3_args(td.N_ROWS, 1, hc.BATCH, policy_delay=delay + 1)
    with pytest.raises(QuadsimError, match="policy_delay"):
        run(torch, "td3", F, dict(hp, policy_delay=delay + 1), t0=0, actor_t0=0)


# ---------------------------------------------------------------------------------------------------- PPO2's norm clip
@pytest.mark.parametrize("layout", hc.PPO2_LAYOUTS)
def test_ppo2_without_a_norm_clip(torch, layout):
    """max_grad_norm -1, 0 and 1e6 (the norm is far below it: the scale is exactly 1): the same bits in every tensor and
    statistic; the run itself is held to the reference by test_case_within_the_references_bounds"""
    F = hc.fixture("ppo2", layout)
    runs = [run(torch, "ppo2", F, dict(hc.DEFAULTS["ppo2"], max_grad_norm=v)) for v in (-1.0, 0.0, 1.0e6)]
    norm = float(runs[0]["stats"][0, 5])
    assert 0.0 < norm < 1.0e6 and pr.clip_scale64(runs[0]["grads"], 1.0e6)[0] == 1.0 and pr.clip_scale64(runs[0]["grads"], 0.0)[0] == 1.0
    for o in runs[1:]:
        assert tgp.state_bits_equal(runs[0]["raw"], o["raw"]) and same_bits(runs[0]["stats"], o["stats"]), layout
        assert all(same_bits(runs[0]["grads"][k], o["grads"][k]) for k in o["grads"]), layout
    clipped = run(torch, "ppo2", F, hc.DEFAULTS["ppo2"])
    assert not tgp.state_bits_equal(runs[0]["raw"], clipped["raw"]) and same_bits(runs[0]["stats"], clipped["stats"])


# ---------------------------------------------------------------------------------------------------- GAIL's entropy coefficient
@pytest.mark.parametrize("hidden", gr.HIDDENS)
@pytest.mark.parametrize("cid", ["entcoeff-0", "entcoeff-0.1"])
def test_gail_entcoeff_at_every_width(torch, hidden, cid):
    """(entcoeff 0 lies within a bound of the default 1e-3 in every gradient: it is held to run within the bounds, and its bits to
    differ from the default's; 0.1 is told apart by the gradient of w1: tests/test_hyper_cases_cpu.py)"""
    row = row_of("gail", cid)
    F, hp = hc.fixture("gail", str(hidden)), hc.hyper_of("gail", row)
    out = run(torch, "gail", F, hp)
    check_step("gail", F, hp, out, "gail hidden %d %s" % (hidden, cid))
    assert not same_bits(out["grads"]["w2"], run(torch, "gail", F, hc.DEFAULTS["gail"])["grads"]["w2"])


# ---------------------------------------------------------------------------------------------------- TRPO's solver settings
@pytest.mark.parametrize("row", hc.TRPO_STEP_CASES, ids=[r["id"] for r in hc.TRPO_STEP_CASES])
def test_trpo_solver_settings(torch, row):
    """max_kl, cg_damping, cg_iters and backtracks away from their defaults, 17 rows in 2 slices: the solver replayed bit for bit
    from the device's own products at the setting (tests/test_gpu_trpo.py's _check_solver: lm = sqrt(shs / max_kl), the damping in
    every product's reference, the iterations run), every evaluated candidate within ls_eval64's bounds, the accepted one the first
    that float64 accepts at the setting's max_kl wherever float64 decides by more than the bounds, theta that candidate's bits"""
    W, data = hc.trpo_step_fixture()
    hp = dict(row["hyper"])
    full = dict(hc.TRPO_STEP_DEFAULT, **hp)
    out = tgr.policy_step(torch, W, data, hp, hc.TRPO_STEP_SLICES)
    _, iters = tgr._check_solver(W, data, hp, out)
    st, T = out["stats"], out["trace"]
    assert 1 <= iters <= full["cg_iters"] and np.isfinite(st).all(), (row["id"], st)
    # why the solver stopped: every iteration asked for has run, or the residual fell below residual_tol at the last one and at none before
    tol = 1e-10
    assert iters == full["cg_iters"] or T["cg"][iters - 1, 2] < tol, (row["id"], iters, T["cg"][:iters, 2])
    assert (T["cg"][:iters - 1, 2] >= tol).all(), (row["id"], "the solver went on below residual_tol", T["cg"][:iters, 2])
    assert row["id"] != "cg-iters-1" or iters == 1
    accepted = int(st[8])
    assert -1 <= accepted < full["backtracks"]
    evaluated = accepted + 1 if accepted >= 0 else full["backtracks"]
    G = tr.grad64(W, data, full["entcoeff"], with_bound=True)
    th0 = tr.flatten(W, f32)
    for k in range(evaluated):
        surr, kl, E_s, E_k = tr.ls_eval64(W, tr.candidate32(th0, T["fullstep"], k), data, full["entcoeff"], with_bound=True)
        tgr.within(T["ls"][k, 0], surr, E_s, "hyper trpo %s surr_%d" % (row["id"], k))
        tgr.within(T["ls"][k, 1], kl, E_k, "hyper trpo %s kl_%d" % (row["id"], k))
        if abs(kl - 1.5 * full["max_kl"]) > E_k and abs(surr - G["surr_before"]) > E_s + G["E_surr"]:
            ok = kl <= 1.5 * full["max_kl"] and surr - G["surr_before"] >= 0.0
            assert ok == (k == accepted), (row["id"], "the float64 decision at the device's candidate %d" % k, surr, kl)
    assert np.isnan(T["ls"][evaluated:]).all()
    new = tr.flatten(out["W"], f32)
    assert same_bits(new, tr.candidate32(th0, T["fullstep"], accepted) if accepted >= 0 else th0), row["id"]
    tgr.untouched(out, W, tr.VALUE_KEYS, row["id"])
    print("hyper trpo %s: cg iterations %d, accepted %d, shs %.6g, lm %.6g" % (row["id"], iters, accepted, st[5], st[6]))
