"""TRPO on the device: the natural-gradient policy step and the value fit of Stable-Baselines 2's ``TRPO``, which its ``GAIL``
subclasses and ``run_docking_gail.py`` of the reference therefore trains with.

``trpo_policy_step`` is one call of ``qst_policy_step`` of libquadsim_trpo.so (include/quadsim_trpo.h has the numerical contract):
the gradient of the surrogate over all rows, ``cg_iters + 1`` Fisher-vector products on every ``fvp_stride``-th row inside a
conjugate-gradient solve whose scalars live on the device, and a backtracking line search on the surrogate and the mean KL, all
enqueued on torch's current stream without a host round trip.  ``trpo_vf_fit`` is one launch of ``qst_vf_fit``: the Adam steps of
the value tower on mean((v - R)^2) over a schedule drawn on the host (``vf_schedule``, SB2's ``iterbatches``).
``torch_trpo_policy_step`` and ``torch_trpo_vf_fit`` are the same updates on torch autograd (double backprop of the mean KL, the
same CG and line search): the comparison paths.  ``TRPO(...).learn(...)`` is SB2's loop over the existing ``Runner``; with
``expert_data`` it is SB2's GAIL loop over ``GailRunner``, ``Discriminator.fit`` and ``discriminator_schedule``.

Not here: the shared-trunk layout (its shared layers would belong to both optimisers; it is refused), the fork's tanh-squashed
policies, a multi-GPU all-reduce, SB2's per-step merge of the discriminator's observation statistics, and ``np.allclose(g, 0)``:
the update is skipped where the gradient is exactly zero.
"""
import ctypes as C
import functools
import math
import time

import numpy as np

from . import _lib
from .ppo2 import SLOT_KEYS, SLOT_SHAPES, _after_update, explained_variance

TRPO_PARAMS, TRPO_STATS, TRPO_CHUNK, TRPO_AUTO_SLICES, TRPO_MAX_SLICES = 18696, 10, 16, 128, 1024
TRPO_MAX_CG_ITERS, TRPO_MAX_BACKTRACKS, TRPO_MAX_BATCH, TRPO_MAX_STEPS = 64, 32, 256, 4096
TRPO_BETA1, TRPO_BETA2, TRPO_EPS = 0.9, 0.999, 1.0e-8        # MpiAdam's defaults
TRPO_RESIDUAL_TOL = 1.0e-10                                 # SB2's cg(residual_tol=1e-10)
STAT_NAMES = ("surr_before", "surr_after", "kl_after", "entropy", "grad_norm", "shs", "lm", "expected_improve", "accepted", "cg_iters_run")
POLICY_SLOTS, VALUE_SLOTS = (0, 1, 2, 3, 4, 5, 12), (6, 7, 8, 9, 10, 11)
POLICY_KEYS, VALUE_KEYS = tuple(SLOT_KEYS[i] for i in POLICY_SLOTS), tuple(SLOT_KEYS[i] for i in VALUE_SLOTS)

# libquadsim_trpo.so is the entry "trpo" of _lib.SIDE: its path, signatures, loader, status check and call helper are _lib's
QstNet, QstBatch, QstHyper, QstTrace, TRPO_EXPORTS = _lib.QstNet, _lib.QstBatch, _lib.QstHyper, _lib.QstTrace, _lib.SIDE["trpo"]["exports"]
load_trpo, check_trpo = functools.partial(_lib.side_load, "trpo"), functools.partial(_lib.side_check, "trpo")


def auto_slices(n):
    """qst_auto_slices: min(chunks of 16 rows, 128).  UNTUNED"""
    n = int(n)
    return 0 if n < 1 else min(-(-n // TRPO_CHUNK), TRPO_AUTO_SLICES)


def check_trpo_args(n, slices=0, max_kl=0.01, cg_iters=10, cg_damping=1.0e-2, entcoeff=0.0, backtracks=10, fvp_stride=5,
                    residual_tol=TRPO_RESIDUAL_TOL):
    """-> (n, slices, {the hyper-parameters}); ValueError for what qst_policy_step would refuse, before anything touches the
    library or the GPU"""
    n, slices, cg_iters, backtracks, fvp_stride = int(n), int(slices), int(cg_iters), int(backtracks), int(fvp_stride)
    if not 1 <= n < 1 << 31:
        raise ValueError("n must be in [1, 2^31), got %d" % n)
    if not 0 <= slices <= TRPO_MAX_SLICES:
        raise ValueError("slices must be in [0, %d], got %d" % (TRPO_MAX_SLICES, slices))
    if not 1 <= cg_iters <= TRPO_MAX_CG_ITERS:
        raise ValueError("cg_iters must be in [1, %d], got %d" % (TRPO_MAX_CG_ITERS, cg_iters))
    if not 1 <= backtracks <= TRPO_MAX_BACKTRACKS:
        raise ValueError("backtracks must be in [1, %d], got %d" % (TRPO_MAX_BACKTRACKS, backtracks))
    if fvp_stride < 1:
        raise ValueError("fvp_stride must be >= 1, got %d" % fvp_stride)
    hp = dict(max_kl=float(max_kl), cg_damping=float(cg_damping), entcoeff=float(entcoeff), residual_tol=float(residual_tol))
    for name, val in hp.items():
        if not math.isfinite(val):
            raise ValueError("%s must be finite, got %r" % (name, val))
    if hp["max_kl"] <= 0.0:
        raise ValueError("max_kl must be > 0, got %r" % (max_kl,))
    for name in ("cg_damping", "residual_tol"):
        if hp[name] < 0.0:
            raise ValueError("%s must be >= 0, got %r" % (name, hp[name]))
    hp.update(cg_iters=cg_iters, backtracks=backtracks, fvp_stride=fvp_stride)
    return n, slices, hp


def check_vf_args(n, steps, batch, lr=3.0e-4, beta1=TRPO_BETA1, beta2=TRPO_BETA2, eps=TRPO_EPS, t0=0):
    """-> (n, steps, batch, lr, beta1, beta2, eps, t0); ValueError for what qst_vf_fit would refuse"""
    n, steps, batch, t0 = int(n), int(steps), int(batch), int(t0)
    if not 1 <= n < 1 << 31:
        raise ValueError("n must be in [1, 2^31), got %d" % n)
    if not 1 <= batch <= TRPO_MAX_BATCH:
        raise ValueError("batch must be in [1, %d], got %d" % (TRPO_MAX_BATCH, batch))
    if not 1 <= steps <= TRPO_MAX_STEPS:
        raise ValueError("steps must be in [1, %d], got %d" % (TRPO_MAX_STEPS, steps))
    lr, beta1, beta2, eps = _lib.check_adam_args(lr, beta1, beta2, eps, t0, steps, "steps")
    return n, steps, batch, lr, beta1, beta2, eps, t0


def vf_schedule(n, batch, vf_iters, generator, device="cpu"):
    """-> indices [vf_iters * (n // batch), batch] int32 on `device`: SB2's iterbatches(batch_size=batch, shuffle=True,
    include_final_partial_batch=False), `vf_iters` times: every pass a fresh permutation of 0 .. n-1 from `generator` (a CPU
    torch.Generator) cut into consecutive full batches, the rest dropped.  ValueError for n < batch (no step at all).  The schedule
    of a + b passes is the schedules of a and of b passes drawn one after another."""
    import torch
    n, batch, vf_iters = int(n), int(batch), int(vf_iters)
    if batch < 1 or vf_iters < 1:
        raise ValueError("batch and vf_iters must be >= 1")
    if n < batch:
        raise ValueError("the roll-out's %d rows do not fill one value batch of %d" % (n, batch))
    if n >= 1 << 31:
        raise ValueError("n must be below 2^31, got %d" % n)
    per = n // batch
    idx = torch.stack([torch.randperm(n, generator=generator)[:per * batch].to(torch.int32) for _ in range(vf_iters)])
    return idx.view(vf_iters * per, batch).to(device)


# ---------------------------------------------------------------------------------------------------- the policy's side
def policy_tensors(policy):
    """the thirteen slots of QstNet over a towers ActorCriticPolicy, checked; ValueError for a squashed policy or the shared layout"""
    import torch
    if getattr(policy, "squash", False):
        raise ValueError("TRPO does not cover the tanh-squashed policies of the fork (squash=True)")
    if not bool(getattr(policy, "towers", False)):
        raise ValueError("TRPO does not cover the shared-trunk layout: its shared layers would belong to the policy step and to the value "
                         "fit; use a towers policy (net_arch=[dict(pi=[128, 128], vf=[128, 128])])")
    ws = []
    for k, shape in zip(SLOT_KEYS, SLOT_SHAPES):
        w = getattr(policy, k, None)
        if not (isinstance(w, torch.Tensor) and w.dtype == torch.float32 and tuple(w.shape) == shape and w.is_contiguous()):
            raise TypeError("trpo: the policy's %s must be a contiguous float32 tensor of shape %s" % (k, shape))
        ws.append(w)
    if any(w.device != ws[0].device for w in ws):
        raise TypeError("trpo: the policy's tensors must be on one device")
    return ws


def reset_trpo_optimizer(policy):
    """forget the value fit's Adam moments and step count and the policy step's workspace"""
    policy._trpo_m = policy._trpo_v = policy._trpo_ws = None
    policy._trpo_steps = 0


def _state(policy, ws):
    import torch
    if getattr(policy, "_trpo_m", None) is None:
        policy._trpo_m = [torch.zeros_like(ws[i]) if i in VALUE_SLOTS else None for i in range(13)]
        policy._trpo_v = [torch.zeros_like(ws[i]) if i in VALUE_SLOTS else None for i in range(13)]
        policy._trpo_steps, policy._trpo_ws = 0, getattr(policy, "_trpo_ws", None)
    return policy._trpo_m, policy._trpo_v


def rollout_tensors(rollout):
    """(obs, actions, returns, values) of what Runner.run() returns (its 9-tuple) or of a dict with those keys"""
    if isinstance(rollout, dict):
        return tuple(rollout[k] for k in ("obs", "actions", "returns", "values"))
    obs, returns, _masks, actions, values = rollout[:5]
    return obs, actions, returns, values


def _check_rollout(dev, obs, actions, returns, values):
    _lib.check_tensor("obs", obs, "float32", ("n", 12), dev)
    n = int(obs.shape[0])
    _lib.check_tensor("actions", actions, "float32", (n, 4), dev)
    for name, t in (("returns", returns), ("values", values)):
        _lib.check_tensor(name, t, "float32", (n,), dev)
    return n


def _need_device(dev, what, other):
    if dev.type != "cuda":
        raise _lib.QuadsimError("%s needs the policy on a HIP device, it is on %s; %s is the host path" % (what, dev, other))


def new_trace(device, cg_iters, backtracks, fill=float("nan")):
    """the six outputs of QstTrace as a dict of device tensors filled with `fill` (rows of iterations that do not run stay so)"""
    import torch
    f = dict(device=device, dtype=torch.float32)
    return {"fvp_in": torch.full((cg_iters + 1, TRPO_PARAMS), fill, **f), "fvp_out": torch.full((cg_iters + 1, TRPO_PARAMS), fill, **f),
            "cg": torch.full((cg_iters, 4), fill, device=device, dtype=torch.float64), "x": torch.full((TRPO_PARAMS,), fill, **f),
            "fullstep": torch.full((TRPO_PARAMS,), fill, **f), "ls": torch.full((backtracks, 2), fill, **f)}


def trpo_policy_step(policy, rollout, *, max_kl=0.01, cg_iters=10, cg_damping=1.0e-2, entcoeff=0.0, backtracks=10, fvp_stride=5,
                     residual_tol=TRPO_RESIDUAL_TOL, slices="auto", return_grad=False, trace=None):
    """ONE TRPO policy update of `policy` (a towers ActorCriticPolicy on a HIP device) over all rows of `rollout` (what Runner.run()
    returns) in one qst_policy_step call, on torch's current stream.  `trace`: True for a fresh new_trace, or a dict of its six
    tensors.  The workspace is kept on the policy.  Afterwards every cached device image of the weights is dropped and
    policy.logstd_host is refreshed (one device -> host copy of 16 bytes, which waits for the update).
    -> {"stats": [10] device tensor (STAT_NAMES), "grad": the gradient [P] on request, "trace": the trace}."""
    ws = policy_tensors(policy)
    dev = ws[0].device
    _need_device(dev, "trpo_policy_step", "torch_trpo_policy_step")
    data = rollout_tensors(rollout)
    n = _check_rollout(dev, *data)
    n, nslices, hp = check_trpo_args(n, 0 if slices == "auto" else slices, max_kl, cg_iters, cg_damping, entcoeff, backtracks, fvp_stride,
                                     residual_tol)
    lib = load_trpo()
    need = C.c_size_t(0)
    _lib.side_call("trpo", lib, "qst_workspace_bytes", n, nslices, C.byref(need))
    if getattr(policy, "_trpo_ws", None) is None or policy._trpo_ws.numel() < need.value:
        policy._trpo_ws = _lib.new_tensor(dev, (need.value,), "uint8")
    stats = _lib.new_tensor(dev, (TRPO_STATS,), "float32")
    grad = _lib.new_tensor(dev, (TRPO_PARAMS,), "float32") if return_grad else None
    if trace is True:
        trace = new_trace(dev, hp["cg_iters"], hp["backtracks"])
    tr = None
    if trace is not None:
        _lib.check_tensor("trace fvp_in", trace["fvp_in"], "float32", (hp["cg_iters"] + 1, TRPO_PARAMS), dev)
        _lib.check_tensor("trace fvp_out", trace["fvp_out"], "float32", (hp["cg_iters"] + 1, TRPO_PARAMS), dev)
        _lib.check_tensor("trace cg", trace["cg"], "float64", (hp["cg_iters"], 4), dev)
        _lib.check_tensor("trace x", trace["x"], "float32", (TRPO_PARAMS,), dev)
        _lib.check_tensor("trace fullstep", trace["fullstep"], "float32", (TRPO_PARAMS,), dev)
        _lib.check_tensor("trace ls", trace["ls"], "float32", (hp["backtracks"], 2), dev)
        tr = QstTrace(C.sizeof(QstTrace), 0, *(_lib.as_arg(trace[k]) for k in ("fvp_in", "fvp_out", "cg", "x", "fullstep", "ls")))
    null = [None] * 13
    net = QstNet(C.sizeof(QstNet), 1, _lib.pointers(ws), _lib.pointers(null), _lib.pointers(null))
    bat = QstBatch(C.sizeof(QstBatch), 0, n, *map(_lib.as_arg, data))
    hyp = QstHyper(C.sizeof(QstHyper), hp["cg_iters"], hp["backtracks"], hp["fvp_stride"], hp["max_kl"], hp["cg_damping"], hp["entcoeff"],
                   hp["residual_tol"])
    _lib.side_call("trpo", lib, "qst_policy_step", C.byref(net), C.byref(bat), nslices, C.byref(hyp), policy._trpo_ws,
                   int(policy._trpo_ws.numel()), stats, grad, None if tr is None else C.byref(tr), device=dev)
    _after_update(policy)
    return {"stats": stats, "grad": grad, "trace": trace}


def trpo_vf_fit(policy, rollout, indices, *, vf_stepsize=3.0e-4, beta1=TRPO_BETA1, beta2=TRPO_BETA2, eps=TRPO_EPS, check_indices=True,
                return_grads=False):
    """indices.shape[0] Adam steps of the value tower on mean((v - returns)^2) in ONE launch of qst_vf_fit (several beyond 4096
    steps).  indices [steps, batch]: a DEVICE int32 tensor (vf_schedule).  Adam's moments and the step count are kept on the policy,
    separate from PPO2's and behaviour cloning's; reset_trpo_optimizer forgets them.
    -> {"stats": [steps] device tensor (the loss before each step), "grads": the six gradients of the last step on request}."""
    import torch
    ws = policy_tensors(policy)
    dev = ws[0].device
    _need_device(dev, "trpo_vf_fit", "torch_trpo_vf_fit")
    obs, _, returns, _ = rollout_tensors(rollout)
    _lib.check_tensor("obs", obs, "float32", ("n", 12), dev)
    n = int(obs.shape[0])
    _lib.check_tensor("returns", returns, "float32", (n,), dev)
    _check_indices(indices, dev, n, check_indices)
    steps, batch = int(indices.shape[0]), int(indices.shape[1])
    m, v = _state(policy, ws)
    lib = load_trpo()
    stats = _lib.new_tensor(dev, (steps,), "float32")
    grads = [torch.empty_like(ws[i]) for i in VALUE_SLOTS] if return_grads else None
    for s0 in range(0, steps, TRPO_MAX_STEPS):
        part = min(TRPO_MAX_STEPS, steps - s0)
        _, _, _, lr, b1, b2, e, t0 = check_vf_args(n, part, batch, vf_stepsize, beta1, beta2, eps, policy._trpo_steps)
        net = QstNet(C.sizeof(QstNet), 1, _lib.pointers(ws), _lib.pointers(m), _lib.pointers(v))
        last = s0 + part == steps
        _lib.side_call("trpo", lib, "qst_vf_fit", C.byref(net), obs, returns, n, indices[s0:s0 + part], part, batch, lr, b1, b2, e, t0,
                       stats[s0:s0 + part], C.byref(_lib.six(grads)) if grads is not None and last else None, device=dev)
        policy._trpo_steps += part
    _after_update(policy)
    return {"stats": stats, "grads": grads}


def _check_indices(indices, dev, n, check):
    import torch
    if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int32 and indices.dim() == 2 and indices.device == dev
            and indices.is_contiguous() and indices.numel() > 0):
        raise ValueError("indices must be a contiguous int32 tensor [steps, batch] on %s" % (dev,))
    if check:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(indices)).tolist())
        if lo < 0 or hi >= n:
            raise ValueError("indices must be in [0, n = %d), got [%d, %d]" % (n, lo, hi))


# ---------------------------------------------------------------------------------------------------- the same updates on torch
def _policy_head(torch, P, obs):
    h = torch.relu(obs @ P["w0"] + P["b0"])
    return torch.relu(h @ P["w1"] + P["b1"]) @ P["w2"] + P["b2"]


def _neglogp(torch, mean, logstd, actions):
    return 0.5 * (((actions - mean) / torch.exp(logstd)) ** 2).sum(-1) + 0.5 * math.log(2.0 * math.pi) * 4.0 + logstd.sum()


def _mean_kl(torch, mean_old, ls_old, mean, ls):
    return (ls - ls_old + (torch.exp(2.0 * ls_old) + (mean_old - mean) ** 2) / (2.0 * torch.exp(2.0 * ls)) - 0.5).sum(-1).mean()


def torch_trpo_policy_step(policy, rollout, *, max_kl=0.01, cg_iters=10, cg_damping=1.0e-2, entcoeff=0.0, backtracks=10, fvp_stride=5,
                           residual_tol=TRPO_RESIDUAL_TOL, return_grad=False, **_ignored):
    """trpo_policy_step as a torch autograd loop on whatever device the policy is on: the surrogate's gradient, the Fisher-vector
    product as double backprop of the mean KL on every fvp_stride-th row, SB2's cg and its line search, every scalar through the
    host as SB2 has it.  Same result dict (no trace); the bits differ."""
    import torch
    ws = policy_tensors(policy)
    obs, actions, returns, values = rollout_tensors(rollout)
    _, _, hp = check_trpo_args(obs.shape[0], 0, max_kl, cg_iters, cg_damping, entcoeff, backtracks, fvp_stride, residual_tol)
    live = [ws[i] for i in POLICY_SLOTS]
    sizes = [w.numel() for w in live]
    adv = returns - values
    adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)

    def unflat(vec):
        return {k: p.view(w.shape) for k, p, w in zip(POLICY_KEYS, torch.split(vec, sizes), live)}

    theta = torch.cat([w.detach().reshape(-1) for w in live])
    with torch.no_grad():
        P0 = unflat(theta)
        mean_old, ls_old = _policy_head(torch, P0, obs), P0["logstd"].clone()
        nlp_old = _neglogp(torch, mean_old, ls_old, actions)

    def losses(vec):
        P = unflat(vec)
        mean = _policy_head(torch, P, obs)
        ent = (P["logstd"] + 0.5 * math.log(2.0 * math.pi * math.e)).sum()
        surr = (adv * torch.exp(nlp_old - _neglogp(torch, mean, P["logstd"], actions))).mean() + hp["entcoeff"] * ent
        return surr, _mean_kl(torch, mean_old, ls_old, mean, P["logstd"]), ent

    def fvp(vec):
        th = theta.clone().requires_grad_(True)
        P = unflat(th)
        kl = _mean_kl(torch, mean_old[::hp["fvp_stride"]], ls_old, _policy_head(torch, P, obs[::hp["fvp_stride"]]), P["logstd"])
        (gk,) = torch.autograd.grad(kl, th, create_graph=True)
        (hv,) = torch.autograd.grad((gk * vec).sum(), th)
        return hv + hp["cg_damping"] * vec

    th = theta.clone().requires_grad_(True)
    surr_before, _, ent0 = losses(th)
    (g,) = torch.autograd.grad(surr_before, th)
    surr_before = float(surr_before)
    stats = [surr_before, surr_before, 0.0, float(ent0), float(g.double().norm()), 0.0, 0.0, 0.0, -2.0, 0.0]
    if float((g.double() ** 2).sum()) != 0.0:
        x, r, p = torch.zeros_like(g), g.clone(), g.clone()
        rdotr, iters = float(r.double().dot(r.double())), 0
        for _ in range(hp["cg_iters"]):
            z = fvp(p)
            a = rdotr / float(p.double().dot(z.double()))
            x, r = x + a * p, r - a * z
            new = float(r.double().dot(r.double()))
            p, rdotr, iters = r + (new / rdotr) * p, new, iters + 1
            if rdotr < hp["residual_tol"]:
                break
        shs = 0.5 * float(x.double().dot(fvp(x).double()))
        lm = math.sqrt(shs / hp["max_kl"]) if shs >= 0.0 else float("nan")
        fullstep = x / lm if lm != 0.0 else x * float("inf")
        stats[5:10] = [shs, lm, float(g.double().dot(fullstep.double())), -1.0, float(iters)]
        with torch.no_grad():
            for k in range(hp["backtracks"]):
                cand = theta + fullstep * 0.5 ** k
                surr, kl, ent = (float(v) for v in losses(cand))
                if math.isfinite(surr) and math.isfinite(kl) and kl <= 1.5 * hp["max_kl"] and surr - surr_before >= 0.0:
                    for w, part in zip(live, torch.split(cand, sizes)):
                        w.copy_(part.view(w.shape))
                    stats[1], stats[2], stats[3], stats[8] = surr, kl, ent, float(k)
                    break
    _after_update(policy)
    return {"stats": torch.tensor(stats, dtype=torch.float32, device=obs.device), "grad": g.detach() if return_grad else None, "trace": None}


def torch_trpo_vf_fit(policy, rollout, indices, *, vf_stepsize=3.0e-4, beta1=TRPO_BETA1, beta2=TRPO_BETA2, eps=TRPO_EPS, return_grads=False,
                      **_ignored):
    """trpo_vf_fit as a torch autograd loop: mean((v - R)^2) and tf.train.AdamOptimizer's formula, the state shared with trpo_vf_fit"""
    import torch
    ws = policy_tensors(policy)
    obs, _, returns, _ = rollout_tensors(rollout)
    m, v = _state(policy, ws)
    steps = int(indices.shape[0])
    _, _, _, lr, beta1, beta2, eps, _ = check_vf_args(obs.shape[0], min(steps, TRPO_MAX_STEPS), indices.shape[1], vf_stepsize, beta1, beta2, eps,
                                                      policy._trpo_steps)
    live, lm, lv = [ws[i] for i in VALUE_SLOTS], [m[i] for i in VALUE_SLOTS], [v[i] for i in VALUE_SLOTS]
    stats = torch.empty((steps,), dtype=torch.float32, device=obs.device)
    grads = None
    for s in range(steps):
        rows = indices[s].long()
        P = [w.detach().requires_grad_(True) for w in live]
        vp = (torch.relu(torch.relu(obs[rows] @ P[0] + P[1]) @ P[2] + P[3]) @ P[4] + P[5])[:, 0]
        loss = ((vp - returns[rows]) ** 2).mean()
        grads = torch.autograd.grad(loss, P)
        stats[s] = loss.detach()
        t = policy._trpo_steps + 1
        lr_t = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        with torch.no_grad():
            for w, g, mm, vv in zip(live, grads, lm, lv):
                mm.mul_(beta1).add_(g, alpha=1.0 - beta1)
                vv.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
                w.sub_(lr_t * mm / (vv.sqrt() + eps))
        policy._trpo_steps += 1
    _after_update(policy)
    return {"stats": stats, "grads": list(grads) if return_grads else None}


# ---------------------------------------------------------------------------------------------------- the loop
class TRPO:
    """``TRPO(policy, env, n_steps=...).learn(total_timesteps)``: SB2's TRPO loop over the package's Runner -- per update one
    roll-out of ``n_steps`` per env (SB2's timesteps_per_batch = num_envs * n_steps), one policy step, then ``vf_iters`` passes of
    value batches.  With ``expert_data`` it is SB2's GAIL loop: ``g_step`` times {a roll-out paid by the discriminator (GailRunner),
    the policy step, the value fit}, then ``d_step`` discriminator fits of ``d_batch`` rows per class on the last roll-out's rows
    against expert rows (discriminator_schedule).  SB2's GAIL uses g_step = 3, d_step = 1.  `update`: "hip" or "torch" (the
    comparison paths).  A CPU policy, the shared layout, squash=True and a roll-out smaller than one value batch raise here,
    before anything touches the GPU."""

    def __init__(self, policy, env, *, n_steps, max_kl=0.01, cg_iters=10, cg_damping=1.0e-2, entcoeff=0.0, gamma=0.99, lam=0.98,
                 vf_stepsize=3.0e-4, vf_iters=3, vf_batch=128, fvp_stride=5, update="hip", expert_data=None, discriminator=None, g_step=1,
                 d_step=1, d_batch=256, d_stepsize=3.0e-4, seed=0, backtracks=10, slices="auto", precision="f32", fused=None, runner=None):
        import torch
        if update not in ("hip", "torch"):
            raise ValueError("update must be 'hip' or 'torch', got %r" % (update,))
        ws = policy_tensors(policy)
        if update == "hip":
            _need_device(ws[0].device, "TRPO(update='hip')", "update='torch'")
        self.policy, self.env = policy, env
        self.n_steps, self.n_batch = int(n_steps), int(env.num_envs) * int(n_steps)
        _, self.slices, self.hp = check_trpo_args(self.n_batch, 0 if slices == "auto" else slices, max_kl, cg_iters, cg_damping, entcoeff,
                                                  backtracks, fvp_stride)
        self.vf_stepsize, self.vf_iters, self.vf_batch = float(vf_stepsize), int(vf_iters), int(vf_batch)
        if self.n_batch < self.vf_batch:
            raise ValueError("the roll-out's %d rows do not fill one value batch of %d" % (self.n_batch, self.vf_batch))
        check_vf_args(self.n_batch, self.vf_iters * (self.n_batch // self.vf_batch), self.vf_batch, self.vf_stepsize)
        self.update, self.g_step, self.d_step, self.d_batch, self.d_stepsize = update, int(g_step), int(d_step), int(d_batch), float(d_stepsize)
        if self.g_step < 1 or self.d_step < 0:
            raise ValueError("g_step must be >= 1 and d_step >= 0")
        self.generator = torch.Generator().manual_seed(int(seed))
        self.expert, self.discriminator, self.cursor = expert_data, discriminator, None
        if expert_data is not None:
            from .gail import Discriminator, ExpertCursor, GailRunner, check_gail_args
            check_gail_args(self.n_batch, expert_data.obs.shape[0], max(self.d_step, 1), self.d_batch, lr=self.d_stepsize)
            if self.d_batch > self.n_batch:
                raise ValueError("d_batch = %d exceeds the roll-out's %d rows" % (self.d_batch, self.n_batch))
            if self.discriminator is None:
                self.discriminator = Discriminator(device=env.device)
            rows = getattr(expert_data, "train_rows", None)
            self.cursor = ExpertCursor(rows if rows is not None else np.arange(int(expert_data.obs.shape[0])))
            if runner is None:
                runner = GailRunner(discriminator=self.discriminator, env=env, model=policy, n_steps=self.n_steps, gamma=gamma, lam=lam,
                                    collect_ep_infos=False, precision=precision, fused=fused)
        elif runner is None:
            from .runner import Runner
            runner = Runner(env=env, model=policy, n_steps=self.n_steps, gamma=gamma, lam=lam, collect_ep_infos=False, precision=precision)
        self.runner = runner
        self.num_timesteps = 0

    def _generator_step(self):
        """one roll-out, one policy step, the value fit -> (rollout, the policy step's result, the value fit's result)"""
        step = trpo_policy_step if self.update == "hip" else torch_trpo_policy_step
        fit = trpo_vf_fit if self.update == "hip" else torch_trpo_vf_fit
        rollout = self.runner.run()
        self.num_timesteps += self.n_batch
        hp = self.hp
        out = step(self.policy, rollout, max_kl=hp["max_kl"], cg_iters=hp["cg_iters"], cg_damping=hp["cg_damping"], entcoeff=hp["entcoeff"],
                   backtracks=hp["backtracks"], fvp_stride=hp["fvp_stride"], slices=self.slices or "auto")
        indices = vf_schedule(self.n_batch, self.vf_batch, self.vf_iters, self.generator, rollout[0].device)
        vf = fit(self.policy, rollout, indices, vf_stepsize=self.vf_stepsize, check_indices=False)
        return rollout, out, vf

    def learn(self, total_timesteps, callback=None, log_interval=1):
        """-> a list of one dict per logged update: the ten statistics of the (last) policy step (STAT_NAMES), `vf_loss` (the mean
        over the value fit's steps), explained_variance, the timestep counters, the episode statistics where the Runner has them
        and, with an expert, the five discriminator statistics (DISC_STAT_NAMES, the mean over the d_step fits; its entropy
        under `disc_entropy`: `entropy` is the policy's), `disc_reward_mean` and `true_ep_reward_mean`.  callback(locals_, globals_) returning False stops the loop."""
        per_update = self.n_batch * (self.g_step if self.expert is not None else 1)
        n_updates = int(total_timesteps) // per_update
        logs, t_first = [], time.time()
        for update in range(1, n_updates + 1):
            t_start = time.time()
            d_stats = None
            if self.expert is None:
                rollout, out, vf = self._generator_step()
            else:
                from .gail import DISC_STAT_NAMES, discriminator_schedule, torch_discriminator_fit
                for _ in range(self.g_step):
                    rollout, out, vf = self._generator_step()
                d_fit = self.discriminator.fit if self.update == "hip" else functools.partial(torch_discriminator_fit, self.discriminator)
                if self.d_step > 0:
                    gen_idx, exp_idx = discriminator_schedule(self.n_batch, self.cursor, self.d_batch, self.d_step, self.generator)
                    d_stats = d_fit(rollout[0], rollout[3], self.expert, gen_idx, exp_idx, lr=self.d_stepsize)["stats"]
            if log_interval and (update % log_interval == 0 or update == 1):
                vals = out["stats"].double().tolist()                      # the update is over here: the one wait of an update
                t_now = time.time()
                log = {"n_updates": update, "total_timesteps": self.num_timesteps, "fps": int(per_update / max(t_now - t_start, 1e-9)),
                       "explained_variance": float(explained_variance(rollout[4], rollout[1])), "time_elapsed": t_start - t_first,
                       "vf_loss": float(vf["stats"].double().mean())}
                log.update(zip(STAT_NAMES, vals))
                rets, lens = getattr(self.runner, "last_ep_returns", None), getattr(self.runner, "last_ep_lengths", None)
                if rets is not None and rets.numel() > 0:
                    log["ep_reward_mean"], log["ep_len_mean"] = float(rets.double().mean()), float(lens.double().mean())
                    if self.expert is not None:
                        log["true_ep_reward_mean"] = log["ep_reward_mean"]
                if d_stats is not None:
                    # (both tuples of names have an "entropy": the policy step's keeps the key, the discriminator's is disc_entropy)
                    log.update(("disc_entropy" if k in STAT_NAMES else k, v) for k, v in zip(DISC_STAT_NAMES, d_stats.double().mean(0).tolist()))
                paid = getattr(self.runner, "last_reward", None)
                if self.expert is not None and paid is not None:
                    log["disc_reward_mean"] = float(paid.double().mean())
                logs.append(log)
            if callback is not None and callback(locals(), globals()) is False:
                break
        return logs
