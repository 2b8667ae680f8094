"""The PPO2 update on the device (rl_baselines/ppo2/ppo2.py:138-207, 244-300, 321-404): what consumes ``Runner.run()``.

``ppo2_update`` runs the ``noptepochs x nminibatches`` Adam steps on the clipped-surrogate loss through ``qsp_update`` of
libquadsim_ppo.so (include/quadsim_ppo.h): per step a gradient kernel over ``slices x 2`` workgroups (the policy and the value
branch of the net, each in LDS), a float64 reduction and a clip-and-Adam kernel, all enqueued on torch's current stream.  The
minibatch schedule is drawn on the host (``minibatch_schedule``) and lives on the device.  ``PPO2(...).learn(...)`` is the
reference's loop over the existing ``Runner``.  ``torch_ppo2_update`` is the same update as a plain autograd loop: the comparison
path of examples/ppo2_train.py and tools/ppo2_update_rate.py, and what runs where there is no device.

Not here: the fork's tanh-squashed policies (``squash=True`` is refused), recurrent policies, a multi-GPU gradient all-reduce.
"""
import ctypes as C
import functools
import math
import time

import numpy as np

from . import _lib

PPO_MAX_STEPS, PPO_MAX_SLICES, PPO_AUTO_SLICES, PPO_CHUNK = 4096, 1024, 128, 16
PPO_BETA1, PPO_BETA2, PPO_EPS = 0.9, 0.999, 1.0e-5       # ppo2.py:206: tf.train.AdamOptimizer(epsilon=1e-5)
STAT_NAMES = ("policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac", "grad_norm")
# the slots of QspNet: the policy's attributes and their shapes; wv0, bv0 exist in the tower layout alone
SLOT_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2", "wv0", "bv0", "wv1", "bv1", "wv2", "bv2", "logstd")
SLOT_SHAPES = ((12, 128), (128,), (128, 128), (128,), (128, 4), (4,), (12, 128), (128,), (128, 128), (128,), (128, 1), (1,), (4,))

# libquadsim_ppo.so is the entry "ppo" of _lib.SIDE: its path, signatures, loader, status check and call helper are _lib's
QspNet, QspBatch, QspHyper, PPO_EXPORTS = _lib.QspNet, _lib.QspBatch, _lib.QspHyper, _lib.SIDE["ppo"]["exports"]
load_ppo, check_ppo = functools.partial(_lib.side_load, "ppo"), functools.partial(_lib.side_check, "ppo")


def auto_slices(batch):
    """qsp_auto_slices: min(chunks of 16 rows, 128), one workgroup per compute unit over the two branches.  UNTUNED"""
    batch = int(batch)
    return 0 if batch < 1 else min(-(-batch // PPO_CHUNK), PPO_AUTO_SLICES)


def check_ppo2_args(n, steps, batch, slices=0, learning_rate=3.0e-4, cliprange=0.2, cliprange_vf=-1.0, ent_coef=0.0, vf_coef=0.5,
                    max_grad_norm=0.5, beta1=PPO_BETA1, beta2=PPO_BETA2, eps=PPO_EPS, t0=0):
    """-> (n, steps, batch, slices, {the hyper-parameters as floats}, t0); ValueError for what qsp_update would refuse, before
    anything touches the library or the GPU"""
    n, steps, batch, slices, t0 = int(n), int(steps), int(batch), int(slices), int(t0)
    if not 1 <= steps <= PPO_MAX_STEPS:
        raise ValueError("steps must be in [1, %d], got %d" % (PPO_MAX_STEPS, steps))
    if not 1 <= batch < 1 << 31:
        raise ValueError("batch must be in [1, 2^31), got %d" % batch)
    if not 0 <= slices <= PPO_MAX_SLICES:
        raise ValueError("slices must be in [0, %d], got %d" % (PPO_MAX_SLICES, slices))
    if not 1 <= n < 1 << 31:
        raise ValueError("n must be in [1, 2^31), got %d" % n)
    lr, beta1, beta2, eps = _lib.check_adam_args(learning_rate, beta1, beta2, eps, t0, steps, "steps")
    hp = dict(lr=lr, cliprange=float(cliprange), cliprange_vf=float(cliprange_vf), ent_coef=float(ent_coef), vf_coef=float(vf_coef),
              max_grad_norm=float(max_grad_norm), beta1=beta1, beta2=beta2, eps=eps)
    for name, val in hp.items():
        if not math.isfinite(val):
            raise ValueError("%s must be finite, got %r" % (name, val))
    if hp["cliprange"] < 0.0:
        raise ValueError("cliprange must be >= 0, got %r" % (cliprange,))
    return n, steps, batch, slices, hp, t0


def minibatch_schedule(n_batch, nminibatches, noptepochs, generator, device="cpu"):
    """-> indices [noptepochs * nminibatches, n_batch // nminibatches] int32 on `device`: every epoch a fresh permutation of
    0 .. n_batch-1 from `generator` (a CPU torch.Generator), cut into consecutive minibatches (ppo2.py:350-357).  ValueError
    unless nminibatches divides n_batch, which the reference asserts.  The schedule of E epochs is E one-epoch schedules drawn one
    after another from the same generator."""
    import torch
    n_batch, nminibatches, noptepochs = int(n_batch), int(nminibatches), int(noptepochs)
    if n_batch < 1 or nminibatches < 1 or noptepochs < 1:
        raise ValueError("n_batch, nminibatches and noptepochs must be >= 1")
    if n_batch % nminibatches != 0:
        raise ValueError("nminibatches = %d is not a factor of n_batch = %d: some samples would not be used" % (nminibatches, n_batch))
    if n_batch >= 1 << 31:
        raise ValueError("n_batch must be below 2^31, got %d" % n_batch)
    idx = torch.stack([torch.randperm(n_batch, generator=generator).to(torch.int32) for _ in range(noptepochs)])
    return idx.view(noptepochs * nminibatches, n_batch // nminibatches).to(device)


# ---------------------------------------------------------------------------------------------------- the policy's side
def policy_tensors(policy):
    """the thirteen slots of QspNet over an ActorCriticPolicy of either layout (None where the layout has no tensor), checked"""
    import torch
    if getattr(policy, "squash", False):
        raise ValueError("the PPO2 update does not cover the tanh-squashed policies of the fork (squash=True)")
    towers = bool(getattr(policy, "towers", False))
    ws = []
    for k, shape in zip(SLOT_KEYS, SLOT_SHAPES):
        if k in ("wv0", "bv0") and not towers:
            ws.append(None)
            continue
        w = getattr(policy, k, None)
        if not (isinstance(w, torch.Tensor) and w.dtype == torch.float32 and tuple(w.shape) == shape and w.is_contiguous()):
            raise TypeError("ppo2_update: the policy's %s must be a contiguous float32 tensor of shape %s" % (k, shape))
        ws.append(w)
    if any(w is not None and w.device != ws[0].device for w in ws):
        raise TypeError("ppo2_update: the policy's tensors must be on one device")
    return ws


def reset_ppo2_optimizer(policy):
    """forget Adam's moments, the step count and the workspace (the next update creates them again, zeros)"""
    policy._ppo_m = policy._ppo_v = policy._ppo_ws = None
    policy._ppo_steps = 0


def _state(policy, ws):
    import torch
    if getattr(policy, "_ppo_m", None) is None:
        policy._ppo_m = [None if w is None else torch.zeros_like(w) for w in ws]
        policy._ppo_v = [None if w is None else torch.zeros_like(w) for w in ws]
        policy._ppo_steps, policy._ppo_ws = 0, None
    return policy._ppo_m, policy._ppo_v


def rollout_tensors(rollout):
    """(obs, actions, returns, values, neglogp) of what Runner.run() returns (its 9-tuple) or of a dict with those keys"""
    if isinstance(rollout, dict):
        return tuple(rollout[k] for k in ("obs", "actions", "returns", "values", "neglogp"))
    obs, returns, _masks, actions, values, neglogp = rollout[:6]
    return obs, actions, returns, values, neglogp


def _check_rollout(dev, obs, actions, returns, values, neglogp):
    _lib.check_tensor("obs", obs, "float32", ("n", 12), dev)
    n = int(obs.shape[0])
    _lib.check_tensor("actions", actions, "float32", (n, 4), dev)
    for name, t in (("returns", returns), ("values", values), ("neglogp", neglogp)):
        _lib.check_tensor(name, t, "float32", (n,), dev)
    return n


def _check_indices(indices, dev, n, check):
    import torch
    if not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int32 and indices.dim() == 2 and indices.device == dev
            and indices.is_contiguous() and indices.numel() > 0):
        raise ValueError("indices must be a contiguous int32 tensor [steps, batch] on %s" % (dev,))
    if check:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(indices)).tolist())
        if lo < 0 or hi >= n:
            raise ValueError("indices must be in [0, n = %d), got [%d, %d]" % (n, lo, hi))


def _after_update(policy):
    """the weights changed behind the policy's back: forget every device image built from them, and refresh the host copy of
    logstd that the Runner passes by value (ONE device -> host copy of 16 bytes per update; it waits for the update)"""
    from .bc import drop_cached_images
    drop_cached_images(policy)
    policy.logstd_host = policy.logstd.detach().cpu().numpy().astype(np.float32).reshape(4).copy()


def ppo2_update(policy, rollout, indices, *, learning_rate, cliprange, cliprange_vf=None, ent_coef, vf_coef, max_grad_norm,
                slices="auto", check_indices=True, return_grads=False):
    """indices.shape[0] Adam steps of PPO2 on `policy` (an ActorCriticPolicy of either layout, on a HIP device) over `rollout`
    (what Runner.run() returns) in ONE qsp_update call (several beyond 4096 steps).  indices [steps, batch]: a DEVICE int32 tensor
    (minibatch_schedule); with `check_indices` one device-side min / max holds them inside the roll-out.  cliprange_vf None: the
    policy's cliprange (SB2's default), < 0: no value clipping.  max_grad_norm None or <= 0: no clipping.
    Adam's moments, the step count and the workspace are kept on the policy (separate from behaviour cloning's): a second call
    continues from them, reset_ppo2_optimizer forgets them.  Afterwards every cached device image of the weights is dropped and
    policy.logstd_host is refreshed from policy.logstd -- the Runner passes logstd by value from that host copy and would
    otherwise go on sampling with the old standard deviation; that is one device -> host copy of 16 bytes per update.
    -> {"stats": [steps, 6] device tensor (STAT_NAMES), "grads": the thirteen slots' gradients of the last step on request}."""
    import torch
    ws = policy_tensors(policy)
    dev = ws[0].device
    if dev.type != "cuda":
        raise _lib.QuadsimError("ppo2_update needs the policy on a HIP device, it is on %s; torch_ppo2_update is the host path" % dev)
    data = rollout_tensors(rollout)
    n = _check_rollout(dev, *data)
    _check_indices(indices, dev, n, check_indices)
    steps, batch = int(indices.shape[0]), int(indices.shape[1])
    nslices = 0 if slices == "auto" else int(slices)
    m, v = _state(policy, ws)
    crv = cliprange if cliprange_vf is None else cliprange_vf
    mgn = 0.0 if max_grad_norm is None else max_grad_norm
    lib = load_ppo()
    stats = _lib.new_tensor(dev, (steps, len(STAT_NAMES)), "float32")
    grads = [None if w is None else torch.empty_like(w) for w in ws] if return_grads else None
    for s0 in range(0, steps, PPO_MAX_STEPS):
        part = min(PPO_MAX_STEPS, steps - s0)
        _, _, _, _, hp, t0 = check_ppo2_args(n, part, batch, nslices, learning_rate, cliprange, crv, ent_coef, vf_coef, mgn,
                                             t0=policy._ppo_steps)
        need = C.c_size_t(0)
        _lib.side_call("ppo", lib, "qsp_workspace_bytes", batch, nslices, C.byref(need))
        if policy._ppo_ws is None or policy._ppo_ws.numel() < need.value:
            policy._ppo_ws = _lib.new_tensor(dev, (need.value,), "uint8")
        net = QspNet(C.sizeof(QspNet), 1 if ws[6] is not None else 0, _lib.pointers(ws), _lib.pointers(m), _lib.pointers(v))
        bat = QspBatch(C.sizeof(QspBatch), 0, n, *map(_lib.as_arg, data))
        hyp = QspHyper(C.sizeof(QspHyper), 0, *(hp[k] for k in ("lr", "cliprange", "cliprange_vf", "ent_coef", "vf_coef", "max_grad_norm",
                                                               "beta1", "beta2", "eps")))
        last = s0 + part == steps
        _lib.side_call("ppo", lib, "qsp_update", C.byref(net), C.byref(bat), indices[s0:s0 + part], part, batch, nslices, C.byref(hyp), t0,
                       policy._ppo_ws, int(policy._ppo_ws.numel()), stats[s0:s0 + part],
                       C.byref(_lib.pointers(grads)) if grads is not None and last else None, device=dev)
        policy._ppo_steps += part
    _after_update(policy)
    return {"stats": stats, "grads": grads}


# ---------------------------------------------------------------------------------------------------- the same update on torch
def ppo2_loss(torch, P, obs, actions, returns, values, neglogp, cliprange, cliprange_vf, ent_coef, vf_coef):
    """the loss of ppo2.py:147-188 on torch -> (loss, (pg_loss, vf_loss, entropy, approxkl, clipfrac)); P: {slot key: tensor}"""
    adv = returns - values
    adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    h = torch.relu(obs @ P["w0"] + P["b0"])
    mean = torch.relu(h @ P["w1"] + P["b1"]) @ P["w2"] + P["b2"]
    hv = torch.relu(obs @ P["wv0"] + P["bv0"]) if "wv0" in P else h
    vpred = (torch.relu(hv @ P["wv1"] + P["bv1"]) @ P["wv2"] + P["bv2"])[:, 0]
    logstd = P["logstd"]
    nl = 0.5 * (((actions - mean) / torch.exp(logstd)) ** 2).sum(-1) + 0.5 * math.log(2.0 * math.pi) * 4.0 + logstd.sum()
    entropy = (logstd + 0.5 * math.log(2.0 * math.pi * math.e)).sum()
    if cliprange_vf < 0:
        vclip = vpred
    else:
        vclip = values + torch.clamp(vpred - values, -cliprange_vf, cliprange_vf)
    vf_loss = 0.5 * torch.maximum((vpred - returns) ** 2, (vclip - returns) ** 2).mean()
    ratio = torch.exp(neglogp - nl)
    pg_loss = torch.maximum(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - cliprange, 1.0 + cliprange)).mean()
    approxkl = 0.5 * ((nl - neglogp) ** 2).mean()
    clipfrac = ((ratio - 1.0).abs() > cliprange).to(obs.dtype).mean()
    return pg_loss - entropy * ent_coef + vf_loss * vf_coef, (pg_loss, vf_loss, entropy, approxkl, clipfrac)


def torch_ppo2_update(policy, rollout, indices, *, learning_rate, cliprange, cliprange_vf=None, ent_coef, vf_coef, max_grad_norm,
                      return_grads=False, **_ignored):
    """ppo2_update as a plain torch autograd loop on whatever device the policy is on: the loss transcribed from ppo2.py:147-188,
    tf.clip_by_global_norm and tf.train.AdamOptimizer's formula (not torch.optim.Adam's, whose epsilon sits elsewhere).  Shares the
    optimiser state kept on the policy with ppo2_update.  Same result dict; the bits differ (library GEMMs, float32 reductions)."""
    import torch
    ws = policy_tensors(policy)
    data = rollout_tensors(rollout)
    obs, actions, returns, values, neglogp = data
    m, v = _state(policy, ws)
    crv = float(cliprange if cliprange_vf is None else cliprange_vf)
    steps = int(indices.shape[0])
    _, _, _, _, hp, _ = check_ppo2_args(obs.shape[0], min(steps, PPO_MAX_STEPS), indices.shape[1], 0, learning_rate, cliprange, crv, ent_coef,
                                        vf_coef, 0.0 if max_grad_norm is None else max_grad_norm, t0=policy._ppo_steps)
    keys = [k for k, w in zip(SLOT_KEYS, ws) if w is not None]
    live = [w for w in ws if w is not None]
    lm, lv = [x for x in m if x is not None], [x for x in v if x is not None]
    stats = torch.empty((steps, len(STAT_NAMES)), dtype=torch.float32, device=obs.device)
    grads = None
    for s in range(steps):
        rows = indices[s].long()
        P = {k: w.detach().requires_grad_(True) for k, w in zip(keys, live)}
        loss, parts = ppo2_loss(torch, P, obs[rows], actions[rows], returns[rows], values[rows], neglogp[rows], hp["cliprange"], crv,
                                hp["ent_coef"], hp["vf_coef"])
        grads = torch.autograd.grad(loss, [P[k] for k in keys])
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).float()
        stats[s] = torch.stack([p.detach().float() for p in parts] + [norm])
        scale = hp["max_grad_norm"] / torch.clamp(norm, min=hp["max_grad_norm"]) if hp["max_grad_norm"] > 0.0 else 1.0
        t = policy._ppo_steps + 1
        lr_t = hp["lr"] * math.sqrt(1.0 - hp["beta2"] ** t) / (1.0 - hp["beta1"] ** t)
        with torch.no_grad():
            for w, g, mm, vv in zip(live, grads, lm, lv):
                g = g * scale
                mm.mul_(hp["beta1"]).add_(g, alpha=1.0 - hp["beta1"])
                vv.mul_(hp["beta2"]).addcmul_(g, g, value=1.0 - hp["beta2"])
                w.sub_(lr_t * mm / (vv.sqrt() + hp["eps"]))
        policy._ppo_steps += 1
    _after_update(policy)
    out = None
    if return_grads:
        it = iter(grads)
        out = [None if w is None else next(it) for w in ws]
    return {"stats": stats, "grads": out}


# ---------------------------------------------------------------------------------------------------- the loop
def explained_variance(values, returns):
    """1 - Var[returns - values] / Var[returns] (nan for constant returns), a device scalar"""
    var = returns.var(unbiased=False)
    return 1.0 - (returns - values).var(unbiased=False) / var


class PPO2:
    """``PPO2(policy, env, ...).learn(total_timesteps)``: the loop of ppo2.py:321-404 over the package's Runner, the roll-out and
    the update on the device.  learning_rate and cliprange are floats or callables of the remaining progress ``frac`` (1 -> 0);
    no other schedule.  `update`: "hip" (ppo2_update) or "torch" (torch_ppo2_update).  `runner`: a ready Runner (tests)."""

    def __init__(self, policy, env, *, n_steps=128, nminibatches=4, noptepochs=4, gamma=0.99, lam=0.95, ent_coef=0.01, vf_coef=0.5,
                 learning_rate=2.5e-4, max_grad_norm=0.5, cliprange=0.2, cliprange_vf=None, seed=0, precision="f32", update="hip",
                 slices="auto", runner=None):
        import torch
        if getattr(policy, "squash", False):
            raise ValueError("PPO2 does not cover the tanh-squashed policies of the fork (squash=True)")
        if update not in ("hip", "torch"):
            raise ValueError("update must be 'hip' or 'torch', got %r" % (update,))
        self.policy, self.env = policy, env
        self.n_steps, self.nminibatches, self.noptepochs = int(n_steps), int(nminibatches), int(noptepochs)
        self.n_batch = int(env.num_envs) * self.n_steps
        if self.n_batch % self.nminibatches != 0:
            raise ValueError("nminibatches = %d is not a factor of n_batch = %d" % (self.nminibatches, self.n_batch))
        self.ent_coef, self.vf_coef, self.max_grad_norm = float(ent_coef), float(vf_coef), max_grad_norm
        self.learning_rate, self.cliprange, self.cliprange_vf = learning_rate, cliprange, cliprange_vf
        self.update, self.slices = update, slices
        self.generator = torch.Generator().manual_seed(int(seed))
        if runner is None:
            from .runner import Runner
            runner = Runner(env=env, model=policy, n_steps=self.n_steps, gamma=gamma, lam=lam, collect_ep_infos=False, precision=precision)
        self.runner = runner
        self.num_timesteps = 0

    @staticmethod
    def _now(x, frac):
        return float(x(frac)) if callable(x) else float(x)

    def learn(self, total_timesteps, callback=None, log_interval=1):
        """-> a list of one dict per logged update (what the reference hands to logger.dumpkvs).  callback(locals_, globals_)
        returning False stops the loop."""
        fn = ppo2_update if self.update == "hip" else torch_ppo2_update
        n_updates = int(total_timesteps) // self.n_batch
        logs, t_first = [], time.time()
        for update in range(1, n_updates + 1):
            t_start = time.time()
            frac = 1.0 - (update - 1.0) / n_updates
            lr_now, cliprange_now = self._now(self.learning_rate, frac), self._now(self.cliprange, frac)
            crv_now = None if self.cliprange_vf is None else self._now(self.cliprange_vf, frac)
            rollout = self.runner.run()
            self.num_timesteps += self.n_batch
            obs, returns, _, _, values = rollout[:5]
            indices = minibatch_schedule(self.n_batch, self.nminibatches, self.noptepochs, self.generator, obs.device)
            out = fn(self.policy, rollout, indices, learning_rate=lr_now, cliprange=cliprange_now, cliprange_vf=crv_now,
                     ent_coef=self.ent_coef, vf_coef=self.vf_coef, max_grad_norm=self.max_grad_norm, slices=self.slices,
                     check_indices=False)
            if log_interval and (update % log_interval == 0 or update == 1):
                loss_vals = out["stats"].double().mean(0).tolist()       # the update is over here: the one wait of an update
                t_now = time.time()
                log = {"serial_timesteps": update * self.n_steps, "n_updates": update, "total_timesteps": self.num_timesteps,
                       "fps": int(self.n_batch / max(t_now - t_start, 1e-9)), "explained_variance": float(explained_variance(values, returns)),
                       "time_elapsed": t_start - t_first, "learning_rate": lr_now, "cliprange": cliprange_now}
                rets, lens = getattr(self.runner, "last_ep_returns", None), getattr(self.runner, "last_ep_lengths", None)
                if rets is not None and rets.numel() > 0:
                    log["ep_reward_mean"], log["ep_len_mean"] = float(rets.double().mean()), float(lens.double().mean())
                log.update(zip(STAT_NAMES, loss_vals))
                logs.append(log)
            if callback is not None and callback(locals(), globals()) is False:
                break
        return logs
