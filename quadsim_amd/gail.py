"""GAIL on the device: generative adversarial imitation of the PID expert (run_docking_gail.py of the reference).

SB2's ``GAIL`` trains a ``TransitionClassifier`` -- a small net D(obs, act) -> logit that tells the policy's transitions (label 0,
the "generator") from the expert's (label 1) -- and hands the policy ``-log(1 - sigmoid(D) + 1e-8)`` as its reward instead of the
environment's.  Here the classifier is ``Discriminator``: its Adam steps run in ONE launch of one resident workgroup (``qsg_fit``
of libquadsim_gail.so, include/quadsim_gail.h has the numerical contract) and its reward pass over every row of a roll-out runs on
the exact-float32 matrix pipe (``qsg_reward``), writing the step-major array ``gae_and_flatten`` takes.  ``GailRunner`` is the
fused Runner with that reward between the roll-out and GAE; ``GAIL`` is the loop.

Decisions, where SB2 leaves a choice or we depart from it:
  * the generator of ``GAIL`` is this package's PPO2.  SB2's GAIL wraps TRPO: ``quadsim_amd.trpo.TRPO(..., expert_data=...)`` is that
    loop over the same ``GailRunner`` and ``Discriminator`` (towers layout, one GPU; the shared layout and multi-GPU are not built).
  * generator and expert actions pass the same clamp to [-1, 1]: the Runner stores the unclipped sample u and the env received
    clip(u); on expert rows the clamp is a no-op.
  * the running observation statistics (SB2's RunningMeanStd, float64, kept here in Python) take ONE merge per ``fit`` call, over
    the observations of every row that call's schedule touches, before the steps.  SB2 merges per step.
  * the reward is computed as -log(1 / (1 + exp(l)) + 1e-8): the same value without the float32 cancellation of 1 - sigmoid.
Squashed policies are refused, as ``ppo2_update`` refuses them.  There is no CPU path for the device entry points;
``torch_discriminator_fit`` is the same update as a torch autograd loop, the comparison path.
"""
import ctypes as C
import functools
import math
import time

import numpy as np

from . import _lib
from .ppo2 import PPO2, STAT_NAMES, explained_variance, minibatch_schedule, ppo2_update, torch_ppo2_update
from .rollout_buffer import gae_and_flatten, swap_and_flatten
from .runner import Runner, fused_runner_rollout

GAIL_MAX_HIDDEN, GAIL_MAX_BATCH, GAIL_MAX_STEPS = 128, 256, 4096
GAIL_BETA1, GAIL_BETA2 = 0.9, 0.999                 # tf.train.AdamOptimizer's defaults, which SB2's adversary leaves alone
GAIL_WIDTHS = (64, 128)                             # the compiled (padded) hidden widths, cheapest first
DISC_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
DISC_STAT_NAMES = ("gen_loss", "exp_loss", "entropy", "gen_acc", "exp_acc")

# libquadsim_gail.so is the entry "gail" of _lib.SIDE: its path, signatures, loader, status check and call helper are _lib's.
# The names below stay this module's so that callers and tests can replace the loader
QsgNet, GAIL_EXPORTS = _lib.QsgNet, _lib.SIDE["gail"]["exports"]
load_gail, check_gail = functools.partial(_lib.side_load, "gail"), functools.partial(_lib.side_check, "gail")


def disc_shapes(hidden):
    h = int(hidden)
    return ((16, h), (h,), (h, h), (h,), (h, 1), (1,))


def compiled_width(hidden):
    """the first compiled width that covers `hidden`"""
    return next(w for w in GAIL_WIDTHS if int(hidden) <= w)


def check_gail_args(n_gen, n_exp, steps, batch, hidden=100, entcoeff=1.0e-3, lr=3.0e-4, beta1=GAIL_BETA1, beta2=GAIL_BETA2, eps=1.0e-8,
                    t0=0, counts=None, gen_idx=None, exp_idx=None):
    """-> (n_gen, n_exp, steps, batch, hidden, entcoeff, lr, beta1, beta2, eps, t0); ValueError for what qsg_fit would refuse and,
    given the host arrays `counts` [steps] and `gen_idx` / `exp_idx` [steps,batch], for what it cannot check (a count outside
    [1, batch], a row it would read outside its array), before anything touches the library or the GPU"""
    n_gen, n_exp, steps, batch, hidden, t0 = int(n_gen), int(n_exp), int(steps), int(batch), int(hidden), int(t0)
    if not 1 <= hidden <= GAIL_MAX_HIDDEN:
        raise ValueError("hidden must be in [1, %d], got %d" % (GAIL_MAX_HIDDEN, hidden))
    if not 1 <= batch <= GAIL_MAX_BATCH:
        raise ValueError("batch must be in [1, %d], got %d" % (GAIL_MAX_BATCH, batch))
    if not 1 <= steps <= GAIL_MAX_STEPS:
        raise ValueError("steps must be in [1, %d], got %d" % (GAIL_MAX_STEPS, steps))
    for name, n in (("n_gen", n_gen), ("n_exp", n_exp)):
        if not 1 <= n < 1 << 31:
            raise ValueError("%s must be in [1, 2^31), got %d" % (name, n))
    entcoeff = float(entcoeff)
    if not math.isfinite(entcoeff):
        raise ValueError("entcoeff must be finite, got %r" % (entcoeff,))
    lr, beta1, beta2, eps = _lib.check_adam_args(lr, beta1, beta2, eps, t0, steps, "steps")
    if counts is not None:
        counts = np.asarray(counts)
        if counts.shape != (steps,) or counts.min() < 1 or counts.max() > batch:
            raise ValueError("counts must be [%d] values in [1, batch = %d]" % (steps, batch))
    for name, idx, n in (("gen_idx", gen_idx, n_gen), ("exp_idx", exp_idx, n_exp)):
        if idx is None:
            continue
        idx = np.asarray(idx)
        if idx.shape != (steps, batch):
            raise ValueError("%s must be [%d, %d], got %s" % (name, steps, batch, idx.shape))
        used = idx if counts is None else idx[np.arange(batch)[None, :] < counts[:, None]]
        if used.min() < 0 or used.max() >= n:
            raise ValueError("the rows of %s the fit would read must be in [0, %d), got [%d, %d]" % (name, n, used.min(), used.max()))
    return n_gen, n_exp, steps, batch, hidden, entcoeff, lr, beta1, beta2, eps, t0


def check_reward_args(rows, n_envs=None, n_steps=None, grid=0):
    """-> (rows, n_envs, n_steps, grid) as qsg_reward takes them (0, 0: no transposition); ValueError for what it would refuse"""
    rows, grid = int(rows), int(grid)
    if not 1 <= rows < 1 << 31:
        raise ValueError("rows must be in [1, 2^31), got %d" % rows)
    if (n_envs is None) != (n_steps is None):
        raise ValueError("n_envs and n_steps go together")
    n_envs, n_steps = (0, 0) if n_envs is None else (int(n_envs), int(n_steps))
    if (n_envs or n_steps) and (n_envs < 1 or n_steps < 1 or n_envs * n_steps != rows):
        raise ValueError("n_envs x n_steps must be rows = %d, got %d x %d" % (rows, n_envs, n_steps))
    if not 0 <= grid <= 65535:
        raise ValueError("grid must be in [0, 65535], got %d" % grid)
    return rows, n_envs, n_steps, grid


# ---------------------------------------------------------------------------------------------------- the schedule
class ExpertCursor:
    """the walk through successive shuffles of the expert's train rows, carried across calls of discriminator_schedule"""

    def __init__(self, rows):
        import torch
        self.rows = torch.as_tensor(rows).to(torch.int32).reshape(-1).cpu()
        if self.rows.numel() < 1:
            raise ValueError("the expert has no train rows")
        self.order, self.pos = None, 0

    def take(self, k, generator):
        """the next k rows: a step never holds a row twice unless the expert has fewer than k rows"""
        import torch
        n = int(self.rows.numel())
        out = []
        while k > 0:
            if self.order is None or self.pos >= n:
                self.order, self.pos = torch.randperm(n, generator=generator), 0
            part = self.order[self.pos:self.pos + k]
            self.pos += int(part.numel())
            k -= int(part.numel())
            out.append(part)
        return self.rows[torch.cat(out)]


def discriminator_schedule(n_gen, expert_rows, batch, steps, generator):
    """-> (gen_idx, exp_idx), two CPU int32 [steps, batch] arrays.  Generator rows: consecutive pieces of permutations of
    0 .. n_gen-1 (a fresh one wherever the rest of the current one cannot fill a step, so no row twice inside a step).  Expert rows:
    `expert_rows` is an ExpertCursor (or the train rows, for a one-off cursor): consecutive pieces of successive shuffles, the
    position carried across calls; a step that would straddle two shuffles starts the next one, unless the expert has fewer than
    `batch` rows.  Draws from `generator` (a CPU torch.Generator) step by step, generator rows first: the schedule of a + b steps is
    the schedules of a and of b steps drawn one after another."""
    import torch
    n_gen, batch, steps = int(n_gen), int(batch), int(steps)
    if n_gen < 1 or batch < 1 or steps < 1:
        raise ValueError("n_gen, batch and steps must be >= 1")
    if batch > n_gen:
        raise ValueError("batch = %d exceeds the roll-out's %d rows" % (batch, n_gen))
    cur = expert_rows if isinstance(expert_rows, ExpertCursor) else ExpertCursor(expert_rows)
    n_exp = int(cur.rows.numel())
    gen = torch.empty((steps, batch), dtype=torch.int32)
    exp = torch.empty((steps, batch), dtype=torch.int32)
    perm, pos = None, 0
    for s in range(steps):
        if perm is None or pos + batch > n_gen:
            perm, pos = torch.randperm(n_gen, generator=generator).to(torch.int32), 0
        gen[s] = perm[pos:pos + batch]
        pos += batch
        if batch <= n_exp and cur.order is not None and cur.pos + batch > n_exp:
            cur.pos = n_exp                                  # the rest of this shuffle cannot fill the step: start the next
        exp[s] = cur.take(batch, generator)
    return gen, exp


# ---------------------------------------------------------------------------------------------------- the discriminator
class RunningMeanStd:
    """SB2's RunningMeanStd of the adversary's observations, float64 on the host: sum, sum of squares and count start at 0, 1e-2
    and 1e-2; mean = sum / count, std = sqrt(max(sumsq / count - mean^2, 1e-2))"""

    def __init__(self, dim=12, epsilon=1.0e-2):
        self.sum, self.sumsq, self.count = np.zeros(dim, np.float64), np.full(dim, epsilon, np.float64), float(epsilon)

    def update(self, x):
        x = np.asarray(x, np.float64).reshape(-1, self.sum.shape[0])
        self.sum += x.sum(0)
        self.sumsq += np.square(x).sum(0)
        self.count += float(x.shape[0])

    @property
    def mean(self):
        return self.sum / self.count

    @property
    def std(self):
        return np.sqrt(np.maximum(self.sumsq / self.count - np.square(self.mean), 1.0e-2))


class Discriminator:
    """D(obs[12], act[4]) -> logit, 16 -> hidden -> hidden -> 1 with tanh (SB2's TransitionClassifier, hidden_size_adversary =
    100).  Xavier-uniform weights and zero biases, as tf.contrib.layers.fully_connected gives them, drawn from `seed`; weights in
    the policy's (in, out) layout, float32, with Adam's moments and step count on the object."""

    def __init__(self, hidden=100, entcoeff=1.0e-3, seed=0, device="cuda", weights=None):
        import torch
        self.hidden, self.entcoeff = int(hidden), float(entcoeff)
        check_gail_args(1, 1, 1, 1, self.hidden, self.entcoeff)
        self.device = torch.device(device)
        shapes = disc_shapes(self.hidden)
        if weights is None:
            rng = np.random.default_rng(int(seed))
            weights = {}
            for k, shape in zip(DISC_KEYS, shapes):
                if len(shape) == 2:
                    lim = math.sqrt(6.0 / (shape[0] + shape[1]))
                    weights[k] = rng.uniform(-lim, lim, shape).astype(np.float32)
                else:
                    weights[k] = np.zeros(shape, np.float32)
        for k, shape in zip(DISC_KEYS, shapes):
            w = np.ascontiguousarray(weights[k], np.float32)
            if w.shape != shape:
                raise ValueError("%s must be of shape %s, got %s" % (k, shape, w.shape))
            setattr(self, k, torch.as_tensor(w.copy()).to(self.device))
        self.device = self.w0.device                     # "cuda" -> the device the tensors landed on
        self.stats = RunningMeanStd(12)
        self.reset_optimizer()
        self._norm = None

    # -- state
    def tensors(self):
        return [getattr(self, k) for k in DISC_KEYS]

    def reset_optimizer(self):
        """forget Adam's moments and the step count"""
        import torch
        self.m, self.v, self.steps = [torch.zeros_like(w) for w in self.tensors()], [torch.zeros_like(w) for w in self.tensors()], 0

    def norm_tensors(self):
        """(mean, rscale) [12] float32 on the device, from the running statistics as they stand"""
        import torch
        if self._norm is None:
            mean, rscale = self.stats.mean.astype(np.float32), (1.0 / self.stats.std).astype(np.float32)
            self._norm = (torch.as_tensor(mean).to(self.device), torch.as_tensor(rscale).to(self.device))
        return self._norm

    def update_stats(self, obs_rows):
        """one merge of the running observation statistics (host float64)"""
        self.stats.update(obs_rows)
        self._norm = None

    def save_npz(self, path):
        arrays = {k: getattr(self, k).detach().cpu().numpy() for k in DISC_KEYS}
        arrays.update({"m_" + k: m.cpu().numpy() for k, m in zip(DISC_KEYS, self.m)})
        arrays.update({"v_" + k: v.cpu().numpy() for k, v in zip(DISC_KEYS, self.v)})
        np.savez(path, hidden=self.hidden, entcoeff=self.entcoeff, steps=self.steps, rms_sum=self.stats.sum, rms_sumsq=self.stats.sumsq,
                 rms_count=self.stats.count, **arrays)

    @classmethod
    def from_npz(cls, path, device="cuda"):
        import torch
        with np.load(path, allow_pickle=False) as z:
            d = cls(int(z["hidden"]), float(z["entcoeff"]), device=device, weights={k: z[k] for k in DISC_KEYS})
            d.m = [torch.as_tensor(z["m_" + k].copy()).to(d.device) for k in DISC_KEYS]
            d.v = [torch.as_tensor(z["v_" + k].copy()).to(d.device) for k in DISC_KEYS]
            d.steps = int(z["steps"])
            d.stats.sum, d.stats.sumsq, d.stats.count = z["rms_sum"].astype(np.float64), z["rms_sumsq"].astype(np.float64), float(z["rms_count"])
        return d

    def _net(self, with_state=True):
        mean, rscale = self.norm_tensors()
        null = (C.c_void_p * 6)()
        return QsgNet(C.sizeof(QsgNet), self.hidden, _lib.six(self.tensors()), _lib.six(self.m) if with_state else null,
                      _lib.six(self.v) if with_state else null, _lib.as_arg(mean), _lib.as_arg(rscale))

    def _need_device(self, what):
        if self.device.type != "cuda":
            raise _lib.QuadsimError("%s needs the discriminator on a HIP device, it is on %s; torch_discriminator_fit is the host path"
                                    % (what, self.device))

    # -- the two device entry points
    def fit(self, gen_obs, gen_act, expert, gen_idx, exp_idx, counts=None, lr=3.0e-4, beta1=GAIL_BETA1, beta2=GAIL_BETA2, eps=1.0e-8,
            return_grads=False, update_stats=True):
        """ONE launch of qsg_fit: gen_idx.shape[0] Adam steps.  gen_obs [n,12] / gen_act [n,4]: the roll-out's rows, device
        tensors; expert: an ExpertData (or anything with .obs / .actions on the device); gen_idx, exp_idx [steps,batch] int32 and
        counts [steps] int32 (or None): HOST tensors, checked here (check_gail_args) and uploaded.  With update_stats the running
        observation statistics first take one merge over every row the schedule touches.  The weights, the moments and the step
        count are updated in place.  -> {"stats": [steps, 5] device tensor (DISC_STAT_NAMES, from the weights before each
        step), "grads": six device tensors of the last step on request}.  Launched on torch's current stream."""
        return _fit(self, gen_obs, gen_act, expert, gen_idx, exp_idx, counts, lr, beta1, beta2, eps, return_grads, update_stats, device=True)

    def reward(self, obs, act, n_envs=None, n_steps=None, return_logits=False, grid=0):
        """qsg_reward: -log(1 - sigmoid(D(obs, act)) + 1e-8) of obs [rows,12] / act [rows,4] (device tensors) -> reward [rows], or
        with n_envs and n_steps (rows = n_envs n_steps, the rows env-major as Runner.run() flattens them) the step-major
        [n_steps, n_envs] array gae_and_flatten takes; return_logits: (reward, logits) of the same shape.  The bits do not depend
        on `grid`."""
        self._need_device("reward")
        dev = self.device
        _lib.check_tensor("obs", obs, "float32", ("rows", 12), dev)
        _lib.check_tensor("act", act, "float32", (int(obs.shape[0]), 4), dev)
        rows, ne, ns, grid = check_reward_args(obs.shape[0], n_envs, n_steps, grid)
        shape = (ns, ne) if ne else (rows,)
        reward = _lib.new_tensor(dev, shape, "float32")
        logits = _lib.new_tensor(dev, shape, "float32") if return_logits else None
        net = self._net(with_state=False)
        _lib.side_call("gail", load_gail(), "qsg_reward", C.byref(net), obs, act, rows, ne, ns, reward, logits, grid, device=dev)
        return (reward, logits) if return_logits else reward


def _host_schedule(torch, idx, name):
    idx = torch.as_tensor(idx)
    if idx.dtype != torch.int32 or idx.dim() != 2 or idx.device.type != "cpu":
        raise ValueError("%s must be a host int32 tensor [steps, batch]" % name)
    return idx.contiguous()


def _fit(disc, gen_obs, gen_act, expert, gen_idx, exp_idx, counts, lr, beta1, beta2, eps, return_grads, update_stats, device):
    """what Discriminator.fit and torch_discriminator_fit share: the checks, the merge of the statistics, the state"""
    import torch
    dev = disc.device
    if device:
        disc._need_device("fit")
    exp_obs, exp_act = expert.obs, expert.actions
    for name, o, a in (("gen", gen_obs, gen_act), ("expert", exp_obs, exp_act)):
        _lib.check_tensor(name + " obs", o, "float32", ("n", 12), dev)
        _lib.check_tensor(name + " actions", a, "float32", (int(o.shape[0]), 4), dev)
    gen_idx, exp_idx = _host_schedule(torch, gen_idx, "gen_idx"), _host_schedule(torch, exp_idx, "exp_idx")
    if counts is not None:
        counts = torch.as_tensor(counts)
        if counts.dtype != torch.int32 or counts.device.type != "cpu":
            raise ValueError("counts must be a host int32 tensor [steps]")
    steps, batch = int(gen_idx.shape[0]), int(gen_idx.shape[1])
    n_gen, n_exp, steps, batch, hidden, entcoeff, lr, beta1, beta2, eps, t0 = check_gail_args(
        gen_obs.shape[0], exp_obs.shape[0], steps, batch, disc.hidden, disc.entcoeff, lr, beta1, beta2, eps, disc.steps,
        None if counts is None else counts.numpy(), gen_idx.numpy(), exp_idx.numpy())
    if update_stats:
        used = torch.ones((steps, batch), dtype=torch.bool) if counts is None else torch.arange(batch)[None, :] < counts[:, None].long()
        g_rows, e_rows = gen_idx[used].long().to(dev), exp_idx[used].long().to(dev)
        disc.update_stats(torch.cat([gen_obs[g_rows], exp_obs[e_rows]]).double().cpu().numpy())
    ws = disc.tensors()
    out = {"stats": _lib.new_tensor(dev, (steps, len(DISC_STAT_NAMES)), "float32"), "grads": None}
    if device:
        gi, ei = gen_idx.to(dev), exp_idx.to(dev)
        cnt = None if counts is None else counts.contiguous().to(dev)
        if return_grads:
            out["grads"] = [torch.empty_like(w) for w in ws]
        net = disc._net()
        _lib.side_call("gail", load_gail(), "qsg_fit", C.byref(net), gen_obs, gen_act, n_gen, exp_obs, exp_act, n_exp, gi, ei, cnt, steps, batch,
                       entcoeff, lr, beta1, beta2, eps, t0, out["stats"], _lib.six(out["grads"]) if return_grads else None, device=dev)
        disc.steps += steps
        return out
    mean, rscale = disc.norm_tensors()
    F = torch.nn.functional
    for s in range(steps):
        c = batch if counts is None else int(counts[s])
        rows = [gen_idx[s, :c].long().to(dev), exp_idx[s, :c].long().to(dev)]
        x = torch.cat([torch.cat([(gen_obs[rows[0]] - mean) * rscale, gen_act[rows[0]].clamp(-1.0, 1.0)], 1),
                       torch.cat([(exp_obs[rows[1]] - mean) * rscale, exp_act[rows[1]].clamp(-1.0, 1.0)], 1)])
        P = [w.detach().requires_grad_(True) for w in ws]
        l = (torch.tanh(torch.tanh(x @ P[0] + P[1]) @ P[2] + P[3]) @ P[4] + P[5])[:, 0]
        lg, le = l[:c], l[c:]
        gen_loss = F.binary_cross_entropy_with_logits(lg, torch.zeros_like(lg))
        exp_loss = F.binary_cross_entropy_with_logits(le, torch.ones_like(le))
        entropy = (torch.sigmoid(-l) * l + F.softplus(-l)).mean()
        grads = torch.autograd.grad(gen_loss + exp_loss - entcoeff * entropy, P)
        out["stats"][s] = torch.stack([gen_loss.detach(), exp_loss.detach(), entropy.detach(), (lg < 0).float().mean(), (le > 0).float().mean()])
        t = disc.steps + 1
        lr_t = lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        with torch.no_grad():
            for w, g, mm, vv in zip(ws, grads, disc.m, disc.v):
                mm.mul_(beta1).add_(g, alpha=1.0 - beta1)
                vv.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
                w.sub_(lr_t * mm / (vv.sqrt() + eps))
        disc.steps += 1
        if return_grads:
            out["grads"] = list(grads)
    return out


def torch_discriminator_fit(disc, gen_obs, gen_act, expert, gen_idx, exp_idx, counts=None, lr=3.0e-4, beta1=GAIL_BETA1, beta2=GAIL_BETA2,
                            eps=1.0e-8, return_grads=False, update_stats=True):
    """Discriminator.fit as a plain torch autograd loop on whatever device the discriminator is on: sigmoid cross-entropy through
    binary_cross_entropy_with_logits, the entropy bonus, tf.train.AdamOptimizer's formula (not torch.optim.Adam's, whose epsilon
    sits elsewhere), the same state and the same merge of the statistics.  Same result dict; the bits differ (library GEMMs)."""
    return _fit(disc, gen_obs, gen_act, expert, gen_idx, exp_idx, counts, lr, beta1, beta2, eps, return_grads, update_stats, device=False)


# ---------------------------------------------------------------------------------------------------- the loop
class GailRunner(Runner):
    """the Runner whose policy is paid by the discriminator: ``run()`` replaces the env's rewards by
    ``discriminator.reward(...)`` between the roll-out and ``gae_and_flatten``.  The returns are GAE over the discriminator's
    rewards; the 9th element of the tuple (true_reward) and the episode statistics keep the env's TRUE rewards.  `fused` is the
    Runner's: None = the fused roll-out wherever its kernel applies, else the spelt-out loop -- which is what docking-v1 gets,
    whose stored initial states the fused kernel refuses."""

    def __init__(self, *, discriminator, fused=None, **kw):
        env = kw["env"]
        if fused is None and getattr(env, "kind", None) == _lib.KIND_V1:
            fused = False
        super().__init__(fused=fused, **kw)
        self.discriminator = discriminator
        self.last_reward = None                      # [n_steps, n_envs]: what the policy was paid in the last run()

    def run(self, noise=None):
        env, T = self.env, self.n_steps
        mb_states = self.states
        if self.fused:
            ro = fused_runner_rollout(env, self.model, T, noise=noise, dones_in=self.dones, precision=self.precision, env_major=True)
            flat_obs, flat_actions = ro["obs"].view(T * env.num_envs, 12), ro["actions"].view(T * env.num_envs, 4)
        else:
            ro = self._stepwise_rollout(noise)
            flat_obs, flat_actions = swap_and_flatten(env, ro["obs"]), swap_and_flatten(env, ro["actions"])
        self.num_timesteps += T * env.num_envs
        self.last_reward = self.discriminator.reward(flat_obs, flat_actions, n_envs=env.num_envs, n_steps=T)
        gf = gae_and_flatten(env, self.last_reward, ro["values"], ro["neglogp"], ro["dones"], ro["last_values"], ro["last_dones"],
                             self.gamma, self.lam)
        ep_infos = []
        if self.track_episodes:
            ep_infos = self._episode_infos(ro["rewards"], ro["dones"], ro["last_dones"])
        self.obs, self.dones = ro["last_obs"], ro["last_dones"]
        out = (flat_obs, gf["returns"], gf["masks"], flat_actions, gf["values"], gf["neglogp"], mb_states, ep_infos,
               swap_and_flatten(env, ro["rewards"]))
        if self.reset_after_run:
            self.obs = env.reset()
        return out


class GAIL(PPO2):
    """``GAIL(policy, env, expert_data, ...).learn(total_timesteps)``: per update one roll-out scored by the current discriminator
    (GailRunner), one PPO2 update on it, then `d_steps` discriminator steps of `d_batch` rows per class on that roll-out's rows
    against expert rows (discriminator_schedule, the expert's shuffles carried from update to update).  The generator is this
    package's PPO2 -- SB2's GAIL wraps TRPO.  `update`: "hip" (ppo2_update and Discriminator.fit) or "torch" (the two torch
    comparison paths).  `fused`: GailRunner's (None: the fused roll-out where its kernel applies; docking-v1 takes the spelt-out
    loop).  Every other keyword is PPO2's."""

    def __init__(self, policy, env, expert_data, *, discriminator=None, d_steps=1, d_batch=256, d_learning_rate=3.0e-4, update="hip",
                 gamma=0.99, lam=0.95, precision="f32", fused=None, **ppo2_kwargs):
        if getattr(policy, "squash", False):
            raise ValueError("GAIL does not cover the tanh-squashed policies of the fork (squash=True)")
        if update not in ("hip", "torch"):
            raise ValueError("update must be 'hip' or 'torch', got %r" % (update,))
        self.d_steps, self.d_batch, self.d_learning_rate = int(d_steps), int(d_batch), float(d_learning_rate)
        n_steps = int(ppo2_kwargs.get("n_steps", 128))
        check_gail_args(int(env.num_envs) * n_steps, expert_data.obs.shape[0], self.d_steps, self.d_batch, lr=self.d_learning_rate)
        if self.d_batch > int(env.num_envs) * n_steps:
            raise ValueError("d_batch = %d exceeds the roll-out's %d rows" % (self.d_batch, int(env.num_envs) * n_steps))
        self.expert = expert_data
        self.discriminator = discriminator if discriminator is not None else Discriminator(device=env.device)
        runner = ppo2_kwargs.pop("runner", None)
        if runner is None:
            runner = GailRunner(discriminator=self.discriminator, env=env, model=policy, n_steps=n_steps, gamma=gamma, lam=lam,
                                collect_ep_infos=False, precision=precision, fused=fused)
        super().__init__(policy, env, gamma=gamma, lam=lam, precision=precision, update=update, runner=runner, **ppo2_kwargs)
        self.cursor = ExpertCursor(getattr(expert_data, "train_rows", None) if getattr(expert_data, "train_rows", None) is not None
                                   else np.arange(int(expert_data.obs.shape[0])))

    def learn(self, total_timesteps, callback=None, log_interval=1):
        """-> a list of one dict per logged update: PPO2's fields, the five discriminator statistics (DISC_STAT_NAMES, the mean
        over the update's d_steps), `disc_reward_mean` (what the policy was paid) and `true_ep_reward_mean` (the mean TRUE return of
        the episodes that ended in the roll-out, where any did)"""
        fn = ppo2_update if self.update == "hip" else torch_ppo2_update
        d_fit = self.discriminator.fit if self.update == "hip" else functools.partial(torch_discriminator_fit, self.discriminator)
        n_updates = int(total_timesteps) // self.n_batch
        logs, t_first = [], time.time()
        for update in range(1, n_updates + 1):
            t_start = time.time()
            frac = 1.0 - (update - 1.0) / n_updates
            lr_now, cliprange_now = self._now(self.learning_rate, frac), self._now(self.cliprange, frac)
            crv_now = None if self.cliprange_vf is None else self._now(self.cliprange_vf, frac)
            rollout = self.runner.run()
            self.num_timesteps += self.n_batch
            obs, returns, _, actions, values = rollout[:5]
            indices = minibatch_schedule(self.n_batch, self.nminibatches, self.noptepochs, self.generator, obs.device)
            out = fn(self.policy, rollout, indices, learning_rate=lr_now, cliprange=cliprange_now, cliprange_vf=crv_now,
                     ent_coef=self.ent_coef, vf_coef=self.vf_coef, max_grad_norm=self.max_grad_norm, slices=self.slices,
                     check_indices=False)
            gen_idx, exp_idx = discriminator_schedule(self.n_batch, self.cursor, self.d_batch, self.d_steps, self.generator)
            d_out = d_fit(obs, actions, self.expert, gen_idx, exp_idx, lr=self.d_learning_rate)
            if log_interval and (update % log_interval == 0 or update == 1):
                loss_vals = out["stats"].double().mean(0).tolist()
                t_now = time.time()
                log = {"serial_timesteps": update * self.n_steps, "n_updates": update, "total_timesteps": self.num_timesteps,
                       "fps": int(self.n_batch / max(t_now - t_start, 1e-9)), "explained_variance": float(explained_variance(values, returns)),
                       "time_elapsed": t_start - t_first, "learning_rate": lr_now, "cliprange": cliprange_now}
                rets, lens = getattr(self.runner, "last_ep_returns", None), getattr(self.runner, "last_ep_lengths", None)
                if rets is not None and rets.numel() > 0:
                    log["ep_reward_mean"] = log["true_ep_reward_mean"] = float(rets.double().mean())
                    log["ep_len_mean"] = float(lens.double().mean())
                log.update(zip(STAT_NAMES, loss_vals))
                log.update(zip(DISC_STAT_NAMES, d_out["stats"].double().mean(0).tolist()))
                paid = getattr(self.runner, "last_reward", None)
                if paid is not None:
                    log["disc_reward_mean"] = float(paid.double().mean())
                logs.append(log)
            if callback is not None and callback(locals(), globals()) is False:
                break
        return logs
