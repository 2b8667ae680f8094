"""TD3 on the device: DDPG with two critics, target-policy smoothing and a delayed actor (SB2's ``stable_baselines.td3``).

One update is up to seven forward passes, three backward passes, three Adam steps and a Polyak average of three target nets over
about 57 000 parameters: ``td3_update`` runs every update of a call through ``qstd_update`` of libquadsim_td3.so (include/quadsim_td3.h
is the numerical contract), one launch per update of two workgroups (q1, q2) or, on every `policy_delay`-th update, three (the actor as
well).  ``torch_td3_update`` is the same update as a plain autograd loop, the comparison.  Collection is ddpg.py's per-step loop.

The nets are SB2's TD3 ``MlpPolicy`` with ``layers = [128, 128]``, no layer norm, ReLU: the actor 12 -> 128 -> 128 -> 4 with tanh (the six
tensors of ``MlpPolicy``), two critics [12 obs + 4 actions] -> 128 -> 128 -> 1 (the action enters at the input: not DDPGPolicy's critic),
and a target copy of each.  The target noise is the caller's, or keyed Philox draws that depend on (seed, update index, row slot)
alone.  Not built: layer norm, prioritised replay, observation and return normalisation.
"""
import ctypes as C
import functools
import math

import numpy as np

from . import _lib, offpolicy
from .ddpg import NET_KEYS, OUNoise, ReplayBuffer, collect_and_train, replay_schedule  # noqa: F401  (the pieces TD3 shares with DDPG)

TD3_MAX_BATCH, TD3_MAX_STEPS, TD3_MAX_DELAY = 256, 4096, 1 << 16
TD3_BETA1, TD3_BETA2, TD3_EPS = 0.9, 0.999, 1.0e-8             # tf.train.AdamOptimizer's defaults, which SB2's TD3 leaves alone
TD3_NOISE_STREAM = 6                                           # the Philox stream of the target noise (include/quadsim_td3.h)
ACTOR_SHAPES = ((12, 128), (128,), (128, 128), (128,), (128, 4), (4,))
CRITIC_SHAPES = ((16, 128), (128,), (128, 128), (128,), (128, 1), (1,))
ONLINE_NAMES = ("actor", "q1", "q2")
NET_NAMES = ONLINE_NAMES + ("actor_target", "q1_target", "q2_target")
TD3_STAT_NAMES = ("q1_loss", "q2_loss", "q1_mean", "q2_mean", "y_mean", "actor_loss")

# libquadsim_td3.so is the entry "td3" of _lib.SIDE: its path, signatures, loader, status check and call helper are _lib's.
# The names below stay this module's so that callers and tests can replace the loader
QstdNets, QstdReplay, QstdHyper, TD3_EXPORTS = _lib.QstdNets, _lib.QstdReplay, _lib.QstdHyper, _lib.SIDE["td3"]["exports"]
load_td3, check_td3 = functools.partial(_lib.side_load, "td3"), functools.partial(_lib.side_check, "td3")


def shapes_of(name):
    return ACTOR_SHAPES if name.startswith("actor") else CRITIC_SHAPES


def actor_steps(t0, steps, policy_delay):
    """the number of updates u in [t0, t0 + steps) with u % policy_delay == 0: the actor steps of such a call"""
    first = lambda t: (t + policy_delay - 1) // policy_delay           # noqa: E731  (multiples of the delay below t)
    return first(t0 + steps) - first(t0)


def check_td3_args(n, steps, batch, gamma=0.99, tau=5.0e-3, actor_lr=3.0e-4, critic_lr=3.0e-4, policy_delay=2, target_policy_noise=0.2,
                   target_noise_clip=0.5, beta1=TD3_BETA1, beta2=TD3_BETA2, eps=TD3_EPS, t0=0, actor_t0=0, counts=None, indices=None):
    """-> (n, steps, batch, gamma, tau, actor_lr, critic_lr, policy_delay, target_policy_noise, target_noise_clip, beta1, beta2, eps,
    t0, actor_t0); ValueError for what qstd_update would refuse and, given the host arrays `counts` [steps] and `indices`
    [steps,batch], for what it cannot check (a count outside [1, batch], a row it would read outside [0, n)), before anything touches
    the library or the GPU"""
    n, steps, batch, t0, actor_t0, policy_delay = int(n), int(steps), int(batch), int(t0), int(actor_t0), int(policy_delay)
    offpolicy.check_extent(n, steps, batch, TD3_MAX_BATCH, TD3_MAX_STEPS)
    if not 1 <= policy_delay <= TD3_MAX_DELAY:
        raise ValueError("policy_delay must be in [1, %d], got %d" % (TD3_MAX_DELAY, policy_delay))
    if not (actor_t0 >= 0 and actor_t0 + steps < 1 << 31):
        raise ValueError("actor_t0 must be >= 0 with actor_t0 + steps below 2^31, got %d" % actor_t0)
    gamma, tau, actor_lr, critic_lr = float(gamma), float(tau), float(actor_lr), float(critic_lr)
    target_policy_noise, target_noise_clip = float(target_policy_noise), float(target_noise_clip)
    offpolicy.check_discount(gamma, tau)
    if not (target_policy_noise >= 0.0 and math.isfinite(target_policy_noise)):
        raise ValueError("target_policy_noise must be finite and >= 0, got %r" % target_policy_noise)
    if not target_noise_clip >= 0.0:
        raise ValueError("target_noise_clip must be >= 0 (inf: no clip), got %r" % target_noise_clip)
    for name, val in (("actor_lr", actor_lr), ("critic_lr", critic_lr)):
        if not math.isfinite(val):
            raise ValueError("%s must be finite, got %r" % (name, val))
    _, beta1, beta2, eps = _lib.check_adam_args(0.0, beta1, beta2, eps, t0, steps, "steps")
    offpolicy.check_schedule(n, steps, batch, counts, indices)
    return (n, steps, batch, gamma, tau, actor_lr, critic_lr, policy_delay, target_policy_noise, target_noise_clip, beta1, beta2, eps, t0,
            actor_t0)


def keyed_noise(seed, t0, steps, batch, stream=TD3_NOISE_STREAM):
    """-> [steps, batch, 4] float32: the target noise that a call without `noise` draws, restated on the host
    (offpolicy.keyed_noise; ``noise_out`` of td3_update has the device's values).  `stream`: the Philox stream in place of 6 (sac.py
    draws on 7)"""
    return offpolicy.keyed_noise(seed, t0, steps, batch, stream)


# ---------------------------------------------------------------------------------------------------- the nets
class TD3Policy(offpolicy.Nets):
    """the six nets of TD3 in the policy's (in, out) layout, as lists of six tensors: ``actor``, ``q1``, ``q2`` and ``actor_target``,
    ``q1_target``, ``q2_target``; Adam's moments of the three online nets (``m``, ``v``: {"actor": [...], "q1": [...], "q2": [...]}),
    the update count ``steps`` and the actor's own step count ``actor_steps``.  SB2's initialisation drawn from `seed`:
    Glorot-uniform weights, zero biases, the targets equal to the online nets.  `weights`: {"actor": {w0 ..}, "q1": {..}, "q2": {..}
    and optionally the three targets}.  `dtype`: "float32" (the device path needs it) or "float64" (torch_td3_update alone)."""

    NET_NAMES, ONLINE_NAMES, LIB = NET_NAMES, ONLINE_NAMES, ("td3", "qstd_workspace_bytes")
    shapes_of, load = staticmethod(shapes_of), staticmethod(lambda: load_td3())

    def __init__(self, seed=0, device="cuda", weights=None, dtype="float32"):
        self.init_nets(seed, device, weights, dtype)
        self.reset_optimizer()

    def reset_optimizer(self):
        """forget Adam's moments and both step counts"""
        self.zero_moments()
        self.steps, self.actor_steps = 0, 0

    def predict(self, obs):
        """obs [N,12] -> tanh actions [N,4] of the online actor (plain torch)"""
        import torch
        w = self.actor
        h = torch.relu(torch.addmm(w[1], obs.to(self.dtype), w[0]))
        h = torch.relu(torch.addmm(w[3], h, w[2]))
        return torch.tanh(torch.addmm(w[5], h, w[4]))

    def actor_weights(self):
        """the online actor in MlpPolicy's key names (numpy; cached until the next update): MlpPolicy clips where this actor
        squashes"""
        if "actor" not in self._images:
            self._images["actor"] = {k: w.detach().cpu().numpy().copy() for k, w in zip(NET_KEYS, self.actor)}   # (a host tensor's numpy() aliases it)
        return self._images["actor"]

    def npz_state(self):
        return {"steps": self.steps, "actor_steps": self.actor_steps}

    def set_npz_state(self, z):
        self.steps, self.actor_steps = int(z["steps"]), int(z["actor_steps"])


def reset_td3_optimizer(policy):
    """forget Adam's moments and both step counts of a TD3Policy"""
    policy.reset_optimizer()


class NormalActionNoise:
    """SB2's NormalActionNoise with mean 0: independent N(0, sigma^2) per env and action component, drawn on the device from `seed`;
    ``reset`` is a no-op (there is no state)"""

    def __init__(self, n_envs, sigma=0.1, device="cuda", seed=0):
        import torch
        self.sigma, self.n_envs = float(sigma), int(n_envs)
        self.device = torch.device(device)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))

    def __call__(self):
        import torch
        return self.sigma * torch.randn((self.n_envs, 4), generator=self.generator, device=self.device, dtype=torch.float32)

    def reset(self, done=None):
        pass


# ---------------------------------------------------------------------------------------------------- the update
def _update_args(policy, replay, indices, counts, hyper, noise, need_device):
    dev = policy.device
    dtype = str(policy.dtype).split(".")[-1]
    if need_device and (dev.type != "cuda" or dtype != "float32"):
        raise _lib.QuadsimError("td3_update needs a float32 policy on a HIP device, it is %s on %s; torch_td3_update is the host path"
                                % (dtype, dev))
    data, n, indices, counts = offpolicy.update_tensors(policy, replay, indices, counts, dtype)
    args = check_td3_args(n, indices.shape[0], indices.shape[1], t0=policy.steps, actor_t0=policy.actor_steps,
                          counts=None if counts is None else counts.numpy(), indices=indices.numpy(), **hyper)
    if noise is not None:
        _lib.check_tensor("noise", noise, "float32", (args[1], args[2], 4), dev)
    return data, indices.contiguous(), counts, args


def td3_update(policy, replay, indices, counts=None, gamma=0.99, tau=5.0e-3, actor_lr=3.0e-4, critic_lr=3.0e-4, policy_delay=2,
               target_policy_noise=0.2, target_noise_clip=0.5, noise=None, seed=0, return_grads=False, return_noise=False):
    """ONE call of qstd_update: indices.shape[0] TD3 updates of the policy's six nets.  replay: a ReplayBuffer or the five device
    tensors (obs0 [n,12], act [n,4], rew [n], obs1 [n,12], done [n]); indices [steps,batch] int32 and counts [steps] int32 (or None):
    HOST tensors, checked here (check_td3_args) and uploaded.  noise: [steps,batch,4] float32 standard normals on the device, or None:
    keyed Philox draws from `seed`, the update index and the row slot.  The 36 weights, the 36 moments and both step counts are
    updated in place.  -> {"stats": [steps, 6] device tensor (TD3_STAT_NAMES, from the weights before each step), "grads": {"actor":
    six, "q1": six, "q2": six} device tensors of the last step on request (the actor's are None where that step is no actor step),
    "noise": the [steps,batch,4] normals that were used, on request}.  Launched on torch's current stream; nothing waits for the
    device."""
    import torch
    hyper = dict(gamma=gamma, tau=tau, actor_lr=actor_lr, critic_lr=critic_lr, policy_delay=policy_delay,
                 target_policy_noise=target_policy_noise, target_noise_clip=target_noise_clip)
    data, indices, counts, args = _update_args(policy, replay, indices, counts, hyper, noise, True)
    n, steps, batch, gamma, tau, actor_lr, critic_lr, policy_delay, sigma, clip, beta1, beta2, eps, t0, actor_t0 = args
    dev = policy.device
    idx_d = indices.to(dev)
    cnt_d = None if counts is None else counts.contiguous().to(dev)
    out = {"stats": _lib.new_tensor(dev, (steps, len(TD3_STAT_NAMES)), "float32"), "grads": None, "noise": None}
    if return_noise:
        out["noise"] = torch.zeros((steps, batch, 4), dtype=torch.float32, device=dev)
    grads = None
    if return_grads:
        out["grads"] = {k: [torch.empty_like(w) for w in getattr(policy, k)] for k in ONLINE_NAMES}
        grads = _lib.pointers([g for k in ONLINE_NAMES for g in out["grads"][k]])
    nets = QstdNets(C.sizeof(QstdNets), 0, _lib.pointers([w for ws in policy.nets() for w in ws]),
                    _lib.pointers([t for k in ONLINE_NAMES for t in policy.m[k]]), _lib.pointers([t for k in ONLINE_NAMES for t in policy.v[k]]))
    rp = QstdReplay(C.sizeof(QstdReplay), 0, n, *map(_lib.as_arg, data))
    hp = QstdHyper(C.sizeof(QstdHyper), policy_delay, gamma, tau, actor_lr, critic_lr, sigma, clip, beta1, beta2, eps)
    ws = policy.workspace()
    _lib.side_call("td3", load_td3(), "qstd_update", C.byref(nets), C.byref(rp), idx_d, cnt_d, steps, batch, C.byref(hp), t0, actor_t0,
                   noise, int(seed), out["noise"], ws, int(ws.numel()), out["stats"], grads, device=dev)
    if return_grads and (t0 + steps - 1) % policy_delay != 0:
        out["grads"] = dict(out["grads"], actor=None)                           # (dropped after the call: it checked them for overlap)
    policy.steps += steps
    policy.actor_steps += actor_steps(t0, steps, policy_delay)
    policy.updated()
    return out


def torch_td3_update(policy, replay, indices, counts=None, gamma=0.99, tau=5.0e-3, actor_lr=3.0e-4, critic_lr=3.0e-4, policy_delay=2,
                     target_policy_noise=0.2, target_noise_clip=0.5, noise=None, seed=0, return_grads=False, return_noise=False):
    """td3_update as a plain torch autograd loop on whatever device and in whatever dtype the policy is: the same losses, the same
    noise (the caller's, or keyed_noise), the selects of the header (torch.where: a NaN stays), tf.train.AdamOptimizer's formula, the
    same state.  Same result dict; the bits differ (library GEMMs, float64 Box-Muller)."""
    import torch
    hyper = dict(gamma=gamma, tau=tau, actor_lr=actor_lr, critic_lr=critic_lr, policy_delay=policy_delay,
                 target_policy_noise=target_policy_noise, target_noise_clip=target_noise_clip)
    data, indices, counts, args = _update_args(policy, replay, indices, counts, hyper, noise, False)
    n, steps, batch, gamma, tau, actor_lr, critic_lr, policy_delay, sigma, clip, beta1, beta2, eps, t0, actor_t0 = args
    dev, dt = policy.device, policy.dtype
    gamma, sigma, clip = (float(np.float32(x)) for x in (gamma, sigma, clip))           # the header's G, SIGMA and CL
    obs0, act, rew, obs1, done = (t.to(dt) for t in data)
    if noise is None:
        noise = torch.as_tensor(keyed_noise(seed, t0, steps, batch)).to(dev)
    z_all = noise.to(dt)
    out = {"stats": torch.zeros((steps, len(TD3_STAT_NAMES)), dtype=dt, device=dev), "grads": None, "noise": noise if return_noise else None}

    def actor(w, o):
        h = torch.relu(torch.addmm(w[1], o, w[0]))
        return torch.tanh(torch.addmm(w[5], torch.relu(torch.addmm(w[3], h, w[2])), w[4]))

    def critic(w, o, a):
        h = torch.relu(torch.addmm(w[1], torch.cat([o, a], 1), w[0]))
        return torch.addmm(w[5], torch.relu(torch.addmm(w[3], h, w[2])), w[4])[:, 0]

    def clampsel(v, lo, hi):
        return torch.where(v < lo, torch.full_like(v, lo), torch.where(v > hi, torch.full_like(v, hi), v))

    for s in range(steps):
        u = policy.steps
        c = batch if counts is None else int(counts[s])
        rows = indices[s, :c].long().to(dev)
        o0, o1 = obs0[rows], obs1[rows]
        Q = {k: [w.detach().requires_grad_(True) for w in getattr(policy, k)] for k in ("q1", "q2")}
        with torch.no_grad():
            e = clampsel(sigma * z_all[s, :c], -clip, clip)
            a1 = clampsel(actor(policy.actor_target, o1) + e, -1.0, 1.0)
            qa, qb = critic(policy.q1_target, o1, a1), critic(policy.q2_target, o1, a1)
            m = torch.where(torch.isnan(qa), qa, torch.where(torch.isnan(qb), qb, torch.where(qb < qa, qb, qa)))
            d = done[rows]
            y = torch.where(d >= 1.0, rew[rows], rew[rows] + (1.0 - d) * gamma * m)
        q = {k: critic(Q[k], o0, act[rows]) for k in Q}
        loss = {k: ((q[k] - y) ** 2).mean() for k in Q}
        g = {k: torch.autograd.grad(loss[k], Q[k]) for k in Q}
        todo = [("q1", g["q1"], critic_lr, u + 1, False), ("q2", g["q2"], critic_lr, u + 1, False)]
        actor_loss = torch.zeros((), dtype=dt, device=dev)
        if u % policy_delay == 0:
            A = [w.detach().requires_grad_(True) for w in policy.actor]
            actor_loss = -critic([w.detach() for w in policy.q1], o0, actor(A, o0)).mean()
            g["actor"] = torch.autograd.grad(actor_loss, A)
            todo = [("actor", g["actor"], actor_lr, policy.actor_steps + 1, True), ("q1", g["q1"], critic_lr, u + 1, True),
                    ("q2", g["q2"], critic_lr, u + 1, True)]
        out["stats"][s] = torch.stack([loss["q1"].detach(), loss["q2"].detach(), q["q1"].detach().mean(), q["q2"].detach().mean(), y.mean(),
                                       actor_loss.detach()])
        with torch.no_grad():
            for name, grads, lr, t, polyak in todo:
                corr = math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
                for w, gw, mm, vv, tw in zip(getattr(policy, name), grads, policy.m[name], policy.v[name], getattr(policy, name + "_target")):
                    mm.mul_(beta1).add_(gw, alpha=1.0 - beta1)
                    vv.mul_(beta2).addcmul_(gw, gw, value=1.0 - beta2)
                    w.sub_(lr * corr * mm / (vv.sqrt() + eps))
                    if polyak:
                        tw.mul_(1.0 - tau).add_(w, alpha=tau)
        policy.steps += 1
        policy.actor_steps += int(u % policy_delay == 0)
        if return_grads:
            out["grads"] = {k: (list(g[k]) if k in g else None) for k in ONLINE_NAMES}
    policy.updated()
    return out


# ---------------------------------------------------------------------------------------------------- the loop
class TD3:
    """``TD3(policy, env, ...).learn(total_timesteps)``: SB2's TD3 loop on N device envs, with SB2's defaults.  Per env step: before
    `learning_starts` transitions a uniform action, after them the tanh actor plus `action_noise()` (a NormalActionNoise, an OUNoise
    or None) clipped to [-1, 1]; ``env.step``; ``replay.add`` of the N transitions (ddpg.py's collection loop).  After every
    `train_freq` calls of ``env.step``, once `learning_starts` transitions are in, ONE update call of `gradient_steps` updates of
    `batch_size` rows drawn uniformly from the replay.  ``total_timesteps`` counts transitions: N per step.  `update`: "hip"
    (td3_update) or "torch" (torch_td3_update); either draws its target noise from `seed` and the update index."""

    def __init__(self, policy, env, *, gamma=0.99, learning_rate=3.0e-4, buffer_size=50000, learning_starts=100, train_freq=100,
                 gradient_steps=100, batch_size=128, tau=5.0e-3, policy_delay=2, action_noise=None, target_policy_noise=0.2,
                 target_noise_clip=0.5, update="hip", seed=0, replay=None):
        import torch
        if update not in ("hip", "torch"):
            raise ValueError("update must be 'hip' or 'torch', got %r" % (update,))
        self.policy, self.env, self.update, self.seed = policy, env, update, int(seed)
        self.train_freq, self.gradient_steps, self.batch_size, self.learning_starts = int(train_freq), int(gradient_steps), int(batch_size), \
            int(learning_starts)
        if self.train_freq < 1:
            raise ValueError("train_freq must be >= 1, got %d" % self.train_freq)
        if self.learning_starts < 0:
            raise ValueError("learning_starts must be >= 0, got %d" % self.learning_starts)
        self.hyper = dict(gamma=gamma, tau=tau, actor_lr=learning_rate, critic_lr=learning_rate, policy_delay=policy_delay,
                          target_policy_noise=target_policy_noise, target_noise_clip=target_noise_clip)
        check_td3_args(int(buffer_size), self.gradient_steps, self.batch_size, **self.hyper)
        self.action_noise = action_noise
        self.replay = replay if replay is not None else ReplayBuffer(buffer_size, env.device)
        self.generator = torch.Generator().manual_seed(self.seed)                       # the replay schedule, on the host
        self.explore = torch.Generator(device=env.device).manual_seed(self.seed + 1)    # the uniform actions, on the env's device
        self.num_timesteps, self.obs = 0, None

    def act(self, obs):
        """the behaviour action of every env for `obs`"""
        import torch
        with torch.no_grad():
            if self.num_timesteps < self.learning_starts:
                a = torch.rand((obs.shape[0], 4), generator=self.explore, device=obs.device) * 2.0 - 1.0
            else:
                a = self.policy.predict(obs).to(torch.float32)
                if self.action_noise is not None:
                    a = a + self.action_noise()
                a = a.clamp(-1.0, 1.0)
        return a.contiguous()

    def learn(self, total_timesteps, log_interval=1):
        """-> a list of one dict per logged cycle: the cycle, `total_timesteps` so far, the six statistics (TD3_STAT_NAMES, the mean
        over the cycle's updates), the mean reward of the cycle's env steps and `fps`"""
        fn = td3_update if self.update == "hip" else torch_td3_update

        def train():
            if self.num_timesteps < self.learning_starts:
                return None
            indices = replay_schedule(self.replay.size, self.gradient_steps, self.batch_size, self.generator)
            return fn(self.policy, self.replay, indices, seed=self.seed, **self.hyper)["stats"]
        return collect_and_train(self, total_timesteps, log_interval, self.train_freq, train, TD3_STAT_NAMES)
