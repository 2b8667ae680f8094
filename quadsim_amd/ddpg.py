"""DDPG on the device (the last trainer script of the reference: run_docking_ddpg.py).

The script alternates ``nb_rollout_steps = 1500`` env steps with ``nb_train_steps = 100`` updates of ``batch_size = 10``.  One update
is four forward passes, two backward passes, two Adam steps and a Polyak average over about 37 500 parameters: ``ddpg_update`` runs
every update of a cycle through ``qsdd_update`` of libquadsim_ddpg.so (include/quadsim_ddpg.h is the numerical contract), one launch
of two workgroups per update.  ``torch_ddpg_update`` is the same update as a plain autograd loop, the comparison.  Collection stays
a per-step loop over ``env.step``: it is not where DDPG spends its time.

The nets are SB2's ``CustomDDPGPolicy`` with ``layers = [128, 128]``, no layer norm, ReLU: the actor 12 -> 128 -> 128 -> 4 with tanh
(the six tensors of ``MlpPolicy``), the critic 12 -> 128, [128 + 4 actions] -> 128 -> 1, and a target copy of each.  Not built:
observation and return normalisation, critic_l2_reg, clip_norm, parameter noise, reward_scale != 1.  Nothing is drawn on the device.
"""
import ctypes as C
import functools
import math
import time

from . import _lib, offpolicy
from .offpolicy import NET_KEYS

DDPG_MAX_BATCH, DDPG_MAX_STEPS = 256, 4096
DDPG_BETA1, DDPG_BETA2, DDPG_EPS = 0.9, 0.999, 1.0e-8          # MpiAdam's defaults, which SB2's DDPG leaves alone
ACTOR_SHAPES = ((12, 128), (128,), (128, 128), (128,), (128, 4), (4,))
CRITIC_SHAPES = ((12, 128), (128,), (132, 128), (128,), (128, 1), (1,))
NET_NAMES = ("actor", "critic", "actor_target", "critic_target")
DDPG_STAT_NAMES = ("critic_loss", "actor_loss", "q_mean", "y_mean")

# libquadsim_ddpg.so is the entry "ddpg" of _lib.SIDE: its path, signatures, loader, status check and call helper are _lib's.
# The names below stay this module's so that callers and tests can replace the loader
QsddNets, QsddReplay, QsddHyper, DDPG_EXPORTS = _lib.QsddNets, _lib.QsddReplay, _lib.QsddHyper, _lib.SIDE["ddpg"]["exports"]
load_ddpg, check_ddpg = functools.partial(_lib.side_load, "ddpg"), functools.partial(_lib.side_check, "ddpg")


def check_ddpg_args(n, steps, batch, gamma=0.99, tau=1.0e-3, actor_lr=1.0e-4, critic_lr=1.0e-3, obs_clip=5.0, beta1=DDPG_BETA1,
                    beta2=DDPG_BETA2, eps=DDPG_EPS, t0=0, counts=None, indices=None):
    """-> (n, steps, batch, gamma, tau, actor_lr, critic_lr, obs_clip, beta1, beta2, eps, t0); ValueError for what qsdd_update would
    refuse and, given the host arrays `counts` [steps] and `indices` [steps,batch], for what it cannot check (a count outside
    [1, batch], a row it would read outside [0, n)), before anything touches the library or the GPU"""
    n, steps, batch, t0 = int(n), int(steps), int(batch), int(t0)
    offpolicy.check_extent(n, steps, batch, DDPG_MAX_BATCH, DDPG_MAX_STEPS)
    gamma, tau, actor_lr, critic_lr, obs_clip = float(gamma), float(tau), float(actor_lr), float(critic_lr), float(obs_clip)
    offpolicy.check_discount(gamma, tau)
    if not obs_clip > 0.0:
        raise ValueError("obs_clip must be > 0 (inf: no clamp), got %r" % obs_clip)
    for name, val in (("actor_lr", actor_lr), ("critic_lr", critic_lr)):
        if not math.isfinite(val):
            raise ValueError("%s must be finite, got %r" % (name, val))
    _, beta1, beta2, eps = _lib.check_adam_args(0.0, beta1, beta2, eps, t0, steps, "steps")
    offpolicy.check_schedule(n, steps, batch, counts, indices)
    return n, steps, batch, gamma, tau, actor_lr, critic_lr, obs_clip, beta1, beta2, eps, t0


def shapes_of(name):
    return ACTOR_SHAPES if name.startswith("actor") else CRITIC_SHAPES


# ---------------------------------------------------------------------------------------------------- the nets
class DDPGPolicy(offpolicy.Nets):
    """the four nets of DDPG, float32 in the policy's (in, out) layout, as lists of six tensors: ``actor``, ``critic``,
    ``actor_target``, ``critic_target``; Adam's moments of the two online nets (``m``, ``v``: {"actor": [...], "critic": [...]}) and
    the step count.  SB2's initialisation drawn from `seed`: Glorot-uniform hidden layers, U(-3e-3, 3e-3) output layers, zero
    biases, the targets equal to the online nets.  `weights`: {"actor": {w0 ..}, "critic": {..}, and optionally the two targets}."""

    NET_NAMES, ONLINE_NAMES, OUT_LIM, TAKES_DTYPE, LIB = NET_NAMES, ("actor", "critic"), 3.0e-3, False, ("ddpg", "qsdd_workspace_bytes")
    shapes_of, load = staticmethod(shapes_of), staticmethod(lambda: load_ddpg())

    def __init__(self, seed=0, device="cuda", weights=None):
        self.init_nets(seed, device, weights, "float32")
        self.reset_optimizer()

    def reset_optimizer(self):
        """forget Adam's moments and the step count"""
        self.zero_moments()
        self.steps = 0

    def predict(self, obs, obs_clip=5.0):
        """obs [N,12] float32 -> tanh actions [N,4] of the online actor (plain torch)"""
        import torch
        w = self.actor
        h = torch.relu(torch.addmm(w[1], obs.clamp(-obs_clip, obs_clip), w[0]))
        h = torch.relu(torch.addmm(w[3], h, w[2]))
        return torch.tanh(torch.addmm(w[5], h, w[4]))

    def actor_weights(self):
        """the online actor in MlpPolicy's key names (numpy): MlpPolicy clips where this actor squashes"""
        return {k: w.detach().cpu().numpy() for k, w in zip(NET_KEYS, self.actor)}


class ReplayBuffer:
    """a ring of `capacity` transitions in device tensors: obs0 [cap,12], act [cap,4], rew [cap], obs1 [cap,12], done [cap] (0 / 1
    float32).  ``add`` takes a batch of N transitions, writes them at the ring's position in order and wraps; ``size`` is the
    number of valid rows, ``pos`` the next row to write."""

    def __init__(self, capacity, device="cuda"):
        import torch
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("capacity must be >= 1, got %d" % self.capacity)
        self.device = torch.device(device)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)       # noqa: E731
        self.obs0, self.act, self.rew, self.obs1, self.done = z(self.capacity, 12), z(self.capacity, 4), z(self.capacity), z(self.capacity, 12), \
            z(self.capacity)
        self.device = self.obs0.device
        self.pos, self.size = 0, 0

    def tensors(self):
        return self.obs0, self.act, self.rew, self.obs1, self.done

    def add(self, obs0, act, rew, obs1, done):
        import torch
        n = int(obs0.shape[0])
        if n > self.capacity:
            raise ValueError("a batch of %d transitions does not fit a ring of %d" % (n, self.capacity))
        rows = (torch.arange(n, device=self.device) + self.pos) % self.capacity
        for dst, src in zip(self.tensors(), (obs0, act, rew, obs1, done)):
            dst[rows] = torch.as_tensor(src, device=self.device).to(torch.float32).reshape((n,) + tuple(dst.shape[1:]))
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.size + n, self.capacity)


def replay_schedule(size, steps, batch, generator):
    """-> indices [steps, batch] int32, CPU: uniform over 0 .. size-1 with replacement (SB2's ReplayBuffer.sample), drawn from
    `generator` (a CPU torch.Generator) in one draw; nothing is drawn on the device"""
    import torch
    size, steps, batch = int(size), int(steps), int(batch)
    if size < 1 or steps < 1 or batch < 1:
        raise ValueError("size, steps and batch must be >= 1")
    return torch.randint(0, size, (steps, batch), generator=generator, dtype=torch.int32)


class OUNoise:
    """SB2's OrnsteinUhlenbeckActionNoise with mean 0, one state [4] per env on the device:
    x <- x + theta (0 - x) dt + sigma sqrt(dt) N(0, 1); ``reset(done)`` zeroes the state of the envs where `done`."""

    def __init__(self, n_envs, sigma=0.5, theta=0.15, dt=1.0e-2, device="cuda", seed=0):
        import torch
        self.sigma, self.theta, self.dt = float(sigma), float(theta), float(dt)
        self.device = torch.device(device)
        self.x = torch.zeros((int(n_envs), 4), dtype=torch.float32, device=self.device)
        self.generator = torch.Generator(device=self.device).manual_seed(int(seed))

    def __call__(self):
        import torch
        n = torch.randn(self.x.shape, generator=self.generator, device=self.x.device, dtype=torch.float32)
        self.x = self.x + self.theta * (0.0 - self.x) * self.dt + self.sigma * math.sqrt(self.dt) * n
        return self.x

    def reset(self, done=None):
        if done is None:
            self.x = self.x * 0.0
        else:
            self.x = self.x * (~done.to(self.x.device).bool()).to(self.x.dtype)[:, None]


# ---------------------------------------------------------------------------------------------------- the update
def _update_args(policy, replay, indices, counts, gamma, tau, actor_lr, critic_lr, obs_clip, need_device):
    dev = policy.device
    if need_device and dev.type != "cuda":
        raise _lib.QuadsimError("ddpg_update needs the policy on a HIP device, it is on %s; torch_ddpg_update is the host path" % (dev,))
    data, n, indices, counts = offpolicy.update_tensors(policy, replay, indices, counts, "float32")
    args = check_ddpg_args(n, indices.shape[0], indices.shape[1], gamma, tau, actor_lr, critic_lr, obs_clip, t0=policy.steps,
                           counts=None if counts is None else counts.numpy(), indices=indices.numpy())
    return data, indices.contiguous(), counts, args


def ddpg_update(policy, replay, indices, counts=None, gamma=0.99, tau=1.0e-3, actor_lr=1.0e-4, critic_lr=1.0e-3, obs_clip=5.0,
                return_grads=False):
    """ONE call of qsdd_update: indices.shape[0] DDPG updates of the policy's four nets.  replay: a ReplayBuffer or the five device
    tensors (obs0 [n,12], act [n,4], rew [n], obs1 [n,12], done [n]); indices [steps,batch] int32 and counts [steps] int32 (or None):
    HOST tensors, checked here (check_ddpg_args) and uploaded.  The 24 weights, the 24 moments and the step count are updated in
    place.  -> {"stats": [steps, 4] device tensor (DDPG_STAT_NAMES, from the weights before each step), "grads": {"actor": six,
    "critic": six} device tensors of the last step on request}.  Launched on torch's current stream; nothing waits for the device."""
    import torch
    data, indices, counts, (n, steps, batch, gamma, tau, actor_lr, critic_lr, obs_clip, beta1, beta2, eps, t0) = _update_args(
        policy, replay, indices, counts, gamma, tau, actor_lr, critic_lr, obs_clip, True)
    dev = policy.device
    idx_d = indices.to(dev)
    cnt_d = None if counts is None else counts.contiguous().to(dev)
    out = {"stats": _lib.new_tensor(dev, (steps, len(DDPG_STAT_NAMES)), "float32"), "grads": None}
    grads = None
    if return_grads:
        out["grads"] = {k: [torch.empty_like(w) for w in getattr(policy, k)] for k in ("actor", "critic")}
        grads = _lib.pointers(out["grads"]["actor"] + out["grads"]["critic"])
    nets = QsddNets(C.sizeof(QsddNets), 0, _lib.pointers([w for ws in policy.nets() for w in ws]),
                    _lib.pointers(policy.m["actor"] + policy.m["critic"]), _lib.pointers(policy.v["actor"] + policy.v["critic"]))
    rp = QsddReplay(C.sizeof(QsddReplay), 0, n, *map(_lib.as_arg, data))
    hp = QsddHyper(C.sizeof(QsddHyper), 0, gamma, tau, actor_lr, critic_lr, obs_clip, beta1, beta2, eps)
    ws = policy.workspace()
    _lib.side_call("ddpg", load_ddpg(), "qsdd_update", C.byref(nets), C.byref(rp), idx_d, cnt_d, steps, batch, C.byref(hp), t0, ws,
                   int(ws.numel()), out["stats"], grads, device=dev)
    policy.steps += steps
    return out


def torch_ddpg_update(policy, replay, indices, counts=None, gamma=0.99, tau=1.0e-3, actor_lr=1.0e-4, critic_lr=1.0e-3, obs_clip=5.0,
                      return_grads=False):
    """ddpg_update as a plain torch autograd loop on whatever device the policy is on: the same losses, MpiAdam's formula (not
    torch.optim.Adam's, whose epsilon sits elsewhere), the same state.  Same result dict; the bits differ (library GEMMs)."""
    import torch
    data, indices, counts, (n, steps, batch, gamma, tau, actor_lr, critic_lr, obs_clip, beta1, beta2, eps, t0) = _update_args(
        policy, replay, indices, counts, gamma, tau, actor_lr, critic_lr, obs_clip, False)
    dev = policy.device
    obs0, act, rew, obs1, done = data
    out = {"stats": _lib.new_tensor(dev, (steps, len(DDPG_STAT_NAMES)), "float32"), "grads": None}

    def actor(w, o):
        h = torch.relu(torch.addmm(w[1], o, w[0]))
        return torch.tanh(torch.addmm(w[5], torch.relu(torch.addmm(w[3], h, w[2])), w[4]))

    def critic(w, o, a):
        h = torch.relu(torch.addmm(w[1], o, w[0]))
        return torch.addmm(w[5], torch.relu(torch.addmm(w[3], torch.cat([h, a], 1), w[2])), w[4])[:, 0]

    for s in range(steps):
        c = batch if counts is None else int(counts[s])
        rows = indices[s, :c].long().to(dev)
        o0, o1 = obs0[rows].clamp(-obs_clip, obs_clip), obs1[rows].clamp(-obs_clip, obs_clip)
        A = [w.detach().requires_grad_(True) for w in policy.actor]
        Cr = [w.detach().requires_grad_(True) for w in policy.critic]
        with torch.no_grad():
            q1 = critic(policy.critic_target, o1, actor(policy.actor_target, o1))
            d = done[rows]
            y = torch.where(d >= 1.0, rew[rows], rew[rows] + (1.0 - d) * gamma * q1)
        q = critic(Cr, o0, act[rows])
        critic_loss = ((q - y) ** 2).mean()
        g_critic = torch.autograd.grad(critic_loss, Cr)
        actor_loss = -critic([w.detach() for w in policy.critic], o0, actor(A, o0)).mean()
        g_actor = torch.autograd.grad(actor_loss, A)
        out["stats"][s] = torch.stack([critic_loss.detach(), actor_loss.detach(), q.detach().mean(), y.mean()])
        t = policy.steps + 1
        corr = math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        with torch.no_grad():
            for name, grads, lr in (("actor", g_actor, actor_lr), ("critic", g_critic, critic_lr)):
                for w, g, mm, vv, tw in zip(getattr(policy, name), grads, policy.m[name], policy.v[name], getattr(policy, name + "_target")):
                    mm.mul_(beta1).add_(g, alpha=1.0 - beta1)
                    vv.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
                    w.sub_(lr * corr * mm / (vv.sqrt() + eps))
                    tw.mul_(1.0 - tau).add_(w, alpha=tau)
        policy.steps += 1
        if return_grads:
            out["grads"] = {"actor": list(g_actor), "critic": list(g_critic)}
    return out


# ---------------------------------------------------------------------------------------------------- the loop
class DDPG:
    """``DDPG(policy, env, ...).learn(total_timesteps)``: SB2's DDPG loop on N device envs.  Per env step: act with the tanh actor,
    add `action_noise()` (an OUNoise or None), clip to [-1, 1], with probability `random_exploration` per env take a uniform action
    instead, ``env.step``, ``replay.add`` of the N transitions.  After every `nb_rollout_steps` calls of ``env.step`` (the
    reference's count, on its one env) ONE update call of `nb_train_steps` updates of `batch_size` rows drawn uniformly from the
    replay.  ``total_timesteps`` counts transitions: N per step.  `update`:
    "hip" (ddpg_update) or "torch" (torch_ddpg_update).  Collection uses the env's own step kernel: there is no fused collector."""

    def __init__(self, policy, env, *, gamma=0.99, tau=1.0e-3, actor_lr=1.0e-4, critic_lr=1.0e-3, obs_clip=5.0, nb_rollout_steps=1500,
                 nb_train_steps=100, batch_size=10, buffer_size=50000, random_exploration=0.3, action_noise=None, update="hip", seed=0,
                 replay=None):
        import torch
        if update not in ("hip", "torch"):
            raise ValueError("update must be 'hip' or 'torch', got %r" % (update,))
        if not 0.0 <= float(random_exploration) <= 1.0:
            raise ValueError("random_exploration must be in [0, 1], got %r" % (random_exploration,))
        self.policy, self.env, self.update = policy, env, update
        self.nb_rollout_steps, self.nb_train_steps, self.batch_size = int(nb_rollout_steps), int(nb_train_steps), int(batch_size)
        if self.nb_rollout_steps < 1:
            raise ValueError("nb_rollout_steps must be >= 1, got %d" % self.nb_rollout_steps)
        self.hyper = dict(gamma=gamma, tau=tau, actor_lr=actor_lr, critic_lr=critic_lr, obs_clip=obs_clip)
        check_ddpg_args(int(buffer_size), self.nb_train_steps, self.batch_size, **self.hyper)
        self.random_exploration, self.action_noise = float(random_exploration), action_noise
        self.replay = replay if replay is not None else ReplayBuffer(buffer_size, env.device)
        self.generator = torch.Generator().manual_seed(int(seed))                       # the replay schedule, on the host
        self.explore = torch.Generator(device=env.device).manual_seed(int(seed) + 1)    # the uniform actions, on the env's device
        self.num_timesteps, self.obs = 0, None

    def act(self, obs):
        """the behaviour action of every env for `obs`"""
        import torch
        with torch.no_grad():
            a = self.policy.predict(obs, self.hyper["obs_clip"])
            if self.action_noise is not None:
                a = a + self.action_noise()
            a = a.clamp(-1.0, 1.0)
            if self.random_exploration > 0.0:
                n = a.shape[0]
                take = torch.rand((n,), generator=self.explore, device=a.device) < self.random_exploration
                uniform = torch.rand((n, 4), generator=self.explore, device=a.device) * 2.0 - 1.0
                a = torch.where(take[:, None], uniform, a)
        return a.contiguous()

    def learn(self, total_timesteps, log_interval=1):
        """-> a list of one dict per logged cycle: the cycle, `total_timesteps` so far, the four statistics (DDPG_STAT_NAMES, the
        mean over the cycle's updates), the mean reward of the cycle's env steps and `fps`"""
        fn = ddpg_update if self.update == "hip" else torch_ddpg_update

        def train():
            indices = replay_schedule(self.replay.size, self.nb_train_steps, self.batch_size, self.generator)
            return fn(self.policy, self.replay, indices, **self.hyper)["stats"]
        return collect_and_train(self, total_timesteps, log_interval, self.nb_rollout_steps, train, DDPG_STAT_NAMES)


def collect_and_train(agent, total_timesteps, log_interval, rollout_steps, train, stat_names):
    """the per-step collection loop of the off-policy trainers (DDPG here, TD3 in td3.py).  `agent` has env, replay, action_noise,
    obs, num_timesteps and act(obs).  Per env step: ``agent.act``, ``env.step``, ``replay.add`` of the N transitions, the noise
    reset where done.  After every `rollout_steps` calls of ``env.step`` one call of `train()` -> the cycle's statistics [updates,
    len(stat_names)] (None: nothing was trained, the cycle is not logged) -> the list of logged cycles"""
    env, n = agent.env, int(agent.env.num_envs)
    if agent.obs is None:
        agent.obs = env.reset().clone()
    logs, cycle, since, rew_sum, rew_n, t_start = [], 0, 0, None, 0, time.time()
    target = agent.num_timesteps + int(total_timesteps)
    while agent.num_timesteps < target:
        a = agent.act(agent.obs)
        obs1, rew, done, _ = env.step(a)
        agent.replay.add(agent.obs, a, rew, obs1, done)
        if agent.action_noise is not None:
            agent.action_noise.reset(done)
        agent.obs = obs1.clone()
        agent.num_timesteps += n
        since += 1
        rew_sum = rew.double().sum() if rew_sum is None else rew_sum + rew.double().sum()
        rew_n += n
        if since >= rollout_steps:
            cycle += 1
            stats = train()
            if stats is not None and log_interval and (cycle % log_interval == 0 or cycle == 1):
                t_now = time.time()
                log = {"cycle": cycle, "total_timesteps": agent.num_timesteps, "reward_mean": float(rew_sum) / rew_n,
                       "fps": int(since * n / max(t_now - t_start, 1e-9))}
                log.update(zip(stat_names, stats.double().mean(0).tolist()))
                logs.append(log)
            since, rew_sum, rew_n, t_start = 0, None, 0, time.time()
    return logs
