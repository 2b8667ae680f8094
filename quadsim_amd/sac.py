"""Soft Actor-Critic on the device: a sampled tanh-Gaussian actor, twin critics, a value net with a Polyak target and a learned
temperature (SB2's ``stable_baselines.sac``, the form with the value net).

One update is two sampled forward passes of the actor, eight more forward passes, four backward passes, four Adam steps, the
temperature's own Adam step and a Polyak average: ``sac_update`` runs every update of a call through ``qss_update`` of
libquadsim_sac.so (include/quadsim_sac.h is the numerical contract), ONE launch of four workgroups (q1, q2, value, actor) per update.
``torch_sac_update`` is the same update as a plain autograd loop, the comparison.  Collection is ddpg.py's per-step loop.

The nets are SB2's SAC ``MlpPolicy`` with ``layers = [128, 128]``, no layer norm, ReLU: the actor 12 -> 128 -> 128 -> 8 (four means, four
raw log standard deviations clamped to [-20, 2]), two critics [12 obs + 4 actions] -> 128 -> 128 -> 1, the value net 12 -> 128 -> 128 -> 1
and its target.  The sample's noise is the caller's, or keyed Philox draws that depend on (seed, update index, row slot) alone.
Not built: SAC without the value net, layer norm, prioritised replay, observation and return normalisation.
"""
import ctypes as C
import functools
import math

import numpy as np

from . import _lib, offpolicy
from .ddpg import NET_KEYS, ReplayBuffer, collect_and_train, replay_schedule  # noqa: F401  (the pieces SAC shares with DDPG)

SAC_MAX_BATCH, SAC_MAX_STEPS = 256, 4096
SAC_BETA1, SAC_BETA2, SAC_EPS = 0.9, 0.999, 1.0e-8             # tf.train.AdamOptimizer's defaults, which SB2's SAC leaves alone
SAC_NOISE_STREAM = 7                                           # the Philox stream of the sample's noise (include/quadsim_sac.h)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
SAC_E6 = float(np.float32(1.0e-6))                             # the header's E6, the float32 constant taken exactly
ACTOR_SHAPES = ((12, 128), (128,), (128, 128), (128,), (128, 8), (8,))
CRITIC_SHAPES = ((16, 128), (128,), (128, 128), (128,), (128, 1), (1,))
VALUE_SHAPES = ((12, 128), (128,), (128, 128), (128,), (128, 1), (1,))
ONLINE_NAMES = ("actor", "q1", "q2", "v")
NET_NAMES = ONLINE_NAMES + ("v_target",)
SAC_STAT_NAMES = ("q1_loss", "q2_loss", "value_loss", "actor_loss", "alpha_loss", "alpha", "logp_mean", "y_mean")
SAC_FWD_NAMES = ("v_target", "y", "qa", "qb", "vb")

# libquadsim_sac.so is the entry "sac" of _lib.SIDE: its path, signatures, loader, status check and call helper are _lib's.
# The names below stay this module's so that callers and tests can replace the loader
QssNets, QssReplay, QssHyper, QssTrace, SAC_EXPORTS = _lib.QssNets, _lib.QssReplay, _lib.QssHyper, _lib.QssTrace, _lib.SIDE["sac"]["exports"]
load_sac, check_sac = functools.partial(_lib.side_load, "sac"), functools.partial(_lib.side_check, "sac")


def shapes_of(name):
    return ACTOR_SHAPES if name == "actor" else CRITIC_SHAPES if name.startswith("q") else VALUE_SHAPES


def check_sac_args(n, steps, batch, gamma=0.99, tau=5.0e-3, lr=3.0e-4, target_entropy=-4.0, auto_alpha=True, beta1=SAC_BETA1, beta2=SAC_BETA2,
                   eps=SAC_EPS, t0=0, counts=None, indices=None):
    """-> (n, steps, batch, gamma, tau, lr, target_entropy, auto_alpha, beta1, beta2, eps, t0); ValueError for what qss_update would
    refuse and, given the host arrays `counts` [steps] and `indices` [steps,batch], for what it cannot check (a count outside
    [1, batch], a row it would read outside [0, n)), before anything touches the library or the GPU"""
    n, steps, batch, t0 = int(n), int(steps), int(batch), int(t0)
    offpolicy.check_extent(n, steps, batch, SAC_MAX_BATCH, SAC_MAX_STEPS)
    gamma, tau, target_entropy = float(gamma), float(tau), float(target_entropy)
    offpolicy.check_discount(gamma, tau)
    if not math.isfinite(target_entropy):
        raise ValueError("target_entropy must be finite, got %r" % target_entropy)
    if auto_alpha not in (0, 1, False, True):
        raise ValueError("auto_alpha must be 0 or 1, got %r" % (auto_alpha,))
    lr, beta1, beta2, eps = _lib.check_adam_args(lr, beta1, beta2, eps, t0, steps, "steps")
    offpolicy.check_schedule(n, steps, batch, counts, indices)
    return n, steps, batch, gamma, tau, lr, target_entropy, int(bool(auto_alpha)), beta1, beta2, eps, t0


def keyed_noise(seed, t0, steps, batch):
    """-> [steps, batch, 4] float32: the noise that a call without `noise` draws, restated on the host: offpolicy.keyed_noise on Philox
    stream 7 (the device's own arithmetic is float32: ``noise_out`` of sac_update has the device's values)"""
    return offpolicy.keyed_noise(seed, t0, steps, batch, SAC_NOISE_STREAM)


# ---------------------------------------------------------------------------------------------------- the nets
class SACPolicy(offpolicy.Nets):
    """the five nets of SAC in the policy's (in, out) layout, as lists of six tensors: ``actor`` (head eight wide: four means, four raw
    log standard deviations), ``q1``, ``q2``, ``v`` and ``v_target``; Adam's moments of the four online nets (``m``, ``v_``: {"actor":
    [...], ..}), ``alpha_state`` = [log_alpha, m, v] and the update count ``steps``.  SB2's initialisation drawn from `seed`:
    Glorot-uniform weights, zero biases, the target equal to the value net, log_alpha = log(`ent_coef`) (1.0: SB2's "auto").
    `weights`: {"actor": {w0 ..}, "q1": {..}, "q2": {..}, "v": {..} and optionally "v_target"}.  `dtype`: "float32" (the device path
    needs it) or "float64" (torch_sac_update alone)."""

    NET_NAMES, ONLINE_NAMES, V, LIB = NET_NAMES, ONLINE_NAMES, "v_", ("sac", "qss_workspace_bytes")
    shapes_of, load = staticmethod(shapes_of), staticmethod(lambda: load_sac())

    def __init__(self, seed=0, device="cuda", weights=None, dtype="float32", ent_coef=1.0):
        import torch
        self.init_nets(seed, device, weights, dtype)
        self.alpha_state = torch.zeros(3, dtype=self.dtype, device=self.device)
        self.alpha_state[0] = math.log(float(ent_coef))
        self.reset_optimizer()

    def reset_optimizer(self):
        """forget Adam's moments (the temperature's too) and the step count; log_alpha stays"""
        self.zero_moments()
        self.alpha_state[1:] = 0.0
        self.steps = 0

    @property
    def alpha(self):
        return float(self.alpha_state[0].exp())

    def head(self, obs):
        """obs [N,12] -> (mu [N,4], log_std [N,4] clamped to [-20, 2]) of the online actor (plain torch)"""
        import torch
        w = self.actor
        h = torch.relu(torch.addmm(w[1], obs.to(self.dtype), w[0]))
        h = torch.relu(torch.addmm(w[3], h, w[2]))
        out = torch.addmm(w[5], h, w[4])
        return out[:, :4], out[:, 4:].clamp(LOG_STD_MIN, LOG_STD_MAX)

    def predict(self, obs, deterministic=True, generator=None):
        """obs [N,12] -> actions [N,4]: tanh(mu), or a sample where not `deterministic`"""
        import torch
        if not deterministic:
            return self.sample(obs, generator)
        return torch.tanh(self.head(obs)[0])

    def sample(self, obs, generator=None):
        """obs [N,12] -> tanh(mu + exp(log_std) z), z standard normals from `generator` (on the policy's device)"""
        import torch
        mu, ls = self.head(obs)
        z = torch.randn(mu.shape, generator=generator, device=mu.device, dtype=mu.dtype)
        return torch.tanh(mu + ls.exp() * z)

    def actor_as_mlp(self):
        """the mean head of the online actor in MlpPolicy's key names (numpy; cached until the next update), for the per-step
        evaluation of the deterministic action: MlpPolicy clips where this actor squashes"""
        if "actor" not in self._images:
            W = {k: w.detach().cpu().numpy().copy() for k, w in zip(NET_KEYS, self.actor)}
            W["w2"], W["b2"] = np.ascontiguousarray(W["w2"][:, :4]), np.ascontiguousarray(W["b2"][:4])
            self._images["actor"] = W
        return self._images["actor"]

    def npz_state(self):
        return {"steps": self.steps, "alpha_state": self.alpha_state.cpu().numpy()}

    def set_npz_state(self, z):
        import torch
        self.alpha_state = torch.as_tensor(z["alpha_state"].copy()).to(self.device)
        self.steps = int(z["steps"])


def reset_sac_optimizer(policy):
    """forget Adam's moments and the step count of a SACPolicy"""
    policy.reset_optimizer()


# ---------------------------------------------------------------------------------------------------- the update
def _update_args(policy, replay, indices, counts, hyper, noise, need_device):
    dev = policy.device
    dtype = str(policy.dtype).split(".")[-1]
    if need_device and (dev.type != "cuda" or dtype != "float32"):
        raise _lib.QuadsimError("sac_update needs a float32 policy on a HIP device, it is %s on %s; torch_sac_update is the host path"
                                % (dtype, dev))
    data, n, indices, counts = offpolicy.update_tensors(policy, replay, indices, counts, dtype)
    _lib.check_tensor("alpha_state", policy.alpha_state, dtype, (3,), dev)
    args = check_sac_args(n, indices.shape[0], indices.shape[1], t0=policy.steps, counts=None if counts is None else counts.numpy(),
                          indices=indices.numpy(), **hyper)
    if noise is not None:
        _lib.check_tensor("noise", noise, "float32", (args[1], args[2], 4), dev)
    return data, indices.contiguous(), counts, args


def sac_update(policy, replay, indices, counts=None, gamma=0.99, tau=5.0e-3, lr=3.0e-4, target_entropy=-4.0, auto_alpha=True, noise=None,
               seed=0, return_grads=False, return_noise=False, return_trace=False):
    """ONE call of qss_update: indices.shape[0] SAC updates of the policy's five nets and of its temperature.  replay: a ReplayBuffer
    or the five device tensors (obs0 [n,12], act [n,4], rew [n], obs1 [n,12], done [n]); indices [steps,batch] int32 and counts [steps]
    int32 (or None): HOST tensors, checked here (check_sac_args) and uploaded.  noise: [steps,batch,4] float32 standard normals on the
    device, or None: keyed Philox draws from `seed`, the update index and the row slot.  The 30 weights, the 48 moments, alpha_state and
    the step count are updated in place.  -> {"stats": [steps, 8] device tensor (SAC_STAT_NAMES, from the weights before each step),
    "grads": {"actor": six, "q1": six, "q2": six, "v": six} device tensors of the last step on request, "noise": the [steps,batch,4]
    normals that were used, on request, "trace": {"logp", "vlogp" [steps,batch], "act" [steps,batch,4], "fwd" [steps,batch,5]
    (SAC_FWD_NAMES)} on request}.  Launched on torch's current stream; nothing waits for the device."""
    import torch
    hyper = dict(gamma=gamma, tau=tau, lr=lr, target_entropy=target_entropy, auto_alpha=auto_alpha)
    data, indices, counts, args = _update_args(policy, replay, indices, counts, hyper, noise, True)
    n, steps, batch, gamma, tau, lr, target_entropy, auto_alpha, beta1, beta2, eps, t0 = args
    dev = policy.device
    idx_d = indices.to(dev)
    cnt_d = None if counts is None else counts.contiguous().to(dev)
    out = {"stats": _lib.new_tensor(dev, (steps, len(SAC_STAT_NAMES)), "float32"), "grads": None, "noise": None, "trace": None}
    if return_noise:
        out["noise"] = torch.zeros((steps, batch, 4), dtype=torch.float32, device=dev)
    grads = trace = None
    if return_grads:
        out["grads"] = {k: [torch.empty_like(w) for w in getattr(policy, k)] for k in ONLINE_NAMES}
        grads = _lib.pointers([g for k in ONLINE_NAMES for g in out["grads"][k]])
    if return_trace:
        out["trace"] = {k: torch.zeros((steps, batch) + tail, dtype=torch.float32, device=dev)
                        for k, tail in (("logp", ()), ("vlogp", ()), ("act", (4,)), ("fwd", (len(SAC_FWD_NAMES),)))}
        trace = C.byref(QssTrace(C.sizeof(QssTrace), 0, *[_lib.as_arg(out["trace"][k]) for k in ("logp", "vlogp", "act", "fwd")]))
    nets = QssNets(C.sizeof(QssNets), 0, _lib.pointers([w for ws in policy.nets() for w in ws]),
                   _lib.pointers([t for k in ONLINE_NAMES for t in policy.m[k]]), _lib.pointers([t for k in ONLINE_NAMES for t in policy.v_[k]]),
                   _lib.as_arg(policy.alpha_state))
    rp = QssReplay(C.sizeof(QssReplay), 0, n, *map(_lib.as_arg, data))
    hp = QssHyper(C.sizeof(QssHyper), auto_alpha, gamma, tau, lr, target_entropy, beta1, beta2, eps)
    ws = policy.workspace()
    _lib.side_call("sac", load_sac(), "qss_update", C.byref(nets), C.byref(rp), idx_d, cnt_d, steps, batch, C.byref(hp), t0, noise,
                   int(seed), out["noise"], ws, int(ws.numel()), out["stats"], trace, grads, device=dev)
    policy.steps += steps
    policy.updated()
    return out


def sac_math(which, x):
    """qss_math on a float32 device tensor: 0 exp, 1 ln, 2 ln(1 - tanh(x)^2 + 1e-6), the device functions of the log-probability"""
    import torch
    _lib.check_tensor("x", x, "float32", None, x.device)
    y = torch.empty_like(x)
    _lib.side_call("sac", load_sac(), "qss_math", int(which), x, y, int(x.numel()), device=x.device)
    return y


def torch_sac_update(policy, replay, indices, counts=None, gamma=0.99, tau=5.0e-3, lr=3.0e-4, target_entropy=-4.0, auto_alpha=True,
                     noise=None, seed=0, return_grads=False, return_noise=False, return_trace=False):
    """sac_update as a plain torch autograd loop on whatever device and in whatever dtype the policy is: the same losses, the same
    noise (the caller's, or keyed_noise), the selects of the header (torch.where: a NaN stays), tf.train.AdamOptimizer's formula, the
    same state.  Same result dict ("grads" gains "log_alpha"); the bits differ (library GEMMs, float64 Box-Muller)."""
    import torch
    hyper = dict(gamma=gamma, tau=tau, lr=lr, target_entropy=target_entropy, auto_alpha=auto_alpha)
    data, indices, counts, args = _update_args(policy, replay, indices, counts, hyper, noise, False)
    n, steps, batch, gamma, tau, lr, target_entropy, auto_alpha, beta1, beta2, eps, t0 = args
    dev, dt = policy.device, policy.dtype
    gamma, te = float(np.float32(gamma)), float(np.float32(target_entropy))          # the header's G and TE
    obs0, act, rew, obs1, done = (t.to(dt) for t in data)
    if noise is None:
        noise = torch.as_tensor(keyed_noise(seed, t0, steps, batch)).to(dev)
    z_all = noise.to(dt)
    out = {"stats": torch.zeros((steps, len(SAC_STAT_NAMES)), dtype=dt, device=dev), "grads": None, "noise": noise if return_noise else None,
           "trace": None}
    if return_trace:
        out["trace"] = {k: torch.zeros((steps, batch) + tail, dtype=dt, device=dev)
                        for k, tail in (("logp", ()), ("vlogp", ()), ("act", (4,)), ("fwd", (len(SAC_FWD_NAMES),)))}
    l2pi = float(np.float32(math.log(2.0 * math.pi)))

    def mlp(w, x):
        h = torch.relu(torch.addmm(w[1], x, w[0]))
        return torch.addmm(w[5], torch.relu(torch.addmm(w[3], h, w[2])), w[4])

    def clampsel(v, lo, hi):
        return torch.where(v < lo, torch.full_like(v, lo), torch.where(v > hi, torch.full_like(v, hi), v))

    def sample(w, o, z):
        head = mlp(w, o)
        mu, ls = head[:, :4], clampsel(head[:, 4:], LOG_STD_MIN, LOG_STD_MAX)
        sigma = ls.exp()
        a = torch.tanh(mu + sigma * z)
        t = sigma * z / (sigma + SAC_E6)
        logp = (-0.5 * (t * t + 2.0 * ls + l2pi) - torch.log(1.0 - a * a + SAC_E6)).sum(1)
        return a, logp

    def critic(w, o, a):
        return mlp(w, torch.cat([o, a], 1))[:, 0]

    for s in range(steps):
        u = policy.steps
        c = batch if counts is None else int(counts[s])
        rows = indices[s, :c].long().to(dev)
        o0, o1, z = obs0[rows], obs1[rows], z_all[s, :c]
        la = policy.alpha_state[0].detach().clone()
        alpha = la.exp()
        W = {k: [w.detach().requires_grad_(True) for w in getattr(policy, k)] for k in ONLINE_NAMES}
        frozen = {k: [w.detach() for w in getattr(policy, k)] for k in ONLINE_NAMES}
        with torch.no_grad():
            d = done[rows]
            vt = mlp(policy.v_target, o1)[:, 0]
            y = torch.where(d >= 1.0, rew[rows], rew[rows] + (1.0 - d) * gamma * vt)
            a_v, logp_v = sample(frozen["actor"], o0, z)
            qa, qb = critic(frozen["q1"], o0, a_v), critic(frozen["q2"], o0, a_v)
            mn = torch.where(torch.isnan(qa), qa, torch.where(torch.isnan(qb), qb, torch.where(qb < qa, qb, qa)))
            vb = mn - alpha * logp_v
        loss = {k: 0.5 * ((critic(W[k], o0, act[rows]) - y) ** 2).mean() for k in ("q1", "q2")}
        loss["v"] = 0.5 * ((mlp(W["v"], o0)[:, 0] - vb) ** 2).mean()
        a_pi, logp = sample(W["actor"], o0, z)
        loss["actor"] = (alpha * logp - critic(frozen["q1"], o0, a_pi)).mean()
        g = {k: torch.autograd.grad(loss[k], W[k]) for k in ONLINE_NAMES}
        mean_ent = (logp.detach() + te).mean()
        g_la = -mean_ent
        out["stats"][s] = torch.stack([loss["q1"].detach(), loss["q2"].detach(), loss["v"].detach(), loss["actor"].detach(), -(la * mean_ent), alpha,
                                       logp.detach().mean(), y.mean()])
        if return_trace:
            T = out["trace"]
            T["logp"][s, :c], T["vlogp"][s, :c], T["act"][s, :c] = logp.detach(), logp_v, a_pi.detach()
            T["fwd"][s, :c] = torch.stack([torch.where(d >= 1.0, torch.zeros_like(vt), vt), y, qa, qb, vb], 1)
        with torch.no_grad():
            t = u + 1
            corr = math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
            for name in ONLINE_NAMES:
                for i, (w, gw, mm, vv) in enumerate(zip(getattr(policy, name), g[name], policy.m[name], policy.v_[name])):
                    mm.mul_(beta1).add_(gw, alpha=1.0 - beta1)
                    vv.mul_(beta2).addcmul_(gw, gw, value=1.0 - beta2)
                    w.sub_(lr * corr * mm / (vv.sqrt() + eps))
                    if name == "v":
                        policy.v_target[i].mul_(1.0 - tau).add_(w, alpha=tau)
            if auto_alpha:
                A = policy.alpha_state
                A[1] = beta1 * A[1] + (1.0 - beta1) * g_la
                A[2] = beta2 * A[2] + (1.0 - beta2) * g_la * g_la
                A[0] = A[0] - lr * corr * A[1] / (A[2].sqrt() + eps)
        policy.steps += 1
        if return_grads:
            out["grads"] = {k: list(g[k]) for k in ONLINE_NAMES}
            out["grads"]["log_alpha"] = g_la
    policy.updated()
    return out


# ---------------------------------------------------------------------------------------------------- the loop
class SAC:
    """``SAC(policy, env, ...).learn(total_timesteps)``: SB2's SAC loop on N device envs, with SB2's defaults.  Per env step: before
    `learning_starts` transitions a uniform action, after them a sample of the actor (``policy.sample``: the actor's own
    state-dependent exploration, there is no action noise); ``env.step``; ``replay.add`` of the N transitions (ddpg.py's collection
    loop).  After every `train_freq` calls of ``env.step``, once `learning_starts` transitions are in, ONE update call of
    `gradient_steps` updates of `batch_size` rows drawn uniformly from the replay.  ``total_timesteps`` counts transitions: N per step.
    `ent_coef`: "auto" (the temperature is learned from 1.0), "auto_X" (learned from X) or a number (fixed).  `target_entropy`: "auto"
    is -4, minus the action dimension.  `update`: "hip" (sac_update) or "torch" (torch_sac_update); either draws the sample's noise
    from `seed` and the update index."""

    def __init__(self, policy, env, *, gamma=0.99, learning_rate=3.0e-4, buffer_size=50000, learning_starts=100, train_freq=1,
                 gradient_steps=1, batch_size=64, tau=5.0e-3, ent_coef="auto", target_entropy="auto", update="hip", seed=0, replay=None):
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
        auto, init = True, None
        if isinstance(ent_coef, str):
            if ent_coef != "auto" and not ent_coef.startswith("auto_"):
                raise ValueError("ent_coef must be 'auto', 'auto_<value>' or a number, got %r" % (ent_coef,))
            if ent_coef != "auto":
                init = float(ent_coef[len("auto_"):])
        else:
            auto, init = False, float(ent_coef)
        if init is not None:
            if not (init > 0.0 and math.isfinite(init)):
                raise ValueError("ent_coef must be finite and > 0, got %r" % (ent_coef,))
            policy.alpha_state[0] = math.log(init)
        if isinstance(target_entropy, str) and target_entropy != "auto":
            raise ValueError("target_entropy must be 'auto' or a number, got %r" % (target_entropy,))
        self.hyper = dict(gamma=gamma, tau=tau, lr=learning_rate, target_entropy=-4.0 if isinstance(target_entropy, str) else float(target_entropy),
                          auto_alpha=auto)
        check_sac_args(int(buffer_size), self.gradient_steps, self.batch_size, **self.hyper)
        self.action_noise = None
        self.replay = replay if replay is not None else ReplayBuffer(buffer_size, env.device)
        self.generator = torch.Generator().manual_seed(self.seed)                       # the replay schedule, on the host
        self.explore = torch.Generator(device=env.device).manual_seed(self.seed + 1)    # the uniform actions and the samples, on the env's device
        self.num_timesteps, self.obs = 0, None

    def act(self, obs):
        """the behaviour action of every env for `obs`"""
        import torch
        with torch.no_grad():
            if self.num_timesteps < self.learning_starts:
                a = torch.rand((obs.shape[0], 4), generator=self.explore, device=obs.device) * 2.0 - 1.0
            else:
                a = self.policy.sample(obs, self.explore).to(torch.float32)
        return a.contiguous()

    def learn(self, total_timesteps, log_interval=1):
        """-> a list of one dict per logged cycle: the cycle, `total_timesteps` so far, the eight statistics (SAC_STAT_NAMES, the mean
        over the cycle's updates), the mean reward of the cycle's env steps and `fps`"""
        fn = sac_update if self.update == "hip" else torch_sac_update

        def train():
            if self.num_timesteps < self.learning_starts:
                return None
            indices = replay_schedule(self.replay.size, self.gradient_steps, self.batch_size, self.generator)
            return fn(self.policy, self.replay, indices, seed=self.seed, **self.hyper)["stats"]
        return collect_and_train(self, total_timesteps, log_interval, self.train_freq, train, SAC_STAT_NAMES)
