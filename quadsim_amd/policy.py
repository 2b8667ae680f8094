"""Policy-in-the-loop roll-outs on the device.

``MlpPolicy`` is the deterministic actor of the PPO2 model the reference ships
(`trained_model/best_model_v0.zip`: shared_fc0 12->128, pi_fc0 128->128, pi 128->4,
ReLU, actions clipped to [-1, 1]) as `run_trained_docking_ppo2.py:37-45` uses it:
``action, _ = model.predict(obs, deterministic=True); env.step(action)``.
The three GEMMs are plain library GEMMs (torch -> hipBLASLt); the env step is the
fused HIP kernel.  The loop never leaves the GPU: no host sync between steps.
"""
import numpy as np


class MlpPolicy:
    def __init__(self, weights, device="cuda"):
        import torch
        self.torch = torch
        g = lambda k: torch.as_tensor(np.asarray(weights[k], np.float32)).to(device)  # noqa: E731
        self.w0, self.b0 = g("w0"), g("b0")
        self.w1, self.b1 = g("w1"), g("b1")
        self.w2, self.b2 = g("w2"), g("b2")

    @classmethod
    def from_npz(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            return cls({k: z[k] for k in z.files}, device)

    @classmethod
    def from_sb2_zip(cls, path, device="cuda"):
        """the deterministic actor of a stable-baselines PPO2 archive (quadsim_amd.sb2): shared_fc0 -> pi_fc0 -> pi of the
        shared-trunk layout or pi_fc0 -> pi_fc1 -> pi of the tower layout -- the same 12 -> 128 -> 128 -> 4 ReLU network
        either way, so every actor kernel runs both"""
        from .sb2 import read_sb2_weights
        return cls(read_sb2_weights(path)[1], device)

    def predict(self, obs):
        """obs [N,12] float32 (device) -> actions [N,4] in [-1,1]"""
        t = self.torch
        h = t.relu(t.addmm(self.b0, obs, self.w0))
        h = t.relu(t.addmm(self.b1, h, self.w1))
        return t.clamp(t.addmm(self.b2, h, self.w2), -1.0, 1.0)

    def transposed_weights(self):
        """[W0^T, b0, W1^T, b1, W2^T, b2], contiguous: the weight arguments of every exact-f32 actor kernel (built once)"""
        if not hasattr(self, "_wt"):
            self._wt = [self.w0.t().contiguous(), self.b0.contiguous(), self.w1.t().contiguous(),
                        self.b1.contiguous(), self.w2.t().contiguous(), self.b2.contiguous()]
        return self._wt

    def fast_blob(self):
        """pack_fast_weights as a device tensor: the weight argument of every split-bf16 actor kernel (built once)"""
        if not hasattr(self, "_blob"):
            from . import _lib
            blob = pack_fast_weights(self)
            assert blob.size == _lib.fast_blob_bytes("qs_policy_rollout_fast")
            self._blob = self.torch.as_tensor(blob.copy()).to(self.w0.device)
        return self._blob

    def pretrain(self, dataset, **kw):
        """behaviour cloning on the device: quadsim_amd.bc.pretrain(self, dataset, ...)"""
        from .bc import pretrain
        return pretrain(self, dataset, **kw)

    def reset_pretrain_optimizer(self):
        from .bc import reset_pretrain_optimizer
        reset_pretrain_optimizer(self)

    def predict_hip(self, env, obs, precision="f32", out=None):
        """the same actor as ONE hand-written kernel on the matrix cores (qs_policy_forward: exact-f32 MFMA; "bf16x3":
        split-bf16 operands, ~1e-5 on an action), launched on `env`'s stream: obs [n,12] float32 device tensor -> actions
        [n,4].  65 536 rows: ~22 us against ~80 us for the three library GEMMs of predict()."""
        import torch
        if (not isinstance(obs, torch.Tensor) or obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[1] != 12
                or obs.device != env.device):
            raise ValueError("predict_hip: obs must be a float32 [n, 12] tensor on %s" % (env.device,))
        obs = obs.contiguous()
        n = int(obs.shape[0])
        if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (n, 4) or not out.is_contiguous() or out.device != obs.device):
            raise ValueError("predict_hip: out must be a contiguous float32 [n, 4] tensor on the same device")
        acts = out if out is not None else torch.empty((n, 4), dtype=torch.float32, device=obs.device)
        if precision == "bf16x3":
            env._call("qs_policy_forward_fast", n, self.fast_blob(), obs, acts)
        elif precision == "f32":
            env._call("qs_policy_forward", n, *self.transposed_weights(), obs, acts)
        else:
            raise ValueError("precision must be 'f32' or 'bf16x3'")
        return acts


def _bf16_bits(x):
    """float32 -> bfloat16 bit pattern, round to nearest even (what v_cvt_pk_bf16_f32 does)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) >> 16).astype(np.uint16)


def _bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def pack_fast_weights(policy):
    """Weight image of qs_policy_rollout_fast: every weight split into bf16 hi + lo, A-operand fragments stored
    ready-made in the k-order the accumulator-as-B-operand chaining needs (csrc/mlp.hpp, 'Fast actor')."""
    w1t = policy.w0.t().contiguous().cpu().numpy()      # [128][12]
    w2t = policy.w1.t().contiguous().cpu().numpy()      # [128][128]
    w3t = policy.w2.t().contiguous().cpu().numpy()      # [4][128]
    lane = np.arange(64); g, c = lane >> 4, lane & 15
    j = np.arange(8)
    hid = lambda p: 16 * (2 * p + (j[None, :] >> 2)) + 4 * g[:, None] + (j[None, :] & 3)       # noqa: E731  [lane][j]
    a2 = np.zeros((8, 4, 64, 8), np.float32)
    for nt in range(8):
        for p in range(4):
            a2[nt, p] = w2t[(16 * nt + c)[:, None], hid(p)]
    a1 = np.zeros((8, 64, 8), np.float32)
    k1 = 8 * g[:, None] + j[None, :]
    for rt in range(8):
        a1[rt] = np.where(k1 < 12, w1t[(16 * rt + c)[:, None], np.minimum(k1, 11)], 0.0)
    a3 = np.zeros((4, 64, 8), np.float32)
    for q in range(4):
        a3[q] = np.where((c < 4)[:, None], w3t[np.minimum(c, 3)[:, None], hid(q)], 0.0)
    parts = []
    for a in (a2, a1, a3):
        hi = _bf16_bits(a)
        lo = _bf16_bits(a - _bf16_to_f32(hi))
        parts += [hi.tobytes(), lo.tobytes()]
    b3 = np.zeros(16, np.float32); b3[:4] = policy.b2.cpu().numpy()
    parts += [policy.b0.cpu().numpy().astype(np.float32).tobytes(), policy.b1.cpu().numpy().astype(np.float32).tobytes(),
              b3.tobytes()]
    blob = np.frombuffer(b"".join(parts), np.uint8)
    return blob


def fused_policy_rollout(env, policy, T, want_actions=True, precision="f32"):
    """The same loop as rollout_with_policy in ONE kernel launch: MLP on the matrix cores + fused env step, T steps,
    no host involvement.  Starts from the envs' current state.
    precision "f32": qs_policy_rollout, exact-float32 MFMA (an ordinary float32 network evaluation);
    precision "bf16x3": qs_policy_rollout_fast, split-bf16 operands on the 16x faster bf16 matrix rate, ~1e-5 error
    on the actions.  Returns (obs [T,N,12], reward [T,N], done [T,N] u8, flags [T,N] u8, actions [T,N,4] or None)."""
    import torch
    n, dev = env.num_envs, env.device
    obs = torch.empty((T, n, 12), dtype=torch.float32, device=dev)
    rew = torch.empty((T, n), dtype=torch.float32, device=dev)
    done = torch.empty((T, n), dtype=torch.uint8, device=dev)
    flags = torch.empty((T, n), dtype=torch.uint8, device=dev)
    acts = torch.empty((T, n, 4), dtype=torch.float32, device=dev) if want_actions else None
    if precision == "bf16x3":
        env._call("qs_policy_rollout_fast", T, policy.fast_blob(), obs, rew, done, flags, acts)
    elif precision == "f32":
        env._call("qs_policy_rollout", T, *policy.transposed_weights(), obs, rew, done, flags, acts)
    else:
        raise ValueError("precision must be 'f32' or 'bf16x3'")
    return obs, rew, done, flags, acts


def rollout_with_policy(env, policy, T, obs0=None):
    """T steps of ``a = policy(obs); obs, r, d, info = env.step(a)`` on a torch-backend VecDockingEnv.
    Returns stacked (obs [T,N,12], reward [T,N], done [T,N] bool, flags [T,N] u8, actions [T,N,4])."""
    import torch
    obs = env.reset() if obs0 is None else obs0
    O, R, D, F, A = [], [], [], [], []
    for _ in range(T):
        a = policy.predict(obs)
        obs, r, d, info = env.step(a)
        O.append(obs.clone()); R.append(r.clone()); D.append(d.clone()); F.append(env._flags.clone()); A.append(a)
    return torch.stack(O), torch.stack(R), torch.stack(D), torch.stack(F), torch.stack(A)


# ---------------------------------------------------------------- deterministic evaluation (qs_policy_evaluate)
EPISODE_STEPS = 600          # DockingEnv's time-out: done_overtime = t >= 600 (docking_env.py:152) bounds every episode


def _actor_of(policy):
    """the deterministic actor (an MlpPolicy) of an MlpPolicy or an ActorCriticPolicy (either layout: its pi weights)"""
    if isinstance(policy, MlpPolicy):
        return policy
    from .runner import ActorCriticPolicy
    if isinstance(policy, ActorCriticPolicy):
        if policy.squash:
            raise ValueError("the evaluation kernels run the clipped actor; a squashed (tanh) ActorCriticPolicy is not supported")
        actor = getattr(policy, "_eval_actor", None)
        if actor is None:
            actor = MlpPolicy.__new__(MlpPolicy)
            actor.torch = policy.torch
            actor.w0, actor.b0, actor.w1, actor.b1, actor.w2, actor.b2 = (policy.w0, policy.b0, policy.w1, policy.b1, policy.w2,
                                                                          policy.b2)
            policy._eval_actor = actor
        return actor
    raise TypeError("expected an MlpPolicy or an ActorCriticPolicy, got %s" % type(policy).__name__)


class EvalResult:
    """K episodes of N envs, as device tensors: returns [K,N] float64, lengths [K,N] int32, flags [K,N] uint8 (OR of the step
    flags), docked_steps [K,N] int32, finished [N] int32.  Slot (k, env) holds an episode iff k < finished[env]; the summary
    helpers use those episodes only."""

    def __init__(self, returns, lengths, flags, docked_steps, finished):
        self.returns, self.lengths, self.flags, self.docked_steps, self.finished = returns, lengths, flags, docked_steps, finished

    @classmethod
    def empty(cls, K, n, device):
        """the result of K episodes of n envs before the evaluation kernel has run: the slots of unfinished episodes stay as
        they are here (returns NaN, the rest 0)"""
        import torch
        kk = max(int(K), 0)          # K < 1 is refused by the library (QuadsimError)
        return cls(torch.full((kk, n), float("nan"), dtype=torch.float64, device=device),
                   torch.zeros((kk, n), dtype=torch.int32, device=device), torch.zeros((kk, n), dtype=torch.uint8, device=device),
                   torch.zeros((kk, n), dtype=torch.int32, device=device), torch.empty((n,), dtype=torch.int32, device=device))

    def tensors(self):
        """(returns, lengths, flags, docked_steps, finished): the output arguments of the evaluation entry points, in order"""
        return self.returns, self.lengths, self.flags, self.docked_steps, self.finished

    @property
    def episodes_per_env(self):
        return int(self.returns.shape[0])

    def valid(self):
        """[K,N] bool: the slots that hold a finished episode"""
        import torch
        k = torch.arange(self.episodes_per_env, device=self.finished.device)[:, None]
        return k < self.finished[None, :]

    def _sel(self, t):
        return t[self.valid()]

    def num_episodes(self):
        return int(self.finished.sum().item())

    def mean_return(self):
        return float(self._sel(self.returns).mean().item())

    def std_return(self):
        """population std (ddof = 0), as np.std in SB2's evaluate_policy"""
        return float(self._sel(self.returns).std(unbiased=False).item())

    def mean_length(self):
        return float(self._sel(self.lengths).double().mean().item())

    def docked_fraction(self):
        """share of episodes with at least one docked step"""
        return float((self._sel(self.docked_steps) > 0).double().mean().item())

    def overlimit_fraction(self):
        """share of episodes that ended out of bounds (QS_FLAG_OVERLIMIT among their flags)"""
        from ._lib import FLAG_OVERLIMIT
        return float(((self._sel(self.flags) & FLAG_OVERLIMIT) != 0).double().mean().item())

    def numpy(self):
        return {k: t.cpu().numpy() for k, t in zip(("returns", "lengths", "flags", "docked_steps", "finished"), self.tensors())}


def evaluate_policy_episodes(policy, env, episodes_per_env=1, precision="f32", max_steps=None):
    """`episodes_per_env` complete episodes of ``action = policy.predict(obs, deterministic=True); env.step(action)`` for every
    env of `env` (a VecDockingEnv: docking-v0 / v1 / v2, any randomise mode, per-env params) in ONE kernel launch
    (qs_policy_evaluate: exact-f32 actor, or qs_policy_evaluate_fast with precision="bf16x3").  Each env starts from its current
    state; the auto-reset between episodes is the step API's.  The same episodes, bit for bit, as the loop
    ``obs -> policy.predict_hip(env, obs, precision) -> env.step`` from the same handle -- which the call leaves untouched (state,
    parameters, step counter): every evaluation of a handle sees the same starts.  max_steps (default K x 600: the env's
    time-out bounds every episode) caps the steps per env.  Returns an EvalResult of device tensors, on env's stream."""
    K = int(episodes_per_env)          # K < 1 and max_steps < 1 are refused by the library (QuadsimError)
    max_steps = K * EPISODE_STEPS if max_steps is None else int(max_steps)
    actor = _actor_of(policy)
    if precision not in ("f32", "bf16x3"):
        raise ValueError("precision must be 'f32' or 'bf16x3'")
    res = EvalResult.empty(K, env.num_envs, env.device)
    if precision == "bf16x3":
        env._call("qs_policy_evaluate_fast", K, max_steps, actor.fast_blob(), *res.tensors())
    else:
        env._call("qs_policy_evaluate", K, max_steps, *actor.transposed_weights(), *res.tensors())
    return res


def episodes_for(n_eval_episodes, num_envs):
    """episodes per env of an evaluation of n_eval_episodes over num_envs envs (every env runs the same number)"""
    n_eval_episodes, num_envs = int(n_eval_episodes), int(num_envs)
    if n_eval_episodes < 1 or n_eval_episodes % num_envs:
        raise ValueError("n_eval_episodes (%d) must be a positive multiple of the env's num_envs (%d): every env runs the same "
                         "number of episodes" % (n_eval_episodes, num_envs))
    return n_eval_episodes // num_envs


def summarise_episodes(returns, lengths, finished, return_episode_rewards=False):
    """host side of evaluate_policy on NumPy arrays returns [K,N], lengths [K,N], finished [N]: SB2's result -- (mean, std)
    of the episode returns (np.mean / np.std), or (episode_rewards, episode_lengths) as lists in (k, env) order"""
    returns, lengths, finished = np.asarray(returns), np.asarray(lengths), np.asarray(finished)
    K = returns.shape[0]
    if np.any(finished < K):
        raise RuntimeError("%d of %d envs did not finish %d episodes within max_steps" % (int(np.sum(finished < K)), finished.size, K))
    episode_rewards = [float(r) for r in returns.reshape(-1)]
    episode_lengths = [int(x) for x in lengths.reshape(-1)]
    if return_episode_rewards:
        return episode_rewards, episode_lengths
    return float(np.mean(episode_rewards)), float(np.std(episode_rewards))


def evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, return_episode_rewards=False, precision="f32"):
    """stable_baselines.common.evaluation.evaluate_policy (run_docking_ppo2.py:8, the EvalCallback of :75-83) on the device:
    -> (mean_reward, std_reward), or (episode_rewards, episode_lengths) lists with return_episode_rewards=True.
    Differs from SB2, which runs n_eval_episodes one after another on one env: here every one of env.num_envs envs runs
    n_eval_episodes / num_envs episodes in one launch (evaluate_policy_episodes), so n_eval_episodes must be a multiple of
    num_envs (ValueError otherwise); the lists are in (episode k, env) order.  Deterministic actions only."""
    if not deterministic:
        raise NotImplementedError("evaluate_policy: only deterministic evaluation runs on the device")
    K = episodes_for(n_eval_episodes, env.num_envs)
    res = evaluate_policy_episodes(model, env, K, precision=precision)
    h = res.numpy()
    return summarise_episodes(h["returns"], h["lengths"], h["finished"], return_episode_rewards)
