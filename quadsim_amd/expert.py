"""PID expert + expert-dataset writer.

``PIDExpert`` is the scripted docking policy of run_expert_policy.py:49-69: a velocity controller that flies the
chaser to 0.2 m behind the target.  ``record_expert_dataset`` is run_expert_record.py:121-189 for N parallel envs:
it returns / saves the SB2 ``ExpertDataset`` dictionary (keys actions, obs, rewards, episode_returns,
episode_starts) that run_pretrained_ppo2_docking.py:50-69 feeds to behaviour cloning and GAIL.

The expert runs in the loop on the device: ``PIDExpert.rollout`` is T steps of ``a = expert.act(); env.step(a)`` in one
launch (qs_expert_rollout), ``PIDExpert.evaluate`` K complete episodes per env, read-only (qs_expert_evaluate); both give
the per-step loop's results bit for bit.
"""
import numpy as np

from . import _lib


class PIDExpert:
    def __init__(self, env, kp=0.35, kd=0.0):
        import torch
        self.env, self.kp, self.kd = env, float(kp), float(kd)
        n = env.num_envs
        try:
            c, _ = env.get_init_state()                     # stored initial states (docking-v1 / set_init_state)
        except _lib.QuadsimError:
            c = np.tile(np.array([8, -50, 5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], np.float32), (n, 1))
        self.state_des = torch.as_tensor(np.ascontiguousarray(c, np.float32)).to(env.device)   # = env.chaser_ini_state (:44)
        self._actions = torch.empty((n, 4), dtype=torch.float32, device=env.device)

    def act(self):
        """expert actions [N,4] for the envs' current states (a fresh tensor view is overwritten by the next call)"""
        self.env._call("qs_expert_action", self.state_des, self.kp, self.kd, self._actions)
        return self._actions

    def rollout(self, T, flags=False, env_major=False):
        """T steps of ``a = self.act(); env.step(a)`` in ONE launch (qs_expert_rollout), bit for bit that loop's results.
        Returns a dict of device tensors: obs [T,N,12] (the observation BEFORE step t: row 0 is what the preceding step / reset
        returned), actions [T,N,4] (not clipped), rewards [T,N], dones [T,N] bool, flags [T,N] uint8 if asked for, last_obs
        [N,12].  env_major=True: obs [N,T,12] and actions [N,T,4] (QS_LAYOUT_ENV_MAJOR, the order of an ExpertDataset); the
        scalars stay [T,N].  Advances the env and ``self.state_des``."""
        import torch
        e, T = self.env, int(T)
        n, kw = e.num_envs, dict(device=e.device)
        tt = max(T, 0)                        # T < 1 is refused by the library (QuadsimError)
        wide = (n, tt) if env_major else (tt, n)
        out = {"obs": torch.empty(wide + (12,), dtype=torch.float32, **kw), "actions": torch.empty(wide + (4,), dtype=torch.float32, **kw),
               "rewards": torch.empty((tt, n), dtype=torch.float32, **kw), "dones": torch.empty((tt, n), dtype=torch.uint8, **kw)}
        if flags:
            out["flags"] = torch.empty((tt, n), dtype=torch.uint8, **kw)
        out["last_obs"] = torch.empty((n, 12), dtype=torch.float32, **kw)
        e._call("qs_set_rollout_layout", 1 if env_major else 0)
        e._call("qs_expert_rollout", T, self.state_des, self.kp, self.kd, out["obs"], out["actions"], out["rewards"], out["dones"],
                out.get("flags"), out["last_obs"])
        e._nstep += T
        out["dones"] = out["dones"].view(torch.bool)
        return out

    def evaluate(self, n_episodes=1, max_steps=None):
        """`n_episodes` complete expert episodes for every env from its CURRENT state in ONE launch (qs_expert_evaluate), or
        `max_steps` steps per env at most (default n_episodes x 600: the env's time-out bounds every episode).  The env and
        ``self.state_des`` are left untouched.  Returns an EvalResult, as evaluate_policy_episodes does."""
        from .policy import EPISODE_STEPS, EvalResult
        e, K = self.env, int(n_episodes)      # K < 1 and max_steps < 1 are refused by the library (QuadsimError)
        max_steps = K * EPISODE_STEPS if max_steps is None else int(max_steps)
        res = EvalResult.empty(K, e.num_envs, e.device)
        e._call("qs_expert_evaluate", K, max_steps, self.state_des, self.kp, self.kd, *res.tensors())
        return res


class IncompleteEpisodes(RuntimeError):
    """an env did not finish the requested number of episodes within the recorded steps: record more"""


def assemble_expert_dataset(dones, rewards, n_episodes=None):
    """The bookkeeping of the recorder (run_expert_record.py:121-156) for N envs at once, as tensor operations (CPU or device
    tensors, no loop over steps or episodes).  dones, rewards: [N,T], each env's time series in a row.  Returns
    (episode_starts [N,T] bool, episode_returns float64 [E], mask):
      episode_starts  True on row 0 and after every done (:111, :146);
      episode_returns one entry per COMPLETE episode in env-major order (env by env, in time order): the float64 sum of that
                      episode's own float32 rewards -- a segmented sum, not a difference of running totals;
      mask            None (n_episodes is None: all rows of the recording), or [N,T] bool: the rows of every env's first
                      n_episodes complete episodes; episode_returns then holds exactly those N x n_episodes episodes.
    Raises IncompleteEpisodes if an env finished fewer than n_episodes episodes: a cut episode is never emitted."""
    import torch
    dones = torch.as_tensor(dones).bool()
    rewards = torch.as_tensor(rewards)
    n, T = dones.shape
    starts = torch.ones_like(dones)
    starts[:, 1:] = dones[:, :-1]
    seg = torch.cumsum(starts.reshape(-1).long(), 0) - 1                  # episode (segment) of every row, env-major
    nseg = int(seg[-1].item()) + 1 if seg.numel() else 0
    sums = torch.zeros(nseg, dtype=torch.float64, device=dones.device).index_add_(0, seg, rewards.reshape(-1).double())
    complete = torch.zeros(nseg, dtype=torch.bool, device=dones.device)
    complete[seg[dones.reshape(-1)]] = True                               # an episode is complete iff its last row is a done
    if n_episodes is None:
        return starts, sums[complete], None
    K = int(n_episodes)
    if K < 1:
        raise ValueError("n_episodes must be >= 1")
    count = dones.sum(dim=1)
    if bool((count < K).any()):
        raise IncompleteEpisodes("%d of %d envs finished fewer than %d episodes within %d steps: record more steps"
                                 % (int((count < K).sum()), n, K, T))
    d = dones.long()
    ep = torch.cumsum(d, dim=1) - d                                       # episodes the env completed BEFORE this row
    mask = ep < K
    seg_ep = torch.zeros(nseg, dtype=torch.long, device=dones.device)
    seg_ep[seg] = ep.reshape(-1)                                          # every row of a segment carries the same value
    return starts, sums[complete & (seg_ep < K)], mask


def _record_per_step(env, expert, n_steps):
    """two launches per step from Python -> obs [T,N,12], actions [T,N,4], rewards [T,N], dones [T,N]"""
    import torch
    obs = env.reset()
    O, A, R, D = [], [], [], []
    for _ in range(n_steps):
        a = expert.act()
        O.append(obs.clone()); A.append(a.clone())
        obs, r, d, _ = env.step(a)
        R.append(r.clone()); D.append(d.clone())
    return torch.stack(O), torch.stack(A), torch.stack(R), torch.stack(D)


def record_expert_dataset(env, n_steps=None, expert=None, save_path=None, n_episodes=None, fused=True):
    """Record the expert in every env (auto-reset on) from a reset and return the ExpertDataset dict with the env-major
    flattening the single-env recorder produces (each env's time series is contiguous).  Exactly one of
      n_steps     that many steps per env: N x n_steps rows (the last episode of every env is cut off), or
      n_episodes  every env's first n_episodes COMPLETE episodes and nothing after them, as run_expert_record.py:121-156
                  records for each env in turn: len(episode_returns) == N x n_episodes.
    fused=True: qs_expert_rollout in env-major layout (one launch per 600 steps at most), the bookkeeping
    (assemble_expert_dataset) on the device, one copy to the host.  fused=False: two launches per step and host loops --
    the same rows, kept as the comparison."""
    import torch
    if (n_steps is None) == (n_episodes is None):
        raise ValueError("record_expert_dataset: give exactly one of n_steps and n_episodes")
    if (n_steps if n_steps is not None else n_episodes) < 1:
        raise ValueError("record_expert_dataset: n_steps / n_episodes must be >= 1")
    from .policy import EPISODE_STEPS
    from .rollout_buffer import swap_and_flatten
    expert = expert or PIDExpert(env)
    n = env.num_envs
    if not fused:
        T = int(n_steps) if n_steps is not None else int(n_episodes) * EPISODE_STEPS      # an episode lasts at most 600 steps
        O, A, R, D = _record_per_step(env, expert, T)
        flat = lambda x: swap_and_flatten(env, x).cpu().numpy()       # noqa: E731
        if n_episodes is not None:
            starts, rets, mask = assemble_expert_dataset(D.t().cpu(), R.t().cpu(), n_episodes)
            m = mask.reshape(-1).numpy()
            data = {"actions": flat(A)[m], "obs": flat(O)[m], "rewards": flat(R)[m], "episode_returns": rets.numpy(),
                    "episode_starts": starts.reshape(-1).numpy()[m]}
        else:
            starts = torch.ones((T, n), dtype=torch.bool, device=env.device)
            starts[1:] = D[:-1]                                       # episode_starts.append(done) shifted by one (:111,:146)
            rets = []
            Rn, Dn = R.cpu().numpy(), D.cpu().numpy()
            acc = np.zeros(n)
            for t in range(T):                                        # episode_returns in env-major order, like the recorder
                acc += Rn[t]
                for i in np.nonzero(Dn[t])[0]:
                    rets.append((i, t, acc[i])); acc[i] = 0.0
            rets.sort()
            data = {"actions": flat(A), "obs": flat(O), "rewards": flat(R), "episode_returns": np.array([x[2] for x in rets]),
                    "episode_starts": starts.cpu().numpy().swapaxes(0, 1).reshape(-1)}
    else:
        env.reset()
        if n_steps is not None:
            ro = expert.rollout(int(n_steps), env_major=True)
            obs, act, rew, done = ro["obs"], ro["actions"], ro["rewards"].t(), ro["dones"].t()
        else:
            K = int(n_episodes)
            chunks, count = [], torch.zeros(n, dtype=torch.long, device=env.device)
            for _ in range(K):                                        # K x 600 steps always suffice; stop as soon as every env has K
                chunks.append(expert.rollout(EPISODE_STEPS, env_major=True))
                count += chunks[-1]["dones"].sum(dim=0)
                if bool((count >= K).all()):
                    break
            cat = lambda k, d: chunks[0][k] if len(chunks) == 1 else torch.cat([c[k] for c in chunks], dim=d)   # noqa: E731
            obs, act, rew, done = cat("obs", 1), cat("actions", 1), cat("rewards", 0).t(), cat("dones", 0).t()
        starts, rets, mask = assemble_expert_dataset(done, rew, n_episodes)
        rew = rew.contiguous()
        if mask is None:
            obs, act, rew, starts = obs.reshape(-1, 12), act.reshape(-1, 4), rew.reshape(-1), starts.reshape(-1)
        else:
            obs, act, rew, starts = obs[mask], act[mask], rew[mask], starts[mask]
        data = {"actions": act.cpu().numpy(), "obs": obs.cpu().numpy(), "rewards": rew.cpu().numpy(),
                "episode_returns": rets.cpu().numpy(), "episode_starts": starts.cpu().numpy()}
    if save_path is not None:
        np.savez(save_path, **data)
    return data
