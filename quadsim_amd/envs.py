"""Single-env shims with the old-gym ``Env`` protocol of the reference:
``DockingEnv`` (gym-docking/gym_docking/envs/docking_env.py:12-254) and
``MovingDockingEnv`` (moving_docking_env.py).  One env (N = 1) on the GPU with
host I/O: ``reset() -> ndarray(12,)``, ``step(a) -> (obs, reward, done, info)``;
``step`` never resets by itself (docking_env.py:104-231).  The attribute surface
the reference scripts rely on is kept.
"""
import numpy as np

from . import _lib
from .drone import Drone
from .spaces import docking_spaces


class _ChaserView(Drone):
    """env.chaser / env.target: constants + get_* only (run_expert_policy.py:41, run_trained_docking_ppo2.py:45)"""


class _HostHandle:
    """a QS_IO_HOST handle of one env: numpy arrays in and out, every call complete when it returns -- no stream protocol"""
    metadata = {"render.modes": ["human"]}

    def _create(self, cfg):
        self._lib = _lib.load()
        self._h = _lib.create(cfg)

    def _call(self, name, *args):
        _lib.call(self._h, name, *args)

    def render(self, mode="human"):
        return None

    def seed(self, seed=None):
        self.np_random = np.random.RandomState(seed)
        return [seed]

    def close(self):
        if getattr(self, "_h", None):
            self._lib.qs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _SingleDockingEnv(_HostHandle):
    _kind = _lib.KIND_V0
    spec = None
    reward_range = (-float("inf"), float("inf"))

    def __init__(self, device=0, integrator="frozen"):
        cfg = _lib.default_config()
        cfg.kind = self._kind
        cfg.num_envs = 1
        cfg.device = device
        cfg.integrator = _lib.INTEG_RK4 if integrator == "rk4" else _lib.INTEG_FROZEN
        cfg.auto_reset = 0
        cfg.io_space = _lib.IO_HOST
        self._config_hook(cfg)
        self.cfg = cfg
        self._create(cfg)
        self._nominal_chaser = np.array([8, -50, 5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float64)
        self.chaser = _ChaserView(device)
        self.target = _ChaserView(device)
        self.observation_space, self.action_space = docking_spaces()
        self.obs_low, self.obs_high = self.observation_space.low, self.observation_space.high
        self.chaser_ini_state = np.array([8, -50, 5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float64)
        self.target_ini_state = np.array([10, -50, 5, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0], dtype=np.float64)
        self.chaser_dock_port = np.array([0.1, 0.0, 0.0])
        self.target_dock_port = np.array([-0.1, 0.0, 0.0])
        self.action_mean = np.ones(4) * self.chaser.mass * self.chaser.gravity / 2.0
        self.action_std = np.ones(4) * self.chaser.mass * self.chaser.gravity / 2.0
        self.t = 0
        self.done = False
        self.reward = 0.0
        self.last_shaping = 0.0
        self.np_random = None
        self._pull_state()
        self.rel_state = self._obs_now()
        self.seed()

    def _config_hook(self, cfg):
        pass

    # -- helpers -------------------------------------------------------------
    def _pull_state(self):
        sc = np.zeros((1, 13), np.float32); st = np.zeros((1, 13), np.float32)
        ls = np.zeros(1, np.float32); t = np.zeros(1, np.float32)
        self._call("qs_get_state", sc, st, None, None, ls, t)
        self.state_chaser = sc[0].astype(np.float64)
        self.state_target = st[0].astype(np.float64)
        self.last_shaping = float(ls[0])

    def _obs_now(self):
        from .drone import rel_obs_batch
        return rel_obs_batch(self.state_chaser[None], self.state_target[None])[0].astype(np.float64)

    # -- gym.Env protocol ------------------------------------------------------
    def reset(self):
        obs = np.zeros((1, 12), np.float32)
        # honour a script-mutated chaser_ini_state (run_expert_policy.py:44,63-64): reset() restores THAT state
        if not np.array_equal(self.chaser_ini_state, self._nominal_chaser):
            sc = np.ascontiguousarray(self.chaser_ini_state[None], dtype=np.float32)
            st = np.ascontiguousarray(self.target_ini_state[None], dtype=np.float32)
            self._call("qs_set_init_state", sc, st)
            self._nominal_chaser = self.chaser_ini_state.copy()
        self._call("qs_reset", None, obs)
        self._pull_state()
        self.done = False
        self.t = 0.0
        self.reward = 0.0
        self.rel_state = obs[0].astype(np.float64)
        return self.rel_state

    def step(self, action):
        a = np.ascontiguousarray(np.asarray(action, dtype=np.float32).reshape(1, 4))
        obs = np.zeros((1, 12), np.float32); rew = np.zeros(1, np.float32)
        done = np.zeros(1, np.uint8); flags = np.zeros(1, np.uint8)
        self._call("qs_step", a, obs, rew, done, flags, None)
        self.t += 1
        self._pull_state()
        self.rel_state = obs[0].astype(np.float64)
        self.reward = float(rew[0])
        self.done = bool(done[0])
        info = {"chaser": self.state_chaser, "target": self.state_target,
                "flag_docking": bool(flags[0] & _lib.FLAG_DOCKED),
                "done_overlimit": bool(flags[0] & _lib.FLAG_OVERLIMIT)}
        return self.rel_state, self.reward, self.done, info

    def shooting_plan(self, horizon=20, paths=200, objective="reward", splits="auto", return_scores=False, return_sequence=False):
        """Mpc_Controller.choose_action (MPC-based_RL.py:170-210) on the env itself: the best of `paths` random action
        sequences of `horizon` steps from the current state, which is not modified.  -> dict of numpy results: actions [4]
        (pass it to step()), best_score, best_index, plus sequence [horizon,4] and scores [paths] on request; `splits` as in
        quadsim_amd.mpc.shooting_plan"""
        from .mpc import shooting_plan_host
        return shooting_plan_host(self, horizon, paths, objective, splits, return_scores, return_sequence)

    def mppi_plan(self, horizon=20, paths=200, iterations=2, objective="reward", lam=None, sigma=None, nominal=None, shift=False,
                  noise=None, splits="auto", return_scores=False, return_trace=False, return_candidates=False):
        """MPPI on the env itself from the current state, which is not modified: `iterations` rounds of `paths` Gaussian
        candidates around `nominal` [horizon,4] (None: zeros; shifted by one step first if `shift`).  -> dict of numpy results:
        actions [4] (pass it to step()), nominal [horizon,4] (carry it to the next plan with shift=True), best_score, plus
        scores, trace and candidates on request; `lam` and `sigma` default to, and every argument is as in,
        quadsim_amd.mpc.mppi_plan"""
        from . import mpc
        return mpc.mppi_plan_host(self, horizon, paths, iterations, objective, mpc.MPPI_DEFAULT_LAMBDA if lam is None else lam,
                                  mpc.MPPI_DEFAULT_SIGMA if sigma is None else sigma, nominal, shift, noise, splits, return_scores,
                                  return_trace, return_candidates)

class DockingEnv(_SingleDockingEnv):
    """docking-v0"""
    _kind = _lib.KIND_V0


class MovingDockingEnv(_SingleDockingEnv):
    """docking-v2"""
    _kind = _lib.KIND_V2


class ImitatingDockingEnv(_SingleDockingEnv):
    """docking-v1 (imitating_docking_env.py): v0 whose chaser start is jittered once at construction (:34).
    The jitter comes from the rocRAND INIT stream keyed by `seed`; set ``chaser_ini_state`` + reset() to inject one."""
    _kind = _lib.KIND_V1

    def __init__(self, device=0, integrator="frozen", seed=0):
        self._seed0 = seed
        super().__init__(device, integrator)
        sc = np.zeros((1, 13), np.float32); st = np.zeros((1, 13), np.float32)
        self._call("qs_get_init_state", sc, st)
        self.chaser_ini_state = sc[0].astype(np.float64)
        self._nominal_chaser = self.chaser_ini_state.copy()

    def _config_hook(self, cfg):
        cfg.seed = int(self._seed0)


class HoveringEnv(_HostHandle):
    """hovering-v0 (hovering_env.py:10-92): one drone, obs = raw state [13], action in [0,1]^4, step never resets."""

    def __init__(self, device=0, integrator="frozen", seed=0):
        from .spaces import hovering_spaces
        cfg = _lib.default_config()
        cfg.kind, cfg.num_envs, cfg.device, cfg.auto_reset, cfg.io_space = _lib.KIND_HOVER, 1, device, 0, _lib.IO_HOST
        cfg.integrator = _lib.INTEG_RK4 if integrator == "rk4" else _lib.INTEG_FROZEN
        cfg.seed = int(seed)
        self._create(cfg)
        self.drone = _ChaserView(device)
        self.observation_space, self.action_space = hovering_spaces()
        self.action_max = np.ones(4) * self.drone.mass * self.drone.gravity
        ini = np.zeros((1, 13), np.float32)
        self._call("qs_get_init_state", ini, None)
        self.ini_state = ini[0].astype(np.float64)
        self.state_des = np.array([0, 0, 5.0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0])
        self.state = np.zeros(13)
        self.np_random = np.random.RandomState(seed)

    def reset(self):
        ini = np.ascontiguousarray(self.ini_state[None], dtype=np.float32)      # honours a caller-set ini_state
        self._call("qs_set_init_state", ini, None)
        obs = np.zeros((1, 13), np.float32)
        self._call("qs_reset", None, obs)
        self.state = obs[0].astype(np.float64)
        return self.state

    def step(self, action):
        a = np.ascontiguousarray(np.asarray(action, dtype=np.float32).reshape(1, 4))
        obs = np.zeros((1, 13), np.float32); rew = np.zeros(1, np.float32); done = np.zeros(1, np.uint8)
        self._call("qs_step", a, obs, rew, done, None, None)
        self.state = obs[0].astype(np.float64)
        return self.state, float(rew[0]), bool(done[0]), {}

def register_gym_ids():
    """register 'docking-v0' / 'docking-v2' with gym when gym is importable
    (gym-docking/gym_docking/__init__.py:3-17); returns True if registered."""
    try:
        from gym.envs.registration import register
    except Exception:  # noqa: BLE001
        return False
    for gid, cls in (("docking-v0", "DockingEnv"), ("docking-v2", "MovingDockingEnv"),
                     ("docking-v1", "ImitatingDockingEnv"), ("hovering-v0", "HoveringEnv")):
        try:
            register(id=gid, entry_point="quadsim_amd.envs:%s" % cls)
        except Exception:  # already registered
            pass
    return True


def make(env_id, **kw):
    """gym.make stand-in for the two ids of the hot path"""
    name = env_id.split(":")[-1]
    if name == "docking-v0":
        return DockingEnv(**kw)
    if name == "docking-v2":
        return MovingDockingEnv(**kw)
    if name == "docking-v1":
        return ImitatingDockingEnv(**kw)
    if name == "hovering-v0":
        return HoveringEnv(**kw)
    raise ValueError("unknown env id %r" % env_id)
