"""Random-shooting MPC on the exact simulator (qs_shooting_plan).

``Mpc_Controller.choose_action`` of MPC-based_RL.py:170-210 rolls 200 random action sequences of horizon 20 through a learned
dynamics net, scores each by ``-sum |rel_pos|^2`` and applies the first action of the best one.  Here the model is the env
itself: ``shooting_plan`` rolls ``paths`` candidates per env through ``horizon`` env steps in ONE launch, read-only on the
env, and ``ShootingMPC`` is the closed loop of ``model_train`` (:213-241) without the dynamics net and its training.
"""
import ctypes as C

from . import _lib

OBJECTIVES = {"reward": _lib.SHOOT_REWARD, "position": _lib.SHOOT_POSITION}
MAX_PATHS, MAX_HORIZON = 65536, 256


def check_plan_args(horizon, paths, objective):
    """-> (horizon, paths, objective id); ValueError for what qs_shooting_plan would refuse, before anything touches the GPU"""
    if objective not in OBJECTIVES:
        raise ValueError("objective must be one of %s, got %r" % (sorted(OBJECTIVES), objective))
    horizon, paths = int(horizon), int(paths)
    if not 1 <= horizon <= MAX_HORIZON:
        raise ValueError("horizon must be in [1, %d], got %d" % (MAX_HORIZON, horizon))
    if not 1 <= paths <= MAX_PATHS:
        raise ValueError("paths must be in [1, %d], got %d" % (MAX_PATHS, paths))
    return horizon, paths, OBJECTIVES[objective]


def shooting_plan(env, horizon=20, paths=200, objective="reward", return_scores=False, return_sequence=False):
    """One plan for every env of `env` from its current state (the env is not modified).  objective "reward": the sum of the
    step rewards; "position": the reference's ``-sum |rel_pos|^2`` over the observations before each step.  Returns a dict of
    device tensors: actions [N,4] (the best candidate's first action), best_score [N] float64, best_index [N] int32, plus
    sequence [N,horizon,4] and scores [N,paths] float64 on request.  Candidates are keyed by (seed, env id, step counter,
    candidate, horizon step): a plan repeated before the same step is identical, and fewer paths are a prefix of more."""
    horizon, paths, obj = check_plan_args(horizon, paths, objective)
    import torch
    n, dev = env.num_envs, env.device
    out = {"actions": torch.empty((n, 4), dtype=torch.float32, device=dev),
           "best_score": torch.empty((n,), dtype=torch.float64, device=dev),
           "best_index": torch.empty((n,), dtype=torch.int32, device=dev)}
    if return_sequence:
        out["sequence"] = torch.empty((n, horizon, 4), dtype=torch.float32, device=dev)
    if return_scores:
        out["scores"] = torch.empty((n, paths), dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    env._use_current_stream()
    env._inputs_ready()
    _lib.check(env._lib.qs_shooting_plan(env._h, horizon, paths, obj, p(out["actions"]), p(out["best_score"]), p(out["best_index"]),
                                         p(out.get("sequence")), p(out.get("scores"))), "qs_shooting_plan")
    env._outputs_ready()
    return out


class ShootingMPC:
    """The sampling-based controller as a policy object beside PIDExpert: ``act()`` plans and returns the actions [N,4],
    ``run(steps)`` is the closed loop ``a = act(); env.step(a)``.  Defaults as Mpc_Controller.__init__ (:171)."""

    def __init__(self, env, horizon=20, paths=200, objective="reward"):
        self.horizon, self.paths, _ = check_plan_args(horizon, paths, objective)
        self.env, self.objective = env, objective
        self.last_plan = None

    def act(self):
        self.last_plan = shooting_plan(self.env, self.horizon, self.paths, self.objective)
        return self.last_plan["actions"]

    def run(self, steps):
        """`steps` times plan + env.step -> (rewards [steps,N] float32, dones [steps,N] bool), device tensors"""
        import torch
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        R, D = [], []
        for _ in range(steps):
            _, r, d, _ = self.env.step(self.act())
            R.append(torch.as_tensor(r).clone()); D.append(torch.as_tensor(d).clone())
        return torch.stack(R), torch.stack(D)
