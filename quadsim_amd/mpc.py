"""Sampling-based MPC on the exact simulator: random shooting (qs_shooting_plan) and MPPI (qs_mppi_plan).

``Mpc_Controller.choose_action`` of MPC-based_RL.py:170-210 rolls 200 random action sequences of horizon 20 through a learned
dynamics net, scores each by ``-sum |rel_pos|^2`` and applies the first action of the best one.  Here the model is the env
itself: ``shooting_plan`` rolls ``paths`` candidates per env through ``horizon`` env steps in ONE launch, read-only on the
env, and ``ShootingMPC`` is the closed loop of ``model_train`` (:213-241) without the dynamics net and its training.
With ``splits`` one env's candidates are spread over that many workgroups (qs_shooting_plan_split: two launches, the same
bits), which is what a handle of one or a few envs needs to use more than one compute unit.

``mppi_plan`` / ``MPPI`` are the iterated, warm-started member of the same family (model-predictive path integral control):
Gaussian candidates around a nominal action sequence, scored the same way, and the nominal replaced by their softmax-weighted
mean, ``iterations`` times in one launch; the nominal is carried from plan to plan.  With ``splits`` the candidates of one env
are spread over that many workgroups here too (qs_mppi_plan_split: three launches per iteration, up to 65536 paths; the order
of the update's sums depends on the number of parts, so the nominal agrees with the unsplit one to one float32 rounding).
"""
import ctypes as C
import operator

from . import _lib

OBJECTIVES = {"reward": _lib.SHOOT_REWARD, "position": _lib.SHOOT_POSITION}
MAX_PATHS, MAX_HORIZON, MAX_SPLITS = 65536, 256, 1024
MPPI_MAX_PATHS, MPPI_MAX_HORIZON, MPPI_MAX_ITERATIONS = 4096, 128, 16
MPPI_SPLIT_MAX_PATHS = 65536          # qs_mppi_plan_split; one part (splits = 1) is qs_mppi_plan's kernel and keeps its 4096
# Tuned on ONE setting only (4096 docking-v0 envs, horizon 20, 200 paths, 2 iterations, objective "reward", 600 steps):
# the sweep is in profiles/mppi/README.md.
MPPI_DEFAULT_LAMBDA, MPPI_DEFAULT_SIGMA = 0.05, 0.25


def _check_common(horizon, paths, objective, max_horizon, max_paths):
    """-> (horizon, paths, objective id), what both planners check alike"""
    if objective not in OBJECTIVES:
        raise ValueError("objective must be one of %s, got %r" % (sorted(OBJECTIVES), objective))
    horizon, paths = int(horizon), int(paths)
    if not 1 <= horizon <= max_horizon:
        raise ValueError("horizon must be in [1, %d], got %d" % (max_horizon, horizon))
    if not 1 <= paths <= max_paths:
        raise ValueError("paths must be in [1, %d], got %d" % (max_paths, paths))
    return horizon, paths, OBJECTIVES[objective]


def _closed_loop(env, act, steps, after_step=None):
    """`steps` times ``env.step(act())`` -> (rewards [steps,N] float32, dones [steps,N] bool); after_step(done) follows each step"""
    import torch
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be >= 1")
    R, D = [], []
    for _ in range(steps):
        _, r, d, _ = env.step(act())
        d = torch.as_tensor(d).clone()
        if after_step is not None:
            after_step(d)
        R.append(torch.as_tensor(r).clone()); D.append(d)
    return torch.stack(R), torch.stack(D)


def check_splits(splits, paths):
    """-> None (qs_shooting_plan), 0 ("auto": the library chooses) or the int S in [1, min(paths, 1024)]; ValueError otherwise"""
    if splits is None:
        return None
    if isinstance(splits, str):
        if splits != "auto":
            raise ValueError("splits must be None, \"auto\" or an int, got %r" % (splits,))
        return 0
    if isinstance(splits, (bool, float)):
        raise ValueError("splits must be None, \"auto\" or an int, got %r" % (splits,))
    try:
        s = operator.index(splits)
    except TypeError:
        raise ValueError("splits must be None, \"auto\" or an int, got %r" % (splits,)) from None
    if not 1 <= s <= min(paths, MAX_SPLITS):
        raise ValueError("splits must be in [1, min(paths, %d)] = [1, %d], got %d" % (MAX_SPLITS, min(paths, MAX_SPLITS), s))
    return s


def check_plan_args(horizon, paths, objective, splits=None):
    """-> (horizon, paths, objective id, splits as check_splits returns it); ValueError for what qs_shooting_plan /
    qs_shooting_plan_split would refuse, before anything touches the GPU"""
    horizon, paths, obj = _check_common(horizon, paths, objective, MAX_HORIZON, MAX_PATHS)
    return horizon, paths, obj, check_splits(splits, paths)


def plan_splits(env, paths):
    """the number of parts per env that ``splits="auto"`` gives a plan of `paths` candidates on the handle of `env`
    (qs_shooting_plan_splits; `env` a VecDockingEnv or a single-env shim)"""
    _, paths, _, _ = check_plan_args(1, paths, "reward")
    s = C.c_int32(0)
    env._call("qs_shooting_plan_splits", paths, C.byref(s))
    return int(s.value)


def _torch_arrays(env):
    """the array factory of the device path -> (new(shape, dtype), float32, float64, int32): uninitialised tensors on the env's
    device"""
    import torch
    dev = env.device
    return (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)), torch.float32, torch.float64, torch.int32


def _numpy_arrays():
    """the array factory of the host path, as _torch_arrays: zeroed numpy arrays"""
    import numpy as np
    return np.zeros, np.float32, np.float64, np.int32


def _host_result(out, **as_python):
    """the host path's view of an output dict: the leading env axis (of length 1) stripped"""
    return {k: as_python[k](v[0]) if k in as_python else v[0] for k, v in out.items()}


def _shooting_buffers(arrays, n, horizon, paths, return_scores, return_sequence):
    """-> (the output dict of a shooting plan over n envs, the entry points' buffer arguments) from an array factory"""
    new, f4, f8, i4 = arrays
    out = {"actions": new((n, 4), f4), "best_score": new((n,), f8), "best_index": new((n,), i4)}
    if return_sequence:
        out["sequence"] = new((n, horizon, 4), f4)
    if return_scores:
        out["scores"] = new((n, paths), f8)
    return out, (out["actions"], out["best_score"], out["best_index"], out.get("sequence"), out.get("scores"))


def shooting_plan(env, horizon=20, paths=200, objective="reward", return_scores=False, return_sequence=False, splits=None):
    """One plan for every env of `env` from its current state (the env is not modified).  objective "reward": the sum of the
    step rewards; "position": the reference's ``-sum |rel_pos|^2`` over the observations before each step.  Returns a dict of
    device tensors: actions [N,4] (the best candidate's first action), best_score [N] float64, best_index [N] int32, plus
    sequence [N,horizon,4] and scores [N,paths] float64 on request.  Candidates are keyed by (seed, env id, step counter,
    candidate, horizon step): a plan repeated before the same step is identical, and fewer paths are a prefix of more.
    `splits`: None plans with one workgroup per env (qs_shooting_plan); an int S in [1, min(paths, 1024)] spreads every env's
    candidates over S workgroups and "auto" lets the library choose S (qs_shooting_plan_split).  The results have the same
    bits either way."""
    horizon, paths, obj, splits = check_plan_args(horizon, paths, objective, splits)
    out, bufs = _shooting_buffers(_torch_arrays(env), env.num_envs, horizon, paths, return_scores, return_sequence)
    if splits is None:
        env._call("qs_shooting_plan", horizon, paths, obj, *bufs)
    else:
        env._call("qs_shooting_plan_split", horizon, paths, obj, splits, *bufs)
    return out


def shooting_plan_host(env, horizon=20, paths=200, objective="reward", splits="auto", return_scores=False,
                       return_sequence=False):
    """``shooting_plan`` for the ONE env of a QS_IO_HOST handle (`env` a single-env gym shim): numpy results through the host
    path of qs_shooting_plan_split -- actions [4] float32, best_score (numpy float64), best_index (int), plus sequence
    [horizon,4] and scores [paths] float64 on request.  `splits` None counts as 1: the split entry point is the only one that
    takes host handles, and with one part it launches the kernel of qs_shooting_plan."""
    horizon, paths, obj, splits = check_plan_args(horizon, paths, objective, splits)
    out, bufs = _shooting_buffers(_numpy_arrays(), 1, horizon, paths, return_scores, return_sequence)
    env._call("qs_shooting_plan_split", horizon, paths, obj, 1 if splits is None else splits, *bufs)
    return _host_result(out, best_index=int)


class ShootingMPC:
    """The sampling-based controller as a policy object beside PIDExpert: ``act()`` plans and returns the actions [N,4],
    ``run(steps)`` is the closed loop ``a = act(); env.step(a)``.  Defaults as Mpc_Controller.__init__ (:171); `splits` as in
    ``shooting_plan``."""

    def __init__(self, env, horizon=20, paths=200, objective="reward", splits=None):
        self.horizon, self.paths, _, _ = check_plan_args(horizon, paths, objective, splits)
        self.env, self.objective, self.splits = env, objective, splits
        self.last_plan = None

    def act(self):
        self.last_plan = shooting_plan(self.env, self.horizon, self.paths, self.objective, splits=self.splits)
        return self.last_plan["actions"]

    def run(self, steps):
        """`steps` times plan + env.step -> (rewards [steps,N] float32, dones [steps,N] bool), device tensors"""
        return _closed_loop(self.env, self.act, steps)


def _check_mppi(horizon, paths, iterations, objective, lam, sigma, shift, max_paths):
    import math
    horizon, paths, obj = _check_common(horizon, paths, objective, MPPI_MAX_HORIZON, max_paths)
    iterations = int(iterations)
    if not 1 <= iterations <= MPPI_MAX_ITERATIONS:
        raise ValueError("iterations must be in [1, %d], got %d" % (MPPI_MAX_ITERATIONS, iterations))
    lam, sigma = float(lam), float(sigma)
    if not (lam > 0.0 and math.isfinite(lam)):
        raise ValueError("lam must be positive and finite, got %r" % lam)
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError("sigma must be non-negative and finite, got %r" % sigma)
    if not (isinstance(shift, (bool, int)) and shift in (0, 1)):
        raise ValueError("shift must be False / True (or the int 0 / 1), got %r" % (shift,))
    return horizon, paths, iterations, obj, lam, sigma, int(shift)


def check_mppi_args(horizon, paths, iterations, objective, lam, sigma, shift):
    """-> (horizon, paths, iterations, objective id, lam, sigma, shift as 0 / 1); ValueError for what qs_mppi_plan would
    refuse, before anything touches the GPU"""
    return _check_mppi(horizon, paths, iterations, objective, lam, sigma, shift, MPPI_MAX_PATHS)


def check_mppi_split_args(horizon, paths, iterations, objective, lam, sigma, shift, splits):
    """-> check_mppi_args' tuple plus `splits` as check_splits returns it.  None is qs_mppi_plan and its 4096 paths; with
    `splits` (qs_mppi_plan_split) up to 65536 paths, except that one part is qs_mppi_plan's kernel and keeps its limit"""
    if splits is None:
        return check_mppi_args(horizon, paths, iterations, objective, lam, sigma, shift) + (None,)
    out = _check_mppi(horizon, paths, iterations, objective, lam, sigma, shift, MPPI_SPLIT_MAX_PATHS)
    splits = check_splits(splits, out[1])
    if splits == 1 and out[1] > MPPI_MAX_PATHS:
        raise ValueError("splits=1 plans with qs_mppi_plan's kernel, which takes at most %d paths, got %d" % (MPPI_MAX_PATHS, out[1]))
    return out + (splits,)


def _mppi_buffers(arrays, n, horizon, paths, iterations, nominal, noise, return_scores, return_trace, return_candidates):
    """-> (the output dict of an MPPI plan over n envs, the entry points' buffer arguments) from an array factory"""
    new, f4, f8, _ = arrays
    out = {"actions": new((n, 4), f4), "nominal": new((n, horizon, 4), f4), "best_score": new((n,), f8)}
    if return_scores:
        out["scores"] = new((n, iterations, paths), f8)
    if return_trace:
        out["trace"] = new((n, iterations + 1, horizon, 4), f4)
    if return_candidates:
        out["candidates"] = new((n, paths, horizon, 4), f4)
    return out, (nominal, noise, out["actions"], out["nominal"], out["best_score"], out.get("scores"), out.get("trace"),
                 out.get("candidates"))


def mppi_plan(env, horizon=20, paths=200, iterations=2, objective="reward", lam=MPPI_DEFAULT_LAMBDA, sigma=MPPI_DEFAULT_SIGMA,
              nominal=None, shift=False, noise=None, return_scores=False, return_trace=False, return_candidates=False,
              splits=None):
    """One MPPI plan for every env of `env` from its current state (the env is not modified), `iterations` refinement rounds in
    one launch.  Candidate c >= 1 of a round is clamp(nominal + sigma z, -1, 1), candidate 0 the nominal itself; the new
    nominal is the mean of the candidates weighted by exp((score - best score) / lam).  `nominal` [N,horizon,4] (float32,
    device, contiguous) is the warm start, shifted by one step first if `shift`; None starts from zeros.  It is not written:
    the result is a new tensor.  `noise` [iterations,paths,horizon,4] replaces the keyed in-kernel normals (shared by all envs).
    Returns a dict of device tensors: actions [N,4] (= nominal[:,0]), nominal [N,horizon,4], best_score [N] float64, plus
    scores [N,iterations,paths] float64, trace [N,iterations+1,horizon,4] (the nominal before the first round and after each)
    and candidates [N,paths,horizon,4] (the last round's) on request.  The defaults of `lam` and `sigma` are tuned on one
    setting only (4096 docking-v0 envs, horizon 20, 200 paths x 2 iterations, "reward"; profiles/mppi/README.md).
    `splits`: None plans with one workgroup per env (qs_mppi_plan, at most 4096 paths); an int S in [1, min(paths, 1024)]
    spreads every env's candidates over S workgroups and "auto" lets the library choose S (qs_mppi_plan_split, at most 65536
    paths, three launches per iteration).  S = 1 gives qs_mppi_plan's bits; for S > 1 the scores of the first iteration are
    the same bits and the nominal after an update is within one float32 rounding of the unsplit one, because the order of the
    update's float64 sums depends on S; for a fixed S the plan is reproducible."""
    horizon, paths, iterations, obj, lam, sigma, shift, splits = check_mppi_split_args(horizon, paths, iterations, objective, lam,
                                                                                       sigma, shift, splits)
    import torch
    n, dev = env.num_envs, env.device

    def given(t, shape, name):
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == torch.device(dev)
                and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 tensor of shape %s on %s" % (name, shape, dev))
        return t
    out, bufs = _mppi_buffers(_torch_arrays(env), n, horizon, paths, iterations, given(nominal, (n, horizon, 4), "nominal"),
                              given(noise, (iterations, paths, horizon, 4), "noise"), return_scores, return_trace, return_candidates)
    if splits is None:
        env._call("qs_mppi_plan", horizon, paths, iterations, obj, lam, sigma, shift, *bufs)
    else:
        env._call("qs_mppi_plan_split", horizon, paths, iterations, obj, lam, sigma, shift, splits, *bufs)
    return out


def mppi_plan_host(env, horizon=20, paths=200, iterations=2, objective="reward", lam=MPPI_DEFAULT_LAMBDA, sigma=MPPI_DEFAULT_SIGMA,
                   nominal=None, shift=False, noise=None, splits="auto", return_scores=False, return_trace=False,
                   return_candidates=False):
    """``mppi_plan`` for the ONE env of a QS_IO_HOST handle (`env` a single-env gym shim): numpy in and out through the host
    path of qs_mppi_plan_split -- `nominal` [horizon,4] and `noise` [iterations,paths,horizon,4] float32 arrays or None;
    actions [4] float32, nominal [horizon,4], best_score (numpy float64), plus scores [iterations,paths] float64, trace
    [iterations+1,horizon,4] and candidates [paths,horizon,4] on request.  `splits` None counts as 1: the split entry point is
    the only one that takes host handles, and with one part it launches the kernel of qs_mppi_plan."""
    import numpy as np
    horizon, paths, iterations, obj, lam, sigma, shift, splits = check_mppi_split_args(
        horizon, paths, iterations, objective, lam, sigma, shift, 1 if splits is None else splits)

    def given(a, shape, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != shape:
            raise ValueError("%s must have shape %s, got %s" % (name, shape, a.shape))
        return a
    out, bufs = _mppi_buffers(_numpy_arrays(), 1, horizon, paths, iterations, given(nominal, (horizon, 4), "nominal"),
                              given(noise, (iterations, paths, horizon, 4), "noise"), return_scores, return_trace, return_candidates)
    env._call("qs_mppi_plan_split", horizon, paths, iterations, obj, lam, sigma, shift, splits, *bufs)
    return _host_result(out)


class MPPI:
    """MPPI as a policy object beside ShootingMPC.  The nominal sequence [N,horizon,4] stays on the device between plans:
    ``act()`` plans (shifting the previous nominal by one step after the first call) and returns the actions [N,4];
    ``run(steps)`` is the closed loop ``a = act(); env.step(a)`` and, after each step, zeroes the nominal of the envs whose
    episode ended (one masked op, no host synchronisation); ``reset()`` forgets the nominal.  `lam` and `sigma` default to
    values tuned on one setting only (see ``mppi_plan``); `splits` as in ``mppi_plan``."""

    def __init__(self, env, horizon=20, paths=200, iterations=2, objective="reward", lam=MPPI_DEFAULT_LAMBDA,
                 sigma=MPPI_DEFAULT_SIGMA, splits=None):
        self.horizon, self.paths, self.iterations, _, self.lam, self.sigma, _, _ = check_mppi_split_args(
            horizon, paths, iterations, objective, lam, sigma, False, splits)
        self.env, self.objective, self.splits = env, objective, splits
        self.nominal = None
        self.last_plan = None

    def reset(self):
        self.nominal = None

    def act(self):
        self.last_plan = mppi_plan(self.env, self.horizon, self.paths, self.iterations, self.objective, self.lam, self.sigma,
                                   nominal=self.nominal, shift=self.nominal is not None, splits=self.splits)
        self.nominal = self.last_plan["nominal"]
        return self.last_plan["actions"]

    def run(self, steps):
        """`steps` times plan + env.step -> (rewards [steps,N] float32, dones [steps,N] bool), device tensors"""
        # a new episode starts from a cold nominal
        return _closed_loop(self.env, self.act, steps, lambda d: self.nominal.masked_fill_(d.bool().view(-1, 1, 1), 0.0))
