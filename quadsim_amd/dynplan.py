"""Random-shooting MPC through a LEARNED dynamics net (libquadsim_dyn.so, include/quadsim_dyn.h).

``Mpc_Controller.choose_action(state, dynn)`` of MPC-based_RL.py:170-210 rolls 200 random action sequences of horizon 20 through
``Dynamic_Net`` (:83-136: a 16 -> 200 -> 100 -> 12 ReLU MLP that predicts the normalised observation delta), scores each by
``-sum |rel_pos|^2`` (:203-210) and applies the first action of the first arg-max (:199) -- 20 ``sess.run`` calls per action.
``learned_shooting_plan`` is that planner for N observations at once in one launch (plus one small arg-max launch): it needs an
observation and a net, no env handle and no simulator state.  The candidates are keyed like ``mpc.shooting_plan``'s, so with the
same (seed, env id, step counter) the two planners score the same action sequences.

``DynamicsNet`` holds the weights as torch tensors: ``predict`` is the same formula in plain torch (training and debugging
need no kernel; the fit of the net is the caller's -- examples/mpc_learned.py), ``pack`` builds the padded device image the
kernels read.  ``LearnedShootingMPC`` is the closed loop on a VecDockingEnv or a single-env shim.  Nothing here imports oracle/.

``DynamicsNet.fit`` is Dynamic_Net.train_dynamic (:120-128) on the device: every Adam step of a fit in one launch, through a
fourth library (libquadsim_dynfit.so, include/quadsim_dyn_fit.h).

``learned_mppi_plan`` / ``LearnedMPPI`` are MPPI (``mpc.mppi_plan``'s candidates, weights and update) over the same net and
image, through a third library (libquadsim_dynmppi.so, include/quadsim_dyn_mppi.h).

All three libraries are entries of ``_lib.SIDE``, loaded and called through ``_lib``'s one side-library path.
"""
import ctypes as C
import functools

from . import _lib
from .mpc import MPPI_DEFAULT_LAMBDA, MPPI_DEFAULT_SIGMA

OBS_DIM, ACT_DIM, IN_DIM = 12, 4, 16
MAX_PATHS, MAX_HORIZON, MAX_K = 65536, 1024, 1 << 36
# the compiled (padded) width pairs of k_dyn_plan, cheapest first: a net runs on the first pair that covers it
COMPILED_WIDTHS = ((64, 64), (128, 128), (208, 112))
STD_EPS = 1.0e-6                       # Dynamic_Net.prediction: (s_a - mean) / (std + 1e-6)

# the three libraries bound here are entries of _lib.SIDE: their paths, signatures, loader, status check and call helper are
# _lib's.  The names below stay this module's so that callers and tests can replace a loader
QsdNet, QsdfNet = _lib.QsdNet, _lib.QsdfNet
EXPORTS, MPPI_EXPORTS, FIT_EXPORTS = (_lib.SIDE[key]["exports"] for key in ("dyn", "dynmppi", "dynfit"))
load, load_mppi, load_fit = (functools.partial(_lib.side_load, key) for key in ("dyn", "dynmppi", "dynfit"))
check, check_mppi, check_fit = (functools.partial(_lib.side_check, key) for key in ("dyn", "dynmppi", "dynfit"))


def check_widths(h1, h2):
    """-> (h1, h2, the compiled pair the net runs on); ValueError for widths qsd_net_pack would refuse"""
    h1, h2 = int(h1), int(h2)
    if h1 < 1 or h2 < 1:
        raise ValueError("hidden widths must be >= 1, got (%d, %d)" % (h1, h2))
    for p1, p2 in COMPILED_WIDTHS:
        if h1 <= p1 and h2 <= p2:
            return h1, h2, (p1, p2)
    raise ValueError("hidden widths (%d, %d) are outside the supported range: h1, h2 <= 128, or h1 <= 208 and h2 <= 112" % (h1, h2))


def check_plan_args(horizon, paths, k=0, n=1):
    """-> (horizon, paths, k, n); ValueError for what qsd_shooting_plan would refuse, before anything touches the GPU"""
    horizon, paths, k, n = int(horizon), int(paths), int(k), int(n)
    if not 1 <= horizon <= MAX_HORIZON:
        raise ValueError("horizon must be in [1, %d], got %d" % (MAX_HORIZON, horizon))
    if not 1 <= paths <= MAX_PATHS:
        raise ValueError("paths must be in [1, %d], got %d" % (MAX_PATHS, paths))
    if not 0 <= k < MAX_K:
        raise ValueError("k must be in [0, 2^36), got %d" % k)
    if n < 1:
        raise ValueError("the plan needs at least one observation, got n = %d" % n)
    if n * ((paths + 15) // 16) >= 1 << 31:
        raise ValueError("n * ceil(paths / 16) must be below 2^31, got %d x %d" % (n, (paths + 15) // 16))
    return horizon, paths, k, n


def check_keys(seed, gid0, n):
    """-> (seed, gid0) as ints; ValueError unless they key the candidates of n rows"""
    seed, gid0 = int(seed), int(gid0)
    if not (0 <= seed < 1 << 64 and 0 <= gid0 and gid0 + n <= 1 << 48):
        raise ValueError("seed must fit 64 bits and gid0 + N 48 bits")
    return seed, gid0

# ---------------------------------------------------------------------------------------------------- the fit of the net
# libquadsim_dynfit.so (include/quadsim_dyn_fit.h): a library of its own.  It takes the net's own tensors (DynamicsNet.fit), not
# the packed image.
FIT_MAX_BATCH, FIT_MAX_ITERS, FIT_MAX_K = 256, 4096, 1 << 48
FIT_BETA1, FIT_BETA2, FIT_EPS = 0.9, 0.999, 1.0e-8          # tf.train.AdamOptimizer's defaults


def check_fit_args(h1, h2, capacity, size, iters=100, batch=128, lr=1.0e-4, beta1=FIT_BETA1, beta2=FIT_BETA2, eps=FIT_EPS, t0=0, seed=0, k=0):
    """-> (size, iters, batch, lr, beta1, beta2, eps, t0, seed, k); ValueError for what qsdf_fit would refuse, before anything
    touches the library or the GPU"""
    check_widths(h1, h2)
    capacity, size, iters, batch, t0, seed, k = int(capacity), int(size), int(iters), int(batch), int(t0), int(seed), int(k)
    if not 1 <= batch <= FIT_MAX_BATCH:
        raise ValueError("batch must be in [1, %d], got %d" % (FIT_MAX_BATCH, batch))
    if not 1 <= iters <= FIT_MAX_ITERS:
        raise ValueError("iters must be in [1, %d], got %d" % (FIT_MAX_ITERS, iters))
    if not 1 <= capacity < 1 << 31:
        raise ValueError("capacity must be in [1, 2^31), got %d" % capacity)
    if not 1 <= size <= capacity:
        raise ValueError("size must be in [1, capacity = %d], got %d" % (capacity, size))
    lr, beta1, beta2, eps = _lib.check_adam_args(lr, beta1, beta2, eps, t0, iters, "iters")
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits, got %d" % seed)
    if not 0 <= k < FIT_MAX_K:
        raise ValueError("k must be in [0, 2^48), got %d" % k)
    return size, iters, batch, lr, beta1, beta2, eps, t0, seed, k


class DynamicsNet:
    """Dynamic_Net (MPC-based_RL.py:83-136): 16 -> h1 -> h2 -> 12, ReLU, on normalised inputs and outputs.  The weights are
    float32 torch tensors in torch's Linear layout (out, in): w1 [h1,16], b1 [h1], w2 [h2,h1], b2 [h2], w3 [12,h2], b3 [12];
    the normalisers in_mean / in_std [16] and out_mean / out_std [12] (zeros / ones until ``set_normalisers``).  A fresh net is
    initialised as the reference's (:97-105: N(0, 0.1) kernels, 0.1 biases; the output layer Glorot-uniform with zero bias)."""

    WEIGHTS = ("w1", "b1", "w2", "b2", "w3", "b3")

    def __init__(self, h1=200, h2=100, device="cuda", seed=0):
        import torch
        self.h1, self.h2, self.compiled = check_widths(h1, h2)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:     # tensors report an indexed device
            self.device = torch.device("cuda", torch.cuda.current_device())
        g = torch.Generator().manual_seed(int(seed))
        lim = (6.0 / (self.h2 + OBS_DIM)) ** 0.5
        init = {"w1": torch.randn(self.h1, IN_DIM, generator=g) * 0.1, "b1": torch.full((self.h1,), 0.1),
                "w2": torch.randn(self.h2, self.h1, generator=g) * 0.1, "b2": torch.full((self.h2,), 0.1),
                "w3": (torch.rand(OBS_DIM, self.h2, generator=g) * 2.0 - 1.0) * lim, "b3": torch.zeros(OBS_DIM)}
        for k, v in init.items():
            setattr(self, k, v.to(self.device, torch.float32).contiguous())
        self._image, self._image_key = None, None
        self.adam_m, self.adam_v, self.fit_steps = None, None, 0
        self.set_normalisers()

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, w1, b1, w2, b2, w3, b3, device="cuda"):
        """weights in the (out, in) layout from anything ``torch.as_tensor`` takes; the widths are read off the shapes"""
        import torch
        t = [torch.as_tensor(a).detach().to(torch.float32) for a in (w1, b1, w2, b2, w3, b3)]
        h1, h2 = int(t[0].shape[0]), int(t[2].shape[0])
        want = [(h1, IN_DIM), (h1,), (h2, h1), (h2,), (OBS_DIM, h2), (OBS_DIM,)]
        for name, a, shape in zip(cls.WEIGHTS, t, want):
            if tuple(a.shape) != shape:
                raise ValueError("%s must have shape %s, got %s" % (name, shape, tuple(a.shape)))
        net = cls(h1, h2, device)
        for name, a in zip(cls.WEIGHTS, t):
            setattr(net, name, a.to(net.device).contiguous().clone())
        return net

    @classmethod
    def from_torch(cls, module, device="cuda"):
        """from a torch module whose three ``torch.nn.Linear`` layers, in order, are the net (ReLU between them)"""
        import torch
        lin = [m for m in module.modules() if isinstance(m, torch.nn.Linear)]
        if len(lin) != 3 or any(m.bias is None for m in lin):
            raise ValueError("expected a module with exactly three biased Linear layers, found %d" % len(lin))
        return cls.from_arrays(lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias, device=device)

    def set_normalisers(self, in_mean=None, in_std=None, out_mean=None, out_std=None):
        """obs_action_mean / obs_action_std [16] and delta_mean / delta_std [12] of the reference (None: zeros / ones).  The
        input scale is kept as in_rscale = 1 / (in_std + 1e-6), computed in float64 and rounded once."""
        import numpy as np
        import torch

        def arr(a, n, fill):
            a = np.full(n, fill, np.float64) if a is None else np.asarray(
                a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float64).reshape(-1)
            if a.shape != (n,):
                raise ValueError("a normaliser has %d elements, expected %d" % (a.size, n))
            return a
        vals = {"in_mean": arr(in_mean, IN_DIM, 0.0), "in_rscale": 1.0 / (arr(in_std, IN_DIM, 1.0) + STD_EPS),
                "out_mean": arr(out_mean, OBS_DIM, 0.0), "out_std": arr(out_std, OBS_DIM, 1.0)}
        vals["out_rscale"] = 1.0 / (vals["out_std"] + STD_EPS)     # the scale of the fit's target, kept as in_rscale is
        for k, v in vals.items():
            setattr(self, k, torch.as_tensor(v.astype(np.float32)).to(self.device).contiguous())
        self._image_key = None
        return self

    def parameters(self):
        """the six weight tensors (what an optimiser trains; set ``requires_grad_`` on them for a fit)"""
        return [getattr(self, k) for k in self.WEIGHTS]

    # ------------------------------------------------------------------ the formula in plain torch
    def predict(self, obs, act):
        """Dynamic_Net.prediction (:130-136) for obs [...,12] and act [...,4] -> the next observation [...,12], computed in the
        dtype of `obs` with the operations of the kernel's contract: (x - mean) * rscale, three Linear layers with ReLU,
        delta * out_std + out_mean + obs"""
        return self.delta_to_obs(self.predict_delta(obs, act), obs)

    def predict_delta(self, obs, act):
        """the net's output: the normalised delta [...,12] (what the reference's loss compares with (delta - mean) / std)"""
        import torch
        dt = obs.dtype
        c = lambda k: getattr(self, k).to(device=obs.device, dtype=dt)     # noqa: E731
        x = (torch.cat([obs, act.to(dt)], dim=-1) - c("in_mean")) * c("in_rscale")
        h = torch.relu(torch.nn.functional.linear(x, c("w1"), c("b1")))
        h = torch.relu(torch.nn.functional.linear(h, c("w2"), c("b2")))
        return torch.nn.functional.linear(h, c("w3"), c("b3"))

    def delta_to_obs(self, delta, obs):
        c = lambda k: getattr(self, k).to(device=obs.device, dtype=obs.dtype)     # noqa: E731
        return delta * c("out_std") + c("out_mean") + obs

    # ------------------------------------------------------------------ the device image
    def _tensors(self):
        return [getattr(self, k) for k in self.WEIGHTS + ("in_mean", "in_rscale", "out_std", "out_mean")]

    def pack(self):
        """-> the padded device image (a torch uint8 tensor the net owns), rebuilt by qsd_net_pack on the current stream when a
        weight or a normaliser has changed (in place or by assignment) since the last call"""
        import torch
        if self.device.type != "cuda":
            raise _lib.QuadsimError("DynamicsNet.pack needs the net on a HIP device, it is on %s; there is no CPU path" % self.device)
        ts = self._tensors()
        key = tuple((_lib.as_arg(t), t._version) for t in ts)
        if self._image is not None and key == self._image_key:
            return self._image
        for k, t in zip(self.WEIGHTS + ("in_mean", "in_rscale", "out_std", "out_mean"), ts):
            _lib.check_tensor(k, t, "float32", None, self.device)
        lib = load()
        if self._image is None:
            nbytes = C.c_size_t(0)
            _lib.side_call("dyn", lib, "qsd_net_image_bytes", self.h1, self.h2, C.byref(nbytes))
            self._image = _lib.new_tensor(self.device, (int(nbytes.value),), "uint8")
        net = QsdNet(C.sizeof(QsdNet), self.h1, self.h2, 0, *map(_lib.as_arg, ts))
        _lib.side_call("dyn", lib, "qsd_net_pack", C.byref(net), self._image, device=self.device)
        self._image_key = key
        return self._image

    # ------------------------------------------------------------------ the fit on the device
    def reset_optimizer(self):
        """forget Adam's moments and the step count (``fit`` creates them again, zeros, on its next call)"""
        self.adam_m, self.adam_v, self.fit_steps = None, None, 0

    def fit(self, buf_x, buf_d, size, iters=100, batch=128, lr=1.0e-4, seed=0, indices=None, return_indices=False, return_grads=False,
            k=None, beta1=FIT_BETA1, beta2=FIT_BETA2, eps=FIT_EPS):
        """Dynamic_Net.train_dynamic (MPC-based_RL.py:120-128) in ONE launch (qsdf_fit of libquadsim_dynfit.so): `iters` Adam
        steps (tf.train.AdamOptimizer's formula) on batches of `batch` rows drawn with replacement from the first `size` rows of
        buf_x [capacity,16] (observation and action) / buf_d [capacity,12] (delta), contiguous float32 tensors on the net's
        device.  The weights, ``adam_m`` / ``adam_v`` (lists of six tensors, zeros on first use) and ``fit_steps`` are updated
        in place; the draws are keyed by (seed, k, Adam step, row), k = ``fit_steps`` at the call unless given, or replaced
        by `indices` [iters,batch] int32.  Returns a dict of device tensors: loss [iters] (the batch loss before each step), plus
        indices [iters,batch] int32 and grads (the six gradients of the last iteration) on request.  Launched on torch's current
        stream; nothing synchronises with the host.  A repeated fit from the same state gives the same bits."""
        import torch
        if self.device.type != "cuda":
            raise _lib.QuadsimError("DynamicsNet.fit needs the net on a HIP device, it is on %s; there is no CPU path" % self.device)
        _lib.check_tensor("buf_x", buf_x, "float32", ("capacity", IN_DIM), self.device)
        _lib.check_tensor("buf_d", buf_d, "float32", ("capacity", OBS_DIM), self.device)
        if buf_x.shape[0] != buf_d.shape[0]:
            raise ValueError("buf_x and buf_d must have the same capacity, got %d and %d" % (buf_x.shape[0], buf_d.shape[0]))
        k = self.fit_steps if k is None else k
        size, iters, batch, lr, beta1, beta2, eps, t0, seed, k = check_fit_args(
            self.h1, self.h2, buf_x.shape[0], size, iters, batch, lr, beta1, beta2, eps, self.fit_steps, seed, k)
        if indices is not None:
            _lib.check_tensor("indices", indices, "int32", (iters, batch), self.device)
        ws = self.parameters()
        norms = [self.in_mean, self.in_rscale, self.out_mean, self.out_rscale]
        for name, t in zip(self.WEIGHTS + ("in_mean", "in_rscale", "out_mean", "out_rscale"), ws + norms):
            _lib.check_tensor(name, t, "float32", None, self.device)
        if self.adam_m is None:
            self.adam_m, self.adam_v = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
        out = {"loss": _lib.new_tensor(self.device, (iters,), "float32")}
        if return_indices:
            out["indices"] = _lib.new_tensor(self.device, (iters, batch), "int32")
        if return_grads:
            out["grads"] = [torch.empty_like(w) for w in ws]
        net = QsdfNet(C.sizeof(QsdfNet), self.h1, self.h2, 0, _lib.six(ws), _lib.six(self.adam_m), _lib.six(self.adam_v), *map(_lib.as_arg, norms))
        _lib.side_call("dynfit", load_fit(), "qsdf_fit", C.byref(net), buf_x, buf_d, buf_x.shape[0], size, iters, batch, lr, beta1, beta2, eps,
                       t0, seed, k, indices, out["loss"], out.get("indices"), _lib.six(out["grads"]) if return_grads else None,
                       device=self.device)
        self.fit_steps += iters
        self._image_key = None        # the kernel wrote the weights behind torch's back: their _version did not move
        return out


def learned_shooting_plan(net, obs, horizon=20, paths=200, seed=0, k=0, gid0=0, return_scores=False, return_sequence=False,
                          return_traj=False):
    """One plan per row of `obs` [N,12] (a contiguous float32 tensor on the net's device) through `net`.  Returns a dict of
    device tensors: actions [N,4] (the best candidate's first action), best_score [N] float64, best_index [N] int32, plus
    sequence [N,horizon,4], scores [N,paths] float64 and traj [N,paths,horizon,12] (traj[:, c, h] = the prediction after step
    h) on request.  Candidate c of row i is keyed by (seed, gid0 + i, k, c, horizon step): a repeated plan is identical, fewer
    paths are a prefix of more, and a row planned alone equals the same row (same gid) inside a batch, bit for bit.  Launched on
    torch's current stream; nothing synchronises with the host."""
    import torch
    if not isinstance(net, DynamicsNet):
        raise ValueError("net must be a DynamicsNet, got %r" % type(net).__name__)
    _lib.check_tensor("obs", obs, "float32", ("N", OBS_DIM), net.device)
    horizon, paths, k, n = check_plan_args(horizon, paths, k, obs.shape[0])
    seed, gid0 = check_keys(seed, gid0, n)
    image = net.pack()
    new = functools.partial(_lib.new_tensor, net.device)
    out = {"actions": new((n, 4), "float32"), "best_score": new((n,), "float64"), "best_index": new((n,), "int32")}
    if return_sequence:
        out["sequence"] = new((n, horizon, 4), "float32")
    if return_scores:
        out["scores"] = new((n, paths), "float64")
    if return_traj:
        out["traj"] = new((n, paths, horizon, OBS_DIM), "float32")
    lib = load()
    nbytes = C.c_size_t(0)
    _lib.side_call("dyn", lib, "qsd_plan_workspace_bytes", n, paths, C.byref(nbytes))
    _lib.side_call("dyn", lib, "qsd_shooting_plan", image, n, obs, seed, gid0, k, horizon, paths, new((int(nbytes.value),), "uint8"),
                   out["actions"], out["best_score"], out["best_index"], out.get("sequence"), out.get("scores"), out.get("traj"),
                   device=net.device)
    return out


class LearnedShootingMPC:
    """``ShootingMPC`` with a learned model: ``act()`` plans from the env's LAST observation and returns the actions,
    ``run(steps)`` is the closed loop ``a = act(); env.step(a)``.  The step counter of the env is `k`, its seed and env id
    offset key the candidates, so with the same env the candidates are those of ``ShootingMPC``.  `env` is a VecDockingEnv
    (device tensors in and out) or a single-env shim such as DockingEnv (numpy at the boundary: ``act()`` returns float32 [4]).
    Defaults as Mpc_Controller.__init__ (:171)."""

    def __init__(self, env, net, horizon=20, paths=200):
        self.horizon, self.paths, _, _ = check_plan_args(horizon, paths)
        if not isinstance(net, DynamicsNet):
            raise ValueError("net must be a DynamicsNet, got %r" % type(net).__name__)
        self.env, self.net = env, net
        self.single = not hasattr(env, "num_envs")
        self.last_plan = None

    def _inputs(self):
        import torch
        env = self.env
        k = C.c_uint64(0)
        env._call("qs_get_step_counter", C.byref(k))
        if self.single:
            import numpy as np
            obs = torch.as_tensor(np.asarray(env.rel_state, np.float32).reshape(1, OBS_DIM)).to(self.net.device)
        else:
            if not env._follow_torch_stream:
                env.sync()                                 # an owned stream is not ordered with torch's
            obs = env._obs
            if obs.shape[1] != OBS_DIM:
                raise ValueError("the learned planner takes docking observations [N, %d], the env gives [N, %d]" % (OBS_DIM, obs.shape[1]))
        return obs.contiguous(), int(env.cfg.seed), int(k.value), int(env.cfg.env_id_offset)

    def act(self):
        obs, seed, k, gid0 = self._inputs()
        self.last_plan = learned_shooting_plan(self.net, obs, self.horizon, self.paths, seed=seed, k=k, gid0=gid0)
        a = self.last_plan["actions"]
        return a[0].cpu().numpy() if self.single else a

    def run(self, steps):
        """`steps` times plan + env.step -> (rewards [steps,N] float32, dones [steps,N] bool), device tensors (a single-env shim:
        [steps,1] on the host; its step never resets, so stop at the first done yourself)"""
        from .mpc import _closed_loop
        if not self.single:
            return _closed_loop(self.env, self.act, steps, self._after_step)
        import torch
        R, D = [], []
        for _ in range(int(steps)):
            _, r, d, _ = self.env.step(self.act())
            if self._after_step is not None:
                self._after_step(d)
            R.append([float(r)]); D.append([bool(d)])
        return torch.tensor(R, dtype=torch.float32), torch.tensor(D, dtype=torch.bool)

    _after_step = None      # the per-done hook of mpc._closed_loop: a planner with state between plans defines it


# ---------------------------------------------------------------------------------------------------- MPPI over the net
# libquadsim_dynmppi.so (include/quadsim_dyn_mppi.h): a library of its own, bound here beside the shooting planner's.  It takes
# the image that DynamicsNet.pack builds and the net's widths; nothing of libquadsim_dyn.so's host state.
MPPI_MAX_ITERATIONS, MPPI_MAX_K = 16, 1 << 33

def check_mppi_plan_args(horizon, paths, iterations, lam, sigma, shift=False, k=0, n=1):
    """-> (horizon, paths, iterations, lam, sigma, shift as 0 / 1, k, n); ValueError for what qsdm_mppi_plan would refuse, before
    anything touches the library or the GPU"""
    import math
    horizon, paths, _, n = check_plan_args(horizon, paths, 0, n)
    iterations, k = int(iterations), int(k)
    if not 1 <= iterations <= MPPI_MAX_ITERATIONS:
        raise ValueError("iterations must be in [1, %d], got %d" % (MPPI_MAX_ITERATIONS, iterations))
    if not 0 <= k < MPPI_MAX_K:
        raise ValueError("k must be in [0, 2^33), got %d" % k)
    lam, sigma = float(lam), float(sigma)
    if not (lam > 0.0 and math.isfinite(lam)):
        raise ValueError("lam must be positive and finite, got %r" % lam)
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError("sigma must be >= 0 and finite, got %r" % sigma)
    if isinstance(shift, bool):
        shift = int(shift)
    if shift not in (0, 1) or isinstance(shift, float):
        raise ValueError("shift must be False / True (0 / 1), got %r" % (shift,))
    return horizon, paths, iterations, lam, sigma, int(shift), k, n


def learned_mppi_plan(net, obs, horizon=20, paths=200, iterations=2, lam=MPPI_DEFAULT_LAMBDA, sigma=MPPI_DEFAULT_SIGMA, nominal=None,
                      shift=False, noise=None, seed=0, k=0, gid0=0, return_scores=False, return_trace=False, return_candidates=False,
                      return_traj=False):
    """One MPPI plan per row of `obs` [N,12] (a contiguous float32 tensor on the net's device) through `net`: `iterations`
    rounds of `paths` Gaussian candidates (standard deviation `sigma`, clamped to [-1, 1]) around the nominal action sequence,
    rolled through the net and scored by position as ``learned_shooting_plan`` scores them; after each round the nominal becomes
    the mean of the candidates weighted by exp((score - best) / lam).  `nominal` [N,horizon,4] warm-starts the plan (zeros
    without it), read one step ahead with `shift`; `noise` [iterations,paths,horizon,4] replaces the keyed draws (shared by the
    rows).  Returns a dict of device tensors: actions [N,4] (= nominal[:, 0]), nominal [N,horizon,4], best_score [N] float64,
    plus scores [N,iterations,paths] float64, trace [N,iterations+1,horizon,4], candidates [N,paths,horizon,4] and traj
    [N,paths,horizon,12] (both of the last round) on request.  The draws are keyed by (seed, gid0 + i, k, round, candidate,
    step) as ``mpc.mppi_plan``'s: a repeated plan is identical, and a row planned alone equals the same row (same gid) inside a
    batch, bit for bit.  2 x iterations launches on torch's current stream; nothing synchronises with the host.

    The defaults of `lam` and `sigma` are ``mpc.mppi_plan``'s, tuned on the exact simulator's REWARD objective; they were not
    tuned on this position score or on a learned model and are untuned here."""
    import torch
    if not isinstance(net, DynamicsNet):
        raise ValueError("net must be a DynamicsNet, got %r" % type(net).__name__)
    _lib.check_tensor("obs", obs, "float32", ("N", OBS_DIM), net.device)
    horizon, paths, iterations, lam, sigma, shift, k, n = check_mppi_plan_args(horizon, paths, iterations, lam, sigma, shift, k, obs.shape[0])
    seed, gid0 = check_keys(seed, gid0, n)
    for name, t, shape in (("nominal", nominal, (n, horizon, 4)), ("noise", noise, (iterations, paths, horizon, 4))):
        if t is not None:
            _lib.check_tensor(name, t, "float32", shape, net.device)
    image = net.pack()
    new = functools.partial(_lib.new_tensor, net.device)
    out = {"actions": new((n, 4), "float32"), "nominal": new((n, horizon, 4), "float32"), "best_score": new((n,), "float64")}
    if return_scores:
        out["scores"] = new((n, iterations, paths), "float64")
    if return_trace:
        out["trace"] = new((n, iterations + 1, horizon, 4), "float32")
    if return_candidates:
        out["candidates"] = new((n, paths, horizon, 4), "float32")
    if return_traj:
        out["traj"] = new((n, paths, horizon, OBS_DIM), "float32")
    lib = load_mppi()
    nbytes = C.c_size_t(0)
    _lib.side_call("dynmppi", lib, "qsdm_workspace_bytes", n, horizon, paths, C.byref(nbytes))
    _lib.side_call("dynmppi", lib, "qsdm_mppi_plan", image, net.h1, net.h2, n, obs, seed, gid0, k, horizon, paths, iterations, lam, sigma, shift,
                   nominal, noise, new((int(nbytes.value),), "uint8"), out["actions"], out["nominal"], out["best_score"], out.get("scores"),
                   out.get("trace"), out.get("candidates"), out.get("traj"), device=net.device)
    return out


class LearnedMPPI(LearnedShootingMPC):
    """``mpc.MPPI`` with a learned model, with the interface of ``LearnedShootingMPC``: ``act()`` plans from the env's LAST
    observation (shifting the previous nominal by one step after the first call) and returns the actions; ``run(steps)`` is the
    closed loop ``a = act(); env.step(a)`` and, after each step, zeroes the nominal of the envs whose episode ended;
    ``reset()`` forgets the nominal.  The nominal [N,horizon,4] stays on the device between plans.  `env` is a VecDockingEnv or
    a single-env shim.  `lam` and `sigma` default to ``mpc.mppi_plan``'s values, which were tuned on the exact simulator's reward
    and are untuned for this planner."""

    def __init__(self, env, net, horizon=20, paths=200, iterations=2, lam=MPPI_DEFAULT_LAMBDA, sigma=MPPI_DEFAULT_SIGMA):
        super().__init__(env, net, horizon, paths)
        _, _, self.iterations, self.lam, self.sigma, _, _, _ = check_mppi_plan_args(horizon, paths, iterations, lam, sigma)
        self.nominal = None

    def reset(self):
        self.nominal = None

    def act(self):
        obs, seed, k, gid0 = self._inputs()
        self.last_plan = learned_mppi_plan(self.net, obs, self.horizon, self.paths, self.iterations, self.lam, self.sigma,
                                           nominal=self.nominal, shift=self.nominal is not None, seed=seed, k=k, gid0=gid0)
        self.nominal = self.last_plan["nominal"]
        a = self.last_plan["actions"]
        return a[0].cpu().numpy() if self.single else a

    def _after_step(self, d):
        """``run`` is ``LearnedShootingMPC.run``; a new episode starts from a cold nominal"""
        if not self.single:
            self.nominal.masked_fill_(d.bool().view(-1, 1, 1), 0.0)
        elif d:
            self.nominal.zero_()
