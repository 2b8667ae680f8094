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
fourth library (libquadsim_dynfit.so, include/quadsim_dyn_fit.h) bound above the class.

``learned_mppi_plan`` / ``LearnedMPPI`` are MPPI (``mpc.mppi_plan``'s candidates, weights and update) over the same net and
image, through a third library (libquadsim_dynmppi.so, include/quadsim_dyn_mppi.h) bound at the end of this module.
"""
import ctypes as C
import os

from . import _lib
from .mpc import MPPI_DEFAULT_LAMBDA, MPPI_DEFAULT_SIGMA

OBS_DIM, ACT_DIM, IN_DIM = 12, 4, 16
MAX_PATHS, MAX_HORIZON, MAX_K = 65536, 1024, 1 << 36
# the compiled (padded) width pairs of k_dyn_plan, cheapest first: a net runs on the first pair that covers it
COMPILED_WIDTHS = ((64, 64), (128, 128), (208, 112))
STD_EPS = 1.0e-6                       # Dynamic_Net.prediction: (s_a - mean) / (std + 1e-6)

EXPORTS = ["qsd_version", "qsd_last_error", "qsd_net_image_bytes", "qsd_net_pack", "qsd_plan_workspace_bytes", "qsd_shooting_plan"]


class QsdNet(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("h1", C.c_int32), ("h2", C.c_int32), ("reserved", C.c_int32)] + [
        (k, C.c_void_p) for k in ("wt1", "b1", "wt2", "b2", "wt3", "b3", "in_mean", "in_rscale", "out_std", "out_mean")]


_dyn = None


def load():
    """dlopen libquadsim_dyn.so; raises QuadsimError if it has not been built (there is no fallback)"""
    global _dyn
    if _dyn is not None:
        return _dyn
    if not os.path.exists(_lib.DYN_LIB_PATH):
        raise _lib.QuadsimError("%s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'`." % _lib.DYN_LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime must be the resident one: see _lib.load)
    lib = C.CDLL(_lib.DYN_LIB_PATH)
    vp, i64, u64, i32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32
    sig = {
        "qsd_version": [],
        "qsd_net_image_bytes": [i32, i32, C.POINTER(C.c_size_t)],
        "qsd_net_pack": [C.POINTER(QsdNet), vp, vp],
        "qsd_plan_workspace_bytes": [i64, i32, C.POINTER(C.c_size_t)],
        "qsd_shooting_plan": [vp, i64, vp, u64, u64, u64, i32, i32] + [vp] * 8,
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    lib.qsd_last_error.argtypes, lib.qsd_last_error.restype = [], C.c_char_p
    _dyn = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise _lib.QuadsimError("%s failed (%d): %s" % (what, rc, load().qsd_last_error().decode("utf-8", "replace")))


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

# ---------------------------------------------------------------------------------------------------- the fit of the net
# libquadsim_dynfit.so (include/quadsim_dyn_fit.h): a library of its own.  It takes the net's own tensors (DynamicsNet.fit), not
# the packed image.
FIT_EXPORTS = ["qsdf_version", "qsdf_last_error", "qsdf_fit"]
FIT_MAX_BATCH, FIT_MAX_ITERS, FIT_MAX_K = 256, 4096, 1 << 48
FIT_BETA1, FIT_BETA2, FIT_EPS = 0.9, 0.999, 1.0e-8          # tf.train.AdamOptimizer's defaults


class QsdfNet(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("h1", C.c_int32), ("h2", C.c_int32), ("reserved", C.c_int32),
                ("w", C.c_void_p * 6), ("m", C.c_void_p * 6), ("v", C.c_void_p * 6)] + [
        (k, C.c_void_p) for k in ("in_mean", "in_rscale", "out_mean", "out_rscale")]


_dynfit = None


def load_fit():
    """dlopen libquadsim_dynfit.so; raises QuadsimError if it has not been built (there is no fallback)"""
    global _dynfit
    if _dynfit is not None:
        return _dynfit
    if not os.path.exists(_lib.DYNFIT_LIB_PATH):
        raise _lib.QuadsimError("%s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'`." % _lib.DYNFIT_LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime must be the resident one: see _lib.load)
    lib = C.CDLL(_lib.DYNFIT_LIB_PATH)
    vp, i64, u64, i32, f64 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_double
    lib.qsdf_version.argtypes, lib.qsdf_version.restype = [], C.c_int
    lib.qsdf_fit.argtypes = [C.POINTER(QsdfNet), vp, vp, i64, i64, i32, i32, f64, f64, f64, f64, i64, u64, u64, vp, vp, vp,
                             C.POINTER(C.c_void_p * 6), vp]
    lib.qsdf_fit.restype = C.c_int
    lib.qsdf_last_error.argtypes, lib.qsdf_last_error.restype = [], C.c_char_p
    _dynfit = lib
    return lib


def check_fit(rc, what):
    if rc != 0:
        raise _lib.QuadsimError("%s failed (%d): %s" % (what, rc, load_fit().qsdf_last_error().decode("utf-8", "replace")))


def check_fit_args(h1, h2, capacity, size, iters=100, batch=128, lr=1.0e-4, beta1=FIT_BETA1, beta2=FIT_BETA2, eps=FIT_EPS, t0=0, seed=0, k=0):
    """-> (size, iters, batch, lr, beta1, beta2, eps, t0, seed, k); ValueError for what qsdf_fit would refuse, before anything
    touches the library or the GPU"""
    import math
    check_widths(h1, h2)
    capacity, size, iters, batch, t0, seed, k = int(capacity), int(size), int(iters), int(batch), int(t0), int(seed), int(k)
    lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
    if not 1 <= batch <= FIT_MAX_BATCH:
        raise ValueError("batch must be in [1, %d], got %d" % (FIT_MAX_BATCH, batch))
    if not 1 <= iters <= FIT_MAX_ITERS:
        raise ValueError("iters must be in [1, %d], got %d" % (FIT_MAX_ITERS, iters))
    if not 1 <= capacity < 1 << 31:
        raise ValueError("capacity must be in [1, 2^31), got %d" % capacity)
    if not 1 <= size <= capacity:
        raise ValueError("size must be in [1, capacity = %d], got %d" % (capacity, size))
    if not (t0 >= 0 and t0 + iters < 1 << 31):
        raise ValueError("t0 must be >= 0 with t0 + iters below 2^31, got %d" % t0)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits, got %d" % seed)
    if not 0 <= k < FIT_MAX_K:
        raise ValueError("k must be in [0, 2^48), got %d" % k)
    for name, val in (("lr", lr), ("eps", eps)):
        if not math.isfinite(val):
            raise ValueError("%s must be finite, got %r" % (name, val))
    for name, val in (("beta1", beta1), ("beta2", beta2)):
        if not 0.0 <= val < 1.0:
            raise ValueError("%s must be in [0, 1), got %r" % (name, val))
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
        key = tuple((t.data_ptr(), t._version) for t in ts)
        if self._image is not None and key == self._image_key:
            return self._image
        for k, t in zip(self.WEIGHTS + ("in_mean", "in_rscale", "out_std", "out_mean"), ts):
            if not (t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 tensor on %s" % (k, self.device))
        lib = load()
        if self._image is None:
            nbytes = C.c_size_t(0)
            check(lib.qsd_net_image_bytes(self.h1, self.h2, C.byref(nbytes)), "qsd_net_image_bytes")
            self._image = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        net = QsdNet(C.sizeof(QsdNet), self.h1, self.h2, 0, *[t.data_ptr() for t in ts])
        with torch.cuda.device(self.device):
            check(lib.qsd_net_pack(C.byref(net), C.c_void_p(self._image.data_ptr()),
                                   C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "qsd_net_pack")
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
        for name, t, cols in (("buf_x", buf_x, IN_DIM), ("buf_d", buf_d, OBS_DIM)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == cols
                    and t.device == self.device and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 tensor of shape [capacity, %d] on %s" % (name, cols, self.device))
        if buf_x.shape[0] != buf_d.shape[0]:
            raise ValueError("buf_x and buf_d must have the same capacity, got %d and %d" % (buf_x.shape[0], buf_d.shape[0]))
        k = self.fit_steps if k is None else k
        size, iters, batch, lr, beta1, beta2, eps, t0, seed, k = check_fit_args(
            self.h1, self.h2, buf_x.shape[0], size, iters, batch, lr, beta1, beta2, eps, self.fit_steps, seed, k)
        if indices is not None and not (isinstance(indices, torch.Tensor) and indices.dtype == torch.int32 and tuple(indices.shape) == (iters, batch)
                                        and indices.device == self.device and indices.is_contiguous()):
            raise ValueError("indices must be a contiguous int32 tensor of shape [%d, %d] on %s" % (iters, batch, self.device))
        ws = self.parameters()
        for name, t in zip(self.WEIGHTS + ("in_mean", "in_rscale", "out_mean", "out_rscale"), self._tensors()[:8] + [self.out_mean, self.out_rscale]):
            if not (t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 tensor on %s" % (name, self.device))
        if self.adam_m is None:
            self.adam_m, self.adam_v = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=self.device)     # noqa: E731
        out = {"loss": new((iters,), torch.float32)}
        if return_indices:
            out["indices"] = new((iters, batch), torch.int32)
        grads = None
        if return_grads:
            out["grads"] = [torch.empty_like(w) for w in ws]
            grads = (C.c_void_p * 6)(*[g.data_ptr() for g in out["grads"]])
        six = lambda ts: (C.c_void_p * 6)(*[t.data_ptr() for t in ts])     # noqa: E731
        net = QsdfNet(C.sizeof(QsdfNet), self.h1, self.h2, 0, six(ws), six(self.adam_m), six(self.adam_v), self.in_mean.data_ptr(),
                      self.in_rscale.data_ptr(), self.out_mean.data_ptr(), self.out_rscale.data_ptr())
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
        lib = load_fit()
        with torch.cuda.device(self.device):
            check_fit(lib.qsdf_fit(C.byref(net), p(buf_x), p(buf_d), buf_x.shape[0], size, iters, batch, lr, beta1, beta2, eps, t0, seed, k,
                                   p(indices), p(out["loss"]), p(out.get("indices")), grads,
                                   C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "qsdf_fit")
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
    if not (isinstance(obs, torch.Tensor) and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == OBS_DIM
            and obs.device == net.device and obs.is_contiguous()):
        raise ValueError("obs must be a contiguous float32 tensor of shape [N, %d] on %s" % (OBS_DIM, net.device))
    horizon, paths, k, n = check_plan_args(horizon, paths, k, obs.shape[0])
    seed, gid0 = int(seed), int(gid0)
    if not (0 <= seed < 1 << 64 and 0 <= gid0 and gid0 + n <= 1 << 48):
        raise ValueError("seed must fit 64 bits and gid0 + N 48 bits")
    image = net.pack()
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=net.device)     # noqa: E731
    out = {"actions": new((n, 4), torch.float32), "best_score": new((n,), torch.float64), "best_index": new((n,), torch.int32)}
    if return_sequence:
        out["sequence"] = new((n, horizon, 4), torch.float32)
    if return_scores:
        out["scores"] = new((n, paths), torch.float64)
    if return_traj:
        out["traj"] = new((n, paths, horizon, OBS_DIM), torch.float32)
    lib = load()
    nbytes = C.c_size_t(0)
    check(lib.qsd_plan_workspace_bytes(n, paths, C.byref(nbytes)), "qsd_plan_workspace_bytes")
    work = new((int(nbytes.value),), torch.uint8)         # torch's caching allocator: no device allocation in steady state
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
    with torch.cuda.device(net.device):
        check(lib.qsd_shooting_plan(p(image), n, p(obs), seed, gid0, k, horizon, paths, p(work), p(out["actions"]), p(out["best_score"]),
                                    p(out["best_index"]), p(out.get("sequence")), p(out.get("scores")), p(out.get("traj")),
                                    C.c_void_p(torch.cuda.current_stream(net.device).cuda_stream)), "qsd_shooting_plan")
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
            return _closed_loop(self.env, self.act, steps)
        import torch
        R, D = [], []
        for _ in range(int(steps)):
            _, r, d, _ = self.env.step(self.act())
            R.append([float(r)]); D.append([bool(d)])
        return torch.tensor(R, dtype=torch.float32), torch.tensor(D, dtype=torch.bool)


# ---------------------------------------------------------------------------------------------------- MPPI over the net
# libquadsim_dynmppi.so (include/quadsim_dyn_mppi.h): a library of its own, bound here beside the shooting planner's.  It takes
# the image that DynamicsNet.pack builds and the net's widths; nothing of libquadsim_dyn.so's host state.
MPPI_EXPORTS = ["qsdm_version", "qsdm_last_error", "qsdm_workspace_bytes", "qsdm_mppi_plan"]
MPPI_MAX_ITERATIONS, MPPI_MAX_K = 16, 1 << 33

_dynmppi = None


def load_mppi():
    """dlopen libquadsim_dynmppi.so; raises QuadsimError if it has not been built (there is no fallback)"""
    global _dynmppi
    if _dynmppi is not None:
        return _dynmppi
    if not os.path.exists(_lib.DYNMPPI_LIB_PATH):
        raise _lib.QuadsimError("%s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'`." % _lib.DYNMPPI_LIB_PATH)
    import torch  # noqa: F401  (its HIP runtime must be the resident one: see _lib.load)
    lib = C.CDLL(_lib.DYNMPPI_LIB_PATH)
    vp, i64, u64, i32, f32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_float
    sig = {
        "qsdm_version": [],
        "qsdm_workspace_bytes": [i64, i32, i32, C.POINTER(C.c_size_t)],
        "qsdm_mppi_plan": [vp, i32, i32, i64, vp, u64, u64, u64, i32, i32, i32, f32, f32, i32] + [vp] * 11,
    }
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    lib.qsdm_last_error.argtypes, lib.qsdm_last_error.restype = [], C.c_char_p
    _dynmppi = lib
    return lib


def check_mppi(rc, what):
    if rc != 0:
        raise _lib.QuadsimError("%s failed (%d): %s" % (what, rc, load_mppi().qsdm_last_error().decode("utf-8", "replace")))


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
    if not (isinstance(obs, torch.Tensor) and obs.dtype == torch.float32 and obs.dim() == 2 and obs.shape[1] == OBS_DIM
            and obs.device == net.device and obs.is_contiguous()):
        raise ValueError("obs must be a contiguous float32 tensor of shape [N, %d] on %s" % (OBS_DIM, net.device))
    horizon, paths, iterations, lam, sigma, shift, k, n = check_mppi_plan_args(horizon, paths, iterations, lam, sigma, shift, k, obs.shape[0])
    seed, gid0 = int(seed), int(gid0)
    if not (0 <= seed < 1 << 64 and 0 <= gid0 and gid0 + n <= 1 << 48):
        raise ValueError("seed must fit 64 bits and gid0 + N 48 bits")
    for name, t, shape in (("nominal", nominal, (n, horizon, 4)), ("noise", noise, (iterations, paths, horizon, 4))):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and tuple(t.shape) == shape
                                  and t.device == net.device and t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 tensor of shape %s on %s" % (name, list(shape), net.device))
    image = net.pack()
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=net.device)     # noqa: E731
    out = {"actions": new((n, 4), torch.float32), "nominal": new((n, horizon, 4), torch.float32), "best_score": new((n,), torch.float64)}
    if return_scores:
        out["scores"] = new((n, iterations, paths), torch.float64)
    if return_trace:
        out["trace"] = new((n, iterations + 1, horizon, 4), torch.float32)
    if return_candidates:
        out["candidates"] = new((n, paths, horizon, 4), torch.float32)
    if return_traj:
        out["traj"] = new((n, paths, horizon, OBS_DIM), torch.float32)
    lib = load_mppi()
    nbytes = C.c_size_t(0)
    check_mppi(lib.qsdm_workspace_bytes(n, horizon, paths, C.byref(nbytes)), "qsdm_workspace_bytes")
    work = new((int(nbytes.value),), torch.uint8)         # torch's caching allocator: no device allocation in steady state
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())     # noqa: E731
    with torch.cuda.device(net.device):
        check_mppi(lib.qsdm_mppi_plan(p(image), net.h1, net.h2, n, p(obs), seed, gid0, k, horizon, paths, iterations, lam, sigma, shift,
                                      p(nominal), p(noise), p(work), p(out["actions"]), p(out["nominal"]), p(out["best_score"]),
                                      p(out.get("scores")), p(out.get("trace")), p(out.get("candidates")), p(out.get("traj")),
                                      C.c_void_p(torch.cuda.current_stream(net.device).cuda_stream)), "qsdm_mppi_plan")
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

    def run(self, steps):
        """as ``LearnedShootingMPC.run``; a new episode starts from a cold nominal"""
        from .mpc import _closed_loop
        if not self.single:
            return _closed_loop(self.env, self.act, steps, lambda d: self.nominal.masked_fill_(d.bool().view(-1, 1, 1), 0.0))
        import torch
        R, D = [], []
        for _ in range(int(steps)):
            _, r, d, _ = self.env.step(self.act())
            if d:
                self.nominal.zero_()
            R.append([float(r)]); D.append([bool(d)])
        return torch.tensor(R, dtype=torch.float32), torch.tensor(D, dtype=torch.bool)
