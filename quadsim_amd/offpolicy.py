"""What the wrappers of the three off-policy trainers share (ddpg.py, td3.py, sac.py): the container of a trainer's nets, the host
checks of an update's replay, indices and counts, and the keyed noise restated on the host.  The replay ring, its schedule and the
collection loop are ddpg.py's."""
import ctypes as C
import math

import numpy as np

from . import _lib

NET_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")


class Nets:
    """a trainer's nets in the policy's (in, out) layout, each a list of six tensors under its name, with Adam's moments of the online
    nets ({name: six tensors} under ``m`` and under the attribute named by V) and the device workspace of the library's update.  A
    trainer's policy class states: NET_NAMES (the ABI's order, the online nets first), ONLINE_NAMES, shapes_of(name), V, OUT_LIM (the
    bound of the output layer's initial weights where it is not Glorot's), TAKES_DTYPE (whether its constructor takes one), LIB (the
    key of its side library and the entry point that sizes the workspace) and load (the wrapper's loader, looked up at the call)."""
    V, OUT_LIM, TAKES_DTYPE = "v", None, True

    def init_nets(self, seed, device, weights, dtype):
        """the nets from `weights` ({name: {w0 ..}}, a target's defaulting to its online net's), shape-checked, or, where None, SB2's
        initialisation drawn from `seed`: Glorot-uniform weights, zero biases"""
        import torch
        self.device, self.dtype = torch.device(device), getattr(torch, dtype)
        if weights is None:
            rng = np.random.default_rng(int(seed))
            weights = {}
            for name in self.ONLINE_NAMES:
                W = {}
                for k, shape in zip(NET_KEYS, self.shapes_of(name)):
                    if len(shape) == 1:
                        W[k] = np.zeros(shape, np.float32)
                    else:
                        lim = self.OUT_LIM if k == "w2" and self.OUT_LIM else math.sqrt(6.0 / (shape[0] + shape[1]))
                        W[k] = rng.uniform(-lim, lim, shape).astype(np.float32)
                weights[name] = W
        for name in self.NET_NAMES:
            src = weights.get(name, weights[name.split("_")[0]])
            ws = []
            for k, shape in zip(NET_KEYS, self.shapes_of(name)):
                w = np.ascontiguousarray(src[k])
                if w.shape != shape:
                    raise ValueError("%s %s must be of shape %s, got %s" % (name, k, shape, w.shape))
                ws.append(torch.as_tensor(w.copy()).to(self.dtype).to(self.device))
            setattr(self, name, ws)
        self.device = self.actor[0].device
        self._workspace, self._images = None, {}

    def zero_moments(self):
        import torch
        self.m = {k: [torch.zeros_like(w) for w in getattr(self, k)] for k in self.ONLINE_NAMES}
        setattr(self, self.V, {k: [torch.zeros_like(w) for w in getattr(self, k)] for k in self.ONLINE_NAMES})

    def nets(self):
        return [getattr(self, name) for name in self.NET_NAMES]

    def updated(self):
        """an update wrote the weights in place: every cached image of them is dropped"""
        self._images = {}

    def save_npz(self, path):
        arrays = {}
        for name in self.NET_NAMES:
            arrays.update({"%s_%s" % (name, k): w.detach().cpu().numpy() for k, w in zip(NET_KEYS, getattr(self, name))})
        for name in self.ONLINE_NAMES:
            arrays.update({"m_%s_%s" % (name, k): t.cpu().numpy() for k, t in zip(NET_KEYS, self.m[name])})
            arrays.update({"v_%s_%s" % (name, k): t.cpu().numpy() for k, t in zip(NET_KEYS, getattr(self, self.V)[name])})
        np.savez(path, **self.npz_state(), **arrays)

    @classmethod
    def from_npz(cls, path, device="cuda"):
        import torch
        with np.load(path, allow_pickle=False) as z:
            kw = {"dtype": str(z["actor_w0"].dtype)} if cls.TAKES_DTYPE else {}
            p = cls(device=device, weights={name: {k: z["%s_%s" % (name, k)] for k in NET_KEYS} for name in cls.NET_NAMES}, **kw)
            for name in cls.ONLINE_NAMES:
                p.m[name] = [torch.as_tensor(z["m_%s_%s" % (name, k)].copy()).to(p.device) for k in NET_KEYS]
                getattr(p, cls.V)[name] = [torch.as_tensor(z["v_%s_%s" % (name, k)].copy()).to(p.device) for k in NET_KEYS]
            p.set_npz_state(z)
        return p

    def npz_state(self):
        """what an archive holds beside the nets and the moments"""
        return {"steps": self.steps}

    def set_npz_state(self, z):
        self.steps = int(z["steps"])

    def workspace(self):
        """the device workspace of the library's update, allocated once"""
        if self._workspace is None:
            nbytes = C.c_size_t(0)
            _lib.side_call(self.LIB[0], self.load(), self.LIB[1], C.byref(nbytes))
            self._workspace = _lib.new_tensor(self.device, (int(nbytes.value),), "uint8")
        return self._workspace


def check_extent(n, steps, batch, max_batch, max_steps):
    """ValueError for a batch, a step count or a replay size that every update refuses"""
    if not 1 <= batch <= max_batch:
        raise ValueError("batch must be in [1, %d], got %d" % (max_batch, batch))
    if not 1 <= steps <= max_steps:
        raise ValueError("steps must be in [1, %d], got %d" % (max_steps, steps))
    if not 1 <= n < 1 << 31:
        raise ValueError("n must be in [1, 2^31), got %d" % n)


def check_discount(gamma, tau):
    if not 0.0 <= gamma <= 1.0:
        raise ValueError("gamma must be in [0, 1], got %r" % gamma)
    if not 0.0 < tau <= 1.0:
        raise ValueError("tau must be in (0, 1], got %r" % tau)


def check_schedule(n, steps, batch, counts, indices):
    """ValueError for what no update can check of the host arrays `counts` [steps] and `indices` [steps,batch] (either may be None):
    a count outside [1, batch], a row the update would read outside [0, n)"""
    if counts is not None:
        counts = np.asarray(counts)
        if counts.shape != (steps,) or counts.min() < 1 or counts.max() > batch:
            raise ValueError("counts must be [%d] values in [1, batch = %d]" % (steps, batch))
    if indices is not None:
        indices = np.asarray(indices)
        if indices.shape != (steps, batch):
            raise ValueError("indices must be [%d, %d], got %s" % (steps, batch, indices.shape))
        used = indices if counts is None else indices[np.arange(batch)[None, :] < counts[:, None]]
        if used.min() < 0 or used.max() >= n:
            raise ValueError("indices the update would read must be in [0, n = %d), got [%d, %d]" % (n, used.min(), used.max()))


def update_tensors(policy, replay, indices, counts, dtype):
    """the tensor checks of an update: the policy's nets (of `dtype` and their shapes), the replay (a ReplayBuffer or its five device
    tensors) and the host int32 tensors `indices` and `counts` -> (the five replay tensors, n, indices, counts)"""
    import torch
    dev = policy.device
    for name in policy.NET_NAMES:
        for k, w, shape in zip(NET_KEYS, getattr(policy, name), policy.shapes_of(name)):
            _lib.check_tensor("%s %s" % (name, k), w, dtype, shape, dev)
    obs0, act, rew, obs1, done = replay if isinstance(replay, (tuple, list)) else replay.tensors()
    n = int(obs0.shape[0])
    for name, t, shape in (("obs0", obs0, (n, 12)), ("act", act, (n, 4)), ("rew", rew, (n,)), ("obs1", obs1, (n, 12)), ("done", done, (n,))):
        _lib.check_tensor(name, t, "float32", shape, dev)
    indices = torch.as_tensor(indices)
    if indices.dtype != torch.int32 or indices.dim() != 2 or indices.device.type != "cpu":
        raise ValueError("indices must be a host int32 tensor [steps, batch]")
    if counts is not None:
        counts = torch.as_tensor(counts)
        if counts.dtype != torch.int32 or counts.device.type != "cpu":
            raise ValueError("counts must be a host int32 tensor [steps]")
    return (obs0, act, rew, obs1, done), n, indices, counts


def keyed_noise(seed, t0, steps, batch, stream):
    """-> [steps, batch, 4] float32: the normals that an update without `noise` draws, restated on the host: Box-Muller in float64 on
    the words of Philox4x32-10 block t0 + s of subsequence (stream << 48) | row slot, key `seed` (the device's own arithmetic is
    float32: it differs from this in the last digits; ``noise_out`` of the update has the device's values)"""
    m32 = np.uint64(0xFFFFFFFF)
    block = np.broadcast_to(np.arange(int(t0), int(t0) + int(steps), dtype=np.uint64)[:, None], (int(steps), int(batch)))
    sub = (np.uint64(stream) << np.uint64(48)) | np.arange(int(batch), dtype=np.uint64)[None, :]
    c0, c1, c2, c3 = block & m32, block >> np.uint64(32), np.broadcast_to(sub & m32, block.shape), np.broadcast_to(sub >> np.uint64(32), block.shape)
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    w = np.stack([c0, c1, c2, c3], axis=-1)
    u = ((w.astype(np.float32).astype(np.float64) + 1.0) * 2.0 ** -32).astype(np.float32).astype(np.float64)
    z = np.empty(u.shape, np.float64)
    for a, b in ((0, 1), (2, 3)):
        r, th = np.sqrt(-2.0 * np.log(u[..., a])), 2.0 * np.pi * u[..., b]
        z[..., a], z[..., b] = r * np.cos(th), r * np.sin(th)
    return z.astype(np.float32)
