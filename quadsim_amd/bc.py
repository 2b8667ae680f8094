"""Behaviour cloning of the actor on the device (the step between ``record_expert_dataset`` and
``evaluate_policy_episodes``): ``model.pretrain(dataset, n_epochs)`` of run_pretrained_ppo2_docking.py:50-69.

SB2's ``BaseRLModel.pretrain`` regresses the policy's deterministic (mean) action onto the expert's with Adam, one small
minibatch after another.  ``pretrain`` here runs every step of up to 4096 minibatches in ONE launch of one resident workgroup
(``qsbc_fit`` of libquadsim_bc.so, include/quadsim_bc.h): weights in LDS, Adam's moments in registers.  Nothing is drawn on the
device: ``epoch_schedule`` shuffles on the host, as ``ExpertDataset``'s data loader does.  The validation loss is ``qsbc_loss``,
a forward-only pass over many workgroups.

Both policies of the package have the same actor (``w0, b0, w1, b1, w2, b2``: 12 -> 128 -> 128 -> 4, ReLU), so ``MlpPolicy`` and
``ActorCriticPolicy`` of either layout are trained by the same kernel; only those six tensors change (in the shared layout the
trunk moves under the critic, as it does in SB2).  There is no CPU path.
"""
import ctypes as C
import functools
import os

import numpy as np

from . import _lib

BC_MAX_BATCH, BC_MAX_STEPS, BC_LOSS_BLOCK = 256, 4096, 256
BC_BETA1, BC_BETA2 = 0.9, 0.999                     # tf.train.AdamOptimizer's defaults, which SB2's pretrain leaves alone
ACTOR_KEYS = ("w0", "b0", "w1", "b1", "w2", "b2")
ACTOR_SHAPES = ((12, 128), (128,), (128, 128), (128,), (128, 4), (4,))


# libquadsim_bc.so is the entry "bc" of _lib.SIDE: its path, signatures, loader, status check and call helper are _lib's.  The
# names below stay this module's so that callers and tests can replace the loader
QsbcNet, BC_EXPORTS = _lib.QsbcNet, _lib.SIDE["bc"]["exports"]
load_bc, check_bc = functools.partial(_lib.side_load, "bc"), functools.partial(_lib.side_check, "bc")


def check_bc_args(n, steps, batch, lr=1.0e-4, beta1=BC_BETA1, beta2=BC_BETA2, eps=1.0e-8, t0=0, counts=None, indices=None):
    """-> (n, steps, batch, lr, beta1, beta2, eps, t0); ValueError for what qsbc_fit would refuse and, given the host arrays
    `counts` [steps] and `indices` [steps,batch], for what it cannot check (a count outside [1, batch], a row it would read
    outside [0, n)), before anything touches the library or the GPU"""
    n, steps, batch, t0 = int(n), int(steps), int(batch), int(t0)
    if not 1 <= batch <= BC_MAX_BATCH:
        raise ValueError("batch must be in [1, %d], got %d" % (BC_MAX_BATCH, batch))
    if not 1 <= steps <= BC_MAX_STEPS:
        raise ValueError("steps must be in [1, %d], got %d" % (BC_MAX_STEPS, steps))
    if not 1 <= n < 1 << 31:
        raise ValueError("n must be in [1, 2^31), got %d" % n)
    lr, beta1, beta2, eps = _lib.check_adam_args(lr, beta1, beta2, eps, t0, steps, "steps")
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
            raise ValueError("indices the fit would read must be in [0, n = %d), got [%d, %d]" % (n, used.min(), used.max()))
    return n, steps, batch, lr, beta1, beta2, eps, t0


# ---------------------------------------------------------------------------------------------------- the data and the schedule
class ExpertData:
    """SB2's ``ExpertDataset`` split (traj_limitation = -1) on the device.  `source`: the dict ``record_expert_dataset`` returns
    or the path of an ``.npz`` with its keys; only ``obs`` [n,12] and ``actions`` [n,4] are used.  A permutation of the rows is
    drawn once from `seed`; its first int(train_fraction n) entries are the train rows, the rest the validation rows."""

    def __init__(self, source, train_fraction=0.7, batch_size=64, seed=0, device="cuda"):
        import torch
        if isinstance(source, (str, os.PathLike)):
            with np.load(source, allow_pickle=False) as z:
                source = {k: z[k] for k in ("obs", "actions")}
        obs = np.ascontiguousarray(source["obs"], np.float32)
        act = np.ascontiguousarray(source["actions"], np.float32)
        if obs.ndim != 2 or obs.shape[1] != 12 or act.ndim != 2 or act.shape[1] != 4 or obs.shape[0] != act.shape[0] or obs.shape[0] < 1:
            raise ValueError("obs must be [n, 12] and actions [n, 4] with n >= 1, got %s and %s" % (obs.shape, act.shape))
        if not 0.0 < float(train_fraction) <= 1.0:
            raise ValueError("train_fraction must be in (0, 1], got %r" % (train_fraction,))
        if not 1 <= int(batch_size) <= BC_MAX_BATCH:
            raise ValueError("batch_size must be in [1, %d], got %r" % (BC_MAX_BATCH, batch_size))
        self.n, self.batch_size, self.seed = obs.shape[0], int(batch_size), int(seed)
        perm = torch.randperm(self.n, generator=torch.Generator().manual_seed(self.seed)).to(torch.int32)
        n_train = max(1, int(float(train_fraction) * self.n))
        self.train_rows, self.val_rows = perm[:n_train].contiguous(), perm[n_train:].contiguous()      # CPU int32
        self.device = torch.device(device)
        self.obs, self.actions = torch.as_tensor(obs).to(self.device), torch.as_tensor(act).to(self.device)
        self._val_dev = None

    @property
    def n_train(self):
        return int(self.train_rows.numel())

    @property
    def n_val(self):
        return int(self.val_rows.numel())

    def val_rows_device(self):
        if self._val_dev is None:
            self._val_dev = self.val_rows.to(self.device)
        return self._val_dev


def epoch_schedule(n_train, batch_size, n_epochs, generator):
    """-> (indices [steps, batch_size] int32, counts [steps] int32), CPU: every epoch a fresh shuffle of 0 .. n_train-1 from
    `generator` (a CPU torch.Generator), cut into consecutive minibatches; the last, partial minibatch of an epoch is kept and
    its unused entries are 0.  steps = n_epochs ceil(n_train / batch_size).  The schedule of n_epochs epochs is the schedules of
    one epoch drawn one after another from the same generator."""
    import torch
    n_train, batch_size, n_epochs = int(n_train), int(batch_size), int(n_epochs)
    if n_train < 1 or batch_size < 1 or n_epochs < 1:
        raise ValueError("n_train, batch_size and n_epochs must be >= 1")
    per = -(-n_train // batch_size)
    idx = torch.zeros((n_epochs, per * batch_size), dtype=torch.int32)
    for e in range(n_epochs):
        idx[e, :n_train] = torch.randperm(n_train, generator=generator).to(torch.int32)
    cnt = torch.full((n_epochs, per), batch_size, dtype=torch.int32)
    cnt[:, -1] = n_train - (per - 1) * batch_size
    return idx.view(n_epochs * per, batch_size), cnt.view(-1)


# ---------------------------------------------------------------------------------------------------- the policy's side
def actor_tensors(policy):
    """the six tensors of the actor of an MlpPolicy or an ActorCriticPolicy (either layout), checked for the kernel"""
    import torch
    ws = [getattr(policy, k, None) for k in ACTOR_KEYS]
    for k, w, shape in zip(ACTOR_KEYS, ws, ACTOR_SHAPES):
        if not (isinstance(w, torch.Tensor) and w.dtype == torch.float32 and tuple(w.shape) == shape and w.is_contiguous()):
            raise TypeError("pretrain: the policy's %s must be a contiguous float32 tensor of shape %s" % (k, shape))
    if ws[0].device.type != "cuda" or any(w.device != ws[0].device for w in ws):
        raise _lib.QuadsimError("pretrain needs the policy on a HIP device, it is on %s; there is no CPU path" % ws[0].device)
    return ws


def drop_cached_images(policy):
    """the kernels wrote the weights behind the policy's back: forget every device image built from them (the transposed copies
    and the packed split-bf16 blobs of MlpPolicy and ActorCriticPolicy, and the evaluation actor with images of its own)"""
    from .runner import ActorCriticPolicy
    if isinstance(policy, ActorCriticPolicy):
        policy._wt = policy._ac_blob = None
    else:
        for name in ("_wt", "_blob"):
            if hasattr(policy, name):
                delattr(policy, name)
    if hasattr(policy, "_eval_actor"):
        del policy._eval_actor


def reset_pretrain_optimizer(policy):
    """forget Adam's moments and the step count (the next fit creates them again, zeros)"""
    policy._bc_m, policy._bc_v, policy._bc_steps = None, None, 0


def _state(policy, ws):
    import torch
    if getattr(policy, "_bc_m", None) is None:
        policy._bc_m, policy._bc_v = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
        policy._bc_steps = 0
    return policy._bc_m, policy._bc_v


def _dataset_tensors(ws, obs, act):
    _lib.check_tensor("obs", obs, "float32", ("n", 12), ws[0].device)
    _lib.check_tensor("act", act, "float32", ("n", 4), ws[0].device)
    if obs.shape[0] != act.shape[0]:
        raise ValueError("obs and act must have the same number of rows, got %d and %d" % (obs.shape[0], act.shape[0]))


def bc_fit(policy, obs, act, indices, counts=None, lr=1.0e-4, beta1=BC_BETA1, beta2=BC_BETA2, eps=1.0e-8, return_grads=False):
    """ONE launch of qsbc_fit: indices.shape[0] Adam steps on the policy's actor.  obs [n,12], act [n,4]: device tensors; indices
    [steps,batch] int32 and counts [steps] int32 (or None): HOST tensors, checked here (check_bc_args) and uploaded.  The
    weights, the moments kept on the policy and its step count are updated in place and every cached device image of the weights
    is dropped.  -> dict(loss [steps] device tensor, grads: six device tensors on request).  Launched on torch's current stream;
    nothing waits for the device."""
    import torch
    ws = actor_tensors(policy)
    _dataset_tensors(ws, obs, act)
    indices = torch.as_tensor(indices)
    if indices.dtype != torch.int32 or indices.dim() != 2 or indices.device.type != "cpu":
        raise ValueError("indices must be a host int32 tensor [steps, batch]")
    if counts is not None:
        counts = torch.as_tensor(counts)
        if counts.dtype != torch.int32 or counts.device.type != "cpu":
            raise ValueError("counts must be a host int32 tensor [steps]")
    steps, batch = int(indices.shape[0]), int(indices.shape[1])
    m, v = _state(policy, ws)
    n, steps, batch, lr, beta1, beta2, eps, t0 = check_bc_args(
        obs.shape[0], steps, batch, lr, beta1, beta2, eps, policy._bc_steps, None if counts is None else counts.numpy(), indices.numpy())
    dev = ws[0].device
    idx_d = indices.contiguous().to(dev)
    cnt_d = None if counts is None else counts.contiguous().to(dev)
    out = {"loss": _lib.new_tensor(dev, (steps,), "float32")}
    if return_grads:
        out["grads"] = [torch.empty_like(w) for w in ws]
    net = QsbcNet(C.sizeof(QsbcNet), 0, _lib.six(ws), _lib.six(m), _lib.six(v))
    _lib.side_call("bc", load_bc(), "qsbc_fit", C.byref(net), obs, act, n, idx_d, cnt_d, steps, batch, lr, beta1, beta2, eps, t0, out["loss"],
                   _lib.six(out["grads"]) if return_grads else None, device=dev)
    policy._bc_steps += steps
    drop_cached_images(policy)
    return out


def bc_loss(policy, obs, act, rows=None, grid=0):
    """qsbc_loss: mean((a_expert - mean_action)^2) of the policy's actor over the rows `rows` (a device int32 tensor; None: every
    row) -> a float64 device tensor [1].  The value does not depend on `grid`."""
    import torch
    ws = actor_tensors(policy)
    _dataset_tensors(ws, obs, act)
    dev = ws[0].device
    if rows is not None and not (isinstance(rows, torch.Tensor) and rows.dtype == torch.int32 and rows.dim() == 1 and rows.device == dev
                                 and rows.is_contiguous()):
        raise ValueError("rows must be a contiguous int32 tensor [count] on %s" % (dev,))
    count = int(obs.shape[0]) if rows is None else int(rows.numel())
    if not 1 <= count < 1 << 31:
        raise ValueError("count must be in [1, 2^31), got %d" % count)
    if not 0 <= int(grid) <= 65535:
        raise ValueError("grid must be in [0, 65535], got %r" % (grid,))
    lib = load_bc()
    partials = _lib.new_tensor(dev, (_lib.side_call("bc", lib, "qsbc_loss_blocks", count),), "float64")
    out = _lib.new_tensor(dev, (1,), "float64")
    _lib.side_call("bc", lib, "qsbc_loss", _lib.six(ws), obs, act, obs.shape[0], rows, count, partials, out, int(grid), device=dev)
    return out


def pretrain(policy, dataset, n_epochs=10, learning_rate=1.0e-4, adam_epsilon=1.0e-8, val_interval=None, seed=0):
    """SB2's ``BaseRLModel.pretrain(dataset, n_epochs, learning_rate, adam_epsilon, val_interval)`` for the continuous actor:
    Adam on mean((a_expert - mean_action)^2) over the minibatches of `dataset` (an ExpertData), every epoch a fresh shuffle of
    its train rows from `seed`, the partial last minibatch kept.  The steps run in launches of at most 4096 (qsbc_fit); the
    validation loss (qsbc_loss over the validation rows) is taken every `val_interval` epochs (None: max(1, n_epochs // 10)).
    Adam's moments and step count stay on the policy: a second call continues from them (``reset_pretrain_optimizer``).
    -> {"train_loss": [n_epochs] the mean of each epoch's step losses, "val_loss": {epoch (from 1): value}, "steps": total}."""
    import torch
    n_epochs = int(n_epochs)
    if n_epochs < 1:
        raise ValueError("n_epochs must be >= 1, got %d" % n_epochs)
    val_interval = max(1, n_epochs // 10) if val_interval is None else int(val_interval)
    if val_interval < 1:
        raise ValueError("val_interval must be >= 1, got %d" % val_interval)
    gen = torch.Generator().manual_seed(int(seed))
    means, vals, total = [], {}, 0
    for epoch in range(1, n_epochs + 1):
        pos, counts = epoch_schedule(dataset.n_train, dataset.batch_size, 1, gen)
        indices = dataset.train_rows[pos.long()]          # positions in the train set -> rows of the dataset
        losses = []
        for s in range(0, indices.shape[0], BC_MAX_STEPS):
            losses.append(bc_fit(policy, dataset.obs, dataset.actions, indices[s:s + BC_MAX_STEPS], counts[s:s + BC_MAX_STEPS],
                                 lr=learning_rate, eps=adam_epsilon)["loss"])
        means.append(torch.cat(losses).double().mean())
        total += int(indices.shape[0])
        if epoch % val_interval == 0 and dataset.n_val > 0:
            vals[epoch] = bc_loss(policy, dataset.obs, dataset.actions, dataset.val_rows_device())
    train = [float(x) for x in torch.stack(means).cpu()]
    if vals:
        host = torch.cat(list(vals.values())).cpu()
        vals = {e: float(x) for e, x in zip(vals, host)}
    return {"train_loss": train, "val_loss": vals, "steps": total}
