"""stable-baselines (SB2) PPO2 archives -> the package's policies, with no TensorFlow and no unpickling.

An SB2 ``model.save(path)`` zip holds ``data`` (JSON; class-valued fields carry a cloudpickle blob under ``:serialized:``
next to plain-text renderings), ``parameters`` (an npz of the TensorFlow variables) and ``parameter_list`` (JSON, the
variable names in order).  The reference's scripts load them with ``PPO2.load(path)`` (e.g. run_trained_docking_ppo2.py).
Here the network layout is read from the variable names and shapes and the activation from the plain-text
``policy_kwargs.act_fun``; the ``:serialized:`` blobs are never decoded.

Two layouts of rl_baselines/common/policies.py:35-92 (mlp_extractor), both ReLU, 12 observations -> 4 actions, 128 wide:
  "shared"  net_arch [128, dict(pi=[128], vf=[128])] (trained_model/best_model_v0.zip)
            w0,b0 = shared_fc0 | w1,b1 = pi_fc0 | w2,b2 = pi | wv1,bv1 = vf_fc0 | wv2,bv2 = vf | logstd
  "towers"  net_arch [dict(pi=[128, 128], vf=[128, 128])] (every ppo2_docking*.zip, run_docking_gail.py:56)
            w0,b0 = pi_fc0 | w1,b1 = pi_fc1 | w2,b2 = pi | wv0,bv0 = vf_fc0 | wv1,bv1 = vf_fc1 | wv2,bv2 = vf | logstd
The presence of ``wv0`` marks the tower layout everywhere in the package.  Anything else raises ``ValueError``.
"""
import io
import json
import re
import zipfile

import numpy as np

OBS_DIM, ACT_DIM, HIDDEN = 12, 4, 128


def _activation(data):
    """the activation named in the plain-text rendering of policy_kwargs.act_fun; SB2's default (absent) is tanh"""
    kw = data.get("policy_kwargs") or {}
    txt = kw.get("act_fun") if isinstance(kw, dict) else None
    if txt is None:
        return "tanh"
    m = re.search(r"<function\s+([A-Za-z_][\w.]*)", str(txt))
    return m.group(1).rsplit(".", 1)[-1] if m else str(txt)


def read_sb2_weights(path):
    """-> (layout "shared" | "towers", {key: float32 array}) in the package's weight keys (module docstring).
    Raises ValueError for anything the device kernels do not run: another activation, width, obs / action size or depth."""
    with zipfile.ZipFile(path) as z:
        names = set(z.namelist())
        for need in ("data", "parameters", "parameter_list"):
            if need not in names:
                raise ValueError("%s: not a stable-baselines archive (no '%s' entry)" % (path, need))
        data = json.loads(z.read("data").decode("utf-8"))
        plist = json.loads(z.read("parameter_list").decode("utf-8"))
        with np.load(io.BytesIO(z.read("parameters")), allow_pickle=False) as npz:
            raw = {k: np.asarray(npz[k]) for k in npz.files}
    P = {}
    for name in plist:
        if name not in raw:
            raise ValueError("%s: parameter_list names %r, which 'parameters' lacks" % (path, name))
        m = re.fullmatch(r"model/(.+):0", name)
        if m:
            P[m.group(1)] = raw[name]
    act = _activation(data)
    if act != "relu":
        raise ValueError("%s: activation %r is unsupported (the device kernels run ReLU policies only)" % (path, act))
    layers = {k.split("/")[0] for k in P if "/" in k}
    shared = sorted(k for k in layers if k.startswith("shared_fc"))
    pi_fc = sorted(k for k in layers if re.fullmatch(r"pi_fc\d+", k))
    vf_fc = sorted(k for k in layers if re.fullmatch(r"vf_fc\d+", k))
    if shared == ["shared_fc0"] and pi_fc == ["pi_fc0"] and vf_fc == ["vf_fc0"]:
        layout = "shared"
        order = (("w0", "b0", "shared_fc0", OBS_DIM, HIDDEN), ("w1", "b1", "pi_fc0", HIDDEN, HIDDEN),
                 ("wv1", "bv1", "vf_fc0", HIDDEN, HIDDEN))
    elif not shared and pi_fc == ["pi_fc0", "pi_fc1"] and vf_fc == ["vf_fc0", "vf_fc1"]:
        layout = "towers"
        order = (("w0", "b0", "pi_fc0", OBS_DIM, HIDDEN), ("w1", "b1", "pi_fc1", HIDDEN, HIDDEN),
                 ("wv0", "bv0", "vf_fc0", OBS_DIM, HIDDEN), ("wv1", "bv1", "vf_fc1", HIDDEN, HIDDEN))
    else:
        raise ValueError("%s: network layout unsupported (shared %s, pi %s, vf %s); supported: net_arch "
                         "[128, dict(pi=[128], vf=[128])] and [dict(pi=[128, 128], vf=[128, 128])]" % (path, shared, pi_fc, vf_fc))
    order += (("w2", "b2", "pi", HIDDEN, ACT_DIM), ("wv2", "bv2", "vf", HIDDEN, 1))
    W = {}
    for wk, bk, layer, n_in, n_out in order:
        w, b = P.get(layer + "/w"), P.get(layer + "/b")
        if w is None or b is None:
            raise ValueError("%s: layer %s has no w / b" % (path, layer))
        if w.shape != (n_in, n_out) or b.shape != (n_out,):
            what = "observation size" if n_in == OBS_DIM and w.ndim == 2 and w.shape[0] != OBS_DIM else \
                   "action size" if layer == "pi" and w.ndim == 2 and w.shape[0] == HIDDEN else "hidden width"
            raise ValueError("%s: %s unsupported: %s/w is %s, expected %s (%d observations, %d actions, %d wide)"
                             % (path, what, layer, w.shape, (n_in, n_out), OBS_DIM, ACT_DIM, HIDDEN))
        W[wk], W[bk] = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)
    ls = P.get("pi/logstd")
    if ls is None or ls.size != ACT_DIM:
        raise ValueError("%s: pi/logstd missing or not %d long" % (path, ACT_DIM))
    W["logstd"] = np.ascontiguousarray(ls, np.float32).reshape(-1)
    return layout, W


def load_sb2_model(path, device="cuda", squash=False):
    """``PPO2.load(path)``'s policy as an ActorCriticPolicy (actor + critic + logstd), either layout; ``squash`` selects the
    fork's tanh-squashed Gaussian.  Runs on the fused Runner kernels (Runner, fused_runner_rollout)."""
    from .runner import ActorCriticPolicy
    _, W = read_sb2_weights(path)
    return ActorCriticPolicy(W, device, squash)
