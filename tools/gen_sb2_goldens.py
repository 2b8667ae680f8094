"""Fixtures of the stable-baselines archive loader and the tower actor-critic (run where the reference tree exists, like
oracle/gen_goldens.py, whose reference bootstrap and helpers it re-uses; writes under tests/golden/):

  sb2_ppo2_docking_621_h_30M.zip, sb2_best_model_v0.zip   the reference's PPO2 archives of the two layouts, re-packed in
      the same container format (data JSON, parameters npz, parameter_list JSON) with every cloudpickle ':serialized:'
      field of `data` dropped: numbers and plain JSON only
  g13_towers_episode.npz   the reference DockingEnv (v0) driven by the deterministic actor of ppo2_docking_621_h_30M
      (pi_fc0 -> pi_fc1 -> pi, ReLU, clip; float32 as gen_g5 evaluates best_model_v0), recorded like g5, plus the float64
      value of the vf tower (vf_fc0 -> vf_fc1 -> vf; rl_baselines/common/policies.py:35-92 mlp_extractor) for every
      observation acted on ("obs_in") and for the last one.  The values are parity-unpinned by TensorFlow (not installed).

    python tools/gen_sb2_goldens.py
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_goldens as G  # noqa: E402  (loads the reference; exits with an error where it is absent)

ARCHIVES = (("ppo2_docking_621_h_30M.zip", "sb2_ppo2_docking_621_h_30M.zip"),
            (os.path.join("trained_model", "best_model_v0.zip"), "sb2_best_model_v0.zip"))


def _strip(obj):
    if isinstance(obj, dict):
        return {k: _strip(v) for k, v in obj.items() if k != ":serialized:"}
    if isinstance(obj, list):
        return [_strip(v) for v in obj]
    return obj


def repack(src, dst):
    with zipfile.ZipFile(src) as z:
        data = _strip(json.loads(z.read("data").decode("utf-8")))
        params, plist = z.read("parameters"), z.read("parameter_list")
    np.load(io.BytesIO(params), allow_pickle=False).files        # plain arrays only
    with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:
        z.writestr("data", json.dumps(data, indent=4))
        z.writestr("parameters", params)
        z.writestr("parameter_list", plist)
    print("%-34s %8.1f KiB" % (os.path.basename(dst), os.path.getsize(dst) / 1024.0))


def tower_value64(P, obs):
    f = lambda k: np.asarray(P[k], np.float64)                    # noqa: E731
    h = np.maximum(np.asarray(obs, np.float64) @ f("model/vf_fc0/w:0") + f("model/vf_fc0/b:0"), 0.0)
    h = np.maximum(h @ f("model/vf_fc1/w:0") + f("model/vf_fc1/b:0"), 0.0)
    return (h @ f("model/vf/w:0") + f("model/vf/b:0"))[..., 0]


def gen_g13():
    z = zipfile.ZipFile(os.path.join(G.REF, "ppo2_docking_621_h_30M.zip"))
    P = np.load(io.BytesIO(z.read("parameters")), allow_pickle=False)
    P = {k: P[k] for k in P.files}

    def policy(o):
        h = np.maximum(o.astype(np.float32) @ P["model/pi_fc0/w:0"] + P["model/pi_fc0/b:0"], 0)
        h = np.maximum(h @ P["model/pi_fc1/w:0"] + P["model/pi_fc1/b:0"], 0)
        return np.clip(h @ P["model/pi/w:0"] + P["model/pi/b:0"], -1, 1).astype(np.float32)

    env = G.env_v0.DockingEnv()
    o = env.reset()
    A, RB, RA, OI, O, R, D, F = [], [], [], [], [], [], [], []
    for t in range(600):
        a = policy(np.asarray(o))
        RB.append(G.snapshot(env)); OI.append(np.array(o, np.float64))
        o, r, d, info = env.step(a.astype(np.float64))
        RA.append(G.snapshot(env)); A.append(a); O.append(np.array(o)); R.append(r); D.append(d)
        F.append((1 if info["flag_docking"] else 0) | (2 if info["done_overlimit"] else 0) | (4 if env.t >= 600 else 0))
        if d:
            break
    OI = np.array(OI)
    print("g13: steps %d, return %.4f, docked steps %d, last flags %d" % (len(A), float(np.sum(R)), int(np.sum(np.array(F) & 1)), F[-1]))
    G.save("g13_towers_episode", actions=np.array(A, np.float32), rec_before=np.array(RB), rec_after=np.array(RA),
           obs=np.array(O), obs_in=OI, reward=np.array(R), done=np.array(D, np.uint8), flags=np.array(F, np.uint8),
           values=tower_value64(P, OI), last_value=np.array(tower_value64(P, np.array(O[-1])[None])[0]))


if __name__ == "__main__":
    for src, dst in ARCHIVES:
        repack(os.path.join(G.REF, src), os.path.join(G.OUT, dst))
    gen_g13()
