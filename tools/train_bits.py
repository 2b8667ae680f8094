"""sha256 of every output array of every trainer entry point at fixed seeds, as sorted JSON on stdout:

    QUADSIM_BC_LIB=PARENT/libquadsim_bc.so QUADSIM_PPO_LIB=... python tools/train_bits.py > parent.json
    python tools/train_bits.py > branch.json

One line per case: the number of its arrays and one sha256 over their records (name, dtype, shape, sha256 of the bytes); with
--arrays one line per array, to find which one moved.  One process per build; QUADSIM_BC_LIB, QUADSIM_PPO_LIB, QUADSIM_TRPO_LIB,
QUADSIM_DDPG_LIB, QUADSIM_TD3_LIB, QUADSIM_SAC_LIB, QUADSIM_GAIL_LIB and QUADSIM_DYNFIT_LIB pick it.  A refactor of
csrc/train_pieces.hpp, of csrc/train_offpolicy.hpp or of a trainer's kernels leaves the two files byte-equal; any difference is a
behaviour change.  Only public wrapper names are used, so the same file runs from a checkout of an older commit.

Every tower trainer (bc_fit, ppo2_update, trpo_vf_fit, ddpg_update; trpo_policy_step has no steps): five steps to move Adam's
moments and step count off zero, then the three hashed steps from t0 = 5 -- the bias correction across steps, k_bc_fit's
prefetch of the next step's chunk, both of DDPG's buffers.  Shapes: batch 17 (one full chunk of 16 rows and a one-row tail), and
batch 40 (three chunks) with counts 33, 40, 17 where the entry point has counts.  Each with and without the gradients, and with
one NaN in a row that the schedule touches.  PPO2 and TRPO also at 300 rows in 8 slices of 3 chunks: 19 chunks, so the last slice
is empty.  TRPO's policy step with the full trace: the clean roll-out's line search accepts a candidate, the NaN one's accepts
none (asserted here).  One small fit each of GAIL's discriminator and of the learned dynamics net.

TD3 and SAC under the same recipe, at batch 1, 16 (one full chunk), 17, 40 with counts and 256, each with the caller's noise and with
keyed noise handed back.  TD3 at policy_delay 1 (every hashed step an actor update) and 2 (from t0 = 5 the steps are critic-only,
actor, critic-only: the last step is each kind once); SAC with the learned and with the fixed temperature, the full trace on."""
import hashlib, json, os, sys  # noqa: E401

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import quadsim_amd as qa  # noqa: E402
from quadsim_amd import ppo2  # noqa: E402

V0_NPZ = os.path.join(ROOT, "tests", "golden", "policy_best_model_v0.npz")
ROWS, WARM, STEPS = 96, 5, 3
OUT = {}
DEV = torch.device("cuda", 0)


def put(key, x):
    if isinstance(x, (list, tuple)):
        for i, t in enumerate(x):
            if t is not None:
                put("%s.%d" % (key, i), t)
        return
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    OUT[key] = "%s %s %s" % (a.dtype, list(a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def put_result(key, res):
    for name, x in sorted(res.items()):
        if isinstance(x, dict):
            put_result("%s/%s" % (key, name), x)
        elif x is not None:
            put("%s/%s" % (key, name), x)


def schedule(seed, steps, batch, n=ROWS):
    """[steps, batch] int32 on the host; row 3 of the data (the one that carries the NaN) is in every step"""
    idx = torch.randint(0, n, (steps, batch), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    idx[:, min(1, batch - 1)] = 3
    return idx


def towers(seed):
    rng = np.random.default_rng(seed)
    w = {}
    for key, shape in zip(ppo2.SLOT_KEYS, ppo2.SLOT_SHAPES):
        w[key] = ((rng.standard_normal(shape) * np.sqrt(2.0 / shape[0]) * (0.1 if key == "w2" else 1.0)) if len(shape) == 2
                  else rng.standard_normal(shape) * 0.05).astype(np.float32)
    return qa.ActorCriticPolicy(w, device=DEV)


def rollout(n, nan, seed=11):
    g = torch.Generator().manual_seed(seed)
    obs = (torch.rand(n, 12, generator=g) - 0.5) * 4.0
    ro = {"obs": obs, "actions": torch.randn(n, 4, generator=g) * 0.5, "returns": torch.randn(n, generator=g),
          "values": torch.randn(n, generator=g) * 0.5, "neglogp": 3.0 + torch.rand(n, generator=g)}
    if nan:
        ro["obs"][3, 5] = float("nan")
    return {k: v.to(DEV).contiguous() for k, v in ro.items()}


def shapes(with_counts):
    """(name, batch, counts of the three hashed steps)"""
    return (("b17", 17, None), ("b40", 40, torch.tensor([33, 40, 17], dtype=torch.int32) if with_counts else None))


def variants():
    for grads in (False, True):
        for nan in (False, True):
            yield "%s/%s" % ("grads" if grads else "nograds", "nan" if nan else "clean"), grads, nan


def bc_cases():
    for name, batch, counts in shapes(True):
        for tag, grads, nan in variants():
            key = "bc_fit/%s/%s" % (name, tag)
            pol = qa.MlpPolicy.from_npz(V0_NPZ)
            ro = rollout(ROWS, nan)
            qa.bc_fit(pol, ro["obs"], ro["actions"], schedule(1, WARM, batch))
            put_result(key, qa.bc_fit(pol, ro["obs"], ro["actions"], schedule(2, STEPS, batch), counts, return_grads=grads))
            put(key + "/w", [getattr(pol, k) for k in ("w0", "b0", "w1", "b1", "w2", "b2")])
            put(key + "/m", pol._bc_m)
            put(key + "/v", pol._bc_v)
            if not grads:
                put(key + "/bc_loss", qa.bc_loss(pol, ro["obs"], ro["actions"]))


def put_towers(key, pol, tag):
    put(key + "/w", [getattr(pol, k) for k in ppo2.SLOT_KEYS])
    put(key + "/m", getattr(pol, "_%s_m" % tag))
    put(key + "/v", getattr(pol, "_%s_v" % tag))


def ppo_cases():
    hyper = dict(learning_rate=3.0e-4, cliprange=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5)
    for name, n, batch, slices in (("b17", ROWS, 17, "auto"), ("b40", ROWS, 40, "auto"), ("b300_last_slice_empty", 300, 300, 8)):
        for tag, grads, nan in variants():
            key = "ppo2_update/%s/%s" % (name, tag)
            pol, ro = towers(2), rollout(n, nan)
            qa.ppo2_update(pol, ro, schedule(1, WARM, batch, n).to(DEV), slices=slices, **hyper)
            put_result(key, qa.ppo2_update(pol, ro, schedule(2, STEPS, batch, n).to(DEV), slices=slices, return_grads=grads, **hyper))
            put_towers(key, pol, "ppo")


def trpo_cases():
    for name, n, slices in (("n17", 17, "auto"), ("n40", 40, "auto"), ("n300_last_slice_empty", 300, 8)):
        for tag, grad, nan in variants():
            key = "trpo_policy_step/%s/%s" % (name, tag)
            pol, ro = towers(3), rollout(n, nan)
            res = qa.trpo_policy_step(pol, ro, entcoeff=0.01, slices=slices, return_grad=grad, trace=True)
            accepted = float(res["stats"][8])
            assert (accepted == -1.0) if nan else (accepted >= 0.0), (key, accepted)
            put_result(key, res)
            put(key + "/w", [getattr(pol, k) for k in ppo2.SLOT_KEYS])
    for name, batch, _ in shapes(False):
        for tag, grads, nan in variants():
            key = "trpo_vf_fit/%s/%s" % (name, tag)
            pol, ro = towers(4), rollout(ROWS, nan)
            qa.trpo_vf_fit(pol, ro, schedule(1, WARM, batch).to(DEV))
            put_result(key, qa.trpo_vf_fit(pol, ro, schedule(2, STEPS, batch).to(DEV), return_grads=grads))
            put_towers(key, pol, "trpo")


def ddpg_cases():
    for name, batch, counts in shapes(True):
        for tag, grads, nan in variants():
            key = "ddpg_update/%s/%s" % (name, tag)
            pol, ro = qa.DDPGPolicy(seed=5, device=DEV), rollout(ROWS, nan)
            g = torch.Generator().manual_seed(13)
            obs1 = ((torch.rand(ROWS, 12, generator=g) - 0.5) * 4.0).to(DEV)
            done = (torch.rand(ROWS, generator=g) < 0.2).to(torch.float32).to(DEV)
            replay = (ro["obs"], torch.tanh(ro["actions"]).contiguous(), ro["returns"], obs1, done)
            qa.ddpg_update(pol, replay, schedule(1, WARM, batch))
            put_result(key, qa.ddpg_update(pol, replay, schedule(2, STEPS, batch), counts, return_grads=grads))
            put(key + "/w", [w for ws in pol.nets() for w in ws])
            put(key + "/m", pol.m["actor"] + pol.m["critic"])
            put(key + "/v", pol.v["actor"] + pol.v["critic"])


def offpolicy_shapes():
    return (("b1", 1, None), ("b16", 16, None)) + shapes(True) + (("b256", 256, None),)


def replay_of(nan):
    ro = rollout(ROWS, nan)
    g = torch.Generator().manual_seed(13)
    obs1 = ((torch.rand(ROWS, 12, generator=g) - 0.5) * 4.0).to(DEV)
    done = (torch.rand(ROWS, generator=g) < 0.2).to(torch.float32).to(DEV)
    return (ro["obs"], torch.tanh(ro["actions"]).contiguous(), ro["returns"], obs1, done)


def noise_args(fed, steps, batch, seed):
    """the caller's normals, or keyed draws that the call hands back"""
    if fed:
        return dict(noise=torch.randn(steps, batch, 4, generator=torch.Generator().manual_seed(seed)).to(DEV))
    return dict(seed=seed, return_noise=True)


def td3_cases():
    for name, batch, counts in offpolicy_shapes():
        for tag, grads, nan in variants():
            for delay in (1, 2):
                for fed in (True, False):
                    key = "td3_update/%s/%s/delay%d/%s" % (name, tag, delay, "fed" if fed else "keyed")
                    pol, replay = qa.TD3Policy(seed=8, device=DEV), replay_of(nan)
                    qa.td3_update(pol, replay, schedule(1, WARM, batch), policy_delay=delay, **noise_args(fed, WARM, batch, 21))
                    put_result(key, qa.td3_update(pol, replay, schedule(2, STEPS, batch), counts, policy_delay=delay, return_grads=grads,
                                                  **noise_args(fed, STEPS, batch, 22)))
                    put(key + "/w", [w for ws in pol.nets() for w in ws])
                    put(key + "/m", [t for k in ("actor", "q1", "q2") for t in pol.m[k]])
                    put(key + "/v", [t for k in ("actor", "q1", "q2") for t in pol.v[k]])


def sac_cases():
    for name, batch, counts in offpolicy_shapes():
        for tag, grads, nan in variants():
            for auto in (True, False):
                for fed in (True, False):
                    key = "sac_update/%s/%s/%s/%s" % (name, tag, "auto" if auto else "fixed", "fed" if fed else "keyed")
                    pol, replay = qa.SACPolicy(seed=9, device=DEV, ent_coef=0.5), replay_of(nan)
                    qa.sac_update(pol, replay, schedule(1, WARM, batch), auto_alpha=auto, **noise_args(fed, WARM, batch, 23))
                    put_result(key, qa.sac_update(pol, replay, schedule(2, STEPS, batch), counts, auto_alpha=auto, return_grads=grads,
                                                  return_trace=True, **noise_args(fed, STEPS, batch, 24)))
                    put(key + "/w", [w for ws in pol.nets() for w in ws])
                    put(key + "/m", [t for k in ("actor", "q1", "q2", "v") for t in pol.m[k]])
                    put(key + "/v", [t for k in ("actor", "q1", "q2", "v") for t in pol.v_[k]])
                    put(key + "/alpha_state", pol.alpha_state)


class Expert:
    pass


def other_fits():
    ro, ex = rollout(ROWS, False), Expert()
    ex.obs, ex.actions = rollout(ROWS, False, seed=12)["obs"], rollout(ROWS, False, seed=12)["actions"]
    disc = qa.Discriminator(hidden=100, seed=6, device=DEV)
    put_result("gail_fit", disc.fit(ro["obs"], ro["actions"], ex, schedule(1, STEPS, 17), schedule(2, STEPS, 17), return_grads=True))
    put("gail_fit/w", disc.tensors())
    put("gail_fit/m", disc.m)
    put("gail_fit/v", disc.v)
    put("gail_reward", disc.reward(ro["obs"], ro["actions"]))
    g = torch.Generator().manual_seed(14)
    buf_x, buf_d = torch.randn(ROWS, 16, generator=g).to(DEV), (torch.randn(ROWS, 12, generator=g) * 0.1).to(DEV)
    net = qa.DynamicsNet(64, 32, device=DEV, seed=7)
    put_result("dynfit", net.fit(buf_x, buf_d, ROWS, iters=STEPS, batch=17, seed=3, return_indices=True, return_grads=True))
    put("dynfit/w", net.parameters())
    put("dynfit/m", net.adam_m)
    put("dynfit/v", net.adam_v)


if __name__ == "__main__":
    bc_cases()
    ppo_cases()
    trpo_cases()
    ddpg_cases()
    td3_cases()
    sac_cases()
    other_fits()
    torch.cuda.synchronize()
    if "--arrays" not in sys.argv[1:]:
        cases = {}
        for key, rec in sorted(OUT.items()):
            cases.setdefault(key.rsplit("/", 1)[0], []).append("%s %s" % (key, rec))
        OUT = {case: "%d arrays %s" % (len(recs), hashlib.sha256("\n".join(recs).encode()).hexdigest()) for case, recs in cases.items()}
    json.dump(OUT, sys.stdout, indent=0, sort_keys=True)
    print()
