"""sha256 of every output array of every kernel path with a network in it, at fixed seeds, as sorted JSON on stdout:

    QUADSIM_HIP_LIB=PARENT.so python tools/net_bits.py > parent.json;  QUADSIM_HIP_LIB=BRANCH.so python tools/net_bits.py > branch.json

one process per library.  A refactor of csrc/mlp.hpp leaves the two files byte-equal; any difference is a behaviour change.
Paths: predict_hip (n = 1, 65, 221), fused_policy_rollout, step_policy and evaluate_policy_episodes (n = 221), each in both
precisions, and fused_runner_rollout x {f32, bf16x3} x {shared, towers} x {role-split, one wave per tile} x {kernel, caller
noise} at n = 221 and n = 1 with T = 12, every env at t = 592 (so each one resets inside the roll-out), 30 % dones_in, the
final env state and step counter included.  221 = 64 * 3 + 29: full tiles, a ragged tile, a partly absent four-tile workgroup."""
import ctypes as C
import hashlib, json, os, sys  # noqa: E401

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import quadsim_amd as qa  # noqa: E402

V0_NPZ, TOWERS_ZIP = (os.path.join(ROOT, "tests", "golden", f) for f in ("policy_best_model_v0.npz", "sb2_ppo2_docking_621_h_30M.zip"))
N, T, PRECISIONS = 64 * 3 + 29, 12, ("f32", "bf16x3")
OUT = {}


def put(key, x):
    a = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    OUT[key] = "%s %s %s" % (a.dtype, list(a.shape), hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def make_env(n, seed, t0=None):
    env = qa.VecDockingEnv("docking-v0", num_envs=n, randomise=1, seed=seed, init_range=qa.C3_INIT_RANGE)
    env.reset()
    if t0 is not None:
        env.set_state(t=np.full_like(env.get_state()["t"], t0))
    return env


def put_handle(key, env):
    for k, v in sorted(env.get_state().items()):
        put("%s/state.%s" % (key, k), v)
    put(key + "/step_counter", np.int64(env.step_counter))


def actor_paths(pol):
    for prec in PRECISIONS:
        for n in (1, 65, N):
            env = make_env(n, 3)
            g = torch.Generator().manual_seed(100 + n)
            obs = ((torch.rand((n, 12), generator=g) - 0.5) * 4.0).to(env.device)
            put("predict_hip/%s/n%d" % (prec, n), pol.predict_hip(env, obs, precision=prec))
            env.close()
        env = make_env(N, 4)
        for name, x in zip(("obs", "rewards", "dones", "flags", "actions"), qa.fused_policy_rollout(env, pol, T, precision=prec)):
            put("policy_rollout/%s/%s" % (prec, name), x)
        put_handle("policy_rollout/" + prec, env)
        for i in range(3):
            o, r, d, a = env.step_policy(pol, precision=prec)
            for name, x in (("obs", o), ("reward", r), ("done", d), ("actions", a), ("flags", env.last_flags)):
                put("step_policy/%s/%d/%s" % (prec, i, name), x)
        put_handle("step_policy/" + prec, env)
        res = qa.evaluate_policy_episodes(pol, env, episodes_per_env=2, precision=prec, max_steps=40)
        for name in ("returns", "lengths", "flags", "docked_steps", "finished"):
            put("evaluate/%s/%s" % (prec, name), getattr(res, name))
        env.close()


def runner_paths(nets):
    for net, ac in sorted(nets.items()):
        for prec in PRECISIONS:
            for serial in (0, 1):
                for noise_src in ("kernel", "caller"):
                    for n in (N, 1):
                        env = make_env(n, 5, t0=592.0)
                        lib = env._lib
                        lib.qs_debug_set_runner_serial.argtypes = [C.c_int]
                        g = torch.Generator().manual_seed(7 + n)
                        noise = torch.randn((T, n, 4), generator=g) if noise_src == "caller" else None
                        dones_in = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
                        before = lib.qs_debug_set_runner_serial(serial)
                        try:
                            ro = qa.fused_runner_rollout(env, ac, T, noise=noise, dones_in=dones_in, want_flags=True, precision=prec)
                            torch.cuda.synchronize()
                        finally:
                            lib.qs_debug_set_runner_serial(before)
                        key = "runner/%s/%s/%s/%s/n%d" % (net, prec, ("split", "serial")[serial], noise_src, n)
                        assert bool(ro["dones"][1:].all(dim=1).any()), key       # the time-out resets ran inside the roll-out
                        for name, x in sorted(ro.items()):
                            if x is not None:
                                put("%s/%s" % (key, name), x)
                        put_handle(key, env)
                        env.close()


if __name__ == "__main__":
    actor_paths(qa.MlpPolicy.from_npz(V0_NPZ))
    runner_paths({"shared": qa.ActorCriticPolicy.from_npz(V0_NPZ), "towers": qa.load_sb2_model(TOWERS_ZIP)})
    json.dump(OUT, sys.stdout, indent=0, sort_keys=True)
    print()
