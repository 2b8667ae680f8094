#!/usr/bin/env python3
"""What one call of the Python wrappers costs, at 65 536 docking-v0 envs (torch backend) on one MI355X: a host clock around
--calls calls that ends in a device synchronise, for the five loops a user writes

  step_nocopy      env.step(a) on a VecDockingEnv(copy=False)
  step_copy        env.step(a) on a VecDockingEnv(copy=True)
  step_policy      env.step_policy(policy), exact-f32 actor
  predict_hip_step env.step(policy.predict_hip(env, obs))
  expert_step      env.step(expert.act())

Each loop is warmed with --warmup calls first.  Where the device step is shorter than the wrapper, the figure is the host's
cost per call (the launches queue up behind one another otherwise: then it is the device's).  Uses the public wrappers only,
so the same file runs from a checkout of any commit: to compare two commits run it from both, alternating, and compare the
medians of the rounds against their spread.  One JSON object on stdout; --out appends it to a JSON-lines file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--label", default="")
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "policy_best_model_v0.npz"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa

    n = args.envs
    pol = qa.MlpPolicy.from_npz(args.weights)

    def timed(env, call):
        """us per call of `call()`: --warmup calls, then the host clock around --calls calls and a device synchronise"""
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call()
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) * 1e6 / args.calls
        env.close()
        return us

    def fresh(**kw):
        env = qa.VecDockingEnv("docking-v0", num_envs=n, seed=11, **kw)
        env.reset()
        return env

    res = {}
    for name, copy in (("step_nocopy", False), ("step_copy", True)):
        env = fresh(copy=copy)
        a = env.random_actions(1)[0]
        res[name] = timed(env, lambda: env.step(a))
    env = fresh(copy=False)
    res["step_policy"] = timed(env, lambda: env.step_policy(pol))
    env = fresh(copy=False)
    last = [env.reset()]

    def predict_and_step():
        last[0] = env.step(pol.predict_hip(env, last[0]))[0]
    res["predict_hip_step"] = timed(env, predict_and_step)
    env = fresh(copy=False)
    ex = qa.PIDExpert(env)
    res["expert_step"] = timed(env, lambda: env.step(ex.act()))
    line = dict(label=args.label, root=ROOT, envs=n, calls=args.calls, device=torch.cuda.get_device_name(0), us_per_call=res)
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
