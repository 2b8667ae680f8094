"""Runner.run() throughput for both actor-critic layouts the loader reads (the shared trunk of best_model_v0 and the pi / vf
towers of ppo2_docking_621_h_30M, from the re-packed archives under tests/golden/) x both head precisions (f32, bf16x3):
65 536 docking-v0 envs, T = 32 by default, fused Runner (role-split kernel), rocRAND resets, GAE + flatten included, episode
infos off.  Each configuration: warm-up runs, then --reps timed runs between events; prints one JSON line per configuration
and writes them all to --out.

    python tools/runner_layouts_time.py [--envs 65536] [--steps 32] [--reps 20] [--layouts shared,towers] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARCHIVES = {"shared": "sb2_best_model_v0.zip", "towers": "sb2_ppo2_docking_621_h_30M.zip"}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--envs", type=int, default=65536)
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--layouts", default="shared,towers")
    p.add_argument("--precisions", default="f32,bf16x3")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    import quadsim_amd as qa
    rows = []
    for layout in a.layouts.split(","):
        model = qa.load_sb2_model(os.path.join(ROOT, "tests", "golden", ARCHIVES[layout]))
        for prec in a.precisions.split(","):
            env = qa.VecDockingEnv("docking-v0", num_envs=a.envs, randomise=1, seed=1, init_range=qa.C3_INIT_RANGE)
            runner = qa.Runner(env=env, model=model, n_steps=a.steps, gamma=0.99, lam=0.95, precision=prec,
                               collect_ep_infos=False)
            assert runner.fused
            for _ in range(a.warmup):
                runner.run()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                runner.run()
                t1.record()
                t1.synchronize()
                ms.append(t0.elapsed_time(t1))
            ms.sort()
            med = ms[len(ms) // 2]
            row = {"layout": layout, "precision": prec, "envs": a.envs, "T": a.steps, "reps": a.reps,
                   "run_ms_median": round(med, 4), "run_ms_min": round(ms[0], 4), "run_ms_max": round(ms[-1], 4),
                   "us_per_step": round(1e3 * med / a.steps, 3),
                   "genv_steps_per_s": round(a.envs * a.steps / (med * 1e-3) / 1e9, 4),
                   "device": torch.cuda.get_device_name(0)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            env.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
