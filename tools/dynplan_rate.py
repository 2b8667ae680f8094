#!/usr/bin/env python3
"""Random-shooting MPC through the learned 16 -> 200 -> 100 -> 12 dynamics net on one MI355X: N in {1, 64, 4096} observations x
paths in {200, 1024} candidates, horizon 20.

  a  fused      learned_shooting_plan (qsd_shooting_plan: one launch for every candidate and step, one small arg-max launch)
  b  composed   the same plan from torch calls on the same device: `horizon` x (concat, normalise, three linear + ReLU,
                de-normalise, score in float64) and one argmax -- DynamicsNet.predict in a loop, as the reference's
                choose_action loops over sess.run.  Its candidate actions are drawn BEFORE the timed window (the fused plan
                draws its own inside), which favours (b).

(a) and (b) alternate for --rounds rounds after a warm-up round, first (a) in odd rounds and first (b) in even ones; every
figure is stream time per call between two events around --reps calls, reported per round and as a [min, max] range, never a
mean.  The expectation this tool reports on: (a) faster than (b) in EVERY round at 1 x 200 (the reference's own shape) and at
4096 x 200; the spread between rounds is the noise measure.  One JSON line per (shape, round) on stdout, everything in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plan_timing  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1,64,4096")
    ap.add_argument("--paths", default="200,1024")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls inside one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa

    H = args.horizon
    dev = torch.device("cuda", 0)
    net = qa.DynamicsNet(200, 100, device=dev, seed=1)
    g = torch.Generator().manual_seed(2)
    net.set_normalisers(in_mean=torch.randn(16, generator=g) * 0.5, in_std=torch.rand(16, generator=g) * 1.5 + 0.5,
                        out_mean=torch.randn(12, generator=g) * 0.01, out_std=torch.rand(12, generator=g) * 0.08 + 0.02)
    net.pack()

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            r = fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.reps, r

    results = []
    for n in [int(x) for x in args.envs.split(",")]:
        for paths in [int(x) for x in args.paths.split(",")]:
            obs = ((torch.rand(n, 12, generator=g) - 0.5) * 4.0).to(dev)
            acts = (torch.rand(n * paths, H, 4, generator=g) * 2.0 - 1.0).to(dev)
            rows_i = torch.arange(n, device=dev)

            def fused():
                return qa.learned_shooting_plan(net, obs, H, paths, seed=3, k=7)["actions"]

            def composed():
                with torch.no_grad():
                    s = obs.repeat_interleave(paths, dim=0)
                    score = torch.zeros(n * paths, dtype=torch.float64, device=dev)
                    for h in range(H):
                        score -= (s[:, 0:3] * s[:, 0:3]).sum(1).double()
                        if h + 1 < H:
                            s = net.predict(s, acts[:, h])
                    best = score.view(n, paths).argmax(1)
                    return acts.view(n, paths, H, 4)[rows_i, best, 0]

            for rnd in range(args.rounds + 1):               # round 0 warms every shape up and is not reported
                row = dict(envs=n, paths=paths, horizon=H, round=rnd, model_steps=n * paths * (H - 1))
                for name, fn in ((("a_fused", fused), ("b_composed", composed)) if rnd % 2 else (("b_composed", composed), ("a_fused", fused))):
                    torch.cuda.synchronize()
                    row[name + "_ms"], _ = window(fn)
                row["b_over_a"] = row["b_composed_ms"] / row["a_fused_ms"]
                row["a_g_model_steps_per_s"] = row["model_steps"] / row["a_fused_ms"] / 1e6
                if rnd:
                    results.append(row)
                    print(json.dumps(row), flush=True)
            del acts, obs
            torch.cuda.empty_cache()
    summary = []
    for n, paths in sorted({(r["envs"], r["paths"]) for r in results}):
        rows = [r for r in results if (r["envs"], r["paths"]) == (n, paths)]
        summary.append(dict(envs=n, paths=paths, rounds=len(rows),
                            **plan_timing.ranges(rows, ("a_fused_ms", "b_composed_ms", "b_over_a", "a_g_model_steps_per_s")),
                            a_faster_than_b_in_every_round=all(r["a_fused_ms"] < r["b_composed_ms"] for r in rows)))
        print(json.dumps(dict(summary=summary[-1])), flush=True)
    plan_timing.write_out(args.out, torch, rounds=results, summary=summary)


if __name__ == "__main__":
    main()
