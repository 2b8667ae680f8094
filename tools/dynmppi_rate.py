#!/usr/bin/env python3
"""MPPI through the learned 16 -> 200 -> 100 -> 12 dynamics net on one MI355X: N x paths in {1, 64, 4096} x {200, 1024} and
1 x 65536, iterations in {1, 2, 4}, horizon 20.

  m  fused      learned_mppi_plan (qsdm_mppi_plan: per iteration one roll-out launch and one update launch)
  a  composed   the same plan from torch calls on the same device: per iteration torch.randn + clamp around the nominal, the
                `horizon`-step loop of tools/dynplan_rate.py (concat, normalise, three linear + ReLU, de-normalise, float64
                score) and the softmax-weighted mean of the candidates
  b  shooting   learned_shooting_plan (qsd_shooting_plan) at the same `paths`: the same 444 MFMAs per wave and model step, uniform
                draws instead of normals, an arg-max instead of the update

The three alternate for --rounds rounds after a warm-up round, in this order in odd rounds and reversed in even ones; every
figure is stream time per call between two events around --reps calls, reported per round and as a [min, max] range, never a
mean.  The condition this tool reports on: (m) faster than (a) in EVERY round of EVERY cell.  Recorded, not gated: (m) per
iteration over (b).  One JSON line per (cell, round) on stdout, everything in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plan_timing  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="1x200,1x1024,64x200,64x1024,4096x200,4096x1024,1x65536", help="N x paths, comma separated")
    ap.add_argument("--iterations", default="1,2,4")
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls inside one timed window")
    ap.add_argument("--lam", type=float, default=None)
    ap.add_argument("--sigma", type=float, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa
    from quadsim_amd import mpc

    H = args.horizon
    lam = mpc.MPPI_DEFAULT_LAMBDA if args.lam is None else args.lam
    sigma = mpc.MPPI_DEFAULT_SIGMA if args.sigma is None else args.sigma
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
    for cell in args.cells.split(","):
        n, paths = (int(x) for x in cell.split("x"))
        obs = ((torch.rand(n, 12, generator=g) - 0.5) * 4.0).to(dev)
        for iters in [int(x) for x in args.iterations.split(",")]:

            def fused():
                return qa.learned_mppi_plan(net, obs, H, paths, iters, lam, sigma, seed=3, k=7)["actions"]

            def shooting():
                return qa.learned_shooting_plan(net, obs, H, paths, seed=3, k=7)["actions"]

            def composed():
                with torch.no_grad():
                    U = torch.zeros(n, H, 4, device=dev)
                    for _ in range(iters):
                        cand = torch.clamp(U[:, None] + sigma * torch.randn(n, paths, H, 4, device=dev), -1.0, 1.0)
                        cand[:, 0] = torch.clamp(U, -1.0, 1.0)
                        acts = cand.view(n * paths, H, 4)
                        s = obs.repeat_interleave(paths, dim=0)
                        score = torch.zeros(n * paths, dtype=torch.float64, device=dev)
                        for h in range(H):
                            score -= (s[:, 0:3] * s[:, 0:3]).sum(1).double()
                            if h + 1 < H:
                                s = net.predict(s, acts[:, h])
                        w = torch.softmax(score.view(n, paths) / lam, dim=1)
                        U = (w[:, :, None, None] * cand.double()).sum(1).float()
                    return U[:, 0]

            order = (("m_fused", fused), ("a_composed", composed), ("b_shooting", shooting))
            for rnd in range(args.rounds + 1):               # round 0 warms every cell up and is not reported
                row = dict(envs=n, paths=paths, iterations=iters, horizon=H, round=rnd, model_steps=n * paths * (H - 1) * iters)
                for name, fn in (order if rnd % 2 else order[::-1]):
                    torch.cuda.synchronize()
                    row[name + "_ms"], _ = window(fn)
                row["a_over_m"] = row["a_composed_ms"] / row["m_fused_ms"]
                row["m_per_iteration_over_b"] = row["m_fused_ms"] / iters / row["b_shooting_ms"]
                row["m_g_model_steps_per_s"] = row["model_steps"] / row["m_fused_ms"] / 1e6
                if rnd:
                    results.append(row)
                    print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        del obs
    summary = []
    keys = ("m_fused_ms", "a_composed_ms", "b_shooting_ms", "a_over_m", "m_per_iteration_over_b", "m_g_model_steps_per_s")
    for n, paths, iters in sorted({(r["envs"], r["paths"], r["iterations"]) for r in results}):
        rows = [r for r in results if (r["envs"], r["paths"], r["iterations"]) == (n, paths, iters)]
        summary.append(dict(envs=n, paths=paths, iterations=iters, rounds=len(rows), **plan_timing.ranges(rows, keys),
                            m_faster_than_a_in_every_round=all(r["m_fused_ms"] < r["a_composed_ms"] for r in rows)))
        print(json.dumps(dict(summary=summary[-1])), flush=True)
    print(json.dumps(dict(m_faster_than_a_in_every_round_of_every_cell=all(s["m_faster_than_a_in_every_round"] for s in summary))), flush=True)
    plan_timing.write_out(args.out, torch, lam=lam, sigma=sigma, rounds=results, summary=summary)


if __name__ == "__main__":
    main()
