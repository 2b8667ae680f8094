#!/usr/bin/env python3
"""The fit of the learned dynamics net on one MI355X: stream time per fit of

  f  fused   DynamicsNet.fit (qsdf_fit: every Adam step of the fit in one launch of one workgroup)
  t  torch   the loop train_dynamic of examples/mpc_learned.py: per step randint, two gathers, the target, predict_delta
             (normalise, three linear + ReLU), the mean squared error, backward, torch.optim.Adam.step

on the same device and the same buffer (65 536 rows of random observations, actions and small deltas).  Cells: the net
h1 x h2 in {200x100 (the reference's), 128x128, 64x64} at iters 100, batch 128, plus the 200x100 net at iters 1 and 1000.

The two alternate for --rounds rounds after a warm-up round, in this order in odd rounds and reversed in even ones; every
figure is stream time per fit between two events around --reps fits, reported per round and as a [min, max] range, never a
mean.  The condition this tool reports on, per cell: (f) faster than (t) in EVERY round, by more than the round-to-round spread
(max - min) of either.  One JSON line per (cell, round) on stdout, everything in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import plan_timing  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="200x100x100,128x128x100,64x64x100,200x100x1,200x100x1000", help="h1 x h2 x iters, comma separated")
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2, help="fits inside one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa
    from mpc_learned import train_dynamic

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(2)
    buf_x = ((torch.rand(args.rows, 16, generator=g) - 0.5) * 4.0).to(dev)
    buf_d = (torch.randn(args.rows, 12, generator=g) * 0.05).to(dev)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.reps

    results = []
    for cell in args.cells.split(","):
        h1, h2, iters = (int(x) for x in cell.split("x"))
        nets = []
        for _ in range(2):
            net = qa.DynamicsNet(h1, h2, device=dev, seed=1)
            net.set_normalisers(in_mean=buf_x.mean(0), in_std=buf_x.std(0), out_mean=buf_d.mean(0), out_std=buf_d.std(0))
            nets.append(net)
        for p in nets[1].parameters():
            p.requires_grad_(True)
        opt = torch.optim.Adam(nets[1].parameters(), lr=1.0e-4)

        def fused():
            nets[0].fit(buf_x, buf_d, args.rows, iters=iters, batch=args.batch, lr=1.0e-4, seed=3)

        def loop():
            train_dynamic(nets[1], opt, buf_x, buf_d, args.rows, iters=iters, batch=args.batch)

        order = (("f_fused", fused), ("t_torch", loop))
        for rnd in range(args.rounds + 1):                   # round 0 warms every cell up and is not reported
            row = dict(h1=h1, h2=h2, iters=iters, batch=args.batch, round=rnd)
            for name, fn in (order if rnd % 2 else order[::-1]):
                torch.cuda.synchronize()
                row[name + "_ms"] = window(fn)
            row["t_over_f"] = row["t_torch_ms"] / row["f_fused_ms"]
            row["f_us_per_step"] = row["f_fused_ms"] * 1e3 / iters
            if rnd:
                results.append(row)
                print(json.dumps(row), flush=True)
    summary = []
    keys = ("f_fused_ms", "t_torch_ms", "t_over_f", "f_us_per_step")
    for h1, h2, iters in sorted({(r["h1"], r["h2"], r["iters"]) for r in results}):
        rows = [r for r in results if (r["h1"], r["h2"], r["iters"]) == (h1, h2, iters)]
        rg = plan_timing.ranges(rows, keys)
        spread = max(rg["f_fused_ms"][1] - rg["f_fused_ms"][0], rg["t_torch_ms"][1] - rg["t_torch_ms"][0])
        summary.append(dict(h1=h1, h2=h2, iters=iters, batch=args.batch, rounds=len(rows), **rg, spread_ms=spread,
                            f_faster_than_t_in_every_round_by_more_than_the_spread=all(r["t_torch_ms"] - r["f_fused_ms"] > spread for r in rows)))
        print(json.dumps(dict(summary=summary[-1])), flush=True)
    plan_timing.write_out(args.out, torch, batch=args.batch, rows=args.rows, rounds=results, summary=summary)


if __name__ == "__main__":
    main()
