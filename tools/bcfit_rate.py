#!/usr/bin/env python3
"""Behaviour cloning of the actor on one MI355X: stream time per launch's worth of Adam steps of

  f  fused   quadsim_amd.bc_fit (qsbc_fit: every step of the schedule in one launch of one workgroup)
  t  torch   torch_steps of examples/pretrain_policy.py: per step a gather, three linear + ReLU, the mean squared error, backward,
             torch.optim.Adam.step

on the same device, the same dataset (65 536 rows of random observations and actions) and the same schedule (epoch_schedule, on
the device before the window opens for both).  Cells batch x steps: 10 x 256 (the reference's batch), 64 x 256 (SB2's default),
256 x 256, 64 x 1 (one step) and 10 x 4096 (the largest launch).  An epoch is ceil(0.7 rows / batch) steps.

The two alternate for --rounds rounds after a warm-up round, in this order in odd rounds and reversed in even ones; every
figure is stream time between two events around --reps runs of the schedule, reported per round and as a [min, max] range, never
a mean.  The condition this tool reports on, per cell: (f) faster than (t) in EVERY round, by more than the round-to-round spread
(max - min) of either.  One JSON line per (cell, round) on stdout, everything in --out."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import plan_timing  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", default="10x256,64x256,256x256,64x1,10x4096", help="batch x steps, comma separated")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2, help="runs of the schedule inside one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa
    from quadsim_amd import bc
    from pretrain_policy import sb2_actor_weights, torch_steps

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(2)
    obs = ((torch.rand(args.rows, 12, generator=g) - 0.5) * 4.0).to(dev)
    act = (torch.rand(args.rows, 4, generator=g) * 2.0 - 1.0).to(dev)
    n_train = int(0.7 * args.rows)

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
        batch, steps = (int(x) for x in cell.split("x"))
        pos, counts = qa.epoch_schedule(n_train, batch, -(-steps * batch // n_train), torch.Generator().manual_seed(3))
        pos, counts = pos[:steps].contiguous(), counts[:steps].contiguous()
        idx_d, cnt_d, cnt_h = pos.to(dev), counts.to(dev), counts.tolist()
        pols = [qa.MlpPolicy(sb2_actor_weights(1)) for _ in range(2)]
        ws = bc.actor_tensors(pols[0])
        m, v = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
        loss = torch.empty(steps, dtype=torch.float32, device=dev)
        six = lambda ts: (C.c_void_p * 6)(*[t.data_ptr() for t in ts])     # noqa: E731
        net = bc.QsbcNet(C.sizeof(bc.QsbcNet), 0, six(ws), six(m), six(v))
        lib = bc.load_bc()
        params = [getattr(pols[1], k).requires_grad_(True) for k in bc.ACTOR_KEYS]
        opt = torch.optim.Adam(params, lr=1.0e-4)
        done = [0]

        def fused():
            # the raw entry point on the schedule already on the device: bc_fit's host work (the index check and the upload) is
            # outside the window for both sides
            bc.check_bc(lib.qsbc_fit(C.byref(net), obs.data_ptr(), act.data_ptr(), args.rows, idx_d.data_ptr(), cnt_d.data_ptr(), steps,
                                     batch, 1.0e-4, 0.9, 0.999, 1.0e-8, done[0], loss.data_ptr(), None,
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)), "qsbc_fit")
            done[0] += steps

        def loop():
            torch_steps(params, opt, obs, act, idx_d, cnt_h)

        order = (("f_fused", fused), ("t_torch", loop))
        for rnd in range(args.rounds + 1):                   # round 0 warms every cell up and is not reported
            row = dict(batch=batch, steps=steps, round=rnd)
            for name, fn in (order if rnd % 2 else order[::-1]):
                torch.cuda.synchronize()
                row[name + "_ms"] = window(fn)
            per_epoch = -(-n_train // batch)
            row["t_over_f"] = row["t_torch_ms"] / row["f_fused_ms"]
            row["f_us_per_step"] = row["f_fused_ms"] * 1e3 / steps
            row["t_us_per_step"] = row["t_torch_ms"] * 1e3 / steps
            row["f_ms_per_epoch"] = row["f_us_per_step"] * per_epoch / 1e3
            row["t_ms_per_epoch"] = row["t_us_per_step"] * per_epoch / 1e3
            if rnd:
                results.append(row)
                print(json.dumps(row), flush=True)
        assert bool(torch.isfinite(loss).all())
    summary = []
    keys = ("f_fused_ms", "t_torch_ms", "t_over_f", "f_us_per_step", "t_us_per_step", "f_ms_per_epoch", "t_ms_per_epoch")
    for batch, steps in sorted({(r["batch"], r["steps"]) for r in results}):
        rows = [r for r in results if (r["batch"], r["steps"]) == (batch, steps)]
        rg = plan_timing.ranges(rows, keys)
        spread = max(rg["f_fused_ms"][1] - rg["f_fused_ms"][0], rg["t_torch_ms"][1] - rg["t_torch_ms"][0])
        summary.append(dict(batch=batch, steps=steps, steps_per_epoch=-(-n_train // batch), rounds=len(rows), **rg, spread_ms=spread,
                            f_faster_than_t_in_every_round_by_more_than_the_spread=all(r["t_torch_ms"] - r["f_fused_ms"] > spread for r in rows)))
        print(json.dumps(dict(summary=summary[-1])), flush=True)
    plan_timing.write_out(args.out, torch, rows=args.rows, train_rows=n_train, rounds=results, summary=summary)


if __name__ == "__main__":
    main()
