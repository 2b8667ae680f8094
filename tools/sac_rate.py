#!/usr/bin/env python3
"""The SAC update on one MI355X: stream time of

  d  device  sac_update (qss_update: one launch of four workgroups per update, between two copies)
  t  torch   torch_sac_update: per update the gathers, ten forward passes of library GEMMs, autograd four times, Adam's formula and
             the Polyak average tensor by tensor
  g  td3     td3_update (qstd_update, policy_delay 2) of the same number of updates at the same batch: the yardstick

per update at batch 10 x 100 updates (the reference's rhythm), 64 (SB2 SAC's default), 128 and 256 x 100 updates, and a 4096-update
call at batch 10, on the same device, replay, schedule and noise.  The sides alternate for --rounds rounds after a warm-up round, in
this order in odd rounds and reversed in even ones; every figure is stream time between two events, reported per round and as a
[min, max] range, never a mean.  One JSON line per (cell, round) on stdout, everything in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plan_timing  # noqa: E402  (tools/ is the script's directory)

CELLS = ((10, 100), (64, 100), (128, 100), (256, 100), (10, 4096))       # (batch, updates of a call)
REPLAY = 50000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sac", "sac_rate.json"))
    ap.add_argument("--max-steps", type=int, default=4096)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa

    dev = torch.device("cuda", 0)

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    g = torch.Generator().manual_seed(7)
    obs0 = ((torch.rand(REPLAY, 12, generator=g) - 0.5) * 6.0).to(dev)
    replay = (obs0, (torch.rand(REPLAY, 4, generator=g) * 2.0 - 1.0).to(dev), torch.randn(REPLAY, generator=g).to(dev),
              (obs0 + 0.1 * torch.randn(REPLAY, 12, generator=g).to(dev)).contiguous(), (torch.rand(REPLAY, generator=g) < 0.01).float().to(dev))

    results, summary = [], []
    for batch, steps in CELLS:
        if steps > args.max_steps:
            continue
        idx = qa.replay_schedule(REPLAY, steps, batch, torch.Generator().manual_seed(3))
        noise = torch.randn((steps, batch, 4), generator=torch.Generator().manual_seed(5)).to(dev)
        pols = {k: qa.SACPolicy(seed=1, device=dev) for k in "dt"}
        yard = qa.TD3Policy(seed=1, device=dev)
        sides = (("d_device", lambda: qa.sac_update(pols["d"], replay, idx, noise=noise)),
                 ("t_torch", lambda: qa.torch_sac_update(pols["t"], replay, idx, noise=noise)),
                 ("g_td3", lambda: qa.td3_update(yard, replay, idx, noise=noise)))
        cell = dict(kind="update", batch=batch, steps=steps)
        rows = []
        for rnd in range(args.rounds + 1):                       # round 0 warms every cell up and is not reported
            row = dict(cell, round=rnd)
            for name, fn in (sides if rnd % 2 else sides[::-1]):
                torch.cuda.synchronize()
                row[name + "_ms"] = window(fn)
            if rnd:
                rows.append(row)
                print(json.dumps(row), flush=True)
        results += rows
        keys = ["d_device_ms", "t_torch_ms", "g_td3_ms"]
        rg = plan_timing.ranges(rows, keys)
        s = dict(cell, rounds=len(rows), **rg)
        spread = max(rg[k][1] - rg[k][0] for k in ("d_device_ms", "t_torch_ms"))
        s["t_torch_over_d_device"] = plan_timing.ratio_range(rows, "t_torch_ms", "d_device_ms")
        s["d_device_over_g_td3"] = plan_timing.ratio_range(rows, "d_device_ms", "g_td3_ms")
        s["d_device_faster_than_t_torch_in_every_round_by_more_than_the_spread"] = all(r["t_torch_ms"] - r["d_device_ms"] > spread for r in rows)
        for k in keys:
            s[k[:-3] + "_us_per_step"] = [x * 1e3 / steps for x in s[k]]
        summary.append(s)
        print(json.dumps(dict(summary=s)), flush=True)
    plan_timing.write_out(args.out, torch, rounds=results, summary=summary)


if __name__ == "__main__":
    main()
