#!/usr/bin/env python3
"""The TRPO update on one MI355X: stream time of

  d  device  trpo_policy_step (qst_policy_step: gradient, cg_iters + 1 Fisher-vector products, CG and line search without a host
             round trip) and trpo_vf_fit (qst_vf_fit: every Adam step of the value tower in one launch)
  t  torch   torch_trpo_policy_step (double backprop of the mean KL, every CG and line-search scalar through the host, as SB2 has it)
             and torch_trpo_vf_fit (an autograd loop)

per policy step and per value fit (vf_iters = 3 passes of batch 128) at the reference's shape (1024 rows, 10 CG iterations), at 6 000
rows and at 65 536 x 32 rows, on the same device and roll-out.  The sides alternate for --rounds rounds after a warm-up round, in this
order in odd rounds and reversed in even ones; every figure is stream time between two events (the torch path's host waits fall
inside its window: they are part of that path), reported per round and as a [min, max] range, never a mean.  One JSON line per
(cell, round) on stdout, everything in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (1024, 6000, 65536 * 32)


def he_towers(seed=0):
    import numpy as np
    from quadsim_amd.ppo2 import SLOT_KEYS, SLOT_SHAPES
    rng = np.random.default_rng(seed)
    out = {}
    for key, shape in zip(SLOT_KEYS, SLOT_SHAPES):
        if len(shape) == 2:
            out[key] = (rng.standard_normal(shape) * np.sqrt(2.0 / shape[0]) * (0.1 if key == "w2" else 1.0)).astype(np.float32)
        else:
            out[key] = np.zeros(shape, np.float32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trpo", "trpo_rate.json"))
    ap.add_argument("--max-rows", type=int, default=ROWS[-1])
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

    results, summary = [], []
    for n in ROWS:
        if n > args.max_rows:
            continue
        g = torch.Generator().manual_seed(7)
        pols = {k: qa.ActorCriticPolicy(he_towers(1), device=dev) for k in "dt"}
        obs = torch.randn(n, 12, generator=g).to(dev)
        with torch.no_grad():
            mean, value = pols["d"]._heads(obs)
        rollout = {"obs": obs, "actions": (mean + torch.randn(n, 4, generator=g).to(dev)).contiguous(),
                   "values": value.contiguous(), "returns": (value + torch.randn(n, generator=g).to(dev)).contiguous()}
        idx = qa.vf_schedule(n, 128, 3, torch.Generator().manual_seed(3), dev)
        if idx.shape[0] > 4096:
            idx = idx[:4096].contiguous()
        accepted = {}

        def step(side, fn):
            accepted[side] = fn(pols[side[0]], rollout)["stats"]

        cells = (("policy_step", (("d_device", lambda: step("d", qa.trpo_policy_step)), ("t_torch", lambda: step("t", qa.torch_trpo_policy_step)))),
                 ("vf_fit", (("d_device", lambda: qa.trpo_vf_fit(pols["d"], rollout, idx, check_indices=False)),
                             ("t_torch", lambda: qa.torch_trpo_vf_fit(pols["t"], rollout, idx)))))
        for kind, sides in cells:
            rows = []
            for rnd in range(args.rounds + 1):
                order = sides if rnd % 2 else sides[::-1]
                ms = {name: window(fn) for name, fn in order}
                if rnd == 0:
                    continue                                                 # the warm-up round: allocations, first launches
                row = dict(kind=kind, rows=n, vf_steps=int(idx.shape[0]), round=rnd, ms=ms)
                if kind == "policy_step":
                    row["accepted"] = {s: float(v[8]) for s, v in accepted.items()}
                rows.append(row)
                print(json.dumps(row), flush=True)
            rng = {name: [min(r["ms"][name] for r in rows), max(r["ms"][name] for r in rows)] for name, _ in sides}
            spread = max(hi - lo for lo, hi in rng.values())
            faster = all(r["ms"]["t_torch"] - r["ms"]["d_device"] > spread for r in rows)
            summary.append(dict(kind=kind, rows=n, vf_steps=int(idx.shape[0]), ms_range=rng, speedup_range=[
                min(r["ms"]["t_torch"] / r["ms"]["d_device"] for r in rows), max(r["ms"]["t_torch"] / r["ms"]["d_device"] for r in rows)],
                device_faster_in_every_round_by_more_than_the_spread=faster))
            results += rows
    out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, cg_iters=10, fvp_stride=5, vf_batch=128, vf_iters=3, summary=summary,
               results=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for s in summary:
        print(json.dumps(s))


if __name__ == "__main__":
    main()
