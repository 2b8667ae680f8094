#!/usr/bin/env python3
"""The PPO2 update on one MI355X: stream time per update (all Adam steps of one roll-out's schedule) of

  f  fused   quadsim_amd.ppo2_update (qsp_update: per step a gradient kernel over slices x 2 workgroups, a reduction, clip + Adam)
  t  torch   quadsim_amd.torch_ppo2_update: per step a gather, the loss of ppo2.py:147-188 on library GEMMs, autograd, the clip
             and tf.train.AdamOptimizer's formula

on the same device, the same synthetic roll-out (random observations and actions, the policy's own neglogp and values plus noise)
and the same schedule (minibatch_schedule, on the device before the window opens for both).  Cells envs x n_steps / nminibatches x
noptepochs: the reference's 10 x 600 / 10 x 10; 256 x 600 / 10 x 10; 65 536 x 32 / 4 x 1 and / 32 x 1; and one step at batch 16,
600 and 65 536.  Then `slices` in {1, 8, 32, 128, 512, auto} at three batch sizes, fused alone.

The two alternate for --rounds rounds after a warm-up round, in this order in odd rounds and reversed in even ones; every figure
is stream time between two events around one update, reported per round and as a [min, max] range, never a mean.  One JSON line
per (cell, round) on stdout, everything in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import plan_timing  # noqa: E402  (tools/ is the script's directory)

CELLS = ((10, 600, 10, 10), (256, 600, 10, 10), (65536, 32, 4, 1), (65536, 32, 32, 1))
ONE_STEP = (16, 600, 65536)
SWEEP_BATCHES = (600, 15360, 65536)
SWEEP_SLICES = (1, 8, 32, 128, 512, "auto")
HP = dict(learning_rate=3e-4, cliprange=0.2, cliprange_vf=None, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-torch-above", type=int, default=1 << 62, help="rows of a roll-out above which the torch side is left out")
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa
    from ppo2_train import sb2_actor_critic_weights

    dev = torch.device("cuda", 0)

    def synthetic(n, seed=2):
        g = torch.Generator().manual_seed(seed)
        obs = ((torch.rand(n, 12, generator=g) - 0.5) * 4.0).to(dev)
        pol = qa.ActorCriticPolicy(sb2_actor_critic_weights(1))
        noise = torch.randn(n, 4, generator=g).to(dev)
        act, val, _, nl = pol.step(obs, noise=noise)
        ret = val + 0.5 * torch.randn(n, generator=g).to(dev)
        return dict(obs=obs, actions=act.contiguous(), returns=ret.contiguous(), values=val.contiguous(), neglogp=nl.contiguous())

    def window(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop)

    def cell_rounds(cell, data, idx, sides):
        rows = []
        pols = {name: qa.ActorCriticPolicy(sb2_actor_critic_weights(1)) for name, _ in sides}
        for rnd in range(args.rounds + 1):                       # round 0 warms every cell up and is not reported
            row = dict(cell, round=rnd)
            for name, fn in (sides if rnd % 2 else sides[::-1]):
                torch.cuda.synchronize()
                row[name + "_ms"] = window(lambda: fn(pols[name], data, idx))
            if rnd:
                rows.append(row)
                print(json.dumps(row), flush=True)
        for p in pols.values():
            assert bool(torch.isfinite(p.w1).all())
        return rows

    def fused(slices):
        return lambda p, data, idx: qa.ppo2_update(p, data, idx, slices=slices, check_indices=False, **HP)

    def loop(p, data, idx):
        qa.torch_ppo2_update(p, data, idx, **HP)

    results, summary = [], []
    shapes = [dict(envs=e, n_steps=t, nminibatches=m, noptepochs=k, rows=e * t, batch=e * t // m, steps=m * k) for e, t, m, k in CELLS]
    shapes += [dict(envs=0, n_steps=0, nminibatches=1, noptepochs=1, rows=max(b, 65536), batch=b, steps=1) for b in ONE_STEP]
    for cell in shapes:
        data = synthetic(cell["rows"])
        gen = torch.Generator().manual_seed(3)
        if cell["envs"]:
            idx = qa.minibatch_schedule(cell["rows"], cell["nminibatches"], cell["noptepochs"], gen, dev)
        else:
            idx = torch.randperm(cell["rows"], generator=gen)[:cell["batch"]].to(torch.int32).view(1, -1).to(dev)
        sides = (("f_fused", fused("auto")),) + ((("t_torch", loop),) if cell["rows"] <= args.skip_torch_above else ())
        rows = cell_rounds(cell, data, idx, sides)
        results += rows
        keys = [k for k in ("f_fused_ms", "t_torch_ms") if k in rows[0]]
        rg = plan_timing.ranges(rows, keys)
        s = dict(cell, slices=qa.ppo2.auto_slices(cell["batch"]), rounds=len(rows), **rg,
                 f_us_per_step=[x * 1e3 / cell["steps"] for x in rg["f_fused_ms"]])
        if "t_torch_ms" in rg:
            spread = max(rg[k][1] - rg[k][0] for k in keys)
            s.update(t_us_per_step=[x * 1e3 / cell["steps"] for x in rg["t_torch_ms"]], t_over_f=plan_timing.ratio_range(rows, "t_torch_ms", "f_fused_ms"),
                     spread_ms=spread, f_faster_than_t_in_every_round_by_more_than_the_spread=all(r["t_torch_ms"] - r["f_fused_ms"] > spread for r in rows))
        summary.append(s)
        print(json.dumps(dict(summary=s)), flush=True)
        del data
    sweep = []
    for batch in SWEEP_BATCHES:
        data = synthetic(max(batch, 65536))
        idx = torch.randperm(max(batch, 65536), generator=torch.Generator().manual_seed(4))[:batch].to(torch.int32).view(1, -1).to(dev)
        sides = tuple(("slices_%s" % s, fused(s)) for s in SWEEP_SLICES)
        rows = cell_rounds(dict(batch=batch, steps=1), data, idx, sides)
        rg = plan_timing.ranges(rows, [n + "_ms" for n, _ in sides])
        sweep.append(dict(batch=batch, auto=qa.ppo2.auto_slices(batch), rounds=len(rows), **rg))
        print(json.dumps(dict(sweep=sweep[-1])), flush=True)
    plan_timing.write_out(args.out, torch, rounds=results, summary=summary, slices_sweep=sweep)


if __name__ == "__main__":
    main()
