#!/usr/bin/env python3
"""MPPI at N docking-v0 envs (default 4096), horizon 20, paths 200 and 1024 x iterations 1, 2 and 4, on one MI355X:

  a  plan        qs_mppi_plan: one launch for all iterations (roll-outs, weights and the weighted mean on the device)
  b  shooting    qs_shooting_plan at paths x iterations candidates: the floor -- the same roll-outs without pass 2 (the weights,
                 the regenerated candidates and the float64 sums)
  c  composed    the path (a) replaces, kernels alone, per iteration: torch normal + clamp around the nominal, a twin handle of
                 N x paths envs with the replicated state, qs_rollout(T = horizon), torch's masked float64 sum and softmax mean.
                 The replication of the state (get_state -> repeat_interleave -> set_state) is redone in front of every timed
                 window, so every window's first roll-out starts from the planner's states, and is NOT in the window (inside
                 it the twin steps on from wherever the previous roll-out left it, which costs the composed path nothing).

(a), (b) and (c) alternate for --rounds rounds after a warm-up round; every figure is reported per round and as a range, with
(a)/(b) and (c)/(a).  Timed with qs_timer_start / qs_timer_stop on the handles' stream (= torch's current stream).  The
acceptance condition of the planner: (a) below (c) in every round.  One JSON line per (paths, iterations, round) on stdout,
everything in --out, with the VGPRs, SGPRs, scratch and waves per SIMD of the four k_mppi instantiations read from the notes of
the library's gfx950 code object (through tests.kernel_notes, so pytest must be importable; llvm-readelf; the tool fails if the
ROCm LLVM tools are missing, with kernel_notes' Skipped exception) and the dynamic LDS."""
import argparse
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import plan_timing  # noqa: E402  (tools/ is the script's directory)
from tests.kernel_notes import code_object, kernel_notes  # noqa: E402


def code_object_notes(so):
    """{instantiation: vgprs, sgprs, scratch bytes, spills, waves per SIMD} of the k_mppi kernels in the library's gfx950 code
    object (gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, 8 waves at most)"""
    with tempfile.TemporaryDirectory() as d:
        notes = kernel_notes(code_object(d, so), ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size",
                                                  "vgpr_spill_count", "group_segment_fixed_size"))
    out = {}
    for name, f in notes.items():
        m = re.search(r"k_mppiILi(\d)ELb([01])EEEv", name)
        if m:
            v = f["vgpr_count"] + f["agpr_count"]
            out["k_mppi<%s, %s params>" % ("RK4" if m.group(1) == "1" else "frozen", "per-env" if m.group(2) == "1" else "nominal")] = dict(
                vgprs=v, sgprs=f["sgpr_count"], scratch_bytes=f["private_segment_fixed_size"], vgpr_spills=f["vgpr_spill_count"],
                static_lds_bytes=f["group_segment_fixed_size"], waves_per_simd=min(8, 512 // ((v + 7) // 8 * 8)))
    assert len(out) == 4, sorted(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--paths", default="200,1024")
    ap.add_argument("--iterations", default="1,2,4")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls inside one timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import quadsim_amd as qa
    from quadsim_amd import mpc

    n, H = args.envs, args.horizon
    notes = code_object_notes(qa._lib.LIB_PATH)
    print(json.dumps(dict(code_object_notes=notes)), flush=True)
    lam, sigma = mpc.MPPI_DEFAULT_LAMBDA, mpc.MPPI_DEFAULT_SIGMA
    results = []
    for paths in [int(p) for p in args.paths.split(",")]:
        m = n * paths
        env = plan_timing.stepped_env(qa, n)
        big = qa.VecDockingEnv("docking-v0", num_envs=m, seed=6)    # qs_rollout needs auto_reset; steps after a done are masked
        out = tuple(torch.empty(s, dtype=d, device=env.device) for s, d in
                    (((H, m, 12), torch.float32), ((H, m), torch.float32), ((H, m), torch.uint8)))

        def replicate():
            st = env.get_state(as_numpy=False)
            big.set_state(**{k: v.repeat_interleave(paths, dim=0) for k, v in st.items()})     # ends in a synchronisation

        nominal = torch.zeros((n, H, 4), device=env.device)
        acts = torch.empty((H, n, paths, 4), device=env.device)

        def composed(iterations):
            U = nominal
            for _ in range(iterations):
                acts.normal_()
                acts.mul_(sigma).add_(U.transpose(0, 1).unsqueeze(2)).clamp_(-1.0, 1.0)
                acts[:, :, 0] = U.transpose(0, 1).clamp(-1.0, 1.0)
                _, rew, done, _ = big.rollout(acts.view(H, m, 4), out=out + (None,), want_flags=False)
                d = done.to(torch.int32)
                alive = (torch.cumsum(d, 0) - d) == 0
                score = (rew.double() * alive).sum(0).view(n, paths)
                w = torch.softmax(score / lam, dim=1)
                U = torch.einsum("np,hnpi->nhi", w, acts.double()).float()
            return U

        window = lambda env_, fn: plan_timing.window(env_, fn, args.reps)    # noqa: E731

        for iterations in [int(i) for i in args.iterations.split(",")]:
            steps = m * H * iterations
            for rnd in range(args.rounds + 1):               # round 0 warms every shape up and is not reported
                row = dict(envs=n, paths=paths, horizon=H, iterations=iterations, round=rnd, candidate_steps=steps)
                row["a_mppi_ms"], _ = window(env, lambda: env.mppi_plan(H, paths, iterations, "reward", lam, sigma, nominal=nominal))
                row["b_shooting_ms"], _ = window(env, lambda: env.shooting_plan(H, paths * iterations, "reward"))
                replicate()
                row["c_composed_ms"], _ = window(big, lambda: composed(iterations))
                row["a_over_b"] = row["a_mppi_ms"] / row["b_shooting_ms"]
                row["c_over_a"] = row["c_composed_ms"] / row["a_mppi_ms"]
                row["a_g_steps_per_s"] = steps / row["a_mppi_ms"] / 1e6
                if rnd:
                    results.append(row)
                    print(json.dumps(row), flush=True)
        env.close(); big.close()
        del out, acts
        torch.cuda.empty_cache()
    summary = []
    for key in sorted({(r["paths"], r["iterations"]) for r in results}):
        rows = [r for r in results if (r["paths"], r["iterations"]) == key]
        summary.append(dict(paths=key[0], iterations=key[1], rounds=len(rows),
                            lds_bytes=64 + H * 200 + key[0] * 8,
                            **plan_timing.ranges(rows, ("a_mppi_ms", "b_shooting_ms", "c_composed_ms", "a_over_b", "c_over_a", "a_g_steps_per_s")),
                            a_below_c_in_every_round=all(r["a_mppi_ms"] < r["c_composed_ms"] for r in rows)))
        print(json.dumps(dict(summary=summary[-1])), flush=True)
    plan_timing.write_out(args.out, torch, lam=lam, sigma=sigma, code_object_notes=notes, rounds=results, summary=summary)

if __name__ == "__main__":
    main()
