"""A/B of the two host-ordered private-queue step paths at the bench's shape: the resident step kernel (one dispatch per queue,
one descriptor per qs_step) against the packet chain (one AQL dispatch per qs_step and queue, QS_RESIDENT=0).

    python tools/resident_ab.py [--envs 65536] [--steps 2000] [--queues 1] [--reps 3]

Each leg runs in a fresh child process (QS_RESIDENT is read at qs_set_queue_mode), interleaved, and prints one JSON line:
wall us per step of K raw qs_step calls + the draining qs_sync, the host-side cost of the issue loop alone (the qs_step calls,
timed without the drain: with the resident kernel a call writes one 64-B descriptor), and the resident dispatches issued."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    import ctypes as C
    import time
    sys.path.insert(0, ROOT)
    import torch
    import quadsim_amd as qa
    env = qa.VecDockingEnv("docking-v0", num_envs=a.envs, randomise=1, seed=1234, init_range=qa.C3_INIT_RANGE, copy=False)
    env.reset()
    pool = env.random_actions(min(512, max(1, (1 << 29) // (a.envs * 16))), step0=0)
    env.set_queue_mode(True, a.queues, ordering="host")
    lib, h = env._lib, env._h
    lib.qs_debug_chain_resident.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    p = lambda t: C.c_void_p(t.data_ptr())             # noqa: E731
    args = (p(env._obs), p(env._rew), p(env._done), p(env._flags), p(env._term))
    seq = [p(pool[k % pool.shape[0]]) for k in range(a.steps)]
    qs = lib.qs_step
    for k in range(a.warmup):
        qs(h, seq[k % len(seq)], *args)
    env.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in seq:
        qs(h, s, *args)
    t1 = time.perf_counter()
    env.sync()
    t2 = time.perf_counter()
    d = C.c_uint64(0)
    lib.qs_debug_chain_resident(h, C.byref(d))
    print(json.dumps({"resident": os.environ.get("QS_RESIDENT", "1") != "0", "envs": a.envs, "queues": a.queues, "steps": a.steps,
                      "us_per_step": (t2 - t0) * 1e6 / a.steps, "issue_us_per_call": (t1 - t0) * 1e6 / a.steps,
                      "resident_dispatches": int(d.value)}))
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--queues", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    base = [sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs), "--steps", str(a.steps), "--warmup",
            str(a.warmup), "--queues", str(a.queues)]
    for _ in range(a.reps):
        for res in ("1", "0"):
            r = subprocess.run(base, env=dict(os.environ, QS_RESIDENT=res), capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit("leg QS_RESIDENT=%s failed with %d" % (res, r.returncode))
            print(r.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
