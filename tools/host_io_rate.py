#!/usr/bin/env python3
"""Times of the C-ABI calls on QS_IO_HOST handles: wall clock around the call (each ends in a stream sync), median of K calls.

    QUADSIM_HIP_LIB=PARENT.so python tools/host_io_rate.py            the calls profiles/host_io/README.md compares with the parent
    QUADSIM_HIP_LIB=AB.so     python tools/host_io_rate.py --sweep    the same calls against the bytes they move

One JSON line per run ("RATE {...}" / "SWEEP {...}"); run the libraries alternating, three rounds or more, and take the median
of the rounds.  The two libraries of a sweep are builds with -DQS_MIRROR_BYTES=65536 (above 64 KiB every slice is copied between
the caller's array and the device buffer) and "-DQS_MIRROR_BYTES=(size_t(1)<<40)" (always one DMA each way through the pinned
mirror): kMirrorBytes in csrc/host_util.hpp is the size from which the first is never slower."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import quadsim_amd as qa  # noqa: E402
from quadsim_amd import _lib  # noqa: E402

lib = _lib.load()


def p(x):
    return x.ctypes.data_as(C.c_void_p) if x is not None else None


def tm(f, K, warm=5):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(K):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts) * 1e6), 1)


def host_handle(n):
    cfg = _lib.default_config()
    cfg.kind, cfg.num_envs, cfg.io_space, cfg.auto_reset, cfg.randomise, cfg.seed = _lib.KIND_V0, n, _lib.IO_HOST, 1, 1, 3
    cfg.init_range = (C.c_float * 4)(*qa.C3_INIT_RANGE)
    h = C.c_void_p()
    _lib.check(lib.qs_create(C.byref(cfg), C.byref(h)), "qs_create")
    obs = np.zeros((n, 12), np.float32)
    _lib.check(lib.qs_reset(h, None, p(obs)), "qs_reset")
    return h


def rollout_buffers(h, n, T):
    acts = np.zeros((T, n, 4), np.float32)
    _lib.check(lib.qs_fill_random_actions(h, T, 0, p(acts)), "qs_fill_random_actions")
    return acts, (np.zeros((T, n, 12), np.float32), np.zeros((T, n), np.float32), np.zeros((T, n), np.uint8), np.zeros((T, n), np.uint8))


def drone_buffers(m):
    rng = np.random.RandomState(0)
    s = rng.uniform(-1, 1, (m, 13)).astype(np.float32)
    s[:, 6:10] /= np.linalg.norm(s[:, 6:10], axis=1, keepdims=True)
    up = rng.uniform(-1, 1, (m, 4)).astype(np.float32)
    return s, up, up.copy(), np.zeros(m, np.uint8)


def rates():
    out = {}
    e = qa.DockingEnv()
    e.reset()

    def stp():
        o, r, d, info = e.step(np.zeros(4))
        if d:
            e.reset()
    out["shim_step_us"] = tm(stp, 500, 20)
    out["shim_reset_us"] = tm(e.reset, 300, 20)
    a, obs, rew = np.zeros((1, 4), np.float32), np.zeros((1, 12), np.float32), np.zeros(1, np.float32)
    done, flags = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    out["qs_step_n1_us"] = tm(lambda: lib.qs_step(e._h, p(a), p(obs), p(rew), p(done), p(flags), None), 1000, 20)
    ctx = qa.drone._context()
    for m in (1, 2500):
        s, up, u, lim = drone_buffers(m)
        out["drone_step_n%d_us" % m] = tm(lambda: lib.qs_drone_step(ctx, m, p(s), p(up), p(u), None, p(lim)), 500, 20)
    n, T = 4096, 128
    h = host_handle(n)
    acts, (O, R, D, F) = rollout_buffers(h, n, T)
    out["rollout_n4096_T128_us"] = tm(lambda: lib.qs_rollout(h, T, p(acts), p(O), p(R), p(D), p(F)), 15, 3)
    out["rollout_n4096_T128_noact_us"] = tm(lambda: lib.qs_rollout(h, T, None, p(O), p(R), p(D), p(F)), 15, 3)
    out["fill_actions_n4096_T128_us"] = tm(lambda: lib.qs_fill_random_actions(h, T, 0, p(acts)), 15, 3)
    out["rollout_sha"] = hashlib.sha1(O.tobytes() + R.tobytes() + D.tobytes() + F.tobytes()).hexdigest()[:12]
    lib.qs_destroy(h)
    return out


def sweep():
    out = {}
    n = 1024
    h = host_handle(n)
    for T in (8, 12, 16, 18, 20, 22, 24, 28, 32, 64):       # 70 B per env-step
        acts, (O, R, D, F) = rollout_buffers(h, n, T)
        out["rollout_%dKiB" % (T * n * 70 // 1024)] = tm(lambda: lib.qs_rollout(h, T, p(acts), p(O), p(R), p(D), p(F)), 60)
    lib.qs_destroy(h)
    n = 4096
    h = host_handle(n)
    for T in (8, 12, 16, 20, 24, 28, 32, 64):               # 16 B per env-step, output only
        acts = np.zeros((T, n, 4), np.float32)
        out["fill_%dKiB" % (T * n * 16 // 1024)] = tm(lambda: lib.qs_fill_random_actions(h, T, 0, p(acts)), 60)
    lib.qs_destroy(h)
    ctx = qa.drone._context()
    for m in (7500, 10000, 12500, 15000, 17500, 20000, 25000, 40000):      # 85 B per row, mostly in-out
        s, up, u, lim = drone_buffers(m)
        out["drone_%dKiB" % (m * 85 // 1024)] = tm(lambda: lib.qs_drone_step(ctx, m, p(s), p(up), p(u), None, p(lim)), 60)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--label", default=os.path.basename(os.environ.get("QUADSIM_HIP_LIB", "default")))
    args = ap.parse_args()
    res = {"lib": args.label}
    res.update(sweep() if args.sweep else rates())
    print(("SWEEP " if args.sweep else "RATE ") + json.dumps(res))
