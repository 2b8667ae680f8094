#!/usr/bin/env python3
"""bench.py -- env-steps/s of the fused docking env.step() hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: run as is -- the parent spawns one child per GPU before it touches the GPU -- or under
     python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...)

A "step" is one pass of the hot path over the batch: every env of this GPU stepped once through the step API (state
round-trips through HBM every step, U(-1,1) random actions already resident in HBM, rocRAND randomised auto-reset).  The
workload follows BASELINE.json's configs by GPU count unless --env / --envs-per-gpu / --randomise say otherwise:
    N = 1, 2: config 3   65 536 docking-v0 envs per GPU, randomised init state            (392 B per env-step)
    N = 4:    config 4   262 144 docking-v2 envs = 65 536 per GPU, randomised init state  (392 B)
    N = 8:    config 5   1 048 576 docking-v2 envs = 131 072 per GPU, + per-env mass / inertia domain randomisation (408 B)
Envs shard over GPUs by env id with no data-path collective (scaling "weak"); the RCCL all-gather of roll-out slabs that
configs 4/5 name is timed separately and reported under "allgather", never mixed into `value`.

ONE clock: `value`, `ms_per_step` and `roofline.achieved / frac / read_frac` all come from the same host wall-clock
interval (barrier + synchronize on both sides, max over ranks).  The interval holds EXACTLY K = --steps steps after W =
--warmup untimed ones; the synchronisation that closes it costs ~30 us, so the per-step time is only meaningful over a few
thousand steps (a 20-step interval is shorter than that synchronisation).  Beside it, under their own names: the
HIP-event time of the same launches (`roofline.gpu_timeline_*`), the in-kernel s_memrealtime timeline of the same chain
from the committed stamped-build run (`roofline.stamp_*`) and the rocprofv3 kernel average of the committed profile
(`roofline.rocprof_*`, computed from the launch shape that profile was TAKEN with -- its sidecar json).

What the headline mode is and is not: with --queue-mode auto/private the timed loop is a pre-staged
random-action ROLL-OUT -- qs_step packets back to back on the handle's private AQL queue(s), no end-of-kernel release, the
outputs of a step consumable after the roll-out (qs_sync, or the stream-ordered hand-shake of qs_rollout_stepwise), not
between two steps.  The rate a per-step `obs -> policy -> env.step` loop gets is `hip_stream_mode` (every launch releases)
and `policy_between_steps`; `config.mode` / `config.outputs_consumable` say so in the line.

Prints ONE JSON line (rank 0) with the headline and its "roofline" (derived from the same clock and the committed profiles;
no run of its own).  A plain run does nothing else: it sets up, picks and settles the launch path, warms up, times the K
steps, writes the last step's outputs if --dump-outputs DIR is given, and prints the line.  --full adds every other leg:
"parity" (fixtures g4 / g5 / g7 / g1 = outputs of the NumPy reference replayed through the C ABI), "cpu_baseline" (the C
oracle on the host cores + what the reference itself would reach there), "config1", "hip_stream_mode",
"actions_cache_resident", "policy_between_steps", "rollout_stepwise", "step_api_131072_envs", ...; its side legs time R =
ceil(--min-timed-steps / K) blocks of K steps each.

--dump-outputs DIR: what the timed path handed its caller in its last timed step (qs_step's observation, reward, done, flags
and terminal observation) as float32 DIR/<name>.npy, at most 64 MB in all (above that, a fixed seeded sample of env rows,
their ids in env_index.npy).  The timed steps start from the env's state right after its reset, restored after the
launch-path probes and the settling steps, so the same arguments give the same outputs in every run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec peak
BYTES_PER_ENV_STEP = 392       # read 176 B + write 216 B per env-step (step-API mode)
BYTES_PER_ENV_STEP_DR = 408    # + mass, Ixx, Iyy, Izz read (per-env params)
READ_TARGET = 0.40             # north_star / SURVEY.md 8(d): >= 40 % of the HBM-read roofline <=> 18.2 G env-steps/s
PROFILE_DIRS = [os.path.join(ROOT, "profiles", d) for d in ("r03", "r02")]    # newest first

# BASELINE.json configs by GPU count (run_docking_ppo2.py:65-67 is the reference's only parallelism: envs over workers)
CONFIGS = {
    1: dict(tag="config 3", env="docking-v0", envs_per_gpu=65536, randomise=1,
            text="65 536 parallel docking-v0 envs, random actions, SoA tiles + rocRAND randomised auto-reset"),
    2: dict(tag="config 3 per GPU (x2)", env="docking-v0", envs_per_gpu=65536, randomise=1,
            text="65 536 parallel docking-v0 envs per GPU, random actions, SoA tiles + rocRAND randomised auto-reset"),
    4: dict(tag="config 4", env="docking-v2", envs_per_gpu=65536, randomise=1,
            text="262 144 docking-v2 envs (moving target + random init) sharded over 4 GPUs = 65 536 per GPU; the RCCL all-gather "
                 "of roll-out slabs is the separate `allgather` leg"),
    8: dict(tag="config 5", env="docking-v2", envs_per_gpu=131072, randomise=2,
            text="1 048 576 docking-v2 envs with per-env mass / inertia domain randomisation sharded over 8 GPUs = 131 072 per "
                 "GPU (408 B per env-step); the RCCL all-gather of roll-out slabs is the separate `allgather` leg"),
}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--warmup", type=int, default=200)
    p.add_argument("--envs-per-gpu", type=int, default=None, help="default: BASELINE's config for --gpus (see the docstring)")
    p.add_argument("--env", default=None, choices=["docking-v0", "docking-v2"], help="default: by --gpus")
    p.add_argument("--integrator", default="frozen", choices=["frozen", "rk4"])
    p.add_argument("--randomise", type=int, default=None, help="0 nominal resets, 1 rocRAND init state, 2 + mass/inertia; default: by --gpus")
    p.add_argument("--action-pool", type=int, default=512, help="distinct pre-generated [N,4] action batches cycled")
    p.add_argument("--groups", type=int, default=-1,
                   help="env groups in flight (qs_set_groups): 1 = one launch per step; G > 1 = G chains on G streams, "
                        "each with a native launcher thread; -1 = the default of this build (see DESIGN.md section 5)")
    p.add_argument("--group-threads", type=int, default=1, help="0: issue the group launches from the calling thread")
    p.add_argument("--queues", type=int, default=2, help="private queues with --queue-mode private (1..4)")
    p.add_argument("--queue-mode", default="auto", choices=["auto", "hip", "private"],
                   help="private: step launches on an AQL queue owned by the handle, without HIP's end-of-kernel cache write-back "
                        "(qs_set_queue_mode; bit-identical results; a pre-staged roll-out: outputs consumable after it, not per "
                        "step); hip: ordinary launches on the HIP stream; auto: private if it opens AND reproduces the HIP-stream "
                        "chain bit for bit on this machine, else hip")
    p.add_argument("--min-timed-steps", type=int, default=2000,
                   help="--full side legs: their timed interval holds R = ceil(this / K) back-to-back blocks of K steps")
    p.add_argument("--rollout-T", type=int, default=64, help="steps per launch of the fused roll-out leg")
    p.add_argument("--full", action="store_true",
                   help="run every leg beside the headline too (parity, CPU baseline, other modes / sizes / precisions)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the outputs of the last timed step to DIR/<name>.npy (float32, at most 64 MB)")
    p.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline / config1")
    p.add_argument("--no-extras", action="store_true", help="with --full: skip every leg but the headline (and parity / cpu_baseline)")
    p.add_argument("--no-parity", action="store_true", help="with --full: skip the parity leg")
    p.add_argument("--cpu-seconds", type=float, default=12.0)
    p.add_argument("--repeats", type=int, default=1, help="timed intervals of K steps each; the median one is reported")
    p.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                   help="nccl (= RCCL over xGMI, the real thing) or gloo (rehearsal of the multi-rank control flow, "
                        "e.g. several ranks sharing one GPU; skips the all-gather leg)")
    p.add_argument("--spawn-timeout", type=float, default=1500.0)
    args = p.parse_args()
    cfg = CONFIGS.get(args.gpus, CONFIGS[2] if args.gpus < 4 else (CONFIGS[4] if args.gpus < 8 else CONFIGS[8]))
    args.config_tag = cfg["tag"] if (args.env is None and args.envs_per_gpu is None and args.randomise is None) else None
    args.config_text = cfg["text"]
    if args.env is None:
        args.env = cfg["env"]
    if args.envs_per_gpu is None:
        args.envs_per_gpu = cfg["envs_per_gpu"]
    if args.randomise is None:
        args.randomise = cfg["randomise"]
    return args


DEFAULT_GROUPS = 1   # measured on MI355X (profiles/r02/groups_sweep.txt): more chains in flight do not raise the rate
SETTLE_STEPS = 2000  # untimed steps on the chosen launch path before the headline's own warm-up (see settle_and_restart)


# --------------------------------------------------------------------------------------------------------------------
# self-launch: `python bench.py --gpus N` with no launcher around it
# --------------------------------------------------------------------------------------------------------------------
def spawn_ranks(args):
    """WORLD_SIZE unset and --gpus N > 1: start N children (one per GPU) BEFORE this process touches the GPU, wait for
    them, exit with the worst return code.  Rank 0's child prints the JSON line on the inherited stdout."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), QS_BENCH_CHILD="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    deadline = time.time() + args.spawn_timeout
    rc = 0
    try:
        for p in procs:
            left = max(1.0, deadline - time.time())
            try:
                rc = rc or p.wait(timeout=left)
            except subprocess.TimeoutExpired:
                rc = rc or 124
            if rc:
                break              # a failed / hung rank: do not wait for peers stuck in a collective
    finally:
        for p in procs:            # stragglers: the exact PIDs started above, nothing else
            if p.poll() is None:
                p.terminate()
        for p in procs:
            if p.poll() is None:
                try:
                    p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill()
    return rc


# --------------------------------------------------------------------------------------------------------------------
# CPU legs (the oracle as the measured baseline; test infrastructure, never on the product path)
# --------------------------------------------------------------------------------------------------------------------
def cpu_baseline(kind, seconds, seed=1234):
    """The C oracle (oracle/quadsim_oracle.c, f64 build == the reference's float64 arithmetic restated)
    timed on the host cores, one thread per core (ctypes releases the GIL), same workload shape:
    U(-1,1) actions, auto-reset with randomised init.  Bounded sample."""
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from oracle.pyoracle import Oracle, PAR_NOMINAL
    orc = Oracle("f64")
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 64))
    n, T = 1024, 50
    rr = (0.5, 0.1, 0.2, 0.1, 1.0, 1.0, 1.0, 1.0)
    rs = np.random.RandomState(seed)
    acts = rs.uniform(-1, 1, (T, n, 4))

    def worker(w):
        rec = orc.env_init(n)
        par = np.tile(np.array(PAR_NOMINAL, np.float64), (n, 1))
        orc.vec_reset(rec, par, randomise=1, seed=seed, gid0=w * n, rr=rr)
        done_steps, k = 0, 0
        t_end = time.perf_counter() + seconds
        while time.perf_counter() < t_end:
            orc.vec_rollout(rec, par, acts, kind=kind, randomise=1, seed=seed, step_idx0=k, gid0=w * n, rr=rr)
            k += T
            done_steps += n * T
        return done_steps

    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        total = sum(ex.map(worker, range(cores)))
    dt = time.perf_counter() - t0
    cpu_model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu_model = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "unknown")
    except OSError:
        pass
    out = {"value": total / dt, "unit": "env-steps/s", "cores": cores, "cpu_model": cpu_model, "kind": "port",
           "sample": "C oracle (f64 restatement of the reference path), %d threads x 1024 envs, U(-1,1) actions, "
                     "randomised auto-reset, %.1f s wall" % (cores, dt)}
    # the NumPy twin (oracle/np_oracle.py: the same closed form as array code), one process, 4 096 envs per call
    import warnings
    from oracle import np_oracle
    rec = orc.env_init(4096)
    a4 = rs.uniform(-1, 1, (4096, 4))
    k, t0 = 0, time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        while time.perf_counter() - t0 < 2.0:
            rec2, _, _, d, _ = np_oracle.env_step(rec, a4, kind=kind)
            rec = np.where(d[:, None], rec, rec2)            # finished envs restart from the nominal record
            k += 1
    out["numpy_twin"] = {"value": k * 4096 / (time.perf_counter() - t0), "unit": "env-steps/s", "cores": 1,
                         "what": "oracle/np_oracle.py, float64, 4 096 envs per vectorised call"}
    # relate the port's rate to the TRUE reference.  oracle/calibrate_cpu.py measured, on one core of
    # the build container (where the reference can be imported), port rate / reference rate; the reference itself would
    # therefore reach about value / ratio on these host cores.
    try:
        with open(os.path.join(ROOT, "oracle", "cpu_calibration.json")) as f:
            cal = json.load(f)
        c = cal["docking-v0" if kind == 0 else "docking-v2"]
        out["reference_equivalent"] = {"value": out["value"] / c["ratio"], "unit": "env-steps/s", "cores": cores,
                                       "ratio_port_over_reference": c["ratio"],
                                       "reference_env_steps_per_s_one_core": c["reference_env_steps_per_s"],
                                       "source": "oracle/cpu_calibration.json (oracle/calibrate_cpu.py: C oracle vs the imported "
                                                 "NumPy/SciPy reference, one core, build container, %s)" % cal["host"].get("cpu", "?")}
    except (OSError, KeyError, ValueError):
        out["reference_equivalent"] = None
    return out


def config1_cpu(seconds=2.0):
    """BASELINE config 1 (1 env, CPU only) on the build's CPU oracle, one core: the run_sim_PID.py:43-54 loop
    (fixture g6's set-up) and a docking-v0 episode with the hover action a = (-0.5)^4, both as single C calls; and the
    same episode driven per step through ctypes (what a Python caller of a C env pays).  SURVEY.md section 8(d) c1."""
    import numpy as np
    from oracle.pyoracle import Oracle, PAR_NOMINAL
    orc = Oracle("f64")
    out = {"cores": 1, "kind": "port", "what": "C oracle (f64), one env, one host core; the true Python reference runs "
                                               "600-720 env-steps/s per core (BASELINE.md section 2)"}
    g6 = os.path.join(ROOT, "tests", "golden", "g6_sim_pid.npz")
    if os.path.exists(g6):
        with np.load(g6) as z:
            s0, sdes = z["ini_state"].copy(), z["state_des"].copy()
    else:
        s0 = np.zeros(13); s0[2] = 5.0; s0[6] = 1.0
        sdes = s0.copy(); sdes[0:3] = (1.0, 1.0, 6.0)
    T, n_calls = 2000, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        orc.sim_pid(T, s0, sdes)
        n_calls += 1
    out["sim_pid_loop_steps_per_s"] = n_calls * T / (time.perf_counter() - t0)
    # docking-v0, hover action, one episode per C call (auto-reset keeps it going through the 600-step time-out)
    Te = 600
    acts = np.full((Te, 1, 4), -0.5)
    rec = orc.env_init(1)
    par = np.tile(np.array(PAR_NOMINAL, np.float64), (1, 1))
    n_calls = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        orc.vec_rollout(rec, par, acts, kind=0)
        n_calls += 1
    out["docking_v0_hover_steps_per_s"] = n_calls * Te / (time.perf_counter() - t0)
    # the same env stepped one ctypes call per step from Python (gym-style driver loop)
    rec1 = orc.env_init(1)[0]
    a = np.full(4, -0.5)
    k = 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < min(seconds, 1.0):
        rec1, _, _, done, _ = orc.env_step(rec1, a)
        if done:
            rec1 = orc.env_init(1)[0]
        k += 1
    out["docking_v0_hover_python_loop_steps_per_s"] = k / (time.perf_counter() - t0)
    return out


# --------------------------------------------------------------------------------------------------------------------
# parity: the BASELINE metric's second half ("per-step state L2 err vs NumPy ref")
# --------------------------------------------------------------------------------------------------------------------
def parity_vs_reference(qa, device):
    """The metric's second half, for every fixture family the reference produced (oracle/gen_goldens.py), replayed through
    the C ABI with inputs rounded to float32 -- each recorded reference step becomes env s of ONE batch and is stepped once:
      g4  1 500 steps each of docking-v0 / -v2 under random and near-hover actions (27 + 13 episodes, over-limit ends)
      g5  the 600-step docking-v0 episode driven by the shipped policy: 183 docked steps, ends by time-out
      g7  six trajectories with patched mass / inertia (per-env params path), v0 and v2
      g1  2 500 adversarial Drone.step cases: 1 712 attitude-limiter hits, 1 166 active rotor clamps (qs_drone_step)
    Outside the timed region; the oracle is not involved."""
    import numpy as np
    gold = os.path.join(ROOT, "tests", "golden")
    out = {"source": "tests/golden/g{4,5,7,1}*.npz = outputs of the NumPy reference (oracle/gen_goldens.py)",
           "tolerance": "north_star: 1e-5 relative per step (float32)"}
    worst = {"state_l2_rel": 0.0, "obs_l2_rel": 0.0, "obs_abs_err": 0.0, "obs_err_over_tolerance": 0.0, "reward_abs_scaled": 0.0}
    l2 = lambda a, b: np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30)   # noqa: E731

    def env_family(g, env_id, prefix="", par=None):
        n = len(g[prefix + "rec_before"])
        env = qa.VecDockingEnv(env_id, num_envs=n, device=device, auto_reset=False)
        rec = g[prefix + "rec_before"].astype(np.float32)
        env.set_state(chaser=rec[:, 0:13], target=rec[:, 13:26], u_prev=rec[:, 26:34], qdes=rec[:, 34:38],
                      last_shaping=rec[:, 38], t=rec[:, 39])
        if par is not None:
            env.set_params(np.full(n, par[0], np.float32), np.tile(np.asarray(par[1:4], np.float32), (n, 1)))
        obs, rew, done, infos = env.step(g[prefix + "actions"].astype(np.float32))
        flags = infos.flags
        st = env.get_state()
        obs, rew, done = obs.cpu().numpy().astype(np.float64), rew.cpu().numpy().astype(np.float64), done.cpu().numpy()
        env.close()
        ref = g[prefix + "rec_after"]
        e_c = l2(st["chaser"].astype(np.float64), ref[:, 0:13])
        e_t = l2(st["target"].astype(np.float64), ref[:, 13:26])
        e_o = l2(obs, g[prefix + "obs"])
        # element-wise, in units of the tests' tolerance (rtol 1e-5 + atol 2e-5): the relative position is a DIFFERENCE of two
        # ~50 m positions, which float32 state holds to 4e-6 m each -- an absolute floor, however small the difference itself is
        # (a docked chaser sits 0.07 m from the port: 4e-6 m is 6e-5 of that, and nothing in the arithmetic can win it back)
        e_oa = np.abs(obs - g[prefix + "obs"])
        e_ot = (e_oa / (2e-5 + 1e-5 * np.abs(g[prefix + "obs"]))).max(axis=1)
        e_r = np.abs(rew - g[prefix + "reward"]) / np.maximum(1.0, np.abs(ref[:, 38]))
        # done / flags are decided by thresholds: exclude the steps the reference itself decides within 1e-4 of one
        rmax = 3.0 if env_id == "docking-v0" else 10.0
        npos = np.linalg.norm(g[prefix + "obs"][:, 0:3], axis=1)
        nvel = np.linalg.norm(g[prefix + "obs"][:, 3:6], axis=1)
        margin = np.minimum(np.abs(npos - rmax), np.abs(ref[:, 2] - 0.1))
        flips = int(np.sum((done != g[prefix + "done"].astype(bool)) & (margin > 1e-4)))
        dmargin = np.minimum(np.minimum(np.abs(npos - 0.1), np.abs(nvel - 0.1)),
                             np.min(np.abs(np.abs(g[prefix + "obs"][:, 6:9]) - np.deg2rad(10.0)), axis=1))
        dock_flips = int(np.sum(((flags & 1) != (g[prefix + "flags"].astype(np.uint8) & 1)) & (dmargin > 1e-4)))
        r = {"steps": n, "chaser_state_l2_rel_max": float(e_c.max()), "target_state_l2_rel_max": float(e_t.max()),
             "state_l2_rel_mean": float(0.5 * (e_c.mean() + e_t.mean())), "obs_l2_rel_max": float(e_o.max()),
             "obs_l2_rel_mean": float(e_o.mean()), "obs_abs_err_max": float(e_oa.max()), "obs_err_over_tolerance_max": float(e_ot.max()),
             "reward_abs_over_max1shaping_max": float(e_r.max()),
             "done_flips_outside_1e-4_margin": flips, "docked_flag_flips_outside_1e-4_margin": dock_flips,
             "docked_steps": int((flags & 1).sum()), "done_steps": int(done.sum())}
        worst["state_l2_rel"] = max(worst["state_l2_rel"], r["chaser_state_l2_rel_max"], r["target_state_l2_rel_max"])
        worst["obs_l2_rel"] = max(worst["obs_l2_rel"], r["obs_l2_rel_max"])
        worst["obs_abs_err"] = max(worst["obs_abs_err"], r["obs_abs_err_max"])
        worst["obs_err_over_tolerance"] = max(worst["obs_err_over_tolerance"], r["obs_err_over_tolerance_max"])
        worst["reward_abs_scaled"] = max(worst["reward_abs_scaled"], r["reward_abs_over_max1shaping_max"])
        return r

    def load(name):
        path = os.path.join(gold, name + ".npz")
        if not os.path.exists(path):
            return None
        with np.load(path) as z:
            return {k: z[k] for k in z.files}

    fams, flips_total = {}, 0
    for name, env_id in (("g4_traj_v0", "docking-v0"), ("g4_traj_v2", "docking-v2")):
        g = load(name)
        if g is None:
            return None
        fams.setdefault("g4_trajectories", {})[env_id] = env_family(g, env_id)
    g = load("g5_policy_episode")
    if g is not None:
        fams["g5_policy_episode_docked_and_timeout"] = env_family(g, "docking-v0")
    g = load("g7_domain_rand")
    if g is not None:
        fams["g7_mass_inertia"] = {}
        for kind, env_id in ((0, "docking-v0"), (1, "docking-v2")):
            for j in range(3):
                key = "k%d_s%d_" % (kind, j)
                fams["g7_mass_inertia"]["%s/set%d" % (env_id, j)] = env_family(g, env_id, prefix=key, par=g[key + "par"])
    g = load("g1_drone_step")
    if g is not None:
        s2, up2, lim = qa.drone_step_batch(g["state"], g["u_prev"], g["u"], dt=float(g["dt"]), device=device)
        safe = g["margin"] > 1e-4                # fp32 cannot decide a limiter knife-edge closer than this
        e_s = l2(s2[safe].astype(np.float64), g["state_out"][safe])
        e_u = np.abs(up2[safe].astype(np.float64) - g["u_prev_out"][safe]).max(axis=1) / np.maximum(1.0, np.abs(g["u_prev_out"][safe]).max(axis=1))
        fams["g1_drone_step_limiter_and_clamps"] = {
            "cases": int(safe.sum()), "limiter_hits": int(g["limited"][safe].sum()),
            "limiter_flag_mismatches_outside_1e-4_margin": int(np.sum(lim[safe] != g["limited"][safe].astype(bool))),
            "state_l2_rel_max": float(e_s.max()), "state_l2_rel_mean": float(e_s.mean()), "limited_control_abs_scaled_max": float(e_u.max())}
        worst["state_l2_rel"] = max(worst["state_l2_rel"], float(e_s.max()))
    out["families"] = fams

    def walk(d):
        for v in d.values():
            if isinstance(v, dict):
                if "done_flips_outside_1e-4_margin" in v:
                    yield v["done_flips_outside_1e-4_margin"] + v["docked_flag_flips_outside_1e-4_margin"]
                else:
                    yield from walk(v)
    flips_total = sum(walk(fams)) + fams.get("g1_drone_step_limiter_and_clamps", {}).get("limiter_flag_mismatches_outside_1e-4_margin", 0)
    out.update(worst)
    out["decision_flips_outside_margin"] = int(flips_total)
    out["criteria"] = ("state: L2-relative error per step <= 1e-5 (the metric's `per-step state L2 err`); obs: every element within "
                       "rtol 1e-5 + atol 2e-5 (obs_err_over_tolerance <= 1; obs_l2_rel is reported too but is not a criterion: on docked "
                       "steps the observation itself is ~0.07 and float32 positions of ~50 m resolve its position part to 4e-6); reward: "
                       "|error| <= 2e-5 max(1, |shaping|); no done / docked / limiter decision flipped outside a 1e-4 margin of its threshold")
    out["within_tolerance"] = bool(worst["state_l2_rel"] <= 1e-5 and worst["obs_err_over_tolerance"] <= 1.0
                                   and worst["reward_abs_scaled"] <= 2e-5 and flips_total == 0)
    return out


# --------------------------------------------------------------------------------------------------------------------
def profile_file(fname):
    """newest committed profile directory that holds fname"""
    for d in PROFILE_DIRS:
        path = os.path.join(d, fname)
        if os.path.exists(path):
            return path
    return None


def rocprof_kernel_average(kernel_substr, fname):
    """(average us, calls, relative path, sidecar dict) of the step kernel in a committed `rocprofv3 --kernel-trace --stats`
    summary.  The sidecar <fname minus .csv>.json records the launch shape the profile was TAKEN with (queue mode, queues, envs
    per launch): the bytes of one launch come from there, never from what this run happens to use."""
    import csv
    path = profile_file(fname)
    if not path:
        return None
    side = {}
    try:
        with open(path[:-4] + ".json") as f:
            side = json.load(f)
    except (OSError, ValueError):
        pass
    try:
        with open(path) as f:
            for row in csv.DictReader(f):
                if kernel_substr in row.get("Name", ""):
                    return float(row["AverageNs"]) / 1e3, int(row["Calls"]), os.path.relpath(path, ROOT), side
    except (OSError, KeyError, ValueError):
        pass
    return None


DUMP_BYTES = 64 * 1000 * 1000 - 4096      # --dump-outputs: all files of one run together, .npy headers included
DUMP_SEED = 20251015                       # the env-row sample above that size: the same rows in every run


def dump_outputs(path, env, rank, world, lo):
    """--dump-outputs: the arrays the timed path handed its caller in its last step -- qs_step's observation, reward, done,
    flags and terminal observation (rows of envs that did not finish zeroed: a caller only reads it where done) -- as float32
    .npy files.  Above the budget, a fixed seeded sample of env rows, sorted, with their global env ids in env_index.npy.
    Several ranks: each writes its own shard as rank<r>_<name>.npy within its share of the budget.  Called after the timed
    interval has been drained and synchronised (time_steps)."""
    import numpy as np
    n = env.num_envs
    done = env._done.cpu().numpy().astype(bool)
    arrays = {"obs": env._obs.cpu().numpy(),
              "reward": env._rew.cpu().numpy(),
              "done": done.astype(np.float32),
              "flags": env._flags.cpu().numpy().astype(np.float32),
              "terminal_obs": np.where(done[:, None], env._term.cpu().numpy(), np.float32(0.0)).astype(np.float32)}
    row_bytes = sum(a.nbytes for a in arrays.values()) // n
    budget = DUMP_BYTES // world - 1024 * (len(arrays) + 1)
    idx = np.arange(n)
    if n * row_bytes > budget:
        m = budget // (row_bytes + 8)
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, m, replace=False))
        arrays = {k: v[idx] for k, v in arrays.items()}
        arrays["env_index"] = (lo + idx).astype(np.float64)
    os.makedirs(path, exist_ok=True)
    prefix = "" if world == 1 else "rank%d_" % rank
    for k, v in arrays.items():
        np.save(os.path.join(path, prefix + k + ".npy"), np.ascontiguousarray(v))
    return {"dir": path, "files": sorted(prefix + k + ".npy" for k in arrays), "envs": int(len(idx)),
            "sampled": bool(len(idx) < n), "step": "last timed step"}


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))          # the parent never initialises the GPU

    # stdout carries the ONE JSON line and nothing else: whatever libraries print there while the bench runs (the RCCL
    # version banner, gloo's connection messages) goes to stderr instead -- fd 1 is pointed at fd 2 until the line is due
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d but --gpus=%d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    ndev = torch.cuda.device_count()
    if args.backend == "gloo":
        local_rank = local_rank % ndev          # rehearsal: ranks may share a GPU
    elif local_rank >= ndev:
        raise SystemExit("--gpus %d with backend nccl needs %d visible GPUs, found %d (use --backend gloo to rehearse "
                         "the multi-rank control flow on fewer)" % (args.gpus, args.gpus, ndev))
    torch.cuda.set_device(local_rank)
    distributed = world > 1 or bool(os.environ.get("QS_BENCH_FORCE_DIST"))   # the env hook rehearses the RCCL path on one GPU
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    import ctypes as C
    import quadsim_amd as qa
    from quadsim_amd import C3_INIT_RANGE, VecDockingEnv, shard_range

    n = args.envs_per_gpu
    total_envs = n * world
    lo, hi = shard_range(total_envs, rank, world)
    assert hi - lo == n
    kind = 0 if args.env == "docking-v0" else 1
    groups = DEFAULT_GROUPS if args.groups < 0 else max(1, args.groups)

    def make_env(integrator, num=n, offset=lo, env_id=None, randomise=None):
        return VecDockingEnv(env_id or args.env, num_envs=num, device=local_rank, integrator=integrator,
                             randomise=args.randomise if randomise is None else randomise,
                             seed=1234, env_id_offset=offset, init_range=C3_INIT_RANGE, mass_scale=(0.8, 1.2),
                             inertia_scale=(0.8, 1.2), copy=False)

    def barrier():
        torch.cuda.synchronize()
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if not distributed:
            return x
        t = torch.tensor([x], dtype=torch.float64, device="cuda" if args.backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def time_steps(env, K, R, W, pool, G=1):
        """W untimed steps, then ONE timed interval of R blocks of exactly K steps, barrier + synchronize on both sides.
        -> (wall seconds, max over ranks; HIP-event ms on the launching stream(s) of the same launches)"""
        lib, h = env._lib, env._h
        P = pool.shape[0]
        aptr = [C.c_void_p(pool[i].data_ptr()) for i in range(P)]
        obs, rew, done, flags, term = (env._ptr(env._obs), env._ptr(env._rew), env._ptr(env._done),
                                       env._ptr(env._flags), env._ptr(env._term))
        # the host loop is as lean as Python allows (a private-queue step takes the GPU ~5 us: a lambda and a modulo per step
        # would make the interpreter the bottleneck): the action pointers of the K steps are laid out beforehand
        seq = [aptr[k % P] for k in range(K * R)]
        for k in range(W):
            (lib.qs_step_groups(h, aptr[k % P], obs, rew, done, flags, term, None) if G > 1 else
             lib.qs_step(h, aptr[k % P], obs, rew, done, flags, term))
        barrier()
        err = None
        try:
            env.timer_start()                # event on the main stream; group streams are ordered behind it
            t0 = time.perf_counter()
            if G > 1:
                qs = lib.qs_step_groups
                for a in seq:
                    qs(h, a, obs, rew, done, flags, term, None)
            else:
                qs = lib.qs_step
                for a in seq:
                    qs(h, a, obs, rew, done, flags, term)
            ev_ms = env.timer_stop()         # joins the group streams / drains the private queues, records the stop event
        except qa.QuadsimError as ex:        # the private queues' placement guard (reported by the draining call)
            err, ev_ms, t0 = str(ex), float("nan"), time.perf_counter()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        if distributed:
            dist.barrier()
        if max_over_ranks(1.0 if err else 0.0) > 0.5:      # every rank raises together: the callers hold collectives
            raise qa.QuadsimError(err or "the private-queue placement guard fired on another rank")
        return max_over_ranks(wall), ev_ms

    def verify_private_queue(mk, pool, queues=1):
        """The private-queue mode rests on hardware behaviour HIP does not promise (block -> XCD placement).  Before it is
        used for a timed leg it has to open on this machine AND reproduce the HIP-stream chain bit for bit: two fresh envs,
        the same 96 steps (auto-resets included), every output of the last step and the whole final state compared."""
        a, b = mk(), mk()
        try:
            a.reset(); b.reset()
            b.set_queue_mode(True, queues, ordering="host")
            for k in range(96):
                oa, ra, da, _ = a.step(pool[k % pool.shape[0]])
                ob, rb, db, _ = b.step(pool[k % pool.shape[0]])
            torch.cuda.synchronize(); b.sync()
            same = bool(torch.equal(oa, ob) and torch.equal(ra, rb) and torch.equal(da, db))
            sa, sb = a.get_state(as_numpy=False), b.get_state(as_numpy=False)
            same = same and all(torch.equal(sa[k], sb[k]) for k in sa) and a.step_counter == b.step_counter
            return same, "ok" if same else "the private-queue chain differs from the HIP-stream chain"
        except Exception as ex:                                    # noqa: BLE001  (any failure means: do not use the mode)
            return False, "%s: %s" % (type(ex).__name__, ex)
        finally:
            a.close(); b.close()

    def pick_launch_path(env, mk, pool, probe):
        """candidates: the HIP stream and 1..3 private queues (host-ordered: pre-staged actions); each private candidate has to
        pass the bit-identity check on THIS machine on every rank, and the fastest one on a short probe is used (the private
        queues lose above ~200 000 envs, where the state outgrows the L2s).  -> (queue_mode, queues, note); env is left in it"""
        if args.queue_mode == "hip" or groups > 1:
            return "hip", 0, None
        cand = [int(args.queues)] if args.queue_mode == "private" else [1, 2, 3]
        best_t = time_steps(env, probe, 1, 50, pool)[0] if args.queue_mode == "auto" else float("inf")
        notes, queues = [], 0
        for q in cand:
            ok, why = verify_private_queue(mk, pool, q)
            if -max_over_ranks(-float(ok)) < 0.5:          # every rank must agree (the legs below hold collective barriers)
                notes.append("%d private queue(s) not used: %s" % (q, why if not ok else "another rank could not verify it"))
                if args.queue_mode == "private":
                    raise SystemExit("--queue-mode private: " + notes[-1])
                continue
            env.set_queue_mode(True, q, ordering="host")
            try:
                t = time_steps(env, probe, 1, 50, pool)[0]
            except qa.QuadsimError as ex:
                notes.append("%d private queue(s) not used: %s" % (q, ex))
                env.reset()
                continue
            notes.append("%d private queue(s): %.2f us per step on the probe" % (q, t / probe * 1e6))
            if t < best_t:
                best_t, queues = t, q
        if queues:
            env.set_queue_mode(True, queues, ordering="host")
        else:
            env.set_queue_mode(False)
        return ("private" if queues else "hip"), queues, "; ".join(notes)

    K, W = args.steps, args.warmup
    if K < 1 or W < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    R = max(1, -(-args.min_timed_steps // K))          # the --full side legs' blocks of K steps; the headline times K steps
    env = make_env(args.integrator)
    env.reset()
    if groups > 1:
        groups = env.set_groups(groups, threads=bool(args.group_threads))
    P = max(1, min(args.action_pool, (1 << 29) // (n * 16)))      # at most 512 MiB of action batches
    pool = env.random_actions(P, step0=0)               # [P,N,4] U(-1,1), resident in HBM before timing
    # the state right after the reset, restored before the timed steps: they start from it in every run of the same arguments,
    # whatever the probes and the settling steps did (q_des persists over resets, so a second reset would not bring it back)
    start = env.get_state(as_numpy=False)
    start_par = env.get_params() if args.randomise >= 2 else None
    queue_mode, queues, queue_note = pick_launch_path(env, lambda: make_env(args.integrator), pool, 1000)

    def settle_and_restart():
        """the first ~2 000 steps of a newly opened launch path run a few per cent slower than the rest: they are stepped here,
        untimed, then the env is put back to its post-reset state and step counter 0"""
        time_steps(env, SETTLE_STEPS, 1, 0, pool, groups)
        env.set_state(**start)
        if start_par is not None:
            env.set_params(*start_par)
        env.step_counter = 0

    try:
        settle_and_restart()
        runs = [time_steps(env, K, 1, W, pool, groups) for _ in range(max(1, args.repeats))]
        guard = None
    except qa.QuadsimError as ex:
        # the private queue's placement guard fired while timing (seen when several processes share one GPU: another process's
        # queues in flight change where the dispatcher deals the workgroups): the handle failed loudly, as designed -- the
        # release-free chain cannot be used here, so the HIP-stream chain is what is timed (time_steps raises on every rank)
        if queue_mode != "private":
            raise
        guard = str(ex)
    if guard is not None:
        queue_note = ((queue_note + "; ") if queue_note else "") + (
            "private queues ABANDONED during timing: %s -- timed on the HIP stream instead" % guard)
        queue_mode, queues = "hip", 0
        try:
            env.set_queue_mode(False)
        except qa.QuadsimError:
            env.set_queue_mode(False)                       # the first call reports the pending error, the second switches
        settle_and_restart()
        runs = [time_steps(env, K, 1, W, pool, groups) for _ in range(max(1, args.repeats))]
    if args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, env, rank, world, lo)
    order = sorted(range(len(runs)), key=lambda i: runs[i][0])
    wall, ev_ms = runs[order[len(order) // 2]]
    steps_timed = K
    steps_side = K * R
    value = total_envs * steps_timed / wall
    bpe = BYTES_PER_ENV_STEP_DR if args.randomise >= 2 else BYTES_PER_ENV_STEP
    rbpe = 176 if bpe == 392 else 192
    step_us = wall * 1e6 / steps_timed
    achieved = bpe * n / (step_us * 1e-6) / 1e9          # GB/s per GPU: algorithmic bytes of one step / wall time of one step
    ev_us = ev_ms * 1e3 / steps_timed
    split = n <= 131072
    kname = "k_env_split" if split else "k_env<"
    frac_of = lambda us, b=bpe, nn=n: b * nn / (us * 1e-6) / 1e9 / HBM_PEAK_GBS      # noqa: E731

    if groups > 1:
        mode_text = ("step-API: one qs_step_groups call per step = %d launches (env groups of %d envs on %d streams, %s), "
                     "bit-identical to qs_step" % (groups, n // groups, groups, "one launcher thread per group" if args.group_threads
                                                   else "issued by the calling thread"))
        consumable = "per step, in stream order (qs_groups_join)"
    elif queue_mode == "private":
        mode_text = ("step-API, pre-staged random-action ROLL-OUT: one qs_step call per step = one AQL packet per private queue of "
                     "the handle (%d queue(s), each stepping a contiguous range of tiles; a packet is ordered behind the previous step "
                     "of its queue, acquires at agent scope and carries NO end-of-kernel release: a tile's state stays in the L2 of the "
                     "XCD that steps it; verified bit-identical to the HIP-stream chain on this machine before timing; requires the "
                     "hardware's round-robin workgroup->XCD placement, checked per tile in-kernel, else the handle fails loudly and "
                     "`hip_stream_mode` is what remains)" % queues)
        consumable = ("after the roll-out (qs_sync, or the stream-ordered hand-shake of qs_rollout_stepwise: `rollout_stepwise`), NOT "
                      "between two steps; a per-step obs -> policy -> env.step loop runs at `hip_stream_mode` / `policy_between_steps`")
    else:
        mode_text = "step-API: one qs_step launch per step on the HIP stream"
        consumable = "per step, in stream order"
    tag = args.config_tag
    workload = ("BASELINE %s: %s" % (tag, args.config_text)) if tag else (
        "custom (flags override BASELINE's config for %d GPU(s)): %d parallel %s envs per GPU, U(-1,1) random actions, randomise %d"
        % (world, n, args.env, args.randomise))
    out = {
        "metric": "env-steps/sec at N parallel envs (1/2/4/8 GPU); per-step state L2 err vs NumPy ref",
        "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": K, "warmup": W,
        "ms_per_step": wall * 1e3 / steps_timed, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "timed_region": {"steps_timed": steps_timed, "wall_s": wall,
                         "policy": "median of %d interval(s); each = %d untimed + %d timed steps between barrier + "
                                   "synchronize; value, ms_per_step and roofline.frac all derive from this one wall clock"
                                   % (len(runs), W, K),
                         "env_steps_per_s_all_intervals": [total_envs * steps_timed / r[0] for r in runs]},
        "config": {"workload": workload, "baseline_config": tag,
                   "envs_per_gpu": n, "total_envs": total_envs, "env": args.env, "integrator": args.integrator,
                   "dt": 0.02, "randomise": args.randomise, "action_pool_batches": P,
                   "queue_mode": queue_mode, "private_queues": queues,
                   "mode": mode_text, "outputs_consumable": consumable,
                   "groups": groups,
                   "parallelism": "env-sharded x%d, no data-path collective" % world},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                     "kernel": ("k_env_split<%s> (T=1): chaser wave + target wave + reset-preparation wave per tile (two waves where "
                                "the reset is not rocRAND's or the launch exceeds 1 365 tiles)" if split else "k_env<%s> (T=1)") % args.integrator
                               + (", dispatched from the handle's private AQL queue" if queue_mode == "private" else ""),
                     "bytes_per_env_step": bpe, "bytes_per_step": bpe * n, "launches_per_step": max(groups, queues, 1),
                     "step_period_us": step_us,
                     "read_frac": frac_of(step_us, rbpe),
                     "read_frac_target": READ_TARGET,
                     "read_frac_target_met": bool(frac_of(step_us, rbpe) >= READ_TARGET),
                     "gpu_timeline_us_per_step": ev_us,
                     "gpu_timeline_frac": frac_of(ev_us),
                     "basis": "achieved = %d B x %d envs / wall time per step (the SAME clock as value and ms_per_step); "
                              "gpu_timeline_* = HIP events around the same launches; working set %.1f MB is "
                              "Infinity-Cache resident" % (bpe, n, n * 160 / 1e6)},
    }
    c3_shape = n == 65536 and args.env == "docking-v0" and args.integrator == "frozen" and args.randomise == 1
    # (1) in-kernel timeline of the SAME chain from the committed stamped-build run (tools/stamp_timeline.py: s_memrealtime
    #     stamps held in registers; unlike rocprofv3 they leave the queue alone)
    sp = profile_file("step_kernel_timeline_private_q%d.json" % queues) if queue_mode == "private" else profile_file("step_kernel_timeline_hip.json")
    if sp and c3_shape:
        try:
            with open(sp) as f:
                st = json.load(f)
            out["roofline"].update({"stamp_period_us": st["stamp_period_us"], "stamp_kernel_span_us": st["stamp_kernel_span_us"],
                                    "stamp_gap_us": st["stamp_gap_us"], "stamp_frac": frac_of(st["stamp_period_us"]),
                                    "stamp_source": os.path.relpath(sp, ROOT),
                                    "stamp_note": "light stamped build (-DQS_STAMP=2: one workgroup in 64 records the first / last "
                                                  "s_memrealtime of its waves; steps within 1-3 %% of the product build), %s, %d-batch action "
                                                  "pool; period = consecutive starts of the same workgroups (the chain's own); span / gap are "
                                                  "approximate (span ends at 'stores issued' of the sampled workgroups)"
                                                  % ("%d private queue(s)" % st["queues"] if st.get("queues") else "HIP stream", st.get("action_pool", 0))})
        except (OSError, KeyError, ValueError):
            pass
    # (2) rocprofv3 kernel averages of the committed profiles: per-launch duration of the step kernel, with the bytes of ONE
    #     launch taken from the shape the profile was TAKEN with (sidecar json), not from this run's queue count
    if c3_shape:
        for key, fname in (("rocprof_private", "step_api_kernel_stats_private.csv"), ("rocprof_hip_stream", "step_api_kernel_stats_hip.csv"),
                           ("rocprof", "step_api_kernel_stats.csv")):
            rp = rocprof_kernel_average(kname, fname)
            if not rp or (key == "rocprof" and "rocprof_private" in out["roofline"]):
                continue
            avg_us, calls, src, side = rp
            envs_per_launch = int(side.get("envs_per_launch", n // max(int(side.get("queues", 1)), 1)))
            out["roofline"][key] = {"kernel_avg_us": avg_us, "calls": calls, "source": src,
                                    "envs_per_launch": envs_per_launch, "profiled_queue_mode": side.get("queue_mode", "private"),
                                    "profiled_queues": side.get("queues", 1),
                                    "kernel_frac": bpe * envs_per_launch / (avg_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                                    "note": side.get("note", "bytes of ONE launch / its average duration in the profiled process; rocprofv3 "
                                                             "wraps every HSA queue and adds a completion signal per dispatch, so a "
                                                             "private-queue launch is slower under the profiler than in this run")}
    # HBM-side bytes per step from the PMC passes (collected separately: rocprofv3 --pmc cannot run inside
    # this process); only quoted when the profile was taken on this very configuration
    try:
        pmc = json.load(open(profile_file("pmc_traffic.json")))
        if pmc["envs"] == n and c3_shape:
            src = pmc["private_queue"] if queue_mode == "private" and "private_queue" in pmc else pmc
            out["roofline"]["traffic"] = src["traffic_bytes_per_step"]
            out["roofline"]["traffic_source"] = pmc["source"] + ("; " + src["note"] if "note" in src else "")
            if src is not pmc:
                out["roofline"]["traffic_hip_stream_mode"] = pmc["traffic_bytes_per_step"]
    except (OSError, ValueError, KeyError, TypeError):
        pass

    if queue_note:
        out["config"]["queue_note"] = queue_note
    if args.dump_outputs:
        out["outputs"] = dumped
    # everything below the headline runs with --full only: a plain run is set-up, warm-up, the K timed steps and the line
    side_legs = args.full and not args.no_extras
    if queue_mode == "private" and side_legs:
        # the headline cycles several hundred distinct action batches (every step reads actions the caches have never seen);
        # straight behind a policy kernel the actions are cache-resident instead: the same chain with a 16-batch pool
        best = None
        try:
            for q in (1, 2):
                env.set_queue_mode(True, q, ordering="host")
                wq, _ = time_steps(env, K, R, min(W, 50), pool[:16])
                if best is None or wq < best[0]:
                    best = (wq, q)
            out["actions_cache_resident"] = {"value": total_envs * steps_side / best[0], "unit": "env-steps/s", "private_queues": best[1],
                                             "step_period_us": best[0] * 1e6 / steps_side,
                                             "frac": frac_of(best[0] * 1e6 / steps_side),
                                             "what": "16-batch action pool (%d MB) instead of the headline's %d batches (%.0f MB)"
                                                     % (16 * n * 16 // 1000000, P, P * n * 16 / 1e6)}
            env.set_queue_mode(True, queues, ordering="host")
        except qa.QuadsimError as ex:
            out["actions_cache_resident"] = {"invalid": "the placement guard fired during this leg: %s" % ex}
            env.reset()
    if queue_mode == "private" and not side_legs:
        env.set_queue_mode(False)                          # nothing below steps this env again (profiling runs: no HIP-stream twin)
    elif queue_mode == "private":
        # the same chain as ordinary HIP launches: every kernel ends with the agent-scope release, i.e. every step's outputs are
        # consumable by the next kernel on the stream -- the rate of a per-step `obs -> policy -> env.step` loop's env side
        env.set_queue_mode(False)
        wh, msh = time_steps(env, K, R, min(W, 50), pool, 1)
        out["hip_stream_mode"] = {"value": total_envs * steps_side / wh, "unit": "env-steps/s", "step_period_us": wh * 1e6 / steps_side,
                                  "frac": frac_of(wh * 1e6 / steps_side), "read_frac": frac_of(wh * 1e6 / steps_side, rbpe),
                                  "gpu_timeline_us_per_step": msh * 1e3 / steps_side,
                                  "what": "identical launches through hipLaunchKernel on the HIP stream (agent-scope release after every "
                                          "kernel: outputs consumable per step, in stream order)"}
    if args.full and not args.no_parity and rank == 0:
        out["parity"] = parity_vs_reference(qa, local_rank)

    if side_legs:
        extras(args, out, env, pool, make_env, time_steps, verify_private_queue, barrier, max_over_ranks, queue_mode, queues,
               dict(n=n, world=world, rank=rank, local_rank=local_rank, total_envs=total_envs, K=K, R=R, W=W, P=P, bpe=bpe, rbpe=rbpe,
                    groups=groups, steps_timed=steps_side, distributed=distributed))

    # the CPU legs run on rank 0 whatever the world size (they are CPU-only; the other ranks wait in the barrier below)
    if rank == 0 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(kind, args.cpu_seconds)
        out["config1"] = config1_cpu()
    elif rank == 0 and args.full:
        out["cpu_baseline"] = None
    env.close()
    if distributed:
        dist.barrier()
        dist.destroy_process_group()
    sys.stdout.flush()
    os.dup2(saved_stdout, 1)
    os.close(saved_stdout)
    if rank == 0:
        print(json.dumps(out), flush=True)


def extras(args, out, env, pool, make_env, time_steps, verify_private_queue, barrier, max_over_ranks, queue_mode, queues, X):
    """every leg beside the headline; each under its own name in the line"""
    import torch
    import torch.distributed as dist
    import quadsim_amd as qa

    def leave_private(e):
        """back to the HIP stream; a pending placement error (see main) is reported by the first call and cleared"""
        try:
            e.set_queue_mode(False)
            return None
        except qa.QuadsimError as ex:
            e.set_queue_mode(False)
            e.reset()
            return str(ex)
    n, world, rank, local_rank, total_envs = X["n"], X["world"], X["rank"], X["local_rank"], X["total_envs"]
    K, R, W, P, bpe, rbpe, groups, steps_timed = X["K"], X["R"], X["W"], X["P"], X["bpe"], X["rbpe"], X["groups"], X["steps_timed"]
    frac_of = lambda us, b=bpe, nn=n: b * nn / (us * 1e-6) / 1e9 / HBM_PEAK_GBS      # noqa: E731
    # the same step with ONE launch per step (no groups): the per-kernel view
    if groups > 1:
        env.set_groups(1)
        w1, ms1 = time_steps(env, K, R, min(W, 50), pool, 1)
        out["single_launch_per_step"] = {"value": total_envs * steps_timed / w1, "unit": "env-steps/s",
                                         "step_period_us": w1 * 1e6 / steps_timed, "frac": frac_of(w1 * 1e6 / steps_timed),
                                         "gpu_timeline_us_per_step": ms1 * 1e3 / steps_timed}
    # ---- roll-out through the step API with every step's outputs KEPT: T = 600 single-step launches per call (the reference's
    #      n_steps, run_docking_ppo2.py:95), [T,N,...] output arrays; private queues stream-ordered: ONE GPU-side hand-shake with
    #      the caller's stream and ONE release per call (qs_rollout_stepwise), no host synchronisation
    Tr = 600 if n <= 131072 else 64
    acts_r = env.random_actions(Tr, step0=0)
    ro = {}
    for mode in (("hip", "private_stream_ordered") if queue_mode == "private" else ("hip",)):
        if mode == "hip":
            env.set_queue_mode(False)
        else:
            env.set_queue_mode(True, queues, ordering="stream")
            if env.queue_ordering != "stream":
                continue
        # as everywhere in this function: a placement-guard error on ONE rank must not change the sequence of collectives
        err, bufs = None, None
        try:
            bufs = env.rollout(acts_r, stepwise=True)
        except qa.QuadsimError as ex:
            err = str(ex)
        barrier()
        t0 = time.perf_counter()
        if err is None:
            try:
                for _ in range(3):
                    env.rollout(acts_r, stepwise=True, out=bufs)
                torch.cuda.synchronize()
            except qa.QuadsimError as ex:
                err = str(ex)
        wr = max_over_ranks(time.perf_counter() - t0) / (3 * Tr)
        ro[mode] = {"value": total_envs / wr, "unit": "env-steps/s", "step_period_us": wr * 1e6, "frac": frac_of(wr * 1e6),
                    "read_frac": frac_of(wr * 1e6, rbpe)}
        del bufs
        if mode != "hip":
            err = err or leave_private(env)
        if max_over_ranks(float(bool(err))) > 0.5:
            ro[mode] = {"invalid": "the placement guard fired during this leg (several processes on one GPU?)" + (": " + err[:160] if err else " on another rank")}
            leave_private(env)
    ro["T"] = Tr
    ro["what"] = ("qs_rollout_stepwise: T single-step launches per call, outputs of all T steps kept ([T,N,12] obs, [T,N] reward / done / "
                  "flags, %.1f GB per call) and consumable in stream order when the call's hand-shake passes" % (Tr * n * 54 / 1e9))
    out["rollout_stepwise"] = ro
    del acts_r
    leave_private(env)
    # ---- policy BETWEEN the steps (rl_baselines/ppo2/ppo2.py:472-499): obs -> the shipped MlpPolicy (three torch GEMMs +
    #      activations on torch's stream) -> env.step, nothing pre-staged, no host synchronisation in either launch path
    wpath = os.path.join(ROOT, "tests", "golden", "policy_best_model_v0.npz")
    if os.path.exists(wpath):
        from quadsim_amd import MlpPolicy
        pol = MlpPolicy.from_npz(wpath, device="cuda:%d" % local_rank)
        pb = {}
        for mode in (("hip_stream", "private_stream_ordered") if queue_mode == "private" else ("hip_stream",)):
            if mode == "hip_stream":
                env.set_queue_mode(False)
            else:
                env.set_queue_mode(True, queues, ordering="stream")
                if env.queue_ordering != "stream":
                    continue
            # the placement guard may fire on ANY rank in the private mode (it did when two rehearsal ranks shared one GPU): every
            # rank runs the same sequence of collectives whatever happens, and the leg is marked invalid for all of them
            err = None
            try:
                obs = env.reset()
                for _ in range(30):
                    obs, _, _, _ = env.step(pol.predict(obs))
            except qa.QuadsimError as ex:
                err = str(ex)
            barrier()
            t0 = time.perf_counter()
            if err is None:
                try:
                    for _ in range(300):
                        obs, _, _, _ = env.step(pol.predict(obs))
                    torch.cuda.synchronize()
                except qa.QuadsimError as ex:
                    err = str(ex)
            wp = max_over_ranks(time.perf_counter() - t0) / 300
            if max_over_ranks(float(err is not None)) > 0.5:
                pb[mode] = {"invalid": "the placement guard fired during this leg%s" % (": " + err[:160] if err else " on another rank")}
                leave_private(env)
            else:
                pb[mode] = {"us_per_step": wp * 1e6, "value": total_envs / wp, "unit": "env-steps/s"}
        # the env side alone, per-step consumable, from the raw C-ABI loop: HIP stream = `hip_stream_mode`; private queue with the
        # per-step hand-shake (hipStreamWriteValue64 + hipStreamWaitValue64 per step are host-bound)
        if "us_per_step" in pb.get("private_stream_ordered", {}):
            env.set_queue_mode(True, queues, ordering="stream")
            try:
                ws, _ = time_steps(env, 500, 1, 50, pool[:16])
                pb["private_stream_ordered"]["env_step_alone_us"] = ws / 500 * 1e6
            except qa.QuadsimError as ex:
                pb["private_stream_ordered"] = {"invalid": "the placement guard fired during this leg: %s" % ex}
        leave_private(env)
        # the same per-step loop captured ONCE into a hipGraph (torch.cuda.graphs: 10 x [three GEMMs + activations + qs_step], no
        # Python, no launch calls at replay; the step counter that keys the reset RNG lives in device memory, so every replay draws
        # fresh resets) and replayed 30 times
        gr, gr_err = None, ""
        try:                                                          # capture support varies with the torch build: never cost the line
            env.set_queue_mode(False)
            env.reset()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    pol.predict(env._obs)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(10):
                    env.step(pol.predict(env._obs))
            for _ in range(3):
                gr.replay()
            torch.cuda.synchronize()
        except Exception as ex:
            gr, gr_err = None, str(ex)[:200]
        if -max_over_ranks(-float(gr is not None)) > 0.5:             # every rank captured (the timing below holds collectives)
            barrier()
            t0 = time.perf_counter()
            for _ in range(30):
                gr.replay()
            torch.cuda.synchronize()
            wp = max_over_ranks(time.perf_counter() - t0) / 300
            pb["hip_stream_graph"] = {"us_per_step": wp * 1e6, "value": total_envs / wp, "unit": "env-steps/s",
                                      "what": "10 steps of obs -> MlpPolicy (torch GEMMs) -> qs_step captured into one hipGraph, replayed 30 x"}
        else:
            pb["hip_stream_graph"] = {"error": gr_err or "capture failed on another rank"}
        del gr
        # the same loop with the actor as ONE hand-written kernel (qs_policy_forward, MlpPolicy.predict_hip) and qs_step as a call of
        # its own: two launches per step, the full VecEnv return (infos, terminal observations)
        env.set_queue_mode(False)
        for prec in ("f32", "bf16x3"):
            obs = env.reset()
            for _ in range(30):
                obs, _, _, _ = env.step(pol.predict_hip(env, obs, precision=prec))
            barrier()
            t0 = time.perf_counter()
            for _ in range(300):
                obs, _, _, _ = env.step(pol.predict_hip(env, obs, precision=prec))
            torch.cuda.synchronize()
            wp = max_over_ranks(time.perf_counter() - t0) / 300
            pb["hip_stream_mfma_policy_" + prec] = {"us_per_step": wp * 1e6, "value": total_envs / wp, "unit": "env-steps/s"}
        # the same loop with the shipped actor INSIDE the launch: VecDockingEnv.step_policy = qs_policy_rollout(T = 1), one launch
        # per step on the HIP stream, outputs consumable per step
        env.set_queue_mode(False)
        for prec in ("f32", "bf16x3"):
            env.reset()
            for _ in range(30):
                env.step_policy(pol, precision=prec)
            barrier()
            t0 = time.perf_counter()
            for _ in range(300):
                env.step_policy(pol, precision=prec)
            torch.cuda.synchronize()
            wp = max_over_ranks(time.perf_counter() - t0) / 300
            pb["one_launch_per_step_" + prec] = {"us_per_step": wp * 1e6, "value": total_envs / wp, "unit": "env-steps/s"}
        pb["one_launch_per_step_what"] = ("VecDockingEnv.step_policy(policy): the actor on the matrix cores (exact-f32 MFMA / split-bf16 "
                                          "operands) and the env step in ONE launch per step, outputs consumable per step")
        pb["what"] = ("VecDockingEnv.step(MlpPolicy.predict(obs)) per step, 300 steps; the policy is three torch GEMMs and dominates "
                      "both; per-step consumable outputs cost a release per step in either path, so the private queue buys nothing "
                      "here (DESIGN.md section 4a): use the HIP-stream mode for per-step loops, the fused qs_policy_rollout / "
                      "qs_runner_rollout kernels for throughput")
        out["policy_between_steps"] = pb
        leave_private(env)
    # fused roll-out leg: T steps per launch, state in registers (different algorithmic bytes: see DESIGN.md)
    T = args.rollout_T
    acts = pool[:T] if P >= T else env.random_actions(T)
    reps = max(1, min(20, steps_timed // T))
    env.rollout(acts)
    barrier()
    env.timer_start()
    t0 = time.perf_counter()
    for _ in range(reps):
        o_, r_, d_, f_ = env.rollout(acts, want_flags=False)
    env.timer_stop()
    torch.cuda.synchronize()
    w2 = max_over_ranks(time.perf_counter() - t0)
    b_roll = 16 + 48 + 4 + 1 + 320.0 / T
    out["rollout_fused"] = {"value": total_envs * T * reps / w2, "unit": "env-steps/s", "T": T, "launches": reps,
                            "bytes_per_env_step": b_roll,
                            "hbm_frac": b_roll * n * T * reps / w2 / 1e9 / HBM_PEAK_GBS,
                            "note": "qs_rollout: identical results to T qs_step calls; VALU-bound, not HBM-bound"}
    del o_, r_, d_, f_
    # rk4 integrator (the physically intended mode; same kernel, 4 df evaluations per drone)
    other = "rk4" if args.integrator == "frozen" else "frozen"
    env_o = make_env(other)
    env_o.reset()
    Ko = max(100, steps_timed // 4)
    w3, ms3 = time_steps(env_o, Ko, 1, min(W, 50), pool)
    out["other_integrator"] = {"integrator": other, "value": total_envs * Ko / w3, "unit": "env-steps/s",
                               "step_period_us": w3 * 1e6 / Ko}
    env_o.close()
    # ---- the step API at 131 072 envs per GPU, on the driver's clock: docking-v0 (config 3's env) and the config-5 share
    #      (docking-v2, per-env mass / inertia, 408 B): where the blueprint's 0.40 read-roofline target is (not) met
    if n != 131072:
        nb = 131072
        legs = {}
        for key, env_id, rnd, b_, rb_ in (("docking-v0", "docking-v0", 1, 392, 176), ("config5_share_docking-v2_mass_inertia", "docking-v2", 2, 408, 192)):
            mk = lambda: make_env(args.integrator, nb, rank * nb, env_id, rnd)      # noqa: E731
            e2 = mk()
            e2.reset()
            pool2 = e2.random_actions(min(128, P), step0=0)
            qm, qq, note = _pick(args, e2, mk, pool2, time_steps, verify_private_queue, max_over_ranks, groups)
            try:
                w5 = sorted(time_steps(e2, K, R, min(W, 50), pool2)[0] for _ in range(3))[1]
                bad = 0.0
            except qa.QuadsimError:
                bad = 1.0
            if max_over_ranks(bad) > 0.5:                   # placement guard fired on some rank: time the HIP-stream chain
                note = (note or "") + "; private queues abandoned during timing (placement guard): timed on the HIP stream"
                qm, qq = "hip", 0
                leave_private(e2)
                e2.reset()
                w5 = sorted(time_steps(e2, K, R, min(W, 50), pool2)[0] for _ in range(3))[1]
            us = w5 * 1e6 / steps_timed
            legs[key] = {"envs_per_gpu": nb, "value": nb * world / (us * 1e-6), "unit": "env-steps/s", "step_period_us": us,
                         "bytes_per_env_step": b_, "frac": b_ * nb / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                         "read_frac": rb_ * nb / (us * 1e-6) / 1e9 / HBM_PEAK_GBS,
                         "read_frac_target_met": bool(rb_ * nb / (us * 1e-6) / 1e9 / HBM_PEAK_GBS >= READ_TARGET),
                         "queue_mode": qm, "private_queues": qq, "queue_note": note, "action_pool_batches": int(pool2.shape[0])}
            e2.close()
            del pool2
        out["step_api_131072_envs"] = legs
    # the same step kernel where it is not latency-bound: 1 048 576 envs per GPU (168 MB of state, 16 waves per
    # SIMD): shows the kernel's bandwidth ceiling beside the headline
    if n < (1 << 20):
        nb = 1 << 20
        env_b = make_env(args.integrator, nb, rank * nb)
        env_b.reset()
        pool_b = env_b.random_actions(8, step0=0)
        wb, msb = time_steps(env_b, 200, 1, 20, pool_b)
        out["step_api_1M_envs"] = {"envs_per_gpu": nb, "value": nb * world * 200 / wb, "unit": "env-steps/s",
                                   "step_period_us": wb * 1e6 / 200,
                                   "hbm_frac": bpe * nb / (wb / 200) / 1e9 / HBM_PEAK_GBS}
        env_b.close()
        del pool_b
    # what the HBM of THIS box delivers ("report both spec and measured"): device copy and triad over arrays far
    # beyond the 256 MB Infinity Cache, plain torch ops, HIP events; bytes counted as read + written
    try:
        nel = 1 << 28                                                 # 1 GiB of float32 per array
        xa = torch.empty(nel, dtype=torch.float32, device="cuda:%d" % local_rank).normal_()
        xb = torch.empty_like(xa).normal_()
        xc = torch.empty_like(xa)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        res = {}
        for name, fn, nbytes in (("copy", lambda: xc.copy_(xa), 2 * 4 * nel), ("triad", lambda: torch.add(xa, xb, alpha=1.5, out=xc), 3 * 4 * nel)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[name + "_GBs"] = nbytes * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9
        del xa, xb, xc
        best = max(res.values())
        out["hbm_measured"] = dict(res, array_bytes=4 * nel, spec_peak_GBs=HBM_PEAK_GBS, measured_over_spec=best / HBM_PEAK_GBS,
                                   what="torch device copy / triad over 1 GiB float32 arrays (beyond the Infinity Cache), read + written "
                                        "bytes per HIP-event time: what this box's HBM delivers to a streaming kernel")
        if "step_api_1M_envs" in out:
            out["step_api_1M_envs"]["frac_of_measured_hbm"] = out["step_api_1M_envs"]["hbm_frac"] * HBM_PEAK_GBS / best
    except Exception as ex:                                           # a micro-benchmark must never cost the line
        out["hbm_measured"] = {"error": str(ex)}
    # policy in the loop, fused: a = clip(MLP(obs)); env.step(a), T steps per launch, the shipped PPO2
    # actor (weights fixture) on the matrix cores.  Needs nominal / rocRAND-initialised resets and no per-env params.
    if args.randomise <= 1 and os.path.exists(wpath):
        from quadsim_amd import MlpPolicy, fused_policy_rollout
        pol = MlpPolicy.from_npz(wpath, device="cuda:%d" % local_rank)
        Tp = 32
        flop = 2 * (12 * 128 + 128 * 128 + 128 * 4)
        for prec, key in (("f32", "policy_rollout_f32_mfma"), ("bf16x3", "policy_rollout_bf16x3_mfma")):
            fused_policy_rollout(env, pol, Tp, want_actions=False, precision=prec)
            barrier()
            t0 = time.perf_counter()
            for _ in range(4):
                fused_policy_rollout(env, pol, Tp, want_actions=False, precision=prec)
            torch.cuda.synchronize()
            w5 = max_over_ranks(time.perf_counter() - t0)
            out[key] = {"value": total_envs * Tp * 4 / w5, "unit": "env-steps/s", "T": Tp,
                        "mlp_tflops": total_envs * Tp * 4 * flop / w5 / 1e12}
        out["policy_rollout_f32_mfma"]["roofline"] = {
            "bound": "mfma", "peak": 157.3 * world, "unit": "TFLOP/s",
            "achieved": out["policy_rollout_f32_mfma"]["mlp_tflops"],
            "frac": out["policy_rollout_f32_mfma"]["mlp_tflops"] / (157.3 * world),
            "note": "exact-f32 MFMA (v_mfma_f32_16x16x4_f32); 36 864 MLP flop per env-step"}
        out["policy_rollout_bf16x3_mfma"]["note"] = "split-bf16 operands, 3 MFMAs per product, ~1e-5 action error (opt-in)"
    if os.path.exists(wpath):
        # PPO2 data collection (Runner._run, rl_baselines/ppo2/ppo2.py:472-527): actor + critic + Gaussian sampling +
        # neglogp + env.step for n_steps in one launch, then GAE + flatten + episode accounting
        from quadsim_amd import ActorCriticPolicy, Runner
        Tp = 32
        ac = ActorCriticPolicy.from_npz(wpath, device="cuda:%d" % local_rank)
        flop_ac = 2 * (12 * 128 + 2 * 128 * 128 + 128 * 4 + 128)
        for prec, key in (("f32", "ppo2_runner_f32_mfma"), ("bf16x3", "ppo2_runner_bf16x3_mfma")):
            runner = Runner(env=env, model=ac, n_steps=Tp, gamma=0.99, lam=0.95, collect_ep_infos=False, precision=prec)
            runner.run()
            barrier()
            t0 = time.perf_counter()
            for _ in range(4):
                runner.run()
            torch.cuda.synchronize()
            w6 = max_over_ranks(time.perf_counter() - t0)
            out[key] = {"value": total_envs * Tp * 4 / w6, "unit": "env-steps/s", "T": Tp,
                        "mlp_tflops": total_envs * (Tp + 1) * 4 * flop_ac / w6 / 1e12}
        out["ppo2_runner_f32_mfma"]["what"] = (
            "Runner.run(): qs_runner_rollout (policy + value nets on exact-f32 MFMA, rocRAND Gaussian sampling, "
            "neglogp, fused env.step) + qs_gae_flatten + qs_episode_stats + swap_and_flatten of obs / actions")
        out["ppo2_runner_bf16x3_mfma"]["note"] = "the same with split-bf16 operands (qs_runner_rollout_fast), ~1e-5 error on means / values (opt-in)"
    if X["distributed"] and args.backend == "nccl":
        # BASELINE configs 4/5: RCCL all-gather of the roll-out slabs (obs, reward, done) once per T-step roll-out
        from quadsim_amd.distributed import gather_slab
        slab = env.rollout_slab(acts)
        gathered = gather_slab(slab)
        barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            env.rollout_slab(acts, out=slab)
            gather_slab(slab, out=gathered)
        torch.cuda.synchronize()
        w4 = max_over_ranks(time.perf_counter() - t0)
        out["allgather"] = {"value": total_envs * T * reps / w4, "unit": "env-steps/s", "world_size": dist.get_world_size(),
                            "backend": dist.get_backend(),
                            "what": "qs_rollout_slab(T=%d) + ONE RCCL all_gather of the packed (obs, reward, done) slab "
                                    "(%.1f MB per rank per roll-out)" % (T, T * n * 56 / 1e6)}
        # the same with roll-out k+1 overlapped with the gather of roll-out k (double-buffered slabs)
        from quadsim_amd.distributed import SlabGatherPipeline
        del gathered
        pipe = SlabGatherPipeline(lambda buf: env.rollout_slab(acts, out=buf), slab.shape, dtype=slab.dtype, device=slab.device, depth=2)
        for _ in range(3):
            pipe.step()
        pipe.flush()
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            pipe.step()
        pipe.flush()
        torch.cuda.synchronize()
        w5 = max_over_ranks(time.perf_counter() - t0)
        out["allgather"]["overlapped"] = {"value": total_envs * T * reps / w5, "unit": "env-steps/s",
                                          "what": "SlabGatherPipeline(depth=2): the all-gather of roll-out k runs on RCCL's stream "
                                                  "while roll-out k+1 is computed"}
        del pipe


def _pick(args, env, mk, pool, time_steps, verify_private_queue, max_over_ranks, groups):
    """launch path for a side leg: as the headline's pick_launch_path (verified bit-identical per candidate, fastest on a probe)"""
    if args.queue_mode == "hip" or groups > 1:
        return "hip", 0, None
    cand = [int(args.queues)] if args.queue_mode == "private" else [1, 2, 3]
    best_t = time_steps(env, 300, 1, 50, pool)[0] if args.queue_mode == "auto" else float("inf")
    notes, queues = ["HIP stream: %.2f us per step on the probe" % (best_t / 300 * 1e6)] if args.queue_mode == "auto" else [], 0
    for q in cand:
        ok, why = verify_private_queue(mk, pool, q)
        if -max_over_ranks(-float(ok)) < 0.5:
            notes.append("%d private queue(s) not used: %s" % (q, why if not ok else "another rank could not verify it"))
            continue
        env.set_queue_mode(True, q, ordering="host")
        try:
            t = time_steps(env, 300, 1, 50, pool)[0]
        except Exception as ex:                              # noqa: BLE001  (the placement guard: QuadsimError)
            notes.append("%d private queue(s) not used: %s" % (q, ex))
            env.reset()
            continue
        notes.append("%d private queue(s): %.2f us per step on the probe" % (q, t / 300 * 1e6))
        if t < best_t:
            best_t, queues = t, q
    if queues:
        env.set_queue_mode(True, queues, ordering="host")
    else:
        env.set_queue_mode(False)
    return ("private" if queues else "hip"), queues, "; ".join(notes)


if __name__ == "__main__":
    main()
