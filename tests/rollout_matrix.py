"""One row per instantiation of the roll-out kernels with a network in the loop: k_runner_rollout / k_runner_split
<INTEG, RMODE, PARAMS, FAST, NET> (PPO2 data collection) and k_policy_rollout / k_policy_rollout_fast <INTEG, RMODE> (the
deterministic actor; VecDockingEnv.step_policy is one of them with T = 1).

Imported by tests/test_rollout_matrix_cpu.py, which checks that the rows are exactly the instantiations in the built code object,
and by tests/test_gpu_rollout_matrix.py, which runs every row.  Plain Python: no torch here.

A row holds the handle configuration that reaches its instantiation through the production dispatch (env id, integrator, dt,
randomise, set_params, env count; for the Runner also precision, network layout, kernel flavour and the source of the noise) and
the variant qs_debug_rollout_variant must report for it: (kernel index, INTEG, RMODE, PARAMS, FAST, NET), -1 where the kernel has
no such template parameter.  Env ids and dt alternate across the rows as in step_matrix._step_row, on an index that advances by
five per group of four (FAST, NET) rows, so that neither is tied to the precision or the network layout.
"""
from step_matrix import INTEGS

RUNNER_KERNELS = ("k_runner_rollout", "k_runner_split")            # qs_debug_rollout_variant's kernel 0, 1
POLICY_KERNELS = ("k_policy_rollout", "k_policy_rollout_fast")     # ... 2, 3
KERNELS = RUNNER_KERNELS + POLICY_KERNELS
# the (PARAMS, RMODE) pairs runner_dispatch launches: step_matrix.PAIRS without the stored initial states (RMODE 3)
RUNNER_PAIRS = ((0, 0), (1, 0), (0, 1), (1, 1), (1, 2))
NETS = ("shared", "towers")                                        # kNetShared = 0, kNetTowers = 1
PRECISIONS = ("f32", "bf16x3")                                     # FAST = 0, 1

T = 12
FULL_N = 64 * 3 + 29             # full tiles, a ragged tile, and a k_runner_split workgroup (four tiles) that is partly absent
RUNNER_TEST = "tests/test_gpu_rollout_matrix.py::test_runner_row[%s]"
POLICY_TEST = "tests/test_gpu_rollout_matrix.py::test_policy_rollout_row[%s]"
# rows (by index) below one tile, the single-env row among them, and the T = 1 rows
RUNNER_SMALL_N = {7: 1, 22: 37, 45: 63, 68: 5}
RUNNER_T1 = (13, 58)
POLICY_SMALL_N = {2: 1, 5: 41}


def _common(i, kernel, key, integ, rmode, params, n, t):
    rid = "-".join(str(x) for x in key)
    j = i + i // 4
    return dict(
        id=rid, kernel=kernel, key=key, env_id=("docking-v0", "docking-v2")[j % 2], integ=INTEGS[integ],
        dt=(0.02, 0.01)[(j // 2) % 2], randomise=rmode,
        set_params=bool(params) and rmode != 2 or (rmode == 2 and j % 2 == 0),
        n=n, T=t, combo=(integ, params, rmode))


def _runner_rows():
    rows = []
    i = 0
    for serial, kernel in ((1, "k_runner_rollout"), (0, "k_runner_split")):
        for integ in (0, 1):
            for p, (params, rmode) in enumerate(RUNNER_PAIRS):
                for fast in (0, 1):
                    for net in (0, 1):
                        key = (kernel, integ, rmode, params, fast, net)      # template arguments in declaration order
                        n = RUNNER_SMALL_N.get(i, FULL_N + 64 * (i % 3))
                        row = _common(i, kernel, key, integ, rmode, params, n, 1 if i in RUNNER_T1 else T)
                        row.update(precision=PRECISIONS[fast], net=NETS[net], serial=serial,
                                   noise=("caller", "kernel")[(integ + p + fast + net) % 2],
                                   variant=(RUNNER_KERNELS.index(kernel), integ, rmode, params, fast, net),
                                   test=RUNNER_TEST % row["id"])
                        rows.append(row)
                        i += 1
    return rows


def _policy_rows():
    rows = []
    i = 0
    for kernel in POLICY_KERNELS:
        for integ in (0, 1):
            for rmode in (0, 1):
                key = (kernel, integ, rmode)
                row = _common(i, kernel, key, integ, rmode, 0, POLICY_SMALL_N.get(i, FULL_N + 64 * (i % 3)), T)
                row.update(precision=PRECISIONS[POLICY_KERNELS.index(kernel)],
                           variant=(2 + POLICY_KERNELS.index(kernel), integ, rmode, -1, -1, -1),
                           test=POLICY_TEST % row["id"])
                rows.append(row)
                i += 1
    return rows


RUNNER_ROWS = _runner_rows()
POLICY_ROWS = _policy_rows()
ROWS = RUNNER_ROWS + POLICY_ROWS
