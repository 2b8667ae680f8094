"""One row per instantiation of the env-step kernels (k_env, k_env_split, k_env_resident, k_hover) and of the evaluation
kernels that share their step (k_policy_evaluate, k_policy_evaluate_fast).

Imported by tests/test_step_matrix_cpu.py, which checks that the rows are exactly the instantiations in the built code
object, and by the GPU tests named in each row's "test".  Plain Python: no torch here.

A step row holds the handle configuration that reaches its instantiation through the production selection (env count,
queue count, integrator, randomise, set_params / set_init_state) and the variant qs_debug_step_variant must report for it:
(family, INTEG, PARAMS, RMODE, PREP), -1 where the family has no such template parameter.  The env counts that pick the
role-split PREP 0 variant of RMODE 1/2 (more than kPrepMaxTiles = 1365 tiles in one launch) and the resident one (one private
queue, the tiles x 2 waves within the MI355X's 256 CUs x 12) are those of production on an MI355X: no row forces a variant.
"""

SERIAL, SPLIT, RESIDENT, CHAIN_SPLIT, CHAIN_SERIAL, HOVER = 0, 1, 2, 3, 4, 5
FAMILY_KERNEL = {SERIAL: "k_env", SPLIT: "k_env_split", RESIDENT: "k_env_resident", HOVER: "k_hover"}

# the (PARAMS, RMODE) pairs launch_integ dispatches: RMODE 0 fixed reset, 1 rocRAND initial state, 2 + per-episode mass /
# inertia (implies per-env params), 3 stored per-env initial state (docking-v1, set_init_state)
PAIRS = ((0, 0), (1, 0), (0, 1), (1, 1), (1, 2), (0, 3), (1, 3))
INTEGS = ("frozen", "rk4")

SERIAL_N = 131072 + 64 * 3 + 29          # above kSplitMaxEnvs: the serial kernel; a ragged last tile
BIG_N = 1400 * 64 - 27                   # 1400 tiles > kPrepMaxTiles: PREP 0 for RMODE 1/2; 2800 resident waves <= 3072
ROCRAND_GID0 = 2 ** 32 - 40              # env_id_offset of the rocRAND rows: gid0 + env crosses 32 bits inside the handle
ROCRAND_K0 = 2 ** 32 - 3                 # step counter of the rocRAND rows: k and k + 1 cross 32 bits inside the window

STEP_TEST = "tests/test_gpu_step_matrix.py::test_step_kernel_row[%s]"
EVAL_TEST = "tests/test_gpu_policy_evaluate.py::%s"


def _step_row(i, family, integ, params, rmode, prep, n, queues=0, env_id=None):
    kernel = FAMILY_KERNEL[family]
    I = INTEGS.index(integ)
    if family == SERIAL:
        key = (kernel, I, params, rmode)
    elif family == HOVER:
        key = (kernel, I, params)
    else:
        key = (kernel, I, params, rmode, prep)
    if env_id is None:
        env_id = "hovering-v0" if family == HOVER else ("docking-v0", "docking-v2")[i % 2]
    # RMODE 3: the docking-v1 construction-time initial states on the resident rows, set_init_state elsewhere
    set_init = rmode == 3 and env_id != "docking-v1"
    if family == HOVER:
        set_init = False                 # hovering-v0 resets to its jittered construction-time state (stored: RMODE 3)
    rid = "-".join(str(x) for x in key)
    return dict(
        id=rid, kernel=kernel, key=key, env_id=env_id, integ=integ, dt=(0.02, 0.01)[(i // 2) % 2],
        randomise=rmode if rmode in (1, 2) else 0,
        set_params=bool(params) and rmode != 2 or (rmode == 2 and i % 2 == 0),
        set_init=set_init, n=n, queues=queues, ordering="host" if queues else None, force_prep=None,
        rocrand=rmode in (1, 2),
        variant=(family, I, params, -1 if family == HOVER else rmode, prep),
        production=True,
        test=STEP_TEST % rid)


def _step_rows():
    rows = []
    i = 0
    for integ in INTEGS:
        for params, rmode in PAIRS:
            # k_env: every (INTEG, PARAMS, RMODE) above kSplitMaxEnvs
            rows.append(_step_row(i, SERIAL, integ, params, rmode, -1, SERIAL_N))
            # k_env_split PREP 0: RMODE 0/3 at any size, RMODE 1/2 above kPrepMaxTiles tiles
            rows.append(_step_row(i + 1, SPLIT, integ, params, rmode, 0, BIG_N if rmode in (1, 2) else 1000 + 64 * i + 37))
            # k_env_resident PREP 0: host-ordered private queues; RMODE 1/2 with one queue above kPrepMaxTiles tiles
            big = rmode in (1, 2)
            rows.append(_step_row(i, RESIDENT, integ, params, rmode, 0, BIG_N if big else 2000 + 64 * i + 13,
                                  queues=1 if big else 1 + i % 3,
                                  env_id="docking-v1" if rmode == 3 and params == 0 else None))
            if rmode in (1, 2):
                # PREP 2 (the reset-preparation wave): up to kPrepMaxTiles tiles per launch / per queue
                rows.append(_step_row(i + 1, SPLIT, integ, params, rmode, 2, 3000 + 64 * i + 5))
                rows.append(_step_row(i, RESIDENT, integ, params, rmode, 2, 4000 + 64 * i + 51, queues=1 + (i + 1) % 3))
            i += 1
        for params in (0, 1):
            rows.append(_step_row(i + params, HOVER, integ, params, 3, -1, 1500 + 64 * params + 19))
    return rows


STEP_ROWS = _step_rows()

# The evaluation kernels: (INTEG, PARAMS, RMODE) as launch_integ picks them, precision "f32" -> k_policy_evaluate,
# "bf16x3" -> k_policy_evaluate_fast.  Five frozen combinations are the cases of test_evaluate_equals_per_step_loop (K = 2); the
# others are test_evaluate_matrix_equals_per_step_loop (K = 1).
EVAL_PRECISION = {"k_policy_evaluate": "f32", "k_policy_evaluate_fast": "bf16x3"}
_EXISTING = {(0, 0, 0): "docking-v0-0-False-%s-shared-1000", (0, 0, 1): "docking-v0-1-False-%s-shared-4096",
             (0, 1, 2): "docking-v0-2-False-%s-shared-1000", (0, 0, 3): "docking-v1-0-False-%s-shared-1000",
             (0, 1, 1): "docking-v0-1-True-%s-shared-4096"}


def _eval_rows():
    rows = []
    for kernel, prec in EVAL_PRECISION.items():
        for j, (I, (params, rmode)) in enumerate((I, pr) for I in (0, 1) for pr in PAIRS):
            key = (kernel, I, params, rmode)
            rid = "-".join(str(x) for x in key)
            row = dict(id=rid, kernel=kernel, key=key, integ=INTEGS[I], precision=prec, combo=(I, params, rmode),
                       env_id="docking-v1" if rmode == 3 else ("docking-v0", "docking-v2")[j % 2],
                       randomise=rmode if rmode in (1, 2) else 0, set_params=bool(params) and rmode != 2,
                       ckpt=("shared", "towers")[j % 2], n=1000 + 64 * (j % 3) + 7, production=True)
            if (I, params, rmode) in _EXISTING:
                row["test"] = EVAL_TEST % ("test_evaluate_equals_per_step_loop[%s]" % (_EXISTING[(I, params, rmode)] % prec))
            else:
                row["test"] = EVAL_TEST % ("test_evaluate_matrix_equals_per_step_loop[%s]" % rid)
            rows.append(row)
    return rows


EVAL_ROWS = _eval_rows()
NEW_EVAL_ROWS = [r for r in EVAL_ROWS if "matrix" in r["test"]]
ROWS = STEP_ROWS + EVAL_ROWS
