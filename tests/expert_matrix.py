"""One row per instantiation of the PID-expert kernels of csrc/expert_rollout.hpp: k_expert_action<PARAMS>, k_expert_rollout
<INTEG, PARAMS, RMODE> and k_expert_evaluate<INTEG, PARAMS, RMODE>, 2 + 14 + 14 = 30.

Imported by tests/test_expert_matrix_cpu.py, which checks that the rows are exactly the instantiations in the built code object,
and by tests/test_gpu_expert_matrix.py, which runs every row.  Plain Python: no torch here.

A row holds the handle configuration that reaches its instantiation through the production dispatch (env id, integrator,
randomise, set_params / set_init_state, a ragged env count), the expert's gains (kp, kd), the layout of the roll-out's obs /
actions rows and the (INTEG, PARAMS, RMODE) qs_debug_step_variant must report for it (qs_expert_rollout and qs_expert_evaluate
dispatch on the same step_combo; k_expert_action takes PARAMS alone).  RMODE 3 (stored initial states) is docking-v1's
construction-time starts on the rows without per-env parameters and set_init_state on the others.  The two non-default gain
pairs and the env-major layout are spread over the rows by the row index, so that neither is tied to a template argument.
"""
from expert_ref import GAINS
from step_matrix import INTEGS, PAIRS

KERNELS = ("k_expert_rollout", "k_expert_evaluate", "k_expert_action")
LAYOUTS = ("time_major", "env_major")

T = 12                           # steps of a roll-out row
K = 2                            # episodes of an evaluation row
ACTION_N = (1, 63, 65, 257)      # below a tile, a ragged second tile, and one env past a 256-thread block
ROLLOUT_N = (257, 203, 41, 300, 131, 65, 259)
EVAL_N = (130, 67, 101, 41, 129, 33, 93)

ACTION_TEST = "tests/test_gpu_expert_matrix.py::test_action_row[%s]"
ROLLOUT_TEST = "tests/test_gpu_expert_matrix.py::test_rollout_row[%s]"
EVAL_TEST = "tests/test_gpu_expert_matrix.py::test_evaluate_row[%s]"


def _fused_row(i, kernel, integ, params, rmode, n, test):
    key = (kernel, integ, params, rmode)
    rid = "-".join(str(x) for x in key)
    if rmode == 3:
        env_id = "docking-v1" if not params else ("docking-v0", "docking-v2")[integ]
    else:
        env_id = ("docking-v0", "docking-v2")[i % 2]
    return dict(
        id=rid, kernel=kernel, key=key, env_id=env_id, integ=INTEGS[integ], randomise=rmode if rmode in (1, 2) else 0,
        set_params=bool(params) and rmode != 2 or (rmode == 2 and i % 2 == 0),
        set_init=rmode == 3 and env_id != "docking-v1",
        n=n, gains=GAINS[i % 3], layout=LAYOUTS[(i // 2 + i // 7) % 2] if kernel == "k_expert_rollout" else LAYOUTS[0],
        combo=(integ, params, rmode), test=test % rid)


def _fused_rows(kernel, sizes, test, shift):
    rows = []
    for integ in (0, 1):
        for params, rmode in PAIRS:
            i = len(rows) + shift
            rows.append(_fused_row(i, kernel, integ, params, rmode, sizes[(len(rows)) % len(sizes)], test))
    return rows


def _action_rows():
    rows = []
    for params in (0, 1):
        key = ("k_expert_action", params)
        rid = "-".join(str(x) for x in key)
        rows.append(dict(id=rid, kernel="k_expert_action", key=key, env_id=("docking-v0", "docking-v2")[params], integ=INTEGS[params],
                         randomise=0, set_params=bool(params), set_init=False, n=ACTION_N, gains=GAINS, layout=LAYOUTS[0],
                         combo=(params, params, 0), test=ACTION_TEST % rid))
    return rows


ACTION_ROWS = _action_rows()
ROLLOUT_ROWS = _fused_rows("k_expert_rollout", ROLLOUT_N, ROLLOUT_TEST, 0)
EVAL_ROWS = _fused_rows("k_expert_evaluate", EVAL_N, EVAL_TEST, 1)
ROWS = ACTION_ROWS + ROLLOUT_ROWS + EVAL_ROWS
