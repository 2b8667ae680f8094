"""One row per compiled instantiation of the seven planner kernels on the exact simulator (csrc/shooting.hpp, shooting_split.hpp,
mppi.hpp, mppi_split.hpp): k_shooting_plan, k_wide_candidates, k_mppi and k_pathint_part_roll for INTEG x PARAMS (4 each), and
the plain k_wide_finish, k_pathint_part_sums and k_pathint_part_finish: 16 + 3 = 19.

Imported by tests/test_plan_edges_cpu.py, which checks that the rows are exactly the instantiations in the built code object
and that every `test` is collected, and by the census of tests/lifecycle_matrix.py.  Plain Python: no torch here.

A row holds the C ABI entry point that launches the kernel, the handle configuration (env id, integrator, per-env parameters)
that reaches the instantiation, and the id of one GPU case of tests/test_gpu_plan_edges.py that holds its VALUES: every
candidate's score bit for bit against the step API on a twin handle, with the candidates' keys at a step counter of 2^32 or above
(the largest the handle's cases have) and global ids on both sides of 2^32 or at the top of the 48-bit id space.  The resources of the kernels stay with
the *_instantiations_and_resources tests of the four test_*_cpu.py files.
"""
from plan_cases import EDGE_COMBOS, MPPI_K, SHOOT_K, key_cases

TEMPLATED = ("k_shooting_plan", "k_wide_candidates", "k_mppi", "k_pathint_part_roll")     # <int INTEG, bool PARAMS>
PLAIN = ("k_wide_finish", "k_pathint_part_sums", "k_pathint_part_finish")
KERNELS = TEMPLATED + PLAIN

_F = "tests/test_gpu_plan_edges.py::"
_ENTRY = {"k_shooting_plan": "qs_shooting_plan", "k_wide_candidates": "qs_shooting_plan_split", "k_wide_finish": "qs_shooting_plan_split",
          "k_mppi": "qs_mppi_plan", "k_pathint_part_roll": "qs_mppi_plan_split", "k_pathint_part_sums": "qs_mppi_plan_split",
          "k_pathint_part_finish": "qs_mppi_plan_split"}


def _case(ks, combo):
    """the key case of `combo` with the largest step counter -> its id"""
    return max((c for c in key_cases(ks) if c[1:4] == combo), key=lambda c: c[5])[0]


def _row(kernel, combo):
    env_id, integ, params = combo
    shooting = kernel in ("k_shooting_plan", "k_wide_candidates", "k_wide_finish")
    test = "%stest_%s_keys[%s]" % (_F, "shooting" if shooting else "mppi", _case(SHOOT_K if shooting else MPPI_K, combo))
    key = (kernel, int(integ == "rk4"), int(params)) if kernel in TEMPLATED else (kernel,)
    return dict(id="-".join(str(x) for x in key), kernel=kernel, key=key, entry=_ENTRY[kernel], env_id=env_id, integ=integ,
                params=params, test=test)


ROWS = [_row(k, combo) for k in TEMPLATED for combo in EDGE_COMBOS] + [_row(k, EDGE_COMBOS[1]) for k in PLAIN]
