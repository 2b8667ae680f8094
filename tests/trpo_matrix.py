"""One row per kernel of libquadsim_trpo.so's code object (csrc/trpo_kernels.hpp): the nine kernels of a policy step and the value
fit.  None is a template.  The library takes its device functions from train_pieces.hpp, which defines
no kernel.

Imported by tests/test_trpo_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_trpo_prep", "k_trpo_grad", "k_trpo_reduce", "k_trpo_cg_init", "k_trpo_fvp", "k_trpo_cg_iter", "k_trpo_step", "k_trpo_ls_eval",
           "k_trpo_ls_decide", "k_trpo_vf_fit")

_F = "tests/test_gpu_trpo.py::"


def _row(kernel, block, test):
    return dict(id=kernel, kernel=kernel, key=(kernel,), block=block, test=test)


ROWS = [
    _row("k_trpo_prep", 256, _F + "test_gradient_and_statistics_against_float64[300-7]"),
    _row("k_trpo_grad", 512, _F + "test_gradient_and_statistics_against_float64[17-7]"),
    _row("k_trpo_reduce", 256, _F + "test_one_fisher_vector_product_against_float64[301-5]"),
    _row("k_trpo_cg_init", 256, _F + "test_zero_gradient_skips_the_update"),
    _row("k_trpo_fvp", 512, _F + "test_one_fisher_vector_product_against_float64[17-5]"),
    _row("k_trpo_cg_iter", 256, _F + "test_conjugate_gradient_and_step_replay_bit_for_bit"),
    _row("k_trpo_step", 256, _F + "test_residual_tol_stops_the_solver_and_leaves_the_trace_rows"),
    _row("k_trpo_ls_eval", 512, _F + "test_line_search[small]"),
    _row("k_trpo_ls_decide", 512 // 2, _F + "test_line_search[none]"),
    _row("k_trpo_vf_fit", 512, _F + "test_value_fit_one_step_against_float64[17]"),
]
