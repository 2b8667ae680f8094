"""One row per kernel of libquadsim_ppo.so's code object (csrc/ppo2_kernels.hpp): the advantage statistics k_ppo_adv_stats, the
gradient kernel k_ppo_grad, the reduction k_ppo_reduce and the clip-and-Adam kernel k_ppo_apply.  None is a template; the library
takes its device functions from train_pieces.hpp, which defines no kernel.

Imported by tests/test_ppo2_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_ppo_adv_stats", "k_ppo_grad", "k_ppo_reduce", "k_ppo_apply")

_F = "tests/test_gpu_ppo2.py::"


def _row(kernel, block, test):
    return dict(id=kernel, kernel=kernel, key=(kernel,), block=block, test=test)


ROWS = [
    _row("k_ppo_adv_stats", 256, _F + "test_gradients_statistics_clip_and_adam_of_one_step[he-shared]"),
    _row("k_ppo_grad", 512, _F + "test_gradients_statistics_clip_and_adam_of_one_step[he-towers]"),
    _row("k_ppo_reduce", 256, _F + "test_slices_within_the_same_bounds_and_the_same_bits_on_another_stream[300]"),
    _row("k_ppo_apply", 256, _F + "test_five_steps_are_five_calls_bit_for_bit"),
]
