"""One row per kernel instantiation of libquadsim_gail.so's code object (csrc/gail_kernels.hpp): the fit k_gail_fit<W> and the
reward pass k_gail_reward<W> at both compiled widths, and the tests' window on the device math, k_gail_math.  The library takes
its shared device functions from train_pieces.hpp, which defines no kernel.

Imported by tests/test_gail_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_gail_fit", "k_gail_reward", "k_gail_math")

_F = "tests/test_gpu_gail.py::"


def _row(kernel, args, block, test):
    return dict(id=kernel + "".join("-%d" % a for a in args), kernel=kernel, key=(kernel,) + tuple(args), block=block, test=test)


ROWS = [
    _row("k_gail_fit", (64,), 512, _F + "test_gradients_statistics_and_adam_of_one_step[64-17]"),
    _row("k_gail_fit", (128,), 512, _F + "test_gradients_statistics_and_adam_of_one_step[100-17]"),
    _row("k_gail_reward", (64,), 256, _F + "test_reward_and_logits[64-65]"),
    _row("k_gail_reward", (128,), 256, _F + "test_reward_and_logits[100-65]"),
    _row("k_gail_math", (), 256, _F + "test_device_math_sweep[tanh_abs]"),
]
