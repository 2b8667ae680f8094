"""One row per kernel of libquadsim_sac.so's code object (csrc/sac_kernels.hpp): the update k_sac_step (four workgroups: q1, q2, value,
actor), the copy into and out of the workspace, k_sac_copy, and the element-wise device functions of the log-probability,
k_sac_math.  None is a template.  The library takes its device functions from train_pieces.hpp and quadsim_device.hpp, which define
no kernel of it.

Imported by tests/test_sac_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_sac_step", "k_sac_copy", "k_sac_math")

_F = "tests/test_gpu_sac.py::"


def _row(kernel, args, block, test):
    return dict(id=kernel + "".join("-%d" % a for a in args), kernel=kernel, key=(kernel,) + tuple(args), block=block, test=test)


ROWS = [
    _row("k_sac_step", (), 512, _F + "test_one_step_against_float64[17]"),
    _row("k_sac_copy", (), 256, _F + "test_split_ragged_and_stream_invariance"),
    _row("k_sac_math", (), 256, _F + "test_device_math_sweep"),
]
