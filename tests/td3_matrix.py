"""One row per kernel of libquadsim_td3.so's code object (csrc/td3_kernels.hpp): the update k_td3_step (two workgroups on a
critic-only update, three on an actor update) and the copy into and out of the workspace, k_td3_copy.  Neither is a template.  The
library takes its device functions from train_pieces.hpp and quadsim_device.hpp, which define no kernel of it.

Imported by tests/test_td3_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_td3_step", "k_td3_copy")

_F = "tests/test_gpu_td3.py::"


def _row(kernel, args, block, test):
    return dict(id=kernel + "".join("-%d" % a for a in args), kernel=kernel, key=(kernel,) + tuple(args), block=block, test=test)


ROWS = [
    _row("k_td3_step", (), 512, _F + "test_one_step_against_float64[17]"),
    _row("k_td3_copy", (), 256, _F + "test_delay_split_and_stream_invariance"),
]
