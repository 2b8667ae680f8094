"""One row per kernel of libquadsim_ddpg.so's code object (csrc/ddpg_kernels.hpp): the train step k_ddpg_step (two workgroups:
the critic branch and the actor branch) and the copy into and out of the workspace, k_ddpg_copy.  Neither is a template.  The library
takes its device functions from train_pieces.hpp, which defines no kernel.

Imported by tests/test_ddpg_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_ddpg_step", "k_ddpg_copy")

_F = "tests/test_gpu_ddpg.py::"


def _row(kernel, args, block, test):
    return dict(id=kernel + "".join("-%d" % a for a in args), kernel=kernel, key=(kernel,) + tuple(args), block=block, test=test)


ROWS = [
    _row("k_ddpg_step", (), 512, _F + "test_one_step_against_float64[17]"),
    _row("k_ddpg_copy", (), 256, _F + "test_split_and_stream_invariance"),
]
