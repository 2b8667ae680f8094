"""One row per kernel of libquadsim_bc.so's code object (csrc/bcfit_kernels.hpp): the fit k_bc_fit, the validation pass k_bc_loss
and its one-workgroup sum k_bc_loss_sum.  None is a template; the library takes its device functions from train_pieces.hpp,
which defines no kernel.

Imported by tests/test_bcfit_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_bc_fit", "k_bc_loss", "k_bc_loss_sum")

_F = "tests/test_gpu_bcfit.py::"


def _row(kernel, block, test):
    return dict(id=kernel, kernel=kernel, key=(kernel,), block=block, test=test)


ROWS = [
    _row("k_bc_fit", 512, _F + "test_gradients_loss_and_adam_of_one_step[he]"),
    _row("k_bc_loss", 512, _F + "test_validation_loss[257]"),
    _row("k_bc_loss_sum", 256, _F + "test_validation_loss[257]"),
]
