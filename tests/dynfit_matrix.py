"""One row per kernel instantiation of libquadsim_dynfit.so's code object (csrc/dynfit_kernels.hpp): the fit k_dyn_fit<P1, P2> for
each compiled pair of padded widths.  The library includes none of the planners' fragments, so it inherits no kernel.

Imported by tests/test_dynfit_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.
"""
KERNELS = ("k_dyn_fit",)

_F = "tests/test_gpu_dynfit.py::"


def _row(key, widths, test):
    return dict(id="-".join(str(x) for x in key), kernel=key[0], key=key, widths=widths, block=512, test=test)


ROWS = [
    _row(("k_dyn_fit", 64, 64), (64, 64), _F + "test_gradients_loss_and_adam_of_one_step[edge_64_64]"),
    _row(("k_dyn_fit", 128, 128), (128, 128), _F + "test_gradients_loss_and_adam_of_one_step[he_128_128]"),
    _row(("k_dyn_fit", 208, 112), (208, 112), _F + "test_gradients_loss_and_adam_of_one_step[edge_208_112]"),
]
