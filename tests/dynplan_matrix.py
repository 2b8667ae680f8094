"""One row per kernel and instantiation of libquadsim_dyn.so's code object (csrc/dynplan_kernels.hpp, dynplan_image.hpp): the
planner k_dyn_plan<T1, T2> for each compiled pair of tile counts, the arg-max k_dyn_finish and the packer k_dyn_pack.

Imported by tests/test_dynplan_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test of tests/test_gpu_dynplan.py that holds each to the float64 restatement.  Plain Python.

A row holds the hidden widths of a net that runs on the instantiation (the widest it takes), and the id of one GPU test case
that checks every element of every output between sentinel bytes.
"""
KERNELS = ("k_dyn_plan", "k_dyn_finish", "k_dyn_pack")

_F = "tests/test_gpu_dynplan.py::"


def _row(key, widths, test):
    return dict(id="-".join(str(x) for x in key), kernel=key[0], key=key, widths=widths, block=256, test=_F + test)


ROWS = [
    _row(("k_dyn_plan", 4, 4), (64, 64), "test_steps_scores_and_winner[he_64_64]"),
    _row(("k_dyn_plan", 8, 8), (128, 128), "test_steps_scores_and_winner[he_128_128]"),
    _row(("k_dyn_plan", 13, 7), (208, 112), "test_edge_widths[edge_208_112]"),
    _row(("k_dyn_finish",), None, "test_draws[3]"),
    _row(("k_dyn_pack",), None, "test_padding_is_invisible"),
]
