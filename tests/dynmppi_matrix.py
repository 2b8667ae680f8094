"""One row per kernel and instantiation of libquadsim_dynmppi.so's code object (csrc/dynmppi_kernels.hpp and, included unchanged
for the model step, csrc/dynplan_kernels.hpp and dynplan_image.hpp): the roll-out k_dynm_roll<T1, T2> for each compiled pair of
tile counts, the update k_dynm_update, and the two non-template kernels that come in with dynplan_kernels.hpp.

Imported by tests/test_dynmppi_cpu.py, which checks that the rows are exactly the kernels of the built code object and their
resources, and names the GPU test that holds each.  Plain Python.

The two inherited kernels are never launched by this library ("inherited": True): the same source, compiled with the same
flags, is launched by libquadsim_dyn.so, where tests/dynplan_matrix.py pins it; their rows name those tests.
"""
KERNELS = ("k_dynm_roll", "k_dynm_update", "k_dyn_finish", "k_dyn_pack")
INHERITED_NOTE = "inherited, pinned by tests/dynplan_matrix.py"

_F = "tests/test_gpu_dynmppi.py::"
_D = "tests/test_gpu_dynplan.py::"


def _row(key, widths, test, inherited=False, block=256):
    return dict(id="-".join(str(x) for x in key), kernel=key[0], key=key, widths=widths, block=block, test=test, inherited=inherited,
                note=INHERITED_NOTE if inherited else "")


ROWS = [
    _row(("k_dynm_roll", 4, 4), (64, 64), _F + "test_steps_scores_and_update[edge_64_64]"),
    _row(("k_dynm_roll", 8, 8), (128, 128), _F + "test_steps_scores_and_update[he_128_128]"),
    _row(("k_dynm_roll", 13, 7), (208, 112), _F + "test_steps_scores_and_update[edge_208_112]"),
    _row(("k_dynm_update",), None, _F + "test_shapes_keyed_draws_every_iteration[257-5-3]", block=1024),
    _row(("k_dyn_finish",), None, _D + "test_draws[3]", inherited=True),
    _row(("k_dyn_pack",), None, _D + "test_padding_is_invisible", inherited=True),
]
