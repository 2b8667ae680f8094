"""One row per compiled instantiation of the roll-out post-processing kernels of csrc/rollout_ops.hpp: key = (kernel, template
arguments...) as kernel_notes.instantiations_with_types reads them from the code object, entry = the C ABI call that launches
it, test = the case of tests/test_gpu_postproc.py that holds it to the float64 reference of tests/postproc_ref.py with guard
bands around every buffer.  tests/test_postproc_cpu.py fails when an instantiation has no row or a row no test."""

KERNELS = ("k_gae_reduce", "k_gae_apply", "k_gae_serial", "k_gae_flatten", "k_swap_flatten", "k_swap_flatten_v4", "k_episode_stats")

_F = "tests/test_gpu_postproc.py::"

ROWS = [
    # the two-pass scan: three chunks, a done before, on and behind a seam
    dict(key=("k_gae_reduce",), entry="qs_gae", test=_F + "test_gae_two_pass[129-257]"),
    dict(key=("k_gae_apply",), entry="qs_gae", test=_F + "test_gae_two_pass[129-257]"),
    # the serial chain: two groups of 16 and a tail, a ragged last block
    dict(key=("k_gae_serial",), entry="qs_gae", test=_F + "test_gae_serial[47-16385]"),
    # a vector group, a scalar tail, a second block whose later waves idle
    dict(key=("k_gae_flatten",), entry="qs_gae_flatten", test=_F + "test_gae_flatten[20-257]"),
    dict(key=("k_swap_flatten", 1, "float"), entry="qs_swap_and_flatten", test=_F + "test_swap_and_flatten[1-65-97]"),
    dict(key=("k_swap_flatten", 13, "float"), entry="qs_swap_and_flatten", test=_F + "test_swap_and_flatten[13-65-97]"),
    dict(key=("k_swap_flatten", 1, "uint8_t"), entry="qs_swap_and_flatten_u8", test=_F + "test_swap_and_flatten_u8[65-97]"),
    dict(key=("k_swap_flatten_v4", 1), entry="qs_swap_and_flatten", test=_F + "test_swap_and_flatten[4-65-97]"),
    dict(key=("k_swap_flatten_v4", 3), entry="qs_swap_and_flatten", test=_F + "test_swap_and_flatten[12-65-97]"),
    dict(key=("k_episode_stats",), entry="qs_episode_stats", test=_F + "test_episode_stats[33-257]"),
]
