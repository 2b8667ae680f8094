"""One row per (kernel, runtime branch) of the layer-0 / layer-1 batch kernels of csrc/layer1_kernels.hpp: k_drone_step
(integrator x per-row parameters x limited pointer: 8), k_ctrl (mode 0 without and with a state_last it must ignore, mode 1: 3),
k_transform (op 0..3: 4) and k_rel_obs (1): 16.  The kernels are plain kernels of the anonymous namespace, so a variant is a
branch taken at run time, not an instantiation; the key names the branch.

Imported by tests/test_layer1_cpu.py, which checks that the kernels are exactly the __global__ functions of the header and are in
the built code object, and by tests/test_gpu_layer1.py, which runs every row at every env count of layer1_ref.N_ENVS.  Plain
Python: no torch here.

A row holds the C ABI entry point that launches the kernel and the id of one GPU test case that holds it to its float64
reference on every element between sentinel bytes.
"""
KERNELS = ("k_drone_step", "k_ctrl", "k_transform", "k_rel_obs")

_F = "tests/test_gpu_layer1.py::"

INTEG = ("frozen", "rk4")
PAR = ("par_null", "par_given")
LIMITED = ("limited_null", "limited_given")
CTRL = ("mode0_last_null", "mode0_last_given", "mode1")
OPS = ("quat2euler", "euler2quat", "quat2rot", "rot2euler")


def _row(key, entry, test):
    return dict(id="-".join(str(x) for x in key), kernel=key[0], key=key, entry=entry, test=_F + test)


ROWS = (
    [_row(("k_drone_step", i, p, l), "qs_drone_step", "test_drone_step[%s-%s-%s-257]" % (i, p, l))
     for i in INTEG for p in PAR for l in LIMITED]
    + [_row(("k_ctrl", c), "qs_ctrl", "test_ctrl[%s-257]" % c) for c in CTRL]
    + [_row(("k_transform", op), "qs_transform", "test_transform[%s-257]" % name) for op, name in enumerate(OPS)]
    + [_row(("k_rel_obs",), "qs_rel_obs", "test_rel_obs[257]")]
)
