"""-m "not gpu": everything of the learned-dynamics planner that needs no device.  include/quadsim_dyn.h is plain C99 and every
symbol it declares is exported by libquadsim_dyn.so; every refusal the header promises happens before anything is launched
(no device is present here, so a launch could not succeed); tests/dynplan_matrix.py has exactly one row per kernel and
instantiation of the new library's code object, no kernel uses scratch or spills and each fits the compute unit's LDS; the
float32 k-ordered emulation of the contract stays inside the derived bound of tests/dynplan_ref.py on every weight set of the GPU
tests, and DynamicsNet.predict in float64 is the float64 restatement; the width-edge fixtures of tests/dynplan_ref.py route
to the instantiation their table names and can detect a dropped last unit of either hidden layer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dynplan_matrix
import dynplan_ref as dr
import side_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from quadsim_amd import _lib, dynplan
    _lib.build_library()
    return dynplan.load()


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return side_cases.code_object_notes("dyn", tmp_path_factory)


# ---------------------------------------------------------------------------------------------------- the header and the ABI
def test_every_declared_symbol_is_exported(lib):
    from quadsim_amd import dynplan
    side_cases.check_exports("dyn", lib, ["qsd_last_error", "qsd_net_image_bytes", "qsd_net_pack", "qsd_plan_workspace_bytes", "qsd_shooting_plan",
                                          "qsd_version"])
    assert sorted(dynplan.EXPORTS) == side_cases.declared("dyn")


C_CALLER = r"""
#include <stdio.h>
#include <string.h>
#include "quadsim_dyn.h"

static int refused(int rc, const char *what)
{
    if (rc == QSD_OK || strlen(qsd_last_error()) == 0) { printf("NOT-REFUSED:%s\n", what); return 0; }
    return 1;
}

int main(void)
{
    size_t bytes = 0, wbytes = 0;
    float x[16];
    double s[1];
    int32_t bi[1];
    QsdNet net;
    int ok = 1;
    void *fns[] = {(void *)qsd_version, (void *)qsd_last_error, (void *)qsd_net_image_bytes, (void *)qsd_net_pack,
                   (void *)qsd_plan_workspace_bytes, (void *)qsd_shooting_plan};
    memset(&net, 0, sizeof net);
    if (qsd_version() != QSD_VERSION) return 2;
    if (qsd_net_image_bytes(200, 100, &bytes) != QSD_OK || bytes != 120656) return 3;
    if (bytes > QSD_LDS_BYTES) return 4;
    if (qsd_plan_workspace_bytes(3, 200, &wbytes) != QSD_OK || wbytes != 3 * 200 * sizeof(double)) return 5;
    ok &= refused(qsd_net_image_bytes(209, 100, &bytes), "h1");
    ok &= refused(qsd_net_image_bytes(200, 113, &bytes), "h2");
    ok &= refused(qsd_net_image_bytes(0, 10, &bytes), "h1=0");
    ok &= refused(qsd_net_image_bytes(10, 10, NULL), "bytes");
    ok &= refused(qsd_plan_workspace_bytes(0, 200, &wbytes), "n=0");
    ok &= refused(qsd_net_pack(NULL, x, NULL), "net");
    net.struct_size = sizeof net; net.h1 = 20; net.h2 = 10;
    ok &= refused(qsd_net_pack(&net, NULL, NULL), "image");
    ok &= refused(qsd_net_pack(&net, x, NULL), "weights");
    ok &= refused(qsd_shooting_plan(NULL, 1, x, 0, 0, 0, 20, 200, x, x, s, bi, x, s, x, NULL), "image");
    ok &= refused(qsd_shooting_plan(x, 1, x, 0, 0, 0, 20, 200, x, x, s, bi, x, s, x, NULL), "unpacked image");
    ok &= refused(qsd_shooting_plan(x, 0, x, 0, 0, 0, 20, 200, x, x, s, bi, x, s, x, NULL), "n");
    ok &= refused(qsd_shooting_plan(x, 1, x, 0, 0, 0, 1025, 200, x, x, s, bi, x, s, x, NULL), "horizon");
    ok &= refused(qsd_shooting_plan(x, 1, x, 0, 0, 0, 20, 65537, x, x, s, bi, x, s, x, NULL), "paths");
    ok &= refused(qsd_shooting_plan(x, 1, x, 0, 0, (uint64_t)1 << 36, 20, 200, x, x, s, bi, x, s, x, NULL), "k");
    ok &= refused(qsd_shooting_plan(x, 1, NULL, 0, 0, 0, 20, 200, x, x, s, bi, x, s, x, NULL), "obs");
    ok &= refused(qsd_shooting_plan(x, 1, x, 0, 0, 0, 20, 200, NULL, x, s, bi, x, s, x, NULL), "workspace");
    ok &= refused(qsd_shooting_plan(x, 1, x, 0, 0, 0, 20, 200, x, NULL, s, bi, x, s, x, NULL), "actions");
    printf("%s %d\n", ok ? "ALL-REFUSED" : "FAILED", (int)(sizeof fns / sizeof fns[0]));
    return ok ? 0 : 1;
}
"""


def test_header_is_c99_and_every_refusal_launches_nothing(lib, tmp_path):
    """a plain C program, -std=c99 -Wall -Werror, linked against the new library alone; it runs here, without a device, so
    every call it makes returns before a launch"""
    side_cases.run_c_caller("dyn", C_CALLER, tmp_path)


def test_python_checks_refuse_before_the_library_is_touched():
    import torch
    from quadsim_amd import dynplan
    for bad in ((0, 10), (10, 0), (209, 100), (200, 113), (129, 128)):
        with pytest.raises(ValueError):
            dynplan.check_widths(*bad)
    assert dynplan.check_widths(200, 100)[2] == (208, 112)
    assert dynplan.check_widths(100, 50)[2] == (128, 128)
    assert dynplan.check_widths(20, 10)[2] == (64, 64)
    for kw in (dict(horizon=0), dict(horizon=1025), dict(paths=0), dict(paths=65537), dict(k=1 << 36), dict(k=-1), dict(n=0)):
        args = dict(horizon=20, paths=200, k=0, n=1)
        args.update(kw)
        with pytest.raises(ValueError):
            dynplan.check_plan_args(**args)
    assert dynplan.check_plan_args(1024, 65536, (1 << 36) - 1, 1) == (1024, 65536, (1 << 36) - 1, 1)
    net = dr.to_net(dr.weight_set("he_20_10"), "cpu")
    obs = torch.zeros(2, 12)
    for kw in (dict(horizon=0), dict(paths=65537), dict(k=1 << 36), dict(gid0=-1), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            dynplan.learned_shooting_plan(net, obs, **kw)
    for wrong in (torch.zeros(2, 13), torch.zeros(2, 12, dtype=torch.float64), torch.zeros(12), torch.zeros(0, 12)):
        with pytest.raises(ValueError):
            dynplan.learned_shooting_plan(net, wrong)
    with pytest.raises(ValueError):
        dynplan.learned_shooting_plan(object(), obs)
    with pytest.raises(ValueError):
        dynplan.DynamicsNet.from_arrays(np.zeros((20, 15)), np.zeros(20), np.zeros((10, 20)), np.zeros(10), np.zeros((12, 10)), np.zeros(12),
                                        device="cpu")
    with pytest.raises(ValueError):
        net.set_normalisers(in_mean=np.zeros(12))


# ---------------------------------------------------------------------------------------------------- the census
def _instantiations(notes):
    got = set()
    for sym in notes:
        m = re.match(r"^_ZN3qsd(\d+)(k_\w+?)(?:I((?:Li\d+E)+)E)?(?:E|Ev)", sym)
        assert m and int(m.group(1)) == len(m.group(2)), "a kernel outside namespace qsd: %s" % sym
        got.add((m.group(2),) + tuple(int(a) for a in re.findall(r"Li(\d+)E", m.group(3) or "")))
    return got


@pytest.fixture(scope="module")
def census(notes):
    return side_cases.check_census(notes, dynplan_matrix, _instantiations, "dynplan")


def test_rows_are_exactly_the_kernels_of_the_code_object(census):
    keys = [r["key"] for r in dynplan_matrix.ROWS]
    from quadsim_amd import dynplan
    assert {(16 * k[1], 16 * k[2]) for k in keys if k[0] == "k_dyn_plan"} == set(dynplan.COMPILED_WIDTHS)
    assert {r["widths"] for r in dynplan_matrix.ROWS if r["widths"]} == set(dynplan.COMPILED_WIDTHS)


def test_rows_name_existing_gpu_tests():
    side_cases.check_rows_name_gpu_tests(dynplan_matrix)


def test_no_kernel_uses_scratch_or_spills_and_each_fits_lds(census):
    assert max(fl["group_segment_fixed_size"] for k, fl in census.items() if k[0] == "k_dyn_plan") == 120656        # the 208 x 112 image, as the header says


def test_main_library_is_built_without_the_new_fragments():
    """the second library's fragments are not dependencies of libquadsim_hip.so, and its kernels are not in it"""
    from quadsim_amd import _lib
    assert not [h for h in _lib.HEADERS if "side_host" in h]
    side_cases.check_entry("dyn", ["dynplan_host.hpp", "dynplan_image.hpp", "dynplan_kernels.hpp", "quadsim_device.hpp", "quadsim_dyn.h",
                                   "side_host.hpp"], "dynplan.hip")
    assert _lib.build_library() == _lib.LIB_PATH and os.path.exists(_lib.SIDE["dyn"]["path"])
    side_cases.check_no_foreign_kernels("dyn")


# ---------------------------------------------------------------------------------------------------- the image's permutation
def test_pi_orders_every_chain_ascending():
    """csrc/dynplan_image.hpp: unit u sits at row pi(u); k-step i of tile t sums the rows {16 t + 4 g + i}, g ascending"""
    pi = lambda u: (u & ~15) | ((u & 3) << 2) | ((u >> 2) & 3)     # noqa: E731
    assert all(pi(pi(u)) == u for u in range(208))
    order = [pi(16 * t + 4 * g + i) for t in range(13) for i in range(4) for g in range(4)]
    assert order == list(range(208))


# ---------------------------------------------------------------------------------------------------- reference and bound
@pytest.mark.parametrize("name", sorted(dr.WEIGHT_SETS) + ["zero", "wiring"])
def test_float32_chain_is_inside_the_bound(name):
    W = {"zero": dr.weights_zero, "wiring": dr.weights_wiring}[name]() if name in ("zero", "wiring") else dr.weight_set(name)
    rng = np.random.default_rng(7)
    n = 192
    s = dr.sample_obs(n, seed=43)
    s[:8] *= 8.0                                           # far observations too
    a = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    worst = 0.0
    for _ in range(4):                                     # a few steps along the model's own trajectory
        ref, bound = dr.step64(W, s, a, with_bound=True)
        got = dr.step32(W, s, a)
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), "%s: worst err / bound %.3g" % (name, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
        s = got
    print("dynplan ratio float32-emulation %s worst err/bound %.3g" % (name, worst))
    # on the generic nets the bound is within a small factor of what float32 does (the cancelling net is built so that it is not)
    assert worst < 1.0 and (not name.startswith(("he_", "ref_")) or worst > 1e-3)


# ---------------------------------------------------------------------------------------------------- the width edges
def _image_bytes(p1, p2):
    """include/quadsim_dyn.h: header, three padded layers with rows 16 T + 4 floats apart, four normalisers"""
    t1, t2 = p1 // 16, p2 // 16
    return 4 * (4 + 16 * t1 * 20 + 16 * t1 + 16 * t2 * (16 * t1 + 4) + 16 * t2 + 16 * (16 * t2 + 4) + 16 + 64)


def test_edge_widths_route_to_the_table(lib):
    """check_widths, qsd_net_image_bytes (choose_tiles) and DynamicsNet agree with dynplan_ref.EDGE_WIDTHS on every entry: the
    first compiled pair that covers both widths"""
    from quadsim_amd import dynplan
    assert _image_bytes(208, 112) == 120656
    assert len(dr.EDGE_WIDTHS) == 9 and set(dr.EDGE_WIDTHS.values()) == set(dynplan.COMPILED_WIDTHS)
    for (h1, h2), compiled in dr.EDGE_WIDTHS.items():
        assert dynplan.check_widths(h1, h2) == (h1, h2, compiled)
        nbytes = C.c_size_t(0)
        assert lib.qsd_net_image_bytes(h1, h2, C.byref(nbytes)) == 0, lib.qsd_last_error()
        assert nbytes.value == _image_bytes(*compiled), (h1, h2)
        W = dr.weight_set(dr.edge_name(h1, h2))
        net = dr.to_net(W, "cpu")
        assert (net.h1, net.h2, net.compiled) == (h1, h2, compiled)
        assert W["w1"].shape == (h1, 16) and W["w2"].shape == (h2, h1) and W["w3"].shape == (12, h2)
        assert all(np.all(W[k] != 0) for k in dr.WEIGHT_KEYS), "an edge set is dense"
        assert W["b1"][-1] == 2.0 and W["b2"][-1] == 2.0


@pytest.mark.parametrize("name", dr.EDGE_SETS)
def test_edge_fixture_detects_a_dropped_last_unit(name):
    """on the model steps of the planners' edge test (dynplan_ref.edge_plan_rows), the float64 step of the net with the last
    unit of layer 1 cut off (column h1 - 1 of w2 zeroed), and of the net with the last unit of layer 2 cut off (column h2 - 1 of
    w3 zeroed), is out of step_bound on at least one element: a kernel that dropped the unit could not pass.  The float32 chain
    of the whole net stays inside the bound on the same rows."""
    W = dr.weight_set(name)
    h1, h2 = W["w1"].shape[0], W["w2"].shape[0]
    obs, acts, before = dr.edge_plan_rows(W)
    assert before.shape == (2, 33, 5, 12) and np.array_equal(before[:, :, 0], np.repeat(obs[:, None], 33, axis=1))
    ref, bound = dr.step64(W, before, acts, with_bound=True)
    ratios = []
    for key, col in (("w2", h1 - 1), ("w3", h2 - 1)):
        M = dict(W)
        M[key] = W[key].copy()
        M[key][:, col] = 0.0
        r = np.abs(dr.step64(M, before, acts) - ref) / bound
        ratios.append(float(r.max()))
        assert (r > 1.0).any(), "%s: zeroing column %d of %s stays inside the bound everywhere (worst %.3g)" % (name, col, key, r.max())
    err = np.abs(dr.step32(W, before.astype(np.float32), acts).astype(np.float64) - dr.step64(W, before.astype(np.float32), acts))
    r32 = float((err / dr.step_bound(W, before.astype(np.float32), acts)).max())
    print("dynplan edge %s seed %d mutant err/bound: w2 column %.3g, w3 column %.3g; float32 chain %.3g" % (
        name, dr.EDGE_WEIGHT_SEEDS[(h1, h2)], ratios[0], ratios[1], r32))
    assert r32 < 1.0


def test_rows_with_widths_name_a_net_of_exactly_those_widths():
    """a row's `widths` are the hidden widths of the net its test id names (the widest the instantiation takes)"""
    from quadsim_amd import dynplan
    for r in dynplan_matrix.ROWS:
        if r["widths"]:
            W = dr.weight_set(re.search(r"\[(\w+)\]$", r["test"]).group(1))
            assert (W["w1"].shape[0], W["w2"].shape[0]) == r["widths"], r
            assert dynplan.check_widths(*r["widths"])[2] == r["widths"] == (16 * r["key"][1], 16 * r["key"][2]), r


@pytest.mark.parametrize("name", ["ref_200_100", "he_20_10", "cancel"])
def test_predict_in_float64_is_the_restatement(name):
    import torch
    W = dr.weight_set(name)
    net = dr.to_net(W, "cpu")
    assert np.array_equal(net.in_rscale.numpy(), dr.rscale(W))
    s = dr.sample_obs(64, seed=44)
    a = np.random.default_rng(8).uniform(-1, 1, (64, 4)).astype(np.float32)
    got = net.predict(torch.as_tensor(s, dtype=torch.float64), torch.as_tensor(a, dtype=torch.float64)).numpy()
    ref, bound = dr.step64(W, s, a, with_bound=True)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-13)
    got32 = net.predict(torch.as_tensor(s), torch.as_tensor(a)).numpy()            # the float32 formula: torch's summation order
    assert got32.dtype == np.float32 and (np.abs(got32 - ref) <= bound).all()


def test_choose64_is_choose_action_on_the_wiring_net():
    """closed form: with delta = 0.1 a the costs follow from the cumulative sums of the actions"""
    W = dr.weights_wiring()
    rng = np.random.default_rng(9)
    obs = dr.sample_obs(2, seed=45)
    acts = rng.uniform(-1, 1, (2, 50, 6, 4)).astype(np.float32)
    first, j, costs = dr.choose64(W, obs, acts)
    csum = np.cumsum(np.float32(0.1).astype(np.float64) * acts[..., :3].astype(np.float64), axis=2)
    pos = obs[:, None, None, :3].astype(np.float64) + np.concatenate([np.zeros((2, 50, 1, 3)), csum[:, :, :-1]], axis=2)
    closed = -np.sum(pos ** 2, axis=(2, 3))
    np.testing.assert_allclose(costs, closed, rtol=1e-12)
    assert np.array_equal(j, np.argmax(closed, axis=1)) and np.array_equal(first, acts[np.arange(2), j, 0])


def test_pack_is_cached_until_a_weight_changes():
    """the cache key follows in-place updates and assignments; packing itself needs a device and is refused without one"""
    from quadsim_amd import QuadsimError
    net = dr.to_net(dr.weight_set("he_20_10"), "cpu")
    with pytest.raises(QuadsimError):
        net.pack()
    key = lambda: tuple((t.data_ptr(), t._version) for t in net._tensors())     # noqa: E731
    k0 = key()
    net.w2.mul_(1.5)
    assert key() != k0
    k1 = key()
    net.set_normalisers(in_std=np.full(16, 2.0))
    assert key() != k1 and net._image_key is None


def test_from_torch_reads_the_three_linear_layers():
    import torch
    from quadsim_amd.dynplan import DynamicsNet
    torch.manual_seed(3)
    module = torch.nn.Sequential(torch.nn.Linear(16, 20), torch.nn.ReLU(), torch.nn.Linear(20, 10), torch.nn.ReLU(), torch.nn.Linear(10, 12))
    net = DynamicsNet.from_torch(module, device="cpu").set_normalisers(in_std=np.full(16, 1.0 - 1.0e-6))
    assert (net.h1, net.h2, net.compiled) == (20, 10, (64, 64)) and bool((net.in_rscale == 1.0).all())
    s, a = torch.as_tensor(dr.sample_obs(8, seed=46)), torch.rand(8, 4) * 2 - 1
    with torch.no_grad():
        want = module(torch.cat([s, a], dim=1)) + s
    assert torch.equal(net.predict(s, a), want)
    assert not any(p.requires_grad for p in net.parameters())
    with pytest.raises(ValueError):
        DynamicsNet.from_torch(torch.nn.Linear(16, 12), device="cpu")
