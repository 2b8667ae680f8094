"""-m "not gpu": the harness of tests/test_gpu_layer1.py is checked before the GPU is.  tests/layer1_matrix.py names exactly the
__global__ functions of csrc/layer1_kernels.hpp, all in the built code object, and the census points at it; the input builders of
tests/layer1_ref.py put every row where it was meant to be (the float64 reference says so); the float32 oracle -- libm float32 --
meets every bound on the inputs the GPU rows use, so every bound can be met; each of twenty-odd wrong kernels, a small edit of the
reference's own output, is rejected by its checker; and no quaternion an env can hold hands q_atan2 an argument outside the
domain include/quadsim.h states."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kernel_notes
import layer1_matrix
import layer1_ref as L
import lifecycle_matrix
import lifecycle_ref
from oracle.pyoracle import Oracle
from test_lifecycle_cpu import _collected, notes  # noqa: F401  (notes: the module-scoped fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
CPU_N = (1, 65, 257, 1000)                 # the references have no lanes or blocks: four of the GPU env counts
N = 257


def _dev(a):
    return np.asarray(a).astype(f32)


# ---------------------------------------------------------------------------------------------------- the matrix and the census
def test_rows_are_unique_and_cover_every_branch():
    keys = [r["key"] for r in layer1_matrix.ROWS]
    assert len(keys) == len(set(keys)) == 16
    per = {k: sum(1 for r in layer1_matrix.ROWS if r["kernel"] == k) for k in layer1_matrix.KERNELS}
    assert per == {"k_drone_step": 8, "k_ctrl": 3, "k_transform": 4, "k_rel_obs": 1}
    assert {tuple(r) for r in map(sorted, map(dict.keys, layer1_matrix.ROWS))} == {("entry", "id", "kernel", "key", "test")}
    assert L.N_ENVS == lifecycle_ref.N_ENVS


def test_kernel_list_is_every_plain_kernel_of_the_header(notes):  # noqa: F811
    src = open(os.path.join(ROOT, "quadsim_amd", "csrc", "layer1_kernels.hpp")).read()
    found = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src))
    assert found == set(layer1_matrix.KERNELS), found ^ set(layer1_matrix.KERNELS)
    got = kernel_notes.anon_instantiations(notes, layer1_matrix.KERNELS)
    assert got == {(k,) for k in layer1_matrix.KERNELS}, got


def test_rows_name_existing_gpu_tests():
    ids = _collected({r["test"].split("::")[0] for r in layer1_matrix.ROWS})
    missing = [r["test"] for r in layer1_matrix.ROWS if r["test"] not in ids]
    assert not missing, missing


def test_census_points_at_this_matrix():
    for k in layer1_matrix.KERNELS:
        assert lifecycle_matrix.CENSUS[k] == "layer1_matrix"


# ---------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("integ", [0, 1])
def test_drone_inputs_are_where_they_were_meant_to_be(integ):
    o64 = Oracle("f64")
    for n in (1, N):
        x = L.drone_inputs(n, integ, True)
        flat = np.concatenate([x[k].reshape(-1) for k in ("state", "u_prev", "u", "par")])
        assert len(np.unique(flat)) == flat.size, "two words of the input are equal"
        assert np.abs(x["par"] / np.asarray(L.PAR_NOM, f32) - 1).max() <= 0.1501 and L.PAR_NOM != (0.18, 0.00025, 0.000232, 0.0003738)
        pre = L.pre_clamp(o64, x, integ)
        assert (pre["margin"] >= L.MARGIN).all() and (pre["cond"] <= L.COND_MAX).all()
        ref = L.drone_ref(x, integ)
        # the float64 integration + limiter decision of this module is the oracle's own
        assert np.array_equal(L.violated(pre).any(1), ref["limited"] != 0)
    norm = np.linalg.norm(x["state"][:, 6:10].astype(f64), axis=1)
    assert norm.min() < 0.7 and norm.max() > 1.5 and 20 < ref["limited"].sum() < n - 20
    clamped = np.abs(ref["u_prev"][:, 0] - x["u"][:, 0]) > 1e-3
    assert 20 < clamped.sum() < n - 20, "the rotor clamp is active on a part of the rows, not all"


@pytest.mark.parametrize("integ", [0, 1])
def test_limiter_inputs_violate_every_subset(integ):
    o64 = Oracle("f64")
    x, which = L.limiter_inputs(integ)
    pre = L.pre_clamp(o64, x, integ)
    v = L.violated(pre)
    body = which >= 0
    assert (pre["margin"][body] >= L.MARGIN).all()
    for k, sub in enumerate(L.SUBSETS):
        rows = which == k
        assert rows.sum() >= 32 and (v[rows] == np.array(sub, bool)).all()
        for a in np.nonzero(sub)[0]:
            sg = np.sign(pre["angles"][rows][:, a])
            assert (sg > 0).sum() >= 4 and (sg < 0).sum() >= 4, "subset %s: one sign of axis %d only" % (sub, a)
        if sub[0] and not sub[1]:
            assert (pre["r12"][rows] >= 1).sum() >= 4 and (pre["r12"][rows] < -1).sum() >= 4, "saturated branches of subset %s" % (sub,)
    # the last row: r12 == -1.0f exactly in float32 arithmetic, not saturated, limited on roll
    q = x["state"][-1, 6:10]
    assert f32(2) * (q[0] * q[1] + q[2] * q[3]) == f32(-1) and pre["r12"][-1] == -1.0 and not pre["sat"][-1] and v[-1].tolist() == [True, False, False]
    assert L.drone_ref(x, integ)["limited"].all()


@pytest.mark.parametrize("integ", [0, 1])
def test_band_rungs_outside_the_band_are_on_their_side(integ):
    x, axis, want, actual = L.band_inputs(integ)
    assert len(axis) == 3 * 2 * len(L.LADDER) * L.BAND_ROWS
    for a, name in enumerate(L.AXES):
        assert 1e-7 < L.DELTA0[name] < 1e-5, "DELTA0 is far below the 1e-4 of the golden test"
        clear = (axis == a) & (np.abs(want) >= 5 * L.DELTA0[name])
        assert clear.sum() >= 6 * L.BAND_ROWS
        assert (np.sign(actual[clear]) == np.sign(want[clear])).all() and (np.abs(actual[clear]) >= L.DELTA0[name]).all()
        assert np.abs(actual[axis == a] - want[axis == a]).max() < L.DELTA0[name], "a row is further from its rung than float32 explains"
    out = L.outside_band(axis, actual)
    assert 0.6 * len(axis) < out.sum() < len(axis)
    ref = L.drone_ref(x, integ)
    assert np.array_equal(ref["limited"] != 0, actual >= 0)
    o32 = L.drone_ref(x, integ, prec="f32")
    flips = ref["limited"] != o32["limited"]
    print("layer1 band float32-oracle integ=%d flips inside %d of %d, outside %d" % (integ, (flips & ~out).sum(), (~out).sum(), (flips & out).sum()))
    assert not (flips & out).any()


def test_other_inputs_are_what_the_cases_need():
    x = L.ctrl_inputs(N)
    flat = np.concatenate([v.reshape(-1) for v in x.values()])
    assert len(np.unique(flat)) == flat.size and (np.abs(x["state_des"][:, 10:13]) >= 0.1).all()
    r = L.rel_obs_inputs(N)
    assert len(np.unique(np.concatenate([r["chaser"], r["target"]]))) == 2 * N * 13
    q = L.transform_inputs(0, N).astype(f64)
    e = L.entries(q)
    assert (e["r12"] >= 1).sum() >= 4 and (e["r12"] < -1).sum() >= 4 and (e["r12"] == -1).sum() == 1
    R = L.transform_inputs(3, N)
    assert (R[:, 5] == 1).sum() == 1 and (R[:, 5] == -1).sum() == 1 and (R[:, 5] > 1).sum() > 30 and (R[:, 5] < -1).sum() > 30
    assert np.abs(L.transform_inputs(1, N)).max() > 6
    Ra, xs = L.asin_sweep()
    X, a = L.sincos_sweep()
    assert max(len(Ra), len(L.atan2_sweep()), len(X)) <= 2 ** 22
    for v in (0.0, 0.5, 1.0, np.nextafter(f32(1), f32(2)), np.nextafter(f32(0.5), f32(1))):
        assert (xs == f32(v)).any() and (xs == -f32(v)).any()
    assert np.signbit(xs[xs == 0]).any() and not np.signbit(xs[xs == 0]).all()
    assert np.abs(a).max() == f32(1e4) and (X[:, 0].astype(f64) == 2.0 * a.astype(f64)).all()


def test_bounds_are_what_the_docstring_says():
    assert abs(L.sincos_bound(0.3) - 1.04e-7) < 1e-9 and abs(L.sincos_bound(2.0) - 1.34e-7) < 1e-9
    assert L.sincos_bound(1e4) - L.sincos_bound(2.0) < 1.3e-11
    assert L.sincos_bound(6.0) <= 1.5e-7, "no looser than the figure test_gpu_parity.py asserts on |x| <= 6"
    xs = np.linspace(-1, 1, 20001)
    assert L.asin_bound(xs).max() < 2.7e-7 and L.asin_bound(0.5) < 6.9e-8 and L.asin_bound(1e-3) < 1.3e-10
    ang = np.linspace(-np.pi, np.pi, 20001)
    b = L.atan2_bound(np.sin(ang), np.cos(ang))
    assert b.max() < 5.1e-7 and b[np.abs(ang) < np.pi / 4].max() < 1.93e-7 and b[np.abs(ang) < np.pi / 2].max() < 3.0e-7
    assert b.max() <= 6e-7, "no looser than the yaw figure of test_gpu_parity.py"
    out = subprocess.run([sys.executable, os.path.join("tools", "fit_polys.py")], cwd=ROOT, capture_output=True, text=True, timeout=600).stdout
    # what the tool prints for the polynomials in use, never above the constants of layer1_ref
    m = re.search(r"atan deg 8 max abs err (\S+) max ulp-ish rel (\S+)", out)
    assert float(m.group(1)) <= L.RES_ATAN_ABS and float(m.group(2)) <= L.RES_ATAN_REL, out
    m = re.search(r"asin deg 4 max abs err lo (\S+) hi (\S+)", out)
    assert float(m.group(1)) <= L.RES_ASIN_LO and float(m.group(2)) <= L.RES_ASIN_HI, out
    m = re.search(r"series-defined targets\nsincos deg 2 sin err (\S+) cos err (\S+)", out)
    assert float(m.group(1)) <= L.RES_SIN and float(m.group(2)) <= L.RES_COS, out


# ---------------------------------------------------------------------------------------------------- float32 within the bounds
@pytest.mark.parametrize("n", CPU_N)
def test_float32_oracle_meets_every_bound(n):
    worst = {}
    for integ in (0, 1):
        for par_given in (False, True):
            x = L.drone_inputs(n, integ, par_given)
            b = dict(x, limited=np.full(n, 0xA5, np.uint8))
            ref = L.drone_ref(x, integ)
            o32 = L.drone_ref(x, integ, prec="f32")
            worst["drone_step-%d-%d" % (integ, par_given)] = L.check_drone_step(b, L.as_device(o32), ref)
            L.check_drone_step(b, L.as_device(o32, False), ref, limited_given=False)
    x = L.ctrl_inputs(n)
    for mode in (0, 1):
        ref, o32 = L.ctrl_ref(x, mode), L.ctrl_ref(x, mode, prec="f32")
        worst["ctrl-%d" % mode] = L.check_ctrl(x, dict(state_des=_dev(o32["state_des"]), u=_dev(o32["u"])), ref, mode)
    for op in range(4):
        xi = L.transform_inputs(op, n)
        worst["transform-%d" % op] = L.check_transform(op, xi, dict(out=_dev(L.transform_ref(op, xi, prec="f32"))), L.transform_ref(op, xi))
    x = L.rel_obs_inputs(n)
    worst["rel_obs"] = L.check_rel_obs(x, dict(obs=_dev(L.rel_obs_ref(x, prec="f32"))), L.rel_obs_ref(x))
    for k, v in worst.items():
        print("layer1 ratio float32-oracle %s n=%d %s" % (k, n, {a: round(b, 4) for a, b in v.items()}))


@pytest.mark.parametrize("integ", [0, 1])
def test_float32_oracle_meets_the_bounds_on_the_limiter_rows(integ):
    x, which = L.limiter_inputs(integ)
    ref, o32 = L.drone_ref(x, integ), L.drone_ref(x, integ, prec="f32")
    r = L.check_drone_step(dict(x, limited=np.full(len(which), 0xA5, np.uint8)), L.as_device(o32), ref)
    print("layer1 ratio float32-oracle limiter-subsets integ=%d %s" % (integ, r))
    x, axis, want, actual = L.band_inputs(integ)
    out = L.outside_band(axis, actual)
    sel = lambda d: {k: (None if v is None else v[out]) for k, v in d.items()}            # noqa: E731
    ref, o32 = L.drone_ref(x, integ), L.drone_ref(x, integ, prec="f32")
    r = L.check_drone_step(dict(sel(x), limited=np.full(out.sum(), 0xA5, np.uint8)), sel(L.as_device(o32)), sel(ref))
    print("layer1 ratio float32-oracle limiter-band integ=%d %s" % (integ, r))


def _libm_rot2euler(R):
    out = np.zeros((len(R), 3), f32)
    sat = (R[:, 5] >= 1) | (R[:, 5] < -1)
    out[:, 0] = np.arcsin(np.clip(R[:, 5].astype(f64), -1, 1))
    out[:, 1] = np.where(sat, 0.0, np.arctan2(-R[:, 2].astype(f64), R[:, 8].astype(f64)))
    out[:, 2] = np.arctan2(-R[:, 3].astype(f64), R[:, 4].astype(f64))
    return out


def test_correctly_rounded_float32_meets_the_sweep_bounds():
    """float64 results rounded to float32 (what a correctly rounded float32 libm gives) are inside every sweep bound, and every
    binade of float32 is clean: the sweeps and the domain search work"""
    R, _ = L.asin_sweep()
    print("layer1 ratio float32-rounded asin %.4f" % L.check_asin_sweep(R, _libm_rot2euler(R)))
    R = L.atan2_sweep()
    print("layer1 ratio float32-rounded atan2 %.4f" % L.check_atan2_sweep(R, _libm_rot2euler(R)))
    X, a = L.sincos_sweep()
    out = np.zeros((len(a), 4), f32)
    out[:, 0], out[:, 1] = np.cos(a.astype(f64)), np.sin(a.astype(f64))
    print("layer1 ratio float32-rounded sin %.4f cos %.4f" % L.check_sincos_sweep(a, out))
    R, es = L.domain_sweep()
    out = _libm_rot2euler(R)
    assert L.clean_binades(R, es, out) == (-149, 127)
    out[es > L.ATAN2_HI + 1, 1] = np.nan
    out[es < L.ATAN2_LO - 1, 2] = 0
    assert L.clean_binades(R, es, out) == (L.ATAN2_LO - 1, L.ATAN2_HI + 1)
    q, es = L.quat_domain_sweep()
    lo, hi = L.clean_quat_binades(q, es, _dev(L.transform_ref(0, q, prec="f32")), _dev(L.transform_ref(2, q, prec="f32")))
    assert lo <= L.QUAT_LO - 1 and hi >= L.QUAT_HI + 1, (lo, hi)


# ---------------------------------------------------------------------------------------------------- wrong kernels
def _drone_case(integ=0, limiter=False):
    x = L.limiter_inputs(integ)[0] if limiter else L.drone_inputs(N, integ, True)
    n = x["state"].shape[0]
    ref = L.drone_ref(x, integ)
    before = dict(x, limited=np.full(n, 0xA5, np.uint8))
    L.check_drone_step(before, L.as_device(ref), ref)                     # the reference's own output passes
    return x, before, ref


def _with(x, **kw):
    y = {k: (None if v is None else v.copy()) for k, v in x.items()}
    y.update(kw)
    return y


def _drone_mutants():
    def nominal_par(x, ref, integ):
        return L.as_device(L.drone_ref(_with(x, par=None), integ))

    def mass_from_inertia(x, ref, integ):
        par = x["par"].copy(); par[:, 0] = par[:, 1]
        return L.as_device(L.drone_ref(_with(x, par=par), integ))

    def other_integrator(x, ref, integ):
        return L.as_device(L.drone_ref(x, 1 - integ))

    def row_from_previous(x, ref, integ):
        return {k: np.roll(v, 1, axis=0) for k, v in L.as_device(ref).items()}

    def last_row_not_written(x, ref, integ):
        d = L.as_device(ref)
        d["state"][-1], d["u_prev"][-1], d["limited"][-1] = x["state"][-1], x["u_prev"][-1], 0xA5
        return d

    def limited_inverted(x, ref, integ):
        d = L.as_device(ref); d["limited"] = (1 - d["limited"]).astype(np.uint8)
        return d

    def limited_255(x, ref, integ):
        d = L.as_device(ref); d["limited"] = (d["limited"] * 255).astype(np.uint8)
        return d

    def control_not_limited(x, ref, integ):
        d = L.as_device(ref); d["u_prev"] = x["u"].copy()
        return d

    def integrated_with_new_control(x, ref, integ):
        d = L.as_device(L.drone_ref(_with(x, u_prev=x["u"]), integ))
        d["u_prev"] = L.as_device(ref)["u_prev"]
        return d

    def rates_not_zeroed(x, ref, integ):
        d = L.as_device(ref)
        o64 = Oracle("f64")
        for i in np.nonzero(ref["limited"])[0]:
            d["state"][i, 10:13] = L.integrate64(o64, x["state"][i], x["u_prev"][i], x["par"][i], L.DT, integ)[10:13]
        return d

    def first_axis_wins(x, ref, integ):
        return L.as_device(L.first_axis_wins(x, ref, integ))

    return {"nominal_parameters_although_par_is_given": (nominal_par, 0, False), "mass_read_from_the_inertia_column": (mass_from_inertia, 0, False),
            "frozen_where_rk4_was_asked": (other_integrator, 1, False), "rk4_where_frozen_was_asked": (other_integrator, 0, False),
            "row_i_from_row_i_minus_1": (row_from_previous, 0, False), "last_row_not_written": (last_row_not_written, 0, False),
            "limited_inverted": (limited_inverted, 0, False), "limited_written_as_255": (limited_255, 0, False),
            "new_control_not_limited": (control_not_limited, 0, False), "integrated_with_the_new_control": (integrated_with_new_control, 1, False),
            "rates_not_zeroed_after_a_clamp": (rates_not_zeroed, 1, False), "first_violated_axis_wins": (first_axis_wins, 0, True)}


@pytest.mark.parametrize("mutant", sorted(_drone_mutants()))
def test_wrong_drone_steps_are_rejected(mutant):
    edit, integ, limiter = _drone_mutants()[mutant]
    x, before, ref = _drone_case(integ, limiter)
    with pytest.raises(AssertionError):
        L.check_drone_step(before, edit(x, ref, integ), ref)


def test_a_limited_buffer_written_although_null_is_rejected():
    x, before, ref = _drone_case()
    L.check_drone_step(before, L.as_device(ref, False), ref, limited_given=False)
    with pytest.raises(AssertionError):
        L.check_drone_step(before, L.as_device(ref, True), ref, limited_given=False)
    with pytest.raises(AssertionError):                                   # ... and an input that was written
        L.check_drone_step(before, dict(L.as_device(ref), u=x["u"] + f32(1)), ref)


def _ctrl_mutants():
    def keeps_desired_rates(x, d, mode):
        d["state_des"][:, 10:12] = x["state_des"][:, 10:12]

    def clears_word_12(x, d, mode):
        d["state_des"][:, 12] = 0

    def mode0_uses_state_last(x, d, mode):
        d["u"][:, 0] += f32(L.MASS) * f32(0.1) * (x["state"][:, 5] - x["state_last"][:, 5])

    def mode1_dv_zero(x, d, mode):
        r = L.ctrl_ref(x, 1, use_last=x["state"])
        d["u"], d["state_des"] = _dev(r["u"]), _dev(r["state_des"])

    def writes_position_words(x, d, mode):
        d["state_des"][-1, 2] = np.nextafter(d["state_des"][-1, 2], f32(0))

    return {"desired_rates_left_as_they_were": (keeps_desired_rates, 0), "word_12_cleared": (clears_word_12, 0),
            "mode_0_uses_state_last": (mode0_uses_state_last, 0), "mode_1_with_dv_zero": (mode1_dv_zero, 1),
            "a_position_word_moved_by_one_ulp": (writes_position_words, 1)}


@pytest.mark.parametrize("mutant", sorted(_ctrl_mutants()))
def test_wrong_controllers_are_rejected(mutant):
    edit, mode = _ctrl_mutants()[mutant]
    x = L.ctrl_inputs(N)
    ref = L.ctrl_ref(x, mode)
    d = dict(state_des=_dev(ref["state_des"]), u=_dev(ref["u"]))
    L.check_ctrl(x, d, ref, mode)
    edit(x, d, mode)
    with pytest.raises(AssertionError):
        L.check_ctrl(x, d, ref, mode)


def _transform_mutants():
    def computed_diagonal(x, out):
        n = x.astype(f64)[:, 1:4] / np.linalg.norm(x.astype(f64), axis=1, keepdims=True)
        out[:, 0] = 1 - 2 * (n[:, 1] ** 2 + n[:, 2] ** 2)
        out[:, 4] = 1 - 2 * (n[:, 0] ** 2 + n[:, 2] ** 2)
        out[:, 8] = 1 - 2 * (n[:, 0] ** 2 + n[:, 1] ** 2)

    def symmetric_saturation_op0(x, out):
        r12 = L.entries(x.astype(f64))["r12"]
        out[r12 == -1, 1] = 0

    def symmetric_saturation_op3(x, out):
        out[x[:, 5] == -1, 1] = 0

    def theta_not_zeroed_op0(x, out):
        e = L.entries(x.astype(f64))
        sat = (e["r12"] >= 1) | (e["r12"] < -1)
        out[sat, 1] = np.arctan2(-e["r02"], e["r22"])[sat]

    def theta_not_zeroed_op3(x, out):
        sat = (x[:, 5] >= 1) | (x[:, 5] < -1)
        out[sat, 1] = np.arctan2(-x[:, 2].astype(f64), x[:, 8].astype(f64))[sat]

    def last_row_not_written(x, out):
        out[-1] = L.SENTINEL

    def row_from_previous(x, out):
        out[:] = np.roll(out, 1, axis=0)

    return {"quat2rot_with_a_computed_diagonal": (computed_diagonal, 2), "op_0_saturation_test_symmetric": (symmetric_saturation_op0, 0),
            "op_3_saturation_test_symmetric": (symmetric_saturation_op3, 3), "op_0_theta_not_zeroed_when_saturated": (theta_not_zeroed_op0, 0),
            "op_3_theta_not_zeroed_when_saturated": (theta_not_zeroed_op3, 3), "op_1_last_row_not_written": (last_row_not_written, 1),
            "op_2_row_i_from_row_i_minus_1": (row_from_previous, 2)}


@pytest.mark.parametrize("mutant", sorted(_transform_mutants()))
def test_wrong_transforms_are_rejected(mutant):
    edit, op = _transform_mutants()[mutant]
    x = L.transform_inputs(op, N)
    ref = L.transform_ref(op, x)
    out = _dev(ref)
    L.check_transform(op, x, dict(out=out), ref)
    edit(x, out)
    with pytest.raises(AssertionError):
        L.check_transform(op, x, dict(out=out), ref)


def test_atan2_of_zeros_equal_to_half_pi_is_rejected():
    R = L.atan2_sweep(m=1024)
    out = _libm_rot2euler(R)
    L.check_atan2_sweep(R, out)
    both0 = (R[:, 2] == 0) & (R[:, 8] == 0)
    assert both0.sum() == 4
    out[both0, 1] = np.pi / 2
    with pytest.raises(AssertionError):
        L.check_atan2_sweep(R, out)
    # ... and so is an asin that loses the sign of zero, or a clamp that lets nextafter(1) through
    R, x = L.asin_sweep()
    good = _libm_rot2euler(R)
    for edit in (lambda o: o.__setitem__((x == 0, 0), 0.0), lambda o: o.__setitem__((x > 1, 0), np.nextafter(f32(np.pi / 2), f32(2))),
                 lambda o: o.__setitem__((x == -1, 1), 0.0)):
        out = good.copy()
        edit(out)
        with pytest.raises(AssertionError):
            L.check_asin_sweep(R, out)


@pytest.mark.parametrize("mutant", ["observation_blocks_swapped", "chaser_and_target_swapped", "last_row_not_written"])
def test_wrong_observations_are_rejected(mutant):
    x = L.rel_obs_inputs(N)
    ref = L.rel_obs_ref(x)
    obs = _dev(ref)
    L.check_rel_obs(x, dict(obs=obs), ref)
    if mutant == "observation_blocks_swapped":
        obs[:, 0:6] = obs[:, [3, 4, 5, 0, 1, 2]]
    elif mutant == "chaser_and_target_swapped":
        obs = _dev(L.rel_obs_ref(dict(chaser=x["target"], target=x["chaser"])))
    else:
        obs[-1] = L.SENTINEL
    with pytest.raises(AssertionError):
        L.check_rel_obs(x, dict(obs=obs), ref)


# ---------------------------------------------------------------------------------------------------- the domain of q_atan2
def _entries_float32(q, fused):
    """(r10, r11, r02, r22) as the device evaluates them: every operation rounded to float32, or with every product fused into
    the sum that follows it (float64 holds a product of two float32 exactly)"""
    w, x, y, z = (q[:, i] for i in range(4))
    if not fused:
        two = f32(2)
        return two * (x * y - w * z), w * w - x * x + y * y - z * z, two * (x * z - w * y), w * w - x * x - y * y + z * z
    W, X, Y, Z = (q[:, i].astype(f64) for i in range(4))
    r = lambda v: v.astype(f32).astype(f64)                                               # noqa: E731
    r10 = 2 * r(X * Y - r(W * Z)); r02 = 2 * r(X * Z - r(W * Y))
    r11 = r(r(r(W * W - r(X * X)) + Y * Y) - Z * Z)
    r22 = r(r(r(W * W - r(X * X)) - Y * Y) + Z * Z)
    return r10.astype(f32), r11.astype(f32), r02.astype(f32), r22.astype(f32)


def test_no_env_quaternion_leaves_the_domain_of_q_atan2():
    """Every quaternion an env can hold -- |q| in [0.5, 2], widened to [0.4, 2.5]: the drift term K_quat e_quat q of Drone.df pulls
    N = |q|^2 towards 1 from both sides (dN/dt = 4 N (1 - N) + rotation, which preserves N), so a state that starts inside stays
    inside; the margin covers one step of float32 rounding many times over -- hands q_atan2 a pair that is two exact zeros or has
    max(|y|, |x|) inside [2^ATAN2_LO, 2^(ATAN2_HI + 1)), and never x = -0: random attitudes, gimbal lock to the last bit, exact cancellations, and
    components down to the denormals"""
    rs = np.random.RandomState(8)
    m = 200000
    qs = [L.quat_of(rs.uniform(-np.pi / 2, np.pi / 2, m), rs.uniform(-np.pi, np.pi, m), rs.uniform(-np.pi, np.pi, m))]
    qs.append(L.quat_of(np.where(rs.uniform(size=m) < 0.5, -1, 1) * (np.pi / 2 - 10.0 ** rs.uniform(-9, -1, m)), rs.uniform(-np.pi, np.pi, m),
                        rs.uniform(-np.pi, np.pi, m)))                                    # towards gimbal lock
    a, b = rs.uniform(0.1, 1, m), rs.uniform(0.1, 1, m)
    for perm in ((0, 0, 1, 1), (0, 1, 0, 1), (0, 1, 1, 0)):
        for sg in ((1, 1, 1, 1), (1, -1, 1, -1), (1, 1, -1, -1), (1, -1, -1, 1)):
            qs.append(np.stack([(a, b)[p] * s for p, s in zip(perm, sg)], -1)[:m // 10])  # exact cancellations: (a, a, b, b) in every order
    tiny = L.quat_of(rs.uniform(-1.5, 1.5, m), rs.uniform(-3, 3, m), rs.uniform(-3, 3, m))
    k = rs.randint(0, 4, m)
    tiny[np.arange(m), k] = 10.0 ** rs.uniform(-46, -15, m)                               # one component down to the denormals
    tiny[np.arange(m), (k + 1) % 4] *= np.where(rs.uniform(size=m) < 0.5, 1.0, 10.0 ** rs.uniform(-30, -10, m))
    qs.append(tiny)
    q = np.concatenate(qs)
    q = q / np.linalg.norm(q, axis=1, keepdims=True) * rs.uniform(0.4, 2.5, (len(q), 1))
    q = q.astype(f32)
    lo, hi = 2.0 ** L.ATAN2_LO, 2.0 ** (L.ATAN2_HI + 1)
    for fused in (False, True):
        r10, r11, r02, r22 = _entries_float32(q, fused)
        for y, x in ((r10, r11), (r02, r22)):
            mx = np.maximum(np.abs(y), np.abs(x)).astype(f64)
            assert ((mx == 0) | ((mx >= lo) & (mx < hi))).all(), q[~((mx == 0) | ((mx >= lo) & (mx < hi)))][:4]
            # ... and x is never -0: the default q_atan2 need not tell it from +0
            assert not (np.signbit(x) & (x == 0)).any()
    assert (np.maximum(np.abs(r10), np.abs(r11)) == 0).any() and (np.maximum(np.abs(r10), np.abs(r11)) < 1e-6).sum() > 1000
