"""-m "not gpu": the harness of tests/test_gpu_lifecycle.py is checked before the GPU is.  lifecycle_ref.reset_ref agrees with
Oracle("f64") (vec_reset, random_init, ctor_init) on every element those expose; the float32 oracle -- libm cosf / sinf
quaternions -- passes check_reset on the inputs the GPU rows use, so every bound can be met; twelve wrong resets, each a small
edit of the reference's output, are rejected; tests/lifecycle_matrix.py has exactly one row per compiled instantiation of the
twelve lifecycle kernels, and its census names every kernel of the built code object."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_notes
import lifecycle_matrix
import lifecycle_ref as lr
import step_matrix
from oracle.pyoracle import REC_LS, REC_QD, REC_UC, Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GID0, K0 = step_matrix.ROCRAND_GID0, step_matrix.ROCRAND_K0
CPU_N = (1, 65, 257, 1000)                 # the references have no lanes or blocks: four of the GPU env counts


def _before(n, source):
    rec = lr.busy_rec(n, 100 + n, hover=source == "hover")
    par = lr.distinct_par(n) if source == "rocrand2" else np.tile(np.asarray(lr.PAR_NOM, f32), (n, 1))
    return dict(rec=rec, par=par, ctr=K0)


def _args(source, n, rr=lr.RR):
    if source in ("rocrand1", "rocrand2"):
        return dict(seed=lr.SEED, ctr=K0, gid0=GID0, rr=rr, par_nom=lr.PAR_NOM)
    if source == "stored":
        return dict(init=np.concatenate(lr.stored_init(n, 7), 1))
    if source == "hover":
        return dict(init=lr.stored_init(n, 8, hover=True)[0])
    return {}


@pytest.fixture(scope="module")
def o64():
    return Oracle("f64")


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("randomise", [0, 1, 2])
@pytest.mark.parametrize("mask_kind", ["null", "alternating", "bytes_2_255"])
def test_reset_ref_agrees_with_the_float64_oracle(o64, randomise, mask_kind):
    """Oracle("f64").vec_reset on the same records: every word but the reset quaternion bit for bit (the oracle's is float32
    cosf / sinf: within QUAT_TOL), parameters bit for bit, observations within OBS_TOL"""
    n = 257
    source = ("nominal", "rocrand1", "rocrand2")[randomise]
    b = _before(n, source)
    mask = lr.make_mask(mask_kind, n)
    ref = lr.reset_ref(b["rec"], b["par"], mask, source, **_args(source, n))
    rec = b["rec"].astype(np.float64); par = b["par"].astype(np.float64)
    kw = dict(seed=lr.SEED, step_idx=K0, gid0=GID0, rr=lr.RR, par_nom=lr.PAR_NOM) if randomise else {}
    obs = o64.vec_reset(rec, par, mask=mask, randomise=randomise, **kw)
    notq = np.ones(40, bool); notq[6:10] = False
    assert np.array_equal(ref["rec"][:, notq], rec[:, notq])
    assert np.abs(ref["rec"][:, 6:10] - rec[:, 6:10]).max() <= lr.QUAT_TOL
    assert lr.same_bits(ref["par"], par.astype(f32))
    m = ref["masked"]
    np.testing.assert_allclose(ref["obs"][m], obs[m], rtol=1e-5, atol=2e-5)
    assert not ref["obs"][~m].any()
    if randomise:
        assert not ref["exact_rec"][m][:, 6:10].any() and ref["exact_rec"][m][:, :6].all() and ref["exact_rec"][~m].all()
        # the quaternion is the float64 one: unit to float64 rounding, which no float32 quaternion is
        assert np.abs(np.linalg.norm(ref["rec"][m][:, 6:10], axis=1) - 1).max() < 1e-15


def test_random_draw_and_ctor_ref_agree_with_the_oracle(o64):
    """every element random_init and ctor_init expose, at gids on both sides of 2^32"""
    for i in (0, 39, 40, 41, 999):
        gid = GID0 + i
        sc, st, par, u = o64.random_init(lr.SEED, lr.STREAM_RESET, gid, K0, lr.RR, lr.PAR_NOM)
        c, t, p, e = lr.random_draw(o64, lr.SEED, lr.STREAM_RESET, gid, K0, lr.RR, lr.PAR_NOM)
        assert np.array_equal(c[:6], sc[:6]) and np.array_equal(c[10:], sc[10:]) and np.array_equal(t, st) and np.array_equal(p, par)
        assert np.abs(c[6:10] - sc[6:10]).max() <= lr.QUAT_TOL and np.abs(e).max() <= 0.2
        # the float32 Euler angles are exactly what euler2quat received: the oracle's own transform gives the same quaternion
        np.testing.assert_allclose(o64.euler2quat(e.astype(np.float64)), c[6:10], rtol=0, atol=1e-15)
        for hover in (False, True):
            ref, exact = lr.ctor_ref(o64, lr.SEED, gid, hover)
            got = o64.ctor_init(lr.SEED, gid, 3 if hover else 2)
            assert np.array_equal(ref[exact], got[exact])
            assert np.abs(ref - got).max() <= lr.QUAT_TOL
            assert exact.sum() == (9 if hover else 26)
    assert GID0 < 2 ** 32 < GID0 + 41 and K0 < 2 ** 32 < 2 * K0 + 1


def test_inputs_are_what_the_cases_need():
    for n in lr.N_ENVS:
        masks = {k: lr.make_mask(k, n) for k in lr.MASKS}
        assert masks["null"] is None and masks["all"].all() and not masks["none"].any()
        assert masks["last"].sum() == 1 and masks["last"][-1]
        first = int(np.argmax(masks["first_of_last_tile"]))
        assert masks["first_of_last_tile"].sum() == 1 and first % 64 == 0 and n - 64 <= first < n
        if n >= 3:
            assert set(np.unique(masks["bytes_2_255"])) == {0, 2, 255}
    w = lr.raw_words((257, 13), 5).view(np.uint32).reshape(-1)
    for pattern in (0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000):
        assert (w == pattern).any()
    rec = lr.busy_rec(257, 3)
    assert np.abs(np.linalg.norm(rec[:, REC_QD:REC_QD + 4], axis=1) - 1).max() < 1e-6 and (np.abs(rec[:, REC_QD + 1:REC_QD + 4]) > 0).all()
    assert len(lr.field_subsets()) == 14
    lr.distinct_rec(257, 1); lr.distinct_par(257)
    assert lr.QUAT_TOL <= lr.QUAT_CEILING < 1.02e-6


# ---------------------------------------------------------------------------------------------------- float32 within the bounds
SOURCES_CPU = ("nominal", "rocrand1", "rocrand2", "stored", "hover")


@pytest.mark.parametrize("n", CPU_N)
@pytest.mark.parametrize("source", SOURCES_CPU)
def test_float32_oracle_passes_check_reset(source, n):
    """libm float32 (Oracle("f32"): cosf / sinf quaternion, float32 observation) is inside every bound at every env, for every
    mask of the GPU rows"""
    rr = lr.RR
    b = _before(n, source)
    worst = {"quat": 0.0, "obs": 0.0, "ls": 0.0}
    for mask_kind in lr.MASKS:
        mask = lr.make_mask(mask_kind, n)
        ref = lr.reset_ref(b["rec"], b["par"], mask, source, **_args(source, n, rr))
        dev = lr.reset_ref(b["rec"], b["par"], mask, source, quat="f32", **_args(source, n, rr))
        rec, par, obs = lr.as_device(dev)
        r = lr.check_reset(b, dict(rec=rec, par=par, ctr=K0), obs, mask, ref)
        lr.check_reset(b, dict(rec=rec, par=par, ctr=K0), None, mask, ref)
        worst = {k: max(worst[k], r[k]) for k in worst}
    print("lifecycle ratio float32-oracle %s n=%d %s" % (source, n, worst))
    if source.startswith("rocrand"):
        assert worst["quat"] > 0.05                                   # the bound is within a small factor of what float32 does


def test_float32_oracle_over_the_whole_half_angle_domain():
    """Euler half-range pi/2 (the widest qs_create admits): libm float32 keeps the reset quaternion within QUAT_TOL at every env;
    the observation is not asked for -- near roll = pi/2 its Euler angles are singular and the float32 oracle misses OBS_TOL by
    orders of magnitude, which is why the GPU row passes obs_out = NULL"""
    n = 1000
    b = _before(n, "rocrand1")
    ref = lr.reset_ref(b["rec"], b["par"], None, "rocrand1", **_args("rocrand1", n, lr.RR_WIDE))
    dev = lr.reset_ref(b["rec"], b["par"], None, "rocrand1", quat="f32", **_args("rocrand1", n, lr.RR_WIDE))
    rec, par, obs = lr.as_device(dev)
    r = lr.check_reset(b, dict(rec=rec, par=par, ctr=K0), None, None, ref)
    print("lifecycle ratio float32-oracle Euler half-range pi/2 %s" % r)
    assert 0.05 < r["quat"] <= 1.0
    with pytest.raises(AssertionError):
        lr.check_reset(b, dict(rec=rec, par=par, ctr=K0), obs, None, ref)


# ---------------------------------------------------------------------------------------------------- wrong resets
def _swap_halves(rec, par, obs, b, ref, mask):
    i = int(np.nonzero(ref["masked"])[0][-1])
    w = rec.view(np.uint32)
    w[i, 1] = (w[i, 1] >> 16) | ((w[i, 1] & 0xFFFF) << 16)


def _mutants():
    """name -> (altered arguments of reset_ref, or None; edit of (rec, par, obs) in place, or None)"""
    def clears_qdes(rec, par, obs, b, ref, mask):
        rec[ref["masked"], REC_QD:REC_QD + 4] = (1, 0, 0, 0)

    def leaves_target_u_prev(rec, par, obs, b, ref, mask):
        rec[ref["masked"], REC_UC + 4:REC_UC + 8] = b["rec"][ref["masked"], REC_UC + 4:REC_UC + 8]

    def leaves_last_shaping(rec, par, obs, b, ref, mask):
        rec[ref["masked"], REC_LS] = b["rec"][ref["masked"], REC_LS]

    def params_for_unmasked(rec, par, obs, b, ref, mask):
        i = int(np.nonzero(~ref["masked"])[0][-1])
        par[i] = np.asarray(lr.PAR_NOM, f32) * f32(1.01)

    def writes_unmasked_obs(rec, par, obs, b, ref, mask):
        i = int(np.nonzero(~ref["masked"])[0][0])
        obs[i] = obs[ref["masked"]][0]

    return {
        "clears_qdes": (None, clears_qdes),
        "leaves_target_half_of_u_prev": (None, leaves_target_u_prev),
        "leaves_last_shaping": (None, leaves_last_shaping),
        "draws_from_autoreset_stream": (dict(stream=lr.STREAM_AUTORESET), None),
        "draws_at_ctr_plus_1": (dict(ctr=K0 + 1), None),
        "forgets_env_id_offset": (dict(gid0=0), None),
        "stores_params_with_randomise_1": (dict(source="rocrand2"), None),
        "stores_params_for_unmasked_env": (None, params_for_unmasked),
        "honours_only_mask_1": (dict(mask="ones"), None),
        "swaps_16_bit_halves_of_a_word": (None, _swap_halves),
        "writes_unmasked_obs_row": (None, writes_unmasked_obs),
        "keys_every_tile_by_tile_0": (dict(ctr=K0), None),
    }


@pytest.mark.parametrize("mutant", sorted(_mutants()))
def test_wrong_resets_are_rejected(mutant):
    """each mutant is the reference's own output with one small edit; the unedited output passes first"""
    n = 257
    alter, edit = _mutants()[mutant]
    source = "rocrand1" if mutant == "stores_params_with_randomise_1" else "rocrand2"
    mask = lr.make_mask("bytes_2_255", n)
    b = _before(n, source)
    args = _args(source, n)
    if mutant == "keys_every_tile_by_tile_0":             # a handle whose tiles have stepped unevenly: the reference keys per tile
        args["ctr"] = lr.tile_counters([K0, K0, K0 + 3, K0 + 1, K0 + 3], n)
        b["ctr"] = [K0, K0, K0 + 3, K0 + 1, K0 + 3]
    ref = lr.reset_ref(b["rec"], b["par"], mask, source, **args)
    rec, par, obs = lr.as_device(ref)
    after = dict(rec=rec, par=par, ctr=b["ctr"])
    lr.check_reset(b, after, obs, mask, ref)                   # unedited: passes
    if alter:
        a2 = dict(args); a2.update(alter)
        src2 = a2.pop("source", source)
        mask2 = (mask == 1).astype(np.uint8) if a2.pop("mask", None) == "ones" else mask
        wrong = lr.reset_ref(b["rec"], b["par"], mask2, src2, **a2)
        rec, par, obs = lr.as_device(wrong)
    else:
        edit(rec, par, obs, b, ref, mask)
    with pytest.raises(AssertionError):
        lr.check_reset(b, dict(rec=rec, par=par, ctr=b["ctr"]), obs, mask, ref)


def test_a_changed_step_counter_is_rejected():
    n = 65
    b = _before(n, "nominal")
    ref = lr.reset_ref(b["rec"], b["par"], None, "nominal")
    rec, par, obs = lr.as_device(ref)
    lr.check_reset(b, dict(rec=rec, par=par, ctr=K0), obs, None, ref)
    with pytest.raises(AssertionError):
        lr.check_reset(b, dict(rec=rec, par=par, ctr=K0 + 1), obs, None, ref)


def test_hover_reset_that_writes_the_whole_record_is_rejected():
    n = 65
    b = _before(n, "hover")
    init = lr.stored_init(n, 8, hover=True)[0]
    ref = lr.reset_ref(b["rec"], b["par"], None, "hover", init=init)
    rec, par, obs = lr.as_device(ref)
    lr.check_reset(b, dict(rec=rec, par=par, ctr=b["ctr"]), obs, None, ref)
    rec[:, 39] = 0
    with pytest.raises(AssertionError):
        lr.check_reset(b, dict(rec=rec, par=par, ctr=b["ctr"]), obs, None, ref)


# ---------------------------------------------------------------------------------------------------- the matrix and the census
@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return kernel_notes.kernel_notes(kernel_notes.code_object(tmp_path_factory.mktemp("isa_lifecycle")))


def test_anon_instantiations_on_known_symbols():
    syms = ["_ZN12_GLOBAL__N_17k_resetENS_8StepArgsEPKhi", "_ZN12_GLOBAL__N_110k_state_ioILb0EEEvPflNS_7StateIOE",
            "_ZN12_GLOBAL__N_110k_state_ioILb1EEEvPflNS_7StateIOE", "_ZN12_GLOBAL__N_18k_par_ioILb1EEEvPflS1_S1_",
            "_ZN12_GLOBAL__N_111k_reset_allENS_8StepArgsE", "_ZN12_GLOBAL__N_15k_envILi0ELb1ELi2EEEvNS_8StepArgsE",
            "_ZN2qs7k_resetENS_8StepArgsE", "_ZN12_GLOBAL__N_113k_nominal_obsEPf"]
    got = kernel_notes.anon_instantiations(syms, ("k_reset", "k_state_io", "k_par_io", "k_nominal_obs", "k_env"))
    assert got == {("k_reset",), ("k_state_io", 0), ("k_state_io", 1), ("k_par_io", 1), ("k_nominal_obs",)}
    assert kernel_notes.base_names(syms + ["_Z6k_flatPfl", "plain_c_kernel"]) == {
        "k_reset", "k_state_io", "k_par_io", "k_reset_all", "k_env", "k_nominal_obs", "k_flat", "plain_c_kernel"}


def test_rows_are_exactly_the_instantiations(notes):
    keys = [r["key"] for r in lifecycle_matrix.ROWS]
    assert len(keys) == len(set(keys)) == 12, "duplicate rows"
    got = kernel_notes.anon_instantiations(notes, lifecycle_matrix.KERNELS)
    assert {k[0] for k in got} == set(lifecycle_matrix.KERNELS)
    assert set(keys) == got, "rows without an instantiation: %s; instantiations without a row: %s" % (
        sorted(set(keys) - got, key=str), sorted(got - set(keys), key=str))


def test_kernel_list_is_every_plain_kernel_of_the_header():
    """a thirteenth plain or <bool> kernel added to step_kernels.hpp has to be added to KERNELS (and then needs a row)"""
    import re
    src = open(os.path.join(ROOT, "quadsim_amd", "csrc", "step_kernels.hpp")).read()
    tail = src[src.index("void k_ctor_init") - 200:]
    found = set(re.findall(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", tail))
    assert found == set(lifecycle_matrix.KERNELS), found ^ set(lifecycle_matrix.KERNELS)


def _collected(files):
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + sorted(files), cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return set(out.stdout.split())


def test_rows_name_existing_gpu_tests():
    ids = _collected({r["test"].split("::")[0] for r in lifecycle_matrix.ROWS})
    missing = [r["test"] for r in lifecycle_matrix.ROWS if r["test"] not in ids]
    assert not missing, missing


def test_census_names_every_kernel_of_the_code_object(notes):
    """every kernel base name of the built code object has an entry, every entry has a kernel, and every entry names a matrix
    with a row for that kernel or a test id that exists"""
    built = kernel_notes.base_names(notes)
    census = lifecycle_matrix.CENSUS
    assert built == set(census), "kernels nobody claims: %s; names without a kernel: %s" % (
        sorted(built - set(census)), sorted(set(census) - built))
    direct = {}
    for kernel, where in census.items():
        if where.endswith("_matrix"):
            rows = importlib.import_module(where).ROWS
            tests = [r["test"] for r in rows if r["key"][0] == kernel]
            assert tests, "%s has no row in tests/%s.py" % (kernel, where)
            direct[kernel] = tests[0]
        else:
            direct[kernel] = where
    ids = _collected({t.split("::")[0] for t in direct.values()})
    bare = {i.split("[")[0] for i in ids}
    missing = {k: t for k, t in direct.items() if t not in ids and t not in bare}
    assert not missing, missing
