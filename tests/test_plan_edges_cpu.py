"""-m "not gpu": the edge cases of tests/test_gpu_plan_edges.py are judged before the GPU is, on the references alone.
tests/plan_matrix.py has exactly one row per compiled instantiation of the seven planner kernels and names collected tests; at
every step counter of plan_cases.SHOOT_K / MPPI_K the reference candidates differ from those of a key with a field cut to 32
bits exactly where that field is past 32 bits, and every such fault is seen by some case; the global ids on the two sides of
2^32 draw differently from their low words; at the long horizons a planner that stopped after one trip of a loop strided over h
is outside what the GPU test asserts, and no candidate of the float64 oracle passes a done threshold within the per-step bound;
qs_create refuses a global id past 48 bits before it looks for a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_notes
import mppi_ref
import plan_cases as pc
import plan_matrix
import shooting_ref
from oracle.pyoracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = (1 << 32) - 1
SUB = lambda gid: (shooting_ref.STREAM_PLAN << 48) | gid      # noqa: E731


# ---------------------------------------------------------------- the matrix
@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return kernel_notes.kernel_notes(kernel_notes.code_object(tmp_path_factory.mktemp("isa_plan_edges")))


def test_rows_are_exactly_the_instantiations(notes):
    """the <int INTEG, bool PARAMS> kernels through kernel_notes.instantiations, the plain ones through anon_instantiations
    (which sees plain and <bool> kernels only); the names are those of the *_instantiations_and_resources tests"""
    keys = [r["key"] for r in plan_matrix.ROWS]
    assert len(keys) == len(set(keys)) == 19, "duplicate rows"
    got = kernel_notes.instantiations(notes, plan_matrix.TEMPLATED) | kernel_notes.anon_instantiations(notes, plan_matrix.PLAIN)
    assert {k[0] for k in got} == set(plan_matrix.KERNELS)
    assert set(keys) == got, "rows without an instantiation: %s; instantiations without a row: %s" % (
        sorted(set(keys) - got, key=str), sorted(got - set(keys), key=str))
    assert not kernel_notes.anon_instantiations(notes, plan_matrix.TEMPLATED)       # none of the four has a plain variant
    for r in plan_matrix.ROWS:                                                       # the handle reaches the instantiation
        if len(r["key"]) == 3:
            assert r["key"][1:] == (int(r["integ"] == "rk4"), int(r["params"])), r


def test_rows_name_collected_gpu_tests():
    files = sorted({r["test"].split("::")[0] for r in plan_matrix.ROWS})
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ids = set(out.stdout.split())
    missing = [r["test"] for r in plan_matrix.ROWS if r["test"] not in ids]
    assert not missing, missing


def test_the_edge_handle_is_where_the_issue_puts_it():
    lo, hi = pc.EDGE_OFFSETS
    assert lo < 1 << 32 < lo + pc.EDGE_N - 1 and hi + pc.EDGE_N == 1 << 48 and pc.EDGE_SEED >> 32 and pc.EDGE_SEED & M32
    assert pc.EDGE_N % 6 == 0                                  # two envs of each provoked state
    assert max(pc.SHOOT_K) == (1 << 36) - 1 and max(pc.MPPI_K) == (1 << mppi_ref.K_BITS) - 1
    for cases, ks in ((pc.key_cases(pc.SHOOT_K), pc.SHOOT_K), (pc.key_cases(pc.MPPI_K), pc.MPPI_K)):
        assert len({c[0] for c in cases}) == len(cases) == 2 * len(ks)
        assert {c[1:4] for c in cases} == set(pc.EDGE_COMBOS)
        assert {(c[4], c[5]) for c in cases} == {(o, k) for o in pc.EDGE_OFFSETS for k in ks}
    assert {(int(g == "rk4"), int(p)) for _, g, p in pc.EDGE_COMBOS} == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---------------------------------------------------------------- each key case can see its fault
def _shoot_blocks(k, paths, horizon):
    c = np.arange(paths, dtype=np.uint64)[:, None]
    h = np.arange(horizon, dtype=np.uint64)[None, :]
    return (np.uint64(k) << np.uint64(26)) | (c << np.uint64(10)) | h


def _actions_of(seed, gid, blocks):
    """shooting_ref.actions_fast's conversion on the words of `blocks`"""
    w = shooting_ref.philox_np(seed, SUB(gid), blocks)
    u = ((w.astype(np.float32).astype(np.float64) + 1.0) * 2.0 ** -32).astype(np.float32)
    return (2.0 * u.astype(np.float64) - 1.0).astype(np.float32)


# what a kernel with a field cut to 32 bits would key by -> from which k on the cut changes the key
SHOOT_FAULTS = {
    "k_32": (lambda k, b: _shoot_blocks(k & M32, *b), 1 << 32),
    "block_32": (lambda k, b: _shoot_blocks(k, *b) & np.uint64(M32), 64),                       # (k << 26) >= 2^32
    "offset_32": (lambda k, b: _shoot_blocks(k, *b) & np.uint64((1 << 30) - 1), 16),            # 4 * (k << 26) >= 2^32
}


def test_every_shooting_key_case_sees_the_cuts_it_is_past():
    shape = (pc.EDGE_PATHS, pc.EDGE_HORIZON)
    seen = {name: 0 for name in SHOOT_FAULTS}
    for offset in pc.EDGE_OFFSETS:
        for k in pc.SHOOT_K:
            for gid in (offset, offset + pc.EDGE_N - 1):
                ref = shooting_ref.actions_fast(pc.EDGE_SEED, gid, k, *shape)
                assert pc.same_bits(ref, _actions_of(pc.EDGE_SEED, gid, _shoot_blocks(k, *shape)))       # the helper is the reference
                for name, (cut, first_k) in SHOOT_FAULTS.items():
                    differs = not pc.same_bits(ref, _actions_of(pc.EDGE_SEED, gid, cut(k, shape)))
                    assert differs == (k >= first_k), (name, k, gid)
                    seen[name] += differs
    assert all(seen.values()), seen
    # the pairs of the list sit on the two sides of each crossing
    for name, (_, first_k) in SHOOT_FAULTS.items():
        assert first_k in pc.SHOOT_K and first_k - 1 in pc.SHOOT_K, name
    # and swapped counter words, or a dropped carry of 4 * block into rocRAND's upper word, at the largest k
    k, gid = pc.SHOOT_K[-1], pc.EDGE_OFFSETS[0]
    blocks = _shoot_blocks(k, *shape)
    ref = shooting_ref.actions_fast(pc.EDGE_SEED, gid, k, *shape)
    swapped = (blocks >> np.uint64(32)) | ((blocks & np.uint64(M32)) << np.uint64(32))
    assert not pc.same_bits(ref, _actions_of(pc.EDGE_SEED, gid, swapped))
    # the reference itself at this key is the C oracle's generator
    w = shooting_ref.philox_np(pc.EDGE_SEED, SUB(gid), blocks[-1:, -1])[0]
    assert np.array_equal(w, Oracle("f64").philox(pc.EDGE_SEED, SUB(gid), int(blocks[-1, -1])))


def _mppi_blocks(k, it, paths, horizon, k_shift_mask=(1 << 64) - 1):
    c = np.arange(paths, dtype=np.uint64)[:, None]
    h = np.arange(horizon, dtype=np.uint64)[None, :]
    return np.uint64((1 << 63) | ((k << 30) & k_shift_mask) | (it << 26)) | (c << np.uint64(10)) | h


MPPI_FAULTS = {
    "k_32": (lambda k, it, b: _mppi_blocks(k & M32, it, *b), lambda k, it: k >= 1 << 32),
    "shift_32": (lambda k, it, b: _mppi_blocks(k, it, *b, k_shift_mask=M32), lambda k, it: k >= 4),        # (unsigned)k << 30
    "block_32": (lambda k, it, b: _mppi_blocks(k, it, *b) & np.uint64(M32), lambda k, it: True),          # bit 63 is always set
    "it_0": (lambda k, it, b: _mppi_blocks(k, 0, *b), lambda k, it: it > 0),
}


def test_every_mppi_key_case_sees_the_cuts_it_is_past():
    """MPPI sets the Philox counter itself, so there is no rocRAND offset to cut; its 32-bit faults are a truncated k, a shift
    k << 30 done in 32 bits, a dropped upper counter word, and an iteration that does not reach the key"""
    shape = (pc.EDGE_PATHS, pc.EDGE_HORIZON)
    seen = {name: 0 for name in MPPI_FAULTS}
    for offset in pc.EDGE_OFFSETS:
        for k in pc.MPPI_K:
            for it in (0, 1, 2, 15):
                gid = offset + pc.EDGE_N - 1
                ref = mppi_ref.words(pc.EDGE_SEED, gid, k, it, *shape)
                assert np.array_equal(ref, shooting_ref.philox_np(pc.EDGE_SEED, SUB(gid), _mppi_blocks(k, it, *shape)))
                for name, (cut, visible) in MPPI_FAULTS.items():
                    differs = not np.array_equal(ref, shooting_ref.philox_np(pc.EDGE_SEED, SUB(gid), cut(k, it, shape)))
                    assert differs == visible(k, it), (name, k, it)
                    seen[name] += differs
                # different words are different normals, beyond what the GPU test allows
                z = mppi_ref.normals(pc.EDGE_SEED, gid, k, it, *shape)
                if it:
                    assert np.max(np.abs(z - mppi_ref.normals(pc.EDGE_SEED, gid, k, 0, *shape))) > 1.0
    assert all(seen.values()), seen
    assert 3 in pc.MPPI_K and 4 in pc.MPPI_K and (1 << 32) - 1 in pc.MPPI_K and 1 << 32 in pc.MPPI_K
    # the reference at the largest key is the C oracle's generator (blocks with bit 63 set)
    k, gid = pc.MPPI_K[-1], pc.EDGE_OFFSETS[1] + pc.EDGE_N - 1
    w = mppi_ref.words(pc.EDGE_SEED, gid, k, 15, *shape)[-1, -1]
    assert np.array_equal(w, Oracle("f64").philox(pc.EDGE_SEED, SUB(gid), mppi_ref.block_index(k, 15, shape[0] - 1, shape[1] - 1)))


def test_global_ids_past_32_bits_draw_differently_from_their_low_words():
    shape = (pc.EDGE_PATHS, pc.EDGE_HORIZON)
    past = 0
    for offset in pc.EDGE_OFFSETS:
        for g in range(pc.EDGE_N):
            gid = offset + g
            same_s = pc.same_bits(shooting_ref.actions_fast(pc.EDGE_SEED, gid, pc.SHOOT_K[-1], *shape),
                                  shooting_ref.actions_fast(pc.EDGE_SEED, gid & M32, pc.SHOOT_K[-1], *shape))
            same_m = np.array_equal(mppi_ref.words(pc.EDGE_SEED, gid, pc.MPPI_K[-1], 0, *shape),
                                    mppi_ref.words(pc.EDGE_SEED, gid & M32, pc.MPPI_K[-1], 0, *shape))
            assert same_s == same_m == (gid <= M32), gid
            past += gid > M32
    assert past == pc.EDGE_N - 6 + pc.EDGE_N                   # six envs of the first handle are below 2^32
    # a 64-bit seed: the upper key word matters
    assert not pc.same_bits(shooting_ref.actions_fast(pc.EDGE_SEED, 0, 2, *shape), shooting_ref.actions_fast(pc.EDGE_SEED & M32, 0, 2, *shape))


# ---------------------------------------------------------------- the long horizons
def _kind_integ(env_id, integ):
    return (1 if env_id == "docking-v2" else 0), (1 if integ == "rk4" else 0)


def _long_actions(paths, horizon):
    return np.stack([shooting_ref.actions_fast(pc.EDGE_SEED, pc.EDGE_OFFSETS[0] + g, pc.LONG_K, paths, horizon) for g in range(pc.EDGE_N)])


def _long_mppi(paths, horizon, shift):
    nominal, z = pc.long_mppi_inputs()
    U = nominal[:, :horizon][:, np.minimum(np.arange(horizon) + shift, horizon - 1)]
    return U, mppi_ref.candidates32(U, pc.LONG_SIGMA, z[:paths, :horizon])


def test_long_cases_take_more_than_one_trip():
    """a block is min(256, paths rounded up to a wave) threads: the loops over h += blockDim.x take two and four trips at paths 1
    and 64, the loops over h += 64 two to four at every case"""
    for cases in (pc.LONG_SHOOT, [c[:2] for c in pc.LONG_MPPI]):
        trips = [(-(-h // min(256, -(-p // 64) * 64)), -(-h // 64)) for p, h in cases]
        assert max(t[0] for t in trips) == max(h for _, h in cases) // 64 and min(t[1] for t in trips) >= 2, trips
    assert max(h for _, h in pc.LONG_SHOOT) == 256 and max(c[1] for c in pc.LONG_MPPI) == 128      # the admitted maxima
    assert any(c[2] for c in pc.LONG_MPPI if c[1] == 128)      # the shift runs through min(h + 1, horizon - 1) at horizon 128


@pytest.mark.parametrize("env_id,integ,params", pc.LONG_HANDLES)
def test_no_long_candidate_passes_a_threshold_within_the_step_bound(env_id, integ, params):
    """the condition under which a float32 and a float64 simulator decide every done alike: no candidate is left out of any
    comparison instead.  (64, 256) and (1, 65) are the first candidates and steps of (200, 256): a candidate's actions depend on
    neither `paths` nor `horizon`"""
    _, rec, par = pc.long_states(env_id, integ, params)
    kind, ig = _kind_integ(env_id, integ)
    paths, horizon = max(pc.LONG_SHOOT)
    assert all(p <= paths and h <= horizon for p, h in pc.LONG_SHOOT)
    assert pc.knife_edges(rec, par, _long_actions(paths, horizon), kind, ig) == 0
    if (env_id, integ, params) == pc.LONG_HANDLES[0]:
        for case in pc.LONG_MPPI:
            assert pc.knife_edges(rec, par, _long_mppi(*case)[1], kind, ig) == 0, case
    # the check does see an edge: the falling envs sit 0.03 m over the floor, and a bound of that size flags them
    old = pc.OBS_BOUND
    try:
        pc.OBS_BOUND = 0.05
        assert pc.knife_edges(rec, par, _long_actions(4, 3), kind, ig) > 0
    finally:
        pc.OBS_BOUND = old


@pytest.mark.parametrize("env_id,integ,params", pc.LONG_HANDLES)
def test_a_shooting_plan_that_stops_after_one_trip_is_seen(env_id, integ, params):
    """the winner's sequence is compared bit for bit, and past step 64 no element of it is the zero (or anything else) that an
    unwritten row holds; the roll-outs themselves pass step 64 on the docking-v2 handle (rmax 10 m), so that its scores hold the
    target rows of the second trip too"""
    _, rec, par = pc.long_states(env_id, integ, params)
    kind, ig = _kind_integ(env_id, integ)
    rows = np.arange(pc.EDGE_N)
    for paths, horizon in pc.LONG_SHOOT:
        acts = _long_actions(paths, horizon)
        s_rew, s_pos, _ = shooting_ref.plan_scores_both(rec, par, acts, kind=kind, dt=pc.DT, integ=ig)
        for S in (s_rew, s_pos):
            seq = acts[rows, shooting_ref.first_argmax(S)]
            assert np.all(seq[:, 64:] != 0.0) and seq[:, 64:].size
            assert len(np.unique(pc.bits(seq).reshape(-1, 4), axis=0)) == seq.size // 4      # nor is a row a copy of another
        if kind == 1 and horizon == 256:
            short, _, _ = shooting_ref.plan_scores_both(rec, par, acts[:, :, :64], kind=kind, dt=pc.DT, integ=ig)
            free = rows % 6 >= 3
            flies_on = float(np.mean(np.abs(s_rew - short)[free] > 2 * horizon * 1e-5))
            print("candidates of the free envs whose score past step 64 is beyond the bound: %.3f" % flies_on)
            assert flies_on > 0.9


@pytest.mark.parametrize("paths,horizon,shift", pc.LONG_MPPI)
def test_an_mppi_plan_that_stops_after_one_trip_is_seen(paths, horizon, shift):
    """steps h >= 64 of the new nominal left at zero, or of the old one (the update skipped there): both are outside the bound
    the GPU test asserts end to end, at every env and step; candidates built on a nominal that is zero from step 64 on are not
    the reference's bits"""
    env_id, integ, params = pc.LONG_HANDLES[0]
    _, rec, par = pc.long_states(env_id, integ, params)
    U, cands = _long_mppi(paths, horizon, shift)
    s_rew, s_pos, r = shooting_ref.plan_scores_both(rec, par, cands, kind=0, dt=pc.DT, integ=0)
    for S, ds, lam in ((s_rew, horizon * 1e-5, 0.02), (s_pos, horizon * 2 * r * 2e-5, 1.5)):
        while 4 * ds / lam + 2.0 ** -23 > 0.05:
            lam *= 2.0
        tol = 4 * ds / lam + 2.0 ** -23
        want = mppi_ref.update64(S, cands, lam, U)
        assert np.all(np.abs(want[:, 64:]) > tol) and want[:, 64:].size
        if paths > 1:                                          # one path: the nominal is its own update
            assert np.max(np.abs(want[:, 64:] - U[:, 64:])) > tol
    cut = U.copy()
    cut[:, 64:] = 0.0
    z = pc.long_mppi_inputs()[1][:paths, :horizon]
    assert not pc.same_bits(mppi_ref.candidates32(cut, pc.LONG_SIGMA, z)[:, :, 64:], cands[:, :, 64:])
    if shift:                                                  # the shift is visible, at the last step too
        nominal = pc.long_mppi_inputs()[0][:, :horizon]
        assert not pc.same_bits(U, nominal) and pc.same_bits(U[:, -1], nominal[:, -1]) and pc.same_bits(U[:, -2], nominal[:, -1])


# ---------------------------------------------------------------- the id space
def test_qs_create_refuses_a_global_id_past_48_bits_before_it_looks_for_a_device():
    from quadsim_amd import _lib
    lib = _lib.load()
    cfg = _lib.default_config()
    cfg.num_envs = 12
    for offset in ((1 << 48) - 11, 1 << 48, (1 << 64) - 1):
        cfg.env_id_offset = offset
        h = C.c_void_p()
        assert lib.qs_create(C.byref(cfg), C.byref(h)) == -1 and not h.value, offset
        assert "48 bits" in lib.qs_last_error().decode()
    cfg.env_id_offset = (1 << 48) - 12                         # accepted: what follows is the device's business
    h = C.c_void_p()
    rc = lib.qs_create(C.byref(cfg), C.byref(h))
    assert rc == 0 or "48 bits" not in lib.qs_last_error().decode()
    if rc == 0:
        lib.qs_destroy(h)
    import quadsim_amd
    for kw in (dict(env_id_offset=(1 << 48) - 11), dict(env_id_offset=1 << 48), dict(env_id_offset=-1), dict(env_id_offset=1 << 64)):
        with pytest.raises(ValueError, match="48 bits"):
            quadsim_amd.VecDockingEnv("docking-v0", num_envs=12, **kw)
    header = open(os.path.join(ROOT, "include", "quadsim.h")).read()
    assert "env_id_offset + num_envs > 2^48" in header
