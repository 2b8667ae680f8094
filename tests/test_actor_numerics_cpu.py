"""The float64 reference and the scale-aware error bound of tests/actor_numerics.py, without a GPU: the reference agrees with the
oracle's restatements, the weight sets are what the GPU numerics tests rely on (mostly unclipped, dead ReLUs, cancellation),
numpy float32 and a numpy emulation of the split-bf16 network read from the packed weight images pass the bound -- and the
packing / kernel mistakes that matter fail it: a dropped cross term in any one layer, the lo image of one W2 fragment zeroed,
two k-slots of one fragment swapped, b3 read from the wrong padded slot."""
import numpy as np
import pytest

import actor_numerics as an

MUTANT_SETS = ("v0", "towers", "dead")          # (d) cancels first-layer errors by construction: bound checked, mutants not


@pytest.fixture(scope="module")
def sets():
    return {k: an.weight_set(k) for k in an.WEIGHT_SETS}


@pytest.fixture(scope="module")
def obs_sets():
    return {"box": an.box_obs(4097, 1), "edge_v0": an.edge_obs(4097, 2, an.RMAX["docking-v0"]),
            "edge_v1": an.edge_obs(4097, 3, an.RMAX["docking-v1"])}


def _cpu_policies(W):
    import quadsim_amd as qa
    return qa.MlpPolicy(W, device="cpu"), qa.ActorCriticPolicy(W, device="cpu")


def _blobs(W):
    from quadsim_amd.policy import pack_fast_weights
    from quadsim_amd.runner import pack_fast_actor_critic
    mlp, ac = _cpu_policies(W)
    return pack_fast_weights(mlp).copy(), pack_fast_actor_critic(ac).copy(), ac.towers


# ---------------------------------------------------------------------------------------------------- reference and bound
def test_net64_matches_the_oracle_restatements():
    from oracle.pyoracle import actor_critic_step
    obs = an.box_obs(500, 9)
    W = an.weights_v0()
    _, value, _, _, mean = actor_critic_step(W, obs, np.zeros((500, 4)))
    m, v = an.net64(W, obs)
    np.testing.assert_array_equal(m, mean)
    np.testing.assert_array_equal(v, value)
    W = an.weights_towers()
    f = lambda k: np.asarray(W[k], np.float64)                            # noqa: E731
    x = obs.astype(np.float64)
    hv = np.maximum(np.maximum(x @ f("wv0") + f("bv0"), 0.0) @ f("wv1") + f("bv1"), 0.0)
    hp = np.maximum(np.maximum(x @ f("w0") + f("b0"), 0.0) @ f("w1") + f("b1"), 0.0)
    m, v = an.net64(W, obs)
    np.testing.assert_array_equal(m, hp @ f("w2") + f("b2"))
    np.testing.assert_array_equal(v, (hv @ f("wv2") + f("bv2"))[:, 0])


def test_err_scale_is_the_layerwise_recursion():
    """E of a one-hidden-layer chain written out by hand, and E >= |output| - |bias| terms (every summand is in E)"""
    rng = np.random.default_rng(0)
    W = {"w0": rng.standard_normal((12, 128)), "b0": rng.standard_normal(128), "w1": rng.standard_normal((128, 128)),
         "b1": rng.standard_normal(128), "w2": rng.standard_normal((128, 4)), "b2": rng.standard_normal(4)}
    x = an.box_obs(50, 1).astype(np.float64)
    h1 = np.maximum(x @ W["w0"] + W["b0"], 0)
    h2 = np.maximum(h1 @ W["w1"] + W["b1"], 0)
    E1 = np.abs(x) @ np.abs(W["w0"]) + np.abs(W["b0"])
    E2 = E1 @ np.abs(W["w1"]) + h1 @ np.abs(W["w1"]) + np.abs(W["b1"])
    E3 = E2 @ np.abs(W["w2"]) + h2 @ np.abs(W["w2"]) + np.abs(W["b2"])
    np.testing.assert_allclose(an.err_scale(W, x)[0], E3, rtol=1e-12)
    m = an.net64(W, x)[0]
    assert (np.abs(m) <= E3).all()


def test_weight_sets_are_what_the_numerics_tests_rely_on(sets, obs_sets):
    cal = an.calibration_obs()
    for name, W in sets.items():
        m = an.net64(W, cal)[0]
        assert np.mean(np.abs(m) < 0.95) >= 0.9, name                     # mostly unclipped on the calibration set
        assert np.mean(np.abs(an.net64(W, obs_sets["box"])[0]) < 0.95) >= 0.9, name
        assert all(np.isfinite(np.asarray(v)).all() for v in W.values())
    x = obs_sets["box"].astype(np.float64)
    Wd = sets["dead"]
    dead = (x @ np.asarray(Wd["w0"], np.float64) + np.asarray(Wd["b0"], np.float64)) <= 0
    assert dead.mean() > 0.4                                              # (c): many first-layer ReLUs off
    Wc = sets["cancel"]
    m, v = an.net64(Wc, x)
    Em, Ev = an.err_scale(Wc, x)
    assert np.median(np.abs(m) / Em) < 1e-3 and np.median(np.abs(v) / Ev) < 1e-3    # (d): |output| << E
    assert sets["towers"].get("wv0") is not None and "wv0" not in sets["v0"]


# ---------------------------------------------------------------------------------------------------- the bound holds
@pytest.mark.parametrize("name", an.WEIGHT_SETS)
def test_float32_evaluation_within_bound(sets, obs_sets, name):
    W = sets[name]
    for oname, obs in obs_sets.items():
        m64, v64 = an.net64(W, obs)
        Em, Ev = an.err_scale(W, obs)
        m, v = an.emulate_f32(W, obs)
        an.check_unclipped(m, m64, Em, "f32", "%s/%s mean" % (name, oname))
        an.check_unclipped(v, v64, Ev, "f32", "%s/%s value" % (name, oname))


@pytest.mark.parametrize("name", an.WEIGHT_SETS)
def test_split_bf16_emulation_of_packed_images_within_bound(sets, obs_sets, name):
    """the split-bf16 network as the kernels read the bytes of pack_fast_weights / pack_fast_actor_critic: every weight through
    the fragment decoder, three terms per k-step, one f32 rounding per MFMA"""
    W = sets[name]
    actor, ac, towers = _blobs(W)
    for oname, obs in obs_sets.items():
        m64, v64 = an.net64(W, obs)
        Em, Ev = an.err_scale(W, obs)
        r = an.check_unclipped(an.emulate_actor_blob(actor, obs), m64, Em, "bf16x3", "%s/%s actor" % (name, oname))
        assert r < an.KAPPA["bf16x3"] / 2.5                                # a correct emulation stays far inside kappa16
        m, v = an.emulate_actor_critic_blob(ac, obs, towers)
        an.check_unclipped(m, m64, Em, "bf16x3", "%s/%s actor-critic mean" % (name, oname))
        an.check_unclipped(v, v64, Ev, "bf16x3", "%s/%s actor-critic value" % (name, oname))


def test_kappa16_stays_below_one():
    assert an.KAPPA["bf16x3"] < 1.0 and an.KAPPA["f32"] <= 8.0


# ---------------------------------------------------------------------------------------------------- the images
@pytest.mark.parametrize("layout", ["v0", "towers"])
def test_hi_lo_images_hold_every_weight(layout):
    """every weight of both images, both layouts: hi is the RNE bf16 of the weight, hi + lo within 2^-17 relative, float32
    parts and biases exact, padding zero (the decoders assert coverage and padding)"""
    W = an.weights_v0() if layout == "v0" else an.weights_towers()
    actor, ac, towers = _blobs(W)
    assert towers == (layout == "towers")
    f = lambda k: np.asarray(W[k], np.float32)                            # noqa: E731

    def same(hi, lo, w):
        w = np.asarray(w, np.float32)
        assert np.array_equal(hi, an.bf16_round(w))
        err = np.abs(hi.astype(np.float64) + lo - w)
        assert (err <= np.abs(w.astype(np.float64)) * 2.0 ** -17).all(), float(err.max())

    d = an.decode_actor_blob(actor)
    for l, k in enumerate(("w0", "w1", "w2")):
        same(d["hi"][l], d["lo"][l], f(k).T)
    np.testing.assert_array_equal(d["b"][0], f("b0"))
    np.testing.assert_array_equal(d["b"][1], f("b1"))
    np.testing.assert_array_equal(d["b"][2], np.concatenate([f("b2"), np.zeros(12, np.float32)]))
    d = an.decode_actor_critic_blob(ac, towers)
    np.testing.assert_array_equal(d["w1"], f("w0").T)
    np.testing.assert_array_equal(d["b1"], f("b0"))
    for br, (k2, k3, b2, b3) in (("pi", ("w1", "w2", "b1", "b2")), ("vf", ("wv1", "wv2", "bv1", "bv2"))):
        same(d[br]["hi"][0], d[br]["lo"][0], f(k2).T)
        same(d[br]["hi"][1], d[br]["lo"][1], f(k3).T)
        np.testing.assert_array_equal(d[br]["b"][0], f(b2))
        np.testing.assert_array_equal(d[br]["b"][1], f(b3))
    np.testing.assert_array_equal(d["b3pad"][5:], 0)
    if towers:
        np.testing.assert_array_equal(d["wv1"], f("wv0").T)
        np.testing.assert_array_equal(d["bv1"], f("bv0"))


# ---------------------------------------------------------------------------------------------------- mutants fail the bound
# byte offsets of the images (csrc/mlp.hpp)
ACTOR_A2, ACTOR_A1, ACTOR_A3, ACTOR_B3 = 0, 65536, 81920, 91136
AC_A2PI, AC_A2VF, AC_B3 = 0, 65536, 141824


def _frag(blob, off, shape):
    """writable bf16 view [.., lane, 8] of an image part"""
    n = int(np.prod(shape)) * 2
    return blob[off:off + n].view(np.uint16).reshape(shape)


def _zero_lo(blob, a2):
    b = blob.copy()
    _frag(b, a2 + 32768, (8, 4, 64, 8))[3, 2] = 0                        # lo image of tile 3, k-step 2
    return b


def _swap_j(blob, off, shape, idx, j0=1, j1=6):
    b = blob.copy()
    for part in (0, int(np.prod(shape)) * 2):                             # a packing slip moves both hi and lo
        fr = _frag(b, off + part, shape)[idx]
        fr[..., [j0, j1]] = fr[..., [j1, j0]]
    return b


def _b3_shift(blob, off):
    b = blob.copy()
    b3 = b[off:off + 64].view(np.float32)
    b3[:] = np.concatenate([b3[1:], np.zeros(1, np.float32)])             # slot i reads slot i + 1
    return b


def _fails(y, ref, E):
    return float(an.ratio(y - ref, E, "bf16x3").max()) > an.KAPPA["bf16x3"]


@pytest.mark.parametrize("name", MUTANT_SETS)
def test_actor_image_mutants_fail_the_bound(sets, obs_sets, name):
    W = sets[name]
    actor, _, _ = _blobs(W)
    obs = np.concatenate([obs_sets["box"], obs_sets["edge_v0"]])
    m64 = an.net64(W, obs)[0]
    Em = an.err_scale(W, obs)[0]
    assert not _fails(an.emulate_actor_blob(actor, obs), m64, Em)
    mutants = {("drop", l, t): an.emulate_actor_blob(actor, obs, drop=(l, t)) for l in range(3) for t in an.TERMS[:2]}
    mutants["zero W2 lo fragment"] = an.emulate_actor_blob(_zero_lo(actor, ACTOR_A2), obs)
    mutants["swap j in W2 fragment"] = an.emulate_actor_blob(_swap_j(actor, ACTOR_A2, (8, 4, 64, 8), (5, 1)), obs)
    mutants["swap j in W1 fragment"] = an.emulate_actor_blob(_swap_j(actor, ACTOR_A1, (8, 64, 8), 2, 0, 3), obs)
    mutants["swap j in W3 fragment"] = an.emulate_actor_blob(_swap_j(actor, ACTOR_A3, (4, 64, 8), 1), obs)
    mutants["b3 slot"] = an.emulate_actor_blob(_b3_shift(actor, ACTOR_B3), obs)
    passed = [k for k, m in mutants.items() if not _fails(m, m64, Em)]
    assert not passed, "mutants inside the bound: %s" % passed


@pytest.mark.parametrize("name", MUTANT_SETS)
def test_actor_critic_image_mutants_fail_the_bound(sets, obs_sets, name):
    W = sets[name]
    _, ac, towers = _blobs(W)
    obs = np.concatenate([obs_sets["box"], obs_sets["edge_v0"]])
    m64, v64 = an.net64(W, obs)
    Em, Ev = an.err_scale(W, obs)
    fails = lambda mv: _fails(mv[0], m64, Em) or _fails(mv[1], v64, Ev)  # noqa: E731
    assert not fails(an.emulate_actor_critic_blob(ac, obs, towers))
    mutants = {("drop", br, l, t): an.emulate_actor_critic_blob(ac, obs, towers, drop=(br, l, t))
               for br in ("pi", "vf") for l in (1, 2) for t in an.TERMS[:2]}
    mutants["zero pi W2 lo fragment"] = an.emulate_actor_critic_blob(_zero_lo(ac, AC_A2PI), obs, towers)
    mutants["zero vf W2 lo fragment"] = an.emulate_actor_critic_blob(_zero_lo(ac, AC_A2VF), obs, towers)
    mutants["swap j in pi W2 fragment"] = an.emulate_actor_critic_blob(_swap_j(ac, AC_A2PI, (8, 4, 64, 8), (5, 1)), obs, towers)
    mutants["swap j in vf W2 fragment"] = an.emulate_actor_critic_blob(_swap_j(ac, AC_A2VF, (8, 4, 64, 8), (2, 3)), obs, towers)
    mutants["b3 slot"] = an.emulate_actor_critic_blob(_b3_shift(ac, AC_B3), obs, towers)
    passed = [k for k, mv in mutants.items() if not fails(mv)]
    assert not passed, "mutants inside the bound: %s" % passed
