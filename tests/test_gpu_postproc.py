"""-m gpu: the roll-out post-processing kernels of csrc/rollout_ops.hpp (GAE, GAE + flatten, swap_and_flatten, episode
accounting) against the float64 references and bounds of tests/postproc_ref.py, at the shapes where the code branches: the
64-step chunk seam of the two-pass scan, the switch to the serial scan at n = 16 384, the 16-step groups, the vector / scalar
stores of k_gae_flatten, ragged 32 x 32 tiles, blocks with idle waves.  Every call goes through the C ABI with each buffer a
view into a larger device tensor, 256 bytes of a sentinel pattern on each side: a store outside an output shows as a changed
sentinel byte, never as a fault.  No element is left out of a comparison.  One row per instantiation: tests/postproc_matrix.py."""
import ctypes as C

import numpy as np
import pytest

import postproc_ref as pr
from oracle.pyoracle import episode_stats_ref

pytestmark = pytest.mark.gpu

PAD = 256                      # bytes of sentinel on each side; a multiple of 16 keeps the 16-byte alignment of the vector paths
BAND = ((np.arange(PAD) * 37 + 11) % 251).astype(np.uint8)      # no constant fill or stride-of-two pattern reproduces it
QS_ERR_INVALID = -1


@pytest.fixture(scope="module")
def qa():
    import quadsim_amd
    return quadsim_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def env(qa):
    e = qa.VecDockingEnv("docking-v0", num_envs=64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lib(qa):
    return qa._lib.load()


class Guards:
    """device buffers between sentinel bands: put() an input, out() an output (its payload starts as sentinel bytes too, so an
    element the kernel skips cannot pass a comparison), check() that every band -- and every input -- is unchanged"""

    def __init__(self, torch, device):
        self.torch, self.device, self.items = torch, device, []

    def _make(self, shape, dtype, data):
        torch = self.torch
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        pattern = np.full(PAD + nbytes + PAD, 0xA5, np.uint8)
        pattern[:PAD] = BAND
        pattern[PAD + nbytes:] = BAND[::-1]
        if data is not None:
            pattern[PAD:PAD + nbytes] = np.ascontiguousarray(data, dtype).reshape(-1).view(np.uint8)
        raw = torch.as_tensor(pattern).to(self.device)
        t = raw[PAD:PAD + nbytes].view(getattr(torch, np.dtype(dtype).name)).view(tuple(shape))
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        self.items.append((raw, pattern, nbytes, data is not None))
        return t

    def put(self, data, dtype=None):
        data = np.asarray(data)
        return self._make(data.shape, dtype or data.dtype, data)

    def out(self, shape, dtype=np.float32):
        return self._make(shape, dtype, None)

    def check(self):
        for raw, pattern, nbytes, is_input in self.items:
            front, back = raw[:PAD].cpu().numpy(), raw[PAD + nbytes:].cpu().numpy()
            assert np.array_equal(front, pattern[:PAD]), "bytes in front of a buffer were overwritten"
            assert np.array_equal(back, pattern[PAD + nbytes:]), "bytes behind a buffer were overwritten"
            if is_input:
                assert np.array_equal(raw[PAD:PAD + nbytes].cpu().numpy(), pattern[PAD:PAD + nbytes]), "an input was overwritten"


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _np(t):
    return t.cpu().numpy() if t is not None else None


def _call(torch, env, fn, *args):
    """one C ABI call, ordered against torch by device-wide synchronisation on both sides -> its return code"""
    env._use_current_stream()
    torch.cuda.synchronize()
    rc = fn(env._h, *args)
    torch.cuda.synchronize()
    return rc


def _bits(a, b):
    """bit-for-bit equality of two arrays of one dtype and shape"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def _report(kernel, worst):
    print("postproc ratio %s %.4f" % (kernel, worst))


# ---------------------------------------------------------------------------------------------------- qs_gae
def _qs_gae(torch, env, lib, x, gamma, lam):
    T, n = x["rewards"].shape
    G = Guards(torch, env.device)
    a = [G.put(x[k]) for k in ("rewards", "values", "dones", "last_values", "last_dones")]
    advs, rets = G.out((T, n)), G.out((T, n))
    rc = _call(torch, env, lib.qs_gae, T, n, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), gamma, lam, _p(advs), _p(rets))
    assert rc == 0
    G.check()
    return _np(advs), _np(rets)


def _ref(x, gamma, lam):
    return pr.gae64(x["rewards"], x["values"], x["dones"], x["last_values"], x["last_dones"], gamma, lam)


def _gae_rows(torch, env, lib, T, n, kernel):
    worst = 0.0
    for rate in pr.DONE_RATES:
        x = pr.gae_inputs(T, n, rate)
        for gamma, lam in pr.GAMMA_LAM:
            advs, rets = _qs_gae(torch, env, lib, x, gamma, lam)
            worst = max(worst, pr.check_gae(advs, rets, _ref(x, gamma, lam), "%s T=%d n=%d rate=%g (%g, %g)" % (kernel, T, n, rate, gamma, lam)))
    _report(kernel, worst)


@pytest.mark.parametrize("T,n", pr.GAE_TWO_PASS)
def test_gae_two_pass(torch, env, lib, T, n):
    """k_gae_reduce + k_gae_apply (n < 16 384): no seam, one seam with a done before / on / behind it, two seams"""
    assert n < pr.SERIAL_MIN_N
    _gae_rows(torch, env, lib, T, n, "k_gae_reduce+k_gae_apply")


@pytest.mark.parametrize("T,n", pr.GAE_SERIAL)
def test_gae_serial(torch, env, lib, T, n):
    """k_gae_serial (n >= 16 384): tail loop only, exactly one group, a group and a tail, three groups; a full and a ragged
    last block"""
    assert n >= pr.SERIAL_MIN_N
    _gae_rows(torch, env, lib, T, n, "k_gae_serial")


def test_gae_switch_between_the_scans(torch, env, lib):
    """one data set at n = 16 384 (serial scan) and its first 16 383 columns (two-pass scan): both within the bound of the
    same float64 columns"""
    T, n = pr.GAE_SWITCH
    worst = [0.0, 0.0]
    for rate in pr.DONE_RATES:
        x = pr.gae_inputs(T, n, rate)
        cut = {k: np.ascontiguousarray(v[..., :n - 1]) for k, v in x.items()}
        for gamma, lam in pr.GAMMA_LAM:
            ref = _ref(x, gamma, lam)
            worst[0] = max(worst[0], pr.check_gae(*_qs_gae(torch, env, lib, x, gamma, lam), ref, "serial side"))
            worst[1] = max(worst[1], pr.check_gae(*_qs_gae(torch, env, lib, cut, gamma, lam), tuple(r[:, :n - 1] for r in ref), "two-pass side"))
    _report("k_gae_serial", worst[0])
    _report("k_gae_reduce+k_gae_apply", worst[1])


# ---------------------------------------------------------------------------------------------------- qs_gae_flatten
def _qs_gae_flatten(torch, env, lib, x, gamma, lam, with_neglogp, with_advs):
    T, n = x["rewards"].shape
    G = Guards(torch, env.device)
    rew, val, dn, lv, ld = [G.put(x[k]) for k in ("rewards", "values", "dones", "last_values", "last_dones")]
    nl = G.put(x["neglogp"]) if with_neglogp else None
    f = {k: G.out((n * T,)) for k in ("returns", "values", "rewards")}
    f["neglogp"] = G.out((n * T,)) if with_neglogp else None
    f["masks"] = G.out((n * T,), np.uint8)
    advs = G.out((T, n)) if with_advs else None
    rets = G.out((T, n)) if with_advs else None
    rc = _call(torch, env, lib.qs_gae_flatten, T, n, _p(rew), _p(val), _p(nl), _p(dn), _p(lv), _p(ld), gamma, lam,
               _p(f["returns"]), _p(f["values"]), _p(f["neglogp"]), _p(f["rewards"]), _p(f["masks"]), _p(advs), _p(rets))
    assert rc == 0
    G.check()
    return {k: _np(v) for k, v in f.items()}, _np(advs), _np(rets)


@pytest.mark.parametrize("T,n", pr.GAE_FLATTEN)
def test_gae_flatten(torch, env, lib, T, n):
    """k_gae_flatten: T = 4 takes the vector flag but only the scalar tail, 16 one vector group, 20 / 36 vector groups and a
    tail, 15 / 17 the scalar stores; n = 65 leaves three waves of the block idle, 257 spills into a second block.  With and
    without neglogp, with and without the time-major advs / returns."""
    worst = 0.0
    for rate in pr.DONE_RATES:
        x = pr.gae_inputs(T, n, rate)
        for gamma, lam in pr.GAMMA_LAM:
            ref = _ref(x, gamma, lam)
            what = "k_gae_flatten T=%d n=%d rate=%g (%g, %g)" % (T, n, rate, gamma, lam)
            flat_ref = (pr.flatten_ref(ref[0]), pr.flatten_ref(ref[1]), pr.flatten_ref(ref[2]))
            first = None
            for with_neglogp in (True, False):
                for with_advs in (True, False):
                    f, advs, rets = _qs_gae_flatten(torch, env, lib, x, gamma, lam, with_neglogp, with_advs)
                    worst = max(worst, pr.check_gae(None, f["returns"], flat_ref, what + " flat_returns"))
                    assert _bits(f["values"], pr.flatten_ref(x["values"])) and _bits(f["rewards"], pr.flatten_ref(x["rewards"])), what
                    assert _bits(f["masks"], pr.flatten_ref((x["dones"] != 0).astype(np.uint8))), what       # 0 / 1, whatever the byte
                    if with_neglogp:
                        assert _bits(f["neglogp"], pr.flatten_ref(x["neglogp"])), what
                    if with_advs:
                        worst = max(worst, pr.check_gae(advs, rets, ref, what))
                        assert _bits(f["returns"], pr.flatten_ref(rets)), what
                    if first is None:
                        first = f["returns"]
                    assert _bits(f["returns"], first), what                  # the optional arrays change no result
    _report("k_gae_flatten", worst)


# ---------------------------------------------------------------------------------------------------- swap_and_flatten
@pytest.mark.parametrize("T,n", pr.FLATTEN_SHAPES)
@pytest.mark.parametrize("D", pr.FLATTEN_WIDTHS)
def test_swap_and_flatten(torch, env, lib, D, T, n):
    """k_swap_flatten<1>, <13>, k_swap_flatten_v4<1>, <3> on single rows and columns, tiles one short of, equal to and one
    past 32, and several ragged tiles: arange input (exact in float32), so every misplaced element shows"""
    x = np.arange(T * n * D, dtype=np.float32).reshape(T, n, D)
    assert x[-1, -1, -1] == T * n * D - 1 < 2 ** 24
    G = Guards(torch, env.device)
    src, dst = G.put(x), G.out((n * T, D))
    assert _call(torch, env, lib.qs_swap_and_flatten, T, n, D, _p(src), _p(dst)) == 0
    G.check()
    assert _bits(_np(dst), pr.flatten_ref(x))


@pytest.mark.parametrize("T,n", pr.FLATTEN_SHAPES)
def test_swap_and_flatten_u8(qa, torch, env, lib, T, n):
    """k_swap_flatten<1, uint8_t>: arbitrary bytes and the done bytes {0, 1, 2, 255} of the GAE inputs pass through unchanged;
    bool through the wrapper"""
    rs = np.random.RandomState(T * 1000 + n)
    for x in (rs.randint(0, 256, (T, n)).astype(np.uint8), pr.gae_inputs(T, n, 0.5)["dones"]):
        G = Guards(torch, env.device)
        src, dst = G.put(x), G.out((n * T,), np.uint8)
        assert _call(torch, env, lib.qs_swap_and_flatten_u8, T, n, _p(src), _p(dst)) == 0
        G.check()
        assert _bits(_np(dst), pr.flatten_ref(x))
    b = rs.rand(T, n) < 0.5
    got = qa.swap_and_flatten(env, torch.as_tensor(b))
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), pr.flatten_ref(b))


def test_swap_and_flatten_refuses_other_widths(torch, env, lib):
    x = np.arange(7 * 9 * 5, dtype=np.float32).reshape(7, 9, 5)
    G = Guards(torch, env.device)
    src, dst = G.put(x), G.out((9 * 7, 5))
    before = _np(dst).copy()
    assert _call(torch, env, lib.qs_swap_and_flatten, 7, 9, 5, _p(src), _p(dst)) == QS_ERR_INVALID
    G.check()
    assert _bits(_np(dst), before)


# ---------------------------------------------------------------------------------------------------- qs_episode_stats
class _Episodes:
    """three roll-outs of one (T, n, rate) through the C ABI: the carry stays on the device between them, the float64
    reference (returns, lengths, sum|r|) advances beside it"""

    def __init__(self, torch, env, lib, T, n, rate):
        self.torch, self.env, self.lib, self.T, self.n, self.rate = torch, env, lib, T, n, rate
        self.carry = Guards(torch, env.device)
        self.ep_ret = self.carry.out((n,), np.float32)
        self.ep_len = self.carry.out((n,), np.int32)
        self.ep_ret.zero_(); self.ep_len.zero_()
        self.ret64, self.len64, self.abs64 = np.zeros(n), np.zeros(n, np.int64), np.zeros(n)

    def roll(self, it, cap):
        """-> (count, keys, returns, lengths of the slots below cap, reference list, sum|r| per reference episode)"""
        T, n = self.T, self.n
        rew, dn, ld = pr.episode_inputs(T, n, self.rate, it)
        want = episode_stats_ref(rew, dn, ld, self.ret64, self.len64)
        abs_sum = pr.episode_abs_ref(rew, dn, ld, self.abs64)
        G = Guards(self.torch, self.env.device)
        a = [G.put(rew), G.put(dn), G.put(ld)]
        count = G.out((1,), np.int64)
        key, ret, ln = (G.out((cap,), np.int64), G.out((cap,), np.float32), G.out((cap,), np.int32)) if cap else (None, None, None)
        rc = _call(self.torch, self.env, self.lib.qs_episode_stats, T, n, _p(a[0]), _p(a[1]), _p(a[2]), _p(self.ep_ret), _p(self.ep_len),
                   _p(count), cap, _p(key), _p(ret), _p(ln))
        assert rc == 0
        G.check(); self.carry.check()
        # the carry: lengths exact, returns within the bound of a float32 running sum of that many rewards
        assert np.array_equal(_np(self.ep_len), self.len64)
        assert (np.abs(_np(self.ep_ret).astype(np.float64) - self.ret64) <= pr.sum_bound(self.len64, self.abs64)).all()
        return int(_np(count)[0]), _np(key), _np(ret), _np(ln), want, abs_sum


@pytest.mark.parametrize("T,n", pr.EPISODE_CASES)
def test_episode_stats(torch, env, lib, T, n):
    """k_episode_stats: tail loop only (T < 16), one group, a group and a tail, two groups and a tail; a lone lane, ragged
    waves, several blocks; no episode end, some, one at every step (count = cap = T n)"""
    worst = 0.0
    for rate in pr.EPISODE_RATES:
        ep = _Episodes(torch, env, lib, T, n, rate)
        for it in range(3):
            count, key, ret, ln, want, abs_sum = ep.roll(it, T * n)
            assert count == len(want)
            if rate == 1.0:
                assert count == T * n
            if rate == 0.0:
                assert count == 0
            order = np.argsort(key[:count], kind="stable")
            assert np.array_equal(key[:count][order], np.array([w[0] for w in want], np.int64))
            assert np.array_equal(ln[:count][order], np.array([w[2] for w in want], np.int32))
            err = np.abs(ret[:count][order].astype(np.float64) - np.array([w[1] for w in want], np.float64))
            b = pr.sum_bound([w[2] for w in want], abs_sum)
            assert (err <= b).all(), "T=%d n=%d rate=%g roll-out %d: worst err / bound %.3g" % (T, n, rate, it, float((err / np.maximum(b, 1e-300)).max()))
            if count:
                worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
    print("postproc episode err / bound %.4f" % worst)


def test_episode_stats_cap_below_count(torch, env, lib):
    """include/quadsim.h: *count is the number of episodes found, the first min(count, cap) slots are written"""
    T, n = 17, 257
    ep = _Episodes(torch, env, lib, T, n, 0.1)
    total = len(episode_stats_ref(*pr.episode_inputs(T, n, 0.1, 0), np.zeros(n), np.zeros(n, np.int64)))
    cap = total // 2
    assert cap >= 100
    count, key, ret, ln, want, abs_sum = ep.roll(0, cap)          # the output arrays are cap long: the sentinel starts behind them
    assert count == total == len(want)
    ref = {w[0]: (w[1], w[2], s) for w, s in zip(want, abs_sum)}
    assert len(set(key.tolist())) == cap                           # every slot below cap written, no key twice
    for k, r, le in zip(key.tolist(), ret.tolist(), ln.tolist()):
        assert k in ref and le == ref[k][1] and abs(r - ref[k][0]) <= pr.sum_bound(le, ref[k][2])


def test_episode_stats_counts_without_output_arrays(torch, env, lib):
    """cap = 0 with null output arrays: the count is right and the carry advances (checked inside roll)"""
    T, n = 17, 257
    ep = _Episodes(torch, env, lib, T, n, 0.1)
    for it in range(2):
        count, _, _, _, want, _ = ep.roll(it, 0)
        assert count == len(want) > 0
    assert ep.len64.max() > T                                     # an episode ran through both roll-outs


def test_episode_tracker_refuses_another_width(qa, torch, env):
    """EpisodeTracker.update sizes its carries from env.num_envs: a roll-out of another width is refused before any launch"""
    tr = qa.EpisodeTracker(env)
    for n in (env.num_envs + 1, env.num_envs - 1):
        with pytest.raises(ValueError):
            tr.update(torch.ones((4, n)), torch.ones((4, n), dtype=torch.uint8), torch.ones((n,), dtype=torch.uint8))
    torch.cuda.synchronize()
    assert tr._bufs is None and tr.count == 0
    assert not bool(tr.ep_ret.any()) and not bool(tr.ep_len.any())
    n = env.num_envs
    tr.update(torch.ones((4, n)), torch.zeros((4, n), dtype=torch.uint8), torch.ones((n,), dtype=torch.uint8))
    assert tr.count == n and bool((tr.results()[1] == 4).all())
