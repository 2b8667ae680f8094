"""Float64 references and error bounds of the roll-out post-processing kernels of csrc/rollout_ops.hpp (test helper; CPU only,
no GPU, no torch): GAE(lambda), swap_and_flatten and the episode accounting, with the inputs the CPU and the GPU tests share.

GAE.  gae64() restates rl_baselines/ppo2/ppo2.py:507-520 in float64 and, in the same reverse walk, the first-order error scale

    E_t = |r_t| + |gamma v_{t+1}| nonterm + |v_t| + |k_t A_{t+1}| + k_t E_{t+1},      k_t = gamma lam nonterm,

the magnitudes of everything that is summed into A_t.  A float32 advantage must satisfy |err| <= KAPPA_GAE * 2^-24 * E and a
return the same with E + |returns64| (one more rounded addition), on every element.  Worst ratios err / (2^-24 * E), over every
input of GAE_TWO_PASS / GAE_SERIAL / GAE_SWITCH / GAE_FLATTEN below (four (gamma, lam) pairs, done rates 0 / 0.05 / 0.5):

    numpy float32 emulation, serial chain (tests/test_postproc_cpu.py; 512 columns per input)      2.10   CPU
    numpy float32 emulation, two-pass scan with 64-step chunks (512 columns per input)             2.10   CPU
    k_gae_reduce + k_gae_apply (every column; worst at the 16 383 columns of GAE_SWITCH)            2.40   MI355X
    k_gae_serial (every column, up to 16 385)                                                       2.42   MI355X
    k_gae_flatten (every column, up to 257)                                                         1.94   MI355X
    mutants of the emulations, each at its worst element: P carried across a done on a seam 2.3e5, incoming advantage of a
    chunk dropped 7.7e6, seam reads dones[t] 2.8e8, last_values at T-2 3.2e8, last_dones ignored 2.1e9, returns = A + v_{t+1}
    8.9e10                                                                                                 CPU

A rounding count of one step gives 5 (gamma v, + r, - v, gamma lam, the fma), each on a magnitude that E contains.  KAPPA_GAE = 5
is 2.07 times the worst correct ratio (2.42) and five orders of magnitude below the least visible mutant.  The MI355X figures
are from one run of tests/test_gpu_postproc.py (2026-10-18); profiles/postproc/README.md has the table.

Episode accounting.  A finished episode's float32 return, or a carried ep_ret, is a recursive sum of `len` float32 rewards:
|err| <= len * 2^-24 * sum|r| (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4: gamma_{len-1} sum|r|).  Derived,
not measured; episode_abs_ref() gives sum|r| of every episode and of every carry.
"""
import numpy as np

U32 = 2.0 ** -24

KAPPA_GAE = 5.0

GAMMA_LAM = ((0.99, 0.95), (1.0, 1.0), (0.9, 1.0), (1.0, 0.0))
DONE_RATES = (0.0, 0.05, 0.5)
CHUNK = 64                     # kGaeChunk
SERIAL_MIN_N = 16384           # qs_gae walks one serial chain per env from this width on

# (T, n) of the rows of tests/test_gpu_postproc.py; every one runs with every (gamma, lam) and every done rate
GAE_TWO_PASS = [(T, n) for T in (1, 63, 64, 65, 129) for n in (1, 257)]
GAE_SERIAL = [(T, n) for T in (1, 15, 16, 17, 47, 48) for n in (16384, 16385)]
GAE_SWITCH = (33, 16384)       # one data set at n = 16384 (serial) and its first 16383 columns (two-pass)
GAE_FLATTEN = [(T, n) for T in (1, 4, 15, 16, 17, 20, 36) for n in (1, 63, 64, 65, 257)]


# ---------------------------------------------------------------------------------------------------- inputs
def gae_inputs(T, n, rate, seed=0):
    """rewards ~ N(0,1), values ~ 2 N(0,1), neglogp ~ N(0,1) [T,n] float32, dones [T,n] / last_dones [n] u8 at `rate`, last_values
    [n].  At rate 0.5 the done bytes take the values {1, 2, 255}.  For T >= 65 a done is forced before, on and behind the
    first chunk seam (dones[63], [64], [65]) and, for T >= 129, on the second one (dones[128]), in disjoint groups of envs
    (env % 8 = 1, 2, 3, 4), whatever the rate."""
    rs = np.random.RandomState(1000003 * T + 101 * n + int(round(rate * 100)) + 7919 * seed)
    rew = rs.randn(T, n).astype(np.float32)
    val = (2.0 * rs.randn(T, n)).astype(np.float32)
    nl = rs.randn(T, n).astype(np.float32)
    lv = (2.0 * rs.randn(n)).astype(np.float32)
    dn = (rs.rand(T, n) < rate).astype(np.uint8)
    ld = (rs.rand(n) < rate).astype(np.uint8)
    if rate == 0.5:
        dn *= np.array([1, 2, 255], np.uint8)[rs.randint(0, 3, (T, n))]
        ld *= np.array([1, 2, 255], np.uint8)[rs.randint(0, 3, n)]
    env = np.arange(n)
    for g, t in ((1, 63), (2, 64), (3, 65), (4, 128)):
        if t < T:
            dn[t, env % 8 == g] = 1
    return dict(rewards=rew, values=val, neglogp=nl, dones=dn, last_values=lv, last_dones=ld)


def episode_inputs(T, n, rate, it, seed=0):
    """roll-out `it` of a sequence: rewards ~ N(0,1) [T,n] float32, dones [T,n] / last_dones [n] u8 at `rate`"""
    rs = np.random.RandomState(1000003 * T + 101 * n + int(round(rate * 100)) + 7919 * seed + 17 * it)
    rew = rs.randn(T, n).astype(np.float32)
    dn = (rs.rand(T, n) < rate).astype(np.uint8)
    ld = (rs.rand(n) < rate).astype(np.uint8)
    return rew, dn, ld


# ---------------------------------------------------------------------------------------------------- GAE
def gae64(rewards, values, dones, last_values, last_dones, gamma, lam):
    """ppo2.py:507-520 in float64 -> (advs, returns, E) [T,n]; gamma and lam are rounded to float32 first (what the C ABI
    receives), any nonzero dones byte is a done.  E: the first-order error scale of advs (module docstring)."""
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    r, v = np.asarray(rewards, np.float64), np.asarray(values, np.float64)
    d = np.asarray(dones) != 0
    T, n = r.shape
    advs, E = np.zeros((T, n)), np.zeros((T, n))
    A, e = np.zeros(n), np.zeros(n)                                       # last_gae_lam = 0, :510
    for t in reversed(range(T)):
        if t == T - 1:                                                    # :512-514
            nonterm = 1.0 - (np.asarray(last_dones) != 0)
            nextv = np.asarray(last_values, np.float64)
        else:                                                             # :516-517
            nonterm = 1.0 - d[t + 1]
            nextv = v[t + 1]
        delta = r[t] + g * nextv * nonterm - v[t]                         # :518
        k = g * l * nonterm
        e = np.abs(r[t]) + np.abs(g * nextv) * nonterm + np.abs(v[t]) + np.abs(k * A) + k * e
        A = delta + k * A                                                 # :519
        advs[t], E[t] = A, e
    return advs, advs + v, E                                              # :520


def gae_ratios(advs, returns, ref):
    """worst err / (2^-24 * scale) of float32 advantages and returns against ref = gae64(...) -> (ratio_advs, ratio_returns)"""
    a64, r64, E = ref
    ra = np.abs(np.asarray(advs, np.float64) - a64) / (U32 * np.maximum(E, 1e-300))
    rr = np.abs(np.asarray(returns, np.float64) - r64) / (U32 * np.maximum(E + np.abs(r64), 1e-300))
    return float(ra.max()), float(rr.max())


def check_gae(advs, returns, ref, what=""):
    """every element of advs / returns (either may be None) within KAPPA_GAE * 2^-24 * scale of ref = gae64(...)
    -> worst ratio"""
    a64, r64, E = ref
    worst = 0.0
    for name, got, want, scale in (("advs", advs, a64, E), ("returns", returns, r64, E + np.abs(r64))):
        if got is None:
            continue
        got = np.asarray(got)
        assert got.dtype == np.float32 and got.shape == want.shape, "%s %s: %s %s" % (what, name, got.dtype, got.shape)
        ratio = np.abs(got.astype(np.float64) - want) / (U32 * np.maximum(scale, 1e-300))
        bad = ~(ratio <= KAPPA_GAE)                                       # a NaN is out of bound
        assert not bad.any(), "%s %s: %d of %d elements out of bound, worst ratio %.3g (kappa %.3g) at [t, env] = %s" % (
            what, name, int(bad.sum()), bad.size, float(np.nanmax(ratio)), KAPPA_GAE, np.argwhere(bad)[0].tolist())
        worst = max(worst, float(ratio.max()))
    return worst


# ---------------------------------------------------------------------------------------------------- flatten
def flatten_ref(x):
    """swap_and_flatten, ppo2.py:531-539: [T,n,...] -> [n*T,...]"""
    x = np.asarray(x)
    T, n = x.shape[0], x.shape[1]
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((n * T,) + x.shape[2:])


FLATTEN_SHAPES = ((1, 1), (1, 70), (70, 1), (31, 33), (32, 32), (33, 31), (65, 97))
FLATTEN_WIDTHS = (1, 4, 12, 13)


# ---------------------------------------------------------------------------------------------------- episode accounting
EPISODE_CASES = [(T, n) for T in (1, 15, 16, 17, 33) for n in (1, 63, 65, 257, 1000)]
EPISODE_RATES = (0.0, 0.1, 1.0)


def episode_abs_ref(rewards, dones, last_dones, abs_ret):
    """sum|r| of every episode that ends in the roll-out, in the order of oracle.pyoracle.episode_stats_ref; abs_ret [n]
    float64 carries sum|r| of the unfinished episodes and is updated in place"""
    from oracle.pyoracle import episode_stats_ref
    scratch = np.zeros(len(abs_ret), np.int64)
    return np.array([w[1] for w in episode_stats_ref(np.abs(np.asarray(rewards, np.float64)), dones, last_dones, abs_ret, scratch)])


def sum_bound(length, abs_sum):
    """forward-error bound of a float32 recursive sum of `length` terms whose magnitudes add up to abs_sum"""
    return np.asarray(length, np.float64) * U32 * np.asarray(abs_sum, np.float64)
