"""-m "not gpu": the harness of tests/test_gpu_postproc.py is checked before the GPU is.  Numpy float32 emulations of both
association orders of the device GAE (the serial chain of k_gae_serial / k_gae_flatten; the two-pass scan of k_gae_reduce +
k_gae_apply with 64-step chunks) stay within the bound of postproc_ref.gae64 at every input the GPU rows use, and six mutants
of them exceed it there.  tests/postproc_matrix.py has exactly one row per compiled instantiation of the kernels of
csrc/rollout_ops.hpp, and every row names a GPU test that exists."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_notes
import postproc_matrix
import postproc_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def fma(a, b, c):
    """float32 fused multiply-add through float64: the product of two float32 is exact there"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


class Gae32:
    """the device arithmetic of gae_terms / k_gae_serial in numpy float32, one vector op per step over all envs.
    mutant: None or one of MUTANTS"""

    def __init__(self, x, gamma, lam, mutant=None):
        self.r, self.v, self.d = x["rewards"], x["values"], x["dones"]
        self.lv, self.ld = x["last_values"], x["last_dones"]
        self.T, self.n = self.r.shape
        self.g, self.gl = f32(gamma), f32(gamma) * f32(lam)
        self.mutant = mutant

    def terms(self, t, seam=False):
        """(delta, k, nextv) of step t; seam: t is the last step of a chunk that is not the last chunk"""
        T, m = self.T, self.mutant
        if t == T - 1:
            nonterm = np.ones(self.n, f32) if m == "last_dones_ignored" else (self.ld == 0).astype(f32)
            nextv = self.lv
        else:
            dd = self.d[t] if (m == "seam_reads_dones_t" and seam) else self.d[t + 1]
            nonterm = (dd == 0).astype(f32)
            nextv = self.lv if (m == "last_values_at_T_minus_2" and t == T - 2) else self.v[t + 1]
        delta = (self.r[t] + (self.g * nextv) * nonterm) - self.v[t]
        return delta, self.gl * nonterm, nextv

    def store(self, out, t, A, nextv):
        out[0][t] = A
        out[1][t] = A + (nextv if self.mutant == "returns_add_next_value" else self.v[t])

    def serial(self):
        out = np.zeros((2, self.T, self.n), f32)
        A = np.zeros(self.n, f32)
        for t in reversed(range(self.T)):
            delta, k, nextv = self.terms(t)
            A = fma(k, A, delta)
            self.store(out, t, A, nextv)
        return out[0], out[1]

    def two_pass(self):
        T, n, m = self.T, self.n, self.mutant
        C = (T + pr.CHUNK - 1) // pr.CHUNK
        P, S = np.ones((C, n), f32), np.zeros((C, n), f32)
        for c in range(C):                                                # k_gae_reduce
            t0, t1 = c * pr.CHUNK, min(T, (c + 1) * pr.CHUNK)
            for t in reversed(range(t0, t1)):
                seam = t == t1 - 1 and t1 < T
                delta, k, _ = self.terms(t, seam)
                S[c] = fma(k, S[c], delta)
                P[c] = P[c] * (self.gl * np.ones(n, f32) if (m == "P_carried_over_done_on_seam" and seam) else k)
        out = np.zeros((2, T, n), f32)
        for c in range(C):                                                # k_gae_apply
            A = np.zeros(n, f32)
            if m != "incoming_advantage_dropped":
                for cc in range(C - 1, c, -1):
                    A = fma(P[cc], A, S[cc])
            t0, t1 = c * pr.CHUNK, min(T, (c + 1) * pr.CHUNK)
            for t in reversed(range(t0, t1)):
                delta, k, nextv = self.terms(t, t == t1 - 1 and t1 < T)
                A = fma(k, A, delta)
                self.store(out, t, A, nextv)
        return out[0], out[1]


# mutant -> the scans it changes
MUTANTS = {"seam_reads_dones_t": ("two_pass",), "incoming_advantage_dropped": ("two_pass",),
           "P_carried_over_done_on_seam": ("two_pass",), "last_dones_ignored": ("two_pass", "serial"),
           "last_values_at_T_minus_2": ("two_pass", "serial"), "returns_add_next_value": ("two_pass", "serial")}


EMU_COLUMNS = 512


def _rows():
    """(scan, T, n) of every GAE input of the GPU rows.  The emulations run the first EMU_COLUMNS columns of each data set:
    columns are independent and identically drawn, and an emulation has no lanes or blocks for the width to matter to."""
    rows = [("two_pass", T, n) for T, n in pr.GAE_TWO_PASS]
    rows += [("serial", T, n) for T, n in pr.GAE_SERIAL]
    rows += [("serial", T, n) for T, n in pr.GAE_FLATTEN]
    rows += [(scan, pr.GAE_SWITCH[0], pr.GAE_SWITCH[1]) for scan in ("serial", "two_pass")]
    return rows


@pytest.fixture(scope="module")
def sweep():
    """{(scan, T, n, rate, gamma, lam): (inputs, gae64 reference)}: computed once, shared, left unchanged"""
    out = {}
    for scan, T, n in _rows():
        for rate in pr.DONE_RATES:
            x = {k: np.ascontiguousarray(v[..., :EMU_COLUMNS]) for k, v in pr.gae_inputs(T, n, rate).items()}
            for gamma, lam in pr.GAMMA_LAM:
                out[(scan, T, n, rate, gamma, lam)] = (x, pr.gae64(x["rewards"], x["values"], x["dones"], x["last_values"],
                                                                   x["last_dones"], gamma, lam))
    return out


def test_gae64_on_a_hand_worked_case():
    """T = 3, one env, gamma = lam = 0.5 (exact in float32), a done before step 2:
    A_2 = r_2 + g v_last - v_2 = 1 + 1 - 1 = 1;  A_1 = r_1 - v_1 (step 2 starts a new episode) = 2 - 3 = -1;
    A_0 = r_0 + g v_1 - v_0 + g l A_1 = 4 + 1.5 - 2 - 0.25 = 3.25"""
    a, ret, E = pr.gae64([[4.0], [2.0], [1.0]], [[2.0], [3.0], [1.0]], [[0], [0], [7]], [2.0], [0], 0.5, 0.5)
    assert a[:, 0].tolist() == [3.25, -1.0, 1.0] and ret[:, 0].tolist() == [5.25, 2.0, 2.0]
    assert E[:, 0].tolist() == [4 + 1.5 + 2 + 0.25 + 0.25 * 5, 5.0, 3.0]
    a, _, _ = pr.gae64([[4.0], [2.0], [1.0]], [[2.0], [3.0], [1.0]], [[0], [0], [0]], [2.0], [255], 0.5, 0.5)
    assert a[2, 0] == 0.0                                            # last_dones cuts the bootstrap


def test_inputs_reach_what_they_are_for():
    x = pr.gae_inputs(129, 257, 0.0)
    env = np.arange(257)
    for g, t in ((1, 63), (2, 64), (3, 65), (4, 128)):
        assert x["dones"][t, env % 8 == g].all() and not x["dones"][t, env % 8 != g].any()
    x = pr.gae_inputs(36, 257, 0.5)
    assert set(np.unique(x["dones"])) == {0, 1, 2, 255} and set(np.unique(x["last_dones"])) == {0, 1, 2, 255}
    assert pr.GAE_SWITCH[1] == pr.SERIAL_MIN_N and pr.CHUNK == 64


def test_emulations_stay_within_the_bound(sweep):
    worst = {"serial": 0.0, "two_pass": 0.0}
    for (scan, T, n, rate, gamma, lam), (x, ref) in sweep.items():
        advs, rets = getattr(Gae32(x, gamma, lam), scan)()
        worst[scan] = max(worst[scan], pr.check_gae(advs, rets, ref, "%s T=%d n=%d rate=%g (%g, %g)" % (scan, T, n, rate, gamma, lam)))
    print("worst ratio of the emulations:", worst)
    assert max(worst.values()) > pr.KAPPA_GAE / 4                    # the bound is within a small factor of what float32 does


def test_both_scans_agree_where_the_chain_is_one_chunk(sweep):
    """T <= 64: one chunk, so the two-pass scan is the serial chain, bit for bit (a check of the emulation itself)"""
    for (scan, T, n, rate, gamma, lam), (x, _) in sweep.items():
        if T <= pr.CHUNK:
            e = Gae32(x, gamma, lam)
            assert all(np.array_equal(a, b) for a, b in zip(e.serial(), e.two_pass()))


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutants_exceed_the_bound(sweep, mutant):
    """each mutant is out of bound on at least one input of the GPU rows (and far out: the worst ratio is printed)"""
    worst, caught = 0.0, 0
    for (scan, T, n, rate, gamma, lam), (x, ref) in sweep.items():
        if scan not in MUTANTS[mutant]:
            continue
        advs, rets = getattr(Gae32(x, gamma, lam, mutant), scan)()
        r = max(pr.gae_ratios(advs, rets, ref))
        caught += r > pr.KAPPA_GAE
        worst = max(worst, r)
    print("mutant %s: worst ratio %.3g, out of bound on %d inputs" % (mutant, worst, caught))
    assert caught >= 1 and worst > 2.0 * pr.KAPPA_GAE


def test_summation_bound_on_float32_running_sums():
    """a float32 running sum over episodes of the shared inputs stays within len * 2^-24 * sum|r|"""
    from oracle.pyoracle import episode_stats_ref
    worst = 0.0
    for T, n in ((33, 257), (17, 1000)):
        ep_ret, ep_len, ep_abs = np.zeros(n), np.zeros(n, np.int64), np.zeros(n)
        run = np.zeros(n, f32)
        for it in range(3):
            rew, dn, ld = pr.episode_inputs(T, n, 0.1, it)
            want = episode_stats_ref(rew, dn, ld, ep_ret, ep_len)
            abs_sum = pr.episode_abs_ref(rew, dn, ld, ep_abs)
            after = np.concatenate([dn[1:], ld[None]], 0) != 0
            got = []
            for t in range(T):
                run = run + rew[t]
                got += [float(run[i]) for i in np.nonzero(after[t])[0]]
                run[after[t]] = 0
            err = np.abs(np.array(got) - [w[1] for w in want])
            b = pr.sum_bound([w[2] for w in want], abs_sum)
            assert (err <= b).all()
            worst = max(worst, float((err / np.maximum(b, 1e-300)).max()))
            assert (np.abs(run - ep_ret) <= pr.sum_bound(ep_len, ep_abs)).all()
    assert 0.05 < worst <= 1.0


# ---------------------------------------------------------------------------------------------------- the matrix
@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    return kernel_notes.kernel_notes(kernel_notes.code_object(tmp_path_factory.mktemp("isa_postproc")))


def test_rows_are_exactly_the_instantiations(notes):
    keys = [r["key"] for r in postproc_matrix.ROWS]
    assert len(keys) == len(set(keys)), "duplicate rows"
    got = kernel_notes.instantiations_with_types(notes, postproc_matrix.KERNELS, namespace="qs")
    assert {k[0] for k in got} == set(postproc_matrix.KERNELS)
    assert set(keys) == got, "rows without an instantiation: %s; instantiations without a row: %s" % (
        sorted(set(keys) - got, key=str), sorted(got - set(keys), key=str))


def test_kernel_list_is_every_kernel_of_the_header():
    """a kernel added to rollout_ops.hpp has to be added to KERNELS (and then needs a row)"""
    import re
    src = open(os.path.join(ROOT, "quadsim_amd", "csrc", "rollout_ops.hpp")).read()
    assert set(re.findall(r"__global__.*?\bvoid\s+(k_\w+)\s*\(", src)) == set(postproc_matrix.KERNELS)


def test_instantiations_with_types_on_known_symbols():
    syms = ["_ZN2qs11k_gae_applyENS_7GaeArgsE", "_ZN2qs14k_swap_flattenILi13EfEEvPKT0_PS1_ll",
            "_ZN2qs14k_swap_flattenILi1EhEEvPKT0_PS1_ll", "_ZN2qs17k_swap_flatten_v4ILi3EEEvPK15HIP_vector_typeIfLj4EEPS2_ll",
            "_ZN2qs19k_swap_flatten_v4_xILi3EEEvPKfPfll", "_ZN2qs5k_envILi0ELb1EEEvPf"]
    got = kernel_notes.instantiations_with_types(syms, ("k_gae_apply", "k_swap_flatten", "k_swap_flatten_v4"), namespace="qs")
    assert got == {("k_gae_apply",), ("k_swap_flatten", 13, "float"), ("k_swap_flatten", 1, "uint8_t"), ("k_swap_flatten_v4", 3)}


def test_rows_name_existing_gpu_tests():
    files = sorted({r["test"].split("::")[0] for r in postproc_matrix.ROWS})
    out = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider"] + files, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    ids = set(out.stdout.split())
    missing = [r["test"] for r in postproc_matrix.ROWS if r["test"] not in ids]
    assert not missing, missing
