/* quadsim_dyn_mppi.h -- C ABI of libquadsim_dynmppi.so: MPPI (model-predictive path integral control) through a LEARNED
 * dynamics net.  qs_mppi_plan's contract (include/quadsim.h) with qsd_shooting_plan's model (include/quadsim_dyn.h): per
 * iteration, `paths` Gaussian candidates around a nominal action sequence are rolled through the net from the given observation
 * and scored by position, then the nominal becomes their softmax-weighted mean.  The nominal goes in and comes out (warm start);
 * the closed loop stays with the caller.
 *
 * The library is independent of libquadsim_hip.so and of libquadsim_dyn.so at link time.  `image` is a weight image packed by
 * qsd_net_pack of libquadsim_dyn.so; this library keeps NO host table of images: the caller passes the hidden widths (h1, h2) of
 * the net, the host maps them to the compiled pair by the rule of quadsim_dyn.h, and the kernels check the image header (magic,
 * tile counts, size) against that pair -- on a mismatch they read nothing past the first 16 bytes of the image and write
 * nothing.  Every pointer below is a DEVICE pointer; every call is ordered on `stream` (a hipStream_t, NULL = the default
 * stream) and synchronises nothing with the host.  The library allocates nothing: the caller owns the workspace.  C99-clean.
 *
 * Launches per plan: 2 x iterations -- per iteration one roll-out launch (every candidate of every env) and one update launch
 * (one workgroup per env).  Iteration 0 reads nominal_in directly; there is no launch for the shift.  The boundary between two
 * launches is the only ordering between workgroups.
 *
 * ---- numerical contract ---------------------------------------------------------------------------------------------
 * Nominal.  U[h] = nominal_in[env][min(h + shift, horizon - 1)], zeros when nominal_in is NULL.  All of nominal_in is read
 * before anything is written to nominal_out, so nominal_in may alias nominal_out.
 * Candidates, in iteration `it`: exactly those of qs_mppi_plan.  Candidate 0 is clamp(U[h], -1, 1), no draw.  For c >= 1:
 * a[c][h][j] = clamp(fmaf(sigma, z_j, U[h][j]), -1, 1) in float32, with z = noise[it][c][h] if `noise` is given, otherwise the
 * four normals (Box-Muller on (0,1] uniforms, (w0, w1) -> z0 = r cos, z1 = r sin, (w2, w3) -> z2, z3) of Philox4x32-10 block
 * (1 << 63) | (k << 30) | (it << 26) | (c << 10) | h  of subsequence  (5 << 48) | (gid0 + env)  under `seed`.  For the same
 * nominal these are candidate for candidate those of qs_mppi_plan with the same (seed, env id, step counter k).
 * Model step: word for word that of quadsim_dyn.h (the same device function): normalise, three k-ascending fmaf chains with
 * ReLU after the first two, s' = fmaf(d, out_std, out_mean) + s.  No done flag, no reset.
 * Score (float64) = sum over h = 0 .. horizon-1 of  -fmaf(s_h[2], s_h[2], fmaf(s_h[1], s_h[1], s_h[0] * s_h[0]))  (a float32
 * term), s_0 the given observation: horizon - 1 predictions enter it.  traj[env][c][h] = s_{h+1} of the LAST iteration; the last
 * prediction is computed only when traj is asked for.
 * Weights and update: those of qs_mppi_plan.  Smax = the maximum over the non-NaN scores; w[c] = exp((S[c] - Smax) / lambda) in
 * float64, a NaN giving 0; U'[h] = sum_c w[c] a[c][h] / sum_c w[c], both sums float64, rounded to float32 once.  Summation
 * order: row r of the update workgroup (128 rows of 8 lanes, whatever `paths`) adds c = r, r + 128, ... in ascending order,
 * then the 128 partial sums are added in row order -- a function of `paths` alone.  If no weight is positive (every score NaN), U stays.
 * Outputs: nominal_out [n,horizon,4] = the last U; actions [n,4] = nominal_out[:,0]; best_score [n] = Smax of the last
 * iteration (-inf if every score is NaN); scores [n,iterations,paths] float64; trace [n,iterations+1,horizon,4] (trace[:,0] =
 * the shifted input, trace[:,it+1] = U after iteration it); candidates [n,paths,horizon,4] and traj [n,paths,horizon,12] of
 * the last iteration.  best_score, scores, trace, candidates and traj are nullable, as are nominal_in and noise.
 * Invariants: the bits of candidate c depend on (net, obs, seed, gid, k, it, c, the nominal) only -- not on n, on `paths`, or on
 * where the candidate runs; the first j iterations of a call with more iterations are the call with iterations = j.
 * NON-FINITE VALUES (NaN, +inf, -inf in the net, a normaliser, an observation, nominal_in or the caller's noise):
 * 1. Network.  As in quadsim_dyn.h (the same device function): a predicted delta is non-finite exactly where, and of the kind
 *    that, the float64 reference makes it; ReLU keeps a NaN of either sign bit.  A net poisoned in a weight, a bias or a
 *    normaliser makes every score NaN, for every env and candidate for which the reference does.
 * 2. Candidates.  clamp keeps a NaN and clamps an infinity like any other value: a NaN in nominal_in[env][h][j] or in
 *    noise[it][c][h] makes exactly the candidates NaN that fmaf and clamp make NaN.  Their scores are NaN and their weights 0.
 *    (The weighted sum still adds 0 * NaN: the element of U that a NaN candidate of one iteration touched is NaN from then on,
 *    every candidate of the env is NaN in the next iteration, and U stays.)
 * 3. Outcome.  For an env whose scores are all NaN: U stays, best_score = -inf, as defined above.
 * 4. No leak.  Every env that reads no non-finite value keeps its bits.
 * Not covered: finite inputs whose float32 evaluation overflows.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= horizon <= 1024, 1 <= paths <= 65536, 1 <= iterations <= 16, k < 2^33 (the keying), lambda > 0 and finite, sigma >= 0
 * and finite, shift 0 or 1, 1 <= n, n * ceil(paths / 16) < 2^31.  Hidden widths as in quadsim_dyn.h: (h1, h2) runs on the first
 * of the compiled pairs (64, 64), (128, 128), (208, 112) that covers it.  workspace, actions, nominal_in, nominal_out, noise,
 * trace and candidates are 16-byte aligned (rows of four floats).
 * A refused call returns an error code, leaves a message in qsdm_last_error() and launches nothing.
 */
#ifndef QUADSIM_DYN_MPPI_H
#define QUADSIM_DYN_MPPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSDM_VERSION 1

enum { QSDM_OK = 0, QSDM_ERR_INVALID = 1, QSDM_ERR_HIP = 2, QSDM_ERR_UNSUPPORTED = 3 };

enum { QSDM_MAX_HORIZON = 1024, QSDM_MAX_PATHS = 65536, QSDM_MAX_ITERATIONS = 16, QSDM_LDS_BYTES = 163840 };

int qsdm_version(void);
const char *qsdm_last_error(void); /* host string, per thread */

/* Bytes of the workspace of a plan over n envs: the nominal between the iterations [n,horizon,4] float32, then the float64
 * scores / weights [n,paths] between the two launches of an iteration. */
int qsdm_workspace_bytes(int64_t n, int32_t horizon, int32_t paths, size_t *bytes);

/* One plan per env.  image: packed by qsd_net_pack for a net of hidden widths (h1, h2); obs [n,12] float32; noise (nullable)
 * [iterations,paths,horizon,4] float32, shared by the envs; nominal_in (nullable) / nominal_out [n,horizon,4] float32. */
int qsdm_mppi_plan(const void *image, int32_t h1, int32_t h2, int64_t n, const float *obs, uint64_t seed, uint64_t gid0, uint64_t k,
                   int32_t horizon, int32_t paths, int32_t iterations, float lambda, float sigma, int32_t shift,
                   const float *nominal_in, const float *noise, void *workspace, float *actions, float *nominal_out,
                   double *best_score, double *scores, float *trace, float *candidates, float *traj, void *stream);

#ifdef __cplusplus
}
#endif
#endif
