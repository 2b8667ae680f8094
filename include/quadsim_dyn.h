/* quadsim_dyn.h -- C ABI of libquadsim_dyn.so: random-shooting MPC through a LEARNED dynamics net, every candidate of every
 * env in one launch (plus one small arg-max launch).  The planner of MPC-based_RL.py:170-210 (Mpc_Controller.choose_action,
 * compute_cost) over its Dynamic_Net (:83-136), a 16 -> h1 -> h2 -> 12 ReLU MLP that predicts the normalised observation delta.
 *
 * The library is independent of libquadsim_hip.so: it takes observations, a seed and a net -- no env handle.  Every pointer
 * below is a DEVICE pointer unless it says otherwise; every call is ordered on `stream` (a hipStream_t, NULL = the default
 * stream) and synchronises nothing with the host.  The library allocates nothing per call: the caller owns the image and the
 * workspace.  C99-clean.
 *
 * ---- numerical contract ---------------------------------------------------------------------------------------------
 * Candidate actions.  a[c][h][0..3] = 2 u01(w) - 1 in float32 (u01(v) = fmaf((float)v, 2^-32, 2^-32), then fmaf(2, u, -1)),
 * w the four words of Philox4x32-10 block  (k << 26) | (c << 10) | h  of subsequence  (5 << 48) | (gid0 + env)  under `seed`:
 * exactly the candidates of qs_shooting_plan (include/quadsim.h) for the same (seed, env id, step counter k).
 *
 * One model step for a candidate with observation s (float32[12]) and action a (float32[4]):
 *   x = concat(s, a);  xh_i = (x_i - in_mean_i) * in_rscale_i  (a float32 subtraction, then a float32 product);
 *   layer l = 1, 2, 3:  acc = b_j;  acc = fmaf(w_jk, x_k, acc) for k = 0, 1, 2, ... ascending;  ReLU after layers 1 and 2
 *   (the exact-f32 matrix instruction v_mfma_f32_16x16x4_f32 is this chain, one rounding per product);
 *   s'_i = fmaf(d_i, out_std_i, out_mean_i) + s_i,  d the 12 outputs of layer 3.  No done flag, no reset.
 * Score (float64) = sum over h = 0 .. horizon-1 of  -fmaf(s_h[2], s_h[2], fmaf(s_h[1], s_h[1], s_h[0] * s_h[0]))  (a float32
 * term, the POSITION term of qs_shooting_plan), s_0 the given observation, s_{h+1} the model step of (s_h, a[c][h]): horizon - 1
 * predictions enter the score (compute_cost over ob_as).  traj[env][c][h] = s_{h+1}, h = 0 .. horizon-1; the last prediction
 * is computed only when traj is asked for.
 * Winner: higher score first, then lower index; if every score of an env is NaN the winner is index 0.  best_score is
 * scores[best_index], bit for bit.
 * Mapping-independence: the bits of candidate c depend on (net, obs, seed, gid, k, c) only -- not on n, paths, or where the
 * candidate runs.  Hidden widths are zero-padded to multiples of 16 (and up to the compiled widths below); the padding units
 * sit at the END of every k-ordered chain and add fmaf(0, 0, acc): acc itself (the one exception IEEE leaves: an accumulator
 * that is exactly -0 becomes +0).
 * NON-FINITE VALUES (NaN, +inf, -inf in a weight, a bias, a normaliser or an observation).  A diverged net looks diverged:
 * 1. Network.  A predicted delta is non-finite exactly where the float64 reference over the same net, observation and actions
 *    is (np.maximum(z, 0) and plain sums), and it is the same kind: NaN, +inf or -inf.  So ReLU is a select that keeps a NaN
 *    of either sign bit and any payload, relu = z <= 0 ? 0 : z, never a max that drops one: a net poisoned in w1, b1, w2, b2,
 *    w3, b3 or a normaliser makes every score NaN, for every env and candidate for which the reference does.
 * 2. Outcome.  A NaN score never wins; the outcome of an env whose scores are all NaN is the one defined above: winner index 0,
 *    best_score = scores[0], its NaN bits included.
 * 3. No leak.  An env whose observation is non-finite leaves every other env's outputs bit for bit.
 * Not covered: finite inputs whose float32 evaluation overflows.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= horizon <= 1024, 1 <= paths <= 65536, k < 2^36 (the keying), 1 <= n, n * ceil(paths / 16) < 2^31.
 * Hidden widths: the kernels are compiled for the padded pairs (64, 64), (128, 128) and (208, 112); a net runs on the first
 * pair that covers it, so (h1, h2) is supported iff  1 <= h1 <= 128 and 1 <= h2 <= 128,  or  1 <= h1 <= 208 and 1 <= h2 <= 112.
 * The weight image of the widest pair takes 120 656 bytes of the compute unit's 160 KiB of LDS.
 * A refused call returns an error code, leaves a message in qsd_last_error() and launches nothing.
 */
#ifndef QUADSIM_DYN_H
#define QUADSIM_DYN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSD_VERSION 1

enum { QSD_OK = 0, QSD_ERR_INVALID = 1, QSD_ERR_HIP = 2, QSD_ERR_UNSUPPORTED = 3 };

enum { QSD_OBS_DIM = 12, QSD_ACT_DIM = 4, QSD_IN_DIM = 16, QSD_MAX_HORIZON = 1024, QSD_MAX_PATHS = 65536, QSD_LDS_BYTES = 163840 };

/* The dynamics net as the caller holds it: row-major float32 device arrays, weights transposed (out, in) as torch's Linear
 * keeps them.  in_rscale = 1 / (std + 1e-6), computed by the caller (in float64, rounded once). */
typedef struct QsdNet {
    uint32_t struct_size; /* sizeof(QsdNet) */
    int32_t h1, h2;       /* hidden widths */
    int32_t reserved;
    const float *wt1;     /* [h1][16] */
    const float *b1;      /* [h1] */
    const float *wt2;     /* [h2][h1] */
    const float *b2;      /* [h2] */
    const float *wt3;     /* [12][h2] */
    const float *b3;      /* [12] */
    const float *in_mean;   /* [16] */
    const float *in_rscale; /* [16] */
    const float *out_std;   /* [12] */
    const float *out_mean;  /* [12] */
} QsdNet;

int qsd_version(void);
const char *qsd_last_error(void); /* host string, per thread */

/* Bytes of the padded device image of an (h1, h2) net. */
int qsd_net_image_bytes(int32_t h1, int32_t h2, size_t *bytes);

/* Pack `net` (a HOST struct of device pointers) into the device buffer `image` of qsd_net_image_bytes(h1, h2) bytes, 16-byte
 * aligned.  Pack once, plan many times.  The image starts with a header naming its compiled widths; the library also remembers
 * the widths of `image` on the host (the plan is launched without reading device memory), so an image is planned with through
 * the pointer it was packed into, in the process that packed it. */
int qsd_net_pack(const QsdNet *net, void *image, void *stream);

/* Bytes of the workspace of a plan over n envs x paths candidates (the float64 scores between the two launches). */
int qsd_plan_workspace_bytes(int64_t n, int32_t paths, size_t *bytes);

/* One plan per env.  obs [n,12] float32; actions [n,4] float32 = the winner's first action.  Nullable outputs: best_score [n]
 * float64, best_index [n] int32, sequence [n,horizon,4] float32 (the winner's actions), scores [n,paths] float64,
 * traj [n,paths,horizon,12] float32. */
int qsd_shooting_plan(const void *image, int64_t n, const float *obs, uint64_t seed, uint64_t gid0, uint64_t k, int32_t horizon,
                      int32_t paths, void *workspace, float *actions, double *best_score, int32_t *best_index, float *sequence,
                      double *scores, float *traj, void *stream);

#ifdef __cplusplus
}
#endif
#endif
