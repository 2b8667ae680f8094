/* quadsim_ppo.h -- C ABI of libquadsim_ppo.so: the PPO2 update on the device.
 * The `noptepochs x nminibatches` Adam steps on the clipped-surrogate loss of rl_baselines/ppo2/ppo2.py:138-207, 244-300 over the
 * tensors a Runner roll-out returns.  qsp_update enqueues, per Adam step, three launches on the caller's stream -- k_ppo_grad
 * (grid slices x 2 branches), k_ppo_reduce and k_ppo_apply (both over the parameter elements) -- after one launch of
 * k_ppo_adv_stats for the whole call.  The kernel boundary is the only ordering across workgroups: there is no grid-wide barrier,
 * no workgroup waits for another, and there are no floating-point atomics.  Nothing synchronises with the host.
 *
 * The library is independent of the other five at link time and shares no host state with them.  The net is the actor-critic of
 * quadsim_amd/runner.py in either layout (the constants of QsActorCriticNet in quadsim.h): 12 -> 128 -> 128 -> {4 | 1} with ReLU
 * and a state-independent logstd, given as it is stored: float32 tensors in the policy's (in, out) layout in the slots
 *     0 w0 [12,128]  1 b0 [128]  2 w1 [128,128]  3 b1 [128]  4 w2 [128,4]  5 b2 [4]  6 wv0 [12,128]  7 bv0 [128]
 *     8 wv1 [128,128]  9 bv1 [128]  10 wv2 [128,1]  11 bv2 [1]  12 logstd [4]
 * each with Adam's two moments of the same shape.  QSP_NET_SHARED_TRUNK: slots 6 and 7 must be NULL in w, m and v (the value
 * branch reads w0, b0).  QSP_NET_TOWERS: all thirteen.  All are updated in place.  Every pointer is a DEVICE pointer unless stated
 * otherwise.  The library allocates nothing: the caller passes a workspace of qsp_workspace_bytes.  C99-clean.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add) ---------------------
 * Rows.  Step s (Adam step t0 + s + 1) uses the rows indices[s][0 .. batch-1] of the data.  `indices` is a DEVICE array: the
 * library cannot read it, so entries outside [0, n) are UNDEFINED BEHAVIOUR and keeping them inside is the caller's contract.
 * Advantages (ppo2.py:264-265), once per call and step: d_i = returns_i - values_i (float32); mean = sum d_i / batch and
 * var = sum (d_i - mean)^2 / batch in float64 (thread i of 256 adds the elements i, i + 256, .. in ascending order, the 256 sums
 * are added in a fixed binary tree); stored as float32(mean) and R = float32(1 / (sqrt(var) + 1e-8)).  A_i = (d_i - mean) * R.  A
 * batch of 1 gives A = 0.
 * Slices.  The batch is cut into chunks of 16 rows, chunks = ceil(batch / 16); slice g of `slices` holds the chunks
 * [g c, min((g + 1) c, chunks)) with c = ceil(chunks / slices).  Trailing slices may be empty (they contribute zeros).
 * slices = 0 takes qsp_auto_slices(batch) = min(chunks, 128): UNTUNED, one workgroup per compute unit over the two branches.
 * Branches.  pg_loss - ent_coef * entropy touches the policy branch (slots 0 .. 5, 12) alone, vf_coef * vf_loss the value branch
 * (slots 6 .. 11; 0, 1, 8 .. 11 in the shared layout) alone.  Workgroup (g, b) of k_ppo_grad runs branch b over slice g.
 * Forward, per row and branch: quadsim_bc.h's, z[u] = b[u], then fma(w[k][u], in[k], z[u]) for k ascending, ReLU after the two
 * hidden layers, none on the head (mean[4] or the value v).
 * Policy head.  sigma_j = exp(logstd_j) (ocml expf), z_j = (a_j - mean_j) / sigma_j, q = fma(z_j, z_j, q) from 0 over j = 0 .. 3,
 * neglogp = fma(0.5, q, C), C = float32(2 log(2 pi) + logstd_0 + .. + logstd_3) (the sum in float64).  r = exp(old_neglogp -
 * neglogp), rc = min(max(r, float32(1 - cliprange)), float32(1 + cliprange)), p1 = -A * r, p2 = -A * rc.  The row is ACTIVE if
 * p1 >= p2 (a tie goes to the unclipped term, tf.maximum).  dn = active ? (A * r) * float32(1 / batch) : 0;
 * dmean_j = -(dn * z_j) / sigma_j; the row adds dn * (1 - z_j * z_j) (as fma(-(z_j z_j), dn, dn)) to glogstd_j.
 * Value head.  c = float32(cliprange_vf), d = v - old_v; vc = v if cliprange_vf < 0 or -c <= d <= c, else old_v + c (d > c) or
 * old_v - c (d < -c): a value inside the range is v ITSELF, not old_v + (v - old_v), so that an unclipped row ties exactly.
 * l1 = (v - R)^2, l2 = (vc - R)^2; ACTIVE if l1 >= l2; dv = active ? (v - R) * float32(vf_coef / batch) : 0.
 * Backward.  quadsim_bc.h's, under the COMPUTED ReLU masks: dz1[i] = mask ? (fma chain over the head's outputs ascending) : 0;
 * dz0[i] = mask ? ((S0 + S1) + (S2 + S3)) : 0 with S_q the fma chain over o = q, q + 4, .. , q + 124.
 * Partial gradients.  Every element of a branch's tensors: g = 0 (glogstd_j of slice 0: float32(-ent_coef)), then
 * fma(dz[row][o], a[row][i], g) over the slice's rows in ascending order (biases: g + dz[row][o]; rows past the batch add exact
 * zeros).  Written to the workspace as float32, one vector per (slice, branch).
 * Reduction (k_ppo_reduce).  G = float32(sum of the element's partials in float64): the policy branch's slices in ascending
 * order, then the value branch's (both only for w0 and b0 of the shared layout).  Blocks of 256 consecutive elements of the flat
 * parameter vector (slots ascending) add float64(G)^2 in a fixed binary tree.
 * Clip and Adam (k_ppo_apply).  N = sqrt(sum of the blocks' sums in ascending order), float64;  max_grad_norm > 0:
 * G' = G * float32(max_grad_norm / max(N, max_grad_norm)), else G' = G.  Then tf.train.AdamOptimizer's formula exactly as
 * quadsim_bc.h states it, with t = t0 + s + 1 (lr_t is computed on the host in float64 and rounded to float32 once).
 * Statistics.  stats[s] = policy_loss = sum max(p1, p2) / batch, value_loss = sum 0.5 max(l1, l2) / batch,
 * entropy = logstd_0 + .. + logstd_3 + 2 log(2 pi e), approxkl = sum 0.5 (neglogp - old_neglogp)^2 / batch, clipfrac = the share
 * of rows with |r - 1| > float32(cliprange), and N: the rows' float32 terms are added in float64 in ascending order per slice, the
 * slices in ascending order, divided in float64 and rounded once.  All of the weights BEFORE step s.
 * grads (nullable): a HOST array of thirteen device pointers (NULL where the layout has no tensor) that receive G (before the
 * clip) of the LAST step.
 * Invariants: the bits of a call are a function of (net, data, indices, slices, hyper-parameters, t0) alone -- not of the stream,
 * not of which compute unit ran which workgroup, not of n; one call with steps = a + b equals the call with steps = a followed
 * by the call with t0 + a, steps = b, bit for bit, statistics included.
 * NON-FINITE VALUES (NaN, +inf, -inf in a row, a weight or a moment).  A diverged run looks diverged:
 * 1. Statistics.  A statistic of a step is non-finite exactly when float64 torch autograd of the loss of ppo2.py:147-188 over the
 *    same rows, weights and moments makes it non-finite -- torch.relu, torch.clamp, torch.maximum, tf.clip_by_global_norm: what
 *    update="torch" of the package computes.  So every max / min / comparison above is a select that keeps a NaN:
 *    relu = z <= 0 ? 0 : z;  rc = r < lo ? lo : r > hi ? hi : r;  the row is ACTIVE unless p1 < p2, and its term is p1 then (rc
 *    and p2 are NaN only where r and p1 are);  a row that is not active has dn = 0 * r, which is +0 unless r is infinite (the
 *    chain rule through exp, as autograd has it);  a NaN step d = v - old_v gives vc = NaN;  the value row is ACTIVE unless
 *    l1 < l2 and its term is l1 unless l1 < l2 or l2 alone is NaN;  the clip divides by N < max_grad_norm ? max_grad_norm : N,
 *    so a NaN norm makes every element of the step NaN.
 * 2. State.  After a step the policy holds a non-finite weight exactly when the arbiter's does: for the net as a whole, not per
 *    element (the backward masks stay h > 0 ? acc : 0, which turn a NaN activation's term into 0).  The clip and Adam are held
 *    per element: w', m', v' are non-finite in exactly the elements in which the formula above is, applied to the step's own
 *    gradient G; where it is finite the bounds of the finite case apply.
 * 3. Unread data.  Rows that no index of a step names and every step before the first one that reads a non-finite value are
 *    bit for bit what they are without it.  (The advantage's mean and deviation run over all rows of a step: one non-finite
 *    return or value spoils every row of that step.)
 * 4. No faults.  No loaded float becomes an address, an index or a loop bound: no value of any kind makes a call fault or write
 *    outside its arrays.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= steps <= 4096, 1 <= batch < 2^31, 1 <= n < 2^31, 0 <= slices <= 1024, t0 >= 0 and t0 + steps < 2^31; every
 * hyper-parameter finite, cliprange >= 0, 0 <= beta1, beta2 < 1.  Every tensor is 4-byte aligned, the workspace 8-byte; the
 * tensors the call writes (w, m, v, stats, grads, the workspace) may not overlap each other.  A refused call returns an error code,
 * leaves a message in qsp_last_error() and launches nothing.
 */
#ifndef QUADSIM_PPO_H
#define QUADSIM_PPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSP_VERSION 1

enum { QSP_OK = 0, QSP_ERR_INVALID = 1, QSP_ERR_HIP = 2 };

enum { QSP_NET_SHARED_TRUNK = 0, QSP_NET_TOWERS = 1 };

enum { QSP_MAX_STEPS = 4096, QSP_MAX_SLICES = 1024, QSP_TENSORS = 13, QSP_STATS = 6, QSP_CHUNK = 16, QSP_AUTO_SLICES = 128 };

/* the actor-critic and its optimiser state, in the slot order above */
typedef struct QspNet {
    uint32_t struct_size; /* sizeof(QspNet) */
    int32_t layout;       /* QSP_NET_* */
    float *w[13], *m[13], *v[13];
} QspNet;

/* what Runner.run() returns, flattened: n rows */
typedef struct QspBatch {
    uint32_t struct_size; /* sizeof(QspBatch) */
    int32_t reserved;
    int64_t n;
    const float *obs;     /* [n,12] */
    const float *actions; /* [n,4] */
    const float *returns, *values, *neglogp; /* [n] */
} QspBatch;

typedef struct QspHyper {
    uint32_t struct_size; /* sizeof(QspHyper) */
    int32_t reserved;
    double lr, cliprange;
    double cliprange_vf;  /* < 0: no value clipping */
    double ent_coef, vf_coef;
    double max_grad_norm; /* <= 0: no clipping */
    double beta1, beta2, eps;
} QspHyper;

int qsp_version(void);
const char *qsp_last_error(void); /* host string, per thread */

/* the slices qsp_update takes for slices = 0 (0 for batch < 1) */
int qsp_auto_slices(int64_t batch);

/* the workspace of a call with this batch and slices (0 = auto), for any number of steps */
int qsp_workspace_bytes(int64_t batch, int32_t slices, size_t *bytes);

/* `steps` Adam steps; indices [steps,batch] int32 (device), stats [steps,6] float32 (device), t0: Adam steps taken before */
int qsp_update(const QspNet *net, const QspBatch *data, const int32_t *indices, int32_t steps, int64_t batch, int32_t slices,
               const QspHyper *hp, int64_t t0, void *workspace, uint64_t workspace_bytes, float *stats, float *const *grads,
               void *stream);

#ifdef __cplusplus
}
#endif
#endif
