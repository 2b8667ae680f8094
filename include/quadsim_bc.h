/* quadsim_bc.h -- C ABI of libquadsim_bc.so: behaviour cloning of the actor on the device.
 * SB2's BaseRLModel.pretrain (run_pretrained_ppo2_docking.py:50-69) regresses the policy's deterministic action onto the expert's
 * with many small Adam steps.  qsbc_fit runs `steps` of them in ONE kernel launch of ONE workgroup on the caller's stream: the
 * weights stay in LDS and Adam's moments in registers for the whole call, the minibatch passes through in chunks of 16 rows, and
 * nothing synchronises with the host.  qsbc_loss is the forward-only validation pass over many workgroups.
 *
 * The library is independent of the other four at link time and shares no host state with them.  The net is the actor of
 * quadsim_amd/sb2.py, either layout: 12 -> 128 -> 128 -> 4 with ReLU, given as it is stored, NOT as a packed image: six float32
 * tensors in the policy's (in, out) layout -- w0 [12,128], b0 [128], w1 [128,128], b1 [128], w2 [128,4], b2 [4] -- each with
 * Adam's first and second moment of the same shape.  All eighteen are updated in place.  Every pointer is a DEVICE pointer
 * unless stated otherwise.  The library allocates nothing.  C99-clean.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add) ---------------------
 * Rows.  Step s (Adam step t0 + s) uses dataset rows indices[s][0 .. rows-1], rows = counts[s] (counts == NULL: batch).  Entries
 * at or beyond counts[s] are never read.  Nothing is drawn on the device.  Entries outside [0, n) and counts outside [1, batch]
 * are UNDEFINED BEHAVIOUR (not checked on the device; a count above batch is read as batch).
 * Forward, per row.  z0[u] = b0[u], then z0[u] = fma(w0[k][u], obs[k], z0[u]) for k = 0 .. 11 ascending (the kernel pads the row
 * with four zero inputs 12 .. 15 against zero weights: they contribute exactly nothing); a0 = max(z0, 0); z1 and a1 likewise
 * over k = 0 .. 127; the mean action y[o] = b2[o], then fma(w2[k][o], a1[k], y[o]) over k = 0 .. 127, no ReLU, no clamp, no tanh.
 * Loss = SB2's continuous-action pretrain loss, mean((a_expert - mean_action)^2) over rows x 4: e = y - a_expert;
 * s_row = fma(e[o], e[o], s_row) from 0 for o = 0 .. 3; S = S + s_row over the rows in ascending order from 0;
 * loss[s] = S / float32(4 rows)  (the weights BEFORE step s).
 * Backward.  dy = e * float32(2 / (4 rows)) (the constant computed in float64).  ReLU mask: the COMPUTED pre-activation, z > 0.
 * dz1[i] = mask1[i] ? (acc = 0; acc = fma(w2[i][o], dy[o], acc), o = 0 .. 3 ascending) : 0.
 * dz0[i] = mask0[i] ? ((S0 + S1) + (S2 + S3)) : 0, where S_q = (acc = 0; acc = fma(w1[i][o], dz1[o], acc) over o = q, q + 4,
 * q + 8, .. , q + 124 ascending): four interleaved chains, added in that fixed tree.
 * Gradients: gW[i][o] = 0, then gW[i][o] = fma(dz[row][o], a[row][i], gW[i][o]) over the rows of the step in ascending order
 * (a = obs, a0, a1 for the three layers, dz = dz0, dz1, dy); gb[o] = gb[o] + dz[row][o] likewise.  A step's rows are padded to a
 * multiple of 16 with rows whose dy is zero: they add fma(0, a, g) = g and g + 0.  The bits of a step therefore depend on the
 * net, its rows and counts[s] alone -- not on `batch`, not on the other steps of the launch.
 * Adam: tf.train.AdamOptimizer's formula, exactly as quadsim_dyn_fit.h states it.  With t = t0 + s + 1,
 *     lr_t = float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t))      (float64 pow, sqrt and division, rounded to float32 once)
 *     m' = fma(B1, m, C1 * g)          B1 = float32(beta1), C1 = float32(1 - beta1)  (the difference in float64)
 *     v' = fma(B2, v, C2 * (g * g))    B2 = float32(beta2), C2 = float32(1 - beta2)
 *     w' = w - (lr_t * m') / (sqrt(v') + E)      E = float32(eps), added OUTSIDE the square root; sqrt and the division
 *                                                correctly rounded
 * Outputs.  loss [steps]; grads (nullable): a HOST array of six device pointers, which receive the six gradients of the LAST
 * step in the weights' own layout.
 * Invariants: the same inputs give the same bits on any stream; one call with steps = a + b equals the call with steps = a
 * followed by the call with t0 + a, steps = b, bit for bit in weights, moments and losses; a step with counts[s] = c in a launch
 * of any batch >= c equals the same step in a launch with batch = c.
 *
 * qsbc_loss.  The same forward and s_row over the rows rows[0 .. count-1] (rows == NULL: rows 0 .. count-1 of the dataset).  Block
 * b holds list positions [256 b, 256 b + 256): its partial is the float64 sum of its s_row values (each float32, widened) in
 * ascending order from 0, written to partials[b] by whichever workgroup reaches the block.  A second launch of one workgroup adds
 * partials[0 .. blocks-1] in ascending order in float64 and writes out[0] = sum / (4 count) (float64).  The result does not
 * depend on `grid` (the number of workgroups of the first launch; 0 = the library's choice).
 * NON-FINITE VALUES in qsbc_fit (NaN, +inf, -inf in a row, a weight or a moment).  A diverged run looks diverged:
 * 1. Statistics.  The loss of a step is non-finite exactly when float64 torch autograd over the same rows, weights and moments
 *    makes it non-finite (torch.relu, the mean squared error, tf.train.AdamOptimizer's formula).  So relu is a select that keeps
 *    a NaN, relu = z <= 0 ? 0 : z, never a max that drops one.
 * 2. State.  After a step the net holds a non-finite weight exactly when the arbiter's does: for the net as a whole, not per
 *    element (the backward masks stay h > 0 ? acc : 0, which turn a NaN activation's term into 0).  Adam is held per element:
 *    w', m', v' are non-finite in exactly the elements in which the formula above is, applied to the step's own gradient; where
 *    it is finite the bounds of the finite case apply.
 * 3. Unread data.  Rows that no index of a step names, index entries at and beyond counts[s] and every step before the first
 *    one that reads a non-finite value are bit for bit what they are without it.
 * 4. No faults.  No loaded float becomes an address, an index or a loop bound: no value of any kind makes a call fault or write
 *    outside its arrays.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= batch <= 256, 1 <= counts[s] <= batch, 1 <= steps <= 4096, 1 <= n < 2^31, t0 >= 0 and t0 + steps < 2^31; lr, beta1,
 * beta2 and eps finite, 0 <= beta1, beta2 < 1.  qsbc_loss: 1 <= count < 2^31 (rows == NULL: count <= n), 0 <= grid <= 65535,
 * partials holds qsbc_loss_blocks(count) doubles.  Every tensor is 4-byte aligned (partials and out 8-byte); none may overlap
 * another: the eighteen tensors of the net, loss and the gradients are checked against each other, the rest is the caller's.
 * A refused call returns an error code, leaves a message in qsbc_last_error() and launches nothing.
 */
#ifndef QUADSIM_BC_H
#define QUADSIM_BC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSBC_VERSION 1

enum { QSBC_OK = 0, QSBC_ERR_INVALID = 1, QSBC_ERR_HIP = 2 };

enum { QSBC_MAX_BATCH = 256, QSBC_MAX_STEPS = 4096, QSBC_LOSS_BLOCK = 256 };

/* the actor and its optimiser state; w, m, v in the order w0, b0, w1, b1, w2, b2 */
typedef struct QsbcNet {
    uint32_t struct_size; /* sizeof(QsbcNet) */
    int32_t reserved;
    float *w[6], *m[6], *v[6];
} QsbcNet;

int qsbc_version(void);
const char *qsbc_last_error(void); /* host string, per thread */

/* `steps` Adam steps on rows of obs [n,12] / act [n,4] chosen by indices [steps,batch] and counts [steps] (nullable).
 * t0: Adam steps taken before this call. */
int qsbc_fit(const QsbcNet *net, const float *obs, const float *act, int64_t n, const int32_t *indices, const int32_t *counts,
             int32_t steps, int32_t batch, double lr, double beta1, double beta2, double eps, int64_t t0, float *loss,
             float *const *grads, void *stream);

/* the number of partials qsbc_loss writes for `count` rows (0 for count < 1) */
int64_t qsbc_loss_blocks(int64_t count);

/* w: a HOST array of the six device pointers of the weights.  out [1] float64 = mean((a_expert - mean_action)^2). */
int qsbc_loss(const float *const *w, const float *obs, const float *act, int64_t n, const int32_t *rows, int64_t count,
              double *partials, double *out, int32_t grid, void *stream);

#ifdef __cplusplus
}
#endif
#endif
