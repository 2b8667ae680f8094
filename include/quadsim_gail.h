/* quadsim_gail.h -- C ABI of libquadsim_gail.so: the discriminator of GAIL on the device.
 * SB2's TransitionClassifier (run_docking_gail.py trains it against the PID expert's ExpertDataset) is a small net that tells
 * the policy's transitions (label 0, "generator") from the expert's (label 1) and whose output is the reward the policy is
 * trained on.  qsg_fit runs `steps` Adam steps of it in ONE kernel launch of ONE workgroup on the caller's stream: the weights
 * stay in LDS for the whole call, the rows pass through in chunks of 16, nothing synchronises with the host.  qsg_reward is the
 * forward-only pass over every row of a roll-out, on the exact-float32 matrix pipe over many workgroups.
 *
 * The library is independent of the other six at link time and shares no host state with them.  The net is
 * D(obs[12], act[4]) -> logit: 16 -> H -> H -> 1 with tanh after both hidden layers, 1 <= H <= 128, given as it is stored, NOT as a
 * packed image: six float32 tensors in the policy's (in, out) layout -- w0 [16,H], b0 [H], w1 [H,H], b1 [H], w2 [H,1], b2 [1] --
 * each with Adam's first and second moment of the same shape; qsg_fit updates all eighteen in place.  The kernels run on the first
 * compiled width W that covers H, 64 or 128; units H .. W-1 exist in LDS only, with zero weights: they give tanh(0) = 0, receive
 * no gradient and never reach memory.  Every pointer is a DEVICE pointer unless stated otherwise.  The library allocates
 * nothing.  C99-clean.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add) ---------------------
 * Input, per row.  x[k] = (obs[k] - mean[k]) * rscale[k] for k = 0 .. 11 (a subtraction, then a multiplication);
 * x[12 + k] = min(max(act[k], -1), 1) for k = 0 .. 3: generator and expert actions pass the same clamp.  mean and rscale [12]
 * are fixed for a call.
 * tanh.  (a, d) = (tanh z, 1 - tanh^2 z) is q_tanh of csrc/quadsim_device.hpp: e = exp2(min(2 |z|, 60) log2 e), r = 1 / (e + 1)
 * on the hardware's exp2 and reciprocal, a = copysign(1 - 2 r, z), d = 4 (e r) r.  exp, log and log1p are the device library's
 * expf, logf and log1pf.  tests/gail_ref.py holds the measured error of each as a constant of its bounds.
 *
 * qsg_fit.  Step s (Adam step t0 + s) uses c = counts[s] rows per class (counts == NULL: batch): generator rows
 * gen_idx[s][0 .. c-1] of gen_obs / gen_act, then expert rows exp_idx[s][0 .. c-1] of exp_obs / exp_act.  Entries at or beyond c are
 * never read.  Nothing is drawn on the device.  Entries outside [0, n) and counts outside [1, batch] are UNDEFINED BEHAVIOUR (not
 * checked on the device; a count above batch is read as batch).
 * Forward, per row.  z0[u] = b0[u], then z0[u] = fma(w0[k][u], x[k], z0[u]) for k = 0 .. 15 ascending; (a0, d0) = tanh;
 * z1, a1, d1 likewise over k = 0 .. H-1; the logit l = b2, then l = fma(w2[k], a1[k], l) over k = 0 .. H-1 ascending.
 * Loss terms, per row.  e = exp(-|l|); p = log1p(e); D = 1 + e; s+ = 1 / D, s- = e / D (two divisions);
 * sigmoid(l) = s = (l >= 0 ? s+ : s-), sigmoid(-l) = n = (l >= 0 ? s- : s+); softplus(l) = max(l, 0) + p, softplus(-l) = max(-l, 0) + p;
 * the row's entropy h = fma(n, l, softplus(-l))  (SB2's logit_bernoulli_entropy).
 * Statistics of step s, from the weights BEFORE the step, into stats[s][0 .. 4]; every sum runs from 0 over the rows in the fixed
 * order "all generator rows ascending, then all expert rows ascending", R = float32(c):
 *     gen_loss = (sum over generator rows of softplus(l)) / R        exp_loss = (sum over expert rows of softplus(-l)) / R
 *     entropy  = (sum over all 2 c rows of h) / float32(2 c)
 *     gen_acc  = (number of generator rows with l < 0) / R           exp_acc = (number of expert rows with l > 0) / R
 * The loss that is minimised is total = gen_loss + exp_loss - entcoeff * entropy.
 * Backward.  I = float32(1 / c), K = float32(entcoeff / (2 c)) (both computed in float64).  dl = fma(K, (s * n) * l, base) with
 * base = s * I on a generator row and base = -(n * I) on an expert row.
 * dz1[i] = d1[i] * (w2[i] * dl).  dz0[i] = d0[i] * acc, acc = 0, then acc = fma(w1[i][o], dz1[o], acc) over o = 0 .. H-1 ascending.
 * Gradients: gW[i][o] = 0, then gW[i][o] = fma(dz[row][o], a[row][i], gW[i][o]) over the rows of the step in the fixed order
 * (a = x, a0, a1 for the three layers, dz = dz0, dz1, dl); gb[o] = gb[o] + dz[row][o] likewise.  Each class's rows are padded to a
 * multiple of 16 with rows whose dl is zero: they add fma(0, a, g) = g and g + 0.  The bits of a step therefore depend on the net,
 * its rows and counts[s] alone -- not on `batch`, not on the other steps of the launch.
 * Adam: tf.train.AdamOptimizer's formula, exactly as quadsim_dyn_fit.h states it.  With t = t0 + s + 1,
 *     lr_t = float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t))      (float64 pow, sqrt and division, rounded to float32 once)
 *     m' = fma(B1, m, C1 * g)          B1 = float32(beta1), C1 = float32(1 - beta1)  (the difference in float64)
 *     v' = fma(B2, v, C2 * (g * g))    B2 = float32(beta2), C2 = float32(1 - beta2)
 *     w' = w - (lr_t * m') / (sqrt(v') + E)      E = float32(eps), added OUTSIDE the square root; sqrt and the division
 *                                                correctly rounded
 * grads (nullable): a HOST array of six device pointers, which receive the six gradients of the LAST step in the weights' own
 * layout.
 * Invariants: the same inputs give the same bits on any stream; one call with steps = a + b equals the call with steps = a
 * followed by the call with t0 + a, steps = b, bit for bit in weights, moments and statistics; a step with counts[s] = c in a
 * launch of any batch >= c equals the same step in a launch with batch = c.
 *
 * qsg_reward.  The same input row.  The three layers run as v_mfma_f32_16x16x4_f32 tiles, rows on the columns: a pre-activation
 * starts from its bias and takes its inputs four at a time, k = 4 j .. 4 j + 3 for j ascending, the four products of a group added
 * to the running sum in the instruction's own fixed order (float32 products and sums; not the fit's fma chain, so the logit is
 * NOT promised bit-equal to the fit's forward: it is within the same derived bound).  tanh as above.
 * q = 1 / (1 + exp(l)) (an addition, a division); reward = -log(q + 1e-8f): the reference's -log(1 - sigmoid(l) + 1e-8) without
 * the cancellation of 1 - s.  reward [rows], and logits [rows] where that pointer is not NULL.  With n_envs, n_steps > 0 (then
 * rows must be n_envs * n_steps) input row e * n_steps + t is written to output element t * n_envs + e: an env-major roll-out in,
 * the step-major [n_steps, n_envs] array of qs_gae_flatten out.  With n_envs = n_steps = 0 row i is written to element i.  A row's
 * bits depend on the net and that row alone: not on `grid` (the number of workgroups; 0 = the library's choice), not on the
 * rows beside it, not on the stream.
 *
 * qsg_math is the tests' window on the four device functions above: y[i] = f(x[i]), kind 0 tanh, 1 its 1 - tanh^2, 2 exp,
 * 3 log, 4 log1p, computed by the same device functions the two kernels inline.
 *
 * NON-FINITE VALUES (NaN, +inf, -inf in a row, mean or rscale, a weight or a moment).  A diverged run looks diverged:
 * 1. Statistics.  A statistic of a step of qsg_fit is non-finite exactly when float64 torch autograd over the same rows, weights
 *    and moments makes it non-finite (torch.clamp on the actions, torch.tanh, the loss above, tf.train.AdamOptimizer's formula:
 *    what torch_discriminator_fit of the package computes); a reward and a logit of qsg_reward exactly in the rows in which
 *    torch's are.  So the clamp and tanh keep a NaN: x[12 + k] = act < -1 ? -1 : act > 1 ? 1 : act, and (a, d) = (NaN, NaN) for
 *    z = NaN, where q_tanh alone would give (+-1, 0).  (The two accuracies count comparisons, which are false for a NaN: they
 *    stay finite on both sides.)  NOT COVERED: an infinite logit (an infinite weight of the last layer), where torch's
 *    binary_cross_entropy_with_logits returns NaN for the class whose softplus is 0.
 * 2. State.  After a step the discriminator holds a non-finite weight exactly when the arbiter's does.  Adam is held per
 *    element: w', m', v' are non-finite in exactly the elements in which the formula above is, applied to the step's own
 *    gradient; where it is finite the bounds of the finite case apply.
 * 3. No invention.  An infinite action is its clamped copy, bit for bit, in qsg_fit and in qsg_reward; a NaN is never clamped
 *    away.  (An infinite observation saturates tanh: every statistic stays finite, as it does in the arbiter.)
 * 4. Unread data.  Rows that no index of a step names, index entries at and beyond counts[s], and every step before the first
 *    one that reads a non-finite value are bit for bit what they are without it; in qsg_reward every row but the poisoned one.
 * 5. No faults.  No loaded float becomes an address, an index or a loop bound: no value of any kind makes a call fault or write
 *    outside its arrays.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= H <= 128; 1 <= batch <= 256 rows per class, 1 <= counts[s] <= batch, 1 <= steps <= 4096, 1 <= n_gen, n_exp < 2^31, t0 >= 0
 * and t0 + steps < 2^31; entcoeff, lr and eps finite, 0 <= beta1, beta2 < 1.  qsg_reward: 1 <= rows < 2^31, n_envs and n_steps both
 * 0 or both >= 1 with n_envs * n_steps == rows, 0 <= grid <= 65535.  Every tensor is 4-byte aligned; none that is written may
 * overlap another: the eighteen tensors of the net, stats and the gradients are checked against each other (qsg_reward: reward
 * and logits), the rest is the caller's.  A refused call returns an error code, leaves a message in qsg_last_error() and
 * launches nothing.
 */
#ifndef QUADSIM_GAIL_H
#define QUADSIM_GAIL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSG_VERSION 1

enum { QSG_OK = 0, QSG_ERR_INVALID = 1, QSG_ERR_HIP = 2 };

enum { QSG_MAX_HIDDEN = 128, QSG_MAX_BATCH = 256, QSG_MAX_STEPS = 4096, QSG_STATS = 5 };

/* the discriminator and its optimiser state; w, m, v in the order w0, b0, w1, b1, w2, b2.  qsg_reward reads w, mean and
 * rscale only: m and v may be NULL there. */
typedef struct QsgNet {
    uint32_t struct_size; /* sizeof(QsgNet) */
    int32_t hidden;       /* H */
    float *w[6], *m[6], *v[6];
    const float *mean, *rscale; /* [12] each */
} QsgNet;

int qsg_version(void);
const char *qsg_last_error(void); /* host string, per thread */

/* `steps` Adam steps.  gen_obs [n_gen,12] / gen_act [n_gen,4]: the roll-out; exp_obs [n_exp,12] / exp_act [n_exp,4]: the expert;
 * gen_idx, exp_idx [steps,batch], counts [steps] (nullable); stats [steps,5]; t0: Adam steps taken before this call. */
int qsg_fit(const QsgNet *net, const float *gen_obs, const float *gen_act, int64_t n_gen, const float *exp_obs, const float *exp_act,
            int64_t n_exp, const int32_t *gen_idx, const int32_t *exp_idx, const int32_t *counts, int32_t steps, int32_t batch,
            double entcoeff, double lr, double beta1, double beta2, double eps, int64_t t0, float *stats, float *const *grads,
            void *stream);

/* reward [rows] and, where not NULL, logits [rows] of obs [rows,12] / act [rows,4] */
int qsg_reward(const QsgNet *net, const float *obs, const float *act, int64_t rows, int64_t n_envs, int64_t n_steps, float *reward,
               float *logits, int32_t grid, void *stream);

/* y[i] = f(x[i]) for i < n, 1 <= n < 2^31; kind 0 .. 4 as above */
int qsg_math(int32_t kind, const float *x, float *y, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
