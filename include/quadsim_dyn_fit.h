/* quadsim_dyn_fit.h -- C ABI of libquadsim_dynfit.so: the fit of the LEARNED dynamics net on the device.
 * Dynamic_Net.train_dynamic of MPC-based_RL.py (:120-128) runs `iters` Adam steps on batches drawn from the experience buffer;
 * qsdf_fit runs all of them in ONE kernel launch of ONE workgroup on the caller's stream: the weights stay in LDS for the whole
 * call, the batch passes through in chunks of 16 rows, and nothing synchronises with the host.
 *
 * The library is independent of the other three at link time and shares no host state with them.  The net is given as it is
 * trained, NOT as a packed image: the six weight tensors in torch's Linear layout (out, in), unpadded float32 -- w1 [h1,16],
 * b1 [h1], w2 [h2,h1], b2 [h2], w3 [12,h2], b3 [12] -- each with Adam's first and second moment of the same shape.  All are
 * updated in place.  Every pointer of QsdfNet and of qsdf_fit is a DEVICE pointer unless stated otherwise.  The library
 * allocates nothing and needs no workspace.  C99-clean.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add) ---------------------
 * Batch draw.  Row j of iteration i (Adam step t0 + i) is buffer row
 *     mulhi32(w, size),   w = word 0 of Philox4x32-10 block ((t0 + i) << 32) | j of subsequence (6 << 48) | k under `seed`
 * (the generator of quadsim_device.hpp's philox_counter; 6 is the fit's own stream).  Rows are drawn WITH replacement, as
 * the `randint` of examples/mpc_learned.py draws them; the reference's random.sample draws without.  The key holds t0 + i,
 * not i: a fit split into two calls draws the rows of one call, and fewer rows are a prefix of more.  With `indices`
 * [iters,batch] given, row j of iteration i is indices[i][j] and nothing is drawn; entries outside [0, size) are UNDEFINED
 * BEHAVIOUR (they are not checked on the device).
 * Forward, per row.  xh = (x - in_mean) * in_rscale (two operations); z1[u] = b1[u], then z1[u] = fma(w1[u][k], xh[k], z1[u])
 * for k = 0 .. 15 ascending; a1 = max(z1, 0); z2 and a2 likewise over k = 0 .. h1-1; y over k = 0 .. h2-1 without the ReLU:
 * word for word the model step of quadsim_dyn.h, so the net the planners run is the net that was fitted.  Target
 * th = (d - out_mean) * out_rscale (two operations), out_rscale = float32(1 / (out_std + 1e-6)) computed in float64.
 * Loss = tf.reduce_mean(tf.square(predict - delta)): e = y - th; s_row = fma(e[o], e[o], s_row) from 0 for o = 0 .. 11;
 * S = S + s_row over the rows of the batch in ascending order from 0; loss[i] = S / (12 batch)  (the weights BEFORE step i).
 * Backward.  dy = e * float32(2 / (12 batch)) (the constant computed in float64).  ReLU mask: the COMPUTED pre-activation,
 * z > 0.  dz2[i] = mask2[i] ? (acc = 0; acc = fma(w3[o][i], dy[o], acc), o = 0 .. 11 ascending) : 0;
 * dz1[i] = mask1[i] ? (the same over w2[o][i], dz2[o], o = 0 .. h2-1) : 0.
 * Gradients: gW[o][i] = 0, then gW[o][i] = fma(dz[row][o], a[row][i], gW[o][i]) over the rows of the batch in ascending
 * order (a = xh, a1, a2 for the three layers, dz = dz1, dz2, dy); gb[o] = gb[o] + dz[row][o] likewise.  The bits of an
 * iteration therefore depend on the net, the rows and `batch` alone.
 * Adam: tf.train.AdamOptimizer's formula.  With t = t0 + i + 1,
 *     lr_t = float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t))      (float64 pow, sqrt and division, rounded to float32 once)
 *     m' = fma(B1, m, C1 * g)          B1 = float32(beta1), C1 = float32(1 - beta1)  (the difference in float64)
 *     v' = fma(B2, v, C2 * (g * g))    B2 = float32(beta2), C2 = float32(1 - beta2)
 *     w' = w - (lr_t * m') / (sqrt(v') + E)      E = float32(eps); sqrt and the division correctly rounded
 * torch.optim.Adam divides by sqrt(v' / (1 - beta2^t)) + eps instead: eps sits in a different place, and the two optimisers
 * are not bit-comparable (they agree to first order in eps).
 * Outputs.  loss [iters]; indices_out [iters,batch] int32 (nullable): the rows used; grads (nullable): a HOST array of six
 * device pointers, which receive the six gradients of the LAST iteration in the weights' own layout.
 * Invariants: one call with iters = a + b equals the call with iters = a followed by the call with t0 + a, iters = b, bit
 * for bit in weights, moments and losses; units padded with zero weights (in and out) have exactly zero gradient and stay zero.
 * NON-FINITE VALUES (NaN, +inf, -inf in a row, a weight or a moment).  A diverged run looks diverged:
 * 1. Statistics.  The loss of a step is non-finite exactly when float64 torch autograd over the same rows, weights and moments
 *    makes it non-finite (torch.relu, the mean squared error, tf.train.AdamOptimizer's formula).  So relu is a select that keeps
 *    a NaN, relu = z <= 0 ? 0 : z, never a max that drops one.
 * 2. State.  After a step the net holds a non-finite weight exactly when the arbiter's does: for the net as a whole, not per
 *    element (the backward masks stay h > 0 ? acc : 0, which turn a NaN activation's term into 0).  Adam is held per element:
 *    w', m', v' are non-finite in exactly the elements in which the formula above is, applied to the step's own gradient; where
 *    it is finite the bounds of the finite case apply.
 * 3. Unread data.  Rows that no index of a step names and every step before the first one that reads a
 *    non-finite value are bit for bit what they are without it.
 * 4. No faults.  No loaded float becomes an address, an index or a loop bound: no value of any kind makes a call fault or write
 *    outside its arrays.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * Hidden widths as in quadsim_dyn.h: (h1, h2) runs on the first of the compiled pairs (64, 64), (128, 128), (208, 112) that
 * covers it.  1 <= batch <= 256, 1 <= iters <= 4096, 1 <= size <= capacity < 2^31, t0 >= 0 and t0 + iters < 2^31, k < 2^48,
 * lr, beta1, beta2 and eps finite, 0 <= beta1, beta2 < 1.  Every tensor is 4-byte aligned; none may overlap another.
 * A refused call returns an error code, leaves a message in qsdf_last_error() and launches nothing.
 */
#ifndef QUADSIM_DYN_FIT_H
#define QUADSIM_DYN_FIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSDF_VERSION 1

enum { QSDF_OK = 0, QSDF_ERR_INVALID = 1, QSDF_ERR_HIP = 2, QSDF_ERR_UNSUPPORTED = 3 };

enum { QSDF_MAX_BATCH = 256, QSDF_MAX_ITERS = 4096 };

/* the net and its optimiser state; w, m, v in the order w1, b1, w2, b2, w3, b3 */
typedef struct QsdfNet {
    uint32_t struct_size; /* sizeof(QsdfNet) */
    int32_t h1, h2, reserved;
    float *w[6], *m[6], *v[6];
    const float *in_mean, *in_rscale; /* [16] */
    const float *out_mean, *out_rscale; /* [12] */
} QsdfNet;

int qsdf_version(void);
const char *qsdf_last_error(void); /* host string, per thread */

/* `iters` Adam steps of batch `batch` on rows of buf_x [capacity,16] (observation and action) / buf_d [capacity,12] (delta),
 * of which the first `size` are valid.  t0: Adam steps taken before this call; k: the fit counter that keys the draws. */
int qsdf_fit(const QsdfNet *net, const float *buf_x, const float *buf_d, int64_t capacity, int64_t size, int32_t iters, int32_t batch,
             double lr, double beta1, double beta2, double eps, int64_t t0, uint64_t seed, uint64_t k, const int32_t *indices,
             float *loss, int32_t *indices_out, float *const *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif
