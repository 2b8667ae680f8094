/* quadsim_trpo.h -- C ABI of libquadsim_trpo.so: one TRPO update on the device.
 * Stable-Baselines 2's TRPO (which its GAIL subclasses) is third-party code outside the reference tree, so this header restates it
 * as a numerical contract: a conjugate-gradient natural-gradient step of the policy tower with a KL line search (qst_policy_step),
 * then Adam steps of the value tower on mean((v - R)^2) (qst_vf_fit).  Both enqueue a fixed sequence of launches on the caller's
 * stream.  The kernel boundary is the only ordering across workgroups: no grid-wide barrier, no workgroup waits for another, no
 * floating-point atomics.  Nothing synchronises with the host; the library allocates nothing (the caller passes a workspace).
 *
 * The library is independent of the other eight at link time and shares no host state with them.  The net is the actor-critic of
 * quadsim_ppo.h in the TOWERS layout only, thirteen float32 tensors in the policy's (in, out) layout in the slots
 *     0 w0 [12,128]  1 b0 [128]  2 w1 [128,128]  3 b1 [128]  4 w2 [128,4]  5 b2 [4]  6 wv0 [12,128]  7 bv0 [128]
 *     8 wv1 [128,128]  9 bv1 [128]  10 wv2 [128,1]  11 bv2 [1]  12 logstd [4]
 * The policy step owns slots 0 .. 5 and 12; flattened in that order they are the vector theta of P = 18 696 elements (w0 at 0,
 * b0 at 1536, w1 at 1664, b1 at 18048, w2 at 18176, b2 at 18688, logstd at 18692).  The value fit owns slots 6 .. 11 and their
 * Adam moments m, v (the moments of the other slots are not read).  The shared-trunk layout is refused: in SB2 its shared layers
 * would belong to both optimisers.  Every pointer is a DEVICE pointer unless stated otherwise.  C99-clean.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add; fl = one rounding) ----------
 * DOT(a, b): the products float64(a_e) float64(b_e) of blocks of 256 consecutive elements (the last padded with zeros) are added in
 * float64 in the binary tree t += t[e + h], h = 128, 64 .. 1; the blocks' sums are added in ascending order from 0.
 *
 * qst_policy_step, over the rows 0 .. n-1 of the roll-out (there are no indices):
 * 1. Advantages.  d_i = fl(returns_i - values_i); mean, var, R = float32(1 / (sqrt(var) + 1e-8)) and A_i = fl(fl(d_i - mean) R)
 *    exactly as quadsim_ppo.h has them (thread i of 256 adds the elements i, i + 256, .. in float64, a fixed binary tree).
 * 2. Gradient pass, all rows.  The rows are cut into chunks of 16 and the chunks into `slices` as in quadsim_ppo.h (slices = 0:
 *    qst_auto_slices(n) = min(chunks, 128), UNTUNED).  Forward: quadsim_bc.h's chain.  sigma_j = expf(logstd_j),
 *    z_j = fl(fl(a_j - mean_j) / sigma_j), q = fma(z_j, z_j, q) from 0, neglogp = fma(0.5, q, C) with C of quadsim_ppo.h.  The
 *    workspace keeps mean [n,4] and neglogp [n]: the OLD policy is the policy at entry (SB2's assign_old_eq_new).
 *    dn = fl(A_i float32(1 / n)); dmean_j = fl(fl(dn z_j) / sigma_j); the row adds fma(fl(z_j z_j), dn, -dn) to glogstd_j, which
 *    starts at float32(entcoeff) in slice 0.  Backward and partial gradients: quadsim_ppo.h's, under the computed ReLU masks.
 *    g = float32(the float64 sum of an element's partials, slices ascending): the gradient of the surrogate
 *    mean(A_i exp(nlp_old_i - neglogp_i)) + entcoeff entropy.  surr_before = sum A_i / n + entcoeff entropy in float64 (the rows'
 *    float32 A_i added per slice in ascending order, the slices ascending), entropy = sum logstd_j + 2 log(2 pi e) in float64.
 *    rdotr = DOT(g, g).  rdotr == 0 SKIPS the update: nothing of the net is written, stats[8] = -2.  (SB2 tests np.allclose(g, 0);
 *    the exact test is the documented deviation.  A batch of one row or of equal advantages with entcoeff = 0 is skipped.)
 * 3. Fisher-vector product F v, the Hessian of mean KL(old || new) at new = old over the rows 0, s, 2s, .. (s = fvp_stride,
 *    n_f = ceil(n / s) rows, chunks of 16 of THOSE rows, the same slices): per row h0, h1 and their masks are recomputed; the
 *    tangent t0[u] = mask0 ? (acc = vb0[u]; fma(V0[k][u], x[k], acc), k ascending) : 0;
 *    t1[u] = mask1 ? (acc = vb1[u]; fma(V1[k][u], h0[k], acc) over k, then fma(w1[k][u], t0[k], acc) over k) : 0;
 *    tmu[o] = (acc = vb2[o]; fma(V2[k][o], h1[k], acc) over k, then fma(w2[k][o], t1[k], acc) over k), V the tensors of v;
 *    dmu_o = fl(fl(tmu_o / fl(sigma_o sigma_o)) float32(1 / n_f)); then step 2's backward from dmu.  Fv_e = float32(the float64 sum of
 *    the partials, slices ascending; on the four logstd elements plus 2 float64(v_e)), z_e = fma(float32(cg_damping), v_e, Fv_e).
 * 4. Conjugate gradient (SB2's cg): x = 0, r = p = g.  Iteration k = 0 .. cg_iters-1: z = (F + damping) p;
 *    alpha = float32(rdotr / DOT(p, z)); x_e = fma(alpha, p_e, x_e); r_e = fma(-alpha, z_e, r_e); rdotr' = DOT(r, r);
 *    mu = float32(rdotr' / rdotr); p_e = fma(mu, p_e, r_e); rdotr = rdotr'.  Once rdotr < residual_tol (SB2: 1e-10) the launches of
 *    the remaining iterations return at once: they read a device flag at entry.  The scalars live on the device.
 * 5. Step.  z = (F + damping) x (the cg_iters + 1-th product, always trace row cg_iters); shs = 0.5 DOT(x, z);
 *    lm = float32(sqrt(shs / max_kl)); fullstep_e = fl(x_e / lm); expected_improve = DOT(g, fullstep).
 * 6. Line search, candidates k = 0 .. backtracks-1: theta_k = fl(theta_old + fl(fullstep 2^-k)).  A forward-only pass over ALL rows:
 *    neglogp_k as in 2; the row's terms fl(A_i expf(fl(nlp_old_i - neglogp_k,i))) and
 *    kl = (acc = 0; acc = fl(acc + fl(fl(fl(ls_k,j - ls_old,j) + fl(fma(d, d, fl(sigma_old,j^2)) / fl(2 fl(sigma_k,j^2)))) - 0.5)), j = 0 .. 3),
 *    d = fl(mean_old,j - mean_k,j), added in float64 like surr_before: surr_k = sum / n + entcoeff entropy_k, kl_k = sum / n.
 *    The first k with surr_k and kl_k finite, kl_k <= 1.5 max_kl and surr_k - surr_before >= 0 (float64) is written to the policy;
 *    the launches of later candidates return at once.  If none is accepted the policy keeps theta_old bit for bit.  A non-finite
 *    g, x or shs therefore ends in a rejected step, never in a fault: no loaded float becomes an address, an index or a loop bound.
 * 7. stats[10] (rounded to float32 once): surr_before, surr_after, kl_after (of the accepted candidate; surr_before and 0 without
 *    one), entropy of the policy at return, |g| = sqrt(rdotr at entry), shs, lm, expected_improve, the accepted k (-1: none, -2:
 *    skipped), CG iterations run.  A skipped call writes stats 0, 1, 3, 4, 8 and zeros elsewhere.
 * The bits of a call are a function of (net, data, slices, hyper-parameters) alone: not of the stream, of the placement of the
 * workgroups or of the trace being requested.
 *
 * qst_vf_fit: `steps` Adam steps in ONE launch of ONE workgroup, the value tower in LDS.  Step s takes the rows indices[s][0 ..
 * batch-1] (a DEVICE array: entries outside [0, n) are undefined behaviour) in chunks of 16, rows ascending: quadsim_bc.h's forward
 * with a head one unit wide, e = fl(v - R), dv = fl(e float32(2 / batch)), quadsim_bc.h's backward, gradients and Adam formula with
 * t = t0 + s + 1 (MpiAdam's is the same formula).  stats[s] = fl((sum over the rows, ascending, of fl(e e)) / float32(batch)): the
 * loss of the weights BEFORE step s.  A call of a + b steps equals the call of a steps followed by the call of b steps with
 * t0 + a, bit for bit.  grads (nullable): a HOST array of six device pointers that receive the gradients of the LAST step.
 *
 * NON-FINITE VALUES (NaN, +inf, -inf in a row, a weight or a moment).  The five rules of quadsim_ddpg.h apply (statistics; state;
 * no invention; unread data; no faults).  For qst_policy_step the arbiter is float64 torch autograd of steps 1 to 7 (torch.relu,
 * the surrogate as mean(A_i exp(nlp_old_i - neglogp_i)) + entcoeff entropy, F v as double backprop of the mean KL, SB2's cg and
 * line search), what update="torch" of the package computes:
 * 1. Statistics.  A statistic is non-finite exactly when the arbiter's is, with ONE documented deviation: surr_before is the
 *    formula of step 2, sum A_i / n + entcoeff entropy, which does not read neglogp.  It is finite whenever the advantages, logstd
 *    and entcoeff entropy are finite, also where a row's neglogp is not (a NaN observation, action or policy weight), where
 *    autograd's mean(A_i exp(nlp_old_i - neglogp_i)) is NaN.  surr_after of a rejected step is surr_before, and the deviation
 *    applies to it in the same way.  Non-finite returns or values make every advantage, and with it surr_before, NaN on both.
 * 2. State.  A step with a non-finite g, x, shs or lm is a REJECTED step.  CG runs all cg_iters products (rdotr < residual_tol is
 *    false for a NaN), the cg_iters + 1-th product and every candidate are evaluated and, where a trace is given, written to every
 *    row of it; accepted = -1, kl_after = 0, entropy is the old policy's, cg_iters_run = cg_iters.  Theta, the value tower and all
 *    moments keep their bits; g is non-finite in at least one element exactly when the arbiter's is.  Which statistics and which
 *    elements of g are non-finite does not depend on the slices, and no bit of a result on the trace being requested.
 * 3. No invention.  No clamp stands between the data and the policy: an infinity is never turned into a finite value, and no
 *    statistic other than surr_before and surr_after is finite where the arbiter's is not.
 * 4. Unread data.  The policy step does not read slots 6 .. 11, any moment, or rows at and beyond n: a non-finite value there
 *    changes no bit of any result.  The workspace's contents at entry mean nothing: the flags (skipped, CG converged, accepted)
 *    and scalars a previous call left, of whatever kind, change no bit of the next call.
 * 5. No faults.  No loaded float becomes an address, an index or a loop bound.
 * qst_vf_fit follows the rules of quadsim_bc.h's NON-FINITE VALUES paragraph as they stand (the loss; the value tower as a whole;
 * Adam per element; unread rows and the steps before the first that reads a non-finite value; no faults).  The policy's slots
 * 0 .. 5 and 12 and the moments of those slots are not read: a non-finite value there changes no bit, and stays what it was.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= n < 2^31, 0 <= slices <= 1024, 1 <= cg_iters <= 64, 1 <= backtracks <= 32, fvp_stride >= 1; max_kl > 0 and every
 * hyper-parameter finite, cg_damping, residual_tol >= 0; 1 <= batch <= 256, 1 <= steps <= 4096, t0 >= 0 and t0 + steps < 2^31,
 * 0 <= beta1, beta2 < 1.  Every tensor is 4-byte aligned, the workspace and the trace's cg 8-byte; the tensors a call writes may not
 * overlap each other.  A refused call returns an error code, leaves a message in qst_last_error() and launches nothing.
 */
#ifndef QUADSIM_TRPO_H
#define QUADSIM_TRPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QST_VERSION 1

enum { QST_OK = 0, QST_ERR_INVALID = 1, QST_ERR_HIP = 2 };

enum { QST_NET_SHARED_TRUNK = 0, QST_NET_TOWERS = 1 };

enum { QST_PARAMS = 18696, QST_TENSORS = 13, QST_STATS = 10, QST_CHUNK = 16, QST_AUTO_SLICES = 128, QST_MAX_SLICES = 1024,
       QST_MAX_CG_ITERS = 64, QST_MAX_BACKTRACKS = 32, QST_MAX_BATCH = 256, QST_MAX_STEPS = 4096, QST_CG_SCALARS = 4 };

/* the actor-critic in the slot order above; m and v are read for the slots 6 .. 11 by qst_vf_fit alone */
typedef struct QstNet {
    uint32_t struct_size; /* sizeof(QstNet) */
    int32_t layout;       /* QST_NET_TOWERS */
    float *w[13], *m[13], *v[13];
} QstNet;

/* what Runner.run() returns, flattened: n rows */
typedef struct QstBatch {
    uint32_t struct_size; /* sizeof(QstBatch) */
    int32_t reserved;
    int64_t n;
    const float *obs;     /* [n,12] */
    const float *actions; /* [n,4] */
    const float *returns, *values; /* [n] */
} QstBatch;

typedef struct QstHyper {
    uint32_t struct_size; /* sizeof(QstHyper) */
    int32_t cg_iters, backtracks, fvp_stride;
    double max_kl, cg_damping, entcoeff, residual_tol;
} QstHyper;

/* what the solver saw (nullable as a whole; every member must then be set).  Rows of iterations that did not run are not written */
typedef struct QstTrace {
    uint32_t struct_size; /* sizeof(QstTrace) */
    int32_t reserved;
    float *fvp_in, *fvp_out; /* [cg_iters + 1, P]: the vector handed to product k and (F + damping) times it */
    double *cg;              /* [cg_iters, 4]: DOT(p, z), alpha, the new rdotr, mu */
    float *x, *fullstep;     /* [P] */
    float *ls;               /* [backtracks, 2]: surr_k, kl_k of every evaluated candidate */
} QstTrace;

int qst_version(void);
const char *qst_last_error(void); /* host string, per thread */

/* the slices qst_policy_step takes for slices = 0 (0 for n < 1) */
int qst_auto_slices(int64_t n);

/* the workspace of a policy step over n rows with these slices (0 = auto) */
int qst_workspace_bytes(int64_t n, int32_t slices, size_t *bytes);

/* one policy update; stats [10] float32 (device), grad: nullable [P] (device), receives g */
int qst_policy_step(const QstNet *net, const QstBatch *data, int32_t slices, const QstHyper *hp, void *workspace,
                    uint64_t workspace_bytes, float *stats, float *grad, const QstTrace *trace, void *stream);

/* `steps` Adam steps of the value tower; indices [steps,batch] int32 (device), stats [steps] float32 (device) */
int qst_vf_fit(const QstNet *net, const float *obs, const float *returns, int64_t n, const int32_t *indices, int32_t steps,
               int32_t batch, double lr, double beta1, double beta2, double eps, int64_t t0, float *stats, float *const *grads,
               void *stream);

#ifdef __cplusplus
}
#endif
#endif
