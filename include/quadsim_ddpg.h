/* quadsim_ddpg.h -- C ABI of libquadsim_ddpg.so: the DDPG update on the device.
 * run_docking_ddpg.py alternates 1500 env steps with nb_train_steps = 100 updates of batch_size = 10; one update is four forward
 * passes, two backward passes, two Adam steps and a Polyak average.  qsdd_update runs `steps` such updates on the caller's stream,
 * ONE launch of two workgroups per update (the critic branch and the actor branch) between one copy into the workspace and one
 * out of it; nothing synchronises with the host and nothing is drawn on the device.
 *
 * SB2 is not part of this project: this header is the definition.  The library is independent of the other seven at link time
 * and shares no host state with them.  Every pointer is a DEVICE pointer unless stated otherwise.  The library allocates nothing.
 * C99-clean.
 *
 * ---- the nets (CustomDDPGPolicy, layers = [128, 128], no layer norm, ReLU) ---------------------------------------------
 * Four nets of six float32 tensors each, in the policy's (in, out) layout, in the order w0, b0, w1, b1, w2, b2:
 *   actor          w0 [12,128], b0 [128], w1 [128,128], b1 [128], w2 [128,4], b2 [4]     (the six tensors of QsbcNet)
 *                  h0 = relu(w0^T obs + b0), h1 = relu(w1^T h0 + b1), a = tanh(w2^T h1 + b2)
 *   critic         w0 [12,128], b0 [128], w1 [132,128], b1 [128], w2 [128,1], b2 [1]
 *                  h0 = relu(w0^T obs + b0), h1 = relu(w1^T [h0 ; act] + b1), q = w2^T h1 + b2: the action enters after layer 0,
 *                  rows 128 .. 131 of w1 are the action's
 *   actor target, critic target: copies of the same shapes.  Only the two online nets have Adam moments (m, v).
 * Observations are clamped to [-obs_clip, obs_clip] as they are loaded, obs = min(max(obs, -obs_clip), obs_clip) (SB2's
 * observation_range is (-5, 5); obs_clip = inf disables the clamp).  Actions, rewards and done flags are used as stored.
 * NOT BUILT: observation and return normalisation, critic_l2_reg, clip_norm, parameter noise, reward_scale != 1, layer norm.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add) ---------------------
 * Rows.  Step s (Adam step t0 + s) uses replay rows indices[s][0 .. rows-1], rows = counts[s] (counts == NULL: batch).  Entries
 * at or beyond counts[s] are never read.  Entries outside [0, n) and counts outside [1, batch] are UNDEFINED BEHAVIOUR (not
 * checked on the device; a count above batch is read as batch).  Every gradient of a step is taken at the weights from BEFORE
 * the step: the actor term sees the critic before its update, the critic's target value the targets before theirs.
 * Forward, every net, per row: z[u] = b[u], then z[u] = fma(w[k][u], in[k], z[u]) for k ascending over the layer's inputs
 * (layer 0 of a net held on chip is padded with four zero inputs against zero weights, which contribute exactly nothing; the
 * critic's layer 1 runs k = 0 .. 131, the action last); relu = max(z, 0).  tanh is q_tanh of the main library: e = exp2(min(2 |z|,
 * 60) log2 e), r = 1 / (e + 1) (hardware exp2 and rcp, 1 ulp each), a = copysign(1 - 2 r, z).
 * 1. Target value.  a1 = actor_target(obs1), q1 = critic_target(obs1, a1),
 *        y = done >= 1 ? rew : fma((1 - done) * G, q1, rew)        G = float32(gamma)
 *    (a terminal row does not read q1 at all: a target net that overflows there changes nothing).
 * 2. Critic.  q = critic(obs0, act); d = q - y; critic_loss = S / float32(rows), S = fma(d, d, S) over the rows ascending from 0.
 *    dq = d * float32(2 / rows) (the constant in float64).  ReLU mask: the COMPUTED activation, h > 0.
 *    dz1[i] = mask1[i] ? fma(w2[i], dq, 0) : 0.  dz0[i] = mask0[i] ? ((S0 + S1) + (S2 + S3)) : 0 for i = 0 .. 127, S_c = (acc = 0;
 *    acc = fma(w1[i][o], dz1[o], acc) over o = c, c + 4, .. , c + 124 ascending): four interleaved chains in that fixed tree.
 * 3. Actor.  pi = actor(obs0), qpi = critic(obs0, pi) with the ONLINE critic; actor_loss = -(T / float32(rows)), T = T + qpi over
 *    the rows ascending from 0.  This term gives the critic no gradient.  Only the critic's layers 1 and 2 are differentiated:
 *    dzc[o] = maskc1[o] ? w2c[o] * N : 0, N = -float32(1 / rows); da[j] = (acc = 0; acc = fma(w1c[128 + j][o], dzc[o], acc), o = 0 ..
 *    127 ascending); dz2[j] = da[j] * fma(-a[j], a[j], 1): the tanh derivative 1 - a^2 from the computed a.  Then dz1 (over
 *    o = 0 .. 3 ascending) and dz0 of the actor exactly as quadsim_bc.h states them.
 *    Gradients of either net: gW[i][o] = 0, then gW[i][o] = fma(dz[row][o], in[row][i], gW[i][o]) over the rows of the step in
 *    ascending order; gb[o] = gb[o] + dz[row][o] likewise.  A step's rows are padded to a multiple of 16 with rows whose dq (or
 *    dzc) is zero: they add fma(0, a, g) = g and g + 0.  The bits of a step therefore depend on the nets, its rows and counts[s]
 *    alone -- not on `batch`, not on the other steps of the call, not on which half of the workspace held the nets.
 * 4. Adam on either online net with its own learning rate: tf.train.AdamOptimizer's formula, exactly as quadsim_dyn_fit.h states
 *    it (MpiAdam's lr sqrt(1 - beta2^t) / (1 - beta1^t) m / (sqrt(v) + eps) is the same expression).  With t = t0 + s + 1,
 *        lr_t = float32(lr * sqrt(1 - beta2^t) / (1 - beta1^t))      (float64 on the host, per step, rounded to float32 once)
 *        m' = fma(B1, m, C1 * g)          B1 = float32(beta1), C1 = float32(1 - beta1)  (the difference in float64)
 *        v' = fma(B2, v, C2 * (g * g))    B2 = float32(beta2), C2 = float32(1 - beta2)
 *        w' = w - (lr_t * m') / (sqrt(v') + E)      E = float32(eps); sqrt and the division correctly rounded
 * 5. Targets, every element of the two target nets: t' = fma(T, w', U * t), T = float32(tau), U = float32(1 - tau) (the
 *    difference in float64), w' the online weight AFTER step 4.  tau = 1 gives t' = w' for every finite t.
 * Outputs.  stats [steps,4]: critic_loss, actor_loss, mean q = (sum of q, rows ascending) / float32(rows), mean y likewise, each
 * with the weights from before that step.  grads (nullable): a HOST array of twelve device pointers, which receive the gradients
 * of the LAST step in the weights' own layout: the actor's six, then the critic's six.
 * Invariants: the same inputs give the same bits on any stream; one call with steps = a + b equals the call with steps = a
 * followed by the call with t0 + a, steps = b, bit for bit in all 48 tensors and the stats; a step with counts[s] = c in a call of
 * any batch >= c equals the same step in a call with batch = c.
 * NON-FINITE VALUES (NaN, +inf, -inf in a row, a weight or a moment).  A diverged run looks diverged:
 * 1. Statistics.  A statistic of a step is non-finite exactly when float64 torch autograd over the same rows, weights and moments
 *    makes it non-finite -- torch.relu, torch.clamp, torch.where for the terminal rows, MpiAdam's formula: what update="torch" of
 *    the package computes.  So relu, the clamp and tanh are selects that keep a NaN (relu = z <= 0 ? 0 : z; the clamp
 *    v < -c ? -c : v > c ? c : v; tanh(NaN) = NaN, where q_tanh alone would give +-1), never a max / min that drops one.
 * 2. State.  After a step a net (actor, critic, either target) holds a non-finite weight exactly when the arbiter's does: per
 *    net, not per element (the backward masks stay h > 0 ? acc : 0, which turn a NaN activation's term into 0).  Adam is held
 *    per element: w', m', v' are non-finite in exactly the elements in which the formula of 4. is, applied to the step's own
 *    gradient; where it is finite the bounds of the finite case apply.
 * 3. No invention.  With a finite obs_clip an infinite observation is its clamped copy, bit for bit; a NaN is never clamped
 *    away.  A terminal row (done >= 1) never selects q1: non-finite target nets change nothing but themselves there.
 * 4. Unread data.  Rows that no index of a step names, index entries at and beyond counts[s], and every step before the first
 *    one that reads a non-finite value are bit for bit what they are without it.
 * 5. No faults.  No loaded float becomes an address, an index or a loop bound: no value of any kind makes a call fault or write
 *    outside its arrays.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= batch <= 256, 1 <= counts[s] <= batch, 1 <= steps <= 4096, 1 <= n < 2^31, t0 >= 0 and t0 + steps < 2^31; 0 <= gamma <= 1,
 * 0 < tau <= 1, obs_clip > 0 (inf allowed), actor_lr, critic_lr and eps finite, 0 <= beta1, beta2 < 1.  The workspace holds
 * qsdd_workspace_bytes() bytes, 16-byte aligned; its contents between calls mean nothing.  Every tensor is 4-byte aligned; none
 * may overlap another: the 48 tensors of the nets, stats, the workspace and the gradients are checked against each other, the
 * replay is the caller's.  A refused call returns an error code, leaves a message in qsdd_last_error() and launches nothing.
 */
#ifndef QUADSIM_DDPG_H
#define QUADSIM_DDPG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSDD_VERSION 1

enum { QSDD_OK = 0, QSDD_ERR_INVALID = 1, QSDD_ERR_HIP = 2 };

enum { QSDD_MAX_BATCH = 256, QSDD_MAX_STEPS = 4096, QSDD_STATS = 4, QSDD_CHUNK = 16 };

enum { QSDD_ACTOR = 0, QSDD_CRITIC = 1, QSDD_ACTOR_TARGET = 2, QSDD_CRITIC_TARGET = 3 };

/* the four nets and the optimiser state of the two online ones; tensors in the order w0, b0, w1, b1, w2, b2 */
typedef struct QsddNets {
    uint32_t struct_size; /* sizeof(QsddNets) */
    int32_t reserved;
    float *w[4][6]; /* QSDD_ACTOR .. QSDD_CRITIC_TARGET */
    float *m[2][6], *v[2][6]; /* QSDD_ACTOR, QSDD_CRITIC */
} QsddNets;

/* a replay of n transitions: obs0 [n,12], act [n,4], rew [n], obs1 [n,12], done [n] (0 or 1) */
typedef struct QsddReplay {
    uint32_t struct_size; /* sizeof(QsddReplay) */
    int32_t reserved;
    int64_t n;
    const float *obs0, *act, *rew, *obs1, *done;
} QsddReplay;

typedef struct QsddHyper {
    uint32_t struct_size; /* sizeof(QsddHyper) */
    int32_t reserved;
    double gamma, tau, actor_lr, critic_lr, obs_clip, beta1, beta2, eps;
} QsddHyper;

int qsdd_version(void);
const char *qsdd_last_error(void); /* host string, per thread */

/* the size of the workspace of any call */
int qsdd_workspace_bytes(size_t *bytes);

/* `steps` updates on rows of the replay chosen by indices [steps,batch] and counts [steps] (nullable).  t0: Adam steps taken
 * before this call.  stats [steps,4].  grads: nullable HOST array of twelve device pointers. */
int qsdd_update(const QsddNets *nets, const QsddReplay *replay, const int32_t *indices, const int32_t *counts, int32_t steps,
                int32_t batch, const QsddHyper *hp, int64_t t0, void *workspace, uint64_t workspace_bytes, float *stats,
                float *const *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif
