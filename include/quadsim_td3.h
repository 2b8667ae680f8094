/* quadsim_td3.h -- C ABI of libquadsim_td3.so: the TD3 update on the device.
 * TD3 is DDPG with two critics whose smaller target value is the regression target, clipped Gaussian noise on the target action,
 * and an actor (with all three target nets) that moves only on every policy_delay-th update.  qstd_update runs `steps` such updates
 * on the caller's stream, ONE launch per update -- two workgroups (q1, q2) on a critic-only update, three (q1, q2, actor) on an
 * actor update -- between one copy into the workspace and one out of it; nothing synchronises with the host.
 *
 * SB2 is not part of this project: this header is the definition (it restates stable_baselines/td3 as recalled, not checked against
 * it).  The library is independent of the other nine at link time and shares no host state with them.  Every pointer is a DEVICE
 * pointer unless stated otherwise.  The library allocates nothing.  C99-clean.
 *
 * ---- the nets (layers = [128, 128], no layer norm, ReLU) -------------------------------------------------------------------
 * Six nets of six float32 tensors each, in the policy's (in, out) layout, in the order w0, b0, w1, b1, w2, b2:
 *   actor          w0 [12,128], b0 [128], w1 [128,128], b1 [128], w2 [128,4], b2 [4]     (the six tensors of QsbcNet)
 *                  h0 = relu(w0^T obs + b0), h1 = relu(w1^T h0 + b1), a = tanh(w2^T h1 + b2)
 *   q1, q2         w0 [16,128], b0 [128], w1 [128,128], b1 [128], w2 [128,1], b2 [1]
 *                  h0 = relu(w0^T [obs ; act] + b0), h1 = relu(w1^T h0 + b1), q = w2^T h1 + b2: the action enters at the input, rows
 *                  12 .. 15 of w0 are the action's (SB2 TD3's make_critics; NOT quadsim_ddpg.h's critic)
 *   actor target, q1 target, q2 target: copies of the same shapes.  Only the three online nets have Adam moments (m, v).
 * Observations, actions, rewards and done flags are used as stored: there is no observation clamp.
 * NOT BUILT: layer norm, prioritised replay, observation and return normalisation.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add) ---------------------
 * Rows.  Step s is update u = t0 + s.  It uses replay rows indices[s][0 .. rows-1], rows = counts[s] (counts == NULL: batch);
 * position j of indices[s] is ROW SLOT j.  Entries at or beyond counts[s] are never read.  Entries outside [0, n) and counts outside
 * [1, batch] are UNDEFINED BEHAVIOUR (not checked on the device; a count above batch is read as batch).  Every gradient of an update
 * is taken at the weights from BEFORE the update: the actor term sees q1 before its step, the target value the targets before theirs.
 * Forward, every net, per row: z[u] = b[u], then z[u] = fma(w[k][u], in[k], z[u]) for k ascending over the layer's inputs (layer 0
 * of the actor held on chip is padded with four zero inputs against zero weights, which contribute exactly nothing; a critic's
 * layer 0 runs k = 0 .. 15, the action last); relu = z <= 0 ? 0 : z.  tanh is q_tanh of the main library with tanh(NaN) = NaN.
 * clampsel(v, lo, hi) = v < lo ? lo : v > hi ? hi : v: a NaN stays.
 * 1. Noise.  z[j][0..3], four standard normals per row slot, is the caller's noise[s][j][0..3] where noise != NULL, and otherwise
 *    the keyed draw normals_from_words(Philox4x32-10 with key `seed`, counter (block = u, subsequence = (6 << 48) | j)): the four
 *    normals of that ONE block are the four action components, Box-Muller as quadsim.h states it for the policy's noise.  The
 *    draw depends on (seed, u, j) alone -- not on the replay index, on batch or on how a run is split into calls.  noise_out
 *    (nullable) [steps,batch,4] receives the z that was used, slots 0 .. rows-1 of every step; other slots are not written.
 * 2. Target value.  a1 = actor_target(obs1); e[c] = clampsel(SIGMA * z[c], -CL, CL); a'[c] = clampsel(a1[c] + e[c], -1, 1);
 *    qa = q1_target(obs1, a'), qb = q2_target(obs1, a'); m = qa if qa is NaN, else qb if qb is NaN, else (qb < qa ? qb : qa);
 *        y = done >= 1 ? rew : fma((1 - done) * G, m, rew)
 *    SIGMA, CL, G = float32 of target_policy_noise, target_noise_clip, gamma.  A terminal row does not read m at all.
 * 3. Critics, each of q1, q2 alike.  q = critic(obs0, act); d = q - y; loss = S / float32(rows), S = fma(d, d, S) over the rows
 *    ascending from 0.  dq = d * float32(2 / rows) (the constant in float64).  ReLU mask: the COMPUTED activation, h > 0.
 *    dz1[i] = mask1[i] ? fma(w2[i], dq, 0) : 0.  dz0[i] = mask0[i] ? ((S0 + S1) + (S2 + S3)) : 0 for i = 0 .. 127, S_c = (acc = 0;
 *    acc = fma(w1[i][o], dz1[o], acc) over o = c, c + 4, .. , c + 124 ascending): four interleaved chains in that fixed tree.
 *    Gradients: gW[i][o] = 0, then gW[i][o] = fma(dz[row][o], in[row][i], gW[i][o]) over the rows of the step in ascending order;
 *    gb[o] = gb[o] + dz[row][o] likewise; w0's sixteen input rows alike.  A step's rows are padded to a multiple of 16 with rows
 *    whose dq is zero: they add fma(0, a, g) = g and g + 0.
 *    Adam with critic_lr at step t = u + 1, exactly as quadsim_ddpg.h item 4 states it.
 * 4. Actor and targets, ONLY on updates with u % policy_delay == 0.  pi = actor(obs0), qpi = q1(obs0, pi) with the ONLINE q1 from
 *    before its step; actor_loss = -(T / float32(rows)), T = T + qpi over the rows ascending from 0.  Neither critic gets a
 *    gradient from this term.  dq/da runs back through all three layers of q1, N = -float32(1 / rows):
 *        dc1[o] = h1[o] <= 0 ? 0 : w2[o] * N                                                            o = 0 .. 127
 *        dc0[i] = h0[i] <= 0 ? 0 : (acc = 0; acc = fma(w1[i][o], dc1[o], acc), o = 0 .. 127 ascending)       i = 0 .. 127
 *        da[c]  = (acc = 0; acc = fma(w0[12 + c][i], dc0[i], acc), i = 0 .. 127 ascending)                   c = 0 .. 3
 *    with q1's computed activations h0, h1 of this pass (for every finite h the mask h > 0; a NaN activation hands its term on, as
 *    float64 autograd's ReLU does, so an actor behind a diverged q1 diverges too); padding rows have dc1 = 0.
 *    dz2[c] = da[c] * fma(-a[c], a[c], 1).
 *    Then dz1 (over o = 0 .. 3 ascending), dz0 and the gradients of the actor exactly as quadsim_bc.h states them.
 *    Adam with actor_lr at step t = actor_t0 + k + 1, k = the actor steps taken before this update IN THIS CALL.
 *    Targets, every element of the three target nets: t' = fma(T, w', U * t), T = float32(tau), U = float32(1 - tau) (the difference
 *    in float64), w' the online weight AFTER its Adam step of this update.  tau = 1 gives t' = w' for every finite t.
 *    On every other update the actor, its moments and all three targets keep their bits.
 * Outputs.  stats [steps,6]: q1_loss, q2_loss, mean q1 = (sum of q, rows ascending) / float32(rows), mean q2, mean y likewise,
 * actor_loss -- 0.0 on an update without an actor step -- each with the weights from before that step.  grads (nullable): a HOST
 * array of eighteen device pointers, which receive the gradients of the LAST step in the weights' own layout: the actor's six, q1's
 * six, q2's six; where the last step is no actor step the actor's six are not written.
 * Invariants: the same inputs give the same bits on any stream; one call with steps = a + b equals the call with steps = a followed
 * by the call with t0 + a, actor_t0 + (the actor steps of the first call), steps = b, bit for bit in all 72 tensors and the stats;
 * a step with counts[s] = c in a call of any batch >= c equals the same step in a call with batch = c; a keyed call equals the
 * call that is fed its own noise_out, bit for bit.
 * NON-FINITE VALUES.  The five rules of quadsim_ddpg.h hold as they stand there (statistics; state per net; no invention; unread
 * data; no faults), the arbiter being float64 torch autograd with torch.where for the twin minimum, both clamps and the terminal
 * rows.  The minimum and both clamps are the selects above: a NaN in either target critic reaches y of every non-terminal row,
 * a NaN in the noise or in a1 reaches a'.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= batch <= 256, 1 <= counts[s] <= batch, 1 <= steps <= 4096, 1 <= n < 2^31, t0 >= 0 and t0 + steps < 2^31, actor_t0 >= 0 and
 * actor_t0 + steps < 2^31, 1 <= policy_delay <= 2^16; 0 <= gamma <= 1, 0 < tau <= 1, target_policy_noise >= 0,
 * target_noise_clip >= 0 (inf allowed), actor_lr, critic_lr and eps finite, 0 <= beta1, beta2 < 1.  The workspace holds
 * qstd_workspace_bytes() bytes, 16-byte aligned; its contents between calls mean nothing.  Every tensor is 4-byte aligned; none
 * may overlap another: the 72 tensors of the nets, stats, noise_out, the workspace and the gradients are checked against each
 * other, the replay and the noise are the caller's.  A refused call returns an error code, leaves a message in qstd_last_error()
 * and launches nothing.
 */
#ifndef QUADSIM_TD3_H
#define QUADSIM_TD3_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSTD_VERSION 1

enum { QSTD_OK = 0, QSTD_ERR_INVALID = 1, QSTD_ERR_HIP = 2 };

enum { QSTD_MAX_BATCH = 256, QSTD_MAX_STEPS = 4096, QSTD_MAX_DELAY = 65536, QSTD_STATS = 6, QSTD_CHUNK = 16, QSTD_NOISE_STREAM = 6 };

enum { QSTD_ACTOR = 0, QSTD_Q1 = 1, QSTD_Q2 = 2, QSTD_ACTOR_TARGET = 3, QSTD_Q1_TARGET = 4, QSTD_Q2_TARGET = 5 };

/* the six nets and the optimiser state of the three online ones; tensors in the order w0, b0, w1, b1, w2, b2 */
typedef struct QstdNets {
    uint32_t struct_size; /* sizeof(QstdNets) */
    int32_t reserved;
    float *w[6][6]; /* QSTD_ACTOR .. QSTD_Q2_TARGET */
    float *m[3][6], *v[3][6]; /* QSTD_ACTOR, QSTD_Q1, QSTD_Q2 */
} QstdNets;

/* a replay of n transitions: obs0 [n,12], act [n,4], rew [n], obs1 [n,12], done [n] (0 or 1) */
typedef struct QstdReplay {
    uint32_t struct_size; /* sizeof(QstdReplay) */
    int32_t reserved;
    int64_t n;
    const float *obs0, *act, *rew, *obs1, *done;
} QstdReplay;

typedef struct QstdHyper {
    uint32_t struct_size; /* sizeof(QstdHyper) */
    int32_t policy_delay;
    double gamma, tau, actor_lr, critic_lr, target_policy_noise, target_noise_clip, beta1, beta2, eps;
} QstdHyper;

int qstd_version(void);
const char *qstd_last_error(void); /* host string, per thread */

/* the size of the workspace of any call */
int qstd_workspace_bytes(size_t *bytes);

/* `steps` updates on rows of the replay chosen by indices [steps,batch] and counts [steps] (nullable).  t0: updates (critic Adam
 * steps) taken before this call; actor_t0: actor Adam steps taken before it.  noise [steps,batch,4] (nullable: keyed draws from
 * `seed`), noise_out [steps,batch,4] (nullable).  stats [steps,6].  grads: nullable HOST array of eighteen device pointers. */
int qstd_update(const QstdNets *nets, const QstdReplay *replay, const int32_t *indices, const int32_t *counts, int32_t steps,
                int32_t batch, const QstdHyper *hp, int64_t t0, int64_t actor_t0, const float *noise, uint64_t seed, float *noise_out,
                void *workspace, uint64_t workspace_bytes, float *stats, float *const *grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif
