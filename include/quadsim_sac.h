/* quadsim_sac.h -- C ABI of libquadsim_sac.so: the Soft Actor-Critic update on the device.
 * SAC (the form with a state-value net) trains a tanh-squashed Gaussian actor whose head emits a mean AND a log standard deviation,
 * two critics, a value net with a Polyak target and, optionally, its own temperature.  qss_update runs `steps` such updates on the
 * caller's stream, ONE launch of four workgroups (q1, q2, value, actor) per update, between one copy into the workspace and one out
 * of it; nothing synchronises with the host.
 *
 * SB2 is not part of this project: this header is the definition (it restates stable_baselines/sac as recalled, not checked against
 * it).  The library is independent of the other ten at link time and shares no host state with them.  Every pointer is a DEVICE
 * pointer unless stated otherwise.  The library allocates nothing.  C99-clean.
 *
 * ---- the nets (layers = [128, 128], no layer norm, ReLU) -------------------------------------------------------------------
 * Five nets of six float32 tensors each, in the policy's (in, out) layout, in the order w0, b0, w1, b1, w2, b2:
 *   actor          w0 [12,128], b0 [128], w1 [128,128], b1 [128], w2 [128,8], b2 [8]
 *                  h0 = relu(w0^T obs + b0), h1 = relu(w1^T h0 + b1), head = w2^T h1 + b2; columns 0 .. 3 of the head are mu, columns
 *                  4 .. 7 the raw log standard deviation ls_raw.  The deterministic action is tanh(mu).
 *   q1, q2         w0 [16,128], b0 [128], w1 [128,128], b1 [128], w2 [128,1], b2 [1] on [obs ; act]: quadsim_td3.h's critic, rows
 *                  12 .. 15 of w0 are the action's
 *   v, v_target    w0 [12,128], b0 [128], w1 [128,128], b1 [128], w2 [128,1], b2 [1] on obs
 * Only the four online nets (actor, q1, q2, v) have Adam moments (m, v).  alpha_state [3] holds log_alpha and its Adam moments m, v.
 * NOT BUILT: SAC without the value net, layer norm, prioritised replay, observation and return normalisation.
 *
 * ---- numerical contract (float32, every named operation rounded once; fma = fused multiply-add) ---------------------
 * Rows, the forward chain, relu, tanh (tanh(NaN) = NaN) and clampsel are quadsim_td3.h's, word for word: step s is update u = t0 + s on
 * replay rows indices[s][0 .. rows-1], rows = counts[s] (counts == NULL: batch); every gradient of an update is taken at the weights
 * and at the log_alpha from BEFORE the update.  exp is expf, ln(x) = log2(x) * float32(ln 2) on the hardware log2 (q_ln of the main
 * library).  R = float32(1 / rows) (the quotient in float64), F = float32(rows), alpha = exp(log_alpha), TE = float32(target_entropy),
 * G = float32(gamma), L2PI = float32(log(2 pi)), E6 = 1e-6f.
 * 1. Noise.  z[j][0..3], four standard normals per row slot: the caller's noise[s][j][0..3] where noise != NULL, otherwise the keyed
 *    draw of quadsim_td3.h item 1 on Philox stream 7 (subsequence (7 << 48) | j, block u, key `seed`).  noise_out (nullable)
 *    [steps,batch,4] receives the z that was used, slots 0 .. rows-1.  The actor branch and the value branch use the same z.
 * 2. Sample and log-probability, per row and component c, head = actor(obs0):
 *        ls = clampsel(ls_raw, -20, 2); sigma = exp(ls); p = sigma * z; u = fma(sigma, z, mu); a = tanh(u)
 *        den = sigma + E6; t = p / den; g = fma(t, t, fma(2, ls, L2PI))
 *        s2 = fma(-a, a, 1); J = ln(s2 + E6); term = (-0.5 * g) - J
 *        logp = ((((0 + term[0]) + term[1]) + term[2]) + term[3])
 * 3. Critics, each of q1, q2 alike.  vt = v_target(obs1); y = done >= 1 ? rew : fma((1 - done) * G, vt, rew): a terminal row does not
 *    read vt.  q = critic(obs0, act); d = q - y; loss = 0.5 * (S / F), S = fma(d, d, S) over the rows ascending from 0; dq = d * R.
 *    The backward pass and the gradient sums are quadsim_td3.h item 3's.  Adam with lr at step t = u + 1 (quadsim_ddpg.h item 4).
 * 4. Value.  a, logp of item 2 with the ONLINE actor; qa = q1(obs0, a), qb = q2(obs0, a) with the online critics from before their
 *    step; mn = qa if qa is NaN, else qb if qb is NaN, else (qb < qa ? qb : qa); vb = mn - alpha * logp.  val = v(obs0); d = val - vb;
 *    loss = 0.5 * (S / F) as above; dv = d * R; backward pass as the critics' (twelve inputs).  Adam with lr at t = u + 1.  Then, every
 *    update, every element of v_target: t' = fma(T, w', U * t), T = float32(tau), U = float32(1 - tau), w' the value net's weight
 *    AFTER its Adam step.
 * 5. Actor.  loss = (sum over rows ascending of (alpha * logp - qpi)) / F with qpi = q1(obs0, a), the online q1 from before its step
 *    (q1 alone).  da[c], the derivative of -R * qpi with respect to a[c], runs back through all three layers of q1 exactly as
 *    quadsim_td3.h item 4 states it (N = -R).  AR = alpha * R on a row of the step, 0 on a padding row.  Per component:
 *        jd  = ((2 * a) * s2) / (s2 + E6)                 the Jacobian term's derivative with respect to u
 *        du  = fma(AR, jd, da * s2)
 *        dtl = (p * E6) / (den * den); gl = fma(t, dtl, 1)     t's derivative with respect to ls, and half the Gaussian term's
 *        dls = fma(du, p, (-AR) * gl)
 *        dz2[c] = du; dz2[4 + c] = (ls_raw < -20 or ls_raw > 2) ? 0 : dls     (the clamp passes a gradient on [-20, 2], ends included)
 *    Then dz1[i] = mask1[i] ? (acc = 0; acc = fma(w2[i][o], dz2[o], acc), o = 0 .. 7 ascending) : 0, dz0 and the gradient sums exactly
 *    as quadsim_bc.h states them, the head eight wide.  Adam with lr at t = u + 1.
 *    Temperature.  mean = (sum over rows ascending of (logp + TE)) / F; alpha_loss = -(log_alpha * mean); its gradient is -mean (the mean
 *    is a constant).  auto_alpha = 1: Adam with lr at t = u + 1 on log_alpha.  auto_alpha = 0: the three floats keep their bits.
 * 6. Statistics.  stats [steps,8]: q1_loss, q2_loss, value_loss, actor_loss, alpha_loss, alpha, mean logp = (sum of logp, rows ascending)
 *    / F of the actor branch, mean y likewise, each with the weights from before that step.
 * 7. Traces (QssTrace, nullable as a whole and per field).  logp_out, vlogp_out [steps,batch]: the actor branch's and the value
 *    branch's logp of every row slot below rows (bit for bit the same); act_out [steps,batch,4]: the sampled a of the actor branch;
 *    fwd_out [steps,batch,5]: vt (0 on a terminal row, which does not read it), y, qa, qb, vb.  grads (nullable): a HOST array of 24
 *    device pointers, which receive the gradients of the LAST step in the weights' own layout: the actor's six, q1's, q2's, v's.
 * 8. Invariants: the same inputs give the same bits on any stream; one call with steps = a + b equals the call with steps = a followed
 *    by the call with t0 + a, steps = b, bit for bit in all 30 tensors, the moments, alpha_state and the stats; a step with counts[s] =
 *    c in a call of any batch >= c equals the same step in a call with batch = c; a keyed call equals the call that is fed its own
 *    noise_out, bit for bit.
 *    NON-FINITE VALUES.  The five rules of quadsim_ddpg.h hold as they stand there, the arbiter being float64 torch autograd with
 *    torch.where for the twin minimum, the clamp and the terminal rows.
 * 9. qss_math(which, in, out, n, stream): out[i] = exp(in[i]) (QSS_MATH_EXP), ln(in[i]) (QSS_MATH_LN) or ln(fma(-a, a, 1) + E6) with
 *    a = tanh(in[i]) (QSS_MATH_JAC): the device functions of item 2, element-wise, so that a test can sweep them.
 *
 * ---- limits ---------------------------------------------------------------------------------------------------------
 * 1 <= batch <= 256, 1 <= counts[s] <= batch, 1 <= steps <= 4096, 1 <= n < 2^31, t0 >= 0 and t0 + steps < 2^31; 0 <= gamma <= 1,
 * 0 < tau <= 1, lr, target_entropy and eps finite, 0 <= beta1, beta2 < 1, auto_alpha 0 or 1.  The workspace holds
 * qss_workspace_bytes() bytes, 16-byte aligned; its contents between calls mean nothing.  Every tensor is 4-byte aligned; none may
 * overlap another: the 78 tensors of the nets, alpha_state, stats, noise_out, the traces, the workspace and the gradients are checked
 * against each other, the replay and the noise are the caller's.  A refused call returns an error code, leaves a message in
 * qss_last_error() and launches nothing.
 */
#ifndef QUADSIM_SAC_H
#define QUADSIM_SAC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QSS_VERSION 1

enum { QSS_OK = 0, QSS_ERR_INVALID = 1, QSS_ERR_HIP = 2 };

enum { QSS_MAX_BATCH = 256, QSS_MAX_STEPS = 4096, QSS_STATS = 8, QSS_FWD = 5, QSS_CHUNK = 16, QSS_NOISE_STREAM = 7 };

enum { QSS_ACTOR = 0, QSS_Q1 = 1, QSS_Q2 = 2, QSS_V = 3, QSS_V_TARGET = 4 };

enum { QSS_MATH_EXP = 0, QSS_MATH_LN = 1, QSS_MATH_JAC = 2 };

/* the five nets and the optimiser state of the four online ones; tensors in the order w0, b0, w1, b1, w2, b2 */
typedef struct QssNets {
    uint32_t struct_size; /* sizeof(QssNets) */
    int32_t reserved;
    float *w[5][6]; /* QSS_ACTOR .. QSS_V_TARGET */
    float *m[4][6], *v[4][6]; /* QSS_ACTOR, QSS_Q1, QSS_Q2, QSS_V */
    float *alpha_state; /* [3]: log_alpha, m, v */
} QssNets;

/* a replay of n transitions: obs0 [n,12], act [n,4], rew [n], obs1 [n,12], done [n] (0 or 1) */
typedef struct QssReplay {
    uint32_t struct_size; /* sizeof(QssReplay) */
    int32_t reserved;
    int64_t n;
    const float *obs0, *act, *rew, *obs1, *done;
} QssReplay;

typedef struct QssHyper {
    uint32_t struct_size; /* sizeof(QssHyper) */
    int32_t auto_alpha;
    double gamma, tau, lr, target_entropy, beta1, beta2, eps;
} QssHyper;

typedef struct QssTrace {
    uint32_t struct_size; /* sizeof(QssTrace) */
    int32_t reserved;
    float *logp_out, *vlogp_out, *act_out, *fwd_out; /* each nullable */
} QssTrace;

int qss_version(void);
const char *qss_last_error(void); /* host string, per thread */

/* the size of the workspace of any call */
int qss_workspace_bytes(size_t *bytes);

/* `steps` updates on rows of the replay chosen by indices [steps,batch] and counts [steps] (nullable).  t0: updates taken before this
 * call.  noise [steps,batch,4] (nullable: keyed draws from `seed`), noise_out [steps,batch,4] (nullable).  stats [steps,8].  trace:
 * nullable.  grads: nullable HOST array of 24 device pointers. */
int qss_update(const QssNets *nets, const QssReplay *replay, const int32_t *indices, const int32_t *counts, int32_t steps,
               int32_t batch, const QssHyper *hp, int64_t t0, const float *noise, uint64_t seed, float *noise_out, void *workspace,
               uint64_t workspace_bytes, float *stats, const QssTrace *trace, float *const *grads, void *stream);

/* out[i] = f(in[i]) for i < n, f chosen by `which` (QSS_MATH_*) */
int qss_math(int32_t which, const float *in, float *out, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
