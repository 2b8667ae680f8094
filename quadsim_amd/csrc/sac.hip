// sac.hip -- libquadsim_sac.so: the C ABI of include/quadsim_sac.h over the kernels of sac_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other ten libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the streamed nets, the backward pass and the Adam step), quadsim_device.hpp (q_tanh, q_ln, the Philox counter and the
// normals) and side_offpolicy.hpp on side_host.hpp (error text, the checks, the table of the call's tensors and the copy launches).
#include "../../include/quadsim_sac.h"
#include "side_offpolicy.hpp"
#include "sac_kernels.hpp"

static_assert(QSS_OK == kOk && QSS_ERR_INVALID == kErrInvalid && QSS_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_sac.h");
static_assert(QSS_CHUNK == qsf::kRows && QSS_ACTOR == 0 && QSS_Q1 == 1 && QSS_Q2 == 2 && QSS_V == 3 && QSS_V_TARGET == 4 &&
                  QSS_NOISE_STREAM == (int)qssac::kStreamNoise && QSS_STATS == 8 && QSS_FWD == 5,
              "quadsim_sac.h states the kernels' geometry");

namespace {

using namespace qssac;

// the six tensors of net k (the ABI's order: the actor's shape, two critics', two value nets') that lie at `at`, into the call's table
template <class Table>
void add_net(Table &T, int k, float *const *six, int at)
{
    if (k == 0) T.template add_net<FA>(six, at);
    else if (k < 3) T.template add_net<FC>(six, at);
    else T.template add_net<FV>(six, at);
}

}  // namespace

extern "C" {

int qss_version(void) { return QSS_VERSION; }

const char *qss_last_error(void) { return g_err; }

int qss_workspace_bytes(size_t *bytes)
{
    if (!bytes) return fail(QSS_ERR_INVALID, "bytes must not be NULL");
    *bytes = sizeof(float) * (size_t)kWsFloats;
    return QSS_OK;
}

int qss_update(const QssNets *nets, const QssReplay *replay, const int32_t *indices, const int32_t *counts, int32_t steps,
               int32_t batch, const QssHyper *hp, int64_t t0, const float *noise, uint64_t seed, float *noise_out, void *workspace,
               uint64_t workspace_bytes, float *stats, const QssTrace *trace, float *const *grads, void *stream)
{
    if (int rc = check_call(nets, replay, indices, hp, workspace, stats, "Qss")) return rc;
    if (trace && trace->struct_size != sizeof(QssTrace))
        return fail(QSS_ERR_INVALID, "QssTrace.struct_size is %u, expected %zu", trace->struct_size, sizeof(QssTrace));
    if (int rc = check_extent(batch, QSS_MAX_BATCH, steps, QSS_MAX_STEPS, replay->n, t0)) return rc;
    if (hp->auto_alpha != 0 && hp->auto_alpha != 1) return fail(QSS_ERR_INVALID, "auto_alpha must be 0 or 1, got %d", hp->auto_alpha);
    if (int rc = check_discount(hp->gamma, hp->tau)) return rc;
    if (!isfinite(hp->target_entropy)) return fail(QSS_ERR_INVALID, "target_entropy must be finite, got %g", hp->target_entropy);
    if (int rc = check_adam_rates(hp->lr, hp->beta1, hp->beta2, hp->eps)) return rc;
    float *tr[4] = {trace ? trace->logp_out : nullptr, trace ? trace->vlogp_out : nullptr, trace ? trace->act_out : nullptr,
                    trace ? trace->fwd_out : nullptr};
    bool bad = misaligned(noise) || misaligned(noise_out) || !nets->alpha_state || misaligned(nets->alpha_state);
    for (int i = 0; i < 4; ++i) bad = bad || misaligned(tr[i]);
    const size_t need = sizeof(float) * (size_t)kWsFloats;
    if (int rc = check_tensors(bad, replay, indices, counts, stats, workspace, workspace_bytes, need, &nets->w[0][0], kNets, &nets->m[0][0],
                               &nets->v[0][0], kOnlineNets, grads))
        return rc;

    // the tensors of the call, where they lie in the workspace, and everything the call writes against each other
    CallTable<CopyArgs, 7> T;
    for (int k = 0; k < kNets; ++k) add_net(T, k, nets->w[k], net_at(k));
    for (int k = 0; k < kOnlineNets; ++k) {
        add_net(T, k, nets->m[k], kWsM + net_at(k));
        add_net(T, k, nets->v[k], kWsV + net_at(k));
    }
    const int ialpha = T.nt;
    T.add(nets->alpha_state, kWsAlpha, 1);               // log_alpha into its first place
    T.add(nets->alpha_state + 1, kWsAlpha + 2, 2);       // its m and v
    const int nstate = T.nt;
    if (grads)
        for (int k = 0; k < kOnlineNets; ++k) add_net(T, k, grads + 6 * k, kWsG + net_at(k));
    const size_t sb = (size_t)steps * (size_t)batch;
    T.writes(stats, 4 * (size_t)QSS_STATS * (size_t)steps);
    T.writes(workspace, need);
    if (noise_out) T.writes(noise_out, 4 * (size_t)kAct * sb);
    const size_t trn[4] = {sb, sb, kAct * sb, QSS_FWD * sb};
    for (int i = 0; i < 4; ++i)
        if (tr[i]) T.writes(tr[i], 4 * trn[i]);
    if (int rc = T.check_overlap()) return rc;

    float *ws = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_copy(k_sac_copy, T.in, nstate, ws, 1, st)) return rc;       // every net into its first place

    StepArgs S{};
    fill_step_head(S, ws, replay, hp, batch);
    S.te = (float)hp->target_entropy;
    S.auto_alpha = hp->auto_alpha;
    S.seed = seed;
    for (int s = 0; s < steps; ++s) {
        const int64_t u = t0 + s;
        const size_t so = (size_t)s * batch;
        S.lr_t = (float)(hp->lr * adam_corr(hp, (double)u + 1.0));
        S.indices = indices + so;
        S.counts = counts ? counts + s : nullptr;
        S.noise = noise ? noise + so * kAct : nullptr;
        S.noise_out = noise_out ? noise_out + so * kAct : nullptr;
        S.stats = stats + (size_t)QSS_STATS * s;
        S.logp_out = tr[0] ? tr[0] + so : nullptr;
        S.vlogp_out = tr[1] ? tr[1] + so : nullptr;
        S.act_out = tr[2] ? tr[2] + so * kAct : nullptr;
        S.fwd_out = tr[3] ? tr[3] + so * QSS_FWD : nullptr;
        S.u = (uint64_t)u;
        S.cur = s & 1;                           // every step writes every net: they all change places together
        S.want_grads = grads && s == steps - 1;
        hipLaunchKernelGGL(k_sac_step, dim3(4), dim3(kFitBlock), 0, st, S);
        HIP_TRY(hipGetLastError());
    }
    // every net and log_alpha from where they ended, the moments and the gradients back into the caller's tensors
    const int cur = steps & 1;
    for (int i = 0; i < 6 * kNets; ++i) T.out.at[i] += cur * kBuf;
    T.out.at[ialpha] += cur;
    return launch_copy(k_sac_copy, T.out, T.nt, ws, 0, st);
}

int qss_math(int32_t which, const float *in, float *out, int64_t n, void *stream)
{
    if (which < QSS_MATH_EXP || which > QSS_MATH_JAC) return fail(QSS_ERR_INVALID, "which must be in [0, 2], got %d", which);
    if (!in || !out || misaligned(in) || misaligned(out)) return fail(QSS_ERR_INVALID, "in and out must not be NULL and must be 4-byte aligned");
    if (n < 1 || n > 0x7fffffffll) return fail(QSS_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)n);
    hipLaunchKernelGGL(k_sac_math, dim3((unsigned)((n + kMathBlock - 1) / kMathBlock)), dim3(kMathBlock), 0, (hipStream_t)stream, (int)which, in, out, n);
    HIP_TRY(hipGetLastError());
    return QSS_OK;
}

}  // extern "C"
