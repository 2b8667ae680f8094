// td3.hip -- libquadsim_td3.so: the C ABI of include/quadsim_td3.h over the kernels of td3_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other nine libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the streamed nets, the backward pass and the Adam step), quadsim_device.hpp (q_tanh, the Philox counter and the normals)
// and side_offpolicy.hpp on side_host.hpp (error text, the checks, the table of the call's tensors and the copy launches).
#include "../../include/quadsim_td3.h"
#include "side_offpolicy.hpp"
#include "td3_kernels.hpp"

static_assert(QSTD_OK == kOk && QSTD_ERR_INVALID == kErrInvalid && QSTD_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_td3.h");
static_assert(QSTD_CHUNK == qsf::kRows && QSTD_ACTOR == 0 && QSTD_Q1 == 1 && QSTD_Q2 == 2 && QSTD_ACTOR_TARGET == 3 &&
                  QSTD_NOISE_STREAM == (int)qstd::kStreamNoise && QSTD_STATS == 6,
              "quadsim_td3.h states the kernels' geometry");

namespace {

using namespace qstd;

// the six tensors of net k (the ABI's order: the actor's shape, then two critics', for the online nets and again for the targets)
// that lie at `at`, into the call's table
template <class Table>
void add_net(Table &T, int k, float *const *six, int at)
{
    if (k % kOnlineNets == 0) T.template add_net<Flat<1>>(six, at);
    else T.template add_net<Flat<0>>(six, at);
}

}  // namespace

extern "C" {

int qstd_version(void) { return QSTD_VERSION; }

const char *qstd_last_error(void) { return g_err; }

int qstd_workspace_bytes(size_t *bytes)
{
    if (!bytes) return fail(QSTD_ERR_INVALID, "bytes must not be NULL");
    *bytes = sizeof(float) * (size_t)kWsFloats;
    return QSTD_OK;
}

int qstd_update(const QstdNets *nets, const QstdReplay *replay, const int32_t *indices, const int32_t *counts, int32_t steps,
                int32_t batch, const QstdHyper *hp, int64_t t0, int64_t actor_t0, const float *noise, uint64_t seed, float *noise_out,
                void *workspace, uint64_t workspace_bytes, float *stats, float *const *grads, void *stream)
{
    if (int rc = check_call(nets, replay, indices, hp, workspace, stats, "Qstd")) return rc;
    if (int rc = check_extent(batch, QSTD_MAX_BATCH, steps, QSTD_MAX_STEPS, replay->n, t0)) return rc;
    if (actor_t0 < 0 || actor_t0 + steps > 0x7fffffffll)
        return fail(QSTD_ERR_INVALID, "actor_t0 must be >= 0 with actor_t0 + steps below 2^31, got %lld", (long long)actor_t0);
    if (hp->policy_delay < 1 || hp->policy_delay > QSTD_MAX_DELAY)
        return fail(QSTD_ERR_INVALID, "policy_delay must be in [1, %d], got %d", QSTD_MAX_DELAY, hp->policy_delay);
    if (int rc = check_discount(hp->gamma, hp->tau)) return rc;
    if (!(hp->target_policy_noise >= 0.0) || !isfinite(hp->target_policy_noise))
        return fail(QSTD_ERR_INVALID, "target_policy_noise must be finite and >= 0, got %g", hp->target_policy_noise);
    if (!(hp->target_noise_clip >= 0.0)) return fail(QSTD_ERR_INVALID, "target_noise_clip must be >= 0 (inf: no clip), got %g", hp->target_noise_clip);
    if (!isfinite(hp->actor_lr)) return fail(QSTD_ERR_INVALID, "actor_lr must be finite, got %g", hp->actor_lr);
    if (!isfinite(hp->critic_lr)) return fail(QSTD_ERR_INVALID, "critic_lr must be finite, got %g", hp->critic_lr);
    if (int rc = check_adam_rates(0.0, hp->beta1, hp->beta2, hp->eps)) return rc;
    const size_t need = sizeof(float) * (size_t)kWsFloats;
    if (int rc = check_tensors(misaligned(noise) || misaligned(noise_out), replay, indices, counts, stats, workspace, workspace_bytes, need,
                               &nets->w[0][0], kNets, &nets->m[0][0], &nets->v[0][0], kOnlineNets, grads))
        return rc;

    // the tensors of the call, where they lie in the workspace, and everything the call writes against each other
    CallTable<CopyArgs, 3> T;
    for (int k = 0; k < kNets; ++k) add_net(T, k, nets->w[k], net_at(k));
    for (int k = 0; k < kOnlineNets; ++k) {
        add_net(T, k, nets->m[k], kWsM + online_at(k));
        add_net(T, k, nets->v[k], kWsV + online_at(k));
    }
    const int nstate = T.nt;
    if (grads)
        for (int k = 0; k < kOnlineNets; ++k) add_net(T, k, grads + 6 * k, kWsG + online_at(k));
    T.writes(stats, 4 * (size_t)QSTD_STATS * (size_t)steps);
    T.writes(workspace, need);
    if (noise_out) T.writes(noise_out, 4 * (size_t)kAct * (size_t)batch * (size_t)steps);
    if (int rc = T.check_overlap()) return rc;

    float *ws = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_copy(k_td3_copy, T.in, nstate, ws, 1, st)) return rc;       // every net into its first place

    StepArgs S{};
    fill_step_head(S, ws, replay, hp, batch);
    S.sigma = (float)hp->target_policy_noise; S.cl = (float)hp->target_noise_clip;
    S.seed = seed;
    int cur = 0, last_actor = 0;                 // bit k: the place that holds net k
    int64_t actor_steps = 0;
    for (int s = 0; s < steps; ++s) {
        const int64_t u = t0 + s;
        const int actor_step = u % hp->policy_delay == 0;
        S.lr_t[0] = (float)(hp->critic_lr * adam_corr(hp, (double)u + 1.0));
        S.lr_t[1] = (float)(hp->actor_lr * adam_corr(hp, (double)(actor_t0 + actor_steps) + 1.0));
        S.indices = indices + (int64_t)s * batch;
        S.counts = counts ? counts + s : nullptr;
        S.noise = noise ? noise + (size_t)s * batch * kAct : nullptr;
        S.noise_out = noise_out ? noise_out + (size_t)s * batch * kAct : nullptr;
        S.stats = stats + (size_t)QSTD_STATS * s;
        S.u = (uint64_t)u;
        S.cur = cur;
        S.actor_step = actor_step;
        S.want_grads = grads && s == steps - 1;
        hipLaunchKernelGGL(k_td3_step, dim3(actor_step ? 3 : 2), dim3(kFitBlock), 0, st, S);
        HIP_TRY(hipGetLastError());
        cur ^= actor_step ? 0x3f : 0x06;         // the nets the step wrote changed places
        actor_steps += actor_step;
        last_actor = actor_step;
    }
    // every net from where it ended, the moments and the gradients back into the caller's tensors
    for (int k = 0; k < kNets; ++k)
        for (int i = 0; i < 6; ++i) T.out.at[6 * k + i] += ((cur >> k) & 1) * kBuf;
    if (grads && !last_actor)
        for (int i = 0; i < 6; ++i) T.out.t[nstate + i] = nullptr;     // no actor step: no actor gradient
    return launch_copy(k_td3_copy, T.out, T.nt, ws, 0, st);
}

}  // extern "C"
