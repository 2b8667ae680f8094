// ddpg.hip -- libquadsim_ddpg.so: the C ABI of include/quadsim_ddpg.h over the kernels of ddpg_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other seven libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the backward pass and the Adam step), quadsim_device.hpp (q_tanh) and side_offpolicy.hpp on side_host.hpp (error text, the
// checks, the table of the call's tensors and the copy launches).
#include "../../include/quadsim_ddpg.h"
#include "side_offpolicy.hpp"
#include "ddpg_kernels.hpp"

static_assert(QSDD_OK == kOk && QSDD_ERR_INVALID == kErrInvalid && QSDD_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_ddpg.h");
static_assert(QSDD_CHUNK == qsf::kRows && QSDD_ACTOR == 0 && QSDD_CRITIC == 1, "quadsim_ddpg.h states the kernels' geometry");

namespace {

using namespace qsdd;

// the six tensors of net `which` (the ABI's order: 0 an actor, 1 a critic) that lie at `at`, into the call's table
template <class Table>
void add_net(Table &T, int which, float *const *six, int at)
{
    if (which == 0) T.template add_net<Flat<1>>(six, at);
    else T.template add_net<Flat<0>>(six, at);
}

// the flat place of net `which` in a buffer, in the moments or in the gradients
int flat_at(int which) { return net_at(which == 0 ? 1 : 0); }

}  // namespace

extern "C" {

int qsdd_version(void) { return QSDD_VERSION; }

const char *qsdd_last_error(void) { return g_err; }

int qsdd_workspace_bytes(size_t *bytes)
{
    if (!bytes) return fail(QSDD_ERR_INVALID, "bytes must not be NULL");
    *bytes = sizeof(float) * (size_t)kWsFloats;
    return QSDD_OK;
}

int qsdd_update(const QsddNets *nets, const QsddReplay *replay, const int32_t *indices, const int32_t *counts, int32_t steps,
                int32_t batch, const QsddHyper *hp, int64_t t0, void *workspace, uint64_t workspace_bytes, float *stats,
                float *const *grads, void *stream)
{
    if (int rc = check_call(nets, replay, indices, hp, workspace, stats, "Qsdd")) return rc;
    if (int rc = check_extent(batch, QSDD_MAX_BATCH, steps, QSDD_MAX_STEPS, replay->n, t0)) return rc;
    if (int rc = check_discount(hp->gamma, hp->tau)) return rc;
    if (!(hp->obs_clip > 0.0)) return fail(QSDD_ERR_INVALID, "obs_clip must be > 0 (inf: no clamp), got %g", hp->obs_clip);
    if (!isfinite(hp->actor_lr)) return fail(QSDD_ERR_INVALID, "actor_lr must be finite, got %g", hp->actor_lr);
    if (!isfinite(hp->critic_lr)) return fail(QSDD_ERR_INVALID, "critic_lr must be finite, got %g", hp->critic_lr);
    if (int rc = check_adam_rates(0.0, hp->beta1, hp->beta2, hp->eps)) return rc;
    const size_t need = sizeof(float) * (size_t)kWsFloats;
    if (int rc = check_tensors(false, replay, indices, counts, stats, workspace, workspace_bytes, need, &nets->w[0][0], 4, &nets->m[0][0],
                               &nets->v[0][0], 2, grads))
        return rc;

    // the tensors of the call, where they lie in the workspace, and everything the call writes against each other
    CallTable<CopyArgs, 2> T;
    for (int k = 0; k < 4; ++k) add_net(T, k & 1, nets->w[k], flat_at(k & 1) + (k >> 1) * kOnline);
    for (int k = 0; k < 2; ++k) {
        add_net(T, k, nets->m[k], kWsM + flat_at(k));
        add_net(T, k, nets->v[k], kWsV + flat_at(k));
    }
    const int nstate = T.nt;
    if (grads)
        for (int k = 0; k < 2; ++k) add_net(T, k, grads + 6 * k, kWsG + flat_at(k));
    T.writes(stats, 4 * (size_t)QSDD_STATS * (size_t)steps);
    T.writes(workspace, need);
    if (int rc = T.check_overlap()) return rc;

    float *ws = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_copy(k_ddpg_copy, T.in, nstate, ws, 1, st)) return rc;      // the weights into buffer 0

    StepArgs S{};
    fill_step_head(S, ws, replay, hp, batch);
    S.clip = (float)hp->obs_clip;
    for (int s = 0; s < steps; ++s) {
        const double corr = adam_corr(hp, (double)(t0 + s) + 1.0);
        S.lr_t[0] = (float)(hp->critic_lr * corr);
        S.lr_t[1] = (float)(hp->actor_lr * corr);
        S.indices = indices + (int64_t)s * batch;
        S.counts = counts ? counts + s : nullptr;
        S.stats = stats + (size_t)QSDD_STATS * s;
        S.cur = s & 1;
        S.want_grads = grads && s == steps - 1;
        hipLaunchKernelGGL(k_ddpg_step, dim3(2), dim3(kFitBlock), 0, st, S);
        HIP_TRY(hipGetLastError());
    }
    // the final buffer, the moments and the gradients back into the caller's tensors
    for (int i = 0; i < 24; ++i) T.out.at[i] += (steps & 1) * kBuf;
    return launch_copy(k_ddpg_copy, T.out, T.nt, ws, 0, st);
}

}  // extern "C"
