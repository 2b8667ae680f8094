// ddpg.hip -- libquadsim_ddpg.so: the C ABI of include/quadsim_ddpg.h over the kernels of ddpg_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other seven libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the backward pass and the Adam step), quadsim_device.hpp (q_tanh) and side_host.hpp (error
// text, the Adam and pointer checks).
#include "../../include/quadsim_ddpg.h"
#include "side_host.hpp"
#include "ddpg_kernels.hpp"

static_assert(QSDD_OK == kOk && QSDD_ERR_INVALID == kErrInvalid && QSDD_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_ddpg.h");
static_assert(QSDD_CHUNK == qsf::kRows && QSDD_ACTOR == 0 && QSDD_CRITIC == 1, "quadsim_ddpg.h states the kernels' geometry");

namespace {

using namespace qsdd;

// the six tensors of the actor and of the critic, and where each lies in a flat net
const int kElems[2][6] = {{kIn * kH, kH, kH * kH, kH, kH * kAct, kAct}, {kIn * kH, kH, (kH + kAct) * kH, kH, kH, 1}};
const int kAt[2][6] = {{Flat<1>::w0, Flat<1>::b0, Flat<1>::w1, Flat<1>::b1, Flat<1>::w2, Flat<1>::b2},
                       {Flat<0>::w0, Flat<0>::b0, Flat<0>::w1, Flat<0>::b1, Flat<0>::w2, Flat<0>::b2}};

struct Range {
    uintptr_t lo, hi;
};

// the flat place of net `which` (the ABI's order: 0 actor, 1 critic) in a buffer, in the moments or in the gradients
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
    if (!nets || !replay || !indices || !hp || !workspace || !stats)
        return fail(QSDD_ERR_INVALID, "nets, replay, indices, hp, workspace and stats must not be NULL");
    if (nets->struct_size != sizeof(QsddNets))
        return fail(QSDD_ERR_INVALID, "QsddNets.struct_size is %u, expected %zu", nets->struct_size, sizeof(QsddNets));
    if (replay->struct_size != sizeof(QsddReplay))
        return fail(QSDD_ERR_INVALID, "QsddReplay.struct_size is %u, expected %zu", replay->struct_size, sizeof(QsddReplay));
    if (hp->struct_size != sizeof(QsddHyper))
        return fail(QSDD_ERR_INVALID, "QsddHyper.struct_size is %u, expected %zu", hp->struct_size, sizeof(QsddHyper));
    if (batch < 1 || batch > QSDD_MAX_BATCH) return fail(QSDD_ERR_INVALID, "batch must be in [1, %d], got %d", QSDD_MAX_BATCH, batch);
    if (steps < 1 || steps > QSDD_MAX_STEPS) return fail(QSDD_ERR_INVALID, "steps must be in [1, %d], got %d", QSDD_MAX_STEPS, steps);
    if (replay->n < 1 || replay->n > 0x7fffffffll) return fail(QSDD_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)replay->n);
    if (int rc = check_adam_t0(t0, steps, "steps")) return rc;
    if (!(hp->gamma >= 0.0 && hp->gamma <= 1.0)) return fail(QSDD_ERR_INVALID, "gamma must be in [0, 1], got %g", hp->gamma);
    if (!(hp->tau > 0.0 && hp->tau <= 1.0)) return fail(QSDD_ERR_INVALID, "tau must be in (0, 1], got %g", hp->tau);
    if (!(hp->obs_clip > 0.0)) return fail(QSDD_ERR_INVALID, "obs_clip must be > 0 (inf: no clamp), got %g", hp->obs_clip);
    if (!isfinite(hp->actor_lr)) return fail(QSDD_ERR_INVALID, "actor_lr must be finite, got %g", hp->actor_lr);
    if (!isfinite(hp->critic_lr)) return fail(QSDD_ERR_INVALID, "critic_lr must be finite, got %g", hp->critic_lr);
    if (int rc = check_adam_rates(0.0, hp->beta1, hp->beta2, hp->eps)) return rc;
    bool bad = misaligned(replay->obs0) || misaligned(replay->act) || misaligned(replay->rew) || misaligned(replay->obs1) ||
               misaligned(replay->done) || misaligned(indices) || misaligned(counts) || misaligned(stats) || misaligned(workspace, 15) ||
               !replay->obs0 || !replay->act || !replay->rew || !replay->obs1 || !replay->done;
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 6; ++i) bad = bad || !nets->w[k][i] || misaligned(nets->w[k][i]);
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 6; ++i)
            bad = bad || !nets->m[k][i] || misaligned(nets->m[k][i]) || !nets->v[k][i] || misaligned(nets->v[k][i]) ||
                  (grads && (!grads[6 * k + i] || misaligned(grads[6 * k + i])));
    if (bad) return fail(QSDD_ERR_INVALID, "a tensor of the nets, of the replay or of the call is NULL or not aligned");
    const size_t need = sizeof(float) * (size_t)kWsFloats;
    if (workspace_bytes < need)
        return fail(QSDD_ERR_INVALID, "the workspace has %llu bytes, the call needs %zu", (unsigned long long)workspace_bytes, need);

    // the tensors of the call, where they lie in the workspace, and everything the call writes against each other
    CopyArgs in{}, out{};
    Range rs[kCopyTensors + 2];
    int nt = 0;
    auto add = [&](float *p, int at, int n) {
        in.t[nt] = out.t[nt] = p;
        in.at[nt] = out.at[nt] = at;
        in.n[nt] = out.n[nt] = n;
        rs[nt] = Range{(uintptr_t)p, (uintptr_t)p + 4 * (size_t)n};
        ++nt;
    };
    for (int k = 0; k < 4; ++k)
        for (int i = 0; i < 6; ++i) add(nets->w[k][i], flat_at(k & 1) + (k >> 1) * kOnline + kAt[k & 1][i], kElems[k & 1][i]);
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 6; ++i) {
            add(nets->m[k][i], kWsM + flat_at(k) + kAt[k][i], kElems[k][i]);
            add(nets->v[k][i], kWsV + flat_at(k) + kAt[k][i], kElems[k][i]);
        }
    const int nstate = nt;
    if (grads)
        for (int k = 0; k < 2; ++k)
            for (int i = 0; i < 6; ++i) add(grads[6 * k + i], kWsG + flat_at(k) + kAt[k][i], kElems[k][i]);
    int nr = nt;
    rs[nr++] = Range{(uintptr_t)stats, (uintptr_t)stats + 4 * (size_t)QSDD_STATS * (size_t)steps};
    rs[nr++] = Range{(uintptr_t)workspace, (uintptr_t)workspace + need};
    for (int a = 0; a < nr; ++a)
        for (int b = a + 1; b < nr; ++b)
            if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) return fail(QSDD_ERR_INVALID, "two tensors the call writes overlap");

    float *ws = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    in.ws = out.ws = ws;
    in.to_ws = 1;
    hipLaunchKernelGGL(k_ddpg_copy, dim3((unsigned)nstate), dim3(kCopyBlock), 0, st, in);       // the weights into buffer 0
    HIP_TRY(hipGetLastError());

    StepArgs S{};
    S.ws = ws;
    S.obs0 = replay->obs0; S.act = replay->act; S.rew = replay->rew; S.obs1 = replay->obs1; S.done = replay->done;
    S.b1f = (float)hp->beta1; S.b2f = (float)hp->beta2; S.omb1 = (float)(1.0 - hp->beta1); S.omb2 = (float)(1.0 - hp->beta2);
    S.eps = (float)hp->eps;
    S.gamma = (float)hp->gamma; S.tau = (float)hp->tau; S.omt = (float)(1.0 - hp->tau); S.clip = (float)hp->obs_clip;
    S.batch = batch;
    for (int s = 0; s < steps; ++s) {
        const double tt = (double)(t0 + s) + 1.0, corr = sqrt(1.0 - pow(hp->beta2, tt)) / (1.0 - pow(hp->beta1, tt));
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
    for (int i = 0; i < 24; ++i) out.at[i] += (steps & 1) * kBuf;
    out.to_ws = 0;
    hipLaunchKernelGGL(k_ddpg_copy, dim3((unsigned)nt), dim3(kCopyBlock), 0, st, out);
    HIP_TRY(hipGetLastError());
    return QSDD_OK;
}

}  // extern "C"
