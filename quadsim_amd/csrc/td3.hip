// td3.hip -- libquadsim_td3.so: the C ABI of include/quadsim_td3.h over the kernels of td3_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other nine libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the streamed nets, the backward pass and the Adam step), quadsim_device.hpp (q_tanh, the Philox counter and the normals)
// and side_host.hpp (error text, the Adam and pointer checks).
#include "../../include/quadsim_td3.h"
#include "side_host.hpp"
#include "td3_kernels.hpp"

static_assert(QSTD_OK == kOk && QSTD_ERR_INVALID == kErrInvalid && QSTD_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_td3.h");
static_assert(QSTD_CHUNK == qsf::kRows && QSTD_ACTOR == 0 && QSTD_Q1 == 1 && QSTD_Q2 == 2 && QSTD_ACTOR_TARGET == 3 &&
                  QSTD_NOISE_STREAM == (int)qstd::kStreamNoise && QSTD_STATS == 6,
              "quadsim_td3.h states the kernels' geometry");

namespace {

using namespace qstd;

// the six tensors of the actor and of a critic, and where each lies in a flat net
const int kElems[2][6] = {{kIn * kH, kH, kH * kH, kH, kH * kAct, kAct}, {kCIn * kH, kH, kH * kH, kH, kH, 1}};
const int kAt[2][6] = {{Flat<1>::w0, Flat<1>::b0, Flat<1>::w1, Flat<1>::b1, Flat<1>::w2, Flat<1>::b2},
                       {Flat<0>::w0, Flat<0>::b0, Flat<0>::w1, Flat<0>::b1, Flat<0>::w2, Flat<0>::b2}};

struct Range {
    uintptr_t lo, hi;
};

// the shape of net k (the ABI's order): 0 the actor's, 1 a critic's
int shape_of(int k) { return k % kOnlineNets == 0 ? 0 : 1; }

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
    if (!nets || !replay || !indices || !hp || !workspace || !stats)
        return fail(QSTD_ERR_INVALID, "nets, replay, indices, hp, workspace and stats must not be NULL");
    if (nets->struct_size != sizeof(QstdNets))
        return fail(QSTD_ERR_INVALID, "QstdNets.struct_size is %u, expected %zu", nets->struct_size, sizeof(QstdNets));
    if (replay->struct_size != sizeof(QstdReplay))
        return fail(QSTD_ERR_INVALID, "QstdReplay.struct_size is %u, expected %zu", replay->struct_size, sizeof(QstdReplay));
    if (hp->struct_size != sizeof(QstdHyper))
        return fail(QSTD_ERR_INVALID, "QstdHyper.struct_size is %u, expected %zu", hp->struct_size, sizeof(QstdHyper));
    if (batch < 1 || batch > QSTD_MAX_BATCH) return fail(QSTD_ERR_INVALID, "batch must be in [1, %d], got %d", QSTD_MAX_BATCH, batch);
    if (steps < 1 || steps > QSTD_MAX_STEPS) return fail(QSTD_ERR_INVALID, "steps must be in [1, %d], got %d", QSTD_MAX_STEPS, steps);
    if (replay->n < 1 || replay->n > 0x7fffffffll) return fail(QSTD_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)replay->n);
    if (int rc = check_adam_t0(t0, steps, "steps")) return rc;
    if (actor_t0 < 0 || actor_t0 + steps > 0x7fffffffll)
        return fail(QSTD_ERR_INVALID, "actor_t0 must be >= 0 with actor_t0 + steps below 2^31, got %lld", (long long)actor_t0);
    if (hp->policy_delay < 1 || hp->policy_delay > QSTD_MAX_DELAY)
        return fail(QSTD_ERR_INVALID, "policy_delay must be in [1, %d], got %d", QSTD_MAX_DELAY, hp->policy_delay);
    if (!(hp->gamma >= 0.0 && hp->gamma <= 1.0)) return fail(QSTD_ERR_INVALID, "gamma must be in [0, 1], got %g", hp->gamma);
    if (!(hp->tau > 0.0 && hp->tau <= 1.0)) return fail(QSTD_ERR_INVALID, "tau must be in (0, 1], got %g", hp->tau);
    if (!(hp->target_policy_noise >= 0.0) || !isfinite(hp->target_policy_noise))
        return fail(QSTD_ERR_INVALID, "target_policy_noise must be finite and >= 0, got %g", hp->target_policy_noise);
    if (!(hp->target_noise_clip >= 0.0)) return fail(QSTD_ERR_INVALID, "target_noise_clip must be >= 0 (inf: no clip), got %g", hp->target_noise_clip);
    if (!isfinite(hp->actor_lr)) return fail(QSTD_ERR_INVALID, "actor_lr must be finite, got %g", hp->actor_lr);
    if (!isfinite(hp->critic_lr)) return fail(QSTD_ERR_INVALID, "critic_lr must be finite, got %g", hp->critic_lr);
    if (int rc = check_adam_rates(0.0, hp->beta1, hp->beta2, hp->eps)) return rc;
    bool bad = misaligned(replay->obs0) || misaligned(replay->act) || misaligned(replay->rew) || misaligned(replay->obs1) ||
               misaligned(replay->done) || misaligned(indices) || misaligned(counts) || misaligned(stats) || misaligned(noise) ||
               misaligned(noise_out) || misaligned(workspace, 15) || !replay->obs0 || !replay->act || !replay->rew || !replay->obs1 ||
               !replay->done;
    for (int k = 0; k < kNets; ++k)
        for (int i = 0; i < 6; ++i) bad = bad || !nets->w[k][i] || misaligned(nets->w[k][i]);
    for (int k = 0; k < kOnlineNets; ++k)
        for (int i = 0; i < 6; ++i)
            bad = bad || !nets->m[k][i] || misaligned(nets->m[k][i]) || !nets->v[k][i] || misaligned(nets->v[k][i]) ||
                  (grads && (!grads[6 * k + i] || misaligned(grads[6 * k + i])));
    if (bad) return fail(QSTD_ERR_INVALID, "a tensor of the nets, of the replay or of the call is NULL or not aligned");
    const size_t need = sizeof(float) * (size_t)kWsFloats;
    if (workspace_bytes < need)
        return fail(QSTD_ERR_INVALID, "the workspace has %llu bytes, the call needs %zu", (unsigned long long)workspace_bytes, need);

    // the tensors of the call, where they lie in the workspace, and everything the call writes against each other
    CopyArgs in{}, out{};
    Range rs[kCopyTensors + 3];
    int nt = 0;
    auto add = [&](float *p, int at, int n) {
        in.t[nt] = out.t[nt] = p;
        in.at[nt] = out.at[nt] = at;
        in.n[nt] = out.n[nt] = n;
        rs[nt] = Range{(uintptr_t)p, (uintptr_t)p + 4 * (size_t)n};
        ++nt;
    };
    for (int k = 0; k < kNets; ++k)
        for (int i = 0; i < 6; ++i) add(nets->w[k][i], net_at(k) + kAt[shape_of(k)][i], kElems[shape_of(k)][i]);
    for (int k = 0; k < kOnlineNets; ++k)
        for (int i = 0; i < 6; ++i) {
            add(nets->m[k][i], kWsM + online_at(k) + kAt[shape_of(k)][i], kElems[shape_of(k)][i]);
            add(nets->v[k][i], kWsV + online_at(k) + kAt[shape_of(k)][i], kElems[shape_of(k)][i]);
        }
    const int nstate = nt;
    if (grads)
        for (int k = 0; k < kOnlineNets; ++k)
            for (int i = 0; i < 6; ++i) add(grads[6 * k + i], kWsG + online_at(k) + kAt[shape_of(k)][i], kElems[shape_of(k)][i]);
    int nr = nt;
    rs[nr++] = Range{(uintptr_t)stats, (uintptr_t)stats + 4 * (size_t)QSTD_STATS * (size_t)steps};
    rs[nr++] = Range{(uintptr_t)workspace, (uintptr_t)workspace + need};
    if (noise_out) rs[nr++] = Range{(uintptr_t)noise_out, (uintptr_t)noise_out + 4 * (size_t)kAct * (size_t)batch * (size_t)steps};
    for (int a = 0; a < nr; ++a)
        for (int b = a + 1; b < nr; ++b)
            if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) return fail(QSTD_ERR_INVALID, "two tensors the call writes overlap");

    float *ws = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    in.ws = out.ws = ws;
    in.to_ws = 1;
    hipLaunchKernelGGL(k_td3_copy, dim3((unsigned)nstate), dim3(kCopyBlock), 0, st, in);        // every net into its first place
    HIP_TRY(hipGetLastError());

    StepArgs S{};
    S.ws = ws;
    S.obs0 = replay->obs0; S.act = replay->act; S.rew = replay->rew; S.obs1 = replay->obs1; S.done = replay->done;
    S.b1f = (float)hp->beta1; S.b2f = (float)hp->beta2; S.omb1 = (float)(1.0 - hp->beta1); S.omb2 = (float)(1.0 - hp->beta2);
    S.eps = (float)hp->eps;
    S.gamma = (float)hp->gamma; S.tau = (float)hp->tau; S.omt = (float)(1.0 - hp->tau);
    S.sigma = (float)hp->target_policy_noise; S.cl = (float)hp->target_noise_clip;
    S.batch = batch;
    S.seed = seed;
    auto corr = [&](double tt) { return sqrt(1.0 - pow(hp->beta2, tt)) / (1.0 - pow(hp->beta1, tt)); };
    int cur = 0, last_actor = 0;                 // bit k: the place that holds net k
    int64_t actor_steps = 0;
    for (int s = 0; s < steps; ++s) {
        const int64_t u = t0 + s;
        const int actor_step = u % hp->policy_delay == 0;
        S.lr_t[0] = (float)(hp->critic_lr * corr((double)u + 1.0));
        S.lr_t[1] = (float)(hp->actor_lr * corr((double)(actor_t0 + actor_steps) + 1.0));
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
        for (int i = 0; i < 6; ++i) out.at[6 * k + i] += ((cur >> k) & 1) * kBuf;
    if (grads && !last_actor)
        for (int i = 0; i < 6; ++i) out.t[nstate + i] = nullptr;       // no actor step: no actor gradient
    out.to_ws = 0;
    hipLaunchKernelGGL(k_td3_copy, dim3((unsigned)nt), dim3(kCopyBlock), 0, st, out);
    HIP_TRY(hipGetLastError());
    return QSTD_OK;
}

}  // extern "C"
