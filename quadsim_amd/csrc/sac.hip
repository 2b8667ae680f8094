// sac.hip -- libquadsim_sac.so: the C ABI of include/quadsim_sac.h over the kernels of sac_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other ten libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the streamed nets, the backward pass and the Adam step), quadsim_device.hpp (q_tanh, q_ln, the Philox counter and the
// normals) and side_host.hpp (error text, the Adam and pointer checks).
#include "../../include/quadsim_sac.h"
#include "side_host.hpp"
#include "sac_kernels.hpp"

static_assert(QSS_OK == kOk && QSS_ERR_INVALID == kErrInvalid && QSS_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_sac.h");
static_assert(QSS_CHUNK == qsf::kRows && QSS_ACTOR == 0 && QSS_Q1 == 1 && QSS_Q2 == 2 && QSS_V == 3 && QSS_V_TARGET == 4 &&
                  QSS_NOISE_STREAM == (int)qssac::kStreamNoise && QSS_STATS == 8 && QSS_FWD == 5,
              "quadsim_sac.h states the kernels' geometry");

namespace {

using namespace qssac;

// the six tensors of the actor, of a critic and of a value net, and where each lies in a flat net
const int kElems[3][6] = {{kIn * kH, kH, kH * kH, kH, kH * kHead, kHead}, {kCIn * kH, kH, kH * kH, kH, kH, 1}, {kIn * kH, kH, kH * kH, kH, kH, 1}};
const int kAt[3][6] = {{FA::w0, FA::b0, FA::w1, FA::b1, FA::w2, FA::b2},
                       {FC::w0, FC::b0, FC::w1, FC::b1, FC::w2, FC::b2},
                       {FV::w0, FV::b0, FV::w1, FV::b1, FV::w2, FV::b2}};

struct Range {
    uintptr_t lo, hi;
};

// the shape of net k (the ABI's order): 0 the actor's, 1 a critic's, 2 a value net's
int shape_of(int k) { return k == 0 ? 0 : k < 3 ? 1 : 2; }

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
    if (!nets || !replay || !indices || !hp || !workspace || !stats)
        return fail(QSS_ERR_INVALID, "nets, replay, indices, hp, workspace and stats must not be NULL");
    if (nets->struct_size != sizeof(QssNets))
        return fail(QSS_ERR_INVALID, "QssNets.struct_size is %u, expected %zu", nets->struct_size, sizeof(QssNets));
    if (replay->struct_size != sizeof(QssReplay))
        return fail(QSS_ERR_INVALID, "QssReplay.struct_size is %u, expected %zu", replay->struct_size, sizeof(QssReplay));
    if (hp->struct_size != sizeof(QssHyper))
        return fail(QSS_ERR_INVALID, "QssHyper.struct_size is %u, expected %zu", hp->struct_size, sizeof(QssHyper));
    if (trace && trace->struct_size != sizeof(QssTrace))
        return fail(QSS_ERR_INVALID, "QssTrace.struct_size is %u, expected %zu", trace->struct_size, sizeof(QssTrace));
    if (batch < 1 || batch > QSS_MAX_BATCH) return fail(QSS_ERR_INVALID, "batch must be in [1, %d], got %d", QSS_MAX_BATCH, batch);
    if (steps < 1 || steps > QSS_MAX_STEPS) return fail(QSS_ERR_INVALID, "steps must be in [1, %d], got %d", QSS_MAX_STEPS, steps);
    if (replay->n < 1 || replay->n > 0x7fffffffll) return fail(QSS_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)replay->n);
    if (int rc = check_adam_t0(t0, steps, "steps")) return rc;
    if (hp->auto_alpha != 0 && hp->auto_alpha != 1) return fail(QSS_ERR_INVALID, "auto_alpha must be 0 or 1, got %d", hp->auto_alpha);
    if (!(hp->gamma >= 0.0 && hp->gamma <= 1.0)) return fail(QSS_ERR_INVALID, "gamma must be in [0, 1], got %g", hp->gamma);
    if (!(hp->tau > 0.0 && hp->tau <= 1.0)) return fail(QSS_ERR_INVALID, "tau must be in (0, 1], got %g", hp->tau);
    if (!isfinite(hp->target_entropy)) return fail(QSS_ERR_INVALID, "target_entropy must be finite, got %g", hp->target_entropy);
    if (int rc = check_adam_rates(hp->lr, hp->beta1, hp->beta2, hp->eps)) return rc;
    float *tr[4] = {trace ? trace->logp_out : nullptr, trace ? trace->vlogp_out : nullptr, trace ? trace->act_out : nullptr,
                    trace ? trace->fwd_out : nullptr};
    bool bad = misaligned(replay->obs0) || misaligned(replay->act) || misaligned(replay->rew) || misaligned(replay->obs1) ||
               misaligned(replay->done) || misaligned(indices) || misaligned(counts) || misaligned(stats) || misaligned(noise) ||
               misaligned(noise_out) || misaligned(workspace, 15) || !replay->obs0 || !replay->act || !replay->rew || !replay->obs1 ||
               !replay->done || !nets->alpha_state || misaligned(nets->alpha_state);
    for (int i = 0; i < 4; ++i) bad = bad || misaligned(tr[i]);
    for (int k = 0; k < kNets; ++k)
        for (int i = 0; i < 6; ++i) bad = bad || !nets->w[k][i] || misaligned(nets->w[k][i]);
    for (int k = 0; k < kOnlineNets; ++k)
        for (int i = 0; i < 6; ++i)
            bad = bad || !nets->m[k][i] || misaligned(nets->m[k][i]) || !nets->v[k][i] || misaligned(nets->v[k][i]) ||
                  (grads && (!grads[6 * k + i] || misaligned(grads[6 * k + i])));
    if (bad) return fail(QSS_ERR_INVALID, "a tensor of the nets, of the replay or of the call is NULL or not aligned");
    const size_t need = sizeof(float) * (size_t)kWsFloats;
    if (workspace_bytes < need)
        return fail(QSS_ERR_INVALID, "the workspace has %llu bytes, the call needs %zu", (unsigned long long)workspace_bytes, need);

    // the tensors of the call, where they lie in the workspace, and everything the call writes against each other
    CopyArgs in{}, out{};
    Range rs[kCopyTensors + 7];
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
            add(nets->m[k][i], kWsM + net_at(k) + kAt[shape_of(k)][i], kElems[shape_of(k)][i]);
            add(nets->v[k][i], kWsV + net_at(k) + kAt[shape_of(k)][i], kElems[shape_of(k)][i]);
        }
    const int ialpha = nt;
    add(nets->alpha_state, kWsAlpha, 1);                 // log_alpha into its first place
    add(nets->alpha_state + 1, kWsAlpha + 2, 2);         // its m and v
    const int nstate = nt;
    if (grads)
        for (int k = 0; k < kOnlineNets; ++k)
            for (int i = 0; i < 6; ++i) add(grads[6 * k + i], kWsG + net_at(k) + kAt[shape_of(k)][i], kElems[shape_of(k)][i]);
    int nr = nt;
    const size_t sb = (size_t)steps * (size_t)batch;
    rs[nr++] = Range{(uintptr_t)stats, (uintptr_t)stats + 4 * (size_t)QSS_STATS * (size_t)steps};
    rs[nr++] = Range{(uintptr_t)workspace, (uintptr_t)workspace + need};
    if (noise_out) rs[nr++] = Range{(uintptr_t)noise_out, (uintptr_t)noise_out + 4 * (size_t)kAct * sb};
    const size_t trn[4] = {sb, sb, kAct * sb, QSS_FWD * sb};
    for (int i = 0; i < 4; ++i)
        if (tr[i]) rs[nr++] = Range{(uintptr_t)tr[i], (uintptr_t)tr[i] + 4 * trn[i]};
    for (int a = 0; a < nr; ++a)
        for (int b = a + 1; b < nr; ++b)
            if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) return fail(QSS_ERR_INVALID, "two tensors the call writes overlap");

    float *ws = (float *)workspace;
    hipStream_t st = (hipStream_t)stream;
    in.ws = out.ws = ws;
    in.to_ws = 1;
    hipLaunchKernelGGL(k_sac_copy, dim3((unsigned)nstate), dim3(kCopyBlock), 0, st, in);        // every net into its first place
    HIP_TRY(hipGetLastError());

    StepArgs S{};
    S.ws = ws;
    S.obs0 = replay->obs0; S.act = replay->act; S.rew = replay->rew; S.obs1 = replay->obs1; S.done = replay->done;
    S.b1f = (float)hp->beta1; S.b2f = (float)hp->beta2; S.omb1 = (float)(1.0 - hp->beta1); S.omb2 = (float)(1.0 - hp->beta2);
    S.eps = (float)hp->eps;
    S.gamma = (float)hp->gamma; S.tau = (float)hp->tau; S.omt = (float)(1.0 - hp->tau);
    S.te = (float)hp->target_entropy;
    S.auto_alpha = hp->auto_alpha;
    S.batch = batch;
    S.seed = seed;
    auto corr = [&](double tt) { return sqrt(1.0 - pow(hp->beta2, tt)) / (1.0 - pow(hp->beta1, tt)); };
    for (int s = 0; s < steps; ++s) {
        const int64_t u = t0 + s;
        const size_t so = (size_t)s * batch;
        S.lr_t = (float)(hp->lr * corr((double)u + 1.0));
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
    for (int i = 0; i < 6 * kNets; ++i) out.at[i] += cur * kBuf;
    out.at[ialpha] += cur;
    out.to_ws = 0;
    hipLaunchKernelGGL(k_sac_copy, dim3((unsigned)nt), dim3(kCopyBlock), 0, st, out);
    HIP_TRY(hipGetLastError());
    return QSS_OK;
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
