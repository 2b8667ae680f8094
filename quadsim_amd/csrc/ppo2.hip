// ppo2.hip -- libquadsim_ppo.so: the C ABI of include/quadsim_ppo.h over the kernels of ppo2_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other five libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the backward pass and the Adam step), and side_host.hpp (error text, the Adam and pointer checks).
#include "../../include/quadsim_ppo.h"
#include "side_host.hpp"
#include "ppo2_kernels.hpp"

static_assert(QSP_OK == kOk && QSP_ERR_INVALID == kErrInvalid && QSP_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_ppo.h");
static_assert(QSP_TENSORS == qsp::kTensors && QSP_CHUNK == qsf::kRows, "quadsim_ppo.h states the kernels' geometry");

namespace {

using namespace qsp;

const int kElems[kTensors] = {kIn * kH, kH, kH * kH, kH, kH * kOut, kOut, kIn * kH, kH, kH * kH, kH, kH, 1, kOut};
// the slot's place in the partial of the policy branch and of the value branch (towers); the shared layout adds w0, b0 to the
// value branch and has no slots 6, 7
const int kLocPolicy[kTensors] = {kLW0, kLB0, kLW1, kLB1, kLW2, kLB2, -1, -1, -1, -1, -1, -1, kLLS};
const int kLocValue[kTensors] = {-1, -1, -1, -1, -1, -1, kLW0, kLB0, kLW1, kLB1, kLW2, kLB2, -1};

struct Range {
    uintptr_t lo, hi;
};

// the workspace: doubles first
struct Workspace {
    size_t statp, ssq, adv, part, gflat, bytes;
};

int64_t chunks_of(int64_t batch) { return (batch + QSP_CHUNK - 1) / QSP_CHUNK; }

Workspace workspace_of(int slices)
{
    Workspace W{};
    const size_t nblk = ((size_t)kPart * 2 + kElemBlock - 1) / kElemBlock;      // an upper bound of either layout's blocks
    size_t at = 0;
    W.statp = at; at += sizeof(double) * 8 * (size_t)slices;
    W.ssq = at; at += sizeof(double) * nblk;
    W.adv = at; at += sizeof(float) * 2 * QSP_MAX_STEPS;
    W.part = at; at += sizeof(float) * 2 * (size_t)slices * kPart;
    W.gflat = at; at += sizeof(float) * 2 * kPart;
    W.bytes = at;
    return W;
}

int check_batch_slices(int64_t batch, int slices)
{
    if (batch < 1 || batch > 0x7fffffffll) return fail(QSP_ERR_INVALID, "batch must be in [1, 2^31), got %lld", (long long)batch);
    if (slices < 0 || slices > QSP_MAX_SLICES) return fail(QSP_ERR_INVALID, "slices must be in [0, %d], got %d", QSP_MAX_SLICES, slices);
    return QSP_OK;
}

}  // namespace

extern "C" {

int qsp_version(void) { return QSP_VERSION; }

const char *qsp_last_error(void) { return g_err; }

int qsp_auto_slices(int64_t batch)
{
    if (batch < 1) return 0;
    const int64_t c = chunks_of(batch);
    return (int)(c < QSP_AUTO_SLICES ? c : QSP_AUTO_SLICES);
}

int qsp_workspace_bytes(int64_t batch, int32_t slices, size_t *bytes)
{
    if (!bytes) return fail(QSP_ERR_INVALID, "bytes must not be NULL");
    if (int rc = check_batch_slices(batch, slices)) return rc;
    *bytes = workspace_of(slices ? slices : qsp_auto_slices(batch)).bytes;
    return QSP_OK;
}

int qsp_update(const QspNet *net, const QspBatch *data, const int32_t *indices, int32_t steps, int64_t batch, int32_t slices,
               const QspHyper *hp, int64_t t0, void *workspace, uint64_t workspace_bytes, float *stats, float *const *grads,
               void *stream)
{
    if (!net || !data || !indices || !hp || !workspace || !stats)
        return fail(QSP_ERR_INVALID, "net, data, indices, hp, workspace and stats must not be NULL");
    if (net->struct_size != sizeof(QspNet))
        return fail(QSP_ERR_INVALID, "QspNet.struct_size is %u, expected %zu", net->struct_size, sizeof(QspNet));
    if (data->struct_size != sizeof(QspBatch))
        return fail(QSP_ERR_INVALID, "QspBatch.struct_size is %u, expected %zu", data->struct_size, sizeof(QspBatch));
    if (hp->struct_size != sizeof(QspHyper))
        return fail(QSP_ERR_INVALID, "QspHyper.struct_size is %u, expected %zu", hp->struct_size, sizeof(QspHyper));
    if (net->layout != QSP_NET_SHARED_TRUNK && net->layout != QSP_NET_TOWERS)
        return fail(QSP_ERR_INVALID, "QspNet.layout must be 0 (shared trunk) or 1 (towers), got %d", net->layout);
    if (steps < 1 || steps > QSP_MAX_STEPS) return fail(QSP_ERR_INVALID, "steps must be in [1, %d], got %d", QSP_MAX_STEPS, steps);
    if (int rc = check_batch_slices(batch, slices)) return rc;
    if (data->n < 1 || data->n > 0x7fffffffll) return fail(QSP_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)data->n);
    if (int rc = check_adam_t0(t0, steps, "steps")) return rc;
    if (int rc = check_adam_rates(hp->lr, hp->beta1, hp->beta2, hp->eps)) return rc;
    if (!isfinite(hp->cliprange) || hp->cliprange < 0.0) return fail(QSP_ERR_INVALID, "cliprange must be finite and >= 0, got %g", hp->cliprange);
    if (!isfinite(hp->cliprange_vf)) return fail(QSP_ERR_INVALID, "cliprange_vf must be finite, got %g", hp->cliprange_vf);
    if (!isfinite(hp->ent_coef)) return fail(QSP_ERR_INVALID, "ent_coef must be finite, got %g", hp->ent_coef);
    if (!isfinite(hp->vf_coef)) return fail(QSP_ERR_INVALID, "vf_coef must be finite, got %g", hp->vf_coef);
    if (!isfinite(hp->max_grad_norm)) return fail(QSP_ERR_INVALID, "max_grad_norm must be finite, got %g", hp->max_grad_norm);
    const bool towers = net->layout == QSP_NET_TOWERS;
    bool bad = misaligned(data->obs) || misaligned(data->actions) || misaligned(data->returns) || misaligned(data->values) ||
               misaligned(data->neglogp) || misaligned(indices) || misaligned(stats) || misaligned(workspace, 7) || !data->obs ||
               !data->actions || !data->returns || !data->values || !data->neglogp;
    for (int k = 0; k < kTensors; ++k) {
        float *const ps[4] = {net->w[k], net->m[k], net->v[k], grads ? grads[k] : nullptr};
        const bool has = towers || (k != 6 && k != 7);
        for (int j = 0; j < 4; ++j) bad = bad || misaligned(ps[j]) || (has ? (!ps[j] && (j < 3 || grads)) : ps[j] != nullptr);
    }
    if (bad) return fail(QSP_ERR_INVALID, "a tensor of the net or of the call is NULL (or not NULL where the layout has none) or not aligned");
    const int nslices = slices ? slices : qsp_auto_slices(batch);
    const Workspace W = workspace_of(nslices);
    if (workspace_bytes < W.bytes)
        return fail(QSP_ERR_INVALID, "the workspace has %llu bytes, the call needs %zu", (unsigned long long)workspace_bytes, W.bytes);
    // everything the call writes, against each other
    Range rs[4 * kTensors + 2];
    int nr = 0;
    for (int k = 0; k < kTensors; ++k) {
        float *const ps[4] = {net->w[k], net->m[k], net->v[k], grads ? grads[k] : nullptr};
        for (int j = 0; j < 4; ++j)
            if (ps[j]) rs[nr++] = Range{(uintptr_t)ps[j], (uintptr_t)ps[j] + 4 * (size_t)kElems[k]};
    }
    rs[nr++] = Range{(uintptr_t)stats, (uintptr_t)stats + 4 * (size_t)QSP_STATS * (size_t)steps};
    rs[nr++] = Range{(uintptr_t)workspace, (uintptr_t)workspace + W.bytes};
    for (int a = 0; a < nr; ++a)
        for (int b = a + 1; b < nr; ++b)
            if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) return fail(QSP_ERR_INVALID, "two tensors the call writes overlap");

    char *ws = (char *)workspace;
    double *statp = (double *)(ws + W.statp), *ssq = (double *)(ws + W.ssq);
    float *adv = (float *)(ws + W.adv), *part = (float *)(ws + W.part), *gflat = (float *)(ws + W.gflat);

    ParamTable T{};
    int total = 0;
    for (int k = 0; k < kTensors; ++k) {
        T.w[k] = net->w[k]; T.m[k] = net->m[k]; T.v[k] = net->v[k];
        T.grads[k] = grads ? grads[k] : nullptr;
        T.start[k] = total;
        total += net->w[k] ? kElems[k] : 0;
        T.loc[0][k] = kLocPolicy[k];
        T.loc[1][k] = kLocValue[k];
        T.stride[k] = k == 10 ? kOut : 1;
    }
    T.start[kTensors] = total;
    if (!towers) { T.loc[1][0] = kLW0; T.loc[1][1] = kLB0; }
    const int nblk = (total + kElemBlock - 1) / kElemBlock;

    GradArgs G{};
    for (int i = 0; i < 6; ++i) G.w[0][i] = net->w[i];
    G.w[1][0] = towers ? net->w[6] : net->w[0];
    G.w[1][1] = towers ? net->w[7] : net->w[1];
    for (int i = 2; i < 6; ++i) G.w[1][i] = net->w[6 + i];
    G.logstd = net->w[12];
    G.obs = data->obs; G.act = data->actions; G.ret = data->returns; G.val = data->values; G.nlp = data->neglogp;
    G.part = part; G.statp = statp;
    G.lo = (float)(1.0 - hp->cliprange); G.hi = (float)(1.0 + hp->cliprange); G.clip = (float)hp->cliprange;
    G.use_crv = hp->cliprange_vf >= 0.0;
    G.crv = G.use_crv ? (float)hp->cliprange_vf : 0.0f;
    G.inv_batch = (float)(1.0 / (double)batch);
    G.vf_scale = (float)(hp->vf_coef / (double)batch);
    G.neg_ent = (float)(-hp->ent_coef);
    G.batch = (int)batch; G.slices = nslices;
    G.cps = (int)((chunks_of(batch) + nslices - 1) / nslices);

    ApplyArgs A{};
    A.gflat = gflat; A.ssq = ssq; A.statp = statp;
    A.max_grad_norm = hp->max_grad_norm; A.batch = (double)batch;
    A.b1f = (float)hp->beta1; A.b2f = (float)hp->beta2; A.omb1 = (float)(1.0 - hp->beta1); A.omb2 = (float)(1.0 - hp->beta2);
    A.eps = (float)hp->eps;
    A.total = total; A.nblk = nblk; A.slices = nslices;

    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_ppo_adv_stats, dim3((unsigned)steps), dim3(kAdvBlock), 0, st, data->returns, data->values, indices, (int)batch, adv);
    HIP_TRY(hipGetLastError());
    for (int s = 0; s < steps; ++s) {
        G.indices = indices + (int64_t)s * batch;
        G.adv = adv + 2 * s;
        hipLaunchKernelGGL(k_ppo_grad, dim3((unsigned)nslices, 2), dim3(kFitBlock), 0, st, G);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_ppo_reduce, dim3((unsigned)nblk), dim3(kElemBlock), 0, st, T, (const float *)part, nslices, total, gflat, ssq);
        HIP_TRY(hipGetLastError());
        const double tt = (double)(t0 + s) + 1.0;
        A.lr_t = (float)(hp->lr * sqrt(1.0 - pow(hp->beta2, tt)) / (1.0 - pow(hp->beta1, tt)));
        A.stats = stats + (size_t)QSP_STATS * s;
        A.want_grads = grads && s == steps - 1;
        hipLaunchKernelGGL(k_ppo_apply, dim3((unsigned)nblk), dim3(kElemBlock), 0, st, T, A);
        HIP_TRY(hipGetLastError());
    }
    return QSP_OK;
}

}  // extern "C"
