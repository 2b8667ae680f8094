// trpo.hip -- libquadsim_trpo.so: the C ABI of include/quadsim_trpo.h over the kernels of trpo_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other eight libraries.  Shared at the source level only: train_pieces.hpp (the forward
// chain, the backward pass and the Adam step), and side_host.hpp (error text, the Adam and pointer checks).
#include "../../include/quadsim_trpo.h"
#include "side_host.hpp"
#include "trpo_kernels.hpp"

static_assert(QST_OK == kOk && QST_ERR_INVALID == kErrInvalid && QST_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_trpo.h");
static_assert(QST_PARAMS == qst::kP && QST_CHUNK == qsf::kRows && QST_CG_SCALARS == 4, "quadsim_trpo.h states the kernels' geometry");

namespace {

using namespace qst;

const int kPolicySlot[kPolicySlots] = {0, 1, 2, 3, 4, 5, 12};
const int kPolicyElems[kPolicySlots] = {kIn * kH, kH, kH * kH, kH, kH * kOut, kOut, kOut};
const int kValueElems[6] = {kIn * kH, kH, kH * kH, kH, kH, 1};

struct Range {
    uintptr_t lo, hi;
};

bool overlap(const Range *rs, int nr)
{
    for (int a = 0; a < nr; ++a)
        for (int b = a + 1; b < nr; ++b)
            if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) return true;
    return false;
}

Range range_of(const void *p, size_t bytes) { return Range{(uintptr_t)p, (uintptr_t)p + bytes}; }

// the workspace: doubles first
struct Offsets {
    size_t sc, statp, flag, adv, vec, mu_old, nlp_old, part, bytes;
};

int64_t chunks_of(int64_t rows) { return (rows + QST_CHUNK - 1) / QST_CHUNK; }

Offsets workspace_of(int64_t n, int slices)
{
    Offsets W{};
    size_t at = 0;
    W.sc = at; at += sizeof(double) * 4;
    W.statp = at; at += sizeof(double) * 2 * (size_t)slices;
    W.flag = at; at += sizeof(int32_t) * 4;
    W.adv = at; at += sizeof(float) * 4;
    W.vec = at; at += sizeof(float) * 7 * (size_t)kP;
    W.mu_old = at; at += sizeof(float) * 4 * (size_t)n;
    W.nlp_old = at; at += sizeof(float) * (size_t)n;
    W.part = at; at += sizeof(float) * (size_t)slices * kP;
    W.bytes = at;
    return W;
}

int check_n_slices(int64_t n, int slices)
{
    if (n < 1 || n > 0x7fffffffll) return fail(QST_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)n);
    if (slices < 0 || slices > QST_MAX_SLICES) return fail(QST_ERR_INVALID, "slices must be in [0, %d], got %d", QST_MAX_SLICES, slices);
    return QST_OK;
}

int check_net(const QstNet *net)
{
    if (net->struct_size != sizeof(QstNet))
        return fail(QST_ERR_INVALID, "QstNet.struct_size is %u, expected %zu", net->struct_size, sizeof(QstNet));
    if (net->layout == QST_NET_SHARED_TRUNK)
        return fail(QST_ERR_INVALID, "the shared-trunk layout is not covered: its shared layers would belong to the policy step and to the "
                                     "value fit; TRPO runs on the towers layout (QstNet.layout = 1)");
    if (net->layout != QST_NET_TOWERS) return fail(QST_ERR_INVALID, "QstNet.layout must be 1 (towers), got %d", net->layout);
    return QST_OK;
}

}  // namespace

extern "C" {

int qst_version(void) { return QST_VERSION; }

const char *qst_last_error(void) { return g_err; }

int qst_auto_slices(int64_t n)
{
    if (n < 1) return 0;
    const int64_t c = chunks_of(n);
    return (int)(c < QST_AUTO_SLICES ? c : QST_AUTO_SLICES);
}

int qst_workspace_bytes(int64_t n, int32_t slices, size_t *bytes)
{
    if (!bytes) return fail(QST_ERR_INVALID, "bytes must not be NULL");
    if (int rc = check_n_slices(n, slices)) return rc;
    *bytes = workspace_of(n, slices ? slices : qst_auto_slices(n)).bytes;
    return QST_OK;
}

int qst_policy_step(const QstNet *net, const QstBatch *data, int32_t slices, const QstHyper *hp, void *workspace,
                    uint64_t workspace_bytes, float *stats, float *grad, const QstTrace *trace, void *stream)
{
    if (!net || !data || !hp || !workspace || !stats) return fail(QST_ERR_INVALID, "net, data, hp, workspace and stats must not be NULL");
    if (int rc = check_net(net)) return rc;
    if (data->struct_size != sizeof(QstBatch))
        return fail(QST_ERR_INVALID, "QstBatch.struct_size is %u, expected %zu", data->struct_size, sizeof(QstBatch));
    if (hp->struct_size != sizeof(QstHyper))
        return fail(QST_ERR_INVALID, "QstHyper.struct_size is %u, expected %zu", hp->struct_size, sizeof(QstHyper));
    if (trace && trace->struct_size != sizeof(QstTrace))
        return fail(QST_ERR_INVALID, "QstTrace.struct_size is %u, expected %zu", trace->struct_size, sizeof(QstTrace));
    const int64_t n = data->n;
    if (int rc = check_n_slices(n, slices)) return rc;
    if (hp->cg_iters < 1 || hp->cg_iters > QST_MAX_CG_ITERS)
        return fail(QST_ERR_INVALID, "cg_iters must be in [1, %d], got %d", QST_MAX_CG_ITERS, hp->cg_iters);
    if (hp->backtracks < 1 || hp->backtracks > QST_MAX_BACKTRACKS)
        return fail(QST_ERR_INVALID, "backtracks must be in [1, %d], got %d", QST_MAX_BACKTRACKS, hp->backtracks);
    if (hp->fvp_stride < 1) return fail(QST_ERR_INVALID, "fvp_stride must be >= 1, got %d", hp->fvp_stride);
    if (!isfinite(hp->max_kl) || hp->max_kl <= 0.0) return fail(QST_ERR_INVALID, "max_kl must be finite and > 0, got %g", hp->max_kl);
    if (!isfinite(hp->cg_damping) || hp->cg_damping < 0.0) return fail(QST_ERR_INVALID, "cg_damping must be finite and >= 0, got %g", hp->cg_damping);
    if (!isfinite(hp->entcoeff)) return fail(QST_ERR_INVALID, "entcoeff must be finite, got %g", hp->entcoeff);
    if (!isfinite(hp->residual_tol) || hp->residual_tol < 0.0)
        return fail(QST_ERR_INVALID, "residual_tol must be finite and >= 0, got %g", hp->residual_tol);
    bool bad = !data->obs || !data->actions || !data->returns || !data->values || misaligned(data->obs) || misaligned(data->actions) ||
               misaligned(data->returns) || misaligned(data->values) || misaligned(stats) || misaligned(grad) || misaligned(workspace, 7);
    for (int q = 0; q < kPolicySlots; ++q) bad = bad || !net->w[kPolicySlot[q]] || misaligned(net->w[kPolicySlot[q]]);
    if (trace)
        bad = bad || !trace->fvp_in || !trace->fvp_out || !trace->cg || !trace->x || !trace->fullstep || !trace->ls || misaligned(trace->fvp_in) ||
              misaligned(trace->fvp_out) || misaligned(trace->cg, 7) || misaligned(trace->x) || misaligned(trace->fullstep) || misaligned(trace->ls);
    if (bad) return fail(QST_ERR_INVALID, "a tensor of the net, of the call or of the trace is NULL or not aligned");
    const int nslices = slices ? slices : qst_auto_slices(n);
    const Offsets O = workspace_of(n, nslices);
    if (workspace_bytes < O.bytes)
        return fail(QST_ERR_INVALID, "the workspace has %llu bytes, the call needs %zu", (unsigned long long)workspace_bytes, O.bytes);
    // everything the call writes, against each other
    Range rs[kPolicySlots + 9];
    int nr = 0;
    for (int q = 0; q < kPolicySlots; ++q) rs[nr++] = range_of(net->w[kPolicySlot[q]], 4 * (size_t)kPolicyElems[q]);
    rs[nr++] = range_of(stats, 4 * (size_t)QST_STATS);
    rs[nr++] = range_of(workspace, O.bytes);
    if (grad) rs[nr++] = range_of(grad, 4 * (size_t)kP);
    if (trace) {
        const size_t rows = (size_t)hp->cg_iters + 1;
        rs[nr++] = range_of(trace->fvp_in, 4 * rows * kP);
        rs[nr++] = range_of(trace->fvp_out, 4 * rows * kP);
        rs[nr++] = range_of(trace->cg, 8 * (size_t)QST_CG_SCALARS * (size_t)hp->cg_iters);
        rs[nr++] = range_of(trace->x, 4 * (size_t)kP);
        rs[nr++] = range_of(trace->fullstep, 4 * (size_t)kP);
        rs[nr++] = range_of(trace->ls, 4 * 2 * (size_t)hp->backtracks);
    }
    if (overlap(rs, nr)) return fail(QST_ERR_INVALID, "two tensors the call writes overlap");

    char *ws = (char *)workspace;
    Ws W{};
    W.sc = (double *)(ws + O.sc); W.statp = (double *)(ws + O.statp); W.flag = (int32_t *)(ws + O.flag); W.adv = (float *)(ws + O.adv);
    float *vec = (float *)(ws + O.vec);
    W.theta = vec; W.g = vec + kP; W.p = vec + 2 * kP; W.r = vec + 3 * kP; W.x = vec + 4 * kP; W.z = vec + 5 * kP; W.fs = vec + 6 * kP;
    W.mu_old = (float *)(ws + O.mu_old); W.nlp_old = (float *)(ws + O.nlp_old); W.part = (float *)(ws + O.part);
    Policy Pol{};
    for (int q = 0; q < kPolicySlots; ++q) Pol.w[q] = net->w[kPolicySlot[q]];
    Rows R{data->obs, data->actions, data->returns, data->values, (int)n, nslices, (int)((chunks_of(n) + nslices - 1) / nslices)};
    const int64_t nf = (n + hp->fvp_stride - 1) / hp->fvp_stride;
    Rows Rf = R;
    Rf.cps = (int)((chunks_of(nf) + nslices - 1) / nslices);
    const float inv_n = (float)(1.0 / (double)n), inv_nf = (float)(1.0 / (double)nf);
    const dim3 one(1), grid((unsigned)nslices), elems((unsigned)kBlocks);

    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_trpo_prep, one, dim3(kVecBlock), 0, st, Pol, R, W);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_trpo_grad, grid, dim3(kFitBlock), 0, st, R, W, inv_n, (float)hp->entcoeff);
    HIP_TRY(hipGetLastError());
    ReduceArgs Q{};
    Q.part = W.part; Q.out = W.g; Q.flag = W.flag; Q.slices = nslices;
    hipLaunchKernelGGL(k_trpo_reduce, elems, dim3(kVecBlock), 0, st, Q);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_trpo_cg_init, one, dim3(kVecBlock), 0, st, W, nslices, (double)n, hp->entcoeff, stats, grad);
    HIP_TRY(hipGetLastError());
    Q.out = W.z; Q.damping = (float)hp->cg_damping;
    for (int k = 0; k <= hp->cg_iters; ++k) {
        const bool solve = k < hp->cg_iters;                 // the last product is (F + damping) x of the step
        const float *v = solve ? W.p : W.x;
        hipLaunchKernelGGL(k_trpo_fvp, grid, dim3(kFitBlock), 0, st, Rf, W, v, (int)hp->fvp_stride, inv_nf, (int)solve);
        HIP_TRY(hipGetLastError());
        Q.v = v; Q.until_converged = solve;
        Q.tr_in = trace ? trace->fvp_in + (size_t)k * kP : nullptr;
        Q.tr_out = trace ? trace->fvp_out + (size_t)k * kP : nullptr;
        hipLaunchKernelGGL(k_trpo_reduce, elems, dim3(kVecBlock), 0, st, Q);
        HIP_TRY(hipGetLastError());
        if (solve) {
            hipLaunchKernelGGL(k_trpo_cg_iter, one, dim3(kVecBlock), 0, st, W, k, hp->residual_tol, trace ? trace->cg : nullptr);
            HIP_TRY(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_trpo_step, one, dim3(kVecBlock), 0, st, W, hp->max_kl, stats, trace ? trace->x : nullptr,
                       trace ? trace->fullstep : nullptr);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < hp->backtracks; ++k) {
        const float scale = ldexpf(1.0f, -k);
        hipLaunchKernelGGL(k_trpo_ls_eval, grid, dim3(kFitBlock), 0, st, R, W, scale);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_trpo_ls_decide, one, dim3(kVecBlock), 0, st, Pol, W, k, (int)(k == hp->backtracks - 1), scale, nslices, (double)n,
                           hp->entcoeff, hp->max_kl, stats, trace ? trace->ls : nullptr);
        HIP_TRY(hipGetLastError());
    }
    return QST_OK;
}

int qst_vf_fit(const QstNet *net, const float *obs, const float *returns, int64_t n, const int32_t *indices, int32_t steps,
               int32_t batch, double lr, double beta1, double beta2, double eps, int64_t t0, float *stats, float *const *grads,
               void *stream)
{
    if (!net || !obs || !returns || !indices || !stats) return fail(QST_ERR_INVALID, "net, obs, returns, indices and stats must not be NULL");
    if (int rc = check_net(net)) return rc;
    if (n < 1 || n > 0x7fffffffll) return fail(QST_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)n);
    if (batch < 1 || batch > QST_MAX_BATCH) return fail(QST_ERR_INVALID, "batch must be in [1, %d], got %d", QST_MAX_BATCH, batch);
    if (steps < 1 || steps > QST_MAX_STEPS) return fail(QST_ERR_INVALID, "steps must be in [1, %d], got %d", QST_MAX_STEPS, steps);
    if (int rc = check_adam_t0(t0, steps, "steps")) return rc;
    if (int rc = check_adam_rates(lr, beta1, beta2, eps)) return rc;
    if (bad_six(net->w + 6, net->m + 6, net->v + 6, grads) || misaligned(obs) || misaligned(returns) || misaligned(indices) || misaligned(stats))
        return fail(QST_ERR_INVALID, "a tensor of the value tower or of the call is NULL or not aligned");
    Range rs[4 * 6 + 1];
    int nr = 0;
    for (int i = 0; i < 6; ++i) {
        float *const ps[4] = {net->w[6 + i], net->m[6 + i], net->v[6 + i], grads ? grads[i] : nullptr};
        for (int j = 0; j < 4; ++j)
            if (ps[j]) rs[nr++] = range_of(ps[j], 4 * (size_t)kValueElems[i]);
    }
    rs[nr++] = range_of(stats, 4 * (size_t)steps);
    if (overlap(rs, nr)) return fail(QST_ERR_INVALID, "two tensors the call writes overlap");

    VfArgs F{};
    fill_fit_args(F, net->w + 6, net->m + 6, net->v + 6, grads, lr, beta1, beta2, eps, batch, t0);
    F.obs = obs; F.ret = returns; F.indices = indices; F.loss = stats; F.steps = steps;
    hipLaunchKernelGGL(k_trpo_vf_fit, dim3(1), dim3(kFitBlock), 0, (hipStream_t)stream, F);
    HIP_TRY(hipGetLastError());
    return QST_OK;
}

}  // extern "C"
