// bcfit.hip -- libquadsim_bc.so: the C ABI of include/quadsim_bc.h over the kernels of bcfit_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other four libraries.  Shared at the source level only: train_pieces.hpp with the
// other trainers (the forward chain, the backward pass and the Adam step) and side_host.hpp with all the side
// libraries (error text, the Adam and pointer checks and the fill of the args the two fits have in common).
#include "../../include/quadsim_bc.h"
#include "side_host.hpp"
#include "bcfit_kernels.hpp"

static_assert(QSBC_OK == kOk && QSBC_ERR_INVALID == kErrInvalid && QSBC_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_bc.h");

namespace {

const size_t kElems[6] = {qsb::kIn * qsb::kH, qsb::kH, qsb::kH * qsb::kH, qsb::kH, qsb::kH * qsb::kOut, qsb::kOut};

struct Range {
    uintptr_t lo, hi;
};

}  // namespace

extern "C" {

int qsbc_version(void) { return QSBC_VERSION; }

const char *qsbc_last_error(void) { return g_err; }

int qsbc_fit(const QsbcNet *net, const float *obs, const float *act, int64_t n, const int32_t *indices, const int32_t *counts,
             int32_t steps, int32_t batch, double lr, double beta1, double beta2, double eps, int64_t t0, float *loss,
             float *const *grads, void *stream)
{
    if (!net || !obs || !act || !indices || !loss) return fail(QSBC_ERR_INVALID, "net, obs, act, indices and loss must not be NULL");
    if (net->struct_size != sizeof(QsbcNet))
        return fail(QSBC_ERR_INVALID, "QsbcNet.struct_size is %u, expected %zu", net->struct_size, sizeof(QsbcNet));
    if (batch < 1 || batch > QSBC_MAX_BATCH) return fail(QSBC_ERR_INVALID, "batch must be in [1, %d], got %d", QSBC_MAX_BATCH, batch);
    if (steps < 1 || steps > QSBC_MAX_STEPS) return fail(QSBC_ERR_INVALID, "steps must be in [1, %d], got %d", QSBC_MAX_STEPS, steps);
    if (n < 1 || n > 0x7fffffffll) return fail(QSBC_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)n);
    if (int rc = check_adam_t0(t0, steps, "steps")) return rc;
    if (int rc = check_adam_rates(lr, beta1, beta2, eps)) return rc;
    if (misaligned(obs) || misaligned(act) || misaligned(indices) || misaligned(counts) || misaligned(loss) ||
        bad_six(net->w, net->m, net->v, grads))
        return fail(QSBC_ERR_INVALID, "a tensor of the net or of the call is NULL or not 4-byte aligned");
    // everything the kernel writes, against each other
    Range rs[25];
    int nr = 0;
    for (int i = 0; i < 6; ++i) {
        float *const ps[4] = {net->w[i], net->m[i], net->v[i], grads ? grads[i] : nullptr};
        for (int j = 0; j < 4; ++j)
            if (ps[j]) rs[nr++] = Range{(uintptr_t)ps[j], (uintptr_t)ps[j] + 4 * kElems[i]};
    }
    rs[nr++] = Range{(uintptr_t)loss, (uintptr_t)loss + 4 * (size_t)steps};
    for (int a = 0; a < nr; ++a)
        for (int b = a + 1; b < nr; ++b)
            if (rs[a].lo < rs[b].hi && rs[b].lo < rs[a].hi) return fail(QSBC_ERR_INVALID, "two tensors the call writes overlap");

    qsb::FitArgs F{};
    fill_fit_args(F, net->w, net->m, net->v, grads, lr, beta1, beta2, eps, batch, t0);
    F.obs = obs; F.act = act; F.indices = indices; F.counts = counts; F.loss = loss;
    F.steps = steps;
    hipLaunchKernelGGL(qsb::k_bc_fit, dim3(1), dim3(qsb::kFitBlock), 0, (hipStream_t)stream, F);   // one workgroup: one CU's worth of work
    HIP_TRY(hipGetLastError());
    return QSBC_OK;
}

int64_t qsbc_loss_blocks(int64_t count) { return count < 1 ? 0 : (count + QSBC_LOSS_BLOCK - 1) / QSBC_LOSS_BLOCK; }

int qsbc_loss(const float *const *w, const float *obs, const float *act, int64_t n, const int32_t *rows, int64_t count,
              double *partials, double *out, int32_t grid, void *stream)
{
    if (!w || !obs || !act || !partials || !out) return fail(QSBC_ERR_INVALID, "w, obs, act, partials and out must not be NULL");
    if (n < 1 || n > 0x7fffffffll) return fail(QSBC_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)n);
    if (count < 1 || count > 0x7fffffffll) return fail(QSBC_ERR_INVALID, "count must be in [1, 2^31), got %lld", (long long)count);
    if (!rows && count > n) return fail(QSBC_ERR_INVALID, "count must be at most n = %lld without a row list, got %lld", (long long)n, (long long)count);
    if (grid < 0 || grid > 65535) return fail(QSBC_ERR_INVALID, "grid must be in [0, 65535], got %d", grid);
    bool bad = misaligned(obs) || misaligned(act) || misaligned(rows) || misaligned(partials, 7) || misaligned(out, 7);
    for (int i = 0; i < 6; ++i) bad = bad || !w[i] || misaligned(w[i]);
    if (bad) return fail(QSBC_ERR_INVALID, "a tensor of the call is NULL or misaligned");
    const int64_t blocks = qsbc_loss_blocks(count);
    if ((uintptr_t)out < (uintptr_t)(partials + blocks) && (uintptr_t)partials < (uintptr_t)(out + 1))
        return fail(QSBC_ERR_INVALID, "partials and out overlap");

    qsb::LossArgs L{};
    for (int i = 0; i < 6; ++i) L.w[i] = w[i];
    L.obs = obs; L.act = act; L.rows = rows; L.partials = partials; L.count = (int)count; L.blocks = (int)blocks;
    const int64_t g = grid ? grid : (blocks < 1024 ? blocks : 1024);
    hipLaunchKernelGGL(qsb::k_bc_loss, dim3((unsigned)(g < blocks ? g : blocks)), dim3(qsb::kFitBlock), 0, (hipStream_t)stream, L);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(qsb::k_bc_loss_sum, dim3(1), dim3(qsb::kSumBlock), 0, (hipStream_t)stream, (const double *)partials, (int)blocks,
                       (int)count, out);
    HIP_TRY(hipGetLastError());
    return QSBC_OK;
}

}  // extern "C"
