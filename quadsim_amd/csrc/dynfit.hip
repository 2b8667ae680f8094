// dynfit.hip -- libquadsim_dynfit.so: the C ABI of include/quadsim_dyn_fit.h over the kernel of dynfit_kernels.hpp.  ONE
// translation unit of its own: nothing here is part of the other libraries.  Shared with them at the source level only:
// train_pieces.hpp (the chunk primitives), quadsim_device.hpp (the Philox generator of the batch draws) and side_host.hpp (error text, the width rule, the Adam and
// pointer checks and the fill of the args the two fits have in common).
#include "../../include/quadsim_dyn_fit.h"
#include "side_host.hpp"
#include "dynfit_kernels.hpp"

static_assert(QSDF_OK == kOk && QSDF_ERR_INVALID == kErrInvalid && QSDF_ERR_HIP == kErrHip && QSDF_ERR_UNSUPPORTED == kErrUnsupported,
              "side_host.hpp returns the codes of quadsim_dyn_fit.h");

extern "C" {

int qsdf_version(void) { return QSDF_VERSION; }

const char *qsdf_last_error(void) { return g_err; }

int qsdf_fit(const QsdfNet *net, const float *buf_x, const float *buf_d, int64_t capacity, int64_t size, int32_t iters, int32_t batch,
             double lr, double beta1, double beta2, double eps, int64_t t0, uint64_t seed, uint64_t k, const int32_t *indices,
             float *loss, int32_t *indices_out, float *const *grads, void *stream)
{
    if (!net || !buf_x || !buf_d || !loss) return fail(QSDF_ERR_INVALID, "net, buf_x, buf_d and loss must not be NULL");
    if (net->struct_size != sizeof(QsdfNet))
        return fail(QSDF_ERR_INVALID, "QsdfNet.struct_size is %u, expected %zu", net->struct_size, sizeof(QsdfNet));
    const int h1 = net->h1, h2 = net->h2;
    int pair = 0;
    if (int rc = width_pair(h1, h2, &pair)) return rc;
    if (batch < 1 || batch > QSDF_MAX_BATCH) return fail(QSDF_ERR_INVALID, "batch must be in [1, %d], got %d", QSDF_MAX_BATCH, batch);
    if (iters < 1 || iters > QSDF_MAX_ITERS) return fail(QSDF_ERR_INVALID, "iters must be in [1, %d], got %d", QSDF_MAX_ITERS, iters);
    if (capacity < 1 || capacity > 0x7fffffffll) return fail(QSDF_ERR_INVALID, "capacity must be in [1, 2^31), got %lld", (long long)capacity);
    if (size < 1 || size > capacity)
        return fail(QSDF_ERR_INVALID, "size must be in [1, capacity = %lld], got %lld", (long long)capacity, (long long)size);
    if (int rc = check_adam_t0(t0, iters, "iters")) return rc;
    if (k >> 48) return fail(QSDF_ERR_INVALID, "k must be below 2^48, got %llu", (unsigned long long)k);
    if (int rc = check_adam_rates(lr, beta1, beta2, eps)) return rc;
    if (misaligned(buf_x) || misaligned(buf_d) || misaligned(indices) || misaligned(loss) || misaligned(indices_out) || !net->in_mean ||
        !net->in_rscale || !net->out_mean || !net->out_rscale || bad_six(net->w, net->m, net->v, grads))
        return fail(QSDF_ERR_INVALID, "a tensor of the net or of the call is NULL or not 4-byte aligned");

    qsf::FitArgs F{};
    fill_fit_args(F, net->w, net->m, net->v, grads, lr, beta1, beta2, eps, batch, t0);
    F.in_mean = net->in_mean; F.in_rscale = net->in_rscale; F.out_mean = net->out_mean; F.out_rscale = net->out_rscale;
    F.buf_x = buf_x; F.buf_d = buf_d; F.indices = indices; F.loss = loss; F.indices_out = indices_out;
    F.seed = seed; F.k = k;
    F.dscale = (float)(2.0 / (12.0 * batch)); F.count = (float)(12 * batch);
    F.h1 = h1; F.h2 = h2; F.size = (int)size; F.iters = iters;
    const dim3 grid(1), block(qsf::kFitBlock);               // one workgroup: the whole fit is one CU's worth of work
    if (pair == 0) hipLaunchKernelGGL((qsf::k_dyn_fit<64, 64>), grid, block, 0, (hipStream_t)stream, F);
    else if (pair == 1) hipLaunchKernelGGL((qsf::k_dyn_fit<128, 128>), grid, block, 0, (hipStream_t)stream, F);
    else hipLaunchKernelGGL((qsf::k_dyn_fit<208, 112>), grid, block, 0, (hipStream_t)stream, F);
    HIP_TRY(hipGetLastError());
    return QSDF_OK;
}

}  // extern "C"
