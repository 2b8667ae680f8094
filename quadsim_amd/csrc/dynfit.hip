// dynfit.hip -- libquadsim_dynfit.so: the C ABI of include/quadsim_dyn_fit.h over the kernel of dynfit_kernels.hpp.  ONE
// translation unit of its own: nothing here is part of the other three libraries.  Shared with them at the source level only:
// quadsim_device.hpp (the Philox generator of the batch draws).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/quadsim_dyn_fit.h"
#include "dynfit_kernels.hpp"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define QSDF_HIP_TRY(expr)                                                                             \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(QSDF_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

bool misaligned(const void *p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace

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
    if (h1 < 1 || h2 < 1) return fail(QSDF_ERR_INVALID, "hidden widths must be >= 1, got (%d, %d)", h1, h2);
    const int pair = h1 <= 64 && h2 <= 64 ? 0 : h1 <= 128 && h2 <= 128 ? 1 : h1 <= 208 && h2 <= 112 ? 2 : -1;
    if (pair < 0)
        return fail(QSDF_ERR_UNSUPPORTED, "hidden widths (%d, %d) are outside the supported range: h1, h2 <= 128, or h1 <= 208 and h2 <= 112",
                    h1, h2);
    if (batch < 1 || batch > QSDF_MAX_BATCH) return fail(QSDF_ERR_INVALID, "batch must be in [1, %d], got %d", QSDF_MAX_BATCH, batch);
    if (iters < 1 || iters > QSDF_MAX_ITERS) return fail(QSDF_ERR_INVALID, "iters must be in [1, %d], got %d", QSDF_MAX_ITERS, iters);
    if (capacity < 1 || capacity > 0x7fffffffll) return fail(QSDF_ERR_INVALID, "capacity must be in [1, 2^31), got %lld", (long long)capacity);
    if (size < 1 || size > capacity)
        return fail(QSDF_ERR_INVALID, "size must be in [1, capacity = %lld], got %lld", (long long)capacity, (long long)size);
    if (t0 < 0 || t0 + iters > 0x7fffffffll) return fail(QSDF_ERR_INVALID, "t0 must be >= 0 with t0 + iters below 2^31, got %lld", (long long)t0);
    if (k >> 48) return fail(QSDF_ERR_INVALID, "k must be below 2^48, got %llu", (unsigned long long)k);
    if (!isfinite(lr)) return fail(QSDF_ERR_INVALID, "lr must be finite, got %g", lr);
    if (!isfinite(eps)) return fail(QSDF_ERR_INVALID, "eps must be finite, got %g", eps);
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(QSDF_ERR_INVALID, "beta1 must be in [0, 1), got %g", beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(QSDF_ERR_INVALID, "beta2 must be in [0, 1), got %g", beta2);
    bool bad = misaligned(buf_x) || misaligned(buf_d) || misaligned(indices) || misaligned(loss) || misaligned(indices_out) ||
               !net->in_mean || !net->in_rscale || !net->out_mean || !net->out_rscale;
    for (int i = 0; i < 6; ++i)
        bad = bad || !net->w[i] || !net->m[i] || !net->v[i] || misaligned(net->w[i]) || misaligned(net->m[i]) || misaligned(net->v[i]) ||
              (grads && (!grads[i] || misaligned(grads[i])));
    if (bad) return fail(QSDF_ERR_INVALID, "a tensor of the net or of the call is NULL or not 4-byte aligned");

    qsf::FitArgs F{};
    for (int i = 0; i < 6; ++i) {
        F.w[i] = net->w[i]; F.m[i] = net->m[i]; F.v[i] = net->v[i];
        F.grads[i] = grads ? grads[i] : nullptr;
    }
    F.in_mean = net->in_mean; F.in_rscale = net->in_rscale; F.out_mean = net->out_mean; F.out_rscale = net->out_rscale;
    F.buf_x = buf_x; F.buf_d = buf_d; F.indices = indices; F.loss = loss; F.indices_out = indices_out;
    F.seed = seed; F.k = k; F.lr = lr; F.beta1 = beta1; F.beta2 = beta2;
    F.b1f = (float)beta1; F.b2f = (float)beta2; F.omb1 = (float)(1.0 - beta1); F.omb2 = (float)(1.0 - beta2); F.eps = (float)eps;
    F.dscale = (float)(2.0 / (12.0 * batch)); F.count = (float)(12 * batch);
    F.h1 = h1; F.h2 = h2; F.size = (int)size; F.iters = iters; F.batch = batch; F.t0 = (int)t0;
    const dim3 grid(1), block(qsf::kFitBlock);               // one workgroup: the whole fit is one CU's worth of work
    if (pair == 0) hipLaunchKernelGGL((qsf::k_dyn_fit<64, 64>), grid, block, 0, (hipStream_t)stream, F);
    else if (pair == 1) hipLaunchKernelGGL((qsf::k_dyn_fit<128, 128>), grid, block, 0, (hipStream_t)stream, F);
    else hipLaunchKernelGGL((qsf::k_dyn_fit<208, 112>), grid, block, 0, (hipStream_t)stream, F);
    QSDF_HIP_TRY(hipGetLastError());
    return QSDF_OK;
}

}  // extern "C"
