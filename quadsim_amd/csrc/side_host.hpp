// side_host.hpp -- the host plumbing the four side libraries share at the source level (dynplan.hip, dynmppi.hip, dynfit.hip,
// bcfit.hip): the error text, the HIP status check, the pointer and Adam-argument checks of the two fits and the width rule.
// Host code only, in an anonymous namespace: every library compiles a copy of its own, so each keeps its own thread-local
// error text behind its own q??_last_error.  The main library has host_util.hpp (negative codes, much more state).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <unordered_map>

namespace {

// the status codes of the four public headers, which each .hip file static_asserts against its own enum
constexpr int kOk = 0, kErrInvalid = 1, kErrHip = 2, kErrUnsupported = 3;

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) return fail(kErrHip, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

bool misaligned(const void *p, uintptr_t mask = 3) { return ((uintptr_t)p & mask) != 0; }

// the compute units of the current device, asked once per device
int cu_count(int *out)
{
    static std::mutex m;
    static std::unordered_map<int, int> cus;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(m);
    auto it = cus.find(dev);
    if (it == cus.end()) {
        int v = 0;
        HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        it = cus.emplace(dev, v > 0 ? v : 1).first;
    }
    *out = it->second;
    return kOk;
}

// the compiled (padded) hidden-width pairs, cheapest first: a net runs on the first pair that covers it -> its index
constexpr int kWidths[3][2] = {{64, 64}, {128, 128}, {208, 112}};

int width_pair(int h1, int h2, int *pair)
{
    if (h1 < 1 || h2 < 1) return fail(kErrInvalid, "hidden widths must be >= 1, got (%d, %d)", h1, h2);
    for (int i = 0; i < 3; ++i)
        if (h1 <= kWidths[i][0] && h2 <= kWidths[i][1]) {
            *pair = i;
            return kOk;
        }
    return fail(kErrUnsupported, "hidden widths (%d, %d) are outside the supported range: h1, h2 <= 128, or h1 <= 208 and h2 <= 112", h1,
                h2);
}

// Adam's step count: `what` is the library's word for the steps of one call ("iters", "steps")
int check_adam_t0(int64_t t0, int steps, const char *what)
{
    if (t0 < 0 || t0 + steps > 0x7fffffffll) return fail(kErrInvalid, "t0 must be >= 0 with t0 + %s below 2^31, got %lld", what, (long long)t0);
    return kOk;
}

int check_adam_rates(double lr, double beta1, double beta2, double eps)
{
    if (!isfinite(lr)) return fail(kErrInvalid, "lr must be finite, got %g", lr);
    if (!isfinite(eps)) return fail(kErrInvalid, "eps must be finite, got %g", eps);
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return fail(kErrInvalid, "beta1 must be in [0, 1), got %g", beta1);
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return fail(kErrInvalid, "beta2 must be in [0, 1), got %g", beta2);
    return kOk;
}

// true if one of the six weights, moments or (where asked for) gradients is NULL or not 4-byte aligned
bool bad_six(float *const *w, float *const *m, float *const *v, float *const *grads)
{
    bool bad = false;
    for (int i = 0; i < 6; ++i)
        bad = bad || !w[i] || !m[i] || !v[i] || misaligned(w[i]) || misaligned(m[i]) || misaligned(v[i]) ||
              (grads && (!grads[i] || misaligned(grads[i])));
    return bad;
}

// what the args structs of both fit kernels begin with and share: the four arrays and Adam's constants
template <class Args>
void fill_fit_args(Args &F, float *const *w, float *const *m, float *const *v, float *const *grads, double lr, double beta1, double beta2,
                   double eps, int batch, int64_t t0)
{
    for (int i = 0; i < 6; ++i) {
        F.w[i] = w[i]; F.m[i] = m[i]; F.v[i] = v[i];
        F.grads[i] = grads ? grads[i] : nullptr;
    }
    F.lr = lr; F.beta1 = beta1; F.beta2 = beta2;
    F.b1f = (float)beta1; F.b2f = (float)beta2; F.omb1 = (float)(1.0 - beta1); F.omb2 = (float)(1.0 - beta2); F.eps = (float)eps;
    F.batch = batch; F.t0 = (int)t0;
}

}  // namespace
