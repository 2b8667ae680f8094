// dynmppi.hip -- libquadsim_dynmppi.so: the C ABI of include/quadsim_dyn_mppi.h over the kernels of dynmppi_kernels.hpp.  ONE
// translation unit of its own: nothing here is part of libquadsim_hip.so or libquadsim_dyn.so.  Shared with them at the source
// level only: quadsim_device.hpp (Philox keying, normals) and dynplan_kernels.hpp / dynplan_image.hpp (the model step and the
// layout of the image that qsd_net_pack writes).  No host table of images: the caller names the widths, the kernels check the
// image header.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <mutex>
#include <unordered_map>

#include "../../include/quadsim_dyn_mppi.h"
#include "dynmppi_kernels.hpp"

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

#define QSDM_HIP_TRY(expr)                                                                             \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(QSDM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// the compiled instantiations, cheapest first: a net runs on the first pair of tile counts that covers it (the rule of
// quadsim_dyn.h, by which qsd_net_pack chose the image's layout)
struct Tiles { int t1, t2; };
constexpr Tiles kTiles[] = {{4, 4}, {8, 8}, {13, 7}};

int choose_tiles(int h1, int h2, Tiles *out)
{
    if (h1 < 1 || h2 < 1) return fail(QSDM_ERR_INVALID, "hidden widths must be >= 1, got (%d, %d)", h1, h2);
    for (const Tiles &t : kTiles)
        if (h1 <= 16 * t.t1 && h2 <= 16 * t.t2) {
            *out = t;
            return QSDM_OK;
        }
    return fail(QSDM_ERR_UNSUPPORTED, "hidden widths (%d, %d) are outside the supported range: h1, h2 <= 128, or h1 <= 208 and h2 <= 112", h1,
                h2);
}

template <class F>
int with_roll_kernel(Tiles t, F &&f)
{
    if (t.t1 == 4 && t.t2 == 4) return f.template operator()<4, 4>();
    if (t.t1 == 8 && t.t2 == 8) return f.template operator()<8, 8>();
    if (t.t1 == 13 && t.t2 == 7) return f.template operator()<13, 7>();
    return fail(QSDM_ERR_UNSUPPORTED, "no kernel for %d x %d tiles", t.t1, t.t2);
}

int cu_count(int *out)
{
    static std::mutex m;
    static std::unordered_map<int, int> cus;
    int dev = 0;
    QSDM_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(m);
    auto it = cus.find(dev);
    if (it == cus.end()) {
        int v = 0;
        QSDM_HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        it = cus.emplace(dev, v > 0 ? v : 1).first;
    }
    *out = it->second;
    return QSDM_OK;
}

bool misaligned(const void *p) { return ((uintptr_t)p & 15) != 0; }

// workspace: the nominal [n,horizon,4] float32 first (rows of 16 bytes), then the scores / weights [n,paths] float64
size_t nominal_bytes(int64_t n, int horizon) { return (size_t)n * (size_t)horizon * 4 * sizeof(float); }

int check_shape(int64_t n, int horizon, int paths)
{
    if (n <= 0) return fail(QSDM_ERR_INVALID, "n must be >= 1, got %lld", (long long)n);
    if (horizon < 1 || horizon > QSDM_MAX_HORIZON) return fail(QSDM_ERR_INVALID, "horizon must be in [1, %d], got %d", QSDM_MAX_HORIZON, horizon);
    if (paths < 1 || paths > QSDM_MAX_PATHS) return fail(QSDM_ERR_INVALID, "paths must be in [1, %d], got %d", QSDM_MAX_PATHS, paths);
    const int tiles_per_env = (paths + 15) / 16;
    if (n > (int64_t)0x7fffffff / tiles_per_env)
        return fail(QSDM_ERR_INVALID, "n * ceil(paths / 16) must be below 2^31, got %lld x %d", (long long)n, tiles_per_env);
    return QSDM_OK;
}

}  // namespace

extern "C" {

int qsdm_version(void) { return QSDM_VERSION; }

const char *qsdm_last_error(void) { return g_err; }

int qsdm_workspace_bytes(int64_t n, int32_t horizon, int32_t paths, size_t *bytes)
{
    if (!bytes) return fail(QSDM_ERR_INVALID, "bytes is NULL");
    if (int rc = check_shape(n, horizon, paths)) return rc;
    *bytes = nominal_bytes(n, horizon) + (size_t)n * (size_t)paths * sizeof(double);
    return QSDM_OK;
}

int qsdm_mppi_plan(const void *image, int32_t h1, int32_t h2, int64_t n, const float *obs, uint64_t seed, uint64_t gid0, uint64_t k,
                   int32_t horizon, int32_t paths, int32_t iterations, float lambda, float sigma, int32_t shift,
                   const float *nominal_in, const float *noise, void *workspace, float *actions, float *nominal_out,
                   double *best_score, double *scores, float *trace, float *candidates, float *traj, void *stream)
{
    if (!image || !obs || !workspace || !actions || !nominal_out)
        return fail(QSDM_ERR_INVALID, "image, obs, workspace, actions and nominal_out must not be NULL");
    if (int rc = check_shape(n, horizon, paths)) return rc;
    if (iterations < 1 || iterations > QSDM_MAX_ITERATIONS)
        return fail(QSDM_ERR_INVALID, "iterations must be in [1, %d], got %d", QSDM_MAX_ITERATIONS, iterations);
    if (k >> 33) return fail(QSDM_ERR_INVALID, "k must be below 2^33, got %llu", (unsigned long long)k);
    if (!(lambda > 0.0f) || !isfinite(lambda)) return fail(QSDM_ERR_INVALID, "lambda must be positive and finite, got %g", (double)lambda);
    if (!(sigma >= 0.0f) || !isfinite(sigma)) return fail(QSDM_ERR_INVALID, "sigma must be >= 0 and finite, got %g", (double)sigma);
    if (shift != 0 && shift != 1) return fail(QSDM_ERR_INVALID, "shift must be 0 or 1, got %d", shift);
    Tiles t;
    if (int rc = choose_tiles(h1, h2, &t)) return rc;
    if (misaligned(image) || misaligned(workspace) || misaligned(actions) || misaligned(nominal_out) || misaligned(nominal_in) ||
        misaligned(noise) || misaligned(trace) || misaligned(candidates))
        return fail(QSDM_ERR_INVALID, "image, workspace, actions, nominal_in, nominal_out, noise, trace and candidates must be 16-byte aligned");
    int cus = 1;
    if (int rc = cu_count(&cus)) return rc;

    float *const U_ws = (float *)workspace;
    double *const S = (double *)((char *)workspace + nominal_bytes(n, horizon));
    const int tiles_per_env = (paths + 15) / 16;
    const int64_t tiles_total = n * tiles_per_env;
    const int64_t groups = (tiles_total + qsd::kDynBlock / 64 - 1) / (qsd::kDynBlock / 64);
    for (int it = 0; it < iterations; ++it) {
        const bool last = it == iterations - 1;
        const qsd::DrawArgs D{seed, gid0, k, horizon, paths, it, sigma, noise};
        // iteration 0 reads the caller's nominal through the shift; the later ones the workspace's, as it stands
        const float *U = it == 0 ? nominal_in : U_ws;
        const int sh = it == 0 ? shift : 0;
        const qsd::RollArgs A{(const float *)image, obs, D, U, sh, tiles_per_env, tiles_total, S, last ? traj : nullptr};
        int rc = with_roll_kernel(t, [&]<int T1, int T2>() -> int {
            // persistent grid: as many workgroups as the image lets the device hold at once (at most 4 per CU), each loads the image once
            constexpr size_t lds = (size_t)qsd::image_layout(T1, T2).floats * sizeof(float);
            constexpr int per_cu = QSDM_LDS_BYTES / lds < 4 ? (int)(QSDM_LDS_BYTES / lds) : 4;
            static_assert(per_cu >= 1, "image does not fit in LDS");
            const int64_t resident = (int64_t)cus * per_cu;
            hipLaunchKernelGGL((qsd::k_dynm_roll<T1, T2>), dim3((unsigned)(groups < resident ? groups : resident)), dim3(qsd::kDynBlock), 0,
                               (hipStream_t)stream, A);
            return QSDM_OK;
        });
        if (rc) return rc;
        QSDM_HIP_TRY(hipGetLastError());
        const qsd::UpdateArgs X{(const float *)image, t.t1, t.t2, qsd::image_layout(t.t1, t.t2).floats, D, iterations, sh, (double)lambda, U,
                                U_ws, S, actions, nominal_out, best_score, scores, trace, candidates};
        hipLaunchKernelGGL(qsd::k_dynm_update, dim3((unsigned)n), dim3(qsd::kUpdBlock), 0, (hipStream_t)stream, X);
        QSDM_HIP_TRY(hipGetLastError());
    }
    return QSDM_OK;
}

}  // extern "C"
