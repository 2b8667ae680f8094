// dynplan.hip -- libquadsim_dyn.so: the C ABI of include/quadsim_dyn.h over the kernels of dynplan_kernels.hpp.  ONE translation
// unit of its own: nothing here is part of libquadsim_hip.so, and the only thing shared with it is quadsim_device.hpp (Philox
// keying of the candidate actions).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <mutex>
#include <unordered_map>

#include "../../include/quadsim_dyn.h"
#include "dynplan_kernels.hpp"

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

#define QSD_HIP_TRY(expr)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return fail(QSD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// the compiled instantiations, cheapest first: a net runs on the first pair of tile counts that covers it
struct Tiles { int t1, t2; };
constexpr Tiles kTiles[] = {{4, 4}, {8, 8}, {13, 7}};

int choose_tiles(int h1, int h2, Tiles *out)
{
    if (h1 < 1 || h2 < 1) return fail(QSD_ERR_INVALID, "hidden widths must be >= 1, got (%d, %d)", h1, h2);
    for (const Tiles &t : kTiles)
        if (h1 <= 16 * t.t1 && h2 <= 16 * t.t2) {
            const size_t bytes = (size_t)qsd::image_layout(t.t1, t.t2).floats * sizeof(float);
            if (bytes > QSD_LDS_BYTES) return fail(QSD_ERR_UNSUPPORTED, "the image of a (%d, %d) net (%zu bytes) does not fit in LDS", h1, h2, bytes);
            *out = t;
            return QSD_OK;
        }
    return fail(QSD_ERR_UNSUPPORTED, "hidden widths (%d, %d) are outside the supported range: h1, h2 <= 128, or h1 <= 208 and h2 <= 112", h1,
                h2);
}

// image pointer -> the tile counts it was packed for (the plan is launched without reading device memory)
std::mutex g_images_mutex;
std::unordered_map<const void *, Tiles> g_images;

template <class F>
int with_plan_kernel(Tiles t, F &&f)
{
    if (t.t1 == 4 && t.t2 == 4) return f.template operator()<4, 4>();
    if (t.t1 == 8 && t.t2 == 8) return f.template operator()<8, 8>();
    if (t.t1 == 13 && t.t2 == 7) return f.template operator()<13, 7>();
    return fail(QSD_ERR_UNSUPPORTED, "no kernel for %d x %d tiles", t.t1, t.t2);
}

int cu_count(int *out)
{
    static std::mutex m;
    static std::unordered_map<int, int> cus;
    int dev = 0;
    QSD_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(m);
    auto it = cus.find(dev);
    if (it == cus.end()) {
        int v = 0;
        QSD_HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
        it = cus.emplace(dev, v > 0 ? v : 1).first;
    }
    *out = it->second;
    return QSD_OK;
}

}  // namespace

extern "C" {

int qsd_version(void) { return QSD_VERSION; }

const char *qsd_last_error(void) { return g_err; }

int qsd_net_image_bytes(int32_t h1, int32_t h2, size_t *bytes)
{
    if (!bytes) return fail(QSD_ERR_INVALID, "bytes is NULL");
    Tiles t;
    if (int rc = choose_tiles(h1, h2, &t)) return rc;
    *bytes = (size_t)qsd::image_layout(t.t1, t.t2).floats * sizeof(float);
    return QSD_OK;
}

int qsd_net_pack(const QsdNet *net, void *image, void *stream)
{
    if (!net || !image) return fail(QSD_ERR_INVALID, "net or image is NULL");
    if (net->struct_size != sizeof(QsdNet)) return fail(QSD_ERR_INVALID, "QsdNet.struct_size is %u, expected %zu", net->struct_size, sizeof(QsdNet));
    if (((uintptr_t)image & 15) != 0) return fail(QSD_ERR_INVALID, "image must be 16-byte aligned");
    Tiles t;
    if (int rc = choose_tiles(net->h1, net->h2, &t)) return rc;
    if (!net->wt1 || !net->b1 || !net->wt2 || !net->b2 || !net->wt3 || !net->b3 || !net->in_mean || !net->in_rscale || !net->out_std ||
        !net->out_mean)
        return fail(QSD_ERR_INVALID, "a weight, bias or normaliser pointer of the net is NULL");
    const qsd::ImageLayout L = qsd::image_layout(t.t1, t.t2);
    const qsd::PackArgs N{net->h1, net->h2, net->wt1, net->b1, net->wt2, net->b2, net->wt3, net->b3,
                          net->in_mean, net->in_rscale, net->out_std, net->out_mean};
    hipLaunchKernelGGL(qsd::k_dyn_pack, dim3((L.floats + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, L, (float *)image);
    QSD_HIP_TRY(hipGetLastError());
    std::lock_guard<std::mutex> lock(g_images_mutex);
    g_images[image] = t;
    return QSD_OK;
}

int qsd_plan_workspace_bytes(int64_t n, int32_t paths, size_t *bytes)
{
    if (!bytes) return fail(QSD_ERR_INVALID, "bytes is NULL");
    if (n <= 0) return fail(QSD_ERR_INVALID, "n must be >= 1, got %lld", (long long)n);
    if (paths < 1 || paths > QSD_MAX_PATHS) return fail(QSD_ERR_INVALID, "paths must be in [1, %d], got %d", QSD_MAX_PATHS, paths);
    *bytes = (size_t)n * (size_t)paths * sizeof(double);
    return QSD_OK;
}

int qsd_shooting_plan(const void *image, int64_t n, const float *obs, uint64_t seed, uint64_t gid0, uint64_t k, int32_t horizon,
                      int32_t paths, void *workspace, float *actions, double *best_score, int32_t *best_index, float *sequence,
                      double *scores, float *traj, void *stream)
{
    if (!image || !obs || !workspace || !actions) return fail(QSD_ERR_INVALID, "image, obs, workspace and actions must not be NULL");
    if (n <= 0) return fail(QSD_ERR_INVALID, "n must be >= 1, got %lld", (long long)n);
    if (horizon < 1 || horizon > QSD_MAX_HORIZON) return fail(QSD_ERR_INVALID, "horizon must be in [1, %d], got %d", QSD_MAX_HORIZON, horizon);
    if (paths < 1 || paths > QSD_MAX_PATHS) return fail(QSD_ERR_INVALID, "paths must be in [1, %d], got %d", QSD_MAX_PATHS, paths);
    if (k >> 36) return fail(QSD_ERR_INVALID, "k must be below 2^36, got %llu", (unsigned long long)k);
    const int tiles_per_env = (paths + 15) / 16;
    if (n > (int64_t)0x7fffffff / tiles_per_env) return fail(QSD_ERR_INVALID, "n * ceil(paths / 16) must be below 2^31, got %lld x %d", (long long)n, tiles_per_env);
    Tiles t;
    {
        std::lock_guard<std::mutex> lock(g_images_mutex);
        auto it = g_images.find(image);
        if (it == g_images.end()) return fail(QSD_ERR_INVALID, "image %p was not packed by qsd_net_pack", image);
        t = it->second;
    }
    int cus = 1;
    if (int rc = cu_count(&cus)) return rc;

    qsd::DynArgs A{};
    A.image = (const float *)image; A.obs = obs; A.seed = seed; A.gid0 = gid0; A.k = k;
    A.horizon = horizon; A.paths = paths; A.tiles_per_env = tiles_per_env; A.n = n; A.tiles_total = n * tiles_per_env;
    A.scores = scores ? scores : (double *)workspace; A.traj = traj;
    const int64_t groups = (A.tiles_total + qsd::kDynBlock / 64 - 1) / (qsd::kDynBlock / 64);
    int rc = with_plan_kernel(t, [&]<int T1, int T2>() -> int {
        // persistent grid: as many workgroups as the image lets the device hold at once (at most 4 per CU), each loads the image once
        constexpr size_t lds = (size_t)qsd::image_layout(T1, T2).floats * sizeof(float);
        constexpr int per_cu = QSD_LDS_BYTES / lds < 4 ? (int)(QSD_LDS_BYTES / lds) : 4;
        static_assert(per_cu >= 1, "image does not fit in LDS");
        const int64_t resident = (int64_t)cus * per_cu;
        hipLaunchKernelGGL((qsd::k_dyn_plan<T1, T2>), dim3((unsigned)(groups < resident ? groups : resident)), dim3(qsd::kDynBlock), 0,
                           (hipStream_t)stream, A);
        return QSD_OK;
    });
    if (rc) return rc;
    QSD_HIP_TRY(hipGetLastError());
    const qsd::FinishArgs X{seed, gid0, k, horizon, paths, A.scores, actions, best_score, best_index, sequence};
    hipLaunchKernelGGL(qsd::k_dyn_finish, dim3((unsigned)n), dim3(qsd::kDynBlock), 0, (hipStream_t)stream, X);
    QSD_HIP_TRY(hipGetLastError());
    return QSD_OK;
}

}  // extern "C"
