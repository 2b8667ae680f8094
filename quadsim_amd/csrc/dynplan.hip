// dynplan.hip -- libquadsim_dyn.so: the C ABI of include/quadsim_dyn.h over the kernels of dynplan_kernels.hpp.  ONE translation
// unit of its own: nothing here is part of libquadsim_hip.so.  Shared at the source level only: quadsim_device.hpp with the main
// library (Philox keying of the candidate actions), side_host.hpp with the other side libraries (error text, checks) and
// dynplan_host.hpp with dynmppi.hip (tiles, dispatch, grid, shape checks).
#include "../../include/quadsim_dyn.h"
#include "side_host.hpp"
#include "dynplan_kernels.hpp"
#include "dynplan_host.hpp"

static_assert(QSD_OK == kOk && QSD_ERR_INVALID == kErrInvalid && QSD_ERR_HIP == kErrHip && QSD_ERR_UNSUPPORTED == kErrUnsupported,
              "side_host.hpp returns the codes of quadsim_dyn.h");

namespace {

// image pointer -> the tile counts it was packed for (the plan is launched without reading device memory)
std::mutex g_images_mutex;
std::unordered_map<const void *, Tiles> g_images;

}  // namespace

extern "C" {

int qsd_version(void) { return QSD_VERSION; }

const char *qsd_last_error(void) { return g_err; }

int qsd_net_image_bytes(int32_t h1, int32_t h2, size_t *bytes)
{
    if (!bytes) return fail(QSD_ERR_INVALID, "bytes is NULL");
    Tiles t;
    if (int rc = choose_tiles(h1, h2, QSD_LDS_BYTES, &t)) return rc;
    *bytes = (size_t)qsd::image_layout(t.t1, t.t2).floats * sizeof(float);
    return QSD_OK;
}

int qsd_net_pack(const QsdNet *net, void *image, void *stream)
{
    if (!net || !image) return fail(QSD_ERR_INVALID, "net or image is NULL");
    if (net->struct_size != sizeof(QsdNet)) return fail(QSD_ERR_INVALID, "QsdNet.struct_size is %u, expected %zu", net->struct_size, sizeof(QsdNet));
    if (misaligned(image, 15)) return fail(QSD_ERR_INVALID, "image must be 16-byte aligned");
    Tiles t;
    if (int rc = choose_tiles(net->h1, net->h2, QSD_LDS_BYTES, &t)) return rc;
    if (!net->wt1 || !net->b1 || !net->wt2 || !net->b2 || !net->wt3 || !net->b3 || !net->in_mean || !net->in_rscale || !net->out_std ||
        !net->out_mean)
        return fail(QSD_ERR_INVALID, "a weight, bias or normaliser pointer of the net is NULL");
    const qsd::ImageLayout L = qsd::image_layout(t.t1, t.t2);
    const qsd::PackArgs N{net->h1, net->h2, net->wt1, net->b1, net->wt2, net->b2, net->wt3, net->b3,
                          net->in_mean, net->in_rscale, net->out_std, net->out_mean};
    hipLaunchKernelGGL(qsd::k_dyn_pack, dim3((L.floats + 255) / 256), dim3(256), 0, (hipStream_t)stream, N, L, (float *)image);
    HIP_TRY(hipGetLastError());
    std::lock_guard<std::mutex> lock(g_images_mutex);
    g_images[image] = t;
    return QSD_OK;
}

int qsd_plan_workspace_bytes(int64_t n, int32_t paths, size_t *bytes)
{
    if (!bytes) return fail(QSD_ERR_INVALID, "bytes is NULL");
    if (int rc = check_plan_shape(n, 1, QSD_MAX_HORIZON, paths, QSD_MAX_PATHS)) return rc;       // the workspace has no horizon
    *bytes = (size_t)n * (size_t)paths * sizeof(double);
    return QSD_OK;
}

int qsd_shooting_plan(const void *image, int64_t n, const float *obs, uint64_t seed, uint64_t gid0, uint64_t k, int32_t horizon,
                      int32_t paths, void *workspace, float *actions, double *best_score, int32_t *best_index, float *sequence,
                      double *scores, float *traj, void *stream)
{
    if (!image || !obs || !workspace || !actions) return fail(QSD_ERR_INVALID, "image, obs, workspace and actions must not be NULL");
    if (int rc = check_plan_shape(n, horizon, QSD_MAX_HORIZON, paths, QSD_MAX_PATHS)) return rc;
    if (k >> 36) return fail(QSD_ERR_INVALID, "k must be below 2^36, got %llu", (unsigned long long)k);
    int tiles_per_env = 0;
    if (int rc = check_plan_tiles(n, paths, &tiles_per_env)) return rc;
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
    int rc = with_tiles_kernel(t, [&]<int T1, int T2>() -> int {
        hipLaunchKernelGGL((qsd::k_dyn_plan<T1, T2>), dim3(persistent_grid<T1, T2, QSD_LDS_BYTES>(cus, A.tiles_total)), dim3(qsd::kDynBlock),
                           0, (hipStream_t)stream, A);
        return QSD_OK;
    });
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    const qsd::FinishArgs X{seed, gid0, k, horizon, paths, A.scores, actions, best_score, best_index, sequence};
    hipLaunchKernelGGL(qsd::k_dyn_finish, dim3((unsigned)n), dim3(qsd::kDynBlock), 0, (hipStream_t)stream, X);
    HIP_TRY(hipGetLastError());
    return QSD_OK;
}

}  // extern "C"
