// dynmppi.hip -- libquadsim_dynmppi.so: the C ABI of include/quadsim_dyn_mppi.h over the kernels of dynmppi_kernels.hpp.  ONE
// translation unit of its own: nothing here is part of libquadsim_hip.so or libquadsim_dyn.so.  Shared with them at the source
// level only: quadsim_device.hpp (Philox keying, normals), dynplan_kernels.hpp / dynplan_image.hpp (the model step and the
// layout of the image that qsd_net_pack writes), side_host.hpp (error text, checks) and dynplan_host.hpp (tiles, dispatch, grid,
// shape checks).  No host table of images: the caller names the widths, the kernels check the image header.
#include "../../include/quadsim_dyn_mppi.h"
#include "side_host.hpp"
#include "dynmppi_kernels.hpp"
#include "dynplan_host.hpp"

static_assert(QSDM_OK == kOk && QSDM_ERR_INVALID == kErrInvalid && QSDM_ERR_HIP == kErrHip && QSDM_ERR_UNSUPPORTED == kErrUnsupported,
              "side_host.hpp returns the codes of quadsim_dyn_mppi.h");

namespace {

// workspace: the nominal [n,horizon,4] float32 first (rows of 16 bytes), then the scores / weights [n,paths] float64
size_t nominal_bytes(int64_t n, int horizon) { return (size_t)n * (size_t)horizon * 4 * sizeof(float); }

int check_shape(int64_t n, int horizon, int paths, int *tiles_per_env)
{
    if (int rc = check_plan_shape(n, horizon, QSDM_MAX_HORIZON, paths, QSDM_MAX_PATHS)) return rc;
    return check_plan_tiles(n, paths, tiles_per_env);
}

}  // namespace

extern "C" {

int qsdm_version(void) { return QSDM_VERSION; }

const char *qsdm_last_error(void) { return g_err; }

int qsdm_workspace_bytes(int64_t n, int32_t horizon, int32_t paths, size_t *bytes)
{
    if (!bytes) return fail(QSDM_ERR_INVALID, "bytes is NULL");
    int tiles_per_env = 0;
    if (int rc = check_shape(n, horizon, paths, &tiles_per_env)) return rc;
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
    int tiles_per_env = 0;
    if (int rc = check_shape(n, horizon, paths, &tiles_per_env)) return rc;
    if (iterations < 1 || iterations > QSDM_MAX_ITERATIONS)
        return fail(QSDM_ERR_INVALID, "iterations must be in [1, %d], got %d", QSDM_MAX_ITERATIONS, iterations);
    if (k >> 33) return fail(QSDM_ERR_INVALID, "k must be below 2^33, got %llu", (unsigned long long)k);
    if (!(lambda > 0.0f) || !isfinite(lambda)) return fail(QSDM_ERR_INVALID, "lambda must be positive and finite, got %g", (double)lambda);
    if (!(sigma >= 0.0f) || !isfinite(sigma)) return fail(QSDM_ERR_INVALID, "sigma must be >= 0 and finite, got %g", (double)sigma);
    if (shift != 0 && shift != 1) return fail(QSDM_ERR_INVALID, "shift must be 0 or 1, got %d", shift);
    Tiles t;
    if (int rc = choose_tiles(h1, h2, QSDM_LDS_BYTES, &t)) return rc;
    if (misaligned(image, 15) || misaligned(workspace, 15) || misaligned(actions, 15) || misaligned(nominal_out, 15) ||
        misaligned(nominal_in, 15) || misaligned(noise, 15) || misaligned(trace, 15) || misaligned(candidates, 15))
        return fail(QSDM_ERR_INVALID, "image, workspace, actions, nominal_in, nominal_out, noise, trace and candidates must be 16-byte aligned");
    int cus = 1;
    if (int rc = cu_count(&cus)) return rc;

    float *const U_ws = (float *)workspace;
    double *const S = (double *)((char *)workspace + nominal_bytes(n, horizon));
    const int64_t tiles_total = n * tiles_per_env;
    for (int it = 0; it < iterations; ++it) {
        const bool last = it == iterations - 1;
        const qsd::DrawArgs D{seed, gid0, k, horizon, paths, it, sigma, noise};
        // iteration 0 reads the caller's nominal through the shift; the later ones the workspace's, as it stands
        const float *U = it == 0 ? nominal_in : U_ws;
        const int sh = it == 0 ? shift : 0;
        const qsd::RollArgs A{(const float *)image, obs, D, U, sh, tiles_per_env, tiles_total, S, last ? traj : nullptr};
        int rc = with_tiles_kernel(t, [&]<int T1, int T2>() -> int {
            hipLaunchKernelGGL((qsd::k_dynm_roll<T1, T2>), dim3(persistent_grid<T1, T2, QSDM_LDS_BYTES>(cus, tiles_total)),
                               dim3(qsd::kDynBlock), 0, (hipStream_t)stream, A);
            return QSDM_OK;
        });
        if (rc) return rc;
        HIP_TRY(hipGetLastError());
        const qsd::UpdateArgs X{(const float *)image, t.t1, t.t2, qsd::image_layout(t.t1, t.t2).floats, D, iterations, sh, (double)lambda, U,
                                U_ws, S, actions, nominal_out, best_score, scores, trace, candidates};
        hipLaunchKernelGGL(qsd::k_dynm_update, dim3((unsigned)n), dim3(qsd::kUpdBlock), 0, (hipStream_t)stream, X);
        HIP_TRY(hipGetLastError());
    }
    return QSDM_OK;
}

}  // extern "C"
