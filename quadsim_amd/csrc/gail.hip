// gail.hip -- libquadsim_gail.so: the C ABI of include/quadsim_gail.h over the kernels of gail_kernels.hpp.  ONE translation unit
// of its own: nothing here is part of the other six libraries.  Shared at the source level only: train_pieces.hpp (the Adam
// step and the chunk geometry), quadsim_device.hpp (q_tanh) and side_host.hpp (error
// text, the Adam and pointer checks, the fill of the args the fits have in common, the compute-unit count).
#include "../../include/quadsim_gail.h"
#include "side_host.hpp"
#include "gail_kernels.hpp"

static_assert(QSG_OK == kOk && QSG_ERR_INVALID == kErrInvalid && QSG_ERR_HIP == kErrHip, "side_host.hpp returns the codes of quadsim_gail.h");
static_assert(QSG_STATS == qsg::kStats, "the statistics of a step");

namespace {

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

void elems(int H, size_t e[6])
{
    const size_t h = (size_t)H;
    e[0] = 16 * h; e[1] = h; e[2] = h * h; e[3] = h; e[4] = h; e[5] = 1;
}

int check_net(const QsgNet *net)
{
    if (net->struct_size != sizeof(QsgNet))
        return fail(QSG_ERR_INVALID, "QsgNet.struct_size is %u, expected %zu", net->struct_size, sizeof(QsgNet));
    if (net->hidden < 1 || net->hidden > QSG_MAX_HIDDEN)
        return fail(QSG_ERR_INVALID, "hidden must be in [1, %d], got %d", QSG_MAX_HIDDEN, net->hidden);
    if (!net->mean || !net->rscale || misaligned(net->mean) || misaligned(net->rscale))
        return fail(QSG_ERR_INVALID, "mean or rscale is NULL or not 4-byte aligned");
    return kOk;
}

}  // namespace

extern "C" {

int qsg_version(void) { return QSG_VERSION; }

const char *qsg_last_error(void) { return g_err; }

int qsg_fit(const QsgNet *net, const float *gen_obs, const float *gen_act, int64_t n_gen, const float *exp_obs, const float *exp_act,
            int64_t n_exp, const int32_t *gen_idx, const int32_t *exp_idx, const int32_t *counts, int32_t steps, int32_t batch,
            double entcoeff, double lr, double beta1, double beta2, double eps, int64_t t0, float *stats, float *const *grads,
            void *stream)
{
    if (!net || !gen_obs || !gen_act || !exp_obs || !exp_act || !gen_idx || !exp_idx || !stats)
        return fail(QSG_ERR_INVALID, "net, the four data arrays, gen_idx, exp_idx and stats must not be NULL");
    if (int rc = check_net(net)) return rc;
    if (batch < 1 || batch > QSG_MAX_BATCH) return fail(QSG_ERR_INVALID, "batch must be in [1, %d], got %d", QSG_MAX_BATCH, batch);
    if (steps < 1 || steps > QSG_MAX_STEPS) return fail(QSG_ERR_INVALID, "steps must be in [1, %d], got %d", QSG_MAX_STEPS, steps);
    if (n_gen < 1 || n_gen > 0x7fffffffll) return fail(QSG_ERR_INVALID, "n_gen must be in [1, 2^31), got %lld", (long long)n_gen);
    if (n_exp < 1 || n_exp > 0x7fffffffll) return fail(QSG_ERR_INVALID, "n_exp must be in [1, 2^31), got %lld", (long long)n_exp);
    if (!isfinite(entcoeff)) return fail(QSG_ERR_INVALID, "entcoeff must be finite, got %g", entcoeff);
    if (int rc = check_adam_t0(t0, steps, "steps")) return rc;
    if (int rc = check_adam_rates(lr, beta1, beta2, eps)) return rc;
    if (misaligned(gen_obs) || misaligned(gen_act) || misaligned(exp_obs) || misaligned(exp_act) || misaligned(gen_idx) ||
        misaligned(exp_idx) || misaligned(counts) || misaligned(stats) || bad_six(net->w, net->m, net->v, grads))
        return fail(QSG_ERR_INVALID, "a tensor of the net or of the call is NULL or not 4-byte aligned");
    // everything the kernel writes, against each other
    size_t e[6];
    elems(net->hidden, e);
    Range rs[25];
    int nr = 0;
    for (int i = 0; i < 6; ++i) {
        float *const ps[4] = {net->w[i], net->m[i], net->v[i], grads ? grads[i] : nullptr};
        for (int j = 0; j < 4; ++j)
            if (ps[j]) rs[nr++] = Range{(uintptr_t)ps[j], (uintptr_t)ps[j] + 4 * e[i]};
    }
    rs[nr++] = Range{(uintptr_t)stats, (uintptr_t)stats + 4 * (size_t)steps * QSG_STATS};
    if (overlap(rs, nr)) return fail(QSG_ERR_INVALID, "two tensors the call writes overlap");

    qsg::FitArgs F{};
    fill_fit_args(F, net->w, net->m, net->v, grads, lr, beta1, beta2, eps, batch, t0);
    F.mean = net->mean; F.rscale = net->rscale;
    F.obs[0] = gen_obs; F.act[0] = gen_act; F.idx[0] = gen_idx;
    F.obs[1] = exp_obs; F.act[1] = exp_act; F.idx[1] = exp_idx;
    F.counts = counts; F.stats = stats; F.entcoeff = entcoeff;
    F.hidden = net->hidden; F.steps = steps;
    if (net->hidden <= 64)                                   // one workgroup: one CU's worth of work
        hipLaunchKernelGGL(qsg::k_gail_fit<64>, dim3(1), dim3(qsg::kFitBlock), 0, (hipStream_t)stream, F);
    else
        hipLaunchKernelGGL(qsg::k_gail_fit<128>, dim3(1), dim3(qsg::kFitBlock), 0, (hipStream_t)stream, F);
    HIP_TRY(hipGetLastError());
    return QSG_OK;
}

int qsg_reward(const QsgNet *net, const float *obs, const float *act, int64_t rows, int64_t n_envs, int64_t n_steps, float *reward,
               float *logits, int32_t grid, void *stream)
{
    if (!net || !obs || !act || !reward) return fail(QSG_ERR_INVALID, "net, obs, act and reward must not be NULL");
    if (int rc = check_net(net)) return rc;
    if (rows < 1 || rows > 0x7fffffffll) return fail(QSG_ERR_INVALID, "rows must be in [1, 2^31), got %lld", (long long)rows);
    if (n_envs < 0 || n_steps < 0 || (n_envs == 0) != (n_steps == 0) || (n_envs > 0 && (n_envs > rows || n_steps > rows || n_envs * n_steps != rows)))
        return fail(QSG_ERR_INVALID, "n_envs and n_steps must both be 0 or multiply to rows = %lld, got %lld x %lld", (long long)rows,
                    (long long)n_envs, (long long)n_steps);
    if (grid < 0 || grid > 65535) return fail(QSG_ERR_INVALID, "grid must be in [0, 65535], got %d", grid);
    bool bad = misaligned(obs) || misaligned(act) || misaligned(reward) || misaligned(logits);
    for (int i = 0; i < 6; ++i) bad = bad || !net->w[i] || misaligned(net->w[i]);
    if (bad) return fail(QSG_ERR_INVALID, "a tensor of the net or of the call is NULL or not 4-byte aligned");
    Range rs[2] = {{(uintptr_t)reward, (uintptr_t)reward + 4 * (size_t)rows}, {(uintptr_t)logits, (uintptr_t)logits + 4 * (size_t)rows}};
    if (logits && overlap(rs, 2)) return fail(QSG_ERR_INVALID, "reward and logits overlap");

    qsg::RewardArgs A{};
    for (int i = 0; i < 6; ++i) A.w[i] = net->w[i];
    A.mean = net->mean; A.rscale = net->rscale; A.obs = obs; A.act = act; A.reward = reward; A.logits = logits;
    A.rows = rows; A.tiles = (rows + 15) / 16; A.n_envs = (int)n_envs; A.n_steps = (int)n_steps; A.hidden = net->hidden;
    constexpr int kWaves = qsg::kRewardBlock / 64;
    const int64_t need = (A.tiles + kWaves - 1) / kWaves;    // workgroups with a tile for every wave
    int64_t g = grid;
    if (!g) {
        int cus = 0;
        if (int rc = cu_count(&cus)) return rc;
        g = cus;                                             // the image leaves room for one workgroup a compute unit
    }
    g = g < need ? g : need;
    if (net->hidden <= 64)
        hipLaunchKernelGGL(qsg::k_gail_reward<64>, dim3((unsigned)g), dim3(qsg::kRewardBlock), 0, (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(qsg::k_gail_reward<128>, dim3((unsigned)g), dim3(qsg::kRewardBlock), 0, (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return QSG_OK;
}

int qsg_math(int32_t kind, const float *x, float *y, int64_t n, void *stream)
{
    if (!x || !y || misaligned(x) || misaligned(y)) return fail(QSG_ERR_INVALID, "x or y is NULL or not 4-byte aligned");
    if (kind < 0 || kind > 4) return fail(QSG_ERR_INVALID, "kind must be in [0, 4], got %d", kind);
    if (n < 1 || n > 0x7fffffffll) return fail(QSG_ERR_INVALID, "n must be in [1, 2^31), got %lld", (long long)n);
    const int64_t blocks = (n + qsg::kMathBlock - 1) / qsg::kMathBlock;
    hipLaunchKernelGGL(qsg::k_gail_math, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(qsg::kMathBlock), 0, (hipStream_t)stream,
                       (int)kind, x, y, n);
    HIP_TRY(hipGetLastError());
    return QSG_OK;
}

}  // extern "C"
