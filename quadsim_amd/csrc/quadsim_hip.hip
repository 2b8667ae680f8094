// quadsim_hip.hip -- kernels + C ABI of libquadsim_hip.so (gfx950 only).
//
// HBM layout of the persistent env state: AoSoA tiles of 64 envs (one
// wavefront).  Tile k holds kRecWords (40) field rows of 64 floats:
//     st[(k*40 + f)*64 + lane]
// so every field access of a wave is one fully coalesced 256-B segment and a
// tile is one contiguous 10 KiB block.  Per-env params (mass, Ixx, Iyy, Izz)
// live in a parallel [tile][4][64] array that is only read when the handle
// uses per-env params.  API-facing buffers keep the reference's row-major
// shapes ([N,4] actions, [N,12] obs, ...).
//
// See include/quadsim.h for the contract of each entry point and the reference
// file:line it replaces.
//
// ONE translation unit (the private-queue code looks the step kernels up by their mangled names in the code object of this
// very library), kept in pieces that are included below at fixed positions:
//     quadsim_device.hpp   the per-env device functions (drone step, controller, state2rel, reward, rocRAND draws)
//     rollout_ops.hpp      GAE, flatten, episode statistics            mlp.hpp              the MLP on the matrix cores
//     kernel_diag.hpp      the in-kernel stamps of the diagnostic builds, the store flavour of the step kernels
//     step_kernels.hpp     StepArgs, the tile I/O helpers, the env step kernels, the reset / fill / state I/O kernels
//     layer1_kernels.hpp   drone step, controller, transforms and state2rel on row-major user arrays
//     policy_kernels.hpp   the actor alone, in a T-step roll-out and over K complete episodes per env (qs_policy_*)
//     runner_kernels.hpp   PPO2 data collection: the one-wave-per-tile and the role-split Runner kernel (qs_runner_rollout*)
//     expert_rollout.hpp   the PID expert: one action, T steps, K complete episodes per env (qs_expert_*)
//     shooting.hpp         random-shooting MPC (qs_shooting_plan)      mppi.hpp             the MPPI planner (qs_mppi_plan)
//     shooting_split.hpp   random shooting with one env's candidates over several workgroups (qs_shooting_plan_split)
//     mppi_split.hpp       MPPI with one env's candidates over several workgroups (qs_mppi_plan_split)
//     env_groups.hpp       env groups (qs_set_groups)                  private_queue.hpp    private AQL queues (qs_set_queue_mode)
//     host_util.hpp        host only: the last-error text (fail), HIP_TRY, roctx ranges, the device guard, and UserIO: how every
//                          entry point hands the caller's buffers to its kernels (in place on a QS_IO_DEVICE handle, through the
//                          staging buffer and its pinned mirror on a QS_IO_HOST handle)
// and here: the handle (QsEnv), its launch / reset helpers, and the C ABI.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <hsa/amd_hsa_signal.h>

#include <elf.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

// -DQS_DEBUG: in-kernel bound checks of every global index (a failed check prints file:line and traps the wave); the
// release build compiles them away.  tools/build_debug.sh builds libquadsim_hip_dbg.so for QUADSIM_HIP_LIB=...
#ifdef QS_DEBUG
#include <cassert>
#define QS_ASSERT(c) assert(c)
#else
#define QS_ASSERT(c) ((void)0)
#endif

#include "../../include/quadsim.h"
#include "host_util.hpp"
#include "quadsim_device.hpp"
#include "rollout_ops.hpp"
#include "mlp.hpp"

using namespace qs;

#include "kernel_diag.hpp"
#include "step_kernels.hpp"
#include "layer1_kernels.hpp"
#include "policy_kernels.hpp"
#include "runner_kernels.hpp"
#include "expert_rollout.hpp"
#include "plan_common.hpp"
#include "shooting.hpp"
#include "mppi.hpp"
#include "shooting_split.hpp"
#include "mppi_split.hpp"

#ifdef QS_STAMP
static unsigned long long *g_host_stamps = nullptr;     // qs_debug_set_stamps: handed to every launch through StepArgs
static unsigned long long g_host_stamp_cap = 0;
#endif

struct QsEnv {
    QsConfig cfg;
    int64_t n = 0, tiles = 0;
    float *st = nullptr, *par = nullptr;
    bool per_env_params = false;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    unsigned long long *d_ctr = nullptr;   // device: step counter, one copy per tile
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float nominal_obs[12] = {0};
    float *gae_ws = nullptr;    // workspace of the chunked GAE scan
    size_t gae_ws_floats = 0;
    float *init = nullptr;      // stored per-env initial states (docking-v1, hovering-v0, qs_set_init_state)
    int obs_dim = 12;
    HostStage stage;            // QS_IO_HOST: where UserIO keeps the caller's buffers during a call
    // env groups (qs_set_groups): contiguous tile ranges stepped on their own streams, optionally by their own launcher threads
    std::vector<struct QsGroup *> groups;
    hipEvent_t fork_ev = nullptr;
    bool main_dirty = true;     // the handle enqueued work on its main stream that the group streams have not been ordered behind
    bool groups_dirty = false;  // group streams hold work the main stream has not been ordered behind
    bool runner_env_major = false;   // qs_set_rollout_layout
    struct QsChain *chain = nullptr; // qs_set_queue_mode: private AQL queue for the step launches
    char *plan_ws = nullptr;    // qs_shooting_plan_split, qs_mppi_plan_split: what crosses between a plan's kernels (plan_workspace)
    size_t plan_ws_bytes = 0;
    int cu_count = 0;           // multiProcessorCount of cfg.device, read at the first automatic choice of `splits`
};

namespace {

StepArgs make_args(const QsEnv *e)
{
    StepArgs A;
    memset(&A, 0, sizeof A);
    A.st = e->st;
    A.par = e->par;
    A.n = e->n;
    A.tile0 = 0; A.tile_end = e->tiles;
    A.io_env0 = 0; A.io_n = e->n;
    A.T = 1;
    A.step_idx = 0;
    A.ctr = e->d_ctr;
    A.gid0 = e->cfg.env_id_offset;
    A.C.kind = e->cfg.kind == QS_KIND_DOCKING_V2 ? 1 : 0;
    A.C.dt = e->cfg.dt;
    A.C.rmax = e->cfg.kind == QS_KIND_DOCKING_V2 ? 10.0f : 3.0f;
    A.C.vdes_x = e->cfg.kind == QS_KIND_DOCKING_V2 ? 0.2f : 0.0f;
    A.init = e->init;
    A.rc.seed = e->cfg.seed;
    for (int i = 0; i < 4; ++i) A.rc.rr[i] = e->cfg.init_range[i];
    A.rc.rr[4] = e->cfg.mass_scale[0]; A.rc.rr[5] = e->cfg.mass_scale[1];
    A.rc.rr[6] = e->cfg.inertia_scale[0]; A.rc.rr[7] = e->cfg.inertia_scale[1];
    A.rc.par_nom[0] = e->cfg.mass;
    for (int i = 0; i < 3; ++i) A.rc.par_nom[1 + i] = e->cfg.inertia[i];
    A.par_nom = Par{e->cfg.mass, e->cfg.inertia[0], e->cfg.inertia[1], e->cfg.inertia[2]};
    A.auto_reset = e->cfg.auto_reset;
    A.randomise = e->cfg.randomise;

    for (int i = 0; i < 12; ++i) A.nominal_obs[i] = e->nominal_obs[i];
#ifdef QS_STAMP
    A.stamps = g_host_stamps; A.stamp_cap = g_host_stamp_cap; A.stamp_tiles = (unsigned long long)e->tiles;
#endif
    return A;
}

// the user buffers of one call of the handle (host_util.hpp)
UserIO user_io(QsEnv *e) { return UserIO(e->cfg.io_space == QS_IO_HOST ? &e->stage : nullptr, e->stream); }

// reset-preparation variant of the role-split kernel for a launch of `tiles` tiles (see kPrepMaxTiles)
std::atomic<int> &prep_forced()
{
    static std::atomic<int> f{getenv("QS_RESET_PREP") ? atoi(getenv("QS_RESET_PREP")) : -1};
    return f;
}

int prep_for(int rmode, int64_t tiles)
{
    const int forced = prep_forced().load(std::memory_order_relaxed);
    if (rmode != 1 && rmode != 2) return 0;
    if (forced == 0 || forced == 2) return forced;
    return tiles <= kPrepMaxTiles ? 2 : 0;
}

// ---- which step-kernel instantiation a launch of the handle uses ---------------------------------------------------------
// The one choice behind launch_env_on (HIP stream), chain_resolve_kernel / res_resolve_kernel (private queues),
// policy_evaluate and qs_debug_step_variant: they all call the helpers below, so that they cannot drift apart.
enum StepFamily { kFamSerial = 0, kFamSplit = 1, kFamResident = 2, kFamChainSplit = 3, kFamChainSerial = 4, kFamHover = 5 };
struct StepVariant {
    int family, integ, params, rmode, prep;    // prep -1: the family has no PREP parameter; rmode -1: k_hover (no RMODE)
};

// (INTEG, PARAMS, RMODE) of the handle as it is now (qs_set_params / qs_set_init_state change it)
StepVariant step_combo(const QsEnv *e)
{
    StepVariant v{kFamSplit, e->cfg.integrator == QS_INTEG_FROZEN ? 0 : 1, 0, 0, -1};
    v.rmode = e->init ? 3 : e->cfg.randomise;          // stored initial states take precedence over `randomise`
    v.params = (v.rmode == 2 || e->per_env_params) ? 1 : 0;    // per-episode params imply per-env params
    return v;
}

// ... and the one mapping of that combination onto template arguments: f.operator()<INTEG, PARAMS, RMODE>() for the combinations
// the step kernels exist in (per-episode params imply per-env params: RMODE 2 only with PARAMS), which every kernel family that
// takes these parameters is instantiated through, guarding with `if constexpr` what it does not support
template <int INTEG, class F>
void with_combo_integ(const StepVariant &v, F &&f)
{
    if (v.rmode == 3) { if (v.params) f.template operator()<INTEG, true, 3>(); else f.template operator()<INTEG, false, 3>(); }
    else if (v.rmode == 2) f.template operator()<INTEG, true, 2>();
    else if (v.rmode == 1) { if (v.params) f.template operator()<INTEG, true, 1>(); else f.template operator()<INTEG, false, 1>(); }
    else { if (v.params) f.template operator()<INTEG, true, 0>(); else f.template operator()<INTEG, false, 0>(); }
}
template <class F>
void with_combo(const StepVariant &v, F &&f)
{
    if (v.integ == 0) with_combo_integ<0>(v, f);
    else with_combo_integ<1>(v, f);
}
// ... and f.operator()<INTEG, PARAMS>() for the kernels that have no RMODE (k_hover, k_shooting_plan, k_mppi).  <.., false> is named before
// <.., true>: the order of instantiation shows in the machine code of two k_shooting_plan (one instruction each)
template <class F>
void with_integ_params(const StepVariant &v, F &&f)
{
    if (v.integ == 0) { if (!v.params) f.template operator()<0, false>(); else f.template operator()<0, true>(); }
    else { if (!v.params) f.template operator()<1, false>(); else f.template operator()<1, true>(); }
}

// role-split kernel up to kSplitMaxEnvs envs (few waves per SIMD: the two half-length streams of a tile overlap), the serial
// kernel above (SIMDs already saturated: the hand-overs only cost).  Both inline the same device functions and the library is
// built with -ffp-contract=on, so they compute the same bits.  QS_SPLIT=0/1 forces one (A/B runs).  The choice follows the
// handle's env count, not the launch's: the groups of a handle are in flight together.
bool split_for(const QsEnv *e)
{
    static const int forced = getenv("QS_SPLIT") ? atoi(getenv("QS_SPLIT")) : -1;
    return forced >= 0 ? forced != 0 : e->n <= kSplitMaxEnvs;
}

// the instantiation a launch of `tiles` tiles of the handle takes (HIP stream; the private queues map it onto their own)
StepVariant step_variant(const QsEnv *e, int64_t tiles)
{
    StepVariant v = step_combo(e);
    if (e->cfg.kind == QS_KIND_HOVERING_V0) { v.family = kFamHover; v.rmode = -1; return v; }
    if (split_for(e)) { v.family = kFamSplit; v.prep = prep_for(v.rmode, tiles); }
    else v.family = kFamSerial;
    return v;
}

template <int INTEG, bool PARAMS, int RMODE>
void launch_one(hipStream_t s, const StepArgs &A, const StepVariant &v)
{
    const int64_t tiles = A.tile_end - A.tile0;
    if (v.family == kFamSplit && v.prep == 2 && (RMODE == 1 || RMODE == 2))
        hipLaunchKernelGGL((k_env_split<INTEG, PARAMS, RMODE, (RMODE == 1 || RMODE == 2) ? 2 : 0>), dim3((unsigned)tiles), dim3(3 * kTile), 0, s, A);
    else if (v.family == kFamSplit) hipLaunchKernelGGL((k_env_split<INTEG, PARAMS, RMODE, 0>), dim3((unsigned)tiles), dim3(2 * kTile), 0, s, A);
    else hipLaunchKernelGGL((k_env<INTEG, PARAMS, RMODE>), dim3((unsigned)((tiles + kBlock / kTile - 1) / (kBlock / kTile))), dim3(kBlock), 0, s, A);
}

// the resident form of every role-split instantiation: dispatched by name from the private queues only (private_queue.hpp)
#define QS_RES_KERNELS(I)                                                                                               \
    template __global__ void k_env_resident<I, false, 0, 0>(StepArgs, ResArgs);                                         \
    template __global__ void k_env_resident<I, true, 0, 0>(StepArgs, ResArgs);                                          \
    template __global__ void k_env_resident<I, false, 1, 0>(StepArgs, ResArgs);                                         \
    template __global__ void k_env_resident<I, true, 1, 0>(StepArgs, ResArgs);                                          \
    template __global__ void k_env_resident<I, false, 1, 2>(StepArgs, ResArgs);                                         \
    template __global__ void k_env_resident<I, true, 1, 2>(StepArgs, ResArgs);                                          \
    template __global__ void k_env_resident<I, true, 2, 0>(StepArgs, ResArgs);                                          \
    template __global__ void k_env_resident<I, true, 2, 2>(StepArgs, ResArgs);                                          \
    template __global__ void k_env_resident<I, false, 3, 0>(StepArgs, ResArgs);                                         \
    template __global__ void k_env_resident<I, true, 3, 0>(StepArgs, ResArgs);
QS_RES_KERNELS(0)
QS_RES_KERNELS(1)
#undef QS_RES_KERNELS

// the env kernels of tiles [A.tile0, A.tile_end) on stream s
int launch_env_on(QsEnv *e, const StepArgs &A, hipStream_t s)
{
    const StepVariant v = step_variant(e, A.tile_end - A.tile0);
    if (v.family == kFamHover) {
        const unsigned grid = (unsigned)((A.tile_end - A.tile0 + kBlock / kTile - 1) / (kBlock / kTile));
        with_integ_params(v, [&]<int INTEG, bool PARAMS>() { hipLaunchKernelGGL((k_hover<INTEG, PARAMS>), dim3(grid), dim3(kBlock), 0, s, A); });
    } else with_combo(v, [&]<int INTEG, bool PARAMS, int RMODE>() { launch_one<INTEG, PARAMS, RMODE>(s, A, v); });
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int launch_env(QsEnv *e, StepArgs &A) { return launch_env_on(e, A, e->stream); }

}  // namespace

#include "env_groups.hpp"

#include "private_queue.hpp"

namespace {

// entry points that use the main stream: order it behind pending group work / the private queue first
int main_stream_entry(QsEnv *e)
{
    if (e->groups_dirty) { int rc = groups_join(e); if (rc) return rc; }
    e->main_dirty = true;
    if (e->chain) {
        int rc = chain_drain(e);
        e->chain->hip_dirty = true;
        e->chain->res_dbg_packets = false;            // a placement-guard test's packet steps end here
        if (rc) return rc;
    }
    return QS_OK;
}

int fill_params(QsEnv *e)
{
    Par P{e->cfg.mass, e->cfg.inertia[0], e->cfg.inertia[1], e->cfg.inertia[2]};
    hipLaunchKernelGGL(k_fill_par, dim3(grid_tiles(e->n)), dim3(kBlock), 0, e->stream, e->par, e->n, P);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

// init_all (qs_create): every env gets its initial state (nominal / stored) and q_des = identity; the per-episode randomisation
// starts at the first reset
int do_reset(QsEnv *e, const uint8_t *d_mask, float *d_obs, int init_all)
{
    StepArgs A = make_args(e);
    A.obs = d_obs;
    if (init_all) A.randomise = 0;
    if (e->cfg.kind == QS_KIND_HOVERING_V0)
        hipLaunchKernelGGL(k_hover_reset, dim3(grid_tiles(e->n)), dim3(kBlock), 0, e->stream, A, d_mask);
    else
        hipLaunchKernelGGL(k_reset, dim3(grid_tiles(e->n)), dim3(kBlock), 0, e->stream, A, d_mask, init_all);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

// CHECK_ENV_RAW: handle + device; CHECK_ENV: + this call uses the main stream (joins pending group work first)
#define CHECK_ENV_RAW(e)                                               \
    if (!(e)) return fail(QS_ERR_INVALID, "%s: null handle", __func__); \
    DeviceGuard guard_((e)->cfg.device);                               \
    if (!guard_.ok) return fail(QS_ERR_HIP, "%s: hipSetDevice(%d) failed", __func__, (e)->cfg.device)
#define CHECK_ENV(e)                                                   \
    CHECK_ENV_RAW(e);                                                  \
    if (!(e)->groups.empty() || (e)->chain) { int rcj_ = main_stream_entry(e); if (rcj_) return rcj_; }

}  // namespace

extern "C" {

int qs_version(void) { return QS_VERSION; }

#ifdef QS_STAMP
int qs_debug_set_stamps(void *dev_ptr, uint64_t capacity_words)
{
    g_host_stamps = (unsigned long long *)dev_ptr;
    g_host_stamp_cap = capacity_words;
    return QS_OK;
}
#endif
const char *qs_last_error(void) { return g_err; }

// Diagnostic (not in quadsim.h; used by tools/hsa_chain_exp.py only): the kernel-argument block qs_step would pass to the
// step kernel for these buffers, so that an experiment can dispatch the very same kernel through a queue of its own.
int qs_debug_step_kernargs(QsEnv *e, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags,
                           float *terminal_obs, void *out, uint64_t cap, uint64_t *size, int32_t *split, int64_t *tiles,
                           int64_t tile0, int64_t tile_end)
{
    if (!e || !out || !size) return fail(QS_ERR_INVALID, "qs_debug_step_kernargs: null argument");
    StepArgs A = make_args(e);
    if (tile_end > tile0) { A.tile0 = tile0; A.tile_end = tile_end; }
    A.actions = actions; A.obs = obs; A.reward = reward; A.done = done; A.flags = flags; A.term_obs = terminal_obs;
    if (cap < sizeof A) return fail(QS_ERR_INVALID, "qs_debug_step_kernargs: buffer too small (%zu needed)", sizeof A);
    memcpy(out, &A, sizeof A);
    *size = sizeof A;
    if (split) *split = split_for(e) ? 1 : 0;
    if (tiles) *tiles = e->tiles;
    return QS_OK;
}

int qs_config_default(QsConfig *cfg)
{
    if (!cfg) return fail(QS_ERR_INVALID, "qs_config_default: null cfg");
    memset(cfg, 0, sizeof *cfg);
    cfg->struct_size = (int32_t)sizeof(QsConfig);
    cfg->kind = QS_KIND_DOCKING_V0;
    cfg->num_envs = 1;
    cfg->device = 0;
    cfg->integrator = QS_INTEG_FROZEN;
    cfg->dt = 0.02f;
    cfg->auto_reset = 0;
    cfg->randomise = QS_RANDOMISE_NONE;
    cfg->io_space = QS_IO_DEVICE;
    cfg->seed = 0;
    cfg->env_id_offset = 0;
    cfg->mass_scale[0] = cfg->mass_scale[1] = 1.0f;
    cfg->inertia_scale[0] = cfg->inertia_scale[1] = 1.0f;
    cfg->mass = 0.18f;
    cfg->inertia[0] = 0.00025f; cfg->inertia[1] = 0.000232f; cfg->inertia[2] = 0.0003738f;
    cfg->stream = nullptr;
    cfg->external_stream = 0;
    return QS_OK;
}

int qs_create(const QsConfig *cfg, QsEnv **out)
{
    if (!cfg || !out) return fail(QS_ERR_INVALID, "qs_create: null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(QsConfig))
        return fail(QS_ERR_INVALID, "qs_create: QsConfig size mismatch (got %d, want %zu)", cfg->struct_size, sizeof(QsConfig));
    if (cfg->num_envs < 1) return fail(QS_ERR_INVALID, "qs_create: num_envs must be >= 1");
    if (cfg->num_envs > ((int64_t)1 << 31)) return fail(QS_ERR_INVALID, "qs_create: num_envs too large");
    // a Philox subsequence is (stream << 48) | gid: a global id of 2^48 or above would draw from another stream
    if (cfg->env_id_offset > ((uint64_t)1 << 48) || cfg->env_id_offset + (uint64_t)cfg->num_envs > ((uint64_t)1 << 48))
        return fail(QS_ERR_INVALID, "qs_create: env_id_offset + num_envs must fit the 48 bits of a global env id (at most 2^48), got %llu + %lld",
                    (unsigned long long)cfg->env_id_offset, (long long)cfg->num_envs);
    if (cfg->kind < QS_KIND_DOCKING_V0 || cfg->kind > QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "qs_create: unknown env kind %d", cfg->kind);
    if ((cfg->kind == QS_KIND_DOCKING_V1 || cfg->kind == QS_KIND_HOVERING_V0) && cfg->randomise == QS_RANDOMISE_INIT)
        return fail(QS_ERR_INVALID, "qs_create: docking-v1 / hovering-v0 reset to their stored initial state; randomise must be 0");
    if (cfg->kind == QS_KIND_HOVERING_V0 && cfg->randomise != 0) return fail(QS_ERR_INVALID, "qs_create: hovering-v0 has no randomised resets");
    if (cfg->integrator != QS_INTEG_FROZEN && cfg->integrator != QS_INTEG_RK4) return fail(QS_ERR_INVALID, "qs_create: unknown integrator %d", cfg->integrator);
    if (cfg->randomise < 0 || cfg->randomise > 2) return fail(QS_ERR_INVALID, "qs_create: randomise must be 0..2");
    if (cfg->io_space != QS_IO_DEVICE && cfg->io_space != QS_IO_HOST) return fail(QS_ERR_INVALID, "qs_create: bad io_space");
    if (cfg->randomise && !(cfg->init_range[2] >= 0.0f && cfg->init_range[2] <= 1.5707964f))
        return fail(QS_ERR_INVALID, "qs_create: init_range[2] (euler half-range) must be within [0, pi/2]");
    if (!(cfg->dt > 0.0f) || !(cfg->mass > 0.0f) || !(cfg->inertia[0] > 0.0f) || !(cfg->inertia[1] > 0.0f) || !(cfg->inertia[2] > 0.0f))
        return fail(QS_ERR_INVALID, "qs_create: dt, mass and inertia must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(QS_ERR_NO_DEVICE, "qs_create: no HIP device visible (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(QS_ERR_INVALID, "qs_create: device %d out of range (%d visible)", cfg->device, ndev);
    DeviceGuard guard(cfg->device);
    if (!guard.ok) return fail(QS_ERR_HIP, "qs_create: hipSetDevice(%d) failed", cfg->device);

    QsEnv *e = new (std::nothrow) QsEnv();
    if (!e) return fail(QS_ERR_NOMEM, "qs_create: out of host memory");
    e->cfg = *cfg;
    e->n = cfg->num_envs;
    e->tiles = tiles_of(e->n);
    e->per_env_params = cfg->randomise >= QS_RANDOMISE_PARAMS;
    e->obs_dim = cfg->kind == QS_KIND_HOVERING_V0 ? 13 : 12;
    auto body = [&]() -> int {
        if (cfg->external_stream) e->stream = (hipStream_t)cfg->stream;
        else { HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)); e->own_stream = true; }
        HIP_TRY(hipEventCreate(&e->ev0));
        HIP_TRY(hipEventCreate(&e->ev1));
        const size_t st_bytes = (size_t)e->tiles * kRecWords * kTile * sizeof(float);
        const size_t par_bytes = (size_t)e->tiles * kParWords * kTile * sizeof(float) + 64;  // + scratch for nominal_obs
        HIP_TRY(hipMalloc((void **)&e->st, st_bytes));
        HIP_TRY(hipMalloc((void **)&e->par, par_bytes));
        HIP_TRY(hipMalloc((void **)&e->d_ctr, (size_t)e->tiles * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(e->d_ctr, 0, (size_t)e->tiles * sizeof(unsigned long long), e->stream));
        HIP_TRY(hipMemsetAsync(e->st, 0, st_bytes, e->stream));
        HIP_TRY(hipMemsetAsync(e->par, 0, par_bytes, e->stream));
        int r = fill_params(e);
        if (r) return r;
        // observation of the nominal reset, evaluated once by the same device code the kernels use
        hipLaunchKernelGGL(k_nominal_obs, dim3(1), dim3(1), 0, e->stream, e->par + (size_t)e->tiles * kParWords * kTile);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(e->nominal_obs, e->par + (size_t)e->tiles * kParWords * kTile, 12 * sizeof(float),
                               hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (cfg->kind == QS_KIND_DOCKING_V1 || cfg->kind == QS_KIND_HOVERING_V0) {
            const bool hover = cfg->kind == QS_KIND_HOVERING_V0;
            HIP_TRY(hipMalloc((void **)&e->init, (size_t)e->n * (hover ? 13 : 26) * sizeof(float)));
            hipLaunchKernelGGL(k_ctor_init, dim3(grid_flat(e->n)), dim3(kBlock), 0, e->stream, e->init, e->n, hover ? 1 : 0,
                               cfg->seed, cfg->env_id_offset);
            HIP_TRY(hipGetLastError());
        }
        if ((r = do_reset(e, nullptr, nullptr, 1))) return r;          // __init__
        HIP_TRY(hipStreamSynchronize(e->stream));
        return QS_OK;
    };
    const int rc = body();
    if (rc != QS_OK) { qs_destroy(e); return rc; }
    *out = e;
    return QS_OK;
}

int qs_destroy(QsEnv *e)
{
    if (!e) return QS_OK;
    DeviceGuard guard(e->cfg.device);
    groups_destroy(e);
    if (e->chain) { (void)chain_drain(e); chain_close(e); }
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->st) (void)hipFree(e->st);
    if (e->par) (void)hipFree(e->par);
    if (e->init) (void)hipFree(e->init);
    if (e->d_ctr) (void)hipFree(e->d_ctr);
    if (e->gae_ws) (void)hipFree(e->gae_ws);
    if (e->plan_ws) (void)hipFree(e->plan_ws);
    if (e->stage.dev) (void)hipFree(e->stage.dev);
    if (e->stage.pin) (void)hipHostFree(e->stage.pin);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return QS_OK;
}

int qs_set_stream(QsEnv *e, void *hip_stream, int32_t external)
{
    CHECK_ENV(e);                                      // drains the private queues
    // a stream-ordered chain leaves `wait until rev == n` commands on the stream it was stepped from; they must have passed
    // before a step is issued from another stream (which would move `rev` past n)
    if (e->chain && e->chain->stream_ordered && e->chain->fwd_seq) HIP_TRY(hipStreamSynchronize(e->stream));
    // an owned stream is drained and destroyed; switching between caller-owned streams is the caller's ordering
    // problem (torch does it for stream capture) and must not synchronise
    if (e->own_stream) { HIP_TRY(hipStreamSynchronize(e->stream)); HIP_TRY(hipStreamDestroy(e->stream)); e->own_stream = false; }
    if (external) e->stream = (hipStream_t)hip_stream;
    else { HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)); e->own_stream = true; }
    return QS_OK;
}

int qs_sync(QsEnv *e)
{
    CHECK_ENV(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QS_OK;
}

int qs_timer_start(QsEnv *e)
{
    CHECK_ENV(e);
    HIP_TRY(hipEventRecord(e->ev0, e->stream));
    return QS_OK;
}

int qs_timer_stop(QsEnv *e, float *ms)
{
    CHECK_ENV(e);
    if (!ms) return fail(QS_ERR_INVALID, "qs_timer_stop: null output");
    HIP_TRY(hipEventRecord(e->ev1, e->stream));
    HIP_TRY(hipEventSynchronize(e->ev1));
    HIP_TRY(hipEventElapsedTime(ms, e->ev0, e->ev1));
    return QS_OK;
}

int qs_get_step_counter(QsEnv *e, uint64_t *k)
{
    if (!k) return fail(QS_ERR_INVALID, "qs_get_step_counter: null argument");
    CHECK_ENV(e);
    unsigned long long v = 0;
    HIP_TRY(hipMemcpyAsync(&v, e->d_ctr, sizeof v, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *k = v;
    return QS_OK;
}

int qs_set_step_counter(QsEnv *e, uint64_t k)
{
    CHECK_ENV(e);
    hipLaunchKernelGGL(k_fill_ctr, dim3(grid_flat(e->tiles)), dim3(kBlock), 0, e->stream, e->d_ctr, e->tiles, (unsigned long long)k);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QS_OK;
}

int qs_reset(QsEnv *e, const uint8_t *mask, float *obs_out)
{
    Range rg_("qs_reset");
    CHECK_ENV(e);
    UserIO io = user_io(e);
    io.in(mask, e->n);
    if (mask) io.inout(obs_out, e->n * e->obs_dim);     // rows of envs that are not reset keep the caller's values
    else io.out(obs_out, e->n * e->obs_dim);
    int r = io.push();
    if (r || (r = do_reset(e, mask, obs_out, 0))) return r;
    return io.pull();
}

int qs_step_ex(QsEnv *e, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags, float *terminal_obs,
               float *terminal_state)
{
    Range rg_("qs_step_ex");
    CHECK_ENV_RAW(e);
    if (!actions || !obs || !reward || !done) return fail(QS_ERR_INVALID, "qs_step: actions, obs, reward and done are required");
    if (terminal_state && e->cfg.kind == QS_KIND_HOVERING_V0)
        return fail(QS_ERR_INVALID, "qs_step_ex: hovering-v0 has no terminal_state (its terminal observation IS the state)");
    if (e->chain) {
        // private-queue mode: one hand-written AQL packet behind the previous step's; nothing of the HIP stream is touched
        if (e->groups_dirty) { int rj = groups_join(e); if (rj) return rj; HIP_TRY(hipStreamSynchronize(e->stream)); }
        StepArgs A = make_args(e);
        A.actions = actions; A.obs = obs; A.reward = reward; A.done = done; A.flags = flags; A.term_obs = terminal_obs;
        A.term_state = terminal_state;
        return chain_step(e, A);
    }
    if (!e->groups.empty()) { int rcj = main_stream_entry(e); if (rcj) return rcj; }
    const int64_t n = e->n, od = e->obs_dim;
    StepArgs A = make_args(e);
    A.actions = actions; A.obs = obs; A.reward = reward; A.done = done; A.flags = flags; A.term_obs = terminal_obs;
    A.term_state = terminal_state;
    UserIO io = user_io(e);
    io.in(A.actions, n * 4);
    io.out(A.obs, n * od); io.out(A.reward, n); io.out(A.done, n); io.out(A.flags, n);
    io.inout(A.term_obs, n * od); io.inout(A.term_state, n * 26);    // rows of envs that did not finish keep the caller's values
    int r = io.push();
    if (r || (r = launch_env(e, A))) return r;
    return io.pull();
}

int qs_step(QsEnv *e, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags, float *terminal_obs)
{
    return qs_step_ex(e, actions, obs, reward, done, flags, terminal_obs, nullptr);
}

// ---- env groups: see the QsGroup comment above ---------------------------------------------------------------------
int qs_set_groups(QsEnv *e, int32_t groups, int32_t launcher_threads)
{
    CHECK_ENV(e);                                     // joins and thereby retires any previous grouping's work
    if (groups < 0 || groups > 64) return fail(QS_ERR_INVALID, "qs_set_groups: groups must be 0..64");
    if (e->cfg.io_space != QS_IO_DEVICE && groups > 1) return fail(QS_ERR_INVALID, "qs_set_groups: device buffers only");
    HIP_TRY(hipStreamSynchronize(e->stream));
    groups_destroy(e);
    if (groups <= 1) return QS_OK;
    if (groups > e->tiles) groups = (int32_t)e->tiles;
    HIP_TRY(hipEventCreateWithFlags(&e->fork_ev, hipEventDisableTiming));
    const int64_t base = e->tiles / groups, rem = e->tiles % groups;
    int64_t t0 = 0;
    try { e->groups.reserve((size_t)groups); }           // no C++ exception may cross the C ABI (push_back below cannot throw now)
    catch (...) { return fail(QS_ERR_NOMEM, "qs_set_groups: out of host memory"); }
    for (int32_t i = 0; i < groups; ++i) {
        QsGroup *g = new (std::nothrow) QsGroup();
        if (!g) return fail(QS_ERR_NOMEM, "qs_set_groups: out of host memory");
        e->groups.push_back(g);
        g->env = e;
        g->index = i;
        g->tile0 = t0;
        g->tile_end = t0 + base + (i < rem ? 1 : 0);
        t0 = g->tile_end;
        g->env0 = g->tile0 * kTile;
        g->env_end = g->tile_end * kTile < e->n ? g->tile_end * kTile : e->n;
        hipError_t he = hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking);
        if (he == hipSuccess) { g->own_stream = true; he = hipEventCreateWithFlags(&g->done_ev, hipEventDisableTiming); }
        if (he != hipSuccess) { groups_destroy(e); return fail(QS_ERR_HIP, "qs_set_groups: %s", hipGetErrorString(he)); }
    }
    for (QsGroup *g : e->groups) {
        g->threaded = launcher_threads != 0;
        if (g->threaded) g->th = std::thread(group_worker, g);
    }
    e->main_dirty = true;
    return QS_OK;
}

int qs_group_count(QsEnv *e, int32_t *groups)
{
    if (!e || !groups) return fail(QS_ERR_INVALID, "qs_group_count: null argument");
    *groups = e->groups.empty() ? 1 : (int32_t)e->groups.size();
    return QS_OK;
}

int qs_group_range(QsEnv *e, int32_t g, int64_t *env_begin, int64_t *env_end)
{
    if (!e || !env_begin || !env_end) return fail(QS_ERR_INVALID, "qs_group_range: null argument");
    if (e->groups.empty()) {
        if (g != 0) return fail(QS_ERR_INVALID, "qs_group_range: group %d out of range", g);
        *env_begin = 0; *env_end = e->n;
        return QS_OK;
    }
    if (g < 0 || g >= (int32_t)e->groups.size()) return fail(QS_ERR_INVALID, "qs_group_range: group %d out of range", g);
    *env_begin = e->groups[g]->env0; *env_end = e->groups[g]->env_end;
    return QS_OK;
}

int qs_group_stream(QsEnv *e, int32_t g, void **hip_stream)
{
    if (!e || !hip_stream) return fail(QS_ERR_INVALID, "qs_group_stream: null argument");
    if (g < 0 || g >= (int32_t)e->groups.size()) return fail(QS_ERR_INVALID, "qs_group_stream: group %d out of range", g);
    *hip_stream = (void *)e->groups[g]->stream;
    return QS_OK;
}

int qs_group_set_stream(QsEnv *e, int32_t g, void *hip_stream)
{
    CHECK_ENV(e);                                     // joins: nothing of this group is pending on its old stream afterwards
    if (g < 0 || g >= (int32_t)e->groups.size()) return fail(QS_ERR_INVALID, "qs_group_set_stream: group %d out of range", g);
    QsGroup *G = e->groups[g];
    HIP_TRY(hipStreamSynchronize(G->stream));
    if (G->own_stream) { HIP_TRY(hipStreamDestroy(G->stream)); G->own_stream = false; }
    G->stream = (hipStream_t)hip_stream;
    return QS_OK;
}

int qs_groups_fork(QsEnv *e)
{
    CHECK_ENV_RAW(e);
    return groups_fork(e);
}

int qs_groups_join(QsEnv *e)
{
    CHECK_ENV_RAW(e);
    return groups_join(e);
}

static int step_group_post(QsEnv *e, QsGroup *G, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags,
                           float *terminal_obs, float *terminal_state, bool group_local)
{
    QsGroup::Req r;
    r.type = QsGroup::REQ_LAUNCH;
    r.ev = nullptr;
    r.A = make_args(e);
    r.A.tile0 = G->tile0; r.A.tile_end = G->tile_end;
    if (group_local) { r.A.io_env0 = G->env0; r.A.io_n = G->env_end - G->env0; }
    r.A.actions = actions; r.A.obs = obs; r.A.reward = reward; r.A.done = done; r.A.flags = flags;
    r.A.term_obs = terminal_obs; r.A.term_state = terminal_state;
    return group_post(G, r);
}

int qs_step_group(QsEnv *e, int32_t g, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags,
                  float *terminal_obs, float *terminal_state)
{
    Range rg_("qs_step_group");
    CHECK_ENV_RAW(e);
    if (g < 0 || g >= (int32_t)e->groups.size()) return fail(QS_ERR_INVALID, "qs_step_group: group %d out of range (qs_set_groups first)", g);
    if (!actions || !obs || !reward || !done) return fail(QS_ERR_INVALID, "qs_step_group: actions, obs, reward and done are required");
    if (terminal_state && e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "qs_step_group: hovering-v0 has no terminal_state");
    if (e->main_dirty) { int rc = groups_fork(e); if (rc) return rc; }
    e->groups_dirty = true;
    int rc = step_group_post(e, e->groups[g], actions, obs, reward, done, flags, terminal_obs, terminal_state, true);
    // with a launcher thread the record is only POSTED here; the contract (quadsim.h) lets the caller enqueue the group's
    // policy on the group's stream right after this call, so the launch has to be on that stream before the call returns
    group_wait_issued(e->groups[g]);
    return rc;
}

int qs_step_groups(QsEnv *e, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags, float *terminal_obs,
                   float *terminal_state)
{
    Range rg_("qs_step_groups");
    CHECK_ENV_RAW(e);
    if (e->groups.empty() || e->chain) return qs_step_ex(e, actions, obs, reward, done, flags, terminal_obs, terminal_state);
    if (!actions || !obs || !reward || !done) return fail(QS_ERR_INVALID, "qs_step_groups: actions, obs, reward and done are required");
    if (terminal_state && e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "qs_step_groups: hovering-v0 has no terminal_state");
    if (e->main_dirty) { int rc = groups_fork(e); if (rc) return rc; }
    e->groups_dirty = true;
    for (QsGroup *G : e->groups) {
        int rc = step_group_post(e, G, actions, obs, reward, done, flags, terminal_obs, terminal_state, false);
        if (rc) return rc;
    }
    // the launcher threads issue the G launches concurrently; all of them are on their streams when the call returns
    for (QsGroup *G : e->groups) group_wait_issued(G);
    return QS_OK;
}

int qs_rollout(QsEnv *e, int64_t T, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags)
{
    Range rg_("qs_rollout");
    CHECK_ENV(e);
    if (T < 1) return fail(QS_ERR_INVALID, "qs_rollout: T must be >= 1");
    if (!obs || !reward || !done) return fail(QS_ERR_INVALID, "qs_rollout: obs, reward and done are required");
    if (!e->cfg.auto_reset) return fail(QS_ERR_INVALID, "qs_rollout: requires auto_reset (a roll-out runs through episode ends)");
    const int64_t tn = T * e->n, od = e->obs_dim;
    StepArgs A = make_args(e);
    A.T = T; A.actions = actions; A.obs = obs; A.reward = reward; A.done = done; A.flags = flags;
    UserIO io = user_io(e);
    io.in(A.actions, tn * 4);
    io.out(A.obs, tn * od); io.out(A.reward, tn); io.out(A.done, tn); io.out(A.flags, tn);
    int r = io.push();
    if (r || (r = launch_env(e, A))) return r;
    return io.pull();
}

int qs_rollout_slab(QsEnv *e, int64_t T, const float *actions, float *slab, uint8_t *flags)
{
    Range rg_("qs_rollout_slab");
    CHECK_ENV(e);
    if (T < 1 || !slab) return fail(QS_ERR_INVALID, "qs_rollout_slab: bad arguments");
    if (!e->cfg.auto_reset) return fail(QS_ERR_INVALID, "qs_rollout_slab: requires auto_reset");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_rollout_slab: device buffers only");
    if (e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "qs_rollout_slab: docking envs only");
    StepArgs A = make_args(e);
    A.T = T; A.actions = actions; A.slab = slab; A.flags = flags;
    return launch_env(e, A);
}

int qs_rollout_stepwise(QsEnv *e, int64_t T, const float *actions, float *obs, float *reward, uint8_t *done, uint8_t *flags)
{
    Range rg_("qs_rollout_stepwise");
    CHECK_ENV_RAW(e);
    if (e->chain) {                                   // as qs_step_ex: packets behind the previous ones, no drain
        if (e->groups_dirty) { int rj = groups_join(e); if (rj) return rj; HIP_TRY(hipStreamSynchronize(e->stream)); }
    } else if (!e->groups.empty()) { int rcj = main_stream_entry(e); if (rcj) return rcj; }
    if (T < 1 || !actions || !obs || !reward || !done) return fail(QS_ERR_INVALID, "qs_rollout_stepwise: bad arguments");
    if (!e->cfg.auto_reset) return fail(QS_ERR_INVALID, "qs_rollout_stepwise: requires auto_reset");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_rollout_stepwise: device buffers only");
    const int64_t n = e->n;
    StepArgs A = make_args(e);
    std::vector<StepArgs> steps;
    if (e->chain) {
        try { steps.reserve((size_t)T); }                // no C++ exception may cross the C ABI
        catch (...) { return fail(QS_ERR_NOMEM, "qs_rollout_stepwise: out of host memory for %lld kernel-argument blocks", (long long)T); }
    }
    for (int64_t t = 0; t < T; ++t) {
        A.actions = actions + t * n * 4;
        A.obs = obs + t * n * e->obs_dim;
        A.reward = reward + t * n;
        A.done = done + t * n;
        A.flags = flags ? flags + t * n : nullptr;
        if (e->chain) { steps.push_back(A); continue; }
        int r = launch_env(e, A);
        if (r) return r;
    }
    // queue mode: T packets per queue behind ONE hand-shake with the handle's stream (stream-ordered chains), or drained by the
    // next entry point (host-ordered chains)
    return e->chain ? chain_submit(e, steps.data(), T) : QS_OK;
}

int qs_fill_random_actions(QsEnv *e, int64_t T, uint64_t step0, float *actions)
{
    CHECK_ENV(e);
    if (T < 1 || !actions) return fail(QS_ERR_INVALID, "qs_fill_random_actions: bad arguments");
    const int64_t tn = T * e->n;
    UserIO io = user_io(e);
    io.out(actions, tn * 4);
    if (int r = io.push()) return r;
    hipLaunchKernelGGL(k_fill_actions, dim3(grid_flat(tn)), dim3(kBlock), 0, e->stream, actions, e->n, T, e->cfg.seed,
                       e->cfg.env_id_offset, step0);
    HIP_TRY(hipGetLastError());
    return io.pull();
}

static int state_io(QsEnv *e, bool to_user, float *chaser, float *target, float *u_prev, float *qdes, float *ls, float *t)
{
    const int64_t n = e->n;
    const int64_t words[6] = {13, 13, 8, 4, 1, 1};
    float *p[6] = {chaser, target, u_prev, qdes, ls, t};
    UserIO io = user_io(e);
    for (int i = 0; i < 6; ++i) {
        if (to_user) io.out(p[i], n * words[i]);
        else io.in(p[i], n * words[i]);
    }
    if (int r = io.push()) return r;
    const StateIO sio{p[0], p[1], p[2], p[3], p[4], p[5]};
    if (to_user) hipLaunchKernelGGL(k_state_io<true>, dim3(grid_tiles(n)), dim3(kBlock), 0, e->stream, e->st, n, sio);
    else hipLaunchKernelGGL(k_state_io<false>, dim3(grid_tiles(n)), dim3(kBlock), 0, e->stream, e->st, n, sio);
    HIP_TRY(hipGetLastError());
    return io.pull();
}

int qs_get_state(QsEnv *e, float *chaser, float *target, float *u_prev, float *qdes, float *last_shaping, float *t)
{
    CHECK_ENV(e);
    return state_io(e, true, chaser, target, u_prev, qdes, last_shaping, t);
}

int qs_set_state(QsEnv *e, const float *chaser, const float *target, const float *u_prev, const float *qdes,
                 const float *last_shaping, const float *t)
{
    CHECK_ENV(e);
    return state_io(e, false, (float *)chaser, (float *)target, (float *)u_prev, (float *)qdes, (float *)last_shaping, (float *)t);
}

static int par_io(QsEnv *e, bool to_user, float *mass, float *inertia)
{
    const int64_t n = e->n;
    UserIO io = user_io(e);
    if (to_user) { io.out(mass, n); io.out(inertia, n * 3); }
    else { io.in(mass, n); io.in(inertia, n * 3); }
    if (int r = io.push()) return r;
    if (to_user) hipLaunchKernelGGL(k_par_io<true>, dim3(grid_tiles(n)), dim3(kBlock), 0, e->stream, e->par, n, mass, inertia);
    else hipLaunchKernelGGL(k_par_io<false>, dim3(grid_tiles(n)), dim3(kBlock), 0, e->stream, e->par, n, mass, inertia);
    HIP_TRY(hipGetLastError());
    return io.pull();
}

int qs_set_params(QsEnv *e, const float *mass, const float *inertia)
{
    CHECK_ENV(e);
    if (!mass && !inertia) return fail(QS_ERR_INVALID, "qs_set_params: nothing to set");
    int r = par_io(e, false, (float *)mass, (float *)inertia);
    if (r) return r;
    e->per_env_params = true;
    return QS_OK;
}

int qs_get_params(QsEnv *e, float *mass, float *inertia)
{
    CHECK_ENV(e);
    return par_io(e, true, mass, inertia);
}

int qs_obs_dim(QsEnv *e, int32_t *dim)
{
    if (!e || !dim) return fail(QS_ERR_INVALID, "qs_obs_dim: null argument");
    *dim = e->obs_dim;
    return QS_OK;
}

static int init_io(QsEnv *e, bool to_user, float *chaser, float *target)
{
    const int64_t n = e->n;
    const bool hover = e->cfg.kind == QS_KIND_HOVERING_V0;
    const int64_t w = hover ? 13 : 26;
    // the store is row-major [n][w]; user arrays are [n][13] each: strided 2-D copies
    const hipMemcpyKind kd = e->cfg.io_space == QS_IO_HOST ? (to_user ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice)
                                                             : hipMemcpyDeviceToDevice;
    if (chaser) {
        if (to_user) HIP_TRY(hipMemcpy2DAsync(chaser, 52, e->init, w * 4, 52, n, kd, e->stream));
        else HIP_TRY(hipMemcpy2DAsync(e->init, w * 4, chaser, 52, 52, n, kd, e->stream));
    }
    if (target && !hover) {
        if (to_user) HIP_TRY(hipMemcpy2DAsync(target, 52, e->init + 13, w * 4, 52, n, kd, e->stream));
        else HIP_TRY(hipMemcpy2DAsync(e->init + 13, w * 4, target, 52, 52, n, kd, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return QS_OK;
}

int qs_set_init_state(QsEnv *e, const float *chaser_init, const float *target_init)
{
    CHECK_ENV(e);
    if (!chaser_init) return fail(QS_ERR_INVALID, "qs_set_init_state: chaser_init is required");
    if (!e->init) {
        // first use on a docking-v0/v2 handle: start from the nominal pair for every env
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMalloc((void **)&e->init, (size_t)e->n * 26 * sizeof(float)));
        hipLaunchKernelGGL(k_fill_init_nominal, dim3(grid_flat(e->n)), dim3(kBlock), 0, e->stream, e->init, e->n);
        HIP_TRY(hipGetLastError());
    }
    return init_io(e, false, (float *)chaser_init, (float *)target_init);
}

int qs_get_init_state(QsEnv *e, float *chaser_init, float *target_init)
{
    CHECK_ENV(e);
    if (!e->init) return fail(QS_ERR_INVALID, "qs_get_init_state: this handle resets to the nominal / randomised state (no stored initial states)");
    return init_io(e, true, chaser_init, target_init);
}

// ---- roll-out post-processing -------------------------------------------
int qs_gae(QsEnv *e, int64_t T, int64_t n, const float *rewards, const float *values, const uint8_t *dones,
           const float *last_values, const uint8_t *last_dones, float gamma, float lam, float *advs, float *returns)
{
    Range rg_("qs_gae");
    CHECK_ENV(e);
    if (T < 1 || n < 1 || !rewards || !values || !dones || !last_values || !last_dones || !advs || !returns)
        return fail(QS_ERR_INVALID, "qs_gae: bad arguments");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_gae: device buffers only");
    GaeArgs G;
    G.rewards = rewards; G.values = values; G.last_values = last_values; G.dones = dones; G.last_dones = last_dones;
    G.advs = advs; G.returns = returns;
    G.T = T; G.N = n; G.C = (T + kGaeChunk - 1) / kGaeChunk;
    G.gamma = gamma; G.lam = lam;
    if (n >= 16384) {
        // wide batch: enough lanes to cover the latency of a T-long serial walk; read everything once
        G.ws = nullptr;
        hipLaunchKernelGGL(k_gae_serial, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, G);
        HIP_TRY(hipGetLastError());
        return QS_OK;
    }
    const size_t need = (size_t)2 * G.C * n;
    if (e->gae_ws_floats < need) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->gae_ws) HIP_TRY(hipFree(e->gae_ws));
        e->gae_ws = nullptr; e->gae_ws_floats = 0;
        HIP_TRY(hipMalloc((void **)&e->gae_ws, need * sizeof(float)));
        e->gae_ws_floats = need;
    }
    G.ws = e->gae_ws;
    dim3 grid((unsigned)((n + 255) / 256), (unsigned)G.C);
    hipLaunchKernelGGL(k_gae_reduce, grid, dim3(256), 0, e->stream, G);
    hipLaunchKernelGGL(k_gae_apply, grid, dim3(256), 0, e->stream, G);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_swap_and_flatten(QsEnv *e, int64_t T, int64_t n, int64_t d, const float *in, float *out)
{
    Range rg_("qs_swap_and_flatten");
    CHECK_ENV(e);
    if (T < 1 || n < 1 || !in || !out) return fail(QS_ERR_INVALID, "qs_swap_and_flatten: bad arguments");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_swap_and_flatten: device buffers only");
    dim3 grid((unsigned)((n + 31) / 32), (unsigned)((T + 31) / 32));
    switch (d) {
        case 1: hipLaunchKernelGGL(k_swap_flatten<1>, grid, dim3(256), 0, e->stream, in, out, T, n); break;
        case 4: hipLaunchKernelGGL(k_swap_flatten_v4<1>, grid, dim3(256), 0, e->stream, (const float4 *)in, (float4 *)out, T, n); break;
        case 12: hipLaunchKernelGGL(k_swap_flatten_v4<3>, grid, dim3(256), 0, e->stream, (const float4 *)in, (float4 *)out, T, n); break;
        case 13: hipLaunchKernelGGL(k_swap_flatten<13>, grid, dim3(256), 0, e->stream, in, out, T, n); break;
        default: return fail(QS_ERR_INVALID, "qs_swap_and_flatten: row width %lld not supported (1, 4, 12, 13)", (long long)d);
    }
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_swap_and_flatten_u8(QsEnv *e, int64_t T, int64_t n, const uint8_t *in, uint8_t *out)
{
    CHECK_ENV(e);
    if (T < 1 || n < 1 || !in || !out) return fail(QS_ERR_INVALID, "qs_swap_and_flatten_u8: bad arguments");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_swap_and_flatten_u8: device buffers only");
    dim3 grid((unsigned)((n + 31) / 32), (unsigned)((T + 31) / 32));
    hipLaunchKernelGGL((k_swap_flatten<1, uint8_t>), grid, dim3(256), 0, e->stream, in, out, T, n);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_gae_flatten(QsEnv *e, int64_t T, int64_t n, const float *rewards, const float *values, const float *neglogp,
                   const uint8_t *dones, const float *last_values, const uint8_t *last_dones, float gamma, float lam,
                   float *flat_returns, float *flat_values, float *flat_neglogp, float *flat_rewards, uint8_t *flat_masks,
                   float *advs, float *returns)
{
    Range rg_("qs_gae_flatten");
    CHECK_ENV(e);
    if (T < 1 || n < 1 || !rewards || !values || !dones || !last_values || !last_dones || !flat_returns || !flat_values ||
        !flat_rewards || !flat_masks)
        return fail(QS_ERR_INVALID, "qs_gae_flatten: bad arguments");
    if ((neglogp == nullptr) != (flat_neglogp == nullptr)) return fail(QS_ERR_INVALID, "qs_gae_flatten: neglogp and flat_neglogp go together");
    if ((advs == nullptr) != (returns == nullptr)) return fail(QS_ERR_INVALID, "qs_gae_flatten: advs and returns go together");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_gae_flatten: device buffers only");
    GaeFlatArgs G;
    G.rewards = rewards; G.values = values; G.neglogp = neglogp; G.last_values = last_values;
    G.dones = dones; G.last_dones = last_dones;
    G.f_returns = flat_returns; G.f_values = flat_values; G.f_neglogp = flat_neglogp; G.f_rewards = flat_rewards;
    G.f_masks = flat_masks; G.advs = advs; G.returns = returns;
    G.T = T; G.N = n; G.gamma = gamma; G.lam = lam;
    hipLaunchKernelGGL(k_gae_flatten, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, G);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_episode_stats(QsEnv *e, int64_t T, int64_t n, const float *rewards, const uint8_t *dones, const uint8_t *last_dones,
                     float *ep_ret, int32_t *ep_len, uint64_t *count, int64_t cap, int64_t *out_key, float *out_ret, int32_t *out_len)
{
    Range rg_("qs_episode_stats");
    CHECK_ENV(e);
    if (T < 1 || n < 1 || cap < 0 || !rewards || !dones || !last_dones || !ep_ret || !ep_len || !count || (cap > 0 && (!out_key || !out_ret || !out_len)))
        return fail(QS_ERR_INVALID, "qs_episode_stats: bad arguments");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_episode_stats: device buffers only");
    EpisodeArgs E;
    E.rewards = rewards; E.dones = dones; E.last_dones = last_dones; E.ep_ret = ep_ret; E.ep_len = ep_len;
    E.count = (unsigned long long *)count; E.out_key = out_key; E.out_ret = out_ret; E.out_len = out_len;
    E.T = T; E.N = n; E.cap = cap;
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint64_t), e->stream));
    hipLaunchKernelGGL(k_episode_stats, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, E);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

// The weights of a qs_policy_* call are M (exact f32: six arrays) or else blob (the packed split-bf16 image); the static helpers
// below take both, check the one that is given first of all, and launch its kernel.
static int check_mlp_args(const char *who, const MlpArgs &M)
{
    if (!M.wt1 || !M.b1 || !M.wt2 || !M.b2 || !M.wt3 || !M.b3) return fail(QS_ERR_INVALID, "%s: null weight pointer", who);
    if ((((uintptr_t)M.wt2) | ((uintptr_t)M.wt3)) & 15u) return fail(QS_ERR_INVALID, "%s: wt2 and wt3 must be 16-byte aligned", who);
    return QS_OK;
}

static int check_blob(const char *who, const void *blob)
{
    if (!blob) return fail(QS_ERR_INVALID, "%s: null packed_weights", who);
    if (((uintptr_t)blob & 15) != 0) return fail(QS_ERR_INVALID, "%s: packed weights must be 16-byte aligned", who);
    return QS_OK;
}

// the handles qs_policy_rollout* takes, and the one choice of its kernel: f.operator()<INTEG, RMODE, FAST>() for the launch and
// for qs_debug_rollout_variant
static int policy_rollout_handle_ok(const QsEnv *e, const char *who)
{
    if (e->cfg.kind == QS_KIND_HOVERING_V0 || e->per_env_params || e->init || e->cfg.randomise > 1)
        return fail(QS_ERR_INVALID, "%s: docking-v0/v2 with nominal or rocRAND-initialised resets only", who);
    return QS_OK;
}

extern "C++" template <class F>
static void with_policy_rollout_kernel(const QsEnv *e, bool fast, F &&f)
{
    with_combo(step_combo(e), [&]<int INTEG, bool PARAMS, int RMODE>() {     // policy_rollout_handle_ok leaves RMODE 0 / 1 without PARAMS
        if constexpr (!PARAMS && RMODE < 2) {
            if (fast) f.template operator()<INTEG, RMODE, true>();
            else f.template operator()<INTEG, RMODE, false>();
        }
    });
}

static int policy_rollout(QsEnv *e, const char *who, int64_t T, const MlpArgs *M, const void *blob, float *obs, float *reward,
                          uint8_t *done, uint8_t *flags, float *actions)
{
    Range rg_(who);
    if (int rc = M ? check_mlp_args(who, *M) : check_blob(who, blob)) return rc;
    if (T < 1 || !obs || !reward || !done) return fail(QS_ERR_INVALID, "%s: bad arguments", who);
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "%s: device buffers only", who);
    if (!e->cfg.auto_reset) return fail(QS_ERR_INVALID, "%s: requires auto_reset", who);
    if (int rc = policy_rollout_handle_ok(e, who)) return rc;
    StepArgs A = make_args(e);
    A.T = T; A.obs = obs; A.reward = reward; A.done = done; A.flags = flags;
    const unsigned grid = grid_tiles(e->n);
    with_policy_rollout_kernel(e, blob != nullptr, [&]<int INTEG, int RMODE, bool FAST>() {
        if constexpr (FAST) hipLaunchKernelGGL((k_policy_rollout_fast<INTEG, RMODE>), dim3(grid), dim3(kBlock), 0, e->stream, A, (const uint4 *)blob, actions);
        else hipLaunchKernelGGL((k_policy_rollout<INTEG, RMODE>), dim3(grid), dim3(kBlock), 0, e->stream, A, *M, actions);
    });
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_policy_rollout(QsEnv *e, int64_t T, const float *wt1, const float *b1, const float *wt2, const float *b2,
                      const float *wt3, const float *b3, float *obs, float *reward, uint8_t *done, uint8_t *flags, float *actions)
{
    CHECK_ENV(e);
    const MlpArgs M{wt1, b1, wt2, b2, wt3, b3};
    return policy_rollout(e, "qs_policy_rollout", T, &M, nullptr, obs, reward, done, flags, actions);
}

int qs_policy_rollout_fast(QsEnv *e, int64_t T, const void *packed_weights, float *obs, float *reward, uint8_t *done,
                           uint8_t *flags, float *actions)
{
    CHECK_ENV(e);
    return policy_rollout(e, "qs_policy_rollout_fast", T, nullptr, packed_weights, obs, reward, done, flags, actions);
}

static int policy_forward(QsEnv *e, const char *who, int64_t n, const MlpArgs *M, const void *blob, const float *obs, float *actions)
{
    Range rg_(who);
    if (int rc = M ? check_mlp_args(who, *M) : check_blob(who, blob)) return rc;
    if (n < 1 || !obs || !actions) return fail(QS_ERR_INVALID, "%s: bad arguments", who);
    if ((((uintptr_t)obs) | ((uintptr_t)actions)) & 15u) return fail(QS_ERR_INVALID, "%s: obs and actions must be 16-byte aligned", who);
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "%s: device buffers only", who);
    if (blob) hipLaunchKernelGGL(k_policy_forward_fast, dim3(grid_tiles(n)), dim3(kBlock), 0, e->stream, (const uint4 *)blob, obs, actions, n);
    else hipLaunchKernelGGL(k_policy_forward, dim3(grid_tiles(n)), dim3(kBlock), 0, e->stream, *M, obs, actions, n);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_policy_forward(QsEnv *e, int64_t n, const float *wt1, const float *b1, const float *wt2, const float *b2, const float *wt3,
                      const float *b3, const float *obs, float *actions)
{
    CHECK_ENV(e);
    const MlpArgs M{wt1, b1, wt2, b2, wt3, b3};
    return policy_forward(e, "qs_policy_forward", n, &M, nullptr, obs, actions);
}

int qs_policy_forward_fast(QsEnv *e, int64_t n, const void *packed_weights, const float *obs, float *actions)
{
    CHECK_ENV(e);
    return policy_forward(e, "qs_policy_forward_fast", n, nullptr, packed_weights, obs, actions);
}

int qs_policy_rollout_fast_blob_bytes(void) { return kFastBlobBytes; }

static int policy_evaluate(QsEnv *e, const char *who, int32_t episodes, int64_t max_steps, const MlpArgs *M, const void *blob,
                           double *ep_return, int32_t *ep_length, uint8_t *ep_flags, int32_t *ep_docked, int32_t *finished)
{
    Range rg_(who);
    if (int rc = M ? check_mlp_args(who, *M) : check_blob(who, blob)) return rc;
    if (episodes < 1) return fail(QS_ERR_INVALID, "%s: episodes must be >= 1", who);
    if (max_steps < 1) return fail(QS_ERR_INVALID, "%s: max_steps must be >= 1", who);
    if (!ep_return || !ep_length || !finished) return fail(QS_ERR_INVALID, "%s: ep_return, ep_length and finished are required", who);
    if (e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "%s: docking envs only (hovering-v0 has a 13-d observation)", who);
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "%s: device buffers only", who);
    if (!e->cfg.auto_reset) return fail(QS_ERR_INVALID, "%s: requires auto_reset (episodes follow each other as in the step API)", who);
    if ((((uintptr_t)ep_return) & 7u) || ((((uintptr_t)ep_length) | ((uintptr_t)ep_docked) | ((uintptr_t)finished)) & 3u))
        return fail(QS_ERR_INVALID, "%s: ep_return must be 8-byte aligned, ep_length, ep_docked and finished 4-byte aligned", who);
    StepArgs A = make_args(e);
    EvalArgs E{ep_return, ep_length, ep_flags, ep_docked, finished, max_steps, episodes};
    const unsigned grid = grid_tiles(e->n);
    with_combo(step_combo(e), [&]<int INTEG, bool PARAMS, int RMODE>() {     // as launch_env_on
        if (blob) hipLaunchKernelGGL((k_policy_evaluate_fast<INTEG, PARAMS, RMODE>), dim3(grid), dim3(kBlock), 0, e->stream, A, (const uint4 *)blob, E);
        else hipLaunchKernelGGL((k_policy_evaluate<INTEG, PARAMS, RMODE>), dim3(grid), dim3(kBlock), 0, e->stream, A, *M, E);
    });
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_policy_evaluate(QsEnv *e, int32_t episodes, int64_t max_steps, const float *wt1, const float *b1, const float *wt2,
                       const float *b2, const float *wt3, const float *b3, double *ep_return, int32_t *ep_length,
                       uint8_t *ep_flags, int32_t *ep_docked, int32_t *finished)
{
    CHECK_ENV(e);
    const MlpArgs M{wt1, b1, wt2, b2, wt3, b3};
    return policy_evaluate(e, "qs_policy_evaluate", episodes, max_steps, &M, nullptr, ep_return, ep_length, ep_flags, ep_docked, finished);
}

int qs_policy_evaluate_fast(QsEnv *e, int32_t episodes, int64_t max_steps, const void *packed_weights, double *ep_return,
                            int32_t *ep_length, uint8_t *ep_flags, int32_t *ep_docked, int32_t *finished)
{
    CHECK_ENV(e);
    return policy_evaluate(e, "qs_policy_evaluate_fast", episodes, max_steps, nullptr, packed_weights, ep_return, ep_length, ep_flags,
                           ep_docked, finished);
}

// 1: the one-wave-per-tile Runner kernels, 0: the role-split ones (default; QUADSIM_RUNNER_SERIAL=1 or the diagnostic entry
// below select the former for A/B runs and for the bit-identity test)
static std::atomic<int> &runner_serial_flag()
{
    static std::atomic<int> flag{[] { const char *v = getenv("QUADSIM_RUNNER_SERIAL"); return (v && v[0] == '1') ? 1 : 0; }()};
    return flag;
}

extern "C++" template <int NET>
static void runner_dispatch(QsEnv *e, const StepArgs &A, const RunnerArgs &R, bool fast);

// the handles qs_runner_rollout* takes, and the one choice of its kernel: f.operator()<SERIAL, INTEG, RMODE, PARAMS, FAST>()
// (SERIAL: k_runner_rollout, else k_runner_split) for the launch and for qs_debug_rollout_variant
static int runner_handle_ok(const QsEnv *e, const char *who)
{
    if (e->cfg.kind == QS_KIND_HOVERING_V0 || e->init)
        return fail(QS_ERR_INVALID, "%s: docking-v0/v2 with nominal or rocRAND resets only (no stored initial states)", who);
    return QS_OK;
}

extern "C++" template <class F>
static void with_runner_kernel(const QsEnv *e, bool fast, F &&f)
{
    // the role-split kernel (matrix waves + env waves); QUADSIM_RUNNER_SERIAL=1 keeps the one-wave-per-tile kernel for A/B
    // runs (same results bit for bit: the same instruction sequences on the same operands)
    const bool serial = runner_serial_flag().load(std::memory_order_relaxed) != 0;
    with_combo(step_combo(e), [&]<int INTEG, bool PARAMS, int RMODE>() {
        if constexpr (RMODE != 3) {           // runner_handle_ok rejects stored initial states
            auto go = [&]<bool FAST>() {
                if (serial) f.template operator()<true, INTEG, RMODE, PARAMS, FAST>();
                else f.template operator()<false, INTEG, RMODE, PARAMS, FAST>();
            };
            if (fast) go.template operator()<true>();
            else go.template operator()<false>();
        }
    });
}

// layout: QS_NET_SHARED_TRUNK / QS_NET_TOWERS; wtv1 / bv1: the towers' vf_fc0 (exact f32 only)
static int runner_launch(QsEnv *e, const char *who, int64_t T, const float logstd[4], int squash, const AcArgs *net,
                         const void *blob, const float *noise, const uint8_t *dones_in, float *mb_obs, float *mb_actions,
                         float *mb_values, float *mb_neglogp, uint8_t *mb_dones, float *mb_rewards, uint8_t *mb_flags,
                         float *last_obs, float *last_values, uint8_t *last_dones, int layout = QS_NET_SHARED_TRUNK,
                         const float *wtv1 = nullptr, const float *bv1 = nullptr)
{
    Range rg_(who);
    if (T < 1 || !mb_obs || !mb_actions || !mb_values || !mb_neglogp || !mb_dones || !mb_rewards || !last_values || !last_dones)
        return fail(QS_ERR_INVALID, "%s: bad arguments", who);
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "%s: device buffers only", who);
    if (!e->cfg.auto_reset) return fail(QS_ERR_INVALID, "%s: requires auto_reset", who);
    if (int rc = runner_handle_ok(e, who)) return rc;
    StepArgs A = make_args(e);
    A.T = T; A.obs = mb_obs; A.reward = mb_rewards; A.done = mb_dones; A.flags = mb_flags;
    RunnerArgs R{};
    if (net) R.net = *net;
    R.blob = (const uint4 *)blob;
    double ls = 0.0;
    for (int i = 0; i < 4; ++i) {
        if (!(logstd[i] == logstd[i])) return fail(QS_ERR_INVALID, "%s: logstd is NaN", who);
        R.std[i] = expf(logstd[i]);
        R.inv_std[i] = 1.0f / R.std[i];
        ls += (double)logstd[i];
    }
    R.nl_const = (float)(0.5 * 1.8378770664093453 * 4.0 + ls);      // 0.5 log(2 pi) d + sum logstd
    R.squash = squash;
    R.noise = noise; R.dones_in = dones_in;
    R.actions = mb_actions; R.values = mb_values; R.neglogp = mb_neglogp;
    R.last_obs = last_obs; R.last_values = last_values; R.last_dones = last_dones;
    R.env_major = e->runner_env_major ? 1 : 0;
    R.wtv1 = wtv1; R.bv1 = bv1;
    if (layout == QS_NET_TOWERS) runner_dispatch<kNetTowers>(e, A, R, blob != nullptr);
    else runner_dispatch<kNetShared>(e, A, R, blob != nullptr);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

extern "C++" template <int NET>
static void runner_dispatch(QsEnv *e, const StepArgs &A, const RunnerArgs &R, bool fast)
{
    const unsigned grid = grid_tiles(e->n);
    with_runner_kernel(e, fast, [&]<bool SERIAL, int INTEG, int RMODE, bool PARAMS, bool FAST>() {
        if constexpr (SERIAL) hipLaunchKernelGGL((k_runner_rollout<INTEG, RMODE, PARAMS, FAST, NET>), dim3(grid), dim3(kBlock), 0, e->stream, A, R);
        else hipLaunchKernelGGL((k_runner_split<INTEG, RMODE, PARAMS, FAST, NET>), dim3(grid), dim3(2 * kBlock), 0, e->stream, A, R);
    });
}

int qs_runner_rollout(QsEnv *e, int64_t T, const QsActorCritic *pol, const float *noise, const uint8_t *dones_in,
                      float *mb_obs, float *mb_actions, float *mb_values, float *mb_neglogp, uint8_t *mb_dones,
                      float *mb_rewards, uint8_t *mb_flags, float *last_obs, float *last_values, uint8_t *last_dones)
{
    CHECK_ENV(e);
    if (!pol) return fail(QS_ERR_INVALID, "qs_runner_rollout: bad arguments");
    if (pol->struct_size != sizeof(QsActorCritic)) return fail(QS_ERR_INVALID, "qs_runner_rollout: QsActorCritic.struct_size mismatch");
    if (!pol->wt1 || !pol->b1 || !pol->wt2 || !pol->b2 || !pol->wt3 || !pol->b3 || !pol->wtv2 || !pol->bv2 || !pol->wtv3 || !pol->bv3)
        return fail(QS_ERR_INVALID, "qs_runner_rollout: null weight pointer");
    const AcArgs net{pol->wt1, pol->b1, pol->wt2, pol->b2, pol->wt3, pol->b3, pol->wtv2, pol->bv2, pol->wtv3, pol->bv3};
    return runner_launch(e, "qs_runner_rollout", T, pol->logstd, pol->squash, &net, nullptr, noise, dones_in, mb_obs, mb_actions,
                         mb_values, mb_neglogp, mb_dones, mb_rewards, mb_flags, last_obs, last_values, last_dones);
}

int qs_runner_rollout_fast(QsEnv *e, int64_t T, const void *packed_weights, const float *logstd, int squash, const float *noise,
                           const uint8_t *dones_in, float *mb_obs, float *mb_actions, float *mb_values, float *mb_neglogp,
                           uint8_t *mb_dones, float *mb_rewards, uint8_t *mb_flags, float *last_obs, float *last_values,
                           uint8_t *last_dones)
{
    CHECK_ENV(e);
    if (!packed_weights || !logstd) return fail(QS_ERR_INVALID, "qs_runner_rollout_fast: bad arguments");
    if (((uintptr_t)packed_weights & 15) != 0) return fail(QS_ERR_INVALID, "qs_runner_rollout_fast: packed weights must be 16-byte aligned");
    return runner_launch(e, "qs_runner_rollout_fast", T, logstd, squash, nullptr, packed_weights, noise, dones_in, mb_obs,
                         mb_actions, mb_values, mb_neglogp, mb_dones, mb_rewards, mb_flags, last_obs, last_values, last_dones);
}

int qs_runner_rollout_fast_blob_bytes(void) { return kAcFastBlobBytes; }

int qs_runner_rollout_net(QsEnv *e, int64_t T, const QsActorCriticNet *pol, const float *noise, const uint8_t *dones_in,
                          float *mb_obs, float *mb_actions, float *mb_values, float *mb_neglogp, uint8_t *mb_dones,
                          float *mb_rewards, uint8_t *mb_flags, float *last_obs, float *last_values, uint8_t *last_dones)
{
    CHECK_ENV(e);
    if (!pol) return fail(QS_ERR_INVALID, "qs_runner_rollout_net: bad arguments");
    if (pol->struct_size != sizeof(QsActorCriticNet)) return fail(QS_ERR_INVALID, "qs_runner_rollout_net: QsActorCriticNet.struct_size mismatch");
    if (pol->layout != QS_NET_SHARED_TRUNK && pol->layout != QS_NET_TOWERS)
        return fail(QS_ERR_INVALID, "qs_runner_rollout_net: layout must be QS_NET_SHARED_TRUNK or QS_NET_TOWERS");
    const bool tow = pol->layout == QS_NET_TOWERS;
    if (!pol->wt1 || !pol->b1 || !pol->wt2 || !pol->b2 || !pol->wt3 || !pol->b3 || !pol->wtv2 || !pol->bv2 || !pol->wtv3 || !pol->bv3
        || (tow && (!pol->wtv1 || !pol->bv1)))
        return fail(QS_ERR_INVALID, "qs_runner_rollout_net: null weight pointer");
    const AcArgs net{pol->wt1, pol->b1, pol->wt2, pol->b2, pol->wt3, pol->b3, pol->wtv2, pol->bv2, pol->wtv3, pol->bv3};
    return runner_launch(e, "qs_runner_rollout_net", T, pol->logstd, pol->squash, &net, nullptr, noise, dones_in, mb_obs, mb_actions,
                         mb_values, mb_neglogp, mb_dones, mb_rewards, mb_flags, last_obs, last_values, last_dones, pol->layout,
                         tow ? pol->wtv1 : nullptr, tow ? pol->bv1 : nullptr);
}

int qs_runner_rollout_net_fast(QsEnv *e, int64_t T, int32_t layout, const void *packed_weights, const float *logstd, int squash,
                               const float *noise, const uint8_t *dones_in, float *mb_obs, float *mb_actions, float *mb_values,
                               float *mb_neglogp, uint8_t *mb_dones, float *mb_rewards, uint8_t *mb_flags, float *last_obs,
                               float *last_values, uint8_t *last_dones)
{
    CHECK_ENV(e);
    if (layout != QS_NET_SHARED_TRUNK && layout != QS_NET_TOWERS)
        return fail(QS_ERR_INVALID, "qs_runner_rollout_net_fast: layout must be QS_NET_SHARED_TRUNK or QS_NET_TOWERS");
    if (!packed_weights || !logstd) return fail(QS_ERR_INVALID, "qs_runner_rollout_net_fast: bad arguments");
    if (((uintptr_t)packed_weights & 15) != 0) return fail(QS_ERR_INVALID, "qs_runner_rollout_net_fast: packed weights must be 16-byte aligned");
    return runner_launch(e, "qs_runner_rollout_net_fast", T, logstd, squash, nullptr, packed_weights, noise, dones_in, mb_obs,
                         mb_actions, mb_values, mb_neglogp, mb_dones, mb_rewards, mb_flags, last_obs, last_values, last_dones, layout);
}

int qs_runner_rollout_net_fast_blob_bytes(int32_t layout)
{
    if (layout == QS_NET_SHARED_TRUNK) return kAcFastBlobBytes;
    if (layout == QS_NET_TOWERS) return kAcTowFastBlobBytes;
    return fail(QS_ERR_INVALID, "qs_runner_rollout_net_fast_blob_bytes: unknown layout %d", (int)layout);
}

// Diagnostic (not in quadsim.h; tests and A/B tools only): Runner kernel flavour for every later qs_runner_rollout* call of
// the process -- 1 one wave per tile, 0 role-split (matrix waves + env waves).  Returns the previous setting.
int qs_debug_set_runner_serial(int on) { return runner_serial_flag().exchange(on ? 1 : 0); }

int qs_set_queue_mode(QsEnv *e, int32_t mode)
{
    CHECK_ENV(e);                                     // drains a queue that is being switched off
    if (mode < QS_QUEUE_HIP_STREAM || mode > 4) return fail(QS_ERR_INVALID, "qs_set_queue_mode: mode must be 0 (HIP stream) or 1..4 private queues");
    if (e->chain && e->chain->requested == mode) return QS_OK;
    chain_close(e);
    if (mode == QS_QUEUE_HIP_STREAM) return QS_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    int rc = chain_open(e, mode);
    if (rc == QS_OK) e->chain->requested = mode;
    return rc;
}

// Diagnostic (not in quadsim.h; tests only): pretend every tile is held by an XCD that does not exist, so that the placement
// check of the next private-queue step fires in every workgroup
int qs_debug_chain_poison_owner(QsEnv *e)
{
    if (!e || !e->chain) return fail(QS_ERR_INVALID, "qs_debug_chain_poison_owner: not in private-queue mode");
    DeviceGuard guard(e->cfg.device);
    int rc = chain_drain(e);
    if (rc) return rc;
    HIP_TRY(hipMemset(e->chain->d_owner, 9, (size_t)e->tiles * sizeof(unsigned)));
    e->chain->hip_dirty = false;          // keep the poisoned owners: the next step must not reset them
    e->chain->res_dbg_packets = true;     // ... and is a packet of the guarded chain, as are the steps up to the next drain
    return QS_OK;
}

// Diagnostic (not in quadsim.h; tests and A/B tools only): force the reset-preparation variant of the role-split step kernel for
// every later launch of the process: 0 two waves, 2 three waves, -1 the default choice by tiles per launch.  Returns the previous
// setting.  (Same results bit for bit: tests/test_gpu_groups_and_rollout.py::test_reset_preparation_wave_is_bit_identical.)
int qs_debug_set_reset_prep(int mode) { return prep_forced().exchange((mode == 0 || mode == 2) ? mode : -1); }

// Diagnostic (not in quadsim.h; tests only): the NEXT private-queue step runs with workgroup b stepping tile b + shift of its
// launch -- every tile on another XCD than the one that holds its state -- without any synchronisation in between: the
// placement guard must see the owner words the previous step wrote from the other XCDs.
int qs_debug_chain_shift_once(QsEnv *e, int32_t shift)
{
    if (!e || !e->chain) return fail(QS_ERR_INVALID, "qs_debug_chain_shift_once: not in private-queue mode");
    e->chain->dbg_shift = shift;
    e->chain->res_dbg_packets = true;     // this step and the ones up to the next drain: packets of the guarded chain
    return QS_OK;
}

// Diagnostic (not in quadsim.h; tests and A/B tools only): resident step-kernel dispatches the handle's private queues have
// issued so far (relaunches after the idle limit included); 0 outside private-queue mode
int qs_debug_chain_resident(QsEnv *e, uint64_t *dispatches)
{
    if (!e || !dispatches) return fail(QS_ERR_INVALID, "qs_debug_chain_resident: null argument");
    *dispatches = e->chain ? e->chain->res_dispatches : 0;
    return QS_OK;
}

// Diagnostic (not in quadsim.h; tests only): the step-kernel instantiation the handle's next qs_step launch takes, as
// {family, INTEG, PARAMS, RMODE, PREP} -- family 0 k_env, 1 k_env_split, 2 k_env_resident, 3 / 4 k_env_split / k_env as packets
// of the private queues, 5 k_hover; -1 for a template parameter the family does not have.  Computed by the helpers the launch
// paths call (step_variant, chain_resident_fits).  HIP-stream mode reports the whole-handle launch: a group launch of fewer
// tiles (qs_set_groups) may take PREP 2 where this says 0.
int qs_debug_step_variant(QsEnv *e, int32_t out[5])
{
    if (!e || !out) return fail(QS_ERR_INVALID, "qs_debug_step_variant: null argument");
    DeviceGuard guard(e->cfg.device);
    if (!guard.ok) return fail(QS_ERR_HIP, "qs_debug_step_variant: hipSetDevice(%d) failed", e->cfg.device);
    StepVariant v = step_variant(e, e->tiles);
    if (e->chain) { int rc = chain_step_variant(e, &v); if (rc) return rc; }
    const int32_t w[5] = {v.family, v.integ, v.params, v.rmode, v.prep};
    memcpy(out, w, sizeof w);
    return QS_OK;
}

// Diagnostic (not in quadsim.h; tests only): the roll-out kernel instantiation a call on the handle would launch, without launching
// anything.  family 0: qs_runner_rollout* (fast: the *_fast entry points; layout: QS_NET_SHARED_TRUNK / QS_NET_TOWERS), family 1:
// qs_policy_rollout / _fast (layout ignored).  out = {kernel, INTEG, RMODE, PARAMS, FAST, NET}: kernel 0 k_runner_rollout,
// 1 k_runner_split, 2 k_policy_rollout, 3 k_policy_rollout_fast; -1 for a template parameter the kernel does not have.  Computed
// by the helpers the launches call (runner_handle_ok + with_runner_kernel, policy_rollout_handle_ok + with_policy_rollout_kernel):
// a handle those entry points refuse is refused here with the same message.
int qs_debug_rollout_variant(QsEnv *e, int32_t family, int32_t fast, int32_t layout, int32_t out[6])
{
    if (!e || !out) return fail(QS_ERR_INVALID, "qs_debug_rollout_variant: null argument");
    int32_t w[6] = {-1, -1, -1, -1, -1, -1};
    if (family == 0) {
        if (layout != QS_NET_SHARED_TRUNK && layout != QS_NET_TOWERS)
            return fail(QS_ERR_INVALID, "qs_debug_rollout_variant: layout must be QS_NET_SHARED_TRUNK or QS_NET_TOWERS");
        if (int rc = runner_handle_ok(e, "qs_debug_rollout_variant")) return rc;
        with_runner_kernel(e, fast != 0, [&]<bool SERIAL, int INTEG, int RMODE, bool PARAMS, bool FAST>() {
            const int32_t v[6] = {SERIAL ? 0 : 1, INTEG, RMODE, PARAMS ? 1 : 0, FAST ? 1 : 0, layout == QS_NET_TOWERS ? kNetTowers : kNetShared};
            memcpy(w, v, sizeof v);
        });
    } else if (family == 1) {
        if (int rc = policy_rollout_handle_ok(e, "qs_debug_rollout_variant")) return rc;
        with_policy_rollout_kernel(e, fast != 0, [&]<int INTEG, int RMODE, bool FAST>() {
            const int32_t v[6] = {FAST ? 3 : 2, INTEG, RMODE, -1, -1, -1};
            memcpy(w, v, sizeof v);
        });
    } else return fail(QS_ERR_INVALID, "qs_debug_rollout_variant: family must be 0 (Runner) or 1 (policy roll-out)");
    memcpy(out, w, sizeof w);
    return QS_OK;
}

int qs_get_queue_ordering(QsEnv *e, int32_t *ordering)
{
    if (!e || !ordering) return fail(QS_ERR_INVALID, "qs_get_queue_ordering: null argument");
    *ordering = (e->chain && e->chain->stream_ordered) ? QS_ORDER_STREAM : QS_ORDER_HOST;
    return QS_OK;
}

int qs_set_queue_ordering(QsEnv *e, int32_t ordering)
{
    CHECK_ENV(e);                                     // drains the queues
    if (!e->chain) return fail(QS_ERR_INVALID, "qs_set_queue_ordering: qs_set_queue_mode first");
    if (ordering != QS_ORDER_HOST && ordering != QS_ORDER_STREAM) return fail(QS_ERR_INVALID, "qs_set_queue_ordering: unknown ordering %d", ordering);
    QsChain *c = e->chain;
    if (c->stream_ordered && c->fwd_seq) HIP_TRY(hipStreamSynchronize(e->stream));   // pending hand-shake waits
    if (ordering == QS_ORDER_HOST) { c->stream_ordered = false; return QS_OK; }
    if (!chain_can_stream_order(e))
        return fail(QS_ERR_INVALID, "qs_set_queue_ordering: this device / HIP runtime has no stream memory operations (hipStreamWaitValue64)");
    return chain_enable_stream_order(e);
}

int qs_get_queue_mode(QsEnv *e, int32_t *mode)
{
    if (!e || !mode) return fail(QS_ERR_INVALID, "qs_get_queue_mode: null argument");
    *mode = e->chain ? (int32_t)e->chain->lanes.size() : QS_QUEUE_HIP_STREAM;
    return QS_OK;
}

int qs_set_rollout_layout(QsEnv *e, int32_t layout)
{
    CHECK_ENV(e);
    if (layout != QS_LAYOUT_TIME_MAJOR && layout != QS_LAYOUT_ENV_MAJOR) return fail(QS_ERR_INVALID, "qs_set_rollout_layout: unknown layout %d", layout);
    e->runner_env_major = layout == QS_LAYOUT_ENV_MAJOR;
    return QS_OK;
}

int qs_expert_action(QsEnv *e, float *state_des, float kp, float kd, float *actions)
{
    CHECK_ENV(e);
    if (!state_des || !actions) return fail(QS_ERR_INVALID, "qs_expert_action: null argument");
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "qs_expert_action: device buffers only");
    if (e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "qs_expert_action: docking envs only");
    Par pn{e->cfg.mass, e->cfg.inertia[0], e->cfg.inertia[1], e->cfg.inertia[2]};
    if (e->per_env_params)
        hipLaunchKernelGGL(k_expert_action<true>, dim3(grid_tiles(e->n)), dim3(kBlock), 0, e->stream, e->st, e->par, e->n, state_des, kp, kd, pn, actions);
    else
        hipLaunchKernelGGL(k_expert_action<false>, dim3(grid_tiles(e->n)), dim3(kBlock), 0, e->stream, e->st, e->par, e->n, state_des, kp, kd, pn, actions);
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

// what both fused expert entry points refuse (the step API's other configurations are all taken)
static int expert_fused_checks(const QsEnv *e, const char *who)
{
    if (e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "%s: docking envs only (the reference has no expert for hovering-v0)", who);
    if (e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "%s: device buffers only", who);
    if (!e->cfg.auto_reset) return fail(QS_ERR_INVALID, "%s: requires auto_reset (episodes follow each other as in the step API)", who);
    return QS_OK;
}

int qs_expert_rollout(QsEnv *e, int64_t T, float *state_des, float kp, float kd, float *obs, float *actions, float *reward,
                      uint8_t *done, uint8_t *flags, float *last_obs)
{
    CHECK_ENV(e);
    Range rg_("qs_expert_rollout");
    if (T < 1) return fail(QS_ERR_INVALID, "qs_expert_rollout: T must be >= 1");
    if (!state_des || !obs || !actions || !reward || !done)
        return fail(QS_ERR_INVALID, "qs_expert_rollout: state_des, obs, actions, reward and done are required");
    if (int rc = expert_fused_checks(e, "qs_expert_rollout")) return rc;
    if ((((uintptr_t)obs) | ((uintptr_t)actions) | ((uintptr_t)last_obs)) & 15u)
        return fail(QS_ERR_INVALID, "qs_expert_rollout: obs, actions and last_obs must be 16-byte aligned");
    StepArgs A = make_args(e);
    A.T = T; A.obs = obs; A.reward = reward; A.done = done; A.flags = flags;
    const ExpertArgs X{state_des, kp, kd, actions, last_obs, e->runner_env_major ? 1 : 0};
    const unsigned grid = grid_tiles(e->n);
    with_combo(step_combo(e), [&]<int INTEG, bool PARAMS, int RMODE>() {     // as launch_env_on
        hipLaunchKernelGGL((k_expert_rollout<INTEG, PARAMS, RMODE>), dim3(grid), dim3(kBlock), 0, e->stream, A, X);
    });
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

int qs_expert_evaluate(QsEnv *e, int32_t episodes, int64_t max_steps, const float *state_des, float kp, float kd,
                       double *ep_return, int32_t *ep_length, uint8_t *ep_flags, int32_t *ep_docked, int32_t *finished)
{
    CHECK_ENV(e);
    Range rg_("qs_expert_evaluate");
    if (episodes < 1) return fail(QS_ERR_INVALID, "qs_expert_evaluate: episodes must be >= 1");
    if (max_steps < 1) return fail(QS_ERR_INVALID, "qs_expert_evaluate: max_steps must be >= 1");
    if (!state_des || !ep_return || !ep_length || !finished)
        return fail(QS_ERR_INVALID, "qs_expert_evaluate: state_des, ep_return, ep_length and finished are required");
    if (int rc = expert_fused_checks(e, "qs_expert_evaluate")) return rc;
    if ((((uintptr_t)ep_return) & 7u) || ((((uintptr_t)ep_length) | ((uintptr_t)ep_docked) | ((uintptr_t)finished)) & 3u))
        return fail(QS_ERR_INVALID, "qs_expert_evaluate: ep_return must be 8-byte aligned, ep_length, ep_docked and finished 4-byte aligned");
    const StepArgs A = make_args(e);
    const EvalArgs E{ep_return, ep_length, ep_flags, ep_docked, finished, max_steps, episodes};
    const unsigned grid = grid_tiles(e->n);
    with_combo(step_combo(e), [&]<int INTEG, bool PARAMS, int RMODE>() {
        hipLaunchKernelGGL((k_expert_evaluate<INTEG, PARAMS, RMODE>), dim3(grid), dim3(kBlock), 0, e->stream, A, state_des, kp, kd, E);
    });
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

// ---- the sampling planners: random-shooting MPC and MPPI --------------------------------------
// What every entry point checks alike, after its own arguments; then the step counter, read synchronously: the candidate
// keys hold it in `key_bits` bits (shooting: (k << 26) | (c << 10) | h; MPPI: (1 << 63) | (k << 30) | (it << 26) | (c << 10) | h).
static int plan_check(QsEnv *e, const char *name, int horizon, int max_horizon, int paths, int max_paths, int objective, bool host_ok)
{
    if (e->cfg.kind == QS_KIND_HOVERING_V0) return fail(QS_ERR_INVALID, "%s: docking envs only", name);
    if (!host_ok && e->cfg.io_space != QS_IO_DEVICE) return fail(QS_ERR_INVALID, "%s: device buffers only", name);
    if (paths < 1 || paths > max_paths) return fail(QS_ERR_INVALID, "%s: paths must be in [1, %d], got %d", name, max_paths, paths);
    if (horizon < 1 || horizon > max_horizon)
        return fail(QS_ERR_INVALID, "%s: horizon must be in [1, %d], got %d", name, max_horizon, horizon);
    if (objective != QS_SHOOT_REWARD && objective != QS_SHOOT_POSITION) return fail(QS_ERR_INVALID, "%s: unknown objective %d", name, objective);
    if (e->n > 0x7fffffff) return fail(QS_ERR_INVALID, "%s: one workgroup per env: at most 2^31 - 1 envs", name);
    return QS_OK;
}

static int plan_counter(QsEnv *e, const char *name, int key_bits)
{
    unsigned long long k = 0;
    HIP_TRY(hipMemcpyAsync(&k, e->d_ctr, sizeof k, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (k >> key_bits)
        return fail(QS_ERR_INVALID, "%s: step counter %llu does not fit the %d bits of the candidate keys", name, k, key_bits);
    return QS_OK;
}

// min(256, paths rounded up to a wave) threads
static unsigned plan_block(int paths) { return (unsigned)std::min<int64_t>(kBlock, ((int64_t)paths + kTile - 1) / kTile * kTile); }

// The automatic `splits` of the split entry points (the rule is stated in quadsim.h): 1 where the envs alone give every CU two
// workgroups, else as many parts as reach that, but no part under kWideMinPart candidates and at most kWideMaxSplits parts.
constexpr int kWideMinPart = 256;
static int plan_auto_splits(QsEnv *e, int paths, int *splits)
{
    if (!e->cu_count) HIP_TRY(hipDeviceGetAttribute(&e->cu_count, hipDeviceAttributeMultiprocessorCount, e->cfg.device));
    const int64_t want = 2 * (int64_t)std::max(e->cu_count, 1);
    int64_t s = e->n >= want ? 1 : (want + e->n - 1) / e->n;
    s = std::min<int64_t>(s, (paths + kWideMinPart - 1) / kWideMinPart);
    *splits = (int)std::max<int64_t>(1, std::min<int64_t>(s, kWideMaxSplits));
    return QS_OK;
}

int qs_shooting_plan_splits(QsEnv *e, int32_t paths, int32_t *splits)
{
    CHECK_ENV_RAW(e);
    if (!splits) return fail(QS_ERR_INVALID, "qs_shooting_plan_splits: splits is required");
    if (paths < 1 || paths > 65536) return fail(QS_ERR_INVALID, "qs_shooting_plan_splits: paths must be in [1, 65536], got %d", paths);
    int s = 1;
    if (int rc = plan_auto_splits(e, paths, &s)) return rc;
    *splits = s;
    return QS_OK;
}

// What all four entry points check after their own arguments, in this order: plan_check, the range of `splits` (0: automatic),
// the one-part rule (S = 1 holds at most one_part_max_paths candidates; only MPPI's kernel has such a limit), the automatic
// choice, the grid limit, and last the step counter -> the number of parts S >= 1, or a negative QS_ERR_*.
static int plan_admit(QsEnv *e, const char *name, bool host_ok, int horizon, int max_horizon, int paths, int max_paths,
                      int one_part_max_paths, int objective, int splits, int key_bits)
{
    if (int rc = plan_check(e, name, horizon, max_horizon, paths, max_paths, objective, host_ok)) return rc;
    const int max_splits = std::min<int>(paths, kWideMaxSplits);
    if (splits < 0 || splits > max_splits)
        return fail(QS_ERR_INVALID, "%s: splits must be 0 (automatic) or in [1, min(paths, %d)] = [1, %d], got %d", name,
                    kWideMaxSplits, max_splits, splits);
    if (splits == 1 && paths > one_part_max_paths)
        return fail(QS_ERR_INVALID, "%s: splits = 1 launches qs_mppi_plan's kernel, which holds at most %d paths, got %d", name,
                    one_part_max_paths, paths);
    int S = splits;
    if (S == 0) {
        if (int rc = plan_auto_splits(e, paths, &S)) return rc;
        if (paths > one_part_max_paths) S = std::max(S, 2);
    }
    if (e->n * (int64_t)S > 0x7fffffff)
        return fail(QS_ERR_INVALID, "%s: one workgroup per part: envs x splits must be below 2^31, got %lld x %d", name, (long long)e->n, S);
    if (int rc = plan_counter(e, name, key_bits)) return rc;
    return S;
}

// The one workspace of both planner families, for what crosses from one kernel of a split plan to the next: at least `bytes`,
// grown and never shrunk; each call lays its arrays out from its own sizes.  Sharing it is safe: every planner kernel of a
// handle runs on the handle's one stream, so a plan's kernels have finished with it before the next plan's start, and a
// growth waits for the stream before it frees.  A failed allocation leaves the handle usable, without a workspace.
static int plan_workspace(QsEnv *e, const char *name, uint64_t bytes)
{
    if (e->plan_ws_bytes >= bytes) return QS_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->plan_ws) HIP_TRY(hipFree(e->plan_ws));
    e->plan_ws = nullptr; e->plan_ws_bytes = 0;
    if (hipMalloc((void **)&e->plan_ws, bytes) != hipSuccess) {
        (void)hipGetLastError();                            // reported here
        e->plan_ws = nullptr;
        return fail(QS_ERR_HIP, "%s: cannot allocate the workspace of %llu bytes", name, (unsigned long long)bytes);
    }
    e->plan_ws_bytes = bytes;
    return QS_OK;
}

// ---- random shooting: S = 1 is k_shooting_plan, S > 1 the two kernels of shooting_split.hpp
static int launch_shooting(QsEnv *e, const StepArgs &A, const PlanArgs &X, int S)
{
    const size_t lds = plan_lds_bytes(X.horizon);
    if (S == 1) {
        with_integ_params(step_combo(e), [&]<int INTEG, bool PARAMS>() {
            hipLaunchKernelGGL((k_shooting_plan<INTEG, PARAMS>), dim3((unsigned)e->n), dim3(plan_block(X.paths)), lds, e->stream, A, X);
        });
    } else {
        // workspace: partial winners, score [n S] f64 | index [n S] int32
        const size_t slots = (size_t)e->n * (size_t)S;
        const WideArgs W{S, reinterpret_cast<double *>(e->plan_ws), reinterpret_cast<int32_t *>(e->plan_ws + slots * sizeof(double))};
        const unsigned block = plan_block((X.paths + S - 1) / S);
        with_integ_params(step_combo(e), [&]<int INTEG, bool PARAMS>() {
            hipLaunchKernelGGL((k_wide_candidates<INTEG, PARAMS>), dim3((unsigned)slots), dim3(block), lds, e->stream, A, X, W);
        });
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_wide_finish, dim3((unsigned)e->n), dim3(kTile), 0, e->stream, A, X, W);
    }
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

// A device handle's kernels work on the caller's memory, so its alignment matters; a host handle's buffers are copied through
// the staging slices, which are aligned whatever the caller's are.
static int shooting_check_aligned(const char *name, bool device, const PlanArgs &X)
{
    if (device && (((((uintptr_t)X.actions) | ((uintptr_t)X.sequence)) & 15u) || ((((uintptr_t)X.best_score) | ((uintptr_t)X.scores)) & 7u)
                   || (((uintptr_t)X.best_index) & 3u)))
        return fail(QS_ERR_INVALID, "%s: actions and sequence must be 16-byte aligned, best_score and scores 8-byte, best_index 4-byte", name);
    return QS_OK;
}

// both entry points: the unsplit one is S = 1 on a device handle (host_ok = false), which never takes a workspace
static int shooting_plan(QsEnv *e, const char *name, bool host_ok, int splits, PlanArgs X)
{
    if (!X.actions) return fail(QS_ERR_INVALID, "%s: actions is required", name);
    if (int rc = shooting_check_aligned(name, !host_ok || e->cfg.io_space == QS_IO_DEVICE, X)) return rc;
    const int S = plan_admit(e, name, host_ok, X.horizon, 256, X.paths, 65536, 65536, X.objective, splits, 36);
    if (S < 0) return S;
    if (S > 1)
        if (int rc = plan_workspace(e, name, (uint64_t)e->n * (uint64_t)S * (sizeof(double) + sizeof(int32_t)))) return rc;
    const size_t n = (size_t)e->n;
    UserIO io = user_io(e);
    io.out(X.actions, n * 4); io.out(X.best_score, n); io.out(X.best_index, n);
    io.out(X.sequence, n * X.horizon * 4); io.out(X.scores, n * X.paths);
    if (int r = io.push()) return r;
    if (int r = launch_shooting(e, make_args(e), X, S)) return r;
    return io.pull();
}

int qs_shooting_plan(QsEnv *e, int32_t horizon, int32_t paths, int32_t objective, float *actions, double *best_score,
                     int32_t *best_index, float *sequence, double *scores)
{
    CHECK_ENV(e);
    Range rg_("qs_shooting_plan");
    return shooting_plan(e, "qs_shooting_plan", false, 1, PlanArgs{horizon, paths, objective, actions, best_score, best_index, sequence, scores});
}

int qs_shooting_plan_split(QsEnv *e, int32_t horizon, int32_t paths, int32_t objective, int32_t splits, float *actions,
                           double *best_score, int32_t *best_index, float *sequence, double *scores)
{
    CHECK_ENV(e);
    Range rg_("qs_shooting_plan_split");
    return shooting_plan(e, "qs_shooting_plan_split", true, splits,
                         PlanArgs{horizon, paths, objective, actions, best_score, best_index, sequence, scores});
}

// ---- MPPI: S = 1 is k_mppi (at most kMppiOnePartPaths candidates: their scores live in LDS), S > 1 the three kernels per
// iteration of mppi_split.hpp
constexpr int kMppiOnePartPaths = 4096;

static int mppi_check_scalars(const char *name, const MppiArgs &X)
{
    if (X.iterations < 1 || X.iterations > 16) return fail(QS_ERR_INVALID, "%s: iterations must be in [1, 16], got %d", name, X.iterations);
    if (!(X.lambda > 0.0) || !std::isfinite(X.lambda)) return fail(QS_ERR_INVALID, "%s: lambda must be positive and finite, got %g", name, X.lambda);
    if (!(X.sigma >= 0.0f) || !std::isfinite(X.sigma))
        return fail(QS_ERR_INVALID, "%s: sigma must be non-negative and finite, got %g", name, (double)X.sigma);
    if (X.shift != 0 && X.shift != 1) return fail(QS_ERR_INVALID, "%s: shift must be 0 or 1, got %d", name, X.shift);
    if (!X.actions || !X.nominal_out) return fail(QS_ERR_INVALID, "%s: actions and nominal_out are required", name);
    return QS_OK;
}

// as shooting_check_aligned
static int mppi_check_aligned(const char *name, bool device, const MppiArgs &X)
{
    if (device && (((((uintptr_t)X.actions) | ((uintptr_t)X.nominal_out) | ((uintptr_t)X.nominal_in) | ((uintptr_t)X.noise)
                     | ((uintptr_t)X.trace) | ((uintptr_t)X.candidates)) & 15u) || ((((uintptr_t)X.best_score) | ((uintptr_t)X.scores)) & 7u)))
        return fail(QS_ERR_INVALID, "%s: actions, nominal_in, nominal_out, noise, trace and candidates must be 16-byte aligned, best_score and scores 8-byte", name);
    return QS_OK;
}

// the workspace of a split plan: U [n][horizon] float4 | scores [n][paths] f64 | maxima [n S] f64 | partial sums [n S][horizon 4 + 1] f64
struct MppiWorkspace {
    uint64_t off_score, off_max, off_sum, bytes;
    MppiWorkspace(int64_t n, const MppiArgs &X, int S)
    {
        const uint64_t slots = (uint64_t)n * (uint64_t)S, words = (uint64_t)X.horizon * 4 + 1;
        off_score = (uint64_t)n * (uint64_t)X.horizon * sizeof(float4);
        off_max = off_score + (uint64_t)n * (uint64_t)X.paths * sizeof(double);
        off_sum = off_max + slots * sizeof(double);
        bytes = off_sum + slots * words * sizeof(double);
    }
};

static int launch_mppi(QsEnv *e, const StepArgs &A, const MppiArgs &X, int S)
{
    if (S == 1) {
        const size_t lds = mppi_lds_bytes(X.horizon, X.paths);  // < 64 KiB at the largest horizon and paths: no function attribute
        with_integ_params(step_combo(e), [&]<int INTEG, bool PARAMS>() {
            hipLaunchKernelGGL((k_mppi<INTEG, PARAMS>), dim3((unsigned)e->n), dim3(plan_block(X.paths)), lds, e->stream, A, X);
        });
    } else {
        const MppiWorkspace L(e->n, X, S);
        MppiPartArgs W{S, 0, reinterpret_cast<float4 *>(e->plan_ws), reinterpret_cast<double *>(e->plan_ws + L.off_score),
                       reinterpret_cast<double *>(e->plan_ws + L.off_max), reinterpret_cast<double *>(e->plan_ws + L.off_sum)};
        const unsigned slots = (unsigned)(e->n * S), block = plan_block((X.paths + S - 1) / S);
        const size_t lds_roll = mppi_roll_lds_bytes(X.horizon), lds_sums = mppi_sums_lds_bytes(X.horizon);
        for (int it = 0; it < X.iterations; ++it) {
            W.it = it;
            with_integ_params(step_combo(e), [&]<int INTEG, bool PARAMS>() {
                hipLaunchKernelGGL((k_pathint_part_roll<INTEG, PARAMS>), dim3(slots), dim3(block), lds_roll, e->stream, A, X, W);
            });
            hipLaunchKernelGGL(k_pathint_part_sums, dim3(slots), dim3(block), lds_sums, e->stream, A, X, W);
            hipLaunchKernelGGL(k_pathint_part_finish, dim3((unsigned)e->n), dim3(kTile), 0, e->stream, A, X, W);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipGetLastError());
    return QS_OK;
}

// both entry points, as shooting_plan; the unsplit one keeps k_mppi's limit on `paths` as its own
static int mppi_plan(QsEnv *e, const char *name, bool host_ok, int splits, MppiArgs X)
{
    if (int rc = mppi_check_scalars(name, X)) return rc;
    if (int rc = mppi_check_aligned(name, !host_ok || e->cfg.io_space == QS_IO_DEVICE, X)) return rc;
    const int S = plan_admit(e, name, host_ok, X.horizon, 128, X.paths, host_ok ? 65536 : kMppiOnePartPaths, kMppiOnePartPaths,
                             X.objective, splits, 33);
    if (S < 0) return S;
    if (S > 1)
        if (int rc = plan_workspace(e, name, MppiWorkspace(e->n, X, S).bytes)) return rc;
    const size_t n = (size_t)e->n, seq = (size_t)X.horizon * 4;
    UserIO io = user_io(e);
    io.in(X.nominal_in, n * seq); io.in(X.noise, (size_t)X.iterations * X.paths * seq);
    io.out(X.actions, n * 4); io.out(X.nominal_out, n * seq); io.out(X.best_score, n);
    io.out(X.scores, n * X.iterations * X.paths); io.out(X.trace, n * (X.iterations + 1) * seq); io.out(X.candidates, n * X.paths * seq);
    if (int r = io.push()) return r;
    if (int r = launch_mppi(e, make_args(e), X, S)) return r;
    return io.pull();
}

int qs_mppi_plan(QsEnv *e, int32_t horizon, int32_t paths, int32_t iterations, int32_t objective, float lambda, float sigma,
                 int32_t shift, const float *nominal_in, const float *noise, float *actions, float *nominal_out,
                 double *best_score, double *scores, float *trace, float *candidates)
{
    CHECK_ENV(e);
    Range rg_("qs_mppi_plan");
    return mppi_plan(e, "qs_mppi_plan", false, 1, MppiArgs{horizon, paths, iterations, objective, shift, lambda, sigma, nominal_in, noise,
                                                          actions, nominal_out, best_score, scores, trace, candidates});
}

int qs_mppi_plan_split(QsEnv *e, int32_t horizon, int32_t paths, int32_t iterations, int32_t objective, float lambda, float sigma,
                       int32_t shift, int32_t splits, const float *nominal_in, const float *noise, float *actions,
                       float *nominal_out, double *best_score, double *scores, float *trace, float *candidates)
{
    CHECK_ENV(e);
    Range rg_("qs_mppi_plan_split");
    return mppi_plan(e, "qs_mppi_plan_split", true, splits, MppiArgs{horizon, paths, iterations, objective, shift, lambda, sigma, nominal_in,
                                                                   noise, actions, nominal_out, best_score, scores, trace, candidates});
}

// ---- layer 1 ---------------------------------------------------------------------------------
int qs_drone_step(QsEnv *e, int64_t n, float *state, float *u_prev, const float *u, const float *par, uint8_t *limited)
{
    CHECK_ENV(e);
    if (n < 1 || !state || !u_prev || !u) return fail(QS_ERR_INVALID, "qs_drone_step: bad arguments");
    Par pn{e->cfg.mass, e->cfg.inertia[0], e->cfg.inertia[1], e->cfg.inertia[2]};
    UserIO io = user_io(e);
    io.inout(state, n * 13); io.inout(u_prev, n * 4);
    io.in(u, n * 4); io.in(par, n * 4);
    io.out(limited, n);
    if (int r = io.push()) return r;
    hipLaunchKernelGGL(k_drone_step, dim3(grid_flat(n)), dim3(kBlock), 0, e->stream, n, state, u_prev, u, par, limited, pn, e->cfg.dt,
                       e->cfg.integrator);
    HIP_TRY(hipGetLastError());
    return io.pull();
}

int qs_ctrl(QsEnv *e, int64_t n, int32_t mode, float *state_des, const float *state, const float *state_last, float mass,
            float *u_out)
{
    CHECK_ENV(e);
    if (n < 1 || !state_des || !state || !u_out || (mode != 0 && mode != 1)) return fail(QS_ERR_INVALID, "qs_ctrl: bad arguments");
    if (mode == 1 && !state_last) return fail(QS_ERR_INVALID, "qs_ctrl: vel_controller needs state_last");
    UserIO io = user_io(e);
    io.inout(state_des, n * 13);
    io.in(state, n * 13); io.in(state_last, n * 13);
    io.out(u_out, n * 4);
    if (int r = io.push()) return r;
    hipLaunchKernelGGL(k_ctrl, dim3(grid_flat(n)), dim3(kBlock), 0, e->stream, n, (int)mode, state_des, state, state_last, mass, u_out);
    HIP_TRY(hipGetLastError());
    return io.pull();
}

int qs_transform(QsEnv *e, int32_t op, int64_t n, const float *in, float *out)
{
    CHECK_ENV(e);
    if (n < 1 || !in || !out || op < 0 || op > 3) return fail(QS_ERR_INVALID, "qs_transform: bad arguments");
    const int wi[4] = {4, 3, 4, 9}, wo[4] = {3, 4, 9, 3};
    UserIO io = user_io(e);
    io.in(in, n * wi[op]);
    io.out(out, n * wo[op]);
    if (int r = io.push()) return r;
    hipLaunchKernelGGL(k_transform, dim3(grid_flat(n)), dim3(kBlock), 0, e->stream, (int)op, n, in, out);
    HIP_TRY(hipGetLastError());
    return io.pull();
}

int qs_rel_obs(QsEnv *e, int64_t n, const float *chaser, const float *target, float *obs)
{
    CHECK_ENV(e);
    if (n < 1 || !chaser || !target || !obs) return fail(QS_ERR_INVALID, "qs_rel_obs: bad arguments");
    UserIO io = user_io(e);
    io.in(chaser, n * 13); io.in(target, n * 13);
    io.out(obs, n * 12);
    if (int r = io.push()) return r;
    hipLaunchKernelGGL(k_rel_obs, dim3(grid_flat(n)), dim3(kBlock), 0, e->stream, n, chaser, target, obs);
    HIP_TRY(hipGetLastError());
    return io.pull();
}

}  // extern "C"
