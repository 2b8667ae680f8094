// shooting_split.hpp -- qs_shooting_plan_split: the random-shooting planner of shooting.hpp with ONE ENV'S CANDIDATES SPREAD
// OVER `splits` WORKGROUPS, for handles of few envs (a real-time MPC on one drone) that k_shooting_plan's one workgroup per
// env leaves on one CU.  A fragment of quadsim_hip.hip, included right after mppi.hpp, nowhere else.
//
// Two launches on the handle's stream; the kernel boundary between them is the only ordering across workgroups.  No workgroup
// waits for, polls or counts another one, so there is nothing that could hang, and the partial winners cross from one kernel
// to the next through memory that the first kernel has finished writing before the second starts.
//   1. k_wide_candidates<INTEG, PARAMS>, grid n x S flat: env = blockIdx.x / S, part = blockIdx.x % S.  Part p owns the
//      candidates [p * ceil(paths / S), (p + 1) * ceil(paths / S)) cut at `paths`; trailing parts may be short or empty.  It
//      is k_shooting_plan up to the in-workgroup reduction -- wave 0 integrates the target into the LDS rows (every part
//      repeats that: `horizon` steps of one wave), lanes take c = lo + threadIdx.x, + blockDim.x, ... and keep the float64
//      score and the running best under plan_better -- and thread 0 writes the part's (score, index) to slot env * S + part
//      of the handle's workspace (the one workspace of both split planners: plan_workspace in quadsim_hip.hip).  An empty
//      part writes (-inf, 0x7fffffff), which loses to everything.  `scores` is the only output it writes.
//   2. k_wide_finish, one 64-lane workgroup per env: lanes read parts lane, lane + 64, ..., reduce with plan_better over
//      shuffles, and write best_score, best_index, actions and sequence, regenerated from the winner's index (lane h draws
//      step h).  It needs k, gid and the seed only: no INTEG / PARAMS.
// plan_better is a total order (higher score, then lower index), so any partition gives k_shooting_plan's winner; the
// candidates' scores come from the same inlined device functions under -ffp-contract=on, so they are its bits.
// The roll-out loop is an edited copy of k_shooting_plan's on purpose: a device function shared with it changed the machine
// code of the existing planner kernels (profiles/plan_common/README.md), and those stay as they are.
#pragma once

namespace {

struct WideArgs {
    int splits;                      // S: parts per env
    double *part_score;              // [n * S] workspace of the handle
    int32_t *part_index;             // [n * S]
};

constexpr int kWideMaxSplits = 1024;

template <int INTEG, bool PARAMS>
__global__ __launch_bounds__(kBlock) void k_wide_candidates(StepArgs A, PlanArgs X, WideArgs W)
{
    extern __shared__ __align__(16) unsigned char wide_lds[];
    double *const red_s = reinterpret_cast<double *>(wide_lds);                 // [4]
    int *const red_i = reinterpret_cast<int *>(wide_lds + 32);                  // [4]
    float *const rows = reinterpret_cast<float *>(wide_lds + kPlanHeadBytes);   // [horizon][kPlanRowWords]

    const int64_t env = blockIdx.x / (unsigned)W.splits;    // < A.n: the grid is n x S workgroups
    const int part = (int)(blockIdx.x % (unsigned)W.splits);
    const PlanPart own = plan_part(part, W.splits, X.paths);
    const int lo = own.lo, hi = own.hi;
    const int64_t tile = env / kTile;
    const int slot = (int)(env % kTile);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    QS_ASSERT(env < A.n && tile < A.tile_end);

    double best_s = -__builtin_huge_val();
    int best_i = 0x7fffffff;
    if (lo >= hi) {                                       // an empty part (the whole workgroup: no barrier is skipped by some)
        if (threadIdx.x == 0) { W.part_score[blockIdx.x] = best_s; W.part_index[blockIdx.x] = best_i; }
        return;
    }

    const uint64_t k = step_counter_begin(A, tile);
    const uint64_t gid = A.gid0 + (uint64_t)env;
    Env e;
    load_env(A.st, tile, slot, e);
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, slot);

    if (wave == 0) {
        Env tg = e;
#pragma clang loop unroll(disable)
        for (int h = 0; h < X.horizon; ++h) {
            const bool lim_t = env_step_target<INTEG>(tg, P, A.C);
            if (lane == 0) {
                float *r = rows + h * kPlanRowWords;
#pragma unroll
                for (int i = 0; i < 13; ++i) r[i] = tg.st[i];
                r[13] = lim_t ? 1.0f : 0.0f;
            }
        }
    }
    __syncthreads();

    // the observation before step 0 is the current one, common to all candidates
    float obs0[12];
    rel_obs(e.sc, e.st, obs0);
    const float pos0 = plan_pos(obs0);
    const bool by_position = X.objective != 0;

#pragma clang loop unroll(disable)
    for (int c = lo + (int)threadIdx.x; c < hi; c += blockDim.x) {
        Env ec = e;
        double score = 0.0;
        float pos = pos0;
        bool alive = true;
#pragma clang loop unroll(disable)
        for (int h = 0; h < X.horizon && alive; ++h) {
            if (by_position) score += (double)pos;
            float a[4], obs[12], reward;
            unsigned flags;
            plan_action(A.rc.seed, gid, k, (unsigned)c, (unsigned)h, a);
            const float *r = rows + h * kPlanRowWords;
#pragma unroll
            for (int i = 0; i < 13; ++i) ec.st[i] = r[i];
            env_step_chaser<INTEG>(ec, a, P, A.C, r[13] != 0.0f, obs, reward, flags);
            if (!by_position) score += (double)reward;
            pos = plan_pos(obs);
            alive = (flags & (FLAG_OVERLIMIT | FLAG_OVERTIME)) == 0;      // `done` of the step kernels (maybe_reset)
        }
        if (X.scores) X.scores[env * X.paths + c] = score;
        if (plan_better(score, c, best_s, best_i)) { best_s = score; best_i = c; }
    }

#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(best_s, m);
        const int oi = __shfl_xor(best_i, m);
        if (plan_better(os, oi, best_s, best_i)) { best_s = os; best_i = oi; }
    }
    if (lane == 0) { red_s[wave] = best_s; red_i[wave] = best_i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int waves = (int)(blockDim.x >> 6);
        for (int w = 1; w < waves; ++w)
            if (plan_better(red_s[w], red_i[w], best_s, best_i)) { best_s = red_s[w]; best_i = red_i[w]; }
        W.part_score[blockIdx.x] = best_s;                // slot env * S + part; 0x7fffffff stays if every score was NaN
        W.part_index[blockIdx.x] = best_i;
    }
}

__global__ __launch_bounds__(kTile) void k_wide_finish(StepArgs A, PlanArgs X, WideArgs W)
{
    const int64_t env = blockIdx.x;                       // < A.n: the grid is n workgroups of one wave
    const int lane = threadIdx.x;
    QS_ASSERT(env < A.n && env / kTile < A.tile_end);
    const uint64_t k = step_counter_begin(A, env / kTile);
    const uint64_t gid = A.gid0 + (uint64_t)env;

    double best_s = -__builtin_huge_val();
    int best_i = 0x7fffffff;
    for (int p = lane; p < W.splits; p += kTile) {
        const double s = W.part_score[env * W.splits + p];
        const int i = W.part_index[env * W.splits + p];
        if (plan_better(s, i, best_s, best_i)) { best_s = s; best_i = i; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(best_s, m);
        const int oi = __shfl_xor(best_i, m);
        if (plan_better(os, oi, best_s, best_i)) { best_s = os; best_i = oi; }
    }
    // every lane holds the winner now (the order is total, the butterfly symmetric)
    if (best_i == 0x7fffffff) { best_i = 0; best_s = -__builtin_huge_val(); }   // every score NaN: still a valid index
    if (lane == 0) {
        if (X.best_score) X.best_score[env] = best_s;
        if (X.best_index) X.best_index[env] = best_i;
    }
    for (int h = lane; h < X.horizon; h += kTile) {
        float a[4];
        plan_action(A.rc.seed, gid, k, (unsigned)best_i, (unsigned)h, a);
        const float4 v = make_float4(a[0], a[1], a[2], a[3]);
        if (h == 0) reinterpret_cast<float4 *>(X.actions)[env] = v;
        if (X.sequence) reinterpret_cast<float4 *>(X.sequence)[env * X.horizon + h] = v;
    }
}

}  // namespace
