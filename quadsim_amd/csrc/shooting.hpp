// shooting.hpp -- random-shooting MPC (qs_shooting_plan): `paths` random action sequences of length `horizon` per env, rolled
// through the exact env from the env's CURRENT state, scored, and the best one's first action returned -- the planner of
// MPC-based_RL.py:170-210 (Mpc_Controller.choose_action / compute_cost) with the simulator itself as the model.  Read-only on
// the handle.  A fragment of quadsim_hip.hip, included right after plan_common.hpp, nowhere else.
//
// Mapping: ONE WORKGROUP PER ENV (blockIdx.x = env), candidates on lanes.  Every lane of the workgroup reads the same env
// record, so the loads of the env, its parameters and its step counter are wave-uniform (scalar loads; tile_lane's
// one-tile-per-wave prologue does not apply, load_env / load_par / step_counter_begin do, at (env / 64, env % 64)).
//   1. Wave 0 integrates the TARGET drone `horizon` steps (env_step_target: it never sees the action) and leaves the
//      horizon x (13 state words + target-limited bit) in LDS; its stored control and q_des live and die in that loop.
//   2. After one barrier lane j takes candidates c = j, j + blockDim, ...: it draws a[c][h] from
//      philox_block(seed, STREAM_PLAN, gid, k << 26 | c << 10 | h), runs env_step_chaser against the LDS target row (a
//      broadcast read) and keeps the float64 score and its running best (score, c).  No reset inside a horizon; a candidate
//      stops after its first done step, which is per-lane divergence inside a wave and nothing else.
//   3. (score, index) is reduced with cross-lane shuffles, then over the workgroup's <= 4 waves in LDS; the order
//      "higher score, then lower index" is total, so the winner does not depend on the lane / wave mapping.
//   4. The workgroup regenerates the winner's actions from its index (lane h draws step h) and writes them.
// env_step_target + env_step_chaser are the two halves of env_step (quadsim_device.hpp: same operations on the same operands),
// so candidate c computes the bits of `horizon` qs_step calls on a copy of the env with the same actions.
// The block is min(256, paths rounded up to a wave) threads, so few paths do not pay for idle waves; LDS is sized by horizon.
#pragma once

namespace {

struct PlanArgs {
    int horizon, paths, objective;   // objective: QS_SHOOT_REWARD / QS_SHOOT_POSITION
    float *actions;                  // [n,4]
    double *best_score;              // nullable [n]
    int32_t *best_index;             // nullable [n]
    float *sequence;                 // nullable [n,horizon,4]
    double *scores;                  // nullable [n,paths]
};

constexpr int kPlanRowWords = 14;    // one LDS row per horizon step: target state [13], target-limited bit
constexpr int kPlanHeadBytes = 64;   // reduction scratch in front of the rows: 4 x (double, int), the winner's index
inline size_t plan_lds_bytes(int horizon) { return kPlanHeadBytes + (size_t)horizon * kPlanRowWords * sizeof(float); }

// actions of candidate c at horizon step h, planned before global step k (k < 2^36, c < 2^16, h < 2^10)
__device__ __forceinline__ void plan_action(uint64_t seed, uint64_t gid, uint64_t k, unsigned c, unsigned h, float a[4])
{
    const uint4 w = philox_block(seed, STREAM_PLAN, gid, (k << 26) | ((uint64_t)c << 10) | (uint64_t)h);
    a[0] = sym(u01(w.x)); a[1] = sym(u01(w.y)); a[2] = sym(u01(w.z)); a[3] = sym(u01(w.w));
}

// the total order of the reduction: higher score first, then lower index
__device__ __forceinline__ bool plan_better(double s, int i, double bs, int bi) { return s > bs || (s == bs && i < bi); }

template <int INTEG, bool PARAMS>
__global__ __launch_bounds__(kBlock) void k_shooting_plan(StepArgs A, PlanArgs X)
{
    extern __shared__ __align__(16) unsigned char plan_lds[];
    double *const red_s = reinterpret_cast<double *>(plan_lds);                 // [4]
    int *const red_i = reinterpret_cast<int *>(plan_lds + 32);                  // [4]
    int *const winner = reinterpret_cast<int *>(plan_lds + 48);
    float *const rows = reinterpret_cast<float *>(plan_lds + kPlanHeadBytes);   // [horizon][kPlanRowWords]

    const int64_t env = blockIdx.x;                       // < A.n: the grid is n workgroups
    const int64_t tile = env / kTile;
    const int slot = (int)(env % kTile);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    QS_ASSERT(env < A.n && tile < A.tile_end);
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

    double best_s = -__builtin_huge_val();
    int best_i = 0x7fffffff;
#pragma clang loop unroll(disable)
    for (int c = threadIdx.x; c < X.paths; c += blockDim.x) {
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
        if (best_i == 0x7fffffff) best_i = 0;             // every score NaN (a non-finite state): still a valid index
        *winner = best_i;
        if (X.best_score) X.best_score[env] = best_s;
        if (X.best_index) X.best_index[env] = best_i;
    }
    __syncthreads();
    const int win = *winner;
    for (int h = threadIdx.x; h < X.horizon; h += blockDim.x) {
        float a[4];
        plan_action(A.rc.seed, gid, k, (unsigned)win, (unsigned)h, a);
        const float4 v = make_float4(a[0], a[1], a[2], a[3]);
        if (h == 0) reinterpret_cast<float4 *>(X.actions)[env] = v;
        if (X.sequence) reinterpret_cast<float4 *>(X.sequence)[env * X.horizon + h] = v;
    }
}

}  // namespace
