// mppi_split.hpp -- qs_mppi_plan_split: the MPPI planner of mppi.hpp with ONE ENV'S CANDIDATES SPREAD OVER `splits` WORKGROUPS,
// for handles of few envs (a real-time controller on one drone) that k_mppi's one workgroup per env leaves on one CU, and for
// more candidates than one workgroup's LDS holds scores of (paths up to 65536).  A fragment of quadsim_hip.hip, included right
// after shooting_split.hpp, nowhere else.
//
// The update is a softmax over ALL of an env's candidates, so a partition needs two reductions across workgroups per iteration:
// Smax first, then the weighted sums.  Three launches per iteration on the handle's stream; the kernel boundary between two
// launches is the only ordering across workgroups.  No workgroup waits for, polls, counts or signals another one, so there is
// nothing that could hang; what crosses from one kernel to the next does so through the handle's workspace (the one workspace
// of both split planners: plan_workspace in quadsim_hip.hip, which lays it out for this call), which the earlier
// kernel has finished writing before the later one starts.  Part p of env i owns the candidates
// [p * ceil(paths / S), (p + 1) * ceil(paths / S)) cut at `paths`, as k_wide_candidates cuts them; trailing parts may be
// short or empty.  The two N x S grids are flat: env = blockIdx.x / S, part = blockIdx.x % S, slot = blockIdx.x.
//   1. k_pathint_part_roll<INTEG, PARAMS>, grid N x S.  The nominal of this iteration goes to LDS: in iteration 0 it is
//      nominal_in[env][min(h + shift, horizon - 1)] or zeros (every read of nominal_in happens in this launch, so nominal_in
//      may alias nominal_out), and part 0 -- never empty -- also leaves it in the workspace and in trace[env][0]; later it is
//      the U of the workspace.  Wave 0 integrates the target into LDS rows (every part repeats that: `horizon` steps of one
//      wave).  Lanes take c = lo + tid, + blockDim, ...; the candidates are mppi_action's (same keys, same `noise` indexing,
//      candidate 0 the nominal), the roll-out and the score k_mppi's.  The float64 score goes to the workspace [N, paths] and
//      to scores[env][it][c]; the part's maximum over its non-NaN scores goes to slot env * S + part.
//   2. k_pathint_part_sums, grid N x S.  Smax = the maximum of the env's S slots (exact, so any order).  The weights
//      w = exp((S[c] - Smax) / lambda), float64, NaN -> 0, overwrite the part's scores in the workspace, each by the thread
//      that reads the score.  Then lanes over h, waves over c: wave v adds w[c] a[c][h] for c = lo + v, lo + v + waves, ... in
//      ascending order into float64 fma sums (candidates regenerated, never stored; the last iteration's `candidates` leave
//      from here), the waves are added in wave order, and the part writes [horizon][4] sums and its sum of weights to its slot.
//      It needs k, gid and the seed only: no INTEG / PARAMS.
//   3. k_pathint_part_finish, one 64-lane workgroup per env: lane h adds the S partial sums and the S weight sums in part order
//      p = 0 .. S-1, divides (U stays where the weight sum is not positive), and writes U to the workspace and to
//      trace[env][it + 1]; after the last iteration also nominal_out, actions = U[0] and best_score = Smax.
// A part without candidates writes its neutral element (-inf; zeros) and returns as a whole workgroup, before any barrier.
// The summation order is a function of (paths, S, block size) alone, and the block size one of ceil(paths / S): the result does
// not depend on N, the env index, env_id_offset or the launch path.
// The roll-out loop is an edited copy of k_mppi's on purpose, as shooting_split.hpp's is of k_shooting_plan's: a device function
// shared with it changed the machine code of the existing planner kernels (profiles/plan_common/README.md).
// The kernels are named k_pathint_* (path integral): tests/test_mppi_cpu.py takes every kernel with `mppi` in its name for an
// instantiation of k_mppi, and k_wide* belongs to shooting_split.hpp.
#pragma once

namespace {

struct MppiPartArgs {
    int splits, it;                  // S: parts per env; the iteration these launches belong to
    float4 *U;                       // [n][horizon] workspace of the handle: the nominal between iterations
    double *score;                   // [n][paths]: scores after the roll-out, weights after the sums
    double *part_max;                // [n * S]
    double *part_sum;                // [n * S][horizon * 4 + 1]: weighted sums, then the sum of the weights
};

constexpr int kMppiPartHeadBytes = 64;   // per-wave Smax [4], per-wave sum of weights [4]
// head | nominal [horizon] float4 | target rows
inline size_t mppi_roll_lds_bytes(int horizon)
{
    return kMppiPartHeadBytes + (size_t)horizon * (4 * sizeof(float) + kPlanRowWords * sizeof(float));
}
// head | per-wave partial sums [4][horizon][4] f64
inline size_t mppi_sums_lds_bytes(int horizon) { return kMppiPartHeadBytes + (size_t)horizon * 4 * 4 * sizeof(double); }

template <int INTEG, bool PARAMS>
__global__ __launch_bounds__(kBlock, 4) void k_pathint_part_roll(StepArgs A, MppiArgs X, MppiPartArgs W)
{
    extern __shared__ __align__(16) unsigned char mppi_roll_lds[];
    double *const red_s = reinterpret_cast<double *>(mppi_roll_lds);                                // [4]
    float4 *const U = reinterpret_cast<float4 *>(mppi_roll_lds + kMppiPartHeadBytes);               // [horizon]
    float *const rows = reinterpret_cast<float *>(U + X.horizon);                                   // [horizon][kPlanRowWords]

    const int64_t env = blockIdx.x / (unsigned)W.splits;    // < A.n: the grid is n x S workgroups
    const int part = (int)(blockIdx.x % (unsigned)W.splits);
    const PlanPart own = plan_part(part, W.splits, X.paths);
    const int lo = own.lo, hi = own.hi;
    const int64_t tile = env / kTile;
    const int slot = (int)(env % kTile);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int it = W.it;
    QS_ASSERT(env < A.n && tile < A.tile_end);

    if (lo >= hi) {                                       // an empty part (the whole workgroup: no barrier is skipped by some)
        if (threadIdx.x == 0) W.part_max[blockIdx.x] = -__builtin_huge_val();
        return;
    }

    const uint64_t k = step_counter_begin(A, tile);
    const uint64_t gid = A.gid0 + (uint64_t)env;
    Env e;
    load_env(A.st, tile, slot, e);
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, slot);

    for (int h = threadIdx.x; h < X.horizon; h += blockDim.x) {
        float4 u;
        if (it == 0) {
            u = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (X.nominal_in) u = reinterpret_cast<const float4 *>(X.nominal_in)[env * X.horizon + min(h + X.shift, X.horizon - 1)];
            if (part == 0) {                              // lo = 0 < paths: part 0 always has work
                W.U[env * X.horizon + h] = u;
                if (X.trace) reinterpret_cast<float4 *>(X.trace)[env * (X.iterations + 1) * X.horizon + h] = u;
            }
        } else {
            u = W.U[env * X.horizon + h];
        }
        U[h] = u;
    }
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

    const bool by_position = X.objective != 0;
    double *const S = W.score + env * X.paths;            // this env's [paths]
    // the observation before step 0 is the current one, common to all candidates
    float obs0[12];
    rel_obs(e.sc, e.st, obs0);
    const float pos0 = plan_pos(obs0);
    int tid0 = threadIdx.x;                               // opaque as `tid` below, for k_mppi's reason
    asm volatile("" : "+v"(tid0));
#pragma clang loop unroll(disable)
    for (int c = lo + tid0; c < hi; c += blockDim.x) {
        Env ec = e;
        double score = 0.0;
        float pos = pos0;
        bool alive = true;
#pragma clang loop unroll(disable)
        for (int h = 0; h < X.horizon && alive; ++h) {
            float a[4];
            mppi_action(X, A.rc.seed, gid, k, it, c, h, U[h], a);
            if (by_position) score += (double)pos;
            float obs[12], reward;
            unsigned flags;
            const float *r = rows + h * kPlanRowWords;
#pragma unroll
            for (int i = 0; i < 13; ++i) ec.st[i] = r[i];
            env_step_chaser<INTEG>(ec, a, P, A.C, r[13] != 0.0f, obs, reward, flags);
            if (!by_position) score += (double)reward;
            pos = plan_pos(obs);
            alive = (flags & (FLAG_OVERLIMIT | FLAG_OVERTIME)) == 0;      // `done` of the step kernels (maybe_reset)
        }
        S[c] = score;
        if (X.scores) X.scores[(env * X.iterations + it) * X.paths + c] = score;
    }
    // The maximum is taken from the scores this thread has just stored, re-read through a thread index the compiler cannot see
    // through (mppi.hpp: a running maximum or hoisted addresses would live in vector registers across the roll-out, which the
    // RK4 instantiations do not have to spare).
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int ln = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    double smax = -__builtin_huge_val();
    for (int c = lo + tid; c < hi; c += blockDim.x)
        if (S[c] > smax) smax = S[c];                     // a NaN never enters
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(smax, m);
        if (os > smax) smax = os;
    }
    if (ln == 0) red_s[wv] = smax;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < waves; ++w)
            if (red_s[w] > smax) smax = red_s[w];
        W.part_max[blockIdx.x] = smax;                    // slot env * S + part; -inf if every score was NaN
    }
}

__global__ __launch_bounds__(kBlock) void k_pathint_part_sums(StepArgs A, MppiArgs X, MppiPartArgs W)
{
    extern __shared__ __align__(16) unsigned char mppi_sums_lds[];
    double *const red_s = reinterpret_cast<double *>(mppi_sums_lds);                                // [4]
    double *const red_w = reinterpret_cast<double *>(mppi_sums_lds + 32);                           // [4]
    double *const part_acc = reinterpret_cast<double *>(mppi_sums_lds + kMppiPartHeadBytes);        // [4][horizon][4]

    const int64_t env = blockIdx.x / (unsigned)W.splits;    // < A.n: the grid is n x S workgroups
    const int part = (int)(blockIdx.x % (unsigned)W.splits);
    const PlanPart own = plan_part(part, W.splits, X.paths);
    const int lo = own.lo, hi = own.hi;
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    const int waves = (int)(blockDim.x >> 6);
    const int it = W.it;
    const int words = X.horizon * 4 + 1;
    double *const out = W.part_sum + (int64_t)blockIdx.x * words;
    QS_ASSERT(env < A.n && env / kTile < A.tile_end);

    if (lo >= hi) {                                       // an empty part (the whole workgroup): zeros
        for (int i = tid; i < words; i += blockDim.x) out[i] = 0.0;
        return;
    }

    const uint64_t k = step_counter_begin(A, env / kTile);
    const uint64_t gid = A.gid0 + (uint64_t)env;
    const bool last = it == X.iterations - 1;
    double *const S = W.score + env * X.paths;

    double smax = -__builtin_huge_val();
    for (int p = tid; p < W.splits; p += blockDim.x) {
        const double s = W.part_max[env * W.splits + p];
        if (s > smax) smax = s;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(smax, m);
        if (os > smax) smax = os;
    }
    if (ln == 0) red_s[wv] = smax;
    __syncthreads();
    for (int w = 0; w < waves; ++w)
        if (red_s[w] > smax) smax = red_s[w];
    // weights over this part's scores
    for (int c = lo + tid; c < hi; c += blockDim.x) {
        const double w = exp((S[c] - smax) / X.lambda);
        S[c] = w == w ? w : 0.0;                          // NaN score, or no finite Smax
    }
    __syncthreads();
    // lanes over h, waves over c (the last iteration's candidates leave here: rows of float4, coalesced over h)
    for (int h = ln; h < X.horizon; h += kTile) {
        const float4 u = W.U[env * X.horizon + h];
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0, sw = 0.0;
#pragma clang loop unroll(disable)
        for (int c = lo + wv; c < hi; c += waves) {
            const double w = S[c];
            float a[4];
            mppi_action(X, A.rc.seed, gid, k, it, c, h, u, a);
            if (last && X.candidates)
                reinterpret_cast<float4 *>(X.candidates)[(env * X.paths + c) * X.horizon + h] = make_float4(a[0], a[1], a[2], a[3]);
            acc0 = fma(w, (double)a[0], acc0); acc1 = fma(w, (double)a[1], acc1);
            acc2 = fma(w, (double)a[2], acc2); acc3 = fma(w, (double)a[3], acc3);
            sw += w;
        }
        double *p = part_acc + ((size_t)wv * X.horizon + h) * 4;
        p[0] = acc0; p[1] = acc1; p[2] = acc2; p[3] = acc3;
        if (h == 0) red_w[wv] = sw;
    }
    __syncthreads();
    for (int h = tid; h < X.horizon; h += blockDim.x) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, sw = 0.0;
        for (int w = 0; w < waves; ++w) {
            const double *p = part_acc + ((size_t)w * X.horizon + h) * 4;
            t0 += p[0]; t1 += p[1]; t2 += p[2]; t3 += p[3];
            sw += red_w[w];
        }
        out[h * 4 + 0] = t0; out[h * 4 + 1] = t1; out[h * 4 + 2] = t2; out[h * 4 + 3] = t3;
        if (h == 0) out[words - 1] = sw;
    }
}

__global__ __launch_bounds__(kTile) void k_pathint_part_finish(StepArgs A, MppiArgs X, MppiPartArgs W)
{
    const int64_t env = blockIdx.x;                       // < A.n: the grid is n workgroups of one wave
    const int lane = threadIdx.x;
    const int it = W.it;
    const int words = X.horizon * 4 + 1;
    const bool last = it == X.iterations - 1;
    QS_ASSERT(env < A.n && env / kTile < A.tile_end);
    const double *const sums = W.part_sum + env * W.splits * words;

    for (int h = lane; h < X.horizon; h += kTile) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, sw = 0.0;
        for (int p = 0; p < W.splits; ++p) {              // part order; every lane forms the same sum of weights
            const double *s = sums + (int64_t)p * words;
            t0 += s[h * 4 + 0]; t1 += s[h * 4 + 1]; t2 += s[h * 4 + 2]; t3 += s[h * 4 + 3];
            sw += s[words - 1];
        }
        float4 u = W.U[env * X.horizon + h];
        if (sw > 0.0) u = make_float4((float)(t0 / sw), (float)(t1 / sw), (float)(t2 / sw), (float)(t3 / sw));
        W.U[env * X.horizon + h] = u;
        if (X.trace) reinterpret_cast<float4 *>(X.trace)[(env * (X.iterations + 1) + it + 1) * X.horizon + h] = u;
        if (last) {
            if (h == 0) reinterpret_cast<float4 *>(X.actions)[env] = u;
            reinterpret_cast<float4 *>(X.nominal_out)[env * X.horizon + h] = u;
        }
    }
    if (last && X.best_score) {
        double smax = -__builtin_huge_val();
        for (int p = lane; p < W.splits; p += kTile) {
            const double s = W.part_max[env * W.splits + p];
            if (s > smax) smax = s;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double os = __shfl_xor(smax, m);
            if (os > smax) smax = os;
        }
        if (lane == 0) X.best_score[env] = smax;
    }
}

}  // namespace
