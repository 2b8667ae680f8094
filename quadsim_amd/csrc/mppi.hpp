// mppi.hpp -- MPPI planner (qs_mppi_plan): model-predictive path integral control on the exact env.  `iterations` refinement
// rounds in ONE launch: `paths` Gaussian candidates around a nominal action sequence are rolled through the env from its CURRENT
// state and scored as k_shooting_plan scores them, then the nominal becomes their softmax-weighted mean.  The nominal goes in
// and comes out (warm start); the closed loop stays in Python.  Read-only on the handle.  A fragment of quadsim_hip.hip,
// included right after shooting.hpp, nowhere else.
//
// Mapping: ONE WORKGROUP PER ENV (blockIdx.x = env), as k_shooting_plan: the env record, its parameters and its step counter
// are wave-uniform loads; the block is min(256, paths rounded up to a wave) threads.
//   1. Wave 0 integrates the TARGET `horizon` steps into LDS rows (13 state words + target-limited bit), once for all iterations.
//   2. The nominal U[h] = nominal_in[env][min(h + shift, horizon - 1)] (zeros without nominal_in) is read into LDS before
//      anything is written, so nominal_in may alias nominal_out.
//   3. Per iteration:
//      roll-out  lane j takes candidates c = j, j + blockDim, ...: a[c][h] = clamp(fma(sigma, z, U[h]), -1, 1) (c = 0: the
//                nominal itself, no draw), env_step_chaser against the LDS target row, the float64 score of k_shooting_plan
//                (both objectives, stop after the first done step, no reset) into LDS;
//      weights   Smax over the non-NaN scores (shuffles, then the <= 4 waves in LDS); w[c] = exp((S[c] - Smax) / lambda) in
//                float64 overwrites S[c]; a NaN gives 0;
//      update    lanes over h, waves over c: wave v adds w[c] a[c][h] for c = v, v + waves, ... in ascending order into four
//                float64 sums (the candidates' actions are regenerated from their keys or re-read from `noise`, never stored;
//                w[c] is an LDS broadcast read), then lane h adds the per-wave partial sums in wave order and divides by the
//                sum of the weights, formed in the same order.  The order is a function of (paths, block size) alone: the
//                result does not depend on N, the env index or the launch path.  No positive weight (every score NaN): U stays.
//   4. nominal_out = U, actions = U[0], best_score = the last iteration's Smax.
// Keyed draw: z = Box-Muller (normals_from_words: random_normal4's arithmetic and word pairing) of Philox4x32-10 block
//   (1 << 63) | (k << 30) | (it << 26) | (c << 10) | h of subsequence (STREAM_PLAN << 48) | gid.  qs_shooting_plan's blocks are
//   below 2^62, so the two planners never share a block; a plan repeated at the same k is reproducible; candidate c of
//   iteration `it` does not depend on `paths`; the first j iterations of a call with more are the call with iterations = j.
//   philox_block() cannot express these blocks (rocRAND's offset is 4 x block in 64 bits), so the counter is set directly.
#pragma once

namespace {

struct MppiArgs {
    int horizon, paths, iterations, objective, shift;
    double lambda;                   // the caller's float, widened on the host
    float sigma;
    const float *nominal_in;         // nullable [n,horizon,4]
    const float *noise;              // nullable [iterations,paths,horizon,4]
    float *actions;                  // [n,4]
    float *nominal_out;              // [n,horizon,4]
    double *best_score;              // nullable [n]
    double *scores;                  // nullable [n,iterations,paths]
    float *trace;                    // nullable [n,iterations+1,horizon,4]
    float *candidates;               // nullable [n,paths,horizon,4]
};

constexpr int kMppiHeadBytes = 64;   // per-wave Smax [4], per-wave sum of weights [4]
// head | per-wave partial sums [4][horizon][4] f64 | nominal [horizon] float4 | scores / weights [paths] f64 | target rows
inline size_t mppi_lds_bytes(int horizon, int paths)
{
    return kMppiHeadBytes + (size_t)horizon * (4 * 4 * sizeof(double) + 4 * sizeof(float) + kPlanRowWords * sizeof(float))
           + (size_t)paths * sizeof(double);
}

// philox_counter (the 128-bit counter given directly) and clamp1 are quadsim_device.hpp's, shared with the planner over the
// learned net (dynmppi_kernels.hpp).
//
// actions of candidate c at horizon step h in iteration `it`, around the nominal u (k < 2^33, it < 2^4, c < 2^16, h < 2^10)
__device__ __forceinline__ void mppi_action(const MppiArgs &X, uint64_t seed, uint64_t gid, uint64_t k, int it, int c, int h,
                                            const float4 &u, float a[4])
{
    float z[4];
    const float s = X.sigma;
    if (c == 0) {                                         // the nominal itself, no draw
        a[0] = clamp1(u.x); a[1] = clamp1(u.y); a[2] = clamp1(u.z); a[3] = clamp1(u.w);
        return;
    }
    if (X.noise) {
        const float4 v = reinterpret_cast<const float4 *>(X.noise)[((int64_t)it * X.paths + c) * X.horizon + h];
        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
    } else {
        const uint64_t blk = (1ull << 63) | (k << 30) | ((uint64_t)it << 26) | ((uint64_t)c << 10) | (uint64_t)h;
        normals_from_words(philox_counter(seed, (STREAM_PLAN << 48) | gid, blk), z);
    }
    a[0] = clamp1(__fmaf_rn(s, z[0], u.x)); a[1] = clamp1(__fmaf_rn(s, z[1], u.y));
    a[2] = clamp1(__fmaf_rn(s, z[2], u.z)); a[3] = clamp1(__fmaf_rn(s, z[3], u.w));
}

template <int INTEG, bool PARAMS>
__global__ __launch_bounds__(kBlock, 4) void k_mppi(StepArgs A, MppiArgs X)
{
    extern __shared__ __align__(16) unsigned char mppi_lds[];
    double *const red_s = reinterpret_cast<double *>(mppi_lds);                                     // [4]
    double *const red_w = reinterpret_cast<double *>(mppi_lds + 32);                                // [4]
    double *const part = reinterpret_cast<double *>(mppi_lds + kMppiHeadBytes);                     // [4][horizon][4]
    float4 *const U = reinterpret_cast<float4 *>(part + 16 * (size_t)X.horizon);                    // [horizon]
    double *const S = reinterpret_cast<double *>(U + X.horizon);                                    // [paths]
    float *const rows = reinterpret_cast<float *>(S + X.paths);                                     // [horizon][kPlanRowWords]

    const int64_t env = blockIdx.x;                       // < A.n: the grid is n workgroups
    const int64_t tile = env / kTile;
    const int slot = (int)(env % kTile);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int waves = (int)(blockDim.x >> 6);
    QS_ASSERT(env < A.n && tile < A.tile_end);
    const uint64_t k = step_counter_begin(A, tile);
    const uint64_t gid = A.gid0 + (uint64_t)env;
    Env e;
    load_env(A.st, tile, slot, e);
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, slot);

    for (int h = threadIdx.x; h < X.horizon; h += blockDim.x) {
        float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (X.nominal_in) u = reinterpret_cast<const float4 *>(X.nominal_in)[env * X.horizon + min(h + X.shift, X.horizon - 1)];
        U[h] = u;
        if (X.trace) reinterpret_cast<float4 *>(X.trace)[env * (X.iterations + 1) * X.horizon + h] = u;
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
    double smax = -__builtin_huge_val();

#pragma clang loop unroll(disable)
    for (int it = 0; it < X.iterations; ++it) {
        const bool last = it == X.iterations - 1;
        smax = -__builtin_huge_val();
        // the observation before step 0 is the current one, common to all candidates
        float obs0[12];
        rel_obs(e.sc, e.st, obs0);
        const float pos0 = plan_pos(obs0);
        int tid0 = threadIdx.x;                             // opaque as `tid` below, for the same reason
        asm volatile("" : "+v"(tid0));
#pragma clang loop unroll(disable)
        for (int c = tid0; c < X.paths; c += blockDim.x) {
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
        // Everything below is addressed from a thread index the compiler cannot see through: computed from threadIdx.x, the
        // per-lane addresses of the weights, the update and its outputs are hoisted out of the iteration loop and then live
        // in some twenty vector registers across the roll-out, which the RK4 instantiations do not have (no spills at 128).
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int ln = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        for (int c = tid; c < X.paths; c += blockDim.x)
            if (S[c] > smax) smax = S[c];                                     // this thread's own scores; a NaN never enters
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double os = __shfl_xor(smax, m);
            if (os > smax) smax = os;
        }
        if (ln == 0) red_s[wv] = smax;
        __syncthreads();
        for (int w = 0; w < waves; ++w)
            if (red_s[w] > smax) smax = red_s[w];
        // weights over the scores, each by the thread that wrote the score
        for (int c = tid; c < X.paths; c += blockDim.x) {
            const double w = exp((S[c] - smax) / X.lambda);
            S[c] = w == w ? w : 0.0;                                          // NaN score, or no finite Smax
        }
        __syncthreads();
        // pass 2: lanes over h, waves over c (the last iteration's candidates leave here: rows of float4, coalesced over h)
        for (int h = ln; h < X.horizon; h += kTile) {
            const float4 u = U[h];
            double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0, sw = 0.0;
#pragma clang loop unroll(disable)
            for (int c = wv; c < X.paths; c += waves) {
                const double w = S[c];
                float a[4];
                mppi_action(X, A.rc.seed, gid, k, it, c, h, u, a);
                if (last && X.candidates)
                    reinterpret_cast<float4 *>(X.candidates)[(env * X.paths + c) * X.horizon + h] = make_float4(a[0], a[1], a[2], a[3]);
                acc0 = fma(w, (double)a[0], acc0); acc1 = fma(w, (double)a[1], acc1);
                acc2 = fma(w, (double)a[2], acc2); acc3 = fma(w, (double)a[3], acc3);
                sw += w;
            }
            double *p = part + ((size_t)wv * X.horizon + h) * 4;
            p[0] = acc0; p[1] = acc1; p[2] = acc2; p[3] = acc3;
            if (h == 0) red_w[wv] = sw;
        }
        __syncthreads();
        for (int h = tid; h < X.horizon; h += blockDim.x) {
            double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, sw = 0.0;
            for (int w = 0; w < waves; ++w) {
                const double *p = part + ((size_t)w * X.horizon + h) * 4;
                t0 += p[0]; t1 += p[1]; t2 += p[2]; t3 += p[3];
                sw += red_w[w];
            }
            float4 u = U[h];
            if (sw > 0.0) u = make_float4((float)(t0 / sw), (float)(t1 / sw), (float)(t2 / sw), (float)(t3 / sw));
            U[h] = u;
            if (X.trace) reinterpret_cast<float4 *>(X.trace)[(env * (X.iterations + 1) + it + 1) * X.horizon + h] = u;
        }
        __syncthreads();
    }

    for (int h = threadIdx.x; h < X.horizon; h += blockDim.x) {
        const float4 u = U[h];
        if (h == 0) reinterpret_cast<float4 *>(X.actions)[env] = u;
        reinterpret_cast<float4 *>(X.nominal_out)[env * X.horizon + h] = u;
    }
    if (threadIdx.x == 0 && X.best_score) X.best_score[env] = smax;
}

}  // namespace
