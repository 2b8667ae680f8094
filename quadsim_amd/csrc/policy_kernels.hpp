// policy_kernels.hpp -- the actor in the loop: the MLP alone (k_policy_forward), T steps of  a = clip(MLP(obs)); env.step(a)
// (k_policy_rollout), and K complete episodes per env (k_policy_evaluate), each on exact-f32 MFMA and, `_fast`, on split bf16.
// A fragment of quadsim_hip.hip (ONE translation unit), included there right after layer1_kernels.hpp, nowhere else.
#pragma once

namespace {

// The actor of one workgroup: what its LDS holds, how the weights get there, and the MLP of the calling wave.  Every kernel here
// declares the LDS, stages, __syncthreads, and then each wave runs its loop on its 64-env tile, calling the actor once per step.
//   kLdsBytes                 the kernel declares  __shared__ __attribute__((aligned(16))) char lds[Actor<FAST>::kLdsBytes]
//   Actor(lds)                the carve, for the calling wave (its obs / action stages)
//   stage(weights)            weights -> LDS, by the 256 threads of the workgroup; the caller's __syncthreads follows
//   operator()(obs, a, lane)  a = clip(MLP(obs), -1, 1) for the 64 envs of the calling wave (wave barriers only)
template <bool FAST> struct Actor;

// exact f32 (mlp_actor, v_mfma_f32_16x16x4_f32; mlp.hpp).  LDS image (policy_lds_floats()): W2^T | W3^T (16-row tile) | W1^T |
// b1 | b2 | b3 (16) | per-wave obs / action staging
template <>
struct Actor<false> {
    static constexpr size_t kLdsBytes = policy_lds_floats() * sizeof(float);
    float *W2, *W3, *W1, *B1, *B2, *B3, *sObs, *sAct;

    __device__ __forceinline__ explicit Actor(char *lds)
    {
        const int w = threadIdx.x >> 6;
        W2 = reinterpret_cast<float *>(lds);
        W3 = W2 + kHid * kLdW;
        W1 = W3 + 16 * kLdW;
        B1 = W1 + kHid * kLdW1;
        B2 = B1 + kHid;
        B3 = B2 + kHid;
        sObs = B3 + 16 + w * (12 * 64);
        sAct = B3 + 16 + 4 * (12 * 64) + w * (64 * 4);
    }

    // W2^T | W3^T | W1^T | biases -> LDS (W3^T rows 4..15 and b3[4..15] are zero padding of the 16-row MFMA tile) in two passes of
    // 8 float4 per thread: all requests of a pass go out before its first LDS write (a copy loop of load / wait / write pairs
    // costs a launch with T = 1 one L2 round trip per iteration).  Named registers, no arrays: the compiler keeps a staging array
    // as a stack object (16 float4 in one pass gave k_policy_rollout a 272-byte private segment; 8 were moved to 32 KiB of LDS)
    __device__ __forceinline__ void stage(const MlpArgs &M) const
    {
        static_assert(kHid == 128 && kBlock == 256 && kLdW % 4 == 0, "staging layout");
        const float4 *w2v = reinterpret_cast<const float4 *>(M.wt2);
        const int tid = threadIdx.x;
        auto put2 = [&](int j, const float4 &v) {                                                     // 4 096 float4: row i4 >> 5
            const int i4 = j * kBlock + tid;
            *reinterpret_cast<float4 *>(W2 + (i4 >> 5) * kLdW + (i4 & 31) * 4) = v;
        };
#pragma unroll
        for (int h = 0; h < 16; h += 8) {
            const float4 v0 = w2v[(h + 0) * kBlock + tid], v1 = w2v[(h + 1) * kBlock + tid], v2 = w2v[(h + 2) * kBlock + tid],
                         v3 = w2v[(h + 3) * kBlock + tid], v4 = w2v[(h + 4) * kBlock + tid], v5 = w2v[(h + 5) * kBlock + tid],
                         v6 = w2v[(h + 6) * kBlock + tid], v7 = w2v[(h + 7) * kBlock + tid];
            put2(h + 0, v0); put2(h + 1, v1); put2(h + 2, v2); put2(h + 3, v3);
            put2(h + 4, v4); put2(h + 5, v5); put2(h + 6, v6); put2(h + 7, v7);
        }
        // W3^T: 128 float4 of [4][128], then zero rows 4..15 of the 16-row tile (a `cond ? load : zero` here became a select of
        // two addresses, one of them a stack copy of the zero)
        float4 w3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (tid < 128) w3 = reinterpret_cast<const float4 *>(M.wt3)[tid];
        const float u0 = M.wt1[tid], u1 = M.wt1[kBlock + tid], u2 = M.wt1[2 * kBlock + tid],              // 1 536 floats
                    u3 = M.wt1[3 * kBlock + tid], u4 = M.wt1[4 * kBlock + tid], u5 = M.wt1[5 * kBlock + tid];
        float vb1 = 0.0f, vb2 = 0.0f, vb3 = 0.0f;
        if (tid < kHid) { vb1 = M.b1[tid]; vb2 = M.b2[tid]; }
        if (tid < 4) vb3 = M.b3[tid];
        *reinterpret_cast<float4 *>(W3 + (tid >> 5) * kLdW + (tid & 31) * 4) = w3;                     // rows 0..7
        *reinterpret_cast<float4 *>(W3 + (8 + (tid >> 5)) * kLdW + (tid & 31) * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        auto put1 = [&](int j, float v) { const int i = j * kBlock + tid; W1[(i / 12) * kLdW1 + (i % 12)] = v; };
        put1(0, u0); put1(1, u1); put1(2, u2); put1(3, u3); put1(4, u4); put1(5, u5);
        if (tid < kHid) { B1[tid] = vb1; B2[tid] = vb2; }
        if (tid < 16) B3[tid] = vb3;
    }

    __device__ __forceinline__ void operator()(const float o[12], float a[4], int lane) const
    {
        mlp_actor(o, a, W1, B1, W2, B2, W3, B3, sObs, sAct, lane);
    }
};

// the bf16 matrix rate with split (hi + lo) operands (mlp_actor_fast; mlp.hpp, "Fast actor"): LDS = the host-packed weight image
// (pack_fast_weights, kFastBlobBytes) | per-wave obs / action staging
template <>
struct Actor<true> {
    static constexpr size_t kLdsBytes = kFastBlobBytes + 4 * (12 * 64 + 64 * 4) * sizeof(float);
    char *lds;
    float *sObs, *sAct;

    __device__ __forceinline__ explicit Actor(char *lds_) : lds(lds_)
    {
        const int w = threadIdx.x >> 6;
        float *const stages = reinterpret_cast<float *>(lds + kFastBlobBytes);
        sObs = stages + w * (12 * 64);
        sAct = stages + 4 * (12 * 64) + w * (64 * 4);
    }

    // the weight image verbatim into LDS: all requests first, then the LDS writes
    __device__ __forceinline__ void stage(const uint4 *__restrict__ blob) const
    {
        constexpr int kN16 = kFastBlobBytes / 16, kPer = (kN16 + kBlock - 1) / kBlock;
        uint4 v[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = j * kBlock + threadIdx.x;
            v[j] = i < kN16 ? blob[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = j * kBlock + threadIdx.x;
            if (i < kN16) reinterpret_cast<uint4 *>(lds)[i] = v[j];
        }
    }

    __device__ __forceinline__ void operator()(const float o[12], float a[4], int lane) const
    {
        mlp_actor_fast(o, a, lds, sObs, sAct, lane);
    }
};

// row `row` of obs [n,12]; rows past n read as zeros (MFMA needs the whole wave)
__device__ __forceinline__ void load_obs_row(const float *__restrict__ obs, int64_t row, int64_t n, float o[12])
{
    if (row < n) {
        const float4 *p = reinterpret_cast<const float4 *>(obs + row * 12);
        const float4 v0 = p[0], v1 = p[1], v2 = p[2];
        o[0] = v0.x; o[1] = v0.y; o[2] = v0.z; o[3] = v0.w; o[4] = v1.x; o[5] = v1.y; o[6] = v1.z; o[7] = v1.w;
        o[8] = v2.x; o[9] = v2.y; o[10] = v2.z; o[11] = v2.w;
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = 0.0f;
    }
}

// The actor alone: actions [n,4] = clip(MLP(obs [n,12])) on the matrix cores -- model.predict(obs, deterministic=True) of
// run_trained_docking_ppo2.py:41 for n rows, for loops that need the env step as a call of its own (terminal observations,
// infos).  One wave per 64 rows; the same actor as the fused kernels, hence the same bits for the same observations.
template <bool FAST>
__device__ __forceinline__ void policy_forward_rows(const float *__restrict__ obs, float *__restrict__ actions, int64_t n, const Actor<FAST> &actor)
{
    const TileLane w = tile_lane(n);
    float o[12], a[4];
    load_obs_row(obs, w.env, n, o);
    actor(o, a, w.lane);
    if (w.active) reinterpret_cast<float4 *>(actions)[w.env] = make_float4(a[0], a[1], a[2], a[3]);
}

__global__ __launch_bounds__(kBlock, 1) void k_policy_forward(MlpArgs M, const float *__restrict__ obs, float *__restrict__ actions, int64_t n)
{
    __shared__ __attribute__((aligned(16))) char lds[Actor<false>::kLdsBytes];
    const Actor<false> actor(lds);
    actor.stage(M);
    __syncthreads();
    policy_forward_rows(obs, actions, n, actor);
}

__global__ __launch_bounds__(kBlock, 1) void k_policy_forward_fast(const uint4 *__restrict__ blob, const float *__restrict__ obs,
                                                                   float *__restrict__ actions, int64_t n)
{
    __shared__ __attribute__((aligned(16))) char lds[Actor<true>::kLdsBytes];
    const Actor<true> actor(lds);
    actor.stage(blob);
    __syncthreads();
    policy_forward_rows(obs, actions, n, actor);
}

// Policy-in-the-loop roll-out: T steps of  a = clip(MLP(obs));  obs, r, done = env.step(a)  in one launch
// (run_trained_docking_ppo2.py:37-60 for N envs).  The env step = the device code of k_env; obs_0 is derived from the stored
// state (an observation is always state2rel of the state).  The step loop of one wave.
template <int INTEG, int RMODE, bool FAST>
__device__ __forceinline__ void policy_rollout_steps(const StepArgs &A, float *__restrict__ actions_out, const Actor<FAST> &actor)
{
    const auto [lane, tile, env, active] = tile_lane(A.n);
    Env e;
    load_env_or_nominal(A, tile, lane, active, e);
    Par P = A.par_nom;
    const uint64_t k0 = active ? step_counter_begin(A, tile) : 0;
    float obs[12];
    rel_obs(e.sc, e.st, obs);
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < A.T; ++t) {
        float a[4];
        actor(obs, a, lane);
        float reward;
        unsigned flags;
        bool done;
        step_and_maybe_reset<INTEG, false, RMODE>(e, P, a, A, active ? env : 0, k0 + (uint64_t)t, obs, reward, flags, done, false);
        if (active) {
            const int64_t o = t * A.n + env;
            store_obs(A.obs, o, obs);
            A.reward[o] = reward;
            A.done[o] = done ? 1 : 0;
            if (A.flags) A.flags[o] = (uint8_t)flags;
            if (actions_out) reinterpret_cast<float4 *>(actions_out)[o] = make_float4(a[0], a[1], a[2], a[3]);
        }
    }
    if (active) { store_env(A.st, tile, lane, e); step_counter_end(A, tile, lane, k0); }
}

template <int INTEG, int RMODE>
__global__ __launch_bounds__(kBlock, 1) void k_policy_rollout(StepArgs A, MlpArgs M, float *__restrict__ actions_out)
{
    __shared__ __attribute__((aligned(16))) char lds[Actor<false>::kLdsBytes];
    const Actor<false> actor(lds);
    actor.stage(M);
    __syncthreads();
    policy_rollout_steps<INTEG, RMODE>(A, actions_out, actor);
}

template <int INTEG, int RMODE>
__global__ __launch_bounds__(kBlock, 1) void k_policy_rollout_fast(StepArgs A, const uint4 *__restrict__ blob, float *__restrict__ actions_out)
{
    __shared__ __attribute__((aligned(16))) char lds[Actor<true>::kLdsBytes];
    const Actor<true> actor(lds);
    actor.stage(blob);
    __syncthreads();
    policy_rollout_steps<INTEG, RMODE>(A, actions_out, actor);
}

// ---- deterministic evaluation over K complete episodes per env in one launch (qs_policy_evaluate / _fast) -------------------
// The skeleton of k_policy_rollout: the actor's weights in LDS, one wave per 64-env tile, the env state in registers, the env
// step = step_and_maybe_reset (the step API's device code, auto-reset included, with its Philox keys (gid0 + env, k0 + t + 1)).
// What differs: the only global stores are the episode records and finished[]; the state, the per-env parameters and the step
// counter are read and never written back (evaluating twice gives the same episodes, and the handle steps on afterwards as if
// nothing had happened); a wave leaves its loop as soon as all its lanes hold K records, so the step loop has no workgroup
// barrier -- the waves of a workgroup end independently.
struct EvalArgs {
    double *ret;           // [K, n]: sum of the episode's float32 step rewards, added in step order in float64
    int32_t *len;          // [K, n]: steps of the episode
    uint8_t *flags;        // nullable [K, n]: OR of the episode's step flags
    int32_t *docked;       // nullable [K, n]: steps with FLAG_DOCKED
    int32_t *finished;     // [n]: episodes completed (<= K)
    int64_t max_steps;     // steps per env at most
    int32_t K;             // episodes per env
};

// one lane's episode accounting, shared by every evaluation kernel (the actor's here, the expert's in expert_rollout.hpp)
struct EpisodeAcc {
    double ret = 0.0;
    int32_t len = 0, docked = 0;
    unsigned fl = 0;
    int32_t ep;                // episodes recorded; a lane is finished at K

    __device__ __forceinline__ explicit EpisodeAcc(int32_t first) : ep(first) {}
    // wave-uniform: every lane of the tile is finished
    __device__ __forceinline__ bool all_finished(const EvalArgs &E) const { return __builtin_amdgcn_ballot_w64(ep < E.K) == 0; }
    // one step of env `env` of n; at `done` the episode's record goes to row ep of the [K, n] arrays
    __device__ __forceinline__ void add(const EvalArgs &E, int64_t n, int64_t env, float reward, unsigned flags, bool done)
    {
        if (ep >= E.K) return;
        ret += (double)reward;
        ++len;
        fl |= flags;
        docked += (flags & FLAG_DOCKED) ? 1 : 0;
        if (done) {
            const int64_t o = (int64_t)ep * n + env;
            QS_ASSERT(o >= 0 && o < (int64_t)E.K * n);
            E.ret[o] = ret;
            E.len[o] = len;
            if (E.flags) E.flags[o] = (uint8_t)fl;
            if (E.docked) E.docked[o] = docked;
            ret = 0.0; len = 0; docked = 0; fl = 0;
            ++ep;
        }
    }
    __device__ __forceinline__ void finish(const EvalArgs &E, int64_t env) const { E.finished[env] = ep; }
};

// the episode loop of one wave
template <int INTEG, bool PARAMS, int RMODE, bool FAST>
__device__ __forceinline__ void eval_episodes(const StepArgs &A, const EvalArgs &E, const Actor<FAST> &actor)
{
    const auto [lane, tile, env, active] = tile_lane(A.n);   // MFMA needs the whole wave: idle lanes carry a nominal env, record nothing
    Env e;
    load_env_or_nominal(A, tile, lane, active, e);
    // PARAMS: idle lanes read tile 0's parameters (they record nothing); a Par picked from A.par_nom or the loaded one by
    // `active` lived in a stack object in the RMODE 2 kernels
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, active ? tile : 0, lane);
    const uint64_t k0 = active ? step_counter_begin(A, tile) : 0;
    float obs[12];
    rel_obs(e.sc, e.st, obs);
    EpisodeAcc acc(active ? 0 : E.K);
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < E.max_steps; ++t) {
        if (acc.all_finished(E)) break;
        float a[4];
        actor(obs, a, lane);
        float reward;
        unsigned flags;
        bool done;
        step_and_maybe_reset<INTEG, PARAMS, RMODE>(e, P, a, A, active ? env : 0, k0 + (uint64_t)t, obs, reward, flags, done, false);
        acc.add(E, A.n, env, reward, flags, done);
    }
    if (active) acc.finish(E, env);
}

template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock, 1) void k_policy_evaluate(StepArgs A, MlpArgs M, EvalArgs E)
{
    __shared__ __attribute__((aligned(16))) char lds[Actor<false>::kLdsBytes];
    const Actor<false> actor(lds);
    actor.stage(M);
    __syncthreads();
    eval_episodes<INTEG, PARAMS, RMODE>(A, E, actor);
}

template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock, 1) void k_policy_evaluate_fast(StepArgs A, const uint4 *__restrict__ blob, EvalArgs E)
{
    __shared__ __attribute__((aligned(16))) char lds[Actor<true>::kLdsBytes];
    const Actor<true> actor(lds);
    actor.stage(blob);
    __syncthreads();
    eval_episodes<INTEG, PARAMS, RMODE>(A, E, actor);
}

}  // namespace
