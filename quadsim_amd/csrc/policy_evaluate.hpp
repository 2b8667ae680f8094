// policy_evaluate.hpp -- deterministic evaluation of the actor over K complete episodes per env in one launch
// (qs_policy_evaluate / _fast).  A fragment of quadsim_hip.hip, included right after step_kernels.hpp, nowhere else.
//
// The skeleton of k_policy_rollout: the actor's weights in LDS, one wave per 64-env tile, the env state in registers, the env
// step = step_and_maybe_reset (the step API's device code, auto-reset included, with its Philox keys (gid0 + env, k0 + t + 1)).
// What differs: the only global stores are the episode records and finished[]; the state, the per-env parameters and the step
// counter are read and never written back (evaluating twice gives the same episodes, and the handle steps on afterwards as if
// nothing had happened); a wave leaves its loop as soon as all its lanes hold K records, so the step loop has no workgroup
// barrier -- the waves of a workgroup end independently.
#pragma once

namespace {

struct EvalArgs {
    double *ret;           // [K, n]: sum of the episode's float32 step rewards, added in step order in float64
    int32_t *len;          // [K, n]: steps of the episode
    uint8_t *flags;        // nullable [K, n]: OR of the episode's step flags
    int32_t *docked;       // nullable [K, n]: steps with FLAG_DOCKED
    int32_t *finished;     // [n]: episodes completed (<= K)
    int64_t max_steps;     // steps per env at most
    int32_t K;             // episodes per env
};

// W2^T | W3^T | W1^T | biases -> LDS (the image of mlp_stage_weights) in two passes of 8 float4 per thread: all requests of a
// pass go out before its first LDS write.  Named registers, no arrays: the compiler keeps a staging array as a stack object
// (mlp_stage_weights' 16 float4 give k_policy_rollout a 272-byte private segment; 8 of them here were moved to 32 KiB of LDS)
__device__ __forceinline__ void eval_stage_weights(const MlpArgs &M, const MlpLds &L)
{
    static_assert(kHid == 128 && kBlock == 256 && kLdW % 4 == 0, "staging layout");
    const float4 *w2v = reinterpret_cast<const float4 *>(M.wt2);
    const int tid = threadIdx.x;
    auto put2 = [&](int j, const float4 &v) {                                                     // 4 096 float4: row i4 >> 5
        const int i4 = j * kBlock + tid;
        *reinterpret_cast<float4 *>(L.W2 + (i4 >> 5) * kLdW + (i4 & 31) * 4) = v;
    };
#pragma unroll
    for (int h = 0; h < 16; h += 8) {
        const float4 v0 = w2v[(h + 0) * kBlock + tid], v1 = w2v[(h + 1) * kBlock + tid], v2 = w2v[(h + 2) * kBlock + tid],
                     v3 = w2v[(h + 3) * kBlock + tid], v4 = w2v[(h + 4) * kBlock + tid], v5 = w2v[(h + 5) * kBlock + tid],
                     v6 = w2v[(h + 6) * kBlock + tid], v7 = w2v[(h + 7) * kBlock + tid];
        put2(h + 0, v0); put2(h + 1, v1); put2(h + 2, v2); put2(h + 3, v3);
        put2(h + 4, v4); put2(h + 5, v5); put2(h + 6, v6); put2(h + 7, v7);
    }
    // W3^T: 128 float4 of [4][128], then zero rows 4..15 of the 16-row tile (a `cond ? load : zero` here became a select of two
    // addresses, one of them a stack copy of the zero)
    float4 w3 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tid < 128) w3 = reinterpret_cast<const float4 *>(M.wt3)[tid];
    const float u0 = M.wt1[tid], u1 = M.wt1[kBlock + tid], u2 = M.wt1[2 * kBlock + tid],              // 1 536 floats
                u3 = M.wt1[3 * kBlock + tid], u4 = M.wt1[4 * kBlock + tid], u5 = M.wt1[5 * kBlock + tid];
    float vb1 = 0.0f, vb2 = 0.0f, vb3 = 0.0f;
    if (tid < kHid) { vb1 = M.b1[tid]; vb2 = M.b2[tid]; }
    if (tid < 4) vb3 = M.b3[tid];
    *reinterpret_cast<float4 *>(L.W3 + (tid >> 5) * kLdW + (tid & 31) * 4) = w3;                     // rows 0..7
    *reinterpret_cast<float4 *>(L.W3 + (8 + (tid >> 5)) * kLdW + (tid & 31) * 4) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    auto put1 = [&](int j, float v) { const int i = j * kBlock + tid; L.W1[(i / 12) * kLdW1 + (i % 12)] = v; };
    put1(0, u0); put1(1, u1); put1(2, u2); put1(3, u3); put1(4, u4); put1(5, u5);
    if (tid < kHid) { L.B1[tid] = vb1; L.B2[tid] = vb2; }
    if (tid < 16) L.B3[tid] = vb3;
}

// the episode loop of one wave; actor(obs, a, lane) = the MLP of the kernel (mlp_actor / mlp_actor_fast: wave barriers only)
template <int INTEG, bool PARAMS, int RMODE, class Actor>
__device__ __forceinline__ void eval_episodes(const StepArgs &A, const EvalArgs &E, Actor &&actor)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    const bool active = env < A.n;             // MFMA needs the whole wave: idle lanes carry a nominal env, record nothing
    Env e;
    load_env_or_nominal(A, tile, lane, active, e);
    // PARAMS: idle lanes read tile 0's parameters (they record nothing); a Par picked from A.par_nom or the loaded one by
    // `active` lived in a stack object in the RMODE 2 kernels
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, active ? tile : 0, lane);
    const uint64_t k0 = active ? step_counter_begin(A, tile) : 0;
    float obs[12];
    rel_obs(e.sc, e.st, obs);
    double ret = 0.0;
    int32_t len = 0, docked = 0;
    unsigned fl = 0;
    int32_t ep = active ? 0 : E.K;             // episodes recorded; a lane is finished at K
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < E.max_steps; ++t) {
        if (__builtin_amdgcn_ballot_w64(ep < E.K) == 0) break;      // wave-uniform: every lane of the tile is finished
        float a[4];
        actor(obs, a, lane);
        float reward;
        unsigned flags;
        bool done;
        step_and_maybe_reset<INTEG, PARAMS, RMODE>(e, P, a, A, active ? env : 0, k0 + (uint64_t)t, obs, reward, flags, done, false);
        if (ep < E.K) {
            ret += (double)reward;
            ++len;
            fl |= flags;
            docked += (flags & FLAG_DOCKED) ? 1 : 0;
            if (done) {
                const int64_t o = (int64_t)ep * A.n + env;
                QS_ASSERT(o >= 0 && o < (int64_t)E.K * A.n);
                E.ret[o] = ret;
                E.len[o] = len;
                if (E.flags) E.flags[o] = (uint8_t)fl;
                if (E.docked) E.docked[o] = docked;
                ret = 0.0; len = 0; docked = 0; fl = 0;
                ++ep;
            }
        }
    }
    if (active) E.finished[env] = ep;
}

// exact-f32 actor (mlp_actor, v_mfma_f32_16x16x4_f32): the LDS image of k_policy_rollout
template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock, 1) void k_policy_evaluate(StepArgs A, MlpArgs M, EvalArgs E)
{
    __shared__ __attribute__((aligned(16))) float lds[policy_lds_floats()];
    const MlpLds L = mlp_lds_layout(lds);
    eval_stage_weights(M, L);
    __syncthreads();
    const int w = threadIdx.x >> 6;
    float *const sObs = L.ObsAll + w * (12 * 64), *const sAct = L.ActAll + w * (64 * 4);
    eval_episodes<INTEG, PARAMS, RMODE>(A, E, [&](const float o[12], float a[4], int lane) {
        mlp_actor(o, a, L.W1, L.B1, L.W2, L.B2, L.W3, L.B3, sObs, sAct, lane);
    });
}

// split-bf16 actor (mlp_actor_fast): the LDS image of k_policy_rollout_fast, `blob` = pack_fast_weights' image
template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock, 1) void k_policy_evaluate_fast(StepArgs A, const uint4 *__restrict__ blob, EvalArgs E)
{
    __shared__ __attribute__((aligned(16))) char lds[kFastBlobBytes + 4 * (12 * 64 + 64 * 4) * 4];
    mlp_stage_blob(blob, lds);
    __syncthreads();
    const int w = threadIdx.x >> 6;
    float *const stage = reinterpret_cast<float *>(lds + kFastBlobBytes);
    float *const sObs = stage + w * (12 * 64), *const sAct = stage + 4 * (12 * 64) + w * (64 * 4);
    eval_episodes<INTEG, PARAMS, RMODE>(A, E, [&](const float o[12], float a[4], int lane) {
        mlp_actor_fast(o, a, lds, sObs, sAct, lane);
    });
}

// one launch; called through with_combo (quadsim_hip.hip), so for the step kernels' combinations and no other
template <int INTEG, bool PARAMS, int RMODE>
void eval_launch(hipStream_t s, unsigned grid, const StepArgs &A, const MlpArgs *M, const uint4 *blob, const EvalArgs &E)
{
    if (blob) hipLaunchKernelGGL((k_policy_evaluate_fast<INTEG, PARAMS, RMODE>), dim3(grid), dim3(kBlock), 0, s, A, blob, E);
    else hipLaunchKernelGGL((k_policy_evaluate<INTEG, PARAMS, RMODE>), dim3(grid), dim3(kBlock), 0, s, A, *M, E);
}

}  // namespace
