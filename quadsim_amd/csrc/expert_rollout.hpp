// expert_rollout.hpp -- the PID expert in the loop: T steps of  a = expert(state); obs', r, done = env.step(a)  in one launch
// (qs_expert_rollout: run_expert_policy.py:49-69 / run_expert_record.py:121-156 for N envs), and K complete expert episodes
// per env, read-only (qs_expert_evaluate).  A fragment of quadsim_hip.hip, included right after policy_evaluate.hpp, nowhere else.
//
// One lane per env, 256 threads = 4 tiles, no LDS, no barrier: the env state (40 words), the per-env parameters and the
// expert's desired state stay in registers from the tile load to the tile store.  The expert = expert_action (the body of
// k_expert_action), the env step = step_and_maybe_reset (the step API's device code, auto-reset included, with its Philox keys
// (gid0 + env, k0 + t + 1)): the same bits as the per-step loop qs_expert_action -> qs_step, which is the definition.  The
// desired state persists across an auto-reset, as it does in that loop.
#pragma once

namespace {

struct ExpertArgs {
    float *state_des;      // [n,13]: in / out (roll-out), read only (evaluation)
    float kp, kd;
    float *actions;        // roll-out: [T,n,4] (env-major: [n,T,4]), not clipped
    float *last_obs;       // roll-out: nullable [n,12], the observation after the last step
    int env_major;         // roll-out: obs / actions rows at env*T + t instead of t*n + env (qs_set_rollout_layout)
};

// words 3..12 of the desired state are all the velocity controller reads; 0..2 (the position) are never read nor written
__device__ __forceinline__ void load_state_des(const float *__restrict__ state_des, int64_t env, float sd[13])
{
    const float *p = state_des + env * 13;
    sd[0] = 0.0f; sd[1] = 0.0f; sd[2] = 0.0f;
#pragma unroll
    for (int i = 3; i < 13; ++i) sd[i] = p[i];
}

template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock) void k_expert_rollout(StepArgs A, ExpertArgs X)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    if (env >= A.n) return;                    // no MFMA, no barrier: idle lanes of the tail tile simply leave
    QS_ASSERT(tile < A.tile_end);
    const uint64_t k0 = step_counter_begin_vmem(A, tile);
    Env e;
    load_env(A.st, tile, lane, e);
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, lane);
    float sd[13];
    load_state_des(X.state_des, env, sd);
    float obs[12];
    rel_obs(e.sc, e.st, obs);                  // = what the preceding qs_step / qs_reset returned (an observation is state2rel of the state)
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < A.T; ++t) {
        const int64_t o = t * A.n + env;
        const int64_t ow = X.env_major ? env * A.T + t : o;
        QS_ASSERT(ow >= 0 && ow < A.T * A.n);
        // the observation BEFORE the step: what the recorder appends (run_expert_record.py:122-123)
        if (X.env_major) store_obs_cached(A.obs, ow, obs); else store_obs(A.obs, ow, obs);
        float a[4];
        expert_action(e.sc, e.st, e.t, P.m, X.kp, X.kd, sd, a);
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4 *const ap = reinterpret_cast<f4 *>(X.actions) + ow;
        if (X.env_major) *ap = f4{a[0], a[1], a[2], a[3]}; else QS_SO(ap, (f4{a[0], a[1], a[2], a[3]}));
        float reward;
        unsigned flags;
        bool done;
        step_and_maybe_reset<INTEG, PARAMS, RMODE>(e, P, a, A, env, k0 + (uint64_t)t, obs, reward, flags, done, false);
        QS_SO(&A.reward[o], reward);
        QS_SO(&A.done[o], (uint8_t)(done ? 1 : 0));
        if (A.flags) QS_SO(&A.flags[o], (uint8_t)flags);
    }
    if (X.last_obs) store_obs(X.last_obs, env, obs);
    store_env(A.st, tile, lane, e);
    if (PARAMS && RMODE == 2) store_par(A.par, tile, lane, P);
    step_counter_end(A, tile, lane, k0);
#pragma unroll
    for (int i = 3; i < 12; ++i) X.state_des[env * 13 + i] = sd[i];
}

// K complete expert episodes per env from the env's CURRENT state (the contract of k_policy_evaluate, policy_evaluate.hpp):
// the only global stores are the episode records and finished[]; a wave leaves as soon as all its lanes hold K records.
template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock) void k_expert_evaluate(StepArgs A, const float *__restrict__ state_des, float kp, float kd, EvalArgs E)
{
    const int lane = threadIdx.x & (kTile - 1);
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + (threadIdx.x >> 6);
    const int64_t env = tile * kTile + lane;
    if (env >= A.n) return;
    const uint64_t k0 = step_counter_begin(A, tile);
    Env e;
    load_env(A.st, tile, lane, e);
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, lane);
    float sd[13];
    load_state_des(state_des, env, sd);
    double ret = 0.0;
    int32_t len = 0, docked = 0, ep = 0;
    unsigned fl = 0;
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < E.max_steps; ++t) {
        if (__builtin_amdgcn_ballot_w64(ep < E.K) == 0) break;      // wave-uniform: every live lane of the tile is finished
        float a[4], obs[12], reward;
        unsigned flags;
        bool done;
        expert_action(e.sc, e.st, e.t, P.m, kp, kd, sd, a);
        step_and_maybe_reset<INTEG, PARAMS, RMODE>(e, P, a, A, env, k0 + (uint64_t)t, obs, reward, flags, done, false);
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
    E.finished[env] = ep;
}

}  // namespace
