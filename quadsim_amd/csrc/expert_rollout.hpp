// expert_rollout.hpp -- the PID expert in the loop: T steps of  a = expert(state); obs', r, done = env.step(a)  in one launch
// (qs_expert_rollout: run_expert_policy.py:49-69 / run_expert_record.py:121-156 for N envs), and K complete expert episodes
// per env, read-only (qs_expert_evaluate).  A fragment of quadsim_hip.hip, included right after runner_kernels.hpp, nowhere else.
//
// One lane per env, 256 threads = 4 tiles, no LDS, no barrier: the env state (40 words), the per-env parameters and the
// expert's desired state stay in registers from the tile load to the tile store.  The expert = expert_action (the body of
// k_expert_action), the env step = step_and_maybe_reset (the step API's device code, auto-reset included, with its Philox keys
// (gid0 + env, k0 + t + 1)): the same bits as the per-step loop qs_expert_action -> qs_step, which is the definition.  The
// desired state persists across an auto-reset, as it does in that loop.
#pragma once

namespace {

// PID expert (run_expert_policy.py:49-69, run_expert_record.py:121-136): vel_controller on the chaser towards
// 0.2 m behind the target, inverse action map (inv(rotor2control) u - mean)/std, not clipped.  sd [13] is the
// expert's persistent desired state (pos = chaser start, vel = des_vel, [6:12] rewritten by the controller).  First
// step of an episode (t == 0) keeps the previous des_vel (:58-59).  The one copy of the expert: k_expert_action and the
// fused kernels below inline it, so they compute the same bits (-ffp-contract=on).
__device__ __forceinline__ void expert_action(const float sc[13], const float tp[3], float t, float m, float kp, float kd,
                                              float sd[13], float act[4])
{
    if (t != 0.0f) {
        sd[3] = kp * (tp[0] - 0.2f - sc[0]) + kd * (-sc[3]);
        sd[4] = kp * (tp[1] - sc[1]) + kd * (-sc[4]);
        sd[5] = kp * (tp[2] - sc[2]) + kd * (-sc[5]);
    }
    const float dv[3] = {0.0f, 0.0f, 0.0f};        // state_last aliases the current state
    float u[4];
    target_control(1, sd, sd + 3, sd + 6, sd[12], sc, dv, m, u);
    sd[10] = 0.0f; sd[11] = 0.0f;
    constexpr float a = 1.0f / (2.0f * kL), bq = 1.0f / (4.0f * kLambda);
    const float f4 = 0.25f * u[0];
    const float f0 = f4 - a * u[2] + bq * u[3], f1 = f4 + a * u[1] - bq * u[3];
    const float f2 = f4 + a * u[2] + bq * u[3], f3 = f4 - a * u[1] - bq * u[3];
    const float inv_mean = q_rcp(0.5f * m * kG);
    act[0] = f0 * inv_mean - 1.0f; act[1] = f1 * inv_mean - 1.0f; act[2] = f2 * inv_mean - 1.0f; act[3] = f3 * inv_mean - 1.0f;
}

// qs_expert_action: reads the envs' current chaser / target state straight from the tiles; state_des [N][13]
template <bool PARAMS>
__global__ __launch_bounds__(kBlock) void k_expert_action(const float *__restrict__ st, const float *__restrict__ par, int64_t n,
                                                          float *__restrict__ state_des, float kp, float kd, Par par_nom,
                                                          float *__restrict__ actions)
{
    const auto [lane, tile, env, active] = tile_lane(n);
    if (!active) return;
    const float *b = st + tile * (int64_t)(kRecWords * kTile) + lane;
    float sc[13], tp[3], sd[13];
    for (int i = 0; i < 13; ++i) sc[i] = b[(F_SC + i) * kTile];
    for (int i = 0; i < 3; ++i) tp[i] = b[(F_ST + i) * kTile];
    const float t = b[F_T * kTile];
    for (int i = 0; i < 13; ++i) sd[i] = state_des[env * 13 + i];
    Par P = par_nom;
    if (PARAMS) P = load_par(par, tile, lane);
    float a[4];
    expert_action(sc, tp, t, P.m, kp, kd, sd, a);
    reinterpret_cast<float4 *>(actions)[env] = make_float4(a[0], a[1], a[2], a[3]);
    for (int i = 3; i < 12; ++i) state_des[env * 13 + i] = sd[i];
}

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
    const auto [lane, tile, env, active] = tile_lane(A.n);
    if (!active) return;                       // no MFMA, no barrier: idle lanes of the tail tile simply leave
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

// K complete expert episodes per env from the env's CURRENT state (the contract of k_policy_evaluate, policy_kernels.hpp):
// the only global stores are the episode records and finished[]; a wave leaves as soon as all its lanes hold K records.
template <int INTEG, bool PARAMS, int RMODE>
__global__ __launch_bounds__(kBlock) void k_expert_evaluate(StepArgs A, const float *__restrict__ state_des, float kp, float kd, EvalArgs E)
{
    const auto [lane, tile, env, active] = tile_lane(A.n);
    if (!active) return;
    const uint64_t k0 = step_counter_begin(A, tile);
    Env e;
    load_env(A.st, tile, lane, e);
    Par P = A.par_nom;
    if (PARAMS) P = load_par(A.par, tile, lane);
    float sd[13];
    load_state_des(state_des, env, sd);
    EpisodeAcc acc(0);
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < E.max_steps; ++t) {
        if (acc.all_finished(E)) break;            // every live lane of the tile
        float a[4], obs[12], reward;
        unsigned flags;
        bool done;
        expert_action(e.sc, e.st, e.t, P.m, kp, kd, sd, a);
        step_and_maybe_reset<INTEG, PARAMS, RMODE>(e, P, a, A, env, k0 + (uint64_t)t, obs, reward, flags, done, false);
        acc.add(E, A.n, env, reward, flags, done);
    }
    acc.finish(E, env);
}

}  // namespace
