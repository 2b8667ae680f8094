// layer1_kernels.hpp -- layers 0 / 1 as batch kernels on row-major user arrays: k_drone_step, k_ctrl, k_transform, k_rel_obs
// A fragment of quadsim_hip.hip (ONE translation unit), included there right after step_kernels.hpp, nowhere else.
#pragma once

namespace {

__global__ __launch_bounds__(kBlock) void k_drone_step(int64_t n, float *state, float *u_prev, const float *u,
                                                       const float *par, uint8_t *limited, Par par_nom, float dt,
                                                       int integ)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float s[13], up[4], uu[4];
    for (int j = 0; j < 13; ++j) s[j] = state[i * 13 + j];
    for (int j = 0; j < 4; ++j) { up[j] = u_prev[i * 4 + j]; uu[j] = u[i * 4 + j]; }
    Par P = par_nom;
    if (par) { P.m = par[i * 4]; P.Ixx = par[i * 4 + 1]; P.Iyy = par[i * 4 + 2]; P.Izz = par[i * 4 + 3]; }
    bool over = integ == 0 ? drone_step<0>(s, up, uu, P, dt) : drone_step<1>(s, up, uu, P, dt);
    for (int j = 0; j < 13; ++j) state[i * 13 + j] = s[j];
    for (int j = 0; j < 4; ++j) u_prev[i * 4 + j] = up[j];
    if (limited) limited[i] = over ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void k_ctrl(int64_t n, int mode, float *state_des, const float *state,
                                                 const float *state_last, float mass, float *u_out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float sd[13], s[13], dv[3] = {0.0f, 0.0f, 0.0f}, u[4];
    for (int j = 0; j < 13; ++j) { sd[j] = state_des[i * 13 + j]; s[j] = state[i * 13 + j]; }
    if (mode == 1 && state_last) for (int j = 0; j < 3; ++j) dv[j] = s[3 + j] - state_last[i * 13 + 3 + j];
    target_control(mode, sd, sd + 3, sd + 6, sd[12], s, dv, mass, u);
    for (int j = 0; j < 4; ++j) { state_des[i * 13 + 6 + j] = sd[6 + j]; u_out[i * 4 + j] = u[j]; }
    state_des[i * 13 + 10] = 0.0f;   // roll_rate_des,  PIDController.py:101
    state_des[i * 13 + 11] = 0.0f;   // pitch_rate_des, PIDController.py:102
}

// layer 0: utils/transform.py as batch functions.  op 0 quat2euler [n,4]->[n,3] (:94-120), 1 euler2quat [n,3]->[n,4]
// (:123-136), 2 quat2rot [n,4]->[n,9] (:4-20), 3 rot2euler [n,9]->[n,3] (:23-46)
__global__ __launch_bounds__(kBlock) void k_transform(int op, int64_t n, const float *in, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (op == 0) {
        float q[4] = {in[i * 4], in[i * 4 + 1], in[i * 4 + 2], in[i * 4 + 3]};
        quat2euler(q, out[i * 3], out[i * 3 + 1], out[i * 3 + 2]);
    } else if (op == 1) {
        float q[4];
        euler2quat(in[i * 3], in[i * 3 + 1], in[i * 3 + 2], q);
        for (int j = 0; j < 4; ++j) out[i * 4 + j] = q[j];
    } else if (op == 2) {
        float q[4] = {in[i * 4], in[i * 4 + 1], in[i * 4 + 2], in[i * 4 + 3]};
        Rot R = quat2rot(q);
        const float r[9] = {1.0f, R.r01, R.r02, R.r10, 1.0f, R.r12, R.r20, R.r21, 1.0f};
        for (int j = 0; j < 9; ++j) out[i * 9 + j] = r[j];
    } else {
        const float *R = in + i * 9;
        const float r12 = R[5];
        const bool sat = (r12 >= 1.0f) || (r12 < -1.0f);
        out[i * 3] = q_asin(fminf(fmaxf(r12, -1.0f), 1.0f));
        out[i * 3 + 1] = sat ? 0.0f : q_atan2<true>(-R[2], R[8]);      // a caller's matrix may hold -0: as numpy.arctan2 treats it
        out[i * 3 + 2] = q_atan2<true>(-R[3], R[4]);
    }
}

__global__ __launch_bounds__(kBlock) void k_rel_obs(int64_t n, const float *chaser, const float *target, float *obs)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float sc[13], st[13], o[12];
    for (int j = 0; j < 13; ++j) { sc[j] = chaser[i * 13 + j]; st[j] = target[i * 13 + j]; }
    rel_obs(sc, st, o);
    for (int j = 0; j < 12; ++j) obs[i * 12 + j] = o[j];
}

}  // namespace
