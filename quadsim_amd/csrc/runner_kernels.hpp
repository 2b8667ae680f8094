// runner_kernels.hpp -- PPO2 data collection in one launch: RunnerArgs, the LDS loaders, k_runner_rollout and k_runner_split
// A fragment of quadsim_hip.hip (ONE translation unit), included there right after policy_kernels.hpp, nowhere else.
#pragma once

namespace {

// PPO2 data collection in one launch: the Runner loop of rl_baselines/ppo2/ppo2.py:472-499 (+ last_values, :506) for
// N envs and T = n_steps.  Per step: mb_obs <- obs; (mean, value) <- MLP heads on exact-f32 MFMA; action = mean +
// std * N(0,1) (rocRAND Philox + Box-Muller, or caller-supplied noise); neglogp of the diagonal Gaussian
// (common/distributions.py:406-410); env.step(clip(action, -1, 1)); mb_dones holds the done flags BEFORE the step
// (ppo2.py:479), rewards / the new done after it.  squash: the fork's tanh variant (common/policies.py:238-242,
// distributions.py:412-415): env gets tanh(u), neglogp += sum log(1 - tanh(u)^2 + 1e-6), mb_actions keeps u.
struct RunnerArgs {
    AcArgs net;
    float std[4], inv_std[4];
    float nl_const;            // 0.5 log(2 pi) * 4 + sum(logstd)
    int squash;
    const float *noise;        // nullable [T,N,4]
    const uint8_t *dones_in;   // nullable [N]: done flags carried over from the previous run
    const uint4 *blob;         // FAST only: packed split-bf16 weight image (kAcFastBlobBytes)
    float *actions;            // [T,N,4]
    float *values;             // [T,N]
    float *neglogp;            // [T,N]
    float *last_obs;           // nullable [N,12]
    float *last_values;        // [N]
    uint8_t *last_dones;       // [N]
    int env_major;             // mb_obs / mb_actions rows at env*T + t (already swap_and_flatten-ed) instead of t*N + env
    const float *wtv1, *bv1;   // NET == kNetTowers, exact f32: vf_fc0 [128][12] (out, in), [128] (net.wt1 / b1 = pi_fc0)
};

// Tower image (mlp.hpp "Tower actor-critic") into LDS by `nthr` threads; -> the per-wave stages.  FAST: the packed
// blob plus 2 KiB of zeros right after the stages.  Lp / Lv: the exact image with W1 = pi_fc0 / vf_fc0.
template <bool FAST>
__device__ __forceinline__ float *load_towers_lds(char *lds_raw, const RunnerArgs &R, int nthr, AcLds &Lp, AcLds &Lv)
{
    if constexpr (FAST) {
        for (int i = threadIdx.x; i < kAcTowFastBlobBytes / 16; i += nthr) reinterpret_cast<uint4 *>(lds_raw)[i] = R.blob[i];
        for (int i = threadIdx.x; i < 2048 / 16; i += nthr) reinterpret_cast<uint4 *>(lds_raw + kAcTowFastLdsBytes)[i] = make_uint4(0, 0, 0, 0);
        return reinterpret_cast<float *>(lds_raw + kAcTowFastBlobBytes);
    } else {
        float *sW2 = reinterpret_cast<float *>(lds_raw);                // row r: pi_fc1^T row r | vf_fc1^T row r | pad
        float *sW3p = sW2 + kHid * kLdW2T;
        float *sW3v = sW3p + 4 * kLdW;
        float *sW1 = sW3v + kLdW;
        float *sW1v = sW1 + kHid * kLdW1;
        float *sB1 = sW1v + kHid * kLdW1;
        float *sB2p = sB1 + kHid;
        float *sB2v = sB2p + kHid;
        float *sB1v = sB2v + kHid;
        float *sB3 = sB1v + kHid;
        for (int i = threadIdx.x; i < kHid * kHid; i += nthr) {
            sW2[(i >> 7) * kLdW2T + (i & 127)] = R.net.wt2[i];
            sW2[(i >> 7) * kLdW2T + kHid + (i & 127)] = R.net.wtv2[i];
        }
        for (int i = threadIdx.x; i < 4 * kHid; i += nthr) sW3p[(i >> 7) * kLdW + (i & 127)] = R.net.wt3[i];
        for (int i = threadIdx.x; i < kHid; i += nthr) sW3v[i] = R.net.wtv3[i];
        for (int i = threadIdx.x; i < kHid * 12; i += nthr) {
            sW1[(i / 12) * kLdW1 + (i % 12)] = R.net.wt1[i];
            sW1v[(i / 12) * kLdW1 + (i % 12)] = R.wtv1[i];
        }
        for (int i = threadIdx.x; i < kHid; i += nthr) { sB1[i] = R.net.b1[i]; sB2p[i] = R.net.b2[i]; sB2v[i] = R.net.bv2[i]; sB1v[i] = R.bv1[i]; }
        if (threadIdx.x < 16) sB3[threadIdx.x] = threadIdx.x < 4 ? R.net.b3[threadIdx.x] : (threadIdx.x == 4 ? R.net.bv3[0] : 0.0f);
        Lp = AcLds{sW1, sB1, sW2, sB2p, sW2 + kHid, sB2v, sW3p, sW3v, sB3};
        Lv = Lp;
        Lv.W1 = sW1v; Lv.B1 = sB1v;
        return sB3 + 16;
    }
}

// Shared-trunk image (mlp.hpp) into LDS by `nthr` threads; -> the per-wave stages.  FAST: the packed blob verbatim (the
// kernels zero their 2 KiB for the dead output rows themselves: it lies where their own layout leaves room).
template <bool FAST>
__device__ __forceinline__ float *load_shared_lds(char *lds_raw, const RunnerArgs &R, int nthr, AcLds &L)
{
    if constexpr (FAST) {
        for (int i = threadIdx.x; i < kAcFastBlobBytes / 16; i += nthr) reinterpret_cast<uint4 *>(lds_raw)[i] = R.blob[i];
        return reinterpret_cast<float *>(lds_raw + kAcFastBlobBytes);
    } else {
        float *sW2p = reinterpret_cast<float *>(lds_raw);
        float *sW2v = sW2p + kHid * kLdW;
        float *sW3p = sW2v + kHid * kLdW;
        float *sW3v = sW3p + 4 * kLdW;
        float *sW1 = sW3v + kLdW;
        float *sB1 = sW1 + kHid * kLdW1;
        float *sB2p = sB1 + kHid;
        float *sB2v = sB2p + kHid;
        float *sB3 = sB2v + kHid;
        for (int i = threadIdx.x; i < kHid * kHid; i += nthr) {
            sW2p[(i >> 7) * kLdW + (i & 127)] = R.net.wt2[i];
            sW2v[(i >> 7) * kLdW + (i & 127)] = R.net.wtv2[i];
        }
        for (int i = threadIdx.x; i < 4 * kHid; i += nthr) sW3p[(i >> 7) * kLdW + (i & 127)] = R.net.wt3[i];
        for (int i = threadIdx.x; i < kHid; i += nthr) sW3v[i] = R.net.wtv3[i];
        for (int i = threadIdx.x; i < kHid * 12; i += nthr) sW1[(i / 12) * kLdW1 + (i % 12)] = R.net.wt1[i];
        for (int i = threadIdx.x; i < kHid; i += nthr) { sB1[i] = R.net.b1[i]; sB2p[i] = R.net.b2[i]; sB2v[i] = R.net.bv2[i]; }
        if (threadIdx.x < 16) sB3[threadIdx.x] = threadIdx.x < 4 ? R.net.b3[threadIdx.x] : (threadIdx.x == 4 ? R.net.bv3[0] : 0.0f);
        L = AcLds{sW1, sB1, sW2p, sB2p, sW2v, sB2v, sW3p, sW3v, sB3};
        return sB3 + 16;
    }
}

// action = mean + std * eps, its neglogp under the diagonal Gaussian, and what the env gets: a = clip(u) or the squashed tanh(u)
template <class Mean>
__device__ __forceinline__ void sample_action(const RunnerArgs &R, const Mean &mean, const float eps[4], float u[4], float a[4], float &nl)
{
    nl = R.nl_const;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        u[i] = fmaf(R.std[i], eps[i], mean[i]);                   // distributions.py:429
        const float d = (u[i] - mean[i]) * R.inv_std[i];          // :407
        nl = fmaf(0.5f * d, d, nl);
    }
    if (R.squash) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float sech2;
            a[i] = q_tanh_nan(u[i], sech2);                        // policies.py:238
            nl += q_ln(sech2 + 1e-6f);                            // distributions.py:414, 1 - tanh(u)^2 + 1e-6
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = clamp1(u[i]);   // ppo2.py:483
    }
}

template <bool FAST, int NET>
constexpr int runner_lds_bytes()
{
    return NET == kNetTowers ? (FAST ? kAcTowFastLdsBytes + 2048 : (int)(tow_lds_floats() * sizeof(float)))
                             : (FAST ? kAcFastLdsBytes + 2048 : (int)(ac_lds_floats() * sizeof(float)));
}

// FAST: the networks on the bf16 matrix rate with split operands (mlp_heads<true, NET>; R.blob = host-packed image, and
//       2 KiB of zeros right after the stages)
// PARAMS: per-env mass / inertia (domain randomisation; RMODE 2 redraws them at every episode start)
// NET: kNetShared (shared_fc0 trunk, the shipped best_model_v0) or kNetTowers (separate pi / vf towers)
template <int INTEG, int RMODE, bool PARAMS, bool FAST, int NET = kNetShared>
__global__ __launch_bounds__(kBlock, 1) void k_runner_rollout(StepArgs A, RunnerArgs R)
{
    constexpr bool TOW = NET == kNetTowers;
    constexpr int kZeros = TOW ? kAcTowFastLdsBytes : kAcFastLdsBytes;                               // FAST: 2 KiB of zeros
    __shared__ __attribute__((aligned(16))) char lds_raw[runner_lds_bytes<FAST, NET>()];
    AcLds L{}, Lv{};
    float *sStage;
    if constexpr (TOW) sStage = load_towers_lds<FAST>(lds_raw, R, kBlock, L, Lv);
    else sStage = load_shared_lds<FAST>(lds_raw, R, kBlock, L);
    if (!TOW && FAST && threadIdx.x < 128) reinterpret_cast<uint4 *>(lds_raw + kZeros)[threadIdx.x] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const HeadsLds H{lds_raw, kZeros, L, Lv};

    const int lane = threadIdx.x & (kTile - 1);
    const int w = threadIdx.x >> 6;
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + w;
    const int64_t env = tile * kTile + lane;
    const bool active = env < A.n;             // MFMA needs the whole wave: idle lanes carry a nominal env, store nothing
    float *stage = sStage + w * (12 * 64);
    QS_ASSERT((char *)(stage + 12 * 64) <= lds_raw + sizeof lds_raw);
    Env e;
    load_env_or_nominal(A, tile, lane, active, e);
    Par P = A.par_nom;
    if (PARAMS && active) P = load_par(A.par, tile, lane);
    const uint64_t k0 = active ? step_counter_begin(A, tile) : 0;
    bool done_prev = (active && R.dones_in) ? R.dones_in[env] != 0 : false;
    float obs[12];
    rel_obs(e.sc, e.st, obs);
#pragma clang loop unroll(disable)
    for (int64_t t = 0; t < A.T; ++t) {
        const int64_t o = t * A.n + env;
        QS_ASSERT(!active || (o >= 0 && o < A.T * A.n));
        // the two wide arrays can be written env-major right away (ppo2.py:522-523 flattens them afterwards anyway): a
        // lane's consecutive steps then fill consecutive 48- / 16-byte slots of its own row, which the XCD's L2 merges
        const int64_t ow = R.env_major ? env * A.T + t : o;
        if (active) { if (R.env_major) store_obs_cached(A.obs, ow, obs); else store_obs(A.obs, ow, obs); }   // mb_obs: the observation the policy acts on
        float head[5];
        mlp_heads<FAST, NET>(obs, head, H, stage, lane);
        float eps[4];
        if (R.noise) {
            const float4 nv = active ? reinterpret_cast<const float4 *>(R.noise)[o] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            eps[0] = nv.x; eps[1] = nv.y; eps[2] = nv.z; eps[3] = nv.w;
        } else {
            random_normal4(A.rc.seed, A.gid0 + (uint64_t)(active ? env : 0), k0 + (uint64_t)t, eps);
        }
        float u[4], a[4], nl;
        sample_action(R, head, eps, u, a, nl);
        if (active) {
            reinterpret_cast<float4 *>(R.actions)[ow] = make_float4(u[0], u[1], u[2], u[3]);
            R.values[o] = head[4];
            R.neglogp[o] = nl;
            A.done[o] = done_prev ? 1 : 0;                            // mb_dones: flags before the step (ppo2.py:479)
        }
        float reward;
        unsigned flags;
        bool done;
        step_and_maybe_reset<INTEG, PARAMS, RMODE>(e, P, a, A, active ? env : 0, k0 + (uint64_t)t, obs, reward, flags, done, false);
        done_prev = done;
        if (active) {
            A.reward[o] = reward;
            if (A.flags) A.flags[o] = (uint8_t)flags;
        }
    }
    // last_values = model.value(obs) on the observation after the last step (ppo2.py:506)
    float head[5];
    mlp_heads<FAST, NET>(obs, head, H, stage, lane);
    if (active) {
        R.last_values[env] = head[4];
        R.last_dones[env] = done_prev ? 1 : 0;
        if (R.last_obs) store_obs(R.last_obs, env, obs);
        store_env(A.st, tile, lane, e);
        if (PARAMS && RMODE == 2) store_par(A.par, tile, lane, P);
        step_counter_end(A, tile, lane, k0);
    }
}

// Role-split variant of the Runner kernel: one workgroup = four tiles = EIGHT waves.  Waves 0..3 ("matrix" role,
// one per SIMD) only evaluate the networks, waves 4..7 ("env" role, wave 4 + i next to wave i) own the environment state of
// the same four tiles: sampling, neglogp, env.step, every mb_* store except the values.  Per step and tile
//   env wave:     obs -> LDS | draw N(0,1), target's half of env.step -> #b -> sample, neglogp, stores, chaser's half, new obs -> LDS -> #a
//   matrix wave:  -> #a -> layer 1, policy branch, means -> LDS       -> #b -> value branch, store value
// so the value branch (almost half of a step's MFMAs) and the env step (VALU) run at the same time on the same SIMD, and
// the matrix wave keeps no environment registers: both roles fit 256 registers, two waves per SIMD.  The means travel
// through the tile's obs stage (the matrix wave has its observations in registers by then), the values through a
// buffer private to the matrix wave.  Every wave passes the same 2 T + 1 workgroup barriers.  FAST as in k_runner_rollout;
// the heads are the very pieces mlp_heads runs there (mlp.hpp), in its order, so the two kernels agree bit for bit.
// NET == kNetTowers: the matrix wave runs pi layer 1 -> policy branch -> vf layer 1 (the stage still holds the observations)
// -> means to LDS -> #b -> value branch; the values reach their lanes by ds_bpermute (no value buffer: see the tower image).
template <int INTEG, int RMODE, bool PARAMS, bool FAST, int NET = kNetShared>
__global__ __launch_bounds__(2 * kBlock, 1) void k_runner_split(StepArgs A, RunnerArgs R)
{
    constexpr bool TOW = NET == kNetTowers;
    constexpr int kHeadBytes = FAST ? kAcFastLdsBytes : (int)(ac_lds_floats() * sizeof(float));     // weights + 4 obs stages
    constexpr int kZeros = TOW ? kAcTowFastLdsBytes : kHeadBytes + 4 * kTile * 4;                   // FAST: 2 KiB of zeros
    __shared__ __attribute__((aligned(16))) char lds_raw[TOW ? runner_lds_bytes<FAST, NET>() : kZeros + (FAST ? 2048 : 0)];
    AcLds L{}, Lv{};
    float *sStage;
    if constexpr (TOW) sStage = load_towers_lds<FAST>(lds_raw, R, 2 * kBlock, L, Lv);
    else sStage = load_shared_lds<FAST>(lds_raw, R, 2 * kBlock, L);
    if (!TOW && FAST && threadIdx.x < 128) reinterpret_cast<uint4 *>(lds_raw + kZeros)[threadIdx.x] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const int lane = threadIdx.x & (kTile - 1);
    const int w = (threadIdx.x >> 6) & 3;
    const bool matrix_role = threadIdx.x < kBlock;
    const int64_t tile = (int64_t)blockIdx.x * (kBlock / kTile) + w;
    const int64_t env = tile * kTile + lane;
    const bool active = env < A.n;             // MFMA needs the whole wave: idle lanes carry a nominal env, store nothing
    float *stage = sStage + w * (12 * 64);
    float *sval = reinterpret_cast<float *>(lds_raw + kHeadBytes) + w * kTile;       // shared trunk only
    QS_ASSERT((char *)(stage + 12 * 64) <= lds_raw + (TOW ? (int)sizeof lds_raw : kHeadBytes));
    const HeadsLds H{lds_raw, kZeros, L, Lv};
    if (matrix_role) {
        const int c = lane & 15, g = lane >> 4;
        // layer-1 result = the B operands of both 128 x 128 branches, 128 registers either way
        HeadB<FAST> bh, bl;
        HeadH<FAST> h1;
        f32x4 a3[4];
        QS_PHASE_DECL;
#pragma clang loop unroll(disable)
        for (int64_t t = 0; t <= A.T; ++t) {
            __syncthreads();                                                  // #a: this step's observations are in LDS
            QS_PHASE(0);
            if (!TOW || t < A.T) heads_layer1<FAST, false>(H, stage, lane, bh, bl, h1);
            QS_PHASE(1);
            if (t < A.T) heads_branch<FAST, NET, 0>(H, bh, bl, h1, lane, a3);
            if constexpr (TOW) heads_layer1<FAST, true>(H, stage, lane, bh, bl, h1);   // before the means overwrite the observations
            if (t < A.T) {
                if (g == 0) means_to_stage(a3, stage, c);
                QS_PHASE(2);
                __syncthreads();                                              // #b: the means are in LDS
                QS_PHASE(3);
            }
            heads_branch<FAST, NET, 1>(H, bh, bl, h1, lane, a3);
            QS_PHASE(4);
            float v;
            if constexpr (TOW) {
                v = value_to_owner(a3, lane);
            } else {
                if (g == 1) {
#pragma unroll
                    for (int et = 0; et < 4; ++et) sval[16 * et + c] = a3[et][0];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                v = sval[lane];
                __builtin_amdgcn_wave_barrier();
            }
            if (active) {
                float *vout = t < A.T ? R.values + t * A.n : R.last_values;   // last: model.value(obs) after the last step (ppo2.py:506)
                vout[env] = v;
            }
            QS_PHASE(5);
        }
        QS_PHASE_FLUSH(0);
    } else {
        Env e;
        load_env_or_nominal(A, tile, lane, active, e);
        Par P = A.par_nom;
        if (PARAMS && active) P = load_par(A.par, tile, lane);
        const uint64_t k0 = active ? step_counter_begin(A, tile) : 0;
        bool done_prev = (active && R.dones_in) ? R.dones_in[env] != 0 : false;
        float obs[12];
        rel_obs(e.sc, e.st, obs);
#pragma unroll
        for (int k = 0; k < 12; ++k) stage[k * 64 + lane] = obs[k];
        QS_PHASE_DECL;
#pragma clang loop unroll(disable)
        for (int64_t t = 0; t < A.T; ++t) {
            const int64_t o = t * A.n + env;
            QS_ASSERT(!active || (o >= 0 && o < A.T * A.n));
            const int64_t ow = R.env_major ? env * A.T + t : o;
            if (active) { if (R.env_major) store_obs_cached(A.obs, ow, obs); else store_obs(A.obs, ow, obs); }
            QS_PHASE(0);
            __syncthreads();                                                  // #a
            QS_PHASE(1);
            float eps[4];
            if (R.noise) {
                const float4 nv = active ? reinterpret_cast<const float4 *>(R.noise)[o] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                eps[0] = nv.x; eps[1] = nv.y; eps[2] = nv.z; eps[3] = nv.w;
            } else {
                random_normal4(A.rc.seed, A.gid0 + (uint64_t)(active ? env : 0), k0 + (uint64_t)t, eps);
            }
            // the target's half of env.step does not need the action: it runs here, next to the policy branch
            const bool lim_t = env_step_target<INTEG>(e, P, A.C);
            QS_PHASE(2);
            __syncthreads();                                                  // #b
            QS_PHASE(3);
            const f32x4 mean = *reinterpret_cast<const f32x4 *>(stage + lane * 8);
            float u[4], a[4], nl;
            sample_action(R, mean, eps, u, a, nl);
            if (active) {
                reinterpret_cast<float4 *>(R.actions)[ow] = make_float4(u[0], u[1], u[2], u[3]);
                R.neglogp[o] = nl;
                A.done[o] = done_prev ? 1 : 0;                                // mb_dones: flags before the step (ppo2.py:479)
            }
            QS_PHASE(4);
            float reward;
            unsigned flags;
            bool done;
            env_step_chaser<INTEG>(e, a, P, A.C, lim_t, obs, reward, flags);
            maybe_reset<PARAMS, RMODE>(e, P, A, active ? env : 0, k0 + (uint64_t)t, obs, flags, done, false);
            done_prev = done;
#pragma unroll
            for (int k = 0; k < 12; ++k) stage[k * 64 + lane] = obs[k];
            if (active) {
                A.reward[o] = reward;
                if (A.flags) A.flags[o] = (uint8_t)flags;
            }
            QS_PHASE(5);
        }
        QS_PHASE_FLUSH(1);
        __syncthreads();                                                      // #a of the value-only pass
        if (active) {
            R.last_dones[env] = done_prev ? 1 : 0;
            if (R.last_obs) store_obs(R.last_obs, env, obs);
            store_env(A.st, tile, lane, e);
            if (PARAMS && RMODE == 2) store_par(A.par, tile, lane, P);
            step_counter_end(A, tile, lane, k0);
        }
    }
}

}  // namespace
