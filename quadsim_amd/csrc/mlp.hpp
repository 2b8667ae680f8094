// mlp.hpp -- the MLP device functions of the policy-in-the-loop roll-out in ONE launch:
//   for t in 0..T-1:  a_t = clip(MLP(obs_t), -1, 1);  obs_{t+1}, r_t, done_t = env.step(a_t)
// i.e. the loop of run_trained_docking_ppo2.py:37-60 (model.predict(obs, deterministic=True); env.step(action))
// for N envs with the actor of the shipped PPO2 model (shared_fc0 12->128, pi_fc0 128->128, pi 128->4, ReLU).
// The MLP runs on the matrix cores with exact-f32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, so the
// network output is an ordinary float32 evaluation), the env step is the same device code as k_env.
//
// Orientation: every layer is computed TRANSPOSED, H^T[hidden][env] = W^T[hidden][k] . X^T[k][env], with the
// weights as the A operand and the activations as the B operand.  An accumulator tile D (16 hidden x 16 envs) then
// holds, in register i of lane l, hidden row 4*(l>>4)+i of env column l&15 -- exactly the (k-slot = l>>4,
// column = l&15) placement the NEXT layer's B operand needs if its k-step "i of tile rt" is defined to sum the
// hidden indices {16 rt + 4 g + i : g = 0..3}.  So accumulators feed the next MFMA directly: no LDS round trip, no
// lane shuffles between layers; only the weight fetch address carries the permutation (weights sit in LDS as
// W^T rows with a 132-float stride, one ds_read_b128 per 16 MFMAs).  Layer 3 is folded into the layer-2 loop
// (each finished 16-row tile of H2 is immediately reduced into the 4 action rows), so H2 is never held whole.
// Per wave and step: 96 + 1024 + 128 MFMAs = 40 k SIMD cycles -- the roll-out is bound by the f32 matrix rate.
#pragma once
#include <hip/hip_runtime.h>
#include "quadsim_device.hpp"

namespace qs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kHid = 128;      // hidden width of both layers
constexpr int kLdW = 132;      // LDS row stride of W2^T / W3^T (floats): 132 = 128 + 4 keeps ds_read_b128 conflict-free
constexpr int kLdW1 = 13;      // LDS row stride of W1^T (12 inputs + 1)

struct MlpArgs {
    const float *wt1;   // [128][12]  = shared_fc0 weight transposed (out, in)
    const float *b1;    // [128]
    const float *wt2;   // [128][128] = pi_fc0 weight transposed
    const float *b2;    // [128]
    const float *wt3;   // [4][128]   = pi weight transposed
    const float *b3;    // [4]
};

constexpr size_t policy_lds_floats()
{
    return (size_t)kHid * kLdW + 16 * kLdW + kHid * kLdW1 + kHid + kHid + 16 + 4 * (12 * 64) + 4 * (64 * 4);
}

// (a select, not fmaxf: fmaxf drops a NaN operand, and a NaN weight would act as a dead unit.  -0 <= 0 holds: -0 still becomes +0)
__device__ __forceinline__ float relu1(float z) { return z <= 0.0f ? 0.0f : z; }
__device__ __forceinline__ f32x4 relu4(f32x4 v)
{
    return f32x4{relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)};
}

// ---- the pieces every actor and actor-critic kernel is built from, each written once ------------------------
// obs^T [12][64] of the wave's 64 envs into its stage, so that each lane can fetch the (k, env column) element its B operand needs
__device__ __forceinline__ void stage_obs(const float obs[12], float *stage, int lane)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) stage[k * 64 + lane] = obs[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Layer 1 on the f32 MFMA: H1^T [128][64] = W1^T [128][12] . obs^T [12][64] + b1, 3 k-steps x 4 env tiles per 16-row tile;
// epi(rt, acc) takes the four finished accumulators of row tile rt.  The caller supplies the lane's three base addresses,
// w1 = &W1^T[c][g] (+ 16 rt kLdW1 + 4 s), b1 = &b1[4 g] (+ 16 rt), xs = &stage[g][c] (+ 256 s + 16 et): plain (layer1_relu)
// or through lds_opaque (ac_fast_layer1) -- the addressing is the flavour, the arithmetic is this one body.
template <class Epi>
__device__ __forceinline__ void layer1_f32(const float *w1, const float *b1, const float *xs, Epi &&epi)
{
    float xb[3][4];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int et = 0; et < 4; ++et) xb[s][et] = xs[256 * s + 16 * et];
#pragma unroll
    for (int rt = 0; rt < 8; ++rt) {
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(b1 + 16 * rt);
        float a[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) a[s] = w1[16 * rt * kLdW1 + 4 * s];
        f32x4 acc[4] = {bias, bias, bias, bias};              // k-step outermost: consecutive MFMAs on different accumulators
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int et = 0; et < 4; ++et) acc[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], xb[s][et], acc[et], 0, 0, 0);
        epi(rt, acc);
    }
}

// exact-f32 flavour: ReLU into h1, the B operands of the f32 128 x 128 layer
__device__ __forceinline__ void layer1_relu(const float *W1, const float *B1, const float *stage, int lane, f32x4 (&h1)[8][4])
{
    const int c = lane & 15, g = lane >> 4;
    layer1_f32(W1 + c * kLdW1 + g, B1 + 4 * g, stage + g * 64 + c, [&](int rt, const f32x4 (&acc)[4]) {
#pragma unroll
        for (int et = 0; et < 4; ++et) h1[rt][et] = relu4(acc[et]);
    });
}

// output-layer accumulators of the four env tiles = the lane's four rows of the padded output bias b3 [16]
__device__ __forceinline__ void init_a3(const float *B3, int lane, f32x4 (&a3)[4])
{
    const f32x4 bias3 = *reinterpret_cast<const f32x4 *>(B3 + 4 * (lane >> 4));
#pragma unroll
    for (int et = 0; et < 4; ++et) a3[et] = bias3;
}

// Hand-over of the actors: rows 0..3 of the action tile live in lanes 0..15 (g == 0); through sAct [64][4] to the lane that
// owns the env, clipped to [-1, 1] (clamp1: a NaN mean stays a NaN action)
__device__ __forceinline__ void actions_to_owner(const f32x4 (&a3)[4], float *sAct, int lane, float act[4])
{
    const int c = lane & 15, g = lane >> 4;
    if (g == 0) {
#pragma unroll
        for (int et = 0; et < 4; ++et) *reinterpret_cast<f32x4 *>(sAct + (16 * et + c) * 4) = a3[et];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const f32x4 av = *reinterpret_cast<const f32x4 *>(sAct + lane * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) act[i] = clamp1(av[i]);
    __builtin_amdgcn_wave_barrier();
}

// Hand-over of the heads through the wave's stage, [64][8] floats.  The means are rows 0..3 of a3p, which sit in lanes g == 0
// (the caller's guard; c = lane & 15): into slots 0..3 of their env.  k_runner_split's matrix waves stop here: the env wave of
// the tile reads them after a workgroup barrier.
__device__ __forceinline__ void means_to_stage(const f32x4 (&a3p)[4], float *stage, int c)
{
#pragma unroll
    for (int et = 0; et < 4; ++et) *reinterpret_cast<f32x4 *>(stage + (16 * et + c) * 8) = a3p[et];
}

// ... and the value (row 4 of a3v = register 0 of lanes g == 1) into slot 4, then all five to the lane that owns the env.
// The stage is free by then: every lane of the wave read its layer-1 operands before the branches.
__device__ __forceinline__ void heads_to_owner(const f32x4 (&a3p)[4], const f32x4 (&a3v)[4], float *stage, int lane, float out[5])
{
    const int c = lane & 15, g = lane >> 4;
    if (g == 0) {
        means_to_stage(a3p, stage, c);
    } else if (g == 1) {
#pragma unroll
        for (int et = 0; et < 4; ++et) stage[(16 * et + c) * 8 + 4] = a3v[et][0];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const f32x4 av = *reinterpret_cast<const f32x4 *>(stage + lane * 8);
    out[0] = av[0]; out[1] = av[1]; out[2] = av[2]; out[3] = av[3];
    out[4] = stage[lane * 8 + 4];
    __builtin_amdgcn_wave_barrier();
}

// MLP for the 64 envs of one wave: obs (per owning lane) -> 4 actions (per owning lane), clipped to [-1,1]
__device__ __forceinline__ void mlp_actor(const float obs[12], float act[4], const float *sW1, const float *sB1,
                                          const float *sW2, const float *sB2, const float *sW3, const float *sB3,
                                          float *sObs, float *sAct, int lane)
{
    const int c = lane & 15, g = lane >> 4;
    stage_obs(obs, sObs, lane);
    f32x4 h1[8][4];
    layer1_relu(sW1, sB1, sObs, lane, h1);
    // ---- layers 2 + 3: for each 16-row tile of H2^T: 32 k-steps over H1^T, bias, ReLU, then straight into the
    //      action accumulators (rows 0..3 of a 16-row tile; W3^T rows 4..15 are zero)
    f32x4 a3[4];
    init_a3(sB3, lane, a3);
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(sB2 + 16 * nt + 4 * g);
        f32x4 h2[4] = {bias, bias, bias, bias};
#pragma unroll
        for (int rt = 0; rt < 8; ++rt) {
            const f32x4 w = *reinterpret_cast<const f32x4 *>(sW2 + (16 * nt + c) * kLdW + 16 * rt + 4 * g);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int et = 0; et < 4; ++et)
                    h2[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], h1[rt][et][i], h2[et], 0, 0, 0);
        }
        const f32x4 w3 = *reinterpret_cast<const f32x4 *>(sW3 + c * kLdW + 16 * nt + 4 * g);
        f32x4 r[4];
#pragma unroll
        for (int et = 0; et < 4; ++et) r[et] = relu4(h2[et]);
#pragma unroll
        for (int i = 0; i < 4; ++i)                     // k-step outermost: consecutive MFMAs on different accumulators
#pragma unroll
            for (int et = 0; et < 4; ++et) a3[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(w3[i], r[et][i], a3[et], 0, 0, 0);
        // issue order of this tile: every weight read one 16-MFMA group ahead of its use (left alone, hipcc emits
        // read -> wait -> 16 MFMAs and exposes the LDS latency 8 times per tile): 24.9 -> 24.3 us/step.  The same
        // directives change nothing in the actor-critic heads (43.7 vs 43.8 us/step) and are not applied there.
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            __builtin_amdgcn_sched_group_barrier(0x8, 16, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x8, 16, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    actions_to_owner(a3, sAct, lane, act);
}

// ------------------------------------------------------------------------------------------------------------
// Actor-critic heads of the PPO2 MlpPolicy the reference trains (rl_baselines/common/policies.py:35-92 mlp_extractor
// with net_arch [128, dict(vf=[128], pi=[128])], :583-588): shared_fc0 -> {pi_fc0 -> pi (mean), vf_fc0 -> vf (value)},
// i.e. what model.step evaluates per Runner step (rl_baselines/ppo2/ppo2.py:475).  Same exact-f32 MFMA chaining as
// mlp_actor; the value branch re-uses H1 and lands in row 4 of the 16-row output tile (rows 0..3 = action mean).
// LDS image (floats): W2pi^T 128x132 | W2vf^T 128x132 | W3pi^T 4x132 | W3vf 132 | W1^T 128x13 | b1 128 | b2pi 128 |
// b2vf 128 | b3 16 (mean biases, value bias at [4]) | per-wave stage 4 x 768  = 158 352 B of the CU's 160 KiB.
struct AcArgs {
    const float *wt1, *b1;      // shared_fc0: [128][12] (out, in), [128]
    const float *wt2, *b2;      // pi_fc0:     [128][128], [128]
    const float *wt3, *b3;      // pi:         [4][128], [4]
    const float *wtv2, *bv2;    // vf_fc0:     [128][128], [128]
    const float *wtv3, *bv3;    // vf:         [1][128], [1]
};

struct AcLds {
    const float *W1, *B1, *W2p, *B2p, *W2v, *B2v, *W3p, *W3v, *B3;
};

constexpr size_t ac_lds_floats()
{
    return (size_t)2 * kHid * kLdW + 4 * kLdW + kLdW + kHid * kLdW1 + 3 * kHid + 16 + 4 * (12 * 64);
}

// ------------------------------------------------------------------------------------------------------------
// Fast actor: the same MLP on the bf16 matrix rate (16x the f32 MFMA rate) with SPLIT operands.  Every f32 value v
// is carried as two bf16, hi = bf16(v) and lo = bf16(v - hi), and a product x*w is evaluated as
// hi*hi + hi*lo + lo*hi with f32 accumulation (three v_mfma_f32_16x16x32_bf16); the dropped lo*lo term and the
// 16-bit representation leave a relative error of about 2^-17 per product (~1e-5 on an action) instead of f32's
// 2^-24.  NOT bit-compatible with the float32 policy: an opt-in mode (qs_policy_rollout_fast).
// Layout: the accumulator-feeds-next-B-operand trick of the f32 path carries over.  A 16x16x32 B operand holds, in
// element j of lane (g = l>>4, c = l&15), k-slot 8g+j of column c; two accumulator tiles (2p, 2p+1) of the previous
// layer give that lane exactly 8 values -- hidden index h(p,g,j) = 16(2p + (j>>2)) + 4g + (j&3) -- so k-step p of the
// next layer sums those 32 hidden units, and the host packs the weights in that order: A fragments are stored
// ready-made, [tile][k-step][lane][8 bf16], one linear ds_read_b128 per fragment.
// Packed blob (bytes): A2hi 32768 | A2lo 32768 | A1hi 8192 | A1lo 8192 | A3hi 4096 | A3lo 4096 | b1 512 | b2 512 | b3 64.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kFastBlobBytes = 32768 * 2 + 8192 * 2 + 4096 * 2 + 512 + 512 + 64;

__device__ __forceinline__ void split_bf16(float v, __bf16 &hi, __bf16 &lo)
{
    hi = (__bf16)v;
    lo = (__bf16)(v - (float)hi);
}

// ReLU + hi/lo split of TWO accumulator values into one packed register each: 9 VALU instructions per pair (a compare and a
// select per value = ReLU without a canonicalising v_max; v_cvt_pk_bf16_f32 rounds both at once; the hi halves are widened
// back with a shift and a mask; one packed subtract; one more v_cvt_pk) where the value-at-a-time form takes 14.  Same
// roundings.  The ReLU is relu1's select: a NaN of either sign bit stays (a signed integer max against 0, one instruction less,
// turns a NaN whose sign bit is set -- what inf - inf and 0 / 0 give -- into +0); -0 .. -inf become +0.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void relu_split_pair(float v0, float v1, uint32_t &hi, uint32_t &lo)
{
    v0 = relu1(v0);
    v1 = relu1(v1);
    const f32x2 v = {v0, v1};
    hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
    const f32x2 r = {v0 - __builtin_bit_cast(float, hi << 16), v1 - __builtin_bit_cast(float, hi & 0xffff0000u)};
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2));
}
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4 w) { return __builtin_bit_cast(bf16x8, w); }
__device__ __forceinline__ bf16x8 as_bf16x8(bf16x8 w) { return w; }

// Layer-1 epilogue of every split-bf16 network: ReLU + split of row tile rt, straight into the B operands of layer 2
// (tiles 2p, 2p+1 -> k-step p).  bh / bl [p][et]: element j of the B operand = half (j & 1) of word j >> 1
__device__ __forceinline__ void relu_split_tile(int rt, const f32x4 (&acc)[4], u32x4 (&bh)[4][4], u32x4 (&bl)[4][4])
{
#pragma unroll
    for (int et = 0; et < 4; ++et) {
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            uint32_t h, l;
            relu_split_pair(acc[et][2 * pr], acc[et][2 * pr + 1], h, l);
            bh[rt >> 1][et][2 * (rt & 1) + pr] = h;
            bl[rt >> 1][et][2 * (rt & 1) + pr] = l;
        }
    }
}

// One k-step of a split product over N env tiles: acc[et] += lo*hi + hi*lo + hi*hi of the A fragment (ah, al) and the B
// operands (bh[et], bl[et]); term outermost, so that consecutive MFMAs use different accumulators
template <int N, class B>
__device__ __forceinline__ void mfma_split3(bf16x8 ah, bf16x8 al, const B (&bh)[N], const B (&bl)[N], f32x4 *acc)
{
#pragma unroll
    for (int term = 0; term < 3; ++term)
#pragma unroll
        for (int et = 0; et < N; ++et)
            acc[et] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(term == 0 ? al : ah, as_bf16x8(term == 1 ? bl[et] : bh[et]), acc[et], 0, 0, 0);
}

#ifndef QS_WEAVE
#define QS_WEAVE 1      // 0: layer-2 tiles one after the other (A/B reference), 1: hand-woven software pipeline
#endif

// Layer 2 of the split-bf16 heads: NT row tiles of 16 hidden units (one 128 x 128 layer = 8 tiles; the actor-critic runs its
// two branches as one sequence of 16), each 48 MFMAs over the four env tiles of the wave, followed by ReLU + hi/lo split into
// the B operands of the output layer (`out_step(pair, ch, cl)` after every second tile = one k-step of 32 hidden units).
// The tiles run as a software pipeline: the MFMAs of tile s + 1 are issued around the split of tile s, which depends only on
// tile s's accumulators -- the split's VALU work then rides in the issue shadow of the MFMAs (16 matrix cycles each, 8 of
// which hold the SIMD's vector-issue port) instead of standing between two MFMA runs.  hipcc does not weave the two streams by itself (at this register
// pressure its scheduler falls back to source order, sched_group_barrier patterns included), so the source order IS the woven
// order, pinned by scheduling barriers: MFMA m of tile s + 1 (order k-step | term | env tile, so that consecutive MFMAs use
// different accumulators), then ONE instruction-sized piece of the split of tile s (pair m / 6, piece m % 6); the A fragments
// of k-step p + 1 are requested while k-step p multiplies.  Runner, 65 536 envs: 17.1 -> 15.2 us per step.
struct L2Tile { const bf16x8 *hi, *lo; const float *bias; };     // fragments [k-step][lane] of the tile; the lane's 4 bias rows

// NET / E0: the pass covers env tiles E0 .. E0 + NET - 1 of the wave's four (a 2-tile pass halves the working set of
// accumulators and output-layer operands; the role-split runner's matrix waves run two such passes per branch).
template <int NT, int NET, int E0, class TileOf, class OutStep>
__device__ __forceinline__ void mlp_layer2_split(const u32x4 (&bh)[4][4], const u32x4 (&bl)[4][4], int lane, int g, TileOf &&tile_of,
                                                 OutStep &&out_step)
{
    auto h2_tile = [&](int s2, f32x4 (&h2)[NET]) {
        const L2Tile t = tile_of(s2);
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(t.bias);
#pragma unroll
        for (int et = 0; et < NET; ++et) h2[et] = bias;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const bf16x8 ah = t.hi[p * 64 + lane], al = t.lo[p * 64 + lane];
#pragma unroll
            for (int et = 0; et < NET; ++et) {
                h2[et] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, as_bf16x8(bh[p][E0 + et]), h2[et], 0, 0, 0);
                h2[et] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, as_bf16x8(bl[p][E0 + et]), h2[et], 0, 0, 0);
                h2[et] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, as_bf16x8(bh[p][E0 + et]), h2[et], 0, 0, 0);
            }
        }
    };
    auto split_tile = [&](const f32x4 (&h2)[NET], int half, u32x4 (&ch)[NET], u32x4 (&cl)[NET]) {
#pragma unroll
        for (int et = 0; et < NET; ++et)
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                uint32_t h, l;
                relu_split_pair(h2[et][2 * pr], h2[et][2 * pr + 1], h, l);
                ch[et][2 * half + pr] = h;
                cl[et][2 * half + pr] = l;
            }
    };
    u32x4 ch[NET], cl[NET];                                // split ReLU(H2) of a tile pair = one k-step of the output layer
#if QS_WEAVE == 1
    auto woven_stage = [&](int s2n, f32x4 (&hn)[NET], const f32x4 (&hc)[NET], int half) {
        const L2Tile t = tile_of(s2n);
        const bf16x8 *A2hi = t.hi + lane, *A2lo = t.lo + lane;
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(t.bias);
        bf16x8 ah[2], al[2];
        ah[0] = A2hi[0]; al[0] = A2lo[0];
        float v0[2 * NET], v1[2 * NET], h0[2 * NET], h1[2 * NET];
        uint32_t hu[2 * NET];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 12 * NET; ++m) {
            const int p = m / (3 * NET), term = (m % (3 * NET)) / NET, et = m % NET;
            if (m % (3 * NET) == 0 && p < 3) { ah[(p + 1) & 1] = A2hi[(p + 1) * 64]; al[(p + 1) & 1] = A2lo[(p + 1) * 64]; }
            const f32x4 cin = (p == 0 && term == 0) ? bias : hn[et];
            hn[et] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(term == 0 ? al[p & 1] : ah[p & 1],
                                                             as_bf16x8(term == 1 ? bl[p][E0 + et] : bh[p][E0 + et]), cin, 0, 0, 0);
            const int pair = m / 6, piece = m % 6, se = pair >> 1, pr = pair & 1;
            if (piece == 0) v0[pair] = relu1(hc[se][2 * pr]);
            if (piece == 1) v1[pair] = relu1(hc[se][2 * pr + 1]);
            if (piece == 2) { const f32x2 v = {v0[pair], v1[pair]}; hu[pair] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2)); }
            if (piece == 3) h0[pair] = __builtin_bit_cast(float, hu[pair] << 16);
            if (piece == 4) h1[pair] = __builtin_bit_cast(float, hu[pair] & 0xffff0000u);
            if (piece == 5) {
                const f32x2 r = {v0[pair] - h0[pair], v1[pair] - h1[pair]};
                ch[se][2 * half + pr] = hu[pair];
                cl[se][2 * half + pr] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    f32x4 hcur[NET], hnext[NET];
    h2_tile(0, hcur);
#pragma unroll
    for (int s2 = 0; s2 < NT; ++s2) {
        if (s2 + 1 < NT) woven_stage(s2 + 1, hnext, hcur, s2 & 1);
        else split_tile(hcur, s2 & 1, ch, cl);
        if (s2 & 1) out_step(s2 >> 1, ch, cl);
#pragma unroll
        for (int et = 0; et < NET; ++et) hcur[et] = hnext[et];
    }
#else
#pragma unroll
    for (int s2 = 0; s2 < NT; ++s2) {
        f32x4 h2[NET];
        h2_tile(s2, h2);
        split_tile(h2, s2 & 1, ch, cl);
        if (s2 & 1) out_step(s2 >> 1, ch, cl);
    }
#endif
}

__device__ __forceinline__ void mlp_actor_fast(const float obs[12], float act[4], const char *blob, float *sObs, float *sAct,
                                               int lane)
{
    const bf16x8 *A2hi = reinterpret_cast<const bf16x8 *>(blob);
    const bf16x8 *A2lo = reinterpret_cast<const bf16x8 *>(blob + 32768);
    const bf16x8 *A1hi = reinterpret_cast<const bf16x8 *>(blob + 65536);
    const bf16x8 *A1lo = reinterpret_cast<const bf16x8 *>(blob + 65536 + 8192);
    const bf16x8 *A3hi = reinterpret_cast<const bf16x8 *>(blob + 65536 + 16384);
    const bf16x8 *A3lo = reinterpret_cast<const bf16x8 *>(blob + 65536 + 16384 + 4096);
    const float *sB1 = reinterpret_cast<const float *>(blob + 65536 + 16384 + 8192);
    const float *sB2 = sB1 + 128;
    const float *sB3 = sB2 + 128;
    const int c = lane & 15, g = lane >> 4;
    stage_obs(obs, sObs, lane);
    // ---- layer 1 B operands: k-slot 8g+j = input 8g+j (12 inputs, the rest zero)
    bf16x8 xh[4], xl[4];
#pragma unroll
    for (int et = 0; et < 4; ++et)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * g + j;                       // g is per lane: guard by value, keep the read in range
            const float v = (k < 12) ? sObs[(k < 12 ? k : 0) * 64 + 16 * et + c] : 0.0f;
            __bf16 h, l;
            split_bf16(v, h, l);
            xh[et][j] = h; xl[et][j] = l;
        }
    // ---- layer 1: 8 row tiles, ReLU, straight into split B operands of layer 2 (tiles 2p, 2p+1 -> k-step p)
    u32x4 bh[4][4], bl[4][4];       // [p][et]: element j of the B operand = half (j & 1) of word j >> 1
#pragma unroll
    for (int rt = 0; rt < 8; ++rt) {
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(sB1 + 16 * rt + 4 * g);
        const bf16x8 ah = A1hi[rt * 64 + lane], al = A1lo[rt * 64 + lane];
        f32x4 acc[4] = {bias, bias, bias, bias};
        mfma_split3(ah, al, xh, xl, acc);
        relu_split_tile(rt, acc, bh, bl);
    }
    // ---- layer 2 in row-tile pairs, each pair folded into the action accumulators (layer 3 k-step = the pair)
    f32x4 a3[4];
    init_a3(sB3, lane, a3);
    mlp_layer2_split<8, 4, 0>(bh, bl, lane, g,
        [&](int nt) { return L2Tile{A2hi + nt * 4 * 64, A2lo + nt * 4 * 64, sB2 + 16 * nt + 4 * g}; },
        [&](int q, const u32x4 (&ch)[4], const u32x4 (&cl)[4]) {
            mfma_split3(A3hi[q * 64 + lane], A3lo[q * 64 + lane], ch, cl, a3);
        });
    actions_to_owner(a3, sAct, lane, act);
}

// ------------------------------------------------------------------------------------------------------------
// Fast actor-critic heads (qs_runner_rollout_fast): the heads above with the two 128x128 layers and the output layer
// on the bf16 matrix rate with split (hi + lo) operands, exactly as mlp_actor_fast; the 12-input first layer stays on
// the f32 MFMA (96 MFMAs, and its f32 weights are a third of the size of split fragments padded to k = 32).
// LDS image (bytes): A2pi hi 32768 | lo 32768 | A2vf hi 32768 | lo 32768 | A3pi hi 1024 | lo 1024 | A3vf hi 256 | lo 256 |
// W1^T f32 128x13 6656 | b1 512 | b2pi 512 | b2vf 512 | b3 64 | per-wave stage 4 x 3072  = 154 176 B, + 2 KiB of zeros for the
// dead output rows (ac_fast_branch) = 156 224 B in k_runner_rollout; k_runner_split puts its 1 KiB value buffer in between.
// A3pi keeps only output rows 0..3, A3vf only row 4 of the 16-row tile: [k-step q][row][g][8 bf16] / [q][g][8 bf16].
constexpr int kAcFastA2 = 0;
constexpr int kAcFastA3p = 4 * 32768;
constexpr int kAcFastA3v = kAcFastA3p + 2 * 1024;
constexpr int kAcFastW1 = kAcFastA3v + 2 * 256;
constexpr int kAcFastB = kAcFastW1 + kHid * kLdW1 * 4;
constexpr int kAcFastBlobBytes = kAcFastB + (3 * kHid + 16) * 4;
constexpr int kAcFastLdsBytes = kAcFastBlobBytes + 4 * (12 * 64) * 4;

// ------------------------------------------------------------------------------------------------------------
// The heads in pieces: what mlp_heads runs back to back for one wave per tile (k_runner_rollout), and what a MATRIX wave of
// the role-split runner (k_runner_split) runs while an ENV wave of the same tile steps the environments.  ac_fast_layer1:
// shared layer for the wave's 64 envs (observations read from the tile's LDS stage, [k][env]), result = the B operands of
// BOTH 128 x 128 branches, kept in registers.  ac_fast_branch<BR>: one branch (0 policy -> rows 0..3 of a3, 1 value -> row 4)
// over QS_SPLIT_NET env tiles per pass (256 registers per wave at two waves
// per SIMD: the four-tile pass fits next to the 128 operand registers once the LDS addresses share base registers, lds_opaque).
// An LDS byte offset the optimiser cannot see through: everything addressed as `blob + opaque + constant` then shares ONE
// address register with the constants in the instructions' offset fields, instead of one materialised address per constant
// (the matrix wave has 256 registers for 128 operand registers plus its working set; such addresses went to scratch).
__device__ __forceinline__ int lds_opaque(int off)
{
    asm volatile("" : "+v"(off));
    return off;
}

// W1OFF / B1OFF: byte offsets of the layer's f32 W1^T (128 x 13) and bias in the image (the tower layout's value branch has its own)
template <int W1OFF = kAcFastW1, int B1OFF = kAcFastB>
__device__ __forceinline__ void ac_fast_layer1(const char *blob, const float *stage, int lane, u32x4 (&bh)[4][4], u32x4 (&bl)[4][4])
{
    lane = lds_opaque(lane);       // lane-derived addresses are re-derived here every step instead of living across the step loop
    const int c = lane & 15, g = lane >> 4;
    // one base register per array, the (row tile, k-step, env tile) part in the offset fields (see lds_opaque)
    const float *w1 = reinterpret_cast<const float *>(blob + lds_opaque(W1OFF + (c * kLdW1 + g) * 4));        // + 16 rt kLdW1 + 4 s
    const float *b1 = reinterpret_cast<const float *>(blob + lds_opaque(B1OFF + 16 * g));                     // + 16 rt
    const float *xs = stage + lds_opaque(g * 64 + c);                                                         // + 256 s + 16 et
    layer1_f32(w1, b1, xs, [&](int rt, const f32x4 (&acc)[4]) { relu_split_tile(rt, acc, bh, bl); });
}

#ifndef QS_SPLIT_NET
#define QS_SPLIT_NET 4      // env tiles per layer-2 pass of a matrix wave: 4 = one pass; 2 = two passes with half the working set,
                            // but only two accumulators in flight -- a dependent v_mfma_f32_16x16x32_bf16 two instructions behind
                            // its producer waits for it (measured 22 cycles per MFMA against 18.5 with four)
#endif
// zeros: byte offset (from blob) of 2 KiB of zeros -- what the dead rows of the output-layer A tiles read
template <int BR, int E0>
__device__ __forceinline__ void ac_fast_branch_pass(const char *blob, int zeros, const u32x4 (&bh)[4][4], const u32x4 (&bl)[4][4], int lane,
                                                    f32x4 (&a3)[4])
{
    lane = lds_opaque(lane);       // as in ac_fast_layer1
    const int c = lane & 15, g = lane >> 4;
    const char *bias_base = blob + lds_opaque(kAcFastB + 16 * g);                       // + 512 (1 + BR) + 64 nt
    // output-layer A fragments: rows 0..3 (policy, [q][row][g]) / row 4 (value, [q][g]) hold weights, every other row of the
    // 16-row tile reads zeros: ONE address select per pass, the k-step q and the hi / lo half in the offset field
    const bool row_live = BR == 0 ? c < 4 : c == 4;
    const int a3_off = BR == 0 ? kAcFastA3p + ((c & 3) * 4 + g) * 16 : kAcFastA3v + g * 16;
    const char *a3_base = blob + lds_opaque(row_live ? a3_off : zeros);
    mlp_layer2_split<8, QS_SPLIT_NET, E0>(bh, bl, lane, g,
        [&](int nt) {
            return L2Tile{reinterpret_cast<const bf16x8 *>(blob + kAcFastA2 + BR * 65536) + nt * 4 * 64,
                          reinterpret_cast<const bf16x8 *>(blob + kAcFastA2 + BR * 65536 + 32768) + nt * 4 * 64,
                          reinterpret_cast<const float *>(bias_base + 512 * (1 + BR) + 64 * nt)};
        },
        [&](int q, const u32x4 (&ch)[QS_SPLIT_NET], const u32x4 (&cl)[QS_SPLIT_NET]) {
            const bf16x8 wh = *reinterpret_cast<const bf16x8 *>(a3_base + q * (BR == 0 ? 256 : 64));
            const bf16x8 wl = *reinterpret_cast<const bf16x8 *>(a3_base + q * (BR == 0 ? 256 : 64) + (BR == 0 ? 1024 : 256));
            mfma_split3(wh, wl, ch, cl, a3 + E0);
        });
}

template <int BR>
__device__ __forceinline__ void ac_fast_branch(const char *blob, int zeros, const u32x4 (&bh)[4][4], const u32x4 (&bl)[4][4], int lane,
                                               f32x4 (&a3)[4])
{
    init_a3(reinterpret_cast<const float *>(blob + kAcFastB) + 3 * kHid, lane, a3);
    ac_fast_branch_pass<BR, 0>(blob, zeros, bh, bl, lane, a3);
    if (QS_SPLIT_NET == 2) ac_fast_branch_pass<BR, QS_SPLIT_NET == 2 ? 2 : 0>(blob, zeros, bh, bl, lane, a3);
}

// The exact-float32 heads in the same pieces (layer 1: layer1_relu).  Each branch starts its OWN accumulators from the output
// bias; one set shared by both branches would add the other branch's exact zeros in a different place -- the same sums bit
// for bit.  mlp_heads relies on this: the one-wave kernel and the role-split kernel run these very functions.
// LDW2: row stride (floats) of W2p^T / W2v^T (the tower image interleaves the two: kLdW2T)
template <int BR, int LDW2 = kLdW>
__device__ __forceinline__ void ac_exact_branch(const AcLds &L, const f32x4 (&h1)[8][4], int lane, f32x4 (&a3)[4])
{
    const int c = lane & 15, g = lane >> 4;
    init_a3(L.B3, lane, a3);
    const float *W2 = (BR ? L.W2v : L.W2p) + c * LDW2 + 4 * g;          // + 16 nt LDW2 + 16 rt
    const float *B2 = (BR ? L.B2v : L.B2p) + 4 * g;                     // + 16 nt
    // output-layer A operand: row c of the 16-row tile; only rows 0..3 (policy) / row 4 (value) are non-zero -- every other
    // row reads 16 zero bytes (slots 8..11 of the padded b3): an address select, no branch in the MFMA stream
    const bool row_live = BR == 0 ? c < 4 : c == 4;
    const float *w3row = BR == 0 ? L.W3p + (c & 3) * kLdW + 4 * g : L.W3v + 4 * g;
    // Source order = issue order (scheduling barriers): the weights of k-group G + 1 (16 MFMAs = 512 matrix cycles later) are
    // requested before the MFMAs of group G, across tile boundaries too; left alone, hipcc emits read -> wait -> MFMAs and
    // exposes the LDS latency 4-5 times per tile (36.5 cycles per MFMA instead of the pipe's 32).
    f32x4 wbuf[2];
    wbuf[0] = *reinterpret_cast<const f32x4 *>(W2);
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const f32x4 bias = *reinterpret_cast<const f32x4 *>(B2 + 16 * nt);
        const f32x4 w3 = *reinterpret_cast<const f32x4 *>(row_live ? w3row + 16 * nt : L.B3 + 8);
        f32x4 h2[4] = {bias, bias, bias, bias};
#pragma unroll
        for (int rt = 0; rt < 8; ++rt) {
            const int G = 8 * nt + rt;
            if (G + 1 < 64) wbuf[(G + 1) & 1] = *reinterpret_cast<const f32x4 *>(W2 + 16 * ((G + 1) >> 3) * LDW2 + 16 * ((G + 1) & 7));
            const f32x4 w = wbuf[G & 1];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int et = 0; et < 4; ++et)
                    h2[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i], h1[rt][et][i], h2[et], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        f32x4 r[4];
#pragma unroll
        for (int et = 0; et < 4; ++et) r[et] = relu4(h2[et]);
#pragma unroll
        for (int i = 0; i < 4; ++i)                     // k-step outermost: consecutive MFMAs on different accumulators
#pragma unroll
            for (int et = 0; et < 4; ++et) a3[et] = __builtin_amdgcn_mfma_f32_16x16x4f32(w3[i], r[et][i], a3[et], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------------------------------------------------
// Tower actor-critic: the OTHER layout the reference trains and ships (every ppo2_docking*.zip; run_docking_gail.py:56),
// net_arch [dict(pi=[128, 128], vf=[128, 128])], ReLU -- no shared layer: pi_fc0 12->128 -> pi_fc1 128->128 -> pi 128->4 and
// vf_fc0 12->128 -> vf_fc1 128->128 -> vf 128->1 (rl_baselines/common/policies.py:35-92 with an empty shared part).
// Both Runner kernels evaluate it as the pieces of the shared-trunk heads plus a second layer 1: layer 1 (pi_fc0) -> policy
// branch -> layer 1 (vf_fc0) -> value branch, the second layer 1 written into the registers of the first (a role-split matrix
// wave holds ONE set of layer-1 B operands: 128 registers).  Per wave and step: 2 x 96 more f32 MFMAs than the shared trunk.
// Exact-f32 LDS image (floats): W2^T 128 x 260 (row r = pi_fc1^T row r | vf_fc1^T row r | 4 pad: a 1040-byte row meets the
// banks as the shared image's 528-byte row does, and pads 1 KiB where two 132-float images pad 4 KiB -- the room for the
// second layer 1) | W3pi^T 4x132 | W3vf 132 | W1pi^T 128x13 | W1vf^T 128x13 | b1pi 128 | b2pi 128 | b2vf 128 | b1vf 128 |
// b3 16 | per-wave stage 4 x 768  = 163 472 B.
// Split-bf16 image (bytes): the shared-trunk blob with pi_fc0 as its layer 1 (141 888) | W1vf^T f32 128x13 6656 | b1vf 512 |
// per-wave stage 4 x 3072  = 161 344 B, + 2 KiB of zeros for the dead output rows (ac_fast_branch) = 163 392 B.
// Neither leaves room for the role-split kernel's 1 KiB value buffer: its matrix waves hand the values over by ds_bpermute.
enum : int { kNetShared = 0, kNetTowers = 1 };

constexpr int kLdW2T = 2 * kHid + 4;

constexpr size_t tow_lds_floats()
{
    return (size_t)kHid * kLdW2T + 4 * kLdW + kLdW + 2 * kHid * kLdW1 + 4 * kHid + 16 + 4 * (12 * 64);
}

constexpr int kAcTowFastW1v = kAcFastBlobBytes;
constexpr int kAcTowFastB1v = kAcTowFastW1v + kHid * kLdW1 * 4;
constexpr int kAcTowFastBlobBytes = kAcTowFastB1v + kHid * 4;
constexpr int kAcTowFastLdsBytes = kAcTowFastBlobBytes + 4 * (12 * 64) * 4;
static_assert(tow_lds_floats() * 4 == 163472 && kAcTowFastLdsBytes == 161344, "tower LDS images as documented");

// The heads' LDS image as a wave addresses it.  FAST: the split-bf16 image at `blob`, its 2 KiB of zeros at byte `zeros`;
// else the exact image L, and for the towers Lv = L with W1 / B1 = vf_fc0 (L's = pi_fc0).
struct HeadsLds {
    const char *blob;
    int zeros;
    AcLds L, Lv;
};

// a wave's layer-1 result: FAST the split B operands of the 128 x 128 layer (bh / bl), else the f32 accumulators (h1)
template <bool FAST> using HeadB = u32x4[FAST ? 4 : 1][4];
template <bool FAST> using HeadH = f32x4[FAST ? 1 : 8][4];

// layer 1 of the wave's 64 envs from the observations in `stage`.  VF: vf_fc0 of the tower layout, else shared_fc0 / pi_fc0
template <bool FAST, bool VF>
__device__ __forceinline__ void heads_layer1(const HeadsLds &H, const float *stage, int lane, HeadB<FAST> &bh, HeadB<FAST> &bl, HeadH<FAST> &h1)
{
    if constexpr (FAST) ac_fast_layer1<VF ? kAcTowFastW1v : kAcFastW1, VF ? kAcTowFastB1v : kAcFastB>(H.blob, stage, lane, bh, bl);
    else layer1_relu(VF ? H.Lv.W1 : H.L.W1, VF ? H.Lv.B1 : H.L.B1, stage, lane, h1);
}

// branch BR (0 policy -> rows 0..3 of a3, 1 value -> row 4) from the layer-1 result
template <bool FAST, int NET, int BR>
__device__ __forceinline__ void heads_branch(const HeadsLds &H, const HeadB<FAST> &bh, const HeadB<FAST> &bl, const HeadH<FAST> &h1, int lane,
                                             f32x4 (&a3)[4])
{
    if constexpr (FAST) ac_fast_branch<BR>(H.blob, H.zeros, bh, bl, lane, a3);
    else ac_exact_branch<BR, NET == kNetTowers ? kLdW2T : kLdW>(H.L, h1, lane, a3);
}

// One wave per tile: obs (per owning lane) -> out[0..3] = action mean, out[4] = value (per owning lane).  `stage` = 768 floats
// per wave.  Towers: the second layer 1 is written into the registers of the first.
template <bool FAST, int NET>
__device__ __forceinline__ void mlp_heads(const float obs[12], float out[5], const HeadsLds &H, float *stage, int lane)
{
    stage_obs(obs, stage, lane);
    HeadB<FAST> bh, bl;
    HeadH<FAST> h1;
    f32x4 a3p[4], a3v[4];
    heads_layer1<FAST, false>(H, stage, lane, bh, bl, h1);
    heads_branch<FAST, NET, 0>(H, bh, bl, h1, lane, a3p);
    if constexpr (NET == kNetTowers) heads_layer1<FAST, true>(H, stage, lane, bh, bl, h1);
    heads_branch<FAST, NET, 1>(H, bh, bl, h1, lane, a3v);
    heads_to_owner(a3p, a3v, stage, lane, out);
}

// value of the env of this lane from row 4 of the value tile (register 0 of lanes 16..31) without LDS memory: lane l reads
// a3v[l >> 4][0] of lane 16 + (l & 15)
__device__ __forceinline__ float value_to_owner(const f32x4 (&a3v)[4], int lane)
{
    const int src = (16 + (lane & 15)) * 4;
    float v = 0.0f;
#pragma unroll
    for (int et = 0; et < 4; ++et) {
        const float y = a3v[et][0];
        const float x = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, y)));
        if ((lane >> 4) == et) v = x;
    }
    return v;
}

}  // namespace qs
