// dynplan_kernels.hpp -- the two kernels of qsd_shooting_plan (include/quadsim_dyn.h has the numerical contract).  A fragment
// of dynplan.hip, included after dynplan_image.hpp, nowhere else.
//
// k_dyn_plan<T1, T2>: CANDIDATES are the MFMA column dimension.  A wave owns one tile of 16 candidates of one env for the whole
// horizon; the work items (env, tile) are numbered env * tiles_per_env + tile and dealt to the waves of a persistent grid, so
// one env with 200 paths (13 tiles on 13 SIMDs) and 4096 envs (53 248 tiles) are the same loop.  A workgroup (4 waves) copies
// the weight image into LDS once and meets no barrier afterwards.
// Register layout: lane (c = l & 15, g = l >> 4) holds x[4 i + g] of candidate c in register i -- i < 3 the observation, i = 3
// component g of the action -- which is the B operand of layer-1 k-step i as it stands; the layer-1 accumulators are the B
// operands of layer 2, each finished tile of layer 2 goes straight into the one output tile (layer 3), and the output
// accumulator has the layout of x again (dynplan_image.hpp: the permutation pi).  With ONE column tile per wave H1 is T1 x 4
// registers (52 for the 208-wide net) and stays resident; the independent accumulators the 40-cycle MFMA latency asks for are
// four ROW tiles of the layer in flight instead of mlp_actor's four column tiles.  Per wave and model step:
// 4 T1 + 4 T1 T2 + 4 T2 MFMAs (444 for 13 x 7), one ds_read_b128 per 4 of them.
// k_dyn_finish: one workgroup per env reduces the env's scores in the total order of plan_better and regenerates the winner's
// actions, lane h drawing step h (k_shooting_plan step 4).  The kernel boundary is the only ordering between workgroups.
#pragma once
#include "quadsim_device.hpp"
#include "dynplan_image.hpp"

namespace qsd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DynArgs {
    const float *image;
    const float *obs;                // [n,12]
    uint64_t seed, gid0, k;
    int horizon, paths, tiles_per_env;
    int64_t n, tiles_total;
    double *scores;                  // [n,paths]: the caller's array or the workspace
    float *traj;                     // nullable [n,paths,horizon,12]
};

struct FinishArgs {
    uint64_t seed, gid0, k;
    int horizon, paths;
    const double *scores;            // [n,paths]
    float *actions;                  // [n,4]
    double *best_score;              // nullable [n]
    int32_t *best_index;             // nullable [n]
    float *sequence;                 // nullable [n,horizon,4]
};

// actions of candidate c at horizon step h, planned before global step k: plan_action of shooting.hpp
__device__ __forceinline__ void plan_action(uint64_t seed, uint64_t gid, uint64_t k, unsigned c, unsigned h, float a[4])
{
    const uint4 w = qs::philox_block(seed, qs::STREAM_PLAN, gid, (k << 26) | ((uint64_t)c << 10) | (uint64_t)h);
    a[0] = qs::sym(qs::u01(w.x)); a[1] = qs::sym(qs::u01(w.y)); a[2] = qs::sym(qs::u01(w.z)); a[3] = qs::sym(qs::u01(w.w));
}

// the total order of the reduction: higher score first, then lower index (plan_better of shooting.hpp)
__device__ __forceinline__ bool plan_better(double s, int i, double bs, int bi) { return s > bs || (s == bs && i < bi); }

// (a select, not fmaxf: fmaxf drops a NaN operand, and a net with a NaN weight would plan on as one with a dead unit.  -0 <= 0
// holds: -0 still becomes +0)
__device__ __forceinline__ float relu1(float z) { return z <= 0.0f ? 0.0f : z; }
__device__ __forceinline__ f32x4 relu4(f32x4 v)
{
    return f32x4{relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w)};
}

constexpr int kDynBlock = 256;       // 4 waves: one per SIMD while the 118 KB image leaves room for one workgroup per CU
constexpr int kRowGroup = 4;         // row tiles of a layer in flight = independent MFMA accumulators

// one model step of the wave's 16 candidates: xh (normalised input, register i = input 4 i + g) -> the 16-row output tile
template <int T1, int T2>
__device__ __forceinline__ f32x4 dyn_net(const float *img, const f32x4 xh, int c, int g)
{
    constexpr ImageLayout L = image_layout(T1, T2);
    const float *W1 = img + L.w1 + c * L.ld1 + 4 * g;      // + 16 rt ld1
    const float *B1 = img + L.b1 + 4 * g;                  // + 16 rt
    const float *W2 = img + L.w2 + c * L.ld2 + 4 * g;      // + 16 nt ld2 + 16 rt
    const float *B2 = img + L.b2 + 4 * g;                  // + 16 nt
    const float *W3 = img + L.w3 + c * L.ld3 + 4 * g;      // + 16 nt
    f32x4 h1[T1];
#pragma unroll
    for (int r0 = 0; r0 < T1; r0 += kRowGroup) {
        f32x4 acc[kRowGroup], w[kRowGroup];
#pragma unroll
        for (int j = 0; j < kRowGroup; ++j)
            if (r0 + j < T1) {
                acc[j] = *reinterpret_cast<const f32x4 *>(B1 + 16 * (r0 + j));
                w[j] = *reinterpret_cast<const f32x4 *>(W1 + 16 * (r0 + j) * L.ld1);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)                         // k-step outermost: consecutive MFMAs on different accumulators
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j)
                if (r0 + j < T1) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][i], xh[i], acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < kRowGroup; ++j)
            if (r0 + j < T1) h1[r0 + j] = relu4(acc[j]);
    }
    f32x4 a3 = *reinterpret_cast<const f32x4 *>(img + L.b3 + 4 * g);
#pragma unroll
    for (int n0 = 0; n0 < T2; n0 += kRowGroup) {
        f32x4 h2[kRowGroup];
#pragma unroll
        for (int j = 0; j < kRowGroup; ++j)
            if (n0 + j < T2) h2[j] = *reinterpret_cast<const f32x4 *>(B2 + 16 * (n0 + j));
#pragma unroll
        for (int rt = 0; rt < T1; ++rt) {
            f32x4 w[kRowGroup];
#pragma unroll
            for (int j = 0; j < kRowGroup; ++j)
                if (n0 + j < T2) w[j] = *reinterpret_cast<const f32x4 *>(W2 + 16 * (n0 + j) * L.ld2 + 16 * rt);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < kRowGroup; ++j)
                    if (n0 + j < T2) h2[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][i], h1[rt][i], h2[j], 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < kRowGroup; ++j)
            if (n0 + j < T2) {
                const f32x4 r = relu4(h2[j]);
                const f32x4 w3 = *reinterpret_cast<const f32x4 *>(W3 + 16 * (n0 + j));
#pragma unroll
                for (int i = 0; i < 4; ++i) a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(w3[i], r[i], a3, 0, 0, 0);
            }
    }
    return a3;
}

template <int T1, int T2>
__global__ __launch_bounds__(kDynBlock) void k_dyn_plan(DynArgs A)
{
    constexpr ImageLayout L = image_layout(T1, T2);
    __shared__ __align__(16) float img[L.floats];
    // the header names the instantiation the image was packed for: anything else is not read past its first 16 bytes
    const uint4 hdr = *reinterpret_cast<const uint4 *>(A.image);
    if (hdr.x != kMagic || hdr.y != (uint32_t)T1 || hdr.z != (uint32_t)T2 || hdr.w != (uint32_t)L.floats) return;
    for (int i = threadIdx.x; i < L.floats / 4; i += kDynBlock)
        reinterpret_cast<float4 *>(img)[i] = reinterpret_cast<const float4 *>(A.image)[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int H = A.horizon;
    const int steps = A.traj ? H : H - 1;                                // the last prediction enters no score

    for (int64_t t = (int64_t)blockIdx.x * (kDynBlock / 64) + wave; t < A.tiles_total; t += (int64_t)gridDim.x * (kDynBlock / 64)) {
        const int64_t env = t / A.tiles_per_env;
        const int cand = (int)(t % A.tiles_per_env) * 16 + c;
        const bool valid = cand < A.paths;
        const unsigned cc = (unsigned)(valid ? cand : A.paths - 1);       // columns past the end repeat the last candidate, unstored
        const uint64_t gid = A.gid0 + (uint64_t)env;

        f32x4 x;                                                         // x[i] = input 4 i + g: obs word 4 i + g (i < 3), action word g
#pragma unroll
        for (int i = 0; i < 3; ++i) x[i] = A.obs[env * 12 + 4 * i + g];
        x[3] = 0.0f;
        double score = 0.0;
        float *tr = A.traj ? A.traj + ((env * A.paths + cc) * (int64_t)H) * 12 + g : nullptr;
#pragma clang loop unroll(disable)
        for (int h = 0; h < H; ++h) {
            // rel_pos = inputs 0, 1, 2 = register 0 of the lanes g = 0, 1, 2 of this column
            const float p0 = __shfl(x[0], c), p1 = __shfl(x[0], c + 16), p2 = __shfl(x[0], c + 32);
            score += (double)(-__fmaf_rn(p2, p2, __fmaf_rn(p1, p1, p0 * p0)));
            if (h >= steps) break;
            float a[4];
            plan_action(A.seed, gid, A.k, cc, (unsigned)h, a);
            x[3] = g == 0 ? a[0] : g == 1 ? a[1] : g == 2 ? a[2] : a[3];
            f32x4 xh;
#pragma unroll
            for (int i = 0; i < 4; ++i) xh[i] = (x[i] - img[L.norm + 4 * i + g]) * img[L.norm + 16 + 4 * i + g];
            const f32x4 d = dyn_net<T1, T2>(img, xh, c, g);
#pragma unroll
            for (int i = 0; i < 3; ++i) x[i] = __fmaf_rn(d[i], img[L.norm + 32 + 4 * i + g], img[L.norm + 48 + 4 * i + g]) + x[i];
            if (tr && valid) {
#pragma unroll
                for (int i = 0; i < 3; ++i) tr[h * 12 + 4 * i] = x[i];
            }
        }
        if (valid && g == 0) A.scores[env * A.paths + cand] = score;
    }
}

__global__ __launch_bounds__(kDynBlock) void k_dyn_finish(FinishArgs X)
{
    __shared__ double red_s[kDynBlock / 64];
    __shared__ int red_i[kDynBlock / 64];
    __shared__ int winner;
    const int64_t env = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double *S = X.scores + env * X.paths;
    double best_s = -__builtin_huge_val();
    int best_i = 0x7fffffff;
    for (int c = threadIdx.x; c < X.paths; c += kDynBlock) {
        const double s = S[c];
        if (plan_better(s, c, best_s, best_i)) { best_s = s; best_i = c; }
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
        for (int w = 1; w < kDynBlock / 64; ++w)
            if (plan_better(red_s[w], red_i[w], best_s, best_i)) { best_s = red_s[w]; best_i = red_i[w]; }
        if (best_i == 0x7fffffff) best_i = 0;             // every score NaN: still a valid index
        winner = best_i;
        if (X.best_score) X.best_score[env] = S[best_i];  // the stored score itself: NaN bits included
        if (X.best_index) X.best_index[env] = best_i;
    }
    __syncthreads();
    const int win = winner;
    const uint64_t gid = X.gid0 + (uint64_t)env;
    for (int h = threadIdx.x; h < X.horizon; h += kDynBlock) {
        float a[4];
        plan_action(X.seed, gid, X.k, (unsigned)win, (unsigned)h, a);
        const float4 v = make_float4(a[0], a[1], a[2], a[3]);
        if (h == 0) reinterpret_cast<float4 *>(X.actions)[env] = v;
        if (X.sequence) reinterpret_cast<float4 *>(X.sequence)[env * X.horizon + h] = v;
    }
}

}  // namespace qsd
