// dynmppi_kernels.hpp -- the two kernels of qsdm_mppi_plan (include/quadsim_dyn_mppi.h has the numerical contract): MPPI over
// the learned dynamics net.  A fragment of dynmppi.hip, nowhere else.  The model step (dyn_net), relu4, the image layout and
// kMagic are dynplan_kernels.hpp's, included unchanged: one model step and one set of bits for both planners over the net.
// (That header's non-template k_dyn_finish and k_dyn_pack are compiled into this code object too and never launched here.)
//
// Per iteration two launches; the boundary between them is the only ordering between workgroups.
// k_dynm_roll<T1, T2>: k_dyn_plan's persistent loop with the action source replaced -- the same (env, tile) work items dealt to
//   the waves of a persistent grid, the same register layout (lane (c = l & 15, g = l >> 4) holds x[4 i + g] of candidate c in
//   register i), the weight image copied into LDS once per workgroup and no barrier afterwards.  The action of lane (c, g) at
//   step h is component g of candidate c: clamp(fma(sigma, z_g, U[h][g])), U[h] of the tile's env a wave-uniform 16-byte
//   load, z the caller's noise or the keyed draw (candidate 0: clamp(U[h][g]), no draw).  Writes the float64 score per
//   candidate into the workspace, and traj in the last iteration.
// k_dynm_update: one workgroup of kUpdBlock threads per env, whatever `paths` (so the summation order is a function of `paths`
//   alone).  The nominal is read into LDS before anything is written (nominal_in may alias nominal_out); Smax over the non-NaN
//   scores; the weights exp((S - Smax) / lambda) overwrite the scores IN THE WORKSPACE (65 536 float64 do not fit LDS); then
//   k_mppi's pass 2 with ROWS of 8 lanes in the place of waves, 8 horizon steps at a time: lanes over h, rows over c, row r of
//   128 adding w[c] a[c][h] for c = r, r + 128, ... in ascending order into float64 sums (the candidates regenerated from their
//   keys or re-read from `noise`, never stored between the launches), the rows then added in row order.  Writes the new U and trace; in the last iteration candidates,
//   nominal_out, actions and best_score as well.
#pragma once
#include "dynplan_kernels.hpp"

namespace qsd {

// what a candidate's actions are drawn from, common to both kernels
struct DrawArgs {
    uint64_t seed, gid0, k;
    int horizon, paths, it;
    float sigma;
    const float *noise;              // nullable [iterations,paths,horizon,4]
};

struct RollArgs {
    const float *image;
    const float *obs;                // [n,12]
    DrawArgs D;
    const float *U;                  // [n,horizon,4]: nominal_in (iteration 0, nullable: zeros) or the workspace's nominal
    int shift;                       // U[h] = row min(h + shift, horizon - 1)
    int tiles_per_env;
    int64_t tiles_total;
    double *scores;                  // the workspace's [n,paths]
    float *traj;                     // nullable [n,paths,horizon,12]: given in the last iteration only
};

struct UpdateArgs {
    const float *image;              // only its header is read
    int t1, t2, floats;              // the header the host expects
    DrawArgs D;
    int iterations, shift;
    double lambda;                   // the caller's float, widened on the host
    const float *U_in;               // as RollArgs::U
    float *U_ws;                     // the workspace's nominal [n,horizon,4]
    double *S;                       // the workspace's scores [n,paths]: become the weights
    float *actions;                  // [n,4]
    float *nominal_out;              // [n,horizon,4]
    double *best_score;              // nullable [n]
    double *scores;                  // nullable [n,iterations,paths]
    float *trace;                    // nullable [n,iterations+1,horizon,4]
    float *candidates;               // nullable [n,paths,horizon,4]
};

// the four normals behind candidate c >= 1 at horizon step h: mppi_action's of mppi.hpp (k < 2^33, it < 2^4, c < 2^16, h < 2^10)
__device__ __forceinline__ void dynm_normals(const DrawArgs &D, uint64_t gid, int c, int h, float z[4])
{
    if (D.noise) {
        const float4 v = reinterpret_cast<const float4 *>(D.noise)[((int64_t)D.it * D.paths + c) * D.horizon + h];
        z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
    } else {
        const uint64_t blk = (1ull << 63) | (D.k << 30) | ((uint64_t)D.it << 26) | ((uint64_t)c << 10) | (uint64_t)h;
        qs::normals_from_words(qs::philox_counter(D.seed, ((uint64_t)qs::STREAM_PLAN << 48) | gid, blk), z);
    }
}

// actions of candidate c at horizon step h around the nominal u: mppi_action of mppi.hpp
__device__ __forceinline__ void dynm_action(const DrawArgs &D, uint64_t gid, int c, int h, const float4 &u, float a[4])
{
    if (c == 0) {                                         // the nominal itself, no draw
        a[0] = qs::clamp1(u.x); a[1] = qs::clamp1(u.y); a[2] = qs::clamp1(u.z); a[3] = qs::clamp1(u.w);
        return;
    }
    float z[4];
    dynm_normals(D, gid, c, h, z);
    const float s = D.sigma;
    a[0] = qs::clamp1(__fmaf_rn(s, z[0], u.x)); a[1] = qs::clamp1(__fmaf_rn(s, z[1], u.y));
    a[2] = qs::clamp1(__fmaf_rn(s, z[2], u.z)); a[3] = qs::clamp1(__fmaf_rn(s, z[3], u.w));
}

template <int T1, int T2>
__global__ __launch_bounds__(kDynBlock) void k_dynm_roll(RollArgs A)
{
    constexpr ImageLayout L = image_layout(T1, T2);
    __shared__ __align__(16) float img[L.floats];
    // the header names the instantiation the image was packed for: anything else is not read past its first 16 bytes
    const uint4 hdr = *reinterpret_cast<const uint4 *>(A.image);
    if (hdr.x != kMagic || hdr.y != (uint32_t)T1 || hdr.z != (uint32_t)T2 || hdr.w != (uint32_t)L.floats) return;
    for (int i = threadIdx.x; i < L.floats / 4; i += kDynBlock)
        reinterpret_cast<float4 *>(img)[i] = reinterpret_cast<const float4 *>(A.image)[i];
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);    // the tile, its env and U[h] are wave-uniform
    const int c = lane & 15, g = lane >> 4;
    const int H = A.D.horizon;
    const int steps = A.traj ? H : H - 1;                                // the last prediction enters no score

    for (int64_t t = (int64_t)blockIdx.x * (kDynBlock / 64) + wave; t < A.tiles_total; t += (int64_t)gridDim.x * (kDynBlock / 64)) {
        const int64_t env = t / A.tiles_per_env;
        const int cand = (int)(t % A.tiles_per_env) * 16 + c;
        const bool valid = cand < A.D.paths;
        const int cc = valid ? cand : A.D.paths - 1;                     // columns past the end repeat the last candidate, unstored
        const uint64_t gid = A.D.gid0 + (uint64_t)env;
        const float4 *Urow = A.U ? reinterpret_cast<const float4 *>(A.U) + env * H : nullptr;

        f32x4 x;                                                         // x[i] = input 4 i + g: obs word 4 i + g (i < 3), action word g
#pragma unroll
        for (int i = 0; i < 3; ++i) x[i] = A.obs[env * 12 + 4 * i + g];
        x[3] = 0.0f;
        double score = 0.0;
        float *tr = A.traj ? A.traj + ((env * A.D.paths + cc) * (int64_t)H) * 12 + g : nullptr;
#pragma clang loop unroll(disable)
        for (int h = 0; h < H; ++h) {
            // rel_pos = inputs 0, 1, 2 = register 0 of the lanes g = 0, 1, 2 of this column
            const float p0 = __shfl(x[0], c), p1 = __shfl(x[0], c + 16), p2 = __shfl(x[0], c + 32);
            score += (double)(-__fmaf_rn(p2, p2, __fmaf_rn(p1, p1, p0 * p0)));
            if (h >= steps) break;
            const float4 u = Urow ? Urow[min(h + A.shift, H - 1)] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float a[4];
            dynm_action(A.D, gid, cc, h, u, a);
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
        if (valid && g == 0) A.scores[env * A.D.paths + cand] = score;
    }
}

// The update workgroup is fixed, so that the summation order is a function of `paths` alone: 16 waves, each of 8 ROWS of 8
// lanes -- 128 rows over the candidates, 8 lanes over the horizon steps of a chunk.  One env's update is ONE workgroup, and at
// 65 536 paths x 20 steps it draws 1.3 M normals on one compute unit, so what matters is how many lanes draw: with whole waves
// over h (k_mppi's pass 2 as it stands) 20 of 64 lanes work at horizon 20, and 4 / 16 waves took 7.5 / 4.2 ms per iteration on an
// MI355X against 3.3 ms for the whole plan composed from torch calls; with 8-lane rows 20 of 24 work.
constexpr int kUpdBlock = 1024;
constexpr int kUpdWaves = kUpdBlock / 64;
constexpr int kRowLanes = 8;
constexpr int kUpdRows = kUpdBlock / kRowLanes;

__global__ __launch_bounds__(kUpdBlock) void k_dynm_update(UpdateArgs X)
{
    __shared__ float4 U[1024];                            // the nominal of this env (QSDM_MAX_HORIZON rows)
    __shared__ double part[kUpdRows][kRowLanes][4];       // per-row partial sums of one chunk of kRowLanes horizon steps
    __shared__ double red_s[kUpdWaves], red_w[kUpdRows];
    // an image of another instantiation: the roll-out wrote no score, so nothing is written here either
    const uint4 hdr = *reinterpret_cast<const uint4 *>(X.image);
    if (hdr.x != kMagic || hdr.y != (uint32_t)X.t1 || hdr.z != (uint32_t)X.t2 || hdr.w != (uint32_t)X.floats) return;

    const int64_t env = blockIdx.x;                       // the grid is n workgroups
    const int tid = threadIdx.x, ln = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = X.D.horizon, paths = X.D.paths, it = X.D.it;
    const bool last = it == X.iterations - 1;
    const uint64_t gid = X.D.gid0 + (uint64_t)env;
    double *const S = X.S + env * paths;

    // all of the nominal is read before anything is written: nominal_in may alias nominal_out
    for (int h = tid; h < H; h += kUpdBlock) {
        float4 u = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (X.U_in) u = reinterpret_cast<const float4 *>(X.U_in)[env * H + min(h + X.shift, H - 1)];
        U[h] = u;
    }
    double smax = -__builtin_huge_val();
    for (int c = tid; c < paths; c += kUpdBlock) {
        const double s = S[c];
        if (s > smax) smax = s;                           // a NaN never enters
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double os = __shfl_xor(smax, m);
        if (os > smax) smax = os;
    }
    if (ln == 0) red_s[wv] = smax;
    __syncthreads();
    for (int w = 0; w < kUpdWaves; ++w)
        if (red_s[w] > smax) smax = red_s[w];
    if (it == 0 && X.trace)
        for (int h = tid; h < H; h += kUpdBlock) reinterpret_cast<float4 *>(X.trace)[env * (X.iterations + 1) * H + h] = U[h];
    // weights over the scores, each by the thread that read the score above
    for (int c = tid; c < paths; c += kUpdBlock) {
        const double s = S[c];
        if (X.scores) X.scores[(env * X.iterations + it) * paths + c] = s;
        const double w = exp((s - smax) / X.lambda);
        S[c] = w == w ? w : 0.0;                          // NaN score, or no finite Smax
    }
    __syncthreads();                                      // the weights are read by every wave below

    // pass 2 (k_mppi's, with rows of 8 lanes in the place of waves): lanes over h, rows over c.  Row r adds w[c] a[c][h] for
    // c = r, r + 128, ... in ascending order; the rows are then added in row order.
    const int row = tid / kRowLanes, hl = tid % kRowLanes;
    for (int h0 = 0; h0 < H; h0 += kRowLanes) {
        const int h = h0 + hl;
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0, sw = 0.0;
        if (h < H) {
            const float4 u = U[h];
#pragma clang loop unroll(disable)
            for (int c = row; c < paths; c += kUpdRows) {
                const double w = S[c];
                float a[4];
                dynm_action(X.D, gid, c, h, u, a);
                if (last && X.candidates)
                    reinterpret_cast<float4 *>(X.candidates)[(env * paths + c) * H + h] = make_float4(a[0], a[1], a[2], a[3]);
                acc0 = fma(w, (double)a[0], acc0); acc1 = fma(w, (double)a[1], acc1);
                acc2 = fma(w, (double)a[2], acc2); acc3 = fma(w, (double)a[3], acc3);
                sw += w;
            }
        }
        double *p = part[row][hl];
        p[0] = acc0; p[1] = acc1; p[2] = acc2; p[3] = acc3;
        if (h == 0) red_w[row] = sw;                      // the same sum on every lane of the row: kept from the first chunk
        __syncthreads();
        if (tid < kRowLanes && h < H) {                   // row 0: lane h adds the partial sums in row order
            double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, tw = 0.0;
            for (int r = 0; r < kUpdRows; ++r) {
                const double *q = part[r][hl];
                t0 += q[0]; t1 += q[1]; t2 += q[2]; t3 += q[3];
                tw += red_w[r];
            }
            float4 u = U[h];
            if (tw > 0.0) u = make_float4((float)(t0 / tw), (float)(t1 / tw), (float)(t2 / tw), (float)(t3 / tw));
            reinterpret_cast<float4 *>(X.U_ws)[env * H + h] = u;
            if (X.trace) reinterpret_cast<float4 *>(X.trace)[(env * (X.iterations + 1) + it + 1) * H + h] = u;
            if (last) {
                reinterpret_cast<float4 *>(X.nominal_out)[env * H + h] = u;
                if (h == 0) reinterpret_cast<float4 *>(X.actions)[env] = u;
            }
        }
        __syncthreads();                                  // `part` is reused by the next chunk
    }
    if (last && tid == 0 && X.best_score) X.best_score[env] = smax;
}

}  // namespace qsd
