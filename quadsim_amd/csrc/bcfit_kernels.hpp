// bcfit_kernels.hpp -- the kernels of libquadsim_bc.so (include/quadsim_bc.h has the numerical contract).  A fragment of
// bcfit.hip, nowhere else.  Shared with the fourth library at the source level: forward_layer, adam_step, ld4 / st4 and the
// chunk geometry (kFitBlock, kRows, kRP) of dynfit_kernels.hpp.
//
// k_bc_fit: ONE workgroup of 512 threads runs every Adam step of the call on the actor 12 -> 128 -> 128 -> 4.  The policy stores
// its weights (in, out); in LDS they lie (out, in), rows LD = in + 4 floats apart, as dynfit_kernels.hpp explains.  What differs
// from k_dyn_fit, all of it to shorten a step of ONE chunk (batch 10 of the reference is one chunk):
//   * Adam's m and v of a thread's elements live in REGISTERS for the whole call (32 + 4 + 1 + 1 elements a thread), the weight
//     in LDS: a step reads the step's rows from memory and writes its loss, nothing else.  w, m, v go back to memory once, after
//     the last step.
//   * dz1 and dz0 have buffers of their own, so the gradient of a layer and the back-propagation through it share a phase: a
//     chunk has 7 workgroup barriers, not 10.  The output layer computes e and dy in the same item as y.
//   * the back-propagation into the first hidden layer, 128 items of a 128-term chain in k_dyn_fit, is four interleaved chains
//     per element on four lanes (512 items of 32 terms), added over cross-lane shuffles in the fixed tree of the header.
//   * the first chunk of step s + 1 is fetched while step s runs: its indices at the top of step s, its rows before Adam.
// All ordering is __syncthreads; every product is a plain fmaf chain.
#pragma once
#include "dynfit_kernels.hpp"

namespace qsb {

using qsf::adam_step;
using qsf::Adam;
using qsf::f32x4;
using qsf::forward_layer;
using qsf::kFitBlock;
using qsf::kRG;
using qsf::kRows;
using qsf::kRP;
using qsf::ld4;
using qsf::st4;

constexpr int kIn = 12, kInP = 16, kH = 128, kOut = 4;
constexpr int kLossRows = 256;                   // rows of a block of k_bc_loss (QSBC_LOSS_BLOCK)
constexpr int kSumBlock = 256;

struct FitArgs {
    float *w[6], *m[6], *v[6];                   // w0 b0 w1 b1 w2 b2 and their moments
    float *grads[6];                             // nullable as a whole (grads[0] == nullptr)
    const float *obs, *act;
    const int32_t *indices, *counts;             // [steps,batch], nullable [steps]
    float *loss;                                 // [steps]
    double lr, beta1, beta2;
    float b1f, b2f, omb1, omb2, eps;
    int steps, batch, t0;
};

struct LossArgs {
    const float *w[6];
    const float *obs, *act;
    const int32_t *rows;                         // nullable [count]
    double *partials;                            // [blocks]
    int count, blocks;
};

struct Layout {
    static constexpr int ld1 = kInP + 4, ld2 = kH + 4, ld3 = kH + 4;
    static constexpr int w1 = 0, b1 = w1 + kH * ld1, w2 = b1 + kH, b2 = w2 + kH * ld2, w3 = b2 + kH, b3 = w3 + kOut * ld3;
    static constexpr int x = b3 + 16, a1 = x + kInP * kRP, a2 = a1 + kH * kRP, y = a2 + kH * kRP, th = y + kOut * kRP;
    static constexpr int net_floats = th + kOut * kRP;           // what k_bc_loss needs
    static constexpr int d2 = net_floats, d1 = d2 + kH * kRP;    // dz1 and dz0
    static constexpr int scal = d1 + kH * kRP;                   // lr_t, dscale, 4 rows
    static constexpr int floats = scal + 4;
};

// the net into LDS: zero everything (the padding stays zero for the whole call), then the weights, transposed
template <int FLOATS>
__device__ __forceinline__ void load_net(float *lds, const float *const *w)
{
    using L = Layout;
    const int t = threadIdx.x;
    for (int i = t; i < FLOATS; i += kFitBlock) lds[i] = 0.0f;
    __syncthreads();
    for (int i = t; i < kIn * kH; i += kFitBlock) lds[L::w1 + (i & (kH - 1)) * L::ld1 + (i >> 7)] = w[0][i];
    for (int i = t; i < kH * kH; i += kFitBlock) lds[L::w2 + (i & (kH - 1)) * L::ld2 + (i >> 7)] = w[2][i];
    for (int i = t; i < kH * kOut; i += kFitBlock) lds[L::w3 + (i & (kOut - 1)) * L::ld3 + (i >> 2)] = w[4][i];
    if (t < kH) { lds[L::b1 + t] = w[1][t]; lds[L::b2 + t] = w[3][t]; }
    if (t < kOut) lds[L::b3 + t] = w[5][t];
    __syncthreads();
}

// thread t < 256 of a chunk holds element (row t & 15, column t >> 4): columns 0 .. 11 of obs, then the 4 of act
__device__ __forceinline__ float load_value(const float *obs, const float *act, int idx)
{
    const int c = threadIdx.x >> 4;
    if (idx < 0) return 0.0f;
    return c < kIn ? obs[(int64_t)idx * kIn + c] : act[(int64_t)idx * kOut + (c - kIn)];
}

__device__ __forceinline__ void stage_value(float *lds, float val)
{
    const int t = threadIdx.x, r = t & (kRows - 1), c = t >> 4;
    if (t < (kIn + kOut) * kRows) lds[(c < kIn ? Layout::x + c * kRP : Layout::th + (c - kIn) * kRP) + r] = val;
}

__global__ __launch_bounds__(kFitBlock) void k_bc_fit(FitArgs F)
{
    using L = Layout;
    static_assert(L::floats * 4 <= 160 * 1024, "LDS");
    static_assert(kFitBlock == 512 && kRows == 16 && kH == 128, "the thread maps below");
    __shared__ __align__(16) float lds[L::floats];
    const int t = threadIdx.x;
    load_net<L::floats>(lds, F.w);

    // ---- the elements of this thread, in the policy's (in, out) layout
    const int ti = t & 31, to = t >> 5;                  // w1: inputs 8 to + a, outputs ti + 32 j
    const int o1 = t & 127, ig1 = t >> 7;                // w0: output o1, inputs 4 ig1 + a (ig1 == 3: the zero padding, no element)
    const int o3 = t & 3, i3 = t >> 2;                   // w2: input i3, output o3
    const bool own1 = ig1 < 3;
    const int bk = t < 128 ? 0 : t < 256 ? 1 : t < 260 ? 2 : -1, bu = t & 127;   // one bias at most: b0, b1 or b2, unit bu
    const int bi = bk < 0 ? 0 : 2 * bk + 1, blds = bk == 0 ? L::b1 : bk == 1 ? L::b2 : L::b3;
    float m2[8][4], v2[8][4], m1[4] = {}, v1[4] = {}, m3, v3, mb = 0.0f, vb = 0.0f;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = (8 * to + a) * kH + ti + 32 * j;
            m2[a][j] = F.m[2][idx];
            v2[a][j] = F.v[2][idx];
        }
    if (own1) {
#pragma unroll
        for (int a = 0; a < 4; ++a) { m1[a] = F.m[0][(4 * ig1 + a) * kH + o1]; v1[a] = F.v[0][(4 * ig1 + a) * kH + o1]; }
    }
    m3 = F.m[4][t];
    v3 = F.v[4][t];
    if (bk >= 0) { mb = F.m[bi][bu]; vb = F.v[bi][bu]; }

    auto row_count = [&](int s) {
        const int r = F.counts ? F.counts[s] : F.batch;
        return r < F.batch ? r : F.batch;
    };
    auto load_index = [&](int s, int rows, int r0) {
        const int j = r0 + (t & (kRows - 1));
        return (t < (kIn + kOut) * kRows && j < rows) ? F.indices[(int64_t)s * F.batch + j] : -1;
    };

    int rows = row_count(0);
    float pre = load_value(F.obs, F.act, load_index(0, rows, 0));
    float g2[8][4], g1[4], g3, gb;

    for (int it = 0; it < F.steps; ++it) {
        const bool more = it + 1 < F.steps;
        int nrows = 0, nidx = -1;
        if (more) { nrows = row_count(it + 1); nidx = load_index(it + 1, nrows, 0); }
        if (t == 0) {
            const double tt = (double)(F.t0 + it) + 1.0;
            lds[L::scal] = (float)(F.lr * sqrt(1.0 - pow(F.beta2, tt)) / (1.0 - pow(F.beta1, tt)));
            lds[L::scal + 1] = (float)(2.0 / (4.0 * (double)rows));
            lds[L::scal + 2] = (float)(4 * rows);
        }
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) g2[a][j] = 0.0f;
#pragma unroll
        for (int a = 0; a < 4; ++a) g1[a] = 0.0f;
        g3 = 0.0f;
        gb = 0.0f;
        float lsum = 0.0f;                                // thread 448: the squared error of the rows so far

        for (int r0 = 0; r0 < rows; r0 += kRows) {
            // -- the chunk's rows; rows past the step's count are zeros.  (From the second chunk on: phase C of the chunk
            // before still reads x)
            if (r0 > 0) {
                __syncthreads();
                pre = load_value(F.obs, F.act, load_index(it, rows, r0));
            }
            stage_value(lds, pre);
            __syncthreads();
            forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
            __syncthreads();
            forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
            __syncthreads();
            // -- the mean head, one output x four rows an item, then in the same item e = y - a_expert over th and
            // dy = e dscale over y; rows past the count give zero
            if (t < kOut * kRG) {
                const int u = t >> 2, rg = t & 3;
                const float b = lds[L::b3 + u], dscale = lds[L::scal + 1];
                f32x4 acc = {b, b, b, b};
                const float *w = lds + L::w3 + u * L::ld3, *a = lds + L::a2 + 4 * rg;
                for (int k = 0; k < kH; k += 4) {
                    const f32x4 wk = ld4(w + k);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const f32x4 ak = ld4(a + (k + i) * kRP);
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(wk[i], ak[r], acc[r]);
                    }
                }
                const f32x4 th = ld4(lds + L::th + u * kRP + 4 * rg);
                f32x4 e, dy;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    e[r] = r0 + 4 * rg + r < rows ? __fsub_rn(acc[r], th[r]) : 0.0f;
                    dy[r] = __fmul_rn(e[r], dscale);
                }
                st4(lds + L::th + u * kRP + 4 * rg, e);
                st4(lds + L::y + u * kRP + 4 * rg, dy);
            }
            __syncthreads();
            // -- phase A: the loss, the gradient of the head from (dy, a1), dz1 from (w2, dy) under a1's mask
            if (t == 448) {
                for (int r = 0; r < kRows && r0 + r < rows; ++r) {
                    float s = 0.0f;
#pragma unroll
                    for (int o = 0; o < kOut; ++o) { const float d = lds[L::th + o * kRP + r]; s = __fmaf_rn(d, d, s); }
                    lsum = __fadd_rn(lsum, s);
                }
            }
#pragma clang loop unroll(disable)
            for (int rg = 0; rg < kRG; ++rg) {
                const f32x4 a = ld4(lds + L::a2 + i3 * kRP + 4 * rg), d = ld4(lds + L::y + o3 * kRP + 4 * rg);
#pragma unroll
                for (int r = 0; r < 4; ++r) g3 = __fmaf_rn(d[r], a[r], g3);
            }
            if (bk == 2) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) gb = __fadd_rn(gb, lds[L::y + bu * kRP + r]);
            }
            if (t < (kH >> 2) * kRG) {
                const int ig = t >> 2, rg = t & 3;
                f32x4 acc[4] = {};
#pragma unroll
                for (int o = 0; o < kOut; ++o) {
                    const f32x4 wo = ld4(lds + L::w3 + o * L::ld3 + 4 * ig), dz = ld4(lds + L::y + o * kRP + 4 * rg);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[a][r] = __fmaf_rn(wo[a], dz[r], acc[a][r]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const f32x4 hv = ld4(lds + L::a2 + (4 * ig + a) * kRP + 4 * rg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[a][r] = hv[r] > 0.0f ? acc[a][r] : 0.0f;
                    st4(lds + L::d2 + (4 * ig + a) * kRP + 4 * rg, acc[a]);
                }
            }
            __syncthreads();
            // -- phase B: the gradient of layer 1 from (dz1, a0), dz0 from (w1, dz1) under a0's mask
#pragma clang loop unroll(disable)
            for (int rg = 0; rg < kRG; ++rg) {
                f32x4 dz[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) dz[j] = ld4(lds + L::d2 + (ti + 32 * j) * kRP + 4 * rg);
#pragma unroll
                for (int a = 0; a < 8; ++a) {
                    const f32x4 av = ld4(lds + L::a1 + (8 * to + a) * kRP + 4 * rg);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) g2[a][j] = __fmaf_rn(dz[j][r], av[r], g2[a][j]);
                }
            }
            if (bk == 1) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) gb = __fadd_rn(gb, lds[L::d2 + bu * kRP + r]);
            }
            {
                // four inputs x four rows an item, its 128-term sum over four lanes: chain q takes o = q, q + 4, ...
                const int lane = t & 63, wv = t >> 6;
                const int q = lane >> 4, ig = (lane & 15) + 16 * (wv & 1), rg = wv >> 1;
                f32x4 acc[4] = {};
                const float *w = lds + L::w2 + 4 * ig, *d = lds + L::d2 + 4 * rg;
                for (int o = q; o < kH; o += 4) {
                    const f32x4 wo = ld4(w + o * L::ld2), dz = ld4(d + o * kRP);
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[a][r] = __fmaf_rn(wo[a], dz[r], acc[a][r]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float s = acc[a][r];
                        s = __fadd_rn(s, __shfl_xor(s, 16));          // S0 + S1 | S2 + S3
                        s = __fadd_rn(s, __shfl_xor(s, 32));          // (S0 + S1) + (S2 + S3)
                        acc[a][r] = s;
                    }
                if (q == 0) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const f32x4 hv = ld4(lds + L::a1 + (4 * ig + a) * kRP + 4 * rg);
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[a][r] = hv[r] > 0.0f ? acc[a][r] : 0.0f;
                        st4(lds + L::d1 + (4 * ig + a) * kRP + 4 * rg, acc[a]);
                    }
                }
            }
            __syncthreads();
            // -- phase C: the gradient of layer 0 from (dz0, obs)
            if (own1) {
#pragma clang loop unroll(disable)
                for (int rg = 0; rg < kRG; ++rg) {
                    const f32x4 dz = ld4(lds + L::d1 + o1 * kRP + 4 * rg);
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const f32x4 xv = ld4(lds + L::x + (4 * ig1 + a) * kRP + 4 * rg);
#pragma unroll
                        for (int r = 0; r < 4; ++r) g1[a] = __fmaf_rn(dz[r], xv[r], g1[a]);
                    }
                }
            }
            if (bk == 0) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) gb = __fadd_rn(gb, lds[L::d1 + bu * kRP + r]);
            }
        }

        // ---- the first chunk of the next step is on its way while Adam runs
        if (more) pre = load_value(F.obs, F.act, nidx);

        // ---- Adam on the thread's own elements: m and v in registers, the weight in LDS (no other thread reads a weight
        // between the barrier after phase B and the one that ends the step, except w0 and the biases, which only the forward
        // pass reads)
        const Adam A{F.b1f, F.b2f, F.omb1, F.omb2, F.eps, lds[L::scal]};
        float sink;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                adam_step(A, g2[a][j], lds + L::w2 + (ti + 32 * j) * L::ld2 + 8 * to + a, &sink, &m2[a][j], &v2[a][j], nullptr, 0);
        if (own1) {
#pragma unroll
            for (int a = 0; a < 4; ++a) adam_step(A, g1[a], lds + L::w1 + o1 * L::ld1 + 4 * ig1 + a, &sink, &m1[a], &v1[a], nullptr, 0);
        }
        adam_step(A, g3, lds + L::w3 + o3 * L::ld3 + i3, &sink, &m3, &v3, nullptr, 0);
        if (bk >= 0) adam_step(A, gb, lds + blds + bu, &sink, &mb, &vb, nullptr, 0);
        if (t == 448) F.loss[it] = __fdiv_rn(lsum, lds[L::scal + 2]);
        __syncthreads();
        rows = nrows;
    }

    // ---- the state back to memory: every thread its own elements
    const bool grads = F.grads[0] != nullptr;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = (8 * to + a) * kH + ti + 32 * j;
            F.w[2][idx] = lds[L::w2 + (ti + 32 * j) * L::ld2 + 8 * to + a];
            F.m[2][idx] = m2[a][j];
            F.v[2][idx] = v2[a][j];
            if (grads) F.grads[2][idx] = g2[a][j];
        }
    if (own1) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int idx = (4 * ig1 + a) * kH + o1;
            F.w[0][idx] = lds[L::w1 + o1 * L::ld1 + 4 * ig1 + a];
            F.m[0][idx] = m1[a];
            F.v[0][idx] = v1[a];
            if (grads) F.grads[0][idx] = g1[a];
        }
    }
    F.w[4][t] = lds[L::w3 + o3 * L::ld3 + i3];
    F.m[4][t] = m3;
    F.v[4][t] = v3;
    if (grads) F.grads[4][t] = g3;
    if (bk >= 0) {
        F.w[bi][bu] = lds[blds + bu];
        F.m[bi][bu] = mb;
        F.v[bi][bu] = vb;
        if (grads) F.grads[bi][bu] = gb;
    }
}

// k_bc_loss: the forward pass and the squared error of block b = list positions [256 b, 256 b + 256), in chunks of 16 rows through
// the same forward_layer chains as the fit; thread 0 adds the rows' s_row to the block's float64 partial in ascending order.  A
// workgroup takes the blocks blockIdx.x, blockIdx.x + gridDim.x, ...: which workgroup computes a block changes nothing.
__global__ __launch_bounds__(kFitBlock) void k_bc_loss(LossArgs F)
{
    using L = Layout;
    __shared__ __align__(16) float lds[L::net_floats];
    const int t = threadIdx.x;
    load_net<L::net_floats>(lds, F.w);
    for (int blk = blockIdx.x; blk < F.blocks; blk += gridDim.x) {
        const int64_t base = (int64_t)blk * kLossRows, end = min((int64_t)F.count, base + kLossRows);   // count may be 2^31 - 1
        double part = 0.0;
        for (int64_t r0 = base; r0 < end; r0 += kRows) {
            const int64_t j = r0 + (t & (kRows - 1));
            const int idx = (t < (kIn + kOut) * kRows && j < end) ? (F.rows ? F.rows[j] : (int)j) : -1;
            stage_value(lds, load_value(F.obs, F.act, idx));
            __syncthreads();
            forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
            __syncthreads();
            forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
            __syncthreads();
            forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
            __syncthreads();
            if (t == 0) {
                for (int r = 0; r < kRows && r0 + r < end; ++r) {
                    float s = 0.0f;
#pragma unroll
                    for (int o = 0; o < kOut; ++o) {
                        const float d = __fsub_rn(lds[L::y + o * kRP + r], lds[L::th + o * kRP + r]);
                        s = __fmaf_rn(d, d, s);
                    }
                    part += (double)s;
                }
            }
            __syncthreads();
        }
        if (t == 0) F.partials[blk] = part;
    }
}

// k_bc_loss_sum: one workgroup; the partials pass through LDS 256 at a time and thread 0 adds them in ascending order
__global__ __launch_bounds__(kSumBlock) void k_bc_loss_sum(const double *partials, int blocks, int count, double *out)
{
    __shared__ double p[kSumBlock];
    const int t = threadIdx.x;
    double sum = 0.0;
    for (int base = 0; base < blocks; base += kSumBlock) {
        if (base + t < blocks) p[t] = partials[base + t];
        __syncthreads();
        if (t == 0)
            for (int i = 0; i < kSumBlock && base + i < blocks; ++i) sum += p[i];
        __syncthreads();
    }
    if (t == 0) out[0] = sum / (4.0 * (double)count);
}

}  // namespace qsb
