// bcfit_kernels.hpp -- the kernels of libquadsim_bc.so (include/quadsim_bc.h has the numerical contract).  A fragment of
// bcfit.hip, nowhere else.  Built from train_pieces.hpp: the chunk primitives and the tower pieces (the LDS image and its loader,
// the element map, backward_chunk, the register-resident moments).
//
// k_bc_fit: ONE workgroup of 512 threads runs every Adam step of the call on the actor 12 -> 128 -> 128 -> 4.  What differs from
// k_dyn_fit, all of it to shorten a step of ONE chunk (batch 10 of the reference is one chunk):
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
#include "train_pieces.hpp"

namespace qsb {

using namespace qsf;

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

struct Layout : TowerImage<> {
    static constexpr int th = planes;                            // the expert's actions, then e = y - a_expert
    static constexpr int net_floats = th + kOut * kRP;           // what k_bc_loss needs
    static constexpr int d2 = net_floats, d1 = d2 + kH * kRP;    // dz1 and dz0
    static constexpr int scal = d1 + kH * kRP;                   // lr_t, dscale, 4 rows
    static constexpr int floats = scal + 4;
};

// the net into LDS, and a barrier
template <int FLOATS>
__device__ __forceinline__ void load_net(float *lds, const float *const *w)
{
    load_image<Layout>(lds, FLOATS, kOut, [&](int k, int i) { return w[k][i]; });
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
    __shared__ __align__(16) float lds[L::floats];
    const int t = threadIdx.x;
    load_net<L::floats>(lds, F.w);
    Acc G, M, V;
    load_moments<L, kOut>(M, V, F);

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
        zero_acc(G);
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
            // -- the loss, then the three phases of the backward pass
            if (t == 448) {
                for (int r = 0; r < kRows && r0 + r < rows; ++r) {
                    float s = 0.0f;
#pragma unroll
                    for (int o = 0; o < kOut; ++o) { const float d = lds[L::th + o * kRP + r]; s = __fmaf_rn(d, d, s); }
                    lsum = __fadd_rn(lsum, s);
                }
            }
            backward_chunk<L>(lds, G);
        }

        // ---- the first chunk of the next step is on its way while Adam runs
        if (more) pre = load_value(F.obs, F.act, nidx);

        // ---- Adam on the thread's own elements: m and v in registers, the weight in LDS (no other thread reads a weight
        // between the barrier after phase B and the one that ends the step, except w0 and the biases, which only the forward
        // pass reads)
        const Adam A{F.b1f, F.b2f, F.omb1, F.omb2, F.eps, lds[L::scal]};
        step_moments<L, kOut>(A, lds, G, M, V);
        if (t == 448) F.loss[it] = __fdiv_rn(lsum, lds[L::scal + 2]);
        __syncthreads();
        rows = nrows;
    }

    store_state<L, kOut>(lds, F, G, M, V);
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
