// dynfit_kernels.hpp -- the one kernel of qsdf_fit (include/quadsim_dyn_fit.h has the numerical contract).  A fragment of
// dynfit.hip, nowhere else.  The chunk primitives it is built from (forward_layer, backward_layer, adam_step, the chunk geometry
// and the LDS orientation they assume) are train_pieces.hpp's.
//
// k_dyn_fit<P1, P2>: ONE workgroup of 512 threads runs every Adam step of the call.  The weights of the net live in LDS for the
// whole call, the batch is processed in chunks of kRows = 16 rows.  Every thread owns a fixed set of gradient elements and keeps
// them in registers across the chunks of a step (W2: 8 x ceil(P1 / 32), W1: 8, W3: 3, one of each bias), adding rows in ascending
// order; after the last chunk it applies Adam to exactly those elements, streaming m and v through L2 and writing the weight to
// LDS and to memory.  dz2 overwrites h2 and dz1 overwrites h1 in place once the gradient that needed the activation has been
// taken.  All ordering is __syncthreads; there is no second workgroup to wait for.
#pragma once
#include "train_pieces.hpp"

namespace qsf {

constexpr uint64_t kStreamFit = 6;               // the Philox stream of the batch draws (quadsim_device.hpp uses 0 .. 5)

struct FitArgs {
    float *w[6], *m[6], *v[6];                   // w1 b1 w2 b2 w3 b3 and their moments
    float *grads[6];                             // nullable as a whole (grads[0] == nullptr)
    const float *in_mean, *in_rscale, *out_mean, *out_rscale;
    const float *buf_x, *buf_d;
    const int32_t *indices;                      // nullable [iters,batch]
    float *loss;                                 // [iters]
    int32_t *indices_out;                        // nullable [iters,batch]
    uint64_t seed, k;
    double lr, beta1, beta2;
    float b1f, b2f, omb1, omb2, eps, dscale, count;   // dscale = float32(2 / (12 batch)), count = 12 batch
    int h1, h2, size, iters, batch, t0;
};

template <int P1, int P2>
struct FitLayout {
    static constexpr int ld1 = 20, ld2 = P1 + 4, ld3 = P2 + 4;
    static constexpr int w1 = 0, b1 = w1 + P1 * ld1, w2 = b1 + P1, b2 = w2 + P2 * ld2, w3 = b2 + P2, b3 = w3 + 12 * ld3;
    static constexpr int x = b3 + 16, a1 = x + 16 * kRP, a2 = a1 + P1 * kRP, y = a2 + P2 * kRP, th = y + 12 * kRP;
    static constexpr int norm = th + 12 * kRP;   // in_mean [16] | in_rscale [16] | out_mean [12] | out_rscale [12]
    static constexpr int scal = norm + 56;       // lr_t
    static constexpr int floats = scal + 4;
};

template <int P1, int P2>
__global__ __launch_bounds__(kFitBlock) void k_dyn_fit(FitArgs F)
{
    using L = FitLayout<P1, P2>;
    constexpr int J2 = (P1 + 31) / 32;                   // W2 gradient columns of a thread
    static_assert(P1 % 16 == 0 && P2 % 16 == 0 && P1 <= 256 && P2 <= 128, "the thread maps below");
    static_assert(L::floats * 4 <= 160 * 1024, "LDS");
    __shared__ __align__(16) float lds[L::floats];
    const int t = threadIdx.x;
    const int h1 = F.h1, h2 = F.h2, h1r = (h1 + 3) & ~3, h2r = (h2 + 3) & ~3;

    // ---- the net into LDS: zero everything (the padding stays zero for the whole call), then the weights
    for (int i = t; i < L::floats; i += kFitBlock) lds[i] = 0.0f;
    __syncthreads();
    for (int i = t; i < h1 * 16; i += kFitBlock) lds[L::w1 + (i >> 4) * L::ld1 + (i & 15)] = F.w[0][i];
    for (int i = t; i < h1; i += kFitBlock) lds[L::b1 + i] = F.w[1][i];
    for (int i = t; i < h2 * h1; i += kFitBlock) lds[L::w2 + (i / h1) * L::ld2 + i % h1] = F.w[2][i];
    for (int i = t; i < h2; i += kFitBlock) lds[L::b2 + i] = F.w[3][i];
    for (int i = t; i < 12 * h2; i += kFitBlock) lds[L::w3 + (i / h2) * L::ld3 + i % h2] = F.w[4][i];
    if (t < 12) lds[L::b3 + t] = F.w[5][t];
    if (t < 16) { lds[L::norm + t] = F.in_mean[t]; lds[L::norm + 16 + t] = F.in_rscale[t]; }
    if (t < 12) { lds[L::norm + 32 + t] = F.out_mean[t]; lds[L::norm + 44 + t] = F.out_rscale[t]; }
    __syncthreads();

    // ---- the gradient elements of this thread
    const int to = t >> 5, ti = t & 31;                  // W2: units 8 to + a, inputs ti + 32 j
    const int o1 = t & 255, ig1 = t >> 8;                // W1: unit o1, inputs 8 ig1 + a
    const int i3 = t & 127, og3 = t >> 7;                // W3: input i3, outputs og3, og3 + 4 and og3 + 8
    const bool own2 = 8 * to < h2r, own1 = o1 < h1, own3 = i3 < h2;
    const bool grads = F.grads[0] != nullptr;

    for (int it = 0; it < F.iters; ++it) {
        const int step = F.t0 + it;
        if (t == 0) {
            const double tt = (double)step + 1.0;
            lds[L::scal] = (float)(F.lr * sqrt(1.0 - pow(F.beta2, tt)) / (1.0 - pow(F.beta1, tt)));
        }
        float g2[8][J2] = {}, g1[8] = {}, g3[3] = {}, gb1 = 0.0f, gb2 = 0.0f, gb3 = 0.0f;
        float lsum = 0.0f;                                // thread 0: the squared error of the rows so far

        for (int r0 = 0; r0 < F.batch; r0 += kRows) {
            // -- gather and normalise the chunk's rows; rows past the batch are zeros
            if (t < 28 * kRows) {
                const int r = t & (kRows - 1), c = t >> 4, j = r0 + r;      // c < 16: input c; c >= 16: target c - 16
                float val = 0.0f;
                if (j < F.batch) {
                    int idx;
                    if (F.indices) idx = F.indices[(int64_t)it * F.batch + j];
                    else idx = (int)__umulhi(qs::philox_counter(F.seed, (kStreamFit << 48) | F.k, ((uint64_t)step << 32) | (uint64_t)j).x,
                                             (unsigned)F.size);
                    if (c == 0 && F.indices_out) F.indices_out[(int64_t)it * F.batch + j] = idx;
                    if (c < 16) val = __fmul_rn(__fsub_rn(F.buf_x[(int64_t)idx * 16 + c], lds[L::norm + c]), lds[L::norm + 16 + c]);
                    else val = __fmul_rn(__fsub_rn(F.buf_d[(int64_t)idx * 12 + (c - 16)], lds[L::norm + 32 + (c - 16)]), lds[L::norm + 44 + (c - 16)]);
                }
                lds[(c < 16 ? L::x + c * kRP : L::th + (c - 16) * kRP) + r] = val;
            }
            __syncthreads();
            forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, 16, h1, lds + L::a1);
            __syncthreads();
            forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, h1r, h2, lds + L::a2);
            __syncthreads();
            forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, h2r, 12, lds + L::y);
            __syncthreads();
            // -- y -> dy = (y - th) dscale in place, th -> the difference y - th (the loss); rows past the batch give zero
            if (t < 12 * kRows) {
                const int r = t & (kRows - 1), o = t >> 4;
                const bool valid = r0 + r < F.batch;
                const float d = valid ? __fsub_rn(lds[L::y + o * kRP + r], lds[L::th + o * kRP + r]) : 0.0f;
                lds[L::th + o * kRP + r] = d;
                lds[L::y + o * kRP + r] = __fmul_rn(d, F.dscale);
            }
            __syncthreads();
            if (t == 0) {
                for (int r = 0; r < kRows && r0 + r < F.batch; ++r) {
                    float s = 0.0f;
#pragma unroll
                    for (int o = 0; o < 12; ++o) { const float d = lds[L::th + o * kRP + r]; s = __fmaf_rn(d, d, s); }
                    lsum = __fadd_rn(lsum, s);
                }
            }
            // -- layer 3: gradient from (dy, h2), then dz2 over h2
            if (own3) {
#pragma clang loop unroll(disable)
                for (int rg = 0; rg < kRG; ++rg) {
                    const f32x4 a = ld4(lds + L::a2 + i3 * kRP + 4 * rg);
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const f32x4 d = ld4(lds + L::y + (og3 + 4 * q) * kRP + 4 * rg);
#pragma unroll
                        for (int r = 0; r < 4; ++r) g3[q] = __fmaf_rn(d[r], a[r], g3[q]);
                    }
                }
            }
            if (t < 12) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) gb3 = __fadd_rn(gb3, lds[L::y + t * kRP + r]);
            }
            __syncthreads();
            backward_layer(lds + L::w3, L::ld3, lds + L::y, 12, h2r, lds + L::a2);
            __syncthreads();
            // -- layer 2: gradient from (dz2, h1), then dz1 over h1
            if (own2) {
#pragma clang loop unroll(disable)
                for (int rg = 0; rg < kRG; ++rg) {
                    f32x4 dz[8];
#pragma unroll
                    for (int a = 0; a < 8; ++a) dz[a] = ld4(lds + L::a2 + (8 * to + a) * kRP + 4 * rg);
#pragma unroll
                    for (int j = 0; j < J2; ++j) {
                        const int i = ti + 32 * j;
                        if (i < h1r) {
                            const f32x4 a1 = ld4(lds + L::a1 + i * kRP + 4 * rg);
#pragma unroll
                            for (int a = 0; a < 8; ++a)
#pragma unroll
                                for (int r = 0; r < 4; ++r) g2[a][j] = __fmaf_rn(dz[a][r], a1[r], g2[a][j]);
                        }
                    }
                }
            }
            if (t < h2) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) gb2 = __fadd_rn(gb2, lds[L::a2 + t * kRP + r]);
            }
            __syncthreads();
            backward_layer(lds + L::w2, L::ld2, lds + L::a2, h2, h1r, lds + L::a1);
            __syncthreads();
            // -- layer 1: gradient from (dz1, x)
            if (own1) {
#pragma clang loop unroll(disable)
                for (int rg = 0; rg < kRG; ++rg) {
                    const f32x4 dz = ld4(lds + L::a1 + o1 * kRP + 4 * rg);
#pragma unroll
                    for (int a = 0; a < 8; ++a) {
                        const f32x4 xv = ld4(lds + L::x + (8 * ig1 + a) * kRP + 4 * rg);
#pragma unroll
                        for (int r = 0; r < 4; ++r) g1[a] = __fmaf_rn(dz[r], xv[r], g1[a]);
                    }
                }
            }
            if (t < h1) {
#pragma unroll
                for (int r = 0; r < kRows; ++r) gb1 = __fadd_rn(gb1, lds[L::a1 + t * kRP + r]);
            }
            __syncthreads();
        }

        // ---- Adam on the thread's own elements; m and v stream through L2, the weight goes to LDS and to memory
        // (the thread's element indices are re-derived from an opaque copy of its id: hoisted out of the iteration loop, the
        // 64-bit addresses of every owned element of w, m, v and grads would be held in registers across the whole step)
        int tq = t;
        asm volatile("" : "+v"(tq));
        const int to = tq >> 5, ti = tq & 31, o1 = tq & 255, ig1 = tq >> 8, i3 = tq & 127, og3 = tq >> 7;
        // (likewise the 24 tensor pointers: read from the kernel-argument segment here, where they are used, through an opaque
        // copy of its address; held in scalar registers across the step they leave too few for the loops above)
        typedef const __attribute__((address_space(4))) FitArgs *KernArgs;
        KernArgs kp = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const __attribute__((address_space(4))) FitArgs &K = *kp;
        const Adam A{F.b1f, F.b2f, F.omb1, F.omb2, F.eps, lds[L::scal]};
        const bool out = grads && it == F.iters - 1;
        if (own2) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int j = 0; j < J2; ++j) {
                    const int o = 8 * to + a, i = ti + 32 * j;
                    if (o < h2 && i < h1)
                        adam_step(A, g2[a][j], lds + L::w2 + o * L::ld2 + i, K.w[2], K.m[2], K.v[2], out ? K.grads[2] : nullptr, o * h1 + i);
                }
        }
        if (own1) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
                adam_step(A, g1[a], lds + L::w1 + o1 * L::ld1 + 8 * ig1 + a, K.w[0], K.m[0], K.v[0], out ? K.grads[0] : nullptr, o1 * 16 + 8 * ig1 + a);
        }
        if (own3) {
#pragma unroll
            for (int q = 0; q < 3; ++q)
                adam_step(A, g3[q], lds + L::w3 + (og3 + 4 * q) * L::ld3 + i3, K.w[4], K.m[4], K.v[4], out ? K.grads[4] : nullptr,
                          (og3 + 4 * q) * h2 + i3);
        }
        if (tq < h1) adam_step(A, gb1, lds + L::b1 + tq, K.w[1], K.m[1], K.v[1], out ? K.grads[1] : nullptr, tq);
        if (tq < h2) adam_step(A, gb2, lds + L::b2 + tq, K.w[3], K.m[3], K.v[3], out ? K.grads[3] : nullptr, tq);
        if (tq < 12) adam_step(A, gb3, lds + L::b3 + tq, K.w[5], K.m[5], K.v[5], out ? K.grads[5] : nullptr, tq);
        if (t == 0) F.loss[it] = __fdiv_rn(lsum, F.count);
        __syncthreads();
    }
}

}  // namespace qsf
