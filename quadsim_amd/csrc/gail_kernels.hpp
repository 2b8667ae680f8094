// gail_kernels.hpp -- the kernels of libquadsim_gail.so (include/quadsim_gail.h has the numerical contract).  A fragment of
// gail.hip, nowhere else.  Shared at the source level: adam_step, ld4 / st4 and the chunk geometry (kFitBlock, kRows, kRP) of
// train_pieces.hpp, q_tanh of quadsim_device.hpp.
//
// k_gail_fit<W>: ONE workgroup of 512 threads runs every Adam step of the call on the discriminator 16 -> H -> H -> 1, H <= W.
// It has the shape of k_dyn_fit: the weights in LDS for the whole call in (out, in) orientation, rows LD = in + 4 floats apart,
// a class's rows in chunks of 16 staged unit-major, every thread a fixed set of gradient elements that it keeps in registers over
// the chunks of a step and then gives to Adam, m and v streaming through L2.  What differs: tanh keeps its activation AND its
// derivative (a and d = 1 - a^2 have a buffer each), so dz overwrites d, not a, and the gradient of a layer shares a phase with
// the back-propagation through it: a chunk has 7 workgroup barriers.  A step is two chunk sequences, the generator's rows and
// then the expert's; thread 448 adds the rows' loss terms in that order.
//
// k_gail_reward<W>: ROWS are the MFMA column dimension, as candidates are in k_dyn_plan.  A wave owns a tile of 16 rows; the
// tiles are dealt to the waves of a persistent grid.  A workgroup (4 waves) builds the padded weight image in LDS once, straight
// from the net's tensors, and meets no barrier afterwards.  Lane (c = l & 15, g = l >> 4) holds inputs 4 g .. 4 g + 3 of row c,
// the B operand of layer-1 k-step i being register i; an accumulator tile holds units 16 t + 4 g + i in register i, which is the
// B operand of the next layer as it stands against weights in their natural (out, in) order: no permutation anywhere.
#pragma once
#include "train_pieces.hpp"

namespace qsg {

using qsf::adam_step;
using qsf::Adam;
using qsf::f32x4;
using qsf::kFitBlock;
using qsf::kRG;
using qsf::kRows;
using qsf::kRP;
using qsf::ld4;
using qsf::st4;

constexpr int kObs = 12, kAct = 4, kIn = 16;
constexpr int kStats = 5;
constexpr int kRewardBlock = 256;                // 4 waves: one per SIMD, each with the whole register file (k_dyn_plan's choice)
constexpr int kMathBlock = 256;

// ---------------------------------------------------------------------------------------------------- the device functions
__device__ __forceinline__ float g_exp(float x) { return expf(x); }
__device__ __forceinline__ float g_log(float x) { return logf(x); }
__device__ __forceinline__ float g_log1p(float x) { return log1pf(x); }
// (selects, not fminf(fmaxf()): those would turn a NaN action into -1; an infinity is clamped as any other value)
__device__ __forceinline__ float g_clamp1(float a) { return a < -1.0f ? -1.0f : a > 1.0f ? 1.0f : a; }
// q_tanh bounds its exponent with fminf, which drops a NaN operand: tanh(NaN) would be +-1 with a finite derivative.  Here a NaN
// stays in both; every other value is q_tanh's, bit for bit
__device__ __forceinline__ float g_tanh(float x, float &sech2)
{
    const float a = qs::q_tanh(x, sech2);
    sech2 = x != x ? x : sech2;
    return x != x ? x : a;
}

// input column c of a row: the normalised observation or the clamped action
__device__ __forceinline__ float input_value(const float *obs, const float *act, const float *mean, const float *rscale, int64_t row, int c)
{
    return c < kObs ? __fmul_rn(__fsub_rn(obs[row * kObs + c], mean[c]), rscale[c]) : g_clamp1(act[row * kAct + (c - kObs)]);
}

// reward = -log(1 / (1 + exp(l)) + 1e-8)
__device__ __forceinline__ float reward_of(float l)
{
    const float q = __fdiv_rn(1.0f, __fadd_rn(1.0f, g_exp(l)));
    return -g_log(__fadd_rn(q, 1.0e-8f));
}

// ---------------------------------------------------------------------------------------------------- the fit
struct FitArgs {
    float *w[6], *m[6], *v[6];                   // w0 b0 w1 b1 w2 b2 and their moments
    float *grads[6];                             // nullable as a whole (grads[0] == nullptr)
    const float *mean, *rscale;                  // [12]
    const float *obs[2], *act[2];                // class 0: the generator's rows, class 1: the expert's
    const int32_t *idx[2];                       // [steps,batch] each
    const int32_t *counts;                       // nullable [steps]
    float *stats;                                // [steps,5]
    double lr, beta1, beta2, entcoeff;
    float b1f, b2f, omb1, omb2, eps;
    int hidden, steps, batch, t0;
};

template <int W>
struct FitLayout {
    static constexpr int ld1 = kIn + 4, ld2 = W + 4;
    static constexpr int w1 = 0, b1 = w1 + W * ld1, w2 = b1 + W, b2 = w2 + W * ld2, w3 = b2 + W, b3 = w3 + ld2;
    static constexpr int x = b3 + 4, a1 = x + kIn * kRP, d1 = a1 + W * kRP, a2 = d1 + W * kRP, d2 = a2 + W * kRP;
    static constexpr int lg = d2 + W * kRP, dl = lg + kRP, sp = dl + kRP, en = sp + kRP;      // per row: logit, dl, softplus, entropy
    static constexpr int norm = en + kRP;        // mean [16] | rscale [16]
    static constexpr int scal = norm + 32;       // lr_t, 1 / c, entcoeff / (2 c), c
    static constexpr int floats = scal + 4;
};

// Z[u][r] = B[u] + sum_k Wt[u][k] A[k][r], k ascending, then (A', D')[u][r] = tanh: one item = one unit x four rows
__device__ __forceinline__ void tanh_layer(const float *Wt, int ld, const float *B, const float *A, int K4, int U, float *Za, float *Zd)
{
    for (int item = threadIdx.x; item < U * kRG; item += kFitBlock) {
        const int u = item >> 2, rg = item & 3;
        const float b = B[u];
        f32x4 acc = {b, b, b, b};
        const float *w = Wt + u * ld, *a = A + 4 * rg;
        for (int k = 0; k < K4; k += 4) {
            const f32x4 wk = ld4(w + k);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 ak = ld4(a + (k + i) * kRP);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(wk[i], ak[r], acc[r]);
            }
        }
        f32x4 d;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s2;
            acc[r] = g_tanh(acc[r], s2);
            d[r] = s2;
        }
        st4(Za + u * kRP + 4 * rg, acc);
        st4(Zd + u * kRP + 4 * rg, d);
    }
}

template <int W>
__global__ __launch_bounds__(kFitBlock) void k_gail_fit(FitArgs F)
{
    using L = FitLayout<W>;
    constexpr int J2 = W / 32;                           // w1 gradient columns of a thread
    constexpr int N1 = W / 32;                           // w0 gradient inputs of a thread: 512 / W groups of N1 cover the 16
    static_assert(W == 64 || W == 128, "the thread maps below");
    static_assert(L::floats * 4 <= 160 * 1024, "LDS");
    static_assert(kFitBlock == 512 && kRows == 16, "the thread maps below");
    __shared__ __align__(16) float lds[L::floats];
    const int t = threadIdx.x;
    const int H = F.hidden, h4 = (H + 3) & ~3;

    // ---- the net into LDS: zero everything (the padding stays zero for the whole call), then the weights, transposed
    for (int i = t; i < L::floats; i += kFitBlock) lds[i] = 0.0f;
    __syncthreads();
    for (int i = t; i < kIn * H; i += kFitBlock) lds[L::w1 + (i % H) * L::ld1 + i / H] = F.w[0][i];
    for (int i = t; i < H * H; i += kFitBlock) lds[L::w2 + (i % H) * L::ld2 + i / H] = F.w[2][i];
    for (int i = t; i < H; i += kFitBlock) {
        lds[L::b1 + i] = F.w[1][i];
        lds[L::b2 + i] = F.w[3][i];
        lds[L::w3 + i] = F.w[4][i];
    }
    if (t == 0) lds[L::b3] = F.w[5][0];
    if (t < kObs) { lds[L::norm + t] = F.mean[t]; lds[L::norm + 16 + t] = F.rscale[t]; }
    __syncthreads();

    // ---- the gradient elements of this thread
    const int to = t >> 5, ti = t & 31;                  // w1: units 8 to + a, inputs ti + 32 j
    const int o1 = t & (W - 1), ig1 = t / W;             // w0: unit o1, inputs N1 ig1 + a
    const bool own2 = 8 * to < h4, own1 = o1 < H, ownu = t < H;      // ownu: w2[t], b0[t], b1[t]
    const bool grads = F.grads[0] != nullptr;

    for (int it = 0; it < F.steps; ++it) {
        int cnt = F.counts ? F.counts[it] : F.batch;
        cnt = cnt < F.batch ? cnt : F.batch;
        if (t == 0) {
            const double tt = (double)(F.t0 + it) + 1.0;
            lds[L::scal] = (float)(F.lr * sqrt(1.0 - pow(F.beta2, tt)) / (1.0 - pow(F.beta1, tt)));
            lds[L::scal + 1] = (float)(1.0 / (double)cnt);
            lds[L::scal + 2] = (float)(F.entcoeff / (2.0 * (double)cnt));
        }
        float g2[8][J2] = {}, g1[N1] = {}, g3 = 0.0f, gb1 = 0.0f, gb2 = 0.0f, gb3 = 0.0f;
        float loss[2] = {0.0f, 0.0f}, acc[2] = {0.0f, 0.0f}, ent = 0.0f;      // thread 448

        for (int cls = 0; cls < 2; ++cls) {
            const float *obs = F.obs[cls], *act = F.act[cls];
            const int32_t *idx = F.idx[cls] + (int64_t)it * F.batch;
            for (int r0 = 0; r0 < cnt; r0 += kRows) {
                // -- gather the chunk's rows; rows past the count are zeros
                if (t < kIn * kRows) {
                    const int r = t & (kRows - 1), c = t >> 4, j = r0 + r;
                    float val = 0.0f;
                    if (j < cnt) val = input_value(obs, act, lds + L::norm, lds + L::norm + 16, (int64_t)idx[j], c);
                    lds[L::x + c * kRP + r] = val;
                }
                __syncthreads();
                tanh_layer(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kIn, H, lds + L::a1, lds + L::d1);
                __syncthreads();
                tanh_layer(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, h4, H, lds + L::a2, lds + L::d2);
                __syncthreads();
                // -- the logit of four rows an item, and in the same item the row's loss terms and dl; rows past the count give zero
                if (t < kRG) {
                    const float b = lds[L::b3], inv = lds[L::scal + 1], kent = lds[L::scal + 2];
                    f32x4 l = {b, b, b, b};
                    const float *w = lds + L::w3, *a = lds + L::a2 + 4 * t;
                    for (int k = 0; k < h4; k += 4) {
                        const f32x4 wk = ld4(w + k);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const f32x4 ak = ld4(a + (k + i) * kRP);
#pragma unroll
                            for (int r = 0; r < 4; ++r) l[r] = __fmaf_rn(wk[i], ak[r], l[r]);
                        }
                    }
                    f32x4 dl, sp, en;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float lr = l[r];
                        const float e = g_exp(-fabsf(lr)), p = g_log1p(e), D = __fadd_rn(1.0f, e);
                        const float sa = __fdiv_rn(1.0f, D), sb = __fdiv_rn(e, D);
                        const float s = lr >= 0.0f ? sa : sb, n = lr >= 0.0f ? sb : sa;
                        const float spn = __fadd_rn(fmaxf(-lr, 0.0f), p);                      // softplus(-l)
                        const float base = cls == 0 ? __fmul_rn(s, inv) : -__fmul_rn(n, inv);
                        const bool valid = r0 + 4 * t + r < cnt;
                        dl[r] = valid ? __fmaf_rn(kent, __fmul_rn(__fmul_rn(s, n), lr), base) : 0.0f;
                        sp[r] = cls == 0 ? __fadd_rn(fmaxf(lr, 0.0f), p) : spn;
                        en[r] = __fmaf_rn(n, lr, spn);
                    }
                    st4(lds + L::lg + 4 * t, l);
                    st4(lds + L::dl + 4 * t, dl);
                    st4(lds + L::sp + 4 * t, sp);
                    st4(lds + L::en + 4 * t, en);
                }
                __syncthreads();
                // -- phase A: the statistics, the gradient of the head from (dl, a1), dz1 = d1 (w2 dl) over d1
                if (t == 448) {
                    for (int r = 0; r < kRows && r0 + r < cnt; ++r) {
                        const float lr = lds[L::lg + r];
                        loss[cls] = __fadd_rn(loss[cls], lds[L::sp + r]);
                        ent = __fadd_rn(ent, lds[L::en + r]);
                        if (cls == 0 ? lr < 0.0f : lr > 0.0f) acc[cls] = __fadd_rn(acc[cls], 1.0f);
                    }
#pragma unroll
                    for (int r = 0; r < kRows; ++r) gb3 = __fadd_rn(gb3, lds[L::dl + r]);
                }
                if (ownu) {
#pragma clang loop unroll(disable)
                    for (int rg = 0; rg < kRG; ++rg) {
                        const f32x4 a = ld4(lds + L::a2 + t * kRP + 4 * rg), d = ld4(lds + L::dl + 4 * rg);
#pragma unroll
                        for (int r = 0; r < 4; ++r) g3 = __fmaf_rn(d[r], a[r], g3);
                    }
                }
                for (int item = t; item < h4 * kRG; item += kFitBlock) {
                    const int u = item >> 2, rg = item & 3;
                    const float w3 = lds[L::w3 + u];
                    const f32x4 d = ld4(lds + L::dl + 4 * rg);
                    f32x4 dz = ld4(lds + L::d2 + u * kRP + 4 * rg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dz[r] = __fmul_rn(dz[r], __fmul_rn(w3, d[r]));
                    st4(lds + L::d2 + u * kRP + 4 * rg, dz);
                }
                __syncthreads();
                // -- phase B: the gradient of layer 1 from (dz1, a0), dz0 = d0 (w1 dz1) over d0
                if (own2) {
#pragma clang loop unroll(disable)
                    for (int rg = 0; rg < kRG; ++rg) {
                        f32x4 dz[8];
#pragma unroll
                        for (int a = 0; a < 8; ++a) dz[a] = ld4(lds + L::d2 + (8 * to + a) * kRP + 4 * rg);
#pragma unroll
                        for (int j = 0; j < J2; ++j) {
                            const int i = ti + 32 * j;
                            if (i < h4) {
                                const f32x4 av = ld4(lds + L::a1 + i * kRP + 4 * rg);
#pragma unroll
                                for (int a = 0; a < 8; ++a)
#pragma unroll
                                    for (int r = 0; r < 4; ++r) g2[a][j] = __fmaf_rn(dz[a][r], av[r], g2[a][j]);
                            }
                        }
                    }
                }
                if (ownu) {
#pragma unroll
                    for (int r = 0; r < kRows; ++r) gb2 = __fadd_rn(gb2, lds[L::d2 + t * kRP + r]);
                }
                for (int item = t; item < (h4 >> 2) * kRG; item += kFitBlock) {
                    const int ig = item >> 2, rg = item & 3;
                    f32x4 s[4] = {};
                    const float *w = lds + L::w2 + 4 * ig, *d = lds + L::d2 + 4 * rg;
                    for (int o = 0; o < H; ++o) {
                        const f32x4 wo = ld4(w + o * L::ld2), dz = ld4(d + o * kRP);
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int r = 0; r < 4; ++r) s[a][r] = __fmaf_rn(wo[a], dz[r], s[a][r]);
                    }
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        float *h = lds + L::d1 + (4 * ig + a) * kRP + 4 * rg;
                        const f32x4 dv = ld4(h);
#pragma unroll
                        for (int r = 0; r < 4; ++r) s[a][r] = __fmul_rn(dv[r], s[a][r]);
                        st4(h, s[a]);
                    }
                }
                __syncthreads();
                // -- phase C: the gradient of layer 0 from (dz0, x)
                if (own1) {
#pragma clang loop unroll(disable)
                    for (int rg = 0; rg < kRG; ++rg) {
                        const f32x4 dz = ld4(lds + L::d1 + o1 * kRP + 4 * rg);
#pragma unroll
                        for (int a = 0; a < N1; ++a) {
                            const f32x4 xv = ld4(lds + L::x + (N1 * ig1 + a) * kRP + 4 * rg);
#pragma unroll
                            for (int r = 0; r < 4; ++r) g1[a] = __fmaf_rn(dz[r], xv[r], g1[a]);
                        }
                    }
                }
                if (ownu) {
#pragma unroll
                    for (int r = 0; r < kRows; ++r) gb1 = __fadd_rn(gb1, lds[L::d1 + t * kRP + r]);
                }
                __syncthreads();                         // the next chunk's gather writes x
            }
        }

        // ---- Adam on the thread's own elements; m and v stream through L2, the weight goes to LDS and to memory, both in the
        // policy's (in, out) layout.  (As in k_dyn_fit: the element indices are re-derived from an opaque copy of the thread's id
        // and the 24 tensor pointers read from the kernel-argument segment here, where they are used; hoisted out of the step
        // loop they would be held in registers across the whole step and spill)
        int tq = t;
        asm volatile("" : "+v"(tq));
        const int to = tq >> 5, ti = tq & 31, o1 = tq & (W - 1), ig1 = tq / W;
        typedef const __attribute__((address_space(4))) FitArgs *KernArgs;
        KernArgs kp = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        const __attribute__((address_space(4))) FitArgs &K = *kp;
        const Adam A{F.b1f, F.b2f, F.omb1, F.omb2, F.eps, lds[L::scal]};
        const bool out = grads && it == F.steps - 1;
        if (own2) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int j = 0; j < J2; ++j) {
                    const int o = 8 * to + a, i = ti + 32 * j;
                    if (o < H && i < H)
                        adam_step(A, g2[a][j], lds + L::w2 + o * L::ld2 + i, K.w[2], K.m[2], K.v[2], out ? K.grads[2] : nullptr, i * H + o);
                }
        }
        if (own1) {
#pragma unroll
            for (int a = 0; a < N1; ++a) {
                const int k = N1 * ig1 + a;
                adam_step(A, g1[a], lds + L::w1 + o1 * L::ld1 + k, K.w[0], K.m[0], K.v[0], out ? K.grads[0] : nullptr, k * H + o1);
            }
        }
        if (ownu) {
            adam_step(A, g3, lds + L::w3 + tq, K.w[4], K.m[4], K.v[4], out ? K.grads[4] : nullptr, tq);
            adam_step(A, gb1, lds + L::b1 + tq, K.w[1], K.m[1], K.v[1], out ? K.grads[1] : nullptr, tq);
            adam_step(A, gb2, lds + L::b2 + tq, K.w[3], K.m[3], K.v[3], out ? K.grads[3] : nullptr, tq);
        }
        if (t == 448) {
            adam_step(A, gb3, lds + L::b3, F.w[5], F.m[5], F.v[5], out ? F.grads[5] : nullptr, 0);
            const float R = (float)cnt, R2 = (float)(2 * cnt);
            float *st = F.stats + (int64_t)it * kStats;
            st[0] = __fdiv_rn(loss[0], R);
            st[1] = __fdiv_rn(loss[1], R);
            st[2] = __fdiv_rn(ent, R2);
            st[3] = __fdiv_rn(acc[0], R);
            st[4] = __fdiv_rn(acc[1], R);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------- the reward
struct RewardArgs {
    const float *w[6];
    const float *mean, *rscale;
    const float *obs, *act;
    float *reward, *logits;                      // logits nullable
    int64_t rows, tiles;
    int n_envs, n_steps;                         // 0, 0: row i -> element i
    int hidden;
};

template <int W>
struct RewardLayout {
    static constexpr int ld1 = kIn + 4, ld2 = W + 4;
    static constexpr int w1 = 0, b1 = w1 + W * ld1, w2 = b1 + W, b2 = w2 + W * ld2, w3 = b2 + W, b3 = w3 + ld2, norm = b3 + 4;
    static constexpr int floats = norm + 32;     // mean [16] | rscale [16]
};

__device__ __forceinline__ f32x4 tanh4(f32x4 v)
{
    float s;
    return f32x4{g_tanh(v.x, s), g_tanh(v.y, s), g_tanh(v.z, s), g_tanh(v.w, s)};
}

template <int W>
__global__ __launch_bounds__(kRewardBlock) void k_gail_reward(RewardArgs A)
{
    using L = RewardLayout<W>;
    constexpr int T = W / 16, kGroup = 4;                // row tiles of a layer; of them in flight = independent accumulators
    static_assert(W % 64 == 0 && L::floats * 4 <= 160 * 1024, "tiles and LDS");
    __shared__ __align__(16) float img[L::floats];
    const int H = A.hidden;
    for (int i = threadIdx.x; i < L::floats; i += kRewardBlock) img[i] = 0.0f;
    __syncthreads();
    for (int i = threadIdx.x; i < kIn * H; i += kRewardBlock) img[L::w1 + (i % H) * L::ld1 + i / H] = A.w[0][i];
    for (int i = threadIdx.x; i < H * H; i += kRewardBlock) img[L::w2 + (i % H) * L::ld2 + i / H] = A.w[2][i];
    for (int i = threadIdx.x; i < H; i += kRewardBlock) {
        img[L::b1 + i] = A.w[1][i];
        img[L::b2 + i] = A.w[3][i];
        img[L::w3 + i] = A.w[4][i];
    }
    if (threadIdx.x == 0) img[L::b3] = A.w[5][0];
    if (threadIdx.x < kObs) { img[L::norm + threadIdx.x] = A.mean[threadIdx.x]; img[L::norm + 16 + threadIdx.x] = A.rscale[threadIdx.x]; }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const float *W1 = img + L::w1 + c * L::ld1 + 4 * g;      // + 16 rt ld1
    const float *B1 = img + L::b1 + 4 * g;                   // + 16 rt
    const float *W2 = img + L::w2 + c * L::ld2 + 4 * g;      // + 16 nt ld2 + 16 rt
    const float *B2 = img + L::b2 + 4 * g;                   // + 16 nt
    const float *W3 = img + L::w3 + 4 * g;                   // + 16 nt: the one output row, on matrix row 0
    const float b3 = img[L::b3];
    constexpr int kWaves = kRewardBlock / 64;

    for (int64_t tile = (int64_t)blockIdx.x * kWaves + wave; tile < A.tiles; tile += (int64_t)gridDim.x * kWaves) {
        const int64_t row = tile * 16 + c;
        const bool valid = row < A.rows;
        const int64_t rr = valid ? row : A.rows - 1;         // columns past the end repeat the last row, unstored
        f32x4 x;                                             // x[i] = input 4 g + i
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = input_value(A.obs, A.act, img + L::norm, img + L::norm + 16, rr, 4 * g + i);

        f32x4 h1[T];
#pragma unroll
        for (int r0 = 0; r0 < T; r0 += kGroup) {
            f32x4 acc[kGroup], w[kGroup];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                acc[j] = ld4(B1 + 16 * (r0 + j));
                w[j] = ld4(W1 + 16 * (r0 + j) * L::ld1);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)                      // k-step outermost: consecutive MFMAs on different accumulators
#pragma unroll
                for (int j = 0; j < kGroup; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][i], x[i], acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < kGroup; ++j) h1[r0 + j] = tanh4(acc[j]);
        }
        f32x4 a3 = {g == 0 ? b3 : 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int n0 = 0; n0 < T; n0 += kGroup) {
            f32x4 h2[kGroup];
#pragma unroll
            for (int j = 0; j < kGroup; ++j) h2[j] = ld4(B2 + 16 * (n0 + j));
#pragma unroll
            for (int rt = 0; rt < T; ++rt) {
                f32x4 w[kGroup];
#pragma unroll
                for (int j = 0; j < kGroup; ++j) w[j] = ld4(W2 + 16 * (n0 + j) * L::ld2 + 16 * rt);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < kGroup; ++j) h2[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][i], h1[rt][i], h2[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < kGroup; ++j) {
                const f32x4 a = tanh4(h2[j]);
                const f32x4 wl = ld4(W3 + 16 * (n0 + j));
#pragma unroll
                for (int i = 0; i < 4; ++i) a3 = __builtin_amdgcn_mfma_f32_16x16x4f32(c == 0 ? wl[i] : 0.0f, a[i], a3, 0, 0, 0);
            }
        }
        if (valid && g == 0) {                               // matrix row 0 = register 0 of the lanes g = 0
            int64_t o = row;
            if (A.n_envs > 0) o = (row % A.n_steps) * A.n_envs + row / A.n_steps;
            const float l = a3[0];
            A.reward[o] = reward_of(l);
            if (A.logits) A.logits[o] = l;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the tests' window
__global__ __launch_bounds__(kMathBlock) void k_gail_math(int kind, const float *x, float *y, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * kMathBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMathBlock) {
        const float v = x[i];
        float s2 = 0.0f, r;
        switch (kind) {
        case 0: r = g_tanh(v, s2); break;
        case 1: g_tanh(v, s2); r = s2; break;
        case 2: r = g_exp(v); break;
        case 3: r = g_log(v); break;
        default: r = g_log1p(v); break;
        }
        y[i] = r;
    }
}

}  // namespace qsg
