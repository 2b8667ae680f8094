// train_pieces.hpp -- the device pieces every trainer library is built from.  A fragment of dynfit.hip, gail.hip, bcfit.hip,
// ppo2.hip, trpo.hip, ddpg.hip, td3.hip and sac.hip; it defines no kernel.  Two sections:
//
// CHUNK PRIMITIVES (k_dyn_fit, k_gail_fit and the tower trainers alike).  A net lives in LDS in torch's (out, in) orientation, rows
// LD = in + 4 floats apart (a ds_read_b128 per lane fetches four k of one unit; LD = 4 mod 16 words puts 16 units on 16
// different bank quads).  The batch is processed in chunks of kRows = 16 rows: the chunk's activations are staged in LDS
// unit-major, A[unit][row], rows kRP = 20 floats apart, so that one ds_read_b128 fetches four ROWS of one unit -- the B operand
// of a forward tile (1 unit x 4 rows), of a back-propagation tile (4 units x 4 rows) and of a gradient tile alike.  Every
// product is a plain fmaf chain: the forward is the planners' k-ascending chain from the bias and the gradient sums are
// row-ascending chains, which plain FMAs give as written.  MFMA gradient tiles (rows as the k dimension) were not built.
//
// TOWER PIECES: the 12 -> 128 (+ K extra inputs) -> 128 -> OUTS tower at 512 threads that k_bc_fit, k_ppo_grad, the TRPO kernels
// and k_ddpg_step train.  The policy stores its weights (in, out); in LDS they lie (out, in).  One LDS image and its loader, one
// map from a thread to the gradient elements it owns with one visitor over them, the backward pass of a chunk, Adam's moments
// held in registers for a whole call, and the reductions and constants of the Gaussian head.  Who puts what behind the image,
// where the barriers stand and what the head computes stays with each kernel.
#pragma once
#include "quadsim_device.hpp"

namespace qsf {

// ==================================================================================================== chunk primitives
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFitBlock = 512;
constexpr int kRows = 16;                        // batch rows of a chunk
constexpr int kRG = kRows / 4;                   // groups of four rows
constexpr int kRP = 20;                          // floats between two units of a staged activation

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

// Z[u][r] = B[u] + sum_k W[u][k] A[k][r], k ascending, for u < U and the chunk's 16 rows; K4 = K rounded up to 4 (the padding
// is zero on both sides and adds nothing).  One item = one unit x four rows.
template <bool RELU>
__device__ __forceinline__ void forward_layer(const float *W, int ld, const float *B, const float *A, int K4, int U, float *Z)
{
    for (int item = threadIdx.x; item < U * kRG; item += kFitBlock) {
        const int u = item >> 2, rg = item & 3;
        const float b = B[u];
        f32x4 acc = {b, b, b, b};
        const float *w = W + u * ld, *a = A + 4 * rg;
        for (int k = 0; k < K4; k += 4) {
            const f32x4 wk = ld4(w + k);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 ak = ld4(a + (k + i) * kRP);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(wk[i], ak[r], acc[r]);
            }
        }
        if (RELU) {
            // (a select, not fmaxf: fmaxf drops a NaN operand, and a diverged row would go on as a row of dead units.  -0 <= 0
            // holds, so a negative zero becomes +0 as it did)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = acc[r] <= 0.0f ? 0.0f : acc[r];
        }
        st4(Z + u * kRP + 4 * rg, acc);
    }
}

// H[i][r] <- (H[i][r] > 0) ? sum_o W[o][i] D[o][r], o ascending from 0 : 0, for i < I4 (a multiple of 4).  One item = four
// units x four rows; the item reads and writes its own 16 elements of H only.
__device__ __forceinline__ void backward_layer(const float *W, int ld, const float *D, int O, int I4, float *H)
{
    for (int item = threadIdx.x; item < (I4 >> 2) * kRG; item += kFitBlock) {
        const int ig = item >> 2, rg = item & 3;
        f32x4 acc[4] = {};
        const float *w = W + 4 * ig, *d = D + 4 * rg;
        for (int o = 0; o < O; ++o) {
            const f32x4 wo = ld4(w + o * ld), dz = ld4(d + o * kRP);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[a][r] = __fmaf_rn(wo[a], dz[r], acc[a][r]);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float *h = H + (4 * ig + a) * kRP + 4 * rg;
            const f32x4 hv = ld4(h);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[a][r] = hv[r] > 0.0f ? acc[a][r] : 0.0f;
            st4(h, acc[a]);
        }
    }
}

struct Adam {
    float b1, b2, omb1, omb2, eps, lr_t;
};

// one element: the operation order of the header, every operation rounded once
__device__ __forceinline__ void adam_step(const Adam &A, float g, float *lds_w, float *w, float *m, float *v, float *grad, int idx)
{
    const float mn = __fmaf_rn(A.b1, m[idx], __fmul_rn(A.omb1, g));
    const float vn = __fmaf_rn(A.b2, v[idx], __fmul_rn(A.omb2, __fmul_rn(g, g)));
    const float wn = __fsub_rn(*lds_w, __fdiv_rn(__fmul_rn(A.lr_t, mn), __fadd_rn(__fsqrt_rn(vn), A.eps)));
    m[idx] = mn;
    v[idx] = vn;
    w[idx] = wn;
    *lds_w = wn;
    if (grad) grad[idx] = g;
}

// ==================================================================================================== tower pieces
constexpr int kIn = 12, kInP = 16, kH = 128, kOut = 4;   // the head is always run four outputs wide; a narrower one has zero rows
constexpr int kStatT = 448, kLsT = 264;          // the threads that add the statistics and the logstd gradient of a chunk
constexpr double kLog2Pi = 1.8378770664093453, kLog2PiE = 2.8378770664093453;
static_assert(kFitBlock == 512 && kRows == 16 && kH == 128, "the thread maps below");

// The head of every tower kernel's LDS image: the weights (out, in), then the chunk's planes x, a1 (layer 1's input: A1 units,
// 128 or with DDPG's four action rows 132), a2 and y.  A kernel's Layout derives from it and goes on from `planes`.
template <int LD2 = kH + 4, int A1 = kH>
struct TowerImage {
    static constexpr int ld1 = kInP + 4, ld2 = LD2, ld3 = kH + 4;
    static constexpr int w1 = 0, b1 = w1 + kH * ld1, w2 = b1 + kH, b2 = w2 + kH * ld2, w3 = b2 + kH, b3 = w3 + kOut * ld3;
    static constexpr int x = b3 + 16, a1 = x + kInP * kRP, a2 = a1 + A1 * kRP, y = a2 + kH * kRP;
    static constexpr int planes = y + kOut * kRP;
};

// The image into LDS: zero the first `floats` (the padding stays zero for the whole call), a barrier, then the weights,
// transposed.  at(k, i) is element i of slot k (w0 b0 w1 b1 w2 b2, the policy's (in, out) layout), K1 layer 1's input count and
// outs the head's width.  No barrier at the end: the caller's next one covers it.
template <class L, int K1 = kH, class At>
__device__ __forceinline__ void load_image(float *lds, int floats, int outs, At at)
{
    const int t = threadIdx.x;
    for (int i = t; i < floats; i += kFitBlock) lds[i] = 0.0f;
    __syncthreads();
    for (int i = t; i < kIn * kH; i += kFitBlock) lds[L::w1 + (i & (kH - 1)) * L::ld1 + (i >> 7)] = at(0, i);
    for (int i = t; i < K1 * kH; i += kFitBlock) lds[L::w2 + (i & (kH - 1)) * L::ld2 + (i >> 7)] = at(2, i);
    for (int i = t; i < kH * outs; i += kFitBlock) lds[L::w3 + (i % outs) * L::ld3 + i / outs] = at(4, i);
    if (t < kH) { lds[L::b1 + t] = at(1, t); lds[L::b2 + t] = at(3, t); }
    if (t < outs) lds[L::b3 + t] = at(5, t);
}

// The gradient elements of a thread, in the policy's (in, out) layout:
//   g2[a][j]  w1: input 8 to + a, output ti + 32 j                  (ti = t & 31, to = t >> 5)
//   g1[a]     w0: output o1, input 4 ig1 + a; ig1 == 3 is the zero padding, no element   (o1 = t & 127, ig1 = t >> 7)
//   g3        w2: input i3, output o3; none where o3 is past the head's width            (o3 = t & 3, i3 = t >> 2)
//   gb        one bias at most: unit bu = t & 127 of b0 (t < 128), b1 (t < 256) or b2 (t < 256 + OUTS)
// The same struct holds a thread's Adam moments where they live in registers.
struct Acc {
    float g2[8][4], g1[4], g3, gb;
};

// f(LDS offset of the weight, index in its tensor, slot 0 .. 5, the element of every acc ...) for each element thread t owns
template <class L, int OUTS, class Fn, class... A>
__device__ __forceinline__ void for_own(int t, Fn f, A &...acc)
{
    const int ti = t & 31, to = t >> 5, o1 = t & 127, ig1 = t >> 7, o3 = t & 3, i3 = t >> 2;
    const int bk = t < 128 ? 0 : t < 256 ? 1 : t < 256 + OUTS ? 2 : -1, bu = t & 127;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) f(L::w2 + (ti + 32 * j) * L::ld2 + 8 * to + a, (8 * to + a) * kH + ti + 32 * j, 2, acc.g2[a][j]...);
    if (ig1 < 3) {
#pragma unroll
        for (int a = 0; a < 4; ++a) f(L::w1 + o1 * L::ld1 + 4 * ig1 + a, (4 * ig1 + a) * kH + o1, 0, acc.g1[a]...);
    }
    if (o3 < OUTS) f(L::w3 + o3 * L::ld3 + i3, i3 * OUTS + o3, 4, acc.g3...);
    const int bi = bk < 0 ? 0 : 2 * bk + 1, blds = bk == 0 ? L::b1 : bk == 1 ? L::b2 : L::b3;
    if (bk >= 0) f(blds + bu, bu, bi, acc.gb...);
}

__device__ __forceinline__ void zero_acc(Acc &G)
{
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) G.g2[a][j] = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) G.g1[a] = 0.0f;
    G.g3 = 0.0f;
    G.gb = 0.0f;
}

struct NoExtra {
    __device__ __forceinline__ void operator()() const {}
};

// The backward pass of a chunk from dy in the plane y: the gradients of the chunk's rows into G, rows ascending, dz1 into the
// plane d2 and dz0 into d1 under the masks of a2 and a1.  Three phases, two barriers between them, none before or after.
// `extra` runs in phase B between the gradient of layer 1 and the bias sum (DDPG's critic: the four action rows of w1).
// HEAD: the rows of w3 and of the plane y that dz1 is summed over (SAC's actor: eight, the log-std head behind the mean's; the
// gradient of rows 4 .. 7 is the caller's).
template <class L, class Extra = NoExtra, int HEAD = kOut>
__device__ __forceinline__ void backward_chunk(float *lds, Acc &G, Extra extra = Extra())
{
    const int t = threadIdx.x;
    const int ti = t & 31, to = t >> 5, o1 = t & 127, ig1 = t >> 7, o3 = t & 3, i3 = t >> 2;
    const int bk = t < 128 ? 0 : t < 256 ? 1 : t < 260 ? 2 : -1, bu = t & 127;
    // -- phase A: the gradient of the head from (dy, a1), dz1 from (w2, dy) under a1's mask
#pragma clang loop unroll(disable)
    for (int rg = 0; rg < kRG; ++rg) {
        const f32x4 a = ld4(lds + L::a2 + i3 * kRP + 4 * rg), d = ld4(lds + L::y + o3 * kRP + 4 * rg);
#pragma unroll
        for (int r = 0; r < 4; ++r) G.g3 = __fmaf_rn(d[r], a[r], G.g3);
    }
    if (bk == 2) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) G.gb = __fadd_rn(G.gb, lds[L::y + bu * kRP + r]);
    }
    if (t < (kH >> 2) * kRG) {
        const int ig = t >> 2, rg = t & 3;
        f32x4 acc[4] = {};
#pragma unroll
        for (int o = 0; o < HEAD; ++o) {
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
                for (int r = 0; r < 4; ++r) G.g2[a][j] = __fmaf_rn(dz[j][r], av[r], G.g2[a][j]);
        }
    }
    extra();
    if (bk == 1) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) G.gb = __fadd_rn(G.gb, lds[L::d2 + bu * kRP + r]);
    }
    {
        // four inputs x four rows an item, its 128-term sum over four lanes: chain q takes o = q, q + 4, ...
        const int lane = t & 63, wv = t >> 6;
        const int q = lane >> 4, ig = (lane & 15) + 16 * (wv & 1), rg = wv >> 1;
        f32x4 acc[4] = {};
        const float *wp = lds + L::w2 + 4 * ig, *d = lds + L::d2 + 4 * rg;
        for (int o = q; o < kH; o += 4) {
            const f32x4 wo = ld4(wp + o * L::ld2), dz = ld4(d + o * kRP);
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
    if (ig1 < 3) {
#pragma clang loop unroll(disable)
        for (int rg = 0; rg < kRG; ++rg) {
            const f32x4 dz = ld4(lds + L::d1 + o1 * kRP + 4 * rg);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const f32x4 xv = ld4(lds + L::x + (4 * ig1 + a) * kRP + 4 * rg);
#pragma unroll
                for (int r = 0; r < 4; ++r) G.g1[a] = __fmaf_rn(dz[r], xv[r], G.g1[a]);
            }
        }
    }
    if (bk == 0) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) G.gb = __fadd_rn(G.gb, lds[L::d1 + bu * kRP + r]);
    }
}

// ---- Adam's m and v of a thread's elements in registers for a whole call (k_bc_fit; k_trpo_vf_fit has its own text), the weight
// in LDS: a step touches no memory for them.  OUTS is the head's width; the owners of elements that do not exist keep zeros.  F is the kernel's
// argument struct: w, m, v, grads, six tensors each.
template <class L, int OUTS, class Args>
__device__ __forceinline__ void load_moments(Acc &M, Acc &V, const Args &F)
{
    zero_acc(M);
    zero_acc(V);
    for_own<L, OUTS>(threadIdx.x, [&](int, int idx, int slot, float &mo, float &vo) { mo = F.m[slot][idx]; vo = F.v[slot][idx]; }, M, V);
}

template <class L, int OUTS>
__device__ __forceinline__ void step_moments(const Adam &A, float *lds, const Acc &G, Acc &M, Acc &V)
{
    float sink;
    for_own<L, OUTS>(threadIdx.x, [&](int off, int, int, const float &g, float &mo, float &vo) { adam_step(A, g, lds + off, &sink, &mo, &vo, nullptr, 0); },
                     G, M, V);
}

// the state back to memory after the last step, with the last step's gradients where asked for (F.grads[0] != nullptr)
template <class L, int OUTS, class Args>
__device__ __forceinline__ void store_state(const float *lds, const Args &F, const Acc &G, const Acc &M, const Acc &V)
{
    const bool grads = F.grads[0] != nullptr;
    // (the element indices are re-derived from an opaque copy of the thread's id: shared with load_moments' they would be held,
    // as 64-bit addresses, in registers across the whole call)
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    for_own<L, OUTS>(
        t,
        [&](int off, int idx, int slot, const float &g, const float &mo, const float &vo) {
            F.w[slot][idx] = lds[off];
            F.m[slot][idx] = mo;
            F.v[slot][idx] = vo;
            if (grads) F.grads[slot][idx] = g;
        },
        G, M, V);
}

// ---- a net that lies in MEMORY, forward only (k_ddpg_step and k_td3_step read the nets of the other workgroups this way)
// Z[u][r] = B[u] + sum_k W[k][u] A[k][r], k ascending: forward_layer's chain with the weights read from memory in the policy's
// (in, out) layout.  One item = one unit x four rows, unit along the lanes; K is a multiple of 4
template <bool RELU>
__device__ __forceinline__ void stream_layer(const float *W, const float *Bv, const float *A, int K, float *Z)
{
    const int u = threadIdx.x & (kH - 1), rg = threadIdx.x >> 7;
    const float b = Bv[u];
    f32x4 acc = {b, b, b, b};
    const float *w = W + u, *a = A + 4 * rg;
    for (int k = 0; k < K; k += 4) {
        float wk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wk[i] = w[(k + i) * kH];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 ak = ld4(a + (k + i) * kRP);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(wk[i], ak[r], acc[r]);
        }
    }
    if (RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = acc[r] <= 0.0f ? 0.0f : acc[r];       // forward_layer's select: a NaN stays
    }
    st4(Z + u * kRP + 4 * rg, acc);
}

// the head of a streamed net for thread t < 16 OUTS: output t >> 4 of row t & 15, the same chain
template <int OUTS>
__device__ __forceinline__ float stream_head(const float *W, const float *Bv, const float *A)
{
    const int o = threadIdx.x >> 4, r = threadIdx.x & (kRows - 1);
    float acc = Bv[o];
#pragma unroll 8
    for (int k = 0; k < kH; ++k) acc = __fmaf_rn(W[k * OUTS + o], A[k * kRP + r], acc);
    return acc;
}

// q_tanh bounds its exponent with fminf, which drops a NaN operand: tanh(NaN) would be +-1 and a diverged actor would go on as a
// saturated one.  Here a NaN stays; every other value is q_tanh's, bit for bit
__device__ __forceinline__ float tanh_keep_nan(float x)
{
    float unused;
    const float a = qs::q_tanh(x, unused);
    return x != x ? x : a;
}

// ---- a policy tower as one flat vector (theta, a partial gradient, every vector of TRPO's solver): w0 | b0 | w1 | b1 | w2 | b2 |
// logstd, the tensors in the policy's (in, out) layout and the head four wide
constexpr int kW0 = 0, kB0 = kW0 + kIn * kH, kW1 = kB0 + kH, kB1 = kW1 + kH * kH, kW2 = kB1 + kH, kB2 = kW2 + kH * kOut, kLS = kB2 + kOut,
              kP = kLS + kOut;

__device__ __forceinline__ int slot_start(int k)
{
    return k == 0 ? kW0 : k == 1 ? kB0 : k == 2 ? kW1 : k == 3 ? kB1 : k == 4 ? kW2 : k == 5 ? kB2 : k == 6 ? kLS : kP;
}

// the partial gradient of a slice: every thread its own elements (gls: the logstd element of the threads kLsT .. kLsT + 3)
// (written out, not with for_own: with it k_trpo_grad and k_trpo_fvp compile to other code and measured 0.4 % slower)
__device__ __forceinline__ void store_acc(float *part, const Acc &G, float gls)
{
    const int t = threadIdx.x;
    const int ti = t & 31, to = t >> 5, o1 = t & 127, ig1 = t >> 7;
    const int bk = t < 128 ? 0 : t < 256 ? 1 : t < 260 ? 2 : -1, bu = t & 127;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[kW1 + (8 * to + a) * kH + ti + 32 * j] = G.g2[a][j];
    if (ig1 < 3) {
#pragma unroll
        for (int a = 0; a < 4; ++a) part[kW0 + (4 * ig1 + a) * kH + o1] = G.g1[a];
    }
    part[kW2 + t] = G.g3;
    if (bk >= 0) part[(bk == 0 ? kB0 : bk == 1 ? kB1 : kB2) + bu] = G.gb;
    if (t >= kLsT && t < kLsT + kOut) part[kLS + t - kLsT] = gls;
}

// ---- the sum of the BLOCK values of a workgroup in a fixed binary tree -> every thread
template <int BLOCK>
__device__ __forceinline__ double block_sum(double *p, double x)
{
    const int t = threadIdx.x;
    __syncthreads();
    p[t] = x;
    __syncthreads();
    for (int h = BLOCK >> 1; h > 0; h >>= 1) {
        if (t < h) p[t] += p[t + h];
        __syncthreads();
    }
    return p[0];
}

// the mean and the variance of the n advantages d(i) = returns - values, by one workgroup of BLOCK threads -> every thread
template <int BLOCK, class N, class D>
__device__ __forceinline__ void adv_moments(double *p, N n, D d, double *mean, double *var)
{
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = t; i < n; i += BLOCK) s += (double)d(i);
    *mean = block_sum<BLOCK>(p, s) / (double)n;
    s = 0.0;
    for (int64_t i = t; i < n; i += BLOCK) {
        const double e = (double)d(i) - *mean;
        s += e * e;
    }
    *var = block_sum<BLOCK>(p, s) / (double)n;
}

// what the heads take: float32(mean) and float32(1 / (std + 1e-8))
__device__ __forceinline__ void store_adv(float *adv, double mean, double var)
{
    adv[0] = (float)mean;
    adv[1] = (float)(1.0 / (sqrt(var) + 1.0e-8));
}

// the Gaussian head: sigma_j and the two constants of neglogp and the entropy from four logstd
__device__ __forceinline__ void head_consts(const float *ls, float *sig, float *cnl, double *ent)
{
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kOut; ++j) { sig[j] = expf(ls[j]); s += (double)ls[j]; }
    *cnl = (float)(2.0 * kLog2Pi + s);           // 2 log(2 pi) + sum logstd
    *ent = s + 2.0 * kLog2PiE;                   // sum logstd + 2 log(2 pi e)
}

}  // namespace qsf
