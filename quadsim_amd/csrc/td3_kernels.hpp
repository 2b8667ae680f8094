// td3_kernels.hpp -- the kernels of libquadsim_td3.so (include/quadsim_td3.h has the numerical contract).  A fragment of td3.hip,
// nowhere else.  Built from train_pieces.hpp (the chunk primitives, the tower pieces -- the LDS image and its loader, the element map,
// backward_chunk --, the streamed forward pass of a net that lies in memory and tanh_keep_nan) and from train_offpolicy.hpp (the
// flat net, the copy table, the selects of the target, a critic's forward pass with dq and its sums, the backward pass through the
// streamed q1 and the Adam-and-Polyak tail); philox_counter and normals_from_words are quadsim_device.hpp's.
//
// One update is ONE launch, and the kernel boundary is the only ordering across workgroups:
//   k_td3_step   grid (2) on a critic-only update, (3) on an actor update.  Workgroups 0 and 1 are the critic branches of q1 and q2:
//                the online critic 16 -> 128 -> 128 -> 1 in LDS in the tower's transposed image (layer 0 is sixteen real inputs high,
//                the head run as four outputs of which three have zero weights).  Per 16-row chunk a critic branch computes y
//                ITSELF: it reads the three target nets forward-only from memory (stream_layer), smooths the target action and
//                takes the twin minimum; then the critic forward and backward, gradients in registers, rows ascending.  Both
//                critic branches compute the same y: redundant work, but nothing waits on another workgroup.  Workgroup 2 is the
//                actor branch: the online actor in LDS, the online q1 read forward-only from memory, dq/da back through all three
//                layers of q1 into the actor's backward pass.  Every branch then applies Adam to its net and, on an actor update,
//                the Polyak average to its target, every thread on the elements it accumulated.
//   k_td3_copy   one workgroup per tensor: the caller's 72 tensors into the workspace before the first step, out of it (with the
//                eighteen gradients, where asked for) after the last.
// A branch reads other branches' nets from BEFORE the step, so every net has two places in the workspace and a bit of `cur` says
// which one holds it now: a net that a step writes changes places, a net that it leaves alone (the actor and the three targets on
// a critic-only update) stays where it is and keeps its bits.  Moments and gradients have one copy: only their branch touches
// them.  Nothing waits on another workgroup, there is no grid barrier and no float atomic.
#pragma once
#include "train_offpolicy.hpp"

namespace qstd {

using namespace qsf;

constexpr int kNets = 6, kOnlineNets = 3;                     // the ABI's order: actor, q1, q2, then their targets
constexpr int kCopyTensors = 90;                              // 36 weights, 36 moments, 18 gradients
constexpr uint64_t kStreamNoise = 6;                          // the Philox stream of the target noise (quadsim_device.hpp uses 0 .. 5)

// the flat nets.  B = 0: a critic (sixteen inputs, one output), B = 1: the actor
template <int B>
using Flat = FlatNet<B ? kIn : kCIn, kH, B ? kAct : 1>;
// an online net k = 0 .. 2 among the three: actor | q1 | q2.  A buffer: the three online nets, then the three targets
constexpr int online_at(int k) { return k == 0 ? 0 : Flat<1>::floats + (k - 1) * Flat<0>::floats; }
constexpr int kOnline = Flat<1>::floats + 2 * Flat<0>::floats, kBuf = 2 * kOnline;
constexpr int net_at(int k) { return (k >= kOnlineNets ? kOnline : 0) + online_at(k % kOnlineNets); }
// the workspace, in floats: two buffers, then m, v and the gradients of the three online nets (laid out as the online nets are)
constexpr int kWsM = 2 * kBuf, kWsV = kWsM + kOnline, kWsG = kWsV + kOnline, kWsFloats = kWsG + kOnline;

struct StepArgs {
    float *ws;
    const float *obs0, *act, *rew, *obs1, *done;
    const int32_t *indices, *counts;             // the step's row [batch]; the step's count, nullable
    const float *noise;                          // the step's [batch,4], nullable: keyed draws
    float *noise_out;                            // the step's [batch,4], nullable
    float *stats;                                // the step's six
    uint64_t seed, u;                            // the update index t0 + s keys the draws
    float lr_t[2];                               // critics, actor
    float b1f, b2f, omb1, omb2, eps, gamma, tau, omt, sigma, cl;
    int batch, cur, actor_step, want_grads;      // cur: bit k = the buffer that holds net k before this step
};

struct CopyArgs : CopyTable<kCopyTensors> {};

// where net k lies before the step, and where the step puts it if it writes it
__device__ __forceinline__ const float *net_cur(const StepArgs &S, int k) { return S.ws + ((S.cur >> k) & 1) * kBuf + net_at(k); }
__device__ __forceinline__ float *net_nxt(const StepArgs &S, int k) { return S.ws + (((S.cur >> k) & 1) ^ 1) * kBuf + net_at(k); }

// the tower's image and the planes of backward_chunk, then: the critic's scalars per row (reward, done, y, q, q - y) and the noise;
// the actor's copy of q1's input (obs0 | pi), q1's two hidden planes and q(pi)
struct LayoutC : TowerImage<> {
    static constexpr int d2 = planes, d1 = d2 + kH * kRP;
    static constexpr int zn = d1 + kH * kRP, sc = zn + kAct * kRP;
    static constexpr int floats = sc + 5 * kRP;
};
struct LayoutA : TowerImage<> {
    static constexpr int d2 = planes, d1 = d2 + kH * kRP;
    static constexpr int cx = d1 + kH * kRP, c0 = cx + kCIn * kRP, c1 = c0 + kH * kRP, sc = c1 + kH * kRP;
    static constexpr int floats = sc + kRP;
};
constexpr int kLdsFloats = LayoutC::floats > LayoutA::floats ? LayoutC::floats : LayoutA::floats;
static_assert(kLdsFloats * 4 <= 160 * 1024, "LDS");

// the Adam step of online net k (train_offpolicy.hpp's apply_step), with its target's average where the targets move
template <class L, class F, bool ACTION_ROWS>
__device__ __forceinline__ void apply_step(float *lds, const StepArgs &S, int k, float lr_t, bool polyak, const Acc &G)
{
    const Adam A{S.b1f, S.b2f, S.omb1, S.omb2, S.eps, lr_t};
    const StepPlaces P{net_nxt(S, k), S.ws + kWsM + online_at(k), S.ws + kWsV + online_at(k),
                       S.want_grads ? S.ws + kWsG + online_at(k) : nullptr, net_cur(S, k + kOnlineNets), net_nxt(S, k + kOnlineNets)};
    qsf::apply_step<L, F, ACTION_ROWS>(lds, A, P, S.tau, S.omt, polyak, G, NoMore());
}

// ---- a critic branch: k = 1 (q1) or 2 (q2)
__device__ __forceinline__ void critic_branch(float *lds, const StepArgs &S, int k)
{
    using L = LayoutC;
    using F = Flat<0>;
    const int t = threadIdx.x;
    const float *net = net_cur(S, k);
    const float *at = net_cur(S, 3), *qa_net = net_cur(S, 4), *qb_net = net_cur(S, 5);

    // ---- the online critic into LDS, all sixteen input rows of layer 0 (the chunk loop opens with the barrier)
    load_image<L>(lds, L::floats, F::outs, [&](int slot, int i) { return net[F::at(slot) + i]; });
    for (int i = t; i < kAct * kH; i += kFitBlock) lds[L::w1 + (i & (kH - 1)) * L::ld1 + kIn + (i >> 7)] = net[F::w0 + kIn * kH + i];

    const int rows = step_rows(S);
    const float dscale = (float)(2.0 / (double)rows), frows = (float)rows;

    const int o1 = t & 127, ig1 = t >> 7;
    Acc G;
    zero_acc(G);
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;               // thread kStatT: the sums of the rows so far

    for (int r0 = 0; r0 < rows; r0 += kRows) {
        // (phase C and the action rows of the chunk before still read x and d1: the barrier)
        __syncthreads();
        const int gr = t & (kRows - 1), gc = t >> 4;
        int idx = -1;
        if (gc < kCIn + 2 && r0 + gr < rows) idx = S.indices[r0 + gr];
        // ---- y: the three target nets streamed, the target action smoothed, the smaller of the two target values
        // (the gather and the noise are train_offpolicy.hpp's gather_critic and load_noise written out: called, they compile to
        // another kernel here.  A change to those pieces must be made here too)
        float pre = 0.0f;                                // the thread's value of (obs0 | act), fetched under the target pass
        if (gc < kIn) {
            lds[L::x + gc * kRP + gr] = idx < 0 ? 0.0f : S.obs1[(int64_t)idx * kIn + gc];
            pre = idx < 0 ? 0.0f : S.obs0[(int64_t)idx * kIn + gc];
        } else if (gc < kCIn) {
            pre = idx < 0 ? 0.0f : S.act[(int64_t)idx * kAct + (gc - kIn)];
        } else if (gc == kCIn) {
            lds[L::sc + gr] = idx < 0 ? 0.0f : S.rew[idx];
            lds[L::sc + kRP + gr] = idx < 0 ? 1.0f : S.done[idx];
        } else if (gc == kCIn + 1) {
            // the four normals of row slot r0 + gr: the caller's, or Philox block u of subsequence (6 << 48) | slot
            float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (idx >= 0) {
                const int64_t slot = r0 + gr;
                if (S.noise) {
#pragma unroll
                    for (int c = 0; c < kAct; ++c) z[c] = S.noise[slot * kAct + c];
                } else {
                    qs::normals_from_words(qs::philox_counter(S.seed, (kStreamNoise << 48) | (uint64_t)slot, S.u), z);
                }
                if (S.noise_out && k == 1) {
#pragma unroll
                    for (int c = 0; c < kAct; ++c) S.noise_out[slot * kAct + c] = z[c];
                }
            }
#pragma unroll
            for (int c = 0; c < kAct; ++c) lds[L::zn + c * kRP + gr] = z[c];
        }
        __syncthreads();
        stream_layer<true>(at + Flat<1>::w0, at + Flat<1>::b0, lds + L::x, kIn, lds + L::a1);
        __syncthreads();
        stream_layer<true>(at + Flat<1>::w1, at + Flat<1>::b1, lds + L::a1, kH, lds + L::a2);
        __syncthreads();
        if (t < kAct * kRows) {
            const float a1 = tanh_keep_nan(stream_head<kAct>(at + Flat<1>::w2, at + Flat<1>::b2, lds + L::a2));
            const float e = clampsel(__fmul_rn(S.sigma, lds[L::zn + gc * kRP + gr]), -S.cl, S.cl);
            lds[L::x + (kIn + gc) * kRP + gr] = clampsel(__fadd_rn(a1, e), -1.0f, 1.0f);
        }
        __syncthreads();
        stream_layer<true>(qa_net + F::w0, qa_net + F::b0, lds + L::x, kCIn, lds + L::a1);
        stream_layer<true>(qb_net + F::w0, qb_net + F::b0, lds + L::x, kCIn, lds + L::d1);
        __syncthreads();
        stream_layer<true>(qa_net + F::w1, qa_net + F::b1, lds + L::a1, kH, lds + L::a2);
        stream_layer<true>(qb_net + F::w1, qb_net + F::b1, lds + L::d1, kH, lds + L::d2);
        __syncthreads();
        if (t < kRows) {
            const float qa = stream_head<1>(qa_net + F::w2, qa_net + F::b2, lds + L::a2);
            const float qb = stream_head<1>(qb_net + F::w2, qb_net + F::b2, lds + L::d2);
            const float m = twin_min(qa, qb);
            const float rew = lds[L::sc + t], done = lds[L::sc + kRP + t];
            lds[L::sc + 2 * kRP + t] = td_target(rew, done, S.gamma, m);
        }
        if (gc < kCIn) lds[L::x + gc * kRP + gr] = pre;
        __syncthreads();
        // ---- the critic on (obs0, act), then dq over y's first row
        critic_forward_dq<L, kH, true>(lds, r0, rows, dscale);
        critic_sums<L, true>(lds, r0, rows, s0, s1, s2);
        backward_chunk<L>(lds, G);
        // the four action rows of w0, by the threads that own layer 0's padding in the tower's map and whose g1 backward_chunk
        // leaves alone: phase C's chain on inputs 12 .. 15 (dz0 is complete since phase B's barrier).  (The same text stands in
        // sac_kernels.hpp: as a shared piece it compiled to another kernel in either.  A change here must be made there too)
        if (ig1 == 3) {
#pragma clang loop unroll(disable)
            for (int rg = 0; rg < kRG; ++rg) {
                const f32x4 dz = ld4(lds + L::d1 + o1 * kRP + 4 * rg);
#pragma unroll
                for (int a = 0; a < kAct; ++a) {
                    const f32x4 xv = ld4(lds + L::x + (kIn + a) * kRP + 4 * rg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) G.g1[a] = __fmaf_rn(dz[r], xv[r], G.g1[a]);
                }
            }
        }
    }

    apply_step<L, F, true>(lds, S, k, S.lr_t[0], S.actor_step != 0, G);
    if (t == kStatT) {
        S.stats[k - 1] = __fdiv_rn(s0, frows);
        S.stats[k + 1] = __fdiv_rn(s1, frows);
        if (k == 1) {
            S.stats[4] = __fdiv_rn(s2, frows);
            if (!S.actor_step) S.stats[5] = 0.0f;
        }
    }
}

// ---- the actor branch (actor updates only)
__device__ __forceinline__ void actor_branch(float *lds, const StepArgs &S)
{
    using L = LayoutA;
    using F = Flat<1>;
    using FC = Flat<0>;
    const int t = threadIdx.x;
    const float *net = net_cur(S, 0), *cr = net_cur(S, 1);

    load_image<L>(lds, L::floats, F::outs, [&](int slot, int i) { return net[F::at(slot) + i]; });

    const int rows = step_rows(S);
    const float ninv = -(float)(1.0 / (double)rows), frows = (float)rows;

    Acc G;
    zero_acc(G);
    float s0 = 0.0f;

    for (int r0 = 0; r0 < rows; r0 += kRows) {
        __syncthreads();
        const int gr = t & (kRows - 1), gc = t >> 4;
        if (gc < kIn) {
            const int idx = r0 + gr < rows ? S.indices[r0 + gr] : -1;
            const float v = idx < 0 ? 0.0f : S.obs0[(int64_t)idx * kIn + gc];
            lds[L::x + gc * kRP + gr] = v;
            lds[L::cx + gc * kRP + gr] = v;
        }
        __syncthreads();
        // ---- pi = actor(obs0), q1(obs0, pi) with the online q1 streamed
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        __syncthreads();
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
        __syncthreads();
        if (t < kAct * kRows) {
            const float a = tanh_keep_nan(lds[L::y + gc * kRP + gr]);
            lds[L::y + gc * kRP + gr] = a;
            lds[L::cx + (kIn + gc) * kRP + gr] = a;
        }
        __syncthreads();
        stream_layer<true>(cr + FC::w0, cr + FC::b0, lds + L::cx, kCIn, lds + L::c0);
        __syncthreads();
        stream_layer<true>(cr + FC::w1, cr + FC::b1, lds + L::c0, kH, lds + L::c1);
        __syncthreads();
        if (t < kRows) lds[L::sc + t] = stream_head<1>(cr + FC::w2, cr + FC::b2, lds + L::c1);
        backward_streamed<L, FC>(lds, cr, r0, rows, ninv);
        if (t < kAct * kRows) {
            const float *w = cr + FC::w0 + (kIn + gc) * kH;
            float da = 0.0f;
#pragma unroll 8
            for (int i = 0; i < kH; ++i) da = __fmaf_rn(w[i], lds[L::d1 + i * kRP + gr], da);
            const float a = lds[L::y + gc * kRP + gr];
            lds[L::y + gc * kRP + gr] = __fmul_rn(da, __fmaf_rn(-a, a, 1.0f));
        }
        if (t == kStatT)
            for (int r = 0; r < kRows && r0 + r < rows; ++r) s0 = __fadd_rn(s0, lds[L::sc + r]);
        __syncthreads();
        backward_chunk<L>(lds, G);
    }

    apply_step<L, F, false>(lds, S, 0, S.lr_t[1], true, G);
    if (t == kStatT) S.stats[5] = -__fdiv_rn(s0, frows);
}

__global__ __launch_bounds__(kFitBlock) void k_td3_step(StepArgs S)
{
    __shared__ __align__(16) float lds[kLdsFloats];
    if (blockIdx.x < 2) critic_branch(lds, S, (int)blockIdx.x + 1);
    else actor_branch(lds, S);
}

__global__ __launch_bounds__(kCopyBlock) void k_td3_copy(CopyArgs C)
{
    copy_tensor(C);
}

}  // namespace qstd
