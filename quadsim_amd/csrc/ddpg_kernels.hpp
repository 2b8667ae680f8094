// ddpg_kernels.hpp -- the kernels of libquadsim_ddpg.so (include/quadsim_ddpg.h has the numerical contract).  A fragment of
// ddpg.hip, nowhere else.  Built from train_pieces.hpp (the chunk primitives and the tower pieces: the LDS image and its loader,
// the element map, backward_chunk) and from train_offpolicy.hpp (the flat net, the copy table, clampsel, the TD target and a
// critic's forward pass with dq); q_tanh is quadsim_device.hpp's.  Three pieces of train_offpolicy.hpp are written out below,
// because called they compile to another kernel here: the replay gather (gather_critic, here with the clamp), the sums of the statistics (critic_sums)
// and the Adam-and-Polyak tail (apply_step).  A change to one of them must be made here too.
//
// One train step is ONE launch, and the kernel boundary is the only ordering across workgroups:
//   k_ddpg_step  grid (2).  Workgroup 0 is the critic branch: the online critic 12 -> 128 -> (128 + 4 actions) -> 128 -> 1 in LDS
//                in the tower's transposed image, layer 1 widened to 132 inputs and the head run as four outputs of which three
//                have zero weights (they add exact zeros).  Per 16-row chunk it computes y with the two TARGET nets, which it
//                reads forward-only from memory (stream_layer: lanes along the units, so a weight row is one coalesced read and
//                the activation an LDS broadcast), then runs the critic forward and backward, gradients in registers, rows
//                ascending.  Workgroup 1 is the actor branch: the online actor in LDS, the online critic read forward-only from
//                memory, dq/da through the critic's layers 1 and 2 into the actor's backward pass.  Either branch then applies
//                Adam to its net and the Polyak average to its target, every thread on the elements it accumulated.
//   k_ddpg_copy  one workgroup per tensor: the caller's 48 tensors into the workspace before the first step, out of it (with the
//                twelve gradients, where asked for) after the last.
// A branch reads the other branch's weights from BEFORE the step, so the four nets are double-buffered in the workspace: step s
// of a call reads buffer s & 1 and writes buffer (s + 1) & 1.  Moments and gradients have one copy: only their branch touches
// them.  Nothing waits on another workgroup, there is no grid barrier and no float atomic.
#pragma once
#include "train_offpolicy.hpp"

namespace qsdd {

using namespace qsf;

constexpr int kCopyTensors = 60;            // 24 weights, 24 moments, 12 gradients

// the flat nets.  B = 0: the critic (layer 1 has 132 inputs, one output), B = 1: the actor
template <int B>
using Flat = FlatNet<kIn, B ? kH : kH + kAct, B ? kAct : 1>;
constexpr int net_at(int b) { return b ? 0 : Flat<1>::floats; }                     // in a buffer: actor | critic | the two targets
constexpr int kOnline = Flat<0>::floats + Flat<1>::floats, kBuf = 2 * kOnline;     // a target lies kOnline after its online net
// the workspace, in floats: two buffers, then m, v and the gradients of the two online nets (laid out as the online nets are)
constexpr int kWsM = 2 * kBuf, kWsV = kWsM + kOnline, kWsG = kWsV + kOnline, kWsFloats = kWsG + kOnline;

struct StepArgs {
    float *ws;
    const float *obs0, *act, *rew, *obs1, *done;
    const int32_t *indices, *counts;             // the step's row [batch]; the step's count, nullable
    float *stats;                                // the step's four
    float lr_t[2];                               // critic, actor
    float b1f, b2f, omb1, omb2, eps, gamma, tau, omt, clip;
    int batch, cur, want_grads;
};

struct CopyArgs : CopyTable<kCopyTensors> {};

// the tower's image with a1 132 units high in either branch; the critic's rows of w2 are 140 apart (132 and 140: 4 and 12 mod 32
// words)
template <int B>
struct Layout : TowerImage<B ? kH + 4 : kH + kAct + 8, kH + kAct> {
    using T = TowerImage<B ? kH + 4 : kH + kAct + 8, kH + kAct>;
    static constexpr int d2 = T::planes, d1 = d2 + kH * kRP;
    static constexpr int c1 = d1 + kH * kRP;     // the streamed critic's layer-1 input: h0 | action
    static constexpr int sc = c1 + (kH + kAct) * kRP;    // per row: reward, done, y, q, q - y | q(pi)
    static constexpr int floats = sc + 5 * kRP;
};
constexpr int kLdsFloats = Layout<0>::floats > Layout<1>::floats ? Layout<0>::floats : Layout<1>::floats;

// (stream_layer, stream_head and tanh_keep_nan are train_pieces.hpp's: the TD3 kernels stream their nets the same way)

template <int B>
__device__ __forceinline__ void branch(float *lds, const StepArgs &S)
{
    using L = Layout<B>;
    using F = Flat<B>;
    static_assert(L::floats * 4 <= 160 * 1024, "LDS");
    const int t = threadIdx.x;
    const float *cur = S.ws + S.cur * kBuf;
    float *nxt = S.ws + (S.cur ^ 1) * kBuf;
    const float *net = cur + net_at(B);

    // ---- the online net into LDS (the chunk loop opens with the barrier)
    load_image<L, F::k1>(lds, L::floats, F::outs, [&](int k, int i) { return net[F::at(k) + i]; });

    const int rows = step_rows(S);
    const float dscale = (float)(2.0 / (double)rows), ninv = -(float)(1.0 / (double)rows), frows = (float)rows;

    // ---- the gradient elements of this thread; the critic's four action rows of w1 are one element a thread more: input
    // 128 + ig1, output o1
    const int o1 = t & 127, ig1 = t >> 7;
    Acc G;
    zero_acc(G);
    float gx = 0.0f;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;               // thread kStatT: the sums of the rows so far

    for (int r0 = 0; r0 < rows; r0 += kRows) {
        // (phase C of the chunk before still reads x: the barrier)
        __syncthreads();
        const int gr = t & (kRows - 1), gc = t >> 4;
        int idx = -1;
        if (t < (kIn + kAct + 1) * kRows && r0 + gr < rows) idx = S.indices[r0 + gr];
        if (B == 0) {
            // ---- y = rew + (1 - done) gamma q'(obs1, pi'(obs1)), both target nets streamed
            const float *at = cur + net_at(1) + kOnline, *ct = cur + net_at(0) + kOnline;
            float pre = 0.0f;                            // the thread's value of (obs0 | act), fetched under the target pass
            if (gc < kIn) {
                lds[L::x + gc * kRP + gr] = idx < 0 ? 0.0f : clampsel(S.obs1[(int64_t)idx * kIn + gc], -S.clip, S.clip);
                pre = idx < 0 ? 0.0f : clampsel(S.obs0[(int64_t)idx * kIn + gc], -S.clip, S.clip);
            } else if (gc < kIn + kAct) {
                pre = idx < 0 ? 0.0f : S.act[(int64_t)idx * kAct + (gc - kIn)];
            } else if (gc == kIn + kAct) {
                lds[L::sc + gr] = idx < 0 ? 0.0f : S.rew[idx];
                lds[L::sc + kRP + gr] = idx < 0 ? 1.0f : S.done[idx];
            }
            __syncthreads();
            stream_layer<true>(at + Flat<1>::w0, at + Flat<1>::b0, lds + L::x, kIn, lds + L::a1);
            stream_layer<true>(ct + Flat<0>::w0, ct + Flat<0>::b0, lds + L::x, kIn, lds + L::c1);
            __syncthreads();
            stream_layer<true>(at + Flat<1>::w1, at + Flat<1>::b1, lds + L::a1, kH, lds + L::a2);
            __syncthreads();
            if (t < kAct * kRows) {
                lds[L::c1 + (kH + (t >> 4)) * kRP + gr] = tanh_keep_nan(stream_head<kAct>(at + Flat<1>::w2, at + Flat<1>::b2, lds + L::a2));
            }
            __syncthreads();
            stream_layer<true>(ct + Flat<0>::w1, ct + Flat<0>::b1, lds + L::c1, kH + kAct, lds + L::a2);
            __syncthreads();
            if (t < kRows) {
                const float q1 = stream_head<1>(ct + Flat<0>::w2, ct + Flat<0>::b2, lds + L::a2);
                const float rew = lds[L::sc + t], done = lds[L::sc + kRP + t];
                lds[L::sc + 2 * kRP + t] = td_target(rew, done, S.gamma, q1);
            }
            if (gc < kIn) lds[L::x + gc * kRP + gr] = pre;
            else if (gc < kIn + kAct) lds[L::a1 + (kH + gc - kIn) * kRP + gr] = pre;
            __syncthreads();
            // ---- the critic on (obs0, act), then dq over y's first row
            critic_forward_dq<L, kH + kAct, true>(lds, r0, rows, dscale);
            if (t == kStatT) {
                for (int r = 0; r < kRows && r0 + r < rows; ++r) {
                    const float d = lds[L::sc + 4 * kRP + r];
                    s0 = __fmaf_rn(d, d, s0);
                    s1 = __fadd_rn(s1, lds[L::sc + 3 * kRP + r]);
                    s2 = __fadd_rn(s2, lds[L::sc + 2 * kRP + r]);
                }
            }
        } else {
            // ---- pi = actor(obs0), q(obs0, pi) with the online critic streamed, dq/da into y
            const float *cr = cur + net_at(0);
            if (gc < kIn) lds[L::x + gc * kRP + gr] = idx < 0 ? 0.0f : clampsel(S.obs0[(int64_t)idx * kIn + gc], -S.clip, S.clip);
            __syncthreads();
            forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
            stream_layer<true>(cr + Flat<0>::w0, cr + Flat<0>::b0, lds + L::x, kIn, lds + L::c1);
            __syncthreads();
            forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
            __syncthreads();
            forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
            __syncthreads();
            if (t < kAct * kRows) {
                const float a = tanh_keep_nan(lds[L::y + (t >> 4) * kRP + gr]);
                lds[L::y + (t >> 4) * kRP + gr] = a;
                lds[L::c1 + (kH + (t >> 4)) * kRP + gr] = a;
            }
            __syncthreads();
            stream_layer<true>(cr + Flat<0>::w1, cr + Flat<0>::b1, lds + L::c1, kH + kAct, lds + L::d2);
            __syncthreads();
            if (t < kRows) lds[L::sc + t] = stream_head<1>(cr + Flat<0>::w2, cr + Flat<0>::b2, lds + L::d2);
            {
                // dz1 of the critic: dq/dh1 = w2 under h1's mask, times -1 / rows on the step's rows
                const int u = t & (kH - 1), rg = t >> 7;
                const float w2u = cr[Flat<0>::w2 + u];
                const f32x4 h = ld4(lds + L::d2 + u * kRP + 4 * rg);
                f32x4 dz;
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[r] = (h[r] > 0.0f && r0 + 4 * rg + r < rows) ? __fmul_rn(w2u, ninv) : 0.0f;
                st4(lds + L::d1 + u * kRP + 4 * rg, dz);
            }
            __syncthreads();
            if (t < kAct * kRows) {
                const float *w = cr + Flat<0>::w1 + (kH + (t >> 4)) * kH;
                float da = 0.0f;
#pragma unroll 8
                for (int o = 0; o < kH; ++o) da = __fmaf_rn(w[o], lds[L::d1 + o * kRP + gr], da);
                const float a = lds[L::y + (t >> 4) * kRP + gr];
                lds[L::y + (t >> 4) * kRP + gr] = __fmul_rn(da, __fmaf_rn(-a, a, 1.0f));
            }
            if (t == kStatT)
                for (int r = 0; r < kRows && r0 + r < rows; ++r) s0 = __fadd_rn(s0, lds[L::sc + r]);
            __syncthreads();
        }

        backward_chunk<L>(lds, G, [&] {
            if (B == 0) {
#pragma clang loop unroll(disable)
                for (int rg = 0; rg < kRG; ++rg) {
                    const f32x4 dz = ld4(lds + L::d2 + o1 * kRP + 4 * rg), av = ld4(lds + L::a1 + (kH + ig1) * kRP + 4 * rg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) gx = __fmaf_rn(dz[r], av[r], gx);
                }
            }
        });
    }

    // ---- Adam on the thread's own elements (m and v through memory, the weight from LDS into the next buffer), then the
    // target's average with the new weight.  No thread reads another's element here
    const Adam A{S.b1f, S.b2f, S.omb1, S.omb2, S.eps, S.lr_t[B]};
    float *wn = nxt + net_at(B), *m = S.ws + kWsM + net_at(B), *v = S.ws + kWsV + net_at(B);
    float *gout = S.want_grads ? S.ws + kWsG + net_at(B) : nullptr;
    const float *tc = cur + net_at(B) + kOnline;
    float *tn = nxt + net_at(B) + kOnline;
    auto apply = [&](float g, float *lw, int e) {
        adam_step(A, g, lw, wn, m, v, gout, e);
        tn[e] = __fmaf_rn(S.tau, *lw, __fmul_rn(S.omt, tc[e]));
    };
    for_own<L, F::outs>(t, [&](int off, int idx, int slot, const float &g) { apply(g, lds + off, F::at(slot) + idx); }, G);
    if (B == 0) apply(gx, lds + L::w2 + o1 * L::ld2 + kH + ig1, F::w1 + (kH + ig1) * kH + o1);
    if (t == kStatT) {
        if (B == 0) {
            S.stats[0] = __fdiv_rn(s0, frows);
            S.stats[2] = __fdiv_rn(s1, frows);
            S.stats[3] = __fdiv_rn(s2, frows);
        } else {
            S.stats[1] = -__fdiv_rn(s0, frows);
        }
    }
}

__global__ __launch_bounds__(kFitBlock) void k_ddpg_step(StepArgs S)
{
    __shared__ __align__(16) float lds[kLdsFloats];
    if (blockIdx.x == 0) branch<0>(lds, S);
    else branch<1>(lds, S);
}

__global__ __launch_bounds__(kCopyBlock) void k_ddpg_copy(CopyArgs C)
{
    copy_tensor(C);
}

}  // namespace qsdd
