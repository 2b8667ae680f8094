// sac_kernels.hpp -- the kernels of libquadsim_sac.so (include/quadsim_sac.h has the numerical contract).  A fragment of sac.hip,
// nowhere else.  Built from train_pieces.hpp (the chunk primitives, the tower pieces -- the LDS image and its loader, the element map,
// backward_chunk --, the streamed forward pass of a net that lies in memory and tanh_keep_nan) and from train_offpolicy.hpp (the
// flat net, the copy table, the twin minimum, the noise load, a critic's replay gather and forward pass with dq, the backward pass
// through the streamed q1 and the Adam-and-Polyak tail); q_ln, philox_counter and normals_from_words are quadsim_device.hpp's.
// Three pieces of train_offpolicy.hpp are written out below, because called they compile to another kernel here: td_target and
// critic_sums in the critic branch, and the action rows of w0, which td3_kernels.hpp holds in the same words.  A change to one of
// them must be made here too.
//
// One update is ONE launch, and the kernel boundary is the only ordering across workgroups:
//   k_sac_step   grid (4).  Workgroups 0 and 1 are the critic branches of q1 and q2: the online critic 16 -> 128 -> 128 -> 1 in LDS in
//                the tower's transposed image; per 16-row chunk the branch streams v_target forward-only from memory for y, then the
//                critic forward and backward, gradients in registers, rows ascending.  Workgroup 2 is the value branch: the value net
//                12 -> 128 -> 128 -> 1 in LDS; it streams the online actor, samples, streams both online critics, takes the minimum and
//                regresses v(obs0) on it; after Adam it averages v_target.  Workgroup 3 is the actor branch: the actor with its
//                eight-wide head in LDS, the sample and its log-probability, the online q1 streamed, dq/da back through all three
//                layers of q1, the Jacobian and the Gaussian terms into the mean and the log-std head; its statistics thread steps
//                the temperature.  The value and the actor branch both sample and both compute logp: redundant work, but nothing
//                waits on another workgroup.
//   k_sac_copy   one workgroup per tensor: the caller's tensors into the workspace before the first step, out of it (with the
//                24 gradients, where asked for) after the last.
//   k_sac_math   the device functions of the log-probability, element-wise (qss_math).
// A branch reads other branches' nets from BEFORE the step, so every net and log_alpha have two places in the workspace and the
// parity of the step says which one holds them now.  Moments and gradients have one copy: only their branch touches them.  Nothing
// waits on another workgroup, there is no grid barrier and no float atomic.
#pragma once
#include "train_offpolicy.hpp"

namespace qssac {

using namespace qsf;

constexpr int kHead = 2 * kAct;
constexpr int kNets = 5, kOnlineNets = 4;                     // the ABI's order: actor, q1, q2, v, then v_target
constexpr int kMathBlock = 256;
constexpr int kCopyTensors = 6 * kNets + 12 * kOnlineNets + 6 * kOnlineNets + 2;      // weights, moments, gradients, alpha_state in two parts
constexpr uint64_t kStreamNoise = 7;                          // the Philox stream of the sample's noise (0 .. 6 are taken)
constexpr float kL2Pi = 1.8378770664093453f, kE6 = 1.0e-6f, kLsLo = -20.0f, kLsHi = 2.0f;

// the flat nets
using FA = FlatNet<kIn, kH, kHead>;                    // the actor
using FC = FlatNet<kCIn, kH, 1>;                       // a critic
using FV = FlatNet<kIn, kH, 1>;                        // the value net and its target
// net k in a buffer: actor | q1 | q2 | v | v_target
constexpr int net_at(int k) { return k == 0 ? 0 : FA::floats + (k < 3 ? k - 1 : 2) * FC::floats + (k < 4 ? 0 : FV::floats); }
constexpr int kOnline = net_at(4), kBuf = kOnline + FV::floats;
// the workspace, in floats: two buffers, then m, v and the gradients of the four online nets (laid out as the online nets are), then
// log_alpha's two places and its m and v
constexpr int kWsM = 2 * kBuf, kWsV = kWsM + kOnline, kWsG = kWsV + kOnline, kWsAlpha = kWsG + kOnline, kWsFloats = kWsAlpha + 4;

struct StepArgs {
    float *ws;
    const float *obs0, *act, *rew, *obs1, *done;
    const int32_t *indices, *counts;             // the step's row [batch]; the step's count, nullable
    const float *noise;                          // the step's [batch,4], nullable: keyed draws
    float *noise_out;                            // the step's [batch,4], nullable
    float *stats;                                // the step's eight
    float *logp_out, *vlogp_out, *act_out, *fwd_out;      // the step's traces, each nullable
    uint64_t seed, u;                            // the update index t0 + s keys the draws
    float lr_t;
    float b1f, b2f, omb1, omb2, eps, gamma, tau, omt, te;
    int batch, cur, auto_alpha, want_grads;      // cur: the buffer that holds every net and log_alpha before this step
};

struct CopyArgs : CopyTable<kCopyTensors> {};

// where net k lies before the step, and where the step puts it
__device__ __forceinline__ const float *net_cur(const StepArgs &S, int k) { return S.ws + S.cur * kBuf + net_at(k); }
__device__ __forceinline__ float *net_nxt(const StepArgs &S, int k) { return S.ws + (S.cur ^ 1) * kBuf + net_at(k); }

// the tower image with the head eight wide: the actor's.  TowerImage's names, so that load_image, for_own and backward_chunk take it
struct ImageA {
    static constexpr int ld1 = kInP + 4, ld2 = kH + 4, ld3 = kH + 4;
    static constexpr int w1 = 0, b1 = w1 + kH * ld1, w2 = b1 + kH, b2 = w2 + kH * ld2, w3 = b2 + kH, b3 = w3 + kHead * ld3;
    static constexpr int x = b3 + 16, a1 = x + kInP * kRP, a2 = a1 + kH * kRP, y = a2 + kH * kRP;
    static constexpr int planes = y + kHead * kRP;
};
// behind the image and the planes of backward_chunk, the critics: the scalars per row (reward, done, y, q, q - y)
struct LayoutC : TowerImage<> {
    static constexpr int d2 = planes, d1 = d2 + kH * kRP, sc = d1 + kH * kRP;
    static constexpr int floats = sc + 5 * kRP;
};
// the value branch: the critics' input (obs0 | a), the streamed actor's head, the noise, the four terms of logp, vb and v - vb
struct LayoutV : TowerImage<> {
    static constexpr int d2 = planes, d1 = d2 + kH * kRP, cx = d1 + kH * kRP, hy = cx + kCIn * kRP, zn = hy + kHead * kRP;
    static constexpr int tm = zn + kAct * kRP, sc = tm + kAct * kRP;
    static constexpr int floats = sc + 2 * kRP;
};
// the actor branch: q1's input (obs0 | a), q1's two hidden planes, the noise, the four terms of logp, q(a) and logp
struct LayoutA : ImageA {
    static constexpr int d2 = planes, d1 = d2 + kH * kRP, cx = d1 + kH * kRP, c0 = cx + kCIn * kRP, c1 = c0 + kH * kRP;
    static constexpr int zn = c1 + kH * kRP, tm = zn + kAct * kRP, sc = tm + kAct * kRP;
    static constexpr int floats = sc + 2 * kRP;
};
constexpr int kLdsFloats = LayoutA::floats > LayoutV::floats ? (LayoutA::floats > LayoutC::floats ? LayoutA::floats : LayoutC::floats)
                                                             : (LayoutV::floats > LayoutC::floats ? LayoutV::floats : LayoutC::floats);
static_assert(kLdsFloats * 4 <= 160 * 1024, "LDS");

// ln(1 - a^2 + 1e-6) from the computed a
__device__ __forceinline__ float jac_ln(float a) { return qs::q_ln(__fadd_rn(__fmaf_rn(-a, a, 1.0f), kE6)); }

// one component of one row's sample (the header's item 2): what the value branch needs (a, term) and what the actor's gradient reads
struct Sample {
    float a, s2, p, t, den, term;
};
__device__ __forceinline__ Sample sample(float mu, float ls_raw, float z)
{
    Sample s;
    const float ls = clampsel(ls_raw, kLsLo, kLsHi), sigma = expf(ls);
    s.p = __fmul_rn(sigma, z);
    s.a = tanh_keep_nan(__fmaf_rn(sigma, z, mu));
    s.den = __fadd_rn(sigma, kE6);
    s.t = __fdiv_rn(s.p, s.den);
    const float g = __fmaf_rn(s.t, s.t, __fmaf_rn(2.0f, ls, kL2Pi));
    s.s2 = __fmaf_rn(-s.a, s.a, 1.0f);
    s.term = __fsub_rn(__fmul_rn(-0.5f, g), qs::q_ln(__fadd_rn(s.s2, kE6)));
    return s;
}

// the Adam step of online net k (train_offpolicy.hpp's apply_step); TARGET: the value net's, which takes v_target along
template <class L, class F, bool ACTION_ROWS, bool TARGET, class More>
__device__ __forceinline__ void apply_step(float *lds, const StepArgs &S, int k, const Acc &G, More more)
{
    const Adam A{S.b1f, S.b2f, S.omb1, S.omb2, S.eps, S.lr_t};
    const StepPlaces P{net_nxt(S, k), S.ws + kWsM + net_at(k), S.ws + kWsV + net_at(k), S.want_grads ? S.ws + kWsG + net_at(k) : nullptr,
                       net_cur(S, kOnlineNets), net_nxt(S, kOnlineNets)};
    qsf::apply_step<L, F, ACTION_ROWS>(lds, A, P, S.tau, S.omt, TARGET, G, more);
}

// ---- a critic branch: k = 1 (q1) or 2 (q2)
__device__ __forceinline__ void critic_branch(float *lds, const StepArgs &S, int k)
{
    using L = LayoutC;
    using F = FC;
    const int t = threadIdx.x;
    const float *net = net_cur(S, k), *vt = net_cur(S, kOnlineNets);

    // ---- the online critic into LDS, all sixteen input rows of layer 0 (the chunk loop opens with the barrier)
    load_image<L>(lds, L::floats, F::outs, [&](int slot, int i) { return net[F::at(slot) + i]; });
    for (int i = t; i < kAct * kH; i += kFitBlock) lds[L::w1 + (i & (kH - 1)) * L::ld1 + kIn + (i >> 7)] = net[F::w0 + kIn * kH + i];

    const int rows = step_rows(S);
    const float dscale = (float)(1.0 / (double)rows), frows = (float)rows;

    const int o1 = t & 127, ig1 = t >> 7;
    Acc G;
    zero_acc(G);
    float s0 = 0.0f, s2 = 0.0f;                          // thread kStatT: the sums of the rows so far

    for (int r0 = 0; r0 < rows; r0 += kRows) {
        // (phase C and the action rows of the chunk before still read x and d1: the barrier)
        __syncthreads();
        const int gr = t & (kRows - 1), gc = t >> 4;
        int idx = -1;
        if (gc < kCIn + 1 && r0 + gr < rows) idx = S.indices[r0 + gr];
        // ---- y: v_target streamed on obs1
        // (pre: the thread's value of (obs0 | act), fetched under the target pass)
        const float pre = gather_critic<L>(lds, S, idx, gr, gc);
        __syncthreads();
        stream_layer<true>(vt + FV::w0, vt + FV::b0, lds + L::x, kIn, lds + L::a1);
        __syncthreads();
        stream_layer<true>(vt + FV::w1, vt + FV::b1, lds + L::a1, kH, lds + L::a2);
        __syncthreads();
        if (t < kRows) {
            const float v1 = stream_head<1>(vt + FV::w2, vt + FV::b2, lds + L::a2);
            const float rew = lds[L::sc + t], done = lds[L::sc + kRP + t];
            const float y = done >= 1.0f ? rew : __fmaf_rn(__fmul_rn(__fsub_rn(1.0f, done), S.gamma), v1, rew);      // (td_target)
            lds[L::sc + 2 * kRP + t] = y;
            if (S.fwd_out && k == 1 && r0 + t < rows) {
                S.fwd_out[(int64_t)(r0 + t) * 5 + 0] = done >= 1.0f ? 0.0f : v1;
                S.fwd_out[(int64_t)(r0 + t) * 5 + 1] = y;
            }
        }
        if (gc < kCIn) lds[L::x + gc * kRP + gr] = pre;
        __syncthreads();
        // ---- the critic on (obs0, act), then dq over y's first row
        critic_forward_dq<L, kH, false>(lds, r0, rows, dscale);
        if (t == kStatT) {
            for (int r = 0; r < kRows && r0 + r < rows; ++r) {
                const float d = lds[L::sc + 4 * kRP + r];
                s0 = __fmaf_rn(d, d, s0);
                s2 = __fadd_rn(s2, lds[L::sc + 2 * kRP + r]);
            }
        }
        backward_chunk<L>(lds, G);
        // the four action rows of w0, by the threads that own layer 0's padding in the tower's map and whose g1 backward_chunk
        // leaves alone: phase C's chain on inputs 12 .. 15 (dz0 is complete since phase B's barrier).  (As in td3_kernels.hpp)
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

    apply_step<L, F, true, false>(lds, S, k, G, NoMore());
    if (t == kStatT) {
        S.stats[k - 1] = __fmul_rn(0.5f, __fdiv_rn(s0, frows));
        if (k == 1) S.stats[7] = __fdiv_rn(s2, frows);
    }
}

// ---- the value branch
__device__ __forceinline__ void value_branch(float *lds, const StepArgs &S)
{
    using L = LayoutV;
    using F = FV;
    const int t = threadIdx.x;
    const float *net = net_cur(S, 3), *ac = net_cur(S, 0), *qa_net = net_cur(S, 1), *qb_net = net_cur(S, 2);

    load_image<L>(lds, L::floats, F::outs, [&](int slot, int i) { return net[F::at(slot) + i]; });

    const int rows = step_rows(S);
    const float dscale = (float)(1.0 / (double)rows), frows = (float)rows;
    const float alpha = expf(S.ws[kWsAlpha + S.cur]);

    Acc G;
    zero_acc(G);
    float s0 = 0.0f;

    for (int r0 = 0; r0 < rows; r0 += kRows) {
        __syncthreads();
        const int gr = t & (kRows - 1), gc = t >> 4;
        const bool valid = r0 + gr < rows;
        if (gc < kIn) {
            const float v = valid ? S.obs0[(int64_t)S.indices[r0 + gr] * kIn + gc] : 0.0f;
            lds[L::x + gc * kRP + gr] = v;
            lds[L::cx + gc * kRP + gr] = v;
        } else if (gc == kIn) {
            load_noise<kStreamNoise>(lds + L::zn, S, r0 + gr, gr, valid, false);
        }
        __syncthreads();
        // ---- the online actor streamed, the sample and the four terms of its logp
        stream_layer<true>(ac + FA::w0, ac + FA::b0, lds + L::x, kIn, lds + L::a1);
        __syncthreads();
        stream_layer<true>(ac + FA::w1, ac + FA::b1, lds + L::a1, kH, lds + L::a2);
        __syncthreads();
        if (t < kHead * kRows) lds[L::hy + gc * kRP + gr] = stream_head<kHead>(ac + FA::w2, ac + FA::b2, lds + L::a2);
        __syncthreads();
        if (t < kAct * kRows) {
            const Sample sm = sample(lds[L::hy + gc * kRP + gr], lds[L::hy + (kAct + gc) * kRP + gr], lds[L::zn + gc * kRP + gr]);
            lds[L::cx + (kIn + gc) * kRP + gr] = sm.a;
            lds[L::tm + gc * kRP + gr] = sm.term;
        }
        __syncthreads();
        // ---- both online critics streamed on (obs0, a), the smaller value, vb
        stream_layer<true>(qa_net + FC::w0, qa_net + FC::b0, lds + L::cx, kCIn, lds + L::a1);
        stream_layer<true>(qb_net + FC::w0, qb_net + FC::b0, lds + L::cx, kCIn, lds + L::d1);
        __syncthreads();
        stream_layer<true>(qa_net + FC::w1, qa_net + FC::b1, lds + L::a1, kH, lds + L::a2);
        stream_layer<true>(qb_net + FC::w1, qb_net + FC::b1, lds + L::d1, kH, lds + L::d2);
        __syncthreads();
        if (t < kRows) {
            const float qa = stream_head<1>(qa_net + FC::w2, qa_net + FC::b2, lds + L::a2);
            const float qb = stream_head<1>(qb_net + FC::w2, qb_net + FC::b2, lds + L::d2);
            const float mn = twin_min(qa, qb);
            float lp = 0.0f;
#pragma unroll
            for (int c = 0; c < kAct; ++c) lp = __fadd_rn(lp, lds[L::tm + c * kRP + t]);
            const float vb = __fsub_rn(mn, __fmul_rn(alpha, lp));
            lds[L::sc + t] = vb;
            if (r0 + t < rows) {
                if (S.vlogp_out) S.vlogp_out[r0 + t] = lp;
                if (S.fwd_out) {
                    S.fwd_out[(int64_t)(r0 + t) * 5 + 2] = qa;
                    S.fwd_out[(int64_t)(r0 + t) * 5 + 3] = qb;
                    S.fwd_out[(int64_t)(r0 + t) * 5 + 4] = vb;
                }
            }
        }
        __syncthreads();
        // ---- v(obs0), then dv over y's first row
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        __syncthreads();
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
        __syncthreads();
        if (t < kRows) {
            const float d = r0 + t < rows ? __fsub_rn(lds[L::y + t], lds[L::sc + t]) : 0.0f;
            lds[L::sc + kRP + t] = d;
            lds[L::y + t] = __fmul_rn(d, dscale);
        }
        __syncthreads();
        if (t == kStatT) {
            for (int r = 0; r < kRows && r0 + r < rows; ++r) {
                const float d = lds[L::sc + kRP + r];
                s0 = __fmaf_rn(d, d, s0);
            }
        }
        backward_chunk<L>(lds, G);
    }

    apply_step<L, F, false, true>(lds, S, 3, G, NoMore());
    if (t == kStatT) S.stats[2] = __fmul_rn(0.5f, __fdiv_rn(s0, frows));
}

// ---- the actor branch
__device__ __forceinline__ void actor_branch(float *lds, const StepArgs &S)
{
    using L = LayoutA;
    using F = FA;
    const int t = threadIdx.x;
    const float *net = net_cur(S, 0), *cr = net_cur(S, 1);

    load_image<L>(lds, L::floats, F::outs, [&](int slot, int i) { return net[F::at(slot) + i]; });

    const int rows = step_rows(S);
    const float rinv = (float)(1.0 / (double)rows), ninv = -rinv, frows = (float)rows;
    const float la = S.ws[kWsAlpha + S.cur], alpha = expf(la), ar = __fmul_rn(alpha, rinv);

    const int o3 = t & 3, i3 = t >> 2;
    Acc G;
    zero_acc(G);
    float g3b = 0.0f;                                    // w2[i3][4 + o3], the log-std head's weight of this thread
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;               // thread kStatT: the sums of the rows so far

    for (int r0 = 0; r0 < rows; r0 += kRows) {
        __syncthreads();
        const int gr = t & (kRows - 1), gc = t >> 4;
        const bool valid = r0 + gr < rows;
        if (gc < kIn) {
            const float v = valid ? S.obs0[(int64_t)S.indices[r0 + gr] * kIn + gc] : 0.0f;
            lds[L::x + gc * kRP + gr] = v;
            lds[L::cx + gc * kRP + gr] = v;
        } else if (gc == kIn) {
            load_noise<kStreamNoise>(lds + L::zn, S, r0 + gr, gr, valid, true);
        }
        __syncthreads();
        // ---- the head of the actor on obs0, the sample, q1(obs0, a) with the online q1 streamed
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        __syncthreads();
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kHead, lds + L::y);
        __syncthreads();
        Sample sm = {};
        float ls_raw = 0.0f;
        if (t < kAct * kRows) {
            ls_raw = lds[L::y + (kAct + gc) * kRP + gr];
            sm = sample(lds[L::y + gc * kRP + gr], ls_raw, lds[L::zn + gc * kRP + gr]);
            lds[L::cx + (kIn + gc) * kRP + gr] = sm.a;
            lds[L::tm + gc * kRP + gr] = sm.term;
            if (S.act_out && valid) S.act_out[(int64_t)(r0 + gr) * kAct + gc] = sm.a;
        }
        __syncthreads();
        stream_layer<true>(cr + FC::w0, cr + FC::b0, lds + L::cx, kCIn, lds + L::c0);
        __syncthreads();
        stream_layer<true>(cr + FC::w1, cr + FC::b1, lds + L::c0, kH, lds + L::c1);
        __syncthreads();
        if (t < kRows) {
            lds[L::sc + t] = stream_head<1>(cr + FC::w2, cr + FC::b2, lds + L::c1);
            float lp = 0.0f;
#pragma unroll
            for (int c = 0; c < kAct; ++c) lp = __fadd_rn(lp, lds[L::tm + c * kRP + t]);
            lds[L::sc + kRP + t] = lp;
            if (S.logp_out && r0 + t < rows) S.logp_out[r0 + t] = lp;
        }
        backward_streamed<L, FC>(lds, cr, r0, rows, ninv);
        if (t < kAct * kRows) {
            // da through q1's action rows, then the header's item 5: du into the mean's head, dls into the log-std head
            const float *w = cr + FC::w0 + (kIn + gc) * kH;
            float da = 0.0f;
#pragma unroll 8
            for (int i = 0; i < kH; ++i) da = __fmaf_rn(w[i], lds[L::d1 + i * kRP + gr], da);
            const float arow = valid ? ar : 0.0f;
            const float jd = __fdiv_rn(__fmul_rn(__fmul_rn(2.0f, sm.a), sm.s2), __fadd_rn(sm.s2, kE6));
            const float du = __fmaf_rn(arow, jd, __fmul_rn(da, sm.s2));
            const float dtl = __fdiv_rn(__fmul_rn(sm.p, kE6), __fmul_rn(sm.den, sm.den));
            const float gl = __fmaf_rn(sm.t, dtl, 1.0f);
            const float dls = __fmaf_rn(du, sm.p, __fmul_rn(-arow, gl));
            lds[L::y + gc * kRP + gr] = du;
            lds[L::y + (kAct + gc) * kRP + gr] = (ls_raw < kLsLo || ls_raw > kLsHi) ? 0.0f : dls;
        }
        if (t == kStatT) {
            for (int r = 0; r < kRows && r0 + r < rows; ++r) {
                const float lp = lds[L::sc + kRP + r];
                s0 = __fadd_rn(s0, __fsub_rn(__fmul_rn(alpha, lp), lds[L::sc + r]));
                s1 = __fadd_rn(s1, lp);
                s2 = __fadd_rn(s2, __fadd_rn(lp, S.te));
            }
        }
        __syncthreads();
        // the log-std head's own gradients (rows 4 .. 7 of the plane y), as backward_chunk's phase A takes the mean head's; then
        // the backward pass with dz1 summed over all eight rows
#pragma clang loop unroll(disable)
        for (int rg = 0; rg < kRG; ++rg) {
            const f32x4 a = ld4(lds + L::a2 + i3 * kRP + 4 * rg), d = ld4(lds + L::y + (kAct + o3) * kRP + 4 * rg);
#pragma unroll
            for (int r = 0; r < 4; ++r) g3b = __fmaf_rn(d[r], a[r], g3b);
        }
        if (t >= 256 + kAct && t < 256 + kHead) {
#pragma unroll
            for (int r = 0; r < kRows; ++r) G.gb = __fadd_rn(G.gb, lds[L::y + (t - 256) * kRP + r]);
        }
        backward_chunk<L, NoExtra, kHead>(lds, G);
    }

    apply_step<L, F, false, false>(lds, S, 0, G, [&](auto apply) { apply(g3b, lds + L::w3 + (kAct + o3) * L::ld3 + i3, F::w2 + i3 * kHead + kAct + o3); });
    if (t == kStatT) {
        const float mean = __fdiv_rn(s2, frows);
        S.stats[3] = __fdiv_rn(s0, frows);
        S.stats[4] = -__fmul_rn(la, mean);
        S.stats[5] = alpha;
        S.stats[6] = __fdiv_rn(s1, frows);
        // the temperature: Adam on log_alpha with the gradient -mean, or its bits kept
        float *A = S.ws + kWsAlpha;
        float next = la;
        if (S.auto_alpha) {
            const float g = -mean;
            const float mn = __fmaf_rn(S.b1f, A[2], __fmul_rn(S.omb1, g));
            const float vn = __fmaf_rn(S.b2f, A[3], __fmul_rn(S.omb2, __fmul_rn(g, g)));
            next = __fsub_rn(la, __fdiv_rn(__fmul_rn(S.lr_t, mn), __fadd_rn(__fsqrt_rn(vn), S.eps)));
            A[2] = mn;
            A[3] = vn;
        }
        A[S.cur ^ 1] = next;
    }
}

__global__ __launch_bounds__(kFitBlock) void k_sac_step(StepArgs S)
{
    __shared__ __align__(16) float lds[kLdsFloats];
    if (blockIdx.x < 2) critic_branch(lds, S, (int)blockIdx.x + 1);
    else if (blockIdx.x == 2) value_branch(lds, S);
    else actor_branch(lds, S);
}

__global__ __launch_bounds__(kCopyBlock) void k_sac_copy(CopyArgs C)
{
    copy_tensor(C);
}

__global__ __launch_bounds__(kMathBlock) void k_sac_math(int which, const float *in, float *out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kMathBlock + threadIdx.x;
    if (i >= n) return;
    const float x = in[i];
    out[i] = which == 0 ? expf(x) : which == 1 ? qs::q_ln(x) : jac_ln(tanh_keep_nan(x));
}

}  // namespace qssac
