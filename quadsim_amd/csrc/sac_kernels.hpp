// sac_kernels.hpp -- the kernels of libquadsim_sac.so (include/quadsim_sac.h has the numerical contract).  A fragment of sac.hip,
// nowhere else.  Built from train_pieces.hpp: the chunk primitives, the tower pieces (the LDS image and its loader, the element map,
// backward_chunk), the streamed forward pass of a net that lies in memory and tanh_keep_nan; q_ln, philox_counter and
// normals_from_words are quadsim_device.hpp's.
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
#include "train_pieces.hpp"

namespace qssac {

using namespace qsf;

constexpr int kAct = 4, kHead = 2 * kAct, kCIn = kIn + kAct;
constexpr int kNets = 5, kOnlineNets = 4;                     // the ABI's order: actor, q1, q2, v, then v_target
constexpr int kCopyBlock = 256, kMathBlock = 256;
constexpr int kCopyTensors = 6 * kNets + 12 * kOnlineNets + 6 * kOnlineNets + 2;      // weights, moments, gradients, alpha_state in two parts
constexpr uint64_t kStreamNoise = 7;                          // the Philox stream of the sample's noise (0 .. 6 are taken)
constexpr float kL2Pi = 1.8378770664093453f, kE6 = 1.0e-6f, kLsLo = -20.0f, kLsHi = 2.0f;
static_assert(kCIn == kInP, "a critic's layer 0 fills the tower image's sixteen input rows");

// a net as it lies flat in the workspace, tensors in the ABI's order and the policy's (in, out) layout
template <int K0, int OUTS>
struct Flat {
    static constexpr int k0 = K0, outs = OUTS;
    static constexpr int w0 = 0, b0 = w0 + k0 * kH, w1 = b0 + kH, b1 = w1 + kH * kH, w2 = b1 + kH, b2 = w2 + kH * outs;
    static constexpr int floats = (b2 + outs + 3) & ~3;
    static constexpr int at(int k) { return k == 0 ? w0 : k == 1 ? b0 : k == 2 ? w1 : k == 3 ? b1 : k == 4 ? w2 : b2; }   // slot k's start
};
using FA = Flat<kIn, kHead>;                     // the actor
using FC = Flat<kCIn, 1>;                        // a critic
using FV = Flat<kIn, 1>;                         // the value net and its target
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

struct CopyArgs {
    float *t[kCopyTensors];
    int at[kCopyTensors], n[kCopyTensors];
    float *ws;
    int to_ws;
};

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

// (a select, not fminf(fmaxf()): those would drop a NaN; an infinity is clamped as any other value)
__device__ __forceinline__ float clampsel(float v, float lo, float hi) { return v < lo ? lo : v > hi ? hi : v; }

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

// the four normals of row slot `slot` into the planes zn: the caller's, or Philox block u of subsequence (7 << 48) | slot
__device__ __forceinline__ void load_noise(float *zn, const StepArgs &S, int slot, int gr, bool valid, bool write_out)
{
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        if (S.noise) {
#pragma unroll
            for (int c = 0; c < kAct; ++c) z[c] = S.noise[(int64_t)slot * kAct + c];
        } else {
            qs::normals_from_words(qs::philox_counter(S.seed, (kStreamNoise << 48) | (uint64_t)slot, S.u), z);
        }
        if (S.noise_out && write_out) {
#pragma unroll
            for (int c = 0; c < kAct; ++c) S.noise_out[(int64_t)slot * kAct + c] = z[c];
        }
    }
#pragma unroll
    for (int c = 0; c < kAct; ++c) zn[c * kRP + gr] = z[c];
}

// Adam on the thread's own elements (m and v through memory, the weight from LDS into the net's next place), then, for the value
// net, the target's average with the new weight.  No thread reads another's element here.  ACTION_ROWS: the four action rows of a
// critic's w0, which the owners of layer 0's padding in the tower's map hold in g1
template <class L, class F, bool ACTION_ROWS, bool TARGET, class More>
__device__ __forceinline__ void apply_step(float *lds, const StepArgs &S, int k, const Acc &G, More more)
{
    const int t = threadIdx.x;
    const Adam A{S.b1f, S.b2f, S.omb1, S.omb2, S.eps, S.lr_t};
    float *wn = net_nxt(S, k), *m = S.ws + kWsM + net_at(k), *v = S.ws + kWsV + net_at(k);
    float *gout = S.want_grads ? S.ws + kWsG + net_at(k) : nullptr;
    const float *tc = net_cur(S, kOnlineNets);
    float *tn = net_nxt(S, kOnlineNets);
    auto apply = [&](float g, float *lw, int e) {
        adam_step(A, g, lw, wn, m, v, gout, e);
        if (TARGET) tn[e] = __fmaf_rn(S.tau, *lw, __fmul_rn(S.omt, tc[e]));
    };
    for_own<L, F::outs>(t, [&](int off, int idx, int slot, const float &g) { apply(g, lds + off, F::at(slot) + idx); }, G);
    if (ACTION_ROWS) {
        const int o1 = t & 127;
        if ((t >> 7) == 3) {
#pragma unroll
            for (int a = 0; a < kAct; ++a) apply(G.g1[a], lds + L::w1 + o1 * L::ld1 + kIn + a, F::w0 + (kIn + a) * kH + o1);
        }
    }
    more(apply);
}
struct NoMore {
    template <class Fn>
    __device__ __forceinline__ void operator()(Fn) const {}
};

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

    int rows = S.counts ? S.counts[0] : S.batch;
    rows = rows < S.batch ? rows : S.batch;
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
        float pre = 0.0f;                                // the thread's value of (obs0 | act), fetched under the target pass
        if (gc < kIn) {
            lds[L::x + gc * kRP + gr] = idx < 0 ? 0.0f : S.obs1[(int64_t)idx * kIn + gc];
            pre = idx < 0 ? 0.0f : S.obs0[(int64_t)idx * kIn + gc];
        } else if (gc < kCIn) {
            pre = idx < 0 ? 0.0f : S.act[(int64_t)idx * kAct + (gc - kIn)];
        } else if (gc == kCIn) {
            lds[L::sc + gr] = idx < 0 ? 0.0f : S.rew[idx];
            lds[L::sc + kRP + gr] = idx < 0 ? 1.0f : S.done[idx];
        }
        __syncthreads();
        stream_layer<true>(vt + FV::w0, vt + FV::b0, lds + L::x, kIn, lds + L::a1);
        __syncthreads();
        stream_layer<true>(vt + FV::w1, vt + FV::b1, lds + L::a1, kH, lds + L::a2);
        __syncthreads();
        if (t < kRows) {
            const float v1 = stream_head<1>(vt + FV::w2, vt + FV::b2, lds + L::a2);
            const float rew = lds[L::sc + t], done = lds[L::sc + kRP + t];
            const float y = done >= 1.0f ? rew : __fmaf_rn(__fmul_rn(__fsub_rn(1.0f, done), S.gamma), v1, rew);
            lds[L::sc + 2 * kRP + t] = y;
            if (S.fwd_out && k == 1 && r0 + t < rows) {
                S.fwd_out[(int64_t)(r0 + t) * 5 + 0] = done >= 1.0f ? 0.0f : v1;
                S.fwd_out[(int64_t)(r0 + t) * 5 + 1] = y;
            }
        }
        if (gc < kCIn) lds[L::x + gc * kRP + gr] = pre;
        __syncthreads();
        // ---- the critic on (obs0, act), then dq over y's first row
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        __syncthreads();
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
        __syncthreads();
        if (t < kRows) {
            const bool valid = r0 + t < rows;
            const float q = lds[L::y + t], d = valid ? __fsub_rn(q, lds[L::sc + 2 * kRP + t]) : 0.0f;
            lds[L::sc + 4 * kRP + t] = d;
            lds[L::y + t] = __fmul_rn(d, dscale);
        }
        __syncthreads();
        if (t == kStatT) {
            for (int r = 0; r < kRows && r0 + r < rows; ++r) {
                const float d = lds[L::sc + 4 * kRP + r];
                s0 = __fmaf_rn(d, d, s0);
                s2 = __fadd_rn(s2, lds[L::sc + 2 * kRP + r]);
            }
        }
        backward_chunk<L>(lds, G);
        // the four action rows of w0, by the threads that own layer 0's padding in the tower's map and whose g1 backward_chunk
        // leaves alone: phase C's chain on inputs 12 .. 15 (dz0 is complete since phase B's barrier)
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

    int rows = S.counts ? S.counts[0] : S.batch;
    rows = rows < S.batch ? rows : S.batch;
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
            load_noise(lds + L::zn, S, r0 + gr, gr, valid, false);
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
            const float mn = qa != qa ? qa : qb != qb ? qb : (qb < qa ? qb : qa);
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

    int rows = S.counts ? S.counts[0] : S.batch;
    rows = rows < S.batch ? rows : S.batch;
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
            load_noise(lds + L::zn, S, r0 + gr, gr, valid, true);
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
        {
            // dc1 of q1 into the plane d2: dq/dh1 = w2 under h1's mask, times -1 / rows on the step's rows.  The masks of this
            // pass are h <= 0 ? 0 : acc, float64 autograd's own: a NaN activation hands its term on
            const int u = t & (kH - 1), rg = t >> 7;
            const float w2u = cr[FC::w2 + u];
            const f32x4 h = ld4(lds + L::c1 + u * kRP + 4 * rg);
            f32x4 dz;
#pragma unroll
            for (int r = 0; r < 4; ++r) dz[r] = (h[r] <= 0.0f || r0 + 4 * rg + r >= rows) ? 0.0f : __fmul_rn(w2u, ninv);
            st4(lds + L::d2 + u * kRP + 4 * rg, dz);
        }
        __syncthreads();
        {
            // dc0 into the plane d1: unit u's row of w1 is contiguous in memory (the policy's (in, out) layout), o ascending
            const int u = t & (kH - 1), rg = t >> 7;
            const float *w = cr + FC::w1 + u * kH, *d = lds + L::d2 + 4 * rg;
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int o = 0; o < kH; o += 4) {
                const f32x4 wv = ld4(w + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 dz = ld4(d + (o + i) * kRP);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(wv[i], dz[r], acc[r]);
                }
            }
            const f32x4 h = ld4(lds + L::c0 + u * kRP + 4 * rg);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = h[r] <= 0.0f ? 0.0f : acc[r];
            st4(lds + L::d1 + u * kRP + 4 * rg, acc);
        }
        __syncthreads();
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
    const int k = blockIdx.x;
    float *t = C.t[k], *w = C.ws + C.at[k];
    if (!t) return;
    for (int i = threadIdx.x; i < C.n[k]; i += kCopyBlock) {
        if (C.to_ws) w[i] = t[i];
        else t[i] = w[i];
    }
}

__global__ __launch_bounds__(kMathBlock) void k_sac_math(int which, const float *in, float *out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kMathBlock + threadIdx.x;
    if (i >= n) return;
    const float x = in[i];
    out[i] = which == 0 ? expf(x) : which == 1 ? qs::q_ln(x) : jac_ln(tanh_keep_nan(x));
}

}  // namespace qssac
