// train_offpolicy.hpp -- what the kernels of the three off-policy trainers share (ddpg_kernels.hpp, td3_kernels.hpp, sac_kernels.hpp,
// and nothing else): the flat layout of a net in a workspace, the copy table and the body of the copy kernel, the small selects of
// a TD target, the noise load, the shared parts of a critic's chunk, the backward pass through a streamed critic and the
// Adam-and-Polyak tail.  Built on train_pieces.hpp.  Every piece is written so that it inlines to what the kernels held as their
// own text: the arithmetic in the explicit __f*_rn forms, in the same order.  Where a piece called from a kernel compiled to other
// code than the kernel's own text had, that kernel keeps the text and says so (profiles/offpolicy_pieces/README.md has the list):
// a change to such a piece has to be made there too.  What differs between the trainers on purpose stays with them: the actor's
// masks (DDPG h > 0 ? acc : 0, TD3 and SAC h <= 0 ? 0 : acc, which differ on NaN), dscale, who writes noise_out, the index-load
// thresholds and the way a net's current place is kept.
#pragma once
#include "train_pieces.hpp"

namespace qsf {

constexpr int kAct = 4, kCIn = kIn + kAct;       // the actions; a critic's input where the action enters at layer 0
constexpr int kCopyBlock = 256;
static_assert(kCIn == kInP, "a critic's layer 0 fills the tower image's sixteen input rows");

// a net as it lies flat in the workspace, tensors in the ABI's order and the policy's (in, out) layout: K0 inputs on layer 0, K1
// on layer 1 (a critic's action rows are on the one or on the other), OUTS outputs
template <int K0, int K1, int OUTS>
struct FlatNet {
    static constexpr int k0 = K0, k1 = K1, outs = OUTS;
    static constexpr int w0 = 0, b0 = w0 + k0 * kH, w1 = b0 + kH, b1 = w1 + k1 * kH, w2 = b1 + kH, b2 = w2 + kH * outs;
    static constexpr int floats = (b2 + outs + 3) & ~3;
    static constexpr int at(int k) { return k == 0 ? w0 : k == 1 ? b0 : k == 2 ? w1 : k == 3 ? b1 : k == 4 ? w2 : b2; }   // slot k's start
    static constexpr int elems(int k) { return k == 0 ? k0 * kH : k == 2 ? k1 * kH : k == 4 ? kH * outs : k == 5 ? outs : kH; }
};

// the tensors of a call and where each lies in the workspace.  A library's CopyArgs derives from it (a struct of its own
// namespace, so that its copy kernel keeps its name)
template <int N>
struct CopyTable {
    float *t[N];
    int at[N], n[N];
    float *ws;
    int to_ws;
};

// the body of a copy kernel: one workgroup per tensor
template <class Table>
__device__ __forceinline__ void copy_tensor(const Table &C)
{
    const int k = blockIdx.x;
    float *t = C.t[k], *w = C.ws + C.at[k];
    if (!t) return;
    for (int i = threadIdx.x; i < C.n[k]; i += kCopyBlock) {
        if (C.to_ws) w[i] = t[i];
        else t[i] = w[i];
    }
}

// (a select, not fminf(fmaxf()): those would drop a NaN; an infinity is clamped as any other value)
__device__ __forceinline__ float clampsel(float v, float lo, float hi) { return v < lo ? lo : v > hi ? hi : v; }

// y of a row: the reward alone behind an episode's end
__device__ __forceinline__ float td_target(float rew, float done, float gamma, float v)
{
    return done >= 1.0f ? rew : __fmaf_rn(__fmul_rn(__fsub_rn(1.0f, done), gamma), v, rew);
}

// the smaller of the twin values; a NaN in either is handed on
__device__ __forceinline__ float twin_min(float qa, float qb) { return qa != qa ? qa : qb != qb ? qb : (qb < qa ? qb : qa); }

// the rows of the step: its count, where the caller gave counts, and the batch at the most
template <class Args>
__device__ __forceinline__ int step_rows(const Args &S)
{
    const int rows = S.counts ? S.counts[0] : S.batch;
    return rows < S.batch ? rows : S.batch;
}

// the four normals of row slot `slot` into the planes zn: the caller's, or Philox block u of subsequence (STREAM << 48) | slot; the
// one branch of a trainer that is asked to (write_out) hands them to noise_out
template <uint64_t STREAM, class Args>
__device__ __forceinline__ void load_noise(float *zn, const Args &S, int slot, int gr, bool valid, bool write_out)
{
    float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        if (S.noise) {
#pragma unroll
            for (int c = 0; c < kAct; ++c) z[c] = S.noise[(int64_t)slot * kAct + c];
        } else {
            qs::normals_from_words(qs::philox_counter(S.seed, (STREAM << 48) | (uint64_t)slot, S.u), z);
        }
        if (S.noise_out && write_out) {
#pragma unroll
            for (int c = 0; c < kAct; ++c) S.noise_out[(int64_t)slot * kAct + c] = z[c];
        }
    }
#pragma unroll
    for (int c = 0; c < kAct; ++c) zn[c * kRP + gr] = z[c];
}

// a critic chunk's replay gather by thread (row gr, column gc) for replay row idx (-1: none): obs1 into the plane x, reward and
// done into the first two rows of sc -> the thread's value of (obs0 | act), which goes into the planes once y is there
template <class L, class Args>
__device__ __forceinline__ float gather_critic(float *lds, const Args &S, int idx, int gr, int gc)
{
    float pre = 0.0f;
    if (gc < kIn) {
        lds[L::x + gc * kRP + gr] = idx < 0 ? 0.0f : S.obs1[(int64_t)idx * kIn + gc];
        pre = idx < 0 ? 0.0f : S.obs0[(int64_t)idx * kIn + gc];
    } else if (gc < kCIn) {
        pre = idx < 0 ? 0.0f : S.act[(int64_t)idx * kAct + (gc - kIn)];
    } else if (gc == kCIn) {
        lds[L::sc + gr] = idx < 0 ? 0.0f : S.rew[idx];
        lds[L::sc + kRP + gr] = idx < 0 ? 1.0f : S.done[idx];
    }
    return pre;
}

// the critic in LDS on the planes (K1 inputs on layer 1), then per row of sc: q - y in row 4 (and q in row 3 where KEEP_Q), and
// dq = (q - y) dscale over y's first row.  Ends behind its barrier
template <class L, int K1, bool KEEP_Q>
__device__ __forceinline__ void critic_forward_dq(float *lds, int r0, int rows, float dscale)
{
    const int t = threadIdx.x;
    forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
    __syncthreads();
    forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, K1, kH, lds + L::a2);
    __syncthreads();
    forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
    __syncthreads();
    if (t < kRows) {
        const bool valid = r0 + t < rows;
        const float q = lds[L::y + t], d = valid ? __fsub_rn(q, lds[L::sc + 2 * kRP + t]) : 0.0f;
        if (KEEP_Q) lds[L::sc + 3 * kRP + t] = q;
        lds[L::sc + 4 * kRP + t] = d;
        lds[L::y + t] = __fmul_rn(d, dscale);
    }
    __syncthreads();
}

// thread kStatT: the chunk's rows onto the sums of (q - y)^2, q (where KEEP_Q) and y
template <class L, bool KEEP_Q>
__device__ __forceinline__ void critic_sums(const float *lds, int r0, int rows, float &s0, float &s1, float &s2)
{
    if (threadIdx.x == kStatT) {
        for (int r = 0; r < kRows && r0 + r < rows; ++r) {
            const float d = lds[L::sc + 4 * kRP + r];
            s0 = __fmaf_rn(d, d, s0);
            if (KEEP_Q) s1 = __fadd_rn(s1, lds[L::sc + 3 * kRP + r]);
            s2 = __fadd_rn(s2, lds[L::sc + 2 * kRP + r]);
        }
    }
}

// dq/da of a streamed critic `cr` (layout FC, the action on layer 0) whose hidden planes of this chunk lie in c1 and c0: back through
// its layers 2 and 1 into the plane d1, from where a thread takes da over the action rows of w0.  Ends behind its barrier
template <class L, class FC>
__device__ __forceinline__ void backward_streamed(float *lds, const float *cr, int r0, int rows, float ninv)
{
    const int t = threadIdx.x;
    {
        // dc1 of q1 into the plane d2: dq/dh1 = w2 under h1's mask, times -1 / rows on the step's rows.  The masks of this
        // pass are h <= 0 ? 0 : acc, float64 autograd's own: a NaN activation hands its term on, so that an actor behind a
        // diverged q1 diverges as the arbiter's does (h > 0 ? acc : 0 would feed it zeros)
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
}

// where a branch's Adam step finds its net: the weight's next place, its moments, its gradient's place (or null), and its target's place
// now and next
struct StepPlaces {
    float *wn, *m, *v, *gout;
    const float *tc;
    float *tn;
};

// Adam on the thread's own elements (m and v through memory, the weight from LDS into the net's next place), then, where the
// target moves, the target's average with the new weight.  No thread reads another's element here.  ACTION_ROWS: the four action
// rows of a critic's w0, which the owners of layer 0's padding in the tower's map hold in g1.  more(apply): the elements a branch
// holds beside the tower's map
template <class L, class F, bool ACTION_ROWS, class More>
__device__ __forceinline__ void apply_step(float *lds, const Adam &A, const StepPlaces &P, float tau, float omt, bool polyak, const Acc &G,
                                           More more)
{
    const int t = threadIdx.x;
    auto apply = [&](float g, float *lw, int e) {
        adam_step(A, g, lw, P.wn, P.m, P.v, P.gout, e);
        if (polyak) P.tn[e] = __fmaf_rn(tau, *lw, __fmul_rn(omt, P.tc[e]));
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

}  // namespace qsf
