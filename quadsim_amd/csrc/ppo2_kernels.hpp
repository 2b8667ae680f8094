// ppo2_kernels.hpp -- the kernels of libquadsim_ppo.so (include/quadsim_ppo.h has the numerical contract).  A fragment of
// ppo2.hip, nowhere else.  From train_pieces.hpp: the chunk primitives, the tower's dimensions and LDS image, the flat tower,
// block_sum and the advantage statistics.  k_ppo_grad keeps its own text of the loader, the head constants, the element map and
// the three phases of the backward pass (train_pieces.hpp's load_image, head_consts, for_own and backward_chunk, line for line):
// written with those pieces it computes the same bits, but the compiler assigns the chunk loop other registers and the kernel
// measured 1 .. 2 % slower wherever that loop is all there is (profiles/train_pieces/README.md).  A change to a piece has to be
// made here as well.
//
// One Adam step is three launches, and the kernel boundary is the only ordering across workgroups:
//   k_ppo_grad   grid (slices, 2): workgroup (g, b) holds branch b (0 policy, 1 value) of the net in LDS -- 12 -> 128 -> 128 ->
//                {4 | 1}, the image of k_bc_fit -- and walks the 16-row chunks of slice g of the step's index row: gather,
//                forward, head, backward; every thread accumulates its fixed gradient elements in registers, rows ascending,
//                and writes them once, as float32, to the workspace with the slice's float64 sums of the statistics.
//   k_ppo_reduce grid over the parameter elements: the partials of an element in float64, slices ascending, rounded once; a
//                float64 sum of squares per workgroup.
//   k_ppo_apply  grid over the parameter elements: the global norm, tf.clip_by_global_norm's scale, Adam in place; workgroup 0
//                finishes the step's six statistics.
// k_ppo_adv_stats runs once per call: one workgroup per step, the mean and 1 / (std + 1e-8) of returns - values.
// The value head is run as four outputs of which three have zero weights and a zero dv: they add exact zeros.
#pragma once
#include "train_pieces.hpp"

namespace qsp {

using namespace qsf;

constexpr int kTensors = 13, kElemBlock = 256, kAdvBlock = 256;
// a branch's partial gradient is the flat tower of train_pieces.hpp (the value head at stride 4)
constexpr int kLW0 = kW0, kLB0 = kB0, kLW1 = kW1, kLB1 = kB1, kLW2 = kW2, kLB2 = kB2, kLLS = kLS, kPart = kP;

struct GradArgs {
    const float *w[2][6];                        // the six tensors of either branch
    const float *logstd;
    const float *obs, *act, *ret, *val, *nlp;
    const int32_t *indices;                      // the step's row [batch]
    const float *adv;                            // the step's (mean, 1 / (std + 1e-8))
    float *part;                                 // [2][slices][kPart]
    double *statp;                               // [slices][2][4]
    float lo, hi, clip, crv, inv_batch, vf_scale, neg_ent;
    int batch, cps, slices, use_crv;
};

struct ParamTable {
    float *w[kTensors], *m[kTensors], *v[kTensors], *grads[kTensors];
    int start[kTensors + 1];                     // the slot's first element of the flat parameter vector
    int loc[2][kTensors];                        // the slot's place in a branch's partial, -1: the branch has none
    int stride[kTensors];
};

struct ApplyArgs {
    const float *gflat;
    const double *ssq, *statp;
    float *stats;                                // the step's six
    double max_grad_norm, batch;
    float b1f, b2f, omb1, omb2, eps, lr_t;
    int total, nblk, slices, want_grads;
};

struct Layout : TowerImage<> {
    static constexpr int act = planes;
    static constexpr int sc = act + kOut * kRP;  // per row: returns, values, old neglogp, and the three terms of the statistics
    static constexpr int dl = sc + 6 * kRP;      // per row: the four terms of the logstd gradient
    static constexpr int d2 = dl + kOut * kRP, d1 = d2 + kH * kRP;
    static constexpr int floats = d1 + kH * kRP;
};

__global__ __launch_bounds__(kFitBlock) void k_ppo_grad(GradArgs F)
{
    using L = Layout;
    static_assert(L::floats * 4 <= 160 * 1024, "LDS");
    __shared__ __align__(16) float lds[L::floats];
    const int t = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
    const int64_t chunks = ((int64_t)F.batch + kRows - 1) / kRows;
    const int64_t c0 = (int64_t)g * F.cps, c1 = min(c0 + F.cps, chunks);
    const int64_t begin = c0 * kRows, end = min(c1 * kRows, (int64_t)F.batch);
    float *part = F.part + ((int64_t)b * F.slices + g) * kPart;
    double *statp = F.statp + ((int64_t)g * 2 + b) * 4;
    if (c0 >= c1) {                              // an empty trailing slice: zeros
        for (int i = t; i < kPart; i += kFitBlock) part[i] = 0.0f;
        if (t < 4) statp[t] = 0.0;
        return;
    }

    // ---- the branch into LDS: zero everything (the padding stays zero), then the weights, transposed
    const float *const *w = F.w[b];
    const int outs = b ? 1 : kOut;
    for (int i = t; i < L::floats; i += kFitBlock) lds[i] = 0.0f;
    __syncthreads();
    for (int i = t; i < kIn * kH; i += kFitBlock) lds[L::w1 + (i & (kH - 1)) * L::ld1 + (i >> 7)] = w[0][i];
    for (int i = t; i < kH * kH; i += kFitBlock) lds[L::w2 + (i & (kH - 1)) * L::ld2 + (i >> 7)] = w[2][i];
    for (int i = t; i < kH * outs; i += kFitBlock) lds[L::w3 + (i % outs) * L::ld3 + i / outs] = w[4][i];
    if (t < kH) { lds[L::b1 + t] = w[1][t]; lds[L::b2 + t] = w[3][t]; }
    if (t < outs) lds[L::b3 + t] = w[5][t];

    float sig[kOut], cnl, ent;
    {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < kOut; ++j) { const float ls = F.logstd[j]; sig[j] = expf(ls); s += (double)ls; }
        cnl = (float)(2.0 * kLog2Pi + s);                  // 2 log(2 pi) + sum logstd
        ent = (float)(s + 2.0 * kLog2PiE);                  // sum logstd + 2 log(2 pi e)
    }
    const float amean = F.adv[0], arstd = F.adv[1];

    // ---- the elements of this thread, in the policy's (in, out) layout (k_bc_fit's map)
    const int ti = t & 31, to = t >> 5;                  // w_l1: inputs 8 to + a, outputs ti + 32 j
    const int o1 = t & 127, ig1 = t >> 7;                // w_l0: output o1, inputs 4 ig1 + a (ig1 == 3: the zero padding)
    const int o3 = t & 3, i3 = t >> 2;                   // w_l2: input i3, output o3
    const bool own1 = ig1 < 3;
    const int bk = t < 128 ? 0 : t < 256 ? 1 : t < 260 ? 2 : -1, bu = t & 127;
    float g2[8][4], g1[4] = {}, g3 = 0.0f, gb = 0.0f, gls = 0.0f;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) g2[a][j] = 0.0f;
    if (b == 0 && g == 0 && t >= kLsT && t < kLsT + kOut) gls = F.neg_ent;
    double st0 = 0.0, st1 = 0.0, st2 = 0.0;              // thread kStatT: the slice's sums

    for (int64_t r0 = begin; r0 < end; r0 += kRows) {
        // -- gather: thread t < 256 holds (row t & 15, column t >> 4), columns 0 .. 11 of obs, then the 4 of actions; threads
        // 256 .. 271 the row's returns, values and old neglogp.  Rows past the end are zeros.  (Phase C of the chunk before
        // still reads x: the barrier)
        __syncthreads();
        if (t < (kIn + kOut + 1) * kRows) {
            const int r = t & (kRows - 1), c = t >> 4;
            const int64_t j = r0 + r;
            const int64_t idx = j < end ? (int64_t)F.indices[j] : -1;
            if (c < kIn) lds[L::x + c * kRP + r] = idx < 0 ? 0.0f : F.obs[idx * kIn + c];
            else if (c < kIn + kOut) { if (b == 0) lds[L::act + (c - kIn) * kRP + r] = idx < 0 ? 0.0f : F.act[idx * kOut + (c - kIn)]; }
            else {
                lds[L::sc + 0 * kRP + r] = idx < 0 ? 0.0f : F.ret[idx];
                lds[L::sc + 1 * kRP + r] = idx < 0 ? 0.0f : F.val[idx];
                lds[L::sc + 2 * kRP + r] = idx < 0 ? 0.0f : F.nlp[idx];
            }
        }
        __syncthreads();
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        __syncthreads();
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
        __syncthreads();
        // -- the head, one row a thread: y becomes dmean (dv, 0, 0, 0), sc + 3 .. 5 the row's terms of the statistics
        if (t < kRows) {
            const int r = t;
            const bool valid = r0 + r < end;
            const float ret = lds[L::sc + r], val = lds[L::sc + kRP + r];
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
            if (b == 0) {
                const float A = __fmul_rn(__fsub_rn(__fsub_rn(ret, val), amean), arstd);
                float z[kOut], q = 0.0f;
#pragma unroll
                for (int j = 0; j < kOut; ++j) {
                    z[j] = __fdiv_rn(__fsub_rn(lds[L::act + j * kRP + r], lds[L::y + j * kRP + r]), sig[j]);
                    q = __fmaf_rn(z[j], z[j], q);
                }
                const float nl = __fmaf_rn(0.5f, q, cnl), dnl = __fsub_rn(nl, lds[L::sc + 2 * kRP + r]);
                const float ratio = expf(-dnl);
                // (selects that keep a NaN, as torch.clamp and torch.maximum do: fminf(fmaxf()) would clip a NaN ratio to lo, and
                // p1 >= p2 would then report the finite p2 with a zero gradient.  rc is NaN only where ratio is, so p2 is NaN
                // only where p1 is, and "not p1 < p2" takes p1 exactly where either is NaN)
                const float rc = ratio < F.lo ? F.lo : ratio > F.hi ? F.hi : ratio;
                const float p1 = -__fmul_rn(A, ratio), p2 = -__fmul_rn(A, rc);
                const bool first = !(p1 < p2);
                const bool active = valid && first;
                // (a clipped-off row's zero is 0 * ratio, as the chain rule through exp has it: +0 unless the ratio is infinite)
                const float dn = active ? __fmul_rn(__fmul_rn(A, ratio), F.inv_batch) : valid ? __fmul_rn(0.0f, ratio) : 0.0f;
#pragma unroll
                for (int j = 0; j < kOut; ++j) {
                    lds[L::y + j * kRP + r] = -__fdiv_rn(__fmul_rn(dn, z[j]), sig[j]);
                    lds[L::dl + j * kRP + r] = __fmaf_rn(-__fmul_rn(z[j], z[j]), dn, dn);
                }
                if (valid) {
                    s0 = first ? p1 : p2;
                    s1 = __fmul_rn(0.5f, __fmul_rn(dnl, dnl));
                    s2 = fabsf(__fsub_rn(ratio, 1.0f)) > F.clip ? 1.0f : 0.0f;
                }
            } else {
                const float v = lds[L::y + r];
                const float dv = __fsub_rn(v, val);
                // (a value inside the range is v itself, not val + (v - val): an unclipped row ties exactly and stays active)
                // (a NaN step v - val is no value inside the range: the clipped value is NaN, as val + clamp(v - val) is)
                const float vc = !F.use_crv ? v : dv > F.crv ? __fadd_rn(val, F.crv) : dv < -F.crv ? __fsub_rn(val, F.crv) : dv != dv ? dv : v;
                const float e1 = __fsub_rn(v, ret), e2 = __fsub_rn(vc, ret);
                const float l1 = __fmul_rn(e1, e1), l2 = __fmul_rn(e2, e2);
                // (the larger loss, NaN where either is: l1 unless l1 < l2 or l2 alone is NaN)
                const bool first = !(l1 < l2), take1 = first && l2 == l2;
                const bool active = valid && first;
                lds[L::y + r] = active ? __fmul_rn(e1, F.vf_scale) : 0.0f;
#pragma unroll
                for (int j = 1; j < kOut; ++j) lds[L::y + j * kRP + r] = 0.0f;
                if (valid) s0 = __fmul_rn(0.5f, take1 ? l1 : l2);
            }
            lds[L::sc + 3 * kRP + r] = s0;
            lds[L::sc + 4 * kRP + r] = s1;
            lds[L::sc + 5 * kRP + r] = s2;
        }
        __syncthreads();
        // -- phase A: the statistics, the gradient of the head from (dy, a1), dz1 from (w_l2, dy) under a1's mask
        if (t == kStatT) {
            for (int r = 0; r < kRows && r0 + r < end; ++r) {
                st0 += (double)lds[L::sc + 3 * kRP + r];
                st1 += (double)lds[L::sc + 4 * kRP + r];
                st2 += (double)lds[L::sc + 5 * kRP + r];
            }
        }
        if (b == 0 && t >= kLsT && t < kLsT + kOut) {
#pragma unroll
            for (int r = 0; r < kRows; ++r) gls = __fadd_rn(gls, lds[L::dl + (t - kLsT) * kRP + r]);
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
        // -- phase B: the gradient of layer 1 from (dz1, a0), dz0 from (w_l1, dz1) under a0's mask
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

    // ---- the slice's partial: every thread its own elements
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[kLW1 + (8 * to + a) * kH + ti + 32 * j] = g2[a][j];
    if (own1) {
#pragma unroll
        for (int a = 0; a < 4; ++a) part[kLW0 + (4 * ig1 + a) * kH + o1] = g1[a];
    }
    part[kLW2 + t] = g3;
    if (bk >= 0) part[(bk == 0 ? kLB0 : bk == 1 ? kLB1 : kLB2) + bu] = gb;
    if (t >= kLsT && t < kLsT + kOut) part[kLLS + t - kLsT] = gls;
    if (t == kStatT) {
        statp[0] = st0;
        statp[1] = st1;
        statp[2] = st2;
        statp[3] = (double)ent;
    }
}

// one workgroup per step: float32(mean) and float32(1 / (std + 1e-8)) of d = returns - values over the step's rows
__global__ __launch_bounds__(kAdvBlock) void k_ppo_adv_stats(const float *ret, const float *val, const int32_t *indices, int batch, float *adv)
{
    __shared__ double p[kAdvBlock];
    const int32_t *row = indices + (int64_t)blockIdx.x * batch;
    double mean, var;
    adv_moments<kAdvBlock>(p, batch, [&](int64_t i) { const int64_t idx = row[i]; return __fsub_rn(ret[idx], val[idx]); }, &mean, &var);
    if (threadIdx.x == 0) store_adv(adv + 2 * blockIdx.x, mean, var);
}

__device__ __forceinline__ int slot_of(const ParamTable &T, int e)
{
    int k = 0;
#pragma unroll
    for (int i = 1; i < kTensors; ++i) k = e >= T.start[i] ? i : k;
    return k;
}

__global__ __launch_bounds__(kElemBlock) void k_ppo_reduce(ParamTable T, const float *part, int slices, int total, float *gflat, double *ssq)
{
    __shared__ double p[kElemBlock];
    const int e = blockIdx.x * kElemBlock + threadIdx.x;
    double sq = 0.0;
    if (e < total) {
        const int k = slot_of(T, e), j = (e - T.start[k]) * T.stride[k];
        double sum = 0.0;
        for (int b = 0; b < 2; ++b) {
            if (T.loc[b][k] < 0) continue;
            const float *src = part + (int64_t)b * slices * kPart + T.loc[b][k] + j;
            for (int g = 0; g < slices; ++g) sum += (double)src[(int64_t)g * kPart];
        }
        const float G = (float)sum;
        gflat[e] = G;
        sq = (double)G * (double)G;
    }
    sq = block_sum<kElemBlock>(p, sq);
    if (threadIdx.x == 0) ssq[blockIdx.x] = sq;
}

__global__ __launch_bounds__(kElemBlock) void k_ppo_apply(ParamTable T, ApplyArgs F)
{
    const int e = blockIdx.x * kElemBlock + threadIdx.x;
    double sum = 0.0;
    for (int i = 0; i < F.nblk; ++i) sum += F.ssq[i];
    const double norm = sqrt(sum);
    if (e < F.total) {
        const int k = slot_of(T, e), j = e - T.start[k];
        float g = F.gflat[e];
        if (F.want_grads) T.grads[k][j] = g;
        // (a select, not fmax: a NaN norm scales every element to NaN, as tf.clip_by_global_norm does)
        if (F.max_grad_norm > 0.0) g = __fmul_rn(g, (float)(F.max_grad_norm / (norm < F.max_grad_norm ? F.max_grad_norm : norm)));
        const Adam A{F.b1f, F.b2f, F.omb1, F.omb2, F.eps, F.lr_t};
        float wl = T.w[k][j];
        adam_step(A, g, &wl, T.w[k], T.m[k], T.v[k], nullptr, j);
    }
    if (e == 0) {
        double s[4] = {};
        for (int g = 0; g < F.slices; ++g) {
            const double *q = F.statp + (int64_t)g * 8;
            s[0] += q[0]; s[1] += q[1]; s[2] += q[2]; s[3] += q[4];
        }
        F.stats[0] = (float)(s[0] / F.batch);
        F.stats[1] = (float)(s[3] / F.batch);
        F.stats[2] = (float)F.statp[3];
        F.stats[3] = (float)(s[1] / F.batch);
        F.stats[4] = (float)(s[2] / F.batch);
        F.stats[5] = (float)norm;
    }
}

}  // namespace qsp
