// trpo_kernels.hpp -- the kernels of libquadsim_trpo.so (include/quadsim_trpo.h has the numerical contract).  A fragment of
// trpo.hip, nowhere else.  Built from train_pieces.hpp: the chunk primitives and the tower pieces (the LDS image and its loader,
// the flat tower, backward_chunk, block_sum, the advantage statistics, the Gaussian head).  k_trpo_vf_fit keeps its own text of
// the loader and of the register-resident moments (train_pieces.hpp's load_image, load_moments, step_moments and store_state
// at a head one unit wide): written with those pieces it computes the same bits but spills 13 scalar registers where this text
// spills 9 (profiles/train_pieces/README.md).  A change to those pieces has to be made here as well.
//
// A policy step is a fixed sequence of launches, and the kernel boundary is the only ordering across workgroups:
//   k_trpo_prep      one workgroup: the advantage's mean and 1 / (std + 1e-8), theta flattened into the workspace, the flags.
//   k_trpo_grad      grid slices: the policy tower in LDS, the 16-row chunks of a slice: forward, head, backward_chunk;
//                    keeps the old means and neglogp, writes the slice's partial gradient and its sum of advantages.
//   k_trpo_reduce    grid over the P elements: the partials of an element in float64, slices ascending, rounded once; for a
//                    Fisher-vector product plus 2 v on logstd and the damping.
//   k_trpo_cg_init   one workgroup: r = p = g, x = 0, rdotr, the skip flag.
//   k_trpo_fvp       grid slices: the tower in LDS, the tangent vector STREAMED from memory with lanes along the units (a second
//                    padded image of 74.8 KB does not fit beside the tower and nine activation planes); per chunk of strided rows:
//                    forward, tangent forward, dmu, backward.
//   k_trpo_cg_iter   one workgroup: alpha, x, r, rdotr, mu, p and the convergence flag of one CG iteration.
//   k_trpo_step      one workgroup: shs, lm, fullstep, expected_improve.
//   k_trpo_ls_eval   grid slices: candidate k's tower in LDS, forward only: the slice's sums of the surrogate and the KL terms.
//   k_trpo_ls_decide one workgroup: the candidate's statistics, the test, and on acceptance theta_k into the policy's tensors.
// Flags are written by one-workgroup kernels only and read at the entry of LATER launches: iterations after convergence,
// candidates after acceptance and everything after a skip return at once.
// k_trpo_vf_fit: ONE workgroup runs every Adam step of the value fit, k_bc_fit's scheme with a plain head one unit wide, in its own text.
#pragma once
#include "train_pieces.hpp"

namespace qst {

using namespace qsf;

// theta, a partial gradient and every vector of the solver are flat towers (kW0 .. kLS, kP of train_pieces.hpp)
constexpr int kVecBlock = 256, kBlocks = (kP + kVecBlock - 1) / kVecBlock, kDotBatch = 8;
constexpr int kPolicySlots = 7;
constexpr int kFlagSkip = 0, kFlagCgDone = 1, kFlagAccepted = 2, kFlagIters = 3;
constexpr int kScRdotr = 0, kScSurrBefore = 1;

struct Ws {
    double *sc;                                  // [4]: rdotr, surr_before
    double *statp;                               // [slices][2]
    int32_t *flag;                               // [4]: skipped, CG converged, accepted k (-1), CG iterations run
    float *adv;                                  // mean, 1 / (std + 1e-8)
    float *theta, *g, *p, *r, *x, *z, *fs;       // [kP] each
    float *mu_old, *nlp_old;                     // [n,4], [n]
    float *part;                                 // [slices][kP]
};

struct Policy {
    float *w[kPolicySlots];                      // slots 0 .. 5 and 12
};

struct Rows {
    const float *obs, *act, *ret, *val;
    int n, slices, cps;                          // chunks per slice of the pass
};

struct Layout : TowerImage<> {
    static constexpr int act = planes;
    static constexpr int sc = act + kOut * kRP;  // per row: returns, values, old neglogp, and the row's terms of the statistics
    static constexpr int dl = sc + 6 * kRP;      // per row: the four terms of the logstd gradient (the line search: the old means)
    static constexpr int d2 = dl + kOut * kRP, d1 = d2 + kH * kRP;
    static constexpr int t0 = d1 + kH * kRP, t1 = t0 + kH * kRP;     // the tangents of the two hidden layers
    static constexpr int floats = t1 + kH * kRP;
};
static_assert(Layout::floats * 4 <= 160 * 1024, "LDS");

// element e of theta_old + fullstep 2^-k (fs == nullptr: of theta)
__device__ __forceinline__ float theta_at(const float *theta, const float *fs, float scale, int e)
{
    return fs ? __fadd_rn(theta[e], __fmul_rn(fs[e], scale)) : theta[e];
}

// the tower into LDS, and a barrier
__device__ __forceinline__ void load_tower(float *lds, const float *theta, const float *fs, float scale)
{
    load_image<Layout>(lds, Layout::floats, kOut, [&](int k, int i) { return theta_at(theta, fs, scale, slot_start(k) + i); });
    __syncthreads();
}

// the rows [begin, end) of slice g of a pass over `rows` rows
__device__ __forceinline__ bool slice_rows(int64_t rows, int cps, int g, int64_t *begin, int64_t *end)
{
    const int64_t chunks = (rows + kRows - 1) / kRows;
    const int64_t c0 = (int64_t)g * cps, c1 = min(c0 + cps, chunks);
    *begin = c0 * kRows;
    *end = min(c1 * kRows, rows);
    return c0 < c1;
}

// DOT of the header, by one workgroup of 256 threads, kDotBatch blocks of 256 elements per pass through LDS -> every thread
__device__ __forceinline__ double dot_blocks(const float *a, const float *b, double *p)
{
    const int t = threadIdx.x;
    double total = 0.0;
    for (int b0 = 0; b0 < kBlocks; b0 += kDotBatch) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kDotBatch; ++j) {
            const int e = (b0 + j) * kVecBlock + t;
            p[j * kVecBlock + t] = e < kP ? (double)a[e] * (double)b[e] : 0.0;
        }
        __syncthreads();
        for (int h = kVecBlock >> 1; h > 0; h >>= 1) {
            if (t < h) {
#pragma unroll
                for (int j = 0; j < kDotBatch; ++j) p[j * kVecBlock + t] += p[j * kVecBlock + t + h];
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < kDotBatch; ++j) total += p[j * kVecBlock];
    }
    return total;
}

// ---------------------------------------------------------------------------------------------------- the policy step
__global__ __launch_bounds__(kVecBlock) void k_trpo_prep(Policy Pol, Rows R, Ws W)
{
    __shared__ double p[kVecBlock];
    const int t = threadIdx.x;
    double mean, var;
    adv_moments<kVecBlock>(p, R.n, [&](int64_t i) { return __fsub_rn(R.ret[i], R.val[i]); }, &mean, &var);
    if (t == 0) {
        store_adv(W.adv, mean, var);
        W.flag[kFlagSkip] = 0;
        W.flag[kFlagCgDone] = 0;
        W.flag[kFlagAccepted] = -1;
        W.flag[kFlagIters] = 0;
    }
    for (int k = 0; k < kPolicySlots; ++k) {
        const int s0 = slot_start(k), s1 = slot_start(k + 1);
        for (int i = t; i < s1 - s0; i += kVecBlock) W.theta[s0 + i] = Pol.w[k][i];
    }
}

__global__ __launch_bounds__(kFitBlock) void k_trpo_grad(Rows R, Ws W, float inv_n, float entcoeff)
{
    using L = Layout;
    __shared__ __align__(16) float lds[L::floats];
    const int t = threadIdx.x, g = blockIdx.x;
    int64_t begin, end;
    float *part = W.part + (int64_t)g * kP;
    if (!slice_rows(R.n, R.cps, g, &begin, &end)) {      // an empty trailing slice: zeros
        for (int i = t; i < kP; i += kFitBlock) part[i] = 0.0f;
        if (t < 2) W.statp[2 * g + t] = 0.0;
        return;
    }
    load_tower(lds, W.theta, nullptr, 0.0f);
    float sig[kOut], cnl;
    double ent;
    head_consts(W.theta + kLS, sig, &cnl, &ent);
    const float amean = W.adv[0], arstd = W.adv[1];
    Acc G;
    zero_acc(G);
    float gls = (g == 0 && t >= kLsT && t < kLsT + kOut) ? entcoeff : 0.0f;
    double st0 = 0.0;                                    // thread kStatT: the slice's sum of advantages

    for (int64_t r0 = begin; r0 < end; r0 += kRows) {
        // -- gather: thread t < 256 holds (row t & 15, column t >> 4), columns 0 .. 11 of obs, then the 4 of actions; threads
        // 256 .. 271 the row's returns and values.  Rows past the end are zeros.  (Phase C of the chunk before still reads x)
        __syncthreads();
        if (t < (kIn + kOut + 1) * kRows) {
            const int r = t & (kRows - 1), c = t >> 4;
            const int64_t j = r0 + r;
            const bool in = j < end;
            if (c < kIn) lds[L::x + c * kRP + r] = in ? R.obs[j * kIn + c] : 0.0f;
            else if (c < kIn + kOut) lds[L::act + (c - kIn) * kRP + r] = in ? R.act[j * kOut + (c - kIn)] : 0.0f;
            else {
                lds[L::sc + 0 * kRP + r] = in ? R.ret[j] : 0.0f;
                lds[L::sc + 1 * kRP + r] = in ? R.val[j] : 0.0f;
            }
        }
        __syncthreads();
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        __syncthreads();
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
        __syncthreads();
        // -- the head, one row a thread: y becomes dmean, dl the row's terms of the logstd gradient, sc + 3 its advantage
        if (t < kRows) {
            const int r = t;
            const bool valid = r0 + r < end;
            const float A = __fmul_rn(__fsub_rn(__fsub_rn(lds[L::sc + r], lds[L::sc + kRP + r]), amean), arstd);
            const float dn = valid ? __fmul_rn(A, inv_n) : 0.0f;
            float q = 0.0f;
#pragma unroll
            for (int j = 0; j < kOut; ++j) {
                const float mu = lds[L::y + j * kRP + r];
                const float z = __fdiv_rn(__fsub_rn(lds[L::act + j * kRP + r], mu), sig[j]);
                q = __fmaf_rn(z, z, q);
                lds[L::y + j * kRP + r] = __fdiv_rn(__fmul_rn(dn, z), sig[j]);
                lds[L::dl + j * kRP + r] = __fmaf_rn(__fmul_rn(z, z), dn, -dn);
                if (valid) W.mu_old[(r0 + r) * kOut + j] = mu;
            }
            if (valid) W.nlp_old[r0 + r] = __fmaf_rn(0.5f, q, cnl);
            lds[L::sc + 3 * kRP + r] = valid ? A : 0.0f;
        }
        __syncthreads();
        if (t == kStatT) {
            for (int r = 0; r < kRows && r0 + r < end; ++r) st0 += (double)lds[L::sc + 3 * kRP + r];
        }
        if (t >= kLsT && t < kLsT + kOut) {
#pragma unroll
            for (int r = 0; r < kRows; ++r) gls = __fadd_rn(gls, lds[L::dl + (t - kLsT) * kRP + r]);
        }
        backward_chunk<L>(lds, G);
    }
    store_acc(part, G, gls);
    if (t == kStatT) {
        W.statp[2 * g] = st0;
        W.statp[2 * g + 1] = 0.0;
    }
}

struct ReduceArgs {
    const float *part, *v;                       // v: the vector of a Fisher-vector product, nullptr for the gradient
    float *out;
    float *tr_in, *tr_out;                       // nullable: the trace's rows of this product
    const int32_t *flag;
    float damping;
    int slices, until_converged;
};

__global__ __launch_bounds__(kVecBlock) void k_trpo_reduce(ReduceArgs F)
{
    if (F.v && (F.flag[kFlagSkip] || (F.until_converged && F.flag[kFlagCgDone]))) return;
    const int e = blockIdx.x * kVecBlock + threadIdx.x;
    if (e >= kP) return;
    double sum = 0.0;
    for (int g = 0; g < F.slices; ++g) sum += (double)F.part[(int64_t)g * kP + e];
    if (!F.v) {
        F.out[e] = (float)sum;
        return;
    }
    const float v = F.v[e];
    if (e >= kLS) sum += 2.0 * (double)v;
    const float z = __fmaf_rn(F.damping, v, (float)sum);
    F.out[e] = z;
    if (F.tr_in) { F.tr_in[e] = v; F.tr_out[e] = z; }
}

__global__ __launch_bounds__(kVecBlock) void k_trpo_cg_init(Ws W, int slices, double n, double entcoeff, float *stats, float *grad)
{
    __shared__ double p[kDotBatch * kVecBlock];
    const int t = threadIdx.x;
    const double rd = dot_blocks(W.g, W.g, p);
    for (int e = t; e < kP; e += kVecBlock) {
        const float g = W.g[e];
        W.r[e] = g;
        W.p[e] = g;
        W.x[e] = 0.0f;
        if (grad) grad[e] = g;
    }
    if (t == 0) {
        double s = 0.0, ent = 0.0;
        for (int g = 0; g < slices; ++g) s += W.statp[2 * g];
        for (int j = 0; j < kOut; ++j) ent += (double)W.theta[kLS + j];
        ent += 2.0 * kLog2PiE;
        const double sb = s / n + entcoeff * ent;
        const bool skip = rd == 0.0;
        W.sc[kScRdotr] = rd;
        W.sc[kScSurrBefore] = sb;
        W.flag[kFlagSkip] = skip;
        for (int i = 0; i < 10; ++i) stats[i] = 0.0f;
        stats[0] = (float)sb;
        stats[4] = (float)sqrt(rd);
        if (skip) {
            stats[1] = (float)sb;
            stats[3] = (float)ent;
            stats[8] = -2.0f;
        }
    }
}

__global__ __launch_bounds__(kFitBlock) void k_trpo_fvp(Rows R, Ws W, const float *v, int stride, float inv_nf, int until_converged)
{
    using L = Layout;
    __shared__ __align__(16) float lds[L::floats];
    if (W.flag[kFlagSkip] || (until_converged && W.flag[kFlagCgDone])) return;
    const int t = threadIdx.x, g = blockIdx.x;
    const int64_t nf = ((int64_t)R.n + stride - 1) / stride;
    int64_t begin, end;
    float *part = W.part + (int64_t)g * kP;
    if (!slice_rows(nf, R.cps, g, &begin, &end)) {
        for (int i = t; i < kP; i += kFitBlock) part[i] = 0.0f;
        return;
    }
    load_tower(lds, W.theta, nullptr, 0.0f);
    float s2[kOut];
#pragma unroll
    for (int j = 0; j < kOut; ++j) { const float s = expf(W.theta[kLS + j]); s2[j] = __fmul_rn(s, s); }
    Acc G;
    zero_acc(G);
    const int u = t & (kH - 1), rg = t >> 7;             // the tangents: unit u, rows 4 rg .. 4 rg + 3, lanes along the units

    for (int64_t r0 = begin; r0 < end; r0 += kRows) {
        __syncthreads();
        if (t < kIn * kRows) {
            const int r = t & (kRows - 1), c = t >> 4;
            const int64_t j = r0 + r;
            lds[L::x + c * kRP + r] = j < end ? R.obs[j * stride * kIn + c] : 0.0f;
        }
        __syncthreads();
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        {
            // t0 = mask0 (V0^T x + vb0): x is staged, a1 is being written by others -> the mask after the barrier
            const float b = v[kB0 + u];
            f32x4 acc = {b, b, b, b};
#pragma unroll
            for (int k = 0; k < kIn; ++k) {
                const float vk = v[kW0 + k * kH + u];
                const f32x4 xk = ld4(lds + L::x + k * kRP + 4 * rg);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(vk, xk[r], acc[r]);
            }
            __syncthreads();
            const f32x4 h = ld4(lds + L::a1 + u * kRP + 4 * rg);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = h[r] > 0.0f ? acc[r] : 0.0f;
            st4(lds + L::t0 + u * kRP + 4 * rg, acc);
        }
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        {
            // t1 = mask1 (V1^T h0 + vb1 + W1^T t0)
            const float b = v[kB1 + u];
            f32x4 acc = {b, b, b, b};
            const float *vp = v + kW1 + u;
#pragma unroll 4
            for (int k = 0; k < kH; ++k) {
                const float vk = vp[k * kH];
                const f32x4 hk = ld4(lds + L::a1 + k * kRP + 4 * rg);
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(vk, hk[r], acc[r]);
            }
            const float *w = lds + L::w2 + u * L::ld2;
            for (int k = 0; k < kH; k += 4) {
                const f32x4 wk = ld4(w + k);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 tk = ld4(lds + L::t0 + (k + i) * kRP + 4 * rg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = __fmaf_rn(wk[i], tk[r], acc[r]);
                }
            }
            const f32x4 h = ld4(lds + L::a2 + u * kRP + 4 * rg);
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = h[r] > 0.0f ? acc[r] : 0.0f;
            st4(lds + L::t1 + u * kRP + 4 * rg, acc);
        }
        __syncthreads();
        // -- the tangent of the mean, one (output, row) a thread, and dmu over y; rows past the end give zero
        if (t < kOut * kRows) {
            const int o = t & (kOut - 1), r = t >> 2;
            float acc = v[kB2 + o];
            for (int k = 0; k < kH; ++k) acc = __fmaf_rn(v[kW2 + k * kOut + o], lds[L::a2 + k * kRP + r], acc);
            for (int k = 0; k < kH; ++k) acc = __fmaf_rn(lds[L::w3 + o * L::ld3 + k], lds[L::t1 + k * kRP + r], acc);
            lds[L::y + o * kRP + r] = r0 + r < end ? __fmul_rn(__fdiv_rn(acc, s2[o]), inv_nf) : 0.0f;
        }
        __syncthreads();
        backward_chunk<L>(lds, G);
    }
    store_acc(part, G, 0.0f);
}

__global__ __launch_bounds__(kVecBlock) void k_trpo_cg_iter(Ws W, int k, double tol, double *cg)
{
    __shared__ double p[kDotBatch * kVecBlock];
    if (W.flag[kFlagSkip] || W.flag[kFlagCgDone]) return;
    const int t = threadIdx.x;
    const double rdotr = W.sc[kScRdotr];
    const double pz = dot_blocks(W.p, W.z, p);
    const float alpha = (float)(rdotr / pz);
    for (int e = t; e < kP; e += kVecBlock) {
        W.x[e] = __fmaf_rn(alpha, W.p[e], W.x[e]);
        W.r[e] = __fmaf_rn(-alpha, W.z[e], W.r[e]);
    }
    const double rd = dot_blocks(W.r, W.r, p);           // (its first barrier orders the stores above)
    const float mu = (float)(rd / rdotr);
    for (int e = t; e < kP; e += kVecBlock) W.p[e] = __fmaf_rn(mu, W.p[e], W.r[e]);
    if (t == 0) {
        W.sc[kScRdotr] = rd;
        W.flag[kFlagIters] = k + 1;
        if (rd < tol) W.flag[kFlagCgDone] = 1;
        if (cg) { cg[4 * k] = pz; cg[4 * k + 1] = (double)alpha; cg[4 * k + 2] = rd; cg[4 * k + 3] = (double)mu; }
    }
}

__global__ __launch_bounds__(kVecBlock) void k_trpo_step(Ws W, double max_kl, float *stats, float *tr_x, float *tr_fs)
{
    __shared__ double p[kDotBatch * kVecBlock];
    if (W.flag[kFlagSkip]) return;
    const int t = threadIdx.x;
    const double shs = 0.5 * dot_blocks(W.x, W.z, p);
    const float lm = (float)sqrt(shs / max_kl);
    for (int e = t; e < kP; e += kVecBlock) {
        const float x = W.x[e], fs = __fdiv_rn(x, lm);
        W.fs[e] = fs;
        if (tr_x) { tr_x[e] = x; tr_fs[e] = fs; }
    }
    const double ei = dot_blocks(W.g, W.fs, p);
    if (t == 0) {
        stats[5] = (float)shs;
        stats[6] = lm;
        stats[7] = (float)ei;
        stats[9] = (float)W.flag[kFlagIters];
    }
}

__global__ __launch_bounds__(kFitBlock) void k_trpo_ls_eval(Rows R, Ws W, float scale)
{
    using L = Layout;
    __shared__ __align__(16) float lds[L::floats];
    if (W.flag[kFlagSkip] || W.flag[kFlagAccepted] >= 0) return;
    const int t = threadIdx.x, g = blockIdx.x;
    int64_t begin, end;
    if (!slice_rows(R.n, R.cps, g, &begin, &end)) {
        if (t < 2) W.statp[2 * g + t] = 0.0;
        return;
    }
    load_tower(lds, W.theta, W.fs, scale);
    float lsk[kOut], sig[kOut], cnl, dls[kOut], so2[kOut], den[kOut];
    double ent;
#pragma unroll
    for (int j = 0; j < kOut; ++j) lsk[j] = theta_at(W.theta, W.fs, scale, kLS + j);
    head_consts(lsk, sig, &cnl, &ent);
#pragma unroll
    for (int j = 0; j < kOut; ++j) {
        const float lso = W.theta[kLS + j], so = expf(lso);
        dls[j] = __fsub_rn(lsk[j], lso);
        so2[j] = __fmul_rn(so, so);
        den[j] = __fmul_rn(2.0f, __fmul_rn(sig[j], sig[j]));
    }
    const float amean = W.adv[0], arstd = W.adv[1];
    double st0 = 0.0, st1 = 0.0;

    for (int64_t r0 = begin; r0 < end; r0 += kRows) {
        __syncthreads();
        if (t < (kIn + 2 * kOut + 1) * kRows) {
            const int r = t & (kRows - 1), c = t >> 4;
            const int64_t j = r0 + r;
            const bool in = j < end;
            if (c < kIn) lds[L::x + c * kRP + r] = in ? R.obs[j * kIn + c] : 0.0f;
            else if (c < kIn + kOut) lds[L::act + (c - kIn) * kRP + r] = in ? R.act[j * kOut + (c - kIn)] : 0.0f;
            else if (c < kIn + 2 * kOut) lds[L::dl + (c - kIn - kOut) * kRP + r] = in ? W.mu_old[j * kOut + (c - kIn - kOut)] : 0.0f;
            else {
                lds[L::sc + 0 * kRP + r] = in ? R.ret[j] : 0.0f;
                lds[L::sc + 1 * kRP + r] = in ? R.val[j] : 0.0f;
                lds[L::sc + 2 * kRP + r] = in ? W.nlp_old[j] : 0.0f;
            }
        }
        __syncthreads();
        forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
        __syncthreads();
        forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
        __syncthreads();
        forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
        __syncthreads();
        if (t < kRows) {
            const int r = t;
            const float A = __fmul_rn(__fsub_rn(__fsub_rn(lds[L::sc + r], lds[L::sc + kRP + r]), amean), arstd);
            float q = 0.0f, kl = 0.0f;
#pragma unroll
            for (int j = 0; j < kOut; ++j) {
                const float mu = lds[L::y + j * kRP + r];
                const float z = __fdiv_rn(__fsub_rn(lds[L::act + j * kRP + r], mu), sig[j]);
                q = __fmaf_rn(z, z, q);
                const float d = __fsub_rn(lds[L::dl + j * kRP + r], mu);
                const float tj = __fdiv_rn(__fmaf_rn(d, d, so2[j]), den[j]);
                kl = __fadd_rn(kl, __fsub_rn(__fadd_rn(dls[j], tj), 0.5f));
            }
            const float nl = __fmaf_rn(0.5f, q, cnl);
            lds[L::sc + 3 * kRP + r] = __fmul_rn(A, expf(__fsub_rn(lds[L::sc + 2 * kRP + r], nl)));
            lds[L::sc + 4 * kRP + r] = kl;
        }
        __syncthreads();
        if (t == kStatT) {
            for (int r = 0; r < kRows && r0 + r < end; ++r) {
                st0 += (double)lds[L::sc + 3 * kRP + r];
                st1 += (double)lds[L::sc + 4 * kRP + r];
            }
        }
    }
    if (t == kStatT) {
        W.statp[2 * g] = st0;
        W.statp[2 * g + 1] = st1;
    }
}

__global__ __launch_bounds__(kVecBlock) void k_trpo_ls_decide(Policy Pol, Ws W, int k, int last, float scale, int slices, double n,
                                                               double entcoeff, double max_kl, float *stats, float *ls)
{
    const bool over = W.flag[kFlagSkip] || W.flag[kFlagAccepted] >= 0;
    __syncthreads();                                     // (thread 0 writes the flag below: every wave has read it here)
    if (over) return;
    const int t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, ent = 0.0, ent_old = 0.0;
    for (int g = 0; g < slices; ++g) { s0 += W.statp[2 * g]; s1 += W.statp[2 * g + 1]; }
    for (int j = 0; j < kOut; ++j) {
        ent += (double)theta_at(W.theta, W.fs, scale, kLS + j);
        ent_old += (double)W.theta[kLS + j];
    }
    ent += 2.0 * kLog2PiE;
    ent_old += 2.0 * kLog2PiE;
    const double sb = W.sc[kScSurrBefore];
    const double surr = s0 / n + entcoeff * ent, kl = s1 / n;
    // (every comparison is false for a NaN; an infinite surrogate would pass the improvement test: isfinite)
    const bool ok = isfinite(surr) && isfinite(kl) && kl <= 1.5 * max_kl && surr - sb >= 0.0;
    if (ok) {
        for (int q = 0; q < kPolicySlots; ++q) {
            const int e0 = slot_start(q), e1 = slot_start(q + 1);
            for (int i = t; i < e1 - e0; i += kVecBlock) Pol.w[q][i] = theta_at(W.theta, W.fs, scale, e0 + i);
        }
    }
    if (t == 0) {
        if (ls) { ls[2 * k] = (float)surr; ls[2 * k + 1] = (float)kl; }
        if (ok) {
            W.flag[kFlagAccepted] = k;
            stats[1] = (float)surr;
            stats[2] = (float)kl;
            stats[3] = (float)ent;
            stats[8] = (float)k;
        } else if (last) {
            stats[1] = (float)sb;
            stats[2] = 0.0f;
            stats[3] = (float)ent_old;
            stats[8] = -1.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the value fit
struct VfArgs {
    float *w[6], *m[6], *v[6];                   // wv0 bv0 wv1 bv1 wv2 bv2 and their moments
    float *grads[6];                             // nullable as a whole (grads[0] == nullptr)
    const float *obs, *ret;
    const int32_t *indices;                      // [steps,batch]
    float *loss;                                 // [steps]
    double lr, beta1, beta2;
    float b1f, b2f, omb1, omb2, eps;
    int steps, batch, t0;
};

// k_bc_fit's step on the value tower: the head is the four-output head with three zero rows (they add exact zeros), the target
// plane `act` row 0 holds the returns; the owners of the elements that do not exist (w2 outputs 1 .. 3, b2 1 .. 3) keep zeros
__global__ __launch_bounds__(kFitBlock) void k_trpo_vf_fit(VfArgs F)
{
    using L = Layout;
    __shared__ __align__(16) float lds[L::t0 + 4];       // no tangents here; 4 scalars
    constexpr int scal = L::t0;
    const int t = threadIdx.x;
    for (int i = t; i < L::t0 + 4; i += kFitBlock) lds[i] = 0.0f;
    __syncthreads();
    for (int i = t; i < kIn * kH; i += kFitBlock) lds[L::w1 + (i & (kH - 1)) * L::ld1 + (i >> 7)] = F.w[0][i];
    for (int i = t; i < kH * kH; i += kFitBlock) lds[L::w2 + (i & (kH - 1)) * L::ld2 + (i >> 7)] = F.w[2][i];
    if (t < kH) { lds[L::w3 + t] = F.w[4][t]; lds[L::b1 + t] = F.w[1][t]; lds[L::b2 + t] = F.w[3][t]; }
    if (t == 0) lds[L::b3] = F.w[5][0];
    __syncthreads();

    const int ti = t & 31, to = t >> 5, o1 = t & 127, ig1 = t >> 7, o3 = t & 3, i3 = t >> 2;
    const bool own1 = ig1 < 3, own3 = o3 == 0;
    const int bk = t < 128 ? 0 : t < 256 ? 1 : t == 256 ? 2 : -1, bu = t & 127;
    const int bi = bk < 0 ? 0 : 2 * bk + 1, blds = bk == 0 ? L::b1 : bk == 1 ? L::b2 : L::b3;
    float m2[8][4], v2[8][4], m1[4] = {}, v1[4] = {}, m3 = 0.0f, v3 = 0.0f, mb = 0.0f, vb = 0.0f;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = (8 * to + a) * kH + ti + 32 * j;
            m2[a][j] = F.m[2][idx];
            v2[a][j] = F.v[2][idx];
        }
    if (own1) {
#pragma unroll
        for (int a = 0; a < 4; ++a) { m1[a] = F.m[0][(4 * ig1 + a) * kH + o1]; v1[a] = F.v[0][(4 * ig1 + a) * kH + o1]; }
    }
    if (own3) { m3 = F.m[4][i3]; v3 = F.v[4][i3]; }
    if (bk >= 0) { mb = F.m[bi][bu]; vb = F.v[bi][bu]; }
    Acc G;

    for (int it = 0; it < F.steps; ++it) {
        if (t == 0) {
            const double tt = (double)(F.t0 + it) + 1.0;
            lds[scal] = (float)(F.lr * sqrt(1.0 - pow(F.beta2, tt)) / (1.0 - pow(F.beta1, tt)));
        }
        const float dscale = (float)(2.0 / (double)F.batch);
        zero_acc(G);
        float lsum = 0.0f;                                // thread kStatT: the squared error of the rows so far
        for (int r0 = 0; r0 < F.batch; r0 += kRows) {
            __syncthreads();
            if (t < (kIn + 1) * kRows) {
                const int r = t & (kRows - 1), c = t >> 4, j = r0 + r;
                const int64_t idx = j < F.batch ? (int64_t)F.indices[(int64_t)it * F.batch + j] : -1;
                if (c < kIn) lds[L::x + c * kRP + r] = idx < 0 ? 0.0f : F.obs[idx * kIn + c];
                else lds[L::act + r] = idx < 0 ? 0.0f : F.ret[idx];
            }
            __syncthreads();
            forward_layer<true>(lds + L::w1, L::ld1, lds + L::b1, lds + L::x, kInP, kH, lds + L::a1);
            __syncthreads();
            forward_layer<true>(lds + L::w2, L::ld2, lds + L::b2, lds + L::a1, kH, kH, lds + L::a2);
            __syncthreads();
            forward_layer<false>(lds + L::w3, L::ld3, lds + L::b3, lds + L::a2, kH, kOut, lds + L::y);
            __syncthreads();
            // -- e = v - R over sc, dv = e dscale over y (rows 1 .. 3 of y are exact zeros); rows past the batch give zero
            if (t < kOut * kRows) {
                const int r = t & (kRows - 1), o = t >> 4;
                const float e = (o == 0 && r0 + r < F.batch) ? __fsub_rn(lds[L::y + r], lds[L::act + r]) : 0.0f;
                if (o == 0) lds[L::sc + r] = e;
                lds[L::y + o * kRP + r] = __fmul_rn(e, dscale);
            }
            __syncthreads();
            if (t == kStatT) {
                for (int r = 0; r < kRows && r0 + r < F.batch; ++r) { const float e = lds[L::sc + r]; lsum = __fadd_rn(lsum, __fmul_rn(e, e)); }
            }
            backward_chunk<L>(lds, G);
        }
        // ---- Adam on the thread's own elements: m and v in registers, the weight in LDS
        __syncthreads();
        const Adam A{F.b1f, F.b2f, F.omb1, F.omb2, F.eps, lds[scal]};
        float sink;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                adam_step(A, G.g2[a][j], lds + L::w2 + (ti + 32 * j) * L::ld2 + 8 * to + a, &sink, &m2[a][j], &v2[a][j], nullptr, 0);
        if (own1) {
#pragma unroll
            for (int a = 0; a < 4; ++a) adam_step(A, G.g1[a], lds + L::w1 + o1 * L::ld1 + 4 * ig1 + a, &sink, &m1[a], &v1[a], nullptr, 0);
        }
        if (own3) adam_step(A, G.g3, lds + L::w3 + i3, &sink, &m3, &v3, nullptr, 0);
        if (bk >= 0) adam_step(A, G.gb, lds + blds + bu, &sink, &mb, &vb, nullptr, 0);
        if (t == kStatT) F.loss[it] = __fdiv_rn(lsum, (float)F.batch);
        __syncthreads();
    }

    // ---- the state back to memory: every thread its own elements
    const bool grads = F.grads[0] != nullptr;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = (8 * to + a) * kH + ti + 32 * j;
            F.w[2][idx] = lds[L::w2 + (ti + 32 * j) * L::ld2 + 8 * to + a];
            F.m[2][idx] = m2[a][j];
            F.v[2][idx] = v2[a][j];
            if (grads) F.grads[2][idx] = G.g2[a][j];
        }
    if (own1) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int idx = (4 * ig1 + a) * kH + o1;
            F.w[0][idx] = lds[L::w1 + o1 * L::ld1 + 4 * ig1 + a];
            F.m[0][idx] = m1[a];
            F.v[0][idx] = v1[a];
            if (grads) F.grads[0][idx] = G.g1[a];
        }
    }
    if (own3) {
        F.w[4][i3] = lds[L::w3 + i3];
        F.m[4][i3] = m3;
        F.v[4][i3] = v3;
        if (grads) F.grads[4][i3] = G.g3;
    }
    if (bk >= 0) {
        F.w[bi][bu] = lds[blds + bu];
        F.m[bi][bu] = mb;
        F.v[bi][bu] = vb;
        if (grads) F.grads[bi][bu] = G.gb;
    }
}

}  // namespace qst
