// dynplan_image.hpp -- the padded weight image of a dynamics net (16 -> h1 -> h2 -> 12, ReLU) as the planner kernels of
// dynplan_kernels.hpp read it from LDS, and the kernel that packs it.  A fragment of dynplan.hip, nowhere else.
//
// Orientation as in mlp.hpp: every layer is computed transposed, H^T[unit][candidate] = W^T[unit][k] . X^T[k][candidate], the
// weights as the A operand of v_mfma_f32_16x16x4_f32 and the activations as the B operand, so that an accumulator tile (register
// i of lane l = row 4 (l >> 4) + i of column l & 15) IS the next layer's B operand: k-step i of tile t then sums the rows
// {16 t + 4 g + i : g = 0..3}.  mlp.hpp lets that order stand; here the contract is "k ascending", so the image stores unit
// u = 16 t + 4 i + g at row  pi(u) = 16 t + 4 g + i  (a 4 x 4 transpose inside every block of 16, its own inverse): k-step i of
// tile t sums the units 16 t + 4 i + {0, 1, 2, 3} -- ascending, and the zero padding comes last.  The same pi orders the 16
// inputs (a lane holds x[4 i + g] in register i: three observation words and one action component) and the 12 + 4 outputs, so
// the layer-3 accumulator is the next step's observation in place.  Rows are 16 T + 4 floats apart: one ds_read_b128 per lane
// fetches the A operands of four k-steps, and 4 (4 T + 1) words with 4 T + 1 odd puts the 16 rows of a tile on 16 different
// bank quads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qsd {

constexpr uint32_t kMagic = 0x314e5944u;            // "DYN1"
constexpr int kHdr = 4;                             // header words: magic, T1, T2, image floats

__host__ __device__ constexpr int pi16(int u) { return (u & ~15) | ((u & 3) << 2) | ((u >> 2) & 3); }

// float offsets of the image of T1 x T2 tiles of 16 units
struct ImageLayout {
    int t1, t2, ld1, ld2, ld3, w1, b1, w2, b2, w3, b3, norm, floats;
};
__host__ __device__ constexpr ImageLayout image_layout(int t1, int t2)
{
    ImageLayout L{};
    L.t1 = t1; L.t2 = t2;
    L.ld1 = 20; L.ld2 = 16 * t1 + 4; L.ld3 = 16 * t2 + 4;
    L.w1 = kHdr;
    L.b1 = L.w1 + 16 * t1 * L.ld1;
    L.w2 = L.b1 + 16 * t1;
    L.b2 = L.w2 + 16 * t2 * L.ld2;
    L.w3 = L.b2 + 16 * t2;
    L.b3 = L.w3 + 16 * L.ld3;
    L.norm = L.b3 + 16;                             // in_mean [16] | in_rscale [16] | out_std [16] | out_mean [16], unpermuted
    L.floats = L.norm + 64;
    return L;
}
static_assert(image_layout(13, 7).floats * 4 == 120656, "the 200/100 image as documented in quadsim_dyn.h");

struct PackArgs {
    int h1, h2;
    const float *wt1, *b1, *wt2, *b2, *wt3, *b3, *in_mean, *in_rscale, *out_std, *out_mean;
};

// one thread per image word
__global__ __launch_bounds__(256) void k_dyn_pack(PackArgs N, ImageLayout L, float *image)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= L.floats) return;
    if (idx < kHdr) {
        const uint32_t hdr[kHdr] = {kMagic, (uint32_t)L.t1, (uint32_t)L.t2, (uint32_t)L.floats};
        reinterpret_cast<uint32_t *>(image)[idx] = hdr[idx];
        return;
    }
    float v = 0.0f;
    if (idx < L.b1) {
        const int r = (idx - L.w1) / L.ld1, p = (idx - L.w1) % L.ld1, u = pi16(r);
        if (p < 16 && u < N.h1) v = N.wt1[u * 16 + pi16(p)];
    } else if (idx < L.w2) {
        const int u = pi16(idx - L.b1);
        if (u < N.h1) v = N.b1[u];
    } else if (idx < L.b2) {
        const int r = (idx - L.w2) / L.ld2, p = (idx - L.w2) % L.ld2, u = pi16(r), k = pi16(p);
        if (p < 16 * L.t1 && u < N.h2 && k < N.h1) v = N.wt2[u * N.h1 + k];
    } else if (idx < L.w3) {
        const int u = pi16(idx - L.b2);
        if (u < N.h2) v = N.b2[u];
    } else if (idx < L.b3) {
        const int r = (idx - L.w3) / L.ld3, p = (idx - L.w3) % L.ld3, u = pi16(r), k = pi16(p);
        if (p < 16 * L.t2 && u < 12 && k < N.h2) v = N.wt3[u * N.h2 + k];
    } else if (idx < L.norm) {
        const int u = pi16(idx - L.b3);
        if (u < 12) v = N.b3[u];
    } else {
        const int a = (idx - L.norm) >> 4, i = (idx - L.norm) & 15;
        if (a == 0) v = N.in_mean[i];
        else if (a == 1) v = N.in_rscale[i];
        else if (i < 12) v = a == 2 ? N.out_std[i] : N.out_mean[i];
    }
    image[idx] = v;
}

}  // namespace qsd
