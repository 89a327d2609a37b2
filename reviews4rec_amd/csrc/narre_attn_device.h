// The owner pass of NARRE's explanation kernels, once: the eval-mode review attention (NARRE.attention,
// pytorch_models/NARRE.py:53-64, with the scorer of NARRE.py:24-36) as ONE WAVE walks it for one owner --
// h = relu(W0 [z_r ; other_r] + b0), logit_r = w3 . h + b3, a = softmax_R(logit), o = sum_r a_r z_r.
//
// narre_explain.hip and narre_whatif.hip (the logits) call these functions, so the logits that feed the one's softmax
// are the other's output by construction.  narre_pair.hip's Jacobian keeps the same sequence inline around its ReLU
// ballot (as calls it measured slower); tests/test_gpu_narre_pair.py holds it to these bits.
// Each kernel keeps its own waves per workgroup, its own __shared__ arrays and its barrier.
//
//   attn_stage_w0     the workgroup's LDS image of W0: row stride 2 LMAX + 4 floats (16-byte reads of row l by lane l are
//                     conflict free), zero beyond column 2 L;
//   attn_lane         what lane l keeps for every owner: its row of the image, b0[l], w3[l], b3;
//   attn_group_logits SLOTS slots at a time: the wave stages [z_r ; other_table[nb_r]] in its own LDS rows (an id outside
//                     the table stages zeros); lane l owns hidden unit l of all of them, W0's row out of LDS against the
//                     staged rows read as broadcasts.  The accumulators run the same FMA chain in ascending column order,
//                     so a slot's logit does not depend on where in a group it sits, nor on SLOTS; the sum over the hidden
//                     units is common.h's fixed-order wave_sum.  Slot r's logit lands in lane r;
//   attn_softmax      lane r holds slot r's logit: wave_max, expf, wave_sum, one division -> a_r;
//   attn_pooled       lane l chains a_r z_r[l] over the slots in ascending order (a_r read across lanes).
// LMAX is the class of L (L <= LMAX): it fixes the LDS strides, nothing of the arithmetic.
#pragma once
#include "common.h"

namespace r4r {

template <int LMAX> constexpr int ATTN_WS = 2 * LMAX + 4;  // floats per staged row of W0
template <int LMAX> constexpr int ATTN_CS = 2 * LMAX;      // floats per staged slot: [z_r ; other_r], zero padded

// w0s: LMAX * ATTN_WS floats of the workgroup's LDS; `threads`: the workgroup's size.  The barrier is the caller's.
template <int LMAX>
__device__ __forceinline__ void attn_stage_w0(float *w0s, const float *W0, int L, int threads) {
    constexpr int WS = ATTN_WS<LMAX>;
    for (int i = threadIdx.x; i < L * WS; i += threads) {
        const int l = i / WS, c = i - l * WS;
        w0s[i] = c < 2 * L ? W0[(size_t)l * 2 * L + c] : 0.f;
    }
}

struct AttnLane {
    int lrow;                          // lanes past L walk a row that exists and count for nothing
    const float *wrow;                 // that row of the LDS image
    float bias, w3l, b3;               // b0[lrow]; w3[lane], 0 past L; b3
};

template <int LMAX>
__device__ __forceinline__ AttnLane attn_lane(const float *w0s, const float *b0, const float *w3, const float *b3, int L,
                                              int lane) {
    const int lrow = lane < L ? lane : L - 1;
    return {lrow, w0s + lrow * ATTN_WS<LMAX>, b0[lrow], lane < L ? w3[lane] : 0.f, b3[0]};
}

// The group of SLOTS slots starting at r0, of an owner with R slots: zn its [R, L] latents, nbn its R ids into
// other_table.  cat: SLOTS * ATTN_CS floats of the wave's own LDS.  sc: lane r0 + s receives slot r0 + s's logit.  The
// fences stand before the staging (the reads of the group, or owner, before are done) and after it.
template <int LMAX, int SLOTS>
__device__ __forceinline__ void attn_group_logits(float *cat, const float *zn, const int64_t *nbn, const float *other_table,
                                                  int64_t other_rows, int r0, int R, int L, const AttnLane &ln, int lane,
                                                  float &sc) {
    constexpr int CS = ATTN_CS<LMAX>;
    const int C4 = (2 * L + 3) & ~3;   // the columns walked: 2L rounded up to the 16-byte reads, the pad holds zeros
    wave_lds_fence();
    for (int i = lane; i < SLOTS * CS; i += WAVE) {
        const int s = i / CS, c = i - s * CS, r = r0 + s;
        float v = 0.f;
        if (r < R) {
            if (c < L) {
                v = zn[r * L + c];
            } else if (c < 2 * L) {
                const int64_t id = nbn[r];
                if (id >= 0 && id < other_rows) v = other_table[id * L + (c - L)];
            }
        }
        cat[i] = v;
    }
    wave_lds_fence();
    float acc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) acc[s] = 0.f;
    for (int c = 0; c < C4; c += 4) {
        const float4 w = *reinterpret_cast<const float4 *>(ln.wrow + c);
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const float4 x = *reinterpret_cast<const float4 *>(cat + s * CS + c);
            acc[s] = fmaf(w.x, x.x, acc[s]);
            acc[s] = fmaf(w.y, x.y, acc[s]);
            acc[s] = fmaf(w.z, x.z, acc[s]);
            acc[s] = fmaf(w.w, x.w, acc[s]);
        }
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
        float h = acc[s] + ln.bias;
        h = h > 0.f ? h : 0.f;
        const float t = wave_sum(ln.w3l * h) + ln.b3;
        if (lane == r0 + s) sc = t;
    }
}

// Lane r: a_r of the R logits the lanes hold; 0 in the lanes past R.
__device__ __forceinline__ float attn_softmax(float sc, int R, int lane) {
    if (lane >= R) sc = -INFINITY;
    const float m = wave_max(sc);
    const float e = lane < R ? expf(sc - m) : 0.f;
    const float den = wave_sum(e);
    return e / den;
}

// Lane l: sum_r a_r zn[r, l] over r ascending (lanes past L chain column 0 and count for nothing).
__device__ __forceinline__ float attn_pooled(float a, const float *zn, int R, int L, int lane) {
    float o = 0.f;
    const int l = lane < L ? lane : 0;
    for (int r = 0; r < R; ++r) o = fmaf(lane_value(a, r), zn[r * L + l], o);
    return o;
}

}  // namespace r4r
